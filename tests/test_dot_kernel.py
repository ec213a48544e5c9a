"""Host side of the dot-product kernels (LinearKernel, PolynomialKernel): the C ABI exports and binds the new entry points and returns the
limits, the modules have gpytorch's parameter layout, the descriptor carries the table (q, d + 1) = [variances | offset] and the power in
its kind string, prior_diagonal gives the non-stationary diagonal, the models outside the batched exact engine refuse them, the dense
reference of tests/_dot_dense.py agrees with scikit-learn (tests/golden/dot_third_party_v1.json), and -- on the host, in numpy float32 --
the library's operation order meets the per-element bound the GPU test asserts."""
import ctypes
import json
import os

import pytest
import torch

import _dot_dense as dd

NEW_TYPED = ["plmc_assemble_dot", "plmc_assemble_cross_dot", "plmc_factorize_dot_ex", "plmc_kinv_grad_dot_vd", "plmc_loo_grad_dot"]
SP = torch.nn.functional.softplus


def test_library_exports_and_binds_the_dot_entry_points_and_returns_the_limits():
    from projectedlmc import _hip
    cdll = ctypes.CDLL(_hip.LIB_PATH)
    names = [b + s for b in NEW_TYPED for s in ("_f32", "_f64")] + ["plmc_dot_max_dim", "plmc_dot_max_power"]
    for name in names:
        assert hasattr(cdll, name), name
        assert name in _hip.exported_symbols(), name
    for b in NEW_TYPED:                  # (ell, alpha) -> (var, offset, power): the rational-quadratic form with one more int
        rq = list(_hip._TYPED[b.replace("_dot", "_rq")])
        at = [i for i in range(len(rq)) if _hip._TYPED[b][:i] == rq[:i] and _hip._TYPED[b][i + 1:] == rq[i:]]
        assert at and _hip._TYPED[b][at[0]] is ctypes.c_int, b
    lib = _hip.lib()
    assert lib.cdll.plmc_dot_max_dim() == 16 and lib.cdll.plmc_dot_max_power() == 8
    assert lib.cdll.plmc_dot_max_dim() <= lib.cdll.plmc_max_dim()
    assert lib.cdll.plmc_version() == _hip.ABI_VERSION == 4
    for b in NEW_TYPED:
        for suf in ("_f32", "_f64"):
            assert getattr(lib.cdll, b + suf).argtypes == _hip._TYPED[b]


def test_parameter_names_shapes_state_dict_keys_and_setters():
    import projectedlmc as plmc
    assert plmc.LinearKernel is plmc.kernels.LinearKernel and plmc.PolynomialKernel is plmc.kernels.PolynomialKernel
    lin = plmc.LinearKernel(ard_num_dims=3, batch_shape=torch.Size([2]))
    assert {n: tuple(p.shape) for n, p in lin.named_parameters()} == {"raw_variance": (2, 1, 3)}
    assert tuple(plmc.LinearKernel().raw_variance.shape) == (1, 1)
    pol = plmc.PolynomialKernel(power=2, batch_shape=torch.Size([2]))
    assert {n: tuple(p.shape) for n, p in pol.named_parameters()} == {"raw_offset": (2, 1)}
    assert tuple(plmc.PolynomialKernel(power=1).raw_offset.shape) == (1,)
    for k in (lin, pol):
        assert all(bool((p == 0).all()) for p in k.parameters())
        assert not k.has_lengthscale and k.lengthscale is None and not k.is_stationary
    assert set(lin.state_dict()) == {"raw_variance"} and set(pol.state_dict()) == {"raw_offset"}
    sk = plmc.ScaleKernel(lin, batch_shape=torch.Size([2]))
    assert set(sk.state_dict()) == {"raw_outputscale", "base_kernel.raw_variance"}
    sk = plmc.ScaleKernel(pol, batch_shape=torch.Size([2]))
    assert set(sk.state_dict()) == {"raw_outputscale", "base_kernel.raw_offset"}
    lin, pol = lin.double(), pol.double()
    v, c = torch.rand(2, 1, 3) + 0.1, torch.tensor([[0.3], [4.0]])
    lin.variance, pol.offset = v, c
    assert torch.allclose(lin.variance, v.double()) and torch.allclose(pol.offset, c.double())
    assert bool((lin.raw_variance != 0).all()) and bool((pol.raw_offset != 0).all())
    lin.variance, pol.offset = 0.75, 1.5                     # a scalar broadcasts
    assert torch.allclose(lin.variance, torch.full((2, 1, 3), 0.75, dtype=torch.float64))
    assert torch.allclose(pol.offset, torch.full((2, 1), 1.5, dtype=torch.float64))
    l2 = plmc.LinearKernel(ard_num_dims=3, batch_shape=torch.Size([2])).double()
    l2.load_state_dict(lin.state_dict())
    assert torch.equal(l2.variance, lin.variance)
    from projectedlmc.constraints import Positive
    marker = Positive()
    assert plmc.LinearKernel(variance_constraint=marker).raw_variance_constraint is marker
    assert plmc.PolynomialKernel(power=2, offset_constraint=marker).raw_offset_constraint is marker


@pytest.mark.parametrize("kw", [dict(power=0), dict(power=1.5), dict(), dict(power=-2), dict(power=True)], ids=str)
def test_a_power_that_is_no_positive_int_raises(kw):
    import projectedlmc as plmc
    with pytest.raises(RuntimeError, match="power"):
        plmc.PolynomialKernel(**kw)


def test_table_layout_kind_string_and_autograd():
    import projectedlmc as plmc
    from projectedlmc.kernels import LazyKernel, dot_power
    torch.manual_seed(1)
    q, d = 3, 2
    lin = plmc.LinearKernel(ard_num_dims=d, batch_shape=torch.Size([q])).double()
    pol = plmc.PolynomialKernel(power=3, batch_shape=torch.Size([q])).double()
    with torch.no_grad():
        lin.raw_variance.add_(torch.randn(q, 1, d, dtype=torch.float64))
        pol.raw_offset.add_(torch.randn(q, 1, dtype=torch.float64))
    kind, table, osc = lin._pieces(d)
    assert kind == "linear" and osc is None and table.shape == (q, d + 1) and dot_power(kind) == 1
    assert torch.equal(table[:, :d], lin.variance.reshape(q, d)) and bool((table[:, d] == 0).all())
    kind, tpol, osc = pol._pieces(d)
    assert kind == "poly3" and osc is None and tpol.shape == (q, d + 1) and dot_power(kind) == 3
    assert bool((tpol[:, :d] == 1).all()) and torch.equal(tpol[:, d], pol.offset.reshape(q))
    # two powers, two kinds; the linear kind is not the first power's (its table differs: v free, c = 0)
    assert plmc.PolynomialKernel(power=2).kind == "poly2" != plmc.PolynomialKernel(power=3).kind
    assert plmc.PolynomialKernel(power=1).kind == "poly1" != lin.kind
    assert dot_power("rbf") is None and dot_power("rq") is None and dot_power("polynomial") is None and dot_power("poly") is None
    # the kind survives add_noise
    x = torch.rand(7, d, dtype=torch.float64)
    lazy = pol(x)
    assert isinstance(lazy, LazyKernel) and lazy.kind == "poly3" and lazy.is_square and lazy.shape == (q, 7, 7)
    assert lazy.add_noise(torch.full((q,), 0.25, dtype=torch.float64)).kind == "poly3"
    # one variance serves every dimension; active_dims select the columns
    assert plmc.LinearKernel().double()._pieces(3)[1].shape == (1, 4)
    sel = plmc.LinearKernel(ard_num_dims=2, active_dims=(0, 2)).double()
    x5 = torch.rand(7, 5, dtype=torch.float64)
    assert torch.equal(sel(x5).x1, x5[:, [0, 2]]) and sel(x5).ell.shape == (1, 3)
    # a ScaleKernel hands its output scale on
    sk = plmc.ScaleKernel(pol, batch_shape=torch.Size([q])).double()
    sk.outputscale = torch.tensor([0.5, 2.0, 3.0])
    kind, t2, osc = sk._pieces(d)
    assert kind == "poly3" and torch.equal(t2, tpol) and torch.equal(osc, sk.outputscale)
    # autograd from a weighted sum of the table: the softplus derivative on the free columns, nothing through the constant ones
    w = torch.rand(q, d + 1, dtype=torch.float64) + 0.5
    (table * w).sum().backward()
    assert torch.allclose(lin.raw_variance.grad.reshape(q, d), w[:, :d] * torch.sigmoid(lin.raw_variance.detach()).reshape(q, d), rtol=1e-12)
    (tpol * w).sum().backward()
    assert torch.allclose(pol.raw_offset.grad.reshape(q), w[:, d] * torch.sigmoid(pol.raw_offset.detach()).reshape(q), rtol=1e-12)
    for tab, col, raw in ((lin._pieces(d)[1], slice(d, d + 1), lin.raw_variance), (pol._pieces(d)[1], slice(0, d), pol.raw_offset)):
        gconst = torch.autograd.grad((tab[:, col] * 3.0).sum(), raw, allow_unused=True)[0]       # the constant columns: no dependence
        assert gconst is None or bool((gconst == 0).all())


def test_engine_routes_the_kind_and_sizes_the_gradient_table():
    from projectedlmc import _engine, _hip
    table = torch.ones(3, 6)
    for kind in ("linear", "poly2", "poly8"):
        assert _engine.grad_table_width(table, kind) == 5 + 3 and _engine.n_components(table, kind) == 1
        assert _engine.kind_code(kind) == kind and _engine.is_dot(kind)
    assert not _engine.is_dot("rq") and _engine.kind_code("rbf") == 0
    L = _hip.lib()
    dx, px = L.cdll.plmc_dot_max_dim(), L.cdll.plmc_dot_max_power()
    _engine._check_kernel_shape(L, torch.ones(2, dx + 1), "poly%d" % px)
    with pytest.raises(ValueError, match="plmc_dot_max_dim"):
        _engine._check_kernel_shape(L, torch.ones(2, dx + 2), "linear")
    with pytest.raises(ValueError, match="plmc_dot_max_power"):
        _engine._check_kernel_shape(L, torch.ones(2, 3), "poly%d" % (px + 1))
    with pytest.raises(ValueError, match="variances | offset"):
        _engine._check_kernel_shape(L, torch.ones(2, 1), "linear")
    g = torch.arange(2 * 8, dtype=torch.float64).reshape(2, 8)
    g_tab, g_nz, g_os = _engine._split_grad_table(g, (2, 6), (2,))
    assert torch.equal(g_tab, g[:, :6]) and torch.equal(g_nz, g[:, 6]) and torch.equal(g_os, g[:, 7])


def test_handle_covar_builds_both_with_and_without_output_scales():
    import projectedlmc as plmc
    ps, pw = torch.tensor([0.4, 0.9, 1.7]), torch.ones(3)
    for osc in (False, True):
        cov = plmc.handle_covar_(plmc.LinearKernel, dim=3, prior_scales=ps, prior_width=pw, outputscales=osc, n_funcs=2)
        base = cov.base_kernel if osc else cov
        assert isinstance(cov, plmc.ScaleKernel) == osc and isinstance(base, plmc.LinearKernel)
        assert tuple(base.raw_variance.shape) == (2, 1, 3) and bool((base.raw_variance == 0).all())
        cov = plmc.handle_covar_(plmc.PolynomialKernel, dim=3, ker_kwargs={"power": 3}, outputscales=osc, n_funcs=2)
        base = cov.base_kernel if osc else cov
        assert isinstance(base, plmc.PolynomialKernel) and base.power == 3 and base.kind == "poly3"
        assert tuple(base.raw_offset.shape) == (2, 1) and base.active_dims == (0, 1, 2)
        assert cov(torch.rand(5, 3)).kind == "poly3"


@pytest.mark.parametrize("P", [1, 2, 3])
def test_prior_diagonal_is_the_dense_diagonal(P):
    import projectedlmc as plmc
    from projectedlmc.kernels import prior_diagonal
    g = torch.Generator().manual_seed(P)
    q, n, d = 3, 9, 4
    X = 2 * torch.rand(n, d, generator=g, dtype=torch.float64) - 1
    X[2] = 0
    v, c, os_ = 0.3 + torch.rand(q, d, generator=g, dtype=torch.float64), torch.rand(q, generator=g, dtype=torch.float64), 0.5 + torch.rand(q, generator=g, dtype=torch.float64)
    kind = "linear" if P == 1 else "poly%d" % P
    if P == 1:
        c = torch.zeros_like(c)
    table = torch.cat([v, c[:, None]], 1)
    ref = torch.diagonal(dd.dot_kernel(X, X, v, c, P, os_), dim1=-2, dim2=-1)
    assert torch.allclose(prior_diagonal(kind, X, os_, q, table), ref, rtol=1e-13, atol=0)
    assert torch.allclose(dd.dot_diag(X, v, c, P, os_), ref, rtol=1e-13, atol=0)
    assert torch.allclose(prior_diagonal(kind, X, None, q, table), ref / os_[:, None], rtol=1e-13, atol=0)
    with pytest.raises(ValueError, match="table"):
        prior_diagonal(kind, X, os_, q)
    # every other kind: unchanged, with or without the new argument
    assert torch.equal(prior_diagonal("rbf", X, os_, q), prior_diagonal("rbf", X, os_, q, table)) and torch.equal(prior_diagonal("rbf", X, os_, q), os_[:, None].expand(q, n))
    assert torch.equal(prior_diagonal("spline", X, None, q), prior_diagonal("spline", X, None, q, table))
    # LazyKernel.diagonal passes the table, noise on top
    ker = (plmc.LinearKernel(ard_num_dims=d, batch_shape=torch.Size([q])) if P == 1 else plmc.PolynomialKernel(power=P, batch_shape=torch.Size([q]))).double()
    if P == 1:
        ker.variance = v.reshape(q, 1, d)
    else:
        ker.offset, v = c.reshape(q, 1), torch.ones_like(v)
    sk = plmc.ScaleKernel(ker, batch_shape=torch.Size([q])).double()
    sk.outputscale = os_
    got = sk(X).add_noise(torch.full((q,), 0.25, dtype=torch.float64)).diagonal()
    assert torch.allclose(got, dd.dot_diag(X, v, c, P, os_) + 0.25, rtol=1e-12, atol=0)


@pytest.mark.parametrize("which", ["LinearKernel", "PolynomialKernel"])
def test_models_outside_the_exact_engine_refuse_it(which):
    import projectedlmc as plmc
    K = getattr(plmc.kernels, which)
    kk = {} if which == "LinearKernel" else {"power": 2}
    X, Y = torch.rand(12, 2), torch.randn(12, 3)
    kw = dict(kernel_type=K, ker_kwargs=kk)
    with pytest.raises(NotImplementedError, match=r"handle_covar_\(decomp=\.\.\.\) with several groups.*" + which):
        plmc.handle_covar_(K, dim=2, decomp=[[0], [1]], ker_kwargs=kk)
    with pytest.raises(NotImplementedError, match="SGPR.*" + which):
        plmc.ExactGPModel(X, Y[:, 0], plmc.GaussianLikelihood(), n_inducing_points=4, **kw)
    with pytest.raises(NotImplementedError, match="SGPR.*" + which):
        from projectedlmc.sgpr import InducingPointKernel
        InducingPointKernel(K(**kk), torch.randn(4, 2), plmc.GaussianLikelihood())
    with pytest.raises(NotImplementedError, match="MultitaskGPModel.*" + which):
        plmc.MultitaskGPModel(X, Y, plmc.MultitaskGaussianLikelihood(num_tasks=3), n_tasks=3, n_latents=2, **kw)
    with pytest.raises(NotImplementedError, match="VariationalMultitaskGPModel.*" + which):
        plmc.VariationalMultitaskGPModel(X, n_latents=2, n_tasks=3, **kw)
    # the wording of the rational-quadratic refusal, with the kernel's name; inside a ScaleKernel too
    with pytest.raises(NotImplementedError) as ei:
        plmc.kernels.refuse_dot(plmc.ScaleKernel(K(batch_shape=torch.Size([1]), **kk), batch_shape=torch.Size([1])), "a model")
    with pytest.raises(NotImplementedError) as es:
        plmc.kernels.refuse_rq(plmc.RQKernel(), "a model")
    assert str(ei.value) == str(es.value).replace("RQKernel", which)
    plmc.kernels.refuse_dot(plmc.RBFKernel(), "a model")                      # other kernels pass
    plmc.kernels.refuse_dot(plmc.RQKernel(), "a model")
    plmc.kernels.refuse_rq(K(**kk), "a model")
    # sums (when their table is built) and products (when constructed) name the member they do not take
    with pytest.raises(NotImplementedError, match=which):
        (plmc.RBFKernel() + K(**kk))(torch.rand(5, 2))
    with pytest.raises(NotImplementedError, match=which):
        plmc.kernels.PeriodicKernel() * K(**kk)


def test_models_the_exact_engine_serves_construct_with_them():
    import warnings
    import projectedlmc as plmc
    X, Y = torch.rand(12, 2), torch.randn(12, 3)
    m = plmc.ExactGPModel(X, Y[:, 0], plmc.GaussianLikelihood(), kernel_type=plmc.LinearKernel, outputscales=True)
    assert isinstance(m.covar_module.base_kernel, plmc.LinearKernel)
    mb = plmc.ExactGPModel(X, Y, plmc.GaussianLikelihood(batch_shape=torch.Size([3])), n_tasks=3, kernel_type=plmc.PolynomialKernel,
                           ker_kwargs={"power": 2})
    assert tuple(mb.covar_module.raw_offset.shape) == (3, 1) and mb.covar_module.kind == "poly2"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mp = plmc.ProjectedGPModel(X, Y, 3, 2, mean_type=plmc.ZeroMean, kernel_type=plmc.LinearKernel, init_lmc_coeffs=True)
    assert "covar_module.raw_variance" in {n for n, _ in mp.named_parameters()}


def test_dense_reference_against_scikit_learn():
    """tests/_dot_dense.py against scikit-learn's DotProduct / Exponentiation under GaussianProcessRegressor.log_marginal_likelihood
    (tests/golden/make_dot_third_party.py): the kernel matrix 1e-12, the log marginal likelihood 1e-10 relative, its gradient in
    log os, log sigma_0 (c = sigma_0^2: d / d log sigma_0 = 2 c d / d c) and log noise rtol 1e-7.  The engine is not involved."""
    fx = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dot_third_party_v1.json")))
    assert [c["params"]["power"] for c in fx["cases"]] == [1, 1, 2, 3]
    for case in fx["cases"]:
        P = case["params"]
        X, y = torch.tensor(case["X"], dtype=torch.float64), torch.tensor(case["y"], dtype=torch.float64).reshape(1, -1)
        n = X.shape[0]
        v = torch.tensor([P["v"]], dtype=torch.float64)
        leaves = [torch.tensor([t], dtype=torch.float64, requires_grad=True) for t in (P["os"], P["sigma_0"] ** 2, P["noise"])]
        os_, c, nz = leaves
        K = dd.dot_kernel(X, X, v, c, P["power"], os_)[0] + nz * torch.eye(n, dtype=torch.float64)
        iu = torch.triu_indices(n, n)
        Kref = torch.tensor(case["K_upper"], dtype=torch.float64)
        assert torch.allclose(K.detach()[iu[0], iu[1]], Kref, rtol=1e-12, atol=1e-14)
        lp = dd.dot_logprob(X, y, v, c, P["power"], os_, nz)
        lp.sum().backward()
        assert abs(float(lp.detach()) - case["log_marginal_likelihood"]) <= 1e-10 * abs(case["log_marginal_likelihood"])
        assert ["constant_value" in case["theta_names"][0], "sigma_0" in case["theta_names"][1], "noise_level" in case["theta_names"][2]] == [True] * 3
        got = torch.stack([os_.grad[0] * os_.detach()[0], 2.0 * c.grad[0] * c.detach()[0], nz.grad[0] * nz.detach()[0]])
        want = torch.tensor(case["grad_log_theta"], dtype=torch.float64)
        assert torch.allclose(got, want, rtol=1e-7, atol=1e-9 * float(want.abs().max())), (got, want)


@pytest.mark.parametrize("P", [1, 2, 3, 8])
@pytest.mark.parametrize("d", [1, 5, 16])
def test_fp32_operation_order_meets_the_bound_in_numpy(d, P):
    """The library's operation order (t_k = fl(v_k a_k), an FMA chain from c, P - 1 multiplications, the output scale) in numpy float32
    on inputs uniform in [-1, 1]^d with an all-zero and a duplicated row, against the fp64 formula at the fp32-rounded inputs:
    |err| <= P (d + 3) 2^-24 os S^P per element.  A correct implementation can meet the bound the GPU test asserts."""
    g = torch.Generator().manual_seed(100 * d + P)
    q, n, ns = 2, 129, 40
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    X, Xs = 2 * r(n, d) - 1, 2 * r(ns, d) - 1
    X[7], X[40] = 0.0, X[5]
    v, c, os_ = 0.2 + 1.5 * r(q, d), 1.5 * r(q), 0.5 + r(q)
    c[0] = 0.0
    X, Xs, v, c, os_ = (t.float().double() for t in (X, Xs, v, c, os_))
    worst = 0.0
    for A, B in ((X, X), (X, Xs)):
        ref = dd.dot_kernel(A, B, v, c, P, os_)
        err = (dd.emulated_fp32(A, B, v, c, P, os_).double() - ref).abs()
        bound = dd.fp32_bound(A, B, v, c, P, os_)
        ok = err <= bound
        assert bool(ok.all()), float((err / bound).max())
        worst = max(worst, float((err / bound).max()))
        assert bool((err[dd.dot_S(A, B, v, c) == 0] == 0).all())                       # S = 0 (a zero row, c = 0): exact zeros
    print("d = %d, P = %d: worst err / bound %.3f" % (d, P, worst))
    # negative s under an odd power keeps its sign
    if P % 2 == 1 and d > 1:
        s = dd.dot_s(X, Xs, v, c)
        k = dd.emulated_fp32(X, Xs, v, c, P, os_)
        far = s.abs() > 1e-3
        assert bool((s < 0).any()) and bool((torch.sign(k.double())[far] == torch.sign(s)[far]).all())
