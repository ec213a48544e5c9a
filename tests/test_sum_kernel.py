"""Host side of sums of different kernel families (`k1 + k2`, kind "sum(...)"): `Kernel.__add__` and flattening, gpytorch's parameter
layout, the table (q, G, 3 d + 1) with +inf outside a member's active_dims, folding of an outer ScaleKernel, same-kind stationary sums
unchanged, autograd from the table back into shared and ARD parameters, the refusals, the exports and limits of the built library -- and
the dense reference of the GPU tests (tests/_sum_dense.py) against scikit-learn (tests/golden/sum_third_party_v1.json) and in fp32."""
import ctypes
import json
import math
import os
import warnings

import pytest
import torch

import _sum_dense as sd

NEW_TYPED = ["plmc_assemble_sum", "plmc_assemble_cross_sum", "plmc_factorize_sum_ex", "plmc_kinv_grad_sum_vd", "plmc_loo_grad_sum"]
NEW_PLAIN = ["plmc_sum_max_components", "plmc_sum_max_dim", "plmc_sum_grad_partials_bytes"]
Q3 = torch.Size([3])
INF = float("inf")


def K():
    import projectedlmc
    return projectedlmc.kernels


def factory(**kw):
    k = K()
    kw.pop("lengthscale_prior", None)
    B = kw.get("batch_shape", torch.Size())
    sc = lambda m: k.ScaleKernel(m, batch_shape=B)
    return sc(k.RBFKernel(**kw)) + sc(k.PeriodicKernel(**kw) * k.RBFKernel(**kw)) + sc(k.RQKernel(**kw))


# ------------------------------------------------------------------------------------------------ the library
def test_library_exports_and_binds_the_sum_entry_points():
    from projectedlmc import _hip
    cdll = ctypes.CDLL(_hip.LIB_PATH)
    for name in [b + s for b in NEW_TYPED for s in ("_f32", "_f64")] + NEW_PLAIN:
        assert hasattr(cdll, name), name
        assert name in _hip.exported_symbols(), name
    P, I = _hip._P, _hip._I
    for b in NEW_TYPED:                  # (kind, ..., ncomp, ell, ...) of the `_add` form -> (..., ncomp, fam, table, ...)
        add = _hip._TYPED[b.replace("_sum", "_add")]
        sig = add[1:]                                                              # without the kind
        k = {"plmc_assemble_sum": 3, "plmc_assemble_cross_sum": 5, "plmc_factorize_sum_ex": 3, "plmc_kinv_grad_sum_vd": 8,
             "plmc_loo_grad_sum": 9}[b]                                            # index of ncomp
        assert sig[k] == I and _hip._TYPED[b] == sig[:k + 1] + [P] + sig[k + 1:], b
    lib = _hip.lib()
    assert lib.cdll.plmc_version() == _hip.ABI_VERSION == 4
    for b in NEW_TYPED:
        for suf in ("_f32", "_f64"):
            assert getattr(lib.cdll, b + suf).argtypes == _hip._TYPED[b]


def test_limits_are_what_the_header_says():
    from projectedlmc import _hip
    lib = _hip.lib()
    assert lib.cdll.plmc_sum_max_components() == 4 == lib.cdll.plmc_max_components()
    assert lib.cdll.plmc_sum_max_dim() == 8 == min(lib.cdll.plmc_per_max_dim(), lib.cdll.plmc_rq_max_dim(), lib.cdll.plmc_lper_max_dim())
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "plmc.h")).read()
    assert "int plmc_sum_max_components(void);" in header and "int plmc_sum_max_dim(void);" in header
    for name, code in _hip.FAM.items():
        if code >= 16:
            assert "#define PLMC_FAM_%s %d" % ({"periodic": "PERIODIC", "rq": "RQ", "locally_periodic": "LPER"}[name], code) in header
        else:
            assert _hip.KIND[name] == code
    assert set(_hip.FAM.values()).isdisjoint({_hip.KIND["spline"]}) and _hip.FAM == sd.FAM
    # partial sums: one row of GP fp64 slots per tile AND component + 512 bytes per latent for a one-member sum's re-laid rows; a
    # function of its arguments only
    for esz in (4, 8):
        assert lib.cdll.plmc_sum_grad_partials_bytes(384, 3, 2, esz) == lib.cdll.plmc_grad_partials_bytes(384, 6) + 3 * 512


# ------------------------------------------------------------------------------------------------ __add__, layout, table
def test_add_returns_the_additive_kernel_flattens_and_keeps_gpytorch_names():
    import projectedlmc as plmc
    from projectedlmc.additive import AdditiveKernel
    k = K()
    a, b, c = k.RBFKernel(ard_num_dims=2, batch_shape=Q3), k.PeriodicKernel(ard_num_dims=2, batch_shape=Q3), k.RQKernel(batch_shape=Q3)
    s = a + b
    assert type(s) is AdditiveKernel and isinstance(s.kernels, torch.nn.ModuleList) and list(s.kernels) == [a, b]
    s3 = (a + b) + c
    assert list(s3.kernels) == [a, b, c]
    assert list((a + (b + c)).kernels) == [a, b, c]
    k4 = k.ScaleKernel(a, batch_shape=Q3) + b * k.RBFKernel(ard_num_dims=2, batch_shape=Q3) + c
    assert set(k4.state_dict()) == {"kernels.0.raw_outputscale", "kernels.0.base_kernel.raw_lengthscale", "kernels.1.kernels.0.raw_lengthscale",
                                    "kernels.1.kernels.0.raw_period_length", "kernels.1.kernels.1.raw_lengthscale",
                                    "kernels.2.raw_lengthscale", "kernels.2.raw_alpha"}
    assert plmc.kernels.Kernel.__add__ is not None


def test_the_table_layout_member_list_and_inf_outside_active_dims():
    k = K()
    d = 3
    rbf = k.RBFKernel(ard_num_dims=2, active_dims=[0, 2], batch_shape=Q3)
    lp = k.PeriodicKernel(ard_num_dims=1, active_dims=[1], batch_shape=Q3) * k.RBFKernel(ard_num_dims=1, active_dims=[1], batch_shape=Q3)
    rq = k.RQKernel(batch_shape=Q3)                                                 # no ARD: one lengthscale for the three dimensions
    per = k.PeriodicKernel(ard_num_dims=3, batch_shape=Q3)
    with torch.no_grad():
        for m in (rbf, lp.kernels[0], lp.kernels[1], rq, per):
            m.raw_lengthscale.copy_(torch.randn_like(m.raw_lengthscale))
        lp.kernels[0].raw_period_length.copy_(torch.randn(3, 1, 1))
        per.raw_period_length.copy_(torch.randn(3, 1, 3))
        rq.raw_alpha.copy_(torch.randn(3, 1))
    s = k.ScaleKernel(rbf, batch_shape=Q3) + lp + k.ScaleKernel(rq, batch_shape=Q3) + per
    with torch.no_grad():
        s.kernels[0].raw_outputscale.copy_(torch.randn(3))
        s.kernels[2].raw_outputscale.copy_(torch.randn(3))
    kind, table, os_ = s.table(d)
    assert kind == "sum(rbf,locally_periodic,rq,periodic)"
    assert table.shape == (3, 4, 3 * d + 1) and os_.shape == (3, 4)
    sp = torch.nn.functional.softplus
    ell = sp(rbf.raw_lengthscale).reshape(3, 2)
    assert torch.equal(table[:, 0, [0, 2]], ell) and bool((table[:, 0, 1] == INF).all())
    assert torch.equal(table[:, 1, 1], sp(lp.kernels[0].raw_lengthscale).reshape(3)) and bool((table[:, 1, [0, 2]] == INF).all())
    assert torch.equal(table[:, 1, d + 1], sp(lp.kernels[0].raw_period_length).reshape(3)) and bool(torch.isfinite(table[:, 1, d:2 * d]).all())
    assert torch.equal(table[:, 1, 2 * d + 1], sp(lp.kernels[1].raw_lengthscale).reshape(3)) and bool((table[:, 1, [2 * d, 2 * d + 2]] == INF).all())
    assert torch.equal(table[:, 2, :d], sp(rq.raw_lengthscale).reshape(3, 1).expand(3, d)) and torch.equal(table[:, 2, 3 * d], sp(rq.raw_alpha).reshape(3))
    assert torch.equal(table[:, 3, :d], sp(per.raw_lengthscale).reshape(3, d)) and torch.equal(table[:, 3, d:2 * d], sp(per.raw_period_length).reshape(3, d))
    assert torch.equal(os_[:, 0], sp(s.kernels[0].raw_outputscale)) and torch.equal(os_[:, 2], sp(s.kernels[2].raw_outputscale))
    assert bool((os_[:, [1, 3]] == 1).all())                                        # bare members: ones
    assert bool(torch.isfinite(table[~torch.isinf(table)]).all())
    # the descriptor: kind through add_noise, prior diagonal = sum of the output scales (+ noise)
    X = torch.rand(7, d)
    lazy = s(X)
    assert lazy.kind == kind and lazy.add_noise(torch.full((3,), 0.1)).kind == kind and lazy.ell.shape == table.shape
    assert torch.allclose(lazy.add_noise(torch.full((3,), 0.1)).diagonal(), (os_.sum(-1) + 0.1)[:, None].expand(3, 7))


def test_an_outer_scale_kernel_folds_into_the_component_output_scales():
    k = K()
    inner = factory(batch_shape=Q3)
    outer = k.ScaleKernel(inner, batch_shape=Q3)
    with torch.no_grad():
        outer.raw_outputscale.copy_(torch.tensor([0.3, -0.2, 1.1]))
        for m in inner.kernels:
            m.raw_outputscale.copy_(torch.randn(3))
    kind, table, os_ = outer._pieces(1)
    kind_i, table_i, os_i = inner.table(1)
    assert kind == kind_i == "sum(rbf,locally_periodic,rq)" and torch.equal(table, table_i)
    assert torch.equal(os_, torch.nn.functional.softplus(outer.raw_outputscale).reshape(3, 1) * os_i)


def test_same_kind_stationary_sums_give_todays_component_table():
    from projectedlmc.additive import AdditiveKernel
    k = K()
    subs = [k.ScaleKernel(k.MaternKernel(nu=2.5, ard_num_dims=2, active_dims=g, batch_shape=Q3), batch_shape=Q3) for g in ([0, 1], [1, 2])]
    with torch.no_grad():
        for m in subs:
            m.base_kernel.raw_lengthscale.copy_(torch.randn(3, 1, 2))
            m.raw_outputscale.copy_(torch.randn(3))
    today = AdditiveKernel(*subs)
    assert not today.is_heterogeneous()
    kind, ell, os_ = today.table(3)
    assert kind == "matern52" and ell.shape == (3, 2, 3) and os_.shape == (3, 2)
    kind2, ell2, os2 = (subs[0] + subs[1]).table(3)
    assert kind2 == kind and torch.equal(ell2, ell) and torch.equal(os2, os_)
    sp = torch.nn.functional.softplus
    assert torch.equal(ell[:, 0, :2], sp(subs[0].base_kernel.raw_lengthscale).reshape(3, 2)) and bool((ell[:, 0, 2] == INF).all())
    assert torch.equal(ell[:, 1, 1:], sp(subs[1].base_kernel.raw_lengthscale).reshape(3, 2)) and bool((ell[:, 1, 0] == INF).all())
    mixed = subs[0] + k.ScaleKernel(k.RBFKernel(ard_num_dims=2, active_dims=[1, 2], batch_shape=Q3), batch_shape=Q3)
    assert mixed.is_heterogeneous() and mixed.table(3)[0] == "sum(matern52,rbf)"


def test_autograd_gathers_the_table_gradient_into_ard_and_shared_parameters():
    k = K()
    d = 3
    rbf = k.RBFKernel(ard_num_dims=2, active_dims=[0, 2], batch_shape=Q3)
    rq = k.RQKernel(batch_shape=Q3)                                                 # one lengthscale shared by the d dimensions
    s = rbf + k.ScaleKernel(rq, batch_shape=Q3)
    _, table, os_ = s.table(d)
    g = torch.Generator().manual_seed(0)
    w = torch.rand(table.shape, generator=g)
    wo = torch.rand(os_.shape, generator=g)
    (torch.where(torch.isfinite(table), table, torch.zeros_like(table)) * w).sum().backward(retain_graph=True)
    (os_ * wo).sum().backward()
    dsp = lambda raw: torch.sigmoid(raw)                                            # d softplus
    assert torch.allclose(rbf.raw_lengthscale.grad.reshape(3, 2), w[:, 0, [0, 2]] * dsp(rbf.raw_lengthscale).reshape(3, 2))
    assert torch.allclose(rq.raw_lengthscale.grad.reshape(3), w[:, 1, :d].sum(-1) * dsp(rq.raw_lengthscale).reshape(3))
    assert torch.allclose(rq.raw_alpha.grad.reshape(3), w[:, 1, 3 * d] * dsp(rq.raw_alpha).reshape(3))
    assert torch.allclose(s.kernels[1].raw_outputscale.grad, wo[:, 1] * dsp(s.kernels[1].raw_outputscale))


# ------------------------------------------------------------------------------------------------ refusals
def test_unsupported_members_raise_naming_the_members():
    k = K()
    for bad, word in ((k.RBFKernel() + k.SpectralMixtureKernel(num_mixtures=2), "SpectralMixtureKernel"),
                      (k.RBFKernel() + k.SplineKernel(), "SplineKernel"),
                      (k.PeriodicKernel() + k.ScaleKernel(k.ScaleKernel(k.RBFKernel())), "ScaleKernel"),
                      (k.PeriodicKernel() + k.ScaleKernel(k.RBFKernel() + k.RQKernel()), "AdditiveKernel")):
        with pytest.raises(NotImplementedError, match=word):
            bad.table(1)
    with pytest.raises(NotImplementedError, match="batch_shape"):
        (k.RBFKernel(batch_shape=Q3) + k.PeriodicKernel()).table(1)
    with pytest.raises(NotImplementedError, match="ProductKernel serves"):
        k.RBFKernel() + k.RQKernel() * k.RBFKernel()


def test_models_outside_the_batched_exact_engine_refuse_a_sum_of_families():
    import projectedlmc as plmc
    X, y, Y = torch.rand(20, 2), torch.rand(20), torch.rand(20, 3)
    members = r"AdditiveKernel\(ScaleKernel\(RBFKernel\), ScaleKernel\(ProductKernel\), ScaleKernel\(RQKernel\)\)"
    with pytest.raises(NotImplementedError, match=r"SGPR.*" + members):
        plmc.ExactGPModel(X, y, plmc.GaussianLikelihood(), kernel_type=factory, n_inducing_points=5)
    with pytest.raises(NotImplementedError, match=r"MultitaskGPModel.*" + members):
        plmc.MultitaskGPModel(X, Y, plmc.MultitaskGaussianLikelihood(num_tasks=3), n_tasks=3, n_latents=2, kernel_type=factory)
    with pytest.raises(NotImplementedError, match=r"VariationalMultitaskGPModel.*" + members):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            plmc.VariationalMultitaskGPModel(X, n_tasks=3, n_latents=2, train_ind_ratio=2.0, kernel_type=factory)
    with pytest.raises(NotImplementedError, match=r"decomp.*" + members):
        plmc.ExactGPModel(X, y, plmc.GaussianLikelihood(), kernel_type=factory, decomp=[[0], [1]])
    # served: the exact model without inducing points and the projected model construct; a same-kind stationary sum keeps going under SGPR
    m = plmc.ExactGPModel(X, y, plmc.GaussianLikelihood(), kernel_type=factory)
    assert m.covar_module(X).kind == "sum(rbf,locally_periodic,rq)"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pm = plmc.ProjectedGPModel(X, Y, 3, 2, mean_type=plmc.ZeroMean, kernel_type=factory)
    assert pm.covar_module(X).ell.shape == (2, 3, 7)
    same = lambda **kw: K().RBFKernel(**{**kw, "ard_num_dims": 1, "active_dims": [0]}) + K().RBFKernel(**{**kw, "ard_num_dims": 1, "active_dims": [1]})
    plmc.ExactGPModel(X, y, plmc.GaussianLikelihood(), kernel_type=same, n_inducing_points=5)


def test_the_engine_sizes_things_by_the_kind():
    from projectedlmc import _engine, _hip
    kind = _engine.sum_kind(["rbf", "locally_periodic", "rq"])
    assert kind == "sum(rbf,locally_periodic,rq)" and _engine.is_sum(kind) and _engine.sum_members(kind) == ["rbf", "locally_periodic", "rq"]
    assert not _engine.is_sum("sm") and not _engine.is_sum(None) and _engine.kind_code(kind) == kind
    table = torch.ones(2, 3, 7)
    assert _engine.n_components(table, kind) == 3 and _engine.grad_table_width(table, kind) == 3 * 7 + 1 + 3
    assert _engine._per_kind(kind) == _engine.SUM
    g = torch.arange(2 * 25, dtype=torch.float64).reshape(2, 25)
    ge, gn, go = _engine._split_grad_table(g, table.shape, (2, 3))
    assert ge.shape == (2, 3, 7) and torch.equal(gn, g[:, 21]) and torch.equal(go, g[:, 22:])
    L = _hip.lib()
    _engine._check_kernel_shape(L, table, kind)
    with pytest.raises(ValueError, match=r"\(q, G, 3 d \+ 1\)"):
        _engine._check_kernel_shape(L, torch.ones(2, 2, 7), kind)
    with pytest.raises(ValueError, match="plmc_sum_max_dim"):
        _engine._check_kernel_shape(L, torch.ones(2, 3, 28), kind)
    with pytest.raises(ValueError, match="spline"):
        _engine._check_kernel_shape(L, torch.ones(2, 2, 7), "sum(rbf,spline)")


# ------------------------------------------------------------------------------------------------ the dense reference
def test_the_dense_reference_against_scikit_learn():
    """tests/golden/sum_third_party_v1.json (make_sum_third_party.py): K, the log marginal likelihood and its gradient in scikit-learn's
    log-parameters, rtol 1e-10.  scikit-learn's periodic length l enters as l^2: ell_periodic = l^2, d/d log l = 2 ell d/d ell."""
    D = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sum_third_party_v1.json")))
    P = D["params"]
    X = torch.tensor(D["X"], dtype=torch.float64).reshape(-1, 1)
    y = torch.tensor(D["y"], dtype=torch.float64).reshape(1, -1)
    n = X.shape[0]
    members = ("rbf", "locally_periodic", "rq")
    nan = float("nan")
    table = torch.tensor([[[P["ell_rbf"], nan, nan, nan], [P["ell_ess"] ** 2, P["period"], P["ell_drift"], nan],
                           [P["ell_rq"], nan, nan, P["alpha"]]]], dtype=torch.float64)
    os_ = torch.tensor([[P["os_rbf"], P["os_lper"], P["os_rq"]]], dtype=torch.float64)
    noise = torch.tensor([P["noise"]], dtype=torch.float64)
    Kd = sd.khat(members, X, table, os_, noise)[0]
    Ks = Kd[::D["K_stride"], ::D["K_stride"]]                                       # (the fixture holds K at every tenth point)
    iu = torch.triu_indices(Ks.shape[0], Ks.shape[0])
    assert Ks.shape[0] == 30 and torch.allclose(Ks[iu[0], iu[1]], torch.tensor(D["K_upper"], dtype=torch.float64), rtol=1e-10, atol=0)
    val, g = sd.grads(sd.sum_logprob, members, X, y, table, os_, noise)
    assert abs(float(val) - D["log_marginal_likelihood"]) <= 1e-10 * abs(D["log_marginal_likelihood"])
    gt = g[0, :12].reshape(3, 4)
    nat = {"k1__k1__k1__k1__constant_value": (g[0, 13], P["os_rbf"]), "k1__k1__k1__k2__length_scale": (gt[0, 0], P["ell_rbf"]),
           "k1__k1__k2__k1__k1__constant_value": (g[0, 14], P["os_lper"]),
           "k1__k1__k2__k1__k2__length_scale": (2.0 * gt[1, 0], P["ell_ess"] ** 2),        # d/d log l = (d/d ell) 2 l^2
           "k1__k1__k2__k1__k2__periodicity": (gt[1, 1], P["period"]), "k1__k1__k2__k2__length_scale": (gt[1, 2], P["ell_drift"]),
           "k1__k2__k1__constant_value": (g[0, 15], P["os_rq"]), "k1__k2__k2__alpha": (gt[2, 3], P["alpha"]),
           "k1__k2__k2__length_scale": (gt[2, 0], P["ell_rq"]), "k2__noise_level": (g[0, 12], P["noise"])}
    assert list(nat) == D["theta_names"]
    for name, ref in zip(D["theta_names"], D["grad_log_theta"]):
        got = float(nat[name][0]) * nat[name][1]
        assert abs(got - ref) <= 1e-10 * max(abs(ref), 1.0) or abs(got - ref) <= 1e-10 * abs(ref), (name, got, ref)
    assert 1e3 < D["cond"] < 1e4


@pytest.mark.parametrize("d", [1, 3])
def test_the_fp32_problem_leaves_half_of_the_fp32_tolerances(d):
    """_sum_dense.fp32_problem (the problem of the GPU fp32 test): the dense reference evaluated in torch float32 on the CPU is within HALF
    of that test's tolerances (value 1e-4 relative, gradients 2e-3 of the largest entry) of the fp64 reference, so those tolerances leave
    room for the engine's own fp32 arithmetic; the parameters are in the ranges the test names."""
    members = ("matern52", "locally_periodic", "rq")
    X, y, table, os_, nz = sd.fp32_problem(members, d)
    q, G, rec = table.shape
    assert float(nz.min()) >= 0.05 and float(nz.max()) <= 0.2 and 0.3 < float(os_.sum(-1).min()) and float(os_.sum(-1).max()) < 3.0
    assert float(X.min()) >= 0.0 and float(X.max()) <= 10.0
    assert 0.7 <= float(table[:, :, :d].min()) and float(table[:, :, :d].max()) <= 1.7          # lengthscales of order 1 at every d
    v64, g64 = sd.grads(sd.sum_logprob, members, X, y, table, os_, nz)
    v32, g32 = sd.grads(sd.sum_logprob, members, X.float(), y.float(), table.float(), os_.float(), nz.float())
    assert float(((v32.double() - v64) / v64).abs().max()) < 0.5e-4
    for lo, hi in ((0, G * rec), (G * rec, G * rec + 1), (G * rec + 1, G * rec + 1 + G)):
        a, b = g32.double()[:, lo:hi], g64[:, lo:hi]
        assert float((a - b).abs().max() / b.abs().max()) < 1e-3, (lo, hi)


def test_the_dense_reference_switches_dimensions_off_and_ignores_unowned_slots():
    members = ("periodic", "rbf", "locally_periodic")
    d, q, n = 3, 2, 12
    table, os_ = sd.make_table(members, d, q, seed=1, off={0: [1], 2: [0]})
    assert bool(torch.isnan(table[:, 1, d:]).all()) and bool(torch.isnan(table[:, 0, 2 * d:]).all())
    g = torch.Generator().manual_seed(2)
    X = torch.rand(n, d, generator=g, dtype=torch.float64)
    K1 = sd.sum_kernel(members, X, X, table, os_)
    X2 = X.clone()
    X2[:, 1] += 5.0 * torch.rand(n, generator=g, dtype=torch.float64)               # dimension 1 is off for member 0 only
    t0 = table.clone()
    assert bool(torch.isfinite(K1).all())
    assert torch.equal(sd.member_kernel("periodic", X, X, t0[:, 0]), sd.member_kernel("periodic", X2, X2, t0[:, 0]))
    y = torch.randn(q, n, generator=g, dtype=torch.float64)
    nz = torch.full((q,), 0.1, dtype=torch.float64)
    _, tab = sd.grads(sd.sum_logprob, members, X, y, table, os_, nz)
    gt = tab[:, :3 * (3 * d + 1)].reshape(q, 3, 3 * d + 1)
    assert bool((gt[:, 0, [1, d + 1]] == 0).all()) and bool((gt[:, 2, [0, d, 2 * d]] == 0).all())
    assert bool((gt[:, 1, d:] == 0).all()) and bool(torch.isfinite(tab).all())
    assert math.isfinite(float(tab.abs().sum()))
