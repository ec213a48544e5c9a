"""Host side of the rational-quadratic kernel: the C ABI exports and binds the new entry points, the module has gpytorch's parameter
layout, the descriptor carries the table (q, d + 1) = [lengthscales | alpha], the models outside the batched exact engine refuse it,
and -- on the host, in torch float32 -- the textbook form pow(1 + u, -alpha) misses the per-element bound of the fp32 assembly at large
alpha while an emulation of the prescribed form exp(-alpha log1p(u)) meets it."""
import ctypes
import math

import pytest
import torch

import _rq_dense as rd

NEW_TYPED = ["plmc_assemble_rq", "plmc_assemble_cross_rq", "plmc_factorize_rq_ex", "plmc_kinv_grad_rq_vd", "plmc_loo_grad_rq"]


def test_library_exports_and_binds_the_rq_entry_points():
    from projectedlmc import _hip
    cdll = ctypes.CDLL(_hip.LIB_PATH)
    names = [b + s for b in NEW_TYPED for s in ("_f32", "_f64")] + ["plmc_rq_max_dim"]
    for name in names:
        assert hasattr(cdll, name), name
        assert name in _hip.exported_symbols(), name
    for b in NEW_TYPED:                  # (ell, period) -> (ell, alpha): the signature of the periodic form
        assert _hip._TYPED[b] == _hip._TYPED[b.replace("_rq", "_per")], b
    lib = _hip.lib()
    assert lib.cdll.plmc_rq_max_dim() >= 8
    assert lib.cdll.plmc_rq_max_dim() <= lib.cdll.plmc_max_dim()
    assert lib.cdll.plmc_version() == _hip.ABI_VERSION == 4
    for b in NEW_TYPED:
        for suf in ("_f32", "_f64"):
            assert getattr(lib.cdll, b + suf).argtypes == _hip._TYPED[b]


def test_parameter_names_shapes_and_setters():
    import projectedlmc as plmc
    assert plmc.RQKernel is plmc.kernels.RQKernel
    k = plmc.RQKernel(ard_num_dims=3, batch_shape=torch.Size([2]))
    shapes = {n: tuple(p.shape) for n, p in k.named_parameters()}
    assert shapes == {"raw_lengthscale": (2, 1, 3), "raw_alpha": (2, 1)}
    assert all(bool((p == 0).all()) for p in k.parameters())
    assert k.has_lengthscale and k.kind == "rq"
    k1 = plmc.kernels.RQKernel()
    assert tuple(k1.raw_lengthscale.shape) == (1, 1) and tuple(k1.raw_alpha.shape) == (1,)
    k = k.double()
    ell, al = torch.rand(2, 1, 3) + 0.1, torch.tensor([[0.3], [40.0]])
    k.lengthscale, k.alpha = ell, al
    assert torch.allclose(k.lengthscale, ell.double()) and torch.allclose(k.alpha, al.double())
    assert bool((k.raw_alpha != 0).all()) and bool((k.raw_lengthscale != 0).all())
    k.alpha = 0.75                                           # a scalar broadcasts
    assert torch.allclose(k.alpha, torch.full((2, 1), 0.75, dtype=torch.float64))
    assert set(k.state_dict()) == {"raw_lengthscale", "raw_alpha"}
    # a state-dict round trip
    k2 = plmc.RQKernel(ard_num_dims=3, batch_shape=torch.Size([2])).double()
    k2.load_state_dict(k.state_dict())
    assert torch.equal(k2.alpha, k.alpha) and torch.equal(k2.lengthscale, k.lengthscale)
    # alpha_constraint is a constructor argument
    from projectedlmc.constraints import Positive
    marker = Positive()
    assert plmc.RQKernel(alpha_constraint=marker).raw_alpha_constraint is marker


def test_descriptor_carries_the_table_and_a_scale_kernel_its_output_scale():
    import projectedlmc as plmc
    from projectedlmc.kernels import LazyKernel
    torch.manual_seed(1)
    q, d = 3, 2
    base = plmc.RQKernel(ard_num_dims=d, batch_shape=torch.Size([q])).double()
    with torch.no_grad():
        for prm in base.parameters():
            prm.add_(torch.randn(prm.shape, dtype=prm.dtype))
    kind, table, osc = base._pieces(d)
    assert kind == "rq" and osc is None and table.shape == (q, d + 1)
    assert torch.equal(table[:, :d], base.lengthscale.reshape(q, d)) and torch.equal(table[:, d], base.alpha.reshape(q))
    x = torch.rand(7, d, dtype=torch.float64)
    lazy = base(x)
    assert isinstance(lazy, LazyKernel) and lazy.kind == "rq" and lazy.is_square and lazy.shape == (q, 7, 7)
    assert lazy.ell.shape == (q, d + 1) and lazy.oscale is None
    assert torch.equal(lazy.diagonal(), torch.ones(q, 7, dtype=torch.float64))          # k(x, x) = 1
    sk = plmc.ScaleKernel(base, batch_shape=torch.Size([q])).double()
    sk.outputscale = torch.tensor([0.5, 2.0, 3.0])
    kind, table2, osc = sk._pieces(d)
    assert kind == "rq" and torch.equal(table2, table) and torch.equal(osc, sk.outputscale) and osc.shape == (q,)
    noisy = sk(x).add_noise(torch.full((q,), 0.25, dtype=torch.float64))
    assert torch.allclose(noisy.diagonal(), sk.outputscale[:, None].expand(q, 7) + 0.25)    # prior_diagonal gives os for this kind
    # one ARD-less kernel on d dimensions: the single lengthscale serves every dimension
    iso = plmc.RQKernel().double()
    assert iso._pieces(3)[1].shape == (1, 4)
    # active_dims select the columns the kernel sees
    sel = plmc.RQKernel(ard_num_dims=2, active_dims=(0, 2)).double()
    x5 = torch.rand(7, 5, dtype=torch.float64)
    lz = sel(x5)
    assert lz.x1.shape == (7, 2) and torch.equal(lz.x1, x5[:, [0, 2]]) and lz.ell.shape == (1, 3)
    # autograd reaches both parts of the table
    (table[:, :d].sum() + 2 * table[:, d].sum()).backward()
    assert bool((base.raw_lengthscale.grad != 0).all()) and bool((base.raw_alpha.grad != 0).all())


def test_engine_reads_the_dimension_and_sizes_the_gradient_table_by_kind():
    """(q, d + 1) has the rank of a plain table on d + 1 dimensions: the kind tells them apart."""
    from projectedlmc import _engine, _hip
    table = torch.ones(3, 6)
    assert _engine.grad_table_width(table, "rq") == 5 + 3 and _engine.n_components(table, "rq") == 1
    assert _engine.kind_code("rq") == _engine.RQ == "rq" and _engine.kind_code("periodic") == _engine.PER
    assert _engine.kind_code("sm") is None and _engine.kind_code("rbf") == 0
    L = _hip.lib()
    dx = L.cdll.plmc_rq_max_dim()
    _engine._check_kernel_shape(L, torch.ones(2, dx + 1), "rq")               # d = dx: the table is one wider
    with pytest.raises(ValueError, match="plmc_rq_max_dim"):
        _engine._check_kernel_shape(L, torch.ones(2, dx + 2), "rq")
    with pytest.raises(ValueError, match="lengthscales | alpha"):
        _engine._check_kernel_shape(L, torch.ones(2, 1), "rq")
    # the gradient table [d ell: d | d alpha | d noise | d oscale] splits into the table's gradient, the noise and the output scale
    g = torch.arange(2 * 8, dtype=torch.float64).reshape(2, 8)
    g_tab, g_nz, g_os = _engine._split_grad_table(g, (2, 6), (2,))
    assert torch.equal(g_tab, g[:, :6]) and torch.equal(g_nz, g[:, 6]) and torch.equal(g_os, g[:, 7])


def test_handle_covar_initialises_the_lengthscales_from_prior_scales():
    import projectedlmc as plmc
    ps = torch.tensor([0.4, 0.9, 1.7])
    cov = plmc.handle_covar_(plmc.RQKernel, dim=3, prior_scales=ps, prior_width=torch.ones(3), outputscales=True)
    base = cov.base_kernel
    assert isinstance(base, plmc.RQKernel)
    assert torch.allclose(base.lengthscale.reshape(-1), ps, rtol=1e-6)
    assert bool((base.raw_alpha == 0).all())


def test_models_outside_the_exact_engine_refuse_it():
    import projectedlmc as plmc
    RQ = plmc.kernels.RQKernel
    X, Y = torch.rand(12, 2), torch.randn(12, 3)
    kw = dict(kernel_type=RQ)
    with pytest.raises(NotImplementedError, match=r"handle_covar_\(decomp=\.\.\.\) with several groups.*RQKernel"):
        plmc.handle_covar_(RQ, dim=2, decomp=[[0], [1]])
    with pytest.raises(NotImplementedError, match="SGPR.*RQKernel"):
        plmc.ExactGPModel(X, Y[:, 0], plmc.GaussianLikelihood(), n_inducing_points=4, **kw)
    with pytest.raises(NotImplementedError, match="SGPR.*RQKernel"):
        from projectedlmc.sgpr import InducingPointKernel
        InducingPointKernel(RQ(ard_num_dims=2), torch.randn(4, 2), plmc.GaussianLikelihood())
    with pytest.raises(NotImplementedError, match="MultitaskGPModel.*RQKernel"):
        plmc.MultitaskGPModel(X, Y, plmc.MultitaskGaussianLikelihood(num_tasks=3), n_tasks=3, n_latents=2, **kw)
    with pytest.raises(NotImplementedError, match="VariationalMultitaskGPModel.*RQKernel"):
        plmc.VariationalMultitaskGPModel(X, n_latents=2, n_tasks=3, **kw)
    # the wording of the spectral-mixture refusal, with the kernel's name
    with pytest.raises(NotImplementedError) as ei:
        plmc.kernels.refuse_rq(plmc.ScaleKernel(RQ(batch_shape=torch.Size([1])), batch_shape=torch.Size([1])), "a model")
    with pytest.raises(NotImplementedError) as es:
        plmc.kernels.refuse_sm(plmc.kernels.SpectralMixtureKernel(num_mixtures=1), "a model")
    assert str(ei.value) == str(es.value).replace("SpectralMixtureKernel", "RQKernel")
    plmc.kernels.refuse_rq(plmc.RBFKernel(), "a model")                       # other kernels pass
    plmc.kernels.refuse_rq(plmc.kernels.PeriodicKernel(), "a model")
    plmc.kernels.refuse_sm(RQ(), "a model")
    plmc.kernels.refuse_periodic(RQ(), "a model")


def test_models_the_exact_engine_serves_construct_with_it():
    import warnings
    import projectedlmc as plmc
    RQ = plmc.kernels.RQKernel
    X, Y = torch.rand(12, 2), torch.randn(12, 3)
    m = plmc.ExactGPModel(X, Y[:, 0], plmc.GaussianLikelihood(), kernel_type=RQ)
    assert isinstance(m.covar_module, RQ) and tuple(m.covar_module.raw_alpha.shape) == (1, 1)
    m = plmc.ExactGPModel(X, Y[:, 0], plmc.GaussianLikelihood(), kernel_type=RQ, outputscales=True)
    assert isinstance(m.covar_module.base_kernel, RQ)
    assert tuple(m.lscales().shape) == (2,) and m.outputscale().numel() == 1
    mb = plmc.ExactGPModel(X, Y, plmc.GaussianLikelihood(batch_shape=torch.Size([3])), n_tasks=3, kernel_type=RQ)
    assert tuple(mb.covar_module.raw_alpha.shape) == (3, 1) and tuple(mb.covar_module.raw_lengthscale.shape) == (3, 1, 2)
    for bulk in (True, False):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            mp = plmc.ProjectedGPModel(X, Y, 3, 2, mean_type=plmc.ZeroMean, kernel_type=RQ, init_lmc_coeffs=True, bulk=bulk)
        names = {n for n, _ in mp.named_parameters()}
        assert {"covar_module.raw_lengthscale", "covar_module.raw_alpha"} <= names


@pytest.mark.parametrize("alpha", [1.0, 1.0e2, 1.0e4, 1.0e6])
def test_fp32_pow_form_misses_the_bound_at_large_alpha_and_the_prescribed_form_meets_it(alpha):
    """n = 257 near-uniform points on [0, 1], d = 1, ell = 0.2, everything rounded to fp32; reference: the fp64 formula at the same
    inputs; bound: (d + 8) 2^-24 os = 9 2^-24.  pow(1 + u, -alpha) loses ~alpha 2^-24 (5.9e-4 at alpha = 1e4), exp(-alpha log1p(u))
    about 2 2^-24 for every alpha."""
    X, ell, al, os_ = rd.large_alpha_inputs(alpha)
    ref = rd.rq_kernel(X, X, ell, al, os_)[0]
    bound = float(rd.fp32_bound(1, os_))
    e_pow = float((rd.naive_fp32(X, X, ell, al, os_).double() - ref).abs().max())
    e_l1p = float((rd.prescribed_fp32(X, X, ell, al, os_).double() - ref).abs().max())
    print("alpha %g: bound %.3g = 9 u; pow form %.3g = %.1f u; exp(-alpha log1p) form %.3g = %.1f u"
          % (alpha, bound, e_pow, e_pow / rd.U32, e_l1p, e_l1p / rd.U32))
    assert e_l1p <= bound, (e_l1p, bound)
    if alpha >= 1.0e4:
        assert e_pow > bound, (e_pow, bound)
    if alpha == 1.0e4:
        assert e_pow > 1.0e-4, e_pow


def test_fp32_h_series_against_the_direct_form():
    """h(u) = log1p(u) - u / (1 + u) in float32 over u in [1e-6, 8]: the direct form loses every digit at small u; the series below 1/8
    and the direct form above keep a few tens of ulp (ulp = 2^-23 relative), the figure DESIGN.md 7.5 derives (<= 48 ulp)."""
    u = torch.logspace(-6, math.log10(8.0), 4001, dtype=torch.float64).float().double()
    ref = torch.log1p(u) - u / (1.0 + u)
    # fp64 itself cancels at tiny u: take the series there (its truncation after u^19 is far below 2^-53 for u <= 1e-2)
    ser = sum(((-1.0) ** k) * (k - 1) / k * u ** k for k in range(2, 20))
    ref = torch.where(u < 1.0e-2, ser, ref)
    acc = (rd.h_accurate_fp32(u).double() - ref).abs() / ref
    dirr = (rd.h_direct_fp32(u).double() - ref).abs() / ref
    ulp = 2.0 ** -23
    print("h(u): accurate form max rel err %.3g = %.1f ulp; direct form max rel err %.3g" % (float(acc.max()), float(acc.max()) / ulp, float(dirr.max())))
    assert float(acc.max()) <= 48 * ulp, float(acc.max()) / ulp
    assert float(dirr.max()) > 0.1

