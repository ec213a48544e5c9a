"""Host side of the locally periodic kernel (PeriodicKernel * RBFKernel): the C ABI exports and binds the new entry points, the product
has gpytorch's parameter layout, the descriptor carries the table (q, 3, d) = [periodic lengthscales | periods | RBF lengthscales], the
engine sizes things by the kind, the models outside the batched exact engine refuse it, unsupported products raise, and the models the
engine serves construct with a factory function -- and, on the host in torch float32, the naive restatement of the formula misses the
per-element bound of the fp32 assembly at large phase."""
import ctypes
import warnings

import pytest
import torch

import _lper_dense as ld

NEW_TYPED = ["plmc_assemble_lper", "plmc_assemble_cross_lper", "plmc_factorize_lper_ex", "plmc_kinv_grad_lper_vd", "plmc_loo_grad_lper"]
Q3 = torch.Size([3])


def factory(**kw):
    import projectedlmc as plmc
    return plmc.kernels.PeriodicKernel(**kw) * plmc.kernels.RBFKernel(**kw)


def test_library_exports_and_binds_the_lper_entry_points():
    from projectedlmc import _hip
    cdll = ctypes.CDLL(_hip.LIB_PATH)
    names = [b + s for b in NEW_TYPED for s in ("_f32", "_f64")] + ["plmc_lper_max_dim", "plmc_lper_grad_partials_bytes"]
    for name in names:
        assert hasattr(cdll, name), name
        assert name in _hip.exported_symbols(), name
    P = _hip._P
    for b in NEW_TYPED:                  # (ell, period) -> (ell, period, rbf_ell): the periodic signature with one more pointer behind `period`
        per = _hip._TYPED[b.replace("_lper", "_per")]
        at = {"plmc_assemble_lper": 5, "plmc_assemble_cross_lper": 7, "plmc_factorize_lper_ex": 5, "plmc_kinv_grad_lper_vd": 10,
              "plmc_loo_grad_lper": 11}[b]
        assert _hip._TYPED[b] == per[:at] + [P] + per[at:], b
    lib = _hip.lib()
    assert lib.cdll.plmc_lper_max_dim() == 8 == lib.cdll.plmc_per_max_dim()
    assert lib.cdll.plmc_version() == _hip.ABI_VERSION == 4
    for b in NEW_TYPED:
        for suf in ("_f32", "_f64"):
            assert getattr(lib.cdll, b + suf).argtypes == _hip._TYPED[b]
    # the partial-sum scratch: one row of GP fp64 slots per tile, a function of its arguments only
    for esz in (4, 8):
        assert lib.cdll.plmc_lper_grad_partials_bytes(384, 3, esz) == lib.cdll.plmc_grad_partials_bytes(384, 3) == 9 * 3 * 34 * 8


@pytest.mark.parametrize("order", ["periodic_first", "rbf_first"])
def test_the_product_has_gpytorch_parameter_names_shapes_and_zero_initialisation(order):
    import projectedlmc as plmc
    assert plmc.ProductKernel is plmc.kernels.ProductKernel
    per = plmc.PeriodicKernel(ard_num_dims=2, batch_shape=Q3)
    rbf = plmc.RBFKernel(ard_num_dims=2, batch_shape=Q3)
    k = per * rbf if order == "periodic_first" else rbf * per
    assert isinstance(k, plmc.ProductKernel) and isinstance(k.kernels, torch.nn.ModuleList) and len(k.kernels) == 2
    ip, ir = (0, 1) if order == "periodic_first" else (1, 0)
    assert k.kernels[ip] is per and k.kernels[ir] is rbf
    shapes = {n: tuple(p.shape) for n, p in k.named_parameters()}
    assert shapes == {"kernels.%d.raw_lengthscale" % ip: (3, 1, 2), "kernels.%d.raw_period_length" % ip: (3, 1, 2),
                      "kernels.%d.raw_lengthscale" % ir: (3, 1, 2)}
    assert set(k.state_dict()) == set(shapes)
    assert all(bool((p == 0).all()) for p in k.parameters())
    assert not k.has_lengthscale and k.lengthscale is None and k.kind == "locally_periodic"
    assert k.batch_shape == Q3 and k.ard_num_dims == 2 and k.active_dims is None
    # a state-dict round trip
    with torch.no_grad():
        for prm in k.parameters():
            prm.add_(torch.randn(prm.shape))
    k2 = (plmc.PeriodicKernel(ard_num_dims=2, batch_shape=Q3) * plmc.RBFKernel(ard_num_dims=2, batch_shape=Q3) if order == "periodic_first"
          else plmc.RBFKernel(ard_num_dims=2, batch_shape=Q3) * plmc.PeriodicKernel(ard_num_dims=2, batch_shape=Q3))
    k2.load_state_dict(k.state_dict())
    assert torch.equal(k2._pieces(2)[1], k._pieces(2)[1])


@pytest.mark.parametrize("order", ["periodic_first", "rbf_first"])
def test_descriptor_carries_the_table_and_a_scale_kernel_its_output_scale(order):
    import projectedlmc as plmc
    from projectedlmc.kernels import LazyKernel
    torch.manual_seed(1)
    q, d = 3, 2
    per = plmc.PeriodicKernel(ard_num_dims=d, batch_shape=Q3).double()
    rbf = plmc.RBFKernel(ard_num_dims=d, batch_shape=Q3).double()
    base = per * rbf if order == "periodic_first" else rbf * per
    with torch.no_grad():
        for prm in base.parameters():
            prm.add_(torch.randn(prm.shape, dtype=prm.dtype))
    kind, table, osc = base._pieces(d)
    assert kind == "locally_periodic" and osc is None and table.shape == (q, 3, d)
    assert torch.equal(table[:, 0], per.lengthscale.reshape(q, d)) and torch.equal(table[:, 1], per.period_length.reshape(q, d))
    assert torch.equal(table[:, 2], rbf.lengthscale.reshape(q, d))
    x = torch.rand(7, d, dtype=torch.float64)
    lazy = base(x)
    assert isinstance(lazy, LazyKernel) and lazy.kind == "locally_periodic" and lazy.is_square and lazy.shape == (q, 7, 7)
    assert lazy.ell.shape == (q, 3, d) and lazy.oscale is None
    assert torch.equal(lazy.diagonal(), torch.ones(q, 7, dtype=torch.float64))          # k(x, x) = 1
    sk = plmc.ScaleKernel(base, batch_shape=Q3).double()
    sk.outputscale = torch.tensor([0.5, 2.0, 3.0])
    kind, table2, osc = sk._pieces(d)
    assert kind == "locally_periodic" and torch.equal(table2, table) and torch.equal(osc, sk.outputscale) and osc.shape == (q,)
    noisy = sk(x).add_noise(torch.full((q,), 0.25, dtype=torch.float64))
    assert torch.allclose(noisy.diagonal(), sk.outputscale[:, None].expand(q, 7) + 0.25)    # prior_diagonal gives os for this kind
    # expand: factors with ard_num_dims=None on d dimensions -- each single value serves every dimension
    iso = (plmc.PeriodicKernel() * plmc.RBFKernel()).double()
    iso.kernels[0].lengthscale, iso.kernels[0].period_length, iso.kernels[1].lengthscale = 0.7, 1.9, 2.3
    t3 = iso._pieces(3)[1]
    assert t3.shape == (1, 3, 3)
    assert torch.allclose(t3[0], torch.tensor([[0.7] * 3, [1.9] * 3, [2.3] * 3], dtype=torch.float64))
    # active_dims come from the factors and select the columns the kernel sees; ScaleKernel takes them from the product
    one = torch.Size([1])
    sel = (plmc.PeriodicKernel(ard_num_dims=2, active_dims=(0, 2), batch_shape=one)
           * plmc.RBFKernel(ard_num_dims=2, active_dims=(0, 2), batch_shape=one)).double()
    assert sel.active_dims == (0, 2) and plmc.ScaleKernel(sel, batch_shape=one).active_dims == (0, 2)
    x5 = torch.rand(7, 5, dtype=torch.float64)
    lz = sel(x5)
    assert lz.x1.shape == (7, 2) and torch.equal(lz.x1, x5[:, [0, 2]]) and lz.ell.shape == (1, 3, 2)
    # autograd reaches all three rows of the table
    (table[:, 0].sum() + 2 * table[:, 1].sum() + 3 * table[:, 2].sum()).backward()
    assert all(bool((p.grad != 0).all()) for p in base.parameters())


def test_engine_sizes_things_by_the_kind():
    """(q, 3, d) has the rank of an additive table of three components: the kind tells them apart."""
    from projectedlmc import _engine, _hip
    LP = "locally_periodic"
    assert _engine.LPER == LP and _engine.kind_code(LP) == LP
    for d in (1, 3, 8):
        table = torch.ones(3, 3, d)
        assert _engine.grad_table_width(table, LP) == 3 * d + 2
        assert _engine.n_components(table, LP) == 1
        assert _engine.n_components(table) == 3                                 # (without the kind: an additive table)
    L = _hip.lib()
    dx = L.cdll.plmc_lper_max_dim()
    _engine._check_kernel_shape(L, torch.ones(2, 3, dx), LP)
    with pytest.raises(ValueError, match="plmc_lper_max_dim"):
        _engine._check_kernel_shape(L, torch.ones(2, 3, dx + 1), LP)
    with pytest.raises(ValueError, match="periodic lengthscales | periods | RBF lengthscales"):
        _engine._check_kernel_shape(L, torch.ones(2, 2, 3), LP)
    with pytest.raises(ValueError, match=r"\(q, 3, d\)"):
        _engine._check_kernel_shape(L, torch.ones(2, 3), LP)
    # the gradient table [d ell | d period | d lam | d noise | d oscale] splits into the table's gradient, the noise and the output scale
    d = 2
    g = torch.arange(2 * (3 * d + 2), dtype=torch.float64).reshape(2, 3 * d + 2)
    g_tab, g_nz, g_os = _engine._split_grad_table(g, (2, 3, d), (2,))
    assert torch.equal(g_tab, g[:, :3 * d].reshape(2, 3, d)) and torch.equal(g_nz, g[:, 3 * d]) and torch.equal(g_os, g[:, 3 * d + 1])
    assert _engine._per_kind(LP) == LP and _engine._per_kind("periodic") == "periodic" and not _engine._per_kind("rbf")


def test_models_outside_the_exact_engine_refuse_it():
    import projectedlmc as plmc
    X, Y = torch.rand(12, 2), torch.randn(12, 3)
    kw = dict(kernel_type=factory)
    with pytest.raises(NotImplementedError, match=r"handle_covar_\(decomp=\.\.\.\) with several groups.*ProductKernel"):
        plmc.handle_covar_(factory, dim=2, decomp=[[0], [1]])
    with pytest.raises(NotImplementedError, match=r"ExactGPModel\(n_inducing_points=\.\.\.\) \(SGPR\).*ProductKernel"):
        plmc.ExactGPModel(X, Y[:, 0], plmc.GaussianLikelihood(), n_inducing_points=4, **kw)
    with pytest.raises(NotImplementedError, match=r"ExactGPModel\(n_inducing_points=\.\.\.\) \(SGPR\).*ProductKernel"):
        plmc.ExactGPModel(X, Y[:, 0], plmc.GaussianLikelihood(), n_inducing_points=4, outputscales=True, **kw)
    with pytest.raises(NotImplementedError, match=r"InducingPointKernel \(SGPR\).*ProductKernel"):
        from projectedlmc.sgpr import InducingPointKernel
        InducingPointKernel(factory(ard_num_dims=2), torch.randn(4, 2), plmc.GaussianLikelihood())
    with pytest.raises(NotImplementedError, match="MultitaskGPModel.*ProductKernel"):
        plmc.MultitaskGPModel(X, Y, plmc.MultitaskGaussianLikelihood(num_tasks=3), n_tasks=3, n_latents=2, **kw)
    with pytest.raises(NotImplementedError, match="VariationalMultitaskGPModel.*ProductKernel"):
        plmc.VariationalMultitaskGPModel(X, n_latents=2, n_tasks=3, **kw)
    # the wording of the spectral-mixture refusal, with the kernel's name; an instance bare or inside a ScaleKernel
    one = torch.Size([1])
    with pytest.raises(NotImplementedError) as ei:
        plmc.kernels.refuse_product(plmc.ScaleKernel(factory(batch_shape=one), batch_shape=one), "a model")
    with pytest.raises(NotImplementedError) as eb:
        plmc.kernels.refuse_product(factory(), "a model")
    with pytest.raises(NotImplementedError) as es:
        plmc.kernels.refuse_sm(plmc.kernels.SpectralMixtureKernel(num_mixtures=1), "a model")
    assert str(ei.value) == str(eb.value) == str(es.value).replace("SpectralMixtureKernel", "ProductKernel (PeriodicKernel * RBFKernel)")
    plmc.kernels.refuse_product(plmc.RBFKernel(), "a model")                  # other kernels pass
    plmc.kernels.refuse_product(plmc.kernels.PeriodicKernel(), "a model")
    plmc.kernels.refuse_periodic(factory(), "a model")                        # (the product is not a bare periodic kernel)
    plmc.kernels.refuse_rq(factory(), "a model")


def test_unsupported_products_raise():
    import projectedlmc as plmc
    K = plmc.kernels
    one = torch.Size([1])
    cases = [
        (lambda: K.RBFKernel() * K.RBFKernel(), r"ProductKernel\(RBFKernel, RBFKernel\)"),                        # other kinds
        (lambda: K.PeriodicKernel() * K.PeriodicKernel(), r"ProductKernel\(PeriodicKernel, PeriodicKernel\)"),
        (lambda: K.PeriodicKernel() * K.MaternKernel(nu=2.5), r"ProductKernel\(PeriodicKernel, MaternKernel\)"),
        (lambda: K.RQKernel() * K.RBFKernel(), r"ProductKernel\(RQKernel, RBFKernel\)"),
        (lambda: K.PeriodicKernel() * K.RBFKernel() * K.RBFKernel(), r"ProductKernel\(ProductKernel, RBFKernel\)"),   # three factors
        (lambda: K.ProductKernel(K.PeriodicKernel(), K.RBFKernel(), K.RBFKernel()), r"ProductKernel\(PeriodicKernel, RBFKernel, RBFKernel\)"),
        (lambda: K.ScaleKernel(K.PeriodicKernel(batch_shape=one), batch_shape=one) * K.RBFKernel(batch_shape=one), r"ProductKernel\(ScaleKernel, RBFKernel\)"),  # a ScaleKernel inside
        (lambda: K.PeriodicKernel(batch_shape=one) * K.ScaleKernel(K.RBFKernel(batch_shape=one), batch_shape=one), r"ProductKernel\(PeriodicKernel, ScaleKernel\)"),
        (lambda: K.PeriodicKernel(ard_num_dims=2) * K.RBFKernel(ard_num_dims=3), r"ard_num_dims.*ProductKernel\(PeriodicKernel, RBFKernel\)"),
        (lambda: K.PeriodicKernel(ard_num_dims=2) * K.RBFKernel(), r"ard_num_dims.*ProductKernel"),
        (lambda: K.PeriodicKernel(active_dims=(0,)) * K.RBFKernel(active_dims=(1,)), r"active_dims.*ProductKernel"),
        (lambda: K.PeriodicKernel(batch_shape=Q3) * K.RBFKernel(), r"batch_shape.*ProductKernel"),
    ]
    for build, pattern in cases:
        with pytest.raises(NotImplementedError, match=pattern):
            build()
    with pytest.raises(NotImplementedError, match=r"ProductKernel\(PeriodicKernel, float\)"):
        K.PeriodicKernel() * 2.0


def test_models_the_exact_engine_serves_construct_with_a_factory():
    import projectedlmc as plmc
    PK = plmc.ProductKernel
    X, Y = torch.rand(12, 2), torch.randn(12, 3)
    cov = plmc.handle_covar_(factory, dim=2)
    assert isinstance(cov, plmc.ScaleKernel) and isinstance(cov.base_kernel, PK)
    assert tuple(cov.base_kernel._pieces(2)[1].shape) == (1, 3, 2)
    assert isinstance(plmc.handle_covar_(factory, dim=2, outputscales=False), PK)
    # prior scales reach no lengthscale of a product (has_lengthscale is False, as in the reference): it builds and stays at zero
    cov = plmc.handle_covar_(factory, dim=2, prior_scales=torch.tensor([0.4, 0.9]), prior_width=torch.ones(2))
    assert all(bool((p == 0).all()) for p in cov.base_kernel.parameters())
    m = plmc.ExactGPModel(X, Y[:, 0], plmc.GaussianLikelihood(), kernel_type=factory)
    assert isinstance(m.covar_module, PK)
    names = {n for n, _ in m.named_parameters()}
    assert {"covar_module.kernels.0.raw_lengthscale", "covar_module.kernels.0.raw_period_length", "covar_module.kernels.1.raw_lengthscale"} <= names
    m = plmc.ExactGPModel(X, Y[:, 0], plmc.GaussianLikelihood(), kernel_type=factory, outputscales=True)
    assert isinstance(m.covar_module.base_kernel, PK)
    assert m.outputscale().numel() == 1                                        # outputscale() works through the ScaleKernel
    names = {n for n, _ in m.named_parameters()}
    assert {"covar_module.base_kernel.kernels.0.raw_lengthscale", "covar_module.base_kernel.kernels.0.raw_period_length",
            "covar_module.base_kernel.kernels.1.raw_lengthscale", "covar_module.raw_outputscale"} <= names
    mb = plmc.ExactGPModel(X, Y, plmc.GaussianLikelihood(batch_shape=Q3), n_tasks=3, kernel_type=factory)
    assert tuple(mb.covar_module.kernels[0].raw_period_length.shape) == (3, 1, 2)
    assert tuple(mb.covar_module.kernels[1].raw_lengthscale.shape) == (3, 1, 2)
    plmc.LeaveOneOutPseudoLikelihood(mb.likelihood, mb)                        # constructs; its value is pinned on the device
    for bulk in (True, False):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            mp = plmc.ProjectedGPModel(X, Y, 3, 2, mean_type=plmc.ZeroMean, kernel_type=factory, init_lmc_coeffs=True, bulk=bulk)
        names = {n for n, _ in mp.named_parameters()}
        assert {"covar_module.kernels.0.raw_lengthscale", "covar_module.kernels.0.raw_period_length",
                "covar_module.kernels.1.raw_lengthscale"} <= names
        assert tuple(mp.covar_module(X).ell.shape) == (2, 3, 2)


@pytest.mark.parametrize("lam", [1.0, 0.3])
def test_naive_fp32_form_misses_the_bound_at_large_phase(lam):
    """n = 257 near-uniform points in [0, 1], p = 5e-4 (2000 revolutions), ell = 1, os = 1.3, everything rounded to fp32; reference: the
    fp64 formula at the same inputs; bound: (24 (1 + 1) + 9) 2^-24 os = 4.4e-6.  The all-fp32 restatement is ~7e-4 off at lam = 1 and
    still tens of times the bound at lam = 0.3, where the RBF factor damps the far pairs."""
    n = 257
    g = torch.Generator().manual_seed(0)
    X = ((torch.arange(n, dtype=torch.float64) + 0.3 * torch.rand(n, generator=g, dtype=torch.float64)) / n).reshape(n, 1)
    X[0, 0], X[-1, 0] = 0.0, 1.0
    t = lambda v: torch.tensor(v, dtype=torch.float64).float().double()
    X, ell, per, lm, os_ = X.float().double(), t([[1.0]]), t([[5.0e-4]]), t([[lam]]), t([1.3])
    ref = ld.lper_kernel(X, X, ell, per, lm, os_)[0]
    bound = float(ld.fp32_bound(1, ell, os_))
    e_naive = float((ld.naive_fp32(X, X, ell, per, lm, os_).double() - ref).abs().max())
    print("lam %g: bound %.3g; naive fp32 err %.3g = %.0f x the bound" % (lam, bound, e_naive, e_naive / bound))
    assert abs(bound - 57 * ld.U32 * float(os_[0])) < 1e-12
    assert e_naive > 10 * bound, (e_naive, bound)
