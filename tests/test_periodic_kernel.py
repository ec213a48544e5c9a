"""Host side of the periodic kernel: the C ABI exports and binds the new entry points, the module has gpytorch's parameter layout, the
descriptor carries the table (q, 2, d) = [lengthscale | period], and the models outside the batched exact engine refuse it."""
import ctypes

import pytest
import torch

NEW_TYPED = ["plmc_assemble_per", "plmc_assemble_cross_per", "plmc_factorize_per_ex", "plmc_kinv_grad_per_vd"]


def test_library_exports_and_binds_the_periodic_entry_points():
    from projectedlmc import _hip
    cdll = ctypes.CDLL(_hip.LIB_PATH)
    names = [b + s for b in NEW_TYPED for s in ("_f32", "_f64")] + ["plmc_per_max_dim", "plmc_per_grad_partials_bytes"]
    for name in names:
        assert hasattr(cdll, name), name
        assert name in _hip.exported_symbols(), name
    for b in NEW_TYPED:                  # (kind, ..., ell, oscale) -> (..., ell, period, oscale): the same count
        assert len(_hip._TYPED[b]) == len(_hip._TYPED[b.replace("_per", "")]), b
    lib = _hip.lib()
    assert lib.cdll.plmc_per_max_dim() == 8
    assert lib.cdll.plmc_version() == _hip.ABI_VERSION == 4
    for b in NEW_TYPED:
        for suf in ("_f32", "_f64"):
            assert getattr(lib.cdll, b + suf).argtypes == _hip._TYPED[b]
    # the partial sums: one row per tile, the size of the plain form; the element size does not matter
    assert lib.cdll.plmc_per_grad_partials_bytes(1024, 3, 4) == lib.cdll.plmc_grad_partials_bytes(1024, 3)
    assert lib.cdll.plmc_per_grad_partials_bytes(1024, 3, 8) == lib.cdll.plmc_grad_partials_bytes(1024, 3)


def test_parameter_names_shapes_and_setters():
    import projectedlmc as plmc
    k = plmc.PeriodicKernel(ard_num_dims=3, batch_shape=torch.Size([2]))
    shapes = {n: tuple(p.shape) for n, p in k.named_parameters()}
    assert shapes == {"raw_lengthscale": (2, 1, 3), "raw_period_length": (2, 1, 3)}
    assert all(bool((p == 0).all()) for p in k.parameters())
    assert k.has_lengthscale and k.kind == "periodic"
    k1 = plmc.kernels.PeriodicKernel()
    assert tuple(k1.raw_lengthscale.shape) == (1, 1) and tuple(k1.raw_period_length.shape) == (1, 1)
    k = k.double()
    ell, per = torch.rand(2, 1, 3) + 0.1, torch.rand(2, 1, 3) + 0.1
    k.lengthscale, k.period_length = ell, per
    assert torch.allclose(k.lengthscale, ell.double()) and torch.allclose(k.period_length, per.double())
    assert bool((k.raw_period_length != 0).all()) and bool((k.raw_lengthscale != 0).all())
    k.period_length = 0.75                                   # a scalar broadcasts
    assert torch.allclose(k.period_length, torch.full((2, 1, 3), 0.75, dtype=torch.float64))
    assert set(k.state_dict()) == {"raw_lengthscale", "raw_period_length"}
    marker = object()
    assert plmc.PeriodicKernel(period_length_prior=marker).period_length_prior is marker


def test_descriptor_carries_the_table_and_a_scale_kernel_its_output_scale():
    import projectedlmc as plmc
    from projectedlmc.kernels import LazyKernel
    torch.manual_seed(1)
    q, d = 3, 2
    base = plmc.PeriodicKernel(ard_num_dims=d, batch_shape=torch.Size([q])).double()
    with torch.no_grad():
        for prm in base.parameters():
            prm.add_(torch.randn(prm.shape, dtype=prm.dtype))
    kind, table, osc = base._pieces(d)
    assert kind == "periodic" and osc is None and table.shape == (q, 2, d)
    assert torch.equal(table[:, 0], base.lengthscale.reshape(q, d)) and torch.equal(table[:, 1], base.period_length.reshape(q, d))
    x = torch.rand(7, d, dtype=torch.float64)
    lazy = base(x)
    assert isinstance(lazy, LazyKernel) and lazy.kind == "periodic" and lazy.is_square and lazy.shape == (q, 7, 7)
    assert lazy.ell.shape == (q, 2, d) and lazy.oscale is None
    assert torch.equal(lazy.diagonal(), torch.ones(q, 7, dtype=torch.float64))          # k(x, x) = 1
    sk = plmc.ScaleKernel(base, batch_shape=torch.Size([q])).double()
    sk.outputscale = torch.tensor([0.5, 2.0, 3.0])
    kind, table2, osc = sk._pieces(d)
    assert kind == "periodic" and torch.equal(table2, table) and torch.equal(osc, sk.outputscale) and osc.shape == (q,)
    noisy = sk(x).add_noise(torch.full((q,), 0.25, dtype=torch.float64))
    assert torch.allclose(noisy.diagonal(), sk.outputscale[:, None].expand(q, 7) + 0.25)    # prior_diagonal gives os for this kind
    # one ARD-less kernel on d dimensions: the single lengthscale and period serve every dimension
    iso = plmc.PeriodicKernel().double()
    assert iso._pieces(3)[1].shape == (1, 2, 3)
    # autograd reaches both rows of the table
    (table[:, 0].sum() + 2 * table[:, 1].sum()).backward()
    assert bool((base.raw_lengthscale.grad != 0).all()) and bool((base.raw_period_length.grad != 0).all())


def test_engine_sizes_the_gradient_table_by_kind():
    """(q, 2, d) has the rank of an additive table of two components: the kind tells them apart."""
    from projectedlmc import _engine
    table = torch.ones(3, 2, 5)
    assert _engine.grad_table_width(table, "periodic") == 2 * 5 + 2 and _engine.n_components(table, "periodic") == 1
    assert _engine.grad_table_width(table) == 2 * 5 + 1 + 2 and _engine.n_components(table, "matern52") == 2
    assert _engine.kind_code("periodic") == _engine.PER and _engine.kind_code("sm") is None and _engine.kind_code("rbf") == 0


def test_models_outside_the_exact_engine_refuse_it():
    import projectedlmc as plmc
    PK = plmc.kernels.PeriodicKernel
    X, Y = torch.rand(12, 2), torch.randn(12, 3)
    kw = dict(kernel_type=PK)
    with pytest.raises(NotImplementedError, match=r"handle_covar_\(decomp=\.\.\.\) with several groups.*PeriodicKernel"):
        plmc.handle_covar_(PK, dim=2, decomp=[[0], [1]])
    with pytest.raises(NotImplementedError, match="SGPR.*PeriodicKernel"):
        plmc.ExactGPModel(X, Y[:, 0], plmc.GaussianLikelihood(), n_inducing_points=4, **kw)
    with pytest.raises(NotImplementedError, match="MultitaskGPModel.*PeriodicKernel"):
        plmc.MultitaskGPModel(X, Y, plmc.MultitaskGaussianLikelihood(num_tasks=3), n_tasks=3, n_latents=2, **kw)
    with pytest.raises(NotImplementedError, match="VariationalMultitaskGPModel.*PeriodicKernel"):
        plmc.VariationalMultitaskGPModel(X, n_latents=2, n_tasks=3, **kw)
    # the wording of the spectral-mixture refusal, with the kernel's name
    with pytest.raises(NotImplementedError) as ei:
        plmc.kernels.refuse_periodic(plmc.ScaleKernel(PK(batch_shape=torch.Size([1])), batch_shape=torch.Size([1])), "a model")
    with pytest.raises(NotImplementedError) as es:
        plmc.kernels.refuse_sm(plmc.kernels.SpectralMixtureKernel(num_mixtures=1), "a model")
    assert str(ei.value) == str(es.value).replace("SpectralMixtureKernel", "PeriodicKernel")
    plmc.kernels.refuse_periodic(plmc.RBFKernel(), "a model")                 # other kernels pass
    plmc.kernels.refuse_sm(PK(), "a model")


def test_models_the_exact_engine_serves_construct_with_it():
    import warnings
    import projectedlmc as plmc
    PK = plmc.kernels.PeriodicKernel
    X, Y = torch.rand(12, 2), torch.randn(12, 3)
    m = plmc.ExactGPModel(X, Y[:, 0], plmc.GaussianLikelihood(), kernel_type=PK)
    assert isinstance(m.covar_module, PK) and tuple(m.covar_module.raw_period_length.shape) == (1, 1, 2)
    m = plmc.ExactGPModel(X, Y[:, 0], plmc.GaussianLikelihood(), kernel_type=PK, outputscales=True)
    assert isinstance(m.covar_module.base_kernel, PK)
    mb = plmc.ExactGPModel(X, Y, plmc.GaussianLikelihood(batch_shape=torch.Size([3])), n_tasks=3, kernel_type=PK)
    assert tuple(mb.covar_module.raw_period_length.shape) == (3, 1, 2)
    for bulk in (True, False):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            mp = plmc.ProjectedGPModel(X, Y, 3, 2, mean_type=plmc.ZeroMean, kernel_type=PK, init_lmc_coeffs=True, bulk=bulk)
        names = {n for n, _ in mp.named_parameters()}
        assert {"covar_module.raw_lengthscale", "covar_module.raw_period_length"} <= names
