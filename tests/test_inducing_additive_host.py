"""Host side of additive (`decomp`) kernels under inducing points: the additive kernel hands its component table to the wrappers that ask a
kernel for its pieces, the SGPR and the variational model construct with it on the CPU with the exact model's parameter names, the
inspection helpers see the sub-kernels through the inducing-point wrapper, and the library exports the component-table kernel VJP."""
import ctypes
import warnings

import torch


def test_additive_kernel_pieces_are_its_table():
    import projectedlmc as plmc
    k = plmc.handle_covar_(plmc.MaternKernel, 3, decomp=[[0, 1], [1, 2]], n_funcs=2).double()
    kind, ell, osc = k._pieces(3)
    tkind, tell, tosc = k.table(3)
    assert kind == tkind == "matern52" and torch.equal(ell, tell) and torch.equal(osc, tosc)
    assert ell.shape == (2, 2, 3) and osc.shape == (2, 2)
    assert bool(torch.isinf(ell[:, 0, 2]).all()) and bool(torch.isinf(ell[:, 1, 0]).all())


def _exact_names(decomp, n_tasks=1):
    import projectedlmc as plmc
    m = plmc.ExactGPModel(torch.rand(9, 2), torch.rand(9), plmc.GaussianLikelihood(), n_tasks=n_tasks, decomp=decomp)
    return m, {k for k in m.state_dict() if k.startswith("covar_module.")}


def test_sgpr_model_constructs_with_a_decomposition():
    import projectedlmc as plmc
    from projectedlmc.sgpr import InducingPointKernel
    decomp = [[0], [1]]
    exact, names = _exact_names(decomp)
    torch.manual_seed(0)
    X, y = torch.rand(9, 2), torch.rand(9)
    model = plmc.ExactGPModel(X, y, plmc.GaussianLikelihood(), decomp=decomp, n_inducing_points=4)
    assert isinstance(model.covar_module, InducingPointKernel)
    # (the wrapper also registers the likelihood it was given, as gpytorch's does)
    got = {k for k in model.state_dict() if k.startswith("covar_module.") and not k.startswith("covar_module.likelihood.")}
    assert got == {"covar_module.inducing_points"} | {k.replace("covar_module.", "covar_module.base_kernel.", 1) for k in names}
    kind, ell, osc = model.covar_module._pieces(2)
    assert kind == "rbf" and ell.shape == (1, 2, 2) and osc.shape == (1, 2)
    # the helpers return what the exact model returns for the same decomposition
    ls, ls_exact = model.lscales(), exact.lscales()
    assert len(ls) == len(ls_exact) == 2 and all(a.shape == b.shape for a, b in zip(ls, ls_exact))
    assert model.outputscale().shape == exact.outputscale().shape == (1, 2)
    with torch.no_grad():
        model.covar_module.base_kernel.kernels[1].outputscale = torch.tensor(2.5)
        model.covar_module.base_kernel.kernels[0].base_kernel.lengthscale = torch.tensor(0.25)
    assert abs(float(model.outputscale()[0, 1]) - 2.5) < 1e-6 and abs(float(model.lscales()[0]) - 0.25) < 1e-6
    # the descriptor of the Nystrom prior carries the table (no device needed to build it)
    lazy = model.covar_module(X)
    assert lazy.ell.shape == (1, 2, 2) and lazy.oscale.shape == (1, 2) and lazy.shape == (1, 9, 9)


def test_variational_model_constructs_with_a_decomposition():
    import projectedlmc as plmc
    decomp = [[0], [1]]
    _, names = _exact_names(decomp, n_tasks=3)
    X = torch.rand(12, 2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = plmc.VariationalMultitaskGPModel(X, n_latents=3, n_tasks=4, train_ind_ratio=1.5, decomp=decomp)
        unwh = plmc.VariationalMultitaskGPModel(X, n_latents=3, n_tasks=4, train_ind_ratio=1.0, decomp=decomp)
    for m in (model, unwh):
        assert {k for k in m.state_dict() if k.startswith("covar_module.")} == names
        kind, ell, osc = m.covar_module._pieces(2)
        assert kind == "rbf" and ell.shape == (3, 2, 2) and osc.shape == (3, 2)
        ls = m.lscales()
        assert len(ls) == 2 and all(tuple(t.shape) == (3,) for t in ls)
        assert m.outputscale().shape == (3, 2)
    assert type(unwh.base_variational_strategy).__name__ == "UnwhitenedVariationalStrategy"


def test_prior_variance_sums_the_components():
    from projectedlmc import _var_engine
    from projectedlmc.kernels import prior_diagonal
    osc = torch.tensor([[0.5, 1.5], [2.0, 0.25]], dtype=torch.float64)
    x = torch.zeros(3, 2, dtype=torch.float64)
    pv = _var_engine.prior_variance(osc, 2, torch.float64, osc.device)
    assert torch.equal(pv, osc.sum(-1)) and torch.equal(prior_diagonal("rbf", x, osc, 2), pv[:, None].expand(2, 3))
    assert torch.equal(_var_engine.prior_variance(osc[:, 0], 2, torch.float64, osc.device), osc[:, 0])
    assert torch.equal(_var_engine.prior_variance(None, 2, torch.float64, osc.device), torch.ones(2, dtype=torch.float64))


def test_library_exports_the_component_table_vjp():
    from projectedlmc import _hip
    cdll = ctypes.CDLL(_hip.LIB_PATH)
    for name in ("plmc_kernel_vjp_add_f32", "plmc_kernel_vjp_add_f64"):
        assert hasattr(cdll, name), name
        assert name in _hip.exported_symbols(), name
    assert len(_hip._TYPED["plmc_kernel_vjp_add"]) == len(_hip._TYPED["plmc_kernel_vjp"]) + 1
    lib = _hip.lib()
    for suf in ("_f32", "_f64"):
        assert getattr(lib.cdll, "plmc_kernel_vjp_add" + suf).argtypes == _hip._TYPED["plmc_kernel_vjp_add"]
