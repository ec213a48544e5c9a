"""Input gradients of the exact MLL without a device: the fp64 reference the GPU tests hold plmc_input_grad against
(tests/_input_grad_dense.py) equals autograd of the dense Cholesky log density for every family; the library exports the entry points;
and what is refused -- kernel kinds whose diagonal depends on x, input_transform beside inducing points, the leave-one-out objective
behind an input_transform -- says so before anything looks at a device."""
import ctypes
import warnings

import pytest
import torch

import _input_grad_dense as igd

REFUSED_KINDS = ("spline", "linear", "poly3", "sum(rbf,periodic)")


@pytest.mark.parametrize("family", igd.FAMILIES)
def test_reference_equals_autograd_of_the_dense_log_density(family):
    """With P = Khat^-1 and alpha = Khat^-1 y the row-wise pull-back of alpha alpha^T - P IS d log N(y; 0, Khat) / dX: no factor 1/2."""
    n, d, q = 40, 5, 2
    p = igd.problem(family, d, q, seed=3)
    X = igd.inputs(n, d, seed=3)
    g = torch.Generator().manual_seed(11)
    y = torch.randn(q, n, generator=g, dtype=torch.float64)
    noise = torch.tensor([0.1, 0.3], dtype=torch.float64)
    Khat = p.K(X, X) + noise[:, None, None] * torch.eye(n, dtype=torch.float64)
    P = torch.linalg.inv(Khat)
    P = 0.5 * (P + P.transpose(1, 2))
    alpha = torch.linalg.solve(Khat, y.unsqueeze(-1)).squeeze(-1)
    got, terms = igd.input_grad_ref(p.K, X, P, alpha)
    want = igd.mll_input_grad(p.K, X, noise, y)
    err = float((got - want).abs().max() / want.abs().max())
    print("%s: relative error %.3e" % (family, err))
    assert err <= 1e-10, (family, err)
    assert bool((terms >= got.abs() * (1 - 1e-12)).all())               # a sum of absolute terms bounds the sum
    assert bool((got[:, :, p.zero] == 0).all()) and bool((terms[:, :, p.zero] == 0).all())


def test_library_exports_the_input_gradient_entry_points():
    from projectedlmc import _hip
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for infix in ("", "_add", "_sm", "_per", "_rq", "_lper", "_sum", "_dot"):
        for suf in ("_f32", "_f64"):
            name = "plmc_input_grad" + infix + suf
            assert name in _hip.exported_symbols(), name
            assert hasattr(lib, name), name
    assert lib.plmc_version() == _hip.ABI_VERSION == 4                  # symbols are only added


@pytest.mark.parametrize("kind", REFUSED_KINDS)
def test_refused_kinds_raise_before_the_device_check(kind):
    from projectedlmc import _engine
    n, d, q = 12, 2, 2
    X = torch.rand(n, d)
    y, noise = torch.randn(q, n), torch.full((q,), 0.1)
    ell = torch.ones(q, 2, 3 * d + 1) if kind.startswith("sum") else torch.ones(q, d + 1) if kind != "spline" else torch.ones(q, d)
    with pytest.raises(NotImplementedError, match=kind.replace("(", r"\(").replace(")", r"\)")):
        _engine.exact_latent_log_prob(kind, X.clone().requires_grad_(), ell, None, noise, y)
    # without a gradient for X nothing changes: host tensors meet the device check
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _engine.exact_latent_log_prob(kind, X, ell, None, noise, y)


def test_input_transform_refusals_at_construction():
    import projectedlmc as plmc
    k = plmc.kernels
    X, y, Y = torch.rand(20, 4), torch.rand(20), torch.rand(20, 3)
    tf = lambda: torch.nn.Sequential(torch.nn.Linear(4, 2), torch.nn.Tanh())
    with pytest.raises(NotImplementedError, match="n_inducing_points"):
        plmc.ExactGPModel(X, y, plmc.GaussianLikelihood(), input_transform=tf(), n_inducing_points=5)
    for kw, word in ((dict(kernel_type=plmc.SplineKernel), "spline"), (dict(kernel_type=plmc.LinearKernel), "linear"),
                     (dict(kernel_type=plmc.PolynomialKernel, ker_kwargs={"power": 3}), "poly3"),
                     (dict(kernel_type=lambda **a: k.RBFKernel(**a) + k.PeriodicKernel(**a)), r"sum\(rbf,periodic\)")):
        with pytest.raises(NotImplementedError, match=word):
            plmc.ExactGPModel(X, y, plmc.GaussianLikelihood(), input_transform=tf(), **kw)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with pytest.raises(NotImplementedError, match=word):
                plmc.ProjectedGPModel(X, Y, 3, 2, mean_type=plmc.ZeroMean, input_transform=tf(), **kw)
        plmc.ExactGPModel(X, y, plmc.GaussianLikelihood(), **kw)          # without a transform they are served as before
    with pytest.raises(NotImplementedError, match="input_transform"):
        plmc.MultitaskGPModel(X, Y, plmc.MultitaskGaussianLikelihood(num_tasks=3), n_tasks=3, n_latents=2, input_transform=tf())


def test_input_transform_is_a_submodule_and_sets_the_feature_width():
    import projectedlmc as plmc
    X, y = torch.rand(20, 4), torch.rand(20)
    tf = torch.nn.Sequential(torch.nn.Linear(4, 2), torch.nn.Tanh())
    m = plmc.ExactGPModel(X, y, plmc.GaussianLikelihood(), input_transform=tf, kernel_type=plmc.MaternKernel)
    assert m.dim == 2 and m.covar_module.ard_num_dims == 2
    assert any(p is tf[0].weight for p in m.parameters())
    assert "input_transform.0.weight" in m.state_dict()
    m.train()
    out = m(X)                                                          # the prior is built on the features
    assert out.lazy_covariance_matrix.x1.shape == (20, 2) and out.lazy_covariance_matrix.x1.requires_grad
    with pytest.raises(RuntimeError, match="train on the training inputs"):
        m(X[:10])                                                       # the check stays on the raw inputs
    plain = plmc.ExactGPModel(X, y, plmc.GaussianLikelihood(), kernel_type=plmc.MaternKernel)
    assert plain.dim == 4 and plain.input_transform is None
    assert not any(key.startswith("input_transform") for key in plain.state_dict())


def test_leave_one_out_objective_refuses_an_input_transform():
    import projectedlmc as plmc
    X, y = torch.rand(20, 4), torch.rand(20)
    m = plmc.ExactGPModel(X, y, plmc.GaussianLikelihood(), input_transform=torch.nn.Linear(4, 2))
    m.train()
    loo = plmc.LeaveOneOutPseudoLikelihood(m.likelihood, m)
    with pytest.raises(NotImplementedError, match="input_transform"):
        loo(m(X), y)
