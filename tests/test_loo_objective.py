"""Leave-one-out objective, host side (no GPU): the dense fp64 reference of tests/_loo_dense.py against brute force and against autograd,
the operand algebra of `_engine.loo_gradient_operands`, the public class, its refusals, and the ABI version."""
import inspect
import math

import pytest
import torch

import _loo_dense as ld


def test_dense_helper_equals_brute_force_refits():
    """n = 12: every point predicted by a GP refitted without it, to 1e-10."""
    for family, kw in (("plain", dict(kind="matern52")), ("additive", {}), ("sm", dict(d=2)), ("periodic", dict(d=2))):
        prob = ld.problem(family, 12, 2, seed=7, **kw)
        K = ld.khat(prob)
        a, b = ld.loo_log_prob(K, prob["y"]), ld.loo_brute_force(K, prob["y"])
        assert torch.allclose(a, b, rtol=1e-10, atol=0), (family, a, b)


def test_adjoint_formulas_equal_autograd():
    """G = dL/dKhat and u = dL/dy of the closed form against autograd through the dense inverse."""
    prob = ld.problem("plain", 40, 3, seed=1, kind="rbf")
    K = ld.khat(prob).requires_grad_(True)
    y = prob["y"].clone().requires_grad_(True)
    ld.loo_log_prob(K, y).sum().backward()
    adj = ld.loo_adjoint(K.detach(), y.detach())
    Gsym = 0.5 * (K.grad + K.grad.transpose(-1, -2))
    assert torch.allclose(adj["G"], Gsym, rtol=1e-9, atol=1e-9 * float(Gsym.abs().max()))
    assert torch.allclose(adj["u"], y.grad, rtol=1e-9, atol=1e-9 * float(y.grad.abs().max()))
    assert bool((adj["c"] > 0).all())


def _spd(q, n, seed, cond=1e3):
    g = torch.Generator().manual_seed(seed)
    Q, _ = torch.linalg.qr(torch.randn(q, n, n, generator=g, dtype=torch.float64))
    lam = torch.logspace(0, math.log10(cond), n, dtype=torch.float64)
    return Q @ (lam[:, None] * Q.transpose(-1, -2))


@pytest.mark.parametrize("n,n_pad", [(37, 37), (130, 256)])
@pytest.mark.parametrize("scale", [1.0, 1e3], ids=["balanced", "alpha-1e3-u"])
def test_loo_gradient_operands_reproduce_the_adjoint(n, n_pad, scale):
    """beta beta^T - Xop^T Xop == 2 G to 1e-12 relative on random SPD matrices in fp64; entries at or beyond n are 0.  The second case
    has |alpha| = 1e3 |u|: the two rank-one terms stay the size of their difference."""
    from projectedlmc import _engine
    q = 3
    K = _spd(q, n, seed=n)
    g = torch.Generator().manual_seed(5)
    y = torch.randn(q, n, generator=g, dtype=torch.float64)
    adj = ld.loo_adjoint(K, y)
    alpha, u = adj["alpha"], adj["u"]
    if scale != 1.0:                                          # the identity holds for ANY pair of vectors: force the norms apart
        alpha = alpha * (scale * u.norm(dim=-1, keepdim=True) / alpha.norm(dim=-1, keepdim=True))
    pad = lambda t: torch.nn.functional.pad(t, (0, n_pad - n), value=float("nan"))      # what lies beyond n must not be looked at
    c, gg, beta, rowscale, extra = _engine.loo_gradient_operands(pad(adj["p"]), pad(alpha), pad(u), n)
    c2, g2 = _engine.loo_gradient_operands(pad(adj["p"]), pad(alpha), n=n)
    assert torch.equal(c, c2) and torch.equal(gg, g2)
    for t in (c, gg, beta, rowscale, extra):
        assert t.shape == (q, n_pad) and bool((t[:, n:] == 0).all())
    assert torch.allclose(c[:, :n], 0.5 / adj["p"] + 0.5 * alpha ** 2 / adj["p"] ** 2, rtol=1e-14, atol=0)
    assert torch.allclose(gg[:, :n], -alpha / adj["p"], rtol=1e-14, atol=0)
    P = adj["P"]
    Xop = torch.cat([rowscale[:, :n, None] * P, extra[:, None, :n]], 1)                  # (q, n + 1, n)
    lhs = beta[:, :n, None] * beta[:, None, :n] - Xop.transpose(-1, -2) @ Xop
    au = alpha.unsqueeze(-1) * u.unsqueeze(-2)
    G2 = -2.0 * (P @ (c[:, :n, None] * P) + 0.5 * (au + au.transpose(-1, -2)))
    err = (lhs - G2).abs().amax((-1, -2)) / G2.abs().amax((-1, -2))
    assert float(err.max()) <= 1e-12, err
    # both rank-one vectors are the size of their difference's factors: no term is larger than sqrt(|alpha| |u|) * sqrt 2
    bound = math.sqrt(2.0) * (alpha.norm(dim=-1) * u.norm(dim=-1)).sqrt()
    assert bool((beta.norm(dim=-1) <= bound * (1 + 1e-12)).all()) and bool((extra.norm(dim=-1) <= bound * (1 + 1e-12)).all())


def test_package_exports_the_class_with_the_reference_constructor():
    import projectedlmc as plmc
    assert plmc.LeaveOneOutPseudoLikelihood is plmc.mlls.LeaveOneOutPseudoLikelihood
    assert issubclass(plmc.LeaveOneOutPseudoLikelihood, plmc.ExactMarginalLogLikelihood)
    names = list(inspect.signature(plmc.LeaveOneOutPseudoLikelihood.__init__).parameters)
    assert names == ["self", "likelihood", "model", "train_x", "train_y"]
    X, y = torch.rand(6, 2), torch.rand(6)
    lik = plmc.GaussianLikelihood()
    model = plmc.ExactGPModel(X, y, lik)
    loo = plmc.LeaveOneOutPseudoLikelihood(lik, model, X, y)
    assert loo.train_x is X and loo.train_y is y and loo.likelihood is lik and loo.model is model
    assert plmc.LeaveOneOutPseudoLikelihood(lik, model).train_x is None


def test_non_gaussian_likelihood_is_refused_like_the_exact_mll():
    import projectedlmc as plmc
    X, y = torch.rand(6, 2), torch.rand(6)
    model = plmc.ExactGPModel(X, y, plmc.GaussianLikelihood())
    with pytest.raises(RuntimeError, match="Likelihood must be Gaussian for exact inference"):
        plmc.LeaveOneOutPseudoLikelihood(plmc.likelihoods.Likelihood(), model)


def test_models_outside_the_exact_engine_are_refused_before_the_device_check():
    """Host tensors throughout: a refusal by type arrives as NotImplementedError naming the model, not as the hot path's device error."""
    import warnings
    import projectedlmc as plmc
    g = torch.Generator().manual_seed(0)
    n, d, p = 20, 2, 3
    X = torch.rand(n, d, generator=g)
    y, Y = torch.rand(n, generator=g), torch.rand(n, p, generator=g)
    lik = plmc.GaussianLikelihood()
    sgpr = plmc.ExactGPModel(X, y, lik, kernel_type=plmc.MaternKernel, n_inducing_points=5)
    with pytest.raises(NotImplementedError, match="SGPR"):
        plmc.LeaveOneOutPseudoLikelihood(lik, sgpr)(sgpr(X), y)
    mlik = plmc.MultitaskGaussianLikelihood(num_tasks=p)
    lmc = plmc.MultitaskGPModel(X, Y, mlik, n_tasks=p, n_latents=2)
    with pytest.raises(NotImplementedError, match="MultitaskGPModel"):
        plmc.LeaveOneOutPseudoLikelihood(mlik, lmc)(lmc(X), Y)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        proj = plmc.ProjectedGPModel(X, Y, n_tasks=p, n_latents=2, mean_type=plmc.ZeroMean)
    with pytest.raises(NotImplementedError, match="ProjectedGPModel"):
        plmc.LeaveOneOutPseudoLikelihood(proj.likelihood, proj)(proj(X), Y)
    # the served model on host tensors reaches the device check
    model = plmc.ExactGPModel(X, y, lik)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        plmc.LeaveOneOutPseudoLikelihood(lik, model)(model(X), y)


def test_abi_version_is_unchanged_and_the_new_symbols_resolve():
    from projectedlmc import _hip
    lib = _hip.lib()
    assert lib.cdll.plmc_version() == 4
    names = _hip.exported_symbols()
    for base in ("plmc_loo_grad", "plmc_loo_grad_add", "plmc_loo_grad_sm", "plmc_loo_grad_per", "plmc_loo_operand"):
        for suf in ("_f32", "_f64"):
            assert base + suf in names
            getattr(lib.cdll, base + suf)


def test_bad_arguments_are_reported_through_last_error_without_a_launch():
    """Null pointers and a ragged krows return an error before anything touches a device (this runs without one)."""
    from projectedlmc import _hip
    cd = _hip.lib().cdll
    assert cd.plmc_loo_grad_f64(0, None, 128, 128, 128, 0, None, None, 100, 2, None, None, None, None, 1, None) != 0
    assert b"plmc_loo_grad" in cd.plmc_last_error() or b"loo_grad_impl" in cd.plmc_last_error()
    assert b"null pointer" in cd.plmc_last_error()
    assert cd.plmc_loo_operand_f32(None, 128, 128, 0, None, None, 120, 128, 0, 100, 1, None) != 0
    assert b"null pointer" in cd.plmc_last_error()
    assert cd.plmc_loo_grad_sm_f32(None, 128, 128, 128, 0, None, None, 100, 2, 99, None, None, None, None, None, 1, None) != 0
    assert b"plmc_sm_max_mixtures" in cd.plmc_last_error()
