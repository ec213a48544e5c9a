"""`input_transform` on ExactGPModel and ProjectedGPModel: a learned feature map in front of the mean and the kernel.  The MLL reaches
its parameters through d logp / dX of the engine (they stayed at their initial values before: the engine returned no gradient for X);
the eval-mode posterior is the posterior of a model built on the transformed inputs, bit for bit; and the prediction cache follows the
transform's parameters."""
import copy
import warnings

import pytest
import torch

from oracle import gp_math as gm

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def plmc():
    import projectedlmc
    assert torch.cuda.is_available()
    return projectedlmc


def _transform(seed):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(4, 2), torch.nn.Tanh()).double()


def _data(n, p, seed):
    g = torch.Generator().manual_seed(seed)
    X = 2 * torch.rand(n, 4, generator=g, dtype=torch.float64) - 1
    Y = torch.stack([torch.sin(2.0 * X[:, 0] + k) * torch.cos(X[:, 1] - X[:, 3]) + 0.1 * torch.randn(n, generator=g, dtype=torch.float64)
                     for k in range(p)], 1)
    return X, Y


def _exact_model(plmc, X, y, tf):
    return plmc.ExactGPModel(X, y, plmc.GaussianLikelihood(), kernel_type=plmc.MaternKernel, input_transform=tf).double().to(DEV)


def test_mll_gradients_reach_the_transform(plmc):
    n = 200
    X, Y = _data(n, 1, seed=1)
    y = Y[:, 0]
    tf = _transform(2)
    ref_tf = copy.deepcopy(tf)
    m = _exact_model(plmc, X, y, tf)
    m.train(); m.likelihood.train()
    loss = plmc.ExactMarginalLogLikelihood(m.likelihood, m)(m(X.to(DEV)), y.to(DEV))
    loss.backward()
    # the dense reference on the CPU at the model's values
    ell = m.covar_module.lengthscale.detach().cpu().reshape(1, 2)
    noise = m.likelihood.noise.detach().cpu().reshape(())
    F = ref_tf(X)
    c = m.mean_module(m.input_transform(X.to(DEV))).detach().cpu().reshape(n)
    K = gm.kernel_matrix("matern", F, F, ell, None, 2.5)[0] + noise * torch.eye(n, dtype=torch.float64)
    ref = gm.mvn_log_prob(K, y - c) / n
    ref.backward()
    assert abs(float(loss) - float(ref)) < 1e-9 * abs(float(ref))
    for (name, got), want in zip(m.input_transform.named_parameters(), ref_tf.parameters()):
        assert got.grad is not None and float(got.grad.abs().max()) > 0, name
        assert torch.allclose(got.grad.cpu(), want.grad, rtol=1e-7, atol=1e-9), (name, float((got.grad.cpu() - want.grad).abs().max()))
    # the kernel's own parameters still get theirs
    assert all(p.grad is not None for p in m.parameters())


def test_eval_mode_equals_a_model_on_the_transformed_inputs(plmc):
    n, ns = 200, 30
    X, Y = _data(n, 1, seed=3)
    y = Y[:, 0]
    m = _exact_model(plmc, X, y, _transform(4))
    with torch.no_grad():
        m.covar_module.raw_lengthscale.add_(0.3)
        F = m.input_transform(X.to(DEV))
    plain = plmc.ExactGPModel(F, y.to(DEV), plmc.GaussianLikelihood(), kernel_type=plmc.MaternKernel).double().to(DEV)
    plain.load_state_dict({k: v for k, v in m.state_dict().items() if not k.startswith("input_transform.")})
    Xs = (2 * torch.rand(ns, 4, dtype=torch.float64) - 1).to(DEV)
    m.eval(); m.likelihood.eval(); plain.eval(); plain.likelihood.eval()
    with torch.no_grad():
        a, b = m(Xs), plain(m.input_transform(Xs))
        assert torch.equal(a.mean, b.mean) and torch.equal(a.variance, b.variance)
        s2a, ra = m.compute_loo()
        s2b, rb = plain.compute_loo()
        assert torch.equal(s2a, s2b) and torch.equal(ra, rb)
        assert torch.equal(m.kernel_cond(), plain.kernel_cond())


def test_prediction_cache_follows_the_transform(plmc):
    n, ns = 200, 20
    X, Y = _data(n, 1, seed=5)
    m = _exact_model(plmc, X, Y[:, 0], _transform(6))
    Xs = (2 * torch.rand(ns, 4, dtype=torch.float64) - 1).to(DEV)
    m.eval(); m.likelihood.eval()
    c = m._prediction_cache()
    with torch.no_grad():
        first = m(Xs).mean
        m(Xs)                                       # the second call with one key builds the cache
        assert torch.allclose(m(Xs).mean, first, rtol=1e-7, atol=1e-9)     # (the cached path: other arithmetic, the same posterior)
        hits, misses = c.hits, c.misses
        assert hits >= 1
        m.input_transform[0].weight.add_(0.05)      # what an optimiser step does: an in-place update, the version counter moves
        moved = m(Xs).mean
        assert (c.hits, c.misses) == (hits, misses + 1)
        assert float((moved - first).abs().max()) > 1e-6


def test_projected_model_directional_derivatives(plmc):
    """ProjectedLMCmll behind the same transform, p = 5 tasks, q = 2 latents, fp64: <grad, v> against the central difference of the loss
    along three random directions v in the space of ALL parameters, h = 1e-5.  The truncation error is O(h^2) = 1e-10 and the round-off
    about 2^-53 |loss| / h = 1e-11, both relative to derivatives of order 1: the bound of 1e-6 relative is a loose one."""
    n, p, q, h = 200, 5, 2, 1e-5
    X, Y = _data(n, p, seed=7)
    torch.manual_seed(8)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = plmc.ProjectedGPModel(X, Y, p, q, mean_type=plmc.ZeroMean, kernel_type=plmc.MaternKernel, init_lmc_coeffs=True,
                                  input_transform=_transform(9)).double().to(DEV)
    m.train(); m.likelihood.train()
    mll = plmc.ProjectedLMCmll(m.likelihood, m)
    Xd, Yd = X.to(DEV), Y.to(DEV)
    params = [prm for prm in m.parameters() if prm.requires_grad]
    mll(m(Xd), Yd).backward()
    torch.cuda.synchronize()
    grads = [torch.zeros_like(prm) if prm.grad is None else prm.grad.clone() for prm in params]
    assert any(prm is m.input_transform[0].weight for prm in params)
    assert all(prm.grad is not None and float(prm.grad.abs().max()) > 0 for prm in m.input_transform.parameters())

    def value():
        with torch.no_grad():
            return float(mll(m(Xd), Yd))

    g = torch.Generator().manual_seed(10)
    for _ in range(3):
        v = [torch.randn(prm.shape, generator=g, dtype=torch.float64).to(DEV) for prm in params]
        want = sum(float((gr * vv).sum()) for gr, vv in zip(grads, v))
        with torch.no_grad():
            for prm, vv in zip(params, v):
                prm.add_(h * vv)
            up = value()
            for prm, vv in zip(params, v):
                prm.sub_(2 * h * vv)
            down = value()
            for prm, vv in zip(params, v):
                prm.add_(h * vv)
        fd = (up - down) / (2 * h)
        print("directional derivative: %.12e  central difference: %.12e" % (want, fd))
        assert abs(fd - want) <= 1e-6 * abs(want), (fd, want)
