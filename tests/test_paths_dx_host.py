"""Differentiable posterior paths without a device (projectedlmc/paths.py): the default call still refuses an x that requires a
gradient, and `differentiable=True` reaches the device check -- nothing in front of it objects to a model on the host.  A path object is
put together by hand from host tensors (drawing one solves on the engine), so what runs here is PosteriorPaths.__call__ and .jacobian
alone."""
import warnings

import pytest
import torch


@pytest.fixture(scope="module")
def plmc():
    import projectedlmc
    return projectedlmc


def _host_paths(plmc, P=3, M=16, din=2, **kw):
    from projectedlmc.paths import PosteriorPaths
    g = torch.Generator().manual_seed(0)
    X, y = torch.rand(40, din, generator=g, dtype=torch.float64), torch.randn(40, generator=g, dtype=torch.float64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = plmc.ExactGPModel(X, y, plmc.GaussianLikelihood(), kernel_type=plmc.MaternKernel, **kw).double().eval()
    lazy = m.covar_module(m._features(X, grad=False))
    pp = object.__new__(PosteriorPaths)
    pp._model, pp._projected, pp._kind = m, False, lazy.kind
    pp._X, pp._ell, pp._osc = lazy.x1.detach().contiguous(), lazy.ell.detach().contiguous(), None
    q, d = pp._ell.shape[0], pp._X.shape[1]
    pp._freq, pp._phase = torch.randn(q, M, d, generator=g, dtype=torch.float64), torch.rand(q, M, generator=g, dtype=torch.float64)
    pp._fscale = torch.full((q, M), 0.3, dtype=torch.float64)
    pp._w, pp._eps = torch.randn(P, q, M, generator=g, dtype=torch.float64), torch.zeros(P, q, 40, dtype=torch.float64)
    pp._Wt = (pp._w * pp._fscale[None]).permute(1, 2, 0).contiguous()
    pp._v = torch.randn(q, 40, P, generator=g, dtype=torch.float64)
    return pp


def test_the_default_call_still_refuses_a_differentiable_x(plmc):
    pp = _host_paths(plmc)
    x = torch.rand(7, 2, dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="requires a gradient is not served"):
        pp(x.clone().requires_grad_())
    with pytest.raises(NotImplementedError, match="requires a gradient is not served"):
        pp(x.clone().requires_grad_(), differentiable=False)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="requires a gradient is not served"):
        pp(x.clone().requires_grad_())                                 # as before, whatever the grad mode
    with pytest.raises(RuntimeError, match="no CPU fallback"):        # a plain x goes on to the engine, as before
        pp(x)


def test_differentiable_fails_at_the_device_check_not_earlier(plmc):
    pp = _host_paths(plmc)
    x = torch.rand(7, 2, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pp(x.clone().requires_grad_(), differentiable=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):        # x needs no gradient: the plain evaluation
        pp(x, differentiable=True)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        pp(x.clone().requires_grad_(), differentiable=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pp.jacobian(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):        # a 1-d x is a column of points, as in the default call
        pp(torch.rand(7, dtype=torch.float64).requires_grad_()[:, None].expand(7, 2), differentiable=True)


def test_an_input_transform_and_a_mean_stay_in_plain_autograd(plmc, monkeypatch):
    """With the two engine products replaced by host stand-ins the node's wiring shows: the features reach it with a graph to x, the
    transform's parameters get no gradient, the LinearMean differentiates by itself, backward is G contracted with the Jacobians summed
    over the latents, and the result is once differentiable."""
    from projectedlmc import paths as paths_mod
    torch.manual_seed(0)
    tf = torch.nn.Linear(5, 2).double()
    pp = _host_paths(plmc, din=5, input_transform=tf, mean_type=plmc.LinearMean)
    seen = {}
    A = torch.randn(1, 2, 3, dtype=torch.float64)                      # a stand-in "path": lat[q, s, c] = sum_k xs[s, k] A[q, k, c]

    def latents(self, xs):
        seen["xs_requires_grad"] = xs.requires_grad
        return torch.einsum("sk,qkc->qsc", xs, A)

    def latents_dx(self, xs, G=None, column=None):
        seen["G"] = G
        return torch.einsum("qsc,qkc->qsk", G, A)

    monkeypatch.setattr(paths_mod.PosteriorPaths, "_latents", latents)
    monkeypatch.setattr(paths_mod.PosteriorPaths, "_latents_dx", latents_dx)
    x = torch.rand(7, 5, dtype=torch.float64).requires_grad_()
    out = pp(x, differentiable=True)
    assert out.shape == (3, 7) and out.requires_grad and seen["xs_requires_grad"] is False     # forward runs on detached features
    up = torch.randn(3, 7, dtype=torch.float64)
    g, = torch.autograd.grad((out * up).sum(), x, create_graph=True)
    assert seen["G"].shape == (1, 7, 3) and all(p.grad is None for p in tf.parameters())
    W, wm = tf.weight.detach(), pp._model.mean_module.weights.detach().reshape(2)
    gF = torch.einsum("cs,kc->sk", up, A[0]) + up.sum(0)[:, None] * wm[None, :]        # d / d features: the node's part and the mean's
    assert torch.allclose(g, gF @ W, rtol=1e-13, atol=1e-14)
    # the same values as the plain call, bit for bit
    assert torch.equal(out.detach(), pp(x.detach()))
