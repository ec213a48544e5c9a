"""Differentiable posterior paths through the models (projectedlmc/paths.py): n = 40, n* = 7, d = 2, P = 3 paths, 16
features, fp64 and fp32, for a single-output ExactGPModel, a batch of two tasks, ProjectedGPModel (p = 4, q = 2), an additive decomp, a
LinearMean and an input_transform (a linear embedding of 3 raw dimensions).

  * paths(x, differentiable=True) equals paths(x) bit for bit;
  * x.grad for a random upstream tensor is held against fp64 autograd of the paths written densely from the object's OWN freq, phase,
    feature_scale, w and v (tests/_cross_matvec_dx_ref.py paths_latents: the formula of _cross_matvec_ref.paths_dense with the solved
    weights handed in, so the conditioning of the solve does not enter), at the features the model computed;
  * torch.autograd.gradcheck in fp64; jacobian(x) equals the rows of that gradient; a detached x with the keyword launches no dx kernel;
    the default call still raises.

Tolerance of one element of d / d(features), u = 2^-24 / 2^-53, the kernels' own contracts (tests/test_gpu_cross_matvec_dx.py,
tests/test_gpu_rff_matvec_dx.py) for the G the node hands them plus what plain autograd around the node rounds:
    sum_lat [ tolF T_lat + B_rff,lat ]                   tolF = 4 (d + 4) u (fp64: 1e-10), T = sum_i |w_si d k|, B_rff the features' bound
  + c_mix u sum_lat [ T_lat(|G|, |v|) + 2 pi sum_j |f_jk| sum_c |G_sc| |Wt_jc| ]      G = H^T-folded upstream, formed in the element type:
                                                          p products and adds per element, c_mix = p + 1 (exact models: a permute, 0)
  + (P + 1) u sum_c |up_cs| |m_k|                        the LinearMean's own gradient, P terms
  + 3 u |want|                                           the cast of the node's fp64 result, the mean's addition
and through an input_transform x.grad = gF W: the above folded with |W| plus (d' + 1) u |gF| |W|."""
import functools
import math
import warnings

import pytest
import torch

import _cross_matvec_dx_ref as cdx
from oracle import gp_math as gm

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N, NS, D, NPATHS, NFEAT, P_TASKS, Q = 40, 7, 2, 3, 16, 4, 2
MODELS = ("single", "tasks", "projected", "decomp", "linear_mean", "transform")
JACOBIAN_MODELS = ("single", "tasks", "projected", "decomp")
U = {torch.float64: 2.0 ** -53, torch.float32: 2.0 ** -24}


@pytest.fixture(scope="module")
def plmc():
    import projectedlmc
    assert torch.cuda.is_available()
    return projectedlmc


def _data(din):
    g = torch.Generator().manual_seed(1)
    X = (2 * torch.rand(N, din, generator=g, dtype=torch.float64) - 1).float().double()
    Y = torch.stack([torch.sin(2.0 * X[:, 0] + k) * torch.cos(X[:, 1]) + 0.1 * torch.randn(N, generator=g, dtype=torch.float64)
                     for k in range(P_TASKS)], 1).float().double()
    xs = (2 * torch.rand(NS, din, generator=g, dtype=torch.float64) - 1).float().double()
    return X, Y, xs


@functools.lru_cache(maxsize=None)
def _built(which, dt):
    """(model, paths, raw test points) of a case, built once and left unchanged."""
    import projectedlmc as plmc
    X, Y, xs = _data(3 if which == "transform" else D)
    y = Y[:, 0].contiguous()
    torch.manual_seed(3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if which == "tasks":
            m = plmc.ExactGPModel(X, Y[:, :2].T.contiguous(), plmc.GaussianLikelihood(batch_shape=torch.Size([2])), n_tasks=2,
                                  kernel_type=plmc.MaternKernel)
        elif which == "projected":
            m = plmc.ProjectedGPModel(X, Y, P_TASKS, Q, mean_type=plmc.ZeroMean, kernel_type=plmc.MaternKernel, init_lmc_coeffs=True, BDN=False)
        elif which == "decomp":
            m = plmc.ExactGPModel(X, y, plmc.GaussianLikelihood(), kernel_type=plmc.MaternKernel, decomp=[[0], [1]])
        elif which == "linear_mean":
            m = plmc.ExactGPModel(X, y, plmc.GaussianLikelihood(), kernel_type=plmc.MaternKernel, mean_type=plmc.LinearMean)
        elif which == "transform":
            torch.manual_seed(5)
            m = plmc.ExactGPModel(X, y, plmc.GaussianLikelihood(), kernel_type=plmc.MaternKernel, input_transform=torch.nn.Linear(3, D).double())
        else:
            m = plmc.ExactGPModel(X, y, plmc.GaussianLikelihood(), kernel_type=plmc.MaternKernel, outputscales=True)
    m = m.double()
    m.likelihood.noise = 0.1
    m = m.to(dt).to(DEV).eval()
    pp = m.sample_paths(NPATHS, num_features=NFEAT, generator=torch.Generator().manual_seed(11))
    return m, pp, xs


def _upstream(shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(7), dtype=torch.float64).float().double()


def _dense(pp):
    """(K, X, freq, phase, fscale, w, v) in fp64 on the host, from the object's own tensors."""
    up = lambda t: t.detach().double().cpu()
    ell = up(pp._ell)
    ell = ell[:, None, :] if ell.dim() == 2 else ell
    q, G = ell.shape[:2]
    osc = torch.ones(q, G, dtype=torch.float64) if pp._osc is None else up(pp._osc).reshape(q, G)
    K = lambda A, B: sum(gm.kernel_matrix("matern", A, B, ell[:, g], osc[:, g], 2.5) for g in range(G))
    return K, up(pp._X), up(pp.freq), up(pp.phase), up(pp.feature_scale), up(pp.w), up(pp.v)


def _fold(m, which, up, absolute=False):
    """The upstream gradient of the outputs as G (q, n*, P) of the latents."""
    if which == "projected":
        H = m.lmc_coefficients().detach().double().cpu()
        return torch.einsum("csp,qp->qsc", up.abs(), H.abs()) if absolute else torch.einsum("csp,qp->qsc", up, H)
    G = up[None].permute(0, 2, 1) if which != "tasks" else up.permute(2, 1, 0)
    return G.abs() if absolute else G


def _want(m, pp, which, dt, feats, up):
    """(d sum(up * paths) / d features, its tolerance), (n*, d') fp64 each, at the features the model computed."""
    K, X, freq, phase, fs, w, v = _dense(pp)
    Wt = (w * fs[None]).permute(1, 2, 0).contiguous()
    G, Gabs = _fold(m, which, up), _fold(m, which, up, absolute=True)
    f = feats.clone().requires_grad_()
    lat = cdx.paths_latents(K, X, freq, phase, fs, w, v, f)
    want, = torch.autograd.grad((lat * G).sum(), f)
    # the two parts on their own agree with the autograd of the whole: the references of the kernels' tests
    Jk, Tk = cdx.reference(K, X, feats, v, G)
    Jr, Br = cdx.rff_reference(freq, phase, feats, Wt, G, None, dt)
    assert torch.allclose(want, (Jk + Jr).sum(0), rtol=1e-11, atol=1e-12)
    u, d = U[dt], feats.shape[1]
    tol = (cdx.tolerance("matern52", d, dt) * Tk + Br).sum(0)
    if which == "projected":
        Tabs = cdx.reference(K, X, feats, v.abs(), Gabs)[1]
        Rabs = 2.0 * math.pi * torch.einsum("qsj,qjk->qsk", torch.einsum("qsc,qjc->qsj", Gabs, Wt.abs()), freq.abs())
        tol = tol + (P_TASKS + 1) * u * (Tabs + Rabs).sum(0)
    mean_w = None
    if which == "linear_mean":
        mean_w = m.mean_module.weights.detach().double().cpu().reshape(d)
        want = want + up.sum(0)[:, None] * mean_w[None, :]
        tol = tol + (NPATHS + 1) * u * up.abs().sum(0)[:, None] * mean_w.abs()[None, :]
    return want, tol + 3 * u * want.abs()


def _got(m, pp, which, dt, xs, up):
    x = xs.to(DEV, dt).requires_grad_()
    out = pp(x, differentiable=True)
    (out * up.to(DEV, dt)).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), x.grad


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("which", MODELS)
def test_gradient_of_the_paths_reaches_the_test_inputs(plmc, which, dt):
    """On the parent commit: TypeError, __call__() got an unexpected keyword argument 'differentiable'."""
    m, pp, xs = _built(which, dt)
    plain = pp(xs.to(DEV, dt))
    up = _upstream(plain.shape)
    out, grad = _got(m, pp, which, dt, xs, up)
    assert torch.equal(out, plain)                                    # the same two products: bit for bit
    assert grad is not None and grad.dtype == dt and grad.shape == xs.shape and bool(torch.isfinite(grad).all())
    with torch.no_grad():
        feats = m.covar_module.select(m._features(xs.to(DEV, dt), grad=False)).double().cpu()
    want, tol = _want(m, pp, which, dt, feats, up)
    if which == "transform":                                          # x.grad = gF W, formed by plain autograd in the element type
        W = m.input_transform.weight.detach().double().cpu()
        tol = tol @ W.abs() + (D + 1) * U[dt] * (want.abs() @ W.abs())
        want = want @ W
    err = (grad.double().cpu() - want).abs()
    print("%s %s: largest share of the tolerance %.3f, largest |x.grad| %.3g" % (which, dt, float((err / tol).max()), float(want.abs().max())))
    assert bool((err <= tol).all()), (which, dt, float((err / tol).max()))
    # the draws, the weights, the hyper-parameters and a transform's parameters are constants of the node
    assert all(v.grad is None for k, v in m.named_parameters() if not k.startswith("mean_module"))
    again = _got(m, pp, which, dt, xs, up)[1]
    assert torch.equal(grad, again)                                   # fixed-order sums


@pytest.mark.parametrize("which", MODELS)
def test_gradcheck_in_float64(plmc, which):
    m, pp, xs = _built(which, torch.float64)
    x = xs.to(DEV).requires_grad_()
    assert torch.autograd.gradcheck(lambda t: pp(t, differentiable=True), (x,), eps=1e-6, atol=1e-6, rtol=1e-5, nondet_tol=0.0)


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("which", JACOBIAN_MODELS)
def test_jacobian_equals_the_rows_of_the_gradient(plmc, which, dt):
    m, pp, xs = _built(which, dt)
    x = xs.to(DEV, dt)
    J = pp.jacobian(x)
    plain = pp(x)
    assert J.shape == plain.shape + (D,) and J.dtype == dt and not J.requires_grad
    feats = xs
    flat = J.reshape(NPATHS, NS, -1, D).double().cpu()                 # (P, n*, tasks | 1, d)
    for c in range(NPATHS):
        for t in range(flat.shape[2]):
            up = torch.zeros(plain.shape, dtype=torch.float64)
            up[(c, slice(None)) + ((t,) if plain.dim() == 3 else ())] = 1.0
            want, tol = _want(m, pp, which, dt, feats, up)
            err = (flat[c, :, t] - want).abs()
            assert bool((err <= tol).all()), (which, dt, c, t, float((err / tol).max()))
            if c == 0 and t == 0:                                      # and the autograd node gives the same rows
                g = _got(m, pp, which, dt, xs, up)[1].double().cpu()
                assert bool(((g - want).abs() <= tol).all()) and bool(((g - flat[c, :, t]).abs() <= 2 * tol).all())


@pytest.mark.parametrize("which", ["linear_mean", "transform"])
def test_jacobian_takes_x_as_predictive_gradients_does(plmc, which):
    m, pp, xs = _built(which, torch.float64)
    with pytest.raises(NotImplementedError, match="PosteriorPaths.jacobian serves models without an input_transform"):
        pp.jacobian(xs.to(DEV))


def test_no_dx_kernel_without_a_gradient_and_the_default_call_still_raises(plmc):
    from projectedlmc import _hip
    m, pp, xs = _built("single", torch.float32)
    x = xs.to(DEV, torch.float32)
    _hip.prof_enable(["k_cross_matvec", "k_cross_matvec_dx"])
    try:
        _hip.prof_collect()
        a = pp(x, differentiable=True)                                 # detached: the plain evaluation
        with torch.no_grad():
            b = pp(x.clone().requires_grad_(), differentiable=True)
        out = pp(x.clone().requires_grad_(), differentiable=True)      # attached, but nobody asks for the derivative
        torch.cuda.synchronize()
        rec = _hip.prof_collect()
        assert "k_cross_matvec_dx" not in rec and rec["k_cross_matvec"]["launches"] == 6
        assert not a.requires_grad and not b.requires_grad and out.requires_grad and torch.equal(a, b) and torch.equal(a, out.detach())
        out.sum().backward()
        torch.cuda.synchronize()
        assert _hip.prof_collect()["k_cross_matvec_dx"]["launches"] == 2      # the update's and the features'
    finally:
        _hip.prof_enable(False)
    with pytest.raises(NotImplementedError, match="requires a gradient is not served"):
        pp(x.clone().requires_grad_())
    again = pp.with_draws(w=torch.zeros_like(pp.w))                    # with_draws keeps working: the prior part is gone from the derivative too
    xg = x.clone().requires_grad_()
    again(xg, differentiable=True).sum().backward()
    assert xg.grad is not None and bool(torch.isfinite(xg.grad).all())
