"""Posterior draws as functions (model.sample_paths, projectedlmc/paths.py) and mean-only predictions
(settings.skip_posterior_variances) through the models, n = 130 and 257, fp64 and fp32, d = 3.

  * paths(x) equals Matheron's rule written densely in fp64 from the path's own stored tensors and the model's hyper-parameter values
    (tests/_cross_matvec_ref.py paths_dense): ExactGPModel with rbf, Scale(matern52) and a two-group decomp; ProjectedGPModel (q = 3,
    p = 5) with the mixing matrix in both storage forms;
  * two evaluations at overlapping x agree bit for bit on the shared points; a seeded generator reproduces the draw;
  * a path whose prior weights and noise draws are zero is model(x).mean;
  * under skip_posterior_variances the mean is the default call's and the variance exactly 0, for one kind of every family; n* = 5000
    on an n = 257 model, more test points than any workspace of that model holds columns, works.

Tolerances: |got - want| <= VALUE_TOL max(1, max |want|) with the values the prediction tests hold a model's output to (1e-8 in fp64,
2e-4 in fp32: tests/test_gpu_posterior_dx_model.py, tests/test_gpu_prediction_cache.py); a path is such an output -- a cross-covariance
against solved weights of the size of y.  Where two engine routes are compared their bounds add: 2 VALUE_TOL."""
import math
import warnings

import pytest
import torch
from torch.nn.utils import parametrize

import _cross_matvec_ref as cm
from oracle import gp_math as gm

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
D, P_TASKS, Q, NS, NPATHS, NFEAT = 3, 5, 3, 37, 4, 64
VALUE_TOL = {torch.float64: 1e-8, torch.float32: 2e-4}
KINDS = {"rbf": ("rbf", 2.5), "matern12": ("matern", 0.5), "matern32": ("matern", 1.5), "matern52": ("matern", 2.5)}
PATH_MODELS = ("rbf", "scale_matern52", "decomp", "projected_bulk", "projected_qr")


@pytest.fixture(scope="module")
def plmc():
    import projectedlmc
    assert torch.cuda.is_available()
    return projectedlmc


@pytest.fixture(autouse=True)
def _eager_cache():
    from projectedlmc import settings
    with settings.prediction_cache("eager"):
        yield


def _data(n, seed=1, positive=False):
    g = torch.Generator().manual_seed(seed)
    X = (2 * torch.rand(n, D, generator=g, dtype=torch.float64) - 1).float().double()
    Y = torch.stack([torch.sin(2.0 * X[:, 0] + k) * torch.cos(X[:, 1] - X[:, 2]) + 0.1 * torch.randn(n, generator=g, dtype=torch.float64)
                     for k in range(P_TASKS)], 1).float().double()
    xs = (2 * torch.rand(NS, D, generator=g, dtype=torch.float64) - 1).float().double()
    if positive:
        X, xs = (0.5 * (X + 1)).float().double(), (0.5 * (xs + 1)).float().double()
    return X, Y, xs


def _exact(plmc, X, y, dt, kernel, const=0.3, **kw):
    torch.manual_seed(3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = plmc.ExactGPModel(X, y, plmc.GaussianLikelihood(), kernel_type=kernel, **kw).double()
    if hasattr(m.mean_module, "raw_constant"):
        with torch.no_grad():
            m.mean_module.raw_constant.fill_(const)
    m.likelihood.noise = 0.1
    return m.to(dt).to(DEV).eval()


def _projected(plmc, X, Y, dt, kernel, bulk=True, **kw):
    torch.manual_seed(3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = plmc.ProjectedGPModel(X, Y, P_TASKS, Q, mean_type=plmc.ZeroMean, kernel_type=kernel, init_lmc_coeffs=True, BDN=False, bulk=bulk,
                                  **kw).double()
    return m.to(dt).to(DEV).eval()


def _build(plmc, which, n, dt):
    X, Y, xs = _data(n)
    y = Y[:, 0].contiguous()
    if which == "rbf":
        m = _exact(plmc, X, y, dt, plmc.RBFKernel)
    elif which == "scale_matern52":
        m = _exact(plmc, X, y, dt, plmc.MaternKernel, outputscales=True)
    elif which == "decomp":
        m = _exact(plmc, X, y, dt, plmc.MaternKernel, decomp=[[0, 1], [2]])
    else:
        m = _projected(plmc, X, Y, dt, plmc.MaternKernel, bulk=which == "projected_bulk")
    return m, xs


def _dense_paths(m, pp, xs):
    """paths(xs) in fp64 on the host: paths_dense on the latents, then the prior mean (exact model) or the mixing (projected model)."""
    from projectedlmc import ProjectedGPModel
    up = lambda t: t.detach().double().cpu()
    with torch.no_grad(), parametrize.cached():
        lazy = m.covar_module(m.train_inputs[0])
        ell = up(lazy.ell)
        ell = ell[:, None, :] if ell.dim() == 2 else ell
        q, G = ell.shape[:2]
        osc = torch.ones(q, G, dtype=torch.float64) if lazy.oscale is None else up(lazy.oscale).reshape(q, G)
        okind, nu = KINDS[lazy.kind]
        K = lambda A, B: sum(gm.kernel_matrix(okind, A, B, ell[:, g], osc[:, g], nu) for g in range(G))
        X = up(lazy.x1)
        projected = isinstance(m, ProjectedGPModel)
        if projected:
            noise, resid = up(m.projected_noise()), up(m.project_data(m.train_y))
        else:
            noise = up(m.likelihood.noise).reshape(-1)
            resid = up(m.train_targets).reshape(1, -1) - up(m.mean_module(m.train_inputs[0])).reshape(1, -1)
        lat = cm.paths_dense(K, X, resid, noise, up(pp.freq), up(pp.phase), up(pp.feature_scale), up(pp.w), up(pp.eps), xs)
        if projected:
            return torch.einsum("qsc,qp->csp", lat, up(m.lmc_coefficients()))
        return lat[0].T + up(m.mean_module(xs.to(DEV, m.train_targets.dtype))).reshape(1, -1)


def _close(got, want, tol, what):
    err = float((got.double().cpu() - want).abs().max())
    lim = tol * max(1.0, float(want.abs().max()))
    print("%s: largest error %.3g of %.3g allowed" % (what, err, lim))
    assert err <= lim, (what, err, lim)


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("n", [130, 257])
@pytest.mark.parametrize("which", PATH_MODELS)
def test_paths_equal_matherons_rule_from_their_stored_tensors(plmc, which, n, dt):
    m, xs = _build(plmc, which, n, dt)
    pp = m.sample_paths(NPATHS, num_features=NFEAT, generator=torch.Generator().manual_seed(11))
    G = 2 if which == "decomp" else 1
    q = Q if which.startswith("projected") else 1
    assert pp.freq.shape == (q, G * NFEAT, D) and pp.phase.shape == (q, G * NFEAT) and pp.w.shape == (NPATHS, q, G * NFEAT)
    assert pp.eps.shape == (NPATHS, q, n) and pp.v.shape == (q, n, NPATHS) and pp.freq.dtype == dt and pp.v.device.type == "cuda"
    got = pp(xs.to(DEV, dt))
    assert got.shape == ((NPATHS, NS, P_TASKS) if which.startswith("projected") else (NPATHS, NS)) and not got.requires_grad
    _close(got, _dense_paths(m, pp, xs), VALUE_TOL[dt], "%s n=%d %s" % (which, n, dt))
    if which == "decomp":                                              # a component's frequencies vanish on the dimensions it ignores
        assert bool((pp.freq[:, :NFEAT, 2] == 0).all()) and bool((pp.freq[:, NFEAT:, :2] == 0).all())
        assert bool((pp.freq[:, :NFEAT, :2] != 0).any())
    # evaluable anywhere later, consistent across calls: overlapping sets of points agree bit for bit where they share points
    a, b = pp(xs[:30].to(DEV, dt)), pp(torch.cat([xs[10:], xs[:3] + 0.25]).to(DEV, dt))
    assert torch.equal(a[:, 10:30], b[:, :20]) and torch.equal(a, got[:, :30])
    with pytest.raises(NotImplementedError, match="requires a gradient"):
        pp(xs.to(DEV, dt).requires_grad_())


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("which", ["scale_matern52", "projected_bulk"])
def test_a_path_without_prior_draw_and_noise_is_the_posterior_mean(plmc, which, dt):
    m, xs = _build(plmc, which, 257, dt)
    pp = m.sample_paths(2, num_features=16, generator=torch.Generator().manual_seed(1))
    zero = pp.with_draws(w=torch.zeros_like(pp.w), eps=torch.zeros_like(pp.eps))
    with torch.no_grad():
        mean = m(xs.to(DEV, dt)).mean
    got = zero(xs.to(DEV, dt))
    for c in range(2):
        _close(got[c], mean.double().cpu(), 2 * VALUE_TOL[dt], "%s path %d %s" % (which, c, dt))


def test_a_seeded_generator_reproduces_the_draw(plmc):
    m, xs = _build(plmc, "decomp", 130, torch.float32)
    a = m.sample_paths(3, num_features=32, generator=torch.Generator().manual_seed(5))
    b = m.sample_paths(3, num_features=32, generator=torch.Generator().manual_seed(5))
    c = m.sample_paths(3, num_features=32, generator=torch.Generator().manual_seed(6))
    for name in ("freq", "phase", "w", "eps", "v"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    x = xs.to(DEV, torch.float32)
    assert torch.equal(a(x), b(x)) and not torch.equal(a.w, c.w) and not torch.equal(a(x), c(x))
    cache = m._prediction_cache()
    assert cache.ws is not None and cache.hits >= 2                   # one factorisation served the three draws


def _sum_factory(**kw):
    import projectedlmc
    K = projectedlmc.kernels
    kw.pop("lengthscale_prior", None)
    B = kw.get("batch_shape", torch.Size())
    sc = lambda k: K.ScaleKernel(k, batch_shape=B)
    return sc(K.RBFKernel(**kw)) + sc(K.PeriodicKernel(**kw) * K.RBFKernel(**kw)) + sc(K.RQKernel(**kw))


def _lper_factory(**kw):
    import projectedlmc
    return projectedlmc.kernels.PeriodicKernel(**kw) * projectedlmc.kernels.RBFKernel(**kw)


FAMILY_MODELS = ("rbf", "decomp", "sm", "periodic", "rq", "locally_periodic", "sum", "poly3", "spline", "projected")


def _family_model(plmc, family, n, dt):
    X, Y, xs = _data(n, positive=family == "spline")
    y = Y[:, 0].contiguous()
    if family == "projected":
        return _projected(plmc, X, Y, dt, plmc.MaternKernel), xs
    kernel, kw = {"rbf": (plmc.RBFKernel, {}), "decomp": (plmc.MaternKernel, dict(decomp=[[0, 1], [2]])),
                  "sm": (plmc.SpectralMixtureKernel, dict(ker_kwargs=dict(num_mixtures=2))), "periodic": (plmc.PeriodicKernel, dict(outputscales=True)),
                  "rq": (plmc.RQKernel, dict(outputscales=True)), "locally_periodic": (_lper_factory, dict(outputscales=True)),
                  "sum": (_sum_factory, {}), "poly3": (plmc.PolynomialKernel, dict(ker_kwargs=dict(power=3), outputscales=True)),
                  "spline": (plmc.SplineKernel, dict(outputscales=True))}[family]
    return _exact(plmc, X, y, dt, kernel, **kw), xs


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("family", FAMILY_MODELS)
def test_mean_only_prediction_is_the_default_mean_with_zero_variance(plmc, family, dt):
    m, xs = _family_model(plmc, family, 130, dt)
    x = xs.to(DEV, dt)
    with torch.no_grad():
        full = m(x)
        with plmc.settings.skip_posterior_variances():
            only = m(x)
            again = m(x)                                               # alpha comes from the cache now
    assert type(only) is type(full) and only.mean.shape == full.mean.shape
    _close(only.mean, full.mean.double().cpu(), 2 * VALUE_TOL[dt], "%s %s" % (family, dt))
    assert only.variance.shape == full.variance.shape and bool((only.variance == 0).all())
    assert torch.equal(only.mean, again.mean)
    with torch.no_grad():
        assert bool((m(x).variance > 0).all())                        # the setting is off again


@pytest.mark.parametrize("which", ["scale_matern52", "projected_bulk"])
def test_more_test_points_than_the_workspace_holds_columns(plmc, which):
    m, xs = _build(plmc, which, 257, torch.float32)
    g = torch.Generator().manual_seed(3)
    big = torch.cat([xs, (2 * torch.rand(5000 - NS, D, generator=g, dtype=torch.float64) - 1)]).to(DEV, torch.float32)
    with torch.no_grad():
        few = m(big[:NS]).mean
        c = m._prediction_cache()
        assert c.ws is not None and c.ws.naug < 5000
        with plmc.settings.skip_posterior_variances():
            only = m(big)
        assert c.ws is not None and c.ws.naug < 5000                  # no workspace grew to hold the test points
    assert only.mean.shape[0] == 5000 and bool(torch.isfinite(only.mean).all()) and bool((only.variance == 0).all())
    _close(only.mean[:NS], few.double().cpu(), 2 * VALUE_TOL[torch.float32], which)
    pp = m.sample_paths(2, num_features=32, generator=torch.Generator().manual_seed(2))
    out = pp(big)
    assert out.shape[:2] == (2, 5000) and bool(torch.isfinite(out).all())
    assert torch.equal(out[:, :NS], pp(big[:NS]))
