"""Differentiable predictions through the models: with `x.requires_grad_()` the eval-mode posterior of ExactGPModel (two independent
tasks) and ProjectedGPModel (p = 4, q = 2) carries d mean / dx and d variance / dx from the engine's kernel (plmc_posterior_dx).  The
gradient is held against fp64 torch autograd of a dense posterior written here from the model's own hyper-parameter values, and, in
fp64, against central differences of model(x), which know nothing of the reference's formulas.  Without a gradient for x nothing
changes: same bits, same library calls.  n = 200 (n_pad = 256), n* = 37, d = 3, noise 0.1."""
import functools
import warnings

import pytest
import torch

from oracle import gp_math as gm

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N, NS, D, P, Q = 200, 37, 3, 4, 2
MODELS = ("exact", "projected")
# x.grad: |got - want| <= TOL max(1, max |want|).  fp32: 4 x the worst error measured over the cases of this file against the fp64
# reference, 1.02e-5 (the projected model through the embedding; without a transform 1.9e-6), profiles/posterior_dx_accuracy.md.  For
# scale: the prediction tests hold fp32 values to 2e-4 (VALUE_TOL) and a derivative amplifies that by about 1 / ell_min, here ~2.
TOL = {torch.float64: 1e-8, torch.float32: 4.1e-5}
VALUE_TOL = {torch.float64: 1e-8, torch.float32: 2e-4}


@pytest.fixture(scope="module")
def plmc():
    import projectedlmc
    assert torch.cuda.is_available()
    return projectedlmc


def _data(din=D, seed=1):
    g = torch.Generator().manual_seed(seed)
    X = (2 * torch.rand(N, din, generator=g, dtype=torch.float64) - 1).float().double()
    Y = torch.stack([torch.sin(2.0 * X[:, 0] + k) * torch.cos(X[:, 1] - X[:, -1]) + 0.1 * torch.randn(N, generator=g, dtype=torch.float64)
                     for k in range(P)], 1).float().double()
    xs = (2 * torch.rand(NS, din, generator=g, dtype=torch.float64) - 1).float().double()
    a, b = torch.randn(NS, P, generator=g, dtype=torch.float64), torch.randn(NS, P, generator=g, dtype=torch.float64)
    return X, Y, xs, a, b


def _embedding():
    torch.manual_seed(5)
    return torch.nn.Linear(5, 3).double()


def _build(plmc, which, dt, transform=False, kernel=None):
    """An eval-mode model on the device with perturbed lengthscales, noise 0.1 and (exact) non-zero constant means."""
    X, Y, xs, a, b = _data(5 if transform else D)
    tf = _embedding() if transform else None
    kernel = plmc.MaternKernel if kernel is None else kernel
    torch.manual_seed(3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if which == "exact":
            m = plmc.ExactGPModel(X, Y[:, :2].T.contiguous(), plmc.GaussianLikelihood(batch_shape=torch.Size([2])), n_tasks=2,
                                  kernel_type=kernel, input_transform=tf)
            with torch.no_grad():
                m.mean_module.raw_constant.copy_(torch.tensor([0.3, -0.2]))
        else:
            m = plmc.ProjectedGPModel(X, Y, P, Q, mean_type=plmc.ZeroMean, kernel_type=kernel, init_lmc_coeffs=True, BDN=False,
                                      input_transform=tf)
    m = m.double()
    m.likelihood.noise = 0.1
    if getattr(m.covar_module, "lengthscale", None) is not None:
        g = torch.Generator().manual_seed(9)
        m.covar_module.lengthscale = 0.5 + 0.4 * torch.rand(m.covar_module.lengthscale.shape, generator=g, dtype=torch.float64)
    return m.to(dt).to(DEV).eval()


def _reference_posterior(m, which, X, Y, feats):
    """(mean, variance), (n*, tasks) each, of the model at the FEATURES `feats` (n*, 3): a dense fp64 Cholesky posterior from the model's own
    values, a differentiable function of feats."""
    with torch.no_grad():
        tx = m._features(m.train_inputs[0], grad=False).double().cpu()
        q = 2 if which == "exact" else Q
        ell = m.covar_module.lengthscale.detach().double().cpu().reshape(q, D)
        if which == "exact":
            noise = m.likelihood.noise.detach().double().cpu().reshape(q)
            const = m.mean_module.raw_constant.detach().double().cpu().reshape(q, 1)
            y = m.train_targets.double().cpu().reshape(q, N) - const
        else:
            noise = m.projected_noise().detach().double().cpu().reshape(q)
            y = m.project_data(m.train_y).detach().double().cpu()
            Ht = m.lmc_coefficients().detach().double().cpu()
    K = lambda A, B: gm.kernel_matrix("matern", A, B, ell, None, 2.5)
    Lc = torch.linalg.cholesky(K(tx, tx) + noise[:, None, None] * torch.eye(N, dtype=torch.float64))
    V = torch.linalg.solve_triangular(Lc, K(tx, feats), upper=False)                 # (q, n, n*)
    z = torch.linalg.solve_triangular(Lc, y.unsqueeze(-1), upper=False)
    mean, var = (V * z).sum(1), 1.0 - (V * V).sum(1)                                  # (q, n*)
    if which == "exact":
        return (mean + const).T, var.T
    return mean.T @ Ht, var.T @ (Ht * Ht) + m.eps


def _want(m, which, transform=False):
    """(d sum(a mean + b variance) / dx by fp64 autograd of the reference, mean, variance) at the raw test points."""
    X, Y, xs, a, b = _data(5 if transform else D)
    x = xs.clone().requires_grad_()
    feats = x
    if transform:
        tf = m.input_transform
        W, c = tf.weight.detach().double().cpu(), tf.bias.detach().double().cpu()
        feats = x @ W.T + c
    mean, var = _reference_posterior(m, which, X, Y, feats)
    t = mean.shape[1]
    g, = torch.autograd.grad((a[:, :t] * mean + b[:, :t] * var).sum(), x)
    return g, mean.detach(), var.detach()


def _got(m, which, dt, transform=False, grad=True):
    X, Y, xs, a, b = _data(5 if transform else D)
    x = xs.to(DEV, dt).requires_grad_(grad)
    out = m(x)
    mean, var = out.mean, out.variance
    if which == "exact":                                                             # a batch of independent GPs: (tasks, n*)
        mean, var = mean.T, var.T
    if grad:
        t = mean.shape[1]
        (a[:, :t].to(DEV, dt) * mean + b[:, :t].to(DEV, dt) * var).sum().backward()
    torch.cuda.synchronize()
    return x.grad, mean.detach(), var.detach()


def _close(got, want, tol, what):
    err = float((got.cpu().double() - want).abs().max()) / max(1.0, float(want.abs().max()))
    print("%s: error %.3e of max(1, max |want|) (tolerance %.1e)" % (what, err, tol))
    assert err <= tol, (what, err)


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("which", MODELS)
def test_gradient_of_mean_and_variance_reaches_the_test_inputs(plmc, which, dt):
    """On the parent commit: "element 0 of tensors does not require grad"."""
    m = _build(plmc, which, dt)
    want, wmean, wvar = _want(m, which)
    got, mean, var = _got(m, which, dt)
    assert got is not None and got.dtype == dt and got.shape == (NS, D)
    _close(mean, wmean, VALUE_TOL[dt], "%s %s mean" % (which, dt))
    _close(var, wvar, VALUE_TOL[dt], "%s %s variance" % (which, dt))
    _close(got, want, TOL[dt], "%s %s x.grad" % (which, dt))
    # hyper-parameters, noise and training data are constants of the node (the prior mean is plain torch and differentiates by itself)
    assert all(v.grad is None for k, v in m.named_parameters() if not k.startswith("mean_module"))


@pytest.mark.parametrize("which", MODELS)
def test_central_differences_of_the_model_agree(plmc, which):
    m = _build(plmc, which, torch.float64)
    X, Y, xs, a, b = _data()
    got = _got(m, which, torch.float64)[0].cpu()
    t = 2 if which == "exact" else P
    a, b = a[:, :t].to(DEV), b[:, :t].to(DEV)
    h = 1e-5
    fd = torch.empty(NS, D, dtype=torch.float64)
    with torch.no_grad():
        for k in range(D):
            e = torch.zeros(NS, D, dtype=torch.float64)
            e[:, k] = h
            vals = []
            for sgn in (1.0, -1.0):
                out = m((xs + sgn * e).to(DEV))
                mean, var = (out.mean.T, out.variance.T) if which == "exact" else (out.mean, out.variance)
                vals.append((a * mean + b * var).sum(1))                 # test points do not interact: one difference each
            fd[:, k] = ((vals[0] - vals[1]) / (2 * h)).cpu()
    err = float((got - fd).abs().max() / fd.abs().max())
    print("%s: central differences, relative error %.3e" % (which, err))
    assert err <= 1e-6, err


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("which", MODELS)
def test_values_and_library_calls_do_not_depend_on_requires_grad(plmc, which, dt, monkeypatch):
    """mean and variance are the same bits with and without x.requires_grad -- compared on one route, a cache hit: a differentiable miss
    builds the cache at once, which is another sweep than the plain miss -- and a call without it makes the library calls it made before:
    nothing of the Jacobian path."""
    from projectedlmc import _hip
    L = _hip.lib()
    calls = []
    real = L.call

    def recording(base, dtype, *args):
        if base != "plmc_qr_small":                                                  # (the projected model's mixing matrix, not the posterior)
            calls.append(base)
        return real(base, dtype, *args)

    monkeypatch.setattr(L, "call", recording)
    m = _build(plmc, which, dt)
    _got(m, which, dt, grad=False)                                                   # miss: the plain sweep
    seq_miss = list(calls)
    _got(m, which, dt, grad=False)                                                   # the second call builds the cache
    del calls[:]
    plain = _got(m, which, dt, grad=False)                                           # hit
    seq_plain = list(calls)
    del calls[:]
    withx = _got(m, which, dt, grad=True)                                            # hit, differentiable
    seq_x = list(calls)
    assert plain[0] is None and withx[0] is not None
    assert torch.equal(plain[1], withx[1]) and torch.equal(plain[2], withx[2])
    extra = ("plmc_extract_col", "plmc_wt_matvec", "plmc_gemm_tn_tri", "plmc_posterior_dx")
    assert [c for c in seq_x if c not in extra] == seq_plain
    assert [c for c in seq_x if c in extra] == list(extra)
    assert not any(c in extra for c in seq_miss + seq_plain)
    # what the parent commit's calls were: sweep on a miss, substitution on a hit, then the moments (and the mixing)
    tail = ["plmc_posterior_moments"] + (["plmc_mix_posterior"] if which == "projected" else [])
    assert seq_miss == ["plmc_write_rhs", "plmc_assemble_cross", "plmc_factorize_ex"] + tail
    assert seq_plain == ["plmc_write_rhs", "plmc_assemble_cross", "plmc_potrs_aug_kept" if dt == torch.float32 else "plmc_potrs_aug"] + tail


@pytest.mark.parametrize("which", MODELS)
def test_miss_build_and_hit_give_the_same_gradient(plmc, which):
    """The first differentiable call with a cache present builds it at once; without a cache (settings.prediction_cache("off")) a pooled
    workspace with the inverse factor serves."""
    from projectedlmc import settings
    dt = torch.float32
    m = _build(plmc, which, dt)
    want = _want(m, which)[0]
    cache = m._prediction_cache()
    with settings.prediction_cache("off"):
        off = _got(m, which, dt)[0]
        assert cache.ws is None
    built = _got(m, which, dt)[0]                                                    # miss -> build
    assert cache.ws is not None and cache.ws.with_inverse and (cache.hits, cache.misses) == (0, 1)
    hit = _got(m, which, dt)[0]
    assert (cache.hits, cache.misses) == (1, 1)
    for name, g in (("off", off), ("build", built), ("hit", hit)):
        _close(g, want, TOL[dt], "%s %s" % (which, name))
    m64 = _build(plmc, which, torch.float64)
    want = _want(m64, which)[0]
    for name in ("build", "hit"):
        _close(_got(m64, which, torch.float64)[0], want, TOL[torch.float64], "%s fp64 %s" % (which, name))


@pytest.mark.parametrize("which", MODELS)
def test_mean_only_work_skips_the_product(plmc, which, monkeypatch):
    from projectedlmc import _hip, settings
    dt = torch.float64
    m = _build(plmc, which, dt)
    X, Y, xs, a, b = _data()
    t = 2 if which == "exact" else P
    a = a[:, :t].to(DEV)
    x = xs.to(DEV).requires_grad_()
    a = a.T if which == "exact" else a                                                # (a batch of independent GPs: (tasks, n*))
    (a * m(x).mean).sum().backward()
    both = x.grad.clone()
    L = _hip.lib()
    calls = []
    real = L.call
    monkeypatch.setattr(L, "call", lambda base, dtype, *args: (calls.append(base), real(base, dtype, *args))[1])
    x.grad = None
    with settings.predictive_variance_grad(False):
        out = m(x)
        assert out.mean.requires_grad and not out.variance.requires_grad
        (a * out.mean).sum().backward()
    assert torch.equal(x.grad, both)
    assert "plmc_gemm_tn_tri" not in calls and "plmc_posterior_dx" in calls


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("which", MODELS)
def test_gradient_reaches_the_raw_inputs_through_an_input_transform(plmc, which, dt):
    """A linear embedding 5 -> 3: x.grad is the reference's chain rule, and no parameter of the transform gets a .grad."""
    m = _build(plmc, which, dt, transform=True)
    want = _want(m, which, transform=True)[0]
    got = _got(m, which, dt, transform=True)[0]
    assert got.shape == (NS, 5)
    _close(got, want, TOL[dt], "%s %s through the embedding" % (which, dt))
    assert all(prm.grad is None for prm in m.input_transform.parameters())


@pytest.mark.parametrize("which", MODELS)
def test_refusals_name_the_option_or_the_kind(plmc, which):
    m = _build(plmc, which, torch.float64)
    x = _data()[2].to(DEV).requires_grad_()
    with pytest.raises(NotImplementedError, match="full_cov"):
        m(x, full_cov=True)
    m(x.detach(), full_cov=True)                                                     # served as before without a gradient
    lin = _build(plmc, which, torch.float64, kernel=plmc.LinearKernel)
    with pytest.raises(NotImplementedError, match="linear"):
        lin(x)
    lin(x.detach())
    with pytest.raises(NotImplementedError, match="linear"):
        lin.predictive_gradients(x)


def test_the_latent_sharded_model_refuses_by_name(plmc):
    m = _build(plmc, "projected", torch.float64)
    m.set_latent_shard((0, 2))
    with pytest.raises(NotImplementedError, match="latent_shard"):
        m._latent_posterior(_data()[2].to(DEV).requires_grad_())


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("which", MODELS)
def test_predictive_gradients_equal_the_autograd_jacobian(plmc, which, dt):
    """Back-propagating unit vectors task by task gives the Jacobian (test points do not interact); predictive_gradients reads the same
    kernel output without a graph."""
    m = _build(plmc, which, dt)
    xs = _data()[2].to(DEV, dt)
    m.predictive_gradients(xs)                                                       # builds the cache: every call below is a hit on the same factor
    dm, dv = m.predictive_gradients(xs)
    t = 2 if which == "exact" else P
    assert dm.shape == dv.shape == (NS, t, D) and not dm.requires_grad
    for task in range(t):
        for got, pick in ((dm, lambda o: o.mean), (dv, lambda o: o.variance)):
            x = xs.clone().requires_grad_()
            (pick(m(x))[task] if which == "exact" else pick(m(x))[:, task]).sum().backward()
            tol = 1e-12 if dt == torch.float64 else 1e-5
            scale = max(1.0, float(x.grad.abs().max()))
            assert float((got[:, task] - x.grad).abs().max()) <= tol * scale, (which, task)
    single = plmc.ExactGPModel(*(lambda d: (d[0], d[1][:, 0].contiguous()))(_data()), plmc.GaussianLikelihood(),
                               kernel_type=plmc.MaternKernel).to(dt).to(DEV).eval()
    dm, dv = single.predictive_gradients(xs)
    assert dm.shape == dv.shape == (NS, D)
