"""settings.posterior_hyper_grad through the models: the eval-mode posterior of ExactGPModel (every kernel kind the exact engine trains, one
and two tasks) and of ProjectedGPModel (p = 5, q = 2, bulk and separately parametrised mixing matrix) carries the gradient with respect
to EVERY parameter -- raw, through the constraints -- the noise and the training targets.  The reference is autograd through a dense fp64
posterior restated here from a float64 host copy of the model's own parameters (its constraints, kernel tables, projection and mixing are
plain torch; the dense kernels are _weighted_grad_ref.dense_kernel's).  Two losses: random weights on mean and variance, and the held-out
Gaussian negative log likelihood through the likelihood.  With the setting off nothing changes: same bits, `.grad is None`.
n = 200 (n_pad = 256), n* in {70, 1}, d = 3, noise 0.1.

Tolerance: || got - want || <= TOL max(|| want ||, FLOOR || all gradients ||) per parameter tensor.  fp64: 1e-7, the rtol of the fp64
MLL-gradient parity tests (measured: 5e-11 at most).  fp32: 4 x the worst value measured over the cases of this file against the fp64
reference (profiles/weighted_grad_accuracy.md): 8.84e-4 over every kind but the polynomial kernel, 6.63e-3 for that one (the output
scale's gradient; its Khat is a rank-10 matrix plus the noise, condition number ~ 1e4, and the fp32 factorisation carries that)."""
import copy
import math
import warnings

import pytest
import torch
from torch.nn.utils import parametrize

import _posterior_dx_dense as pdd
import _weighted_grad_ref as wgr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N, D, P_TASKS, Q = 200, 3, 5, 2
TOL = {torch.float64: 1e-7, torch.float32: 3.6e-3}
TOL_POLY32 = 2.7e-2
FLOOR = 1e-3               # a parameter whose gradient nearly vanishes is held to this fraction of the whole gradient's norm
DTYPES = [torch.float64, torch.float32]
DT_IDS = ["float64", "float32"]


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


def _data(ns, positive=False, seed=1):
    g = torch.Generator().manual_seed(seed)
    X = (2 * torch.rand(N, D, generator=g, dtype=torch.float64) - 1).float().double()
    Y = torch.stack([torch.sin(2.0 * X[:, 0] + k) * torch.cos(X[:, 1] - X[:, 2]) + 0.1 * torch.randn(N, generator=g, dtype=torch.float64)
                     for k in range(P_TASKS)], 1).float().double()
    xs = (2 * torch.rand(ns, D, generator=g, dtype=torch.float64) - 1).float().double()
    if positive:
        X, xs = (0.5 * (X + 1)).float().double(), (0.5 * (xs + 1)).float().double()
    yv = torch.stack([torch.sin(2.0 * xs[:, 0] + k) * torch.cos(xs[:, 1] - xs[:, 2]) for k in range(P_TASKS)], 1).float().double()
    w = torch.randn(2, ns, P_TASKS, generator=g, dtype=torch.float64)
    return X, Y, xs, yv, w


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


KINDS = ("matern52", "scale_rbf", "decomp", "sm", "periodic", "rq", "locally_periodic", "poly2", "sum", "spline")


def _kernel(plmc, kind):
    return {"matern52": (plmc.MaternKernel, {}), "scale_rbf": (plmc.RBFKernel, dict(outputscales=True)),
            "decomp": (plmc.MaternKernel, dict(decomp=[[0, 1], [2]])),
            "sm": (plmc.SpectralMixtureKernel, dict(ker_kwargs=dict(num_mixtures=2))), "periodic": (plmc.PeriodicKernel, dict(outputscales=True)),
            "rq": (plmc.RQKernel, dict(outputscales=True)), "locally_periodic": (_lper_factory, dict(outputscales=True)),
            "poly2": (plmc.PolynomialKernel, dict(ker_kwargs=dict(power=2), outputscales=True)), "sum": (_sum_factory, {}),
            "spline": (plmc.SplineKernel, dict(outputscales=True))}[kind]


def _exact(plmc, kind, tasks, dt, ns):
    X, Y, xs, yv, w = _data(ns, positive=kind == "spline")
    kernel, kw = _kernel(plmc, kind)
    torch.manual_seed(3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if tasks == 1:
            m = plmc.ExactGPModel(X, Y[:, 0].contiguous(), plmc.GaussianLikelihood(), kernel_type=kernel, **kw).double()
        else:
            m = plmc.ExactGPModel(X, Y[:, :2].T.contiguous(), plmc.GaussianLikelihood(batch_shape=torch.Size([2])), n_tasks=2,
                                  kernel_type=kernel, **kw).double()
    with torch.no_grad():
        m.mean_module.raw_constant.copy_(torch.tensor([0.3, -0.2])[:tasks].reshape(m.mean_module.raw_constant.shape))
    m.likelihood.noise = 0.1
    return m.to(dt).to(DEV).eval(), xs, yv[:, :tasks], w[:, :, :tasks]


def _projected(plmc, bulk, dt, ns):
    X, Y, xs, yv, w = _data(ns)
    torch.manual_seed(3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = plmc.ProjectedGPModel(X, Y, P_TASKS, Q, mean_type=plmc.ZeroMean, kernel_type=plmc.MaternKernel, init_lmc_coeffs=True, BDN=False,
                                  bulk=bulk).double()
    m.likelihood.noise = 0.1
    return m.to(dt).to(DEV).eval(), xs, yv, w


def _moments(out, m):
    """(mean, variance) as (n*, tasks)"""
    mean, var = out.mean, out.variance
    if mean.dim() == 1:
        return mean[:, None], var[:, None]
    from projectedlmc import ProjectedGPModel
    return (mean, var) if isinstance(m, ProjectedGPModel) else (mean.T, var.T)


def _reference_moments(ref, x):
    """(mean, variance) (n*, tasks) of a float64 host copy `ref` of the model: a dense Cholesky posterior, differentiable in every
    parameter of ref and in ref.train_targets / ref.train_y."""
    from projectedlmc import ProjectedGPModel
    tx = ref.train_inputs[0]
    lazy = ref.covar_module(tx)
    K = wgr.dense_kernel(lazy.kind, lazy.ell, lazy.oscale)
    xsel = ref.covar_module.select(x)
    if isinstance(ref, ProjectedGPModel):
        y, noise = ref.project_data(ref.train_y), ref.projected_noise()
        mean, var = pdd.dense_posterior(K, lazy.x1, y, noise, xsel)
        Ht = ref.lmc_coefficients()
        return mean.T @ Ht, var.T @ (Ht * Ht) + ref.eps
    noise = ref.likelihood.noise.reshape(-1)
    y = ref._latent_targets() - ref.mean_module(tx).reshape(ref.n_tasks, -1)
    mean, var = pdd.dense_posterior(K, lazy.x1, y, noise, xsel)
    return (mean + ref.mean_module(x).reshape(ref.n_tasks, -1)).T, var.T


def _host_copy(m):
    ref = copy.deepcopy(m).cpu().double()
    for p in ref.parameters():
        p.grad = None
    return ref


def _targets(m):
    from projectedlmc import ProjectedGPModel
    return "train_y" if isinstance(m, ProjectedGPModel) else "train_targets"


def _loss_weights(mean, var, w):
    return (w[0].to(mean) * mean).sum() + (w[1].to(var) * var).sum()


def _want(m, xs, loss, targets=True):
    """{name: gradient} of every parameter and of the training targets, by autograd through the dense fp64 posterior"""
    ref = _host_copy(m)
    name = _targets(ref)
    if targets:
        t = getattr(ref, name).detach().clone().requires_grad_(True)
        if name == "train_y":
            del ref._buffers["train_y"]
            ref.train_y = t
        else:
            ref.train_targets = t
    with parametrize.cached():
        mean, var = _reference_moments(ref, xs)
        loss(mean, var, ref).backward()
    out = {k: (torch.zeros_like(p) if p.grad is None else p.grad) for k, p in ref.named_parameters()}
    if targets:
        out["<targets>"] = t.grad
    return out


def _got(m, xs, dt, loss, targets=True, x_grad=False):
    from projectedlmc import settings
    for p in m.parameters():
        p.grad = None
    name = _targets(m)
    t = getattr(m, name)
    t.grad = None
    t.requires_grad_(targets)
    x = xs.to(DEV, dt).requires_grad_(x_grad)
    with settings.posterior_hyper_grad(True):
        mean, var = _moments(m(x), m)
        loss(mean, var, m).backward()
    torch.cuda.synchronize()
    out = {k: (None if p.grad is None else p.grad.detach().double().cpu()) for k, p in m.named_parameters()}
    if targets:
        out["<targets>"] = t.grad.detach().double().cpu()
    t.requires_grad_(False)
    return out, (None if x.grad is None else x.grad.detach().clone()), mean.detach(), var.detach()


def _compare(got, want, dt, what):
    total = math.sqrt(sum(float(v.norm()) ** 2 for v in want.values()))
    worst = 0.0
    for k, w in want.items():
        assert got[k] is not None, "%s: no gradient reached %s" % (what, k)
        g = torch.nan_to_num(got[k].reshape(w.shape), nan=float("inf"))
        err = float((g - torch.nan_to_num(w, nan=0.0)).norm()) / max(float(torch.nan_to_num(w, nan=0.0).norm()), FLOOR * total, 1e-300)
        worst = max(worst, err)
        print("hyper_grad %s %s %-45s error %.3e of its norm" % (what, "f64" if dt == torch.float64 else "f32", k, err))
    tol = TOL_POLY32 if (dt == torch.float32 and "poly" in what) else TOL[dt]
    print("hyper_grad %s %s worst %.3e (tolerance %.1e)" % (what, "f64" if dt == torch.float64 else "f32", worst, tol))
    assert worst <= tol, (what, worst)


def _nll_exact(mean, var, m):
    """held-out Gaussian negative log likelihood, from the moments: what -likelihood(model(x)).log_prob(y) computes"""
    s2 = var + m.likelihood.noise.reshape(1, -1).to(var)
    yv = m._yv.to(mean)
    return 0.5 * ((yv - mean) ** 2 / s2 + s2.log() + math.log(2 * math.pi)).sum()


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("ns", [70, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_exact_model_every_parameter_noise_and_targets(plmc, kind, ns, dt):
    """On the parent commit: no such setting.  Every kind at n* = 70 and at n* = 1 (the test block is one row, r_pad = 16 mostly
    padding); one and two tasks rotate over the kinds."""
    tasks = (2, 1)[(KINDS.index(kind) + (ns == 1)) % 2]
    m, xs, yv, w = _exact(plmc, kind, tasks, dt, ns)
    loss = lambda mean, var, mod: _loss_weights(mean, var, w)
    got = _got(m, xs, dt, loss)[0]
    _compare(got, _want(m, xs, loss), dt, "exact %s tasks=%d n*=%d weights" % (kind, tasks, ns))


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("tasks,ns", [(1, 1), (2, 1), (1, 70), (2, 70)])
def test_exact_model_held_out_nll_through_the_likelihood(plmc, tasks, ns, dt):
    """loss = -likelihood(model(x_val)).log_prob(y_val); loss.backward() -- the lines of the issue -- against the same loss written from
    the reference's moments"""
    from projectedlmc import settings
    m, xs, yv, w = _exact(plmc, "matern52", tasks, dt, ns)
    for p in m.parameters():
        p.grad = None
    m.train_targets.requires_grad_(True)
    x, y_val = xs.to(DEV, dt), (yv[:, 0] if tasks == 1 else yv.T).to(DEV, dt)
    with settings.posterior_hyper_grad(True):
        loss = -m.likelihood(m(x)).log_prob(y_val).sum()
        loss.backward()
    got = {k: p.grad.detach().double().cpu() for k, p in m.named_parameters()}
    got["<targets>"] = m.train_targets.grad.detach().double().cpu()
    m.train_targets.requires_grad_(False)
    m.train_targets.grad = None

    def nll(mean, var, mod):
        mod._yv = yv
        return _nll_exact(mean, var, mod)
    want = _want(m, xs, nll)
    assert all(v is not None for v in got.values())
    _compare(got, want, dt, "exact nll tasks=%d n*=%d" % (tasks, ns))


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_values_are_the_same_bits_and_x_gradient_too(plmc, dt):
    """mean and variance with the setting are the bits of the call without it (compared on one route, a cache hit); with x.requires_grad
    as well one backward fills both, and x.grad is the bits of today's differentiable prediction"""
    from projectedlmc import settings
    m, xs, yv, w = _exact(plmc, "matern52", 2, dt, 70)
    loss = lambda mean, var, mod: _loss_weights(mean, var, w)
    x = xs.to(DEV, dt)
    with torch.no_grad():
        m(x)                                                                         # builds the cache
        plain = _moments(m(x), m)                                                    # hit
    xg = xs.to(DEV, dt).requires_grad_()
    mean, var = _moments(m(xg), m)                                                   # today's differentiable prediction
    loss(mean, var, m).backward()
    x_today = xg.grad.detach().clone()
    assert all(p.grad is None for k, p in m.named_parameters() if not k.startswith("mean_module"))   # the setting is off
    got, x_both, mean_h, var_h = _got(m, xs, dt, loss, x_grad=True)
    assert torch.equal(mean_h, plain[0]) and torch.equal(var_h, plain[1])
    assert x_both is not None and torch.equal(x_both, x_today)
    _compare(got, _want(m, xs, loss), dt, "exact matern52 with x.grad")
    got2, _, mean2, var2 = _got(m, xs, dt, loss)                                     # without x: the transposed product's route
    assert torch.equal(mean2, plain[0]) and torch.equal(var2, plain[1])
    for k in got:
        assert torch.allclose(got[k], got2[k], rtol=TOL[dt], atol=TOL[dt] * float(got[k].abs().max()))


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_mean_only_route_forms_no_b_product(plmc, dt):
    """predictive_variance_grad(False): r = 2, no B product, and the gradients of a loss of the mean are those of the full route"""
    from projectedlmc import settings, _engine
    m, xs, yv, w = _exact(plmc, "scale_rbf", 1, dt, 70)
    loss = lambda mean, var, mod: (w[0].to(mean) * mean).sum()
    full = _got(m, xs, dt, loss)[0]
    before = dict(_engine.hyper_grad_counters)
    with settings.predictive_variance_grad(False):
        only, _, mean, var = _got(m, xs, dt, loss)
    after = _engine.hyper_grad_counters
    assert after["b_products"] == before["b_products"] and after["mean_only_solves"] == before["mean_only_solves"] + 1
    assert after["weighted_grad_calls"] == before["weighted_grad_calls"] + 1
    assert not var.requires_grad
    _compare(only, _want(m, xs, loss), dt, "exact scale_rbf mean-only")
    for k in full:
        assert torch.allclose(only[k], full[k], rtol=10 * TOL[dt], atol=10 * TOL[dt] * max(float(full[k].abs().max()), 1e-30)), k


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_cache_hits_and_rebuild_after_an_optimiser_step(plmc, dt):
    from projectedlmc import settings
    m, xs, yv, w = _exact(plmc, "matern52", 1, dt, 70)
    loss = lambda mean, var, mod: _loss_weights(mean, var, w)
    cache = m._prediction_cache()
    first = _got(m, xs, dt, loss)[0]
    misses = cache.misses
    second = _got(m, xs, dt, loss)[0]
    assert cache.hits >= 1 and cache.misses == misses                                # the second call hits the prediction cache
    for k in first:
        assert torch.equal(first[k], second[k]), k
    opt = torch.optim.SGD(m.parameters(), lr=1e-4)
    opt.step()                                                                       # (the gradients of the second call)
    third = _got(m, xs, dt, loss)[0]
    assert cache.misses == misses + 1                                                # rebuilt for the new parameters
    _compare(third, _want(m, xs, loss), dt, "exact matern52 after a step")


def test_with_the_setting_off_nothing_reaches_the_parameters(plmc):
    m, xs, yv, w = _exact(plmc, "matern52", 1, torch.float64, 70)
    for p in m.parameters():
        p.grad = None
    mean, var = _moments(m(xs.to(DEV)), m)
    assert not var.requires_grad
    _loss_weights(mean, var, w).backward()                                           # (the prior mean at x* is plain torch)
    assert all(p.grad is None for k, p in m.named_parameters() if not k.startswith("mean_module"))


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("bulk", [True, False], ids=["bulk", "q_r"])
def test_projected_model_every_parameter(plmc, bulk, dt):
    """latent kernels, projected noise, the mixing parameters (both routes: through the projection of the data and through the mixing
    of the moments) and the training targets; n* = 70 with the bulk matrix, n* = 1 with the separately parametrised one"""
    m, xs, yv, w = _projected(plmc, bulk, dt, 70 if bulk else 1)
    loss = lambda mean, var, mod: _loss_weights(mean, var, w)
    got = _got(m, xs, dt, loss)[0]
    want = _want(m, xs, loss)
    used = {k: v for k, v in want.items() if float(v.abs().max()) > 0 or got[k] is not None}     # (B~ does not enter the posterior)
    _compare({k: (torch.zeros_like(want[k]) if got[k] is None else got[k]) for k in used}, used, dt, "projected %s" % ("bulk" if bulk else "q_r"))
    assert any("lmc_coefficients" in k and float(v.abs().max()) > 0 for k, v in want.items())


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_projected_model_held_out_nll_through_the_full_likelihood(plmc, dt):
    from projectedlmc import settings
    m, xs, yv, w = _projected(plmc, True, dt, 70)
    for p in m.parameters():
        p.grad = None
    lik = m.full_likelihood()
    Sigma = lik.task_noise_matrix().detach().double().cpu()
    with settings.posterior_hyper_grad(True):
        loss = -lik(m(xs.to(DEV, dt))).log_prob(yv.to(DEV, dt))
        loss.backward()
    got = {k: (None if p.grad is None else p.grad.detach().double().cpu()) for k, p in m.named_parameters()}

    def nll(mean, var, ref):
        Ht = ref.lmc_coefficients()                                                  # the p x p block of every point, from the latent variances
        tx = ref.train_inputs[0]
        lazy = ref.covar_module(tx)
        K = wgr.dense_kernel(lazy.kind, lazy.ell, lazy.oscale)
        _, v = pdd.dense_posterior(K, lazy.x1, ref.project_data(ref.train_y), ref.projected_noise(), ref.covar_module.select(xs))
        C = torch.einsum("qs,qa,qb->sab", v, Ht, Ht) + ref.eps * torch.eye(P_TASKS, dtype=torch.float64) + Sigma
        Lc = torch.linalg.cholesky(C)
        z = torch.linalg.solve_triangular(Lc, (yv - mean).unsqueeze(-1), upper=False).squeeze(-1)
        return 0.5 * (z * z).sum() + torch.diagonal(Lc, dim1=-2, dim2=-1).log().sum() + 0.5 * yv.numel() * math.log(2 * math.pi)
    want = _want(m, xs, nll, targets=False)
    used = {k: v for k, v in want.items() if float(v.abs().max()) > 0 or got[k] is not None}
    _compare({k: (torch.zeros_like(want[k]) if got[k] is None else got[k]) for k in used}, used, dt, "projected nll")
