"""get_fantasy_model: a fitted eval-mode model conditioned on m new observations through the bordered update of its cached
factorisation (plmc_factor_extend) instead of a new sweep.

Parity: the fantasy model's mean and variance equal those of a model of the same class constructed on the concatenated data with the
same state_dict -- a fresh full factorisation on the engine -- within the tolerances of tests/test_gpu_prediction_cache.py (1e-8 of the
largest value in fp64, 2e-4 in fp32), and in fp64 a dense torch posterior (the kernel matrix from the assembly kernel, every solve on the
host in fp64).  ExactGPModel (n = 300, d = 3, two batch tasks, constant mean) and ProjectedGPModel (n = 300, p = 5, q = 3); Matern-5/2,
poly2 (a non-unit diagonal) and a sum of two families; m = 1, 7 and 130 (two chunks, the second in place); prediction_cache("eager").
Cache behaviour, the other eval-mode paths on the fantasy model, a base factor that needed jitter, and every refusal by name."""
import math
import warnings

import pytest
import torch

from _bridge import perturb_

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N, D, NS, MMAX = 300, 3, 40, 130
TOL = {torch.float64: 1e-8, torch.float32: 2e-4}


@pytest.fixture(autouse=True)
def _eager_cache():
    from projectedlmc import settings
    with settings.prediction_cache("eager"):
        yield


@pytest.fixture(scope="module", autouse=True)
def _release_what_the_module_holds():
    """the shared base models and their cached workspaces, the engine's pooled workspaces and the allocator's cached blocks go when the
    module is done: the modules that follow start from the memory they would have found without this one"""
    yield
    import gc
    from projectedlmc import _engine
    _bases.clear()
    _engine.free_workspaces()
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def _nothing_more_after_a_gpu_error():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("HIP error, nothing more is started: %s" % e, returncode=3)


def _sum_factory(**kw):
    """k = ScaleKernel(RBF) + ScaleKernel(RQ): a sum of two families"""
    import projectedlmc
    K = projectedlmc.kernels
    kw.pop("lengthscale_prior", None)
    B = kw.get("batch_shape", torch.Size())
    return K.ScaleKernel(K.RBFKernel(**kw), batch_shape=B) + K.ScaleKernel(K.RQKernel(**kw), batch_shape=B)


def _kernel_args(kind):
    import projectedlmc as plmc
    return {"matern52": dict(kernel_type=plmc.MaternKernel),
            "poly2": dict(kernel_type=plmc.PolynomialKernel, ker_kwargs={"power": 2}, outputscales=True),
            "sum": dict(kernel_type=_sum_factory)}[kind]


def _data(dtype, p):
    g = torch.Generator().manual_seed(5)
    X = (2 * torch.rand(N + MMAX, D, generator=g, dtype=torch.float64) - 1).to(dtype)
    Y = torch.stack([torch.sin(2.0 * X[:, 0].double() + k) * torch.cos(X[:, 1].double() - X[:, 2].double()) for k in range(p)], 1)
    Y = (Y + 0.1 * torch.randn(N + MMAX, p, generator=g, dtype=torch.float64)).to(dtype)
    Xs = (2 * torch.rand(NS, D, generator=g, dtype=torch.float64) - 1).to(dtype)
    return X, Y, Xs


def _build(cls, kind, dtype, X, Y):
    """a model of class `cls` on (X, Y), host side, before any state is loaded"""
    import projectedlmc as plmc
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if cls == "exact":
            m = plmc.ExactGPModel(X, Y, plmc.GaussianLikelihood(batch_shape=torch.Size([2])), n_tasks=2, **_kernel_args(kind))
        else:
            m = plmc.ProjectedGPModel(X, Y, Y.shape[1], 3, mean_type=plmc.ZeroMean, init_lmc_coeffs=True, **_kernel_args(kind))
    return m.to(dtype)


_DATA_BUFFERS = ("train_y", "Y_squared_norm")
_bases = {}


def _base(cls, kind, dtype):
    """(eval-mode model on the first N points with its cache built at NS test points, X, Y, Xs on the device), once per combination"""
    key = (cls, kind, dtype)
    if key not in _bases:
        X, Y, Xs = _data(dtype, 2 if cls == "exact" else 5)
        m = perturb_(_build(cls, kind, dtype, X[:N], Y[:N]), scale=0.1).to(DEV).eval()
        with torch.no_grad():
            m(Xs.to(DEV))
        assert m._prediction_cache().ws is not None
        _bases[key] = (m, X.to(DEV), Y.to(DEV), Xs.to(DEV))
    return _bases[key]


def _refit(cls, kind, dtype, base, X, Y):
    """the same class constructed on (X, Y) with the state_dict of `base` (the buffers that hold training data are the new model's)"""
    m = _build(cls, kind, dtype, X.cpu(), Y.cpu()).to(DEV).eval()
    state = {k: v for k, v in base.state_dict().items() if k not in _DATA_BUFFERS}
    missing, unexpected = m.load_state_dict(state, strict=False)
    assert not unexpected and set(missing) <= set(_DATA_BUFFERS), (missing, unexpected)
    return m


def _moments(model, Xs):
    with torch.no_grad():
        out = model(Xs)
        return out.mean.clone(), out.variance.clone()


def _close(got, want, tol, what):
    err = float((got.double() - want.double()).abs().max())
    bound = tol * max(1.0, float(want.double().abs().max()))
    print("%s: %.3e (bound %.3e)" % (what, err, bound))
    assert err < bound, (what, err, bound)


def _dense_posterior(model, cls, X, Y, Xs):
    """fp64 posterior on the host from the dense kernel matrices of the model's own kernel (assembly kernel), its noise and mean"""
    with torch.no_grad():
        Z = torch.cat([X, Xs])
        K = model.covar_module(Z).evaluate().double().cpu()                      # (q, n + ns, n + ns)
        n = X.shape[0]
        if cls == "exact":
            noise = model.likelihood.noise.reshape(-1).double().cpu()
            mu = model.mean_module(Z).reshape(2, -1).double().cpu()
            y = Y.T.double().cpu() - mu[:, :n]
        else:
            noise = model.projected_noise().double().cpu()
            mu = torch.zeros(3, Z.shape[0], dtype=torch.float64)
            y = model.project_data(model.train_y).double().cpu()
        Khat = K[:, :n, :n] + noise[:, None, None] * torch.eye(n, dtype=torch.float64)
        L = torch.linalg.cholesky(Khat)
        V = torch.linalg.solve_triangular(L, K[:, :n, n:], upper=False)
        z = torch.linalg.solve_triangular(L, y.unsqueeze(-1), upper=False)
        mean = (V.transpose(1, 2) @ z).squeeze(-1) + mu[:, n:]
        var = torch.diagonal(K[:, n:, n:], dim1=1, dim2=2) - (V * V).sum(1)
        if cls == "exact":
            return mean, var                                                   # (a batch of tasks: (n_tasks, ns))
        Ht = model.lmc_coefficients().double().cpu()
        return mean.T @ Ht, var.T @ (Ht * Ht) + model.eps


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("m", [1, 7, 130])
@pytest.mark.parametrize("kind", ["matern52", "poly2", "sum"])
@pytest.mark.parametrize("cls", ["exact", "projected"])
def test_fantasy_model_equals_the_refit_and_hits_its_cache(cls, kind, m, dtype):
    base, X, Y, Xs = _base(cls, kind, dtype)
    before = _moments(base, Xs)
    base_ws, base_key = base._prediction_cache().ws, base._prediction_cache().key
    fant = base.get_fantasy_model(X[N:N + m], Y[N:N + m])
    assert not fant.training and fant is not base and fant.train_inputs[0].shape[0] == N + m
    c = fant._prediction_cache()
    assert c.ws is not None and c.ws is not base_ws and c.ws.n == N + m and c.ws.with_inverse and not c.ws.keep_planes
    got = _moments(fant, Xs)
    assert (c.hits, c.misses) == (1, 0), (c.hits, c.misses)
    # the base model: same cache, the same bits
    after = _moments(base, Xs)
    assert base._prediction_cache().ws is base_ws and base._prediction_cache().key == base_key and base.train_inputs[0].shape[0] == N
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    refit = _refit(cls, kind, dtype, base, X[:N + m], Y[:N + m])
    want = _moments(refit, Xs)
    assert refit._prediction_cache().misses == 1
    tag = "%s %s m=%d %s" % (cls, kind, m, dtype)
    _close(got[0], want[0], TOL[dtype], tag + " mean vs refit")
    _close(got[1], want[1], TOL[dtype], tag + " variance vs refit")
    if dtype == torch.float64:
        dm, dv = _dense_posterior(fant, cls, X[:N + m], Y[:N + m], Xs)
        _close(got[0].cpu(), dm, TOL[dtype], tag + " mean vs dense fp64")
        _close(got[1].cpu(), dv, TOL[dtype], tag + " variance vs dense fp64")


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("cls", ["exact", "projected"])
def test_fantasy_of_a_fantasy_equals_the_one_shot_fantasy(cls, dtype):
    base, X, Y, Xs = _base(cls, "matern52", dtype)
    one = base.get_fantasy_model(X[N:N + 7], Y[N:N + 7])
    two = base.get_fantasy_model(X[N:N + 3], Y[N:N + 3]).get_fantasy_model(X[N + 3:N + 7], Y[N + 3:N + 7])
    a, b = _moments(one, Xs), _moments(two, Xs)
    c = two._prediction_cache()
    assert (c.hits, c.misses) == (1, 0) and c.ws.n == N + 7
    _close(b[0], a[0], TOL[dtype], "fantasy of fantasy, mean")
    _close(b[1], a[1], TOL[dtype], "fantasy of fantasy, variance")


@pytest.mark.parametrize("cls", ["exact", "projected"])
def test_the_other_eval_mode_paths_work_on_the_fantasy_model(cls):
    """predictive_gradients, a prediction under skip_posterior_variances and sample_paths (shared generator seed) against the refit
    model, fp64; zero-mean Matern models (predictive_gradients asks for a plain mean)."""
    from projectedlmc import settings
    import projectedlmc as plmc
    dtype = torch.float64
    X, Y, Xs = (t.to(DEV) for t in _data(dtype, 2 if cls == "exact" else 5))
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        def build(Xh, Yh):
            if cls == "exact":
                return plmc.ExactGPModel(Xh, Yh, plmc.GaussianLikelihood(batch_shape=torch.Size([2])), n_tasks=2, kernel_type=plmc.MaternKernel,
                                         mean_type=plmc.ZeroMean).to(dtype)
            return plmc.ProjectedGPModel(Xh, Yh, 5, 3, mean_type=plmc.ZeroMean, kernel_type=plmc.MaternKernel, init_lmc_coeffs=True).to(dtype)
        base = perturb_(build(X[:N].cpu(), Y[:N].cpu()), scale=0.1).to(DEV).eval()
        refit = build(X[:N + 7].cpu(), Y[:N + 7].cpu()).to(DEV).eval()
    refit.load_state_dict({k: v for k, v in base.state_dict().items() if k not in _DATA_BUFFERS}, strict=False)
    with torch.no_grad():
        base(Xs)
    fant = base.get_fantasy_model(X[N:N + 7], Y[N:N + 7])
    assert fant._prediction_cache().ws is not None
    tol = TOL[dtype]
    for a, b, name in zip(fant.predictive_gradients(Xs), refit.predictive_gradients(Xs), ("d mean / dx", "d variance / dx")):
        _close(a, b, tol, "predictive_gradients " + name)
    assert fant._prediction_cache().misses == 0
    with settings.skip_posterior_variances(True), torch.no_grad():
        _close(fant(Xs).mean, refit(Xs).mean, tol, "mean-only prediction")
    pa = fant.sample_paths(3, num_features=64, generator=torch.Generator().manual_seed(9))
    pb = refit.sample_paths(3, num_features=64, generator=torch.Generator().manual_seed(9))
    with torch.no_grad():
        _close(pa(Xs), pb(Xs), tol, "sample_paths at the test points")


def test_a_base_factor_that_needed_jitter(recwarn):
    """The input of tests/test_gpu_jitter_ladder.py (fp32, RBF, lengthscales 5, noise e^-40): the cached base factor is of noise + jitter.
    The extension puts the same jitter on the new diagonal and agrees with a refit at that jitter, or is dropped (a pivot of the border is
    not positive) and the first prediction on the concatenated data factorises: misses == 1.  The tolerance of the agreement is the forward
    error of a solve with this matrix, kappa_2 u with kappa_2 from fp64 eigenvalues of Khat at that jitter (relative to the largest value)."""
    from projectedlmc import _engine as eng, settings
    from oracle import gp_math as gm
    n, d, q, m = 300, 2, 2, 5
    g = torch.Generator().manual_seed(3)
    X = (2 * torch.rand(n + m, d, generator=g, dtype=torch.float64) - 1).float()
    y = torch.randn(q, n + m, generator=g, dtype=torch.float64).float()
    Xs = (2 * torch.rand(40, d, generator=g, dtype=torch.float64) - 1).float()
    ell, noise = torch.full((q, d), 5.0), torch.full((q,), math.exp(-40.0))
    f = lambda t: t.to(DEV)
    cache, cache2 = eng.PosteriorCache(), eng.PosteriorCache()
    with settings.cholesky_max_tries(8):
        eng.exact_posterior("rbf", f(X[:n]), f(ell), None, f(noise), f(y[:, :n]), f(Xs), cache=cache, key=("base",))
        jit = cache.ws.jitter
        assert jit > 0.0 and cache.misses == 1
        ws = eng.extend_cached_factor("rbf", f(X[:n]), f(ell), None, f(noise), f(y[:, :n]), f(X[n:]), cache, ("base",))
        if ws is not None:
            assert ws.jitter == jit and ws.n == n + m
            cache2.key, cache2.ws = ("fantasy",), ws
        got = eng.exact_posterior("rbf", f(X), f(ell), None, f(noise), f(y), f(Xs), cache=cache2, key=("fantasy",))
        if ws is None:
            assert (cache2.hits, cache2.misses) == (0, 1) and all(bool(torch.isfinite(t).all()) for t in got)
            return
        assert (cache2.hits, cache2.misses) == (1, 0)
        want = eng.exact_posterior("rbf", f(X), f(ell), None, f(noise) + jit, f(y), f(Xs))
    K = gm.kernel_matrix("rbf", X.double(), X.double(), ell.double()) + (math.exp(-40.0) + jit) * torch.eye(n + m, dtype=torch.float64)
    ev = torch.linalg.eigvalsh(K)
    tol = float((ev[:, -1] / ev[:, 0]).max()) * 2.0 ** -24
    _close(got[0], want[0], tol, "jittered base: mean vs refit at the same jitter")
    _close(got[1], want[1], tol, "jittered base: variance vs refit at the same jitter")


def test_what_is_not_served_is_refused_by_name():
    import projectedlmc as plmc
    from projectedlmc import settings
    base, X, Y, Xs = _base("exact", "matern52", torch.float64)
    xn, yn = X[N:N + 2], Y[N:N + 2]
    base.train()
    try:
        with pytest.raises(RuntimeError, match="eval-mode"):
            base.get_fantasy_model(xn, yn)
    finally:
        base.eval()
        del _bases[("exact", "matern52", torch.float64)]          # (train() dropped its cache)
    with settings.prediction_cache("off"), pytest.raises(NotImplementedError, match="prediction_cache"):
        base.get_fantasy_model(xn, yn)
    Xh, Yh = X[:64].cpu(), Y[:64].cpu()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sgpr = plmc.ExactGPModel(Xh, Yh[:, 0], plmc.GaussianLikelihood(), kernel_type=plmc.MaternKernel, n_inducing_points=16).double().to(DEV).eval()
        dense = plmc.MultitaskGPModel(Xh, Yh, plmc.MultitaskGaussianLikelihood(num_tasks=2), n_tasks=2, n_latents=2).double().to(DEV).eval()
        var = plmc.VariationalMultitaskGPModel(Xh, n_latents=2, n_tasks=2, train_y=Yh).double().to(DEV).eval()
        Xp, Yp, _ = _data(torch.float64, 5)
        shard = plmc.ProjectedGPModel(Xp[:64], Yp[:64], 5, 3, mean_type=plmc.ZeroMean, init_lmc_coeffs=True, latent_shard=(0, 2)).double().to(DEV).eval()
    for model, name, args in ((sgpr, "inducing-point", (xn, yn[:, 0])), (dense, "MultitaskGPModel", (xn, yn)), (var, "VariationalMultitaskGPModel", (xn, yn)),
                              (shard, "latent-sharded", (Xp[64:66].to(DEV), Yp[64:66].to(DEV)))):
        with pytest.raises(NotImplementedError, match=name):
            model.get_fantasy_model(*args)
