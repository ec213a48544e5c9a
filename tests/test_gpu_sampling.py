"""Draws through the public surface: MultivariateNormal / MultitaskMultivariateNormal .get_base_samples, .rsample, .sample on the engine
(_engine.sample_lazy, _dense.spd_sample, plmc_trmm_ut).

Identity base samples turn a draw into the factor itself: with z_j = e_j the draws minus the mean are S[j][i] = U[j][i], so S must be
exactly upper triangular and S^T S must reproduce the covariance by the project's own measure of a factorisation,
    rho_U = |S^T S - Khat|_F / (n_pad u |Khat|_F)            (tests/_factor_ref.py),
inside fr.plain_thresholds for fp64 and fr.split_apriori_rho_u for fp32.  Khat is read back from the engine in the same dtype
(evaluate()) plus the jitter the call reports (`sample_jitter`), so assembly error does not enter.
The noise-free case is the reference's own call (experiments.py:150-151): Matern-5/2 on linspace(-1, 1, 200) with lengthscale 0.1.  Its
fp64 Cholesky on the CPU succeeds at the first jitter rung (1e-8; smallest eigenvalue 6.3e-6, asserted below), so the lengthscale stands
as stated.

The statistical tests have Gaussian sampling margins, not tuned ones: every entry of the sample covariance of s draws within
6 sqrt((K_ii K_jj + K_ij^2) / (s - 1)) of K_ij and every sample mean within 6 sqrt(K_ii / s) of loc, at a fixed seed.
"""
import math
import warnings

import pytest
import torch

import _factor_ref as fr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32, F64 = torch.float32, torch.float64


@pytest.fixture(autouse=True)
def _nothing_more_after_a_gpu_error():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("HIP error, nothing more is started: %s" % e, returncode=3)


class _Factored:
    """What fr.plain_thresholds / fr.split_apriori_rho_u ask of a case, for covariances Khat (q, n, n) that were read back from the engine"""

    def __init__(self, K, dtype):
        self.K, self.dtype = K.double().cpu(), dtype
        self.q, self.n = self.K.shape[0], self.K.shape[-1]
        self.n_pad = fr.pad(self.n)
        ev = torch.linalg.eigvalsh(self.K)
        self.kappa = ev[:, -1] / ev[:, 0].clamp_min(1e-300)
        self._ref = None

    def K_pad(self, dtype=F64):
        Kp = torch.eye(self.n_pad, dtype=F64).repeat(self.q, 1, 1)
        Kp[:, :self.n, :self.n] = self.K
        return Kp.to(dtype)

    def ref(self):
        if self._ref is None:
            self._ref = dict(U=torch.linalg.cholesky(self.K_pad()).transpose(1, 2).contiguous())
        return self._ref

    def rho_u(self, S):
        S = S.double().cpu()
        return fr._fro(S.transpose(1, 2) @ S - self.K) / (self.n_pad * fr.UNIT[self.dtype] * fr._fro(self.K))

    def lapack_rho_u(self):
        """the same measure of the CPU LAPACK factorisation in the element type"""
        L = torch.linalg.cholesky(self.K.to(self.dtype))
        return self.rho_u(L.transpose(1, 2))

    def threshold(self):
        if self.dtype == F64:
            return fr.plain_thresholds(self, {"rho_U": self.lapack_rho_u()}, ["rho_U"])["rho_U"]
        groups = -(-(self.n_pad // fr.NB) // 8)
        return fr.split_apriori_rho_u(self, groups)


def _check_identity_draws(dist, Khat, dtype, label):
    """dist: batch of q MVNs on n points.  Draw with base samples = I and hold S to the rho_U rule against Khat + reported jitter."""
    q, n = dist.loc.shape
    Z = torch.eye(n, dtype=dtype, device=DEV)[:, None, :].expand(n, q, n).contiguous()
    draws = dist.sample(base_samples=Z)
    assert draws.shape == (n, q, n)
    S = (draws - dist.loc.detach()).permute(1, 0, 2)                   # S[b][j][i] = U_b[j][i]
    jit = dist.sample_jitter
    case = _Factored(Khat.double().cpu() + jit * torch.eye(n, dtype=F64), dtype)
    if bool(dist.loc.detach().eq(0).all()):
        assert bool((torch.tril(S, -1) == 0).all()), "%s: S is not exactly upper triangular" % label
    else:                                                               # (a shift was added and taken off again: one rounding of |loc|)
        low = torch.tril(S, -1).abs().cpu().double()
        assert bool((low <= 2 * fr.UNIT[dtype] * dist.loc.detach().abs().cpu().double()[:, None, :]).all()), label
        S = torch.triu(S)
    assert bool(torch.isfinite(S).all()), label
    rho, thr = case.rho_u(S), case.threshold()
    print("%s: jitter %.1e, rho_U %s, threshold %s, LAPACK %s" % (label, jit, rho.tolist(), thr.tolist(), case.lapack_rho_u().tolist()))
    assert bool((rho <= thr).all()), (label, rho.tolist(), thr.tolist())
    return jit


def _lazy_prior(dtype, zero_mean):
    """q = 2 Matern-5/2 priors with noise on 200 points in 3 dimensions: the `kernel` family of tests/_factor_ref.py (kappa <= 100)"""
    import projectedlmc as plmc
    from projectedlmc.kernels import LazyKernel
    c = fr.Case("kernel", 200, 2, dtype)
    P = {k: (v.to(dtype).to(DEV) if torch.is_tensor(v) else v) for k, v in c.params.items()}
    lazy = LazyKernel("matern52", P["X"], P["X"], P["ell"], P["oscale"], (2,), noise=P["noise"])
    g = torch.Generator().manual_seed(1)
    loc = torch.zeros(2, 200, dtype=dtype) if zero_mean else torch.randn(2, 200, generator=g, dtype=F64).to(dtype)
    return plmc.MultivariateNormal(loc.to(DEV), lazy)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("zero_mean", [True, False], ids=["zero_mean", "shifted"])
def test_identity_base_samples_reproduce_the_prior_covariance(dtype, zero_mean):
    dist = _lazy_prior(dtype, zero_mean)
    jit = _check_identity_draws(dist, dist.lazy_covariance_matrix.evaluate(), dtype, "kernel prior %s" % dtype)
    assert jit == 0.0


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_identity_base_samples_through_the_likelihood_matern32(dtype):
    import projectedlmc as plmc
    q, n = 2, 200
    g = torch.Generator().manual_seed(2)
    X = (2 * torch.rand(n, 2, generator=g, dtype=F64) - 1).to(dtype).to(DEV)
    k = plmc.MaternKernel(nu=1.5, batch_shape=torch.Size([q])).to(dtype).to(DEV)
    k.lengthscale = torch.tensor([0.3, 0.6]).reshape(q, 1, 1)
    lik = plmc.GaussianLikelihood(batch_shape=torch.Size([q])).to(dtype).to(DEV)
    lik.noise = torch.tensor(0.1)
    dist = lik(plmc.MultivariateNormal(torch.zeros(q, n, dtype=dtype, device=DEV), k(X)))
    assert abs(float(dist.lazy_covariance_matrix.noise.reshape(-1)[0]) - 0.1) < 1e-6
    jit = _check_identity_draws(dist, dist.lazy_covariance_matrix.evaluate(), dtype, "matern32 + likelihood %s" % dtype)
    assert jit == 0.0


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_identity_base_samples_noise_free_prior_the_reference_call(dtype):
    import projectedlmc as plmc
    from projectedlmc import settings
    from oracle import gp_math as gm
    q, n, ell = 2, 200, 0.1
    X64 = torch.linspace(-1, 1, n, dtype=F64)[:, None]
    # on the CPU first: the fp64 Cholesky of the noise-free matrix succeeds at the first jitter rung
    K64 = gm.kernel_matrix("matern", X64, X64, torch.full((1, 1), ell, dtype=F64), None, 2.5)[0]
    first = settings.cholesky_jitter.value(F64)
    assert int(torch.linalg.cholesky_ex(K64 + first * torch.eye(n, dtype=F64))[1]) == 0
    assert float(torch.linalg.eigvalsh(K64)[0]) > 1e-6
    X = X64.to(dtype).to(DEV)
    k = plmc.MaternKernel(batch_shape=torch.Size([q])).to(dtype).to(DEV)
    k.lengthscale = torch.tensor(ell)
    dist = plmc.MultivariateNormal(torch.zeros(q, n, dtype=dtype, device=DEV), k(X))
    assert dist.lazy_covariance_matrix.noise is None
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        jit = _check_identity_draws(dist, dist.lazy_covariance_matrix.evaluate(), dtype, "noise-free matern52 %s" % dtype)
    base = settings.cholesky_jitter.value(dtype)
    assert jit >= base                                     # the jitter stands on the diagonal from the first attempt
    if dtype == F64:
        assert jit == base and not [x for x in w if "not p.d." in str(x.message)]


# ------------------------------------------------------------------------------------------------ statistics
def _moment_check(draws, loc, K, label):
    """draws (s, n), loc (n), K (n, n), fp64 on the host"""
    s = draws.shape[0]
    m = draws.mean(0)
    C = torch.cov(draws.T)
    d = torch.diagonal(K)
    tol_m = 6 * torch.sqrt(d / s)
    tol_c = 6 * torch.sqrt((d[:, None] * d[None, :] + K * K) / (s - 1))
    worst_m, worst_c = float(((m - loc).abs() / tol_m).max()), float(((C - K).abs() / tol_c).max())
    print("%s: worst mean %.2f / 6 sigma, worst covariance %.2f / 6 sigma" % (label, worst_m * 6, worst_c * 6))
    assert worst_m <= 1.0 and worst_c <= 1.0, (label, worst_m, worst_c)


def _stat_kernel(name, q, dtype):
    import projectedlmc as plmc
    if name == "rbf":
        k = plmc.RBFKernel(ard_num_dims=2, batch_shape=torch.Size([q]))
        k.lengthscale = torch.tensor([[0.4, 0.7], [0.9, 0.5]]).reshape(q, 1, 2)
    elif name == "periodic":
        k = plmc.PeriodicKernel(ard_num_dims=2, batch_shape=torch.Size([q]))
        k.lengthscale = torch.tensor([[1.0, 1.5], [0.8, 2.0]]).reshape(q, 1, 2)
        k.period_length = torch.tensor([[0.9, 1.3], [1.1, 0.7]]).reshape(q, 1, 2)
    else:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            k = plmc.handle_covar_(plmc.RBFKernel, dim=2, decomp=[[0], [1]], n_funcs=q)
    return k.to(dtype).to(DEV)


@pytest.mark.parametrize("name,s", [("rbf", 4096), ("periodic", 1024), ("decomp", 1024)])
def test_sample_moments_match_the_prior(name, s):
    import projectedlmc as plmc
    dtype, n, q = F32, 48, 2
    g = torch.Generator().manual_seed(4)
    X = (2 * torch.rand(n, 2, generator=g, dtype=F64) - 1).to(dtype).to(DEV)
    loc = torch.randn(q, n, generator=g, dtype=F64).to(dtype).to(DEV)
    lazy = _stat_kernel(name, q, dtype)(X).add_noise(torch.full((q,), 0.05, dtype=dtype, device=DEV))
    dist = plmc.MultivariateNormal(loc, lazy)
    torch.manual_seed(1234)
    draws = dist.sample(torch.Size([s]))
    assert draws.shape == (s, q, n) and dist.sample_jitter == 0.0
    K = lazy.evaluate().double().cpu()
    for b in range(q):
        _moment_check(draws[:, b].double().cpu(), loc[b].double().cpu(), K[b], "%s latent %d" % (name, b))


def test_seeds_and_sample_shape():
    dist = _lazy_prior(F32, True)
    torch.manual_seed(7)
    a = dist.sample(torch.Size([3, 2]))
    torch.manual_seed(7)
    b = dist.sample(torch.Size([3, 2]))
    torch.manual_seed(8)
    c = dist.sample(torch.Size([3, 2]))
    assert a.shape == (3, 2, 2, 200)
    assert torch.equal(a, b) and not torch.equal(a, c)
    one = dist.sample()
    assert one.shape == (2, 200)
    z = dist.get_base_samples(torch.Size([5]))
    assert torch.equal(dist.rsample(base_samples=z), dist.rsample(torch.Size([5]), base_samples=z))


# ------------------------------------------------------------------------------------------------ posteriors
def _exact_model(dtype, n=150, d=2, seed=0):
    import projectedlmc as plmc
    g = torch.Generator().manual_seed(seed)
    X = 2 * torch.rand(n, d, generator=g, dtype=F64) - 1
    y = torch.sin(3 * X[:, 0]) + 0.1 * torch.randn(n, generator=g, dtype=F64)
    lik = plmc.GaussianLikelihood()
    model = plmc.ExactGPModel(X.to(dtype), y.to(dtype), lik, mean_type=plmc.ConstantMean, kernel_type=plmc.MaternKernel, outputscales=True)
    Xs = 2 * torch.rand(40, d, generator=g, dtype=F64) - 1
    return model.to(dtype).to(DEV).eval(), Xs.to(dtype).to(DEV)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_exact_gp_posterior_draws_and_prediction_cache(dtype):
    import projectedlmc as plmc
    from projectedlmc import settings
    model, Xs = _exact_model(dtype)
    ns = Xs.shape[0]
    with settings.prediction_cache("eager"), torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        dist = model(Xs, full_cov=True)
        c = model._prediction_cache()
        assert (c.hits, c.misses) == (0, 1)
        assert isinstance(dist, plmc.MultivariateNormal) and dist.covariance_matrix.shape == (ns, ns)
        Z = torch.eye(ns, dtype=dtype, device=DEV)

        def check(d, label):
            draws = d.sample(base_samples=Z)
            assert draws.shape == (ns, ns)
            S = (draws - d.mean)[None]
            case = _Factored(d.covariance_matrix.double().cpu()[None] + d.sample_jitter * torch.eye(ns, dtype=F64), dtype)
            low = torch.tril(S, -1).abs().cpu().double()               # (the mean was added and taken off again: one rounding of it)
            assert bool((low <= 2 * fr.UNIT[dtype] * d.mean.abs().cpu().double()[None, None, :]).all())
            rho, thr = case.rho_u(torch.triu(S)), case.threshold()
            print("posterior %s, %s: jitter %.1e rho_U %s threshold %s" % (dtype, label, d.sample_jitter, rho.tolist(), thr.tolist()))
            assert bool((rho <= thr).all()), (label, rho.tolist(), thr.tolist())

        check(dist, "first call")
        # a second call hits the cache; drawing in between has left its counters and its factor alone, as an ordinary prediction would
        dist2 = model(Xs, full_cov=True)
        assert (c.hits, c.misses) == (1, 1)
        check(dist2, "cached call")
        assert (c.hits, c.misses) == (1, 1)
        tol = 1e-8 if dtype == F64 else 2e-4
        assert float((dist2.mean - dist.mean).abs().max()) <= tol * max(1.0, float(dist.mean.abs().max()))
        # through the likelihood: the noisy predictive draws from a dense tensor as well
        noisy = model.likelihood(dist)
        assert noisy.sample(torch.Size([3])).shape == (3, ns)


def _projected_model(dtype, n=120, d=2, p=3, q=2, seed=0):
    import projectedlmc as plmc
    g = torch.Generator().manual_seed(seed)
    X = 2 * torch.rand(n, d, generator=g, dtype=F64) - 1
    Y = torch.randn(n, p, generator=g, dtype=F64)
    torch.manual_seed(seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = plmc.ProjectedGPModel(X.to(dtype), Y.to(dtype), p, q, mean_type=plmc.ZeroMean, kernel_type=plmc.MaternKernel, init_lmc_coeffs=True,
                                  BDN=False)
    Xs = 2 * torch.rand(8, d, generator=g, dtype=F64) - 1
    return m.to(dtype).to(DEV).eval(), Xs.to(dtype).to(DEV)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_projected_model_draws_are_the_mixed_latent_draws(dtype):
    """rsample(base_samples=Z), Z (n*, q + p): mean + sum_i (latent draw_i - latent mean_i) h_i + sqrt(eps) Z[:, q:], where the latent
    draws come from compute_latent_distrib(x).rsample(Z[:, :q]^T).  Tolerance (q + 2) u sum |terms|, the terms being the mean, each
    latent draw times h_i, each latent mean times h_i (taken off again) and the eps term."""
    from projectedlmc.distributions import KroneckerSumCovariance
    model, Xs = _projected_model(dtype)
    q, p, ns = 2, 3, Xs.shape[0]
    u = fr.UNIT[dtype]
    g = torch.Generator().manual_seed(3)
    Z = torch.randn(ns, q + p, generator=g, dtype=F64).to(dtype).to(DEV)
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        Ht = model.lmc_coefficients().detach()
        eps = float(model.eps)
        full = model(Xs, full_cov=True)
        assert isinstance(full.lazy_covariance_matrix, KroneckerSumCovariance)
        assert full.get_base_samples().shape == (ns, q + p)
        got = full.rsample(base_samples=Z)
        assert got.shape == (ns, p)
        latent = model.compute_latent_distrib(Xs)
        lat = latent.rsample(base_samples=Z[:, :q].T.contiguous())                # (q, n*)
        f = lambda t: t.double().cpu()
        want = f(full.mean) + torch.einsum("qn,qp->np", f(lat) - f(latent.mean), f(Ht)) + math.sqrt(eps) * f(Z[:, q:])
        mag = (f(full.mean).abs() + torch.einsum("qn,qp->np", f(lat).abs() + f(latent.mean).abs(), f(Ht).abs()) + math.sqrt(eps) * f(Z[:, q:]).abs())
        assert bool(((f(got) - want).abs() <= (q + 2) * u * mag).all()), ((f(got) - want).abs().max(), ((q + 2) * u * mag).min())
        # full_cov=False: only variances were formed, the draw uses sqrt(var) -- independent points
        marg = model(Xs)
        c = marg.lazy_covariance_matrix
        assert c.cov is None and c.var is not None
        got = marg.rsample(base_samples=Z)
        dev = f(c.var).sqrt() * f(Z[:, :q]).T
        want = f(marg.mean) + torch.einsum("qn,qp->np", dev, f(Ht)) + math.sqrt(eps) * f(Z[:, q:])
        mag = f(marg.mean).abs() + torch.einsum("qn,qp->np", dev.abs(), f(Ht).abs()) + math.sqrt(eps) * f(Z[:, q:]).abs()
        assert bool(((f(got) - want).abs() <= (q + 2) * u * mag).all())
        assert marg.sample(torch.Size([3, 2])).shape == (3, 2, ns, p)


def test_projected_model_sample_moments_match_the_task_covariance():
    model, Xs = _projected_model(F32)
    ns, p, s = Xs.shape[0], 3, 8192
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        dist = model(Xs, full_cov=True)
        torch.manual_seed(99)
        draws = dist.sample(torch.Size([s]))
        assert draws.shape == (s, ns, p)
        K = dist.lazy_covariance_matrix.evaluate().double().cpu()
    _moment_check(draws.reshape(s, ns * p).double().cpu(), dist.mean.reshape(-1).double().cpu(), K, "projected posterior")


def test_rsample_gradient_reaches_loc_only():
    import projectedlmc as plmc
    q, n, dtype = 2, 60, F64
    g = torch.Generator().manual_seed(5)
    X = (2 * torch.rand(n, 2, generator=g, dtype=F64) - 1).to(DEV)
    k = plmc.RBFKernel(batch_shape=torch.Size([q])).to(dtype).to(DEV)
    lik = plmc.GaussianLikelihood(batch_shape=torch.Size([q])).to(dtype).to(DEV)
    loc = torch.zeros(q, n, dtype=dtype, device=DEV, requires_grad=True)
    dist = lik(plmc.MultivariateNormal(loc, k(X)))
    w = torch.randn(3, q, n, generator=g, dtype=F64).to(DEV)
    out = dist.rsample(torch.Size([3]))
    assert out.requires_grad
    (out * w).sum().backward()
    assert torch.allclose(loc.grad, w.sum(0), rtol=1e-13, atol=1e-13)
    assert all(prm.grad is None for prm in list(k.parameters()) + list(lik.parameters()))
    assert not dist.sample(torch.Size([3])).requires_grad
