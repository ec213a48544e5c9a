"""Spectral-mixture kernel on the batched exact engine: the new entry points per element, the log-prob and every entry of the gradient
table of `ExactLatentLogProb`, the fp32 phase reduction at large phase, a cosine factor that is exactly zero, `ExactGPModel` (single
and batched) and `ProjectedGPModel` (dense loss, gradients, eval mode, LOO, prediction cache, latent sharding), the jitter ladder and the argument errors.

Reference values: the dense fp64 formula of tests/_sm_dense.py (torch CPU, autograd).  Tolerances: those of
tests/test_gpu_additive_engine.py for the additive table (named beside each use); the fp32 per-element bound is derived, not measured:
    |err| <= 32 d 2^-24 sum_m w_m   against the fp64 formula at the fp32-rounded inputs and parameters
(a few ulp per cosine factor and per exponential), at small and at large phase alike."""
import math
import warnings

import pytest
import torch

import _sm_dense as smd
from oracle import gp_math as gm
from oracle import projected as pj
from _bridge import perturb_

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U32 = 2.0 ** -24


@pytest.fixture(scope="module")
def eng():
    import types
    from projectedlmc import _hip, _engine, settings
    assert torch.cuda.is_available()
    return types.SimpleNamespace(hip=_hip, exact=_engine, settings=settings)


@pytest.fixture(scope="module")
def plmc():
    import projectedlmc
    assert torch.cuda.is_available()
    return projectedlmc


def _problem(n, d, q, M, seed, ns=1, mu_max=6.0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    X, Xs = r(n, d), r(ns, d)
    y = torch.randn(q, n, generator=g, dtype=torch.float64)
    scales = (0.3 + 0.7 * r(q, M, d)) / math.sqrt(d)
    means = mu_max * r(q, M, d)
    weights = 0.5 + r(q, M)
    noise = 0.05 + 0.5 * r(q)
    return X, Xs, y, scales, means, weights, noise


def _assemble(eng, X, scales, means, weights, noise, dt):
    """plmc_assemble_sm_*: the upper triangle of Khat, (q, n, n) fp64 on the host."""
    hip = eng.hip
    L = hip.lib()
    f = lambda t: t.to(DEV, dt).contiguous()
    n, d = X.shape
    q, M = weights.shape
    ws = eng.exact.Workspace(n, q, 0, dt, DEV, with_inverse=False)
    ws.A.zero_()
    Xd, s_, m_, w_, nz = (f(t) for t in (X, scales, means, weights, noise))
    L.call("plmc_assemble_sm", dt, hip.ptr(Xd), n, d, M, hip.ptr(s_), hip.ptr(m_), hip.ptr(w_), hip.ptr(nz), hip.ptr(ws.A), ws.lda,
           ws.strideA, q, hip.stream_ptr(DEV))
    torch.cuda.synchronize()
    return torch.triu(ws.A[:, :n, :n].cpu().double())


def _cross(eng, X, Xs, scales, means, weights, dt):
    f = lambda t: t.to(DEV, dt).contiguous()
    K = eng.exact.dense_cross("sm", f(X), f(Xs), torch.stack([f(scales), f(means)], 1), f(weights))
    torch.cuda.synchronize()
    return K.cpu().double()


# ------------------------------------------------------------------------------------------------ per element
@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("M", [1, 5, 8])
@pytest.mark.parametrize("d", [1, 3])
def test_assembly_and_cross_against_the_dense_formula(eng, d, M, dt):
    """plmc_assemble_sm / plmc_assemble_cross_sm at moderate phases (up to 6 revolutions), n = 300 (ragged last block), q = 2.
    fp64: |err| <= 1e-12 (|ref| + sum_m w_m) -- rtol 1e-12 with the kernel's scale as an absolute floor, a DEVIATION from a pure rtol:
    the dense reference evaluates cos(2 pi mu tau) at up to 6 revolutions with an absolute error of ~4e-15 sum w itself, so an element
    near a zero crossing of the carrier (or of the sum over components) has no 1e-12 relative accuracy in the reference either.
    fp32: the bound of the module docstring, diagonal (sum w + noise) included."""
    assert M <= eng.hip.lib().cdll.plmc_sm_max_mixtures()
    n, q, ns = 300, 2, 70
    X, Xs, _, sc, mu, w, nz = _problem(n, d, q, M, seed=10 * d + M, ns=ns)
    if dt == torch.float32:
        X, Xs, sc, mu, w, nz = (t.float().double() for t in (X, Xs, sc, mu, w, nz))
    ref = torch.triu(smd.sm_kernel(X, X, sc, mu, w) + nz[:, None, None] * torch.eye(n, dtype=torch.float64))
    refx = smd.sm_kernel(X, Xs, sc, mu, w)
    got, gotx = _assemble(eng, X, sc, mu, w, nz, dt), _cross(eng, X, Xs, sc, mu, w, dt)
    scale = w.sum(-1)[:, None, None]
    for name, a, b in (("assemble", got, ref), ("cross", gotx, refx)):
        err = (a - b).abs()
        if dt == torch.float64:
            print("%s f64: max err / (|ref| + sum w) %.3g" % (name, float((err / (b.abs() + scale)).max())))
            assert bool((err <= 1e-12 * (b.abs() + scale)).all()), name
        else:
            bound = 32 * d * U32 * scale
            print("%s f32: max err / bound %.3g" % (name, float((err / bound).max())))
            assert bool((err <= bound).all()), name


def _large_phase_inputs():
    n, M = 4096, 5
    g = torch.Generator().manual_seed(0)
    X = ((torch.arange(n, dtype=torch.float64) + 0.3 * torch.rand(n, generator=g, dtype=torch.float64)) / n).reshape(n, 1)
    gaps = X[1:, 0] - X[:-1, 0]
    mu = (torch.rand(1, M, 1, generator=g, dtype=torch.float64) * 0.5 / float(gaps.min()))
    mu[0, 0, 0] = 0.5 / float(gaps.min())                  # the initialiser's upper end
    sc = 0.3 + 1.2 * torch.rand(1, M, 1, generator=g, dtype=torch.float64)
    w = 0.5 + torch.rand(1, M, generator=g, dtype=torch.float64)
    return tuple(t.float().double() for t in (X, sc, mu, w))


def test_large_phase_fp32_assembly_meets_the_bound_and_the_naive_form_does_not(eng):
    """n = 4096 near-uniform points in [0, 1), M = 5, means up to 0.5 / (smallest spacing): phases of up to ~2 10^3 revolutions.
    Every element of the fp32 assembly is within the bound; cos(2 pi mu tau) from rounded fp32 products (torch, fp32) is not."""
    X, sc, mu, w = _large_phase_inputs()
    n = X.shape[0]
    nz = torch.tensor([0.1], dtype=torch.float64)
    ref = sum(smd.sm_kernel(X, X, sc[:, m:m + 1], mu[:, m:m + 1], w[:, m:m + 1]) for m in range(mu.shape[1]))
    bound = 32 * 1 * U32 * float(w.sum())
    Xf, scf, muf, wf = (t.float() for t in (X, sc, mu, w))
    tau = Xf[:, None, 0] - Xf[None, :, 0]
    naive = sum(wf[0, m] * torch.exp(-2.0 * math.pi ** 2 * (scf[0, m, 0] * tau) ** 2) * torch.cos(2.0 * math.pi * muf[0, m, 0] * tau)
                for m in range(mu.shape[1]))
    e_naive = float((naive.double() - ref[0]).abs().max())
    got = _assemble(eng, X, sc, mu, w, nz, torch.float32)
    e = float((got[0] - torch.triu(ref[0] + 0.1 * torch.eye(n, dtype=torch.float64))).abs().max())
    print("largest phase %.4g revolutions; bound %.3g; assembly err %.3g; naive fp32 err %.3g"
          % (float(mu.max() * (X.max() - X.min())), bound, e, e_naive))
    assert e_naive > bound, (e_naive, bound)
    assert e <= bound, (e, bound)


# ------------------------------------------------------------------------------------------------ log-prob and the gradient table
def _reference_logprob(X, y, sc, mu, w, nz):
    leaves = [t.clone().requires_grad_() for t in (sc, mu, w, nz, y)]
    lp = smd.sm_logprob(X, leaves[4], leaves[0], leaves[1], leaves[2], leaves[3])
    g = torch.Generator().manual_seed(99)
    wt = 0.5 + torch.rand(lp.shape, generator=g, dtype=torch.float64)
    (lp * wt).sum().backward()
    return [lp.detach()] + [t.grad for t in leaves] + [wt]


def _run_logprob(eng, X, y, sc, mu, w, nz, dt, wt):
    f = lambda t: t.to(DEV, dt)
    table = torch.stack([f(sc), f(mu)], 1).requires_grad_()
    leaves = [f(t).requires_grad_() for t in (w, nz, y)]
    lp = eng.exact.exact_latent_log_prob("sm", f(X), table, leaves[0], leaves[1], leaves[2])
    (lp * f(wt)).sum().backward()
    torch.cuda.synchronize()
    tg = table.grad.cpu().double()
    return [lp.detach().cpu().double(), tg[:, 0], tg[:, 1]] + [t.grad.cpu().double() for t in leaves]


GRAD_NAMES = ("scales", "means", "weights", "noise", "y")


@pytest.mark.parametrize("n,d,M", [(517, 1, 5), (300, 3, 2), (260, 8, 8)])
def test_logprob_and_every_gradient_fp64(eng, n, d, M):
    """q = 3; tolerances of tests/test_gpu_additive_engine.py:172-175 (log-prob rtol 1e-10; gradients rtol 1e-7 / atol 1e-9)."""
    q = 3
    X, _, y, sc, mu, w, nz = _problem(n, d, q, M, seed=n + d, mu_max=3.0)
    ref = _reference_logprob(X, y, sc, mu, w, nz)
    got = _run_logprob(eng, X, y, sc, mu, w, nz, torch.float64, ref[6])
    assert torch.allclose(got[0], ref[0], rtol=1e-10, atol=0), (got[0], ref[0])
    for name, a, b in zip(GRAD_NAMES, got[1:], ref[1:6]):
        assert a.shape == b.shape, name
        assert torch.allclose(a, b, rtol=1e-7, atol=1e-9), (name, float((a - b).abs().max()))


@pytest.mark.parametrize("d,M", [(1, 5), (3, 2)])
def test_logprob_fp32_split_engines_and_fused_assembly(eng, monkeypatch, d, M):
    """n = 1300 (two groups of block rows), q = 3, fp32 under PLMC_SPLIT 2, 3 and 0: value 1e-4 relative, gradients 2e-3 of the
    largest entry (tests/test_gpu_additive_engine.py:172-201).  Fused assembly and PLMC_FUSED_ASSEMBLE=0 are equal as bit patterns.
    d = 1 runs the sweep AND the K^-1 + gradient kernel on each arithmetic.  d = 3: the knob changes the sweep only -- with d > 1 the
    gradient kernel forms K^-1 with the fp32 matrix instructions whatever the knob says (include/plmc.h), so the three passes differ in
    the factorisation they start from, not in the gradient kernel."""
    n, q = 1300, 3
    X, _, y, sc, mu, w, nz = (t.float().double() for t in _problem(n, d, q, M, seed=77 + d, mu_max=3.0))
    ref = _reference_logprob(X, y, sc, mu, w, nz)
    for split in ("2", "3", "0"):
        with eng.hip.knob("PLMC_SPLIT", split):
            got = _run_logprob(eng, X, y, sc, mu, w, nz, torch.float32, ref[6])
            monkeypatch.setenv("PLMC_FUSED_ASSEMBLE", "0")
            two = _run_logprob(eng, X, y, sc, mu, w, nz, torch.float32, ref[6])
            monkeypatch.delenv("PLMC_FUSED_ASSEMBLE")
        for a, b in zip(got, two):
            assert torch.equal(a, b), split
        e = float(((got[0] - ref[0]) / ref[0]).abs().max())
        print("PLMC_SPLIT=%s: log-prob rel err %.3g" % (split, e))
        assert e < 1e-4, (split, e)
        for name, a, b in zip(GRAD_NAMES, got[1:], ref[1:6]):
            e = float((a - b).abs().max() / b.abs().max())
            print("PLMC_SPLIT=%s: d/d %s err %.3g of the largest" % (split, name, e))
            assert e < 2e-3, (split, name, e)


def test_a_cosine_factor_that_is_exactly_zero(eng):
    """Inputs on a grid of quarters and mu = 1: mu tau is a multiple of 1/4, the cosine of many pairs is exactly 0 (and the product's
    derivative with respect to the other dimension's mean vanishes with it).  All gradients finite and equal to dense autograd."""
    q, M, d = 2, 2, 2
    g = torch.Generator().manual_seed(5)
    X = torch.randint(0, 8, (150, d), generator=g).double() / 4.0
    X = torch.unique(X, dim=0)
    n = X.shape[0]
    y = torch.randn(q, n, generator=g, dtype=torch.float64)
    sc = 0.2 + 0.2 * torch.rand(q, M, d, generator=g, dtype=torch.float64)
    mu = torch.ones(q, M, d, dtype=torch.float64)
    mu[:, 1, 1] = 0.5
    w = 0.5 + torch.rand(q, M, generator=g, dtype=torch.float64)
    nz = torch.tensor([0.3, 0.5], dtype=torch.float64)
    assert bool((torch.cos(2 * math.pi * (X[:, None, 0] - X[None, :, 0])).abs() < 1e-15).any())
    ref = _reference_logprob(X, y, sc, mu, w, nz)
    got = _run_logprob(eng, X, y, sc, mu, w, nz, torch.float64, ref[6])
    K = _assemble(eng, X, sc, mu, w, nz, torch.float64)
    assert bool((K[0][(X[:, None, 0] - X[None, :, 0]).abs() == 0.25] == 0).all())       # every component has the exact zero there
    for name, a, b in zip(("logp",) + GRAD_NAMES, got, ref[:6]):
        assert bool(torch.isfinite(a).all()), name
        assert torch.allclose(a, b, rtol=1e-7, atol=1e-9), (name, float((a - b).abs().max()))
    got32 = _run_logprob(eng, X, y, sc, mu, w, nz, torch.float32, ref[6])
    assert all(bool(torch.isfinite(a).all()) for a in got32)


# ------------------------------------------------------------------------------------------------ models
def _kernel_tables(cm, q):
    """(scales, means, weights) fp64 on the host from a (Scale)SpectralMixture module, by its gpytorch parameter names."""
    sp = torch.nn.functional.softplus
    base = cm.base_kernel if hasattr(cm, "base_kernel") else cm
    sd = {k: v.detach().cpu().double() for k, v in base.state_dict().items()}
    M = sd["raw_mixture_weights"].shape[-1]
    sc = sp(sd["raw_mixture_scales"]).reshape(q, M, -1)
    mu = sp(sd["raw_mixture_means"]).reshape(q, M, -1)
    w = sp(sd["raw_mixture_weights"]).reshape(q, M)
    if hasattr(cm, "base_kernel"):
        w = w * sp(cm.raw_outputscale.detach().cpu().double()).reshape(q, 1)
    return sc, mu, w


def _dense_model_loss(model, X, Y, q):
    """-(1 / n) mean over latents of log N(y_i - c_i; 0, K_i + noise_i I) with autograd through the raw parameters (host copies)."""
    sp = torch.nn.functional.softplus
    raw = {k: v.detach().cpu().double().requires_grad_() for k, v in model.named_parameters()}
    pre = "covar_module.base_kernel." if hasattr(model.covar_module, "base_kernel") else "covar_module."
    M = raw[pre + "raw_mixture_weights"].shape[-1]
    sc = sp(raw[pre + "raw_mixture_scales"]).reshape(q, M, -1)
    mu = sp(raw[pre + "raw_mixture_means"]).reshape(q, M, -1)
    w = sp(raw[pre + "raw_mixture_weights"]).reshape(q, M)
    if hasattr(model.covar_module, "base_kernel"):
        w = w * sp(raw["covar_module.raw_outputscale"]).reshape(q, 1)
    lik = model.likelihood
    noise = lik.noise_covar.raw_noise_constraint.transform(raw["likelihood.noise_covar.raw_noise"]).reshape(-1).expand(q)
    c = raw["mean_module.raw_constant"].reshape(q, 1) if "mean_module.raw_constant" in raw else raw["mean_module.constant"].reshape(q, 1)
    y = (Y.reshape(X.shape[0], -1).T if Y.dim() > 1 else Y.reshape(1, -1)) - c
    lp = smd.sm_logprob(X, y, sc, mu, w, noise)
    return -(lp.sum() / X.shape[0]), raw, (sc, mu, w, noise, c)


def _tidal(n, p, seed):
    g = torch.Generator().manual_seed(seed)
    X = torch.sort(torch.rand(n, 1, generator=g, dtype=torch.float64), 0)[0]
    Y = torch.stack([torch.sin(2 * math.pi * (3 + 2 * k) * X[:, 0]) + 0.3 * torch.randn(n, generator=g, dtype=torch.float64) for k in range(p)], 1)
    return X, Y


def test_single_output_exact_model_after_initialize_from_data(plmc):
    """ExactGPModel, ScaleKernel(SpectralMixtureKernel(M = 3)), initialize_from_data first, fp64: loss within 1e-9 relative of dense,
    every parameter gradient rtol 1e-5 / atol 1e-9, eval-mode posterior mean rtol 1e-7."""
    n, ns = 257, 40
    X, Y = _tidal(n, 1, seed=1)
    y = Y[:, 0]
    torch.manual_seed(4)
    m = plmc.ExactGPModel(X, y, plmc.GaussianLikelihood(), kernel_type=plmc.kernels.SpectralMixtureKernel, ker_kwargs={"num_mixtures": 3},
                          outputscales=True).double()
    m.covar_module.base_kernel.initialize_from_data(X, y)
    with torch.no_grad():                                  # scales of 1 / |N(0, 1)| can be huge: keep the kernel away from a pure diagonal
        m.covar_module.base_kernel.mixture_scales = m.covar_module.base_kernel.mixture_scales.clamp(max=3.0)
    m = m.to(DEV)
    m.train(); m.likelihood.train()
    mll = plmc.ExactMarginalLogLikelihood(m.likelihood, m)
    loss = -mll(m(X.to(DEV)), y.to(DEV))
    loss.backward()
    ref, raw, (sc, mu, w, noise, c) = _dense_model_loss(m, X, y, 1)
    ref.backward()
    assert abs(float(loss) - float(ref)) < 1e-9 * abs(float(ref)), (float(loss), float(ref))
    for name, prm in m.named_parameters():
        a, b = prm.grad.cpu().double(), raw[name].grad
        assert torch.allclose(a, b.reshape(a.shape), rtol=1e-5, atol=1e-9), (name, float((a - b.reshape(a.shape)).abs().max()))
    Xs = torch.rand(ns, 1, dtype=torch.float64)
    m.eval(); m.likelihood.eval()
    with torch.no_grad():
        post = m(Xs.to(DEV))
    mean_ref, cov_ref = smd.sm_posterior(X, (y - c.detach()[0]).reshape(1, n), Xs, sc.detach(), mu.detach(), w.detach(), noise.detach())
    assert torch.allclose(post.mean.cpu(), mean_ref[0] + c.detach()[0], rtol=1e-7, atol=1e-9)
    assert torch.allclose(post.variance.cpu(), torch.diagonal(cov_ref[0]), rtol=1e-6, atol=1e-9)


def test_batched_exact_model_latent_moments_against_dense(plmc):
    """n_tasks = 3 batched ExactGPModel, M = 5, fp64: loss and every parameter gradient against dense autograd, eval-mode mean /
    variance and compute_loo against dense conditioning."""
    n, q, ns = 200, 3, 30
    X, Y = _tidal(n, q, seed=2)
    torch.manual_seed(6)
    m = plmc.ExactGPModel(X, Y, plmc.GaussianLikelihood(batch_shape=torch.Size([q])), n_tasks=q,
                          kernel_type=plmc.kernels.SpectralMixtureKernel, ker_kwargs={"num_mixtures": 5}).double()
    perturb_(m)
    m = m.to(DEV)
    # training mode: the MLL (one value per task, / n) and every parameter gradient, tolerances of the single-output test
    m.train(); m.likelihood.train()
    loss = -plmc.ExactMarginalLogLikelihood(m.likelihood, m)(m(X.to(DEV)), Y.T.contiguous().to(DEV)).sum()
    loss.backward()
    ref, raw, _ = _dense_model_loss(m, X, Y, q)
    ref.backward()
    assert abs(float(loss) - float(ref)) < 1e-9 * abs(float(ref)), (float(loss), float(ref))
    for name, prm in m.named_parameters():
        a, b = prm.grad.cpu().double(), raw[name].grad.reshape(prm.shape)
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-9), (name, float((a - b).abs().max()))
    sc, mu, w = _kernel_tables(m.covar_module, q)
    noise = m.likelihood.noise.detach().cpu().double().reshape(-1)
    c = m.mean_module(X.to(DEV)).detach().cpu().double().reshape(q, n)
    Xs = torch.rand(ns, 1, dtype=torch.float64)
    cs = m.mean_module(Xs.to(DEV)).detach().cpu().double().reshape(q, ns)
    m.eval(); m.likelihood.eval()
    with torch.no_grad():
        post = m(Xs.to(DEV))
        s2, r = m.compute_loo()
    mean_ref, cov_ref = smd.sm_posterior(X, Y.T - c, Xs, sc, mu, w, noise)
    assert torch.allclose(post.mean.cpu().reshape(q, ns), mean_ref + cs, rtol=1e-7, atol=1e-9)
    assert torch.allclose(post.variance.cpu().reshape(q, ns), torch.diagonal(cov_ref, dim1=-2, dim2=-1), rtol=1e-6, atol=1e-9)
    Kinv = torch.linalg.inv(smd.sm_kernel(X, X, sc, mu, w) + noise[:, None, None] * torch.eye(n, dtype=torch.float64))
    dg = torch.diagonal(Kinv, dim1=-2, dim2=-1)
    assert torch.allclose(s2.cpu().T, 1.0 / dg, rtol=1e-8) and torch.allclose(r.cpu().T, (Kinv @ (Y.T - c).unsqueeze(-1)).squeeze(-1) / dg, rtol=1e-7, atol=1e-10)


def _projected(plmc, X, Y, q, seed=5, **kw):
    torch.manual_seed(seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return plmc.ProjectedGPModel(X, Y, Y.shape[1], q, mean_type=plmc.ZeroMean, kernel_type=plmc.kernels.SpectralMixtureKernel,
                                     ker_kwargs={"num_mixtures": 3}, init_lmc_coeffs=True, **kw)


def _oracle_dict(model):
    """The oracle's parameter dict (oracle/projected.py) WITHOUT kernel keys, from the state dict, as oracle/bridge.py reads it
    (bulk H, or the parametrised Q_plus . R of bulk=False), and the map product parameter name -> dict key."""
    lb = model.likelihood.noise_covar.raw_noise_constraint.lower_bound
    sd = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
    lmc = model.lmc_coefficients
    P = dict(n_tasks=model.n_tasks, n_latents=model.n_latents, mode=lmc.mode, BDN=not hasattr(model, "M"), eps=model.eps,
             scalar_B=model.scalar_B, diagonal_B=model.diagonal_B, noise_lb=lb, noise_thresh=math.log(lb), bulk=lmc.bulk,
             raw_noise=sd["likelihood.noise_covar.raw_noise"], B_tilde_inv_chol_raw=sd["parametrizations.B_tilde_inv_chol.original"])
    names = {"likelihood.noise_covar.raw_noise": "raw_noise", "parametrizations.B_tilde_inv_chol.original": "B_tilde_inv_chol_raw"}
    if lmc.bulk:
        P["H"] = sd["lmc_coefficients.H"]
        names["lmc_coefficients.H"] = "H"
    else:
        P["Q_plus_original"] = sd["lmc_coefficients.parametrizations.Q_plus.original"]
        P["Q_plus_base"] = sd.get("lmc_coefficients.parametrizations.Q_plus.0.base")
        P["ortho_param"] = lmc.parametrizations.Q_plus[0].orthogonal_map.name
        P["R_original"] = sd["lmc_coefficients.parametrizations.R.original"]
        P["diagonal_R"] = type(lmc.parametrizations.R[0]).__name__ == "PositiveDiagonalParam"
        names["lmc_coefficients.parametrizations.Q_plus.original"] = "Q_plus_original"
        names["lmc_coefficients.parametrizations.R.original"] = "R_original"
    kern = {k: v for k, v in sd.items() if k.startswith("covar_module.")}
    return P, kern, names


def _latent_K(kern, Xa, Xb, q):
    """The latent covariances (q, na, nb) from the kernel's raw parameters (gpytorch names), dense."""
    sp = torch.nn.functional.softplus
    M = kern["covar_module.raw_mixture_weights"].shape[-1]
    return smd.sm_kernel(Xa, Xb, sp(kern["covar_module.raw_mixture_scales"]).reshape(q, M, -1),
                         sp(kern["covar_module.raw_mixture_means"]).reshape(q, M, -1), sp(kern["covar_module.raw_mixture_weights"]).reshape(q, M))


@pytest.mark.parametrize("bulk", [True, False])
def test_projected_model_loss_gradients_and_eval_mode_against_dense(plmc, bulk):
    """fp64, p = 5, q = 3, d = 1, M = 3, perturbed parameters; the body and the tolerances of
    tests/test_gpu_additive_engine.py:258-323.  ProjectedLMCmll and the gradient of every parameter against
    sum_i log N(ytil_i; 0, K_i + noise_i I) / n + the oracle's projection terms (1e-9 relative; rtol 2e-6, atol 1e-8); eval mode (task
    mean / variance, observation variance, latent mean and full covariance) against dense conditioning (rtol 1e-8 / 1e-7); compute_loo
    against 1 / diag(K^-1) and K^-1 y / diag(K^-1) (1e-8).  The second eval call hits the prediction cache."""
    from projectedlmc import settings
    n, p, q, ns = 300, 5, 3, 40
    X, Y = _tidal(n, p, seed=3)
    m = perturb_(_projected(plmc, X, Y, q, bulk=bulk).double())
    P, kern, names = _oracle_dict(m)
    leaves = {**{k: P[k] for k in names.values()}, **kern}
    for v in leaves.values():
        v.requires_grad_(True)
    eye = torch.eye(n, dtype=torch.float64)
    ytil = pj.project_data(P, Y)
    K = _latent_K(kern, X, X, q) + pj.projected_noise(P).reshape(q, 1, 1) * eye
    terms, const = pj.projection_terms(P, Y)
    ref = -(gm.mvn_log_prob(K, ytil).sum() / n + sum(terms) + const)
    ref.backward()

    m = m.to(DEV)
    Xd, Yd = X.to(DEV), Y.to(DEV)
    m.train(); m.likelihood.train()
    mll = plmc.ProjectedLMCmll(m.likelihood, m)
    loss = -mll(m(Xd), Yd)
    loss.backward()
    print("bulk=%s: loss %.12g, dense %.12g" % (bulk, float(loss), float(ref)))
    assert abs(float(loss) - float(ref)) < 1e-9 * abs(float(ref)), (float(loss), float(ref))
    checked = 0
    for pname, prm in m.named_parameters():
        g_ref = leaves[names.get(pname, pname)].grad
        assert prm.grad is not None and g_ref is not None, pname
        assert prm.grad.shape == g_ref.shape, pname
        assert torch.allclose(prm.grad.cpu(), g_ref, rtol=2e-6, atol=1e-8), (pname, prm.grad.cpu(), g_ref)
        checked += 1
    assert checked == len(names) + 3                        # + the three planes of the mixture table

    # ---- eval mode
    with torch.no_grad():
        Pd = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in P.items()}
        kd = {k: v.detach() for k, v in kern.items()}
        K, ytil = K.detach(), ytil.detach()
        Xs = torch.rand(ns, 1, dtype=torch.float64)
        Ks, Kss = _latent_K(kd, X, Xs, q), _latent_K(kd, Xs, Xs, q)
        sol = torch.linalg.solve(K, Ks)
        mu_lat = (sol * ytil.unsqueeze(-1)).sum(1)                                    # (q, ns)
        cov_lat = Kss - Ks.transpose(-1, -2) @ sol
        Ht = pj.lmc_coefficients(Pd)
        mean_ref = mu_lat.T @ Ht
        var_ref = torch.diagonal(cov_lat, dim1=-2, dim2=-1).T @ (Ht * Ht) + Pd["eps"]
        Lf = pj.full_noise_factor(Pd)
        Kinv = torch.linalg.inv(K)
        kdiag = torch.diagonal(Kinv, dim1=-2, dim2=-1)
        alpha = (Kinv @ ytil.unsqueeze(-1)).squeeze(-1)
    m.eval(); m.likelihood.eval()
    with settings.prediction_cache("eager"), torch.no_grad():
        dist = m(Xs.to(DEV))
        c = m._prediction_cache()
        assert (c.hits, c.misses) == (0, 1) and c.ws is not None and c.ws.with_inverse
        again = m(Xs.to(DEV))
        assert (c.hits, c.misses) == (1, 1)
        obs = m.full_likelihood()(dist)
        lat = m.compute_latent_distrib(Xs.to(DEV), full_cov=True)
        s2, r = m.compute_loo()
    for d_ in (dist, again):
        assert torch.allclose(d_.mean.cpu(), mean_ref, rtol=1e-8, atol=1e-10)
        assert torch.allclose(d_.variance.cpu(), var_ref, rtol=1e-7, atol=1e-10)
    assert torch.allclose(obs.variance.cpu(), var_ref + torch.diagonal(Lf @ Lf.T)[None, :], rtol=1e-7, atol=1e-10)
    assert torch.allclose(lat.mean.cpu(), mu_lat, rtol=1e-8, atol=1e-10)
    assert torch.allclose(lat.covariance_matrix.cpu(), cov_lat, rtol=1e-7, atol=1e-10)
    assert torch.allclose(s2.cpu(), (1.0 / kdiag).T, rtol=1e-8, atol=0)
    assert torch.allclose(r.cpu(), (alpha / kdiag).T, rtol=1e-8, atol=1e-12)


def test_latent_shards_sum_to_the_unsharded_loss_and_gradients(plmc):
    """tests/test_gpu_additive_engine.py:346-370 (1e-10 / 1e-8): the table is sliced by latent_ids like ell is."""
    n, p, q, world = 300, 6, 3, 2
    X, Y = _tidal(n, p, seed=21)
    Xd, Yd = X.to(DEV), Y.to(DEV)

    def build(shard):
        m = perturb_(_projected(plmc, X, Y, q, seed=2, latent_shard=shard).double()).to(DEV)
        m.train(); m.likelihood.train()
        return m, plmc.ProjectedLMCmll(m.likelihood, m)

    m0, mll0 = build(None)
    loss0 = -mll0(m0(Xd), Yd)
    loss0.backward()
    total, grads = 0.0, None
    for rank in range(world):
        m1, mll1 = build((rank, world))
        share = -mll1(m1(Xd), Yd)
        share.backward()
        total = total + float(share.detach())
        gs = [torch.zeros_like(prm) if prm.grad is None else prm.grad.clone() for prm in m1.parameters()]
        grads = gs if grads is None else [a + b for a, b in zip(grads, gs)]
    assert abs(total - float(loss0)) < 1e-10 * abs(float(loss0)), (total, float(loss0))
    for (name, prm), g in zip(m0.named_parameters(), grads):
        assert torch.allclose(prm.grad, g, rtol=1e-8, atol=1e-11), (name, (prm.grad - g).abs().max())


# ------------------------------------------------------------------------------------------------ inherited machinery, refusals
def test_table_at_the_noise_floor_walks_the_jitter_ladder(eng):
    """The form of tests/test_gpu_additive_engine.py:373: fp32, n = 300 points on U(0, 1), one nearly constant component (scale 0.02,
    mean 0.01) and noise e^-40.  That it needs jitter is checked on the host first (an fp32 LAPACK Cholesky fails without jitter and
    succeeds at a rung <= 1e-1).  Under cholesky_max_tries(8) the log-prob and its gradients end finite, one warning per rung."""
    n, q = 300, 2
    g = torch.Generator().manual_seed(3)
    X = torch.rand(n, 1, generator=g, dtype=torch.float64).float()
    y = torch.randn(q, n, generator=g, dtype=torch.float64).float()
    sc, mu, w = torch.full((q, 1, 1), 0.02), torch.full((q, 1, 1), 0.01), torch.ones(q, 1)
    noise = torch.full((q,), math.exp(-40.0))
    K = smd.sm_kernel(X, X, sc, mu, w)
    eye = torch.eye(n)
    ok = lambda jit: not bool(torch.linalg.cholesky_ex(K + (math.exp(-40.0) + jit) * eye)[1].any())
    assert K.dtype == torch.float32 and not ok(0.0) and any(ok(1e-6 * 10 ** i) for i in range(6))
    table = torch.stack([sc, mu], 1).to(DEV).requires_grad_()
    with eng.settings.cholesky_max_tries(8), warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        lp = eng.exact.exact_latent_log_prob("sm", X.to(DEV), table, w.to(DEV), noise.to(DEV), y.to(DEV))
        lp.sum().backward()
        torch.cuda.synchronize()
    jit = [str(w_.message) for w_ in rec if "not p.d." in str(w_.message)]
    base = eng.settings.cholesky_jitter.value(torch.float32)
    assert 1 <= len(jit) <= 8
    assert jit == ["A not p.d., added jitter of %.1e to the diagonal" % (base * 10 ** i) for i in range(len(jit))], jit
    assert bool(torch.isfinite(lp).all()) and bool(torch.isfinite(table.grad).all())


def test_limits_are_argument_errors(eng):
    """nmix or d over the limits: refused on the host, nothing is launched."""
    hip = eng.hip
    L = hip.lib()
    Mx, Dx = L.cdll.plmc_sm_max_mixtures(), L.cdll.plmc_sm_max_dim()
    for M, d, word in ((Mx + 1, 1, "mixtures"), (1, Dx + 1, "plmc_sm_max_dim")):
        n, q = 130, 1
        X = torch.rand(n, d, device=DEV, dtype=torch.float64)
        z = torch.ones(q, M, d, device=DEV, dtype=torch.float64)
        w, nz = torch.ones(q, M, device=DEV, dtype=torch.float64), torch.ones(q, device=DEV, dtype=torch.float64)
        ws = eng.exact.Workspace(n, q, 0, torch.float64, DEV, with_inverse=False)
        with pytest.raises(RuntimeError, match=word):
            L.call("plmc_assemble_sm", torch.float64, hip.ptr(X), n, d, M, hip.ptr(z), hip.ptr(z), hip.ptr(w), hip.ptr(nz), hip.ptr(ws.A),
                   ws.lda, ws.strideA, q, hip.stream_ptr(DEV))
        out = torch.empty(q, n, n, device=DEV, dtype=torch.float64)
        with pytest.raises(RuntimeError, match=word):
            L.call("plmc_assemble_cross_sm", torch.float64, hip.ptr(X), n, hip.ptr(X), n, d, M, hip.ptr(z), hip.ptr(z), hip.ptr(w), hip.ptr(out),
                   n, n * n, 0, n, q, hip.stream_ptr(DEV))
        # the fused factorisation and the gradient call check the limits before they touch a pointer
        wi = eng.exact.Workspace(n, q, 1, torch.float64, DEV, with_inverse=True)
        with pytest.raises(RuntimeError, match=word):
            L.call("plmc_factorize_sm_ex", torch.float64, hip.ptr(X), n, d, M, hip.ptr(z), hip.ptr(z), hip.ptr(w), hip.ptr(nz), hip.ptr(wi.A),
                   wi.n_pad, wi.lda, wi.naug, wi.strideA, hip.ptr(wi.Vd), hip.ptr(wi.logdet), hip.ptr(wi.info), 1, q, hip.ptr(nz),
                   hip.stream_ptr(DEV))
        gt = torch.empty(q, 2 * M * d + 1 + M, device=DEV, dtype=torch.float64)
        with pytest.raises(RuntimeError, match=word):
            L.call("plmc_kinv_grad_sm_vd", torch.float64, hip.ptr(wi.W), wi.n_pad, wi.ldw, wi.strideW, hip.ptr(wi.alpha), hip.ptr(X), n, d, M,
                   hip.ptr(z), hip.ptr(z), hip.ptr(w), hip.ptr(gt), None, 0, 0, None, hip.ptr(wi.partials), q, hip.ptr(nz), hip.ptr(wi.Vd),
                   hip.stream_ptr(DEV))
        with pytest.raises(ValueError, match="plmc_sm_max"):
            eng.exact.exact_latent_log_prob("sm", X, torch.stack([z, z], 1), w, nz, torch.zeros(q, n, device=DEV, dtype=torch.float64))
