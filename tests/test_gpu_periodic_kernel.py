"""Periodic kernel on the batched exact engine: the new entry points per element, the fp32 phase reduction at large phase, the
log-prob and every entry of the gradient table of `ExactLatentLogProb` (fp64; fp32 on every arithmetic of the sweep, fused and two-call
assembly), a sine that is exactly zero, `ExactGPModel` (single and batched) and `ProjectedGPModel` (loss, gradients, eval mode, LOO,
prediction cache, latent sharding) and the argument errors.

Reference values: the dense fp64 formula of tests/_periodic_dense.py (torch CPU, autograd).  Sizes: n = 130 (two blocks of 128, ragged
edge, 2 x 2 tiles) and n = 257 (3 x 3 tiles), d in {1, 3, 8} (the three compile-time capacities 1, 4, 8), q in {1, 3}.  Tolerances: those
of tests/test_gpu_sm_kernel.py / tests/test_gpu_additive_engine.py (named beside each use); the fp32 per-element bound is derived in
DESIGN.md ("Periodic kernel: the phase in fp32"), not measured:
    |err| <= 24 d 2^-24 os (1 + 1 / min_k ell_k)   against the fp64 formula at the fp32-rounded inputs and parameters,
at small and at large phase alike."""
import math
import warnings

import pytest
import torch

import _periodic_dense as pd
from oracle import gp_math as gm
from oracle import projected as pj
from _bridge import perturb_

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U32 = 2.0 ** -24
PK = "periodic"


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


def _problem(n, d, q, seed, ns=1):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    X, Xs = r(n, d), r(ns, d)
    y = torch.randn(q, n, generator=g, dtype=torch.float64)
    ell = (0.6 + 1.4 * r(q, d)) * d
    period = 0.3 + 1.2 * r(q, d)
    os_ = 0.5 + r(q)
    noise = 0.05 + 0.5 * r(q)
    return X, Xs, y, ell, period, os_, noise


def fp32_bound(d, ell, os_):
    """(q, 1, 1): 24 d 2^-24 os (1 + 1 / min_k ell_k)."""
    return (24 * d * U32 * os_ * (1.0 + 1.0 / ell.min(-1)[0]))[:, None, None]


def _assemble(eng, X, ell, period, os_, noise, dt):
    """plmc_assemble_per_*: the upper triangle of Khat, (q, n, n) fp64 on the host."""
    hip = eng.hip
    L = hip.lib()
    f = lambda t: t.to(DEV, dt).contiguous()
    n, d = X.shape
    q = ell.shape[0]
    ws = eng.exact.Workspace(n, q, 0, dt, DEV, with_inverse=False)
    ws.A.zero_()
    Xd, l_, p_, o_, nz = (f(t) for t in (X, ell, period, os_, noise))
    L.call("plmc_assemble_per", dt, hip.ptr(Xd), n, d, hip.ptr(l_), hip.ptr(p_), hip.ptr(o_), hip.ptr(nz), hip.ptr(ws.A), ws.lda,
           ws.strideA, q, hip.stream_ptr(DEV))
    torch.cuda.synchronize()
    return torch.triu(ws.A[:, :n, :n].cpu().double())


def _cross(eng, X, Xs, ell, period, os_, dt):
    f = lambda t: t.to(DEV, dt).contiguous()
    K = eng.exact.dense_cross(PK, f(X), f(Xs), torch.stack([f(ell), f(period)], 1), f(os_))
    torch.cuda.synchronize()
    return K.cpu().double()


# ------------------------------------------------------------------------------------------------ per element
@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n,d,q", [(130, 1, 1), (257, 3, 3), (257, 8, 3), (130, 8, 1), (257, 1, 3)])
def test_assembly_and_cross_against_the_dense_formula(eng, n, d, q, dt):
    """plmc_assemble_per / plmc_assemble_cross_per at phases of up to ~3 revolutions.
    fp64: |err| <= 1e-12 (|ref| + os).  fp32: the bound of the module docstring, diagonal (os + noise) included."""
    assert d <= eng.hip.lib().cdll.plmc_per_max_dim()
    ns = 70
    X, Xs, _, ell, per, os_, nz = _problem(n, d, q, seed=10 * d + n, ns=ns)
    if dt == torch.float32:
        X, Xs, ell, per, os_, nz = (t.float().double() for t in (X, Xs, ell, per, os_, nz))
    ref = torch.triu(pd.per_kernel(X, X, ell, per, os_) + nz[:, None, None] * torch.eye(n, dtype=torch.float64))
    refx = pd.per_kernel(X, Xs, ell, per, os_)
    got, gotx = _assemble(eng, X, ell, per, os_, nz, dt), _cross(eng, X, Xs, ell, per, os_, dt)
    scale = os_[:, None, None]
    for name, a, b in (("assemble", got, ref), ("cross", gotx, refx)):
        err = (a - b).abs()
        if dt == torch.float64:
            print("%s f64: max err / (|ref| + os) %.3g" % (name, float((err / (b.abs() + scale)).max())))
            assert bool((err <= 1e-12 * (b.abs() + scale)).all()), name
        else:
            bound = fp32_bound(d, ell, os_)
            print("%s f32: max err / bound %.3g" % (name, float((err / bound).max())))
            assert bool((err <= bound).all()), name
    assert bool((torch.diagonal(got, dim1=-2, dim2=-1) == (os_.to(dt) + nz.to(dt)).double()[:, None]).all())      # k(x, x) = os exactly


def large_phase_inputs():
    """n = 257 near-uniform points in [0, 1], period 5e-4: tau / p reaches ~2000 revolutions.  fp32-rounded, as fp64."""
    n = 257
    g = torch.Generator().manual_seed(0)
    X = ((torch.arange(n, dtype=torch.float64) + 0.3 * torch.rand(n, generator=g, dtype=torch.float64)) / n).reshape(n, 1)
    X[0, 0], X[-1, 0] = 0.0, 1.0
    ell = torch.tensor([[1.0]], dtype=torch.float64)
    per = torch.tensor([[5.0e-4]], dtype=torch.float64)
    os_ = torch.tensor([1.3], dtype=torch.float64)
    return tuple(t.float().double() for t in (X, ell, per, os_))


def naive_fp32(X, ell, per, os_):
    """The naive restatement, all in torch float32 on the CPU: os exp(-2 sin(pi (tau / p))^2 / ell)."""
    Xf, lf, pf, of = (t.float() for t in (X, ell, per, os_))
    tau = Xf[:, None, 0] - Xf[None, :, 0]
    s = torch.sin(math.pi * (tau / pf[0, 0]))
    return of[0] * torch.exp(-2.0 * s * s / lf[0, 0])


def test_large_phase_fp32_assembly_meets_the_bound_and_the_naive_form_does_not(eng):
    X, ell, per, os_ = large_phase_inputs()
    n = X.shape[0]
    nz = torch.tensor([0.1], dtype=torch.float64).float().double()
    ref = pd.per_kernel(X, X, ell, per, os_)
    bound = float(fp32_bound(1, ell, os_))
    e_naive = float((naive_fp32(X, ell, per, os_).double() - ref[0]).abs().max())
    got = _assemble(eng, X, ell, per, os_, nz, torch.float32)
    e = float((got[0] - torch.triu(ref[0] + nz[0] * torch.eye(n, dtype=torch.float64))).abs().max())
    Xs = X[:50] + 0.25
    ex = float((_cross(eng, X, Xs.float().double(), ell, per, os_, torch.float32) - pd.per_kernel(X, Xs.float().double(), ell, per, os_)).abs().max())
    print("largest phase %.4g revolutions; bound %.3g; assembly err %.3g; cross err %.3g; naive fp32 err %.3g"
          % (float((X.max() - X.min()) / per[0, 0]), bound, e, ex, e_naive))
    assert float((X.max() - X.min()) / per[0, 0]) > 1990
    assert e_naive > bound, (e_naive, bound)
    assert e <= bound, (e, bound)
    assert ex <= bound, (ex, bound)


# ------------------------------------------------------------------------------------------------ log-prob and the gradient table
def _reference_logprob(X, y, ell, per, os_, nz):
    leaves = [t.clone().requires_grad_() for t in (ell, per, os_, nz, y)]
    lp = pd.per_logprob(X, leaves[4], leaves[0], leaves[1], leaves[2], leaves[3])
    g = torch.Generator().manual_seed(99)
    wt = 0.5 + torch.rand(lp.shape, generator=g, dtype=torch.float64)
    (lp * wt).sum().backward()
    return [lp.detach()] + [t.grad for t in leaves] + [wt]


def _run_logprob(eng, X, y, ell, per, os_, nz, dt, wt):
    f = lambda t: t.to(DEV, dt)
    table = torch.stack([f(ell), f(per)], 1).requires_grad_()
    leaves = [f(t).requires_grad_() for t in (os_, nz, y)]
    lp = eng.exact.exact_latent_log_prob(PK, f(X), table, leaves[0], leaves[1], leaves[2])
    (lp * f(wt)).sum().backward()
    torch.cuda.synchronize()
    tg = table.grad.cpu().double()
    return [lp.detach().cpu().double(), tg[:, 0], tg[:, 1]] + [t.grad.cpu().double() for t in leaves]


GRAD_NAMES = ("lengthscale", "period", "oscale", "noise", "y")


@pytest.mark.parametrize("n,d,q", [(257, 1, 3), (130, 3, 1), (257, 8, 3)])
def test_logprob_and_every_gradient_fp64(eng, n, d, q):
    """Tolerances of tests/test_gpu_sm_kernel.py: log-prob rtol 1e-10; gradients rtol 1e-7 / atol 1e-9."""
    X, _, y, ell, per, os_, nz = _problem(n, d, q, seed=n + d)
    ref = _reference_logprob(X, y, ell, per, os_, nz)
    got = _run_logprob(eng, X, y, ell, per, os_, nz, torch.float64, ref[6])
    assert torch.allclose(got[0], ref[0], rtol=1e-10, atol=0), (got[0], ref[0])
    for name, a, b in zip(GRAD_NAMES, got[1:], ref[1:6]):
        assert a.shape == b.shape, name
        print("d/d %s: max abs err %.3g" % (name, float((a - b).abs().max())))
        assert torch.allclose(a, b, rtol=1e-7, atol=1e-9), (name, float((a - b).abs().max()))


def test_logprob_without_an_output_scale_fp64(eng):
    """oscale = None (a bare PeriodicKernel): unit output scale, no gradient for it."""
    n, d, q = 130, 3, 3
    X, _, y, ell, per, _, nz = _problem(n, d, q, seed=8)
    one = torch.ones(q, dtype=torch.float64)
    ref = _reference_logprob(X, y, ell, per, one, nz)
    f = lambda t: t.to(DEV)
    table = torch.stack([f(ell), f(per)], 1).requires_grad_()
    nzd = f(nz).requires_grad_()
    lp = eng.exact.exact_latent_log_prob(PK, f(X), table, None, nzd, f(y))
    (lp * f(ref[6])).sum().backward()
    assert torch.allclose(lp.detach().cpu(), ref[0], rtol=1e-10, atol=0)
    assert torch.allclose(table.grad.cpu()[:, 0], ref[1], rtol=1e-7, atol=1e-9) and torch.allclose(table.grad.cpu()[:, 1], ref[2], rtol=1e-7, atol=1e-9)
    assert torch.allclose(nzd.grad.cpu(), ref[4], rtol=1e-7, atol=1e-9)


def _factor_buffer(eng, X, ell, per, os_, nz, y, fused, monkeypatch):
    """The factor buffer of one fp32 factorisation with the inverse factor, zeroed first."""
    f = lambda t: t.to(DEV, torch.float32).contiguous()
    n, q = X.shape[0], ell.shape[0]
    ws = eng.exact.Workspace(n, q, 1, torch.float32, DEV, with_inverse=True)
    ws.A.zero_()
    ws.Vd.zero_()
    if not fused:
        monkeypatch.setenv("PLMC_FUSED_ASSEMBLE", "0")
    eng.exact.factorize(PK, f(X), torch.stack([f(ell), f(per)], 1), f(os_), f(nz), f(y).reshape(q, 1, n), ws)
    if not fused:
        monkeypatch.delenv("PLMC_FUSED_ASSEMBLE")
    torch.cuda.synchronize()
    return ws.A.cpu(), ws.logdet.cpu()


@pytest.mark.parametrize("d", [1, 3])
def test_logprob_fp32_on_every_arithmetic_and_fused_against_two_call_assembly(eng, monkeypatch, d):
    """n = 257, q = 3, fp32 with PLMC_SPLIT unset, 0 and 3: value 1e-4 relative, gradients 2e-3 of the largest entry (the fp32 cases of
    tests/test_gpu_additive_engine.py).  The fused assembly and PLMC_FUSED_ASSEMBLE=0 give the same factor buffer, log-determinant,
    value and gradients as bit patterns.  d = 1 runs the gradient kernel on the arithmetic the knob names; with d > 1 it forms K^-1 with
    the fp32 matrix instructions whatever the knob says (include/plmc.h)."""
    n, q = 257, 3
    X, _, y, ell, per, os_, nz = (t.float().double() for t in _problem(n, d, q, seed=77 + d))
    ref = _reference_logprob(X, y, ell, per, os_, nz)
    monkeypatch.delenv("PLMC_SPLIT", raising=False)                     # "unset" means unset, whatever the caller's environment
    monkeypatch.delenv("PLMC_FUSED_ASSEMBLE", raising=False)
    eng.hip.lib().cdll.plmc_dev_reload_knobs()

    def check(tag):
        got = _run_logprob(eng, X, y, ell, per, os_, nz, torch.float32, ref[6])
        monkeypatch.setenv("PLMC_FUSED_ASSEMBLE", "0")
        two = _run_logprob(eng, X, y, ell, per, os_, nz, torch.float32, ref[6])
        monkeypatch.delenv("PLMC_FUSED_ASSEMBLE")
        for a, b in zip(got, two):
            assert torch.equal(a, b), tag
        A1, ld1 = _factor_buffer(eng, X, ell, per, os_, nz, y, True, monkeypatch)
        A2, ld2 = _factor_buffer(eng, X, ell, per, os_, nz, y, False, monkeypatch)
        assert torch.equal(A1, A2) and torch.equal(ld1, ld2), tag
        e = float(((got[0] - ref[0]) / ref[0]).abs().max())
        print("PLMC_SPLIT %s: log-prob rel err %.3g" % (tag, e))
        assert e < 1e-4, (tag, e)
        for name, a, b in zip(GRAD_NAMES, got[1:], ref[1:6]):
            e = float((a - b).abs().max() / b.abs().max())
            print("PLMC_SPLIT %s: d/d %s err %.3g of the largest" % (tag, name, e))
            assert e < 2e-3, (tag, name, e)

    check("unset")
    for split in ("0", "3"):
        with eng.hip.knob("PLMC_SPLIT", split):
            check(split)


def test_a_sine_that_is_exactly_zero(eng):
    """Inputs on a grid of quarters and periods 0.25 and 0.5: tau is an integer multiple of p for every pair (p = 0.25) or every other
    one (p = 0.5), so sin(pi tau / p) is exactly 0 there and the covariance exactly os.  All gradients finite and equal to dense autograd."""
    q, d = 2, 2
    g = torch.Generator().manual_seed(5)
    X = torch.unique(torch.randint(0, 8, (150, d), generator=g).double() / 4.0, dim=0)
    n = X.shape[0]
    y = torch.randn(q, n, generator=g, dtype=torch.float64)
    ell = 0.7 + torch.rand(q, d, generator=g, dtype=torch.float64)
    per = torch.tensor([[0.25, 0.5], [0.5, 1.0]], dtype=torch.float64)
    os_ = torch.tensor([0.8, 1.4], dtype=torch.float64)
    nz = torch.tensor([0.3, 0.5], dtype=torch.float64)
    ref = _reference_logprob(X, y, ell, per, os_, nz)
    got = _run_logprob(eng, X, y, ell, per, os_, nz, torch.float64, ref[6])
    K = _assemble(eng, X, ell, per, os_, nz, torch.float64)
    tau = X[:, None, :] - X[None, :, :]
    whole = ((tau[..., 0] / 0.25) % 1 == 0) & ((tau[..., 1] / 0.5) % 1 == 0) & torch.triu(torch.ones(n, n, dtype=torch.bool), 1)
    assert bool(whole.any()) and bool((K[0][whole] == os_[0]).all())
    for name, a, b in zip(("logp",) + GRAD_NAMES, got, ref[:6]):
        assert bool(torch.isfinite(a).all()), name
        assert torch.allclose(a, b, rtol=1e-7, atol=1e-9), (name, float((a - b).abs().max()))
    got32 = _run_logprob(eng, X, y, ell, per, os_, nz, torch.float32, ref[6])
    assert all(bool(torch.isfinite(a).all()) for a in got32)
    for name, a, b in zip(GRAD_NAMES, got32[1:], ref[1:6]):
        assert float((a - b).abs().max() / b.abs().max()) < 2e-3, name


# ------------------------------------------------------------------------------------------------ models
def _tables(raw, pre, q):
    """(ell, period) (q, d) from a dict of raw parameters under the gpytorch names `pre`raw_lengthscale / raw_period_length."""
    sp = torch.nn.functional.softplus
    return sp(raw[pre + "raw_lengthscale"]).reshape(q, -1), sp(raw[pre + "raw_period_length"]).reshape(q, -1)


def _dense_model_loss(model, X, Y, q):
    """-(1 / n) sum over latents of log N(y_i - c_i; 0, K_i + noise_i I) with autograd through the raw parameters (host copies)."""
    sp = torch.nn.functional.softplus
    raw = {k: v.detach().cpu().double().requires_grad_() for k, v in model.named_parameters()}
    scaled = hasattr(model.covar_module, "base_kernel")
    ell, per = _tables(raw, "covar_module.base_kernel." if scaled else "covar_module.", q)
    os_ = sp(raw["covar_module.raw_outputscale"]).reshape(q) if scaled else None
    lik = model.likelihood
    noise = lik.noise_covar.raw_noise_constraint.transform(raw["likelihood.noise_covar.raw_noise"]).reshape(-1).expand(q)
    c = raw["mean_module.raw_constant"].reshape(q, 1) if "mean_module.raw_constant" in raw else raw["mean_module.constant"].reshape(q, 1)
    y = (Y.reshape(X.shape[0], -1).T if Y.dim() > 1 else Y.reshape(1, -1)) - c
    lp = pd.per_logprob(X, y, ell, per, os_, noise)
    return -(lp.sum() / X.shape[0]), raw, (ell, per, os_, noise, c)


def _tidal(n, p, seed, d=1):
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(n, d, generator=g, dtype=torch.float64)
    X[:, 0] = torch.sort(X[:, 0])[0]
    Y = torch.stack([torch.sin(2 * math.pi * (1 + k) * X[:, 0]) + 0.3 * torch.randn(n, generator=g, dtype=torch.float64) for k in range(p)], 1)
    return X, Y


def test_single_output_exact_model(plmc):
    """ExactGPModel, ScaleKernel(PeriodicKernel), d = 1, fp64; the tolerances of the spectral-mixture test of the same name: loss within
    1e-9 relative of dense, every parameter gradient rtol 1e-5 / atol 1e-9, eval-mode mean rtol 1e-7, variance rtol 1e-6."""
    n, ns = 257, 40
    X, Y = _tidal(n, 1, seed=1)
    y = Y[:, 0]
    torch.manual_seed(4)
    m = perturb_(plmc.ExactGPModel(X, y, plmc.GaussianLikelihood(), kernel_type=plmc.kernels.PeriodicKernel, outputscales=True).double())
    m = m.to(DEV)
    m.train(); m.likelihood.train()
    mll = plmc.ExactMarginalLogLikelihood(m.likelihood, m)
    loss = -mll(m(X.to(DEV)), y.to(DEV))
    loss.backward()
    ref, raw, (ell, per, os_, noise, c) = _dense_model_loss(m, X, y, 1)
    ref.backward()
    assert abs(float(loss) - float(ref)) < 1e-9 * abs(float(ref)), (float(loss), float(ref))
    names = [nm for nm, _ in m.named_parameters()]
    assert "covar_module.base_kernel.raw_period_length" in names and "covar_module.base_kernel.raw_lengthscale" in names
    for name, prm in m.named_parameters():
        a, b = prm.grad.cpu().double(), raw[name].grad
        assert torch.allclose(a, b.reshape(a.shape), rtol=1e-5, atol=1e-9), (name, float((a - b.reshape(a.shape)).abs().max()))
    Xs = torch.rand(ns, 1, dtype=torch.float64)
    m.eval(); m.likelihood.eval()
    with torch.no_grad():
        post = m(Xs.to(DEV))
        s2, r = m.compute_loo()
    dt_ = lambda t: t.detach()
    mean_ref, cov_ref = pd.per_posterior(X, (y - dt_(c)[0]).reshape(1, n), Xs, dt_(ell), dt_(per), dt_(os_), dt_(noise))
    assert torch.allclose(post.mean.cpu(), mean_ref[0] + dt_(c)[0], rtol=1e-7, atol=1e-9)
    assert torch.allclose(post.variance.cpu(), torch.diagonal(cov_ref[0]), rtol=1e-6, atol=1e-9)
    Kinv = torch.linalg.inv(pd.per_kernel(X, X, dt_(ell), dt_(per), dt_(os_))[0] + dt_(noise)[0] * torch.eye(n, dtype=torch.float64))
    dg = torch.diagonal(Kinv)
    assert torch.allclose(s2.cpu().reshape(-1), 1.0 / dg, rtol=1e-8)
    assert torch.allclose(r.cpu().reshape(-1), (Kinv @ (y - dt_(c)[0, 0])) / dg, rtol=1e-7, atol=1e-10)


def test_batched_exact_model_latent_moments_against_dense(plmc):
    """n_tasks = 3 batched ExactGPModel on d = 3 inputs, fp64: loss and every parameter gradient against dense autograd, eval-mode mean /
    variance and compute_loo against dense conditioning; the tolerances of the spectral-mixture test of the same name."""
    n, q, ns, d = 200, 3, 30, 3
    X, Y = _tidal(n, q, seed=2, d=d)
    torch.manual_seed(6)
    m = plmc.ExactGPModel(X, Y, plmc.GaussianLikelihood(batch_shape=torch.Size([q])), n_tasks=q,
                          kernel_type=plmc.kernels.PeriodicKernel).double()
    perturb_(m)
    m = m.to(DEV)
    m.train(); m.likelihood.train()
    loss = -plmc.ExactMarginalLogLikelihood(m.likelihood, m)(m(X.to(DEV)), Y.T.contiguous().to(DEV)).sum()
    loss.backward()
    ref, raw, (ell, per, os_, noise, _) = _dense_model_loss(m, X, Y, q)
    ref.backward()
    assert abs(float(loss) - float(ref)) < 1e-9 * abs(float(ref)), (float(loss), float(ref))
    for name, prm in m.named_parameters():
        a, b = prm.grad.cpu().double(), raw[name].grad.reshape(prm.shape)
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-9), (name, float((a - b).abs().max()))
    ell, per, noise = ell.detach(), per.detach(), noise.detach()
    os_ = None if os_ is None else os_.detach()
    c = m.mean_module(X.to(DEV)).detach().cpu().double().reshape(q, n)
    Xs = torch.rand(ns, d, dtype=torch.float64)
    cs = m.mean_module(Xs.to(DEV)).detach().cpu().double().reshape(q, ns)
    m.eval(); m.likelihood.eval()
    with torch.no_grad():
        post = m(Xs.to(DEV))
        s2, r = m.compute_loo()
    mean_ref, cov_ref = pd.per_posterior(X, Y.T - c, Xs, ell, per, os_, noise)
    assert torch.allclose(post.mean.cpu().reshape(q, ns), mean_ref + cs, rtol=1e-7, atol=1e-9)
    assert torch.allclose(post.variance.cpu().reshape(q, ns), torch.diagonal(cov_ref, dim1=-2, dim2=-1), rtol=1e-6, atol=1e-9)
    Kinv = torch.linalg.inv(pd.per_kernel(X, X, ell, per, os_) + noise[:, None, None] * torch.eye(n, dtype=torch.float64))
    dg = torch.diagonal(Kinv, dim1=-2, dim2=-1)
    assert torch.allclose(s2.cpu().T, 1.0 / dg, rtol=1e-8) and torch.allclose(r.cpu().T, (Kinv @ (Y.T - c).unsqueeze(-1)).squeeze(-1) / dg, rtol=1e-7, atol=1e-10)


def _projected(plmc, X, Y, q, seed=5, **kw):
    torch.manual_seed(seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return plmc.ProjectedGPModel(X, Y, Y.shape[1], q, mean_type=plmc.ZeroMean, kernel_type=plmc.kernels.PeriodicKernel,
                                     init_lmc_coeffs=True, **kw)


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
    ell, per = _tables(kern, "covar_module.", q)
    return pd.per_kernel(Xa, Xb, ell, per)


@pytest.mark.parametrize("bulk", [True, False])
def test_projected_model_loss_gradients_and_eval_mode_against_dense(plmc, bulk):
    """fp64, p = 5, q = 3, d = 1, perturbed parameters; the body and the tolerances of the spectral-mixture test of the same name.
    ProjectedLMCmll and the gradient of every parameter against sum_i log N(ytil_i; 0, K_i + noise_i I) / n + the oracle's projection
    terms (1e-9 relative; rtol 2e-6, atol 1e-8); eval mode (task mean / variance, observation variance, latent mean and full covariance)
    against dense conditioning (rtol 1e-8 / 1e-7); compute_loo against 1 / diag(K^-1) and K^-1 y / diag(K^-1) (1e-8).  The second eval
    call hits the prediction cache."""
    from projectedlmc import settings
    n, p, q, ns = 257, 5, 3, 40
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
    assert checked == len(names) + 2                        # + the two rows of the periodic table

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
        dense = m.covar_module(Xd).evaluate()
    for d_ in (dist, again):
        assert torch.allclose(d_.mean.cpu(), mean_ref, rtol=1e-8, atol=1e-10)
        assert torch.allclose(d_.variance.cpu(), var_ref, rtol=1e-7, atol=1e-10)
    assert torch.allclose(obs.variance.cpu(), var_ref + torch.diagonal(Lf @ Lf.T)[None, :], rtol=1e-7, atol=1e-10)
    assert torch.allclose(lat.mean.cpu(), mu_lat, rtol=1e-8, atol=1e-10)
    assert torch.allclose(lat.covariance_matrix.cpu(), cov_lat, rtol=1e-7, atol=1e-10)
    assert torch.allclose(s2.cpu(), (1.0 / kdiag).T, rtol=1e-8, atol=0)
    assert torch.allclose(r.cpu(), (alpha / kdiag).T, rtol=1e-8, atol=1e-12)
    assert torch.allclose(dense.cpu(), _latent_K(kd, X, X, q), rtol=1e-10, atol=1e-12)               # evaluate()


def test_latent_shards_sum_to_the_unsharded_loss_and_gradients(plmc):
    """The shards of a latent-sharded projected model sum to the unsharded loss (1e-10) and gradients (rtol 1e-8): the table is sliced by
    latent_ids like ell is."""
    n, p, q, world = 257, 6, 3, 2
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


# ------------------------------------------------------------------------------------------------ limits
def test_limits_are_argument_errors(eng):
    """d = 9 and a null table pointer: refused on the host by every entry point, nothing is launched."""
    hip = eng.hip
    L = hip.lib()
    Dx = L.cdll.plmc_per_max_dim()
    assert Dx == 8
    n, q, f64 = 130, 1, torch.float64
    for d, null, word in ((Dx + 1, False, "plmc_per_max_dim"), (2, True, "null pointer")):
        X = torch.rand(n, d, device=DEV, dtype=f64)
        z = torch.ones(q, d, device=DEV, dtype=f64)
        per = None if null else hip.ptr(z)
        o, nz = torch.ones(q, device=DEV, dtype=f64), torch.ones(q, device=DEV, dtype=f64)
        ws = eng.exact.Workspace(n, q, 0, f64, DEV, with_inverse=False)
        with pytest.raises(RuntimeError, match=word):
            L.call("plmc_assemble_per", f64, hip.ptr(X), n, d, hip.ptr(z), per, hip.ptr(o), hip.ptr(nz), hip.ptr(ws.A), ws.lda, ws.strideA, q,
                   hip.stream_ptr(DEV))
        out = torch.empty(q, n, n, device=DEV, dtype=f64)
        with pytest.raises(RuntimeError, match=word):
            L.call("plmc_assemble_cross_per", f64, hip.ptr(X), n, hip.ptr(X), n, d, hip.ptr(z), per, hip.ptr(o), hip.ptr(out), n, n * n, 0, n, q,
                   hip.stream_ptr(DEV))
        wi = eng.exact.Workspace(n, q, 1, f64, DEV, with_inverse=True, per=True)
        with pytest.raises(RuntimeError, match=word):
            L.call("plmc_factorize_per_ex", f64, hip.ptr(X), n, d, hip.ptr(z), per, hip.ptr(o), hip.ptr(nz), hip.ptr(wi.A), wi.n_pad, wi.lda,
                   wi.naug, wi.strideA, hip.ptr(wi.Vd), hip.ptr(wi.logdet), hip.ptr(wi.info), 1, q, hip.ptr(nz), hip.stream_ptr(DEV))
        gt = torch.empty(q, 2 * d + 2, device=DEV, dtype=f64)
        with pytest.raises(RuntimeError, match=word):
            L.call("plmc_kinv_grad_per_vd", f64, hip.ptr(wi.W), wi.n_pad, wi.ldw, wi.strideW, hip.ptr(wi.alpha), hip.ptr(X), n, d, hip.ptr(z),
                   per, hip.ptr(o), hip.ptr(gt), None, 0, 0, None, hip.ptr(wi.partials), q, hip.ptr(nz), hip.ptr(wi.Vd), hip.stream_ptr(DEV))
    X = torch.rand(n, Dx + 1, device=DEV, dtype=f64)
    table = torch.ones(q, 2, Dx + 1, device=DEV, dtype=f64)
    with pytest.raises(ValueError, match="plmc_per_max_dim"):
        eng.exact.exact_latent_log_prob(PK, X, table, None, torch.ones(q, device=DEV, dtype=f64), torch.zeros(q, n, device=DEV, dtype=f64))
