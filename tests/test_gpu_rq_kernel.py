"""Rational-quadratic kernel on the batched exact engine: the new entry points per element (small and large alpha), the log-prob and
every entry of the gradient table of `ExactLatentLogProb` (fp64; fp32 on every arithmetic of the sweep, fused and two-call assembly),
the alpha-gradient at large alpha, `ExactGPModel` (single and batched), `ProjectedGPModel` (loss, gradients, eval mode, prediction
cache), `LeaveOneOutPseudoLikelihood`, and the argument errors.

Reference values: the dense fp64 formula of tests/_rq_dense.py (torch CPU, autograd).  Sizes: n = 130 (two blocks of 128, ragged edge,
2 x 2 tiles) and n = 257 (3 x 3 tiles), d in {1, 3, 8, plmc_rq_max_dim() = 16} (the compile-time capacities 1, 4, 8, 16), q in {1, 3}.
Tolerances: those of tests/test_gpu_periodic_kernel.py (named beside each use); the fp32 per-element bound is the operation count of
DESIGN.md 7.5, independent of alpha, not measured:
    |err| <= (d + 8) 2^-24 os   against the fp64 formula at the fp32-rounded inputs and parameters."""
import math
import warnings

import pytest
import torch

import _rq_dense as rd
import _loo_dense as ld
from oracle import gp_math as gm
from oracle import projected as pj
from _bridge import perturb_

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
RQ = "rq"


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
    """alpha per latent log-uniform over [0.05, 50]."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    X, Xs = r(n, d), r(ns, d)
    y = torch.randn(q, n, generator=g, dtype=torch.float64)
    ell = (0.3 + 0.7 * r(q, d)) * math.sqrt(d)
    alpha = 0.05 * torch.pow(torch.tensor(1000.0, dtype=torch.float64), r(q))
    os_ = 0.5 + r(q)
    noise = 0.05 + 0.5 * r(q)
    return X, Xs, y, ell, alpha, os_, noise


def _table(ell, alpha):
    return torch.cat([ell, alpha.reshape(-1, 1)], 1)


def _assemble(eng, X, ell, alpha, os_, noise, dt):
    """plmc_assemble_rq_*: the upper triangle of Khat, (q, n, n) in the element type, on the host."""
    hip = eng.hip
    L = hip.lib()
    f = lambda t: t.to(DEV, dt).contiguous()
    n, d = X.shape
    q = ell.shape[0]
    ws = eng.exact.Workspace(n, q, 0, dt, DEV, with_inverse=False)
    ws.A.zero_()
    Xd, l_, a_, o_, nz = (f(t) for t in (X, ell, alpha, os_, noise))
    L.call("plmc_assemble_rq", dt, hip.ptr(Xd), n, d, hip.ptr(l_), hip.ptr(a_), hip.ptr(o_), hip.ptr(nz), hip.ptr(ws.A), ws.lda,
           ws.strideA, q, hip.stream_ptr(DEV))
    torch.cuda.synchronize()
    return torch.triu(ws.A[:, :n, :n].cpu())


def _cross(eng, X, Xs, ell, alpha, os_, dt):
    f = lambda t: t.to(DEV, dt).contiguous()
    K = eng.exact.dense_cross(RQ, f(X), f(Xs), _table(f(ell), f(alpha)), f(os_))
    torch.cuda.synchronize()
    return K.cpu()


# ------------------------------------------------------------------------------------------------ per element
@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n,d,q", [(130, 1, 1), (257, 3, 3), (257, 8, 3), (130, "max", 1)])
def test_assembly_and_cross_against_the_dense_formula(eng, n, d, q, dt):
    """plmc_assemble_rq / plmc_assemble_cross_rq.  fp64: |err| <= 1e-12 (|ref| + os).  fp32: (d + 8) 2^-24 os.  The diagonal is
    os + noise as a bit pattern; a coincident pair off the diagonal (inside a tile, across tiles, and in the cross block) gives
    exactly os."""
    if d == "max":
        d = eng.hip.lib().cdll.plmc_rq_max_dim()
    ns = 70
    X, Xs, _, ell, al, os_, nz = _problem(n, d, q, seed=10 * d + n, ns=ns)
    X[40], X[n - 1], Xs[7] = X[5], X[3], X[11]                   # coincident pairs (5, 40), (3, n - 1) and cross (11, 7)
    if dt == torch.float32:
        X, Xs, ell, al, os_, nz = (t.float().double() for t in (X, Xs, ell, al, os_, nz))
    ref = torch.triu(rd.rq_kernel(X, X, ell, al, os_) + nz[:, None, None] * torch.eye(n, dtype=torch.float64))
    refx = rd.rq_kernel(X, Xs, ell, al, os_)
    got, gotx = _assemble(eng, X, ell, al, os_, nz, dt), _cross(eng, X, Xs, ell, al, os_, dt)
    scale = os_[:, None, None]
    for name, a, b in (("assemble", got.double(), ref), ("cross", gotx.double(), refx)):
        err = (a - b).abs()
        if dt == torch.float64:
            print("%s f64: max err / (|ref| + os) %.3g" % (name, float((err / (b.abs() + scale)).max())))
            assert bool((err <= 1e-12 * (b.abs() + scale)).all()), name
        else:
            bound = rd.fp32_bound(d, os_)
            print("%s f32 d=%d: max err %.2f u, bound %d u (u = 2^-24 os)" % (name, d, float((err / (rd.U32 * scale)).max()), d + 8))
            assert bool((err <= bound).all()), name
    osd, nzd = os_.to(dt), nz.to(dt)
    assert torch.equal(torch.diagonal(got, dim1=-2, dim2=-1), (osd + nzd)[:, None].expand(q, n))       # one rounding: os + noise
    assert torch.equal(got[:, 5, 40], osd) and torch.equal(got[:, 3, n - 1], osd) and torch.equal(gotx[:, 11, 7], osd)


@pytest.mark.parametrize("alpha", [1.0e4, 1.0e6])
def test_large_alpha_fp32_assembly_meets_the_bound_and_the_pow_form_does_not(eng, alpha):
    """The inputs of DESIGN.md 7.5's large-alpha figures (n = 257 on [0, 1], d = 1, ell = 0.2): the fp32 assembly and cross block stay within 9 2^-24 at
    alpha = 1e4 and 1e6; pow(1 + u, -alpha) in fp32, computed here on the CPU, does not."""
    X, ell, al, os_ = rd.large_alpha_inputs(alpha)
    n = X.shape[0]
    nz = torch.tensor([0.1], dtype=torch.float64).float().double()
    ref = rd.rq_kernel(X, X, ell, al, os_)
    bound = float(rd.fp32_bound(1, os_))
    e_naive = float((rd.naive_fp32(X, X, ell, al, os_).double() - ref[0]).abs().max())
    got = _assemble(eng, X, ell, al, os_, nz, torch.float32).double()
    e = float((got[0] - torch.triu(ref[0] + nz[0] * torch.eye(n, dtype=torch.float64))).abs().max())
    Xs = (X[:50] + 0.013).float().double()
    ex = float((_cross(eng, X, Xs, ell, al, os_, torch.float32).double() - rd.rq_kernel(X, Xs, ell, al, os_)).abs().max())
    print("alpha %g: bound %.3g (9 u); assembly err %.2f u; cross err %.2f u; pow form in fp32 %.3g = %.0f u"
          % (alpha, bound, e / rd.U32, ex / rd.U32, e_naive, e_naive / rd.U32))
    assert e_naive > bound, (e_naive, bound)
    assert e <= bound, (e, bound)
    assert ex <= bound, (ex, bound)


# ------------------------------------------------------------------------------------------------ log-prob and the gradient table
def _reference_logprob(X, y, ell, al, os_, nz):
    leaves = [t.clone().requires_grad_() for t in (ell, al, os_, nz, y)]
    lp = rd.rq_logprob(X, leaves[4], leaves[0], leaves[1], leaves[2], leaves[3])
    g = torch.Generator().manual_seed(99)
    wt = 0.5 + torch.rand(lp.shape, generator=g, dtype=torch.float64)
    (lp * wt).sum().backward()
    return [lp.detach()] + [t.grad for t in leaves] + [wt]


def _run_logprob(eng, X, y, ell, al, os_, nz, dt, wt):
    f = lambda t: t.to(DEV, dt)
    d = ell.shape[1]
    table = _table(f(ell), f(al)).requires_grad_()
    leaves = [f(t).requires_grad_() for t in (os_, nz, y)]
    lp = eng.exact.exact_latent_log_prob(RQ, f(X), table, leaves[0], leaves[1], leaves[2])
    (lp * f(wt)).sum().backward()
    torch.cuda.synchronize()
    tg = table.grad.cpu().double()
    return [lp.detach().cpu().double(), tg[:, :d], tg[:, d]] + [t.grad.cpu().double() for t in leaves]


GRAD_NAMES = ("lengthscale", "alpha", "oscale", "noise", "y")


@pytest.mark.parametrize("n,d,q", [(257, 1, 3), (130, 3, 1), (257, 8, 3), (130, "max", 1)])
def test_logprob_and_every_gradient_fp64(eng, n, d, q):
    """Tolerances of tests/test_gpu_periodic_kernel.py: log-prob rtol 1e-10; gradients rtol 1e-7 / atol 1e-9.  The case (257, 1, 3) has a
    latent at alpha = 1e3, where every u is below 1/8: the series branch of h.  In fp64 the direct form would pass as well, so this pins
    the formula, not the branch.  d = plmc_rq_max_dim() is the largest capacity of the gradient kernel (alpha in the slot behind the
    lengthscales')."""
    if d == "max":
        d = eng.hip.lib().cdll.plmc_rq_max_dim()
    X, _, y, ell, al, os_, nz = _problem(n, d, q, seed=n + d)
    if (n, d) == (257, 1):
        al[1] = 1.0e3
    ref = _reference_logprob(X, y, ell, al, os_, nz)
    got = _run_logprob(eng, X, y, ell, al, os_, nz, torch.float64, ref[6])
    assert torch.allclose(got[0], ref[0], rtol=1e-10, atol=0), (got[0], ref[0])
    for name, a, b in zip(GRAD_NAMES, got[1:], ref[1:6]):
        assert a.shape == b.shape, name
        print("d/d %s: max abs err %.3g" % (name, float((a - b).abs().max())))
        assert torch.allclose(a, b, rtol=1e-7, atol=1e-9), (name, float((a - b).abs().max()))


def test_logprob_without_an_output_scale_fp64(eng):
    """oscale = None (a bare RQKernel): unit output scale, no gradient for it."""
    n, d, q = 130, 3, 3
    X, _, y, ell, al, _, nz = _problem(n, d, q, seed=8)
    one = torch.ones(q, dtype=torch.float64)
    ref = _reference_logprob(X, y, ell, al, one, nz)
    f = lambda t: t.to(DEV)
    table = _table(f(ell), f(al)).requires_grad_()
    nzd = f(nz).requires_grad_()
    lp = eng.exact.exact_latent_log_prob(RQ, f(X), table, None, nzd, f(y))
    (lp * f(ref[6])).sum().backward()
    assert torch.allclose(lp.detach().cpu(), ref[0], rtol=1e-10, atol=0)
    assert torch.allclose(table.grad.cpu()[:, :d], ref[1], rtol=1e-7, atol=1e-9) and torch.allclose(table.grad.cpu()[:, d], ref[2], rtol=1e-7, atol=1e-9)
    assert torch.allclose(nzd.grad.cpu(), ref[4], rtol=1e-7, atol=1e-9)


def _factor_buffer(eng, X, ell, al, os_, nz, y, fused, monkeypatch):
    """The factor buffer of one fp32 factorisation with the inverse factor, zeroed first."""
    f = lambda t: t.to(DEV, torch.float32).contiguous()
    n, q = X.shape[0], ell.shape[0]
    ws = eng.exact.Workspace(n, q, 1, torch.float32, DEV, with_inverse=True)
    ws.A.zero_()
    ws.Vd.zero_()
    if not fused:
        monkeypatch.setenv("PLMC_FUSED_ASSEMBLE", "0")
    eng.exact.factorize(RQ, f(X), _table(f(ell), f(al)), f(os_), f(nz), f(y).reshape(q, 1, n), ws)
    if not fused:
        monkeypatch.delenv("PLMC_FUSED_ASSEMBLE")
    torch.cuda.synchronize()
    return ws.A.cpu(), ws.logdet.cpu()


@pytest.mark.parametrize("d", [1, 3, "max"])
def test_logprob_fp32_on_every_arithmetic_and_fused_against_two_call_assembly(eng, monkeypatch, d):
    """n = 257, q = 3, alpha = (0.3, 2, 40), fp32 with PLMC_SPLIT unset, 0 and 3: value 1e-4 relative, each gradient 2e-3 of that
    tensor's largest entry (the project's fp32 tolerances).  The fused assembly and PLMC_FUSED_ASSEMBLE=0 give the same factor buffer,
    log-determinant, value and gradients as bit patterns.  y is drawn from an RQ prior with OTHER parameters, not white noise: with
    white-noise y the alpha-gradient is a sum that cancels 10^4-fold and the tolerance would measure that cancellation.
    d = plmc_rq_max_dim() runs the largest capacity of the 512-thread split-engine kernel (two fp16 planes) and of the fp32 MFMA one."""
    if d == "max":
        d = eng.hip.lib().cdll.plmc_rq_max_dim()
    n, q = 257, 3
    X, _, _, ell, _, os_, nz = _problem(n, d, q, seed=77 + d)
    al = torch.tensor([0.3, 2.0, 40.0], dtype=torch.float64)
    y = rd.prior_draw(X, 1.6 * ell, torch.tensor([1.0, 0.5, 5.0], dtype=torch.float64), 0.8 * os_, 0.5 * nz, seed=3)
    X, y, ell, al, os_, nz = (t.float().double() for t in (X, y, ell, al, os_, nz))
    ref = _reference_logprob(X, y, ell, al, os_, nz)
    monkeypatch.delenv("PLMC_SPLIT", raising=False)                     # "unset" means unset, whatever the caller's environment
    monkeypatch.delenv("PLMC_FUSED_ASSEMBLE", raising=False)
    eng.hip.lib().cdll.plmc_dev_reload_knobs()

    def check(tag):
        got = _run_logprob(eng, X, y, ell, al, os_, nz, torch.float32, ref[6])
        monkeypatch.setenv("PLMC_FUSED_ASSEMBLE", "0")
        two = _run_logprob(eng, X, y, ell, al, os_, nz, torch.float32, ref[6])
        monkeypatch.delenv("PLMC_FUSED_ASSEMBLE")
        for a, b in zip(got, two):
            assert torch.equal(a, b), tag
        A1, ld1 = _factor_buffer(eng, X, ell, al, os_, nz, y, True, monkeypatch)
        A2, ld2 = _factor_buffer(eng, X, ell, al, os_, nz, y, False, monkeypatch)
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


def test_alpha_gradient_at_large_alpha_fp32(eng, monkeypatch):
    """q = 1, d = 1, n = 257, alpha = 1e3 (every u <= 0.0125: the series branch of h), y drawn from a prior with alpha = 0.5.  Asserts the
    project's 2e-3 on dL/dalpha against the fp64 dense value and prints the relative error, beside the same figure of two CPU
    restatements with fp64-exact K^-1 weights: fp32 k and the accurate fp32 h (the reference the GPU figure is read against,
    profiles/rq_accuracy.md), and fp32 k with the direct h (what the series avoids)."""
    X, ell, al, os_ = rd.large_alpha_inputs(1.0e3)
    n = X.shape[0]
    nz = torch.tensor([0.1], dtype=torch.float64).float().double()
    y = rd.prior_draw(X, ell, torch.tensor([0.5], dtype=torch.float64), os_, nz, seed=11).float().double()
    ref = _reference_logprob(X, y, ell, al, os_, nz)
    want = float(ref[2][0] / ref[6][0])                                  # d logp / d alpha (the weight divided out)
    # CPU restatements: W = 1/2 (a a^T - K^-1) exact, d K_ij / d alpha = -k h(u) per element in fp32, summed in fp64
    Kh = rd.rq_kernel(X, X, ell, al, os_)[0] + nz[0] * torch.eye(n, dtype=torch.float64)
    P = torch.linalg.inv(Kh)
    a = P @ y[0]
    W = 0.5 * (a[:, None] * a[None, :] - P)
    sd = (X.float()[:, None, 0] - X.float()[None, :, 0]) * (1.0 / ell.float()[0, 0])
    u = (sd * sd) * (0.5 / al.float()[0])
    k32 = rd.prescribed_fp32(X, X, ell, al, os_)
    cpu_acc = float((W * (-(k32 * rd.h_accurate_fp32(u))).double()).sum())
    cpu_dir = float((W * (-(k32 * rd.h_direct_fp32(u))).double()).sum())
    monkeypatch.delenv("PLMC_SPLIT", raising=False)
    eng.hip.lib().cdll.plmc_dev_reload_knobs()
    got = _run_logprob(eng, X, y, ell, al, os_, nz, torch.float32, ref[6])
    have = float(got[2][0] / ref[6][0])
    rel = abs(have - want) / abs(want)
    print("dL/dalpha at alpha = 1e3: fp64 dense %.9g; GPU fp32 %.9g, rel err %.3g; CPU fp32 accurate h rel err %.3g; CPU fp32 direct h rel err %.3g"
          % (want, have, rel, abs(cpu_acc - want) / abs(want), abs(cpu_dir - want) / abs(want)))
    assert float(u.max()) < 0.125
    assert rel < 2e-3, rel


# ------------------------------------------------------------------------------------------------ models
def _tables(raw, pre, q):
    """(ell (q, d), alpha (q)) from a dict of raw parameters under the gpytorch names `pre`raw_lengthscale / raw_alpha."""
    sp = torch.nn.functional.softplus
    return sp(raw[pre + "raw_lengthscale"]).reshape(q, -1), sp(raw[pre + "raw_alpha"]).reshape(q)


def _dense_pieces(model, X, Y, q):
    """Host copies of the raw parameters (leaves) and the dense (ell, alpha, os, noise, y - c) built from them."""
    sp = torch.nn.functional.softplus
    raw = {k: v.detach().cpu().double().requires_grad_() for k, v in model.named_parameters()}
    scaled = hasattr(model.covar_module, "base_kernel")
    ell, al = _tables(raw, "covar_module.base_kernel." if scaled else "covar_module.", q)
    os_ = sp(raw["covar_module.raw_outputscale"]).reshape(q) if scaled else None
    lik = model.likelihood
    noise = lik.noise_covar.raw_noise_constraint.transform(raw["likelihood.noise_covar.raw_noise"]).reshape(-1).expand(q)
    c = raw["mean_module.raw_constant"].reshape(q, 1) if "mean_module.raw_constant" in raw else raw["mean_module.constant"].reshape(q, 1)
    y = (Y.reshape(X.shape[0], -1).T if Y.dim() > 1 else Y.reshape(1, -1)) - c
    return raw, (ell, al, os_, noise, c, y)


def _dense_model_loss(model, X, Y, q):
    """-(1 / n) sum over latents of log N(y_i - c_i; 0, K_i + noise_i I) with autograd through the raw parameters."""
    raw, (ell, al, os_, noise, c, y) = _dense_pieces(model, X, Y, q)
    lp = rd.rq_logprob(X, y, ell, al, os_, noise)
    return -(lp.sum() / X.shape[0]), raw, (ell, al, os_, noise, c)


def _data(n, p, seed, d=1):
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(n, d, generator=g, dtype=torch.float64)
    X[:, 0] = torch.sort(X[:, 0])[0]
    Y = torch.stack([torch.sin(2 * math.pi * (1 + k) * X[:, 0]) + 0.3 * torch.randn(n, generator=g, dtype=torch.float64) for k in range(p)], 1)
    return X, Y


def test_single_output_exact_model(plmc):
    """ExactGPModel, ScaleKernel(RQKernel), d = 2, fp64; the tolerances of the periodic test of the same name: loss within 1e-9 relative
    of dense, every parameter gradient rtol 1e-5 / atol 1e-9, eval-mode mean rtol 1e-7, variance rtol 1e-6, full_cov likewise;
    kernel_cond(), lscales() and outputscale() read the kernel."""
    n, ns, d = 200, 40, 2
    X, Y = _data(n, 1, seed=1, d=d)
    y = Y[:, 0]
    torch.manual_seed(4)
    m = perturb_(plmc.ExactGPModel(X, y, plmc.GaussianLikelihood(), kernel_type=plmc.RQKernel, outputscales=True).double())
    m = m.to(DEV)
    m.train(); m.likelihood.train()
    mll = plmc.ExactMarginalLogLikelihood(m.likelihood, m)
    loss = -mll(m(X.to(DEV)), y.to(DEV))
    loss.backward()
    ref, raw, (ell, al, os_, noise, c) = _dense_model_loss(m, X, y, 1)
    ref.backward()
    assert abs(float(loss) - float(ref)) < 1e-9 * abs(float(ref)), (float(loss), float(ref))
    names = [nm for nm, _ in m.named_parameters()]
    assert "covar_module.base_kernel.raw_alpha" in names and "covar_module.base_kernel.raw_lengthscale" in names
    for name, prm in m.named_parameters():
        a, b = prm.grad.cpu().double(), raw[name].grad
        assert torch.allclose(a, b.reshape(a.shape), rtol=1e-5, atol=1e-9), (name, float((a - b.reshape(a.shape)).abs().max()))
    Xs = torch.rand(ns, d, dtype=torch.float64)
    m.eval(); m.likelihood.eval()
    with torch.no_grad():
        post = m(Xs.to(DEV))
        full = m(Xs.to(DEV), full_cov=True)
        cond = m.kernel_cond()
    dt_ = lambda t: t.detach()
    mean_ref, cov_ref = rd.rq_posterior(X, (y - dt_(c)[0]).reshape(1, n), Xs, dt_(ell), dt_(al), dt_(os_), dt_(noise))
    assert torch.allclose(post.mean.cpu(), mean_ref[0] + dt_(c)[0], rtol=1e-7, atol=1e-9)
    assert torch.allclose(post.variance.cpu(), torch.diagonal(cov_ref[0]), rtol=1e-6, atol=1e-9)
    assert torch.allclose(full.covariance_matrix.cpu().reshape(ns, ns), cov_ref[0], rtol=1e-6, atol=1e-9)
    Kh = rd.rq_kernel(X, X, dt_(ell), dt_(al), dt_(os_))[0] + dt_(noise)[0] * torch.eye(n, dtype=torch.float64)
    assert abs(float(cond) - float(torch.linalg.cond(Kh))) < 1e-6 * float(torch.linalg.cond(Kh))
    assert torch.allclose(m.lscales().cpu().double().reshape(-1), dt_(ell).reshape(-1), rtol=1e-12)
    assert torch.allclose(m.outputscale().cpu().double().reshape(-1), dt_(os_).reshape(-1), rtol=1e-6)    # (outputscale() returns float32)


def test_loo_pseudo_likelihood_on_the_single_output_model(plmc):
    """LeaveOneOutPseudoLikelihood with an RQKernel: value 1e-9 relative, every raw-parameter gradient rtol 1e-5 / atol 1e-9 against
    the dense objective of tests/_loo_dense.py (the tolerances of tests/test_gpu_loo_objective.py's model tests)."""
    n, d = 150, 3
    X, Y = _data(n, 1, seed=9, d=d)
    y = Y[:, 0]
    lik = plmc.GaussianLikelihood()
    torch.manual_seed(2)
    m = perturb_(plmc.ExactGPModel(X, y, lik, kernel_type=plmc.RQKernel, outputscales=True).double())
    raw, (ell, al, os_, noise, c, resid) = _dense_pieces(m, X, y, 1)
    Kh = rd.rq_kernel(X, X, ell, al, os_) + noise.reshape(1, 1, 1) * torch.eye(n, dtype=torch.float64)
    ref = ld.loo_log_prob(Kh, resid) / n
    ref.sum().backward()
    m, lik = m.to(DEV), lik.to(DEV)
    m.train(); lik.train()
    out = plmc.LeaveOneOutPseudoLikelihood(lik, m, X, y)(m(X.to(DEV)), y.to(DEV))
    out.sum().backward()
    assert abs(float(out.sum()) - float(ref.sum())) <= 1e-9 * abs(float(ref.sum())), (float(out.sum()), float(ref.sum()))
    for name, prm in m.named_parameters():
        assert prm.grad is not None and raw[name].grad is not None, name
        a, b = prm.grad.cpu(), raw[name].grad.reshape(prm.shape)
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-9), (name, a, b)


def test_batched_exact_model_latent_moments_against_dense(plmc):
    """n_tasks = 3 batched ExactGPModel on d = 3 inputs, fp64: loss and every parameter gradient against dense autograd, eval-mode mean /
    variance against dense conditioning; the tolerances of the periodic test of the same name."""
    n, q, ns, d = 200, 3, 30, 3
    X, Y = _data(n, q, seed=2, d=d)
    torch.manual_seed(6)
    m = plmc.ExactGPModel(X, Y, plmc.GaussianLikelihood(batch_shape=torch.Size([q])), n_tasks=q, kernel_type=plmc.RQKernel).double()
    perturb_(m)
    m = m.to(DEV)
    m.train(); m.likelihood.train()
    loss = -plmc.ExactMarginalLogLikelihood(m.likelihood, m)(m(X.to(DEV)), Y.T.contiguous().to(DEV)).sum()
    loss.backward()
    ref, raw, (ell, al, os_, noise, _) = _dense_model_loss(m, X, Y, q)
    ref.backward()
    assert abs(float(loss) - float(ref)) < 1e-9 * abs(float(ref)), (float(loss), float(ref))
    for name, prm in m.named_parameters():
        a, b = prm.grad.cpu().double(), raw[name].grad.reshape(prm.shape)
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-9), (name, float((a - b).abs().max()))
    ell, al, noise = ell.detach(), al.detach(), noise.detach()
    os_ = None if os_ is None else os_.detach()
    c = m.mean_module(X.to(DEV)).detach().cpu().double().reshape(q, n)
    Xs = torch.rand(ns, d, dtype=torch.float64)
    cs = m.mean_module(Xs.to(DEV)).detach().cpu().double().reshape(q, ns)
    m.eval(); m.likelihood.eval()
    with torch.no_grad():
        post = m(Xs.to(DEV))
    mean_ref, cov_ref = rd.rq_posterior(X, Y.T - c, Xs, ell, al, os_, noise)
    assert torch.allclose(post.mean.cpu().reshape(q, ns), mean_ref + cs, rtol=1e-7, atol=1e-9)
    assert torch.allclose(post.variance.cpu().reshape(q, ns), torch.diagonal(cov_ref, dim1=-2, dim2=-1), rtol=1e-6, atol=1e-9)


def _projected(plmc, X, Y, q, seed=5, **kw):
    torch.manual_seed(seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return plmc.ProjectedGPModel(X, Y, Y.shape[1], q, mean_type=plmc.ZeroMean, kernel_type=plmc.RQKernel, init_lmc_coeffs=True, **kw)


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
    ell, al = _tables(kern, "covar_module.", q)
    return rd.rq_kernel(Xa, Xb, ell, al)


@pytest.mark.parametrize("bulk", [True, False])
def test_projected_model_loss_gradients_and_eval_mode_against_dense(plmc, bulk):
    """fp64, p = 5, q = 3, d = 2, n = 200, perturbed parameters; the body and the tolerances of the periodic test of the same name.
    ProjectedLMCmll and the gradient of every parameter against sum_i log N(ytil_i; 0, K_i + noise_i I) / n + the oracle's projection
    terms (1e-9 relative; rtol 2e-6, atol 1e-8); eval mode (task mean / variance, observation variance, latent mean and full covariance)
    against dense conditioning (rtol 1e-8 / 1e-7).  The second eval call hits the prediction cache and equals the first; evaluate()
    gives the dense latent covariances."""
    from projectedlmc import settings
    n, p, q, ns, d = 200, 5, 3, 40, 2
    X, Y = _data(n, p, seed=3, d=d)
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
    assert checked == len(names) + 2                        # + the lengthscales and alpha

    # ---- eval mode
    with torch.no_grad():
        Pd = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in P.items()}
        kd = {k: v.detach() for k, v in kern.items()}
        K, ytil = K.detach(), ytil.detach()
        Xs = torch.rand(ns, d, dtype=torch.float64)
        Ks, Kss = _latent_K(kd, X, Xs, q), _latent_K(kd, Xs, Xs, q)
        sol = torch.linalg.solve(K, Ks)
        mu_lat = (sol * ytil.unsqueeze(-1)).sum(1)                                    # (q, ns)
        cov_lat = Kss - Ks.transpose(-1, -2) @ sol
        Ht = pj.lmc_coefficients(Pd)
        mean_ref = mu_lat.T @ Ht
        var_ref = torch.diagonal(cov_lat, dim1=-2, dim2=-1).T @ (Ht * Ht) + Pd["eps"]
        Lf = pj.full_noise_factor(Pd)
    m.eval(); m.likelihood.eval()
    with settings.prediction_cache("eager"), torch.no_grad():
        dist = m(Xs.to(DEV))
        c = m._prediction_cache()
        assert (c.hits, c.misses) == (0, 1) and c.ws is not None and c.ws.with_inverse
        again = m(Xs.to(DEV))
        assert (c.hits, c.misses) == (1, 1)
        obs = m.full_likelihood()(dist)
        lat = m.compute_latent_distrib(Xs.to(DEV), full_cov=True)
        dense = m.covar_module(Xd).evaluate()
    for d_ in (dist, again):
        assert torch.allclose(d_.mean.cpu(), mean_ref, rtol=1e-8, atol=1e-10)
        assert torch.allclose(d_.variance.cpu(), var_ref, rtol=1e-7, atol=1e-10)
    assert torch.allclose(again.mean, dist.mean, rtol=1e-10, atol=1e-12) and torch.allclose(again.variance, dist.variance, rtol=1e-9, atol=1e-12)
    assert torch.allclose(obs.variance.cpu(), var_ref + torch.diagonal(Lf @ Lf.T)[None, :], rtol=1e-7, atol=1e-10)
    assert torch.allclose(lat.mean.cpu(), mu_lat, rtol=1e-8, atol=1e-10)
    assert torch.allclose(lat.covariance_matrix.cpu(), cov_lat, rtol=1e-7, atol=1e-10)
    assert torch.allclose(dense.cpu(), _latent_K(kd, X, X, q), rtol=1e-10, atol=1e-12)               # evaluate()


def test_latent_shards_sum_to_the_unsharded_loss_and_gradients(plmc):
    """The shards of a latent-sharded projected model sum to the unsharded loss (1e-10) and gradients (rtol 1e-8): the table is sliced
    by latent_ids like ell is, its alpha column with it."""
    n, p, q, world, d = 130, 6, 3, 2, 2
    X, Y = _data(n, p, seed=21, d=d)
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
    """d = plmc_rq_max_dim() + 1, a null alpha and d = 0: refused on the host by every entry point through the library's argument error;
    nothing is launched (the output buffers keep their fill)."""
    hip = eng.hip
    L = hip.lib()
    Dx = L.cdll.plmc_rq_max_dim()
    n, q, f64 = 130, 1, torch.float64
    st = hip.stream_ptr(DEV)
    for d, null, word in ((Dx + 1, False, "plmc_rq_max_dim"), (2, True, "null pointer"), (0, False, "plmc_rq_max_dim")):
        dd = max(d, 1)
        X = torch.rand(n, dd, device=DEV, dtype=f64)
        z = torch.ones(q, dd, device=DEV, dtype=f64)
        al = None if null else hip.ptr(torch.ones(q, device=DEV, dtype=f64))
        o, nz = torch.ones(q, device=DEV, dtype=f64), torch.ones(q, device=DEV, dtype=f64)
        ws = eng.exact.Workspace(n, q, 0, f64, DEV, with_inverse=False)
        ws.A.fill_(-7.0)
        with pytest.raises(RuntimeError, match=word):
            L.call("plmc_assemble_rq", f64, hip.ptr(X), n, d, hip.ptr(z), al, hip.ptr(o), hip.ptr(nz), hip.ptr(ws.A), ws.lda, ws.strideA, q, st)
        out = torch.full((q, n, n), -7.0, device=DEV, dtype=f64)
        with pytest.raises(RuntimeError, match=word):
            L.call("plmc_assemble_cross_rq", f64, hip.ptr(X), n, hip.ptr(X), n, d, hip.ptr(z), al, hip.ptr(o), hip.ptr(out), n, n * n, 0, n, q, st)
        wi = eng.exact.Workspace(n, q, 1, f64, DEV, with_inverse=True)
        wi.A.fill_(-7.0)
        with pytest.raises(RuntimeError, match=word):
            L.call("plmc_factorize_rq_ex", f64, hip.ptr(X), n, d, hip.ptr(z), al, hip.ptr(o), hip.ptr(nz), hip.ptr(wi.A), wi.n_pad, wi.lda,
                   wi.naug, wi.strideA, hip.ptr(wi.Vd), hip.ptr(wi.logdet), hip.ptr(wi.info), 1, q, hip.ptr(nz), st)
        gt = torch.full((q, dd + 3), -7.0, device=DEV, dtype=f64)
        with pytest.raises(RuntimeError, match=word):
            L.call("plmc_kinv_grad_rq_vd", f64, hip.ptr(wi.W), wi.n_pad, wi.ldw, wi.strideW, hip.ptr(wi.alpha), hip.ptr(X), n, d, hip.ptr(z),
                   al, hip.ptr(o), hip.ptr(gt), None, 0, 0, None, hip.ptr(wi.partials), q, hip.ptr(nz), hip.ptr(wi.Vd), st)
        with pytest.raises(RuntimeError, match=word):
            L.call("plmc_loo_grad_rq", f64, hip.ptr(wi.W), wi.n_pad, wi.n_pad, wi.ldw, wi.strideW, hip.ptr(wi.alpha), hip.ptr(X), n, d,
                   hip.ptr(z), al, hip.ptr(o), hip.ptr(gt), hip.ptr(wi.partials), q, st)
        torch.cuda.synchronize()
        for buf in (ws.A, out, wi.A, gt):
            assert bool((buf == -7.0).all())
    X = torch.rand(n, Dx + 1, device=DEV, dtype=f64)
    table = torch.ones(q, Dx + 2, device=DEV, dtype=f64)
    with pytest.raises(ValueError, match="plmc_rq_max_dim"):
        eng.exact.exact_latent_log_prob(RQ, X, table, None, torch.ones(q, device=DEV, dtype=f64), torch.zeros(q, n, device=DEV, dtype=f64))
