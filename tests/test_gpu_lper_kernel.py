"""Locally periodic kernel (PeriodicKernel * RBFKernel) on the batched exact engine: the new entry points per element, the fp32 phase
reduction at large phase, the limits lam = +inf (the periodic kernel) and ell = +inf (the RBF kernel), the log-prob and every entry of
the gradient table of `ExactLatentLogProb` (fp64; fp32 on every arithmetic of the sweep, fused and two-call assembly), a sine that is
exactly zero, the leave-one-out objective, `ExactGPModel` (single and batched) and `ProjectedGPModel` (loss, gradients, eval mode, LOO,
prediction cache, latent sharding) and the argument errors.

Reference values: the dense fp64 formula of tests/_lper_dense.py (torch CPU, autograd).  Shapes and fp64 tolerances: those of
tests/test_gpu_periodic_kernel.py (named beside each use) -- n = 130 (two blocks of 128, ragged edge, 2 x 2 tiles) and n = 257 (3 x 3
tiles), d in {1, 3, 8} (the three compile-time capacities 1, 4, 8), q in {1, 3}.  The fp32 per-element bound is derived in DESIGN.md
("Locally periodic kernel: fp32 numerics"), not measured:
    |err| <= [24 d (1 + 1 / min_k ell_k) + (d + 8)] 2^-24 os   against the fp64 formula at the fp32-rounded inputs and parameters,
at small and at large phase alike."""
import math
import warnings

import pytest
import torch

import _lper_dense as ld
from oracle import gp_math as gm
from oracle import projected as pj
from _bridge import perturb_

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LP = "locally_periodic"
INF = float("inf")


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


def factory(**kw):
    import projectedlmc
    return projectedlmc.kernels.PeriodicKernel(**kw) * projectedlmc.kernels.RBFKernel(**kw)


def _problem(n, d, q, seed, ns=1):
    """The problem of tests/test_gpu_periodic_kernel.py with an RBF lengthscale of 0.4 .. 1.2 sqrt(d) beside it."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    X, Xs = r(n, d), r(ns, d)
    y = torch.randn(q, n, generator=g, dtype=torch.float64)
    ell = (0.6 + 1.4 * r(q, d)) * d
    period = 0.3 + 1.2 * r(q, d)
    os_ = 0.5 + r(q)
    noise = 0.05 + 0.5 * r(q)
    lam = (0.4 + 0.8 * r(q, d)) * math.sqrt(d)
    return X, Xs, y, ell, period, lam, os_, noise


def _table(f, ell, per, lam):
    return torch.stack([f(ell), f(per), f(lam)], 1)


def _assemble(eng, X, ell, period, lam, os_, noise, dt, entry="plmc_assemble_lper"):
    """plmc_assemble_lper_* (or the periodic / plain form it is compared with): the upper triangle of Khat, (q, n, n) fp64 on the host."""
    hip = eng.hip
    L = hip.lib()
    f = lambda t: t.to(DEV, dt).contiguous()
    n, d = X.shape
    q = os_.shape[0]
    ws = eng.exact.Workspace(n, q, 0, dt, DEV, with_inverse=False)
    ws.A.zero_()
    Xd, o_, nz = f(X), f(os_), f(noise)
    tail = (hip.ptr(o_), hip.ptr(nz), hip.ptr(ws.A), ws.lda, ws.strideA, q, hip.stream_ptr(DEV))
    if entry == "plmc_assemble_lper":
        l_, p_, r_ = f(ell), f(period), f(lam)
        L.call(entry, dt, hip.ptr(Xd), n, d, hip.ptr(l_), hip.ptr(p_), hip.ptr(r_), *tail)
    elif entry == "plmc_assemble_per":
        l_, p_ = f(ell), f(period)
        L.call(entry, dt, hip.ptr(Xd), n, d, hip.ptr(l_), hip.ptr(p_), *tail)
    else:
        r_ = f(lam)
        L.call("plmc_assemble", dt, hip.KIND["rbf"], hip.ptr(Xd), n, d, hip.ptr(r_), *tail)
    torch.cuda.synchronize()
    return torch.triu(ws.A[:, :n, :n].cpu().double())


def _cross(eng, X, Xs, ell, period, lam, os_, dt):
    f = lambda t: t.to(DEV, dt).contiguous()
    K = eng.exact.dense_cross(LP, f(X), f(Xs), _table(f, ell, period, lam), f(os_))
    torch.cuda.synchronize()
    return K.cpu().double()


# ------------------------------------------------------------------------------------------------ 1. per element
@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n,d,q", [(130, 1, 1), (257, 3, 3), (257, 8, 3), (130, 8, 1), (257, 1, 3)])
def test_assembly_and_cross_against_the_dense_formula(eng, n, d, q, dt):
    """plmc_assemble_lper / plmc_assemble_cross_lper; shapes and the fp64 tolerance of the test of the same name in
    tests/test_gpu_periodic_kernel.py.  fp64: |err| <= 1e-12 (|ref| + os).  fp32: the bound of the module docstring, diagonal
    (os + noise) included."""
    assert d <= eng.hip.lib().cdll.plmc_lper_max_dim()
    ns = 70
    X, Xs, _, ell, per, lam, os_, nz = _problem(n, d, q, seed=10 * d + n, ns=ns)
    if dt == torch.float32:
        X, Xs, ell, per, lam, os_, nz = (t.float().double() for t in (X, Xs, ell, per, lam, os_, nz))
    ref = torch.triu(ld.lper_kernel(X, X, ell, per, lam, os_) + nz[:, None, None] * torch.eye(n, dtype=torch.float64))
    refx = ld.lper_kernel(X, Xs, ell, per, lam, os_)
    got, gotx = _assemble(eng, X, ell, per, lam, os_, nz, dt), _cross(eng, X, Xs, ell, per, lam, os_, dt)
    scale = os_[:, None, None]
    for name, a, b in (("assemble", got, ref), ("cross", gotx, refx)):
        err = (a - b).abs()
        if dt == torch.float64:
            print("%s f64 n=%d d=%d q=%d: max err / (|ref| + os) %.3g" % (name, n, d, q, float((err / (b.abs() + scale)).max())))
            assert bool((err <= 1e-12 * (b.abs() + scale)).all()), name
        else:
            bound = ld.fp32_bound(d, ell, os_)
            print("%s f32 n=%d d=%d q=%d: max err / bound %.3g" % (name, n, d, q, float((err / bound).max())))
            assert bool((err <= bound).all()), name
    assert bool((torch.diagonal(got, dim1=-2, dim2=-1) == (os_.to(dt) + nz.to(dt)).double()[:, None]).all())      # k(x, x) = os exactly


# ------------------------------------------------------------------------------------------------ 2. large phase
def large_phase_inputs():
    """large_phase_inputs() of tests/test_gpu_periodic_kernel.py -- n = 257 near-uniform points in [0, 1], period 5e-4 (tau / p reaches
    ~2000 revolutions), ell = 1, os = 1.3 -- with lam = 1.0.  fp32-rounded, as fp64."""
    n = 257
    g = torch.Generator().manual_seed(0)
    X = ((torch.arange(n, dtype=torch.float64) + 0.3 * torch.rand(n, generator=g, dtype=torch.float64)) / n).reshape(n, 1)
    X[0, 0], X[-1, 0] = 0.0, 1.0
    ell = torch.tensor([[1.0]], dtype=torch.float64)
    per = torch.tensor([[5.0e-4]], dtype=torch.float64)
    lam = torch.tensor([[1.0]], dtype=torch.float64)
    os_ = torch.tensor([1.3], dtype=torch.float64)
    return tuple(t.float().double() for t in (X, ell, per, lam, os_))


def test_large_phase_fp32_assembly_meets_the_bound_and_the_naive_form_does_not(eng):
    X, ell, per, lam, os_ = large_phase_inputs()
    n = X.shape[0]
    nz = torch.tensor([0.1], dtype=torch.float64).float().double()
    ref = ld.lper_kernel(X, X, ell, per, lam, os_)
    bound = float(ld.fp32_bound(1, ell, os_))
    e_naive = float((ld.naive_fp32(X, X, ell, per, lam, os_).double() - ref[0]).abs().max())
    got = _assemble(eng, X, ell, per, lam, os_, nz, torch.float32)
    e = float((got[0] - torch.triu(ref[0] + nz[0] * torch.eye(n, dtype=torch.float64))).abs().max())
    Xs = (X[:50] + 0.25).float().double()
    ex = float((_cross(eng, X, Xs, ell, per, lam, os_, torch.float32) - ld.lper_kernel(X, Xs, ell, per, lam, os_)).abs().max())
    print("largest phase %.4g revolutions; bound %.3g; assembly err / bound %.3g; cross err / bound %.3g; naive fp32 err %.3g"
          % (float((X.max() - X.min()) / per[0, 0]), bound, e / bound, ex / bound, e_naive))
    assert float((X.max() - X.min()) / per[0, 0]) > 1990
    assert e_naive > bound, (e_naive, bound)
    assert e <= bound, (e, bound)
    assert ex <= bound, (ex, bound)


# ------------------------------------------------------------------------------------------------ log-prob and the gradient table
def _reference_logprob(X, y, ell, per, lam, os_, nz, fn=ld.lper_logprob):
    leaves = [t.clone().requires_grad_() for t in (ell, per, lam, os_, nz, y)]
    lp = fn(X, leaves[5], leaves[0], leaves[1], leaves[2], leaves[3], leaves[4])
    g = torch.Generator().manual_seed(99)
    wt = 0.5 + torch.rand(lp.shape, generator=g, dtype=torch.float64)
    (lp * wt).sum().backward()
    grads = [torch.zeros_like(t) if t.grad is None else torch.nan_to_num(t.grad, nan=0.0) for t in leaves]
    return [lp.detach()] + grads + [wt]


def _run_logprob(eng, X, y, ell, per, lam, os_, nz, dt, wt, fn=None):
    f = lambda t: t.to(DEV, dt)
    table = _table(f, ell, per, lam).requires_grad_()
    leaves = [f(t).requires_grad_() for t in (os_, nz, y)]
    fn = eng.exact.exact_latent_log_prob if fn is None else fn
    lp = fn(LP, f(X), table, leaves[0], leaves[1], leaves[2])
    (lp * f(wt)).sum().backward()
    torch.cuda.synchronize()
    tg = table.grad.cpu().double()
    return [lp.detach().cpu().double(), tg[:, 0], tg[:, 1], tg[:, 2]] + [t.grad.cpu().double() for t in leaves]


GRAD_NAMES = ("lengthscale", "period", "rbf lengthscale", "oscale", "noise", "y")


# ------------------------------------------------------------------------------------------------ 3. limits against pinned kernels
def test_limits_are_the_periodic_and_the_rbf_kernel(eng):
    """fp64, n = 130, d = 3.  1 / lam = 0 (lam = +inf through the C ABI): plmc_assemble_per_f64 to rtol 1e-14.  ell = +inf:
    plmc_assemble_f64 of kind rbf with lengthscales lam to rtol 1e-13.  The gradient entries of the absent factor are EXACTLY 0 (the
    header says so): the tile sums stay finite and the reduction divides them by +inf."""
    n, d, q = 130, 3, 3
    X, _, y, ell, per, lam, os_, nz = _problem(n, d, q, seed=31)
    inf = torch.full_like(lam, INF)
    K_per = _assemble(eng, X, ell, per, None, os_, nz, torch.float64, entry="plmc_assemble_per")
    K_lim = _assemble(eng, X, ell, per, inf, os_, nz, torch.float64)
    print("lam = inf against plmc_assemble_per_f64: max rel err %.3g" % float(((K_lim - K_per).abs() / K_per.abs().clamp_min(1e-300)).max()))
    assert torch.allclose(K_lim, K_per, rtol=1e-14, atol=0)
    K_rbf = _assemble(eng, X, None, None, lam, os_, nz, torch.float64, entry="plmc_assemble")
    K_lim = _assemble(eng, X, inf, per, lam, os_, nz, torch.float64)
    print("ell = inf against plmc_assemble_f64 (rbf): max rel err %.3g" % float(((K_lim - K_rbf).abs() / K_rbf.abs().clamp_min(1e-300)).max()))
    assert torch.allclose(K_lim, K_rbf, rtol=1e-13, atol=0)
    # gradients: the absent factor's entries are exactly 0, the present factor's equal dense autograd
    for tag, e_, r_, zero in (("lam = inf", ell, inf, (3,)), ("ell = inf", inf, lam, (1, 2))):
        ref = _reference_logprob(X, y, e_, per, r_, os_, nz)
        got = _run_logprob(eng, X, y, e_, per, r_, os_, nz, torch.float64, ref[7])
        assert torch.allclose(got[0], ref[0], rtol=1e-10, atol=0), tag
        for i, (name, a, b) in enumerate(zip(GRAD_NAMES, got[1:], ref[1:7]), start=1):
            assert bool(torch.isfinite(a).all()), (tag, name)
            if i in zero:
                assert bool((a == 0).all()), (tag, name, a)
            else:
                assert torch.allclose(a, b, rtol=1e-7, atol=1e-9), (tag, name, float((a - b).abs().max()))


# ------------------------------------------------------------------------------------------------ 4. log-prob and every gradient, fp64
@pytest.mark.parametrize("n,d,q", [(257, 1, 3), (130, 3, 1), (257, 8, 3)])
def test_logprob_and_every_gradient_fp64(eng, n, d, q):
    """Shapes and tolerances of the test of the same name in tests/test_gpu_periodic_kernel.py: log-prob rtol 1e-10; gradients rtol 1e-7 /
    atol 1e-9."""
    X, _, y, ell, per, lam, os_, nz = _problem(n, d, q, seed=n + d)
    ref = _reference_logprob(X, y, ell, per, lam, os_, nz)
    got = _run_logprob(eng, X, y, ell, per, lam, os_, nz, torch.float64, ref[7])
    assert torch.allclose(got[0], ref[0], rtol=1e-10, atol=0), (got[0], ref[0])
    for name, a, b in zip(GRAD_NAMES, got[1:], ref[1:7]):
        assert a.shape == b.shape, name
        print("d/d %s: max abs err %.3g" % (name, float((a - b).abs().max())))
        assert torch.allclose(a, b, rtol=1e-7, atol=1e-9), (name, float((a - b).abs().max()))


def test_logprob_without_an_output_scale_fp64(eng):
    """oscale = None (a bare product): unit output scale, no gradient for it (tests/test_gpu_periodic_kernel.py, the same name)."""
    n, d, q = 130, 3, 3
    X, _, y, ell, per, lam, _, nz = _problem(n, d, q, seed=8)
    one = torch.ones(q, dtype=torch.float64)
    ref = _reference_logprob(X, y, ell, per, lam, one, nz)
    f = lambda t: t.to(DEV)
    table = _table(f, ell, per, lam).requires_grad_()
    nzd = f(nz).requires_grad_()
    lp = eng.exact.exact_latent_log_prob(LP, f(X), table, None, nzd, f(y))
    (lp * f(ref[7])).sum().backward()
    assert torch.allclose(lp.detach().cpu(), ref[0], rtol=1e-10, atol=0)
    for i in range(3):
        assert torch.allclose(table.grad.cpu()[:, i], ref[1 + i], rtol=1e-7, atol=1e-9), GRAD_NAMES[i]
    assert torch.allclose(nzd.grad.cpu(), ref[5], rtol=1e-7, atol=1e-9)


# ------------------------------------------------------------------------------------------------ 5. fp32 on every arithmetic
def _factor_buffer(eng, X, ell, per, lam, os_, nz, y, fused, monkeypatch):
    """The factor buffer of one fp32 factorisation with the inverse factor, zeroed first."""
    f = lambda t: t.to(DEV, torch.float32).contiguous()
    n, q = X.shape[0], ell.shape[0]
    ws = eng.exact.Workspace(n, q, 1, torch.float32, DEV, with_inverse=True)
    ws.A.zero_()
    ws.Vd.zero_()
    if not fused:
        monkeypatch.setenv("PLMC_FUSED_ASSEMBLE", "0")
    eng.exact.factorize(LP, f(X), _table(f, ell, per, lam), f(os_), f(nz), f(y).reshape(q, 1, n), ws)
    if not fused:
        monkeypatch.delenv("PLMC_FUSED_ASSEMBLE")
    torch.cuda.synchronize()
    return ws.A.cpu(), ws.logdet.cpu()


@pytest.mark.parametrize("d", [1, 3])
def test_logprob_fp32_on_every_arithmetic_and_fused_against_two_call_assembly(eng, monkeypatch, d):
    """n = 257, q = 3, fp32 with PLMC_SPLIT unset, 0 and 3; the tolerances of the test of the same name in
    tests/test_gpu_periodic_kernel.py: value 1e-4 relative, gradients 2e-3 of the largest entry.  The fused plmc_factorize_lper_ex and
    PLMC_FUSED_ASSEMBLE=0 (plmc_assemble_lper + plmc_potrf_ex) give the same factor buffer, log-determinant, value and gradients as bit
    patterns.  d = 1 runs the gradient kernel on the arithmetic the knob names; with d > 1 it forms K^-1 with the fp32 matrix instructions
    whatever the knob says (include/plmc.h)."""
    n, q = 257, 3
    X, _, y, ell, per, lam, os_, nz = (t.float().double() for t in _problem(n, d, q, seed=77 + d))
    ref = _reference_logprob(X, y, ell, per, lam, os_, nz)
    monkeypatch.delenv("PLMC_SPLIT", raising=False)                     # "unset" means unset, whatever the caller's environment
    monkeypatch.delenv("PLMC_FUSED_ASSEMBLE", raising=False)
    eng.hip.lib().cdll.plmc_dev_reload_knobs()

    def check(tag):
        got = _run_logprob(eng, X, y, ell, per, lam, os_, nz, torch.float32, ref[7])
        monkeypatch.setenv("PLMC_FUSED_ASSEMBLE", "0")
        two = _run_logprob(eng, X, y, ell, per, lam, os_, nz, torch.float32, ref[7])
        monkeypatch.delenv("PLMC_FUSED_ASSEMBLE")
        for a, b in zip(got, two):
            assert torch.equal(a, b), tag
        A1, ld1 = _factor_buffer(eng, X, ell, per, lam, os_, nz, y, True, monkeypatch)
        A2, ld2 = _factor_buffer(eng, X, ell, per, lam, os_, nz, y, False, monkeypatch)
        assert torch.equal(A1, A2) and torch.equal(ld1, ld2), tag
        e = float(((got[0] - ref[0]) / ref[0]).abs().max())
        print("PLMC_SPLIT %s: log-prob rel err %.3g" % (tag, e))
        assert e < 1e-4, (tag, e)
        for name, a, b in zip(GRAD_NAMES, got[1:], ref[1:7]):
            e = float((a - b).abs().max() / b.abs().max())
            print("PLMC_SPLIT %s: d/d %s err %.3g of the largest" % (tag, name, e))
            assert e < 2e-3, (tag, name, e)

    check("unset")
    for split in ("0", "3"):
        with eng.hip.knob("PLMC_SPLIT", split):
            check(split)


# ------------------------------------------------------------------------------------------------ 6. a sine that is exactly 0
def test_a_sine_that_is_exactly_zero(eng):
    """Inputs on a grid of quarters and periods 0.25 and 0.5 (tests/test_gpu_periodic_kernel.py, the same name): tau is an integer
    multiple of p for every pair (p = 0.25) or every other one (p = 0.5), so sin(pi tau / p) is exactly 0 there and the covariance is the
    RBF factor alone.  All values and gradients finite and equal to dense autograd."""
    q, d = 2, 2
    g = torch.Generator().manual_seed(5)
    X = torch.unique(torch.randint(0, 8, (150, d), generator=g).double() / 4.0, dim=0)
    n = X.shape[0]
    y = torch.randn(q, n, generator=g, dtype=torch.float64)
    ell = 0.7 + torch.rand(q, d, generator=g, dtype=torch.float64)
    per = torch.tensor([[0.25, 0.5], [0.5, 1.0]], dtype=torch.float64)
    lam = torch.tensor([[1.5, 0.9], [0.8, 2.0]], dtype=torch.float64)
    os_ = torch.tensor([0.8, 1.4], dtype=torch.float64)
    nz = torch.tensor([0.3, 0.5], dtype=torch.float64)
    ref = _reference_logprob(X, y, ell, per, lam, os_, nz)
    got = _run_logprob(eng, X, y, ell, per, lam, os_, nz, torch.float64, ref[7])
    K = _assemble(eng, X, ell, per, lam, os_, nz, torch.float64)
    tau = X[:, None, :] - X[None, :, :]
    whole = ((tau[..., 0] / 0.25) % 1 == 0) & ((tau[..., 1] / 0.5) % 1 == 0) & torch.triu(torch.ones(n, n, dtype=torch.bool), 1)
    rbf = os_[0] * torch.exp(-0.5 * ((tau / lam[0]) ** 2).sum(-1))
    assert bool(whole.any()) and torch.allclose(K[0][whole], rbf[whole], rtol=1e-14, atol=0)
    for name, a, b in zip(("logp",) + GRAD_NAMES, got, ref[:7]):
        assert bool(torch.isfinite(a).all()), name
        assert torch.allclose(a, b, rtol=1e-7, atol=1e-9), (name, float((a - b).abs().max()))
    got32 = _run_logprob(eng, X, y, ell, per, lam, os_, nz, torch.float32, ref[7])
    assert all(bool(torch.isfinite(a).all()) for a in got32)
    for name, a, b in zip(GRAD_NAMES, got32[1:], ref[1:7]):
        assert float((a - b).abs().max() / b.abs().max()) < 2e-3, name


# ------------------------------------------------------------------------------------------------ 7. leave-one-out
@pytest.mark.parametrize("d,q", [(1, 1), (3, 3)])
def test_exact_loo_value_and_every_gradient_fp64(eng, d, q):
    """n = 130, fp64; the tolerances of tests/test_gpu_loo_objective.py: value to 1e-10 relative, every gradient group and dL/dy to 1e-8
    of the group's largest magnitude; exact_loo's moments 1 / diag(Khat^-1) and Khat^-1 y / diag(Khat^-1) to 1e-8 relative."""
    n = 130
    X, _, y, ell, per, lam, os_, nz = _problem(n, d, q, seed=50 + d)
    ref = _reference_logprob(X, y, ell, per, lam, os_, nz, fn=ld.lper_loo)
    got = _run_logprob(eng, X, y, ell, per, lam, os_, nz, torch.float64, ref[7], fn=eng.exact.exact_loo_log_prob)
    rel = float(((got[0] - ref[0]) / ref[0]).abs().max())
    print("LOO d=%d q=%d: value %.2e" % (d, q, rel))
    assert rel <= 1e-10, rel
    for name, a, b in zip(GRAD_NAMES, got[1:], ref[1:7]):
        assert a.shape == b.shape, name
        scale, err = float(b.abs().max()), float((a - b).abs().max())
        print("    %s: %.2e of %.3e" % (name, err / scale, scale))
        assert err <= 1e-8 * scale, (name, err, scale)
    f = lambda t: t.to(DEV)
    with torch.no_grad():
        s2, r = eng.exact.exact_loo(LP, f(X), _table(f, ell, per, lam), f(os_), f(nz), f(y))
    Kinv = torch.linalg.inv(ld.khat(X, ell, per, lam, os_, nz))
    dg = torch.diagonal(Kinv, dim1=-2, dim2=-1)
    assert torch.allclose(s2.cpu(), 1.0 / dg, rtol=1e-8, atol=0)
    assert torch.allclose(r.cpu(), (Kinv @ y.unsqueeze(-1)).squeeze(-1) / dg, rtol=1e-8, atol=1e-12)


def _tables(raw, pre, q):
    """(ell, period, lam) (q, d) from a dict of raw parameters under the gpytorch names `pre`kernels.0.raw_lengthscale /
    kernels.0.raw_period_length / kernels.1.raw_lengthscale (the product of `factory`: the periodic factor first)."""
    sp = torch.nn.functional.softplus
    return (sp(raw[pre + "kernels.0.raw_lengthscale"]).reshape(q, -1), sp(raw[pre + "kernels.0.raw_period_length"]).reshape(q, -1),
            sp(raw[pre + "kernels.1.raw_lengthscale"]).reshape(q, -1))


def _dense_model_loss(model, X, Y, q, fn=ld.lper_logprob):
    """-(1 / n) sum over latents of log N(y_i - c_i; 0, K_i + noise_i I) (or of the LOO density, fn=ld.lper_loo) with autograd through
    the raw parameters (host copies)."""
    sp = torch.nn.functional.softplus
    raw = {k: v.detach().cpu().double().requires_grad_() for k, v in model.named_parameters()}
    scaled = hasattr(model.covar_module, "base_kernel")
    ell, per, lam = _tables(raw, "covar_module.base_kernel." if scaled else "covar_module.", q)
    os_ = sp(raw["covar_module.raw_outputscale"]).reshape(q) if scaled else None
    lik = model.likelihood
    noise = lik.noise_covar.raw_noise_constraint.transform(raw["likelihood.noise_covar.raw_noise"]).reshape(-1).expand(q)
    c = raw["mean_module.raw_constant"].reshape(q, 1) if "mean_module.raw_constant" in raw else raw["mean_module.constant"].reshape(q, 1)
    y = (Y.reshape(X.shape[0], -1).T if Y.dim() > 1 else Y.reshape(1, -1)) - c
    lp = fn(X, y, ell, per, lam, os_, noise)
    return -(lp.sum() / X.shape[0]), raw, (ell, per, lam, os_, noise, c)


def _tidal(n, p, seed, d=1):
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(n, d, generator=g, dtype=torch.float64)
    X[:, 0] = torch.sort(X[:, 0])[0]
    Y = torch.stack([torch.sin(2 * math.pi * (1 + k) * X[:, 0]) + 0.3 * torch.randn(n, generator=g, dtype=torch.float64) for k in range(p)], 1)
    return X, Y


@pytest.mark.parametrize("d", [1, 3])
def test_leave_one_out_pseudo_likelihood_on_the_exact_model(plmc, d):
    """LeaveOneOutPseudoLikelihood on ExactGPModel(ScaleKernel(Periodic * RBF)), n = 130, fp64; the tolerances of the model tests of
    tests/test_gpu_loo_objective.py: value 1e-9 relative, every raw-parameter gradient rtol 1e-5 / atol 1e-9."""
    n = 130
    X, Y = _tidal(n, 1, seed=11 + d, d=d)
    y = Y[:, 0]
    torch.manual_seed(3)
    lik = plmc.GaussianLikelihood()
    m = perturb_(plmc.ExactGPModel(X, y, lik, kernel_type=factory, outputscales=True).double())
    neg, raw, _ = _dense_model_loss(m, X, y, 1, fn=ld.lper_loo)
    ref = -neg
    ref.backward()
    m = m.to(DEV)
    m.train(); m.likelihood.train()
    out = plmc.LeaveOneOutPseudoLikelihood(m.likelihood, m, X, y)(m(X.to(DEV)), y.to(DEV))
    out.sum().backward()
    got, want = float(out.detach().sum()), float(ref.detach())
    assert abs(got - want) <= 1e-9 * abs(want), (got, want)
    for name, prm in m.named_parameters():
        a, b = prm.grad.cpu().double(), raw[name].grad.reshape(prm.shape)
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-9), (name, float((a - b).abs().max()))


# ------------------------------------------------------------------------------------------------ 8. models
def test_single_output_exact_model(plmc):
    """ExactGPModel, ScaleKernel(PeriodicKernel * RBFKernel), d = 1, fp64; body and tolerances of the test of the same name in
    tests/test_gpu_periodic_kernel.py: loss within 1e-9 relative of dense, every parameter gradient rtol 1e-5 / atol 1e-9, eval-mode mean
    rtol 1e-7, variance rtol 1e-6, compute_loo 1e-8 / 1e-7."""
    n, ns = 257, 40
    X, Y = _tidal(n, 1, seed=1)
    y = Y[:, 0]
    torch.manual_seed(4)
    m = perturb_(plmc.ExactGPModel(X, y, plmc.GaussianLikelihood(), kernel_type=factory, outputscales=True).double())
    os_host = m.outputscale()                                  # works through the ScaleKernel around the product
    m = m.to(DEV)
    m.train(); m.likelihood.train()
    mll = plmc.ExactMarginalLogLikelihood(m.likelihood, m)
    loss = -mll(m(X.to(DEV)), y.to(DEV))
    loss.backward()
    ref, raw, (ell, per, lam, os_, noise, c) = _dense_model_loss(m, X, y, 1)
    ref.backward()
    assert abs(float(loss) - float(ref)) < 1e-9 * abs(float(ref)), (float(loss), float(ref))
    names = [nm for nm, _ in m.named_parameters()]
    for nm in ("kernels.0.raw_period_length", "kernels.0.raw_lengthscale", "kernels.1.raw_lengthscale"):
        assert "covar_module.base_kernel." + nm in names
    for name, prm in m.named_parameters():
        a, b = prm.grad.cpu().double(), raw[name].grad
        assert torch.allclose(a, b.reshape(a.shape), rtol=1e-5, atol=1e-9), (name, float((a - b.reshape(a.shape)).abs().max()))
    assert os_host.numel() == 1 and torch.allclose(os_host.reshape(-1).double(), os_.detach().reshape(-1))
    Xs = torch.rand(ns, 1, dtype=torch.float64)
    m.eval(); m.likelihood.eval()
    with torch.no_grad():
        post = m(Xs.to(DEV))
        s2, r = m.compute_loo()
    dt_ = lambda t: t.detach()
    args = (dt_(ell), dt_(per), dt_(lam), dt_(os_))
    mean_ref, cov_ref = ld.lper_posterior(X, (y - dt_(c)[0]).reshape(1, n), Xs, *args, dt_(noise))
    assert torch.allclose(post.mean.cpu(), mean_ref[0] + dt_(c)[0], rtol=1e-7, atol=1e-9)
    assert torch.allclose(post.variance.cpu(), torch.diagonal(cov_ref[0]), rtol=1e-6, atol=1e-9)
    Kinv = torch.linalg.inv(ld.lper_kernel(X, X, *args)[0] + dt_(noise)[0] * torch.eye(n, dtype=torch.float64))
    dg = torch.diagonal(Kinv)
    assert torch.allclose(s2.cpu().reshape(-1), 1.0 / dg, rtol=1e-8)
    assert torch.allclose(r.cpu().reshape(-1), (Kinv @ (y - dt_(c)[0, 0])) / dg, rtol=1e-7, atol=1e-10)


def test_batched_exact_model_latent_moments_against_dense(plmc):
    """n_tasks = 3 batched ExactGPModel on d = 3 inputs, fp64: loss and every parameter gradient against dense autograd, eval-mode mean /
    variance and compute_loo against dense conditioning; body and tolerances of the test of the same name in
    tests/test_gpu_periodic_kernel.py."""
    n, q, ns, d = 200, 3, 30, 3
    X, Y = _tidal(n, q, seed=2, d=d)
    torch.manual_seed(6)
    m = plmc.ExactGPModel(X, Y, plmc.GaussianLikelihood(batch_shape=torch.Size([q])), n_tasks=q, kernel_type=factory).double()
    perturb_(m)
    m = m.to(DEV)
    m.train(); m.likelihood.train()
    loss = -plmc.ExactMarginalLogLikelihood(m.likelihood, m)(m(X.to(DEV)), Y.T.contiguous().to(DEV)).sum()
    loss.backward()
    ref, raw, (ell, per, lam, os_, noise, _) = _dense_model_loss(m, X, Y, q)
    ref.backward()
    assert abs(float(loss) - float(ref)) < 1e-9 * abs(float(ref)), (float(loss), float(ref))
    for name, prm in m.named_parameters():
        a, b = prm.grad.cpu().double(), raw[name].grad.reshape(prm.shape)
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-9), (name, float((a - b).abs().max()))
    ell, per, lam, noise = ell.detach(), per.detach(), lam.detach(), noise.detach()
    os_ = None if os_ is None else os_.detach()
    c = m.mean_module(X.to(DEV)).detach().cpu().double().reshape(q, n)
    Xs = torch.rand(ns, d, dtype=torch.float64)
    cs = m.mean_module(Xs.to(DEV)).detach().cpu().double().reshape(q, ns)
    m.eval(); m.likelihood.eval()
    with torch.no_grad():
        post = m(Xs.to(DEV))
        s2, r = m.compute_loo()
    mean_ref, cov_ref = ld.lper_posterior(X, Y.T - c, Xs, ell, per, lam, os_, noise)
    assert torch.allclose(post.mean.cpu().reshape(q, ns), mean_ref + cs, rtol=1e-7, atol=1e-9)
    assert torch.allclose(post.variance.cpu().reshape(q, ns), torch.diagonal(cov_ref, dim1=-2, dim2=-1), rtol=1e-6, atol=1e-9)
    Kinv = torch.linalg.inv(ld.lper_kernel(X, X, ell, per, lam, os_) + noise[:, None, None] * torch.eye(n, dtype=torch.float64))
    dg = torch.diagonal(Kinv, dim1=-2, dim2=-1)
    assert torch.allclose(s2.cpu().T, 1.0 / dg, rtol=1e-8) and torch.allclose(r.cpu().T, (Kinv @ (Y.T - c).unsqueeze(-1)).squeeze(-1) / dg, rtol=1e-7, atol=1e-10)


def _projected(plmc, X, Y, q, seed=5, **kw):
    torch.manual_seed(seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return plmc.ProjectedGPModel(X, Y, Y.shape[1], q, mean_type=plmc.ZeroMean, kernel_type=factory, init_lmc_coeffs=True, **kw)


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
    return ld.lper_kernel(Xa, Xb, *_tables(kern, "covar_module.", q))


@pytest.mark.parametrize("bulk", [True, False])
def test_projected_model_loss_gradients_and_eval_mode_against_dense(plmc, bulk):
    """fp64, p = 5, q = 3, d = 1, perturbed parameters; body and tolerances of the test of the same name in
    tests/test_gpu_periodic_kernel.py.  ProjectedLMCmll and the gradient of every parameter against sum_i log N(ytil_i; 0, K_i + noise_i
    I) / n + the oracle's projection terms (1e-9 relative; rtol 2e-6, atol 1e-8); eval mode (task mean / variance, observation variance,
    latent mean and full covariance) against dense conditioning (rtol 1e-8 / 1e-7); compute_loo against 1 / diag(K^-1) and K^-1 y /
    diag(K^-1) (1e-8).  The second eval call hits the prediction cache."""
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
    assert checked == len(names) + 3                        # + the three rows of the locally periodic table

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
    """The shards of a latent-sharded projected model sum to the unsharded loss (1e-10) and gradients (rtol 1e-8): the table (q, 3, d) is
    sliced by latent_ids like ell is (tests/test_gpu_periodic_kernel.py, the same name)."""
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


# ------------------------------------------------------------------------------------------------ 9. limits
def test_limits_are_argument_errors(eng):
    """d = 9 and a null `period` or `rbf_ell`: refused on the host by every new entry point with the library's error, nothing is
    launched."""
    hip = eng.hip
    L = hip.lib()
    Dx = L.cdll.plmc_lper_max_dim()
    assert Dx == 8
    n, q, f64 = 130, 1, torch.float64
    st = hip.stream_ptr(DEV)
    for d, null, word in ((Dx + 1, None, "plmc_lper_max_dim"), (2, "period", "null pointer"), (2, "rbf_ell", "null pointer")):
        X = torch.rand(n, d, device=DEV, dtype=f64)
        z = torch.ones(q, d, device=DEV, dtype=f64)
        per = None if null == "period" else hip.ptr(z)
        lam = None if null == "rbf_ell" else hip.ptr(z)
        o, nz = torch.ones(q, device=DEV, dtype=f64), torch.ones(q, device=DEV, dtype=f64)
        ws = eng.exact.Workspace(n, q, 0, f64, DEV, with_inverse=False)
        with pytest.raises(RuntimeError, match=word):
            L.call("plmc_assemble_lper", f64, hip.ptr(X), n, d, hip.ptr(z), per, lam, hip.ptr(o), hip.ptr(nz), hip.ptr(ws.A), ws.lda, ws.strideA,
                   q, st)
        out = torch.empty(q, n, n, device=DEV, dtype=f64)
        with pytest.raises(RuntimeError, match=word):
            L.call("plmc_assemble_cross_lper", f64, hip.ptr(X), n, hip.ptr(X), n, d, hip.ptr(z), per, lam, hip.ptr(o), hip.ptr(out), n, n * n, 0,
                   n, q, st)
        wi = eng.exact.Workspace(n, q, 1, f64, DEV, with_inverse=True, per=LP)
        with pytest.raises(RuntimeError, match=word):
            L.call("plmc_factorize_lper_ex", f64, hip.ptr(X), n, d, hip.ptr(z), per, lam, hip.ptr(o), hip.ptr(nz), hip.ptr(wi.A), wi.n_pad, wi.lda,
                   wi.naug, wi.strideA, hip.ptr(wi.Vd), hip.ptr(wi.logdet), hip.ptr(wi.info), 1, q, hip.ptr(nz), st)
        gt = torch.empty(q, 3 * d + 2, device=DEV, dtype=f64)
        with pytest.raises(RuntimeError, match=word):
            L.call("plmc_kinv_grad_lper_vd", f64, hip.ptr(wi.W), wi.n_pad, wi.ldw, wi.strideW, hip.ptr(wi.alpha), hip.ptr(X), n, d, hip.ptr(z),
                   per, lam, hip.ptr(o), hip.ptr(gt), None, 0, 0, None, hip.ptr(wi.partials), q, hip.ptr(nz), hip.ptr(wi.Vd), st)
        Xop = torch.zeros(q, wi.n_pad + wi.NB, wi.n_pad, device=DEV, dtype=f64)
        beta = torch.zeros(q, wi.n_pad, device=DEV, dtype=f64)
        with pytest.raises(RuntimeError, match=word):
            L.call("plmc_loo_grad_lper", f64, hip.ptr(Xop), wi.n_pad, wi.n_pad + 16, wi.n_pad, Xop.shape[1] * wi.n_pad, hip.ptr(beta), hip.ptr(X),
                   n, d, hip.ptr(z), per, lam, hip.ptr(o), hip.ptr(gt), hip.ptr(wi.partials), q, st)
    X = torch.rand(n, Dx + 1, device=DEV, dtype=f64)
    table = torch.ones(q, 3, Dx + 1, device=DEV, dtype=f64)
    with pytest.raises(ValueError, match="plmc_lper_max_dim"):
        eng.exact.exact_latent_log_prob(LP, X, table, None, torch.ones(q, device=DEV, dtype=f64), torch.zeros(q, n, device=DEV, dtype=f64))
    with pytest.raises(ValueError, match=r"\(q, 3, d\)"):
        eng.exact.exact_latent_log_prob(LP, X[:, :2].contiguous(), torch.ones(q, 2, 2, device=DEV, dtype=f64), None,
                                        torch.ones(q, device=DEV, dtype=f64), torch.zeros(q, n, device=DEV, dtype=f64))
