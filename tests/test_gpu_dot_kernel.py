"""Dot-product kernels (LinearKernel, PolynomialKernel) on the batched exact engine: the new entry points per element, the log-prob and
every entry of the gradient table of `ExactLatentLogProb` (fp64; fp32 on every arithmetic of the sweep, fused and two-call assembly),
`ExactGPModel` (train, eval, full_cov, the prediction cache, two powers in one process), `ProjectedGPModel` + `ProjectedLMCmll`,
`LeaveOneOutPseudoLikelihood`, draws with and without noise, a few optimiser steps, and the argument errors.

Reference values: the dense fp64 formula of tests/_dot_dense.py (torch CPU, autograd).  Inputs are uniform in [-1, 1]^d, so products
change sign; every case with n >= 3 has one all-zero row and one duplicated row; noise is 0.1 - 0.5.  Sizes: n in {1, 127, 128, 129, 257}
for the element-wise checks (the tile is 128), n in {65, 129, 257} for the gradients; d in {1, 4, 5, 8, 9, 16}: both sides of every
compile-time capacity (1, 4, 8, 16); P in {1, 2, 3, plmc_dot_max_power()}.
Tolerances: those of tests/test_gpu_rq_kernel.py (named beside each use); the fp32 per-element bound is the operation count of
DESIGN.md 7.9, not measured:
    |err| <= P (d + 3) 2^-24 os S^P,  S = c + sum_k |v_k a_k b_k|,   against the fp64 formula at the fp32-rounded inputs and parameters
(+ the underflow term of tests/_dot_dense.py fp32_bound, 1e-36 here).  fp64: 1e-12 os S^P."""
import math
import warnings

import pytest
import torch

import _dot_dense as dd
import _loo_dense as ld
from oracle import gp_math as gm
from oracle import projected as pj
from _bridge import perturb_

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32, F64 = torch.float32, torch.float64
SP = torch.nn.functional.softplus


@pytest.fixture(autouse=True)
def _nothing_more_after_a_gpu_error():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("HIP error, nothing more is started: %s" % e, returncode=3)


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


def _kind(P, linear=False):
    return "linear" if linear else "poly%d" % P


def _power(eng, P):
    return eng.hip.lib().cdll.plmc_dot_max_power() if P == "max" else P


def _problem(n, d, q, P, seed, ns=1, czero=False, ard=True, unit=False):
    """X, Xs uniform in [-1, 1]^d, row 1 all zero and row n - 1 a copy of row 0 (n >= 3); v in [0.3, 1] / d (`unit`: 1, the polynomial
    kernel's table), c in [0.1, 0.5] or 0, so that S <= 1.5 and k(x, x) stays within 10^3 noise up to the largest power."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g, dtype=F64)
    X, Xs = 2 * r(n, d) - 1, 2 * r(ns, d) - 1
    if n >= 3:
        X[1] = 0.0
        X[n - 1] = X[0]
    y = torch.randn(q, n, generator=g, dtype=F64)
    v = (0.3 + 0.7 * r(q, d if ard else 1)).expand(q, d).contiguous() / d
    if unit:
        v = torch.ones(q, d, dtype=F64)
    c = torch.zeros(q, dtype=F64) if czero else 0.1 + 0.4 * r(q)
    os_ = 0.5 + r(q)
    noise = 0.1 + 0.4 * r(q)
    return X, Xs, y, v, c, os_, noise


def _table(v, c):
    return torch.cat([v, c.reshape(-1, 1)], 1)


def _assemble_full(eng, X, v, c, P, os_, noise, dt, fill=-7.0):
    """plmc_assemble_dot_*: the whole padded buffer (q, n_pad, n_pad) on the host, filled with `fill` first."""
    hip = eng.hip
    L = hip.lib()
    f = lambda t: None if t is None else t.to(DEV, dt).contiguous()
    n, d = X.shape
    q = v.shape[0]
    ws = eng.exact.Workspace(n, q, 0, dt, DEV, with_inverse=False)
    ws.A.fill_(fill)
    Xd, v_, c_, o_, nz = (f(t) for t in (X, v, c, os_, noise))
    L.call("plmc_assemble_dot", dt, hip.ptr(Xd), n, d, hip.ptr(v_), hip.ptr(c_), P, hip.ptr(o_), hip.ptr(nz), hip.ptr(ws.A), ws.lda,
           ws.strideA, q, hip.stream_ptr(DEV))
    torch.cuda.synchronize()
    return ws.A[:, :ws.n_pad, :ws.n_pad].cpu(), ws.n_pad


def _cross(eng, kind, X, Xs, v, c, os_, dt):
    f = lambda t: None if t is None else t.to(DEV, dt).contiguous()
    K = eng.exact.dense_cross(kind, f(X), f(Xs), _table(f(v), f(c)), f(os_))
    torch.cuda.synchronize()
    return K.cpu()


# ------------------------------------------------------------------------------------------------ per element
#         n,   d, q, P,     czero, ard,   with_os
ELEMENT_CASES = [(1, 1, 1, 1, True, True, True),
                 (127, 4, 3, 2, False, True, True),
                 (128, 5, 1, 3, False, False, False),
                 (129, 8, 3, "max", False, True, True),
                 (257, 9, 1, 1, True, True, False),
                 (257, 16, 3, 3, False, False, True),
                 (129, 16, 1, "max", True, True, True),
                 (129, 1, 3, 3, False, True, True),
                 (257, 4, 1, 2, True, False, False)]


@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("n,d,q,P,czero,ard,with_os", ELEMENT_CASES)
def test_assembly_and_cross_against_the_dense_formula(eng, n, d, q, P, czero, ard, with_os, dt):
    """plmc_assemble_dot / plmc_assemble_cross_dot.  fp64: |err| <= 1e-12 os S^P.  fp32: the derived bound.  Only tiles on and right of
    the block diagonal are written; the padding is the identity; an all-zero row gives os c^P (+ noise on the diagonal) -- for c = 0 a
    row of exact zeros and exactly the noise; the duplicated row repeats row 0's values in the columns right of both."""
    P = _power(eng, P)
    ns = 70
    X, Xs, _, v, c, os_, nz = _problem(n, d, q, P, seed=1000 * n + 10 * d + P, ns=ns, czero=czero, ard=ard)
    if n >= 3:
        Xs[7] = 0.0
    if dt == F32:
        X, Xs, v, c, os_, nz = (t.float().double() for t in (X, Xs, v, c, os_, nz))
    osr = os_ if with_os else None
    one = os_ if with_os else torch.ones_like(os_)
    ref = dd.dot_kernel(X, X, v, c, P, osr) + nz[:, None, None] * torch.eye(n, dtype=F64)
    refx = dd.dot_kernel(X, Xs, v, c, P, osr)
    full, n_pad = _assemble_full(eng, X, v, c, P, osr, nz, dt)
    gotx = _cross(eng, _kind(P), X, Xs, v, c, osr, dt)
    got = full[:, :n, :n]
    up = torch.triu(torch.ones(n, n, dtype=torch.bool))
    for name, a, b, A, B, mask in (("assemble", got.double(), ref, X, X, up), ("cross", gotx.double(), refx, X, Xs, None)):
        err = (a - b).abs()
        SPow = one[:, None, None] * dd.dot_S(A, B, v, c) ** P
        bound = 1e-12 * SPow + 1e-300 if dt == F64 else dd.fp32_bound(A, B, v, c, P, osr)
        if name == "assemble":                                     # (the noise on the diagonal: one more rounding of the sum)
            bound = bound + (2.0 ** -53 if dt == F64 else dd.U32) * torch.diag_embed((torch.diagonal(b, dim1=-2, dim2=-1)).abs())
        if mask is not None:
            err, bound = err[:, mask], bound[:, mask]
        print("%s %s n=%d d=%d P=%d: worst err / bound %.3f" % (name, "f64" if dt == F64 else "f32", n, d, P, float((err / bound).max())))
        assert bool((err <= bound).all()), (name, float((err / bound).max()))
    # tiles left of the block diagonal are never written; rows and columns beyond n are the identity
    m = n_pad // 128
    for ib in range(m):
        for jb in range(ib):
            assert bool((full[:, ib * 128:(ib + 1) * 128, jb * 128:(jb + 1) * 128] == -7.0).all()), (ib, jb)
    pad_up = torch.triu(full)[:, :, n:]
    want = torch.zeros_like(pad_up)
    idx = torch.arange(n, n_pad)
    want[:, idx, idx - n] = 1.0
    assert torch.equal(pad_up, want)
    if n >= 3:
        osd, nzd = one.to(dt), nz.to(dt)
        if czero:                                                   # s = 0 exactly: zeros, and the noise alone on the diagonal
            assert bool((got[:, 1, 2:] == 0).all()) and bool((got[:, 0, 1] == 0).all()) and bool((gotx[:, 1, :] == 0).all())
            assert bool((gotx[:, :, 7] == 0).all())
            assert torch.equal(got[:, 1, 1], nzd)
        else:                                                       # os c^P on the whole row: one value
            row = got[:, 1, 2:]
            assert bool((row == row[:, :1]).all()) and bool((gotx[:, 1, :] == row[:, :1]).all())
            cp = (one * c ** P)
            assert torch.allclose(row[:, 0].double(), cp, rtol=(P + 1) * (2.0 ** -52 if dt == F64 else 2 * dd.U32), atol=0)
            assert torch.allclose(got[:, 1, 1].double(), cp + nz, rtol=(P + 2) * (2.0 ** -52 if dt == F64 else 2 * dd.U32), atol=0)
        if n >= 4:                                                  # row n - 1 copies row 0: K[0, j] = K[j, n - 1] up to the scaled side
            a, b = got[:, 0, 2:n - 1].double(), got[:, 2:n - 1, n - 1].double()
            tol = 2 * (1e-12 * one[:, None] * dd.dot_S(X[:1], X[2:n - 1], v, c)[:, 0] ** P + 1e-300 if dt == F64
                       else dd.fp32_bound(X[:1], X[2:n - 1], v, c, P, osr)[:, 0])
            assert bool(((a - b).abs() <= tol).all())


# ------------------------------------------------------------------------------------------------ log-prob and the gradient table
def _reference_logprob(X, y, v, c, P, os_, nz):
    leaves = [t.clone().requires_grad_() for t in (v, c, os_, nz, y)]
    lp = dd.dot_logprob(X, leaves[4], leaves[0], leaves[1], P, leaves[2], leaves[3])
    g = torch.Generator().manual_seed(99)
    wt = 0.5 + torch.rand(lp.shape, generator=g, dtype=F64)
    (lp * wt).sum().backward()
    return [lp.detach()] + [t.grad for t in leaves] + [wt]


def _run_logprob(eng, kind, X, y, v, c, os_, nz, dt, wt):
    f = lambda t: t.to(DEV, dt)
    d = v.shape[1]
    table = _table(f(v), f(c)).requires_grad_()
    leaves = [f(t).requires_grad_() for t in (os_, nz, y)]
    lp = eng.exact.exact_latent_log_prob(kind, f(X), table, leaves[0], leaves[1], leaves[2])
    (lp * f(wt)).sum().backward()
    torch.cuda.synchronize()
    tg = table.grad.cpu().double()
    return [lp.detach().cpu().double(), tg[:, :d], tg[:, d]] + [t.grad.cpu().double() for t in leaves]


GRAD_NAMES = ("variance", "offset", "oscale", "noise", "y")
#             n,   d,  q, P,    czero, ard
GRAD_CASES = [(65, 1, 3, 1, True, True),
              (129, 4, 1, 2, False, True),
              (257, 5, 3, 3, False, False),
              (129, 8, 1, "max", False, True),
              (65, 9, 3, 2, True, True),
              (257, 16, 1, 3, False, True)]


@pytest.mark.parametrize("n,d,q,P,czero,ard", GRAD_CASES)
def test_logprob_and_every_gradient_fp64(eng, n, d, q, P, czero, ard):
    """Tolerances of tests/test_gpu_rq_kernel.py: log-prob rtol 1e-10; gradients rtol 1e-7 / atol 1e-9."""
    P = _power(eng, P)
    X, _, y, v, c, os_, nz = _problem(n, d, q, P, seed=n + 7 * d + P, czero=czero, ard=ard)
    ref = _reference_logprob(X, y, v, c, P, os_, nz)
    got = _run_logprob(eng, _kind(P), X, y, v, c, os_, nz, F64, ref[6])
    assert torch.allclose(got[0], ref[0], rtol=1e-10, atol=0), (got[0], ref[0])
    for name, a, b in zip(GRAD_NAMES, got[1:], ref[1:6]):
        assert a.shape == b.shape, name
        print("d/d %s: max abs err %.3g of %.3g" % (name, float((a - b).abs().max()), float(b.abs().max())))
        assert torch.allclose(a, b, rtol=1e-7, atol=1e-9), (name, float((a - b).abs().max()))


@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
def test_the_diagonal_contributes_to_every_gradient(eng, monkeypatch, dt):
    """P = 3, n = 129, d = 4, one point at 3 x the range: its diagonal entry k(x, x) ~ 300 os dwarfs every off-diagonal one, and so does its
    share of d/dv, d/dc and d/dos.  A diagonal that fed noise and os only would miss the v- and c-gradients by their leading term: asserted
    on the difference a diagonal-free gradient would show (> 10 % of the entry) beside the usual tolerances."""
    n, d, q, P = 129, 4, 2, 3
    X, _, y, v, c, os_, nz = _problem(n, d, q, P, seed=5)
    X[64] = 3.0 * torch.sign(X[64])
    y = dd.prior_draw(X, v, c, P, os_, nz, seed=6)
    if dt == F32:
        X, y, v, c, os_, nz = (t.float().double() for t in (X, y, v, c, os_, nz))
    ref = _reference_logprob(X, y, v, c, P, os_, nz)
    monkeypatch.delenv("PLMC_SPLIT", raising=False)
    eng.hip.lib().cdll.plmc_dev_reload_knobs()
    got = _run_logprob(eng, _kind(P), X, y, v, c, os_, nz, dt, ref[6])
    # what the diagonal adds to d/dc: sum_i 1/2 (a_i^2 - Kinv_ii) os P s_ii^(P - 1), per latent
    Kh = dd.dot_kernel(X, X, v, c, P, os_) + nz[:, None, None] * torch.eye(n, dtype=F64)
    Pm = torch.linalg.inv(Kh)
    a = (Pm @ y.unsqueeze(-1)).squeeze(-1)
    sii = c[:, None] + v @ (X * X).T
    diag_c = (0.5 * (a * a - torch.diagonal(Pm, dim1=-2, dim2=-1)) * os_[:, None] * P * sii ** (P - 1)).sum(-1) * ref[6]
    assert bool((diag_c.abs() > 0.1 * ref[2].abs()).all()), (diag_c, ref[2])
    assert float(torch.diagonal(Kh, dim1=-2, dim2=-1).max()) > 20 * float(torch.triu(Kh, 1)[:, :64, :64].abs().max())
    if dt == F64:
        assert torch.allclose(got[0], ref[0], rtol=1e-10, atol=0)
        for name, g_, r_ in zip(GRAD_NAMES, got[1:], ref[1:6]):
            assert torch.allclose(g_, r_, rtol=1e-7, atol=1e-9), (name, float((g_ - r_).abs().max()))
    else:
        assert float(((got[0] - ref[0]) / ref[0]).abs().max()) < 1e-4
        for name, g_, r_ in zip(GRAD_NAMES, got[1:], ref[1:6]):
            e = float((g_ - r_).abs().max() / r_.abs().max())
            print("far-out point, fp32: d/d %s err %.3g of the largest" % (name, e))
            assert e < 2e-3, (name, e)


def test_logprob_without_an_output_scale_the_linear_kind_fp64(eng):
    """oscale = None (a bare LinearKernel): unit output scale, no gradient for it; kind "linear" runs P = 1."""
    n, d, q = 129, 3, 3
    X, _, y, v, c, _, nz = _problem(n, d, q, 1, seed=8, czero=True)
    one = torch.ones(q, dtype=F64)
    ref = _reference_logprob(X, y, v, c, 1, one, nz)
    f = lambda t: t.to(DEV)
    table = _table(f(v), f(c)).requires_grad_()
    nzd = f(nz).requires_grad_()
    lp = eng.exact.exact_latent_log_prob("linear", f(X), table, None, nzd, f(y))
    (lp * f(ref[6])).sum().backward()
    assert torch.allclose(lp.detach().cpu(), ref[0], rtol=1e-10, atol=0)
    assert torch.allclose(table.grad.cpu()[:, :d], ref[1], rtol=1e-7, atol=1e-9) and torch.allclose(table.grad.cpu()[:, d], ref[2], rtol=1e-7, atol=1e-9)
    assert torch.allclose(nzd.grad.cpu(), ref[4], rtol=1e-7, atol=1e-9)


def _factor_buffer(eng, kind, X, v, c, os_, nz, y, fused, monkeypatch):
    """The factor buffer of one fp32 factorisation with the inverse factor, zeroed first."""
    f = lambda t: t.to(DEV, F32).contiguous()
    n, q = X.shape[0], v.shape[0]
    ws = eng.exact.Workspace(n, q, 1, F32, DEV, with_inverse=True)
    ws.A.zero_()
    ws.Vd.zero_()
    if not fused:
        monkeypatch.setenv("PLMC_FUSED_ASSEMBLE", "0")
    eng.exact.factorize(kind, f(X), _table(f(v), f(c)), f(os_), f(nz), f(y).reshape(q, 1, n), ws)
    if not fused:
        monkeypatch.delenv("PLMC_FUSED_ASSEMBLE")
    torch.cuda.synchronize()
    return ws.A.cpu(), ws.logdet.cpu()


@pytest.mark.parametrize("n,d,P", [(257, 1, 3), (129, 5, 2), (257, 16, "max"), (65, 8, 1)])
def test_logprob_fp32_on_every_arithmetic_and_fused_against_two_call_assembly(eng, monkeypatch, n, d, P):
    """q = 3, fp32 with PLMC_SPLIT unset, 0 and 3: value 1e-4 relative, each gradient 2e-3 of that tensor's largest entry (the project's
    fp32 tolerances).  plmc_factorize_dot_ex (the fused assembly) and PLMC_FUSED_ASSEMBLE=0 (plmc_assemble_dot, then the sweep) give
    the same factor buffer, log-determinant, value and gradients as bit patterns.  y is drawn from the prior with OTHER parameters."""
    P = _power(eng, P)
    q = 3
    X, _, _, v, c, os_, nz = _problem(n, d, q, P, seed=77 + d + n)
    y = dd.prior_draw(X, 1.3 * v, 0.7 * c, P, 0.8 * os_, 0.5 * nz, seed=3)
    X, y, v, c, os_, nz = (t.float().double() for t in (X, y, v, c, os_, nz))
    ref = _reference_logprob(X, y, v, c, P, os_, nz)
    kind = _kind(P)
    monkeypatch.delenv("PLMC_SPLIT", raising=False)                     # "unset" means unset, whatever the caller's environment
    monkeypatch.delenv("PLMC_FUSED_ASSEMBLE", raising=False)
    eng.hip.lib().cdll.plmc_dev_reload_knobs()

    def check(tag):
        got = _run_logprob(eng, kind, X, y, v, c, os_, nz, F32, ref[6])
        monkeypatch.setenv("PLMC_FUSED_ASSEMBLE", "0")
        two = _run_logprob(eng, kind, X, y, v, c, os_, nz, F32, ref[6])
        monkeypatch.delenv("PLMC_FUSED_ASSEMBLE")
        for a, b in zip(got, two):
            assert torch.equal(a, b), tag
        A1, ld1 = _factor_buffer(eng, kind, X, v, c, os_, nz, y, True, monkeypatch)
        A2, ld2 = _factor_buffer(eng, kind, X, v, c, os_, nz, y, False, monkeypatch)
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


# ------------------------------------------------------------------------------------------------ models
def _kernel_tables(raw, pre, q, d, which):
    """(v (q, d), c (q)) from a dict of raw parameters under the gpytorch names `pre`raw_variance / raw_offset."""
    if which == "linear":
        v = SP(raw[pre + "raw_variance"]).reshape(q, -1)
        return v.expand(q, d), torch.zeros(q, dtype=F64)
    return torch.ones(q, d, dtype=F64), SP(raw[pre + "raw_offset"]).reshape(q)


def _dense_pieces(model, X, Y, q, which):
    sp = torch.nn.functional.softplus
    raw = {k: v.detach().cpu().double().requires_grad_() for k, v in model.named_parameters()}
    scaled = hasattr(model.covar_module, "base_kernel")
    v, c = _kernel_tables(raw, "covar_module.base_kernel." if scaled else "covar_module.", q, X.shape[1], which)
    os_ = sp(raw["covar_module.raw_outputscale"]).reshape(q) if scaled else None
    lik = model.likelihood
    noise = lik.noise_covar.raw_noise_constraint.transform(raw["likelihood.noise_covar.raw_noise"]).reshape(-1).expand(q)
    cm = raw["mean_module.raw_constant"].reshape(q, 1) if "mean_module.raw_constant" in raw else raw["mean_module.constant"].reshape(q, 1)
    y = (Y.reshape(X.shape[0], -1).T if Y.dim() > 1 else Y.reshape(1, -1)) - cm
    return raw, (v, c, os_, noise, cm, y)


def _data(n, p, seed, d=2):
    """A quadratic in x plus noise, x uniform in [-1, 1]^d with one all-zero and one duplicated row."""
    g = torch.Generator().manual_seed(seed)
    X = 2 * torch.rand(n, d, generator=g, dtype=F64) - 1
    X[1], X[n - 1] = 0.0, X[0]
    Y = torch.stack([(1 + k) * X[:, 0] ** 2 - X[:, 0] * X[:, -1] + 0.5 * X[:, -1] + 0.3 * torch.randn(n, generator=g, dtype=F64) for k in range(p)], 1)
    return X, Y


@pytest.mark.parametrize("which,P", [("linear", 1), ("poly", 2), ("poly", 3)])
def test_single_output_exact_model_train_eval_full_cov_and_cache(plmc, which, P):
    """ExactGPModel with ScaleKernel(LinearKernel | PolynomialKernel), d = 2, fp64; the tolerances of the rational-quadratic test of the
    same name: loss within 1e-9 relative of dense, every parameter gradient rtol 1e-5 / atol 1e-9, eval-mode mean rtol 1e-7, variance and
    full_cov rtol 1e-6.  The test points reach 2 x the training range, where k(x*, x*) is far from os (asserted): a predictive variance
    that started from os would miss.  A second prediction hits the cache and repeats the first; clear_prediction_cache() drops it."""
    from projectedlmc import settings
    n, ns, d = 129, 40, 2
    X, Y = _data(n, 1, seed=1, d=d)
    y = Y[:, 0]
    torch.manual_seed(4)
    kt = plmc.LinearKernel if which == "linear" else plmc.PolynomialKernel
    kk = {} if which == "linear" else {"power": P}
    m = perturb_(plmc.ExactGPModel(X, y, plmc.GaussianLikelihood(), kernel_type=kt, ker_kwargs=kk, outputscales=True).double())
    with torch.no_grad():
        m.likelihood.noise_covar.raw_noise.fill_(-1.0)               # noise = softplus(-1) = 0.31 + the lower bound
    m = m.to(DEV)
    m.train(); m.likelihood.train()
    mll = plmc.ExactMarginalLogLikelihood(m.likelihood, m)
    loss = -mll(m(X.to(DEV)), y.to(DEV))
    loss.backward()
    raw, (v, c, os_, noise, cm, resid) = _dense_pieces(m, X, y, 1, which)
    ref = -(dd.dot_logprob(X, resid, v, c, P, os_, noise).sum() / n)
    ref.backward()
    assert abs(float(loss.detach()) - float(ref.detach())) < 1e-9 * abs(float(ref.detach())), (float(loss.detach()), float(ref.detach()))
    names = [nm for nm, _ in m.named_parameters()]
    assert ("covar_module.base_kernel.raw_variance" if which == "linear" else "covar_module.base_kernel.raw_offset") in names
    for name, prm in m.named_parameters():
        a, b = prm.grad.cpu().double(), raw[name].grad
        assert torch.allclose(a, b.reshape(a.shape), rtol=1e-5, atol=1e-9), (name, float((a - b.reshape(a.shape)).abs().max()))
    g = torch.Generator().manual_seed(2)
    Xs = 4 * torch.rand(ns, d, generator=g, dtype=F64) - 2
    Xs[3] = 0.0
    dt_ = lambda t: t.detach()
    mean_ref, cov_ref = dd.dot_posterior(X, dt_(resid), Xs, dt_(v), dt_(c), P, dt_(os_), dt_(noise))
    prior = dd.dot_diag(Xs, dt_(v), dt_(c), P, dt_(os_))[0]
    assert float((prior / dt_(os_)[0]).max()) > 3.0 and float((prior / dt_(os_)[0]).min()) < 0.7          # k(x*, x*) is visibly not os
    m.eval(); m.likelihood.eval()
    with settings.prediction_cache("eager"), torch.no_grad():
        post = m(Xs.to(DEV))
        cch = m._prediction_cache()
        assert (cch.hits, cch.misses) == (0, 1) and cch.ws is not None
        again = m(Xs.to(DEV))
        assert (cch.hits, cch.misses) == (1, 1)
        full = m(Xs.to(DEV), full_cov=True)
        m.clear_prediction_cache()
        assert m._prediction_cache().ws is None
        third = m(Xs.to(DEV))
    for p_ in (post, again, third):
        assert torch.allclose(p_.mean.cpu(), mean_ref[0] + dt_(cm)[0], rtol=1e-7, atol=1e-9)
        assert torch.allclose(p_.variance.cpu(), torch.diagonal(cov_ref[0]), rtol=1e-6, atol=1e-9)
    assert torch.allclose(again.mean, post.mean, rtol=1e-10, atol=1e-12) and torch.allclose(again.variance, post.variance, rtol=1e-9, atol=1e-12)
    assert torch.allclose(full.covariance_matrix.cpu().reshape(ns, ns), cov_ref[0], rtol=1e-6, atol=1e-9)


def test_two_powers_do_not_share_a_prediction_cache_entry(eng):
    """The same inputs, parameters and cache key under "poly2" and "poly3": the power travels in the kind, the kind in the cache's key, so
    the second call is a miss and gives the other power's posterior."""
    from projectedlmc import settings
    n, ns, d, q = 65, 9, 2, 1
    X, Xs, y, v, c, os_, nz = _problem(n, d, q, 2, seed=12, ns=ns, unit=True)
    f = lambda t: t.to(DEV)
    cache = eng.exact.PosteriorCache()
    with settings.prediction_cache("eager"), torch.no_grad():
        for P in (2, 3, 2):
            mean, var = eng.exact.exact_posterior(_kind(P), f(X), _table(f(v), f(c)), f(os_), f(nz), f(y), f(Xs), cache=cache, key=("same",))
            ref_m, ref_c = dd.dot_posterior(X, y, Xs, v, c, P, os_, nz)
            assert torch.allclose(mean.cpu(), ref_m, rtol=1e-7, atol=1e-9), P
            assert torch.allclose(var.cpu(), torch.diagonal(ref_c, dim1=-2, dim2=-1), rtol=1e-6, atol=1e-9), P
        mean, _ = eng.exact.exact_posterior(_kind(2), f(X), _table(f(v), f(c)), f(os_), f(nz), f(y), f(Xs), cache=cache, key=("same",))
        assert torch.allclose(mean.cpu(), dd.dot_posterior(X, y, Xs, v, c, 2, os_, nz)[0], rtol=1e-7, atol=1e-9)
    assert (cache.hits, cache.misses) == (1, 3), (cache.hits, cache.misses)       # only the repeat of the last kind hits


def test_loo_pseudo_likelihood_value_and_gradient(plmc):
    """LeaveOneOutPseudoLikelihood with PolynomialKernel(power=2): value 1e-9 relative, every raw-parameter gradient rtol 1e-5 / atol 1e-9
    against the dense objective of tests/_loo_dense.py (the tolerances of tests/test_gpu_loo_objective.py's model tests)."""
    n, d = 150, 3
    X, Y = _data(n, 1, seed=9, d=d)
    y = Y[:, 0]
    lik = plmc.GaussianLikelihood()
    torch.manual_seed(2)
    m = perturb_(plmc.ExactGPModel(X, y, lik, kernel_type=plmc.PolynomialKernel, ker_kwargs={"power": 2}, outputscales=True).double())
    with torch.no_grad():
        m.likelihood.noise_covar.raw_noise.fill_(-1.0)
    raw, (v, c, os_, noise, cm, resid) = _dense_pieces(m, X, y, 1, "poly")
    Kh = dd.dot_kernel(X, X, v, c, 2, os_) + noise.reshape(1, 1, 1) * torch.eye(n, dtype=F64)
    ref = ld.loo_log_prob(Kh, resid) / n
    ref.sum().backward()
    assert torch.allclose(ref.detach() * n, dd.dot_loo(X, resid.detach(), v.detach(), c.detach(), 2, os_.detach(), noise.detach()), rtol=1e-10)
    m, lik = m.to(DEV), lik.to(DEV)
    m.train(); lik.train()
    out = plmc.LeaveOneOutPseudoLikelihood(lik, m, X, y)(m(X.to(DEV)), y.to(DEV))
    out.sum().backward()
    assert abs(float(out.sum().detach()) - float(ref.sum().detach())) <= 1e-9 * abs(float(ref.sum().detach()))
    for name, prm in m.named_parameters():
        assert prm.grad is not None and raw[name].grad is not None, name
        a, b = prm.grad.cpu(), raw[name].grad.reshape(prm.shape)
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-9), (name, a, b)


def _projected(plmc, X, Y, q, kt, kk, seed=5, **kw):
    torch.manual_seed(seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return plmc.ProjectedGPModel(X, Y, Y.shape[1], q, mean_type=plmc.ZeroMean, kernel_type=kt, ker_kwargs=kk, init_lmc_coeffs=True, **kw)


def _oracle_dict(model):
    """The oracle's parameter dict (oracle/projected.py) WITHOUT kernel keys, from the state dict (bulk H), and the map product parameter
    name -> dict key; as tests/test_gpu_rq_kernel.py builds it."""
    lb = model.likelihood.noise_covar.raw_noise_constraint.lower_bound
    sd = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
    lmc = model.lmc_coefficients
    P = dict(n_tasks=model.n_tasks, n_latents=model.n_latents, mode=lmc.mode, BDN=not hasattr(model, "M"), eps=model.eps,
             scalar_B=model.scalar_B, diagonal_B=model.diagonal_B, noise_lb=lb, noise_thresh=math.log(lb), bulk=lmc.bulk,
             raw_noise=sd["likelihood.noise_covar.raw_noise"], B_tilde_inv_chol_raw=sd["parametrizations.B_tilde_inv_chol.original"])
    names = {"likelihood.noise_covar.raw_noise": "raw_noise", "parametrizations.B_tilde_inv_chol.original": "B_tilde_inv_chol_raw"}
    assert lmc.bulk
    P["H"] = sd["lmc_coefficients.H"]
    names["lmc_coefficients.H"] = "H"
    kern = {k: v for k, v in sd.items() if k.startswith("covar_module.")}
    return P, kern, names


@pytest.mark.parametrize("which,P", [("linear", 1), ("poly", 2)])
def test_projected_model_loss_gradients_eval_mode_and_evaluate(plmc, which, P):
    """fp64, p = 5, q = 3, d = 2, n = 129, perturbed parameters; the body and the tolerances of the rational-quadratic test of the same
    name: ProjectedLMCmll and the gradient of every parameter against sum_i log N(ytil_i; 0, K_i + noise_i I) / n + the oracle's projection
    terms (1e-9 relative; rtol 2e-6, atol 1e-8); eval mode (task mean / variance, latent mean and full covariance) against dense
    conditioning (rtol 1e-8 / 1e-7); the cached second call equals the first; evaluate() gives the dense latent covariances."""
    from projectedlmc import settings
    n, p, q, ns, d = 129, 5, 3, 40, 2
    X, Y = _data(n, p, seed=3, d=d)
    kt = plmc.LinearKernel if which == "linear" else plmc.PolynomialKernel
    m = perturb_(_projected(plmc, X, Y, q, kt, {} if which == "linear" else {"power": P}).double())
    Pd_, kern, names = _oracle_dict(m)
    leaves = {**{k: Pd_[k] for k in names.values()}, **kern}
    for t in leaves.values():
        t.requires_grad_(True)
    latent_K = lambda kn, A, B: dd.dot_kernel(A, B, *_kernel_tables(kn, "covar_module.", q, d, which), P)
    eye = torch.eye(n, dtype=F64)
    ytil = pj.project_data(Pd_, Y)
    K = latent_K(kern, X, X) + pj.projected_noise(Pd_).reshape(q, 1, 1) * eye
    terms, const = pj.projection_terms(Pd_, Y)
    ref = -(gm.mvn_log_prob(K, ytil).sum() / n + sum(terms) + const)
    ref.backward()
    m = m.to(DEV)
    Xd, Yd = X.to(DEV), Y.to(DEV)
    m.train(); m.likelihood.train()
    loss = -plmc.ProjectedLMCmll(m.likelihood, m)(m(Xd), Yd)
    loss.backward()
    assert abs(float(loss.detach()) - float(ref.detach())) < 1e-9 * abs(float(ref.detach())), (float(loss.detach()), float(ref.detach()))
    checked = 0
    for pname, prm in m.named_parameters():
        g_ref = leaves[names.get(pname, pname)].grad
        assert prm.grad is not None and g_ref is not None, pname
        assert prm.grad.shape == g_ref.shape, pname
        assert torch.allclose(prm.grad.cpu(), g_ref, rtol=2e-6, atol=1e-8), (pname, prm.grad.cpu(), g_ref)
        checked += 1
    assert checked == len(names) + 1                        # + the variances or the offset
    with torch.no_grad():
        Pd = {k: (t.detach() if torch.is_tensor(t) else t) for k, t in Pd_.items()}
        kd = {k: t.detach() for k, t in kern.items()}
        K, ytil = K.detach(), ytil.detach()
        g = torch.Generator().manual_seed(8)
        Xs = 3 * torch.rand(ns, d, generator=g, dtype=F64) - 1.5
        Ks, Kss = latent_K(kd, X, Xs), latent_K(kd, Xs, Xs)
        sol = torch.linalg.solve(K, Ks)
        mu_lat = (sol * ytil.unsqueeze(-1)).sum(1)
        cov_lat = Kss - Ks.transpose(-1, -2) @ sol
        Ht = pj.lmc_coefficients(Pd)
        mean_ref = mu_lat.T @ Ht
        var_ref = torch.diagonal(cov_lat, dim1=-2, dim2=-1).T @ (Ht * Ht) + Pd["eps"]
    m.eval(); m.likelihood.eval()
    with settings.prediction_cache("eager"), torch.no_grad():
        dist = m(Xs.to(DEV))
        cch = m._prediction_cache()
        assert (cch.hits, cch.misses) == (0, 1) and cch.ws is not None and cch.ws.with_inverse
        again = m(Xs.to(DEV))
        assert (cch.hits, cch.misses) == (1, 1)
        lat = m.compute_latent_distrib(Xs.to(DEV), full_cov=True)
        dense = m.covar_module(Xd).evaluate()
    for d_ in (dist, again):
        assert torch.allclose(d_.mean.cpu(), mean_ref, rtol=1e-8, atol=1e-10)
        assert torch.allclose(d_.variance.cpu(), var_ref, rtol=1e-7, atol=1e-10)
    assert torch.allclose(lat.mean.cpu(), mu_lat, rtol=1e-8, atol=1e-10)
    assert torch.allclose(lat.covariance_matrix.cpu(), cov_lat, rtol=1e-7, atol=1e-10)
    assert torch.allclose(dense.cpu(), latent_K(kd, X, X), rtol=1e-10, atol=1e-12)               # evaluate()


def test_latent_shards_sum_to_the_unsharded_loss_and_gradients(plmc):
    """The shards of a latent-sharded projected model sum to the unsharded loss (1e-10) and gradients (rtol 1e-8): the table is sliced by
    latent_ids like ell is, its offset column with it."""
    n, p, q, world, d = 129, 6, 3, 2, 2
    X, Y = _data(n, p, seed=21, d=d)
    Xd, Yd = X.to(DEV), Y.to(DEV)

    def build(shard):
        m = perturb_(_projected(plmc, X, Y, q, plmc.PolynomialKernel, {"power": 2}, seed=2, latent_shard=shard).double()).to(DEV)
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
    assert abs(total - float(loss0.detach())) < 1e-10 * abs(float(loss0.detach())), (total, float(loss0.detach()))
    for (name, prm), g in zip(m0.named_parameters(), grads):
        assert torch.allclose(prm.grad, g, rtol=1e-8, atol=1e-11), (name, (prm.grad - g).abs().max())


# ------------------------------------------------------------------------------------------------ draws
def test_draws_with_noise_have_the_prior_covariance(plmc):
    """rsample of N(loc, K + noise I), PolynomialKernel(power=2) inside a ScaleKernel, n = 65, q = 2, fp32, 4096 draws: mean and sample
    covariance within the 6-sigma band of tests/test_gpu_sampling.py (_moment_check), against evaluate() + noise."""
    dtype, n, q, s = F32, 65, 2, 4096
    g = torch.Generator().manual_seed(4)
    X = 2 * torch.rand(n, 2, generator=g, dtype=F64) - 1
    X[1], X[n - 1] = 0.0, X[0]
    X = X.to(dtype).to(DEV)
    loc = torch.randn(q, n, generator=g, dtype=F64).to(dtype).to(DEV)
    k = plmc.ScaleKernel(plmc.PolynomialKernel(power=2, batch_shape=torch.Size([q])), batch_shape=torch.Size([q]))
    k.base_kernel.offset = torch.tensor([[0.4], [0.9]])
    k.outputscale = torch.tensor([0.7, 1.2])
    lazy = k.to(dtype).to(DEV)(X).add_noise(torch.full((q,), 0.2, dtype=dtype, device=DEV))
    dist = plmc.MultivariateNormal(loc, lazy)
    torch.manual_seed(1234)
    draws = dist.rsample(torch.Size([s]))
    assert draws.shape == (s, q, n) and dist.sample_jitter == 0.0
    K = lazy.evaluate().double().cpu()
    v, c = torch.ones(q, 2, dtype=F64), torch.tensor([0.4, 0.9], dtype=F64).float().double()
    Kd = dd.dot_kernel(X.double().cpu(), X.double().cpu(), v, c, 2, torch.tensor([0.7, 1.2]).double()) + 0.2 * torch.eye(n, dtype=F64)
    assert torch.allclose(K, Kd, rtol=1e-5, atol=1e-6)
    for b in range(q):
        dr, lc = draws[:, b].double().cpu(), loc[b].double().cpu()
        mu, C, dg = dr.mean(0), torch.cov(dr.T), torch.diagonal(K[b])
        tol_m = 6 * torch.sqrt(dg / s)
        tol_c = 6 * torch.sqrt((dg[:, None] * dg[None, :] + K[b] * K[b]) / (s - 1))
        wm, wc = float(((mu - lc).abs() / tol_m).max()), float(((C - K[b]).abs() / tol_c).max())
        print("latent %d: worst mean %.2f / 6 sigma, worst covariance %.2f / 6 sigma" % (b, wm * 6, wc * 6))
        assert wm <= 1.0 and wc <= 1.0, (b, wm, wc)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_noise_free_linear_prior_goes_up_the_jitter_ladder(plmc, dtype):
    """A noise-free linear prior on d = 2 has rank 2: n = 65 points make K singular.  The draw does not raise; it returns the jitter that
    made the factorisation go through (at least the first rung), and the draws are finite with the prior's covariance up to that jitter:
    S^T S = K + jitter I within 1e-3 |K| (fp32) / 1e-6 |K| (fp64) for identity base samples."""
    from projectedlmc import settings
    q, n, d = 2, 65, 2
    g = torch.Generator().manual_seed(3)
    X = (2 * torch.rand(n, d, generator=g, dtype=F64) - 1).to(dtype).to(DEV)
    k = plmc.LinearKernel(ard_num_dims=d, batch_shape=torch.Size([q])).to(dtype).to(DEV)
    k.variance = torch.tensor([[0.5, 1.5], [1.0, 0.3]]).reshape(q, 1, d)
    dist = plmc.MultivariateNormal(torch.zeros(q, n, dtype=dtype, device=DEV), k(X))
    assert dist.lazy_covariance_matrix.noise is None
    Z = torch.eye(n, dtype=dtype, device=DEV)[:, None, :].expand(n, q, n).contiguous()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        draws = dist.sample(base_samples=Z)
    jit = dist.sample_jitter
    assert jit >= settings.cholesky_jitter.value(dtype) > 0.0
    assert bool(torch.isfinite(draws).all())
    S = draws.permute(1, 0, 2).double().cpu()
    K = dist.lazy_covariance_matrix.evaluate().double().cpu()
    err = (S.transpose(1, 2) @ S - K - jit * torch.eye(n, dtype=F64)).abs().max()
    print("noise-free linear prior %s: jitter %.1e, |S^T S - K - jitter I| max %.3g, |K| max %.3g" % (dtype, jit, float(err), float(K.abs().max())))
    assert float(err) <= (1e-3 if dtype == F32 else 1e-6) * float(K.abs().max())


def test_five_optimiser_steps_decrease_the_loss(plmc):
    """PolynomialKernel(power=2) on data drawn from a quadratic plus noise, fp32, n = 129, Adam(0.05): the loss after five steps is finite
    and below the first; the trained model then predicts in fp32."""
    n, d = 129, 2
    X, Y = _data(n, 1, seed=31, d=d)
    X, y = X.float().to(DEV), Y[:, 0].float().to(DEV)
    torch.manual_seed(0)
    m = plmc.ExactGPModel(X, y, plmc.GaussianLikelihood(), kernel_type=plmc.PolynomialKernel, ker_kwargs={"power": 2}, outputscales=True).to(DEV)
    m.train(); m.likelihood.train()
    mll = plmc.ExactMarginalLogLikelihood(m.likelihood, m)
    opt = torch.optim.Adam(m.parameters(), lr=0.05)
    losses = []
    for _ in range(6):
        opt.zero_grad()
        loss = -mll(m(X), y)
        loss.backward()
        losses.append(float(loss.detach()))
        opt.step()
    print("losses", losses)
    assert all(math.isfinite(l_) for l_ in losses) and losses[-1] < losses[0], losses
    assert all(bool(torch.isfinite(p_).all()) for p_ in m.parameters())
    # ... and the trained fp32 model predicts: mean within 2e-3 of the largest mean, variance within 2e-3 of the largest prior variance
    # (the project's fp32 figure for derived quantities) against dense fp64 conditioning at the model's parameters
    raw, (v, c, os_, noise, cm, resid) = _dense_pieces(m, X.double().cpu(), y.double().cpu(), 1, "poly")
    g = torch.Generator().manual_seed(5)
    Xs = (3 * torch.rand(30, d, generator=g, dtype=F64) - 1.5).float()
    dt_ = lambda t: t.detach()
    mean_ref, cov_ref = dd.dot_posterior(X.double().cpu(), dt_(resid), Xs.double(), dt_(v), dt_(c), 2, dt_(os_), dt_(noise))
    m.eval(); m.likelihood.eval()
    with torch.no_grad():
        post = m(Xs.to(DEV))
    mean_ref = mean_ref[0] + dt_(cm)[0]
    prior = dd.dot_diag(Xs.double(), dt_(v), dt_(c), 2, dt_(os_))[0]
    e_m = float((post.mean.cpu().double() - mean_ref).abs().max() / mean_ref.abs().max())
    e_v = float((post.variance.cpu().double() - torch.diagonal(cov_ref[0])).abs().max() / prior.max())
    print("fp32 prediction after training: mean err %.3g of the largest, variance err %.3g of the largest prior variance" % (e_m, e_v))
    assert e_m < 2e-3 and e_v < 2e-3, (e_m, e_v)


# ------------------------------------------------------------------------------------------------ limits
def test_limits_are_argument_errors(eng):
    """d = plmc_dot_max_dim() + 1, P = plmc_dot_max_power() + 1, P = 0, a null offset and d = 0: refused on the host by every entry point
    through the library's argument error; nothing is launched (the output buffers keep their fill)."""
    hip = eng.hip
    L = hip.lib()
    Dx, Px = L.cdll.plmc_dot_max_dim(), L.cdll.plmc_dot_max_power()
    n, q = 130, 1
    st = hip.stream_ptr(DEV)
    for d, P, null, word in ((Dx + 1, 2, False, "plmc_dot_max_dim"), (2, Px + 1, False, "plmc_dot_max_power"), (2, 0, False, "plmc_dot_max_power"),
                             (2, 2, True, "null pointer"), (0, 2, False, "plmc_dot_max_dim")):
        dd_ = max(d, 1)
        X = torch.rand(n, dd_, device=DEV, dtype=F64)
        z = torch.ones(q, dd_, device=DEV, dtype=F64)
        cc = None if null else hip.ptr(torch.ones(q, device=DEV, dtype=F64))
        o, nz = torch.ones(q, device=DEV, dtype=F64), torch.ones(q, device=DEV, dtype=F64)
        ws = eng.exact.Workspace(n, q, 0, F64, DEV, with_inverse=False)
        ws.A.fill_(-7.0)
        with pytest.raises(RuntimeError, match=word):
            L.call("plmc_assemble_dot", F64, hip.ptr(X), n, d, hip.ptr(z), cc, P, hip.ptr(o), hip.ptr(nz), hip.ptr(ws.A), ws.lda, ws.strideA, q, st)
        out = torch.full((q, n, n), -7.0, device=DEV, dtype=F64)
        with pytest.raises(RuntimeError, match=word):
            L.call("plmc_assemble_cross_dot", F64, hip.ptr(X), n, hip.ptr(X), n, d, hip.ptr(z), cc, P, hip.ptr(o), hip.ptr(out), n, n * n, 0, n, q, st)
        wi = eng.exact.Workspace(n, q, 1, F64, DEV, with_inverse=True)
        wi.A.fill_(-7.0)
        with pytest.raises(RuntimeError, match=word):
            L.call("plmc_factorize_dot_ex", F64, hip.ptr(X), n, d, hip.ptr(z), cc, P, hip.ptr(o), hip.ptr(nz), hip.ptr(wi.A), wi.n_pad, wi.lda,
                   wi.naug, wi.strideA, hip.ptr(wi.Vd), hip.ptr(wi.logdet), hip.ptr(wi.info), 1, q, hip.ptr(nz), st)
        gt = torch.full((q, dd_ + 3), -7.0, device=DEV, dtype=F64)
        with pytest.raises(RuntimeError, match=word):
            L.call("plmc_kinv_grad_dot_vd", F64, hip.ptr(wi.W), wi.n_pad, wi.ldw, wi.strideW, hip.ptr(wi.alpha), hip.ptr(X), n, d, hip.ptr(z),
                   cc, P, hip.ptr(o), hip.ptr(gt), None, 0, 0, None, hip.ptr(wi.partials), q, hip.ptr(nz), hip.ptr(wi.Vd), st)
        with pytest.raises(RuntimeError, match=word):
            L.call("plmc_loo_grad_dot", F64, hip.ptr(wi.W), wi.n_pad, wi.n_pad, wi.ldw, wi.strideW, hip.ptr(wi.alpha), hip.ptr(X), n, d,
                   hip.ptr(z), cc, P, hip.ptr(o), hip.ptr(gt), hip.ptr(wi.partials), q, st)
        torch.cuda.synchronize()
        for buf in (ws.A, out, wi.A, gt):
            assert bool((buf == -7.0).all())
    # ... and by the host layer, before the library is called
    y0, one = torch.zeros(q, n, device=DEV, dtype=F64), torch.ones(q, device=DEV, dtype=F64)
    with pytest.raises(ValueError, match="plmc_dot_max_dim"):
        eng.exact.exact_latent_log_prob("poly2", torch.rand(n, Dx + 1, device=DEV, dtype=F64), torch.ones(q, Dx + 2, device=DEV, dtype=F64), None, one, y0)
    with pytest.raises(ValueError, match="plmc_dot_max_power"):
        eng.exact.exact_latent_log_prob("poly%d" % (Px + 1), torch.rand(n, 2, device=DEV, dtype=F64), torch.ones(q, 3, device=DEV, dtype=F64), None, one, y0)
