"""The dense-LMC kernels (csrc/lmc.hip: k_lmc_assemble, k_lmc_cross, k_lmc_kinv_grad, plmc_w_diag) and the kernel VJP
(csrc/kernel_vjp.hip) against plain fp64 torch references from `oracle/`, called through their Python wrappers: all
four stationary kinds, input dimensions on both sides of every DCAP instantiation, task counts that do not divide the
128-row tile, one and three latents, with and without output scales, coincident and nearly coincident points, fp64
and fp32, and the LDS-table limits of the dense-LMC kernels.  One axis at a time around a small base case."""
import math
import types
import zlib

import pytest
import torch

from oracle import gp_math as gm
from oracle import lmc_dense as ld

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KINDS = {"rbf": ("rbf", 2.5), "matern12": ("matern", 0.5), "matern32": ("matern", 1.5), "matern52": ("matern", 2.5)}
U32 = 2.0 ** -24                                    # unit roundoff of fp32


@pytest.fixture(scope="module")
def eng():
    from projectedlmc import _hip, _engine, _lmc_engine, _var_engine
    assert torch.cuda.is_available()
    return types.SimpleNamespace(hip=_hip, exact=_engine, lmc=_lmc_engine, var=_var_engine)


def _rounded(dt, *ts):
    """The inputs as the kernels see them: rounded to `dt`, back in fp64 for the oracle."""
    return [None if t is None else t.to(dt).double() for t in ts]


def _case_id(c):
    return "-".join("%s=%s" % (k, v) for k, v in c.items()) or "base"


# ------------------------------------------------------------------------------------------------ kernel VJP
# Base case: matern52, d = 5, n1 = 5, n2 = 65, q = 3, with output scales.  d: both sides of DCAP = 4 / 8 / 16 / 32;
# n1: a workgroup handles 4 rows (1, 5 and 257 leave the last one partly empty); n2: lanes stride over b by 64.
_VJP_BASE = dict(kind="matern52", d=5, n1=5, n2=65, q=3, use_os=True, special=None)
_VJP_CASES = ([dict(kind=k) for k in ("rbf", "matern12", "matern32")] + [{}]
              + [dict(d=d) for d in (1, 4, 8, 9, 16, 17, 32)]
              + [dict(n1=n1) for n1 in (1, 257)]
              + [dict(n2=n2) for n2 in (1, 63, 64, 300)]
              + [dict(q=1), dict(use_os=False), dict(q=1, use_os=False)]
              # "same": X1 is X2 (the K_ZZ role); "dup": X2 holds rows of X1 and a duplicated row (r = 0 off the
              # diagonal); "near": a pair ~1e-4 ell apart (next to, not at, the Matern-1/2 r = 0 branch)
              + [dict(kind=k, special=s) for s in ("same", "dup", "near") for k in ("matern12", "matern32")]
              + [dict(kind="rbf", special="dup"), dict(special="same", n1=257, d=17)])
# fp32 "near" too: the oracle sees the rounded inputs, and the kernel forms x1 - x2 with at most one rounding (none,
# by Sterbenz, where the coordinates are within a factor 2) before its one scaling by 1 / ell: the pair's term carries
# a few roundings like any other
_VJP_PARAMS = [pytest.param(c, dt, id="%s-%s" % (_case_id(c), str(dt)[6:]))
               for c in _VJP_CASES for dt in (torch.float64, torch.float32)]


def _vjp_problem(d, n1, n2, q, use_os, special, seed):
    g = torch.Generator().manual_seed(seed)
    X1 = 2 * torch.rand(n1, d, generator=g, dtype=torch.float64) - 1
    X2 = 2 * torch.rand(n2, d, generator=g, dtype=torch.float64) - 1
    # lengthscales ~ sqrt(d): the scaled distances stay O(1) at every d (kernels neither all 1 nor all 0)
    ell = math.sqrt(d) * (0.3 + 0.5 * torch.rand(q, d, generator=g, dtype=torch.float64))
    osc = 0.5 + torch.rand(q, generator=g, dtype=torch.float64)
    if special == "same":
        X2, n2 = X1, n1
    elif special == "dup":
        k = min(3, n1)
        X2 = torch.cat([X1[:k], X2[:n2 - 2 * k - 1], X2[:1], X1[:k]])
        n2 = X2.shape[0]
    elif special == "near":
        X2[0] = X1[0] + 1e-4 * ell[0] / math.sqrt(d)           # scaled distance 1e-4 for latent 0
    G = torch.randn(q, n1, n2, generator=g, dtype=torch.float64)
    return X1, X2, ell, (osc if use_os else None), G


@pytest.mark.parametrize("case,dt", _VJP_PARAMS)
def test_kernel_vjp_against_autograd(eng, case, dt):
    """plmc_kernel_vjp (gX1, gEll, gOs) against autograd of sum_i <G_i, os_i k(X1, X2; ell_i)> in fp64
    (oracle/gp_math.py: kernel_vjp); the oracle is evaluated at the dt-rounded inputs.

    Bound: every output is a sum of terms G_ab dK_ab.  Each term is formed from the scaled differences (2 roundings),
    their squared sum (d additions), the kernel value / derivative factor (sqrt, exp and a polynomial: ~4 roundings at
    the O(1) distances of these problems) and 3-4 products, then accumulated in fp64.  So an a-priori c = 4 (d + 4)
    roundings per term bound the error of an output by c u sum_b |G_ab dK_ab|, with the sum of absolute terms from
    the oracle (oracle/gp_math.py: kernel_vjp_abs_terms).  fp32: u = 2^-24; fp64 is held to 1e-10 of the same sum."""
    c = {**_VJP_BASE, **case}
    okind, nu = KINDS[c["kind"]]
    X1, X2, ell, osc, G = _vjp_problem(c["d"], c["n1"], c["n2"], c["q"], c["use_os"], c["special"],
                                     seed=zlib.crc32(_case_id(case).encode()))
    X1, X2, ell, osc, G = _rounded(dt, X1, X2, ell, osc, G)
    if c["special"] == "same":
        X2 = X1
    f = lambda t: None if t is None else t.to(DEV, dt).contiguous()
    X1d = f(X1)
    X2d = X1d if c["special"] == "same" else f(X2)
    gX, gE, gO = eng.var.kernel_vjp(c["kind"], X1d, X2d, f(ell), f(osc), f(G))
    torch.cuda.synchronize()
    # without output scales the kernel still returns sum G k = d / d os at os = 1
    os_eff = osc if osc is not None else torch.ones(c["q"], dtype=torch.float64)
    wX, wE, wO = gm.kernel_vjp(okind, X1, X2, ell, os_eff, G, nu)
    tX, tE, tO = gm.kernel_vjp_abs_terms(okind, X1, X2, ell, os_eff, G, nu)
    tol = 1e-10 if dt == torch.float64 else 4 * (c["d"] + 4) * U32
    for name, got, want, terms in (("gX1", gX, wX, tX), ("gEll", gE, wE, tE), ("gOs", gO, wO, tO)):
        err = (got.cpu() - want).abs()
        bad = err > tol * terms
        assert not bool(bad.any()), (name, int(bad.sum()), float(err.max()), float((err / terms.clamp_min(1e-300)).max()))


def test_matern12_vjp_coincident_points_contribute_nothing(eng):
    """At r = 0 the Matern-1/2 derivative has no limit; the convention (gpytorch's clamp_min(1e-30).sqrt(), see the
    oracle's docstring) is a zero contribution.  X2 made only of copies of row 1 of X1: that row's gX1 must be exactly 0
    in both dtypes, and every output must equal the oracle's within the bound of test_kernel_vjp_against_autograd."""
    g = torch.Generator().manual_seed(4)
    d, q = 3, 2
    X1 = 2 * torch.rand(4, d, generator=g, dtype=torch.float64) - 1
    X2 = X1[1:2].repeat(70, 1)
    ell = 0.5 + torch.rand(q, d, generator=g, dtype=torch.float64)
    G = torch.randn(q, 4, 70, generator=g, dtype=torch.float64)
    ones = torch.ones(q, dtype=torch.float64)
    for dt in (torch.float64, torch.float32):
        A1, A2, E, Gr = _rounded(dt, X1, X2, ell, G)
        f = lambda t: t.to(DEV, dt).contiguous()
        gX, gE, gO = eng.var.kernel_vjp("matern12", f(A1), f(A2), f(E), None, f(Gr))
        torch.cuda.synchronize()
        wX, wE, wO = gm.kernel_vjp("matern", A1, A2, E, ones, Gr, 0.5)
        tX, tE, tO = gm.kernel_vjp_abs_terms("matern", A1, A2, E, ones, Gr, 0.5)
        assert float(wX[1].abs().max()) == 0.0
        assert float(gX[1].abs().max()) == 0.0, (dt, gX[1])
        tol = 1e-10 if dt == torch.float64 else 4 * (d + 4) * U32
        for got, want, terms in ((gX, wX, tX), (gE, wE, tE), (gO, wO, tO)):
            assert bool(((got.cpu() - want).abs() <= tol * terms).all()), (dt, got, want)


# ------------------------------------------------------------------------------------------------ dense LMC
def _lmc_problem(n, d, p, q, seed, full_sigma=True):
    g = torch.Generator().manual_seed(seed)
    X = 2 * torch.rand(n, d, generator=g, dtype=torch.float64) - 1
    Y = torch.randn(n, p, generator=g, dtype=torch.float64)
    ell = math.sqrt(d) * (0.3 + 0.5 * torch.rand(q, d, generator=g, dtype=torch.float64))
    osc = 0.5 + torch.rand(q, generator=g, dtype=torch.float64)
    F = torch.randn(q, p, 2, generator=g, dtype=torch.float64) / math.sqrt(2.0 * p)
    B = F @ F.transpose(-1, -2) + torch.diag_embed(0.1 + 0.3 * torch.rand(q, p, generator=g, dtype=torch.float64))
    S = torch.diag_embed(0.1 + 0.3 * torch.rand(p, generator=g, dtype=torch.float64))
    if full_sigma:
        Fn = 0.3 * torch.randn(p, p, generator=g, dtype=torch.float64)
        S = S + Fn @ Fn.T / p
    return X, Y, ell, osc, B, S


def _lmc_oracle(kind, X, Y, ell, osc, B, S):
    """log N(vec Y; 0, sum_i os_i K_i (x) B_i + I (x) S) and its gradient w.r.t. (ell, os, B, S, vec Y) by autograd."""
    okind, nu = KINDS[kind]
    n, p = Y.shape
    leaves = [t.detach().clone().requires_grad_(True) for t in (ell, osc, B, S, Y)]
    val = ld.lmc_exact_mll(okind, X, leaves[4], leaves[0], leaves[2], leaves[3], nu=nu, outputscale=leaves[1]) * (n * p)
    grads = torch.autograd.grad(val, leaves)
    return float(val.detach()), list(grads[:4]) + [grads[4].reshape(-1)]


def _lmc_run(eng, kind, X, Y, ell, osc, B, S, dt):
    f = lambda t: t.to(DEV, dt).contiguous()
    leaves = [f(t).requires_grad_(True) for t in (ell, osc, B, S, Y.reshape(-1))]
    lp = eng.lmc.lmc_exact_log_prob(kind, f(X), *leaves)
    lp.backward()
    torch.cuda.synchronize()
    return float(lp.detach()), [t.grad.detach().cpu().double() for t in leaves]


_GRAD_NAMES = ("ell", "oscale", "B", "Sigma", "y")

# Base: matern52, n = 37, d = 4, p = 3, q = 2, full Sigma (N = 111: one ragged tile).
_LMC_BASE = dict(kind="matern52", n=37, d=4, p=3, q=2, full=True)
_LMC_CASES = ([dict(kind=k) for k in ("rbf", "matern12", "matern32")] + [{}]
              + [dict(p=p) for p in (1, 5, 7, 16)]
              + [dict(d=d) for d in (1, 9, 17, 32)]                 # fp64: the GH = 8 walks of the gradient epilogue
              + [dict(q=1), dict(q=3), dict(full=False)]
              # N ~ 2100: 17 block rows, three groups of the sweep; the rows of a data point straddle tiles (p = 7)
              + [dict(n=700), dict(n=300, p=7, d=9, kind="matern12")])
_LMC_FP32 = [{}, dict(kind="matern12"), dict(p=7), dict(d=9), dict(d=17), dict(n=700), dict(n=300, p=7, d=9, kind="matern12")]


def _lmc_case(case):
    c = {**_LMC_BASE, **case}
    return c, _lmc_problem(c["n"], c["d"], c["p"], c["q"], seed=c["n"] + 7 * c["p"] + c["d"], full_sigma=c["full"])


@pytest.mark.parametrize("case", _LMC_CASES, ids=_case_id)
def test_dense_lmc_value_and_gradients_fp64(eng, case):
    """lmc_exact_log_prob (k_lmc_assemble, the sweep, k_lmc_kinv_grad + k_lmc_reduce), with output scales, against
    autograd of the dense oracle: value to 1e-10 relative, every gradient to 1e-8 of its largest entry."""
    c, (X, Y, ell, osc, B, S) = _lmc_case(case)
    ref, rgrads = _lmc_oracle(c["kind"], X, Y, ell, osc, B, S)
    val, grads = _lmc_run(eng, c["kind"], X, Y, ell, osc, B, S, torch.float64)
    assert abs(val - ref) <= 1e-10 * abs(ref), (val, ref)
    for name, got, want in zip(_GRAD_NAMES, grads, rgrads):
        err = float((got - want.reshape(got.shape)).abs().max())
        assert err <= 1e-8 * float(want.abs().max()), (name, err, float(want.abs().max()))


@pytest.mark.parametrize("case", _LMC_FP32, ids=_case_id)
def test_dense_lmc_fp32_split_and_mfma_paths(eng, case):
    """fp32 (plmc_lmc_kinv_grad_f32 included) against the fp64 oracle at the fp32-rounded inputs, with the pattern of
    test_split_engines_against_fp32_mfma_path: the default sweep (no eigenvalue bound: three bf16 planes in the bulk
    products) and PLMC_SPLIT=0 (fp32 MFMAs everywhere) both within the fp32 tolerance (value 1e-4 relative, gradients
    2e-3 of their largest entry), and the split path's error at most 2x the fp32-MFMA path's + 2e-6 (a few fp32 ulps)
    of the largest magnitude."""
    c, prob = _lmc_case(case)
    X, Y, ell, osc, B, S = _rounded(torch.float32, *prob)
    ref, rgrads = _lmc_oracle(c["kind"], X, Y, ell, osc, B, S)
    split = _lmc_run(eng, c["kind"], X, Y, ell, osc, B, S, torch.float32)
    with eng.hip.knob("PLMC_SPLIT", "0"):
        plain = _lmc_run(eng, c["kind"], X, Y, ell, osc, B, S, torch.float32)
    e_s, e_p = abs(split[0] - ref) / abs(ref), abs(plain[0] - ref) / abs(ref)
    assert e_s < 1e-4 and e_p < 1e-4, ("value", e_s, e_p)
    assert e_s < 2.0 * e_p + 2e-6, ("value", e_s, e_p)
    for name, got, base, want in zip(_GRAD_NAMES, split[1], plain[1], rgrads):
        want = want.reshape(got.shape)
        scale = float(want.abs().max())
        e_s, e_p = float((got - want).abs().max()) / scale, float((base - want).abs().max()) / scale
        assert e_s < 2e-3 and e_p < 2e-3, (name, e_s, e_p)
        assert e_s < 2.0 * e_p + 2e-6, (name, e_s, e_p)


@pytest.mark.parametrize("kind", list(KINDS))
def test_dense_lmc_p1_q1_is_the_exact_gp(eng, kind):
    """At p = 1, q = 1 the dense LMC system is the exact GP with outputscale os B and noise Sigma: value and gradients of
    lmc_exact_log_prob equal exact_latent_log_prob's (the exact-GP engine: other assembly, other gradient kernel) to fp64
    round-off, after the chain rule through os B."""
    X, Y, ell, osc, B, S = _lmc_problem(300, 3, 1, 1, seed=13)
    val, (g_ell, g_os, g_B, g_S, g_y) = _lmc_run(eng, kind, X, Y, ell, osc, B, S, torch.float64)
    f = lambda t: t.to(DEV).contiguous().requires_grad_(True)
    e_ell, e_os, e_nz, e_y = f(ell), f(osc * B.reshape(1)), f(S.reshape(1)), f(Y.reshape(1, -1))
    lp = eng.exact.exact_latent_log_prob(kind, X.to(DEV), e_ell, e_os, e_nz, e_y)
    lp.sum().backward()
    torch.cuda.synchronize()
    assert abs(val - float(lp.detach().sum())) <= 1e-11 * abs(val), (val, float(lp.detach().sum()))
    g_oe = e_os.grad.cpu()
    for name, got, want in (("ell", g_ell, e_ell.grad.cpu()), ("oscale", g_os, g_oe * B.reshape(1)),
                            ("B", g_B.reshape(1), g_oe * osc), ("Sigma", g_S.reshape(1), e_nz.grad.cpu()),
                            ("y", g_y, e_y.grad.cpu().reshape(-1))):
        err = float((got.reshape(want.shape) - want).abs().max())
        assert err <= 1e-10 * float(want.abs().max()), (name, err)


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("kind,p", [("matern52", 5), ("rbf", 3), ("matern12", 7), ("matern32", 1)])
def test_dense_lmc_posterior(eng, kind, p, dt):
    """lmc_posterior (k_lmc_cross into the augmented columns; ns p = 65, 39, 91, 13 columns: ragged against the 64-wide
    blocks) against the oracle's dense conditioning at the dt-rounded inputs; fp64 to 1e-9 of the largest mean / prior
    variance, fp32 to 2e-3 (the fp32 tolerance of the repository's solve-based checks)."""
    n, d, q, ns = 60, 3, 2, 13
    X, Y, ell, osc, B, S = _lmc_problem(n, d, p, q, seed=p + 31)
    Xs = 2 * torch.rand(ns, d, generator=torch.Generator().manual_seed(p), dtype=torch.float64) - 1
    X, Y, ell, osc, B, S, Xs = _rounded(dt, X, Y, ell, osc, B, S, Xs)
    okind, nu = KINDS[kind]
    mu, var = ld.lmc_posterior(okind, X, Y, Xs, ell, B, S, nu=nu, outputscale=osc)
    f = lambda t: t.to(DEV, dt).contiguous()
    m, v = eng.lmc.lmc_posterior(kind, f(X), f(ell), f(osc), f(B), f(S), f(Y.reshape(-1)), f(Xs))
    torch.cuda.synchronize()
    tol = 1e-9 if dt == torch.float64 else 2e-3
    prior = float((osc[:, None] * torch.diagonal(B, dim1=-2, dim2=-1)).sum(0).max())
    assert float((m.cpu().double() - mu).abs().max()) <= tol * float(mu.abs().max())
    assert float((v.cpu().double() - var).abs().max()) <= tol * prior


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("kind,p", [("matern52", 4), ("matern12", 5), ("rbf", 7)])
def test_dense_lmc_loo(eng, kind, p, dt):
    """lmc_loo (plmc_w_diag, fp32 included) against the dense formulas sigma2 = 1 / diag(C^-1), r = C^-1 y sigma2 on the
    oracle's covariance at the dt-rounded inputs; fp64 to 1e-8 of the largest entry, fp32 to 2e-3."""
    n, d, q = 50, 3, 2
    X, Y, ell, osc, B, S = _lmc_problem(n, d, p, q, seed=p + 41)
    X, Y, ell, osc, B, S = _rounded(dt, X, Y, ell, osc, B, S)
    okind, nu = KINDS[kind]
    C = ld.lmc_covariance(okind, X, ell, B, S, nu, outputscale=osc)
    Kinv = torch.cholesky_inverse(torch.linalg.cholesky(C))
    s2_ref = 1.0 / torch.diagonal(Kinv)
    r_ref = (Kinv @ Y.reshape(-1)) * s2_ref
    f = lambda t: t.to(DEV, dt).contiguous()
    s2, r = eng.lmc.lmc_loo(kind, f(X), f(ell), f(osc), f(B), f(S), f(Y.reshape(-1)))
    torch.cuda.synchronize()
    tol = 1e-8 if dt == torch.float64 else 2e-3
    assert float((s2.cpu().double() - s2_ref).abs().max()) <= tol * float(s2_ref.abs().max())
    assert float((r.cpu().double() - r_ref).abs().max()) <= tol * float(r_ref.abs().max())


# ------------------------------------------------------------------------------------------------ LDS limits
# Restated from csrc/lmc.hip (lmc_stage_elems, lmc_nacc and the LDS plans of lmc_assemble_impl / lmc_kinv_grad_impl).
NB, NTHREADS, BK = 128, 256, 16
LDS_CAP = 150 * 1024
LMC_PARK_ELEMS = 4 * NTHREADS * 4
LMC_TABLE_INTS = 4 * NB


def _stage_elems(p, q, d):
    return 2 * NB * (d + 1) + q * d + q + q * p * p + p * p


def _nacc(p, q, d):
    return q * p * p + q * d + q + p * p


def _assemble_fits(p, q, d, size):
    return _stage_elems(p, q, d) * size <= LDS_CAP


def _kinv_grad_fits(p, q, d, size):
    epi = (_stage_elems(p, q, d) + 2 * NB) * size + 8 + _nacc(p, q, d) * 8 + LMC_PARK_ELEMS * size + LMC_TABLE_INTS * 4
    return max(epi, 2 * 2 * BK * 144 * size) <= LDS_CAP


def _largest_p(fits, q, d, size):
    p = 1
    while fits(p + 1, q, d, size):
        p += 1
    return p


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["float64", "float32"])
def test_gradient_kernel_lds_limit(eng, dt):
    """The largest p whose accumulator tables fit k_lmc_kinv_grad's LDS (q = 2, d = 8; 45 in fp64, 58 in fp32) gives
    the oracle's value and gradients; p + 1, still within the assembly's budget, is refused with the library's
    message before the gradient kernel launches."""
    q, d, size = 2, 8, torch.finfo(dt).bits // 8
    assert int(eng.hip.lib().cdll.plmc_lmc_grad_len(5, q, d)) == _nacc(5, q, d)
    p = _largest_p(_kinv_grad_fits, q, d, size)
    assert _assemble_fits(p + 1, q, d, size)
    X, Y, ell, osc, B, S = _rounded(dt, *_lmc_problem(2100 // p, d, p, q, seed=p))
    ref, rgrads = _lmc_oracle("matern52", X, Y, ell, osc, B, S)
    val, grads = _lmc_run(eng, "matern52", X, Y, ell, osc, B, S, dt)
    vtol, gtol = (1e-10, 1e-8) if dt == torch.float64 else (1e-4, 2e-3)
    assert abs(val - ref) <= vtol * abs(ref), (p, val, ref)
    for name, got, want in zip(_GRAD_NAMES, grads, rgrads):
        err = float((got - want.reshape(got.shape)).abs().max())
        assert err <= gtol * float(want.abs().max()), (p, name, err)
    X, Y, ell, osc, B, S = _lmc_problem(3, d, p + 1, q, seed=1)
    with pytest.raises(RuntimeError, match="too large for the LDS accumulators"):
        _lmc_run(eng, "matern52", X, Y, ell, osc, B, S, dt)


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["float64", "float32"])
def test_assembly_lds_limit(eng, dt):
    """The largest p whose parameter tables fit k_lmc_assemble's LDS (q = 2, d = 8; 75 in fp64, 109 in fp32): value (no
    gradient) against the oracle; p + 1 is refused with the library's message."""
    q, d, size = 2, 8, torch.finfo(dt).bits // 8
    p = _largest_p(_assemble_fits, q, d, size)
    X, Y, ell, osc, B, S = _rounded(dt, *_lmc_problem(2, d, p, q, seed=p))
    ref = float(ld.lmc_exact_mll("rbf", X, Y, ell, B, S, outputscale=osc)) * Y.numel()
    f = lambda t: t.to(DEV, dt).contiguous()
    val = float(eng.lmc.lmc_exact_log_prob("rbf", f(X), f(ell), f(osc), f(B), f(S), f(Y.reshape(-1))))
    assert abs(val - ref) <= (1e-10 if dt == torch.float64 else 1e-4) * abs(ref), (p, val, ref)
    X, Y, ell, osc, B, S = _lmc_problem(2, d, p + 1, q, seed=1)
    with pytest.raises(RuntimeError, match="too large for the LDS parameter tables"):
        eng.lmc.lmc_exact_log_prob("rbf", f(X), f(ell), f(osc), f(B), f(S), f(Y.reshape(-1)))


def test_sizes_and_kinds_outside_the_kernels_are_refused(eng):
    """d = 33 (above plmc_max_dim()) and kind `spline` (the dense-LMC and VJP kernels take kinds 0-3 only) raise the
    library's error from both entry points."""
    f = lambda t: t.to(DEV).contiguous()
    for d, kind, msg in ((33, "matern52", "bad sizes"), (3, "spline", "unknown kernel kind")):
        X, Y, ell, osc, B, S = _lmc_problem(20, d, 2, 2, seed=d)
        with pytest.raises(RuntimeError, match=msg):
            _lmc_run(eng, kind, X, Y, ell, osc, B, S, torch.float64)
        X1, X2, ell, osc, G = _vjp_problem(d, 5, 7, 2, True, None, seed=d)
        with pytest.raises(RuntimeError, match=msg):
            eng.var.kernel_vjp(kind, f(X1), f(X2), f(ell), f(osc), f(G))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ exact posterior
@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_exact_posterior_all_kinds(eng, kind, dt):
    """exact_posterior (plmc_assemble_cross into the augmented columns) for every kind against dense conditioning at the
    dt-rounded inputs: fp64 as test_posterior_fp64, fp32 to 2e-3 of the largest mean / prior variance."""
    n, d, q, ns = 300, 3, 2, 77
    g = torch.Generator().manual_seed(3)
    X = 2 * torch.rand(n, d, generator=g, dtype=torch.float64) - 1
    y = torch.randn(q, n, generator=g, dtype=torch.float64)
    ell = 0.3 + 0.5 * torch.rand(q, d, generator=g, dtype=torch.float64)
    noise = 0.05 + 0.5 * torch.rand(q, generator=g, dtype=torch.float64)
    osc = 0.5 + torch.rand(q, generator=g, dtype=torch.float64)
    Xs = 2 * torch.rand(ns, d, generator=g, dtype=torch.float64) - 1
    X, y, ell, noise, osc, Xs = _rounded(dt, X, y, ell, noise, osc, Xs)
    okind, nu = KINDS[kind]
    mu, cov = gm.exact_gp_posterior(okind, X, ell, noise, y, Xs, osc, nu)
    var = torch.diagonal(cov, dim1=-2, dim2=-1)
    f = lambda t: t.to(DEV, dt).contiguous()
    m1, v1 = eng.exact.exact_posterior(kind, f(X), f(ell), f(osc), f(noise), f(y), f(Xs))
    torch.cuda.synchronize()
    m1, v1 = m1.cpu().double(), v1.cpu().double()
    if dt == torch.float64:
        assert torch.allclose(m1, mu, rtol=1e-8, atol=1e-10)
        assert torch.allclose(v1, var, rtol=1e-7, atol=1e-10)
    else:
        assert float((m1 - mu).abs().max()) <= 2e-3 * float(mu.abs().max())
        assert float((v1 - var).abs().max()) <= 2e-3 * float(osc.max())
