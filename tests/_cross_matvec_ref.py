"""fp64 references and a-priori bounds of the products with a cross-covariance that is never written,
    plmc_cross_matvec   Out[l, s, c] = sum_{i < n} k_l(xs_s, x_i) V[l, i, c]
    plmc_rff_matvec     Out[l, s, c] = scale_l sum_{j < m} cos(2 pi (freq_lj . xs_s + phase_lj)) Wt[l, j, c]
and of a pathwise posterior draw built from them (paths_dense).  TEST INFRASTRUCTURE ONLY: plain torch on the CPU, nothing from the
package.  K(X*, X) comes from the dense helpers the families' own tests use (oracle.gp_math, _inducing_dense, _sm_dense,
_periodic_dense, _rq_dense, _lper_dense, _sum_dense, _dot_dense); every input is rounded to fp32, so both element types see the same
values and the reference is the exact result of those inputs up to fp64 rounding.

The error contract of one output element, u = 2^-24 (fp32) / 2^-53 (fp64):
    |Out - exact| <= sum_i b_F |V_ic|  +  u |exact|  +  (n + 4) 2^-53 sum_i |k_i V_ic|
b_F: the per-entry bound the family's own assembly test applies to plmc_assemble_cross* (nothing new is derived for the values):
    stationary kinds, spline   6e-7 os                                          tests/test_gpu_engine.py
    additive table             sum_g 6e-7 os_g + (G - 1) 2^-24 sum_g os_g       the members' bounds and the additions, as _sum_dense adds them
    spectral mixture           32 d 2^-24 sum_m w_m                             tests/test_gpu_sm_kernel.py
    periodic                   24 d 2^-24 os (1 + 1 / min_k ell_k)              tests/test_gpu_periodic_kernel.py
    rational quadratic         (d + 8) 2^-24 os                                 _rq_dense.fp32_bound
    locally periodic           _lper_dense.fp32_bound
    sum of families            _sum_dense.fp32_bound
    dot product                _dot_dense.fp32_bound (per pair)
fp64: the per-entry tolerance of the same tests, 1e-12 (|k| + scale) (sum of families: 1e-12 |k|; dot product: 1e-12 os S^P).
One cosine of plmc_rff_matvec: 4 (d + 2) u whatever the phase, in the place of b_F."""
import math

import torch

import _dot_dense
import _input_grad_dense as igd
import _lper_dense
import _rq_dense
import _sum_dense

U = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}
U32 = 2.0 ** -24
SEGMENT = 256                                      # rows of one segment of the kernel's fixed summation order, n <= 64 * 256
SUM_MEMBERS = ("matern52", "periodic", "rq", "locally_periodic")
FAMILIES = tuple(igd.STATIONARY) + ("spline", "add_disjoint", "add_overlap", "sm3", "periodic", "rq", "locally_periodic", "sum", "linear",
                                    "poly3")
GROUPS = {1: [[0], [0]], 3: [[0, 1], [2]], 8: [[0, 1, 2, 3], [4, 5, 6, 7]], 16: [[0, 3, 4, 7], [8, 15], [2, 9], list(range(16))],
          32: [list(range(16)), list(range(16, 32)), [3, 4, 20, 31], [8, 15, 16, 17]]}


def _f32(t):
    return None if t is None else t.float().double()


class Problem:
    """kind, ell, oscale as projectedlmc._engine takes them (fp64, CPU), the dense callable K(Xa, Xb) -> (q, na, nb) and
    value_bound(Xa, Xb, dtype) -> b_F broadcastable to (q, na, nb)."""


def _scale_bound(p, rel32, scale):
    """b_F = rel32 * scale in fp32, 1e-12 (|k| + scale) in fp64; scale (q)."""
    def bound(Xa, Xb, dtype):
        if dtype == torch.float32:
            return (rel32 * scale)[:, None, None]
        return 1e-12 * (p.K(Xa, Xb).abs() + scale[:, None, None])
    return bound


def problem(family, d, q, seed, use_os=True):
    g = torch.Generator().manual_seed(seed + 77)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    one = torch.ones(q, dtype=torch.float64)
    if family == "spline":
        from oracle import gp_math as gm
        p = Problem()
        p.family, p.kind, p.d, p.q = family, "spline", d, q
        p.ell, p.oscale = torch.ones(q, d, dtype=torch.float64), (_f32(0.5 + rnd(q)) if use_os else None)
        p.K = lambda Xa, Xb: gm.kernel_matrix("spline", Xa, Xb, p.ell, p.oscale)
        p.value_bound = _scale_bound(p, 6e-7, one if p.oscale is None else p.oscale)
        return p
    if family == "sum":
        p = Problem()
        members = SUM_MEMBERS
        table, os_ = _sum_dense.make_table(members, d, q, seed)
        table, os_ = _f32(table), _f32(os_)
        p.family, p.kind, p.d, p.q, p.members = family, "sum(%s)" % ",".join(members), d, q, members
        p.ell, p.oscale = table, os_
        p.K = lambda Xa, Xb: _sum_dense.sum_kernel(members, Xa, Xb, table, os_)
        p.value_bound = lambda Xa, Xb, dtype: (_sum_dense.fp32_bound(members, d, table, os_) if dtype == torch.float32
                                               else 1e-12 * p.K(Xa, Xb).abs())
        return p
    if family in ("linear", "poly3"):
        p = Problem()
        P = 1 if family == "linear" else 3
        v, c = _f32(0.2 + rnd(q, d)), _f32(0.1 + rnd(q))
        os_ = _f32(0.5 + rnd(q)) if use_os else None
        p.family, p.kind, p.d, p.q = family, family, d, q
        p.ell, p.oscale = torch.cat([v, c[:, None]], 1), os_
        p.K = lambda Xa, Xb: _dot_dense.dot_kernel(Xa, Xb, v, c, P, os_)
        osr = one if os_ is None else os_
        p.value_bound = lambda Xa, Xb, dtype: (_dot_dense.fp32_bound(Xa, Xb, v, c, P, os_) if dtype == torch.float32 else
                                               1e-12 * osr[:, None, None] * _dot_dense._ipow(_dot_dense.dot_S(Xa, Xb, v, c), P) + 1e-300)
        return p
    groups = GROUPS.get(d) if family.startswith("add_") else None
    if family == "add_overlap" and d == 3:
        groups = [[0, 1], [1, 2]]
    p = igd.problem(family, d, q, seed, use_os, groups=groups)
    osr = one if p.oscale is None else p.oscale
    if family in igd.STATIONARY:
        p.value_bound = _scale_bound(p, 6e-7, osr)
    elif family.startswith("add_"):
        G = p.ell.shape[1]
        tot = osr.sum(-1) if p.oscale is not None else G * one
        bnd32 = 6e-7 * tot + (G - 1) * U32 * tot
        p.value_bound = lambda Xa, Xb, dtype: (bnd32[:, None, None] if dtype == torch.float32
                                               else 1e-12 * (p.K(Xa, Xb).abs() + tot[:, None, None]))
    elif family.startswith("sm"):
        w = p.oscale.sum(-1) if p.oscale is not None else p.ell.shape[2] * one
        p.value_bound = _scale_bound(p, 32 * d * U32, w)
    elif family == "periodic":
        p.value_bound = _scale_bound(p, 24 * d * U32 * (1.0 + 1.0 / p.ell[:, 0].min(-1)[0]), osr)
    elif family == "rq":
        p.value_bound = _scale_bound(p, (d + 8) * U32, osr)
    elif family == "locally_periodic":
        b32 = _lper_dense.fp32_bound(d, p.ell[:, 0], osr)
        p.value_bound = lambda Xa, Xb, dtype: b32 if dtype == torch.float32 else 1e-12 * (p.K(Xa, Xb).abs() + osr[:, None, None])
    else:
        raise ValueError(family)
    return p


def inputs(family, n, ns, d, seed):
    """(X (n, d), Xs (ns, d)), fp32-representable: [-1, 1]^d; the spline lives on x >= 0 and is kept O(1): [0, 1 / 2]^d."""
    g = torch.Generator().manual_seed(seed + 1000)
    X, Xs = torch.rand(n, d, generator=g, dtype=torch.float64), torch.rand(ns, d, generator=g, dtype=torch.float64)
    if family == "spline":
        return _f32(0.5 * X), _f32(0.5 * Xs)
    return _f32(2 * X - 1), _f32(2 * Xs - 1)


def columns(n, r, q, seed):
    """V (q, n, r), fp32-representable, signs mixed."""
    g = torch.Generator().manual_seed(seed + 2000)
    return _f32(torch.randn(q, n, r, generator=g, dtype=torch.float64))


def v_buffer(V, rows, ldv, dtype):
    """(q, rows, ldv) of `dtype`: V in [:, :n, :r], NaN in the rows from n on and in the columns from r up to the leading dimension."""
    q, n, r = V.shape
    buf = torch.full((q, rows, ldv), float("nan"), dtype=dtype)
    buf[:, :n, :r] = V.to(dtype)
    return buf


def reference(p, Xs, X, V, dtype):
    """(exact, bound), (q, ns, r) fp64 each."""
    n = X.shape[0]
    K = p.K(Xs, X)                                                     # (q, ns, n)
    bF = p.value_bound(Xs, X, dtype).expand(K.shape)
    exact = K @ V
    bound = bF @ V.abs() + U[dtype] * exact.abs() + (n + 4) * 2.0 ** -53 * (K.abs() @ V.abs())
    return exact, bound


def violations(got, exact, bound):
    """Elements outside the bound (NaN counts)."""
    return int((~((got.double() - exact).abs() <= bound)).sum())


def worst_share(got, exact, bound):
    return float(((got.double() - exact).abs() / bound).max())


def cpu_product(p, Xs, X, Vbuf, n, r, ldv, dtype, mutate=None):
    """The product as a correct kernel forms it, on the CPU: the fp64 value of every pair rounded to the element type, its products with
    V and the sums in fp64, one rounding -- or with one of the mistakes MUTATIONS names.  Vbuf: the (q, rows, ldv) buffer the kernel
    would get."""
    q = Vbuf.shape[0]
    K = p.K(Xs, X)
    if mutate == "no_oscale":
        K = K / p.oscale[:, None, None]
    K = K.to(dtype).double()
    flat = Vbuf.reshape(q, -1).double()
    step = r if mutate == "ldv_as_r" else ldv
    idx = torch.arange(n)[:, None] * step + torch.arange(r)[None, :]
    V = flat[:, idx]                                                   # (q, n, r)
    rows = n - 1 if mutate == "drop_last_row" else n
    out = torch.zeros(q, Xs.shape[0], r, dtype=torch.float64)
    for s0 in range(0, rows, SEGMENT):
        part = K[:, :, s0:min(s0 + SEGMENT, rows)] @ V[:, s0:min(s0 + SEGMENT, rows)]
        out = out + part
        if mutate == "partial_twice" and s0 == SEGMENT:
            out = out + part
    return out.to(dtype)


MUTATIONS = ("drop_last_row", "no_oscale", "ldv_as_r", "partial_twice")


# ---------------------------------------------------------------------------------------------- random Fourier features
def rff_problem(d, m, q, r, seed, max_rev):
    """freq (q, m, d), phase (q, m), Wt (q, m, r), scale (q), fp32-representable; the phases freq . x of points in [-1, 1]^d run from 0 up
    to about max_rev revolutions (feature 0 has frequency 0; the last one the largest)."""
    g = torch.Generator().manual_seed(seed + 3000)
    amp = torch.linspace(0.0, 1.0, m, dtype=torch.float64) if m > 1 else torch.ones(1, dtype=torch.float64)
    freq = (2 * torch.rand(q, m, d, generator=g, dtype=torch.float64) - 1) * amp[None, :, None] * (max_rev / d)
    freq[:, m - 1] = max_rev / d                                       # x = (1, ..., 1) reaches max_rev there
    phase = torch.rand(q, m, generator=g, dtype=torch.float64)
    Wt = torch.randn(q, m, r, generator=g, dtype=torch.float64)
    scale = 0.5 + torch.rand(q, generator=g, dtype=torch.float64)
    return _f32(freq), _f32(phase), _f32(Wt), _f32(scale)


def rff_features(freq, phase, Xs):
    """cos(2 pi (freq . xs + phase)), (q, ns, m) fp64, accurate at any phase: the products of fp32-representable numbers are exact in
    fp64, each is reduced to its fraction exactly, and only the fractions are added."""
    t = freq[:, None, :, :] * Xs[None, :, None, :]                      # (q, ns, m, d), exact
    frac = (t - torch.round(t)).sum(-1) + (phase - torch.round(phase))[:, None, :]
    return torch.cos(2.0 * math.pi * (frac - torch.round(frac)))


def rff_reference(freq, phase, Xs, Wt, scale, dtype):
    """(exact, bound), (q, ns, r) fp64 each: one cosine within 4 (d + 2) u, then the reduction terms of the contract above."""
    d, m = freq.shape[-1], freq.shape[1]
    Phi = rff_features(freq, phase, Xs)
    sc = torch.ones(freq.shape[0], dtype=torch.float64) if scale is None else scale
    exact = sc[:, None, None] * (Phi @ Wt)
    absW = torch.ones_like(Phi) @ Wt.abs()
    bound = sc.abs()[:, None, None] * (4 * (d + 2) * U[dtype] * absW + (m + 4) * 2.0 ** -53 * (Phi.abs() @ Wt.abs())) + U[dtype] * exact.abs()
    return exact, bound


def rff_cpu_product(freq, phase, Xs, Wt, scale, dtype, mutate=None):
    """The feature product with every cosine rounded to the element type; mutate = "unreduced_phase": the phase formed in the element
    type without reduction, fl(sum_k fl(f_k x_k) + b), and handed to the cosine."""
    if mutate == "unreduced_phase":
        f, x, b = freq.to(dtype), Xs.to(dtype), phase.to(dtype)
        arg = b[:, None, :].expand(freq.shape[0], Xs.shape[0], freq.shape[1]).clone()
        for k in range(freq.shape[-1]):
            arg = arg + f[:, None, :, k] * x[None, :, None, k]
        Phi = torch.cos((2.0 * math.pi) * arg.double()).to(dtype).double()
    else:
        Phi = rff_features(freq, phase, Xs).to(dtype).double()
    sc = torch.ones(freq.shape[0], dtype=torch.float64) if scale is None else scale
    return (sc[:, None, None] * (Phi @ Wt)).to(dtype)


# ---------------------------------------------------------------------------------------------- pathwise posterior draws
def paths_dense(K, X, resid, noise, freq, phase, feature_scale, w, eps, Xs):
    """Matheron's rule in fp64 from a path's stored tensors, per latent and WITHOUT the prior mean:
        f(xs) = Phi(xs) W + K(xs, X) (K(X, X) + noise I)^-1 (resid - Phi(X) W - eps),     W = (feature_scale * w)^T
    K: dense callable (q, na, nb); X (n, d); resid = y - m(X) (q, n); noise (q); freq (q, M, d), phase (q, M) in revolutions;
    feature_scale (q, M); w (P, q, M); eps (P, q, n); Xs (ns, d)  ->  (q, ns, P)."""
    n = X.shape[0]
    Wt = (w * feature_scale[None]).permute(1, 2, 0)                    # (q, M, P)
    fX = rff_features(freq, phase, X) @ Wt                             # (q, n, P)
    Khat = K(X, X) + noise[:, None, None] * torch.eye(n, dtype=torch.float64)
    v = torch.linalg.solve(Khat, resid[:, :, None] - fX - eps.permute(1, 2, 0))
    return rff_features(freq, phase, Xs) @ Wt + K(Xs, X) @ v
