"""fp64 references, tolerances and CPU restatements of the input derivatives of the fused cross-covariance products,
    plmc_cross_matvec_dx   Jx[l, s, k] = sum_{i < n} w_si d k_l(xs_s, x_i) / d xs_s[k],          w_si = sum_c G[l, s, c] V[l, i, c]
    plmc_rff_matvec_dx     Jx[l, s, k] = -2 pi scale_l sum_{j < m} sin(2 pi (f_lj . xs_s + b_lj)) f_ljk w_sj,   w_sj = sum_c G[l, s, c] Wt[l, j, c]
TEST INFRASTRUCTURE ONLY: plain torch on the CPU, nothing from the package.

Kernel families: _posterior_dx_dense.posterior_dx_ref with B = -w / 2 -- its Jv is then sum_i w_si d k, its Tv the sum of absolute terms
sum_i |w_si| |d k| -- on the problems and inputs of _posterior_dx_dense.  The tolerance per element is relative to that sum:
    fp64  1e-10
    fp32  TOL32 2^-24, the constants of tests/test_gpu_posterior_dx_kernel.py: 4 (d + 4) for the stationary kinds and their table, that
          file's TOL32 for rq / periodic / locally periodic / sm.  The unit derivative is the same code with g = 1 and the weights are
          fp64, so those constants apply unchanged.
Features: the dense product of -2 pi sin(.) f with the phase reduced exactly (products of fp32-representable numbers are exact in fp64),
and the bound
    |scale| 2 pi [4 (d + 2) u sum_j |f_jk| |w_sj| + (m + 4) 2^-53 sum_j |sin_j f_jk w_sj|]
one sine within 4 (d + 2) u whatever the phase (the cosine's argument of 7.12 word for word, |d sin / d phase| <= 2 pi)."""
import math

import torch

import _cross_matvec_ref as cm
import _posterior_dx_dense as pdd

U = cm.U
U32 = 2.0 ** -24
SEGMENT = cm.SEGMENT
TOL32 = {"rq": 8.0, "periodic": 4.0, "locally_periodic": 8.0, "sm": 8.0}          # tests/test_gpu_posterior_dx_kernel.py


def group(family):
    return "sm" if family.startswith("sm") else family if family in TOL32 else "stationary"


def tolerance(family, d, dtype):
    """The factor of the sum of absolute terms one element may be off by."""
    if dtype == torch.float64:
        return 1e-10
    g = group(family)
    return (4 * (d + 4) if g == "stationary" else TOL32[g]) * U32


def weights(V, G):
    """w (q, n, ns) = sum_c G[l, s, c] V[l, i, c]; G None: the one column of V for every test point."""
    if G is None:
        return None
    return torch.einsum("qsc,qic->qis", G, V)


def operands(n, ns, r, q, seed, with_g=True):
    """V (q, n, r) and G (q, ns, r) | None, fp32-representable, signs mixed."""
    g = torch.Generator().manual_seed(seed + 5000)
    V = torch.randn(q, n, r, generator=g, dtype=torch.float64).float().double()
    G = torch.randn(q, ns, r, generator=g, dtype=torch.float64).float().double() if with_g else None
    return V, G


def buffers(V, G, dtype, pad_rows=5, ldv=None, pad_points=3):
    """(Vbuf (q, n + pad_rows, ldv), Gbuf (q ns r + pad_points r) | None) of `dtype` with NaN wherever the kernel must not read: the rows of V
    from n on, its columns from r up to the leading dimension, G past its q ns r elements."""
    q, n, r = V.shape
    Vbuf = cm.v_buffer(V, n + pad_rows, r + 2 if ldv is None else ldv, dtype)
    if G is None:
        return Vbuf, None
    Gbuf = torch.full((G.numel() + pad_points * r,), float("nan"), dtype=dtype)
    Gbuf[:G.numel()] = G.to(dtype).reshape(-1)
    return Vbuf, Gbuf


def reference(K, X, Xs, V, G):
    """(Jx, T), (q, ns, d) fp64 each: the value and the sum of absolute terms behind it."""
    q, n, _ = V.shape
    ns = Xs.shape[0]
    w = weights(V, G) if G is not None else V[:, :, :1].expand(q, n, ns)
    _, Jv, _, Tv = pdd.posterior_dx_ref(K, X, Xs, torch.zeros(q, n, dtype=torch.float64), -0.5 * w)
    return Jv, Tv


def violations(got, want, terms, tol):
    """Elements outside tol * (sum of absolute terms) (NaN counts)."""
    return int((~((got.double() - want).abs() <= tol * terms)).sum())


def worst_ratio(got, want, terms, unit=U32):
    live = terms > 0
    return float(((got.double() - want).abs()[live] / (unit * terms[live])).max()) if bool(live.any()) else 0.0


def pair_derivatives(K, X, Xs):
    """d k_l(xs_s, x_i) / d xs_s[k], (q, ns, n, d) fp64: one forward-mode pass per dimension."""
    ns, d = Xs.shape
    out = []
    for k in range(d):
        e = torch.zeros(ns, d, dtype=torch.float64)
        e[:, k] = 1.0
        out.append(torch.func.jvp(lambda Xa: K(Xa, X.detach()), (Xs.detach().clone(),), (e,))[1])
    return torch.stack(out, -1)


def segment_sum(terms, acc_dtype=torch.float64, rows=None):
    """terms (..., n, d) summed over n in the kernel's order as far as a CPU states it: segments of SEGMENT rows, added in order."""
    n = terms.shape[-2] if rows is None else rows
    out = torch.zeros(terms.shape[:-2] + terms.shape[-1:], dtype=acc_dtype)
    for s0 in range(0, n, SEGMENT):
        seg = torch.zeros_like(out)
        for i in range(s0, min(s0 + SEGMENT, n)):
            seg = seg + terms[..., i, :].to(acc_dtype)
        out = out + seg
    return out.double()


MUTATIONS = ("fp32_sums", "drop_last_row", "swap_g_columns")


def cpu_product(K, X, Xs, Vbuf, Gbuf, n, r, dtype, mutate=None):
    """Jx as a correct kernel forms it, on the CPU: the unit derivative of every pair rounded to the element type, the weights from the
    buffers the kernel would get (fp64 sums over the columns in order), their products and the sums in fp64 in segment order -- or with one
    of the mistakes MUTATIONS names."""
    q, ldv, ns = Vbuf.shape[0], Vbuf.shape[2], Xs.shape[0]
    dK = pair_derivatives(K, X, Xs).to(dtype).double()                 # (q, ns, n, d)
    V = Vbuf[:, :n, :r].double()
    if Gbuf is None:
        w = V[:, :, :1].expand(q, n, ns)
    else:
        G = Gbuf[:q * ns * r].reshape(q, ns, r).double()
        if mutate == "swap_g_columns":
            G = G.flip(-1)
        w = torch.zeros(q, n, ns, dtype=torch.float64)
        for c in range(r):
            w = w + G[:, None, :, c] * V[:, :, None, c]
    terms = w.transpose(1, 2)[..., None] * dK
    return segment_sum(terms, torch.float32 if mutate == "fp32_sums" else torch.float64, n - 1 if mutate == "drop_last_row" else None)


# ---------------------------------------------------------------------------------------------- random Fourier features
def rff_fraction(freq, phase, Xs):
    """The phase freq . xs + phase in revolutions brought into [-1/2, 1/2], (q, ns, m) fp64, exact up to the last additions."""
    t = freq[:, None, :, :] * Xs[None, :, None, :]                      # (q, ns, m, d), exact
    frac = (t - torch.round(t)).sum(-1) + (phase - torch.round(phase))[:, None, :]
    return frac - torch.round(frac)


def rff_reference(freq, phase, Xs, Wt, G, scale, dtype):
    """(exact, bound), (q, ns, d) fp64 each."""
    q, m, d = freq.shape
    ns = Xs.shape[0]
    sn = torch.sin(2.0 * math.pi * rff_fraction(freq, phase, Xs))       # (q, ns, m)
    w = torch.einsum("qsc,qjc->qsj", G, Wt) if G is not None else Wt[:, None, :, 0].expand(q, ns, m)
    sc = torch.ones(q, dtype=torch.float64) if scale is None else scale
    exact = -2.0 * math.pi * sc[:, None, None] * torch.einsum("qsj,qjk->qsk", sn * w, freq)
    absfw = torch.einsum("qsj,qjk->qsk", w.abs(), freq.abs())
    terms = torch.einsum("qsj,qjk->qsk", (sn * w).abs(), freq.abs())
    bound = sc.abs()[:, None, None] * 2.0 * math.pi * (4 * (d + 2) * U[dtype] * absfw + (m + 4) * 2.0 ** -53 * terms)
    return exact, bound


def rff_cpu_product(freq, phase, Xs, Wt, G, scale, dtype, mutate=None):
    """The feature derivative with every sine rounded to the element type, products and sums fp64; mutate = "unreduced_phase": the phase
    formed in the element type without reduction, fl(sum_k fl(f_k x_k) + b), and handed to the sine."""
    q, m, d = freq.shape
    ns = Xs.shape[0]
    if mutate == "unreduced_phase":
        f, x, b = freq.to(dtype), Xs.to(dtype), phase.to(dtype)
        arg = b[:, None, :].expand(q, ns, m).clone()
        for k in range(d):
            arg = arg + f[:, None, :, k] * x[None, :, None, k]
        sn = torch.sin((2.0 * math.pi) * arg.double()).to(dtype).double()
    else:
        sn = torch.sin(2.0 * math.pi * rff_fraction(freq, phase, Xs)).to(dtype).double()
    w = torch.einsum("qsc,qjc->qsj", G, Wt) if G is not None else Wt[:, None, :, 0].expand(q, ns, m)
    sc = torch.ones(q, dtype=torch.float64) if scale is None else scale
    return -2.0 * math.pi * sc[:, None, None] * torch.einsum("qsj,qjk->qsk", sn * w, freq)


def rff_violations(got, exact, bound):
    return int((~((got.double() - exact).abs() <= bound)).sum())


# ---------------------------------------------------------------------------------------------- pathwise posterior draws
def paths_latents(K, X, freq, phase, feature_scale, w, v, Xs):
    """A path's latent values from its stored tensors, fp64 and differentiable in Xs: Phi(xs) W + K(xs, X) v, W = (feature_scale * w)^T,
    v (q, n, P) the object's own solved weights (so the conditioning of the solve does not enter) -> (q, ns, P)."""
    Wt = (w * feature_scale[None]).permute(1, 2, 0)                    # (q, M, P)
    return cm.rff_features(freq, phase, Xs) @ Wt + K(Xs, X) @ v
