"""References and the bound of the reductions the host layer calls around the sweep: plmc_posterior_moments, plmc_mix_posterior
(csrc/posterior.hip), plmc_extract_col, plmc_wt_matvec, plmc_w_diag (csrc/potrf.hip).  All of them carry their sums in fp64 and round
once to the element type T.

Shared by tests/test_reduce_ref_host.py (CPU: a sum carried in fp64 passes, one carried in fp32 and seeded mutations fail) and
tests/test_gpu_reductions.py (the kernels).  CPU only: nothing here imports the library or touches a GPU.

Bound, for every fp64-carried sum of L terms rounded once to T (u_T = 2^-24 / 2^-53):
    |got - ref| <= u_T |ref| + (L + 4) 2^-53 sum |terms|
u_T |ref| is the one rounding to T; L terms summed in fp64 in ANY order carry at most gamma_(L-1) ~ (L - 1) 2^-53 of the sum of their
magnitudes (Higham, Accuracy and Stability, 4.2); a product of two fp32 values is exact in fp64, one of two fp64 values (or of three
fp32 values, var H H) carries one more 2^-53, and the rest of the + 4 covers the second-order terms and the fp64 evaluation of the
reference itself.  For T = fp64 the first term is of the size of the second's slack; the formula is kept uniform.  Nothing in it is
tuned on the kernels.  A sum carried in fp32 is outside it for most outputs (tests/test_reduce_ref_host.py).

Inputs are N(0,1) times a per-latent scale 1e-3, 1, 1e3, ROUNDED to the element type (the rounding of the inputs is not counted as
error); every buffer is NaN wherever the kernel must not read.
"""
import torch

import _factor_ref as fr

NB = fr.NB
UNIT = fr.UNIT
SCALES = (1e-3, 1.0, 1e3)
SENTINEL = -777.25
F32, F64 = torch.float32, torch.float64

QS = (1, 3)
# plmc_posterior_moments: n (n_pad = 128, 384) and ns with 1 + ns at and across a workgroup's 64 (fp32) / 32 (fp64) columns and no
# multiple of the 16-byte vector
MOMENT_SIZES = (100, 300)
MOMENT_NS = (1, 3, 31, 32, 63, 64, 65, 130)
W_SIZES = (100, 129, 300)
MIX_CASES = ((1, 1, 1), (3, 50, 7), (8, 257, 16))          # (q, ns, p)
MIX_EPS = (0.0, 1e-3)


def epv(dtype):
    """elements per 16-byte vector"""
    return 4 if dtype == F32 else 2


def round_up(x, m):
    return (x + m - 1) // m * m


def _scale(q):
    return torch.tensor([SCALES[i % 3] for i in range(q)], dtype=F64)


def bound(ref, mag, L, dtype):
    """u_T |ref| + (L + 4) 2^-53 mag,  mag = the sum of the magnitudes of the L terms"""
    return UNIT[dtype] * ref.abs() + (L + 4.0) * 2.0 ** -53 * mag


def violations(got, ref, bnd, limit=5):
    """[(index, |error|, bound)] of the outputs outside the bound (NaN counts), the first `limit` of them"""
    err = (got.double() - ref).abs()
    bad = ~(err <= bnd)
    return [(tuple(i), float(err[tuple(i)]), float(bnd[tuple(i)])) for i in bad.nonzero()[:limit].tolist()]


def outside(got, ref, bnd):
    """how many outputs are outside the bound (NaN counts)"""
    return int((~((got.double() - ref).abs() <= bnd)).sum())


def worst_ratio(got, ref, bnd):
    r = (got.double() - ref).abs() / bnd
    r = torch.where(torch.isnan(r), torch.where(bnd == 0, torch.zeros_like(r), torch.full_like(r, float("inf"))), r)
    return float(r.max())


def carried(terms, dim, carry, out):
    """the sum of `terms` (fp64) along `dim` carried in `carry` and rounded once to `out`"""
    return terms.to(carry).sum(dim).to(out)


# ------------------------------------------------------------------------------------------------ plmc_posterior_moments, plmc_extract_col
def moment_inputs(n, q, ns, dtype, seed=0):
    """[z | V] (q, n_pad, 1 + ns) as fp64 holding values of `dtype`; rows >= n are zero, as plmc_write_rhs leaves them"""
    g = torch.Generator().manual_seed(15485863 * seed + 7919 * n + 104729 * ns + q)
    n_pad = fr.pad(n)
    zV = torch.zeros(q, n_pad, 1 + ns, dtype=F64)
    zV[:, :n] = torch.randn(q, n, 1 + ns, generator=g, dtype=F64) * _scale(q).reshape(-1, 1, 1)
    return zV.to(dtype).double()


def moment_lda_min(n_pad, ns, dtype):
    """the smallest leading dimension include/plmc.h allows: the 1 + ns augmented columns rounded up to the 16-byte vector"""
    return n_pad + round_up(1 + ns, epv(dtype))


def moment_buffer(zV, dtype, lda=None):
    """(q, n_pad, lda) of `dtype`: the augmented columns [n_pad, n_pad + 1 + ns) hold [z | V], everything else -- the square part, the
    augmented columns >= 1 + ns, whatever lies behind -- is NaN"""
    q, n_pad, naug = zV.shape
    lda = moment_lda_min(n_pad, naug - 1, dtype) if lda is None else lda
    A = torch.full((q, n_pad, lda), float("nan"), dtype=dtype)
    A[:, :, n_pad:n_pad + naug] = zV.to(dtype)
    return A


def moment_reference(zV):
    """fp64 (mean, vsq, sum |v z|, sum v^2), (q, ns) each: mean[l][s] = sum_i v(s)_i z_i, vsq = sum_i v(s)_i^2"""
    z, V = zV[:, :, :1].double(), zV[:, :, 1:].double()
    return (V * z).sum(1), (V * V).sum(1), (V * z).abs().sum(1), (V * V).sum(1)


def moment_cpu(A, n_pad, ns, dtype, carry=F64, mutate=None):
    """(mean, vsq) formed on the CPU from the BUFFER, the sums carried in `carry` and rounded once to `dtype` -- or, with `mutate`:
      "wrong_column"  v(s) taken from augmented column s instead of 1 + s"""
    c0 = n_pad if mutate == "wrong_column" else n_pad + 1
    z, V = A[:, :, n_pad:n_pad + 1].double(), A[:, :, c0:c0 + ns].double()
    return carried(V * z, 1, carry, dtype), carried(V * V, 1, carry, dtype)


# ------------------------------------------------------------------------------------------------ plmc_wt_matvec, plmc_w_diag
def w_inputs(n, q, dtype, seed=0):
    """(W (q, n_pad, n_pad) lower triangular, z (q, n_pad)) as fp64 holding values of `dtype`: every row and column of the padding is
    live (the kernels treat all n_pad alike)"""
    g = torch.Generator().manual_seed(32452843 * seed + 7919 * n + q)
    n_pad = fr.pad(n)
    s = _scale(q)
    W = torch.tril(torch.randn(q, n_pad, n_pad, generator=g, dtype=F64)) * s.reshape(-1, 1, 1)
    z = torch.randn(q, n_pad, generator=g, dtype=F64) * s.reshape(-1, 1)
    return W.to(dtype).double(), z.to(dtype).double()


def w_buffer(n, q, dtype, W):
    """A HostWorkspace (one augmented column, W columns at wcol0, ldw = lda > n_pad) that is NaN everywhere except the W tiles on and
    below the block diagonal, laid by tests/_factor_ref.write_factor (explicit zeros above the diagonal inside the diagonal blocks)"""
    ws = fr.HostWorkspace(n, q, 1, dtype, with_inverse=True)
    ws.A.fill_(float("nan"))
    nanU = torch.full((q, ws.n_pad, ws.n_pad), float("nan"), dtype=F64)
    fr.write_factor(ws, nanU, W, None)
    return ws


def w_reference(W, z):
    """fp64 (alpha, sum |W z|, kd): alpha[i] = sum_l W[l][i] z[l], kd[i] = sum_l W[l][i]^2 (its own magnitude)"""
    T = torch.tril(W.double())
    return (T * z[:, :, None]).sum(1), (T * z[:, :, None]).abs().sum(1), (T * T).sum(1)


def w_cpu(ws, z, dtype, carry=F64, mutate=None):
    """(alpha, kd) formed on the CPU from the BUFFER, reading the tiles on and below the block diagonal only (a select) -- or, with
    `mutate`:
      "pad_row"  the last row counted twice (the kernels load past the end from a clamped row and must leave that load out)"""
    n_pad = ws.n_pad
    blk = torch.arange(n_pad) // NB
    Wr = ws.A[:, :, ws.wcol0:ws.wcol0 + n_pad].double()
    T = torch.where(blk[:, None] >= blk[None, :], Wr, torch.zeros((), dtype=F64))
    zz = z.double()
    if mutate == "pad_row":
        T, zz = torch.cat([T, T[:, -1:]], dim=1), torch.cat([zz, zz[:, -1:]], dim=1)
    return carried(T * zz[:, :, None], 1, carry, dtype), carried(T * T, 1, carry, dtype)


# ------------------------------------------------------------------------------------------------ plmc_mix_posterior
def mix_inputs(q, ns, p, dtype, seed=0):
    """(mean_lat (q, ns), var_lat (q, ns) > 0, Ht (q, p)) as fp64 holding values of `dtype`"""
    g = torch.Generator().manual_seed(49979687 * seed + 7919 * q + 104729 * ns + p)
    ml = torch.randn(q, ns, generator=g, dtype=F64) * _scale(q).reshape(-1, 1)
    vl = torch.rand(q, ns, generator=g, dtype=F64) + 0.05
    H = torch.randn(q, p, generator=g, dtype=F64)
    return ml.to(dtype).double(), vl.to(dtype).double(), H.to(dtype).double()


def mix_eps(eps, dtype):
    """eps as a value of the element type (the kernel takes it in T)"""
    return float(torch.tensor(eps, dtype=dtype))


def mix_reference(ml, vl, H, eps):
    """fp64 (mean, var, sum |m H|, sum |v H^2| + |eps|), (ns, p) each"""
    tm = ml[:, :, None] * H[:, None, :]
    tv = vl[:, :, None] * H[:, None, :] * H[:, None, :]
    return tm.sum(0), tv.sum(0) + eps, tm.abs().sum(0), tv.abs().sum(0) + abs(eps)


def mix_cpu(ml, vl, H, eps, dtype, carry=F64, mutate=None):
    """(mean, var) on the CPU, carried in `carry`, rounded once -- or, with `mutate`:
      "h_for_h2"  var H for var H^2          "no_eps"  eps dropped"""
    tm = ml[:, :, None] * H[:, None, :]
    tv = vl[:, :, None] * H[:, None, :] * (1.0 if mutate == "h_for_h2" else H[:, None, :])
    e = 0.0 if mutate == "no_eps" else eps
    return carried(tm, 0, carry, dtype), (tv.to(carry).sum(0) + torch.tensor(e, dtype=carry)).to(dtype)
