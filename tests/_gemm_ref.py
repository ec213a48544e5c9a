"""Reference and bound of the batched TN tile product plmc_gemm_tn / plmc_gemm_tn_tri (csrc/gemm.hip):
    C[b] (=, +=, -=) A[b]^T B[b],   A: K x M, B: K x N, both K-major, C: M x N,
with the triangular structure `tri` (PLMC_TRI_* of include/plmc.h) declared per 128-block.

Shared by tests/test_gemm_ref_host.py (CPU: a product in the element type passes, seeded mutations fail) and
tests/test_gpu_gemm_tn.py (the kernel).  CPU only: nothing here imports the library or touches a GPU.

Reference: fp64, from the inputs ROUNDED to the element type (their rounding is not counted as error), with every block that `tri`
declares zero replaced by 0, combined with C0 by `mode` (0 store, 1 add, 2 subtract).  Under PLMC_TRI_C_LOWER the tiles with
ib < jb hold C0 (left untouched) or, with PLMC_TRI_C_ZERO, +0.

Bound, u = 2^-24 / 2^-53 for the element type, element by element:
    |C - C_ref|[i][j] <= (K + 4) u (sum_k |A_ki| |B_kj| + |C0_ij|)          the C0 term in modes 1 and 2 only
the argument of tests/_trmm_ref.py: K products summed in ANY order carry at most gamma_K ~ K u of the sum of their magnitudes
(Higham, Accuracy and Stability, 3.1), the combine with C0 one more u of what it adds up, the rounding to the element type
another, and one u covers the second-order terms of gamma at these sizes.  In the tiles PLMC_TRI_C_LOWER skips the bound is 0:
what stands there is C0 (or 0) itself.  Nothing in it is tuned on the kernel.

Inputs: N(0,1) entries times a per-batch scale 1e-3, 1, 1e3, and NaN in every 128-block of A and B that `tri` declares zero -- there
the skipped contraction range is a correctness contract, not a saving (the W tiles above the block diagonal of a factor buffer
are never written).  Entries inside the diagonal blocks are arbitrary and nonzero: structure is declared per block.
"""
import torch

import _factor_ref as fr

NB = fr.NB
UNIT = fr.UNIT
BK = 16                                      # contraction slab of the tile engine: K % BK == 0
SCALES = (1e-3, 1.0, 1e3)
SENTINEL = -777.25

AL, BL, AU, CL, CZ = 1, 2, 4, 8, 16          # PLMC_TRI_A_LOWER, _B_LOWER, _A_UPPER, _C_LOWER, _C_ZERO

# (M, N, K): a single slab; K not a block multiple; M > K (empty ranges under A_LOWER, k_hi cut at K under A_UPPER); three block
# rows; K above M and N
SHAPES = ((128, 128, 16), (128, 256, 144), (384, 256, 144), (384, 384, 384), (256, 384, 400))
BATCH = (1, 3)
# every combination projectedlmc/_var_engine.py and _engine.py use, and the block-diagonal one
TRIS = (0, AL, BL, AU, AL | BL, AL | AU, AU | BL, CL, CL | CZ, AL | BL | CL, AU | BL | CL | CZ)
MODES = (0, 1, 2)


def valid_modes(tri):
    """PLMC_TRI_C_ZERO is a mode-0 flag"""
    return (0,) if tri & CZ else MODES


def tri_name(tri):
    return "|".join(n for b, n in ((AL, "AL"), (BL, "BL"), (AU, "AU"), (CL, "CL"), (CZ, "CZ")) if tri & b) or "0"


def zero_masks(M, N, K, tri, lo_late=0, hi_early=0):
    """(zA (K, M), zB (K, N)) bool: the entries `tri` declares zero, per 128-block as in include/plmc.h:
         A_LOWER  A[k][i] = 0 for k < 128 (i / 128)          B_LOWER  B[k][j] = 0 for k < 128 (j / 128)
         A_UPPER  A[k][i] = 0 for k >= 128 (i / 128 + 1)
    lo_late / hi_early (host mutations only): the lower ranges begin that many rows late, the upper range ends that many rows early."""
    k = torch.arange(K)[:, None]
    bi, bj = (torch.arange(M) // NB)[None, :], (torch.arange(N) // NB)[None, :]
    zA = torch.zeros(K, M, dtype=torch.bool)
    zB = torch.zeros(K, N, dtype=torch.bool)
    if tri & AL:
        zA |= k < NB * bi + lo_late
    if tri & AU:
        zA |= k >= NB * (bi + 1) - hi_early
    if tri & BL:
        zB |= k < NB * bj + lo_late
    return zA, zB


def skipped_tiles(M, N, tri):
    """(M, N) bool: the elements of the tiles ib < jb that PLMC_TRI_C_LOWER does not compute (all False without it)"""
    if not tri & CL:
        return torch.zeros(M, N, dtype=torch.bool)
    return (torch.arange(M) // NB)[:, None] < (torch.arange(N) // NB)[None, :]


def make_inputs(M, N, K, batch, tri, dtype, seed=0, garbage=False):
    """(A (batch, K, M), B (batch, K, N), C0 (batch, M, N)) as fp64 tensors holding values of `dtype`; A and B are NaN in every block
    `tri` declares zero.  The random numbers do not depend on `tri`.  garbage (host mutations only): the declared-zero blocks keep
    their finite random values, so a mistake shows as an error and not as NaN."""
    g = torch.Generator().manual_seed(15485863 * seed + 7919 * M + 104729 * N + 1299709 * K + batch)
    scale = torch.tensor([SCALES[b % 3] for b in range(batch)], dtype=torch.float64).reshape(-1, 1, 1)
    A = torch.randn(batch, K, M, generator=g, dtype=torch.float64) * scale
    B = torch.randn(batch, K, N, generator=g, dtype=torch.float64) * scale
    C0 = torch.randn(batch, M, N, generator=g, dtype=torch.float64) * scale
    A, B, C0 = (t.to(dtype).double() for t in (A, B, C0))
    if not garbage:
        zA, zB = zero_masks(M, N, K, tri)
        nan = torch.full((), float("nan"), dtype=torch.float64)
        A, B = torch.where(zA, nan, A), torch.where(zB, nan, B)
    return A, B, C0


def embed(t, ld, col0, fill):
    """t (batch, rows, cols) laid into a buffer (batch, rows, ld) of `fill` at column offset col0, ld > cols: what a caller hands over
    as a strided view (pointer = buffer + col0, leading dimension ld, batch stride rows * ld).  -> the buffer"""
    batch, rows, cols = t.shape
    assert ld > cols and 0 <= col0 and col0 + cols <= ld
    buf = torch.full((batch, rows, ld), fill, dtype=t.dtype)
    buf[:, :, col0:col0 + cols] = t
    return buf


def _masked(A, B, tri):
    K, M, N = A.shape[-2], A.shape[-1], B.shape[-1]
    zA, zB = zero_masks(M, N, K, tri)
    zero = torch.zeros((), dtype=A.dtype)
    return torch.where(zA, zero, A), torch.where(zB, zero, B)


def products(A, B, tri):
    """(A^T B, |A|^T |B|) in fp64 over the blocks `tri` does not declare zero: what reference() and bound() need of the operands, the
    same for every mode (pass it to them as `parts` to form it once)"""
    Az, Bz = _masked(A.double(), B.double(), tri)
    return Az.transpose(1, 2) @ Bz, Az.abs().transpose(1, 2) @ Bz.abs()


def reference(A, B, C0, mode, tri, parts=None):
    """fp64 C: A^T B over the blocks `tri` does not declare zero, combined with C0 by `mode`; the skipped tiles hold C0 or +0"""
    P = (parts or products(A, B, tri))[0]
    C = P if mode == 0 else (C0.double() + P if mode == 1 else C0.double() - P)
    skip = skipped_tiles(C.shape[-2], C.shape[-1], tri)
    return torch.where(skip, torch.zeros_like(C) if tri & CZ else C0.double(), C)


def bound(A, B, C0, mode, tri, dtype, parts=None):
    """(batch, M, N): (K + 4) u (sum_k |A_ki| |B_kj| + |C0_ij| in modes 1 and 2); 0 in the tiles PLMC_TRI_C_LOWER skips"""
    K = A.shape[-2]
    mag = (parts or products(A, B, tri))[1]
    if mode != 0:
        mag = mag + C0.double().abs()
    skip = skipped_tiles(mag.shape[-2], mag.shape[-1], tri)
    return torch.where(skip, torch.zeros_like(mag), (K + 4.0) * UNIT[dtype] * mag)


def violations(C, Cref, bnd, limit=5):
    """[(batch, i, j, |error|, bound)] of the elements outside the bound (NaN counts), the first `limit` of them"""
    err = (C.double() - Cref).abs()
    bad = ~(err <= bnd)
    idx = bad.nonzero()[:limit]
    return [(int(a), int(b), int(c), float(err[a, b, c]), float(bnd[a, b, c])) for a, b, c in idx.tolist()]


def outside(C, Cref, bnd):
    """how many elements are outside the bound (NaN counts)"""
    return int((~((C.double() - Cref).abs() <= bnd)).sum())


def worst_ratio(C, Cref, bnd):
    """largest |error| / bound over the computed elements (bound > 0), and that element (batch, i, j): for the record in profiles/"""
    err = (C.double() - Cref).abs()
    r = torch.where(bnd > 0, err / bnd, torch.zeros_like(err))
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    k = int(r.argmax())
    n2 = r.shape[-1] * r.shape[-2]
    return float(r.reshape(-1)[k]), (k // n2, (k % n2) // r.shape[-1], k % r.shape[-1])


MUTATIONS = ("ignore_a_lower", "ignore_b_lower", "ignore_a_upper", "k_lo_late", "k_hi_early", "sub_as_add", "untransposed", "c_lower_computed")


def cpu_product(A, B, C0, mode, tri, dtype, mutate=None):
    """The product formed on the CPU in the element type from the operands AS THEY STAND IN MEMORY (what a kernel sees), reading
    exactly what the contract allows: the declared-zero blocks are taken out by a select, never by a multiplication -- or, with
    `mutate`, one of the seeded mistakes:
      "ignore_a_lower" / "ignore_b_lower" / "ignore_a_upper"   that bit of `tri` not looked at
      "k_lo_late"          the lower ranges begin one 16-row slab late
      "k_hi_early"         the upper range ends one 128-block early
      "sub_as_add"         mode 2 applied as mode 1
      "untransposed"       A B for A^T B (M = K)
      "c_lower_computed"   the tiles above the block diagonal computed and combined instead of left"""
    K, M, N = A.shape[-2], A.shape[-1], B.shape[-1]
    t = tri
    if mutate in ("ignore_a_lower", "ignore_b_lower", "ignore_a_upper"):
        t = tri & ~{"ignore_a_lower": AL, "ignore_b_lower": BL, "ignore_a_upper": AU}[mutate]
    zA, zB = zero_masks(M, N, K, t, lo_late=BK if mutate == "k_lo_late" else 0, hi_early=NB if mutate == "k_hi_early" else 0)
    zero = torch.zeros((), dtype=dtype)
    Az, Bz = torch.where(zA, zero, A.to(dtype)), torch.where(zB, zero, B.to(dtype))
    P = (Az if mutate == "untransposed" else Az.transpose(1, 2)) @ Bz
    Cd = C0.to(dtype)
    if mutate == "sub_as_add" and mode == 2:
        mode = 1
    C = P if mode == 0 else (Cd + P if mode == 1 else Cd - P)
    if mutate == "c_lower_computed":
        return C
    skip = skipped_tiles(M, N, tri)
    return torch.where(skip, torch.zeros_like(C) if tri & CZ else Cd, C)
