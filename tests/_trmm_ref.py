"""Reference and bound of the draw product plmc_trmm_ut (csrc/trmm.hip):  Y = shift + triu(U)^T Z  per latent.

Shared by tests/test_trmm_ref_host.py (CPU: a product in the element type passes, seeded mutations fail) and
tests/test_gpu_trmm_ut.py (the kernel).  CPU only: nothing here imports the library or touches a GPU.

Reference: fp64, from the inputs ROUNDED to the element type (their rounding is not counted as error).

Bound, u = 2^-24 / 2^-53 for the element type, element by element:
    |Y - Y_ref|[i][j] <= (i + 4) u (sum_{k <= i} |U_ki| |Z_kj| + |shift_i|)
i + 1 products summed in ANY order carry at most gamma_(i+1) ~ (i + 1) u of the sum of their magnitudes (Higham, Accuracy and
Stability, 3.1; a product accumulated in a wider format and rounded once is far inside it), the shift add one more u of what it
adds up, the final rounding to the element type another, and one u covers the second-order terms of gamma at these sizes.
Nothing in it is tuned on the kernel.

Inputs: U random upper triangular with entries scaled 1e-3 ... 1e3 per latent, and NaN everywhere the kernel must not read --
`nan_factor_buffer` lays U into the workspace layout of tests/_factor_ref.py (odd block count per row, augmented and W columns)
through its write_factor, over a buffer that is NaN everywhere: below the diagonal inside the diagonal blocks, the tiles below the
block diagonal, rows and columns >= n, the augmented columns, the W columns.
"""
import torch

import _factor_ref as fr

NB = fr.NB
UNIT = fr.UNIT
SCALES = (1e-3, 1.0, 1e3)
SENTINEL = -777.25

# the shapes of the kernel test: the path switch at ns = 16 | 17, a partial diagonal block, three block rows, the padding of ns
NS = (1, 5, 16, 17, 130)
SIZES = (1, 127, 128, 129, 300)
QS = (1, 3)


def make_inputs(n, q, ns, dtype, seed=0, with_shift=True):
    """(U (q, n, n) upper triangular, Z (q, n, ns), shift (q, n) | None) as fp64 tensors holding values of `dtype`"""
    g = torch.Generator().manual_seed(15485863 * seed + 7919 * n + 104729 * ns + q)
    scale = torch.tensor(SCALES[:q] if q <= len(SCALES) else [SCALES[i % 3] for i in range(q)], dtype=torch.float64)
    U = torch.triu(torch.randn(q, n, n, generator=g, dtype=torch.float64)) * scale.reshape(-1, 1, 1)
    Z = torch.randn(q, n, ns, generator=g, dtype=torch.float64)
    shift = torch.randn(q, n, generator=g, dtype=torch.float64) * scale.reshape(-1, 1) if with_shift else None
    r = lambda t: None if t is None else t.to(dtype).double()
    return r(U), r(Z), r(shift)


def reference(U, Z, shift):
    """fp64 Y = shift + triu(U)^T Z"""
    Y = torch.triu(U.double()).transpose(1, 2) @ Z.double()
    return Y if shift is None else Y + shift.double()[:, :, None]


def bound(U, Z, shift, dtype):
    """(q, n, ns): (i + 4) u (sum_{k <= i} |U_ki| |Z_kj| + |shift_i|)"""
    n = U.shape[-1]
    mag = torch.triu(U.double()).abs().transpose(1, 2) @ Z.double().abs()
    if shift is not None:
        mag = mag + shift.double().abs()[:, :, None]
    i = torch.arange(n, dtype=torch.float64).reshape(1, n, 1)
    return (i + 4.0) * UNIT[dtype] * mag


def violations(Y, Yref, bnd, limit=5):
    """[(latent, i, j, |error|, bound)] of the elements outside the bound (NaN counts), the first `limit` of them"""
    err = (Y.double() - Yref).abs()
    bad = ~(err <= bnd)
    idx = bad.nonzero()[:limit]
    return [(int(a), int(b), int(c), float(err[a, b, c]), float(bnd[a, b, c])) for a, b, c in idx.tolist()]


def nan_factor_buffer(n, q, dtype, U, lower=None):
    """A HostWorkspace (one augmented column, W columns: the layout of a training-step workspace, odd block count per row) that is NaN
    everywhere except the element-wise upper triangle of the leading n x n, which holds U.  lower: (q, n, n) values for the strictly
    lower part of the leading n x n instead of NaN (host mutations only)."""
    ws = fr.HostWorkspace(n, q, 1, dtype, with_inverse=True)
    assert (ws.lda // NB) % 2 == 1
    ws.A.fill_(float("nan"))
    Up = torch.full((q, ws.n_pad, ws.n_pad), float("nan"), dtype=torch.float64)
    Up[:, :n, :n] = torch.triu(U)
    fr.write_factor(ws, Up, None, None)                 # the element-wise upper triangle of the square part, nothing else
    if lower is not None:
        sq = ws.A[:, :n, :n]
        ws.A[:, :n, :n] = torch.where(torch.tril(torch.ones(n, n, dtype=torch.bool), -1), lower.to(dtype), sq)
    return ws


def cpu_product(ws, n, Z, shift, dtype, mutate=None):
    """The product formed on the CPU in the element type from the BUFFER (what a kernel sees), reading exactly what the contract
    allows -- or, with `mutate`, one of the seeded mistakes:
      "block_lower"  the strictly lower part of the diagonal blocks is taken along (a per-block mask instead of an element-wise one)
      "strict"       k < i instead of k <= i
      "untransposed" U z instead of U^T z
      "no_shift"     shift dropped"""
    A = ws.A[:, :n, :n]
    i = torch.arange(n)
    keep = i[:, None] <= i[None, :]                      # [k][i]: k <= i
    if mutate == "block_lower":
        keep = (i[:, None] // NB) <= (i[None, :] // NB)
    elif mutate == "strict":
        keep = i[:, None] < i[None, :]
    Um = torch.where(keep, A, torch.zeros((), dtype=dtype))
    Zt = Z.to(dtype)
    Y = (Um if mutate == "untransposed" else Um.transpose(1, 2)) @ Zt
    if shift is not None and mutate != "no_shift":
        Y = Y + shift.to(dtype)[:, :, None]
    return Y
