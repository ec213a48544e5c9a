"""plmc_gemm_tn / plmc_gemm_tn_tri (csrc/gemm.hip) alone, through the raw C ABI, against the fp64 reference and the bound of
tests/_gemm_ref.py.

Every buffer is written by the test.  A and B are NaN in every 128-block that `tri` declares zero and in the gap columns of an embedded
layout; C stands inside a parent filled with a sentinel: one guard row above and below the M x N window, the gap columns beside it.
{f32, f64} x the five shapes of _gemm_ref.SHAPES (a single slab, K not a block multiple, M > K, three block rows, K above M and N),
inside each case tri x valid mode x batch {1, 3}, each at the dense layout and at lda, ldb, ldc = columns + 4 with a column offset
of 4 elements; strideB = 0 (one B shared by the batch) and A, B as two views of one buffer (W^T W) once per case and mode.
Asserted: the bound element by element, no NaN in C, everything outside the window bit-identical to the sentinel, the tiles
PLMC_TRI_C_LOWER skips bit-identical to what C held (exactly +0 with PLMC_TRI_C_ZERO), two calls bit-identical; the triangular entry
point giving the same bits as the plain one on operands whose declared-zero blocks are true zeros; the call of
_engine._posterior_jacobians on a factor buffer whose W tiles above the block diagonal are NaN; and every argument error refused
with a message before anything is launched.

PLMC_GEMM_RECORD=<file>: the largest measured error / bound per dtype, shape and mode, the CPU product's beside it, is appended to
that file as rows of a markdown table (profiles/gemm_tn_accuracy.md is one such run).
"""
import ctypes
import os

import pytest
import torch

import _factor_ref as fr
import _gemm_ref as gr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32, F64 = torch.float32, torch.float64
NB = gr.NB
NAN = float("nan")
_ROWS = {}


@pytest.fixture(scope="module")
def hip():
    from projectedlmc import _hip
    assert torch.cuda.is_available()
    yield _hip
    path = os.environ.get("PLMC_GEMM_RECORD")
    if path and _ROWS:
        with open(path, "a") as f:
            for (dt, shape, mode), (g, at, c) in _ROWS.items():
                f.write("| %s | %d x %d x %d | %d | %.3f | %s | %.3f |\n" % ((dt,) + shape + (mode, g, at, c)))


@pytest.fixture(autouse=True)
def _nothing_more_after_a_gpu_error():
    """a HIP error is sticky: the session ends at the first one instead of queueing the remaining cases behind it"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("HIP error, nothing more is started: %s" % e, returncode=3)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int64)


class _View:
    """an operand as the C ABI takes it: a device parent, the element offset of the view inside it, leading dimension, batch stride"""

    def __init__(self, parent, off, ld, stride):
        self.parent, self.off, self.ld, self.stride = parent, off, ld, stride

    @property
    def ptr(self):
        return ctypes.c_void_p(self.parent.data_ptr() + self.off * self.parent.element_size())


def _operand(t, dtype, embedded):
    """t (batch, K, cols) fp64 host values -> a dense device copy, or one inside a NaN parent at column offset 4 with ld = cols + 4"""
    cols = t.shape[2]
    if embedded:
        return _View(gr.embed(t, cols + 4, 4, NAN).to(dtype).to(DEV), 4, cols + 4, t.shape[1] * (cols + 4))
    return _View(t.to(dtype).to(DEV).contiguous(), 0, cols, t.shape[1] * cols)


def _c_parent(C0, dtype, embedded):
    """C0 (batch, M, N) inside a sentinel parent (batch, M + 2, ldc): a guard row above and below, with `embedded` the gap columns"""
    batch, M, N = C0.shape
    ldc, col0 = (N + 4, 4) if embedded else (N, 0)
    P = torch.full((batch, M + 2, ldc), gr.SENTINEL, dtype=dtype)
    P[:, 1:M + 1, col0:col0 + N] = C0.to(dtype)
    return P.to(DEV), ldc, col0


def _launch(hip, dtype, mode, tri, M, N, K, a, b, C0, embedded, plain=False):
    """two calls on fresh copies of the same C parent -> (the window of the first (batch, M, N) on the host, messages of what is wrong)"""
    batch = C0.shape[0]
    P0, ldc, col0 = _c_parent(C0, dtype, embedded)
    out = []
    for _ in range(2):
        P = P0.clone()
        c = _View(P, ldc + col0, ldc, (M + 2) * ldc)
        args = (M, N, K, a.ptr, a.ld, a.stride, b.ptr, b.ld, b.stride, c.ptr, c.ld, c.stride, batch, hip.stream_ptr(DEV))
        if plain:
            hip.lib().call("plmc_gemm_tn", dtype, mode, *args)
        else:
            hip.lib().call("plmc_gemm_tn_tri", dtype, mode, tri, *args)
        out.append(P)
    torch.cuda.synchronize()
    bad = []
    if not torch.equal(_bits(out[0]), _bits(out[1])):
        bad.append("two calls differ")
    Ph = out[0].cpu()
    win = Ph[:, 1:M + 1, col0:col0 + N].clone()
    Ph[:, 1:M + 1, col0:col0 + N] = gr.SENTINEL
    if not torch.equal(_bits(Ph), _bits(torch.full_like(Ph, gr.SENTINEL))):
        bad.append("something outside the M x N window was written")
    return win, bad


def _check(win, A, B, C0, mode, tri, dtype, parts):
    """-> (messages of what is wrong, largest error / bound, its element)"""
    bad = []
    if bool(torch.isnan(win).any()):
        bad.append("NaN reached C")
    Cref, bnd = gr.reference(A, B, C0, mode, tri, parts), gr.bound(A, B, C0, mode, tri, dtype, parts)
    v = gr.violations(win, Cref, bnd)
    if v:
        bad.append(("outside the bound (batch, i, j, error, bound)", v))
    skip = gr.skipped_tiles(win.shape[1], win.shape[2], tri)
    if bool(skip.any()):
        want = torch.zeros_like(win) if tri & gr.CZ else C0.to(dtype)
        if not torch.equal(_bits(win[:, skip]), _bits(want[:, skip])):
            bad.append("a tile PLMC_TRI_C_LOWER skips is not bit-identical to %s" % ("+0" if tri & gr.CZ else "what C held"))
    ratio, at = gr.worst_ratio(win, Cref, bnd)
    return bad, ratio, at


def _record(dtype, shape, mode, ratio, at, tag, A, B, C0, tri, parts):
    if not os.environ.get("PLMC_GEMM_RECORD"):
        return
    key = ("f32" if dtype == F32 else "f64", shape, mode)
    cpu = gr.worst_ratio(gr.cpu_product(A, B, C0, mode, tri, dtype), gr.reference(A, B, C0, mode, tri, parts),
                         gr.bound(A, B, C0, mode, tri, dtype, parts))[0]
    g, gat, c = _ROWS.get(key, (0.0, "", 0.0))
    if ratio >= g:
        g, gat = ratio, "%s, member %d element (%d, %d)" % ((tag,) + tuple(at))
    _ROWS[key] = (g, gat, max(c, cpu))


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", gr.SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_product_against_fp64_reference(hip, dtype, shape):
    M, N, K = shape
    wrong = []
    for batch in gr.BATCH:
        for tri in gr.TRIS:
            A, B, C0 = gr.make_inputs(M, N, K, batch, tri, dtype)
            parts = gr.products(A, B, tri)
            for embedded in (False, True):
                a, b = _operand(A, dtype, embedded), _operand(B, dtype, embedded)
                for mode in gr.valid_modes(tri):
                    tag = "%s mode %d batch %d %s" % (gr.tri_name(tri), mode, batch, "embedded" if embedded else "dense")
                    win, bad = _launch(hip, dtype, mode, tri, M, N, K, a, b, C0, embedded)
                    more, ratio, at = _check(win, A, B, C0, mode, tri, dtype, parts)
                    wrong += [(tag, x) for x in bad + more]
                    _record(dtype, shape, mode, ratio, at, tag, A, B, C0, tri, parts)
    assert not wrong, wrong[:6]


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", gr.SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_one_b_shared_by_the_batch(hip, dtype, shape):
    """strideB = 0"""
    M, N, K = shape
    batch, wrong = 3, []
    for tri in (gr.BL, gr.AL | gr.BL | gr.CL):
        A, B, C0 = gr.make_inputs(M, N, K, batch, tri, dtype)
        a, b = _operand(A, dtype, False), _operand(B[1:2], dtype, True)
        b.stride = 0
        Bx = B[1:2].expand(batch, K, N)
        parts = gr.products(A, Bx, tri)
        for mode in gr.valid_modes(tri):
            win, bad = _launch(hip, dtype, mode, tri, M, N, K, a, b, C0, False)
            more, ratio, at = _check(win, A, Bx, C0, mode, tri, dtype, parts)
            wrong += [(gr.tri_name(tri), mode, x) for x in bad + more]
    assert not wrong, wrong[:6]


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", gr.SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_a_and_b_as_two_views_of_one_buffer(hip, dtype, shape):
    """W^T W: A is B with A_LOWER | B_LOWER -- one K x max(M, N) buffer, A its first M columns, B its first N"""
    M, N, K = shape
    W = max(M, N)
    tri, wrong = gr.AL | gr.BL, []
    for batch in gr.BATCH:
        X = gr.make_inputs(W, NB, K, batch, gr.AL, dtype)[0]          # (batch, K, W), NaN where k < 128 (column / 128)
        C0 = gr.make_inputs(M, N, K, batch, 0, dtype)[2]
        x = _operand(X, dtype, False)
        A, B = X[:, :, :M], X[:, :, :N]
        assert bool(torch.isnan(X).any()) == (W > NB)
        parts = gr.products(A, B, tri)
        for mode in gr.MODES:
            win, bad = _launch(hip, dtype, mode, tri, M, N, K, x, x, C0, True)
            more, ratio, at = _check(win, A, B, C0, mode, tri, dtype, parts)
            wrong += [(batch, mode, x_) for x_ in bad + more]
    assert not wrong, wrong[:6]


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_triangular_ranges_give_the_same_number_as_the_plain_product(hip, dtype):
    """the header's "the result is the same number": on operands whose declared-zero blocks are true zeros the skipped terms are exact
    zeros in front of the sum, so plmc_gemm_tn_tri and plmc_gemm_tn agree bit for bit"""
    M = N = K = 384
    batch = 3
    for tri in (gr.AL, gr.BL, gr.AU, gr.AL | gr.BL, gr.AL | gr.AU):
        A, B, C0 = gr.make_inputs(M, N, K, batch, tri, dtype)
        zero = torch.zeros((), dtype=F64)
        A, B = torch.where(torch.isnan(A), zero, A), torch.where(torch.isnan(B), zero, B)
        a, b = _operand(A, dtype, False), _operand(B, dtype, False)
        for mode in gr.MODES:
            t, bad_t = _launch(hip, dtype, mode, tri, M, N, K, a, b, C0, False)
            p, bad_p = _launch(hip, dtype, mode, 0, M, N, K, a, b, C0, False, plain=True)
            assert not bad_t and not bad_p, (gr.tri_name(tri), mode, bad_t, bad_p)
            assert torch.equal(_bits(t), _bits(p)), (gr.tri_name(tri), mode, "the triangular ranges change the number")
            assert not gr.violations(p, gr.reference(A, B, C0, mode, 0), gr.bound(A, B, C0, mode, 0, dtype)), (gr.tri_name(tri), mode)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_the_call_of_the_posterior_jacobians_in_place_on_a_factor_buffer(hip, dtype):
    """B = W^T [z | V] as _engine._posterior_jacobians forms it: tri = PLMC_TRI_A_LOWER, A = the W columns of the factor buffer (ldw =
    lda), B = its augmented block (ldb = lda), C a separate buffer.  The W tiles above the block diagonal are "never written" -- here
    NaN, like the square part; the augmented columns beyond 1 + ns are zeros, as plmc_write_rhs leaves them."""
    n, q, ns = 300, 2, 37
    ws = fr.HostWorkspace(n, q, 1 + ns, dtype, with_inverse=True)
    n_pad, ncols = ws.n_pad, ws.naug_pad
    assert (n_pad, ncols) == (384, 128)
    g = torch.Generator().manual_seed(11)
    scale = torch.tensor(gr.SCALES[:q], dtype=torch.float64).reshape(-1, 1, 1)
    W = torch.tril(torch.randn(q, n_pad, n_pad, generator=g, dtype=torch.float64)) * scale
    Z = torch.zeros(q, n_pad, 1 + ns, dtype=torch.float64)
    Z[:, :n] = torch.randn(q, n, 1 + ns, generator=g, dtype=torch.float64) * scale
    ws.A.fill_(NAN)
    ws.A[:, :, n_pad:n_pad + ncols] = 0.0
    fr.write_factor(ws, torch.eye(n_pad, dtype=torch.float64).expand(q, -1, -1), W, Z)
    Wraw = ws.A[:, :, ws.wcol0:ws.wcol0 + n_pad].double()               # as it stands in memory: NaN above the block diagonal
    blk = torch.arange(n_pad) // NB
    assert bool(torch.isnan(Wraw[:, blk[:, None] < blk[None, :]]).all()) and bool(torch.isnan(ws.A[:, :, :n_pad]).any())
    Baug = ws.A[:, :, n_pad:n_pad + ncols].double()
    Ad = ws.A.to(DEV)
    buf = torch.full((q, n_pad, ncols), gr.SENTINEL, dtype=dtype, device=DEV)
    esz = Ad.element_size()
    hip.lib().call("plmc_gemm_tn_tri", dtype, 0, gr.AL, n_pad, ncols, n_pad, ctypes.c_void_p(Ad.data_ptr() + ws.wcol0 * esz), ws.lda, ws.strideA,
                   ctypes.c_void_p(Ad.data_ptr() + n_pad * esz), ws.lda, ws.strideA, hip.ptr(buf), ncols, n_pad * ncols, q, hip.stream_ptr(DEV))
    torch.cuda.synchronize()
    got = buf.cpu()
    assert not bool(torch.isnan(got).any()), "NaN of a never-written W tile reached B"
    C0 = torch.zeros(q, n_pad, ncols, dtype=torch.float64)
    Cref = torch.tril(W.to(dtype).double()).transpose(1, 2) @ Baug
    assert torch.equal(Cref, gr.reference(Wraw, Baug, C0, 0, gr.AL))
    bad = gr.violations(got, Cref, gr.bound(Wraw, Baug, C0, 0, gr.AL, dtype))
    assert not bad, bad
    assert bool((got[:, :, 1 + ns:] == 0).all())                       # zero columns of the augmented block give zero columns
    assert torch.equal(_bits(Ad.cpu()), _bits(ws.A)), "the factor buffer was written"


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_argument_errors_are_refused_before_any_launch(hip, dtype):
    M, N, K, batch = 256, 256, 144, 3                                  # tile (0, 1) is one PLMC_TRI_C_LOWER skips
    tri = gr.AL | gr.BL | gr.CL
    A, B, C0 = gr.make_inputs(M, N, K, batch, tri, dtype)
    Ad, Bd = A.to(dtype).to(DEV).contiguous(), B.to(dtype).to(DEV).contiguous()
    A0, B0 = Ad.cpu(), Bd.cpu()
    buf = torch.full((2 * batch * M * N,), gr.SENTINEL, dtype=dtype, device=DEV)
    L = hip.lib().cdll
    fn = getattr(L, "plmc_gemm_tn_tri" + ("_f32" if dtype == F32 else "_f64"))
    st = hip.stream_ptr(DEV)
    esz = Ad.element_size()
    epv = 16 // esz
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off * esz)
    good = dict(mode=0, tri=tri, M=M, N=N, K=K, A=P(Ad), lda=M, strideA=K * M, B=P(Bd), ldb=N, strideB=K * N, C=P(buf), ldc=N, strideC=M * N,
                batch=batch)
    order = ["mode", "tri", "M", "N", "K", "A", "lda", "strideA", "B", "ldb", "strideB", "C", "ldc", "strideC", "batch"]
    span = (M - 1) * N + N                                             # elements one batch member of C covers
    cases = {
        "null A": dict(A=None), "null B": dict(B=None), "null C": dict(C=None),
        "mode 3": dict(mode=3), "mode -1": dict(mode=-1), "tri 32": dict(tri=32), "tri -1": dict(tri=-1),
        "C_ZERO without C_LOWER": dict(tri=gr.AL | gr.CZ), "C_ZERO with mode 1": dict(tri=gr.CL | gr.CZ, mode=1),
        "M = 0": dict(M=0), "N = 0": dict(N=0), "K = 0": dict(K=0),
        "M no block multiple": dict(M=M - 64), "N no block multiple": dict(N=N - 1), "K % 16 != 0": dict(K=K - 8),
        "lda < M": dict(lda=M - epv), "ldb < N": dict(ldb=N - epv), "ldc < N": dict(ldc=N - epv),
        "lda not a multiple of 16 bytes": dict(lda=M + 1), "ldb not a multiple of 16 bytes": dict(ldb=N + 1),
        "ldc not a multiple of 16 bytes": dict(ldc=N + 1),
        "A off by one element": dict(A=P(Ad, 1)), "B off by one element": dict(B=P(Bd, 1)), "C off by one element": dict(C=P(buf, 1)),
        "strideA off by one element": dict(strideA=K * M + 1), "strideB off by one element": dict(strideB=K * N + 1),
        "strideC off by one element": dict(strideC=M * N + 1),
        "batch 0": dict(batch=0),
        "strideC = 0 with batch 3": dict(strideC=0),
        "strideC one vector short of a batch member": dict(strideC=span - epv),
        "negative strideC one vector short": dict(strideC=-(span - epv), C=P(buf, 2 * span)),
    }
    for name, change in cases.items():
        args = dict(good, **change)
        rc = fn(*[args[k] for k in order], st)
        msg = L.plmc_last_error().decode()
        assert rc != 0, name
        assert "gemm_tn" in msg, (name, msg)
        assert len(msg.split(":", 1)[1].strip()) > 0, (name, msg)
    torch.cuda.synchronize()
    assert bool((buf == gr.SENTINEL).all()), "a refused call wrote something"
    assert torch.equal(_bits(Ad.cpu()), _bits(A0)) and torch.equal(_bits(Bd.cpu()), _bits(B0)), "a refused call wrote into an operand"
    assert fn(*[good[k] for k in order], st) == 0                      # and the same arguments unchanged are accepted
    one = dict(good, batch=1, strideC=0)                               # a single member has no batch stride to get wrong
    assert fn(*[one[k] for k in order], st) == 0
    torch.cuda.synchronize()
    got = buf[:batch * M * N].reshape(batch, M, N).cpu()
    Cz = torch.full((batch, M, N), gr.SENTINEL, dtype=torch.float64)   # PLMC_TRI_C_LOWER without C_ZERO: the tile above keeps the sentinel
    assert not gr.violations(got, gr.reference(A, B, Cz, 0, tri), gr.bound(A, B, Cz, 0, tri, dtype))
    assert bool((buf[batch * M * N:] == gr.SENTINEL).all())
