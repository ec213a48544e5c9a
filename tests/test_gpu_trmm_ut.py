"""plmc_trmm_ut (csrc/trmm.hip) alone, through the raw C ABI, against the fp64 reference and the bound of tests/_trmm_ref.py.

The factor buffer is written by the test in the workspace layout of tests/_factor_ref.py (odd block count per row, one augmented
column, W columns) and is NaN everywhere the kernel must not read: below the diagonal inside the diagonal blocks, the tiles below the
block diagonal, rows and columns >= n, the augmented and the W columns.  Y is prefilled with a sentinel, the gap columns [ns, ldy)
included.  n in {1, 127, 128, 129, 300} x q in {1, 3} x ns in {1, 5, 16, 17, 130} x {f32, f64} x shift {NULL, given}, the call with a
shift on leading dimensions above ns: both sides of the path switch (16 | 17), a partial diagonal block, three block rows, the
padding of ns inside the call.  Asserted: the bound element by element, no NaN, the sentinel untouched outside i < n, j < ns, two
calls bit-identical, the two paths agreeing on a shared column, the 32- and the 128-column workgroups of the thin path
bit-identical, and every argument error refused with a message before anything is launched.
"""
import ctypes

import pytest
import torch

import _trmm_ref as tr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def hip():
    from projectedlmc import _hip
    assert torch.cuda.is_available()
    return _hip


@pytest.fixture(autouse=True)
def _nothing_more_after_a_gpu_error():
    """a HIP error is sticky: the session ends at the first one instead of queueing the remaining cases behind it"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("HIP error, nothing more is started: %s" % e, returncode=3)


def _raw(hip, dtype):
    return getattr(hip.lib().cdll, "plmc_trmm_ut" + ("_f32" if dtype == F32 else "_f64"))


def _call(hip, ws, A, n, Z, shift, ns, ldz, ldy, dtype):
    """Z (q, n, ns) fp64 host values -> device buffers with the asked leading dimensions; returns the whole Y buffer (q, n, ldy)"""
    q = Z.shape[0]
    Zd = torch.full((q, n, ldz), float("nan"), dtype=dtype, device=DEV)     # the gap columns of Z are not read either
    Zd[:, :, :ns] = Z.to(dtype)
    sh = None if shift is None else shift.to(dtype).to(DEV).contiguous()
    Y = torch.full((q, n, ldy), tr.SENTINEL, dtype=dtype, device=DEV)
    hip.lib().call("plmc_trmm_ut", dtype, hip.ptr(A), ws.n_pad, ws.lda, ws.strideA, n, hip.ptr(Zd), ns, ldz, n * ldz, hip.ptr(sh),
                   hip.ptr(Y), ldy, n * ldy, q, hip.stream_ptr(DEV))
    return Y


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("ns", tr.NS)
@pytest.mark.parametrize("n", tr.SIZES)
def test_product_against_fp64_reference(hip, dtype, n, ns):
    for q in tr.QS:
        U, Z, shift = tr.make_inputs(n, q, ns, dtype)
        ws = tr.nan_factor_buffer(n, q, dtype, U)
        A = ws.A.to(DEV)
        for sh, ldz, ldy in ((None, ns, ns), (shift, ns + 3, ns + 5)):
            Y = _call(hip, ws, A, n, Z, sh, ns, ldz, ldy, dtype)
            Y2 = _call(hip, ws, A, n, Z, sh, ns, ldz, ldy, dtype)
            torch.cuda.synchronize()
            Yh = Y.cpu()
            live, gap = Yh[:, :, :ns], Yh[:, :, ns:]
            assert not bool(torch.isnan(Yh).any()), (n, q, ns, "NaN reached Y")
            assert bool((gap == tr.SENTINEL).all()), (n, q, ns, "the gap columns [ns, ldy) were written")
            bad = tr.violations(live, tr.reference(U, Z, sh), tr.bound(U, Z, sh, dtype))
            assert not bad, (n, q, ns, sh is not None, bad)
            assert torch.equal(Y, Y2), (n, q, ns, "two calls differ")


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_rows_past_n_of_a_larger_y_are_untouched(hip, dtype):
    """Y with room for n_pad rows: rows i >= n keep the sentinel on either path"""
    n, q = 129, 3
    for ns in (5, 17):
        U, Z, shift = tr.make_inputs(n, q, ns, dtype)
        ws = tr.nan_factor_buffer(n, q, dtype, U)
        A = ws.A.to(DEV)
        Zd = Z.to(dtype).to(DEV).contiguous()
        Y = torch.full((q, ws.n_pad, ns), tr.SENTINEL, dtype=dtype, device=DEV)
        hip.lib().call("plmc_trmm_ut", dtype, hip.ptr(A), ws.n_pad, ws.lda, ws.strideA, n, hip.ptr(Zd), ns, ns, n * ns,
                       hip.ptr(shift.to(dtype).to(DEV)), hip.ptr(Y), ns, ws.n_pad * ns, q, hip.stream_ptr(DEV))
        torch.cuda.synchronize()
        Yh = Y.cpu()
        assert bool((Yh[:, n:] == tr.SENTINEL).all())
        assert not tr.violations(Yh[:, :n], tr.reference(U, Z, shift), tr.bound(U, Z, shift, dtype))


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", [129, 300])
def test_the_two_paths_agree_on_a_shared_column(hip, dtype, n):
    q, ns = 3, 17
    U, Z, shift = tr.make_inputs(n, q, ns, dtype)
    ws = tr.nan_factor_buffer(n, q, dtype, U)
    A = ws.A.to(DEV)
    wide = _call(hip, ws, A, n, Z, shift, ns, ns, ns, dtype).cpu()
    for j in (0, 9, 16):
        thin = _call(hip, ws, A, n, Z[:, :, j:j + 1].contiguous(), shift, 1, 1, 1, dtype).cpu()
        bnd = tr.bound(U, Z[:, :, j:j + 1], shift, dtype)
        assert not tr.violations(wide[:, :, j:j + 1], thin.double(), bnd), (n, j)


def test_thin_path_workgroup_widths_are_bit_identical(hip):
    """q n_pad / 128 below the CU count takes 32-column workgroups, above it 128-column ones: the same sums in the same order.  256
    latents of one block row (at least as many workgroups as any MI355X partition has CUs) against the first three alone."""
    dtype, n, ns, q = F32, 100, 5, 256
    props = torch.cuda.get_device_properties(DEV)
    assert props.multi_processor_count <= q
    U, Z, shift = tr.make_inputs(n, q, ns, dtype)
    ws = tr.fr.HostWorkspace(n, q, 0, dtype, with_inverse=False)
    ws.A.fill_(float("nan"))
    Up = torch.full((q, ws.n_pad, ws.n_pad), float("nan"), dtype=torch.float64)
    Up[:, :n, :n] = torch.triu(U)
    tr.fr.write_factor(ws, Up, None, None)
    A = ws.A.to(DEV)
    big = _call(hip, ws, A, n, Z, shift, ns, ns, ns, dtype)
    small = _call(hip, ws, A, n, Z[:3].contiguous(), shift[:3].contiguous(), ns, ns, ns, dtype)
    torch.cuda.synchronize()
    assert torch.equal(big[:3], small)
    assert not tr.violations(big.cpu(), tr.reference(U, Z, shift), tr.bound(U, Z, shift, dtype))


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_argument_errors_are_refused_before_any_launch(hip, dtype):
    n, q, ns = 129, 3, 5
    U, Z, shift = tr.make_inputs(n, q, ns, dtype)
    ws = tr.nan_factor_buffer(n, q, dtype, U)
    A = ws.A.to(DEV)
    Zd = Z.to(dtype).to(DEV).contiguous()
    buf = torch.full((2 * q * n * ns,), tr.SENTINEL, dtype=dtype, device=DEV)
    Y = buf[:q * n * ns]
    fn, L = _raw(hip, dtype), hip.lib().cdll
    st = hip.stream_ptr(DEV)
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    good = dict(A=P(A), n_pad=ws.n_pad, lda=ws.lda, strideA=ws.strideA, n=n, Z=P(Zd), ns=ns, ldz=ns, strideZ=n * ns, shift=None, Y=P(Y),
                ldy=ns, strideY=n * ns, q=q)
    order = ["A", "n_pad", "lda", "strideA", "n", "Z", "ns", "ldz", "strideZ", "shift", "Y", "ldy", "strideY", "q"]
    esz = Zd.element_size()
    cases = {
        "null A": dict(A=None), "null Z": dict(Z=None), "null Y": dict(Y=None),
        "n < 1": dict(n=0), "n > n_pad": dict(n=ws.n_pad + 1), "ns < 1": dict(ns=0), "q < 1": dict(q=0),
        "ldz < ns": dict(ldz=ns - 1), "ldy < ns": dict(ldy=ns - 1),
        "Y is Z": dict(Y=P(Zd)),
        "Y starts inside Z": dict(Y=ctypes.c_void_p(Zd.data_ptr() + (q * n * ns - 1) * esz)),
        "Z starts inside Y": dict(Z=ctypes.c_void_p(Y.data_ptr() + (q * n * ns - 1) * esz)),
    }
    for name, change in cases.items():
        args = dict(good, **change)
        rc = fn(*[args[k] for k in order], st)
        msg = L.plmc_last_error().decode()
        assert rc != 0, name
        assert "plmc_trmm_ut" in msg or "trmm_ut_impl" in msg, (name, msg)
        assert len(msg.split(":", 1)[1].strip()) > 0, (name, msg)
    torch.cuda.synchronize()
    assert bool((buf == tr.SENTINEL).all()), "a refused call wrote something"
    assert torch.equal(Zd.cpu().double(), Z), "a refused call wrote into Z"
    assert fn(*[good[k] for k in order], st) == 0                      # and the same arguments unchanged are accepted
    torch.cuda.synchronize()
    assert not tr.violations(Y.reshape(q, n, ns).cpu(), tr.reference(U, Z, None), tr.bound(U, Z, None, dtype))
