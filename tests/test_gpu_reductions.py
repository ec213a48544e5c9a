"""The reductions around the sweep alone, through the raw C ABI, against the fp64 references and the bound of tests/_reduce_ref.py:
plmc_posterior_moments, plmc_mix_posterior (csrc/posterior.hip), plmc_extract_col, plmc_wt_matvec, plmc_w_diag (csrc/potrf.hip).

Every buffer is written by the test and is NaN wherever the kernel must not read (the square part, the augmented columns beyond
1 + ns, the W tiles above the block diagonal, everything in front of the W columns); every output is prefilled with a sentinel and
has room behind what the call may write.  fp32 and fp64, q in {1, 3}.  Asserted per output: |got - ref| <= u_T |ref| +
(L + 4) 2^-53 sum |terms| -- a kernel that carried its sum in fp32 fails it -- no NaN, nothing written outside the outputs, two calls
bit-identical, plmc_extract_col's copy bit-identical to the column, both workgroup widths of plmc_wt_matvec bit-identical, and every
argument error refused with a message before anything is launched.

PLMC_REDUCE_RECORD=<file>: the largest measured error / bound per kernel and dtype is appended to that file as rows of a markdown
table (profiles/gemm_tn_accuracy.md holds one such run).
"""
import ctypes
import os

import pytest
import torch

import _reduce_ref as rr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32, F64 = torch.float32, torch.float64
GUARD = 64                                   # sentinel elements behind every output
_ROWS = {}


@pytest.fixture(scope="module")
def hip():
    from projectedlmc import _hip
    assert torch.cuda.is_available()
    yield _hip
    path = os.environ.get("PLMC_REDUCE_RECORD")
    if path and _ROWS:
        with open(path, "a") as f:
            for (name, dt), v in _ROWS.items():
                f.write("| %s | %s | %.3f |\n" % (name, dt, v))


@pytest.fixture(autouse=True)
def _nothing_more_after_a_gpu_error():
    """a HIP error is sticky: the session ends at the first one instead of queueing the remaining cases behind it"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("HIP error, nothing more is started: %s" % e, returncode=3)


def _bits(t):
    return t.contiguous().view({F32: torch.int32, F64: torch.int64}[t.dtype])


def _out(numel, dtype):
    return torch.full((numel + GUARD,), rr.SENTINEL, dtype=dtype, device=DEV)


def _split(buf, numel):
    """(the outputs, whether the guard behind them still holds the sentinel) on the host"""
    h = buf.cpu()
    return h[:numel], bool((h[numel:] == rr.SENTINEL).all())


def _record(name, dtype, got, ref, bnd):
    key = (name, "f32" if dtype == F32 else "f64")
    _ROWS[key] = max(_ROWS.get(key, 0.0), rr.worst_ratio(got, ref, bnd))


def _st(hip):
    return hip.stream_ptr(DEV)


# ------------------------------------------------------------------------------------------------ plmc_posterior_moments
def _moments(hip, dtype, Ad, n_pad, lda, ns, q):
    mean, vsq = _out(q * ns, dtype), _out(q * ns, dtype)
    hip.lib().call("plmc_posterior_moments", dtype, hip.ptr(Ad), n_pad, lda, n_pad * lda, ns, hip.ptr(mean), hip.ptr(vsq), q, _st(hip))
    return mean, vsq


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", rr.MOMENT_SIZES)
def test_posterior_moments(hip, dtype, n):
    wrong = []
    for q in rr.QS:
        for ns in rr.MOMENT_NS:
            zV = rr.moment_inputs(n, q, ns, dtype)
            n_pad = zV.shape[1]
            rm, rv, mm, mv = rr.moment_reference(zV)
            # the smallest leading dimension the header allows (the last vector of a row ends the row, that of the last row of the
            # last latent the buffer), and a roomier one
            for lda in (rr.moment_lda_min(n_pad, ns, dtype), rr.moment_lda_min(n_pad, ns, dtype) + 3 * rr.epv(dtype)):
                Ad = rr.moment_buffer(zV, dtype, lda).to(DEV)
                mean, vsq = _moments(hip, dtype, Ad, n_pad, lda, ns, q)
                mean2, vsq2 = _moments(hip, dtype, Ad, n_pad, lda, ns, q)
                torch.cuda.synchronize()
                tag = (n, q, ns, lda)
                for name, buf, buf2, ref, mag in (("mean", mean, mean2, rm, mm), ("vsq", vsq, vsq2, rv, mv)):
                    got, guard = _split(buf, q * ns)
                    got = got.reshape(q, ns)
                    bnd = rr.bound(ref, mag, n_pad, dtype)
                    bad = rr.violations(got, ref, bnd)
                    if bad or not guard or bool(torch.isnan(got).any()) or not torch.equal(_bits(buf), _bits(buf2)):
                        wrong.append((tag, name, "guard intact: %s" % guard, bad))
                    _record("plmc_posterior_moments " + name, dtype, got, ref, bnd)
    assert not wrong, wrong[:4]


# ------------------------------------------------------------------------------------------------ plmc_extract_col
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_extract_col(hip, dtype):
    ns = 5
    for n in rr.MOMENT_SIZES:
        for q in rr.QS:
            zV = rr.moment_inputs(n, q, ns, dtype)
            n_pad = zV.shape[1]
            A = rr.moment_buffer(zV, dtype)
            lda = A.shape[2]
            Ad = A.to(DEV)
            for c in (0, 1, ns):
                z, quad = _out(q * n_pad, dtype), _out(q, F64)
                hip.lib().call("plmc_extract_col", dtype, hip.ptr(Ad), n_pad, lda, n_pad * lda, c, hip.ptr(z), hip.ptr(quad), q, _st(hip))
                torch.cuda.synchronize()
                zh, zg = _split(z, q * n_pad)
                qh, qg = _split(quad, q)
                assert zg and qg, (n, q, c, "something behind an output was written")
                col = A[:, :, n_pad + c]
                assert torch.equal(_bits(zh.reshape(q, n_pad)), _bits(col)), (n, q, c, "z is not the column, rows to n_pad included")
                ref = (col.double() ** 2).sum(1)
                bnd = (n_pad + 4.0) * 2.0 ** -53 * ref
                assert not rr.violations(qh, ref, bnd), (n, q, c)
                _record("plmc_extract_col quad", dtype, qh, ref, bnd)


# ------------------------------------------------------------------------------------------------ plmc_wt_matvec, plmc_w_diag
def _w_calls(hip, dtype, ws, Ad, zd, q):
    """(alpha, kd) output buffers of one call each on the first q latents"""
    n_pad = ws.n_pad
    Wp = ctypes.c_void_p(Ad.data_ptr() + ws.wcol0 * Ad.element_size())
    alpha, kd = _out(q * n_pad, dtype), _out(q * n_pad, dtype)
    hip.lib().call("plmc_wt_matvec", dtype, Wp, n_pad, ws.lda, ws.strideA, hip.ptr(zd), hip.ptr(alpha), q, _st(hip))
    hip.lib().call("plmc_w_diag", dtype, Wp, n_pad, ws.lda, ws.strideA, hip.ptr(kd), q, _st(hip))
    return alpha, kd


def _w_check(dtype, ws, W, z, alpha, kd, q, tag):
    n_pad = ws.n_pad
    ra, ma, rk = rr.w_reference(W, z)
    wrong = []
    for name, buf, ref, mag in (("plmc_wt_matvec", alpha, ra, ma), ("plmc_w_diag", kd, rk, rk)):
        got, guard = _split(buf, q * n_pad)
        got = got.reshape(q, n_pad)
        bnd = rr.bound(ref, mag, n_pad, dtype)
        bad = rr.violations(got, ref, bnd)
        if bad or not guard or bool(torch.isnan(got).any()):
            wrong.append((tag, name, "guard intact: %s" % guard, bad))
        _record(name, dtype, got, ref, bnd)
    return wrong


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", rr.W_SIZES)
def test_wt_matvec_and_w_diag(hip, dtype, n):
    """q (n_pad / 128) < 128: the 32-column workgroups of plmc_wt_matvec"""
    wrong = []
    for q in rr.QS:
        W, z = rr.w_inputs(n, q, dtype)
        ws = rr.w_buffer(n, q, dtype, W)
        Ad, zd = ws.A.to(DEV), z.to(dtype).to(DEV)
        alpha, kd = _w_calls(hip, dtype, ws, Ad, zd, q)
        alpha2, kd2 = _w_calls(hip, dtype, ws, Ad, zd, q)
        torch.cuda.synchronize()
        wrong += _w_check(dtype, ws, W, z, alpha, kd, q, (n, q))
        if not (torch.equal(_bits(alpha), _bits(alpha2)) and torch.equal(_bits(kd), _bits(kd2))):
            wrong.append(((n, q), "two calls differ"))
    assert not wrong, wrong[:4]


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_wt_matvec_workgroup_widths_are_bit_identical(hip, dtype):
    """q (n_pad / 128) >= 128 takes the 128-column workgroups: 128 latents of one block row, against the bound, and the first three
    latents against a q = 3 call (32-column workgroups): the same sums in the same order"""
    n, q = 100, 128
    W, z = rr.w_inputs(n, q, dtype)
    ws = rr.w_buffer(n, q, dtype, W)
    assert q * (ws.n_pad // rr.NB) >= 128 > 3 * (ws.n_pad // rr.NB)
    Ad, zd = ws.A.to(DEV), z.to(dtype).to(DEV)
    alpha, kd = _w_calls(hip, dtype, ws, Ad, zd, q)
    alpha3, kd3 = _w_calls(hip, dtype, ws, Ad, zd, 3)
    torch.cuda.synchronize()
    wrong = _w_check(dtype, ws, W, z, alpha, kd, q, (n, q))
    assert not wrong, wrong[:4]
    m = 3 * ws.n_pad
    assert torch.equal(_bits(alpha[:m]), _bits(alpha3[:m])), "the two workgroup widths of plmc_wt_matvec differ"
    assert torch.equal(_bits(kd[:m]), _bits(kd3[:m]))


# ------------------------------------------------------------------------------------------------ plmc_mix_posterior
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", rr.MIX_CASES, ids=lambda c: "q%d-ns%d-p%d" % c)
def test_mix_posterior(hip, dtype, case):
    q, ns, p = case
    ml, vl, H = rr.mix_inputs(q, ns, p, dtype)
    d = lambda t: t.to(dtype).to(DEV).contiguous()
    mld, vld, Hd = d(ml), d(vl), d(H)
    for eps in rr.MIX_EPS:
        e = rr.mix_eps(eps, dtype)
        outs = []
        for _ in range(2):
            mean, var = _out(ns * p, dtype), _out(ns * p, dtype)
            hip.lib().call("plmc_mix_posterior", dtype, hip.ptr(mld), hip.ptr(vld), hip.ptr(Hd), q, ns, p, e, hip.ptr(mean), hip.ptr(var), _st(hip))
            outs.append((mean, var))
        torch.cuda.synchronize()
        rm, rv, mm, mv = rr.mix_reference(ml, vl, H, e)
        for k, (name, ref, mag) in enumerate((("mean", rm, mm), ("var", rv, mv))):
            got, guard = _split(outs[0][k], ns * p)
            got = got.reshape(ns, p)
            bnd = rr.bound(ref, mag, q, dtype)
            assert guard and not bool(torch.isnan(got).any()), (case, eps, name)
            assert not rr.violations(got, ref, bnd), (case, eps, name, rr.violations(got, ref, bnd))
            assert torch.equal(_bits(outs[0][k]), _bits(outs[1][k])), (case, eps, name, "two calls differ")
            _record("plmc_mix_posterior " + name, dtype, got, ref, bnd)


# ------------------------------------------------------------------------------------------------ argument errors
def _refused(hip, dtype, base, order, good, cases, outputs, inputs):
    """every case of `cases` (changes to the accepted arguments `good`) is refused with a message naming the function, nothing is
    written to `outputs` (sentinel-filled) or `inputs`, and the unchanged call is accepted afterwards"""
    L = hip.lib().cdll
    fn = getattr(L, base + ("_f32" if dtype == F32 else "_f64"))
    st = _st(hip)
    before = [t.cpu() for t in inputs]
    for name, change in cases.items():
        args = dict(good, **change)
        rc = fn(*[args[k] for k in order], st)
        msg = L.plmc_last_error().decode()
        assert rc != 0, (base, name)
        assert base[len("plmc_"):] in msg, (base, name, msg)
        assert len(msg.split(":", 1)[1].strip()) > 0, (base, name, msg)
    torch.cuda.synchronize()
    for t in outputs:
        assert bool((t == rr.SENTINEL).all()), (base, "a refused call wrote something")
    for t, b in zip(inputs, before):
        assert torch.equal(_bits(t.cpu()), _bits(b)), (base, "a refused call wrote into an input")
    assert fn(*[good[k] for k in order], st) == 0, (base, L.plmc_last_error().decode())
    torch.cuda.synchronize()


def _P(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + off * t.element_size())


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_posterior_moments_argument_errors(hip, dtype):
    n, q, ns = 100, 3, 4                                           # 1 + ns = 5: no multiple of the vector in either type
    e = rr.epv(dtype)
    zV = rr.moment_inputs(n, q, ns, dtype)
    n_pad = zV.shape[1]
    lda = rr.moment_lda_min(n_pad, ns, dtype)
    assert lda > n_pad + 1 + ns
    A = rr.moment_buffer(zV, dtype, lda)
    Ad = torch.cat([A.reshape(-1), torch.full((GUARD,), float("nan"), dtype=dtype)]).to(DEV)
    mean, vsq = _out(q * ns, dtype), _out(q * ns, dtype)
    order = ["A", "n_pad", "lda", "strideA", "ns", "mean", "vsq", "q"]
    good = dict(A=_P(Ad), n_pad=n_pad, lda=lda, strideA=n_pad * lda, ns=ns, mean=_P(mean), vsq=_P(vsq), q=q)
    cases = {
        "null A": dict(A=None), "null mean": dict(mean=None), "null vsq": dict(vsq=None),
        "n_pad = 0": dict(n_pad=0), "n_pad no block multiple": dict(n_pad=n), "ns = 0": dict(ns=0), "q = 0": dict(q=0),
        "lda holds 1 + ns columns but not the last vector": dict(lda=n_pad + 1 + ns),
        "lda one vector short": dict(lda=lda - e),
        "lda not a multiple of 16 bytes": dict(lda=lda + 1),
        "strideA off by one element": dict(strideA=n_pad * lda + 1),
        "A off by one element": dict(A=_P(Ad, 1)),
    }
    _refused(hip, dtype, "plmc_posterior_moments", order, good, cases, [mean, vsq], [Ad])
    rm, rv, mm, mv = rr.moment_reference(zV)
    assert not rr.violations(_split(mean, q * ns)[0].reshape(q, ns), rm, rr.bound(rm, mm, n_pad, dtype))
    assert not rr.violations(_split(vsq, q * ns)[0].reshape(q, ns), rv, rr.bound(rv, mv, n_pad, dtype))


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_extract_col_argument_errors(hip, dtype):
    n, q, ns = 100, 3, 4
    zV = rr.moment_inputs(n, q, ns, dtype)
    n_pad = zV.shape[1]
    A = rr.moment_buffer(zV, dtype)
    lda = A.shape[2]
    Ad = A.to(DEV)
    z, quad = _out(q * n_pad, dtype), _out(q, F64)
    order = ["A", "n_pad", "lda", "strideA", "c", "z", "quad", "q"]
    good = dict(A=_P(Ad), n_pad=n_pad, lda=lda, strideA=n_pad * lda, c=1, z=_P(z), quad=_P(quad), q=q)
    cases = {
        "null A": dict(A=None), "null z": dict(z=None), "null quad": dict(quad=None),
        "q = 0": dict(q=0), "n_pad = 0": dict(n_pad=0), "n_pad no block multiple": dict(n_pad=n),
        "lda < n_pad": dict(lda=n_pad - 4), "c < 0": dict(c=-1), "c behind the row": dict(c=lda - n_pad),
    }
    _refused(hip, dtype, "plmc_extract_col", order, good, cases, [z, quad], [Ad])
    assert torch.equal(_bits(_split(z, q * n_pad)[0].reshape(q, n_pad)), _bits(A[:, :, n_pad + 1]))


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_wt_matvec_and_w_diag_argument_errors(hip, dtype):
    n, q = 129, 3
    e = rr.epv(dtype)
    W, z = rr.w_inputs(n, q, dtype)
    ws = rr.w_buffer(n, q, dtype, W)
    n_pad = ws.n_pad
    Ad = torch.cat([ws.A.reshape(-1), torch.full((GUARD,), float("nan"), dtype=dtype)]).to(DEV)
    zd = z.to(dtype).to(DEV)
    alpha, kd = _out(q * n_pad, dtype), _out(q * n_pad, dtype)
    common = {
        "null W": dict(W=None), "q = 0": dict(q=0), "n_pad = 0": dict(n_pad=0), "n_pad no block multiple": dict(n_pad=n),
        "ldw < n_pad": dict(ldw=n_pad - e), "ldw not a multiple of 16 bytes": dict(ldw=ws.lda + 1),
        "W off by one element": dict(W=_P(Ad, ws.wcol0 + 1)), "strideW off by one element": dict(strideW=ws.strideA + 1),
    }
    good = dict(W=_P(Ad, ws.wcol0), n_pad=n_pad, ldw=ws.lda, strideW=ws.strideA, z=_P(zd), alpha=_P(alpha), kd=_P(kd), q=q)
    _refused(hip, dtype, "plmc_wt_matvec", ["W", "n_pad", "ldw", "strideW", "z", "alpha", "q"], good,
             dict(common, **{"null z": dict(z=None), "null alpha": dict(alpha=None)}), [alpha], [Ad, zd])
    _refused(hip, dtype, "plmc_w_diag", ["W", "n_pad", "ldw", "strideW", "kd", "q"], good, dict(common, **{"null kinv_diag": dict(kd=None)}),
             [kd], [Ad])
    assert not _w_check(dtype, ws, W, z, alpha, kd, q, "after the refusals")


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_mix_posterior_argument_errors(hip, dtype):
    q, ns, p = 3, 50, 7
    ml, vl, H = rr.mix_inputs(q, ns, p, dtype)
    d = lambda t: t.to(dtype).to(DEV).contiguous()
    mld, vld, Hd = d(ml), d(vl), d(H)
    mean, var = _out(ns * p, dtype), _out(ns * p, dtype)
    order = ["ml", "vl", "H", "q", "ns", "p", "eps", "mean", "var"]
    good = dict(ml=_P(mld), vl=_P(vld), H=_P(Hd), q=q, ns=ns, p=p, eps=0.0, mean=_P(mean), var=_P(var))
    cases = {
        "null mean_lat": dict(ml=None), "null var_lat": dict(vl=None), "null Ht": dict(H=None), "null mean": dict(mean=None),
        "null var": dict(var=None), "q = 0": dict(q=0), "ns = 0": dict(ns=0), "p = 0": dict(p=0),
    }
    _refused(hip, dtype, "plmc_mix_posterior", order, good, cases, [mean, var], [mld, vld, Hd])
    rm, rv, mm, mv = rr.mix_reference(ml, vl, H, 0.0)
    assert not rr.violations(_split(mean, ns * p)[0].reshape(ns, p), rm, rr.bound(rm, mm, q, dtype))
    assert not rr.violations(_split(var, ns * p)[0].reshape(ns, p), rv, rr.bound(rv, mv, q, dtype))
