"""plmc_assemble*_pn_* and plmc_factorize*_pn_ex_* at the C ABI (include/plmc.h, "Per-point noise").

Assembly: the buffer, pre-filled with NaN, against the output of the entry point without a per-point vector with diagonal[:n] += s
applied in the element type -- an exact statement (one IEEE addition), which also pins that nothing outside the diagonal and nothing in
the identity padding moves and that the NaN positions coincide.  One case per assembly kernel shape and family: plain at d = 3, 7, 12 (the
DCAP 4 / 8 instantiations and the general kernel), _add with two components at d = 3 and d = 12 (table kernel and the general additive
kernel), _sm, _per, _rq, _lper, _sum with three different members, _dot with P = 2; n in {1, 127, 128, 130, 257} (one tile, a straddled
tile, three block rows), q = 2, stride_pn in {0, n, n + 3}, fp32 and fp64; values spread over 1e-3 .. 1e1.
Fused call: plmc_factorize*_pn_ex against plmc_assemble*_pn + plmc_potrf_ex on equal inputs, bit for bit over the factor buffer (factor,
solved augmented columns, inverse-factor region), logdet and info, at n = 300 and n = 1100 (more block rows than one group of the sweep:
the rows assembled on the helper stream), with and without the inverse factor, one plain kind and one table family."""
import pytest
import torch

import _fixed_noise_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
Q = 2

# label -> (kind, d, shape of the table behind q, shape of oscale behind q)
FAMILIES = {
    "plain-d3": ("matern52", 3, (3,), ()),
    "plain-d7": ("matern52", 7, (7,), ()),
    "plain-d12": ("matern52", 12, (12,), ()),
    "add-G2": ("matern52", 3, (2, 3), (2,)),
    "add-G2-d12": ("matern52", 12, (2, 12), (2,)),
    "sm": ("sm", 3, (2, 2, 3), (2,)),
    "per": ("periodic", 3, (2, 3), ()),
    "rq": ("rq", 3, (4,), ()),
    "lper": ("locally_periodic", 3, (3, 3), ()),
    "sum3": ("sum(rbf,periodic,rq)", 3, (3, 10), (3,)),
    "dot-P2": ("poly2", 3, (4,), ()),
}


@pytest.fixture(autouse=True)
def _nothing_more_after_a_gpu_error():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("HIP error, nothing more is started: %s" % e, returncode=3)


@pytest.fixture(scope="module")
def eng():
    from projectedlmc import _engine, _hip
    assert torch.cuda.is_available()
    return _engine, _hip


def _inputs(label, n, dtype):
    kind, d, tshape, oshape = FAMILIES[label]
    g = torch.Generator().manual_seed(n + d)
    f = lambda t: t.to(DEV, dtype).contiguous()
    X = f(2 * torch.rand(n, d, generator=g, dtype=torch.float64) - 1)
    table = f(0.5 + torch.rand(Q, *tshape, generator=g, dtype=torch.float64))
    osc = f(0.5 + torch.rand(Q, *oshape, generator=g, dtype=torch.float64))
    noise = f(0.05 + 0.1 * torch.rand(Q, generator=g, dtype=torch.float64))
    return kind, d, X, table, osc, noise


def _point_values(n, stride, dtype):
    """the per-point buffer as the library reads it and the (q, n) | (n) values in it, spread over 1e-3 .. 1e1"""
    g = torch.Generator().manual_seed(7 * n + stride)
    if stride == 0:
        buf = torch.pow(10.0, -3 + 4 * torch.rand(n, generator=g, dtype=torch.float64)).to(DEV, dtype)
        return buf, buf
    buf = torch.pow(10.0, -3 + 4 * torch.rand(Q, stride, generator=g, dtype=torch.float64)).to(DEV, dtype)
    return buf, buf[:, :n]


_baseline = {}


def _assemble(eng, label, n, dtype, pn=None, stride=0):
    """the NaN-filled buffer (q, n_pad, n_pad + NB) after plmc_assemble<infix>[_pn]"""
    _engine, _hip = eng
    L = _hip.lib()
    kind, d, X, table, osc, noise = _inputs(label, n, dtype)
    NB = L.cdll.plmc_block()
    n_pad = int(L.cdll.plmc_pad(n))
    lda = n_pad + NB
    A = torch.full((Q, n_pad, lda), float("nan"), dtype=dtype, device=DEV)
    st = _hip.stream_ptr(DEV)
    head = (_engine.kind_code(kind), _hip.ptr(X), n, d)
    if pn is None:
        _engine._kernel_call(L, "plmc_assemble", dtype, head, table, (_hip.ptr(osc), _hip.ptr(noise), _hip.ptr(A), lda, n_pad * lda, Q, st))
    else:
        _engine._kernel_call(L, "plmc_assemble_pn", dtype, head, table, (_hip.ptr(osc), _hip.ptr(noise), _hip.ptr(pn), stride, _hip.ptr(A), lda,
                             n_pad * lda, Q, st))
    torch.cuda.synchronize()
    return A


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("stride_extra", [None, 0, 3], ids=["shared", "stride-n", "stride-n+3"])
@pytest.mark.parametrize("n", [1, 127, 128, 130, 257])
@pytest.mark.parametrize("label", list(FAMILIES))
def test_assembly_adds_the_vector_to_the_diagonal_and_moves_nothing_else(eng, label, n, stride_extra, dtype):
    key = (label, n, dtype)
    if key not in _baseline:
        _baseline[key] = _assemble(eng, label, n, dtype).cpu()
    base = _baseline[key]
    stride = 0 if stride_extra is None else n + stride_extra
    buf, s = _point_values(n, stride, dtype)
    got = _assemble(eng, label, n, dtype, buf, stride).cpu()
    # what the baseline itself must look like: the upper tiles written, the padding's diagonal 1, NaN left of the diagonal tiles
    assert not torch.isnan(torch.diagonal(base, dim1=1, dim2=2)).any()
    if base.shape[1] > n:
        assert bool((torch.diagonal(base, dim1=1, dim2=2)[:, n:] == 1).all())
    ref.check_assembly(got, ref.expected_assembly(base, s.cpu(), n))


def _factor(eng, label, n, dtype, with_inverse, fused):
    """(A, logdet, info) of one factorisation with per-point noise and two right-hand sides, buffers zeroed first"""
    _engine, _hip = eng
    L = _hip.lib()
    kind, d, X, table, osc, noise = _inputs(label, n, dtype)
    buf, s = _point_values(n, n + 3, dtype)
    g = torch.Generator().manual_seed(11)
    rhs = torch.randn(Q, 2, n, generator=g, dtype=torch.float64).to(DEV, dtype).contiguous()
    ws = _engine.Workspace(n, Q, 2, dtype, DEV, with_inverse=with_inverse)
    ws.A.zero_()
    ws.Vd.zero_()
    st = _hip.stream_ptr(DEV)
    head = (_engine.kind_code(kind), _hip.ptr(X), n, d)
    bound = (noise + s.amin(-1)).contiguous()                       # eig_lo: noise + min_i pnoise
    flags = 1 if with_inverse else 0
    if not fused:
        _engine._kernel_call(L, "plmc_assemble_pn", dtype, head, table, (_hip.ptr(osc), _hip.ptr(noise), _hip.ptr(buf), n + 3, _hip.ptr(ws.A), ws.lda,
                             ws.strideA, Q, st))
    L.call("plmc_write_rhs", dtype, _hip.ptr(rhs), 2, n, _hip.ptr(ws.A), ws.lda, ws.strideA, 0, ws.naug_pad, Q, st)
    if fused:
        _engine._kernel_call(L, "plmc_factorize_pn_ex", dtype, head, table, (_hip.ptr(osc), _hip.ptr(noise), _hip.ptr(buf), n + 3, _hip.ptr(ws.A),
                             ws.n_pad, ws.lda, ws.naug, ws.strideA, _hip.ptr(ws.Vd), _hip.ptr(ws.logdet), _hip.ptr(ws.info), flags, Q,
                             _hip.ptr(bound), st))
    else:
        L.call("plmc_potrf_ex", dtype, _hip.ptr(ws.A), ws.n_pad, ws.lda, ws.naug, ws.strideA, _hip.ptr(ws.Vd), _hip.ptr(ws.logdet),
               _hip.ptr(ws.info), flags, Q, _hip.ptr(bound), st)
    torch.cuda.synchronize()
    return ws.A.cpu(), ws.logdet.cpu(), ws.info.cpu()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("with_inverse", [False, True], ids=["factor", "with-inverse"])
@pytest.mark.parametrize("n", [300, 1100])
@pytest.mark.parametrize("label", ["plain-d3", "rq"])
def test_fused_call_equals_assembly_then_sweep_bit_for_bit(eng, label, n, with_inverse, dtype):
    A1, ld1, info1 = _factor(eng, label, n, dtype, with_inverse, True)
    A2, ld2, info2 = _factor(eng, label, n, dtype, with_inverse, False)
    assert int(info1.abs().sum()) == 0 and torch.isfinite(ld1).all()
    ndiff = int((A1 != A2).sum())
    assert ndiff == 0, "%d elements of the factor buffer differ" % ndiff
    assert torch.equal(ld1, ld2) and torch.equal(info1, info2)
    if dtype == torch.float64:                                     # and it is the factor of K + diag(noise + s): the log-determinant
        kind, d, X, table, osc, noise = _inputs(label, n, dtype)
        s = _point_values(n, n + 3, dtype)[1]
        K = ref.noisy(ref.kernel(kind, X.cpu(), X.cpu(), table.cpu(), osc.cpu()), noise.cpu(), s.cpu())
        assert torch.allclose(ld1, torch.logdet(K), rtol=1e-10, atol=0)
