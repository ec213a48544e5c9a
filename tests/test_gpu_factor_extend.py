"""plmc_factor_extend at the raw C ABI (csrc/factor_extend.hip), judged apart from the sweep: the source buffer holds
the element-type CPU LAPACK factor of the leading n x n block where a sweep would leave it (fill_buffer + write_factor: NaN in the strictly
lower tiles, above the block diagonal of W and behind it), V comes from plmc_write_rhs + plmc_potrs_aug as in a cached prediction, the
destination is NaN everywhere before the call.  What the call leaves is held to every assertion of the sweep (tests/_factor_ref.py:
structure with the NaN canaries, rho / e measures against the untouched thresholds, log det) for Case(family, n + m, ...);
tests/test_factor_extend_ref_host.py shows that the border formulas themselves pass them and that four mutations do not.

Shapes (tests/_factor_extend_ref.py SHAPES): single row; across a block edge with a larger n_pad; first row of a new block; inside the old
padding; full width; across the first block edge; 129 rows as two calls, the second in place."""
import pytest
import torch

import _factor_extend_ref as fx
import _factor_ref as fr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32, F64 = torch.float32, torch.float64
Q = 3
NB = 128


@pytest.fixture(scope="module")
def eng():
    from projectedlmc import _engine
    assert torch.cuda.is_available()
    yield _engine
    _engine.free_workspaces()
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def _nothing_more_after_a_gpu_error():
    """a HIP error is sticky: the session ends at the first one instead of queueing the remaining cases behind it"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("HIP error, nothing more is started: %s" % e, returncode=3)


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(family, n, dtype):
        key = (family, n, dtype)
        if key not in cache:
            cache[key] = fr.Case(family, n, Q, dtype)
        return cache[key]
    return get


def _solve_columns(ws, live, rhs):
    """rhs (q, c, live) into the first augmented columns of ws (the block is cleared), then U^-T of them: plmc_write_rhs + plmc_potrs_aug.
    plmc_write_rhs places the block at plmc_pad(n) of the n it is given: where the live rows end more than a block short of the buffer's
    n_pad (a factor inside a larger buffer) the columns are laid in with torch, as plmc_assemble_cross would with its explicit column."""
    from projectedlmc import _hip
    L, st = _hip.lib(), _hip.stream_ptr(DEV)
    r = rhs.to(DEV, ws.dtype).contiguous()
    if fr.pad(live) == ws.n_pad:
        L.call("plmc_write_rhs", ws.dtype, _hip.ptr(r), r.shape[1], live, _hip.ptr(ws.A), ws.lda, ws.strideA, 0, ws.naug_pad, ws.q, st)
    else:
        ws.A[:, :, ws.n_pad:ws.wcol0] = 0
        ws.A[:, :live, ws.n_pad:ws.n_pad + r.shape[1]] = r.transpose(1, 2)
    L.call("plmc_potrs_aug", ws.dtype, _hip.ptr(ws.A), ws.n_pad, ws.lda, r.shape[1], ws.wcol0, ws.strideA, _hip.ptr(ws.Vd), ws.q, st)


def _extend(eng, case, n, K=None, dst_rows=None):
    """The leading n x n factor of `case` (CPU LAPACK) extended on the GPU to (dst_rows or case.n) live rows in chunks of at most 128: the
    first call copies source -> destination, the later ones run in place on the destination.  -> destination workspace"""
    from projectedlmc import _hip
    L, st = _hip.lib(), _hip.stream_ptr(DEV)
    dt = case.dtype
    K = case.K if K is None else K
    total = case.n if dst_rows is None else dst_rows
    src = fx.source_workspace(case, n, NB, ws_cls=eng.Workspace, device=DEV, with_inverse=True)
    dst = eng.Workspace(case.n, Q, NB, dt, DEV, True)
    dst.A.fill_(float("nan"))
    dst.logdet.copy_(src.logdet)
    dst.info.fill_(-1)
    esz = 4 if dt == F32 else 8
    cur, k = src, n
    while k < total:
        c = min(NB, total - k)
        _solve_columns(cur, k, K[:, :k, k:k + c].transpose(1, 2))
        K22 = K[:, k:k + c, k:k + c].to(DEV, dt).contiguous()
        nbytes = int(L.cdll.plmc_factor_extend_scratch_bytes(cur.n_pad, c, esz))
        assert nbytes > 0
        scratch = torch.empty(Q * nbytes, dtype=torch.uint8, device=DEV)
        L.call("plmc_factor_extend", dt, _hip.ptr(cur.A), k, cur.n_pad, cur.lda, cur.wcol0, cur.strideA, c, _hip.ptr(K22),
               _hip.ptr(dst.A), dst.n_pad, dst.lda, dst.wcol0, dst.strideA, _hip.ptr(dst.logdet), _hip.ptr(dst.info), _hip.ptr(scratch), Q, st)
        torch.cuda.synchronize()
        cur, k = dst, k + c
    return dst


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("family", ["graded", "kernel"])
@pytest.mark.parametrize("n,m", fx.SHAPES, ids=["%d+%d" % s for s in fx.SHAPES])
def test_extended_buffer_meets_the_post_condition_of_the_sweep(eng, cases, n, m, family, dtype):
    case = cases(family, n + m, dtype)
    dst = _extend(eng, case, n)
    assert bool((dst.A[:, :, dst.n_pad:dst.wcol0] == 0).all()), "the destination's augmented block is not zero"
    bad, meas, tiles = fr.check_sweep(case, dst, None, device=DEV)
    print(family, n, m, dtype, {k: ["%.2e" % x for x in v.tolist()] for k, v in meas.items()}, tiles)
    assert not bad, bad
    # a right-hand side forward-substituted against the extended buffer
    rhs = case.rhs(5, [1.0, 1e4, 1.0, 1.0, 1e4])
    _solve_columns(dst, case.n, rhs)
    torch.cuda.synchronize()
    dst.naug = 5
    bad, meas, tiles = fr.check_sweep(case, dst, rhs, device=DEV)
    print("  with 5 solved columns", {k: ["%.2e" % x for x in meas[k].tolist()] for k in ("rho_Z", "e_Z")})
    assert not bad, bad


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_a_second_chunk_in_place_inside_and_across_the_padding(eng, cases, dtype):
    """(200, 40), then + 30 in place on the same buffer: rows 240 .. 269 cross the block edge at 256 inside the destination"""
    case = cases("graded", 270, dtype)
    from projectedlmc import _hip
    L, st = _hip.lib(), _hip.stream_ptr(DEV)
    dst = _extend(eng, case, 200, dst_rows=240)
    assert dst.info.tolist() == [0] * Q
    _solve_columns(dst, 240, case.K[:, :240, 240:].transpose(1, 2))
    K22 = case.K[:, 240:, 240:].to(DEV, dtype).contiguous()
    scratch = torch.empty(Q * int(L.cdll.plmc_factor_extend_scratch_bytes(dst.n_pad, 30, 4 if dtype == F32 else 8)), dtype=torch.uint8, device=DEV)
    L.call("plmc_factor_extend", dtype, _hip.ptr(dst.A), 240, dst.n_pad, dst.lda, dst.wcol0, dst.strideA, 30, _hip.ptr(K22),
           _hip.ptr(dst.A), dst.n_pad, dst.lda, dst.wcol0, dst.strideA, _hip.ptr(dst.logdet), _hip.ptr(dst.info), _hip.ptr(scratch), Q, st)
    torch.cuda.synchronize()
    bad, meas, _ = fr.check_sweep(case, dst, None, device=DEV)
    assert not bad, bad


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("k", [250, 256, 259])
def test_info_names_the_first_failing_pivot_of_the_border_and_the_neighbours_do_not_notice(eng, cases, k, dtype):
    """latent 1 of 3 with pivot k >= n made -0.5 U_kk^2 (fr.nonpd_matrix): info = [0, 1 + k, 0] through the Schur block, no fault, and
    latents 0 and 2 pass every check of a healthy extension"""
    case = cases("graded", 260, dtype)
    K = fr.nonpd_matrix(case, 1, k)
    # (latent 1 is U_ref^T U_ref recomputed: its leading block, whose factor the source holds, is case.K up to the rounding of that product)
    assert torch.equal(K[[0, 2]], case.K[[0, 2]])
    assert float((K[1, :250, :250] - case.K[1, :250, :250]).abs().max()) <= case.n_pad * fr.UNIT[dtype] * float(case.K[1].abs().max())
    dst = _extend(eng, case, 250, K=K)
    bad, _, _ = fr.check_sweep(case, dst, None, K=K, want_info=[0, k + 1, 0], device=DEV)
    assert not bad, bad


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_argument_errors_are_refused_before_any_launch(eng, cases, dtype):
    from projectedlmc import _hip
    L, st = _hip.lib(), _hip.stream_ptr(DEV)
    case = cases("graded", 260, dtype)
    n, m = 250, 10
    src = fx.source_workspace(case, n, NB, ws_cls=eng.Workspace, device=DEV, with_inverse=True)
    dst = eng.Workspace(case.n, Q, NB, dtype, DEV, True)
    dst.A.fill_(7.0)
    src0 = src.A.clone()
    K22 = case.K[:, n:, n:].to(DEV, dtype).contiguous()
    esz = 4 if dtype == F32 else 8
    nbytes = int(L.cdll.plmc_factor_extend_scratch_bytes(src.n_pad, m, esz))
    scratch = torch.zeros(Q * nbytes + 16, dtype=torch.uint8, device=DEV)
    logdet0 = src.logdet.clone()
    dst.logdet.copy_(logdet0)
    dst.info.fill_(-1)
    for bad_args in ((0, m, esz), (100, m, esz), (256, 0, esz), (256, 129, esz), (256, m, 2)):
        assert L.cdll.plmc_factor_extend_scratch_bytes(*bad_args) == -1, bad_args
    order = ["A_src", "n", "nps", "lds", "wcs", "ss", "m", "K22", "A_dst", "npd", "ldd", "wcd", "sd", "logdet", "info", "scratch", "q"]
    good = dict(A_src=_hip.ptr(src.A), n=n, nps=src.n_pad, lds=src.lda, wcs=src.wcol0, ss=src.strideA, m=m, K22=_hip.ptr(K22), A_dst=_hip.ptr(dst.A),
                npd=dst.n_pad, ldd=dst.lda, wcd=dst.wcol0, sd=dst.strideA, logdet=_hip.ptr(dst.logdet), info=_hip.ptr(dst.info),
                scratch=_hip.ptr(scratch), q=Q)
    in_place = dict(A_dst=good["A_src"], npd=src.n_pad, ldd=src.lda, wcd=src.wcol0, sd=src.strideA)
    errors = {
        "null source": dict(A_src=None), "null K22": dict(K22=None), "null destination": dict(A_dst=None), "null logdet": dict(logdet=None),
        "null info": dict(info=None), "null scratch": dict(scratch=None),
        "q = 0": dict(q=0), "n = 0": dict(n=0), "m = 0": dict(m=0), "m = 129": dict(m=129), "n > n_pad": dict(n=src.n_pad + 1),
        "source n_pad not a multiple of the block": dict(nps=src.n_pad - 1),
        "source lda not a multiple of the block": dict(lds=src.lda + 1),
        "no augmented block in the source": dict(wcs=src.n_pad),
        "source W columns outside lda": dict(wcs=src.lda),
        "destination too small for n + m": dict(npd=256, m=10, n=250),
        "destination W columns outside lda": dict(wcd=dst.lda),
        "destination wcol0 inside the square part": dict(wcd=dst.n_pad - NB),
        "unaligned scratch": dict(scratch=_hip.ptr(scratch[4:])),
        "batch stride shorter than a latent": dict(sd=dst.strideA - NB),
        "in place, n + m beyond n_pad": dict(in_place, n=250, m=10),
        "in place, another lda": dict(in_place, ldd=src.lda + 2 * NB, n=200),
        "overlapping buffers": dict(A_dst=_hip.ptr(src.A[0, 1:]), npd=src.n_pad, ldd=src.lda, wcd=src.wcol0, sd=src.strideA, n=100),
    }
    fn = getattr(L.cdll, "plmc_factor_extend_f32" if dtype == F32 else "plmc_factor_extend_f64")
    for name, change in errors.items():
        args = dict(good, **change)
        rc = fn(*[args[k] for k in order], st)
        msg = L.cdll.plmc_last_error().decode()
        assert rc != 0, name
        assert "factor_extend" in msg and len(msg.split(":", 1)[1].strip()) > 0, (name, msg)
    torch.cuda.synchronize()
    assert bool((dst.A == 7.0).all()) and bool((scratch == 0).all()), "a refused call wrote something"
    assert torch.equal(torch.nan_to_num(src.A), torch.nan_to_num(src0)), "a refused call wrote into the source"
    assert torch.equal(dst.logdet, logdet0) and dst.info.tolist() == [-1] * Q
