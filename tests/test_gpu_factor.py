"""What the blocked Cholesky sweep (csrc/potrf.hip) WRITES, against an fp64 CPU factorisation: U, W = U^-T, the solved augmented
columns, log det and info, element by element and by residual -- the LAPACK-style test of a factorisation (tests/_factor_ref.py:
inputs, measures, thresholds and where each comes from; tests/test_factor_ref_host.py: the same assertions pass for a CPU LAPACK
factorisation and fail for five seeded mutations).  The matrices are written into the factor buffer by the test (wishart /
graded / kernel families, kappa_2 <= 100, scales 1e-3 ... 1e3), everything the sweep must not read or need is NaN, and the raw
C ABI is called: plmc_potrf_ex, plmc_factorize_ex, plmc_write_rhs, plmc_potrs_aug, plmc_potrs_aug_kept.

Block rows m = n_pad / 128: 1 (one diagonal block), 2 and 3 (chain with panels), 8 (one full group), 9 (a second group of one
block row), 17 (three groups, the last of one row), and n = 200 / 1100 (padded rows; 1100 puts them inside the second group).

Every case goes through fr.check_sweep, which asserts: info; finiteness of all that is read; the NaN canary above the block diagonal
of W, finite tiles on and below it; identity / zero padded rows, exactly; the residuals rho_U, rho_W, rho_Z and the tile-wise
errors e_U, e_W, e_Z; log det against the factor's own diagonal and against the fp64 reference.  That the sweep reads no lower
tile and needs no initialised W column follows from finite results on a buffer whose lower tiles and W columns are NaN.

PLMC_FACTOR_RECORD=<file>: every measured figure (GPU, CPU LAPACK reference, ratio; per latent) is appended to that file as rows
of a markdown table (profiles/factor_residuals.md is one such run)."""
import contextlib
import os

import pytest
import torch

import _factor_ref as fr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32, F64 = torch.float32, torch.float64
Q = 3
_ROWS = []


@pytest.fixture(scope="module")
def eng():
    from projectedlmc import _engine
    assert torch.cuda.is_available()
    yield _engine
    path = os.environ.get("PLMC_FACTOR_RECORD")
    if path and _ROWS:
        by_case = {}
        for label, name, lat, v, r, ratio, tile in _ROWS:
            by_case.setdefault((label, name), []).append((v, r, ratio, tile))
        with open(path, "a") as f:                      # one row per case and measure; the latents side by side
            for (label, name), e in by_case.items():
                f.write("| %s | %s | %s | %s | %s | %s |\n" % (label, name, " / ".join("%.2e" % x[0] for x in e), " / ".join("%.2e" % x[1] for x in e),
                                                            " / ".join("%.2f" % x[2] for x in e),
                                                            "" if e[0][3] is None else " ".join("(%d,%d)" % x[3] for x in e)))


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
    """the matrices and their fp64 reference factorisations, made once per (family, n, dtype)"""
    cache = {}

    def get(family, n, dtype):
        key = (family, n, dtype)
        if key not in cache:
            cache[key] = fr.Case(family, n, Q, dtype)
        return cache[key]
    return get


def _knobs(dtype, split, grp):
    from projectedlmc import _hip
    st = contextlib.ExitStack()
    if dtype == F32:
        st.enter_context(_hip.knob("PLMC_SPLIT", str(split)))
    if grp:
        st.enter_context(_hip.knob("PLMC_GRP", str(grp)))
    return st


def _potrf(ws, case, wi, entry_args=None):
    """queue plmc_potrf_ex (or plmc_factorize_ex with entry_args = (kind, X, n, d, ell, oscale, noise)) on ws and wait"""
    from projectedlmc import _hip
    L, st = _hip.lib(), _hip.stream_ptr(DEV)
    eig = case.eig_lo.to(DEV, ws.dtype).contiguous()
    ws.info.fill_(-1)
    ws.logdet.fill_(float("nan"))
    tail = (_hip.ptr(ws.A), ws.n_pad, ws.lda, ws.naug, ws.strideA, _hip.ptr(ws.Vd), _hip.ptr(ws.logdet), _hip.ptr(ws.info), wi, ws.q,
            _hip.ptr(eig), st)
    if entry_args is None:
        L.call("plmc_potrf_ex", ws.dtype, *tail)
    else:
        L.call("plmc_factorize_ex", ws.dtype, *entry_args, *tail)
    torch.cuda.synchronize()


def _groups(ws, wi, split, grp):
    g = 8 if (not grp or ((wi & 4) and (wi & 1) and split != 0)) else grp
    return -(-ws.m // g)


def _factor_and_check(eng, case, wi, naug, split, grp, label, K=None, want_info=None):
    """one sweep on a NaN-canaried buffer and every assertion on what it wrote; a split scheme is run behind PLMC_SPLIT=0 of
    the same call and held to the split rule"""
    dtype = case.dtype
    ws = eng.Workspace(case.n, Q, naug, dtype, DEV, bool(wi & 1), keep_planes=bool(wi & 4))
    rhs = case.rhs(naug) if naug > 0 else None
    Kin = case.K if K is None else K
    bad, plain = [], None
    for sp in ([0] if (dtype == F64 or split == 0) else [0, split]):
        with _knobs(dtype, sp, grp):
            fr.fill_buffer(ws, Kin, rhs)
            _potrf(ws, case, wi)
        tag = "%s %s wi=%d naug=%d grp=%s" % (label, "f64" if dtype == F64 else "f32/split %d" % sp, wi, naug, grp or "default")
        b, meas, tiles = fr.check_sweep(case, ws, rhs, K=K, want_info=want_info, device=DEV, plain=plain if sp else None,
                                        groups=_groups(ws, wi, sp, grp) if sp else None, rows=_ROWS, label=tag)
        print(tag, {k: ["%.2e" % x for x in v.tolist()] for k, v in meas.items()}, tiles)
        bad += [(tag, x) for x in b]
        plain = meas
    assert not bad, bad


# dtype / PLMC_SPLIT modes
MODES = {"f64": (F64, 0), "f32s0": (F32, 0), "f32s2": (F32, 2), "f32s3": (F32, 3)}


@pytest.mark.parametrize("mode", ["f64", "f32s2"])
@pytest.mark.parametrize("n", [128, 256, 384, 1024, 2176, 200])
def test_factor_inverse_factor_and_solved_column_at_every_schedule_size(eng, cases, n, mode):
    dtype, split = MODES[mode]
    _factor_and_check(eng, cases("graded", n, dtype), 1, 1, split, None, "graded n=%d" % n)


# (mode, with_inverse, naug, PLMC_GRP): every value of every axis, at m = 9 and at n = 1100; a sweep that keeps its planes
# (with_inverse | 4 on a split scheme) ignores PLMC_GRP
AXES = [("f64", 1, 1, None), ("f64", 0, 130, 3), ("f64", 5, 0, None),
        ("f32s0", 1, 130, None), ("f32s0", 0, 0, 3), ("f32s0", 5, 1, None),
        ("f32s2", 1, 1, None), ("f32s2", 5, 130, None), ("f32s2", 0, 1, 3), ("f32s2", 1, 130, 3),
        ("f32s3", 1, 130, None), ("f32s3", 5, 1, None), ("f32s3", 0, 0, 3)]


@pytest.mark.parametrize("mode,wi,naug,grp", AXES, ids=["%s-wi%d-naug%d-grp%s" % (a, b, c, d or "def") for a, b, c, d in AXES])
@pytest.mark.parametrize("n", [1152, 1100])
def test_factor_over_dtype_split_inverse_columns_and_group_size(eng, cases, n, mode, wi, naug, grp):
    dtype, split = MODES[mode]
    _factor_and_check(eng, cases("graded", n, dtype), wi, naug, split, grp, "graded n=%d" % n)


@pytest.mark.parametrize("mode", ["f64", "f32s2"])
@pytest.mark.parametrize("family", ["wishart", "kernel"])
def test_factor_other_families(eng, cases, family, mode):
    """wishart: three noise levels; kernel: the Matern-5/2 covariance plus noise the engine normally sees -- the control"""
    dtype, split = MODES[mode]
    _factor_and_check(eng, cases(family, 1100, dtype), 1, 1, split, None, "%s n=1100" % family)


@pytest.mark.parametrize("mode", ["f64", "f32s0", "f32s2"])
def test_factorize_ex_is_the_two_calls_bit_for_bit(eng, cases, mode):
    """plmc_factorize_ex on (X, ell, oscale, noise) against plmc_assemble + plmc_potrf_ex on the same buffers (NaN everywhere
    before the assembly): the same bits in the whole buffer, log det and info, as include/plmc.h promises; and U^T U against the
    matrix the assembler wrote (read back between the two calls)."""
    from projectedlmc import _hip
    dtype, split = MODES[mode]
    case = cases("kernel", 1100, dtype)
    n, p = case.n, case.params
    L, st = _hip.lib(), _hip.stream_ptr(DEV)
    f = lambda t: t.to(DEV, dtype).contiguous()
    X, ell, osc, nz = f(p["X"]), f(p["ell"]), f(p["oscale"]), f(p["noise"])
    rhs = case.rhs(1)
    ws = eng.Workspace(n, Q, 1, dtype, DEV, True)
    asm = (_hip.KIND["matern52"], _hip.ptr(X), n, p["d"], _hip.ptr(ell), _hip.ptr(osc), _hip.ptr(nz))

    def prepare():
        ws.A.fill_(float("nan"))
        L.call("plmc_write_rhs", dtype, _hip.ptr(f(rhs)), 1, n, _hip.ptr(ws.A), ws.lda, ws.strideA, 0, ws.naug_pad, Q, st)

    with _knobs(dtype, split, None):
        prepare()
        L.call("plmc_assemble", dtype, *asm, _hip.ptr(ws.A), ws.lda, ws.strideA, Q, st)
        torch.cuda.synchronize()
        Kup = ws.A[:, :, :ws.n_pad].double().clone()
        _potrf(ws, case, 1)
        two = (ws.A.clone(), ws.logdet.clone(), ws.info.clone())
        prepare()
        _potrf(ws, case, 1, entry_args=asm)
    bits = torch.int32 if dtype == F32 else torch.int64
    assert ws.info.tolist() == [0] * Q and two[2].tolist() == [0] * Q
    assert torch.equal(ws.A.view(bits), two[0].view(bits)), "%d elements differ" % int((ws.A.view(bits) != two[0].view(bits)).sum())
    assert torch.equal(ws.logdet, two[1])
    # the assembled matrix: upper tiles and full diagonal blocks were written, the lower tiles still hold NaN
    blk = torch.arange(ws.n_pad, device=DEV) // 128
    assert bool(torch.isnan(Kup[:, blk[:, None] > blk[None, :]]).all()) and bool(torch.isfinite(Kup[:, blk[:, None] <= blk[None, :]]).all())
    Ksym = torch.triu(Kup) + torch.triu(Kup, 1).transpose(1, 2)
    U = torch.triu(ws.A[:, :, :ws.n_pad].double())
    rho = torch.linalg.matrix_norm(U.transpose(1, 2) @ U - Ksym) / (ws.n_pad * fr.UNIT[dtype] * torch.linalg.matrix_norm(Ksym[:, :n, :n]))
    print(mode, "rho_U against the assembled matrix", rho.tolist())
    # (1 + sqrt kappa) max(rho_ref, 1) with rho_ref < 1 (tests/test_factor_ref_host.py); a split scheme: the a-priori bound
    bound = (1 + torch.sqrt(case.kappa)) if split == 0 else fr.split_apriori_rho_u(case, 2)
    assert bool((rho.cpu() <= bound).all()), (rho.tolist(), bound.tolist())


def _col_scales(naug):
    return [1e4 if c % 3 == 1 else 1.0 for c in range(naug)]


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int64).clone()


def _substitute(ws, case, rhs2, kept):
    from projectedlmc import _hip
    L, st = _hip.lib(), _hip.stream_ptr(DEV)
    naug2 = rhs2.shape[1]
    r = rhs2.to(DEV, ws.dtype).contiguous()
    L.call("plmc_write_rhs", ws.dtype, _hip.ptr(r), naug2, case.n, _hip.ptr(ws.A), ws.lda, ws.strideA, 0, ws.naug_pad, Q, st)
    if kept:
        eig = case.eig_lo.to(DEV, ws.dtype).contiguous()
        L.call("plmc_potrs_aug_kept", ws.dtype, _hip.ptr(ws.A), ws.n_pad, ws.lda, naug2, ws.wcol0, ws.strideA, _hip.ptr(ws.Vd), Q, _hip.ptr(eig), st)
    else:
        L.call("plmc_potrs_aug", ws.dtype, _hip.ptr(ws.A), ws.n_pad, ws.lda, naug2, ws.wcol0, ws.strideA, _hip.ptr(ws.Vd), Q, st)
    torch.cuda.synchronize()


def _factor_then_substitute(eng, case, wi, split, naug2, kept, label, plain=None):
    """sweep with 130 augmented columns, then naug2 FRESH right-hand sides (columns 1e4 apart in magnitude) through the
    substitution; U and W must keep their bits.  -> (violations, measures, bits of the new Z)"""
    ws = eng.Workspace(case.n, Q, 130, case.dtype, DEV, True, keep_planes=bool(wi & 4))
    rhs2 = case.rhs(naug2, _col_scales(naug2), seed=1)
    with _knobs(case.dtype, split, None):
        fr.fill_buffer(ws, case.K, case.rhs(130))
        _potrf(ws, case, wi)
        before = _bits(ws.A[:, :, :ws.n_pad]), _bits(ws.A[:, :, ws.wcol0:ws.wcol0 + ws.n_pad])
        _substitute(ws, case, rhs2, kept)
    after = _bits(ws.A[:, :, :ws.n_pad]), _bits(ws.A[:, :, ws.wcol0:ws.wcol0 + ws.n_pad])
    bad = []
    if not (torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])):
        bad.append("the substitution changed U or W")
    ws.naug = naug2                                    # (what read_factor takes as the live columns)
    b, meas, tiles = fr.check_sweep(case, ws, rhs2, device=DEV, plain=plain, rows=_ROWS, label=label)
    print(label, {k: ["%.2e" % x for x in v.tolist()] for k, v in meas.items()}, tiles)
    return bad + b, meas, _bits(ws.A[:, :, ws.n_pad:ws.n_pad + ws.naug_pad])


@pytest.mark.parametrize("naug2", [77, 130])
@pytest.mark.parametrize("n", [1152, 2176])
def test_substitution_fp64_plain_and_kept_are_the_same_bits(eng, cases, n, naug2):
    case = cases("graded", n, F64)
    bad, _, z_plain = _factor_then_substitute(eng, case, 1, 0, naug2, False, "potrs_aug f64 n=%d naug'=%d" % (n, naug2))
    bad2, _, z_kept = _factor_then_substitute(eng, case, 1, 0, naug2, True, "potrs_aug_kept f64 n=%d naug'=%d" % (n, naug2))
    assert not bad and not bad2, (bad, bad2)
    assert torch.equal(z_plain, z_kept)


@pytest.mark.parametrize("naug2", [77, 130])
@pytest.mark.parametrize("n", [1152, 2176])
def test_substitution_fp32_plain_split_and_kept_planes(eng, cases, n, naug2):
    """plmc_potrs_aug_f32 behind a PLMC_SPLIT=0 sweep (plain thresholds), behind the default sweep, and plmc_potrs_aug_kept_f32
    behind sweeps that kept their planes (with_inverse 1 | 4, Vd of plmc_vd_blocks_keep) under both split schemes: the split rule
    against the plain run"""
    case = cases("graded", n, F32)
    tag = "f32 n=%d naug'=%d" % (n, naug2)
    bad, plain, _ = _factor_then_substitute(eng, case, 1, 0, naug2, False, "potrs_aug split 0 " + tag)
    for wi, split, kept, name in ((1, 2, False, "potrs_aug split 2 "), (5, 2, True, "potrs_aug_kept split 2 "), (5, 3, True, "potrs_aug_kept split 3 ")):
        b, _, _ = _factor_then_substitute(eng, case, wi, split, naug2, kept, name + tag, plain=plain)
        bad += [(name, x) for x in b]
    assert not bad, bad


@pytest.mark.parametrize("mode", ["f64", "f32s2"])
@pytest.mark.parametrize("k", [5, 48, 127, 130, 1030, 1099])
def test_info_is_one_plus_the_first_failing_pivot_and_the_neighbours_do_not_notice(eng, cases, k, mode):
    """latent 1 of 3 with pivot k = -0.5 U_kk^2 (fr.nonpd_matrix; CPU cholesky_ex fails there: tests/test_factor_ref_host.py):
    info = [0, k + 1, 0], and latents 0 and 2 pass every check of a healthy sweep"""
    dtype, split = MODES[mode]
    case = cases("graded", 1100, dtype)
    _factor_and_check(eng, case, 1, 1, split, None, "non-PD pivot %d, n=1100" % k, K=fr.nonpd_matrix(case, 1, k), want_info=[0, k + 1, 0])
