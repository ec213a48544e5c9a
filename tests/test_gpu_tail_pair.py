"""Paired tails of the split-engine sweep (csrc/potrf.hip, Sweep::pair; PLMC_TAIL_PAIR): the far part of every second tail is
applied together with the next one as one product of twice the depth, from four rolling plane slots.

Small groups (PLMC_GRP=2) put many groups into a small matrix.  Block rows m = n_pad / 128 and groups ng = m / 2:
  n_pad  512, 768   2 and 3 groups: no near of double depth and no far -- the launches of PLMC_TAIL_PAIR=0
  n_pad 1024        4 groups: every one of the four slots is used, near(1) is the first product over two slots
  n_pad 1536        6 groups: near(1), far(1), near(3) of double depth; the slots wrap (groups 4, 5 into slots 0, 1)
  n_pad 1792        7 groups: an odd number of tails, the last of them a near of single depth
  n_pad 2816       11 groups: the slots wrap twice, four fars
fp32, q = 2 latents, Matern-5/2 covariance plus a noise of 1e-2, 3 augmented columns, with the inverse factor; PLMC_SPLIT 2 and 3.

What is asserted:
  * fp64 bounds: U, W and the solved columns against an fp64 CPU factorisation, through tests/_factor_ref.check_sweep with the
    bounds tests/test_gpu_factor.py holds a split scheme to (the split rule against PLMC_SPLIT=0 of the same call, the a-priori
    bound of rho_U, structure, log det); the figures with and without pairing are printed side by side (-s);
  * schedule independence: with pairing on, the one-stream schedule, the look-ahead and PLMC_CHAIN=0 give the same bits in the
    whole factor buffer, log det and info;
  * two sweeps in flight from two caller streams give the bits of the same sweeps one after the other;
  * 130 augmented columns (two column tiles, the most the factorisation tests use): the same bounds and the same bits."""
import contextlib

import pytest
import torch

import _factor_ref as fr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32 = torch.float32
Q = 2
GRP = 2
N_PADS = [512, 768, 1024, 1536, 1792, 2816]


class MaternCase(fr.Case):
    """q Matern-5/2 covariance matrices plus a noise of 1e-2 on n points in [-1, 1]^3, rounded to fp32 (the fp64 reference
    factorises the rounded matrix); kappa_2 is whatever it is -- the thresholds of _factor_ref carry it."""

    def __init__(self, n, q, seed=0):
        from oracle import gp_math as gm
        gen = torch.Generator().manual_seed(1000003 * seed + 7919 * n + 4)
        self.family, self.n, self.q, self.dtype, self.n_pad, self.gen = "matern52+1e-2", n, q, F32, fr.pad(n), gen
        d = 3
        X = 2 * torch.rand(n, d, generator=gen, dtype=torch.float64) - 1
        ell = 0.10 + 0.06 * torch.rand(q, d, generator=gen, dtype=torch.float64)
        noise = torch.full((q,), 1e-2, dtype=torch.float64)
        K = gm.kernel_matrix("matern", X, X, ell, None, 2.5) + noise.reshape(-1, 1, 1) * torch.eye(n, dtype=torch.float64)
        self.params = None
        self.K = fr._round(K, F32)
        ev = torch.linalg.eigvalsh(self.K)
        self.eig_min, self.eig_max = ev[:, 0].clone(), ev[:, -1].clone()
        self.kappa = self.eig_max / self.eig_min
        self.eig_lo = 0.9 * noise                       # K - noise I is positive semi-definite; rounding moves eigenvalues by << 1e-3
        assert bool((self.eig_lo <= self.eig_min).all()), (self.eig_lo.tolist(), self.eig_min.tolist())
        self._ref = None
        self._lapack = None


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
    """the matrices and their fp64 reference factorisations, made once per n and shared by every test"""
    cache = {}

    def get(n):
        if n not in cache:
            cache[n] = MaternCase(n, Q)
        return cache[n]
    return get


def _knobs(split, pair, extra=()):
    from projectedlmc import _hip
    st = contextlib.ExitStack()
    for name, val in (("PLMC_SPLIT", split), ("PLMC_GRP", GRP), ("PLMC_TAIL_PAIR", pair)) + tuple(extra):
        st.enter_context(_hip.knob(name, str(val)))
    return st


def _potrf(ws, case, stream=None):
    """queue plmc_potrf_ex with the inverse factor on the current (or the given) stream"""
    from projectedlmc import _hip
    L = _hip.lib()
    st = _hip.stream_ptr(DEV) if stream is None else stream.cuda_stream
    eig = case.eig_lo.to(DEV, ws.dtype).contiguous()
    L.call("plmc_potrf_ex", ws.dtype, _hip.ptr(ws.A), ws.n_pad, ws.lda, ws.naug, ws.strideA, _hip.ptr(ws.Vd), _hip.ptr(ws.logdet),
           _hip.ptr(ws.info), 1, ws.q, _hip.ptr(eig), st)
    return eig                                         # (kept alive by the caller until the sweep is done)


def _bits(ws):
    return ws.A.view(torch.int32).clone(), ws.logdet.clone(), ws.info.clone()


def _fp64_bounds(eng, case, naug, split):
    ws = eng.Workspace(case.n, Q, naug, F32, DEV, True)
    rhs = case.rhs(naug)
    groups = -(-ws.m // GRP)
    runs = {}
    for name, sp, pair in (("plain", 0, 1), ("unpaired", split, 0), ("paired", split, 1)):
        with _knobs(sp, pair):
            fr.fill_buffer(ws, case.K, rhs)
            ws.info.fill_(-1)
            ws.logdet.fill_(float("nan"))
            _potrf(ws, case)
            torch.cuda.synchronize()
        plain = runs["plain"][1] if sp else None
        runs[name] = fr.check_sweep(case, ws, rhs, device=DEV, plain=plain, groups=groups if sp else None)[:2] + (_bits(ws)[0],)
    tag = "n_pad=%d naug=%d split=%d kappa=%s" % (case.n_pad, naug, split, ["%.1e" % k for k in case.kappa.tolist()])
    for k in runs["paired"][1]:
        print(tag, k, " plain", ["%.2e" % x for x in runs["plain"][1][k].tolist()], " unpaired", ["%.2e" % x for x in runs["unpaired"][1][k].tolist()],
              " paired", ["%.2e" % x for x in runs["paired"][1][k].tolist()])
    ndiff = int((runs["paired"][2] != runs["unpaired"][2]).sum())
    print(tag, "elements of the factor buffer that differ between paired and unpaired:", ndiff)
    # the split rule, the a-priori bound, structure and log det: for the paired sweep (and, unchanged code, the unpaired one)
    assert not runs["paired"][0], runs["paired"][0]
    assert not runs["unpaired"][0], runs["unpaired"][0]
    if groups <= 3:                                    # no double depth and no far: the same launches, hence the same bits
        assert ndiff == 0
    del ws


@pytest.mark.parametrize("split", [2, 3])
@pytest.mark.parametrize("n_pad", N_PADS)
def test_paired_sweep_against_fp64(eng, cases, n_pad, split):
    _fp64_bounds(eng, cases(n_pad), 3, split)


def _schedules(eng, case, naug, split):
    ws = eng.Workspace(case.n, Q, naug, F32, DEV, True)
    rhs = case.rhs(naug)
    got = {}
    for name, extra in (("one stream", (("PLMC_SERIAL", 1),)), ("look-ahead", ()), ("look-ahead, PLMC_CHAIN=0", (("PLMC_CHAIN", 0),)),
                        ("one stream, PLMC_CHAIN=0", (("PLMC_SERIAL", 1), ("PLMC_CHAIN", 0)))):
        with _knobs(split, 1, extra):
            fr.fill_buffer(ws, case.K, rhs)
            ws.info.fill_(-1)
            ws.logdet.fill_(float("nan"))
            _potrf(ws, case)
            torch.cuda.synchronize()
        got[name] = _bits(ws)
    A, ld, info = got["one stream"]
    assert info.tolist() == [0] * Q and bool(torch.isfinite(ld).all())
    for name, (A2, ld2, info2) in got.items():
        # NaN canaries compare as bit patterns: the whole buffer
        ndiff = int((A2 != A).sum())
        assert ndiff == 0, "%s: %d elements of the factor buffer differ from the one-stream schedule" % (name, ndiff)
        assert torch.equal(ld2, ld) and torch.equal(info2, info), name
    del ws


@pytest.mark.parametrize("split", [2, 3])
@pytest.mark.parametrize("n_pad", N_PADS)
def test_paired_sweep_is_schedule_independent(eng, cases, n_pad, split):
    _schedules(eng, cases(n_pad), 3, split)


@pytest.mark.parametrize("split", [2, 3])
def test_full_height_augmented_columns(eng, cases, split):
    """130 augmented columns = two column tiles in near and far (odd and even group counts are covered by 7 groups)"""
    _fp64_bounds(eng, cases(1792), 130, split)
    _schedules(eng, cases(1792), 130, split)


@pytest.mark.parametrize("split", [2, 3])
def test_two_paired_sweeps_in_flight(eng, cases, split):
    """Two sweeps from two caller streams, each with its own buffers and its own set of helper streams and events, both rolling
    over four slots (11 and 6 groups; the shorter one runs twice in a row beside the longer one, so a sweep starts on slots a
    sweep of the other context is still reading from): the bits of the same sweeps one after the other."""
    probs = []
    for n_pad in (2816, 1536):
        case = cases(n_pad)
        ws = eng.Workspace(case.n, Q, 3, F32, DEV, True)
        fr.fill_buffer(ws, case.K, case.rhs(3))
        probs.append((case, ws, ws.A.clone(), 1 if n_pad == 2816 else 2))
    with _knobs(split, 1):
        ref = []
        for case, ws, A_in, _ in probs:                 # one after the other, one stream
            _potrf(ws, case)
            torch.cuda.synchronize()
            ref.append(_bits(ws))
            assert ws.info.tolist() == [0] * Q
        streams = [torch.cuda.Stream(DEV) for _ in probs]
        for rep in range(4):
            torch.cuda.synchronize()
            alive = []
            for (case, ws, A_in, times), s in zip(probs, streams):
                with torch.cuda.stream(s):
                    for _ in range(times):
                        ws.A.copy_(A_in, non_blocking=True)
                        alive.append(_potrf(ws, case, s))
            torch.cuda.synchronize()
            for k, ((case, ws, A_in, _), (A, ld, info)) in enumerate(zip(probs, ref)):
                ndiff = int((ws.A.view(torch.int32) != A).sum())
                assert ndiff == 0, "round %d, stream %d: %d elements differ from the sequential sweep" % (rep, k, ndiff)
                assert torch.equal(ws.logdet, ld) and torch.equal(ws.info, info)
    del probs, ref
