"""plmc_cross_matvec_dx* (csrc/cross_matvec_dx.hip), LAPACK-style: the caller owns every buffer.  V stands in a buffer that is NaN wherever
the kernel must not read (rows from n on, columns r .. ldv), G is followed by NaN past its ns points, the scratch of the range split starts
as NaN and Jx stands inside a NaN frame that must stay NaN.  Every element is held against the fp64 autograd reference of
tests/_cross_matvec_dx_ref.py relative to the sum of absolute terms behind it: 1e-10 in fp64, the constants of
tests/test_gpu_posterior_dx_kernel.py times 2^-24 in fp32 (the unit derivative is the same code with g = 1, the weights are fp64).
One axis at a time around the base case matern52, d = 5, n = 129, n* = 37, q = 3, r = 3: every family, training sizes around the staged
chunk of 64 rows and the segment of 256, test sizes on both sides of the block of 64 test points, dimensions on both sides of every
capacity, one column with and without G, the cap, a chunked width, ldv > r, no output scale, a test point that is a training point, and
a range split over several workgroups."""
import functools
import zlib

import pytest
import torch

import _cross_matvec_dx_ref as cdx
import _posterior_dx_dense as pdd

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CAP = 8
TABLE_FAMILIES = ("rq", "periodic", "locally_periodic", "sm3")
GROUPS_BY_D = {1: [[0], [0]], 4: [[0, 1], [1, 2, 3]], 8: [[0, 1, 2, 3], [4, 5, 6, 7]], 9: [[0, 1, 2, 3, 4], [3, 7, 8]],
               16: [[0, 3, 4, 7], [8, 15], [2, 9], list(range(16))],
               17: [[0, 5, 16], [7, 8, 9, 15, 16], [1, 2, 3, 4]],
               32: [list(range(16)), list(range(16, 32)), [3, 4, 20, 31], [8, 15, 16, 17]]}      # those of test_gpu_posterior_dx_kernel.py
BASE = dict(family="matern52", d=5, n=129, ns=37, q=3, r=3, g=True, ldv=None, use_os=True, coincident=False)
SPLIT = dict(n=1100, ns=3)                                               # five segments, five workgroups along the training rows
CASES = ([dict()]
         + [dict(family=f) for f in pdd.FAMILIES]
         + [dict(n=n) for n in (1, 63, 64, 65, 257)]
         + [dict(ns=ns) for ns in (1, 63, 64, 65, 130)]
         + [dict(d=d) for d in (1, 4, 8, 9, 16, 17, 32)]
         + [dict(family="add", d=d) for d in (9, 32)]
         + [dict(family=f, d=d) for f in TABLE_FAMILIES for d in (1, 4, 8)]
         + [dict(family="rq", d=d) for d in (9, 16)]
         + [dict(r=1, g=False), dict(r=1), dict(r=2), dict(r=CAP)]
         + [dict(ldv=7), dict(r=1, g=False, ldv=1)]
         + [dict(family=f, use_os=False) for f in ("matern52", "add_disjoint", "periodic", "sm3")]
         + [dict(family=f, coincident=True) for f in pdd.FAMILIES]
         + [SPLIT, dict(family="sm3", **SPLIT), dict(r=1, g=False, **SPLIT)])


def _case_id(c):
    return "-".join("%s=%s" % kv for kv in c.items()) or "base"


@functools.lru_cache(maxsize=None)
def _reference(cid):
    """(case, problem, X, Xs, V, G, Jx, T) of a case, computed once for both element types and left unchanged."""
    case = next(c for c in CASES if _case_id(c) == cid)
    c = {**BASE, **case}
    seed = zlib.crc32(cid.encode()) % 100000
    if c["family"] == "add":
        p = pdd.problem("add_disjoint", c["d"], c["q"], seed, c["use_os"], groups=GROUPS_BY_D[c["d"]])
    else:
        p = pdd.problem(c["family"], c["d"], c["q"], seed, c["use_os"])
    X = pdd.igd.inputs(c["n"], c["d"], seed)
    Xs = pdd.query_points(c["ns"], c["d"], seed, X, c["coincident"])
    V, G = cdx.operands(c["n"], c["ns"], c["r"], c["q"], seed, c["g"])
    return (c, p, X, Xs, V, G) + cdx.reference(p.K, X, Xs, V, G)


@pytest.fixture(scope="module")
def eng():
    from projectedlmc import _engine
    assert torch.cuda.is_available()
    assert _engine._hip.lib().cdll.plmc_cross_matvec_max_cols() == CAP
    return _engine


def _call(eng, p, X, Xs, V, G, dt, ldv=None):
    """One raw call -> (Jx (q, ns, d) view of the framed buffer, the whole framed buffer, the frame's width)."""
    hip = eng._hip
    L = hip.lib()
    q, n, r = V.shape
    ns, d = Xs.shape
    Vbuf, Gbuf = cdx.buffers(V, G, dt, ldv=ldv)
    Vbuf = Vbuf.to(DEV)
    Gbuf = None if Gbuf is None else Gbuf.to(DEV)
    f = lambda t: None if t is None else t.to(DEV, dt).contiguous()
    Xc, Xsc, ell, osc = f(X), f(Xs), f(p.ell), f(p.oscale)
    pad = 67
    framed = torch.full((pad + q * ns * d + pad,), float("nan"), dtype=torch.float64, device=DEV)
    out = framed[pad:pad + q * ns * d].view(q, ns, d)
    nbytes = int(L.cdll.plmc_cross_matvec_dx_partials_bytes(n, ns, d, q))
    part = torch.full((nbytes // 8,), float("nan"), dtype=torch.float64, device=DEV) if nbytes else None
    eng._kernel_call(L, "plmc_cross_matvec_dx", dt, (eng.kind_code(p.kind), hip.ptr(Xc), n, hip.ptr(Xsc), ns, d), ell,
                     (hip.ptr(osc), hip.ptr(Vbuf), Vbuf.stride(1), Vbuf.stride(0), r, hip.ptr(Gbuf), hip.ptr(out), hip.ptr(part), q,
                      hip.stream_ptr(DEV)))
    torch.cuda.synchronize()
    return out, framed, pad


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_cross_matvec_dx_against_autograd(eng, case, dt):
    c, p, X, Xs, V, G, want, T = _reference(_case_id(case))
    out, framed, pad = _call(eng, p, X, Xs, V, G, dt, c["ldv"])
    again, _, _ = _call(eng, p, X, Xs, V, G, dt, c["ldv"])
    got = out.cpu()
    assert got.shape == want.shape and got.dtype == torch.float64
    assert bool(torch.isfinite(got).all())                            # nothing of the NaN around the live operands came in
    assert bool(torch.isnan(framed[:pad]).all()) and bool(torch.isnan(framed[pad + got.numel():]).all())     # the frame is untouched
    tol = cdx.tolerance(p.family, c["d"], dt)
    print("%s %s: worst err / (2^-24 sum |terms|) = %.3f" % (_case_id(case), dt, cdx.worst_ratio(got, want, T)))
    bad = cdx.violations(got, want, T, tol)
    assert bad == 0, (bad, cdx.worst_ratio(got, want, T))
    assert bool((got[:, :, p.zero] == 0.0).all())                      # dimensions no component uses
    assert torch.equal(out, again)                                    # fixed-order sums, no atomics
    splits = eng._hip.lib().cdll.plmc_cross_matvec_dx_splits(c["n"], c["ns"], c["q"])
    if c["n"] == SPLIT["n"]:
        assert splits == 5
    if c["n"] <= 256:
        assert splits == 1


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("g", [True, False], ids=["G", "noG"])
def test_an_element_does_not_depend_on_the_split_or_on_its_neighbours(eng, dt, g):
    """The summation order is a function of n alone: points 0..2 have the same bits in the call that splits the rows over five workgroups
    (n = 1100, n* = 3), as the first three of 130 points, as the last three of 130 points (other lanes, other blocks) and as the first
    three of 43 712 points, a call that does not split."""
    cid = _case_id(dict(r=1, g=False, **SPLIT) if not g else SPLIT)
    c, p, X, Xs, V, G, _, _ = _reference(cid)
    gen = torch.Generator().manual_seed(1)
    more = (2 * torch.rand(43709, c["d"], generator=gen, dtype=torch.float64) - 1).float().double()
    Gmore = None if G is None else torch.randn(c["q"], 43709, c["r"], generator=gen, dtype=torch.float64).float().double()
    cat = lambda a, b, dim: None if a is None else torch.cat([a, b], dim)
    L = eng._hip.lib().cdll
    assert L.plmc_cross_matvec_dx_splits(1100, 3, 3) == 5 and L.plmc_cross_matvec_dx_splits(1100, 43712, 3) == 1
    few = _call(eng, p, X, Xs, V, G, dt)[0]
    head = _call(eng, p, X, torch.cat([Xs, more[:127]]), V, cat(G, None if G is None else Gmore[:, :127], 1), dt)[0]
    tail = _call(eng, p, X, torch.cat([more[:127], Xs]), V, None if G is None else torch.cat([Gmore[:, :127], G], 1), dt)[0]
    unsplit = _call(eng, p, X, torch.cat([Xs, more]), V, cat(G, Gmore, 1), dt)[0]
    assert torch.equal(few, head[:, :3]) and torch.equal(few, tail[:, 127:]) and torch.equal(few, unsplit[:, :3])


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["float64", "float32"])
def test_the_python_wrapper_chunks_wide_v(eng, dt):
    """r = 19: three calls of 8, 8 and 3 columns whose fp64 results are added in chunk order."""
    c, p, X, Xs, _, _, _, _ = _reference("base")
    V, G = cdx.operands(c["n"], c["ns"], 2 * CAP + 3, c["q"], 9)
    want, T = cdx.reference(p.K, X, Xs, V, G)
    f = lambda t: None if t is None else t.to(DEV, dt)
    got = eng.cross_matvec_dx(p.kind, f(Xs), f(X), f(p.ell), f(p.oscale), f(V), f(G)).cpu()
    assert got.shape == want.shape and got.dtype == torch.float64
    print("r = 19 %s: worst err / (2^-24 sum |terms|) = %.3f" % (dt, cdx.worst_ratio(got, want, T)))
    assert cdx.violations(got, want, T, cdx.tolerance(p.family, c["d"], dt)) == 0
    one = eng.cross_matvec_dx(p.kind, f(Xs), f(X), f(p.ell), f(p.oscale), f(V[:, :, 0].contiguous())).cpu()        # (q, n): one column, no G
    w1, T1 = cdx.reference(p.K, X, Xs, V[:, :, :1], None)
    assert cdx.violations(one, w1, T1, cdx.tolerance(p.family, c["d"], dt)) == 0


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["float64", "float32"])
def test_a_test_point_on_a_training_point_gets_nothing_from_that_pair(eng, dt):
    """Matern-1/2 has no derivative at r = 0: with one training point and every test point on it every output is exactly 0."""
    for family in pdd.FAMILIES:
        p = pdd.problem(family, 5, 2, seed=5)
        X = pdd.igd.inputs(1, 5, seed=5)
        Xs = X.expand(3, 5).clone()
        V, G = cdx.operands(1, 3, 2, 2, seed=5)
        assert bool((_call(eng, p, X, Xs, V, G, dt)[0] == 0.0).all()), family


def test_argument_errors_launch_nothing_and_leave_the_output(eng):
    hip = eng._hip
    c, p, X, Xs, V, G, _, _ = _reference("base")
    dt = torch.float32
    q, n, r = V.shape
    ns, d = Xs.shape
    L = hip.lib()
    f = lambda t: t.to(DEV, dt).contiguous()
    Xc, Xsc, ell, osc, Vc, Gc = f(X), f(Xs), f(p.ell), f(p.oscale), f(V), f(G)
    out = torch.full((q, ns, d), -7.25, dtype=torch.float64, device=DEV)
    st = hip.stream_ptr(DEV)
    ok = dict(kind=3, X=hip.ptr(Xc), n=n, Xs=hip.ptr(Xsc), ns=ns, d=d, ell=hip.ptr(ell), os=hip.ptr(osc), V=hip.ptr(Vc), ldv=r, strideV=n * r,
              r=r, G=hip.ptr(Gc), Jx=hip.ptr(out), part=None, q=q)
    order = ("kind", "X", "n", "Xs", "ns", "d", "ell", "os", "V", "ldv", "strideV", "r", "G", "Jx", "part", "q")
    refused = [("null pointer", dict(X=None)), ("null pointer", dict(Xs=None)), ("null pointer", dict(ell=None)), ("null pointer", dict(V=None)),
               ("null pointer", dict(Jx=None)), ("G == NULL takes r == 1", dict(G=None)), ("n > 0", dict(n=0)), ("ns > 0", dict(ns=0)),
               ("r > 0", dict(r=0)), ("q <= 65535", dict(q=0)), ("plmc_cross_matvec_max_cols", dict(r=CAP + 1, ldv=CAP + 1)),
               ("ldv >= r", dict(ldv=r - 1)), ("strideV", dict(strideV=(n - 1) * r + r - 1)), ("plmc_max_dim", dict(d=33)),
               ("unknown kernel kind", dict(kind=5)), ("spline", dict(kind=4)), ("partials", dict(ns=1))]
    hip.prof_enable(["k_cross_matvec_dx"])
    try:
        hip.prof_collect()
        for word, change in refused:
            args = {**ok, **change}
            if word == "partials":                                    # n = 129 never splits: the split case's rows
                args.update(n=1100, strideV=1100 * r)
            with pytest.raises(RuntimeError, match=r"plmc_cross_matvec_dx_f32 failed.*" + word):
                L.call("plmc_cross_matvec_dx", dt, *(args[k] for k in order), st)
        ones = lambda *s: torch.ones(*s, dtype=dt, device=DEV)
        Xd = lambda dd, rows=n: torch.rand(rows, dd, dtype=dt, device=DEV)
        for kind, dd, table, word in (("matern52", 3, ones(q, 5, 3), "plmc_max_components"), ("sm", 9, ones(q, 2, 2, 9), "plmc_sm_max_dim"),
                                      ("periodic", 9, ones(q, 2, 9), "plmc_per_max_dim"), ("locally_periodic", 9, ones(q, 3, 9), "plmc_lper_max_dim"),
                                      ("rq", 17, ones(q, 18), "plmc_rq_max_dim"), ("sum(rbf,periodic)", 2, ones(q, 2, 7), "sum"),
                                      ("poly3", 3, ones(q, 4), "dot-product")):
            with pytest.raises(RuntimeError, match=r"plmc_cross_matvec_dx\w* failed.*" + word):
                eng._kernel_call(L, "plmc_cross_matvec_dx", dt, (eng.kind_code(kind), hip.ptr(Xd(dd)), n, hip.ptr(Xd(dd, ns)), ns, dd), table,
                                 (None, hip.ptr(Vc), r, n * r, r, hip.ptr(Gc), hip.ptr(out), None, q, st))
        torch.cuda.synchronize()
        assert "k_cross_matvec_dx" not in hip.prof_collect()          # nothing was launched
        assert bool((out == -7.25).all())                             # and the output is as it was
        L.call("plmc_cross_matvec_dx", dt, *(ok[k] for k in order), st)
        torch.cuda.synchronize()
        assert hip.prof_collect()["k_cross_matvec_dx"]["launches"] == 1 and not bool((out == -7.25).any())
    finally:
        hip.prof_enable(False)
