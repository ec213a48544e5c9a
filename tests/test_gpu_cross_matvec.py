"""plmc_cross_matvec* (csrc/cross_matvec.hip) through the C ABI, LAPACK-style: the caller owns every buffer.  V stands in a buffer that is
NaN wherever the kernel must not read (rows from n on, columns outside its r), Out inside a NaN frame that must stay NaN, the scratch of
the range split starts as NaN, and a sum's table has NaN in the slots a member does not own.  Every element is held against the fp64
reference and the a-priori bound of tests/_cross_matvec_ref.py,
    |Out - exact| <= sum_i b_F |V_ic| + u |exact| + (n + 4) 2^-53 sum_i |k_i V_ic|.
One axis at a time around the base case matern52, d = 3, n = 257, n* = 65, q = 3, r = 3: every family, training sizes on both sides of
the staged chunk, of a segment of 256 rows and of the range split, test sizes on both sides of the block of 64 test points, one latent,
one column / the cap, dimensions on both sides of every capacity, no output scale, the alpha form (ldv = 1) and the strided [alpha | B]
form."""
import functools
import zlib

import pytest
import torch

import _cross_matvec_ref as cm

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CAP = 8
BASE = dict(family="matern52", d=3, n=257, ns=65, q=3, r=3, use_os=True, form="strided")
SPLIT = dict(n=700, ns=1)                                             # three segments, three workgroups along the training rows
TABLE8 = ("sm3", "periodic", "locally_periodic", "sum")
CASES = ([dict()]
         + [dict(family=f) for f in cm.FAMILIES if f not in ("matern52", "spline")]
         + [dict(family="spline", d=1)]
         + [dict(n=n) for n in (130, 700)]
         + [dict(ns=ns) for ns in (1, 130)]
         + [dict(q=1)]
         + [dict(r=1), dict(r=CAP), dict(r=1, form="alpha"), dict(r=1, form="alpha", **SPLIT)]
         + [dict(d=d) for d in (1, 8, 32)]
         + [dict(family="add_disjoint", d=d) for d in (1, 8, 16, 32)]
         + [dict(family=f, d=d) for f in ("rq", "poly3") for d in (1, 8, 16)]
         + [dict(family=f, d=d) for f in TABLE8 for d in (1, 8)]
         + [dict(family=f, use_os=False) for f in ("matern52", "add_disjoint", "periodic", "sm3", "linear")]
         + [SPLIT, dict(family="sum", **SPLIT), dict(r=CAP, **SPLIT)])


def _case_id(c):
    return "-".join("%s=%s" % kv for kv in c.items()) or "base"


@functools.lru_cache(maxsize=None)
def _problem(cid):
    """(case, problem, X, Xs, V) of a case, built once for both element types and left unchanged."""
    case = next(c for c in CASES if _case_id(c) == cid)
    c = {**BASE, **case}
    seed = zlib.crc32(cid.encode()) % 100000
    p = cm.problem(c["family"], c["d"], c["q"], seed, c["use_os"])
    X, Xs = cm.inputs(c["family"], c["n"], c["ns"], c["d"], seed)
    return c, p, X, Xs, cm.columns(c["n"], c["r"], c["q"], seed)


@pytest.fixture(scope="module")
def eng():
    from projectedlmc import _engine
    assert torch.cuda.is_available()
    assert _engine._hip.lib().cdll.plmc_cross_matvec_max_cols() == CAP
    return _engine


def _call(eng, p, X, Xs, V, dt, form):
    """One raw call -> (Out (q, ns, r) view of the framed buffer, the whole framed buffer, the frame's width)."""
    hip = eng._hip
    L = hip.lib()
    q, n_, r = V.shape
    n = n_
    ns, d = Xs.shape
    if form == "alpha":                                               # (q, n_pad): r = 1, ldv = 1, strideV = n_pad
        n_pad = (n_ + 127) // 128 * 128 + (128 if n_ % 128 == 0 else 0)
        buf = torch.full((q, n_pad), float("nan"), dtype=dt)
        buf[:, :n_] = V[:, :, 0].to(dt)
        buf = buf.to(DEV)
        vptr, ldv, strideV = buf.data_ptr(), 1, n_pad
    else:                                                             # rows of [alpha | B | padding]: V behind one foreign column
        rows, ldv = n_ + 5, r + 3
        buf = torch.full((q, rows, ldv), float("nan"), dtype=dt)
        buf[:, :n_, 1:1 + r] = V.to(dt)
        buf = buf.to(DEV)
        vptr, strideV = buf[:, :, 1:].data_ptr(), rows * ldv
    f = lambda t: None if t is None else t.to(DEV, dt).contiguous()
    Xc, Xsc, ell, osc = f(X), f(Xs), f(p.ell), f(p.oscale)
    pad = 67
    framed = torch.full((pad + q * ns * r + pad,), float("nan"), dtype=dt, device=DEV)
    out = framed[pad:pad + q * ns * r].view(q, ns, r)
    nbytes = int(L.cdll.plmc_cross_matvec_partials_bytes(n, ns, r, q))
    part = torch.full((nbytes // 8,), float("nan"), dtype=torch.float64, device=DEV) if nbytes else None
    eng._kernel_call(L, "plmc_cross_matvec", dt, (eng.kind_code(p.kind), hip.ptr(Xc), n, hip.ptr(Xsc), ns, d), ell,
                     (hip.ptr(osc), vptr, ldv, strideV, r, hip.ptr(out), hip.ptr(part), q, hip.stream_ptr(DEV)))
    torch.cuda.synchronize()
    return out, framed, pad


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_cross_matvec_against_the_dense_product(eng, case, dt):
    c, p, X, Xs, V = _problem(_case_id(case))
    exact, bound = cm.reference(p, Xs, X, V, dt)
    out, framed, pad = _call(eng, p, X, Xs, V, dt, c["form"])
    again, _, _ = _call(eng, p, X, Xs, V, dt, c["form"])
    got = out.cpu()
    assert bool(torch.isfinite(got).all())                            # nothing of the NaN around the live operands came in
    assert bool(torch.isnan(framed[:pad]).all()) and bool(torch.isnan(framed[pad + got.numel():]).all())     # the frame is untouched
    print("%s %s: largest share of the bound %.3f" % (_case_id(case), dt, cm.worst_share(got, exact, bound)))
    bad = cm.violations(got, exact, bound)
    assert bad == 0, (bad, cm.worst_share(got, exact, bound))
    assert torch.equal(out, again)                                    # fixed-order sums, no atomics
    splits = eng.cross_matvec_splits(c["n"], c["ns"], c["q"])
    if c["n"] == SPLIT["n"] and c["ns"] == SPLIT["ns"]:
        assert splits == 3
    if c["n"] <= 256:
        assert splits == 1


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["float64", "float32"])
def test_an_element_does_not_depend_on_the_split_or_on_its_neighbours(eng, dt):
    """The summation order is a function of n alone: test point s has the same bits alone in a call that splits the rows over three
    workgroups (n* = 1) and as one of 43 712 points of a call that does not."""
    c, p, X, Xs, V = _problem(_case_id(SPLIT))
    g = torch.Generator().manual_seed(1)
    many = torch.cat([Xs, (2 * torch.rand(43711, 3, generator=g, dtype=torch.float64) - 1).float().double()])
    assert eng.cross_matvec_splits(700, 1, 3) == 3 and eng.cross_matvec_splits(700, 43712, 3) == 1
    one = _call(eng, p, X, Xs, V, dt, "strided")[0]
    all_ = _call(eng, p, X, many, V, dt, "strided")[0]
    assert torch.equal(one[:, 0], all_[:, 0])


def test_the_python_wrapper_chunks_wide_v(eng):
    c, p, X, Xs, _ = _problem("base")
    V = cm.columns(257, 2 * CAP + 3, 3, 9)
    exact, bound = cm.reference(p, Xs, X, V, torch.float32)
    f = lambda t: None if t is None else t.to(DEV, torch.float32)
    got = eng.cross_matvec(p.kind, f(Xs), f(X), f(p.ell), f(p.oscale), f(V)).cpu()
    assert got.shape == exact.shape and cm.violations(got, exact, bound) == 0
    alpha = f(V[:, :, 0].contiguous())
    assert torch.equal(eng.cross_matvec(p.kind, f(Xs), f(X), f(p.ell), f(p.oscale), alpha).cpu(), got[:, :, 0])


def test_argument_errors_launch_nothing_and_leave_the_output(eng):
    hip = eng._hip
    c, p, X, Xs, V = _problem("base")
    dt = torch.float32
    q, n, r = V.shape
    ns = Xs.shape[0]
    L = hip.lib()
    f = lambda t: t.to(DEV, dt).contiguous()
    Xc, Xsc, ell, osc, Vc = f(X), f(Xs), f(p.ell), f(p.oscale), f(V)
    out = torch.full((q, ns, r), -7.25, dtype=dt, device=DEV)
    part = torch.empty(int(L.cdll.plmc_cross_matvec_partials_bytes(n, ns, r, q)) // 8, dtype=torch.float64, device=DEV)
    st = hip.stream_ptr(DEV)
    ok = dict(kind=3, X=hip.ptr(Xc), n=n, Xs=hip.ptr(Xsc), ns=ns, d=3, ell=hip.ptr(ell), os=hip.ptr(osc), V=hip.ptr(Vc), ldv=r, strideV=n * r,
              r=r, Out=hip.ptr(out), part=hip.ptr(part), q=q)
    order = ("kind", "X", "n", "Xs", "ns", "d", "ell", "os", "V", "ldv", "strideV", "r", "Out", "part", "q")
    refused = [("null pointer", dict(X=None)), ("null pointer", dict(Xs=None)), ("null pointer", dict(ell=None)), ("null pointer", dict(V=None)),
               ("null pointer", dict(Out=None)), ("n > 0", dict(n=0)), ("ns > 0", dict(ns=0)), ("r > 0", dict(r=0)), ("q <= 65535", dict(q=0)),
               ("plmc_cross_matvec_max_cols", dict(r=CAP + 1, ldv=CAP + 1)), ("ldv >= r", dict(ldv=r - 1)),
               ("strideV", dict(strideV=(n - 1) * r + r - 1)), ("plmc_max_dim", dict(d=33)), ("unknown kernel kind", dict(kind=5)),
               ("partials", dict(part=None))]
    hip.prof_enable(["k_cross_matvec"])
    try:
        hip.prof_collect()
        for word, change in refused:
            args = {**ok, **change}
            with pytest.raises(RuntimeError, match=r"plmc_cross_matvec_f32 failed.*" + word):
                L.call("plmc_cross_matvec", dt, *(args[k] for k in order), st)
        # the families' own limits, through the dispatch every family call takes
        ones = lambda *s: torch.ones(*s, dtype=dt, device=DEV)
        Xd = lambda d, rows=n: torch.rand(rows, d, dtype=dt, device=DEV)
        for kind, d, table, word in (("matern52", 3, ones(q, 5, 3), "plmc_max_components"), ("sm", 9, ones(q, 2, 2, 9), "plmc_sm_max_dim"),
                                     ("sm", 2, ones(q, 2, 9, 2), "plmc_sm_max_mixtures"), ("periodic", 9, ones(q, 2, 9), "plmc_per_max_dim"),
                                     ("locally_periodic", 9, ones(q, 3, 9), "plmc_lper_max_dim"), ("rq", 17, ones(q, 18), "plmc_rq_max_dim"),
                                     ("sum(rbf,periodic)", 9, ones(q, 2, 28), "plmc_sum_max_dim"), ("poly9", 3, ones(q, 4), "plmc_dot_max_power")):
            with pytest.raises(RuntimeError, match=r"plmc_cross_matvec\w* failed.*" + word):
                eng._kernel_call(L, "plmc_cross_matvec", dt, (eng.kind_code(kind), hip.ptr(Xd(d)), n, hip.ptr(Xd(d, ns)), ns, d), table,
                                 (None, hip.ptr(Vc), r, n * r, r, hip.ptr(out), hip.ptr(part), q, st))
        torch.cuda.synchronize()
        assert "k_cross_matvec" not in hip.prof_collect()             # nothing was launched
        assert bool((out == -7.25).all())                             # and the output is as it was
        L.call("plmc_cross_matvec", dt, *(ok[k] for k in order), st)
        torch.cuda.synchronize()
        assert hip.prof_collect()["k_cross_matvec"]["launches"] == 1 and not bool((out == -7.25).any())
    finally:
        hip.prof_enable(False)
