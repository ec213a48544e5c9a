"""plmc_posterior_dx (csrc/posterior_dx.hip) through its Python wrapper `_engine.posterior_dx`, LAPACK-style: the caller owns the buffers.
Random alpha and B stand where the kernel may read and NaN everywhere else -- alpha from n on, the rows of B from n on, its columns from ns
up to the leading dimension; the result is held against the fp64 autograd reference of tests/_posterior_dx_dense.py element by element,
relative to the sum of absolute terms behind each element.  One axis at a time around the base case matern52, d = 5, n = 129, n* = 37,
q = 3: families, training sizes around the staged chunk of 64 rows, test sizes on both sides of the block of 64 test points, dimensions on
both sides of every capacity, no output scale, a test point that is a training point, and a training range split over several
workgroups."""
import functools
import zlib

import pytest
import torch

import _posterior_dx_dense as pdd

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U32 = 2.0 ** -24
TABLE_FAMILIES = ("rq", "periodic", "locally_periodic", "sm3")
# groups that cross the capacities 4 / 8 / 16 / 32 (those of test_gpu_input_grad_kernel.py)
GROUPS_BY_D = {1: [[0], [0]], 4: [[0, 1], [1, 2, 3]], 8: [[0, 1, 2, 3], [4, 5, 6, 7]], 9: [[0, 1, 2, 3, 4], [3, 7, 8]],
               16: [[0, 3, 4, 7], [8, 15], [2, 9], list(range(16))],
               17: [[0, 5, 16], [7, 8, 9, 15, 16], [1, 2, 3, 4]],
               32: [list(range(16)), list(range(16, 32)), [3, 4, 20, 31], [8, 15, 16, 17]]}
BASE = dict(family="matern52", d=5, n=129, ns=37, q=3, use_os=True, coincident=False)
SPLIT = dict(n=1100, ns=3)                                               # the training range over several workgroups
CASES = ([dict()]
         + [dict(family=f) for f in pdd.FAMILIES]
         + [dict(n=n) for n in (1, 2, 63, 64, 65, 127, 128, 257)]
         + [dict(ns=ns) for ns in (1, 2, 63, 64, 65, 130)]
         + [dict(d=d) for d in (1, 4, 8, 9, 16, 17, 32)]
         + [dict(family="add", d=d) for d in GROUPS_BY_D]
         + [dict(family=f, d=d) for f in TABLE_FAMILIES for d in (1, 4, 8)]
         + [dict(family="rq", d=d) for d in (9, 16)]
         + [dict(family=f, use_os=False) for f in ("matern52", "add_disjoint", "periodic", "sm3")]
         + [dict(family=f, coincident=True) for f in pdd.FAMILIES]
         + [SPLIT, dict(family="sm3", **SPLIT)])

# fp32: |got - want| <= TOL32 2^-24 sum |terms| per element.  The stationary kinds and their component table: 4 (d + 4), the bound of the
# kernel-VJP and input-gradient tests, whose arithmetic this is (the weights alpha_i and -2 B_is multiply the unit derivative in fp64).
# The other families have no derived bound for the derivative of the reduced phase / log1p: the constant is the next power of two at or
# above 4 x the worst ratio measured over the cases above against the fp64 reference (profiles/posterior_dx_accuracy.md gives the ratios).
TOL32 = {"rq": 8.0, "periodic": 4.0, "locally_periodic": 8.0, "sm": 8.0}       # measured worst ratios: 1.11, 0.96, 1.11, 1.84


def _group(family):
    return "sm" if family.startswith("sm") else family if family in TOL32 else "stationary"


def _case_id(c):
    return "-".join("%s=%s" % kv for kv in c.items()) or "base"


def _seed(c):
    return zlib.crc32(_case_id(c).encode()) % 100000


@functools.lru_cache(maxsize=None)
def _reference(cid):
    """(problem, X, Xs, alpha, B, Jm, Jv, Tm, Tv) of a case, computed once for both element types and left unchanged."""
    case = next(c for c in CASES if _case_id(c) == cid)
    c = {**BASE, **case}
    seed = _seed(case)
    if c["family"] == "add":
        p = pdd.problem("add_disjoint", c["d"], c["q"], seed, c["use_os"], groups=GROUPS_BY_D[c["d"]])
    else:
        p = pdd.problem(c["family"], c["d"], c["q"], seed, c["use_os"])
    X = pdd.igd.inputs(c["n"], c["d"], seed)
    Xs = pdd.query_points(c["ns"], c["d"], seed, X, c["coincident"])
    alpha, B = pdd.random_operands(c["n"], c["ns"], c["q"], seed)
    return (p, X, Xs, alpha, B) + pdd.posterior_dx_ref(p.K, X, Xs, alpha, B)


def _device_args(p, X, Xs, alpha, B, dt):
    a, b = pdd.nan_buffers(alpha, B, dt)
    f = lambda t: None if t is None else t.to(DEV, dt).contiguous()
    b = b.to(DEV)
    return (p.kind, f(X), f(Xs), f(p.ell), f(p.oscale), a.to(DEV), b[:, :, :B.shape[2]])


def ratio(got, want, terms):
    """Worst |got - want| / (2^-24 sum |terms|) over the elements with a non-zero sum."""
    live = terms > 0
    return float(((got - want).abs()[live] / (U32 * terms[live])).max()) if bool(live.any()) else 0.0


@pytest.fixture(scope="module")
def eng():
    from projectedlmc import _engine
    assert torch.cuda.is_available()
    return _engine


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_posterior_dx_against_autograd(eng, case, dt):
    p, X, Xs, alpha, B, Jm, Jv, Tm, Tv = _reference(_case_id(case))
    args = _device_args(p, X, Xs, alpha, B, dt)
    n = X.shape[0]
    got, again = eng.posterior_dx(*args, n=n), eng.posterior_dx(*args, n=n)
    torch.cuda.synchronize()
    d = Jm.shape[-1]
    grp = _group(p.family)
    tol = 1e-10 if dt == torch.float64 else (4 * (d + 4) if grp == "stationary" else TOL32[grp]) * U32
    for name, g, g2, want, terms in (("Jm", got[0], again[0], Jm, Tm), ("Jv", got[1], again[1], Jv, Tv)):
        g, g2 = g.cpu(), g2.cpu()
        assert g.shape == want.shape and g.dtype == torch.float64
        assert bool(torch.isfinite(g).all()), name                       # nothing of the NaN around the live operands came in
        err = (g - want).abs()
        print("%s %s %s: worst err / (2^-24 sum |terms|) = %.3f" % (_case_id(case), dt, name, ratio(g, want, terms)))
        bad = err > tol * terms
        assert not bool(bad.any()), (name, int(bad.sum()), float(err.max()), ratio(g, want, terms))
        # exact zeros: dimensions no component uses (every slot +inf), mixture dimensions with scale = mean = 0
        assert bool((g[:, :, p.zero] == 0.0).all()), name
        assert torch.equal(g, g2), name                                  # fixed-order sums, no atomics
    if case.get("family") == "add_overlap":
        assert int(p.zero.sum()) == 2
    if str(case.get("family", "")).startswith("sm") and d > 1:
        assert int(p.zero.sum()) == 1
    if case.get("n") == SPLIT["n"]:                                      # the launch really used several workgroups along the training range
        assert eng.posterior_dx_splits(n, Xs.shape[0], alpha.shape[0]) > 1
    if n <= 256:                                                         # (n = 257 is the first size with two ranges, the second ragged)
        assert eng.posterior_dx_splits(n, Xs.shape[0], alpha.shape[0]) == 1


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["float64", "float32"])
def test_without_b_only_the_mean_part_is_written(eng, dt):
    """B = NULL: Jm as with B, bit for bit; a Jv buffer the caller hands in keeps its sentinel."""
    for case in (dict(), SPLIT):
        p, X, Xs, alpha, B, Jm, Jv, Tm, Tv = _reference(_case_id(case))
        args = _device_args(p, X, Xs, alpha, B, dt)
        with_b = eng.posterior_dx(*args, n=X.shape[0])[0]
        sentinel = torch.full(Jv.shape, -7.25, dtype=torch.float64, device=DEV)
        Jm_only, Jv_back = eng.posterior_dx(*args[:-1], None, n=X.shape[0], Jv=sentinel)
        torch.cuda.synchronize()
        assert torch.equal(Jm_only, with_b)
        assert Jv_back is sentinel and bool((sentinel == -7.25).all())
        assert eng.posterior_dx(*args[:-1], None, n=X.shape[0])[1] is None


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["float64", "float32"])
def test_a_test_point_on_a_training_point_gets_nothing_from_that_pair(eng, dt):
    """Matern-1/2 has no derivative at r = 0: the convention of plmc_kernel_vjp (nothing) holds, so with one training point and every test
    point on it every output is exactly 0 whatever alpha and B are -- for every family."""
    for family in pdd.FAMILIES:
        p = pdd.problem(family, 5, 2, seed=5)
        X = pdd.igd.inputs(1, 5, seed=5)
        Xs = X.expand(3, 5).clone()
        alpha, B = pdd.random_operands(1, 3, 2, seed=5)
        Jm, Jv = eng.posterior_dx(*_device_args(p, X, Xs, alpha, B, dt), n=1)
        assert bool((Jm == 0.0).all()) and bool((Jv == 0.0).all()), family


def test_limits_and_refused_families_launch_nothing(eng):
    from projectedlmc import _hip
    n, ns, q = 20, 4, 2
    alpha, B = (t.to(DEV) for t in pdd.nan_buffers(*pdd.random_operands(n, ns, q, seed=1), torch.float64))
    X = lambda d, rows=n: torch.rand(rows, d, dtype=torch.float64, device=DEV)
    ones = lambda *s: torch.ones(*s, dtype=torch.float64, device=DEV)
    refused = [
        ("spline", 3, ones(q, 3), "spline"),
        ("sum(rbf,periodic)", 2, ones(q, 2, 7), "sum"),
        ("linear", 3, ones(q, 4), "dot-product"),
        ("poly3", 3, ones(q, 4), "dot-product"),
        ("matern52", 33, ones(q, 33), "plmc_max_dim"),
        ("matern52", 3, ones(q, 5, 3), "plmc_max_components"),
        ("sm", 9, ones(q, 2, 2, 9), "plmc_sm_max_dim"),
        ("sm", 2, ones(q, 2, 9, 2), "plmc_sm_max_mixtures"),
        ("periodic", 9, ones(q, 2, 9), "plmc_per_max_dim"),
        ("locally_periodic", 9, ones(q, 3, 9), "plmc_lper_max_dim"),
        ("rq", 17, ones(q, 18), "plmc_rq_max_dim"),
    ]
    _hip.prof_enable(["k_posterior_dx"])
    try:
        _hip.prof_collect()
        for kind, d, ell, word in refused:
            with pytest.raises(RuntimeError, match=r"plmc_posterior_dx\w* failed.*" + word):
                eng.posterior_dx(kind, X(d), X(d, ns), ell, None, alpha, B[:, :, :ns], n=n)
        with pytest.raises(RuntimeError, match="n_pad >= n"):              # more training points than alpha holds
            eng.posterior_dx("matern52", X(3, 40), X(3, ns), ones(q, 3), None, alpha, B[:, :, :ns])
        with pytest.raises(RuntimeError, match="ldb >= ns"):
            eng.posterior_dx("matern52", X(3), X(3, 12), ones(q, 3), None, alpha, B[:, :, :ns], n=n)
        torch.cuda.synchronize()
        assert "k_posterior_dx" not in _hip.prof_collect()                           # nothing was launched
        eng.posterior_dx("matern52", X(3), X(3, ns), ones(q, 3), None, alpha, B[:, :, :ns], n=n)
        rec = _hip.prof_collect()["k_posterior_dx"]
        assert rec["launches"] == 1 and rec["bytes"] == q * n * ns * 8
    finally:
        _hip.prof_enable(False)
