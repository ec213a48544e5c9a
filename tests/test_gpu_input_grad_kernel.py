"""plmc_input_grad (csrc/input_grad.hip) through its Python wrapper `_engine.input_grad`, LAPACK-style: the caller owns the buffers.  A
random symmetric P stands in the elements the kernel may read -- the upper triangle of the live block of a (q, n_pad, n_pad + 128)
buffer -- and NaN everywhere else, as in alpha from n on; the result is held against the fp64 autograd reference of
tests/_input_grad_dense.py element by element, relative to the sum of absolute terms behind each element.  One axis at a time around the
base case matern52, d = 5, n = 129, q = 3: families, sizes on both sides of the tile (one tile, the tile edge, two and three block rows,
so that both read directions and the diagonal tile meet), dimensions on both sides of every capacity, no output scale, coincident rows."""
import functools
import zlib

import pytest
import torch

import _input_grad_dense as igd

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U32 = 2.0 ** -24
TABLE_FAMILIES = ("rq", "periodic", "locally_periodic", "sm3")
# groups that cross the capacities 4 / 8 / 16 / 32 (those of test_gpu_kernel_vjp_add.py)
GROUPS_BY_D = {1: [[0], [0]], 4: [[0, 1], [1, 2, 3]], 8: [[0, 1, 2, 3], [4, 5, 6, 7]], 9: [[0, 1, 2, 3, 4], [3, 7, 8]],
               16: [[0, 3, 4, 7], [8, 15], [2, 9], list(range(16))],
               17: [[0, 5, 16], [7, 8, 9, 15, 16], [1, 2, 3, 4]],
               32: [list(range(16)), list(range(16, 32)), [3, 4, 20, 31], [8, 15, 16, 17]]}
BASE = dict(family="matern52", d=5, n=129, q=3, use_os=True, coincident=False)
CASES = ([dict(family=f) for f in igd.FAMILIES]
         + [dict(n=n) for n in (1, 2, 127, 128, 257)]
         + [dict(d=d) for d in (1, 4, 8, 9, 16, 17, 32)]
         + [dict(family="add", d=d) for d in GROUPS_BY_D]
         + [dict(family=f, d=d) for f in TABLE_FAMILIES for d in (1, 4, 8)]
         + [dict(family="rq", d=d) for d in (9, 16)]
         + [dict(family=f, use_os=False) for f in ("matern52", "add_disjoint", "periodic", "sm3")]
         + [dict(family=f, coincident=True) for f in igd.FAMILIES])

# fp32: |got - want| <= TOL32 2^-24 sum |terms| per element.  The stationary kinds and their component table: 4 (d + 4), the bound of the
# kernel-VJP tests, whose arithmetic this is.  The other families have no derived bound for the derivative of the reduced phase / log1p:
# the constant is the next power of two at or above 4 x the worst ratio measured over the cases above against the fp64 reference
# (profiles/input_grad_accuracy.md gives the ratios).
TOL32 = {"rq": 8.0, "periodic": 8.0, "locally_periodic": 8.0, "sm": 8.0}       # measured worst ratios: 1.32, 1.29, 1.20, 1.97


def _group(family):
    return "sm" if family.startswith("sm") else family if family in TOL32 else "stationary"


def _case_id(c):
    return "-".join("%s=%s" % kv for kv in c.items()) or "base"


def _seed(c):
    return zlib.crc32(_case_id(c).encode()) % 100000


@functools.lru_cache(maxsize=None)
def _reference(cid):
    """(problem, X, P, alpha, want, terms) of a case, computed once for both element types and left unchanged."""
    case = next(c for c in CASES if _case_id(c) == cid)
    c = {**BASE, **case}
    seed = _seed(case)
    if c["family"] == "add":
        p = igd.problem("add_disjoint", c["d"], c["q"], seed, c["use_os"], groups=GROUPS_BY_D[c["d"]])
    else:
        p = igd.problem(c["family"], c["d"], c["q"], seed, c["use_os"])
    X = igd.inputs(c["n"], c["d"], seed, c["coincident"])
    P, alpha = igd.random_operands(c["n"], c["q"], seed)
    want, terms = igd.input_grad_ref(p.K, X, P, alpha)
    return p, X, P, alpha, want, terms


def run_case(eng, case, dt):
    """The kernel's output on the CPU, twice, and the reference of the case."""
    p, X, P, alpha, want, terms = _reference(_case_id(case))
    Kinv, a = igd.nan_buffers(P, alpha, dt)
    f = lambda t: None if t is None else t.to(DEV, dt).contiguous()
    args = (p.kind, f(X), f(p.ell), f(p.oscale), Kinv.to(DEV), a.to(DEV))
    got, again = eng.input_grad(*args), eng.input_grad(*args)
    torch.cuda.synchronize()
    return got.cpu(), again.cpu(), p, want, terms


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
def test_input_grad_against_autograd(eng, case, dt):
    got, again, p, want, terms = run_case(eng, case, dt)
    d = want.shape[-1]
    assert got.shape == want.shape and got.dtype == torch.float64
    assert bool(torch.isfinite(got).all())                               # nothing of the NaN around the live triangle came in
    grp = _group(p.family)
    tol = 1e-10 if dt == torch.float64 else (4 * (d + 4) if grp == "stationary" else TOL32[grp]) * U32
    err = (got - want).abs()
    print("%s %s: worst err / (2^-24 sum |terms|) = %.3f" % (_case_id(case), dt, ratio(got, want, terms)))
    bad = err > tol * terms
    assert not bool(bad.any()), (int(bad.sum()), float(err.max()), ratio(got, want, terms))
    # exact zeros: dimensions no component uses (every slot +inf), mixture dimensions with scale = mean = 0
    assert bool((got[:, :, p.zero] == 0.0).all())
    if case.get("family") == "add_overlap":
        assert int(p.zero.sum()) == 2
    if str(case.get("family", "")).startswith("sm") and d > 1:
        assert int(p.zero.sum()) == 1
    assert torch.equal(got, again)                                       # fixed-order sums, no atomics


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["float64", "float32"])
def test_coincident_rows_contribute_nothing_to_each_other(eng, dt):
    """Matern-1/2 has no derivative at r = 0: the convention of oracle/gp_math.kernel_vjp (nothing) holds, so with n = 2 coincident
    rows every output is exactly 0 whatever P and alpha are -- for every family."""
    for family in igd.FAMILIES:
        p = igd.problem(family, 5, 2, seed=5)
        X = igd.inputs(2, 5, seed=5)
        X[1] = X[0]
        P, alpha = igd.random_operands(2, 2, seed=5)
        Kinv, a = igd.nan_buffers(P, alpha, dt)
        f = lambda t: None if t is None else t.to(DEV, dt).contiguous()
        got = eng.input_grad(p.kind, f(X), f(p.ell), f(p.oscale), Kinv.to(DEV), a.to(DEV)).cpu()
        assert bool((got == 0.0).all()), family


def test_limits_and_refused_families_launch_nothing(eng):
    from projectedlmc import _hip
    n, q = 20, 2
    P, alpha = igd.random_operands(n, q, seed=1)
    Kinv, a = (t.to(DEV) for t in igd.nan_buffers(P, alpha, torch.float64))
    X = lambda d: torch.rand(n, d, dtype=torch.float64, device=DEV)
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
    _hip.prof_enable(["k_input_grad"])
    try:
        _hip.prof_collect()
        for kind, d, ell, word in refused:
            with pytest.raises(RuntimeError, match=r"plmc_input_grad\w* failed.*" + word):
                eng.input_grad(kind, X(d), ell, None, Kinv, a)
        with pytest.raises(RuntimeError, match="n_pad must be plmc_pad"):          # a buffer of another size's padding
            eng.input_grad("matern52", torch.rand(200, 3, dtype=torch.float64, device=DEV), ones(q, 3), None, Kinv, a)
        with pytest.raises(RuntimeError, match="ldk >= n_pad"):
            eng.input_grad("matern52", X(3), ones(q, 3), None, Kinv[:, :, :100].contiguous(), a)
        torch.cuda.synchronize()
        assert "k_input_grad" not in _hip.prof_collect()                             # nothing was launched
        eng.input_grad("matern52", X(3), ones(q, 3), None, Kinv, a)
        rec = _hip.prof_collect()["k_input_grad"]
        assert rec["launches"] == 1 and rec["bytes"] == q * n * n * 8
    finally:
        _hip.prof_enable(False)
