"""The component-table kernel VJP (csrc/kernel_vjp.hip: k_kernel_vjp_add, `plmc_kernel_vjp_add_*`) through its Python wrapper
`_var_engine.kernel_vjp` with ell (q, G, d): the pull-back of the adjoints of K_ZZ / K_ZX of an additive (`decomp`) kernel to the inducing
locations and to the component table.  Against fp64 autograd per component (tests/_inducing_dense.py on oracle/gp_math.py), one axis at a
time around the base case of the plain kernel's test (tests/test_gpu_kernel_kinds.py): kinds, component counts, disjoint and overlapping
groups, input dimensions on both sides of every DCAP instantiation (and of the pass split above d = 16), row and column counts."""
import math
import zlib

import pytest
import torch

import _inducing_dense as idn

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KINDS = {"rbf": ("rbf", 2.5), "matern12": ("matern", 0.5), "matern32": ("matern", 1.5), "matern52": ("matern", 2.5)}
U32 = 2.0 ** -24

DISJOINT, OVERLAP = [[0, 1], [2, 3, 4]], [[0, 1], [1, 2]]            # OVERLAP leaves dimensions 3 and 4 unused
# groups that cross the DCAP boundaries 4 / 8 / 16 (d = 16, 17 and 32 with more components than one pass over G takes above d = 16)
_GROUPS_BY_D = {1: [[0], [0]], 4: [[0, 1], [1, 2, 3]], 8: [[0, 1, 2, 3], [4, 5, 6, 7]], 9: [[0, 1, 2, 3, 4], [3, 7, 8]],
                16: [[0, 3, 4, 7], [8, 15], [2, 9], list(range(16))],
                17: [[0, 5, 16], [7, 8, 9, 15, 16], [1, 2, 3, 4]],
                32: [list(range(16)), list(range(16, 32)), [3, 4, 20, 31], [8, 15, 16, 17]]}
_BASE = dict(kind="matern52", d=5, n1=5, n2=65, q=3, groups=DISJOINT, use_os=True, same=False)
_CASES = ([dict(kind=k) for k in ("rbf", "matern12", "matern32")] + [{}]
          + [dict(groups=[[0, 1, 2, 3, 4]]), dict(groups=[[0, 1], [2], [3, 4], [1, 3]]), dict(groups=OVERLAP)]
          + [dict(d=d, groups=g) for d, g in _GROUPS_BY_D.items()]
          + [dict(n1=n1) for n1 in (1, 257)]
          + [dict(n2=n2) for n2 in (1, 63, 64, 300)]
          + [dict(use_os=False), dict(same=True), dict(same=True, kind="matern12", groups=OVERLAP)])


def _case_id(c):
    return "-".join("%s=%s" % (k, "|".join("".join(map(str, g)) if len(g) < 6 else "%d.." % g[0] for g in v) if k == "groups" else v)
                    for k, v in c.items()) or "base"


_PARAMS = [pytest.param(c, dt, id="%s-%s" % (_case_id(c), str(dt)[6:])) for c in _CASES for dt in (torch.float64, torch.float32)]


@pytest.fixture(scope="module")
def var():
    from projectedlmc import _var_engine
    assert torch.cuda.is_available()
    return _var_engine


def _problem(d, n1, n2, q, groups, use_os, seed):
    g = torch.Generator().manual_seed(seed)
    X1 = 2 * torch.rand(n1, d, generator=g, dtype=torch.float64) - 1
    X2 = 2 * torch.rand(n2, d, generator=g, dtype=torch.float64) - 1
    # lengthscales ~ sqrt(|group|): the scaled distances of every component stay O(1)
    ells = [math.sqrt(len(idx)) * (0.3 + 0.5 * torch.rand(q, len(idx), generator=g, dtype=torch.float64)) for idx in groups]
    oss = [(0.5 + torch.rand(q, generator=g, dtype=torch.float64)) if use_os else None for _ in groups]
    return X1, X2, ells, oss


def _rounded(dt, t):
    return None if t is None else t.to(dt).double()


def _run(var, kind, dt, groups, X1, X2, ells, oss, G, same=False):
    """The kernel's outputs (on the CPU) for the dt-rounded problem, and the oracle's values and absolute-term sums at the same inputs."""
    d = X1.shape[1]
    X1, X2, G = _rounded(dt, X1), _rounded(dt, X2), _rounded(dt, G)
    ells, oss = [_rounded(dt, e) for e in ells], [_rounded(dt, o) for o in oss]
    ell, osc = idn.component_table(groups, ells, oss, d)
    f = lambda t: None if t is None else t.to(DEV, dt).contiguous()
    X1d = f(X1)
    got = var.kernel_vjp(kind, X1d, X1d if same else f(X2), f(ell), f(osc), f(G))
    torch.cuda.synchronize()
    okind, nu = KINDS[kind]
    want, terms = idn.table_vjp(okind, nu, groups, X1, X1 if same else X2, ells, oss, G)
    return [t.cpu() for t in got], want, terms, ell


def _check_bound(d, dt, got, want, terms, what=""):
    """The plain kernel's a-priori bound (test_kernel_vjp_against_autograd), per output: 4 (d + 4) u sum |terms| in fp32, 1e-10 of the same
    sum in fp64; the sum runs over b and over the components, and the bound holds term by term."""
    tol = 1e-10 if dt == torch.float64 else 4 * (d + 4) * U32
    for name, g, w, t in zip(("gX1", "gEll", "gOs"), got, want, terms):
        assert g.shape == w.shape, (name, g.shape, w.shape)
        err = (g - w).abs()
        bad = err > tol * t
        assert not bool(bad.any()), (what, name, int(bad.sum()), float(err.max()), float((err / t.clamp_min(1e-300)).max()))


@pytest.mark.parametrize("case,dt", _PARAMS)
def test_table_vjp_against_autograd(var, case, dt):
    c = {**_BASE, **case}
    X1, X2, ells, oss = _problem(c["d"], c["n1"], c["n2"], c["q"], c["groups"], c["use_os"], seed=zlib.crc32(_case_id(case).encode()))
    n2 = c["n1"] if c["same"] else c["n2"]
    G = torch.randn(c["q"], c["n1"], n2, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    got, want, terms, ell = _run(var, c["kind"], dt, c["groups"], X1, X2, ells, oss, G, same=c["same"])
    _check_bound(c["d"], dt, got, want, terms)
    # exact zeros: the slots a component ignores, and the dimensions no group uses
    inactive = torch.isinf(ell)
    assert bool((got[1][inactive] == 0.0).all())
    unused = inactive.all(dim=(0, 1))
    assert bool((got[0][:, unused] == 0.0).all())
    if c["groups"] is OVERLAP:
        assert int(unused.sum()) == 2


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["float64", "float32"])
def test_matern12_component_at_its_own_zero_distance_contributes_nothing(var, dt):
    """decomp [[0], [1]]: every row of X2 equals row 1 of X1 in column 0 only.  Component 0 is at r = 0 for that row although the points
    differ (in column 1, outside its group): the Matern-1/2 convention (oracle/gp_math.kernel_vjp) gives it no share of gX1 / gEll there,
    its value still goes to gOs.  With that row alone (n1 = 1) the row sums the wrapper forms over a are that row's: exact zeros."""
    g = torch.Generator().manual_seed(5)
    q, groups = 2, [[0], [1]]
    X1 = 2 * torch.rand(4, 2, generator=g, dtype=torch.float64) - 1
    X2 = 2 * torch.rand(70, 2, generator=g, dtype=torch.float64) - 1
    X2[:, 0] = X1[1, 0]
    ells = [0.5 + torch.rand(q, 1, generator=g, dtype=torch.float64) for _ in groups]
    oss = [0.5 + torch.rand(q, generator=g, dtype=torch.float64) for _ in groups]
    G = torch.randn(q, 4, 70, generator=g, dtype=torch.float64)
    got, want, terms, _ = _run(var, "matern12", dt, groups, X1, X2, ells, oss, G)
    assert float(want[0][1, 0]) == 0.0 and float(got[0][1, 0]) == 0.0, got[0]
    _check_bound(2, dt, got, want, terms, "four rows")
    got, want, terms, _ = _run(var, "matern12", dt, groups, X1[1:2], X2, ells, oss, G[:, 1:2])
    assert float(got[0][0, 0]) == 0.0 and bool((got[1][:, 0, 0] == 0.0).all()), (got[0], got[1])
    assert bool((got[2][:, 0] != 0.0).all()) and bool((got[1][:, 1, 1] != 0.0).all()) and float(got[0][0, 1]) != 0.0
    _check_bound(2, dt, got, want, terms, "one row")


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["float64", "float32"])
def test_one_component_is_the_plain_kernel(var, dt):
    """A table of one component launches the plain kernel's instantiation: bit-identical outputs."""
    g = torch.Generator().manual_seed(11)
    q, d, n1, n2 = 3, 5, 37, 130
    f = lambda t: t.to(DEV, dt).contiguous()
    X1, X2 = f(torch.rand(n1, d, generator=g, dtype=torch.float64)), f(torch.rand(n2, d, generator=g, dtype=torch.float64))
    ell, osc = f(0.5 + torch.rand(q, d, generator=g, dtype=torch.float64)), f(0.5 + torch.rand(q, generator=g, dtype=torch.float64))
    G = f(torch.randn(q, n1, n2, generator=g, dtype=torch.float64))
    for kind in ("matern52", "matern12"):
        for o2, o3 in ((osc, osc.reshape(q, 1)), (None, None)):
            a = var.kernel_vjp(kind, X1, X2, ell, o2, G)
            b = var.kernel_vjp(kind, X1, X2, ell.reshape(q, 1, d), o3, G)
            assert b[1].shape == (q, 1, d) and b[2].shape == (q, 1)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1].reshape(q, d)) and torch.equal(a[2], b[2].reshape(q))


def test_limits_are_argument_errors(var):
    """Five components, the spline kind in a table and d = 33 raise the library's argument error (nothing is launched)."""
    g = torch.Generator().manual_seed(2)
    f = lambda t: t.to(DEV).contiguous()
    for d, ncomp, kind, msg in ((3, 5, "matern52", r"components <= plmc_max_components\(\)"), (3, 2, "spline", "stationary kinds only"),
                                (33, 2, "matern52", "bad sizes")):
        X1, X2 = torch.rand(5, d, generator=g, dtype=torch.float64), torch.rand(7, d, generator=g, dtype=torch.float64)
        ell = 0.5 + torch.rand(2, ncomp, d, generator=g, dtype=torch.float64)
        osc = 0.5 + torch.rand(2, ncomp, generator=g, dtype=torch.float64)
        with pytest.raises(RuntimeError, match=msg):
            var.kernel_vjp(kind, f(X1), f(X2), f(ell), f(osc), f(torch.randn(2, 5, 7, generator=g, dtype=torch.float64)))
    torch.cuda.synchronize()
