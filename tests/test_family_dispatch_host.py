"""The transcript of the Python engine's family dispatch, on CPU tensors (no GPU).

_engine._kernel_call is driven with a stand-in for the library whose call(name, dt, *args) records its arguments: for every
(operation, covariance family) pair the entry-point name, the argument count and kinds against _hip._TYPED, the head and tail
passed through, the family's integers and -- read back through ctypes from the addresses passed -- the values behind every table
pointer.  _check_kernel_shape (accepted and refused tables, message texts) and the predicates that size things are pinned over the
same tables; those read the limits of the built library.

Not covered here: the side-stream branch (`stream=`: record_stream on each piece of a split table) cannot run on CPU tensors.  The GPU
training-step tests of each family (tests/test_gpu_*_kernel.py, test_gpu_additive_engine.py) run it.
"""
import ctypes
import gc

import pytest
import torch

from projectedlmc import _engine, _hip

Q, D = 2, 3
# operation -> (name pattern with the family's infix slot, arguments in front of the table: the kind and the rest of the head)
OPS = {
    "plmc_assemble": ("plmc_assemble%s", 4),
    "plmc_assemble_cross": ("plmc_assemble_cross%s", 6),
    "plmc_factorize_ex": ("plmc_factorize%s_ex", 4),
    "plmc_kinv_grad_vd": ("plmc_kinv_grad%s_vd", 9),
    "plmc_loo_grad": ("plmc_loo_grad%s", 10),
    "plmc_weighted_grad": ("plmc_weighted_grad%s", 10),
    "plmc_input_grad": ("plmc_input_grad%s", 9),
    "plmc_posterior_dx": ("plmc_posterior_dx%s", 6),
    "plmc_cross_matvec": ("plmc_cross_matvec%s", 6),
    "plmc_cross_matvec_dx": ("plmc_cross_matvec_dx%s", 6),
    "plmc_kernel_vjp": ("plmc_kernel_vjp%s", 6),
}
INTS = (ctypes.c_int, ctypes.c_int64)
SUM_KIND = "sum(rbf,periodic)"


class Recorder:
    """Stands in for _hip.lib(): keeps what _kernel_call hands to the typed entry point."""

    def __init__(self):
        self.calls = []

    def call(self, name, dt, *args):
        self.calls.append((name, dt, args))


def table(shape, dtype):
    n = 1
    for s in shape:
        n *= s
    return (torch.arange(n, dtype=torch.float64).reshape(shape) * 0.25 + 1.0).to(dtype)


class Case:
    """One family: its kind, its table's shape, its infix, whether the kind leads, and what stands in the table's place --
    ("int", value), ("tab", slice of the table) or ("fam", member codes)."""

    def __init__(self, label, kind, shape, infix, lead_kind, flat):
        self.label, self.kind, self.shape, self.infix, self.lead_kind, self.flat = label, kind, shape, infix, lead_kind, flat


def _rows(*idx):
    return lambda t, d: [("tab", t[:, i]) for i in idx]


def _split_last(*more):
    return lambda t, d: [("tab", t[:, :d]), ("tab", t[:, d])] + list(more)


def cases(d=D):
    return [
        Case("plain", "matern52", (Q, d), "", True, lambda t, d: [("tab", t)]),
        Case("add", "matern52", (Q, 2, d), "_add", True, lambda t, d: [("int", 2), ("tab", t)]),
        Case("sm", "sm", (Q, 2, 4, d), "_sm", False, lambda t, d: [("int", 4), ("tab", t[:, 0]), ("tab", t[:, 1])]),
        Case("periodic", "periodic", (Q, 2, d), "_per", False, _rows(0, 1)),
        Case("rq", "rq", (Q, d + 1), "_rq", False, _split_last()),
        Case("locally_periodic", "locally_periodic", (Q, 3, d), "_lper", False, _rows(0, 1, 2)),
        Case("sum", SUM_KIND, (Q, 2, 3 * d + 1), "_sum", False,
             lambda t, d: [("int", 2), ("fam", [_hip.FAM["rbf"], _hip.FAM["periodic"]]), ("tab", t)]),
        Case("linear", "linear", (Q, d + 1), "_dot", False, _split_last(("int", 1))),
        Case("poly3", "poly3", (Q, d + 1), "_dot", False, _split_last(("int", 3))),
    ]


CASES = cases()


def sentinels(types, start):
    """Distinct stand-ins of the kinds the argument types ask for: ints, and pointers that are told apart by identity."""
    return tuple(start + i if t in INTS else ctypes.c_void_p(start + i) for i, t in enumerate(types))


def read_back(arg, count, dtype):
    ctype = ctypes.c_float if dtype == torch.float32 else ctypes.c_double
    return list((ctype * count).from_address(arg.value))


def drive(base, case, dtype, ell=None, kind0=None, d=D):
    """One recorded call of `base` for the family of `case`; checks it against the rule and returns (ell, flat arguments)."""
    pattern, nhead = OPS[base]
    plain = _hip._TYPED[base]
    head_types, tail_types = plain[:nhead], plain[nhead + 1:]
    assert plain[nhead] is ctypes.c_void_p and head_types[0] is ctypes.c_int
    ell = table(case.shape, dtype) if ell is None else ell
    kind0 = _engine.kind_code(case.kind) if kind0 is None else kind0
    head = (kind0,) + sentinels(head_types[1:], 1001)
    tail = sentinels(tail_types, 2001)
    rec = Recorder()
    _engine._kernel_call(rec, base, dtype, head, ell, tail)
    (name, dt, args), = rec.calls
    assert name == pattern % case.infix and dt == dtype
    types = _hip._TYPED[name]
    assert len(args) == len(types)
    lead = head if case.lead_kind else head[1:]
    flat = args[len(lead):len(args) - len(tail)]
    expect = case.flat(ell, d)
    for i, (a, t) in enumerate(zip(args, types)):
        is_fam = len(lead) <= i < len(lead) + len(expect) and expect[i - len(lead)][0] == "fam"
        if t in INTS:
            assert type(a) is int, (name, i, a)
        elif is_fam:                       # the host array of member codes travels as its address
            assert isinstance(a, (int, ctypes.c_void_p)), (name, i, a)
        else:
            assert a is None or isinstance(a, ctypes.c_void_p), (name, i, a)
    assert len(args) == len(lead) + len(expect) + len(tail)
    assert all(a is h for a, h in zip(args, lead)), "head not passed through"
    assert all(a is s for a, s in zip(args[len(args) - len(tail):], tail)), "tail not passed through"
    if case.lead_kind:
        assert args[0] == _hip.KIND[case.kind]
    for a, (what, want) in zip(flat, expect):
        if what == "int":
            assert a == want
        elif what == "fam":
            addr = a if isinstance(a, int) else a.value
            assert list((ctypes.c_int * len(want)).from_address(addr)) == want
        else:
            want = want.contiguous().flatten().tolist()
            assert read_back(a, len(want), dtype) == want
    return ell, flat


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", CASES, ids=[c.label for c in CASES])
@pytest.mark.parametrize("base", [b for b in OPS if b != "plmc_kernel_vjp"])
def test_every_operation_reaches_every_family_form(base, case, dtype):
    drive(base, case, dtype)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", CASES[:2], ids=[c.label for c in CASES[:2]])
def test_kernel_vjp_has_the_plain_and_the_additive_form(case, dtype):
    drive("plmc_kernel_vjp", case, dtype)
    assert sorted(n for n in _hip._TYPED if n.startswith("plmc_kernel_vjp")) == ["plmc_kernel_vjp", "plmc_kernel_vjp_add"]


@pytest.mark.parametrize("label", ["rq", "linear", "poly3"])
def test_one_input_dimension_splits_a_table_of_width_two(label):
    case = next(c for c in cases(1) if c.label == label)
    assert case.shape == (Q, 2)
    drive("plmc_assemble", case, torch.float64, d=1)
    drive("plmc_kinv_grad_vd", case, torch.float32, d=1)


def test_additive_table_of_one_component_keeps_the_additive_entry():
    case = Case("add1", "matern52", (Q, 1, D), "_add", True, lambda t, d: [("int", 1), ("tab", t)])
    drive("plmc_assemble", case, torch.float64)
    drive("plmc_kernel_vjp", case, torch.float32)


@pytest.mark.parametrize("base", ["plmc_assemble_cross", "plmc_kernel_vjp"])
def test_integer_kind_reads_the_family_off_the_rank_of_the_table(base):
    """The variational engine's calls: head[0] is a kind code whatever the table is."""
    code = _hip.KIND["matern32"]
    add = Case("add", "matern32", (Q, 3, D), "_add", True, lambda t, d: [("int", 3), ("tab", t)])
    drive(base, add, torch.float64, kind0=code)
    if base != "plmc_kernel_vjp":
        sm = Case("sm", "sm", (Q, 2, 5, D), "_sm", False, lambda t, d: [("int", 5), ("tab", t[:, 0]), ("tab", t[:, 1])])
        drive(base, sm, torch.float64, kind0=code)


@pytest.mark.parametrize("case", CASES, ids=[c.label for c in CASES])
def test_table_is_split_once(case):
    ell, first = drive("plmc_assemble", case, torch.float64)
    _, second = drive("plmc_kinv_grad_vd", case, torch.float64, ell=ell)
    value = lambda a: a.value if isinstance(a, ctypes.c_void_p) else a
    assert [value(a) for a in first] == [value(a) for a in second]


def test_sum_table_under_another_kind_gets_its_own_member_codes():
    case = CASES[6]
    ell, _ = drive("plmc_assemble", case, torch.float64)
    other = Case("sum", "sum(rq,matern32)", case.shape, "_sum", False,
                 lambda t, d: [("int", 2), ("fam", [_hip.FAM["rq"], _hip.FAM["matern32"]]), ("tab", t)])
    drive("plmc_assemble", other, torch.float64, ell=ell)
    drive("plmc_assemble", case, torch.float64, ell=ell)


def test_member_codes_outlive_a_collection():
    case = CASES[6]
    ell, flat = drive("plmc_assemble", case, torch.float64)
    gc.collect()
    addr = flat[1] if isinstance(flat[1], int) else flat[1].value
    assert list((ctypes.c_int * 2).from_address(addr)) == [_hip.FAM["rbf"], _hip.FAM["periodic"]]
    _, again = drive("plmc_loo_grad", case, torch.float64, ell=ell)
    assert (again[1] if isinstance(again[1], int) else again[1].value) == addr


# ---- the predicates that route and size, over the same tables

PREDICATES = {  # label: (kind_code, _per_kind, n_components, grad_table_width, is_sm, is_sum, is_dot)
    "plain": (3, False, 1, D + 2, False, False, False),
    "add": (3, False, 2, 2 * D + 1 + 2, False, False, False),
    "sm": (None, False, 4, 2 * 4 * D + 1 + 4, True, False, False),
    "periodic": ("periodic", "periodic", 1, 2 * D + 2, False, False, False),
    "rq": ("rq", False, 1, D + 1 + 2, False, False, False),
    "locally_periodic": ("locally_periodic", "locally_periodic", 1, 3 * D + 2, False, False, False),
    "sum": (SUM_KIND, "sum", 2, 2 * (3 * D + 1) + 1 + 2, False, True, False),
    "linear": ("linear", False, 1, D + 1 + 2, False, False, True),
    "poly3": ("poly3", False, 1, D + 1 + 2, False, False, True),
}


@pytest.mark.parametrize("case", CASES, ids=[c.label for c in CASES])
def test_predicates(case):
    ell = table(case.shape, torch.float64)
    got = (_engine.kind_code(case.kind), _engine._per_kind(case.kind), _engine.n_components(ell, case.kind),
           _engine.grad_table_width(ell, case.kind), _engine.is_sm(ell), _engine.is_sum(case.kind), _engine.is_dot(case.kind))
    assert got == PREDICATES[case.label]
    assert [type(g) for g in got] == [type(w) for w in PREDICATES[case.label]]


def test_predicates_without_a_kind_read_the_rank():
    assert _engine.n_components(table((Q, 5, D), torch.float64)) == 5 and _engine.n_components(table((Q, D), torch.float64)) == 1
    assert _engine.n_components(table((Q, 2, 6, D), torch.float64)) == 6
    assert _engine.grad_table_width(table((Q, 5, D), torch.float64)) == 5 * D + 1 + 5
    assert (_engine.PER, _engine.LPER, _engine.RQ, _engine.SUM) == ("periodic", "locally_periodic", "rq", "sum")
    assert _engine.sum_kind(["rbf", "periodic"]) == SUM_KIND and _engine.sum_members(SUM_KIND) == ["rbf", "periodic"]
    assert [_engine.kind_code(k) for k in ("rbf", "matern12", "matern32", "matern52", "spline")] == [0, 1, 2, 3, 4]


# ---- _check_kernel_shape: one accepted and each refused table per family, with the refusal's text

@pytest.fixture(scope="module")
def lib():
    return _hip.lib()


def ones(*shape):
    return torch.ones(*shape, dtype=torch.float64)


@pytest.mark.parametrize("case", CASES, ids=[c.label for c in CASES])
def test_shape_check_accepts_the_tables_of_the_transcript(lib, case):
    assert _engine._check_kernel_shape(lib, ones(*case.shape), case.kind) is None


def refused(lib, ell, kind, text):
    with pytest.raises(ValueError) as e:
        _engine._check_kernel_shape(lib, ell, kind)
    assert str(e.value) == text


def dim_text(lib, d, own):
    """What a table of d dimensions is refused with: the engine-wide limit is looked at first by the families that share it."""
    top = lib.cdll.plmc_max_dim()
    return "input dimension %d exceeds plmc_max_dim()=%d" % (d, top) if d > top else own


def test_shape_check_plain_and_additive(lib):
    top, comps = lib.cdll.plmc_max_dim(), lib.cdll.plmc_max_components()
    refused(lib, ones(Q, top + 1), "rbf", "input dimension %d exceeds plmc_max_dim()=%d" % (top + 1, top))
    refused(lib, ones(Q, top + 1), None, "input dimension %d exceeds plmc_max_dim()=%d" % (top + 1, top))
    refused(lib, ones(Q, 2, top + 1), "rbf", "input dimension %d exceeds plmc_max_dim()=%d" % (top + 1, top))
    refused(lib, ones(Q, comps + 1, D), "rbf", "%d additive components exceed plmc_max_components()=%d" % (comps + 1, comps))
    assert _engine._check_kernel_shape(lib, ones(Q, comps, top), "matern12") is None
    assert _engine._check_kernel_shape(lib, ones(Q, top)) is None


def test_shape_check_spectral_mixture(lib):
    md, mm = lib.cdll.plmc_sm_max_dim(), lib.cdll.plmc_sm_max_mixtures()
    text = "spectral mixture with %d components on %d dimensions exceeds plmc_sm_max_mixtures()=%d / plmc_sm_max_dim()=%d"
    refused(lib, ones(Q, 2, mm + 1, D), "sm", text % (mm + 1, D, mm, md))
    refused(lib, ones(Q, 2, 2, md + 1), "sm", dim_text(lib, md + 1, text % (2, md + 1, mm, md)))
    assert _engine._check_kernel_shape(lib, ones(Q, 2, mm, md), "sm") is None


def test_shape_check_periodic(lib):
    md = lib.cdll.plmc_per_max_dim()
    shape = "a periodic kernel's table is (q, 2, d) = [lengthscales | periods]"
    refused(lib, ones(Q, 3, D), "periodic", shape)
    refused(lib, ones(Q, D), "periodic", shape)
    refused(lib, ones(Q, 2, 2, D), "periodic", shape)
    refused(lib, ones(Q, 2, md + 1), "periodic",
            dim_text(lib, md + 1, "periodic kernel on %d dimensions exceeds plmc_per_max_dim()=%d" % (md + 1, md)))
    assert _engine._check_kernel_shape(lib, ones(Q, 2, md), "periodic") is None


def test_shape_check_locally_periodic(lib):
    md = lib.cdll.plmc_lper_max_dim()
    shape = "a locally periodic kernel's table is (q, 3, d) = [periodic lengthscales | periods | RBF lengthscales]"
    refused(lib, ones(Q, 2, D), "locally_periodic", shape)
    refused(lib, ones(Q, D), "locally_periodic", shape)
    refused(lib, ones(Q, 3, md + 1), "locally_periodic",
            dim_text(lib, md + 1, "locally periodic kernel on %d dimensions exceeds plmc_lper_max_dim()=%d" % (md + 1, md)))
    assert _engine._check_kernel_shape(lib, ones(Q, 3, md), "locally_periodic") is None


def test_shape_check_rational_quadratic(lib):
    md = lib.cdll.plmc_rq_max_dim()
    shape = "a rational-quadratic kernel's table is (q, d + 1) = [lengthscales | alpha]"
    refused(lib, ones(Q, 2, D + 1), "rq", shape)
    refused(lib, ones(Q, 1), "rq", shape)
    refused(lib, ones(Q, md + 2), "rq", "rational-quadratic kernel on %d dimensions exceeds plmc_rq_max_dim()=%d" % (md + 1, md))
    assert _engine._check_kernel_shape(lib, ones(Q, md + 1), "rq") is None


def test_shape_check_dot_product(lib):
    md, mp = lib.cdll.plmc_dot_max_dim(), lib.cdll.plmc_dot_max_power()
    shape = "a dot-product kernel's table is (q, d + 1) = [variances | offset]"
    limit = "dot-product kernel of power %d on %d dimensions exceeds plmc_dot_max_power()=%d / plmc_dot_max_dim()=%d"
    refused(lib, ones(Q, 2, D + 1), "linear", shape)
    refused(lib, ones(Q, 1), "poly2", shape)
    refused(lib, ones(Q, md + 2), "linear", limit % (1, md + 1, mp, md))
    refused(lib, ones(Q, D + 1), "poly%d" % (mp + 1), limit % (mp + 1, D, mp, md))
    refused(lib, ones(Q, D + 1), "poly0", limit % (0, D, mp, md))
    assert _engine._check_kernel_shape(lib, ones(Q, md + 1), "poly%d" % mp) is None


def test_shape_check_sum(lib):
    md, mc = lib.cdll.plmc_sum_max_dim(), lib.cdll.plmc_sum_max_components()
    shape = "the table of a sum of G kernels is (q, G, 3 d + 1) = [lengthscales | periods | RBF lengthscales | alpha] per member"
    limit = "sum of %d kernels on %d dimensions exceeds plmc_sum_max_components()=%d / plmc_sum_max_dim()=%d"
    refused(lib, ones(Q, 3 * D + 1), SUM_KIND, shape)                # no component axis
    refused(lib, ones(Q, 2, 3 * D), SUM_KIND, shape)                 # width is no 3 d + 1
    refused(lib, ones(Q, 2, 1), SUM_KIND, shape)                     # d = 0
    refused(lib, ones(Q, 3, 3 * D + 1), SUM_KIND, shape)             # three records, two members
    refused(lib, ones(Q, 2, 3 * D + 1), "sum(rbf,spline)",
            "a sum takes the stationary kinds, periodic, rq and locally_periodic members, not spline")
    refused(lib, ones(Q, 3, 3 * D + 1), "sum(linear,rbf,sm)",
            "a sum takes the stationary kinds, periodic, rq and locally_periodic members, not linear, sm")
    refused(lib, ones(Q, 2, 3 * (md + 1) + 1), SUM_KIND, limit % (2, md + 1, mc, md))
    many = _engine.sum_kind(["rbf"] * (mc + 1))
    refused(lib, ones(Q, mc + 1, 3 * D + 1), many, limit % (mc + 1, D, mc, md))
    assert _engine._check_kernel_shape(lib, ones(Q, mc, 3 * md + 1), _engine.sum_kind(["rq"] * mc)) is None
