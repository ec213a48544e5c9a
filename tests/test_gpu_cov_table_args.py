"""The covariance-table descriptor of the C library's host layer (csrc/api_common.hpp, CovTable): what its one check and its one
dispatch must preserve for the eight families (plain, additive, spectral mixture, periodic, rational quadratic, locally periodic,
heterogeneous sum, dot product), both element types, through the raw entry points `plmc_assemble*`, `plmc_assemble_cross*`,
`plmc_factorize*_ex`, `plmc_kinv_grad*_vd` and `plmc_loo_grad*`.

1. A bad argument is refused on the host with -1 and the SAME text (the part of plmc_last_error() behind the function name) whatever the
   family and the element type, before anything is launched: the buffers keep their bits.
2. An additive table of one component is the plain kernel: factor buffer, log-determinant and gradient table equal as bit patterns
   (the assembly entry points alone: tests/test_gpu_additive_engine.py::test_assemble_add_and_cross_add_per_element, G = 1).

Shapes: n = 130 (two block rows, ragged edge), q = 2, d = 3, and d = 9 for the plain and additive families (the general assembly kernel).
The refused calls need no valid operands: the leave-one-out entry gets the inverse-factor columns as its operand `Xop` (krows = n_pad).

Two cases cannot be asked through the C ABI and are left out: the row / column range of the assembly is an argument of the sweep's
internal calls only (the entry points always assemble the whole matrix), and plmc_factorize*_ex with d above plmc_max_dim() for the
plain / additive family is refused by the assembly INSIDE the sweep, behind the sweep's first launches."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N, Q = 130, 2
FAMILIES = ("plain", "add", "sm", "per", "rq", "lper", "sum", "dot")
ENTRIES = ("assemble", "cross", "factorize", "kinv_grad", "loo_grad")
NAME = {"assemble": "plmc_assemble%s", "cross": "plmc_assemble_cross%s", "factorize": "plmc_factorize%s_ex", "kinv_grad": "plmc_kinv_grad%s_vd",
        "loo_grad": "plmc_loo_grad%s"}
INFIX = {"plain": "", "add": "_add", "sm": "_sm", "per": "_per", "rq": "_rq", "lper": "_lper", "sum": "_sum", "dot": "_dot"}
MATERN52 = 3
SUM_MEMBERS = (MATERN52, 16, 17, 18, 0)        # kind codes and PLMC_FAM_PERIODIC, PLMC_FAM_RQ, PLMC_FAM_LPER (include/plmc.h)


@pytest.fixture(scope="module")
def eng():
    import types
    from projectedlmc import _hip, _engine
    assert torch.cuda.is_available()
    return types.SimpleNamespace(hip=_hip, exact=_engine)


class _Buffers:
    """One set of device buffers per element type, large enough for every (also every refused) shape below."""

    def __init__(self, eng, dt, ncomp_max, d_max):
        self.dt = dt
        g = torch.Generator().manual_seed(5)
        r = lambda *shape: (0.5 + torch.rand(*shape, generator=g, dtype=torch.float64)).to(DEV, dt)
        self.X, self.ell, self.second, self.osc, self.nz = r(N, d_max), r(Q, ncomp_max, d_max), r(Q, ncomp_max, d_max), r(Q, ncomp_max), r(Q)
        self.third = r(Q, d_max)
        self.fam = (ctypes.c_int * len(SUM_MEMBERS))(*SUM_MEMBERS)      # host array of a sum's member codes
        self.ws = eng.exact.Workspace(N, Q, 1, dt, DEV, with_inverse=True, ncomp=ncomp_max)
        self.out = torch.empty(Q, self.ws.n_pad, N, dtype=dt, device=DEV)
        self.grad = torch.empty(Q, 2 * ncomp_max * d_max + ncomp_max + 1, dtype=torch.float64, device=DEV)


def _call(eng, b, family, entry, d=3, ncomp=2, null_second=False, null_third=False, null_fam=False, n_pad_off=0, lda_off=0, col0=0, ell=None,
          osc=None):
    """(return code, message behind the function name) of one raw call; the keyword arguments are the ones a case spoils.  `ncomp` is
    the component count of an additive table and of a sum, the mixture count of a spectral mixture and the power of a dot product."""
    hip, ws = eng.hip, b.ws
    p, st = hip.ptr, hip.stream_ptr(DEV)
    ell, osc = p(b.ell if ell is None else ell), p(b.osc if osc is None else osc)
    second = None if null_second else p(b.second)
    third = None if null_third else p(b.third)
    fam = None if null_fam else ctypes.addressof(b.fam)
    head = [MATERN52] if family in ("plain", "add") else []
    table = {"plain": [ell, osc], "add": [ncomp, ell, osc], "sm": [ncomp, ell, second, osc], "per": [ell, second, osc],
             "rq": [ell, second, osc], "lper": [ell, second, third, osc], "sum": [ncomp, fam, ell, osc], "dot": [ell, second, ncomp, osc]}[family]
    n_pad, lda = ws.n_pad + n_pad_off, ws.lda + lda_off
    if entry == "assemble":
        args = head + [p(b.X), N, d] + table + [p(b.nz), p(ws.A), lda, ws.strideA, Q, st]
    elif entry == "cross":
        args = head + [p(b.X), N, p(b.X), N, d] + table + [p(b.out), N, ws.n_pad * N, col0, ws.n_pad, Q, st]
    elif entry == "factorize":
        args = head + [p(b.X), N, d] + table + [p(b.nz), p(ws.A), n_pad, lda, ws.naug, ws.strideA, p(ws.Vd), p(ws.logdet), p(ws.info), 1, Q,
                                               p(b.nz), st]
    elif entry == "kinv_grad":
        args = head + [p(ws.W), n_pad, lda, ws.strideW, p(ws.alpha), p(b.X), N, d] + table + [p(b.grad), None, 0, 0, None, p(ws.partials), Q,
                                                                                            p(b.nz), p(ws.Vd), st]
    else:
        args = head + [p(ws.W), n_pad, ws.n_pad, lda, ws.strideW, p(ws.alpha), p(b.X), N, d] + table + [p(b.grad), p(ws.partials), Q, st]
    L = hip.lib()
    fn = getattr(L.cdll, NAME[entry] % INFIX[family] + ("_f32" if b.dt == torch.float32 else "_f64"))
    rc = fn(*args)
    return rc, L.cdll.plmc_last_error().decode().split(": ", 1)[-1]


def _cases(L):
    """(what is spoiled, families, entry -> expected text, keyword arguments of _call)."""
    gmax, mmax, smax, pmax = (L.cdll.plmc_max_components(), L.cdll.plmc_sm_max_mixtures(), L.cdll.plmc_sum_max_components(),
                              L.cdll.plmc_dot_max_power())
    assert (L.cdll.plmc_max_dim(), L.cdll.plmc_sm_max_dim(), L.cdll.plmc_per_max_dim()) == (32, 8, 8)
    assert (L.cdll.plmc_rq_max_dim(), L.cdll.plmc_lper_max_dim(), L.cdll.plmc_sum_max_dim(), L.cdll.plmc_dot_max_dim()) == (16, 8, 8, 16)
    assert smax + 1 <= len(SUM_MEMBERS)
    pad = "n_pad must be plmc_pad(n)"
    every = lambda text: {e: text for e in ENTRIES}
    return [
        ("range outside the matrix", FAMILIES, {"cross": "cross block exceeds the output buffer", "factorize": pad, "kinv_grad": pad,
                                                "loo_grad": pad}, dict(n_pad_off=128, col0=1)),
        ("lda not a multiple of the block", FAMILIES, {"assemble": "lda must be a multiple of NB and >= n_pad",
                                                      "factorize": "n_pad/lda must be multiples of NB", "kinv_grad": pad,
                                                      "loo_grad": "ldx must be a multiple of the block size, at least n_pad"}, dict(lda_off=64)),
        ("null second plane", ("sm", "per", "rq", "lper", "dot"), every("null pointer"), dict(null_second=True)),
        ("null third plane", ("lper",), every("null pointer"), dict(null_third=True)),
        ("null member list", ("sum",), every("null pointer"), dict(null_fam=True)),
        ("d above plmc_max_dim()", ("plain", "add"), {"assemble": "need n>0, q>0, 0<d<=plmc_max_dim()", "cross": "bad sizes",
                                                      "kinv_grad": "need 0<d<=plmc_max_dim(), q>0",
                                                      "loo_grad": "need 0<d<=plmc_max_dim(), q>0"}, dict(d=33)),
        ("d above plmc_sm_max_dim()", ("sm",), every("need 0 < d <= plmc_sm_max_dim()"), dict(d=9)),
        ("d above plmc_per_max_dim()", ("per",), every("need 0 < d <= plmc_per_max_dim()"), dict(d=9)),
        ("d above plmc_rq_max_dim()", ("rq",), every("need 0 < d <= plmc_rq_max_dim()"), dict(d=17)),
        ("d above plmc_lper_max_dim()", ("lper",), every("need 0 < d <= plmc_lper_max_dim()"), dict(d=9)),
        ("d above plmc_sum_max_dim()", ("sum",), every("need 0 < d <= plmc_sum_max_dim()"), dict(d=9)),
        ("d above plmc_dot_max_dim()", ("dot",), every("need 0 < d <= plmc_dot_max_dim()"), dict(d=17)),
        ("components above plmc_max_components()", ("add",), every("need 1 <= components <= plmc_max_components()"), dict(ncomp=gmax + 1)),
        ("mixtures above plmc_sm_max_mixtures()", ("sm",), every("need 1 <= mixtures <= plmc_sm_max_mixtures()"), dict(ncomp=mmax + 1)),
        ("components above plmc_sum_max_components()", ("sum",), every("need 1 <= components <= plmc_sum_max_components()"), dict(ncomp=smax + 1)),
        ("power above plmc_dot_max_power()", ("dot",), every("need 1 <= power <= plmc_dot_max_power()"), dict(ncomp=pmax + 1)),
    ]


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_bad_arguments_are_refused_alike_by_every_family(eng, dt):
    """Every case of _cases(), for every family and entry point it applies to: -1, the expected text, nothing written."""
    L = eng.hip.lib()
    b = _Buffers(eng, dt, ncomp_max=L.cdll.plmc_sm_max_mixtures() + 1, d_max=33)
    ws = b.ws
    ws.A.fill_(-3.0)
    ws.logdet.fill_(-7.0)
    ws.info.fill_(-3)
    b.out.fill_(-3.0)
    b.grad.fill_(-7.0)
    for what, families, expect, spoil in _cases(L):
        for family in families:
            for entry, text in expect.items():
                rc, msg = _call(eng, b, family, entry, **spoil)
                assert rc == -1 and msg == text, (what, family, entry, rc, msg)
    torch.cuda.synchronize()
    assert bool((ws.A == -3.0).all()) and bool((b.out == -3.0).all()) and bool((b.grad == -7.0).all())
    assert bool((ws.logdet == -7.0).all()) and bool((ws.info == -3).all())


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("d", [3, 9])
def test_additive_table_of_one_component_is_the_plain_kernel(eng, d, dt):
    """plmc_factorize_add_ex + plmc_kinv_grad_add_vd with ncomp = 1 against plmc_factorize_ex + plmc_kinv_grad_vd on the same inputs (the
    table (q, 1, d) IS ell (q, d), the scales (q, 1) ARE oscale (q)): the whole factor buffer (factor, inverse factor), the
    log-determinants, info and the gradient table [d ell | noise | oscale], as bit patterns.  fp32 runs the default split engine."""
    b = _Buffers(eng, dt, ncomp_max=1, d_max=d)
    ws = b.ws
    ell, osc = b.ell.reshape(Q, d).contiguous(), b.osc.reshape(Q).contiguous()
    g = torch.Generator().manual_seed(d)
    ws.alpha.copy_(torch.randn(Q, ws.n_pad, generator=g, dtype=torch.float64))
    bits = torch.int32 if dt == torch.float32 else torch.int64
    got = {}
    for family in ("plain", "add"):
        ws.A.zero_()
        b.grad.zero_()
        for entry in ("factorize", "kinv_grad"):
            rc, msg = _call(eng, b, family, entry, d=d, ncomp=1, ell=ell, osc=osc)
            assert rc == 0, (family, entry, msg)
        torch.cuda.synchronize()
        assert bool((ws.info == 0).all()), (family, ws.info)
        got[family] = (ws.A.view(bits).clone(), ws.logdet.view(torch.int64).clone(), b.grad.view(torch.int64).clone())
    for name, x, y in zip(("factor buffer", "log-determinant", "gradient table"), got["plain"], got["add"]):
        assert torch.equal(x, y), (name, int((x != y).sum()))
    assert bool(torch.isfinite(b.grad).all()) and bool((b.grad.view(-1)[:Q * (d + 2)] != 0).any()) and bool(torch.isfinite(ws.logdet).all())
