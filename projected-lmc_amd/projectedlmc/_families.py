"""The covariance families of the batched exact engine, one row each, and the operations that exist once per family: what the Python
host layer knows about a family beside its mathematics.  The rows mirror the C host layer's (csrc/api_common.hpp: CovFamily, FAMILY[],
PLMC_FAMILY_ENTRIES); _hip generates its argument types from them, _engine routes, checks and sizes through them.  Nothing here
touches a device.

Every engine function takes a kernel's hyper-parameters as a kind, its table `ell` and `oscale`; each row's docstring says what they
are for its family and, in parentheses, what its entry points take.  The gradient table of every family is
[d/d table (ell[0].numel()) | d/d noise | d/d oscale (one per component)] and splits alike (_engine._split_grad_table).
"""
import ctypes

from .kernels import dot_power

_P, _I, _L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64

KIND = {"rbf": 0, "matern12": 1, "matern32": 2, "matern52": 3, "spline": 4}
# member codes of a heterogeneous sum (include/plmc.h, PLMC_FAM_*): the stationary kind codes and three more
FAM = {"rbf": 0, "matern12": 1, "matern32": 2, "matern52": 3, "periodic": 16, "rq": 17, "locally_periodic": 18}
PER, LPER, RQ, SUM = "periodic", "locally_periodic", "rq", "sum"


def ptr(t):
    return None if t is None else _P(t.data_ptr())


def is_sum(kind):
    return isinstance(kind, str) and kind.startswith(SUM + "(")


def sum_members(kind):
    return kind[len(SUM) + 1:-1].split(",")


class Family:
    """One row; its docstring is the layout of the family's table."""

    def __init__(self, doc, infix, argtypes, claims, flat, check, lead_kind=False, split=None, split_on_device=True, ncomp=lambda ell: 1,
                 per_kind=False, partials_bytes=lambda cdll, n_pad, q, ncomp, esz: cdll.plmc_grad_partials_bytes(n_pad, q * ncomp)):
        self.__doc__ = doc
        self.infix = infix                      # of its entry points' names (OPERATIONS)
        self.lead_kind = lead_kind              # `int kind` leads their arguments (else head[0], the kind's name, is dropped) ...
        self.argtypes = argtypes                # ... and flat arguments of these types stand where the plain form has `ell`
        self.claims = claims                    # claims(kind, ndim): a kind with a table of this rank is of this family (asked in _PRECEDENCE)
        self.split = split                      # split(ell, kind) -> what a call passes beside the table itself, kept on the table; None: nothing
        self.split_on_device = split_on_device  # ... device tensors, which a side stream has to know; not a host array
        self.flat = flat                        # flat(ell, kept, kind) -> the flat arguments
        self.check = check                      # check(L, ell, kind): ValueError for a table the library would refuse, by the library's limits
        self.ncomp = ncomp                      # ncomp(ell): its components -- entries of oscale and rows of gradient partials per latent
        self.per_kind = per_kind                # what _engine._per_kind answers: the workspace key of a family with a size call of its own ...
        self.partials_bytes = partials_bytes    # ... (cdll, n_pad, q, ncomp, esz) -> bytes of its gradient kernels' per-tile partial sums


def _unstack(count):
    """The split of a table that stacks `count` rows or planes along its second axis: one contiguous copy of each."""
    return lambda ell, kind: tuple(ell[:, i].contiguous() for i in range(count))


def _split_last(ell, kind):
    d = ell.shape[1] - 1
    return ell[:, :d].contiguous(), ell[:, d].contiguous()


def _check_dim(L, ell, kind=None):
    d = ell.shape[-1]
    if d > L.cdll.plmc_max_dim():
        raise ValueError("input dimension %d exceeds plmc_max_dim()=%d" % (d, L.cdll.plmc_max_dim()))


def _check_add(L, ell, kind):
    _check_dim(L, ell)
    if ell.shape[1] > L.cdll.plmc_max_components():
        raise ValueError("%d additive components exceed plmc_max_components()=%d" % (ell.shape[1], L.cdll.plmc_max_components()))


def _check_sm(L, ell, kind):
    _check_dim(L, ell)
    d, M = ell.shape[-1], ell.shape[2]
    if d > L.cdll.plmc_sm_max_dim() or M > L.cdll.plmc_sm_max_mixtures():
        raise ValueError("spectral mixture with %d components on %d dimensions exceeds plmc_sm_max_mixtures()=%d / plmc_sm_max_dim()=%d"
                         % (M, d, L.cdll.plmc_sm_max_mixtures(), L.cdll.plmc_sm_max_dim()))


def _check_rows(rows, shape_text, limit, limit_text):
    """The check of a table of `rows` stacked (q, d) rows."""
    def check(L, ell, kind):
        _check_dim(L, ell)
        if ell.dim() != 3 or ell.shape[1] != rows:
            raise ValueError(shape_text)
        if ell.shape[-1] > getattr(L.cdll, limit)():
            raise ValueError(limit_text % (ell.shape[-1], getattr(L.cdll, limit)()))
    return check


def _check_rq(L, ell, kind):
    d = ell.shape[-1] - 1
    if ell.dim() != 2 or d < 1:
        raise ValueError("a rational-quadratic kernel's table is (q, d + 1) = [lengthscales | alpha]")
    if d > L.cdll.plmc_rq_max_dim():
        raise ValueError("rational-quadratic kernel on %d dimensions exceeds plmc_rq_max_dim()=%d" % (d, L.cdll.plmc_rq_max_dim()))


def _check_sum(L, ell, kind):
    members, d = sum_members(kind), (ell.shape[-1] - 1) // 3
    if ell.dim() != 3 or ell.shape[-1] != 3 * d + 1 or d < 1 or ell.shape[1] != len(members):
        raise ValueError("the table of a sum of G kernels is (q, G, 3 d + 1) = [lengthscales | periods | RBF lengthscales | alpha] per member")
    unknown = [m_ for m_ in members if m_ not in FAM]
    if unknown:
        raise ValueError("a sum takes the stationary kinds, periodic, rq and locally_periodic members, not %s" % ", ".join(unknown))
    if d > L.cdll.plmc_sum_max_dim() or len(members) > L.cdll.plmc_sum_max_components():
        raise ValueError("sum of %d kernels on %d dimensions exceeds plmc_sum_max_components()=%d / plmc_sum_max_dim()=%d"
                         % (len(members), d, L.cdll.plmc_sum_max_components(), L.cdll.plmc_sum_max_dim()))


def _check_dot(L, ell, kind):
    d, P = ell.shape[-1] - 1, dot_power(kind)
    if ell.dim() != 2 or d < 1:
        raise ValueError("a dot-product kernel's table is (q, d + 1) = [variances | offset]")
    if d > L.cdll.plmc_dot_max_dim() or P < 1 or P > L.cdll.plmc_dot_max_power():
        raise ValueError("dot-product kernel of power %d on %d dimensions exceeds plmc_dot_max_power()=%d / plmc_dot_max_dim()=%d"
                         % (P, d, L.cdll.plmc_dot_max_power(), L.cdll.plmc_dot_max_dim()))


def _sum_codes(ell, kind):
    codes = [FAM[m_] for m_ in sum_members(kind)]
    return ((_I * len(codes))(*codes),)


Plain = Family(
    """One ARD kernel of a stationary kind per latent: `ell` (q, d), `oscale` (q) | None.  (kind, ..., ell): the kind's code in front, ell
    where every other family puts its flat arguments.""",
    "", [_P], lead_kind=True, claims=lambda kind, ndim: True, flat=lambda ell, kept, kind: (ptr(ell),), check=_check_dim)
Add = Family(
    """The COMPONENT TABLE of an additive kernel of one stationary kind: `ell` (q, G, d) with +inf (1 / ell = 0) on the dimensions a
    component ignores, `oscale` (q, G) | None (include/plmc.h, "Additive kernels"; additive.py builds it).  (kind, ..., G, ell).""",
    "_add", [_I, _P], lead_kind=True, claims=lambda kind, ndim: ndim == 3, flat=lambda ell, kept, kind: (ell.shape[1], ptr(ell)),
    check=_check_add, ncomp=lambda ell: ell.shape[1])
Sm = Family(
    """Kind "sm" (kernels.SpectralMixtureKernel): `ell` is the two planes of its table stacked, (q, 2, M, d) = [scales | means], `oscale`
    its weights (q, M) | None (include/plmc.h, "Spectral-mixture kernel").  (..., M, scales, means).  The table's rank names it.""",
    "_sm", [_I, _P, _P], claims=lambda kind, ndim: ndim == 4, split=_unstack(2),
    flat=lambda ell, kept, kind: (ell.shape[2], ptr(kept[0]), ptr(kept[1])), check=_check_sm, ncomp=lambda ell: ell.shape[2],
    partials_bytes=lambda cdll, n_pad, q, ncomp, esz: cdll.plmc_sm_grad_partials_bytes(n_pad, q, ncomp, esz))
Per = Family(
    """Kind "periodic" (kernels.PeriodicKernel): `ell` is the two rows of its table stacked, (q, 2, d) = [lengthscales | periods],
    `oscale` (q) | None (include/plmc.h, "Periodic kernel").  (..., lengthscales, periods).  The table has the rank of an additive one,
    so what sizes things takes the kind beside it.""",
    "_per", [_P, _P], claims=lambda kind, ndim: kind == PER, split=_unstack(2), flat=lambda ell, kept, kind: (ptr(kept[0]), ptr(kept[1])),
    check=_check_rows(2, "a periodic kernel's table is (q, 2, d) = [lengthscales | periods]",
                      "plmc_per_max_dim", "periodic kernel on %d dimensions exceeds plmc_per_max_dim()=%d"),
    per_kind=PER, partials_bytes=lambda cdll, n_pad, q, ncomp, esz: cdll.plmc_per_grad_partials_bytes(n_pad, q, esz))
Rq = Family(
    """Kind "rq" (kernels.RQKernel): `ell` is its table (q, d + 1) = [lengthscales | alpha], `oscale` (q) | None (include/plmc.h,
    "Rational-quadratic kernel").  (..., lengthscales, alpha).  The table has the rank of a plain one, so what reads the input
    dimension off the table takes the kind beside it.""",
    "_rq", [_P, _P], claims=lambda kind, ndim: kind == RQ, split=_split_last, flat=lambda ell, kept, kind: (ptr(kept[0]), ptr(kept[1])),
    check=_check_rq)
Lper = Family(
    """Kind "locally_periodic" (kernels.ProductKernel of a periodic and an RBF kernel): `ell` is the three rows of its table stacked,
    (q, 3, d) = [periodic lengthscales | periods | RBF lengthscales], `oscale` (q) | None (include/plmc.h, "Locally periodic kernel").
    (..., lengthscales, periods, RBF lengthscales).  Travels with its kind like the periodic table.""",
    "_lper", [_P, _P, _P], claims=lambda kind, ndim: kind == LPER, split=_unstack(3),
    flat=lambda ell, kept, kind: (ptr(kept[0]), ptr(kept[1]), ptr(kept[2])),
    check=_check_rows(3, "a locally periodic kernel's table is (q, 3, d) = [periodic lengthscales | periods | RBF lengthscales]",
                      "plmc_lper_max_dim", "locally periodic kernel on %d dimensions exceeds plmc_lper_max_dim()=%d"),
    per_kind=LPER, partials_bytes=lambda cdll, n_pad, q, ncomp, esz: cdll.plmc_lper_grad_partials_bytes(n_pad, q, esz))
Sum = Family(
    """Kind "sum(<member>,<member>,...)" (additive.AdditiveKernel with mixed members): the member kinds travel in the kind string, `ell`
    is the table (q, G, 3 d + 1) of records [lengthscales | periods | RBF lengthscales: d each | alpha] of which a member reads its own
    slots only, `oscale` (q, G) (include/plmc.h, "Sums of kernel families").  (..., G, fam, table), `fam` a host array of the members'
    codes that the library reads during the call; the table is not copied.""",
    "_sum", [_I, _P, _P], claims=lambda kind, ndim: is_sum(kind), split=_sum_codes, split_on_device=False,
    flat=lambda ell, kept, kind: (ell.shape[1], ctypes.addressof(kept[0]), ptr(ell)), check=_check_sum, ncomp=lambda ell: ell.shape[1],
    per_kind=SUM, partials_bytes=lambda cdll, n_pad, q, ncomp, esz: cdll.plmc_sum_grad_partials_bytes(n_pad, q, ncomp, esz))
Dot = Family(
    """Kind "linear" / "poly<P>" (kernels.LinearKernel, PolynomialKernel): the dot-product family.  `ell` is its table (q, d + 1) =
    [variances | offset], `oscale` (q) | None (include/plmc.h, "Dot-product kernels").  (..., variances, offset, P), P a host int read
    off the kind string (kernels.dot_power).  Sized and split like the rational-quadratic table.  The kernel is not stationary: what
    needs k(x, x) hands the table to kernels.prior_diagonal.""",
    "_dot", [_P, _P, _I], claims=lambda kind, ndim: dot_power(kind) is not None, split=_split_last,
    flat=lambda ell, kept, kind: (ptr(kept[0]), ptr(kept[1]), dot_power(kind)), check=_check_dot)

FAMILIES = (Plain, Add, Sm, Per, Rq, Lper, Sum, Dot)            # in the order of CovFamily
_PRECEDENCE = (Sum, Dot, Rq, Lper, Per, Sm, Add, Plain)         # a kind that names a family claims the table before its rank does
_claimed = {}


def family_of(kind, ndim=2):
    """The row of a kind (its name, its code or None) and the rank of its table; the predicates look at nothing else, so the answer is
    kept.  The rank matters only for the kinds that name no family."""
    fam = _claimed.get((kind, ndim))
    if fam is None:
        fam = _claimed[kind, ndim] = next(f for f in _PRECEDENCE if f.claims(kind, ndim))
    return fam


# The operations with one entry point per family: base name -> (name pattern with the infix slot, argument types in front of the
# table -- the leading `int kind` included --, argument types behind it, the families that have it).  By the rule of
# PLMC_FAMILY_ENTRIES a family's form drops the kind where it has none and puts its flat arguments where the plain form has `ell`.
OPERATIONS = {
    "plmc_assemble": ("plmc_assemble%s", [_I, _P, _I, _I], [_P, _P, _P, _L, _L, _I, _P], FAMILIES),
    # ... with a per-point noise vector behind the scalar noise: (pnoise, stride_pn) (include/plmc.h, "Per-point noise")
    "plmc_assemble_pn": ("plmc_assemble%s_pn", [_I, _P, _I, _I], [_P, _P, _P, _L, _P, _L, _L, _I, _P], FAMILIES),
    "plmc_factorize_pn_ex": ("plmc_factorize%s_pn_ex", [_I, _P, _I, _I], [_P, _P, _P, _L, _P, _L, _L, _I, _L, _P, _P, _P, _I, _I, _P, _P], FAMILIES),
    "plmc_assemble_cross": ("plmc_assemble_cross%s", [_I, _P, _I, _P, _I, _I], [_P, _P, _L, _L, _L, _L, _I, _P], FAMILIES),
    "plmc_factorize_ex": ("plmc_factorize%s_ex", [_I, _P, _I, _I], [_P, _P, _P, _L, _L, _I, _L, _P, _P, _P, _I, _I, _P, _P], FAMILIES),
    "plmc_kinv_grad_vd": ("plmc_kinv_grad%s_vd", [_I, _P, _L, _L, _L, _P, _P, _I, _I], [_P, _P, _P, _L, _L, _P, _P, _I, _P, _P, _P],
                          FAMILIES),
    "plmc_loo_grad": ("plmc_loo_grad%s", [_I, _P, _L, _L, _L, _L, _P, _P, _I, _I], [_P, _P, _P, _I, _P], FAMILIES),
    "plmc_weighted_grad": ("plmc_weighted_grad%s", [_I, _P, _P, _L, _L, _L, _L, _P, _I, _I], [_P, _P, _P, _I, _P], FAMILIES),
    "plmc_input_grad": ("plmc_input_grad%s", [_I, _P, _L, _L, _L, _P, _P, _I, _I], [_P, _P, _I, _P], FAMILIES),
    "plmc_posterior_dx": ("plmc_posterior_dx%s", [_I, _P, _I, _P, _I, _I], [_P, _P, _L, _P, _L, _L, _P, _P, _P, _I, _P], FAMILIES),
    "plmc_cross_matvec": ("plmc_cross_matvec%s", [_I, _P, _I, _P, _I, _I], [_P, _P, _L, _L, _I, _P, _P, _I, _P], FAMILIES),
    "plmc_cross_matvec_dx": ("plmc_cross_matvec_dx%s", [_I, _P, _I, _P, _I, _I], [_P, _P, _L, _L, _I, _P, _P, _P, _I, _P], FAMILIES),
    "plmc_kernel_vjp": ("plmc_kernel_vjp%s", [_I, _P, _I, _P, _I, _I], [_P, _P, _L, _L, _P, _P, _P, _I, _P], (Plain, Add)),
}


def entry_argtypes():
    """{entry-point name: argument types} of every family form of every operation."""
    return {pattern % f.infix: (head if f.lead_kind else head[1:]) + f.argtypes + tail
            for pattern, head, tail, fams in OPERATIONS.values() for f in fams}
