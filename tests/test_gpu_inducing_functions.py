"""The hand-written autograd functions of the inducing-point paths, called DIRECTLY and compared with dense fp64 references
(tests/_inducing_fn_ref.py): _var_engine.WhitenedInterp, GaussianKLToKernelPrior, LowerTMatmul, prior_cholesky, unwhitened_predictive and
_dense.SpdQuadLogdet, spd_half_solve -- at one, two, three and four block rows (m in 1 .. 500, the real-data size), at sizes that are no
multiple of the 16-row contraction slab, in fp64 and, at the cases whose conditioning lets an fp32 bound say something, in fp32 with
jitter 0 (the SGPR configuration: eig_lo = 0 reaches the split engine's scales).

Every output: max |got - ref| <= 4 sqrt(max(m, n)) kappa u max |ref| (the module docstring of _inducing_fn_ref).  fp32 tensor outputs in
addition: error <= E32_RATIO x the error of the same dense formula in torch fp32 on the CPU; E32_RATIO = the next power of two at or above
4 x the worst ratio measured on the MI355X over all fp32 cases (profiles/inducing_accuracy.md).  Each check prints its figures (an
`ACC|` line) before it asserts."""
import functools
import re

import pytest
import torch

import _gemm_ref as gr
import _inducing_dense as idn
import _inducing_fn_ref as ifr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32, F64 = torch.float32, torch.float64
E32_RATIO = 16.0                 # profiles/inducing_accuracy.md: worst measured ratio x 4, rounded up to a power of two


@pytest.fixture(autouse=True)
def _nothing_more_after_a_gpu_error():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("HIP error, nothing more is started: %s" % e, returncode=3)


@pytest.fixture(scope="module")
def ve():
    from projectedlmc import _var_engine
    assert torch.cuda.is_available()
    return _var_engine


def _jitter(name, dtype):
    from projectedlmc.variational import variational_jitter
    return 0.0 if name == "jit0" else variational_jitter(dtype)


def _dev(t, dtype, grad=False):
    return None if t is None else t.to(DEV, dtype).contiguous().requires_grad_(grad)


def _dtname(dtype):
    return "fp32" if dtype == F32 else "fp64"


def check(label, name, got, ref, bnd, dtype, e32=None):
    """max |got - ref| <= bnd max |ref|; fp32 with an E32: also <= E32_RATIO x E32.  Prints before it asserts."""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (label, name, got.shape, ref.shape)
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max())
    rel = err / scale if scale > 0 else err
    ratio = rel / e32 if (e32 and dtype == F32) else float("nan")
    print("ACC|%s|%s|%s|bound %.3e|E32 %s|err %.3e|ratio %.3f" % (label, _dtname(dtype), name, bnd, "%.3e" % e32 if e32 else "-", rel, ratio))
    assert rel <= bnd, (label, name, rel, bnd)
    if e32 and dtype == F32:
        assert ratio <= E32_RATIO, (label, name, rel, e32, ratio)


# ------------------------------------------------------------------------------------------------ WhitenedInterp
def _run_interp(ve, case, jitter, dtype):
    p = ifr.problem(case)
    Z, X, ell, osc = _dev(p.Z, dtype, True), _dev(p.X, dtype, True), _dev(p.ell, dtype, True), _dev(p.oscale, dtype, True)
    A = ve.whitened_interp(case.kind, Z, X, ell, osc, jitter)
    (A * _dev(p.G, dtype)).sum().backward()
    return A.detach(), Z.grad, ell.grad, None if osc is None else osc.grad, X.grad


def _interp_case(ve, case, jname, dtype):
    jitter = _jitter(jname, dtype)
    ref, kap = ifr.interp_reference(case, jitter)
    bnd = ifr.bound(case.m, case.n, kap, dtype)
    e32 = ifr.interp_e32(case, jitter) if dtype == F32 else (None,) * 4
    label = "interp %s %s" % (ifr.case_id(case), jname)
    *got, gX = _run_interp(ve, case, jitter, dtype)
    assert gX is None                                                         # no gradient with respect to the data points
    for name, g, r, e in zip(("A", "gZ", "gEll", "gOs"), got, ref, e32):
        if r is None:
            assert g is None, name
            continue
        assert g.dtype == dtype
        check(label, name, g, r, bnd, dtype, e if name != "gOs" else None)
    return got


@pytest.mark.parametrize("jname", ["jit0", "vjit"])
@pytest.mark.parametrize("case", ifr.INTERP_CASES, ids=ifr.case_id)
def test_whitened_interp_fp64(ve, case, jname):
    _interp_case(ve, case, jname, F64)


@pytest.mark.parametrize("jname", ["jit0", "vjit"])
@pytest.mark.parametrize("case", ifr.FP32_CASES, ids=ifr.case_id)
def test_whitened_interp_fp32(ve, case, jname):
    """jit0 at m = 500 is the SGPR configuration: `_factorize_kzz` hands eig_lo = 0 to the split engine"""
    _interp_case(ve, case, jname, F32)


@pytest.mark.parametrize("case,dtype", [(ifr.BASE, F64), (ifr.FP32_CASES[1], F32)], ids=["base-fp64", "m500-fp32"])
def test_whitened_interp_two_runs_are_bit_equal(ve, case, dtype):
    a = _run_interp(ve, case, 0.0, dtype)
    b = _run_interp(ve, case, 0.0, dtype)
    for x, y in zip(a[:4], b[:4]):
        assert (x is None and y is None) or torch.equal(x, y)


# ------------------------------------------------------------------------------------------------ the unwhitened strategy
def _run_kl(ve, case, dtype):
    p = ifr.problem(case)
    ins = [_dev(t, dtype, True) for t in (p.Z, p.ell, p.oscale, p.mvar, p.Ls)]
    kl = ve.gaussian_kl_to_kernel_prior(case.kind, *ins, ifr.PRIOR_JITTER)
    (kl * _dev(p.gk, dtype)).sum().backward()
    return [kl.detach()] + [None if t is None else t.grad for t in ins]


def _kl_case(ve, case, dtype):
    ref, kap = ifr.kl_reference(case)
    n = case.m
    bnd = ifr.bound(n, n + 1, kap, dtype)
    e32 = ifr.kl_e32(case) if dtype == F32 else (None,) * 6
    label = "kl %s" % ifr.case_id(case)
    got = _run_kl(ve, case, dtype)
    for name, g, r, e in zip(("KL", "gZ", "gEll", "gOs", "gM", "gLs"), got, ref, e32):
        if r is None:
            assert g is None, name
            continue
        check(label, name, g, r, bnd, dtype, e if name not in ("KL", "gOs") else None)
    assert bool((torch.triu(got[5], 1) == 0).all())                           # the Ls gradient is lower triangular: exact zeros above


@pytest.mark.parametrize("case", ifr.KL_CASES, ids=ifr.case_id)
def test_gaussian_kl_to_kernel_prior_fp64(ve, case):
    _kl_case(ve, case, F64)


def test_gaussian_kl_to_kernel_prior_fp32(ve):
    _kl_case(ve, ifr.KL_CASE_FP32, F32)


@pytest.mark.parametrize("case", [ifr.KL_CASES[0], ifr.KL_CASES[3], ifr.KL_CASES[-1]], ids=ifr.case_id)
def test_prior_cholesky(ve, case):
    p = ifr.problem(case)
    K, _ = ifr.make_kernel(case.kind, p.ell, p.oscale, case.table)
    ref = ifr.prior_cholesky_ref(K, p.Z, ifr.PRIOR_JITTER)
    bnd = ifr.bound(case.m, case.m, ifr.kl_reference(case)[1], F64)
    Lp = ve.prior_cholesky(case.kind, _dev(p.Z, F64), _dev(p.ell, F64), _dev(p.oscale, F64), ifr.PRIOR_JITTER)
    label = "prior_cholesky %s" % ifr.case_id(case)
    check(label, "L", Lp, ref, bnd, F64)
    check(label, "L L^T", Lp @ Lp.transpose(-1, -2), ref @ ref.transpose(-1, -2), bnd, F64)
    assert bool((torch.triu(Lp, 1) == 0).all())


@pytest.mark.parametrize("ns", [1, 17, 130])
@pytest.mark.parametrize("case,dtype", [(ifr.KL_CASES[0], F64), (ifr.KL_CASES[3], F64), (ifr.KL_CASE_FP32, F32)],
                         ids=lambda v: ifr.case_id(v) if isinstance(v, ifr.Case) else _dtname(v))
def test_unwhitened_predictive(ve, case, dtype, ns):
    p = ifr.problem(case)
    g = torch.Generator().manual_seed(ns)
    Xs = ifr.r32(2 * torch.rand(ns, case.d, generator=g, dtype=F64) - 1)
    fn = functools.partial(ifr.predictive_outputs, case.kind, case.table, ifr.PRIOR_JITTER)
    ins = (p.Z, Xs, p.ell, p.oscale, p.mvar, p.Ls)
    ref = fn(*ins)
    e32 = ifr.fp32_dense_error(fn, ins) if dtype == F32 else (None, None)
    bnd = ifr.bound(case.m, ns, ifr.kl_reference(case)[1], dtype)
    with torch.no_grad():
        mean, var = ve.unwhitened_predictive(case.kind, _dev(p.Z, dtype), _dev(Xs, dtype), _dev(p.ell, dtype), _dev(p.oscale, dtype),
                                             _dev(p.mvar, dtype), _dev(p.Ls, dtype), ifr.PRIOR_JITTER)
    label = "predictive %s ns=%d" % (ifr.case_id(case), ns)
    check(label, "mean", mean, ref[0], bnd, dtype, e32[0])
    check(label, "var", var, ref[1], bnd, dtype, e32[1])


# ------------------------------------------------------------------------------------------------ _dense: SpdQuadLogdet, spd_half_solve
def _run_quad_logdet(s, dtype):
    from projectedlmc import _dense
    M, r = _dev(s.M, dtype, True), _dev(s.r, dtype, True)
    quad, logdet = _dense.spd_quad_logdet(M, r)
    ((quad * _dev(s.gq, dtype)).sum() + (logdet * _dev(s.gl, dtype)).sum()).backward()
    return quad.detach(), logdet.detach(), M.grad, r.grad


SPD_CASES = [(m, q, s, F64) for m in ifr.SPD_M for q in (1, 3) for s in (0.05, 1e-3)] + [(129, 3, 0.05, F32), (500, 1, 0.05, F32)]
_spd_id = lambda v: "m%d-q%d-s%g-%s" % (v[0], v[1], v[2], _dtname(v[3]))


@pytest.mark.parametrize("spd", SPD_CASES, ids=_spd_id)
def test_spd_quad_logdet(ve, spd):
    m, q, sval, dtype = spd
    s = ifr.spd_problem(m, q, sval)
    ref = ifr.quad_logdet_with_grads(s.M, s.r, s.gq, s.gl)
    e32 = ifr.fp32_dense_error(ifr.quad_logdet_with_grads, (s.M, s.r, s.gq, s.gl)) if dtype == F32 else (None,) * 4
    bnd = ifr.bound(m, 1, s.kappa, dtype)
    label = "quad_logdet %s kappa %.3g" % (_spd_id(spd), s.kappa)
    for name, g, r, e in zip(("quad", "logdet", "gM", "gr"), _run_quad_logdet(s, dtype), ref, e32):
        check(label, name, g, r, bnd, dtype, e if name in ("gM", "gr") else None)


@pytest.mark.parametrize("k", [1, 26, 130])
@pytest.mark.parametrize("spd", [(129, 3, 0.05, F64), (500, 1, 1e-3, F64), (1, 3, 0.05, F64), (500, 1, 0.05, F32)], ids=_spd_id)
def test_spd_half_solve(ve, spd, k):
    from projectedlmc import _dense
    m, q, sval, dtype = spd
    s = ifr.spd_problem(m, q, sval)
    R = s.R[..., :k].contiguous()
    ref = ifr.spd_half_solve_ref(s.M, R)
    e32, = ifr.fp32_dense_error(lambda M, Rr: (ifr.spd_half_solve_ref(M, Rr),), (s.M, R)) if dtype == F32 else (None,)
    got = _dense.spd_half_solve(_dev(s.M, dtype), _dev(R, dtype))
    check("half_solve %s k=%d" % (_spd_id(spd), k), "V", got, ref, ifr.bound(m, k, s.kappa, dtype), dtype, e32)


# ------------------------------------------------------------------------------------------------ LowerTMatmul
def test_lower_t_matmul_fp32_inside_the_tile_products_bound(ve):
    """fp32 at m = 260, n = 150 against fp64, forward and both adjoints, element by element inside gemm_tn's own bound
    (tests/_gemm_ref.py: (K + 4) u sum_k |a_ki| |b_kj|)"""
    q, m, n = 2, 260, 150
    g = torch.Generator().manual_seed(4)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=F64).float().double()
    Ls0, A0, G0 = torch.tril(rnd(q, m, m)), rnd(q, m, n), rnd(q, m, n)
    Ls, A = _dev(Ls0, F32, True), _dev(A0, F32, True)
    out = ve.lower_t_matmul(Ls, A)
    (out * _dev(G0, F32)).sum().backward()
    mT = lambda t: t.transpose(-1, -2).contiguous()
    # (operands as gemm_tn sees them: K-major A^T B) -> what stands there
    for name, got, a_km, b_kn, low in (("Ls^T A", out, Ls0, A0, False), ("gA = Ls G", A.grad, mT(Ls0), G0, False),
                                       ("gLs = tril(A G^T)", Ls.grad, mT(A0), mT(G0), True)):
        c0 = torch.zeros(q, a_km.shape[-1], b_kn.shape[-1], dtype=F64)
        ref, bnd = gr.reference(a_km, b_kn, c0, 0, 0), gr.bound(a_km, b_kn, c0, 0, 0, F32)
        if low:
            ref, bnd = torch.tril(ref), torch.tril(bnd)
        print("ACC|lower_t_matmul|fp32|%s|worst err / bound %.3f" % (name, gr.worst_ratio(got.detach().cpu(), ref, bnd)[0]))
        assert gr.outside(got.detach().cpu(), ref, bnd) == 0, (name, gr.violations(got.detach().cpu(), ref, bnd))


# ------------------------------------------------------------------------------------------------ workspace reuse
P_CASE, Q_CASE, Q_SAME_SHAPE = ifr.BASE, ifr.BASE._replace(m=257, n=300), ifr.BASE._replace(ell=0.3, kind="rbf")


@pytest.mark.parametrize("other", [Q_CASE, Q_SAME_SHAPE], ids=["another-shape", "same-shape-other-data"])
def test_interp_backward_after_another_forward_is_bit_equal(ve, other):
    """forward P, forward Q, backward P: what P saved for backward is a copy, never a view of the workspace Q has run in since"""
    alone = _run_interp(ve, P_CASE, 0.0, F64)
    p, o = ifr.problem(P_CASE), ifr.problem(other)
    Z, ell, osc = _dev(p.Z, F64, True), _dev(p.ell, F64, True), _dev(p.oscale, F64, True)
    A = ve.whitened_interp(P_CASE.kind, Z, _dev(p.X, F64), ell, osc, 0.0)
    Zo = _dev(o.Z, F64, True)
    Ao = ve.whitened_interp(other.kind, Zo, _dev(o.X, F64), _dev(o.ell, F64), _dev(o.oscale, F64), 0.0)
    assert torch.equal(A.detach(), alone[0])
    (A * _dev(p.G, F64)).sum().backward()
    for got, want in zip((Z.grad, ell.grad, osc.grad), alone[1:4]):
        assert torch.equal(got, want)
    (Ao * _dev(o.G, F64)).sum().backward()                                    # and Q's own backward still matches its reference
    ref, kap = ifr.interp_reference(other, 0.0)
    check("reuse %s" % ifr.case_id(other), "gZ", Zo.grad, ref[1], ifr.bound(other.m, other.n, kap, F64), F64)


@pytest.mark.parametrize("other", [(257, 2, 0.05), (129, 2, 1e-3)], ids=["another-shape", "same-shape-other-data"])
def test_quad_logdet_backward_after_another_forward_is_bit_equal(ve, other):
    from projectedlmc import _dense
    s, o = ifr.spd_problem(129, 2, 0.05), ifr.spd_problem(*other)
    alone = _run_quad_logdet(s, F64)
    M, r = _dev(s.M, F64, True), _dev(s.r, F64, True)
    quad, logdet = _dense.spd_quad_logdet(M, r)
    _dense.spd_quad_logdet(_dev(o.M, F64, True), _dev(o.r, F64, True))
    assert torch.equal(quad.detach(), alone[0]) and torch.equal(logdet.detach(), alone[1])
    ((quad * _dev(s.gq, F64)).sum() + (logdet * _dev(s.gl, F64)).sum()).backward()
    assert torch.equal(M.grad, alone[2]) and torch.equal(r.grad, alone[3])


@pytest.mark.parametrize("full_cov", [False, True])
def test_sgpr_posterior_interp_pair_shares_one_workspace(ve, full_cov):
    """LazySgprKernel.posterior calls interp() and interp(xs) back to back; with as many test points as training points both run in
    the SAME workspace entry, so the first A must have been copied out before the second sweep"""
    from types import SimpleNamespace
    from projectedlmc.sgpr import LazySgprKernel
    case = ifr.BASE
    p = ifr.problem(case)
    g = torch.Generator().manual_seed(3)
    Xs = ifr.r32(2 * torch.rand(case.n, case.d, generator=g, dtype=F64) - 1)
    K, _ = ifr.make_kernel(case.kind, p.ell, p.oscale)
    mu, cov = idn.sgpr_posterior(K, p.X, p.Z, p.noise, p.y, Xs)
    A, kap = ifr.interp_reference(case, 0.0)[0][0], ifr.interp_reference(case, 0.0)[1]
    bnd = ifr.bound(case.m, case.n, max(kap, ifr.kappa(ifr.woodbury_matrix(A, p.noise))), F64)
    lazy = LazySgprKernel(SimpleNamespace(jitter=0.0), case.kind, _dev(p.X, F64), _dev(p.Z, F64), _dev(p.ell, F64), _dev(p.oscale, F64),
                          _dev(p.noise, F64))
    with torch.no_grad():
        alone = lazy.interp().clone()                                         # the first interp, run alone
        A1 = lazy.interp()
        lazy.interp(_dev(Xs, F64))                                            # the second sweep, in the same workspace entry
        assert torch.equal(A1, alone)                                         # bit for bit what it was before that sweep
        mean, v = lazy.posterior(_dev(p.y, F64), _dev(Xs, F64), full_cov=full_cov)
    check("sgpr posterior pair", "mean", mean, mu, bnd, F64)
    check("sgpr posterior pair", "cov" if full_cov else "var", v, cov if full_cov else torch.diagonal(cov, dim1=-2, dim2=-1), bnd, F64)


# ------------------------------------------------------------------------------------------------ the deferred pivot check
def test_indefinite_kzz_raises_in_forward_without_grad_and_in_backward_with(ve):
    """a matrix that is not positive definite is an `info` code: K_ZZ - 0.5 I is certainly indefinite (K_ZZ has eigenvalues below 0.5)"""
    p = ifr.problem(ifr.BASE)
    K, _ = ifr.make_kernel(ifr.BASE.kind, p.ell, p.oscale)
    assert float(torch.linalg.eigvalsh(K(p.Z, p.Z)).min()) < 0.5
    args = lambda grad: (ifr.BASE.kind, _dev(p.Z, F64, grad), _dev(p.X, F64), _dev(p.ell, F64), _dev(p.oscale, F64), -0.5)
    with torch.no_grad(), pytest.raises(RuntimeError, match="K_ZZ \\+ jitter not positive definite"):
        ve.whitened_interp(*args(False))
    A = ve.whitened_interp(*args(True))                                        # with a backward pass to come, the check waits for it
    with pytest.raises(RuntimeError, match="K_ZZ \\+ jitter not positive definite"):
        A.sum().backward()
    _interp_case(ve, ifr.BASE, "jit0", F64)                                    # and the next call is sound


@pytest.mark.parametrize("k", [5, 130])
def test_quad_logdet_names_the_failing_pivot_of_the_failing_matrix(ve, k):
    from projectedlmc import _dense
    s = ifr.spd_problem(257, 3, 0.05)
    M = s.M.clone()
    M[1, k, k] = -1.0
    with pytest.raises(RuntimeError, match=re.escape("first failing pivot per matrix: [0, %d, 0]" % (k + 1))):
        _dense.spd_quad_logdet(_dev(M, F64), _dev(s.r, F64))
