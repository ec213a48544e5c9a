"""The dense references of tests/_inducing_fn_ref.py, checked on the CPU: against oracle/variational.py and oracle/sgpr.py, by
torch.autograd.gradcheck, against the closed-form adjoint of _dense.py's docstring -- and the CONDITIONING of every case the GPU tests
run: each fp32 case has 4 sqrt(max(m, n)) kappa 2^-24 < 1e-2, and the same dense formula run in torch fp32 on the CPU factorises and
stays inside that bound (the reference alone passes what the engine is asked to pass)."""
import functools

import pytest
import torch

import _inducing_fn_ref as ifr
from oracle import gp_math as gm
from oracle import sgpr as osg
from oracle import variational as ov

F64 = torch.float64
SMALL = ifr.Case("matern52", 3, 5, 7, 2, True, 0.6)


def _close(a, b, tol=1e-12):
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), float((a - b).abs().max())


@pytest.mark.parametrize("kind", ["rbf", "matern32"])
def test_whitened_and_kl_refs_agree_with_the_variational_oracle(kind):
    c = ifr.BASE._replace(kind=kind, m=40, n=50)
    p = ifr.problem(c)
    okind, nu = ifr.KINDS[kind]
    K, kxx = ifr.make_kernel(kind, p.ell, p.oscale)
    A = ifr.whitened_interp_ref(K, p.Z, p.X, 1e-6)
    mean_f, var_f, _ = ov.latent_predictive(okind, p.X, p.Z, p.ell, p.mvar, p.Ls, nu, p.oscale, 1e-6)
    _close((A.transpose(-1, -2) @ p.mvar.unsqueeze(-1)).squeeze(-1), mean_f)
    Bm = p.Ls.transpose(-1, -2) @ A
    _close(kxx[:, None] + 1e-6 - (A * A).sum(-2) + (Bm * Bm).sum(-2), var_f)
    kl = ifr.kl_to_kernel_prior_ref(K, p.Z, p.mvar, p.Ls, 1e-3)
    Xs = p.X[:9]
    mean_u, var_u, kl_o = ov.unwhitened_latent_predictive(okind, Xs, p.Z, p.ell, p.mvar, p.Ls, nu, p.oscale, 1e-3)
    _close(kl, kl_o, 1e-11)
    mean, var = ifr.unwhitened_predictive_ref(K, kxx, p.Z, Xs, p.mvar, p.Ls, 1e-3)
    _close(mean, mean_u)
    _close(var, var_u)
    Lp = ifr.prior_cholesky_ref(K, p.Z, 1e-3)
    _close(Lp @ Lp.transpose(-1, -2), gm.kernel_matrix(okind, p.Z, p.Z, p.ell, p.oscale, nu) + 1e-3 * torch.eye(c.m, dtype=F64))
    assert bool((torch.triu(Lp, 1) == 0).all())


def test_table_kernel_is_the_sum_of_its_components():
    c = ifr.BASE._replace(table=True, m=20, n=30)
    p = ifr.problem(c)
    K, kxx = ifr.make_kernel(c.kind, p.ell, p.oscale, True)
    want = sum(gm.kernel_matrix("matern", p.Z[:, idx], p.X[:, idx], p.ell[:, g, idx], p.oscale[:, g], 2.5) for g, idx in enumerate(ifr.DECOMP))
    _close(K(p.Z, p.X), want)
    _close(kxx, p.oscale.sum(-1))
    assert bool(torch.isinf(p.ell[:, 0, 2]).all()) and bool(torch.isinf(p.ell[:, 1, 0]).all())


@pytest.mark.parametrize("table", [False, True])
def test_sgpr_value_ref_agrees_with_the_sgpr_oracle(table):
    c = ifr.BASE._replace(m=30, n=60, table=table)
    p = ifr.problem(c)
    val = ifr.sgpr_value_ref(c.kind, p.X, p.Z, p.ell, p.oscale, p.noise, p.y, table)
    if not table:
        lp, tr = osg.sgpr_terms("matern", p.X, p.Z, p.ell, p.noise, p.y, 2.5, p.oscale)
        assert torch.equal(val, lp + tr)
    # independent of either: Woodbury through the references of this module
    K, kxx = ifr.make_kernel(c.kind, p.ell, p.oscale, table)
    A = ifr.whitened_interp_ref(K, p.Z, p.X, 0.0)
    B = ifr.woodbury_matrix(A, p.noise)
    quad, logdetB = ifr.spd_quad_logdet_ref(B, (A @ p.y.unsqueeze(-1)).squeeze(-1))
    n = c.n
    lp_w = -0.5 * (((p.y * p.y).sum(-1) - quad / p.noise) / p.noise + n * torch.log(p.noise) + logdetB + n * gm.LOG2PI)
    tr_w = -0.5 * (n * kxx - (A * A).sum((-2, -1))) / p.noise
    _close(val, lp_w + tr_w, 1e-10)
    c_half = ifr.spd_half_solve_ref(B, (A @ p.y.unsqueeze(-1)))
    _close((c_half * c_half).sum((-2, -1)), quad, 1e-11)


@pytest.mark.parametrize("table", [False, True])
def test_gradcheck_of_the_differentiable_references(table):
    c = SMALL._replace(table=table)
    p = ifr.problem(c)
    free = lambda t: t.detach().clone().requires_grad_(True)

    def with_kernel(fn):
        def f(Z, ell_free, osc, *rest):
            ell = ell_free if not table else torch.where(torch.isinf(p.ell), p.ell, ell_free)
            return fn(ifr.make_kernel(c.kind, ell, osc, table), Z, *rest)
        return f
    ell0 = torch.where(torch.isinf(p.ell), torch.ones_like(p.ell), p.ell)
    interp = with_kernel(lambda Kk, Z: ifr.whitened_interp_ref(Kk[0], Z, p.X, 1e-6))
    assert torch.autograd.gradcheck(interp, (free(p.Z), free(ell0), free(p.oscale)), atol=1e-7, rtol=1e-6)
    kl = with_kernel(lambda Kk, Z, mv, Ls: ifr.kl_to_kernel_prior_ref(Kk[0], Z, mv, Ls, 1e-3))
    assert torch.autograd.gradcheck(kl, (free(p.Z), free(ell0), free(p.oscale), free(p.mvar), free(p.Ls)), atol=1e-7, rtol=1e-6)
    if not table:
        val = lambda Z, ell, osc, nz, y: ifr.sgpr_value_ref(c.kind, p.X, Z, ell, osc, nz, y)
        assert torch.autograd.gradcheck(val, (free(p.Z), free(p.ell), free(p.oscale), free(p.noise), free(p.y)), atol=1e-7, rtol=1e-6)
    s = ifr.spd_problem(5, 2, 0.05)
    sym = lambda M, r: ifr.spd_quad_logdet_ref(0.5 * (M + M.transpose(-1, -2)), r)
    assert torch.autograd.gradcheck(sym, (free(s.M), free(s.r)), atol=1e-7, rtol=1e-6)


@pytest.mark.parametrize("m,q", [(5, 2), (129, 3)])
def test_quad_logdet_gradients_match_the_closed_form(m, q):
    """dM = -g_q beta beta^T + g_l M^-1, dr = 2 g_q beta, beta = M^-1 r (projectedlmc/_dense.py), evaluated densely"""
    s = ifr.spd_problem(m, q, 0.05)
    quad, logdet, gM, gr = ifr.quad_logdet_with_grads(s.M, s.r, s.gq, s.gl)
    Minv = torch.linalg.inv(s.M)
    beta = (Minv @ s.r.unsqueeze(-1)).squeeze(-1)
    _close(gM, -s.gq[:, None, None] * beta.unsqueeze(-1) * beta.unsqueeze(-2) + s.gl[:, None, None] * Minv, 1e-10)
    _close(gr, 2.0 * s.gq[:, None] * beta, 1e-10)
    _close(quad, (s.r * beta).sum(-1), 1e-11)
    _close(logdet, torch.log(torch.linalg.eigvalsh(s.M)).sum(-1), 1e-11)


def test_problem_is_seeded_and_holds_fp32_values():
    a = ifr.problem(ifr.BASE)
    ifr.problem.cache_clear()
    b = ifr.problem(ifr.BASE)
    for k, v in vars(a).items():
        if torch.is_tensor(v):
            assert torch.equal(v, getattr(b, k)) and torch.equal(v, v.float().double()), k
    assert bool((a.Z.abs() <= 1).all()) and bool((torch.triu(a.Ls, 1) == 0).all())


# ------------------------------------------------------------------------------------------------ conditioning of the GPU cases
@pytest.mark.parametrize("case", ifr.INTERP_CASES, ids=ifr.case_id)
def test_fp64_interp_cases_are_inside_their_cap(case):
    for jitter in (0.0, 1e-6):
        _, kap = ifr.interp_reference(case, jitter)
        print(ifr.case_id(case), jitter, "kappa %.3g bound %.3g" % (kap, ifr.bound(case.m, case.n, kap, F64)))
        assert ifr.bound(case.m, case.n, kap, F64) < ifr.FP64_CAP


@pytest.mark.parametrize("case", ifr.KL_CASES, ids=ifr.case_id)
def test_fp64_kl_cases_are_inside_their_cap(case):
    _, kap = ifr.kl_reference(case)
    assert ifr.bound(case.m, case.m + 1, kap, F64) < ifr.FP64_CAP


@pytest.mark.parametrize("jitter", [0.0, 1e-4])
@pytest.mark.parametrize("case", ifr.FP32_CASES, ids=ifr.case_id)
def test_fp32_interp_cases_qualify_and_the_dense_fp32_run_is_inside_the_bound(case, jitter):
    _, kap = ifr.interp_reference(case, jitter)
    bnd = ifr.bound(case.m, case.n, kap, torch.float32)
    e32 = ifr.interp_e32(case, jitter)                 # a failed fp32 factorisation raises here
    print(ifr.case_id(case), jitter, "kappa %.3g bound %.3g E32(A, gZ, gEll)" % (kap, bnd), e32)
    assert bnd < ifr.FP32_CAP, (kap, bnd)
    assert all(e is None or e <= bnd for e in e32), (e32, bnd)


def test_fp32_kl_case_qualifies():
    case = ifr.KL_CASE_FP32
    _, kap = ifr.kl_reference(case)
    bnd = ifr.bound(case.m, case.m + 1, kap, torch.float32)
    e32 = ifr.kl_e32(case)
    print("kappa %.3g bound %.3g E32(kl, gZ, gEll, gOs, gM, gLs)" % (kap, bnd), e32)
    assert bnd < ifr.FP32_CAP
    assert all(e is None or e <= bnd for e in e32), (e32, bnd)
    p = ifr.problem(case)
    g = torch.Generator().manual_seed(17)
    Xs = ifr.r32(2 * torch.rand(17, case.d, generator=g, dtype=F64) - 1)
    e32 = ifr.fp32_dense_error(functools.partial(ifr.predictive_outputs, case.kind, False, ifr.PRIOR_JITTER),
                               (p.Z, Xs, p.ell, p.oscale, p.mvar, p.Ls))
    assert all(e <= bnd for e in e32), (e32, bnd)


@pytest.mark.parametrize("m,q", [(129, 3), (500, 1)])
def test_fp32_spd_cases_qualify(m, q):
    """M = I + A A^T / s at s = 0.05 is inside the fp32 cap; at s = 1e-3 (kappa 1e4 - 1e5) it is not and runs in fp64 only"""
    s = ifr.spd_problem(m, q, 0.05)
    bnd = ifr.bound(m, 130, s.kappa, torch.float32)
    assert bnd < ifr.FP32_CAP, (s.kappa, bnd)
    e32 = ifr.fp32_dense_error(ifr.quad_logdet_with_grads, (s.M, s.r, s.gq, s.gl))
    assert all(e <= bnd for e in e32), (e32, bnd)
    hard = ifr.spd_problem(m, q, 1e-3)
    assert ifr.bound(m, 130, hard.kappa, torch.float32) > ifr.FP32_CAP and ifr.bound(m, 130, hard.kappa, F64) < ifr.FP64_CAP, hard.kappa


@pytest.mark.parametrize("case", ifr.FP32_CASES[:2], ids=ifr.case_id)
def test_fp32_sgpr_value_is_inside_the_bound(case):
    """the m = 500, jitter-0 SGPR value in dense fp32 (no Woodbury): kappa = the larger of K_ZZ's and B's"""
    p = ifr.problem(case)
    (A, *_), kap = ifr.interp_reference(case, 0.0)
    kap = max(kap, ifr.kappa(ifr.woodbury_matrix(A, p.noise)))
    bnd = ifr.bound(case.m, case.n, kap, torch.float32)
    assert bnd < ifr.FP32_CAP, (kap, bnd)
    e32, = ifr.fp32_dense_error(lambda X, Z, ell, nz, y: (ifr.sgpr_value_ref(case.kind, X, Z, ell, None, nz, y),), (p.X, p.Z, p.ell, p.noise, p.y))
    assert e32 <= bnd, (e32, bnd)


@pytest.mark.parametrize("case", ifr.SGPR_MODEL_CASES, ids=ifr.case_id)
def test_sgpr_model_cases_qualify_for_fp32(case):
    """the whole-model cases of tests/test_gpu_sgpr_sizes.py: inside the fp32 cap, and the dense fp32 run (oracle/sgpr.py, no Woodbury)
    inside the bound"""
    ref, kap, e32 = ifr.sgpr_model_reference(case)
    bnd = ifr.bound(case.m, case.n, kap, torch.float32)
    print(ifr.case_id(case), "kappa %.3g bound %.3g E32(mll, gZ, gEll, gOs, gNoise, mean, cov)" % (kap, bnd), e32)
    assert bnd < ifr.FP32_CAP, (kap, bnd)
    assert all(e is None or e <= bnd for e in e32), (e32, bnd)
    assert ref[1].shape == (case.m, case.d) and ref[6].shape == (1, 25, 25)
