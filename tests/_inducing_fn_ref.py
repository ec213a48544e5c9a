"""Dense fp64 references of the inducing-point FUNCTIONS (projectedlmc/_var_engine.py: WhitenedInterp, GaussianKLToKernelPrior,
prior_cholesky, unwhitened_predictive; projectedlmc/_dense.py: SpdQuadLogdet, spd_half_solve) and of the SGPR value, the seeded problems
they are run on and the yardsticks of their tests.  TEST INFRASTRUCTURE ONLY: plain torch on the CPU, nothing from the package; kernels
are `oracle.gp_math.kernel_matrix`, component tables go through tests/_inducing_dense.py.

Shared by tests/test_inducing_fn_ref_host.py (the references against the oracle, gradcheck, the conditioning of every case),
tests/test_gpu_inducing_functions.py and tests/test_gpu_sgpr_sizes.py.

Tolerance of every output, both element types (u = 2^-53 | 2^-24, kappa of the matrix the sweep factorises, from the fp64 reference):
    max |got - ref| <= 4 sqrt(max(m, n)) kappa u max |ref|
-- the bound of tests/test_gpu_variational.py::test_elbo_and_all_gradients_fp32 (a chain of ~4 products / triangular solves of length
L = max(m, n) that applies L^-1 twice; rounding errors modelled as independent, Higham & Mary 2019).  fp32 tensor outputs are held, in
addition, to a multiple of E32 = the error of the SAME dense formula run in torch fp32 on the CPU (fp32_dense_error)."""
import functools
import math
from collections import namedtuple
from types import SimpleNamespace

import torch

import _inducing_dense as idn
from oracle import gp_math as gm
from oracle import sgpr as osg

KINDS = {"rbf": ("rbf", 2.5), "matern12": ("matern", 0.5), "matern32": ("matern", 1.5), "matern52": ("matern", 2.5)}
UNIT = {torch.float64: 2.0 ** -53, torch.float32: 2.0 ** -24}
DECOMP = [[0, 1], [1, 2]]                    # the component table of the `table` cases: d = 3, dimension 1 shared
FP32_CAP = 1e-2                              # an fp32 case must have bound(...) below this, or its bound says nothing
FP64_CAP = 1e-8

# kind, d, inducing points m, data points n, latents q, output scale, nominal lengthscale, component table
Case = namedtuple("Case", "kind d m n q oscale ell table", defaults=("matern52", 3, 129, 130, 2, True, 0.25, False))
BASE = Case()


def case_id(c):
    return "%s-d%d-m%d-n%d-q%d-%s-ell%g%s" % (c.kind, c.d, c.m, c.n, c.q, "os" if c.oscale else "noos", c.ell, "-table" if c.table else "")


def one_axis(base, **axes):
    """base, then one case per value of each axis with everything else as in base (no duplicates, order kept)"""
    out = [base]
    for name, values in axes.items():
        for v in values:
            c = base._replace(**{name: v})
            if c not in out:
                out.append(c)
    return out


# the qualifying fp32 cases: no output scale, jitter 0 allowed (kappa(K_ZZ) of a few hundred; asserted in the host test)
FP32_CASES = [Case("rbf", 8, 500, 600, 2, False, 0.70), Case("matern52", 3, 500, 600, 2, False, 0.15),
              Case("matern12", 3, 500, 600, 2, False, 0.50), Case("matern52", 3, 257, 300, 2, False, 0.25),
              Case("rbf", 3, 500, 600, 2, False, 0.12)]
INTERP_CASES = one_axis(BASE, m=(1, 127, 128, 257, 500), n=(1, 600), kind=("rbf", "matern12", "matern32"), oscale=(False,), q=(1, 3),
                        table=(True,))
# the unwhitened strategy: Z = the n training inputs, so m == n; 300 needs 301 augmented columns
KL_CASES = one_axis(BASE._replace(m=129, n=129), m=(127, 128, 300), kind=("rbf", "matern12"), oscale=(False,), q=(1, 3), table=(True,))
KL_CASE_FP32 = Case("matern52", 3, 257, 257, 2, False, 0.25)
SPD_M = (1, 30, 128, 129, 500)
PRIOR_JITTER = 1e-3


def bound(m, n, kappa, dtype):
    return 4.0 * math.sqrt(max(m, n)) * kappa * UNIT[dtype]


def kappa(M):
    """largest over smallest eigenvalue per latent, the maximum over the latents"""
    ev = torch.linalg.eigvalsh(M.detach().double())
    return float((ev[..., -1] / ev[..., 0]).max())


def r32(t):
    """rounded to fp32 and widened again: both element types then see equal inputs"""
    return t.float().double()


def make_kernel(kind, ell, oscale, table=False):
    """(K(Xa, Xb) -> (q, na, nb), k(x, x) (q)) from ell (q, d) and oscale (q) | None, or from the component table ell (q, G, d) (inf
    outside a group) and oscale (q, G) | None over DECOMP.  Differentiable in ell and oscale; any floating element type."""
    okind, nu = KINDS[kind]
    q = ell.shape[0]
    if not table:
        kxx = torch.ones(q, dtype=ell.dtype) if oscale is None else oscale
        return (lambda Xa, Xb: gm.kernel_matrix(okind, Xa, Xb, ell, oscale, nu)), kxx
    ells = [ell[:, g, idx] for g, idx in enumerate(DECOMP)]
    oss = [None if oscale is None else oscale[:, g] for g in range(len(DECOMP))]
    kxx = sum(torch.ones(q, dtype=ell.dtype) if o is None else o for o in oss)
    return idn.additive_kernel(okind, nu, DECOMP, ells, oss), kxx


@functools.lru_cache(maxsize=None)
def problem(case):
    """One seeded recipe per case, fp64 tensors holding fp32 values: Z (m,d), X (n,d) uniform in [-1,1]^d, y (q,n), ell, oscale, the
    cotangents G (q,m,n), gk (q), the variational mean mvar (q,m) and factor Ls (q,m,m) lower, r (q,m), 25 test points Xs."""
    c = case
    g = torch.Generator().manual_seed(100 * c.d + c.m)
    rand = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    randn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    Z, X = 2 * rand(c.m, c.d) - 1, 2 * rand(c.n, c.d) - 1
    ell = c.ell * (0.9 + 0.1 * rand(c.q, c.d))
    osc = 0.5 + rand(c.q) if c.oscale else None
    if c.table:
        assert c.d == 3
        full, ell = ell, torch.full((c.q, len(DECOMP), c.d), float("inf"), dtype=torch.float64)
        for k, idx in enumerate(DECOMP):
            ell[:, k, idx] = full[:, idx] * (1.0 + 0.5 * k)
        osc = 0.5 + rand(c.q, len(DECOMP)) if c.oscale else None
    Ls = torch.tril(0.05 * randn(c.q, c.m, c.m), -1) + torch.diag_embed(0.5 + rand(c.q, c.m))
    p = SimpleNamespace(case=c, Z=Z, X=X, ell=ell, oscale=osc, y=randn(c.q, c.n), G=randn(c.q, c.m, c.n), gk=0.5 + rand(c.q),
                        mvar=randn(c.q, c.m), Ls=Ls, r=randn(c.q, c.m), Xs=2 * rand(25, c.d) - 1, noise=0.05 + 0.1 * rand(c.q))
    for k, v in vars(p).items():
        if torch.is_tensor(v):
            setattr(p, k, r32(v))
    return p


# ------------------------------------------------------------------------------------------------ the references
def _eye(m, like):
    return torch.eye(m, dtype=like.dtype)


def whitened_interp_ref(K, Z, X, jitter):
    """A = L^-1 K(Z, X), L L^T = K(Z, Z) + jitter I, (q, m, n); differentiable in whatever K and Z were built from"""
    L = torch.linalg.cholesky(K(Z, Z) + jitter * _eye(Z.shape[0], Z))
    return torch.linalg.solve_triangular(L, K(Z, X), upper=False)


def kl_to_kernel_prior_ref(K, Z, mvar, Ls, jitter):
    """KL(N(m, Ls Ls^T) || N(0, Khat)) = 1/2 [tr(Khat^-1 S) + m^T Khat^-1 m - n + log det Khat - log det S], Khat = K(Z, Z) + jitter I,
    per latent (q)"""
    n = Z.shape[0]
    Khat = K(Z, Z) + jitter * _eye(n, Z)
    Lt = Ls.tril()
    S = Lt @ Lt.transpose(-1, -2)
    tr = torch.diagonal(torch.linalg.solve(Khat, S), dim1=-2, dim2=-1).sum(-1)
    quad = (mvar * torch.linalg.solve(Khat, mvar.unsqueeze(-1)).squeeze(-1)).sum(-1)
    logdetS = 2.0 * torch.log(torch.diagonal(Lt, dim1=-2, dim2=-1).abs()).sum(-1)
    return 0.5 * (tr + quad - n + torch.linalg.slogdet(Khat)[1] - logdetS)


def prior_cholesky_ref(K, Z, jitter):
    return torch.linalg.cholesky(K(Z, Z) + jitter * _eye(Z.shape[0], Z))


def unwhitened_predictive_ref(K, kxx, Z, X, mvar, Ls, jitter):
    """(mean (q, ns), var (q, ns)) of q(f(X)) under the unwhitened strategy, X away from Z"""
    mean, var, _ = idn.unwhitened_latent_predictive(K, kxx, X, Z, mvar, Ls, jitter)
    return mean, var


def spd_quad_logdet_ref(M, r):
    """(r^T M^-1 r, log det M) per matrix"""
    return (r * torch.linalg.solve(M, r.unsqueeze(-1)).squeeze(-1)).sum(-1), torch.linalg.slogdet(M)[1]


def spd_half_solve_ref(M, R):
    """L^-1 R, L L^T = M"""
    return torch.linalg.solve_triangular(torch.linalg.cholesky(M), R, upper=False)


def sgpr_value_ref(kind, X, Z, ell, oscale, noise, y, table=False):
    """log N(y; 0, Q + s I) - 1/2 sum_i (k_ii - q_ii) / s per latent (q): oracle/sgpr.py for the plain kinds, _inducing_dense.sgpr_terms
    for a component table"""
    if not table:
        okind, nu = KINDS[kind]
        lp, tr = osg.sgpr_terms(okind, X, Z, ell, noise, y, nu, oscale)
    else:
        K, kxx = make_kernel(kind, ell, oscale, True)
        lp, tr = idn.sgpr_terms(K, kxx, X, Z, noise, y)
    return lp + tr


def woodbury_matrix(A, s):
    """B = I + A A^T / s per latent: the matrix _dense.py factorises on the SGPR path; s (q) or a number"""
    s = torch.as_tensor(s, dtype=A.dtype).reshape(-1, 1, 1)
    return _eye(A.shape[-2], A) + (A @ A.transpose(-1, -2)) / s


# ------------------------------------------------------------------------------------------------ value + gradients, any element type
def _leaves(*ts):
    return [None if t is None else t.detach().clone().requires_grad_(True) for t in ts]


def _grads(val, leaves):
    live = [t for t in leaves if t is not None]
    g = iter(torch.autograd.grad(val, live, allow_unused=True))
    return [None if t is None else next(g) for t in leaves]


def interp_with_grads(kind, table, jitter, Z, X, ell, oscale, G):
    """(A, gZ, gEll, gOs | None) of <G, A> by autograd of whitened_interp_ref"""
    Z, ell, oscale = _leaves(Z, ell, oscale)
    K, _ = make_kernel(kind, ell, oscale, table)
    A = whitened_interp_ref(K, Z, X, jitter)
    return (A.detach(),) + tuple(_grads((G * A).sum(), [Z, ell, oscale]))


def kl_with_grads(kind, table, jitter, Z, ell, oscale, mvar, Ls, gk):
    """(KL (q), gZ, gEll, gOs | None, gM, gLs) of <gk, KL> by autograd of kl_to_kernel_prior_ref"""
    Z, ell, oscale, mvar, Ls = _leaves(Z, ell, oscale, mvar, Ls)
    K, _ = make_kernel(kind, ell, oscale, table)
    kl = kl_to_kernel_prior_ref(K, Z, mvar, Ls, jitter)
    return (kl.detach(),) + tuple(_grads((gk * kl).sum(), [Z, ell, oscale, mvar, Ls]))


def quad_logdet_with_grads(M, r, gq, gl):
    """(quad, logdet, gM, gr) of <gq, quad> + <gl, logdet> by autograd of spd_quad_logdet_ref"""
    M, r = _leaves(M, r)
    quad, logdet = spd_quad_logdet_ref(M, r)
    return (quad.detach(), logdet.detach()) + tuple(_grads((gq * quad).sum() + (gl * logdet).sum(), [M, r]))


def predictive_outputs(kind, table, jitter, Z, X, ell, oscale, mvar, Ls):
    K, kxx = make_kernel(kind, ell, oscale, table)
    return unwhitened_predictive_ref(K, kxx, Z, X, mvar, Ls, jitter)


def fp32_dense_error(fn, inputs):
    """E32: fn(*inputs) in torch fp32 on the CPU against the same call in fp64, per tensor output max |fp32 - fp64| / max |fp64| (None
    for an output that is None).  The error of an honest fp32 implementation of the same dense formula on the same inputs."""
    cast = lambda t, dt: t.to(dt) if torch.is_tensor(t) and t.is_floating_point() else t
    o64 = fn(*[cast(t, torch.float64) for t in inputs])
    o32 = fn(*[cast(t, torch.float32) for t in inputs])
    out = []
    for a, b in zip(o32, o64):
        if b is None:
            out.append(None)
            continue
        assert a.dtype == torch.float32 and b.dtype == torch.float64
        out.append(float((a.double() - b).abs().max() / b.abs().max()))
    return out


@functools.lru_cache(maxsize=None)
def interp_reference(case, jitter):
    """(fp64 outputs of interp_with_grads, kappa(K_ZZ + jitter I)) of a case: computed once, shared, never modified"""
    p = problem(case)
    out = interp_with_grads(case.kind, case.table, jitter, p.Z, p.X, p.ell, p.oscale, p.G)
    K, _ = make_kernel(case.kind, p.ell, p.oscale, case.table)
    return out, kappa(K(p.Z, p.Z) + jitter * torch.eye(case.m, dtype=torch.float64))


@functools.lru_cache(maxsize=None)
def interp_e32(case, jitter):
    p = problem(case)
    return fp32_dense_error(functools.partial(interp_with_grads, case.kind, case.table, jitter), (p.Z, p.X, p.ell, p.oscale, p.G))


@functools.lru_cache(maxsize=None)
def kl_reference(case, jitter=PRIOR_JITTER):
    p = problem(case)
    out = kl_with_grads(case.kind, case.table, jitter, p.Z, p.ell, p.oscale, p.mvar, p.Ls, p.gk)
    K, _ = make_kernel(case.kind, p.ell, p.oscale, case.table)
    return out, kappa(K(p.Z, p.Z) + jitter * torch.eye(case.m, dtype=torch.float64))


@functools.lru_cache(maxsize=None)
def kl_e32(case, jitter=PRIOR_JITTER):
    p = problem(case)
    return fp32_dense_error(functools.partial(kl_with_grads, case.kind, case.table, jitter), (p.Z, p.ell, p.oscale, p.mvar, p.Ls, p.gk))


@functools.lru_cache(maxsize=None)
def spd_problem(m, q, s):
    """M = I + A A^T / s (q, m, m) from the reference A of the base case at m inducing points, r (q, m), R (q, m, 130), cotangents; fp32
    values.  -> namespace with kappa(M)"""
    case = BASE._replace(m=m, q=q)
    A = interp_reference(case, 0.0)[0][0]
    M = r32(woodbury_matrix(A, s))
    M = 0.5 * (M + M.transpose(-1, -2))
    g = torch.Generator().manual_seed(7 * m + q)
    randn = lambda *sh: r32(torch.randn(*sh, generator=g, dtype=torch.float64))
    return SimpleNamespace(M=M, r=randn(q, m), gq=randn(q), gl=randn(q), R=randn(q, m, 130), kappa=kappa(M))


# ------------------------------------------------------------------------------------------------ whole SGPR models (test_gpu_sgpr_sizes.py)
SGPR_RAW_NOISE = -2.0                        # noise = softplus(-2) + 1e-4 = 0.127
SGPR_MODEL_BASES = {"RBFKernel": Case("rbf", 8, 500, 600, 1, False, 0.70), "MaternKernel": Case("matern52", 3, 500, 600, 1, False, 0.15)}
SGPR_MODEL_CASES = [SGPR_MODEL_BASES[k]._replace(m=m, oscale=o) for k in ("RBFKernel", "MaternKernel") for m in (129, 500) for o in (False, True)]


def sgpr_model_inputs(case):
    """(X, y (1,n), Xs, Z, raw_lengthscale (1,d), raw_outputscale (1) | None, raw_noise (1)) of an ExactGPModel(n_inducing_points=m) at
    `case`: the RAW parameters (softplus constraint, noise lower bound 1e-4), rounded to fp32"""
    p = problem(case)
    raw_os = None if p.oscale is None else r32(gm.inv_softplus(p.oscale))
    return p.X, p.y, p.Xs, p.Z, r32(gm.inv_softplus(p.ell)), raw_os, torch.full((1,), SGPR_RAW_NOISE, dtype=torch.float64)


def sgpr_model_outputs(kind, X, y, Xs, Z, raw_ls, raw_os, raw_nz):
    """(mll, gZ, g raw_lengthscale, g raw_outputscale | None, g raw_noise, mean (1,ns), cov (1,ns,ns)): the Titsias MLL / n with the
    added trace term, its gradients by autograd, and the eval-mode posterior, from oracle/sgpr.py; any floating element type"""
    okind, nu = KINDS[kind]
    Z, raw_ls, raw_os, raw_nz = _leaves(Z, raw_ls, raw_os, raw_nz)
    ell, nz = gm.softplus(raw_ls), gm.softplus(raw_nz) + 1e-4
    osc = None if raw_os is None else gm.softplus(raw_os)
    mll = sgpr_value_ref(kind, X, Z, ell, osc, nz, y).sum() / X.shape[0]
    grads = _grads(mll, [Z, raw_ls, raw_os, raw_nz])
    with torch.no_grad():
        mu, cov = osg.sgpr_posterior(okind, X, Z, ell, nz, y, Xs, nu, osc)
    return (mll.detach(),) + tuple(grads) + (mu, cov)


def sgpr_kappa(kind, X, Z, ell, oscale, noise):
    """the larger of kappa(K_ZZ) and kappa(B), B = I + A A^T / s: the two matrices the SGPR path factorises"""
    K, _ = make_kernel(kind, ell, oscale)
    A = whitened_interp_ref(K, Z, X, 0.0)
    return max(kappa(K(Z, Z)), kappa(woodbury_matrix(A, noise)))


@functools.lru_cache(maxsize=None)
def sgpr_model_reference(case):
    """(fp64 outputs, kappa, E32 per output) of a whole-model case: computed once, shared, never modified"""
    ins = sgpr_model_inputs(case)
    fn = functools.partial(sgpr_model_outputs, case.kind)
    X, y, Xs, Z, raw_ls, raw_os, raw_nz = ins
    kap = sgpr_kappa(case.kind, X, Z, gm.softplus(raw_ls), None if raw_os is None else gm.softplus(raw_os), gm.softplus(raw_nz) + 1e-4)
    return fn(*ins), kap, fp32_dense_error(fn, ins)
