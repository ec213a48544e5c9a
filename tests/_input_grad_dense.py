"""Dense fp64 reference of the input gradient of the exact log density, for a dense-kernel CALLABLE K(Xa, Xb) -> (q, na, nb):
    gX[l, i, k] = sum_{j != i} (alpha_li alpha_lj - P_lij) d k_l(x_i, x_j) / d x_i[k]
-- no factor 1/2, x_i enters row i and column i of Khat -- and the families' problems the tests share.  TEST INFRASTRUCTURE ONLY: plain
torch on the CPU, nothing from the package.  The callables are oracle.gp_math.kernel_matrix, _inducing_dense.additive_kernel and the
kernels of _sm_dense, _periodic_dense, _rq_dense and _lper_dense."""
import math

import torch

import _inducing_dense as idn
import _lper_dense
import _periodic_dense
import _rq_dense
import _sm_dense
from oracle import gp_math as gm

NB = 128
STATIONARY = {"rbf": ("rbf", 2.5), "matern12": ("matern", 0.5), "matern32": ("matern", 1.5), "matern52": ("matern", 2.5)}
DISJOINT, OVERLAP = [[0, 1], [2, 3, 4]], [[0, 1], [1, 2]]            # the groups of test_gpu_kernel_vjp_add.py; OVERLAP leaves 3 and 4 unused
FAMILIES = tuple(STATIONARY) + ("add_disjoint", "add_overlap", "rq", "periodic", "locally_periodic", "sm1", "sm3", "sm8")


def input_grad_ref(K, X, P, alpha):
    """(gX, terms), both (q, n, d) fp64: the values by autograd of sum_ij Omega_lij K_l(X, X')[i, j] with respect to the FIRST argument
    (Omega = alpha alpha^T - P with its diagonal set to 0; the second argument is held constant), and the sums of absolute terms
    sum_j |Omega_lij d k_l(x_i, x_j) / d x_ik| behind each value, the pair derivatives from one forward-mode pass per dimension (K_ij
    depends on row i of the first argument only, so the tangent of K along e_k in every row is d k(x_i, x_j) / d x_ik)."""
    q, (n, d) = P.shape[0], X.shape
    Om = alpha[:, :, None] * alpha[:, None, :] - P
    Om = Om * (1.0 - torch.eye(n, dtype=Om.dtype))
    Xb = X.detach()
    gX = torch.empty(q, n, d, dtype=torch.float64)
    for lat in range(q):
        Xa = X.detach().clone().requires_grad_(True)
        gX[lat], = torch.autograd.grad((Om[lat] * K(Xa, Xb)[lat]).sum(), Xa)
    terms = torch.empty(q, n, d, dtype=torch.float64)
    for k in range(d):
        e = torch.zeros(n, d, dtype=torch.float64)
        e[:, k] = 1.0
        dK = torch.func.jvp(lambda Xa: K(Xa, Xb), (Xb.clone(),), (e,))[1]
        terms[:, :, k] = (Om.abs() * dK.abs()).sum(-1)
    return gX, terms


def mll_input_grad(K, X, noise, y):
    """d sum_l log N(y_l; 0, K_l(X, X) + noise_l I) / dX per latent, (q, n, d), by autograd of the dense Cholesky log density."""
    q, n = y.shape
    out = torch.empty(q, *X.shape, dtype=torch.float64)
    for lat in range(q):
        Xa = X.detach().clone().requires_grad_(True)
        Kh = K(Xa, Xa)[lat] + noise[lat] * torch.eye(n, dtype=torch.float64)
        out[lat], = torch.autograd.grad(gm.mvn_log_prob(Kh, y[lat]), Xa)
    return out


class Problem:
    """One family's table: `kind`, `ell`, `oscale` as projectedlmc._engine takes them (fp64, CPU), the dense callable `K` of the same
    values, and `zero` (d) bool: the dimensions whose gradient is exactly 0 (unused by every component; sm: scale = mean = 0)."""


def _f32(t):
    return None if t is None else t.float().double()


def problem(family, d, q, seed, use_os=True, groups=None, add_kind="matern52"):
    """Random hyper-parameters of `family` on d dimensions for q latents, rounded to fp32 so that both element types see the same values.
    Lengthscales ~ sqrt(d): the scaled distances of points in [-1, 1]^d stay O(1)."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    p = Problem()
    p.family, p.d, p.q = family, d, q
    p.zero = torch.zeros(d, dtype=torch.bool)
    sd = math.sqrt(d)
    osc = _f32(0.5 + rnd(q)) if use_os else None
    if family in STATIONARY:
        okind, nu = STATIONARY[family]
        ell = _f32(sd * (0.3 + 0.5 * rnd(q, d)))
        p.kind, p.ell, p.oscale = family, ell, osc
        p.K = lambda Xa, Xb: gm.kernel_matrix(okind, Xa, Xb, ell, osc, nu)
    elif family.startswith("add_"):
        kind = add_kind
        groups = {"add_disjoint": DISJOINT, "add_overlap": OVERLAP}[family] if groups is None else groups
        okind, nu = STATIONARY[kind]
        ells = [_f32(math.sqrt(len(idx)) * (0.3 + 0.5 * rnd(q, len(idx)))) for idx in groups]
        oss = [(_f32(0.5 + rnd(q)) if use_os else None) for _ in groups]
        p.kind = kind
        p.ell, p.oscale = idn.component_table(groups, ells, oss, d)
        p.K = idn.additive_kernel(okind, nu, groups, ells, oss)
        p.zero = torch.isinf(p.ell).all(dim=(0, 1))
    elif family == "rq":
        ell, a = _f32(sd * (0.3 + 0.5 * rnd(q, d))), _f32(0.5 + 2.0 * rnd(q))
        p.kind, p.ell, p.oscale = "rq", torch.cat([ell, a[:, None]], 1), osc
        p.K = lambda Xa, Xb: _rq_dense.rq_kernel(Xa, Xb, ell, a, osc)
    elif family == "periodic":
        ell, per = _f32(d * (0.5 + rnd(q, d))), _f32(0.7 + rnd(q, d))
        p.kind, p.ell, p.oscale = "periodic", torch.stack([ell, per], 1), osc
        p.K = lambda Xa, Xb: _periodic_dense.per_kernel(Xa, Xb, ell, per, osc)
    elif family == "locally_periodic":
        ell, per, lam = _f32(d * (0.5 + rnd(q, d))), _f32(0.7 + rnd(q, d)), _f32(sd * (0.5 + rnd(q, d)))
        p.kind, p.ell, p.oscale = "locally_periodic", torch.stack([ell, per, lam], 1), osc
        p.K = lambda Xa, Xb: _lper_dense.lper_kernel(Xa, Xb, ell, per, lam, osc)
    elif family.startswith("sm"):
        M = int(family[2:])
        sc, mu = _f32((0.05 + 0.25 * rnd(q, M, d)) / sd), _f32(0.1 + 1.5 * rnd(q, M, d))
        if d > 1:                                   # a dimension the mixture ignores: scale = mean = 0
            sc[:, :, d - 1], mu[:, :, d - 1] = 0.0, 0.0
            p.zero[d - 1] = True
        w = _f32(0.2 + rnd(q, M)) if use_os else None
        p.kind, p.ell, p.oscale = "sm", torch.stack([sc, mu], 1), w
        wt = torch.ones(q, M, dtype=torch.float64) if w is None else w
        p.K = lambda Xa, Xb: _sm_dense.sm_kernel(Xa, Xb, sc, mu, wt)
    else:
        raise ValueError(family)
    return p


def inputs(n, d, seed, coincident=False):
    g = torch.Generator().manual_seed(seed + 1000)
    X = _f32(2 * torch.rand(n, d, generator=g, dtype=torch.float64) - 1)
    if coincident and n > 2:
        X[n - 1] = X[1]
    return X


def random_operands(n, q, seed):
    """A random symmetric P (q, n, n) and alpha (q, n), fp32-representable."""
    g = torch.Generator().manual_seed(seed + 2000)
    P = torch.randn(q, n, n, generator=g, dtype=torch.float64)
    P = _f32(0.5 * (P + P.transpose(1, 2)))
    P = torch.triu(P) + torch.triu(P, 1).transpose(1, 2)          # symmetric after the rounding too
    return P, _f32(torch.randn(q, n, generator=g, dtype=torch.float64))


def nan_buffers(P, alpha, dtype):
    """(Kinv (q, n_pad, n_pad + NB), alpha (q, n_pad)) of `dtype`: P in the elements the kernel may read -- j >= i, both below n -- and NaN
    everywhere else: below the diagonal, in the rows and columns of the padding, beyond n_pad, and in alpha from n on."""
    q, n = alpha.shape
    n_pad = (n + NB - 1) // NB * NB
    Kinv = torch.full((q, n_pad, n_pad + NB), float("nan"), dtype=dtype)
    up = torch.triu(torch.ones(n, n, dtype=torch.bool))
    Kinv[:, :n, :n] = torch.where(up, P.to(dtype), torch.full((), float("nan"), dtype=dtype))
    a = torch.full((q, n_pad), float("nan"), dtype=dtype)
    a[:, :n] = alpha.to(dtype)
    return Kinv, a
