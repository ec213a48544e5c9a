"""Dense fp64 reference of a sum of different kernel families,
    K_i = sum_g os[i][g] k_{member g}(x, x'; table[i][g]),
written from the members' formulas with torch on the CPU (autograd gives the gradients): the kernel, the log-prob, the leave-one-out value
and conditioning.  Members: "rbf", "matern12", "matern32", "matern52" (ARD, on r = |(x - x') / ell|), "periodic", "rq",
"locally_periodic" (the formulas of _periodic_dense, _rq_dense, _lper_dense).  The table is (q, G, 3 d + 1), one record
[ell | period | rbf_ell: d each | alpha] per member; a member reads only the slots it owns, so the others may hold NaN.  An owned
lengthscale of +inf switches that dimension off: tau / inf = 0 and s^2 / inf = 0 exactly, and autograd gives that slot gradient 0.
Imports nothing from the package under test."""
import math

import torch

from _lper_dense import lper_kernel
from _periodic_dense import per_kernel
from _rq_dense import rq_kernel

U32 = 2.0 ** -24
ARD = ("rbf", "matern12", "matern32", "matern52")
MEMBERS = ARD + ("periodic", "rq", "locally_periodic")
# public member codes of the library (include/plmc.h, PLMC_FAM_*)
FAM = {"rbf": 0, "matern12": 1, "matern32": 2, "matern52": 3, "periodic": 16, "rq": 17, "locally_periodic": 18}


def owned(member, d):
    """Boolean mask (3 d + 1) of the record slots a member reads."""
    m = torch.zeros(3 * d + 1, dtype=torch.bool)
    m[:d] = True
    if member in ("periodic", "locally_periodic"):
        m[d:2 * d] = True
    if member == "locally_periodic":
        m[2 * d:3 * d] = True
    if member == "rq":
        m[3 * d] = True
    return m


def ard_kernel(kind, Xa, Xb, ell):
    """(q, na, nb), unit output scale."""
    df = (Xa[:, None, :] - Xb[None, :, :])[None] / ell[:, None, None, :]
    r2 = (df * df).sum(-1)
    if kind == "rbf":
        return torch.exp(-0.5 * r2)
    r = torch.sqrt(r2 + torch.finfo(r2.dtype).tiny)  # (autograd at r = 0; 1e-154 in r -- fp32: 1e-19 -- is far below every tolerance)
    if kind == "matern12":
        return torch.exp(-r)
    if kind == "matern32":
        s = math.sqrt(3.0) * r
        return (1.0 + s) * torch.exp(-s)
    s = math.sqrt(5.0) * r
    return (1.0 + s + 5.0 / 3.0 * r2) * torch.exp(-s)


def member_kernel(member, Xa, Xb, rec):
    """(q, na, nb), unit output scale, from the member's record rec (q, 3 d + 1)."""
    d = Xa.shape[1]
    ell, period, lam, alpha = rec[:, :d], rec[:, d:2 * d], rec[:, 2 * d:3 * d], rec[:, 3 * d]
    if member in ARD:
        return ard_kernel(member, Xa, Xb, ell)
    if member == "periodic":
        return per_kernel(Xa, Xb, ell, period)
    if member == "rq":
        return rq_kernel(Xa, Xb, ell, alpha)
    if member == "locally_periodic":
        return lper_kernel(Xa, Xb, ell, period, lam)
    raise ValueError(member)


def sum_kernel(members, Xa, Xb, table, oscale=None):
    """(q, na, nb) from Xa (na, d), Xb (nb, d), table (q, G, 3 d + 1), oscale (q, G) | None; components added in table order."""
    K = None
    for g, mem in enumerate(members):
        Kg = member_kernel(mem, Xa, Xb, table[:, g])
        if oscale is not None:
            Kg = oscale[:, g, None, None] * Kg
        K = Kg if K is None else K + Kg
    return K


def khat(members, X, table, oscale, noise):
    return sum_kernel(members, X, X, table, oscale) + noise[:, None, None] * torch.eye(X.shape[0], dtype=X.dtype)


def sum_logprob(members, X, y, table, oscale, noise):
    """log N(y_i; 0, K_i + noise_i I) per latent, (q,)."""
    n = X.shape[0]
    L = torch.linalg.cholesky(khat(members, X, table, oscale, noise))
    z = torch.linalg.solve_triangular(L, y.unsqueeze(-1), upper=False).squeeze(-1)
    return -0.5 * (z ** 2).sum(-1) - torch.log(torch.diagonal(L, dim1=-2, dim2=-1)).sum(-1) - 0.5 * n * math.log(2.0 * math.pi)


def sum_loo(members, X, y, table, oscale, noise):
    """Leave-one-out log predictive density per latent, (q,) (Rasmussen & Williams 5.4.2)."""
    n = X.shape[0]
    P = torch.linalg.inv(khat(members, X, table, oscale, noise))
    P = 0.5 * (P + P.transpose(-1, -2))
    alpha = (P @ y.unsqueeze(-1)).squeeze(-1)
    p = torch.diagonal(P, dim1=-2, dim2=-1)
    return (0.5 * p.log() - 0.5 * alpha * alpha / p).sum(-1) - 0.5 * n * math.log(2.0 * math.pi)


def sum_posterior(members, X, y, Xs, table, oscale, noise):
    """Posterior mean (q, ns) and covariance (q, ns, ns) of zero-mean GPs."""
    Ks = sum_kernel(members, X, Xs, table, oscale)
    L = torch.linalg.cholesky(khat(members, X, table, oscale, noise))
    V = torch.linalg.solve_triangular(L, Ks, upper=False)
    z = torch.linalg.solve_triangular(L, y.unsqueeze(-1), upper=False)
    return (V.transpose(-1, -2) @ z).squeeze(-1), sum_kernel(members, Xs, Xs, table, oscale) - V.transpose(-1, -2) @ V


def grads(fn, members, X, y, table, oscale, noise):
    """Value (q,) and the gradient table (q, G (3 d + 1) + 1 + G) = [d table | d noise | d oscale] of fn = sum_logprob / sum_loo; the
    slots a member does not own come out as exactly 0 (they never enter the graph; their NaN is replaced before autograd sees it)."""
    q, G, rec = table.shape
    d = (rec - 1) // 3
    mask = torch.stack([owned(m, d) for m in members])[None].expand(q, G, rec)
    t = torch.where(mask, table, torch.ones_like(table)).clone().requires_grad_(True)
    os_ = (torch.ones(q, G, dtype=table.dtype) if oscale is None else oscale).clone().requires_grad_(True)
    nz = noise.clone().requires_grad_(True)
    val = fn(members, X, y, t, os_, nz)
    gt, go, gn = torch.autograd.grad(val.sum(), (t, os_, nz))
    gt = torch.where(mask, gt, torch.zeros_like(gt))
    return val.detach(), torch.cat([gt.reshape(q, -1), gn[:, None], go], 1)


def make_table(members, d, q, seed, off=None, dtype=torch.float64):
    """A table (q, G, 3 d + 1) with different parameters per latent and member, NaN in every slot its member does not own: lengthscales
    in [0.7, 1.7], periods in [1.5, 3.5], RBF lengthscales in [2, 4], alpha in [0.8, 2.8]; output scales (q, G) in [0.3, 0.8] / ... so
    that their sum is of order 1.  `off`: {g: [dims]} owned lengthscale slots of member g set to +inf (switched-off dimensions)."""
    g_ = torch.Generator().manual_seed(seed)
    G = len(members)
    u = torch.rand(q, G, 3 * d + 1, generator=g_, dtype=torch.float64)
    t = torch.empty_like(u)
    t[..., :d] = 0.7 + u[..., :d]
    t[..., d:2 * d] = 1.5 + 2.0 * u[..., d:2 * d]
    t[..., 2 * d:3 * d] = 2.0 + 2.0 * u[..., 2 * d:3 * d]
    t[..., 3 * d] = 0.8 + 2.0 * u[..., 3 * d]
    for g, m in enumerate(members):
        t[:, g, ~owned(m, d)] = float("nan")
    for g, dims in (off or {}).items():
        for k in dims:
            t[:, g, k] = float("inf")
            if members[g] == "locally_periodic":
                t[:, g, 2 * d + k] = float("inf")
    os_ = (0.3 + 0.5 * torch.rand(q, G, generator=g_, dtype=torch.float64)) * (2.0 / G)
    return t.to(dtype), os_.to(dtype)


def fp32_bound(members, d, table, oscale):
    """(q, 1, 1): per-element bound of the fp32 assembly against the fp64 formula at the fp32 inputs -- the sum of the members' bounds,
    each times its output scale, plus (G - 1) 2^-24 sum_g os_g for the additions:
      periodic           24 d (1 + 1 / min_k ell_k) 2^-24                      
      rq                 (d + 8) 2^-24                                          
      locally periodic   [24 d (1 + 1 / min_k ell_k) + d + 8] 2^-24             
      ARD kinds          6e-7, the per-entry tolerance tests/test_gpu_engine.py applies to the same kinds (relative to 1 + noise there; the
                         value of a unit-scale member is at most 1)
    A switched-off dimension (ell = +inf) does not enter min_k ell_k."""
    q = table.shape[0]
    tot = torch.zeros(q, dtype=torch.float64)
    for g, m in enumerate(members):
        os_g = oscale[:, g].double()
        ell_min = table[:, g, :d].double().min(-1)[0]
        if m in ARD:
            b = torch.full((q,), 6e-7, dtype=torch.float64)
        elif m == "periodic":
            b = 24 * d * (1.0 + 1.0 / ell_min) * U32
        elif m == "rq":
            b = torch.full((q,), (d + 8) * U32, dtype=torch.float64)
        else:
            b = (24 * d * (1.0 + 1.0 / ell_min) + (d + 8)) * U32
        tot = tot + os_g * b
    tot = tot + (len(members) - 1) * U32 * oscale.double().sum(-1)
    return tot[:, None, None]


def fp32_problem(members, d, n=257, q=3, seed=77):
    """The problem of the fp32 tests, rounded to fp32 and returned as fp64: X (n, d) uniform on [0, 10]^d, y (q, n) a draw from the prior,
    the table of make_table as it stands at every d (lengthscales in [0.7, 1.7], periods in [1.5, 3.5], RBF lengthscales in [2, 4]), output
    scales summing to order 1, noise in [0.05, 0.2]."""
    g = torch.Generator().manual_seed(seed + d)
    X = 10.0 * torch.rand(n, d, generator=g, dtype=torch.float64)
    table, os_ = make_table(members, d, q, seed + 10 * d)
    noise = 0.05 + 0.15 * torch.rand(q, generator=g, dtype=torch.float64)
    X, table, os_, noise = (t.float().double() for t in (X, table, os_, noise))
    L = torch.linalg.cholesky(khat(members, X, table, os_, noise))
    y = (L @ torch.randn(q, n, 1, generator=g, dtype=torch.float64)).squeeze(-1).float().double()
    return X, y, table, os_, noise
