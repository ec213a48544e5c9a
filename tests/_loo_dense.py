"""Dense fp64 reference of the leave-one-out objective, written from the formulas with torch on the CPU (autograd gives the
gradients).  With P = Khat^-1, alpha = P y, p = diag P:
    L = sum_i [1/2 log p_i - 1/2 alpha_i^2 / p_i] - n/2 log 2 pi                       (Rasmussen & Williams 5.4.2)
    dL/dy = u = P g,  g = -alpha / p,  c = 1/2 / p + 1/2 alpha^2 / p^2,
    dL/dKhat = G = -[P diag(c) P + 1/2 (alpha u^T + u alpha^T)].
Khat is built with the helpers the family tests use (oracle.gp_math, _sm_dense, _periodic_dense).  Imports nothing from the package
under test."""
import math

import torch

import _periodic_dense as pd
import _sm_dense as smd
from oracle import gp_math as gm

KINDS = {"rbf": ("rbf", 2.5), "matern12": ("matern", 0.5), "matern32": ("matern", 1.5), "matern52": ("matern", 2.5), "spline": ("spline", 2.5)}


def loo_log_prob(Khat, y):
    """(q,) from Khat (q, n, n), y (q, n)."""
    n = y.shape[-1]
    P = torch.linalg.inv(Khat)
    P = 0.5 * (P + P.transpose(-1, -2))
    alpha = (P @ y.unsqueeze(-1)).squeeze(-1)
    p = torch.diagonal(P, dim1=-2, dim2=-1)
    return (0.5 * p.log() - 0.5 * alpha * alpha / p).sum(-1) - 0.5 * n * math.log(2.0 * math.pi)


def loo_brute_force(Khat, y):
    """The same number from n refitted GPs per latent, each without point i: sum_i log N(y_i; mu_-i, s2_-i)."""
    q, n = y.shape
    out = torch.zeros(q, dtype=Khat.dtype)
    for a in range(q):
        for i in range(n):
            keep = [j for j in range(n) if j != i]
            Kr, kr = Khat[a][keep][:, keep], Khat[a][keep, i]
            sol = torch.linalg.solve(Kr, torch.stack([y[a, keep], kr], 1))
            mu, s2 = kr @ sol[:, 0], Khat[a, i, i] - kr @ sol[:, 1]
            out[a] += -0.5 * torch.log(s2) - 0.5 * (y[a, i] - mu) ** 2 / s2 - 0.5 * math.log(2.0 * math.pi)
    return out


def loo_adjoint(Khat, y):
    """dict(P, alpha, p, c, g, u, G) of the formulas above, batched."""
    P = torch.linalg.inv(Khat)
    P = 0.5 * (P + P.transpose(-1, -2))
    alpha = (P @ y.unsqueeze(-1)).squeeze(-1)
    p = torch.diagonal(P, dim1=-2, dim2=-1)
    c = 0.5 / p + 0.5 * alpha * alpha / (p * p)
    g = -alpha / p
    u = (P @ g.unsqueeze(-1)).squeeze(-1)
    au = alpha.unsqueeze(-1) * u.unsqueeze(-2)
    G = -(P @ (c.unsqueeze(-1) * P) + 0.5 * (au + au.transpose(-1, -2)))
    return dict(P=P, alpha=alpha, p=p, c=c, g=g, u=u, G=G)


# ---- the covariance families of the batched exact engine: problem = dict(kind, X, y, noise, ell, osc, dense), where (kind, ell, osc) are
# what _engine takes (ell: the family's table) and dense(ell, osc) -> K (q, n, n) without the noise, differentiable in both.
def _groups(d, G):
    w = min(d, (d + 1) // 2 + 1)
    return [sorted({(g * max(1, d // G) + k) % d for k in range(w)}) for g in range(G)]


def problem(family, n, q, seed, d=3, kind="matern52", G=2, M=2, noise_lo=0.05, noise_hi=0.2, fp32=False):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    y = torch.randn(q, n, generator=g, dtype=torch.float64)
    noise = noise_lo + (noise_hi - noise_lo) * r(q)
    if family == "plain":
        okind, nu = KINDS[kind]
        X = r(n, d) if kind == "spline" else 2 * r(n, d) - 1
        ell = math.sqrt(d) * (0.3 + 0.5 * r(q, d))
        if kind == "spline":                 # no lengthscale: the engine's table holds ones (kernels.SplineKernel) and gets no gradient
            ell = torch.ones(q, d, dtype=torch.float64)
        osc = 0.5 + r(q)
        dense = lambda ell, osc: gm.kernel_matrix(okind, X, X, ell, osc, nu)
    elif family == "additive":
        okind, nu = KINDS[kind]
        X = 2 * r(n, d) - 1
        groups = _groups(d, G)
        ell = torch.full((q, G, d), float("inf"), dtype=torch.float64)
        for gi, idx in enumerate(groups):
            ell[:, gi, idx] = math.sqrt(len(idx)) * (0.3 + 0.5 * r(q, len(idx)))
        osc = 0.5 + r(q, G)
        dense = lambda ell, osc: sum(gm.kernel_matrix(okind, X[:, idx], X[:, idx], ell[:, gi, idx], osc[:, gi], nu)
                                     for gi, idx in enumerate(groups))
    elif family == "sm":
        kind = "sm"
        X = r(n, d)
        ell = torch.stack([0.5 + 1.5 * r(q, M, d), 0.2 + 1.5 * r(q, M, d)], 1)          # (q, 2, M, d) = [scales | means]
        osc = (0.3 + r(q, M)) / M
        dense = lambda ell, osc: smd.sm_kernel(X, X, ell[:, 0], ell[:, 1], osc)
    elif family == "periodic":
        kind = "periodic"
        X = r(n, d)
        ell = torch.stack([(0.6 + 1.4 * r(q, d)) * d, 0.3 + 1.2 * r(q, d)], 1)          # (q, 2, d) = [lengthscales | periods]
        osc = 0.5 + r(q)
        dense = lambda ell, osc: pd.per_kernel(X, X, ell[:, 0], ell[:, 1], osc)
    else:
        raise ValueError(family)
    prob = dict(family=family, kind=kind, X=X, y=y, noise=noise, ell=ell, osc=osc)
    if fp32:                                 # every input exactly representable in fp32: the reference sees what the device sees
        for k in ("X", "y", "noise", "ell", "osc"):
            prob[k] = prob[k].float().double()
        X = prob["X"]
    prob["dense"] = dense
    return prob


def khat(prob, ell=None, osc=None, noise=None):
    ell = prob["ell"] if ell is None else ell
    osc = prob["osc"] if osc is None else osc
    noise = prob["noise"] if noise is None else noise
    n = prob["X"].shape[0]
    return prob["dense"](ell, osc) + noise.reshape(-1, 1, 1) * torch.eye(n, dtype=torch.float64)


def reference(prob, objective=loo_log_prob, weights=None):
    """(value (q), dict of gradients of sum_i w_i value_i w.r.t. ell / osc / noise / y) by fp64 autograd through the dense matrix."""
    leaves = {k: prob[k].clone().requires_grad_(True) for k in ("ell", "osc", "noise", "y")}
    val = objective(khat(prob, leaves["ell"], leaves["osc"], leaves["noise"]), leaves["y"])
    w = torch.ones_like(val) if weights is None else weights
    (val * w).sum().backward()
    grads = {k: (torch.zeros_like(v) if v.grad is None else torch.nan_to_num(v.grad, nan=0.0)) for k, v in leaves.items()}
    return val.detach(), grads


def abs_scales(prob, A):
    """S_theta = sum_ij |A_ij| |dKhat_ij / dtheta| for every hyper-parameter of every latent (A: (q, n, n), the adjoint of Khat):
    dict(ell, osc, noise) shaped like the parameters.  dKhat / dtheta per element by the double-backward identity
    d/dW [d/dtheta sum(K o W)] = dK / dtheta; latents are independent, so one pass per slot serves all q."""
    ell, osc = prob["ell"].clone().requires_grad_(True), prob["osc"].clone().requires_grad_(True)
    q = ell.shape[0]
    K = prob["dense"](ell, osc)
    W = torch.ones_like(K).requires_grad_(True)
    gl, go = torch.autograd.grad((K * W).sum(), (ell, osc), create_graph=True, allow_unused=True)
    out = {}
    for name, gt, par in (("ell", gl, ell), ("osc", go, osc)):
        S = torch.zeros_like(par)
        if gt is not None:
            flat, Sf = gt.reshape(q, -1), S.reshape(q, -1)
            for k in range(flat.shape[1]):
                if not flat[:, k].requires_grad:
                    continue
                (dK,) = torch.autograd.grad(flat[:, k].sum(), W, retain_graph=True, allow_unused=True)
                if dK is not None:
                    Sf[:, k] = (A.abs() * torch.nan_to_num(dK, nan=0.0).abs()).sum((-1, -2))
        out[name] = S.detach()
    out["noise"] = torch.diagonal(A, dim1=-2, dim2=-1).abs().sum(-1)
    return out
