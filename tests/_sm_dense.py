"""Dense fp64 reference of the spectral-mixture kernel, written from the formula
    k(x, x') = sum_m w_m exp(-2 pi^2 sum_k s_mk^2 tau_k^2) prod_k cos(2 pi mu_mk tau_k),   tau = x - x'
with torch on the CPU (autograd gives the gradients).  Imports nothing from the package under test."""
import math

import torch


def sm_kernel(Xa, Xb, scales, means, weights):
    """(q, na, nb) from Xa (na, d), Xb (nb, d), scales / means (q, M, d), weights (q, M)."""
    tau = (Xa[:, None, :] - Xb[None, :, :])[None, None]                       # (1, 1, na, nb, d)
    s, mu = scales[:, :, None, None, :], means[:, :, None, None, :]
    env = torch.exp(-2.0 * math.pi ** 2 * ((s * tau) ** 2).sum(-1))
    car = torch.cos(2.0 * math.pi * mu * tau).prod(-1)
    return (weights[:, :, None, None] * env * car).sum(1)


def sm_logprob(X, y, scales, means, weights, noise):
    """log N(y_i; 0, K_i + noise_i I) per latent, (q,)."""
    n = X.shape[0]
    K = sm_kernel(X, X, scales, means, weights) + noise[:, None, None] * torch.eye(n, dtype=X.dtype)
    L = torch.linalg.cholesky(K)
    z = torch.linalg.solve_triangular(L, y.unsqueeze(-1), upper=False).squeeze(-1)
    return -0.5 * (z ** 2).sum(-1) - torch.log(torch.diagonal(L, dim1=-2, dim2=-1)).sum(-1) - 0.5 * n * math.log(2.0 * math.pi)


def sm_posterior(X, y, Xs, scales, means, weights, noise):
    """Posterior mean (q, ns) and covariance (q, ns, ns) of zero-mean GPs."""
    n = X.shape[0]
    K = sm_kernel(X, X, scales, means, weights) + noise[:, None, None] * torch.eye(n, dtype=X.dtype)
    Ks = sm_kernel(X, Xs, scales, means, weights)
    L = torch.linalg.cholesky(K)
    V = torch.linalg.solve_triangular(L, Ks, upper=False)
    z = torch.linalg.solve_triangular(L, y.unsqueeze(-1), upper=False)
    return (V.transpose(-1, -2) @ z).squeeze(-1), sm_kernel(Xs, Xs, scales, means, weights) - V.transpose(-1, -2) @ V
