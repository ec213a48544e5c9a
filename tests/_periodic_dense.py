"""Dense fp64 reference of the periodic kernel, written from the formula [gpytorch-knowledge: PeriodicKernel.forward, v1.11, unverified
offline]
    k(x, x') = os exp(-2 sum_k sin^2(pi (x_k - x'_k) / p_k) / ell_k)            (the lengthscale is not squared)
with torch on the CPU (autograd gives the gradients).  Imports nothing from the package under test."""
import math

import torch


def per_kernel(Xa, Xb, ell, period, oscale=None):
    """(q, na, nb) from Xa (na, d), Xb (nb, d), ell / period (q, d), oscale (q) | None."""
    tau = (Xa[:, None, :] - Xb[None, :, :])[None]                             # (1, na, nb, d)
    s = torch.sin(math.pi * tau / period[:, None, None, :])
    K = torch.exp(-2.0 * (s * s / ell[:, None, None, :]).sum(-1))
    return K if oscale is None else oscale[:, None, None] * K


def _khat(X, ell, period, oscale, noise):
    return per_kernel(X, X, ell, period, oscale) + noise[:, None, None] * torch.eye(X.shape[0], dtype=X.dtype)


def per_logprob(X, y, ell, period, oscale, noise):
    """log N(y_i; 0, K_i + noise_i I) per latent, (q,)."""
    n = X.shape[0]
    L = torch.linalg.cholesky(_khat(X, ell, period, oscale, noise))
    z = torch.linalg.solve_triangular(L, y.unsqueeze(-1), upper=False).squeeze(-1)
    return -0.5 * (z ** 2).sum(-1) - torch.log(torch.diagonal(L, dim1=-2, dim2=-1)).sum(-1) - 0.5 * n * math.log(2.0 * math.pi)


def per_posterior(X, y, Xs, ell, period, oscale, noise):
    """Posterior mean (q, ns) and covariance (q, ns, ns) of zero-mean GPs."""
    Ks = per_kernel(X, Xs, ell, period, oscale)
    L = torch.linalg.cholesky(_khat(X, ell, period, oscale, noise))
    V = torch.linalg.solve_triangular(L, Ks, upper=False)
    z = torch.linalg.solve_triangular(L, y.unsqueeze(-1), upper=False)
    return (V.transpose(-1, -2) @ z).squeeze(-1), per_kernel(Xs, Xs, ell, period, oscale) - V.transpose(-1, -2) @ V
