"""Dense fp64 reference of the locally periodic kernel (periodic x RBF), written from the formula [gpytorch-knowledge: ProductKernel of
PeriodicKernel and RBFKernel, unverified offline]
    k(x, x') = os exp(-2 sum_k sin^2(pi tau_k / p_k) / ell_k - 1/2 sum_k (tau_k / lam_k)^2),   tau = x - x'
(ell the periodic lengthscale, not squared; p the period; lam the RBF lengthscale) with torch on the CPU (autograd gives the
gradients): the kernel, the log-prob, the leave-one-out value and conditioning.  Imports nothing from the package under test."""
import math

import torch

U32 = 2.0 ** -24


def lper_kernel(Xa, Xb, ell, period, lam, oscale=None):
    """(q, na, nb) from Xa (na, d), Xb (nb, d), ell / period / lam (q, d), oscale (q) | None."""
    tau = (Xa[:, None, :] - Xb[None, :, :])[None]                             # (1, na, nb, d)
    s = torch.sin(math.pi * tau / period[:, None, None, :])
    r = tau / lam[:, None, None, :]
    K = torch.exp(-2.0 * (s * s / ell[:, None, None, :]).sum(-1) - 0.5 * (r * r).sum(-1))
    return K if oscale is None else oscale[:, None, None] * K


def khat(X, ell, period, lam, oscale, noise):
    return lper_kernel(X, X, ell, period, lam, oscale) + noise[:, None, None] * torch.eye(X.shape[0], dtype=X.dtype)


def lper_logprob(X, y, ell, period, lam, oscale, noise):
    """log N(y_i; 0, K_i + noise_i I) per latent, (q,)."""
    n = X.shape[0]
    L = torch.linalg.cholesky(khat(X, ell, period, lam, oscale, noise))
    z = torch.linalg.solve_triangular(L, y.unsqueeze(-1), upper=False).squeeze(-1)
    return -0.5 * (z ** 2).sum(-1) - torch.log(torch.diagonal(L, dim1=-2, dim2=-1)).sum(-1) - 0.5 * n * math.log(2.0 * math.pi)


def lper_loo(X, y, ell, period, lam, oscale, noise):
    """Leave-one-out log predictive density per latent, (q,): sum_i [1/2 log p_i - 1/2 alpha_i^2 / p_i] - n/2 log 2 pi with
    P = Khat^-1, p = diag P, alpha = P y (Rasmussen & Williams 5.4.2)."""
    n = X.shape[0]
    P = torch.linalg.inv(khat(X, ell, period, lam, oscale, noise))
    P = 0.5 * (P + P.transpose(-1, -2))
    alpha = (P @ y.unsqueeze(-1)).squeeze(-1)
    p = torch.diagonal(P, dim1=-2, dim2=-1)
    return (0.5 * p.log() - 0.5 * alpha * alpha / p).sum(-1) - 0.5 * n * math.log(2.0 * math.pi)


def lper_posterior(X, y, Xs, ell, period, lam, oscale, noise):
    """Posterior mean (q, ns) and covariance (q, ns, ns) of zero-mean GPs."""
    Ks = lper_kernel(X, Xs, ell, period, lam, oscale)
    L = torch.linalg.cholesky(khat(X, ell, period, lam, oscale, noise))
    V = torch.linalg.solve_triangular(L, Ks, upper=False)
    z = torch.linalg.solve_triangular(L, y.unsqueeze(-1), upper=False)
    return (V.transpose(-1, -2) @ z).squeeze(-1), lper_kernel(Xs, Xs, ell, period, lam, oscale) - V.transpose(-1, -2) @ V


def fp32_bound(d, ell, os_):
    """(q, 1, 1): the per-element bound of the fp32 assembly ("Locally periodic kernel: fp32 numerics"),
    24 d 2^-24 os (1 + 1 / min_k ell_k) for the periodic exponent + (d + 8) 2^-24 os for the RBF exponent, the sum and the exponential."""
    return ((24 * d * (1.0 + 1.0 / ell.min(-1)[0]) + (d + 8)) * U32 * os_)[:, None, None]


def naive_fp32(Xa, Xb, ell, period, lam, os_):
    """The naive restatement, all in torch float32 on the CPU: os exp(-2 sin(pi (tau / p))^2 / ell - (tau / lam)^2 / 2), d = 1, q = 1."""
    Xf, Xg, lf, pf, rf, of = (t.float() for t in (Xa, Xb, ell, period, lam, os_))
    tau = Xf[:, None, 0] - Xg[None, :, 0]
    s = torch.sin(math.pi * (tau / pf[0, 0]))
    r = tau / rf[0, 0]
    return of[0] * torch.exp(-2.0 * s * s / lf[0, 0] - 0.5 * r * r)
