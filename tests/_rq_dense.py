"""Dense fp64 reference of the rational-quadratic kernel, written from the formula [gpytorch-knowledge: RQKernel, unverified offline]
    k(x, x') = os (1 + r^2 / (2 alpha))^(-alpha),   r^2 = sum_k ((x_k - x'_k) / ell_k)^2,   alpha one scalar per latent
with torch on the CPU (autograd gives the gradients).  Imports nothing from the package under test.

Also the two fp32 restatements the tests compare against: the textbook form pow(1 + u, -alpha), which loses alpha 2^-24, and the
prescribed form exp(-alpha log1p(u)) with the difference taken from the raw inputs."""
import math

import torch

U32 = 2.0 ** -24


def rq_kernel(Xa, Xb, ell, alpha, oscale=None):
    """(q, na, nb) from Xa (na, d), Xb (nb, d), ell (q, d), alpha (q), oscale (q) | None.  exp(-alpha log1p(u)): in fp64 this is the
    formula to a few 2^-53 for every alpha, where pow(1 + u, -alpha) would already lose alpha 2^-53."""
    df = (Xa[:, None, :] - Xb[None, :, :])[None] / ell[:, None, None, :]           # (q, na, nb, d)
    a = alpha[:, None, None]
    K = torch.exp(-a * torch.log1p((df * df).sum(-1) / (2.0 * a)))
    return K if oscale is None else oscale[:, None, None] * K


def _khat(X, ell, alpha, oscale, noise):
    return rq_kernel(X, X, ell, alpha, oscale) + noise[:, None, None] * torch.eye(X.shape[0], dtype=X.dtype)


def rq_logprob(X, y, ell, alpha, oscale, noise):
    """log N(y_i; 0, K_i + noise_i I) per latent, (q,)."""
    n = X.shape[0]
    L = torch.linalg.cholesky(_khat(X, ell, alpha, oscale, noise))
    z = torch.linalg.solve_triangular(L, y.unsqueeze(-1), upper=False).squeeze(-1)
    return -0.5 * (z ** 2).sum(-1) - torch.log(torch.diagonal(L, dim1=-2, dim2=-1)).sum(-1) - 0.5 * n * math.log(2.0 * math.pi)


def rq_posterior(X, y, Xs, ell, alpha, oscale, noise):
    """Posterior mean (q, ns) and covariance (q, ns, ns) of zero-mean GPs."""
    Ks = rq_kernel(X, Xs, ell, alpha, oscale)
    L = torch.linalg.cholesky(_khat(X, ell, alpha, oscale, noise))
    V = torch.linalg.solve_triangular(L, Ks, upper=False)
    z = torch.linalg.solve_triangular(L, y.unsqueeze(-1), upper=False)
    return (V.transpose(-1, -2) @ z).squeeze(-1), rq_kernel(Xs, Xs, ell, alpha, oscale) - V.transpose(-1, -2) @ V


def prior_draw(X, ell, alpha, oscale, noise, seed):
    """y (q, n) ~ N(0, K + noise I), one draw per latent."""
    g = torch.Generator().manual_seed(seed)
    L = torch.linalg.cholesky(_khat(X, ell, alpha, oscale, noise))
    return (L @ torch.randn(ell.shape[0], X.shape[0], 1, generator=g, dtype=X.dtype)).squeeze(-1)


def fp32_bound(d, oscale):
    """(q, 1, 1): (d + 8) 2^-24 os, the per-element bound of the fp32 assembly whatever alpha is."""
    return ((d + 8) * U32 * oscale)[:, None, None]


def large_alpha_inputs(alpha):
    """n = 257 near-uniform points on [0, 1], d = 1, ell = 0.2, all rounded to fp32 and returned as fp64: X, ell, alpha, oscale."""
    n = 257
    g = torch.Generator().manual_seed(0)
    X = ((torch.arange(n, dtype=torch.float64) + 0.3 * torch.rand(n, generator=g, dtype=torch.float64)) / n).reshape(n, 1)
    X[0, 0], X[-1, 0] = 0.0, 1.0
    ell = torch.tensor([[0.2]], dtype=torch.float64)
    al = torch.tensor([float(alpha)], dtype=torch.float64)
    os_ = torch.tensor([1.0], dtype=torch.float64)
    return tuple(t.float().double() for t in (X, ell, al, os_))


def naive_fp32(Xa, Xb, ell, alpha, oscale):
    """The textbook restatement, all in torch float32 on the CPU: os pow(1 + r^2 / (2 alpha), -alpha) on the scaled inputs.  (na, nb)
    of latent 0."""
    a, b, l, al, o = (t.float() for t in (Xa, Xb, ell, alpha, oscale))
    df = a[:, None, :] / l[0] - b[None, :, :] / l[0]
    return o[0] * torch.pow(1.0 + (df * df).sum(-1) / (2.0 * al[0]), -al[0])


def prescribed_fp32(Xa, Xb, ell, alpha, oscale):
    """An fp32 emulation of the prescribed form, every operation rounded to float32: raw difference times fl(1 / ell), the sum of
    squares, times fl(1 / (2 alpha)), log1p, times alpha, exp, times os.  (na, nb) of latent 0."""
    a, b, l, al, o = (t.float() for t in (Xa, Xb, ell, alpha, oscale))
    sd = (a[:, None, :] - b[None, :, :]) * (1.0 / l[0])
    u = (sd * sd).sum(-1) * (0.5 / al[0])
    return o[0] * torch.exp(-(al[0] * torch.log1p(u)))


def h_direct_fp32(u):
    """log1p(u) - u / (1 + u) in float32: two nearly equal terms at small u."""
    u = u.float()
    return torch.log1p(u) - u / (1.0 + u)


def h_accurate_fp32(u, terms=9, threshold=0.125):
    """The library's h(u) restated in float32: below `threshold` the series sum_{k = 2}^{terms} (-1)^k (k - 1) / k u^k (Horner), the
    direct form from there on."""
    u = u.float()
    p = torch.full_like(u, (-1.0 if terms & 1 else 1.0) * (terms - 1) / terms)
    for k in range(terms - 1, 1, -1):
        p = p * u + (-1.0 if k & 1 else 1.0) * (k - 1) / k
    return torch.where(u < threshold, p * (u * u), h_direct_fp32(u))
