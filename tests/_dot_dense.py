"""Dense fp64 reference of the dot-product kernels, written from the formula [gpytorch-knowledge: LinearKernel, PolynomialKernel,
unverified offline]
    k(x, x') = os (c + sum_k v_k x_k x'_k)^P,   v_k > 0, c >= 0, P an integer >= 1
(LinearKernel: P = 1, c = 0; PolynomialKernel: v = 1) with torch on the CPU (autograd gives the gradients).  Imports nothing from the
package under test.

Also the fp32 emulation of the library's operation order and the per-element bound it is held to."""
import math

import numpy as np
import torch

U32 = 2.0 ** -24


def _ipow(s, P):
    """s^P by repeated multiplication: exact in sign for negative s, no pow."""
    out = s
    for _ in range(P - 1):
        out = out * s
    return out


def dot_s(Xa, Xb, v, c):
    """(q, na, nb): s = c + sum_k v_k a_k b_k from Xa (na, d), Xb (nb, d), v (q, d), c (q)."""
    return c[:, None, None] + torch.einsum("ik,qk,jk->qij", Xa, v, Xb)


def dot_S(Xa, Xb, v, c):
    """(q, na, nb): S = c + sum_k |v_k a_k b_k|, what the fp32 bound scales with (mixed signs cancel in s, not in S)."""
    return c[:, None, None] + torch.einsum("ik,qk,jk->qij", Xa.abs(), v.abs(), Xb.abs())


def dot_kernel(Xa, Xb, v, c, P, oscale=None):
    """(q, na, nb)."""
    K = _ipow(dot_s(Xa, Xb, v, c), P)
    return K if oscale is None else oscale[:, None, None] * K


def dot_diag(X, v, c, P, oscale=None):
    """(q, n): k(x, x) = os (c + sum_k v_k x_k^2)^P."""
    dg = _ipow(c[:, None] + v @ (X * X).T, P)
    return dg if oscale is None else oscale[:, None] * dg


def _khat(X, v, c, P, oscale, noise):
    return dot_kernel(X, X, v, c, P, oscale) + noise[:, None, None] * torch.eye(X.shape[0], dtype=X.dtype)


def dot_logprob(X, y, v, c, P, oscale, noise):
    """log N(y_i; 0, K_i + noise_i I) per latent, (q,)."""
    n = X.shape[0]
    L = torch.linalg.cholesky(_khat(X, v, c, P, oscale, noise))
    z = torch.linalg.solve_triangular(L, y.unsqueeze(-1), upper=False).squeeze(-1)
    return -0.5 * (z ** 2).sum(-1) - torch.log(torch.diagonal(L, dim1=-2, dim2=-1)).sum(-1) - 0.5 * n * math.log(2.0 * math.pi)


def dot_posterior(X, y, Xs, v, c, P, oscale, noise):
    """Posterior mean (q, ns) and covariance (q, ns, ns) of zero-mean GPs."""
    Ks = dot_kernel(X, Xs, v, c, P, oscale)
    L = torch.linalg.cholesky(_khat(X, v, c, P, oscale, noise))
    V = torch.linalg.solve_triangular(L, Ks, upper=False)
    z = torch.linalg.solve_triangular(L, y.unsqueeze(-1), upper=False)
    return (V.transpose(-1, -2) @ z).squeeze(-1), dot_kernel(Xs, Xs, v, c, P, oscale) - V.transpose(-1, -2) @ V


def dot_loo(X, y, v, c, P, oscale, noise):
    """Leave-one-out log predictive density per latent, (q,): with Pm = Khat^-1, a = Pm y, p_i = Pm_ii,
    sum_i [ 1/2 log p_i - 1/2 a_i^2 / p_i ] - n/2 log 2 pi."""
    n = X.shape[0]
    Pm = torch.linalg.inv(_khat(X, v, c, P, oscale, noise))
    a = (Pm @ y.unsqueeze(-1)).squeeze(-1)
    p = torch.diagonal(Pm, dim1=-2, dim2=-1)
    return (0.5 * p.log() - 0.5 * a * a / p).sum(-1) - 0.5 * n * math.log(2.0 * math.pi)


def prior_draw(X, v, c, P, oscale, noise, seed):
    """y (q, n) ~ N(0, K + noise I), one draw per latent."""
    g = torch.Generator().manual_seed(seed)
    L = torch.linalg.cholesky(_khat(X, v, c, P, oscale, noise))
    return (L @ torch.randn(v.shape[0], X.shape[0], 1, generator=g, dtype=X.dtype)).squeeze(-1)


TINY32 = 2.0 ** -126


def fp32_bound(Xa, Xb, v, c, P, oscale):
    """(q, na, nb): P (d + 3) 2^-24 os S^P, the per-element bound of the fp32 value against the fp64 formula at the fp32 inputs
    ((d + 1) roundings of the FMA chain, P - 1 multiplications and the output scale, one unit for the second order),
    plus the underflow term of the same derivation: each of the 2 d + P + 1 operations may lose up to the smallest normal number 2^-126
    absolutely when its result is subnormal or flushed to zero, and what follows scales that by at most os max(1, S)^(P - 1).  The term
    is 1e-36 os in the tests' ranges; it matters only where S^P itself underflows (tiny products under a high power)."""
    d = Xa.shape[1]
    os_ = torch.ones_like(c) if oscale is None else oscale
    S = dot_S(Xa, Xb, v, c)
    under = (2 * d + P + 1) * TINY32 * os_[:, None, None].clamp_min(1.0) * _ipow(S.clamp_min(1.0), P) * P
    return P * (d + 3) * U32 * os_[:, None, None] * _ipow(S, P) + under


def emulated_fp32(Xa, Xb, v, c, P, oscale):
    """The library's operation order with every operation rounded to float32, in numpy: t_k = fl(v_k a_k); s = c, then
    s = fma(t_k, b_k, s) for k = 0 .. d - 1 (the product of two floats is exact in float64, so one rounding of the float64 sum to float32
    is the fused operation up to a double rounding); p = 1 * s * ... (P - 1 roundings); os * p.  (q, na, nb) float32."""
    f = lambda t: np.asarray(t.detach().cpu().numpy(), dtype=np.float32)
    A, B, V, C = f(Xa), f(Xb), f(v), f(c)
    O = np.ones_like(C) if oscale is None else f(oscale)
    out = np.empty((V.shape[0], A.shape[0], B.shape[0]), dtype=np.float32)
    for i in range(V.shape[0]):
        T = (V[i][None, :] * A).astype(np.float32)                                  # (na, d), one rounding each
        s = np.full((A.shape[0], B.shape[0]), C[i], dtype=np.float32)
        for k in range(A.shape[1]):
            s = (T[:, k, None].astype(np.float64) * B[None, :, k].astype(np.float64) + s.astype(np.float64)).astype(np.float32)
        p = np.ones_like(s)
        for _ in range(P - 1):
            p = (p * s).astype(np.float32)
        out[i] = (O[i] * (p * s).astype(np.float32)).astype(np.float32)
    return torch.from_numpy(out)
