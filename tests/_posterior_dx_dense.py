"""Dense fp64 reference of the derivative of the eval-mode posterior moments with respect to the test inputs, for a dense-kernel CALLABLE
K(Xa, Xb) -> (q, na, nb):
    Jm[l, s, k] =      sum_i alpha_li  d k_l(xs_s, x_i) / d xs_s[k]
    Jv[l, s, k] = -2 * sum_i B_l[i, s] d k_l(xs_s, x_i) / d xs_s[k]
with alpha (q, n) and B (q, n, ns) held constant, and the dense posterior the host test holds it against.  TEST INFRASTRUCTURE ONLY: plain
torch on the CPU, nothing from the package.  The families, their problems and inputs are those of _input_grad_dense."""
import torch

import _input_grad_dense as igd

FAMILIES = igd.FAMILIES
SMALL_GROUPS = {"add_disjoint": [[0, 1], [2]], "add_overlap": [[0, 1], [1, 2]]}      # the additive families on d = 3


def problem(family, d, q, seed, use_os=True, groups=None):
    """_input_grad_dense.problem, with groups that fit a small d for the two additive families."""
    if groups is None and family in SMALL_GROUPS and d < 5:
        groups = SMALL_GROUPS[family]
    return igd.problem(family, d, q, seed, use_os, groups=groups)


def posterior_dx_ref(K, X, Xs, alpha, B):
    """(Jm, Jv, Tm, Tv), all (q, ns, d) fp64: the values by autograd of K(Xs, X) @ alpha and of -2 (K(Xs, X) * B^T).sum(-1) with respect to
    Xs (row s of K(Xs, X) depends on test point s only, so the gradient of the sum over s is the per-point derivative), and the sums of
    absolute terms sum_i |alpha_i d k / d xs_sk|, 2 sum_i |B_is d k / d xs_sk| behind each value, the pair derivatives from one forward-mode
    pass per dimension."""
    q, (ns, d) = alpha.shape[0], Xs.shape
    Xb = X.detach()
    Bt = B.transpose(1, 2)                                               # (q, ns, n)
    Jm = torch.empty(q, ns, d, dtype=torch.float64)
    Jv = torch.empty(q, ns, d, dtype=torch.float64)
    for lat in range(q):
        Xa = Xs.detach().clone().requires_grad_(True)
        Ksx = K(Xa, Xb)[lat]
        Jm[lat], = torch.autograd.grad((Ksx * alpha[lat][None, :]).sum(), Xa, retain_graph=True)
        Jv[lat], = torch.autograd.grad(-2.0 * (Ksx * Bt[lat]).sum(), Xa)
    Tm = torch.empty(q, ns, d, dtype=torch.float64)
    Tv = torch.empty(q, ns, d, dtype=torch.float64)
    for k in range(d):
        e = torch.zeros(ns, d, dtype=torch.float64)
        e[:, k] = 1.0
        dK = torch.func.jvp(lambda Xa: K(Xa, Xb), (Xs.detach().clone(),), (e,))[1].abs()
        Tm[:, :, k] = (dK * alpha.abs()[:, None, :]).sum(-1)
        Tv[:, :, k] = 2.0 * (dK * Bt.abs()).sum(-1)
    return Jm, Jv, Tm, Tv


def dense_posterior(K, X, y, noise, Xs):
    """(mean, var), (q, ns) each: the posterior of q zero-mean GPs through a dense Cholesky factor, a differentiable function of Xs."""
    q, n = y.shape
    eye = torch.eye(n, dtype=torch.float64)
    Lc = torch.linalg.cholesky(K(X, X) + noise[:, None, None] * eye)
    Ksx = K(Xs, X)                                                       # (q, ns, n)
    V = torch.linalg.solve_triangular(Lc, Ksx.transpose(1, 2), upper=False)        # (q, n, ns)
    z = torch.linalg.solve_triangular(Lc, y.unsqueeze(-1), upper=False)
    mean = (V * z).sum(1)
    prior = torch.stack([torch.diagonal(K(Xs[s:s + 1], Xs[s:s + 1]), dim1=-2, dim2=-1)[:, 0] for s in range(Xs.shape[0])], 1)
    return mean, prior - (V * V).sum(1)


def solved_operands(K, X, y, noise, Xs):
    """alpha = Khat^-1 y (q, n) and B = Khat^-1 K(X, Xs) (q, n, ns)."""
    n = X.shape[0]
    Khat = K(X, X) + noise[:, None, None] * torch.eye(n, dtype=torch.float64)
    alpha = torch.linalg.solve(Khat, y.unsqueeze(-1)).squeeze(-1)
    return alpha, torch.linalg.solve(Khat, K(X, Xs))


def query_points(ns, d, seed, X=None, coincident=False):
    """ns test points in [-1, 1]^d, fp32-representable; coincident: test point 1 (0 if there is one only) is training point 3 (the last
    if there are fewer)."""
    g = torch.Generator().manual_seed(seed + 3000)
    Xs = (2 * torch.rand(ns, d, generator=g, dtype=torch.float64) - 1).float().double()
    if coincident:
        Xs[min(1, ns - 1)] = X[min(3, X.shape[0] - 1)]
    return Xs


def random_operands(n, ns, q, seed):
    """Random alpha (q, n) and B (q, n, ns), fp32-representable."""
    g = torch.Generator().manual_seed(seed + 4000)
    return (torch.randn(q, n, generator=g, dtype=torch.float64).float().double(),
            torch.randn(q, n, ns, generator=g, dtype=torch.float64).float().double())


def nan_buffers(alpha, B, dtype, pad_rows=3, pad_cols=5, pad_alpha=7):
    """(alpha (q, n + pad_alpha), B (q, n + pad_rows, ns + pad_cols)) of `dtype` with NaN wherever the kernel must not read: alpha from n on,
    the rows of B from n on and its columns from ns up to the leading dimension."""
    q, n, ns = B.shape
    a = torch.full((q, n + pad_alpha), float("nan"), dtype=dtype)
    a[:, :n] = alpha.to(dtype)
    b = torch.full((q, n + pad_rows, ns + pad_cols), float("nan"), dtype=dtype)
    b[:, :n, :ns] = B.to(dtype)
    return a, b
