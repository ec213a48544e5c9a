"""Dense fp64 references for kernels that are SUMS of scaled ARD kernels on subsets of the inputs (`decomp`) under inducing points:
the Titsias (SGPR) terms and predictive moments, the variational latent moments and the ELBO, restated for a dense-kernel CALLABLE
K(Xa, Xb) -> (q, na, nb).  `oracle/sgpr.py` and `oracle/variational.py` take a kernel `kind` and cannot express a sum; the formulas here are
theirs.  TEST INFRASTRUCTURE ONLY: plain torch on the CPU, nothing from the package; each component is `oracle.gp_math.kernel_matrix` on the
group's columns with the group's lengthscales.  Also the per-component references of the component-table kernel VJP."""
import math

import torch

from oracle import gp_math as gm


def additive_kernel(kind, nu, decomp, ells, oscales):
    """K(Xa, Xb) = sum_g os_g k(Xa[:, idx_g], Xb[:, idx_g]; ell_g), (q, na, nb).  ells[g]: (q, |idx_g|); oscales[g]: (q) | None."""
    def K(Xa, Xb):
        out = 0
        for idx, ell, osc in zip(decomp, ells, oscales):
            out = out + gm.kernel_matrix(kind, Xa[:, idx], Xb[:, idx], ell, osc, nu)
        return out
    return K


def prior_variance(oscales, q):
    """k(x, x) = sum_g os_g of the stationary kinds, (q)."""
    return sum(torch.ones(q, dtype=torch.float64) if o is None else o for o in oscales)


# ------------------------------------------------------------------------------------------------ SGPR (oracle/sgpr.py)
def sgpr_terms(K, kxx, X, Z, noise, y):
    """Per latent: (log N(y; 0, Q + s I), -1/2 sum_i (k_ii - q_ii) / s), Q = K_xz K_zz^-1 K_zx.  kxx (q): the prior variance."""
    Kzz, Kzx = K(Z, Z), K(Z, X)
    Q = Kzx.transpose(-1, -2) @ torch.linalg.solve(Kzz, Kzx)
    n = X.shape[0]
    lp = gm.mvn_log_prob(Q + noise.reshape(-1, 1, 1) * torch.eye(n, dtype=X.dtype), y)
    trace = -0.5 * (n * kxx - torch.diagonal(Q, dim1=-2, dim2=-1).sum(-1)) / noise
    return lp, trace


def sgpr_posterior(K, X, Z, noise, y, Xs):
    Kzz, Kzx, Kzs = K(Z, Z), K(Z, X), K(Z, Xs)
    n = X.shape[0]
    Q = Kzx.transpose(-1, -2) @ torch.linalg.solve(Kzz, Kzx)
    Qsx = Kzs.transpose(-1, -2) @ torch.linalg.solve(Kzz, Kzx)
    Qss = Kzs.transpose(-1, -2) @ torch.linalg.solve(Kzz, Kzs)
    C = Q + noise.reshape(-1, 1, 1) * torch.eye(n, dtype=X.dtype)
    mean = (Qsx @ torch.linalg.solve(C, y.unsqueeze(-1))).squeeze(-1)
    return mean, Qss - Qsx @ torch.linalg.solve(C, Qsx.transpose(-1, -2))


# ------------------------------------------------------------------------------------------------ variational (oracle/variational.py)
def latent_predictive(K, kxx, X, Z, var_mean, chol_var, jitter):
    """(mean_f (q,n), var_f (q,n), KL (q)) of the q whitened SVGPs."""
    m = Z.shape[0]
    L = torch.linalg.cholesky(K(Z, Z) + jitter * torch.eye(m, dtype=X.dtype))
    A = torch.linalg.solve_triangular(L, K(Z, X), upper=False)
    mean_f = (A.transpose(-1, -2) @ var_mean.unsqueeze(-1)).squeeze(-1)
    Ls = chol_var.tril()
    Bm = Ls.transpose(-1, -2) @ A
    var_f = kxx[:, None] + jitter - (A * A).sum(-2) + (Bm * Bm).sum(-2)
    logdetS = 2.0 * torch.log(torch.diagonal(Ls, dim1=-2, dim2=-1).abs()).sum(-1)
    kl = 0.5 * ((Ls * Ls).sum((-2, -1)) + (var_mean * var_mean).sum(-1) - m - logdetS)
    return mean_f, var_f, kl


def unwhitened_latent_predictive(K, kxx, X, Z, var_mean, chol_var, jitter):
    m = Z.shape[0]
    Khat = K(Z, Z) + jitter * torch.eye(m, dtype=X.dtype)
    Ls = chol_var.tril()
    S = Ls @ Ls.transpose(-1, -2)
    Kinv = torch.linalg.inv(Khat)
    logdetK = torch.linalg.slogdet(Khat)[1]
    logdetS = 2.0 * torch.log(torch.diagonal(Ls, dim1=-2, dim2=-1).abs()).sum(-1)
    quad = (var_mean.unsqueeze(-2) @ Kinv @ var_mean.unsqueeze(-1)).reshape(-1)
    kl = 0.5 * ((Kinv * S).sum((-2, -1)) + quad - m + logdetK - logdetS)
    if X.shape == Z.shape and torch.equal(X, Z):
        return var_mean, torch.diagonal(S, dim1=-2, dim2=-1), kl
    Kzx = K(Z, X)
    B = Kinv @ Kzx
    mean_f = (B.transpose(-1, -2) @ var_mean.unsqueeze(-1)).squeeze(-1)
    var_f = kxx[:, None] - (Kzx * B).sum(-2) + ((Ls.transpose(-1, -2) @ B) ** 2).sum(-2)
    return mean_f, var_f, kl


def variational_elbo(K, kxx, X, Y, Z, var_mean, chol_var, H, task_noise_diag, task_means, jitter, num_data, whitened=True):
    n, p = Y.shape
    pred = latent_predictive if whitened else unwhitened_latent_predictive
    mean_f, var_f, kl = pred(K, kxx, X, Z, var_mean, chol_var, jitter)
    mu = mean_f.T @ H + task_means.reshape(1, p)
    var = var_f.T @ (H * H)
    s = task_noise_diag.reshape(1, p)
    ell_term = -0.5 * (((Y - mu) ** 2 + var) / s + torch.log(s) + math.log(2 * math.pi)).sum()
    return ell_term / n - kl.sum() / num_data


# ------------------------------------------------------------------------------------------------ kernel VJP of a component table
def table_vjp(kind, nu, decomp, X1, X2, ells, oscales, G):
    """Autograd of sum_i <G_i, sum_g os_ig k(X1[:, idx_g], X2[:, idx_g]; ell_ig)> per component (oracle.gp_math.kernel_vjp; X2 is held
    constant) and the sums of absolute terms behind each output (kernel_vjp_abs_terms), laid out like the component table:
    (gX1 (n1,d), gEll (q,G,d), gOs (q,G)) twice.  Slots outside a component's group and dimensions no group uses hold exact zeros."""
    q, (n1, d), ng = G.shape[0], X1.shape, len(decomp)
    wX, tX = torch.zeros(n1, d, dtype=torch.float64), torch.zeros(n1, d, dtype=torch.float64)
    wE, tE = torch.zeros(q, ng, d, dtype=torch.float64), torch.zeros(q, ng, d, dtype=torch.float64)
    wO, tO = torch.zeros(q, ng, dtype=torch.float64), torch.zeros(q, ng, dtype=torch.float64)
    for g, (idx, ell, osc) in enumerate(zip(decomp, ells, oscales)):
        os_eff = torch.ones(q, dtype=torch.float64) if osc is None else osc
        a = gm.kernel_vjp(kind, X1[:, idx], X2[:, idx], ell, os_eff, G, nu)
        b = gm.kernel_vjp_abs_terms(kind, X1[:, idx], X2[:, idx], ell, os_eff, G, nu)
        wX[:, idx] += a[0]
        tX[:, idx] += b[0]
        wE[:, g, idx], tE[:, g, idx] = a[1], b[1]
        wO[:, g], tO[:, g] = a[2], b[2]
    return (wX, wE, wO), (tX, tE, tO)


def component_table(decomp, ells, oscales, d):
    """ell (q, G, d) with +inf outside each group, oscale (q, G) | None."""
    q = ells[0].shape[0]
    ell = torch.full((q, len(decomp), d), float("inf"), dtype=torch.float64)
    for g, (idx, e) in enumerate(zip(decomp, ells)):
        ell[:, g, idx] = e
    osc = None if oscales[0] is None else torch.stack(list(oscales), 1)
    return ell, osc
