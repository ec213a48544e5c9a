"""Dense fp64 reference of a GP with per-point observation noise, plain torch on the CPU (no library, no GPU):
    Khat = K + diag(noise + s),   noise (q) the homoskedastic part, s (n) or (q, n) the per-point vector,
its log density, the autograd gradients of that density, the posterior at test points and the posterior of the model conditioned on
further observations (the "bordered" posterior a fantasy model must reproduce: the new rows' diagonal carries noise + s_new).
The kernels are the engine's kinds in the engine's table layout: "matern52" (table (q, d) lengthscales), "rq" (table (q, d + 1) =
[lengthscales | alpha]) and "poly<P>" (table (q, d + 1) = [variances | offset]), each with an output scale (q) | None.

The assertions the GPU tests apply are here too (check_*), at the tolerances the project applies to the same quantities
(tests/test_gpu_engine.py), so that tests/test_fixed_noise_host.py can hold seeded mutations of this reference against them.
MUTATION switches a deliberate error on: "row" adds the vector to every element of its row of the expected assembly buffer instead of
the diagonal, "border" leaves the new rows' noise off the bordered matrix."""
import math

import torch

LOG2PI = math.log(2.0 * math.pi)
MUTATION = None


def kernel(kind, X1, X2, table, oscale=None):
    """(q, n1, n2) noise-free covariance."""
    if kind == "matern52":
        a, b = X1.unsqueeze(0) / table.unsqueeze(1), X2.unsqueeze(0) / table.unsqueeze(1)
        r2 = ((a.unsqueeze(2) - b.unsqueeze(1)) ** 2).sum(-1)
        r = torch.sqrt(r2.clamp_min(1e-30))
        K = (1.0 + math.sqrt(5.0) * r + (5.0 / 3.0) * r2) * torch.exp(-math.sqrt(5.0) * r)
    elif kind == "rq":
        ell, alpha = table[:, :-1], table[:, -1]
        a, b = X1.unsqueeze(0) / ell.unsqueeze(1), X2.unsqueeze(0) / ell.unsqueeze(1)
        r2 = ((a.unsqueeze(2) - b.unsqueeze(1)) ** 2).sum(-1)
        al = alpha.reshape(-1, 1, 1)
        K = (1.0 + r2 / (2.0 * al)) ** (-al)
    elif kind.startswith("poly"):
        P = int(kind[4:])
        v, c = table[:, :-1], table[:, -1]
        K = (c.reshape(-1, 1, 1) + torch.einsum("ik,qk,jk->qij", X1, v, X2)) ** P
    else:
        raise ValueError(kind)
    return K if oscale is None else K * oscale.reshape(-1, 1, 1)


def noisy(K, noise, s):
    """K + diag(noise + s): K (q, n, n), noise (q), s (n) | (q, n)."""
    q, n = K.shape[0], K.shape[-1]
    return K + torch.diag_embed(noise.reshape(-1, 1) + s.expand(q, n))


def expected_assembly(base, s, n):
    """What plmc_assemble*_pn_* must write, from the buffer `base` (q, rows, lda) that the entry point without a per-point vector wrote:
    diagonal[:n] += s in the element type -- one IEEE addition per entry -- and nothing else, NaN positions included."""
    q = base.shape[0]
    want = base.clone()
    sv = s.to(base.dtype).expand(q, n)
    if MUTATION == "row":
        want[:, :n, :n] += sv.unsqueeze(-1)
        return want
    want.diagonal(dim1=1, dim2=2)[:, :n] += sv
    return want


def check_assembly(got, want):
    """bit equality over the whole buffer; NaN (the pre-fill of what a call does not write) must stand in the same places"""
    nan_g, nan_w = torch.isnan(got), torch.isnan(want)
    assert torch.equal(nan_g, nan_w), "NaN positions differ: %d vs %d" % (int(nan_g.sum()), int(nan_w.sum()))
    assert torch.equal(torch.where(nan_g, torch.zeros_like(got), got), torch.where(nan_w, torch.zeros_like(want), want)), \
        "%d elements differ" % int((torch.where(nan_g, torch.zeros_like(got), got) != torch.where(nan_w, torch.zeros_like(want), want)).sum())


def log_prob(kind, X, table, oscale, noise, s, y):
    """(q,) log N(y_l; 0, Khat_l)."""
    Khat = noisy(kernel(kind, X, X, table, oscale), noise, s)
    L = torch.linalg.cholesky(Khat)
    z = torch.linalg.solve_triangular(L, y.unsqueeze(-1), upper=False).squeeze(-1)
    return -0.5 * ((z * z).sum(-1) + 2.0 * torch.log(torch.diagonal(L, dim1=-2, dim2=-1)).sum(-1) + y.shape[-1] * LOG2PI)


def gradients(kind, X, table, oscale, noise, s, y, weights=None, wrt_x=True):
    """(log density (q), {name: d (sum_l w_l logp_l) / d name}) by autograd, names "X", "table", "oscale", "noise", "s", "y"."""
    leaves = {"X": X, "table": table, "oscale": oscale, "noise": noise, "s": s, "y": y}
    leaves = {k: v.detach().clone().requires_grad_(k != "X" or wrt_x) for k, v in leaves.items() if v is not None}
    lp = log_prob(kind, leaves["X"], leaves["table"], leaves.get("oscale"), leaves["noise"], leaves["s"], leaves["y"])
    w = torch.ones_like(lp) if weights is None else weights
    (lp * w).sum().backward()
    return lp.detach(), {k: v.grad for k, v in leaves.items() if v.requires_grad}


def posterior(kind, X, table, oscale, noise, s, y, Xs):
    """(mean (q, ns), cov (q, ns, ns)) of the latent function at Xs."""
    Khat = noisy(kernel(kind, X, X, table, oscale), noise, s)
    Ks, Kss = kernel(kind, X, Xs, table, oscale), kernel(kind, Xs, Xs, table, oscale)
    L = torch.linalg.cholesky(Khat)
    V = torch.linalg.solve_triangular(L, Ks, upper=False)
    z = torch.linalg.solve_triangular(L, y.unsqueeze(-1), upper=False)
    return (V.transpose(1, 2) @ z).squeeze(-1), Kss - V.transpose(1, 2) @ V


def bordered_posterior(kind, X, table, oscale, noise, s, y, Xn, s_new, y_new, Xs):
    """The posterior at Xs given (X, y, s) and m further observations (Xn, y_new) with per-point noise s_new (m) | (q, m): the dense
    posterior of the bordered matrix [[Khat, K12], [K21, K22 + diag(noise + s_new)]]."""
    q = table.shape[0]
    if MUTATION == "border":
        s_new = torch.zeros_like(s_new)
    Xall = torch.cat([X, Xn])
    sall = torch.cat([s.expand(q, -1), s_new.expand(q, -1)], dim=-1)
    return posterior(kind, Xall, table, oscale, noise, sall, torch.cat([y, y_new], dim=-1), Xs)


# ---- the assertions of the GPU tests (tolerances: tests/test_gpu_engine.py:46-51, :190-192, :224-228)

def check_log_prob(got, want, dtype):
    got, want = got.detach().cpu().double(), want.double()
    if dtype == torch.float64:
        assert torch.allclose(got, want, rtol=1e-10, atol=0), (got, want)
    else:
        rel = ((got - want).abs() / want.abs()).max()
        assert rel < 1e-4, (float(rel), got, want)


def check_gradient(got, want, dtype, what=""):
    got, want = got.detach().cpu().double(), want.double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if dtype == torch.float64:
        assert torch.allclose(got, want, rtol=1e-7, atol=1e-9), (what, float((got - want).abs().max()))
    else:
        err = (got - want).abs().max()
        assert err < 2e-3 * want.abs().max(), (what, float(err), float(want.abs().max()))


def check_moments(mean, var, cov, want_mean, want_cov):
    """fp64 predictions: mean, marginal variance and (if not None) full covariance against posterior()'s output"""
    assert torch.allclose(mean.detach().cpu().double(), want_mean, rtol=1e-8, atol=1e-10), float((mean.detach().cpu() - want_mean).abs().max())
    wv = torch.diagonal(want_cov, dim1=-2, dim2=-1)
    assert torch.allclose(var.detach().cpu().double(), wv, rtol=1e-7, atol=1e-10), float((var.detach().cpu() - wv).abs().max())
    if cov is not None:
        assert torch.allclose(cov.detach().cpu().double(), want_cov, rtol=1e-7, atol=1e-9), float((cov.detach().cpu() - want_cov).abs().max())


FANTASY_TOL = {torch.float64: 1e-8, torch.float32: 2e-4}        # tests/test_gpu_fantasy_model.py: of the largest value


def check_fantasy(got, want, dtype, what=""):
    err = float((got.detach().cpu().double() - want.detach().cpu().double()).abs().max())
    bound = FANTASY_TOL[dtype] * max(1.0, float(want.detach().double().abs().max()))
    assert err < bound, (what, err, bound)


def problem(n, d, q, seed=0, span=(1e-3, 1e1), shared=False):
    """X (n, d) in [-1, 1], y (q, n), lengthscales (q, d), output scales (q), additional noise (q) and a per-point vector spread
    log-uniformly over span[0] .. span[1] times the output scale ((n) if shared, with the first latent's scale, else (q, n))."""
    g = torch.Generator().manual_seed(seed)
    X = 2 * torch.rand(n, d, generator=g, dtype=torch.float64) - 1
    y = torch.randn(q, n, generator=g, dtype=torch.float64)
    ell = 0.4 + 0.5 * torch.rand(q, d, generator=g, dtype=torch.float64)
    osc = 0.5 + torch.rand(q, generator=g, dtype=torch.float64)
    noise = 0.05 + 0.1 * torch.rand(q, generator=g, dtype=torch.float64)
    lo, hi = math.log(span[0]), math.log(span[1])
    u = torch.rand(n, generator=g, dtype=torch.float64) if shared else torch.rand(q, n, generator=g, dtype=torch.float64)
    s = torch.exp(lo + (hi - lo) * u) * (osc[0] if shared else osc[:, None])
    return X, y, ell, osc, noise, s


def table_of(kind, ell, seed=0):
    """the engine's table of a kind from (q, d) positive values: matern52 as they are, rq with an alpha column, poly with an offset"""
    if kind == "matern52":
        return ell.clone()
    g = torch.Generator().manual_seed(100 + seed)
    last = 0.8 + torch.rand(ell.shape[0], 1, generator=g, dtype=ell.dtype)
    return torch.cat([ell, last], dim=1)
