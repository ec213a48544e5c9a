"""The algebra behind predictions that are differentiable in hyper-parameters, noise and targets, on the CPU in fp64:
`_engine.posterior_hyper_operands` and the dense reference of the weighted kernel-gradient sum (`_weighted_grad_ref`) reproduce autograd
through a dense posterior for every family, for y and for the noise; with operands whose product is Khat^-1 - alpha alpha^T the reference
is -2 x the marginal-likelihood gradient; the padding of the operands is exact zeros; seeded mistakes are caught; the fp32 bound of the GPU
test separates an fp16-rounded operand and a dropped contraction row from the fp64 reference; and the refusals carry their names."""
import math

import pytest
import torch

import _posterior_dx_dense as pdd
import _weighted_grad_ref as wgr
from oracle import gp_math as gm

N_TRAIN, N_TEST, D, Q = 23, 7, 3, 2


def _setup(family, seed=3, n=N_TRAIN, ns=N_TEST, d=D, q=Q):
    p = wgr.problem(family, d, q, seed)
    X, Xs = pdd.igd.inputs(n, d, seed), pdd.query_points(ns, d, seed)
    if family.startswith("sum_"):                  # the sum's table is made for inputs of a few lengthscales' extent
        X, Xs = 3.0 * X, 3.0 * Xs
    g = torch.Generator().manual_seed(seed + 9)
    y = torch.randn(q, n, generator=g, dtype=torch.float64)
    noise = 0.05 + 0.2 * torch.rand(q, generator=g, dtype=torch.float64)
    gmean = torch.randn(q, ns, generator=g, dtype=torch.float64)
    gvar = torch.randn(q, ns, generator=g, dtype=torch.float64)
    return p, X, Xs, y, noise, gmean, gvar


def _autograd_through_posterior(p, X, Xs, y, noise, gmean, gvar):
    """d (sum gmean mean + gvar var) / d (ell, noise, oscale, y) through the dense Cholesky posterior."""
    leaves = [p.ell.clone().requires_grad_(True), noise.clone().requires_grad_(True), y.clone().requires_grad_(True)]
    if p.oscale is not None:
        leaves.append(p.oscale.clone().requires_grad_(True))
    K = wgr.dense_kernel(p.kind, leaves[0], leaves[3] if p.oscale is not None else None)
    mean, var = pdd.dense_posterior(K, X, leaves[2], leaves[1], Xs)
    loss = (gmean * mean).sum() + (0 if gvar is None else (gvar * var).sum())
    g = torch.autograd.grad(loss, leaves, allow_unused=True)
    g = [torch.zeros_like(l) if t is None else torch.nan_to_num(t, nan=0.0) for t, l in zip(g, leaves)]
    return g[0], g[1], g[2], (g[3] if p.oscale is not None else None)


def _through_operands(p, X, Xs, y, noise, gmean, gvar, mutate=None):
    from projectedlmc import _engine
    n, ns = X.shape[0], Xs.shape[0]
    K = wgr.dense_kernel(p.kind, p.ell, p.oscale)
    alpha, B = pdd.solved_operands(K, X, y, noise, Xs)
    u = None
    if gvar is None:
        Khat = K(X, X) + noise[:, None, None] * torch.eye(n, dtype=torch.float64)
        u = torch.linalg.solve(Khat, K(X, Xs) @ gmean.unsqueeze(-1)).squeeze(-1)
    Pt, Qt, u = _engine.posterior_hyper_operands(alpha, None if gvar is None else B, gmean, gvar, n, ns, u=u)
    if mutate == "no_rank_one":
        Pt[:, ns:ns + 2] = 0
    elif mutate == "no_e":
        Qt[:, :ns, n:] = 0
        Pt[:, :ns, n:] = 0
    (g_ell, g_noise, g_os), _ = wgr.weighted_grad_ref(p.kind, p.ell, p.oscale, noise, torch.cat([X, Xs]), Pt, Qt,
                                                      mutate=mutate if mutate in ("diag_twice", "lower") else None, terms=False)
    if gvar is not None and mutate != "keep_noise":
        g_noise = g_noise - gvar.sum(-1)
    return g_ell, g_noise, u, g_os


def _close(got, want, tol=1e-9):
    for a, b in zip(got, want):
        if b is None:
            assert a is None
            continue
        scale = max(1.0, float(b.abs().max()))
        if float((a - b).abs().max()) > tol * scale:
            return False
    return True


@pytest.mark.parametrize("family", wgr.FAMILIES)
def test_operands_and_reference_reproduce_autograd_through_the_posterior(family):
    """every hyper-parameter, the noise (with the sum gvar correction) and y, for a loss of mean and variance"""
    args = _setup(family)
    assert _close(_through_operands(*args), _autograd_through_posterior(*args))


@pytest.mark.parametrize("family", ("matern52", "poly2", "sm3", "sum_mixed"))
def test_mean_only_form(family):
    """gvar absent: two rows, B never enters, u handed in"""
    p, X, Xs, y, noise, gmean, _ = _setup(family, seed=5)
    got = _through_operands(p, X, Xs, y, noise, gmean, None)
    assert _close(got, _autograd_through_posterior(p, X, Xs, y, noise, gmean, None))
    from projectedlmc import _engine
    with pytest.raises(ValueError, match="u = Khat\\^-1"):
        _engine.posterior_hyper_operands(y, None, gmean, None, X.shape[0], Xs.shape[0])


@pytest.mark.parametrize("family", ("rbf", "matern32", "add_disjoint", "spline"))
def test_inverse_minus_outer_product_gives_minus_twice_the_mll_gradient(family):
    """At = Bt-shaped operands with At^T Bt = Khat^-1 - alpha alpha^T: the weighted sum is -2 d logp / d theta of the dense helpers"""
    p, X, _, y, noise, _, _ = _setup(family, seed=7)
    n, q = X.shape[0], y.shape[0]
    K = wgr.dense_kernel(p.kind, p.ell, p.oscale)
    Khat = K(X, X) + noise[:, None, None] * torch.eye(n, dtype=torch.float64)
    Wc = torch.linalg.inv(torch.linalg.cholesky(Khat))                   # W with W^T W = Khat^-1, K-major
    alpha = torch.linalg.solve(Khat, y.unsqueeze(-1)).squeeze(-1)
    At = torch.cat([Wc, alpha[:, None, :]], 1)
    Bt = torch.cat([Wc, -alpha[:, None, :]], 1)
    (g_ell, g_noise, g_os), _ = wgr.weighted_grad_ref(p.kind, p.ell, p.oscale, noise, X, At, Bt, terms=False)
    leaves = [p.ell.clone().requires_grad_(True), noise.clone().requires_grad_(True), p.oscale.clone().requires_grad_(True)]
    Kh = wgr.khat(p.kind, leaves[0], leaves[2], leaves[1], X)
    lp = sum(gm.mvn_log_prob(Kh[l], y[l]) for l in range(q))
    want = torch.autograd.grad(lp, leaves, allow_unused=True)
    want = [torch.zeros_like(l) if t is None else t for t, l in zip(want, leaves)]
    assert _close((g_ell, g_noise, g_os), (-2.0 * want[0], -2.0 * want[1], -2.0 * want[2]))


@pytest.mark.parametrize("n,ns,variance", [(23, 7, True), (128, 1, True), (1, 1, True), (127, 130, True), (23, 7, False)])
def test_operand_padding_is_exact_zeros(n, ns, variance):
    from projectedlmc import _engine
    g = torch.Generator().manual_seed(n + ns)
    q = 2
    alpha = torch.randn(q, n + 5, generator=g, dtype=torch.float64)                  # wider buffers than n, ns: views of padded workspaces
    B = torch.randn(q, n + 5, ns + 3, generator=g, dtype=torch.float64)
    gmean, gvar = torch.randn(q, ns, generator=g, dtype=torch.float64), torch.randn(q, ns, generator=g, dtype=torch.float64)
    u0 = None if variance else torch.randn(q, n, generator=g, dtype=torch.float64)
    Pt, Qt, u = _engine.posterior_hyper_operands(alpha, B if variance else None, gmean, gvar if variance else None, n, ns, u=u0)
    r, N = (ns + 2 if variance else 2), n + ns
    assert Pt.shape == Qt.shape == (q, -(-r // wgr.BK) * wgr.BK, -(-N // wgr.NB) * wgr.NB) and u.shape == (q, n)
    for M in (Pt, Qt):
        assert M.is_contiguous() and not M[:, r:].any() and not M[:, :, N:].any()
    r0 = ns if variance else 0
    assert torch.equal(Qt[:, r0, :n], alpha[:, :n]) and not Qt[:, r0, n:].any()
    assert torch.equal(Qt[:, r0 + 1, :n], u) and torch.equal(Qt[:, r0 + 1, n:N], -gmean)
    assert torch.equal(Pt[:, r0], -0.5 * Qt[:, r0 + 1]) and torch.equal(Pt[:, r0 + 1], -0.5 * Qt[:, r0])
    if variance:
        assert torch.equal(u, torch.bmm(B[:, :n, :ns], gmean.unsqueeze(-1)).squeeze(-1))
        assert torch.equal(Qt[:, :ns, :n], B[:, :n, :ns].transpose(1, 2))
        assert torch.equal(Qt[:, :ns, n:N], -torch.eye(ns, dtype=torch.float64).expand(q, ns, ns))
        assert torch.equal(Pt[:, :ns], gvar[:, :, None] * Qt[:, :ns])
        M = Pt.transpose(1, 2) @ Qt                                                  # symmetric, test x test block = diag(gvar)
        assert torch.allclose(M, M.transpose(1, 2), rtol=0, atol=1e-12 * float(M.abs().max()))
        assert torch.allclose(M[:, n:N, n:N], torch.diag_embed(gvar), rtol=0, atol=1e-13)


@pytest.mark.parametrize("mutate", ["diag_twice", "keep_noise", "no_rank_one", "no_e"])
@pytest.mark.parametrize("family", ("matern52", "poly2"))
def test_seeded_mistakes_are_caught(family, mutate):
    """diagonal counted twice, the test diagonal's noise not removed, the two rank-one rows dropped, the -e_c block missing: each moves a
    gradient far outside the agreement of the unmutated construction"""
    args = _setup(family, seed=11)
    want = _autograd_through_posterior(*args)
    assert _close(_through_operands(*args), want)
    assert not _close(_through_operands(*args, mutate=mutate), want, tol=1e-3)


def test_lower_triangle_mistake_is_caught_on_a_product_that_is_not_symmetric():
    """the documented sum for a non-symmetric At^T Bt is the UPPER-weighted one: held against an explicit double loop"""
    p = wgr.problem("rbf", 2, 1, 13)
    Z = pdd.igd.inputs(6, 2, 13)
    noise = torch.tensor([0.3], dtype=torch.float64)
    At, Bt = wgr.random_operands(3, 6, 1, 13, symmetric=False)
    M = (At.transpose(1, 2) @ Bt)[0]
    ell = p.ell.clone().requires_grad_(True)
    Kh = wgr.khat(p.kind, ell, p.oscale, noise, Z)[0]
    tot = 0
    for i in range(6):
        for j in range(i, 6):
            tot = tot + (1.0 if i == j else 2.0) * M[i, j] * Kh[i, j]
    want, = torch.autograd.grad(tot, ell)
    up = wgr.weighted_grad_ref(p.kind, p.ell, p.oscale, noise, Z, At, Bt, terms=False)[0][0]
    low = wgr.weighted_grad_ref(p.kind, p.ell, p.oscale, noise, Z, At, Bt, mutate="lower", terms=False)[0][0]
    assert torch.allclose(up, want, rtol=1e-12, atol=1e-14)
    assert (low - want).abs().max() > 1e-3 * want.abs().max()


@pytest.mark.parametrize("family", ("matern52", "poly2"))
def test_fp32_bound_separates_a_half_precision_operand_and_a_dropped_row(family):
    """at the kappa of the GPU test, kappa (r + d + 4) 2^-24 S_t, an operand rounded to fp16 and one dropped contraction row both fail --
    in the single-term class (n = n* = 1, kappa = 8) and in the class of sums (n = 128, n* = 1 and n = 200, n* = 70, kappa = 1/4), where
    the product runs over whole tiles and a lower-precision product is what the bound has to catch.  The rounding of one operand to 11
    bits averages out like a random walk over the terms while the bound is linear in r and relative to the sum of ABSOLUTE terms: at
    r = 2 over 129 points it is tens of units, at r = 72 over 270 points ~0.1 of a unit -- so there it is shown with both operands rounded."""
    p = wgr.problem(family, D, Q, 17)
    noise = torch.tensor([0.1, 0.2], dtype=torch.float64)

    def outside(n, ns, r, both=False):
        Z = torch.cat([pdd.igd.inputs(n, D, 17), pdd.query_points(ns, D, 17)])
        At, Bt = wgr.random_operands(r, n + ns, Q, 17)
        At = At * (1.0 + 2.0 ** -12)                                     # (values that fp16 cannot hold: the draw is fp32-representable only)
        G, S = wgr.weighted_grad_ref(p.kind, p.ell, p.oscale, noise, Z, At, Bt)
        bound = wgr.kappa(n + ns) * (r + D + 4) * 2.0 ** -24 * wgr.flat_table(S)
        half = wgr.weighted_grad_ref(p.kind, p.ell, p.oscale, noise, Z, At.half().double(), Bt.half().double() if both else Bt, terms=False)[0]
        dropped = wgr.weighted_grad_ref(p.kind, p.ell, p.oscale, noise, Z, At[:, :-1], Bt[:, :-1], terms=False)[0]
        return [bool(((wgr.flat_table(bad) - wgr.flat_table(G)).abs() > bound).any()) for bad in (half, dropped)]

    assert outside(1, 1, 2) == [True, True]
    assert outside(128, 1, 2) == [True, True]
    assert outside(200, 70, 72, both=True) == [True, True]


def test_refusals_by_name_on_host_tensors():
    import projectedlmc as plmc
    from projectedlmc import _engine, settings
    assert settings.posterior_hyper_grad.on() is False
    with settings.posterior_hyper_grad(True):
        assert settings.posterior_hyper_grad.on() is True
        with settings.posterior_hyper_grad(False):
            assert settings.posterior_hyper_grad.on() is False
    assert settings.posterior_hyper_grad.on() is False
    X, Xs = torch.rand(10, 2, dtype=torch.float64), torch.rand(3, 2, dtype=torch.float64)
    ell = torch.ones(1, 2, dtype=torch.float64, requires_grad=True)
    noise, y = torch.full((1,), 0.1, dtype=torch.float64), torch.randn(1, 10, dtype=torch.float64)
    with settings.posterior_hyper_grad(True):
        with pytest.raises(NotImplementedError, match="full_cov=True under settings.posterior_hyper_grad"):
            _engine.exact_posterior("rbf", X, ell, None, noise, y, Xs, full_cov=True)
        with pytest.raises(RuntimeError, match="no CPU fallback"):                   # the node itself runs on the device only
            _engine.exact_posterior("rbf", X, ell, None, noise, y, Xs)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _engine.weighted_grad("rbf", X, ell, None, torch.zeros(1, 16, 128, dtype=torch.float64), torch.zeros(1, 16, 128, dtype=torch.float64), 10)
    train_x, train_y = torch.rand(12, 2), torch.randn(12)
    with settings.posterior_hyper_grad(True):
        m = plmc.ExactGPModel(train_x, train_y, plmc.GaussianLikelihood(), n_inducing_points=4).eval()
        with pytest.raises(NotImplementedError, match="posterior_hyper_grad.*SGPR"):
            m(train_x[:3])
        m = plmc.ExactGPModel(train_x, train_y, plmc.GaussianLikelihood(), input_transform=torch.nn.Linear(2, 2)).eval()
        with pytest.raises(NotImplementedError, match="posterior_hyper_grad.*input_transform"):
            m(train_x[:3])
        m = plmc.ExactGPModel(train_x, train_y, plmc.GaussianLikelihood()).eval()
        with pytest.raises(NotImplementedError, match="posterior_hyper_grad.*full_cov"):
            m(train_x[:3], full_cov=True)
        with settings.skip_posterior_variances(True):
            with pytest.raises(NotImplementedError, match="posterior_hyper_grad.*skip_posterior_variances"):
                m(train_x[:3])
        Y = torch.randn(12, 3)
        pm = plmc.ProjectedGPModel(train_x, Y, 3, 2, mean_type=plmc.ZeroMean, latent_shard=(0, 2)).eval()
        with pytest.raises(NotImplementedError, match="posterior_hyper_grad.*latent-sharded"):
            pm(train_x[:3])
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            mt = plmc.MultitaskGPModel(train_x, Y, plmc.MultitaskGaussianLikelihood(num_tasks=3), n_tasks=3, n_latents=2,
                                       kernel_type=plmc.RBFKernel).eval()
            vm = plmc.VariationalMultitaskGPModel(train_x, n_tasks=3, n_latents=2, train_ind_ratio=2.0).eval()
        with pytest.raises(NotImplementedError, match="posterior_hyper_grad.*MultitaskGPModel"):
            mt(train_x[:3])
        with pytest.raises(NotImplementedError, match="posterior_hyper_grad.*variational"):
            vm(train_x[:3])
        with torch.no_grad():                                                        # no gradient to be partial about: nothing is refused
            try:
                vm(train_x[:3])
            except NotImplementedError as e:
                raise AssertionError("refused without a graph: %s" % e)
            except RuntimeError:
                pass                                                                 # (the variational engine itself runs on the device only)


def test_log_prob_of_predictive_covariances_is_the_dense_gaussian():
    """what `-likelihood(model(x_val)).log_prob(y_val)` ends in: a dense (batched) predictive covariance, and the task-space posterior with
    latent variances -- independent points, one p x p block each -- against torch.distributions; full latent covariances say so"""
    from projectedlmc.distributions import KroneckerSumCovariance, MultitaskMultivariateNormal, MultivariateNormal
    g = torch.Generator().manual_seed(5)
    A = torch.randn(2, 6, 6, generator=g, dtype=torch.float64)
    cov = (A @ A.transpose(1, 2) + 0.5 * torch.eye(6, dtype=torch.float64)).requires_grad_(True)
    mean, y = torch.randn(2, 6, generator=g, dtype=torch.float64), torch.randn(2, 6, generator=g, dtype=torch.float64)
    got = MultivariateNormal(mean, cov).log_prob(y)
    want = torch.distributions.MultivariateNormal(mean, covariance_matrix=cov).log_prob(y)
    assert got.shape == (2,) and torch.allclose(got, want, rtol=1e-12, atol=1e-12)
    assert torch.allclose(torch.autograd.grad(got.sum(), cov, retain_graph=True)[0], torch.autograd.grad(want.sum(), cov)[0], rtol=1e-9, atol=1e-12)
    q, n, p = 2, 5, 3
    Ht = torch.randn(q, p, generator=g, dtype=torch.float64)
    var = torch.rand(q, n, generator=g, dtype=torch.float64) + 0.1
    S = torch.randn(p, p, generator=g, dtype=torch.float64)
    Sigma = S @ S.T + 0.1 * torch.eye(p, dtype=torch.float64)
    mean, y = torch.randn(n, p, generator=g, dtype=torch.float64), torch.randn(n, p, generator=g, dtype=torch.float64)
    got = MultitaskMultivariateNormal(mean, KroneckerSumCovariance(Ht, var=var, eps=1e-3).add_task_noise(Sigma)).log_prob(y)
    blocks = torch.einsum("qs,qa,qb->sab", var, Ht, Ht) + 1e-3 * torch.eye(p, dtype=torch.float64) + Sigma
    want = torch.distributions.MultivariateNormal(mean, covariance_matrix=blocks).log_prob(y).sum()
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)
    full = KroneckerSumCovariance(Ht, cov=torch.diag_embed(var), eps=1e-3)
    with pytest.raises(NotImplementedError, match="latent variances"):
        MultitaskMultivariateNormal(mean, full).log_prob(y)
