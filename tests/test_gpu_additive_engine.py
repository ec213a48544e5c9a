"""Additive (`decomp`) kernels on the batched exact engine: the new entry points per element, the log-prob and every gradient of
`ExactLatentLogProb` with a component table, `ProjectedGPModel(decomp=...)` in training and eval mode, and the machinery the
additive kernel inherits from the exact path (prediction cache, latent sharding, jitter ladder, late pivot check).

Reference values: dense torch-CPU fp64 with autograd, the sub-kernels summed with oracle.gp_math.kernel_matrix over the groups as
tests/test_gpu_additive.py does.  Tolerances are those of the tests named beside them."""
import math
import re
import warnings

import pytest
import torch

from oracle import gp_math as gm
from oracle import projected as pj
from _bridge import perturb_

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KINDS = {"rbf": ("rbf", 2.5), "matern12": ("matern", 0.5), "matern32": ("matern", 1.5), "matern52": ("matern", 2.5)}
U32 = 2.0 ** -24


@pytest.fixture(scope="module")
def eng():
    import types
    from projectedlmc import _hip, _engine, settings
    assert torch.cuda.is_available()
    return types.SimpleNamespace(hip=_hip, exact=_engine, settings=settings)


def _groups(d, G):
    """G overlapping groups of ceil(d / 2) + 1 consecutive dimensions (cyclic); one group: every dimension."""
    if G == 1:
        return [list(range(d))]
    w = min(d, (d + 1) // 2 + 1)
    return [sorted({(g * max(1, d // G) + k) % d for k in range(w)}) for g in range(G)]


def _table_problem(n, d, q, G, seed, ns=0):
    g = torch.Generator().manual_seed(seed)
    X = 2 * torch.rand(n, d, generator=g, dtype=torch.float64) - 1
    Xs = 2 * torch.rand(max(ns, 1), d, generator=g, dtype=torch.float64) - 1
    y = torch.randn(q, n, generator=g, dtype=torch.float64)
    groups = _groups(d, G)
    ell = torch.full((q, G, d), float("inf"), dtype=torch.float64)
    for gi, idx in enumerate(groups):                      # lengthscales ~ sqrt(|group|): scaled distances stay O(1)
        ell[:, gi, idx] = math.sqrt(len(idx)) * (0.3 + 0.5 * torch.rand(q, len(idx), generator=g, dtype=torch.float64))
    osc = 0.5 + torch.rand(q, G, generator=g, dtype=torch.float64)
    noise = 0.05 + 0.5 * torch.rand(q, generator=g, dtype=torch.float64)
    return X, Xs, y, groups, ell, osc, noise


def _dense_terms(kind, Xa, Xb, groups, ell, osc):
    """[os_g k_g(Xa, Xb)] per component, each (q, na, nb), from the active slots of the table."""
    okind, nu = KINDS[kind]
    return [gm.kernel_matrix(okind, Xa[:, idx], Xb[:, idx], ell[:, gi, idx], osc[:, gi], nu) for gi, idx in enumerate(groups)]


# ------------------------------------------------------------------------------------------------ 3. entry points, per element
@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("G", [1, 2, 4])
@pytest.mark.parametrize("d", [3, 8, 12])
@pytest.mark.parametrize("kind", list(KINDS))
def test_assemble_add_and_cross_add_per_element(eng, kind, d, G, dt):
    """plmc_assemble_add / plmc_assemble_cross_add against the dense sum; d = 3, 8: k_assemble_small_add<4 / 8>, d = 12: k_assemble_add;
    n is not a multiple of 128 (identity padding checked too).  Inputs rounded to the dtype first.
    Bound (that of tests/test_gpu_kernel_kinds.py:82-86,103, per component term): a term os_g k_g is formed from the scaled
    differences (2 roundings), their squared sum (d additions), the profile (~4 roundings) and the product with os_g, then added
    to the sum: an a-priori 4 (d + 4) roundings per term, so |error| <= 4 (d + 4) u sum_g |term_g| (on the diagonal the noise is one
    more term of that sum); fp64 is held to 1e-10 of the same sum.  With one component the output is the existing entry
    point's, bit for bit."""
    n, ns, q = 333, 77, 2
    L = eng.hip.lib()
    X, Xs, _, groups, ell, osc, noise = _table_problem(n, d, q, G, seed=1000 * d + 10 * G + len(kind), ns=ns)
    X, Xs, ell, osc, noise = (t.to(dt).double() for t in (X, Xs, ell, osc, noise))
    f = lambda t: t.to(DEV, dt).contiguous()
    Xd, Xsd, elld, osd, nzd = f(X), f(Xs), f(ell), f(osc), f(noise)
    n_pad = int(L.cdll.plmc_pad(n))
    st = eng.hip.stream_ptr(DEV)
    k = eng.hip.KIND[kind]
    ptr = eng.hip.ptr
    tol = 1e-10 if dt == torch.float64 else 4 * (d + 4) * U32

    A = torch.zeros(q, n_pad, n_pad, dtype=dt, device=DEV)
    L.call("plmc_assemble_add", dt, k, ptr(Xd), n, d, G, ptr(elld), ptr(osd), ptr(nzd), ptr(A), n_pad, n_pad * n_pad, q, st)
    C = torch.zeros(q, n, ns, dtype=dt, device=DEV)
    L.call("plmc_assemble_cross_add", dt, k, ptr(Xd), n, ptr(Xsd), ns, d, G, ptr(elld), ptr(osd), ptr(C), ns, n * ns, 0, n, q, st)
    torch.cuda.synchronize()

    terms = _dense_terms(kind, X, X, groups, ell, osc)
    eye = torch.eye(n, dtype=torch.float64)
    want = sum(terms) + noise.reshape(q, 1, 1) * eye
    mag = sum(t.abs() for t in terms) + noise.reshape(q, 1, 1) * eye
    upper = torch.triu(torch.ones(n, n, dtype=torch.bool))
    err = (A.cpu().double()[:, :n, :n] - want).abs()
    print("assemble_add %s d=%d G=%d %s: max err / bound = %.3g" % (kind, d, G, dt, float((err / (tol * mag))[:, upper].max())))
    assert not bool((err > tol * mag)[:, upper].any()), float((err / mag)[:, upper].max())
    # identity padding: the rows / columns beyond n inside the written (upper) tiles
    pad = A.cpu()[:, :, n:]
    want_pad = torch.zeros(n_pad, n_pad - n, dtype=dt)
    want_pad[n:, :] = torch.eye(n_pad - n, dtype=dt)
    rows_written = torch.arange(n_pad) < (n // 128 + 1) * 128
    assert torch.equal(pad[:, rows_written], want_pad[rows_written].expand(q, -1, -1))

    cterms = _dense_terms(kind, X, Xs, groups, ell, osc)
    cerr = (C.cpu().double() - sum(cterms)).abs()
    cmag = sum(t.abs() for t in cterms)
    print("assemble_cross_add %s d=%d G=%d %s: max err / bound = %.3g" % (kind, d, G, dt, float((cerr / (tol * cmag)).max())))
    assert not bool((cerr > tol * cmag).any()), float((cerr / cmag).max())

    if G == 1:
        A1 = torch.zeros_like(A)
        L.call("plmc_assemble", dt, k, ptr(Xd), n, d, ptr(elld), ptr(osd[:, 0].contiguous()), ptr(nzd), ptr(A1), n_pad, n_pad * n_pad, q, st)
        C1 = torch.zeros_like(C)
        os1 = osd[:, 0].contiguous()
        L.call("plmc_assemble_cross", dt, k, ptr(Xd), n, ptr(Xsd), ns, d, ptr(elld), ptr(os1), ptr(C1), ns, n * ns, 0, n, q, st)
        torch.cuda.synchronize()
        assert torch.equal(A, A1) and torch.equal(C, C1)


def test_additive_entry_points_refuse_the_spline_kind_and_too_many_components(eng):
    L = eng.hip.lib()
    dt, n, d, q = torch.float64, 130, 3, 1
    X = torch.rand(n, d, dtype=dt, device=DEV)
    n_pad = int(L.cdll.plmc_pad(n))
    A = torch.zeros(q, n_pad, n_pad, dtype=dt, device=DEV)
    ptr, st = eng.hip.ptr, eng.hip.stream_ptr(DEV)
    gmax = L.cdll.plmc_max_components()
    for kind, G, msg in (("spline", 2, "stationary"), ("spline", 1, "stationary"), ("rbf", gmax + 1, "components"), ("rbf", 0, "components")):
        ell = torch.ones(q, max(G, 1), d, dtype=dt, device=DEV)
        osc = torch.ones(q, max(G, 1), dtype=dt, device=DEV)
        nz = torch.ones(q, dtype=dt, device=DEV)
        with pytest.raises(RuntimeError, match=msg):
            L.call("plmc_assemble_add", dt, eng.hip.KIND[kind], ptr(X), n, d, G, ptr(ell), ptr(osc), ptr(nz), ptr(A), n_pad, n_pad * n_pad, q, st)
        with pytest.raises(RuntimeError, match=msg):
            L.call("plmc_assemble_cross_add", dt, eng.hip.KIND[kind], ptr(X), n, ptr(X), n, d, G, ptr(ell), ptr(osc), ptr(A), n_pad,
                   n_pad * n_pad, 0, n, q, st)


# ------------------------------------------------------------------------------------------------ 4. log-prob and every gradient
def _reference_logprob(kind, X, y, groups, ell, osc, noise):
    """(lp (q), grads of sum_i w_i lp_i w.r.t. table ell / osc / noise / y) by fp64 autograd through the dense sum; w = linspace(0.5, 1.5)."""
    q, n = y.shape
    ell_l = ell.clone().requires_grad_(True)
    osc_l, nz_l, y_l = (t.clone().requires_grad_(True) for t in (osc, noise, y))
    K = sum(_dense_terms(kind, X, X, groups, ell_l, osc_l)) + nz_l.reshape(q, 1, 1) * torch.eye(n, dtype=torch.float64)
    lp = gm.mvn_log_prob(K, y_l)
    w = torch.linspace(0.5, 1.5, q, dtype=torch.float64)
    (lp * w).sum().backward()
    g_ell = torch.nan_to_num(ell_l.grad, nan=0.0)          # the slots outside a group never entered the graph
    return lp.detach(), g_ell, osc_l.grad, nz_l.grad, y_l.grad, w


def _run_logprob(eng, kind, X, y, ell, osc, noise, dt, w):
    f = lambda t: t.to(DEV, dt)
    leaves = [f(t).requires_grad_() for t in (ell, osc, noise, y)]
    lp = eng.exact.exact_latent_log_prob(kind, f(X), leaves[0], leaves[1], leaves[2], leaves[3])
    (lp * f(w)).sum().backward()
    torch.cuda.synchronize()
    return [lp.detach().cpu().double()] + [t.grad.cpu().double() for t in leaves]


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("n,d", [(517, 5), (300, 12)])
def test_table_logprob_and_every_gradient_fp64(eng, kind, n, d):
    """q = 3, G = 2; tolerances of tests/test_gpu_engine.py:46-51.  The gradient on a slot outside its group is exactly 0."""
    q, G = 3, 2
    X, _, y, groups, ell, osc, noise = _table_problem(n, d, q, G, seed=n + d)
    ref = _reference_logprob(kind, X, y, groups, ell, osc, noise)
    got = _run_logprob(eng, kind, X, y, ell, osc, noise, torch.float64, ref[5])
    assert torch.allclose(got[0], ref[0], rtol=1e-10, atol=0), (got[0], ref[0])
    for name, a, b in zip(("ell", "oscale", "noise", "y"), got[1:], ref[1:5]):
        assert a.shape == b.shape, name
        assert torch.allclose(a, b, rtol=1e-7, atol=1e-9), (name, float((a - b).abs().max()))
    assert bool((got[1][torch.isinf(ell)] == 0).all())


def test_table_logprob_fp32_split_engines_and_fused_assembly(eng, monkeypatch):
    """n = 1300 (11 block rows: two groups, so the fused assembly queues rows on its helper stream), d = 8, q = 3, G = 2, fp32 under
    PLMC_SPLIT 2, 3 and 0: value 1e-4 relative, gradients 2e-3 of the largest entry (tests/test_gpu_engine.py:117).  The fused call and
    PLMC_FUSED_ASSEMBLE=0 (assembly and sweep as two calls) run the same kernels on the same data: equal as bit patterns."""
    n, d, q, G = 1300, 8, 3, 2
    X, _, y, groups, ell, osc, noise = _table_problem(n, d, q, G, seed=77)
    X, y, ell, osc, noise = (t.float().double() for t in (X, y, ell, osc, noise))
    ref = _reference_logprob("matern52", X, y, groups, ell, osc, noise)
    for split in ("2", "3", "0"):
        with eng.hip.knob("PLMC_SPLIT", split):
            got = _run_logprob(eng, "matern52", X, y, ell, osc, noise, torch.float32, ref[5])
            monkeypatch.setenv("PLMC_FUSED_ASSEMBLE", "0")
            two = _run_logprob(eng, "matern52", X, y, ell, osc, noise, torch.float32, ref[5])
            monkeypatch.delenv("PLMC_FUSED_ASSEMBLE")
        for a, b in zip(got, two):
            assert torch.equal(a, b), split
        e = float(((got[0] - ref[0]) / ref[0]).abs().max())
        print("PLMC_SPLIT=%s: log-prob rel err %.3g" % (split, e))
        assert e < 1e-4, (split, e)
        for name, a, b in zip(("ell", "oscale", "noise", "y"), got[1:], ref[1:5]):
            e = float((a - b).abs().max() / b.abs().max())
            print("PLMC_SPLIT=%s: d/d %s err %.3g of the largest" % (split, name, e))
            assert e < 2e-3, (split, name, e)
        assert bool((got[1][torch.isinf(ell)] == 0).all())


# ------------------------------------------------------------------------------------------------ 5. ProjectedGPModel(decomp=...)
DECOMP = [[0, 1], [1, 2]]


def _data(n, d, p, seed):
    g = torch.Generator().manual_seed(seed)
    X = 2 * torch.rand(n, d, generator=g, dtype=torch.float64) - 1
    Y = torch.randn(n, p, generator=g, dtype=torch.float64)
    return X, Y


def _decomp_model(plmc, X, Y, q, seed=5, **kw):
    torch.manual_seed(seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = plmc.ProjectedGPModel(X, Y, Y.shape[1], q, mean_type=plmc.ZeroMean, kernel_type=plmc.MaternKernel, decomp=DECOMP,
                                  init_lmc_coeffs=True, **kw)
    return m


def _oracle_dict(model):
    """The oracle's parameter dict (oracle/projected.py) WITHOUT the kernel keys, from the state dict: what project_data,
    projection_terms, projected_noise, lmc_coefficients and full_noise_factor read.  Default variant: bulk H, full B_tilde."""
    lb = model.likelihood.noise_covar.raw_noise_constraint.lower_bound
    sd = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
    P = dict(n_tasks=model.n_tasks, n_latents=model.n_latents, mode=model.lmc_coefficients.mode, BDN=not hasattr(model, "M"),
             eps=model.eps, scalar_B=model.scalar_B, diagonal_B=model.diagonal_B, noise_lb=lb, noise_thresh=math.log(lb), bulk=True,
             raw_noise=sd["likelihood.noise_covar.raw_noise"], H=sd["lmc_coefficients.H"],
             B_tilde_inv_chol_raw=sd["parametrizations.B_tilde_inv_chol.original"])
    kern = {k: v for k, v in sd.items() if k.startswith("covar_module.")}
    return P, kern


NAMES = {"lmc_coefficients.H": "H", "likelihood.noise_covar.raw_noise": "raw_noise",
         "parametrizations.B_tilde_inv_chol.original": "B_tilde_inv_chol_raw"}


def _latent_K(kern, Xa, Xb, q):
    K = 0
    for gi, idx in enumerate(DECOMP):
        ell = gm.softplus(kern["covar_module.kernels.%d.base_kernel.raw_lengthscale" % gi]).reshape(q, -1)
        os_ = gm.softplus(kern["covar_module.kernels.%d.raw_outputscale" % gi]).reshape(q)
        K = K + gm.kernel_matrix("matern", Xa[:, idx], Xb[:, idx], ell, os_, 2.5)
    return K


@pytest.fixture(scope="module")
def plmc():
    import projectedlmc
    assert torch.cuda.is_available()
    return projectedlmc


def test_projected_model_with_decomp_loss_gradients_and_eval_mode(plmc):
    """fp64, p = 6, q = 3, d = 3, decomp = [[0, 1], [1, 2]], perturbed parameters.  ProjectedLMCmll and the gradient of every
    parameter against sum_i log N(ytil_i; 0, K_i + noise_i I) / n + projection terms (tests/test_gpu_projected.py:67-73: 1e-9
    relative; rtol 2e-6, atol 1e-8); eval mode against dense conditioning (:136-138: rtol 1e-8 / 1e-7), compute_loo against
    1 / diag(K^-1) and K^-1 y / diag(K^-1) (1e-8, tests/test_gpu_kernel_kinds.py:283)."""
    n, d, p, q, ns = 333, 3, 6, 3, 48
    X, Y = _data(n, d, p, seed=11)
    m = perturb_(_decomp_model(plmc, X, Y, q).double())
    P, kern = _oracle_dict(m)
    leaves = {**{k: P[k] for k in NAMES.values()}, **kern}
    for v in leaves.values():
        v.requires_grad_(True)
    eye = torch.eye(n, dtype=torch.float64)
    ytil = pj.project_data(P, Y)
    K = _latent_K(kern, X, X, q) + pj.projected_noise(P).reshape(q, 1, 1) * eye
    terms, const = pj.projection_terms(P, Y)
    ref = -(gm.mvn_log_prob(K, ytil).sum() / n + sum(terms) + const)
    ref.backward()

    m = m.to(DEV)
    Xd, Yd = X.to(DEV), Y.to(DEV)
    m.train(); m.likelihood.train()
    mll = plmc.ProjectedLMCmll(m.likelihood, m)
    loss = -mll(m(Xd), Yd)
    assert getattr(mll, "_late", None) is not None            # a training step: the pivot check sits behind the backward pass
    loss.backward()
    assert abs(float(loss) - float(ref)) < 1e-9 * abs(float(ref)), (float(loss), float(ref))
    checked = 0
    for pname, prm in m.named_parameters():
        g_ref = leaves[NAMES.get(pname, pname)].grad
        assert prm.grad is not None and g_ref is not None, pname
        assert prm.grad.shape == g_ref.shape, pname
        assert torch.allclose(prm.grad.cpu(), g_ref, rtol=2e-6, atol=1e-8), (pname, prm.grad.cpu(), g_ref)
        checked += 1
    assert checked == 3 + 2 * len(DECOMP)

    # ---- eval mode
    with torch.no_grad():
        Pd = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in P.items()}
        kd = {k: v.detach() for k, v in kern.items()}
        K, ytil = K.detach(), ytil.detach()
        Xs = 2 * torch.rand(ns, d, dtype=torch.float64) - 1
        Ks, Kss = _latent_K(kd, X, Xs, q), _latent_K(kd, Xs, Xs, q)
        sol = torch.linalg.solve(K, Ks)
        mu_lat = (sol * ytil.unsqueeze(-1)).sum(1)                                    # (q, ns)
        cov_lat = Kss - Ks.transpose(-1, -2) @ sol
        Ht = pj.lmc_coefficients(Pd)
        mean_ref = mu_lat.T @ Ht
        var_ref = torch.diagonal(cov_lat, dim1=-2, dim2=-1).T @ (Ht * Ht) + Pd["eps"]
        Lf = pj.full_noise_factor(Pd)
        Kinv = torch.linalg.inv(K)
        kdiag = torch.diagonal(Kinv, dim1=-2, dim2=-1)
        alpha = (Kinv @ ytil.unsqueeze(-1)).squeeze(-1)
    m.eval(); m.likelihood.eval()
    with torch.no_grad():
        dist = m(Xs.to(DEV))
        obs = m.full_likelihood()(dist)
        lat = m.compute_latent_distrib(Xs.to(DEV), full_cov=True)
        s2, r = m.compute_loo()
    assert torch.allclose(dist.mean.cpu(), mean_ref, rtol=1e-8, atol=1e-10)
    assert torch.allclose(dist.variance.cpu(), var_ref, rtol=1e-7, atol=1e-10)
    assert torch.allclose(obs.variance.cpu(), var_ref + torch.diagonal(Lf @ Lf.T)[None, :], rtol=1e-7, atol=1e-10)
    assert torch.allclose(lat.mean.cpu(), mu_lat, rtol=1e-8, atol=1e-10)
    assert torch.allclose(lat.covariance_matrix.cpu(), cov_lat, rtol=1e-7, atol=1e-10)
    assert torch.allclose(s2.cpu(), (1.0 / kdiag).T, rtol=1e-8, atol=0)
    assert torch.allclose(r.cpu(), (alpha / kdiag).T, rtol=1e-8, atol=1e-12)


# ------------------------------------------------------------------------------------------------ 6. inherited machinery
def test_decomp_second_eval_call_hits_the_prediction_cache(plmc):
    """On the model of tests/test_gpu_prediction_cache.py (eager mode: the first call builds, the second hits)."""
    from projectedlmc import settings
    X, Y = _data(300, 3, 5, seed=4)
    m = perturb_(_decomp_model(plmc, X, Y, 2).double()).to(DEV)
    m.eval(); m.likelihood.eval()
    Xs = (2 * torch.rand(40, 3, dtype=torch.float64) - 1).to(DEV)
    with settings.prediction_cache("eager"), torch.no_grad():
        a = m(Xs)
        c = m._prediction_cache()
        assert (c.hits, c.misses) == (0, 1) and c.ws is not None and c.ws.with_inverse
        b = m(Xs)
        assert (c.hits, c.misses) == (1, 1)
        with settings.prediction_cache("off"):
            plain = m(Xs)
    assert torch.allclose(a.mean, b.mean, rtol=1e-9, atol=1e-11) and torch.allclose(a.variance, b.variance, rtol=1e-8, atol=1e-11)
    assert torch.allclose(a.mean, plain.mean, rtol=1e-9, atol=1e-11) and torch.allclose(a.variance, plain.variance, rtol=1e-8, atol=1e-11)


def test_decomp_latent_shards_sum_to_the_unsharded_loss_and_gradients(plmc):
    """tests/test_gpu_projected.py:251-253 (1e-10 / 1e-8): the table is sliced by latent_ids like ell is."""
    n, d, p, q, world = 300, 3, 6, 3, 2
    X, Y = _data(n, d, p, seed=21)
    Xd, Yd = X.to(DEV), Y.to(DEV)

    def build(shard):
        m = perturb_(_decomp_model(plmc, X, Y, q, seed=2, latent_shard=shard).double()).to(DEV)
        m.train(); m.likelihood.train()
        return m, plmc.ProjectedLMCmll(m.likelihood, m)

    m0, mll0 = build(None)
    loss0 = -mll0(m0(Xd), Yd)
    loss0.backward()
    total, grads = 0.0, None
    for rank in range(world):
        m1, mll1 = build((rank, world))
        share = -mll1(m1(Xd), Yd)
        share.backward()
        total = total + float(share.detach())
        gs = [torch.zeros_like(prm) if prm.grad is None else prm.grad.clone() for prm in m1.parameters()]
        grads = gs if grads is None else [a + b for a, b in zip(grads, gs)]
    assert abs(total - float(loss0)) < 1e-10 * abs(float(loss0)), (total, float(loss0))
    for (name, prm), g in zip(m0.named_parameters(), grads):
        assert torch.allclose(prm.grad, g, rtol=1e-8, atol=1e-11), (name, (prm.grad - g).abs().max())


def test_table_at_the_noise_floor_walks_the_jitter_ladder(eng):
    """The input of tests/test_gpu_jitter_ladder.py as a sum of two one-dimensional RBF components: fp32, n = 300 points on
    U(-1, 1)^2, lengthscales 5, noise e^-40.  That it needs jitter is a property of the input, checked on the host first (an fp32
    LAPACK Cholesky fails without jitter and succeeds at a rung <= 1e-1).  Under cholesky_max_tries(8) the log-prob and its gradients
    end finite, with the reference's warning for every rung walked."""
    n, q = 300, 2
    g = torch.Generator().manual_seed(3)
    X = (2 * torch.rand(n, 2, generator=g, dtype=torch.float64) - 1).float()
    y = torch.randn(q, n, generator=g, dtype=torch.float64).float()
    inf = float("inf")
    ell = torch.tensor([[5.0, inf], [inf, 5.0]]).expand(q, 2, 2).contiguous()
    osc = torch.ones(q, 2)
    noise = torch.full((q,), math.exp(-40.0))
    K = sum(gm.kernel_matrix("rbf", X[:, [k]], X[:, [k]], torch.full((q, 1), 5.0), None) for k in (0, 1))
    eye = torch.eye(n)
    ok = lambda jit: not bool(torch.linalg.cholesky_ex(K + (math.exp(-40.0) + jit) * eye)[1].any())
    assert K.dtype == torch.float32 and not ok(0.0) and any(ok(1e-6 * 10 ** i) for i in range(6))
    ell_d = ell.to(DEV).requires_grad_()
    with eng.settings.cholesky_max_tries(8), warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        lp = eng.exact.exact_latent_log_prob("rbf", X.to(DEV), ell_d, osc.to(DEV), noise.to(DEV), y.to(DEV))
        lp.sum().backward()
        torch.cuda.synchronize()
    jit = [str(w.message) for w in rec if "not p.d." in str(w.message)]
    base = eng.settings.cholesky_jitter.value(torch.float32)
    assert 1 <= len(jit) <= 8
    assert jit == ["A not p.d., added jitter of %.1e to the diagonal" % (base * 10 ** i) for i in range(len(jit))], jit
    assert all(issubclass(w.category, RuntimeWarning) for w in rec if "not p.d." in str(w.message))
    assert bool(torch.isfinite(lp).all()) and bool(torch.isfinite(ell_d.grad).all())
