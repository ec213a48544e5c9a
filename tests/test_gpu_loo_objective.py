"""Leave-one-out objective on the GPU: the gradient product's entry points against the K^-1 + gradient kernels they share their
epilogues with (identity Xop = W, beta = alpha), the operand kernel, `exact_loo_log_prob` value and every gradient in fp64 and fp32 for
every covariance family of the batched exact engine, and `LeaveOneOutPseudoLikelihood` on models.

Reference: tests/_loo_dense.py (dense fp64, autograd).  Sizes: n = 130 (a second tile with 2 live rows) and n = 300 (3 block rows,
padding inside the last), q in {1, 3}, noise in [0.05, 0.2].  Bounds: fp64 value 1e-10 relative, gradients 1e-8 of the group's largest
magnitude; fp32 value 1e-4 relative, dL/dy 2e-3 of max |u| (the project's bounds); the fp32 hyper-parameter gradients are measured
against the cancellation scale sum_ij |G_ij| |dKhat_ij / dtheta| and compared with the same figure of the MLL gradient on the same
inputs: r_loo <= 8 max(r_mll, 16 2^-24) (profiles/loo_accuracy.md has the measured figures)."""
import math

import pytest
import torch

import _loo_dense as ld

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# (family, keyword arguments of _loo_dense.problem): plain (matern52 d = 3, rbf d = 9, spline d = 2), additive (G = 2, d = 3),
# spectral mixture (M = 2, d in {1, 2}), periodic (d in {1, 2})
FAMILIES = [("plain", dict(kind="matern52", d=3)), ("plain", dict(kind="rbf", d=9)), ("plain", dict(kind="spline", d=2)),
            ("additive", dict(kind="matern52", G=2, d=3)), ("sm", dict(M=2, d=1)), ("sm", dict(M=2, d=2)),
            ("periodic", dict(d=1)), ("periodic", dict(d=2))]
IDS = ["matern52-d3", "rbf-d9", "spline-d2", "additive-G2-d3", "sm-d1", "sm-d2", "periodic-d1", "periodic-d2"]


@pytest.fixture(scope="module")
def eng():
    import types
    from projectedlmc import _hip, _engine
    assert torch.cuda.is_available()
    return types.SimpleNamespace(hip=_hip, exact=_engine)


def _factorised(eng, prob, dt):
    """Factorise on the device and run plmc_kinv_grad*_vd_* with Kinv and kinv_diag: (ws, device tensors, table (q, w) fp64, Kinv, kd)."""
    ex, hip = eng.exact, eng.hip
    L = hip.lib()
    f = lambda t: t.to(DEV, dt).contiguous()
    X, ell, osc, noise, y = (f(prob[k]) for k in ("X", "ell", "osc", "noise", "y"))
    kind = prob["kind"]
    q, n = y.shape
    d = X.shape[1]
    ws = ex.get_workspace(n, q, 1, dt, DEV, True, ex.n_components(ell, kind), ex.is_sm(ell), kind == ex.PER)
    st = hip.stream_ptr(DEV)
    ex.factorize_checked(kind, X, ell, osc, noise, y.reshape(q, 1, n), ws)
    L.call("plmc_extract_col", dt, hip.ptr(ws.A), ws.n_pad, ws.lda, ws.strideA, 0, hip.ptr(ws.z), hip.ptr(ws.quad), q, st)
    L.call("plmc_wt_matvec", dt, hip.ptr(ws.W), ws.n_pad, ws.ldw, ws.strideW, hip.ptr(ws.z), hip.ptr(ws.alpha), q, st)
    table = torch.empty(q, ex.grad_table_width(ell, kind), dtype=torch.float64, device=DEV)
    ldk = ws.n_pad + ws.NB
    Kinv = torch.full((q, ws.n_pad, ldk), float("nan"), dtype=dt, device=DEV)
    kd = torch.empty(q, ws.n_pad, dtype=dt, device=DEV)
    ex._kernel_call(L, "plmc_kinv_grad_vd", dt, (ex.kind_code(kind), hip.ptr(ws.W), ws.n_pad, ws.ldw, ws.strideW, hip.ptr(ws.alpha),
                    hip.ptr(X), n, d), ell, (hip.ptr(osc), hip.ptr(table), hip.ptr(Kinv), ldk, ws.n_pad * ldk, hip.ptr(kd),
                    hip.ptr(ws.partials), q, hip.ptr(noise), hip.ptr(ws.Vd), st))
    torch.cuda.synchronize()
    return ws, (X, ell, osc, noise, y), table, Kinv, kd


def _loo_grad(eng, prob, dt, ws, dev, Xop, krows, beta):
    ex, hip = eng.exact, eng.hip
    X, ell, osc = dev[0], dev[1], dev[2]
    kind = prob["kind"]
    q, n, d = ell.shape[0], X.shape[0], X.shape[1]
    table = torch.empty(q, ex.grad_table_width(ell, kind), dtype=torch.float64, device=DEV)
    ex._kernel_call(hip.lib(), "plmc_loo_grad", dt, (ex.kind_code(kind), hip.ptr(Xop), ws.n_pad, krows, Xop.shape[2], Xop.shape[1] * Xop.shape[2],
                    hip.ptr(beta), hip.ptr(X), n, d), ell, (hip.ptr(osc), hip.ptr(table), hip.ptr(ws.partials), q, hip.stream_ptr(DEV)))
    torch.cuda.synchronize()
    return table.cpu()


# ------------------------------------------------------------------------------------------------ 1. identity with the MLL gradient kernels
_F64_TABLES = {}


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n,q", [(130, 3), (300, 1)])
@pytest.mark.parametrize("family,kw", FAMILIES, ids=IDS)
def test_identity_with_the_inverse_factor_returns_the_mll_table(eng, family, kw, n, q, dt):
    """Xop = W (zeros above the diagonal, krows = n_pad), beta = alpha: the table of plmc_kinv_grad*_vd_* on the same factorisation.
    fp64: 1e-12 of the table's largest entry.  fp32: 2e-3 of it, against the fp64 table (the project's fp32 gradient bound)."""
    prob = ld.problem(family, n, q, seed=11, fp32=True, **kw)
    key = (IDS[FAMILIES.index((family, kw))], n, q)
    if dt == torch.float32 and key not in _F64_TABLES:                       # (a run of the fp32 case alone)
        ws, dev, want, _, _ = _factorised(eng, prob, torch.float64)
        _F64_TABLES[key] = want.cpu()
    ws, dev, want, _, _ = _factorised(eng, prob, dt)
    Xop = torch.tril(ws.W).contiguous()                                      # (q, n_pad, n_pad): W is lower triangular; what shares its buffer is not
    got = _loo_grad(eng, prob, dt, ws, dev, Xop, ws.n_pad, ws.alpha)
    if dt == torch.float64:
        _F64_TABLES[key] = want = want.cpu()
        tol = 1e-12
    else:
        want, tol = _F64_TABLES[key], 2e-3
    err = float((got - want).abs().max() / want.abs().max())
    print("identity %s n=%d q=%d %s: %.3e" % (key[0], n, q, "f64" if dt == torch.float64 else "f32", err))
    assert err <= tol, err


def test_bad_arguments_fail_before_any_launch(eng):
    hip = eng.hip
    L = hip.lib()
    dt = torch.float64
    t = torch.ones(256 * 256, dtype=dt, device=DEV)
    g = torch.zeros(8, dtype=torch.float64, device=DEV)
    st = hip.stream_ptr(DEV)
    ok = (0, hip.ptr(t), 128, 128, 128, 128 * 128, hip.ptr(t), hip.ptr(t), 100, 2, hip.ptr(t), None, hip.ptr(g), hip.ptr(t), 1, st)

    def bad(i, v, match):
        a = list(ok)
        a[i] = v
        with pytest.raises(RuntimeError, match=match):
            L.call("plmc_loo_grad", dt, *a)

    bad(1, None, "null pointer")
    bad(3, 120, "multiple of 16")
    bad(4, 64, "ldx")
    bad(2, 100, "plmc_pad")
    bad(0, 9, "unknown kernel kind")
    bad(1, hip._c.c_void_p(t.data_ptr() + 8), "unaligned")
    with pytest.raises(RuntimeError, match="krows"):
        L.call("plmc_loo_operand", dt, hip.ptr(t), 128, 128, 128 * 128, hip.ptr(t), hip.ptr(t), 64, 128, 128 * 128, 100, 1, st)
    with pytest.raises(RuntimeError, match="null pointer"):
        L.call("plmc_loo_operand", dt, hip.ptr(t), 128, 128, 128 * 128, None, hip.ptr(t), 128, 128, 128 * 128, 100, 1, st)
    L.call("plmc_loo_grad", dt, *ok)                                         # and the well-formed call goes through
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. the operand kernel
@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n,q", [(130, 3), (300, 1)])
def test_operand_kernel_mirrors_scales_and_zeroes(eng, n, q, dt):
    """Xop = rowscale o P mirrored from the stored upper triangle (bit for bit: one product per element), exact zeros in the rest of
    [0, krows) x [0, n_pad), nothing written behind krows; and P is the dense inverse."""
    hip = eng.hip
    prob = ld.problem("plain", n, q, seed=3, fp32=True, kind="matern52", d=3)
    ws, dev, _, Kinv, _ = _factorised(eng, prob, dt)
    n_pad, krows = ws.n_pad, ws.n_pad + 16
    g = torch.Generator().manual_seed(1)
    rowscale = (0.5 + torch.rand(q, n_pad, generator=g, dtype=torch.float64)).to(DEV, dt)
    Xop = torch.full((q, n_pad + 128, n_pad), 7.0, dtype=dt, device=DEV)
    hip.lib().call("plmc_loo_operand", dt, hip.ptr(Kinv), n_pad, Kinv.shape[2], n_pad * Kinv.shape[2], hip.ptr(rowscale), hip.ptr(Xop), krows,
                   n_pad, (n_pad + 128) * n_pad, n, q, hip.stream_ptr(DEV))
    torch.cuda.synchronize()
    U = torch.triu(Kinv[:, :n, :n])
    P = U + torch.triu(U, 1).transpose(-1, -2)
    assert torch.equal(Xop[:, :n, :n], rowscale[:, :n, None] * P)
    assert bool((Xop[:, :krows, n:] == 0).all()) and bool((Xop[:, n:krows, :] == 0).all())
    assert bool((Xop[:, krows:, :] == 7.0).all())
    dense = torch.linalg.inv(ld.khat(prob))
    tol = 1e-10 if dt == torch.float64 else 2e-3
    assert float((P.cpu().double() - dense).abs().max() / dense.abs().max()) <= tol


# ------------------------------------------------------------------------------------------------ 3. end to end
def _run(eng, prob, dt, w, fn=None):
    f = lambda t: t.to(DEV, dt)
    leaves = {k: f(prob[k]).requires_grad_() for k in ("ell", "osc", "noise", "y")}
    fn = eng.exact.exact_loo_log_prob if fn is None else fn
    val = fn(prob["kind"], f(prob["X"]), leaves["ell"], leaves["osc"], leaves["noise"], leaves["y"])
    (val * f(w)).sum().backward()
    torch.cuda.synchronize()
    return val.detach().cpu().double(), {k: v.grad.cpu().double() for k, v in leaves.items()}


_E2E = [(fam, kw, 130 if i % 2 == 0 else 300, 1) for i, (fam, kw) in enumerate(FAMILIES)] + \
       [("plain", dict(kind="matern52", d=3), 300, 3), ("additive", dict(kind="matern52", G=2, d=3), 130, 3)]
_E2E_IDS = ["%s-n%d-q%d" % (IDS[FAMILIES.index((fam, kw))], n, q) for fam, kw, n, q in _E2E]


@pytest.mark.parametrize("family,kw,n,q", _E2E, ids=_E2E_IDS)
def test_value_and_every_gradient_fp64(eng, family, kw, n, q):
    """Value to 1e-10 relative; every gradient group and dL/dy to 1e-8 of the group's largest magnitude."""
    prob = ld.problem(family, n, q, seed=n + q, **kw)
    w = torch.linspace(0.5, 1.5, q, dtype=torch.float64) if q > 1 else torch.ones(1, dtype=torch.float64)
    want, gwant = ld.reference(prob, weights=w)
    got, ggot = _run(eng, prob, torch.float64, w)
    rel = float(((got - want) / want).abs().max())
    print("fp64 %s n=%d q=%d: value %.2e" % (family, n, q, rel))
    assert rel <= 1e-10, rel
    for k in ("ell", "osc", "noise", "y"):
        assert ggot[k].shape == gwant[k].shape, k
        scale = float(gwant[k].abs().max())
        err = float((ggot[k] - gwant[k]).abs().max())
        print("    %s: %.2e of %.3e" % (k, err / scale if scale > 0 else err, scale))
        assert err <= 1e-8 * scale, (k, err, scale)
    if family == "additive":
        assert bool((ggot["ell"][torch.isinf(prob["ell"])] == 0).all())


def _ratio(got, want, S):
    """max over the hyper-parameters with a non-zero scale of |got - want| / S."""
    r = 0.0
    for k in ("ell", "osc", "noise"):
        live = S[k] > 0
        if bool(live.any()):
            r = max(r, float(((got[k] - want[k]).abs()[live] / S[k][live]).max()))
    return r


@pytest.mark.parametrize("family,kw,n,q", _E2E, ids=_E2E_IDS)
def test_value_and_every_gradient_fp32(eng, family, kw, n, q):
    """Value to 1e-4 relative, dL/dy to 2e-3 of max |u|.  Hyper-parameters: r_loo = max_theta |got - want| / sum_ij |G_ij| |dKhat_ij /
    dtheta| against r_mll, the same figure of exact_latent_log_prob's fp32 gradient on the same inputs with A = 1/2 (alpha alpha^T - P):
    r_loo <= 8 max(r_mll, 16 2^-24).  The margin: P diag(c) P carries P's error twice, and its product runs on the fp32 MFMA, whose
    error was measured at 2.2-3.3 times the split engine's."""
    from oracle import gp_math as gm
    prob = ld.problem(family, n, q, seed=n + q, fp32=True, **kw)
    w = torch.ones(q, dtype=torch.float64)
    want, gwant = ld.reference(prob, weights=w)
    got, ggot = _run(eng, prob, torch.float32, w)
    rel = float(((got - want) / want).abs().max())
    adj = ld.loo_adjoint(ld.khat(prob), prob["y"])
    ymax = float(adj["u"].abs().max())
    yerr = float((ggot["y"] - gwant["y"]).abs().max())
    r_loo = _ratio(ggot, gwant, ld.abs_scales(prob, adj["G"]))
    mwant, mgwant = ld.reference(prob, objective=gm.mvn_log_prob, weights=w)
    _, mggot = _run(eng, prob, torch.float32, w, fn=eng.exact.exact_latent_log_prob)
    A = 0.5 * (adj["alpha"].unsqueeze(-1) * adj["alpha"].unsqueeze(-2) - adj["P"])
    r_mll = _ratio(mggot, mgwant, ld.abs_scales(prob, A))
    print("fp32 %s n=%d q=%d: value %.2e  dL/dy %.2e of max|u|  r_loo %.3e  r_mll %.3e  ratio %.2f"
          % (_E2E_IDS[_E2E.index((family, kw, n, q))], n, q, rel, yerr / ymax, r_loo, r_mll, r_loo / max(r_mll, 16 * 2.0 ** -24)))
    assert rel <= 1e-4, rel
    assert yerr <= 2e-3 * ymax, (yerr, ymax)
    assert r_loo <= 8.0 * max(r_mll, 16 * 2.0 ** -24), (r_loo, r_mll)


# ------------------------------------------------------------------------------------------------ 4. models
def _perturb(model, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for prm in model.parameters():
            prm.add_(0.3 * torch.randn(prm.shape, generator=g, dtype=prm.dtype))


def _check_model(plmc, model, lik, X, Y, ref, leaves):
    ref.backward()
    model, lik = model.to(DEV), lik.to(DEV)
    model.train()
    lik.train()
    out = plmc.LeaveOneOutPseudoLikelihood(lik, model, X, Y)(model(X.to(DEV)), Y.to(DEV))
    assert out.shape == ref.shape, (out.shape, ref.shape)
    out.sum().backward()
    assert abs(float(out.sum()) - float(ref.sum())) <= 1e-9 * abs(float(ref.sum())), (float(out.sum()), float(ref.sum()))
    for name, prm in model.named_parameters():
        assert prm.grad is not None and leaves[name].grad is not None, name
        assert torch.allclose(prm.grad.cpu(), leaves[name].grad, rtol=1e-5, atol=1e-9), (name, prm.grad.cpu(), leaves[name].grad)


def test_model_single_task_matern_with_constant_mean():
    """ExactGPModel, Matern-5/2, ConstantMean: value = sum_i log N(y_i; mu_-i, s2_-i) / n (the reference's sum_i(term1 + term2) / n - 1/2
    log 2 pi), every raw-parameter gradient through the constraints; the mean's gradient is -sum(u) / n."""
    import projectedlmc as plmc
    from oracle import gp_math as gm
    g = torch.Generator().manual_seed(0)
    n, d = 150, 3
    X = 2 * torch.rand(n, d, generator=g, dtype=torch.float64) - 1
    y = torch.sin(2.0 * X.sum(-1)) + 0.2 * torch.randn(n, generator=g, dtype=torch.float64)
    lik = plmc.GaussianLikelihood()
    model = plmc.ExactGPModel(X, y, lik, mean_type=plmc.ConstantMean, kernel_type=plmc.MaternKernel, outputscales=True).double()
    _perturb(model, 1)
    leaves = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in model.named_parameters()}
    ell = gm.softplus(leaves["covar_module.base_kernel.raw_lengthscale"]).reshape(1, -1)
    os_ = gm.softplus(leaves["covar_module.raw_outputscale"]).reshape(1)
    noise = gm.softplus(leaves["likelihood.noise_covar.raw_noise"]).reshape(1) + 1e-4
    K = gm.kernel_matrix("matern", X, X, ell, os_, 2.5) + noise.reshape(1, 1, 1) * torch.eye(n, dtype=torch.float64)
    resid = (y - leaves["mean_module.raw_constant"].reshape(())).reshape(1, n)
    ref = ld.loo_log_prob(K, resid) / n
    u = ld.loo_adjoint(K.detach(), resid.detach())["u"]
    _check_model(plmc, model, lik, X, y, ref, leaves)
    assert abs(float(leaves["mean_module.raw_constant"].grad.sum()) + float(u.sum()) / n) <= 1e-9 * float(u.abs().sum()) / n
    term = ld.loo_adjoint(K.detach(), resid.detach())
    s2, r = 1.0 / term["p"], term["alpha"] / term["p"]
    formula = (-0.5 * s2.log() - 0.5 * r ** 2 / s2).sum(-1) / n - 0.5 * math.log(2.0 * math.pi)
    assert torch.allclose(formula, ref.detach(), rtol=1e-12, atol=0)


def test_model_three_independent_tasks_with_a_lengthscale_prior():
    """n_tasks = 3 under a MultitaskGaussianLikelihood (the independent-task MultitaskMultivariateNormal): the tasks are summed as log_prob
    sums them, the lengthscale prior is added once, num_data = n * 3."""
    import projectedlmc as plmc
    from oracle import gp_math as gm
    from oracle import priors as opr
    g = torch.Generator().manual_seed(2)
    n, d, p = 140, 2, 3
    X = 2 * torch.rand(n, d, generator=g, dtype=torch.float64) - 1
    Y = torch.randn(n, p, generator=g, dtype=torch.float64)
    ps = torch.linspace(0.4, 0.9, d, dtype=torch.float64)
    pw = torch.linspace(0.3, 0.5, d, dtype=torch.float64)
    lik = plmc.MultitaskGaussianLikelihood(num_tasks=p)
    model = plmc.ExactGPModel(X, Y, lik, n_tasks=p, prior_scales=ps, prior_width=pw, mean_type=plmc.ConstantMean,
                              kernel_type=plmc.RBFKernel).double()
    lik = lik.double()
    _perturb(model, 3)
    leaves = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in model.named_parameters()}
    ell = gm.softplus(leaves["covar_module.raw_lengthscale"]).reshape(p, d)
    noise = (gm.softplus(leaves["likelihood.raw_task_noises"]) + 1e-4) + (gm.softplus(leaves["likelihood.raw_noise"]) + 1e-4)
    K = gm.kernel_matrix("rbf", X, X, ell, None) + noise.reshape(p, 1, 1) * torch.eye(n, dtype=torch.float64)
    resid = Y.T - leaves["mean_module.raw_constant"].reshape(p, 1)
    ref = (ld.loo_log_prob(K, resid).sum() + opr.lengthscale_log_prior(ell, ps, pw)) / (n * p)
    _check_model(plmc, model, lik, X, Y, ref, leaves)


def test_model_with_an_additive_decomposition():
    import projectedlmc as plmc
    from oracle import gp_math as gm
    g = torch.Generator().manual_seed(4)
    n, d = 180, 3
    X = 2 * torch.rand(n, d, generator=g, dtype=torch.float64) - 1
    y = torch.randn(n, generator=g, dtype=torch.float64)
    decomp = [[0, 1], [1, 2]]
    lik = plmc.GaussianLikelihood()
    model = plmc.ExactGPModel(X, y, lik, mean_type=plmc.ConstantMean, kernel_type=plmc.MaternKernel, decomp=decomp).double()
    _perturb(model, 5)
    leaves = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in model.named_parameters()}
    K = torch.zeros(1, n, n, dtype=torch.float64)
    for gi, idx in enumerate(decomp):
        ell = gm.softplus(leaves["covar_module.kernels.%d.base_kernel.raw_lengthscale" % gi]).reshape(1, -1)
        os_ = gm.softplus(leaves["covar_module.kernels.%d.raw_outputscale" % gi]).reshape(1)
        K = K + gm.kernel_matrix("matern", X[:, idx], X[:, idx], ell, os_, 2.5)
    noise = gm.softplus(leaves["likelihood.noise_covar.raw_noise"]).reshape(()) + 1e-4
    resid = (y - leaves["mean_module.raw_constant"].reshape(())).reshape(1, n)
    ref = ld.loo_log_prob(K + noise * torch.eye(n, dtype=torch.float64), resid) / n
    _check_model(plmc, model, lik, X, y, ref, leaves)
