"""GPU parity of additive (`decomp`) kernels under inducing points: ExactGPModel(n_inducing_points) single and batched,
ProjectedGPModel(n_inducing_points) and VariationalMultitaskGPModel (whitened and unwhitened strategies), with the shapes and tolerances
of tests/test_gpu_sgpr.py and tests/test_gpu_variational.py.  The references are dense fp64 formulas on the CPU for the SUM of the
components (tests/_inducing_dense.py; each component is oracle.gp_math.kernel_matrix on its group's columns)."""
import math
import warnings

import pytest
import torch

import _inducing_dense as idn
from oracle import gp_math as gm
from oracle import projected as pj

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DECOMP = [[0, 1], [1, 2]]                    # d = 3: dimension 1 is shared, none is unused
KERNELS = {"MaternKernel": ("matern", 2.5), "RBFKernel": ("rbf", 2.5)}


def _data(n, d, p, seed):
    g = torch.Generator().manual_seed(seed)
    return (2 * torch.rand(n, d, generator=g, dtype=torch.float64) - 1, torch.randn(n, p, generator=g, dtype=torch.float64))


def _dense_kernel(leaves, prefix, kind, nu, q):
    """K(Xa, Xb) and the prior variance from the raw parameters `leaves[prefix + "kernels.<g>...."]` of an additive kernel."""
    ells = [gm.softplus(leaves[prefix + "kernels.%d.base_kernel.raw_lengthscale" % g]).reshape(q, -1) for g in range(len(DECOMP))]
    oss = [gm.softplus(leaves[prefix + "kernels.%d.raw_outputscale" % g]).reshape(q) for g in range(len(DECOMP))]
    return idn.additive_kernel(kind, nu, DECOMP, ells, oss), idn.prior_variance(oss, q)


def _set_kernel(add_kernel, seed):
    """lengthscales ~ 0.3-0.5 (a well-conditioned K_zz), output scales away from their initial value, different per sub-kernel and latent."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k in add_kernel.kernels:
            k.base_kernel.raw_lengthscale.copy_(-1.0 + 0.3 * torch.randn(k.base_kernel.raw_lengthscale.shape, generator=g, dtype=torch.float64))
            k.raw_outputscale.copy_(0.5 * torch.randn(k.raw_outputscale.shape, generator=g, dtype=torch.float64))


# ------------------------------------------------------------------------------------------------ ExactGPModel (SGPR)
@pytest.mark.parametrize("q", [1, 3], ids=["single", "batched"])
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_exact_gp_sgpr_with_decomp(kernel, q):
    """MLL incl. the added trace term (k(x, x) = sum_g os_g), the gradients of the inducing points, of every sub-kernel's raw_lengthscale
    and raw_outputscale and of the noise, and the eval-mode mean and variance at 25 points."""
    import projectedlmc as plmc
    kind, nu = KERNELS[kernel]
    n, d, m = 220, 3, 30
    X, Y = _data(n, d, q, 1)
    y = Y[:, 0].contiguous() if q == 1 else Y.T.contiguous()
    torch.manual_seed(4)
    lik = plmc.GaussianLikelihood() if q == 1 else plmc.GaussianLikelihood(batch_shape=torch.Size([q]))
    model = plmc.ExactGPModel(X, y, lik, n_tasks=q, mean_type=plmc.ZeroMean, kernel_type=getattr(plmc, kernel), decomp=DECOMP,
                              n_inducing_points=m)
    model, lik = model.double(), lik.double()
    with torch.no_grad():
        model.covar_module.inducing_points.copy_(2 * torch.rand(m, d, dtype=torch.float64) - 1)
    _set_kernel(model.covar_module.base_kernel, 8)
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in model.named_parameters()}
    assert len(leaves) == 1 + 2 * len(DECOMP) + 1, sorted(leaves)              # Z, (ell, os) per sub-kernel, the noise
    K, kxx = _dense_kernel(leaves, "covar_module.base_kernel.", kind, nu, q)
    Z = leaves["covar_module.inducing_points"]
    nz = gm.softplus(leaves["likelihood.noise_covar.raw_noise"]).reshape(q) + 1e-4
    lp, tr = idn.sgpr_terms(K, kxx, X, Z, nz, y.reshape(q, n))
    ref = (lp + tr).sum() / n
    ref.backward()
    model, lik = model.to(DEV), lik.to(DEV)
    model.train(); lik.train()
    out = plmc.ExactMarginalLogLikelihood(lik, model)(model(X.to(DEV)), y.to(DEV)).sum()
    out.backward()
    out, ref = out.detach(), ref.detach()
    print("mll", float(out), float(ref))
    assert abs(float(out) - float(ref)) < 1e-8 * abs(float(ref)), (float(out), float(ref))
    for name, prm in model.named_parameters():
        err = (prm.grad.cpu() - leaves[name].grad).abs().max()
        print(name, float(err), float(leaves[name].grad.abs().max()))
        assert torch.allclose(prm.grad.cpu(), leaves[name].grad, rtol=1e-5, atol=1e-8), (name, float(err))
    Xs = 2 * torch.rand(25, d, dtype=torch.float64) - 1
    with torch.no_grad():
        mu, cov = idn.sgpr_posterior(K, X, Z, nz, y.reshape(q, n), Xs)
    model.eval(); lik.eval()
    with torch.no_grad():
        pred = model(Xs.to(DEV))
    assert torch.allclose(pred.mean.cpu().reshape(q, -1), mu, rtol=1e-6, atol=1e-8)
    assert torch.allclose(pred.variance.cpu().reshape(q, -1), torch.diagonal(cov, dim1=-2, dim2=-1), rtol=1e-5, atol=1e-8)
    assert len(model.lscales()) == 2 and model.outputscale().shape == (q, 2)


# ------------------------------------------------------------------------------------------------ ProjectedGPModel
def test_projected_model_with_inducing_points_and_decomp():
    """The loss, the eval-mode mean and variance and the full_cov covariance against the dense latent SGPR posteriors mixed as in
    test_gpu_sgpr.py::test_projected_model_with_inducing_points."""
    import projectedlmc as plmc
    kind, nu = "matern", 2.5
    n, d, p, q, m = 160, 3, 4, 2, 25
    X, Y = _data(n, d, p, 2)
    torch.manual_seed(1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = plmc.ProjectedGPModel(X, Y, p, q, mean_type=plmc.ZeroMean, kernel_type=plmc.MaternKernel, init_lmc_coeffs=True, BDN=True,
                                      scalar_B=True, diagonal_B=True, decomp=DECOMP, n_inducing_points=m).double()
    with torch.no_grad():
        model.covar_module.inducing_points.copy_(2 * torch.rand(m, d, dtype=torch.float64) - 1)
    _set_kernel(model.covar_module.base_kernel, 9)
    sd = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
    lb = model.likelihood.noise_covar.raw_noise_constraint.lower_bound
    P = dict(kind=kind, nu=nu, n_tasks=model.n_tasks, n_latents=model.n_latents, mode=model.lmc_coefficients.mode, BDN=True, eps=model.eps,
             scalar_B=True, diagonal_B=True, noise_lb=lb, noise_thresh=math.log(lb), H=sd["lmc_coefficients.H"],
             raw_noise=sd["likelihood.noise_covar.raw_noise"], raw_lengthscale=None, raw_outputscale=None,
             log_B_tilde=sd["parametrizations.log_B_tilde.original"])
    K, kxx = _dense_kernel(sd, "covar_module.base_kernel.", kind, nu, q)
    Z = sd["covar_module.inducing_points"]
    ytil = pj.project_data(P, Y)
    lp, tr = idn.sgpr_terms(K, kxx, X, Z, pj.projected_noise(P), ytil)
    terms, const = pj.projection_terms(P, Y)
    ref = float((lp + tr).sum() / n + sum(terms) + const)
    model = model.to(DEV)
    model.train()
    val = float(plmc.ProjectedLMCmll(model.likelihood, model)(model(X.to(DEV)), Y.to(DEV)))
    assert abs(val - ref) < 1e-8 * abs(ref), (val, ref)
    model.eval()
    with torch.no_grad():
        pred = model(X[:10].to(DEV))
        full = model(X[:10].to(DEV), full_cov=True)
    mu_lat, cov_lat = idn.sgpr_posterior(K, X, Z, pj.projected_noise(P), ytil, X[:10])
    Ht = pj.lmc_coefficients(P)
    mean_ref = mu_lat.T @ Ht
    cov_ref = sum(torch.kron(cov_lat[i], torch.outer(Ht[i], Ht[i])) for i in range(q)) + P["eps"] * torch.eye(10 * p, dtype=torch.float64)
    assert torch.allclose(pred.mean.cpu(), mean_ref, rtol=1e-6, atol=1e-8)
    assert torch.allclose(pred.variance.cpu(), torch.diagonal(cov_ref).reshape(10, p), rtol=1e-5, atol=1e-8)
    assert torch.allclose(full.mean.cpu(), mean_ref, rtol=1e-6, atol=1e-8)
    assert torch.allclose(full.lazy_covariance_matrix.evaluate().cpu(), cov_ref, rtol=1e-5, atol=1e-8)


# ------------------------------------------------------------------------------------------------ VariationalMultitaskGPModel
def _build_variational(plmc, n, d, p, q, kernel, dtype, ratio, seed=0, ker_kwargs=None):
    g = torch.Generator().manual_seed(seed)
    X = (2 * torch.rand(n, d, generator=g, dtype=torch.float64) - 1).to(dtype)
    Y = torch.randn(n, p, generator=g, dtype=torch.float64).to(dtype)
    torch.manual_seed(seed)
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        lik = plmc.MultitaskGaussianLikelihood(num_tasks=p, rank=2)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            model = plmc.VariationalMultitaskGPModel(X, n_latents=q, n_tasks=p, train_ind_ratio=ratio, seed=0, init_lmc_coeffs=True,
                                                     train_y=Y, mean_type=plmc.ConstantMean, kernel_type=getattr(plmc, kernel),
                                                     decomp=DECOMP, ker_kwargs=ker_kwargs)
    finally:
        torch.set_default_dtype(old)
    return X, Y, model, lik


def _perturb(model, lik, seed):
    g2 = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, prm in list(model.named_parameters()) + list(lik.named_parameters()):
            prm.add_(0.1 * torch.randn(prm.shape, generator=g2, dtype=torch.float64).to(prm.dtype))


def _oracle_elbo(model, lik, X, Y, kind, nu, jitter, whitened):
    sd = {k: v.detach().cpu().double().clone().requires_grad_(True) for k, v in
          list(model.named_parameters()) + [("lik." + k, v) for k, v in lik.named_parameters()]}
    b = "variational_strategy.base_variational_strategy."
    q = model.n_latents
    K, kxx = _dense_kernel(sd, "covar_module.", kind, nu, q)
    F = sd["lik.task_noise_covar_factor"]
    noise_diag = (F * F).sum(-1) + gm.softplus(sd["lik.raw_noise"]).reshape(()) + 1e-4
    Z = sd[b + "inducing_points"] if whitened else model.base_variational_strategy.inducing_points.detach().cpu().double()
    val = idn.variational_elbo(K, kxx, X.double(), Y.double(), Z, sd[b + "_variational_distribution.variational_mean"],
                               sd[b + "_variational_distribution.chol_variational_covar"], sd["variational_strategy.lmc_coefficients"],
                               noise_diag, sd["variational_strategy.output_mean_module.raw_constant"], jitter, X.shape[0], whitened=whitened)
    return val, sd, K


def _compare_gradients(model, lik, sd, check):
    named = dict(list(model.named_parameters()) + [("lik." + k, v) for k, v in lik.named_parameters()])
    seen = set()
    for name, leaf in sd.items():
        if leaf.grad is None:
            continue
        got = named[name].grad
        assert got is not None, name
        got, ref_g = got.cpu().double(), leaf.grad
        if name.endswith("chol_variational_covar"):
            got, ref_g = got.tril(), ref_g.tril()
        print(name, float((got - ref_g).abs().max()), float(ref_g.abs().max()))
        check(name, got, ref_g)
        seen.add(name)
    for g in range(len(DECOMP)):                        # every sub-kernel's lengthscales and output scale were compared
        assert "covar_module.kernels.%d.base_kernel.raw_lengthscale" % g in seen and "covar_module.kernels.%d.raw_outputscale" % g in seen
    return seen


def _allclose_fp64(name, got, ref_g):
    assert torch.allclose(got, ref_g, rtol=2e-5, atol=1e-8), (name, float((got - ref_g).abs().max()))


@pytest.mark.parametrize("kernel,ker_kwargs", [pytest.param("RBFKernel", None, id="RBFKernel"),
                                               pytest.param("MaternKernel", None, id="MaternKernel"),
                                               pytest.param("MaternKernel", {"nu": 0.5}, id="MaternKernel-nu0.5")])
def test_whitened_elbo_and_all_gradients_fp64(kernel, ker_kwargs):
    """Shapes and tolerances of test_gpu_variational.py::test_elbo_and_all_gradients_fp64, d = 3 with the overlapping decomposition."""
    import projectedlmc as plmc
    n, d, p, q = 150, 3, 4, 2
    X, Y, model, lik = _build_variational(plmc, n, d, p, q, kernel, torch.float64, 1.5, ker_kwargs=ker_kwargs)
    _perturb(model, lik, 1)
    model.base_variational_strategy.variational_params_initialized.fill_(1)
    kind, nu = ("rbf", 2.5) if kernel == "RBFKernel" else ("matern", (ker_kwargs or {}).get("nu", 2.5))
    ref, sd, _ = _oracle_elbo(model, lik, X, Y, kind, nu, 1e-6, True)
    ref.backward()
    model, lik = model.to(DEV), lik.to(DEV)
    model.train(); lik.train()
    out = plmc.VariationalELBO(lik, model, num_data=n)(model(X.to(DEV)), Y.to(DEV))
    out.backward()
    out, ref = out.detach(), ref.detach()
    print("elbo", float(out), float(ref))
    assert abs(float(out) - float(ref)) < 1e-9 * abs(float(ref)), (float(out), float(ref))
    seen = _compare_gradients(model, lik, sd, _allclose_fp64)
    assert "variational_strategy.base_variational_strategy.inducing_points" in seen
    assert model.base_variational_strategy.inducing_points.grad.abs().max() > 0


@pytest.mark.parametrize("kernel", ["RBFKernel", "MaternKernel"])
def test_unwhitened_elbo_and_all_gradients_fp64(kernel):
    """Shapes and tolerances of test_gpu_variational.py::test_unwhitened_elbo_and_all_gradients_fp64 (train_ind_ratio == 1), d = 3;
    the first call initialises q(u) to the prior of the SUM kernel, and an eval-mode prediction away from the inducing points uses
    k(x, x) = sum_g os_g."""
    import projectedlmc as plmc
    n, d, p, q = 140, 3, 3, 2
    X, Y, model, lik = _build_variational(plmc, n, d, p, q, kernel, torch.float64, 1.0)
    kind, nu = KERNELS[kernel]
    bvs = model.base_variational_strategy
    assert type(bvs).__name__ == "UnwhitenedVariationalStrategy"
    model, lik = model.to(DEV), lik.to(DEV)
    model.train(); lik.train()
    mll = plmc.VariationalELBO(lik, model, num_data=n)
    with torch.no_grad():
        mll(model(X.to(DEV)), Y.to(DEV))
    model, lik = model.cpu(), lik.cpu()
    K0, _ = _dense_kernel({k: v.detach().double() for k, v in model.named_parameters()}, "covar_module.", kind, nu, q)
    Ls0 = bvs._variational_distribution.chol_variational_covar.detach()
    assert torch.allclose(Ls0 @ Ls0.transpose(-1, -2), K0(X, X) + 1e-3 * torch.eye(n, dtype=torch.float64), rtol=1e-9, atol=1e-11)
    _perturb(model, lik, 5)
    ref, sd, K = _oracle_elbo(model, lik, X, Y, kind, nu, 1e-3, False)
    ref.backward()
    model, lik = model.to(DEV), lik.to(DEV)
    out = mll(model(X.to(DEV)), Y.to(DEV))
    out.backward()
    print("elbo", float(out.detach()), float(ref.detach()))
    assert abs(float(out.detach()) - float(ref.detach())) < 1e-9 * abs(float(ref.detach())), (float(out), float(ref))
    _compare_gradients(model, lik, sd, _allclose_fp64)
    # eval mode away from Z (tolerances of test_unwhitened_eval_predictions_fp64)
    g = torch.Generator().manual_seed(11)
    Xs = 2 * torch.rand(17, d, generator=g, dtype=torch.float64) - 1
    b = "variational_strategy.base_variational_strategy."
    with torch.no_grad():
        _, kxx = _dense_kernel(sd, "covar_module.", kind, nu, q)
        mean_f, var_f, _ = idn.unwhitened_latent_predictive(K, kxx, Xs, X, sd[b + "_variational_distribution.variational_mean"],
                                                            sd[b + "_variational_distribution.chol_variational_covar"], 1e-3)
        H = sd["variational_strategy.lmc_coefficients"]
        mu_ref = mean_f.T @ H + sd["variational_strategy.output_mean_module.raw_constant"].reshape(1, p)
        var_ref = var_f.T @ (H * H)
    model.eval()
    with torch.no_grad():
        dist = model(Xs.to(DEV))
    assert torch.allclose(dist.mean.cpu(), mu_ref, rtol=1e-8, atol=1e-10)
    assert torch.allclose(dist.variance.cpu(), var_ref, rtol=1e-7, atol=1e-10)


def test_whitened_elbo_and_all_gradients_fp32():
    """The fp32 case at the tolerances of test_gpu_variational.py::test_elbo_and_all_gradients_fp32 (its bound: 4 sqrt(L) kappa u of the
    largest entry of each gradient, kappa from the oracle's K_ZZ + jitter I of the sum kernel), n = 300, m = 200, d = 3."""
    import projectedlmc as plmc
    n, d, p, q = 300, 3, 4, 2
    X, Y, model, lik = _build_variational(plmc, n, d, p, q, "RBFKernel", torch.float32, 1.5, seed=3)
    # lengthscales ~ 0.12, below the spacing of 200 inducing points in the 2-d groups: kappa ~ 5e2 and the bound ~ 2e-3 of the largest
    # entry (at the initial lengthscale 0.69 kappa is 1e6 and the bound exceeds 1: it would say nothing)
    with torch.no_grad():
        for k in model.covar_module.kernels:
            k.base_kernel.raw_lengthscale.fill_(-2.1)
    _perturb(model, lik, 4)
    model.base_variational_strategy.variational_params_initialized.fill_(1)
    ref, sd, K = _oracle_elbo(model, lik, X, Y, "rbf", 2.5, 1e-4, True)
    ref.backward()
    Z = sd["variational_strategy.base_variational_strategy.inducing_points"].detach()
    m = Z.shape[0]
    assert m == 200
    with torch.no_grad():
        ev = torch.linalg.eigvalsh(K(Z, Z) + 1e-4 * torch.eye(m, dtype=torch.float64))
    kappa = float((ev[:, -1] / ev[:, 0]).max())
    tol = 4.0 * math.sqrt(max(m, n)) * kappa * 2.0 ** -24
    assert tol < 1e-2, (kappa, tol)
    model, lik = model.to(DEV), lik.to(DEV)
    model.train(); lik.train()
    out = plmc.VariationalELBO(lik, model, num_data=n)(model(X.to(DEV)), Y.to(DEV))
    out.backward()
    print("elbo", float(out.detach()), float(ref.detach()), "kappa", kappa, "tol", tol)
    assert abs(float(out.detach()) - float(ref.detach())) < 1e-4 * abs(float(ref.detach())), (float(out), float(ref))

    def check(name, got, ref_g):
        err, scale = float((got - ref_g).abs().max()), float(ref_g.abs().max())
        assert err <= tol * scale, (name, err / scale, tol, kappa)
    _compare_gradients(model, lik, sd, check)


# ------------------------------------------------------------------------------------------------ the plain path
def test_plain_path_is_unchanged(monkeypatch):
    """decomp=None: loss and gradients of an SGPR step are bit-identical between the model as built and the same step with
    `_factorize_kzz` / `kernel_vjp` forced down the direct plain library calls they made before they learned about tables."""
    import projectedlmc as plmc
    from projectedlmc import _hip, _var_engine
    from projectedlmc._pivot import PivotCheck
    n, d, m = 220, 3, 30
    X, Y = _data(n, d, 1, 1)
    y = Y[:, 0].contiguous()

    def step():
        torch.manual_seed(4)
        lik = plmc.GaussianLikelihood()
        model = plmc.ExactGPModel(X, y, lik, mean_type=plmc.ZeroMean, kernel_type=plmc.MaternKernel, outputscales=True, n_inducing_points=m)
        model, lik = model.double(), lik.double()
        with torch.no_grad():
            model.covar_module.inducing_points.copy_(2 * torch.rand(m, d, dtype=torch.float64) - 1)
            model.covar_module.base_kernel.base_kernel.raw_lengthscale.fill_(-1.0)
        model, lik = model.to(DEV), lik.to(DEV)
        model.train(); lik.train()
        out = plmc.ExactMarginalLogLikelihood(lik, model)(model(X.to(DEV)), y.to(DEV)).sum()
        out.backward()
        return out.detach().clone(), {k: v.grad.clone() for k, v in model.named_parameters()}

    calls = []

    def plain_factorize(kind, Z, ell, oscale, jitter, ws, rhs=None, X=None, eager=False):
        assert ell.dim() == 2
        calls.append("factorize")
        L = _hip.lib()
        dt, dev = ws.dtype, ws.device
        st = _hip.stream_ptr(dev)
        k = _hip.KIND[kind]
        mm, dd = Z.shape
        q = ws.q
        jit = torch.full((q,), float(jitter), dtype=dt, device=dev)
        L.call("plmc_assemble", dt, k, _hip.ptr(Z), mm, dd, _hip.ptr(ell), _hip.ptr(oscale), _hip.ptr(jit), _hip.ptr(ws.A), ws.lda,
               ws.strideA, q, st)
        if ws.naug_pad > 0:
            L.call("plmc_write_rhs", dt, _hip.ptr(rhs), 0 if rhs is None else rhs.shape[1], mm, _hip.ptr(ws.A), ws.lda, ws.strideA, 0,
                   ws.naug_pad, q, st)
        if X is not None:
            L.call("plmc_assemble_cross", dt, k, _hip.ptr(Z), mm, _hip.ptr(X), X.shape[0], dd, _hip.ptr(ell), _hip.ptr(oscale),
                   _hip.ptr(ws.A), ws.lda, ws.strideA, ws.n_pad, ws.n_pad, q, st)
        L.call("plmc_potrf_ex", dt, _hip.ptr(ws.A), ws.n_pad, ws.lda, ws.naug, ws.strideA, _hip.ptr(ws.Vd), _hip.ptr(ws.logdet),
               _hip.ptr(ws.info), int(ws.with_inverse), q, _hip.ptr(jit), st)
        return PivotCheck.eager(ws) if eager else PivotCheck(ws)

    def plain_vjp(kind, X1, X2, ell, oscale, G):
        assert ell.dim() == 2
        calls.append("vjp")
        L = _hip.lib()
        dt, dev = G.dtype, G.device
        q, n1, n2 = G.shape
        dd = X1.shape[1]
        G = G.contiguous()
        gX = torch.empty(q, n1, dd, dtype=torch.float64, device=dev)
        gE = torch.empty(q, n1, dd, dtype=torch.float64, device=dev)
        gO = torch.empty(q, n1, dtype=torch.float64, device=dev)
        L.call("plmc_kernel_vjp", dt, _hip.KIND[kind], _hip.ptr(X1), n1, _hip.ptr(X2), n2, dd, _hip.ptr(ell), _hip.ptr(oscale), _hip.ptr(G),
               n2, n1 * n2, _hip.ptr(gX), _hip.ptr(gE), _hip.ptr(gO), q, _hip.stream_ptr(dev))
        return gX.sum(0), gE.sum(1), gO.sum(1)

    loss_a, grads_a = step()
    monkeypatch.setattr(_var_engine, "_factorize_kzz", plain_factorize)
    monkeypatch.setattr(_var_engine, "kernel_vjp", plain_vjp)
    loss_b, grads_b = step()
    assert calls == ["factorize", "vjp", "vjp"], calls
    assert torch.equal(loss_a, loss_b)
    assert set(grads_a) == set(grads_b) and len(grads_a) == 4
    for name in grads_a:
        assert torch.equal(grads_a[name], grads_b[name]), name
