"""Whole inducing-point models at the sizes that are run (the reference's real-data experiments use 500 inducing points; the variational
models train_ind_ratio = 1.5): ExactGPModel(n_inducing_points in {129, 500}) on n = 600 points, RBF (d = 8) and Matern-5/2 (d = 3), with and
without an output scale, fp64 and fp32; VariationalMultitaskGPModel at m = 400 in fp32.
tests/test_gpu_sgpr.py and tests/test_gpu_inducing_additive.py run the same models at m = 25 / 30 in fp64: one 128-block.

References: oracle/sgpr.py, oracle/variational.py in fp64 on the CPU at the fp32-rounded parameters.  Tolerances:
those of tests/_inducing_fn_ref.py -- 4 sqrt(max(m, n)) kappa u of the largest entry for every output, kappa the larger of K_ZZ's and
B's (B = I + A A^T / s), and for the fp32 tensor outputs E32_RATIO x the error of the dense fp32 CPU run (profiles/inducing_accuracy.md).
In fp32 with jitter 0 `_factorize_kzz` hands eig_lo = 0 to the split engine: these are the cases that measure it."""
import warnings

import pytest
import torch

import _inducing_fn_ref as ifr
from oracle import gp_math as gm
from oracle import projected as pj
from oracle import sgpr as osg
from test_gpu_inducing_functions import check, E32_RATIO          # noqa: F401 (one checker, one constant)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
KERNEL_OF = {"rbf": "RBFKernel", "matern52": "MaternKernel"}


@pytest.fixture(autouse=True)
def _nothing_more_after_a_gpu_error():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("HIP error, nothing more is started: %s" % e, returncode=3)


def _set(prm, value):
    prm.copy_(value.to(prm.dtype).reshape(prm.shape))


@pytest.mark.parametrize("dtype", [F64, F32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("case", ifr.SGPR_MODEL_CASES, ids=ifr.case_id)
def test_exact_gp_sgpr_at_real_data_sizes(case, dtype):
    """MLL incl. the added trace term, the gradients of the inducing locations, lengthscale, output scale and noise, the eval-mode mean
    and variance at 25 points and the full_cov covariance"""
    import projectedlmc as plmc
    X, y, Xs, Z, raw_ls, raw_os, raw_nz = ifr.sgpr_model_inputs(case)
    ref, kap, e32 = ifr.sgpr_model_reference(case)
    bnd = ifr.bound(case.m, case.n, kap, dtype)
    if dtype == F64:
        e32 = (None,) * len(e32)
    lik = plmc.GaussianLikelihood()
    model = plmc.ExactGPModel(X.to(dtype), y[0].to(dtype), lik, mean_type=plmc.ZeroMean, kernel_type=getattr(plmc, KERNEL_OF[case.kind]),
                              outputscales=case.oscale, n_inducing_points=case.m)
    model, lik = model.to(dtype), lik.to(dtype)
    base = model.covar_module.base_kernel
    with torch.no_grad():
        _set(model.covar_module.inducing_points, Z)
        _set((base.base_kernel if case.oscale else base).raw_lengthscale, raw_ls)
        if case.oscale:
            _set(base.raw_outputscale, raw_os)
        _set(lik.noise_covar.raw_noise, raw_nz)
    model, lik = model.to(DEV), lik.to(DEV)
    model.train(); lik.train()
    out = plmc.ExactMarginalLogLikelihood(lik, model)(model(model.train_inputs[0]), model.train_targets).sum()
    out.backward()
    label = "sgpr model %s" % ifr.case_id(case)
    grads = (model.covar_module.inducing_points.grad, (base.base_kernel if case.oscale else base).raw_lengthscale.grad,
             base.raw_outputscale.grad if case.oscale else None, lik.noise_covar.raw_noise.grad)
    assert len(list(model.parameters())) == (4 if case.oscale else 3)
    check(label, "mll", out.reshape(()), ref[0], bnd, dtype)
    for name, g, r, e in zip(("gZ", "gEll", "gOs", "gNoise"), grads, ref[1:5], e32[1:5]):
        if r is None:
            assert g is None
            continue
        check(label, name, g.reshape(r.shape), r, bnd, dtype, e if name in ("gZ", "gEll") else None)
    model.eval(); lik.eval()
    with torch.no_grad():
        pred = model(Xs.to(DEV, dtype))
        full = model(Xs.to(DEV, dtype), full_cov=True)
    mu, cov = ref[5], ref[6]
    check(label, "mean", pred.mean.reshape(mu.shape), mu, bnd, dtype, e32[5])
    check(label, "var", pred.variance.reshape(1, -1), torch.diagonal(cov, dim1=-2, dim2=-1), bnd, dtype, e32[6])
    check(label, "full mean", full.mean.reshape(mu.shape), mu, bnd, dtype, e32[5])
    check(label, "full cov", full.covariance_matrix.reshape(cov.shape), cov, bnd, dtype, e32[6])


def _projected_case(plmc, n, d, p, q, m, ell, dtype):
    """(model on the CPU, X, Y, oracle loss, oracle mean and variance at X[:10], kappa): the recipe of
    test_gpu_sgpr.py::test_projected_model_with_inducing_points with fp32-representable data"""
    from test_gpu_sgpr import oracle_params_like
    g = torch.Generator().manual_seed(2)
    X = ifr.r32(2 * torch.rand(n, d, generator=g, dtype=F64) - 1)
    Y = ifr.r32(torch.randn(n, p, generator=g, dtype=F64))
    Z = ifr.r32(2 * torch.rand(m, d, generator=g, dtype=F64) - 1)
    torch.manual_seed(1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = plmc.ProjectedGPModel(X.to(dtype), Y.to(dtype), p, q, mean_type=plmc.ZeroMean, kernel_type=plmc.MaternKernel,
                                      init_lmc_coeffs=True, BDN=True, scalar_B=True, diagonal_B=True, n_inducing_points=m).to(dtype)
    with torch.no_grad():
        model.covar_module.inducing_points.copy_(Z.to(dtype))
        model.covar_module.base_kernel.raw_lengthscale.fill_(float(gm.inv_softplus(ell)))
    sd = model.state_dict()
    P = dict(oracle_params_like(model, sd))
    Zr = sd["covar_module.inducing_points"].double().cpu()
    ytil = pj.project_data(P, Y)
    ell_r, nz = pj.lengthscale(P), pj.projected_noise(P)
    lp, tr = osg.sgpr_terms("matern", X, Zr, ell_r, nz, ytil)
    terms, const = pj.projection_terms(P, Y)
    loss = ((lp + tr).sum() / n + sum(terms) + const).detach().reshape(())
    mu_lat, cov_lat = osg.sgpr_posterior("matern", X, Zr, ell_r, nz, ytil, X[:10])
    Ht = pj.lmc_coefficients(P)
    cov = sum(torch.kron(cov_lat[i], torch.outer(Ht[i], Ht[i])) for i in range(q)) + P["eps"] * torch.eye(10 * p, dtype=F64)
    return model, X, Y, loss, mu_lat.T @ Ht, torch.diagonal(cov).reshape(10, p), ifr.sgpr_kappa("matern52", X, Zr, ell_r, None, nz)


def test_projected_model_with_500_inducing_points_fp32():
    """the loss and the eval prediction against the oracle mix of test_gpu_sgpr.py::test_projected_model_with_inducing_points, at the
    real-data size in fp32 (q = 2, p = 4, Matern-5/2, d = 3, lengthscale 0.15 as in the qualifying table)"""
    import projectedlmc as plmc
    n, d, p, q, m = 600, 3, 4, 2, 500
    model, X, Y, loss, mean_ref, var_ref, kap = _projected_case(plmc, n, d, p, q, m, 0.15, F32)
    bnd = ifr.bound(m, n, kap, F32)
    print("kappa %.3g bound %.3g" % (kap, bnd))
    assert bnd < ifr.FP32_CAP, (kap, bnd)
    model = model.to(DEV)
    model.train()
    # (the model's own train_targets are zeros, as in the reference: the data go in here)
    val = plmc.ProjectedLMCmll(model.likelihood, model)(model(model.train_inputs[0]), Y.float().to(DEV))
    check("projected m=500", "loss", val.reshape(()), loss, bnd, F32)
    model.eval()
    with torch.no_grad():
        pred = model(X[:10].float().to(DEV))
    check("projected m=500", "mean", pred.mean, mean_ref, bnd, F32)
    check("projected m=500", "var", pred.variance, var_ref, bnd, F32)


def test_variational_model_at_400_inducing_points_fp32():
    """n = 600, train_ind_ratio = 1.5 -> m = 400, RBF, d = 8, lengthscales about 0.7 (the initial value, perturbed): the ELBO within the
    BASELINE fp32 tolerance and EVERY gradient inside the bound, with the builder, oracle and checker of
    test_gpu_variational.py::test_elbo_and_all_gradients_fp32 (the plain-kernel twin of test_gpu_inducing_additive.py's)"""
    import projectedlmc as plmc
    from test_gpu_variational import _build, _oracle_elbo
    n, d, p, q = 600, 8, 4, 2
    X, Y, model, lik = _build(plmc, n, d, p, q, "RBFKernel", False, F32, seed=3)
    ref, sd = _oracle_elbo(model, lik, X, Y, "rbf", 2.5, 1e-4)
    ref.backward()
    Z = sd["variational_strategy.base_variational_strategy.inducing_points"].detach()
    m = Z.shape[0]
    assert m == 400
    ell = gm.softplus(sd["covar_module.raw_lengthscale"].detach()).reshape(q, -1)
    kap = ifr.kappa(gm.kernel_matrix("rbf", Z, Z, ell, None) + 1e-4 * torch.eye(m, dtype=F64))
    bnd = ifr.bound(m, n, kap, F32)
    print("kappa %.3g bound %.3g" % (kap, bnd))
    assert bnd < ifr.FP32_CAP, (kap, bnd)
    model, lik = model.to(DEV), lik.to(DEV)
    model.train(); lik.train()
    out = plmc.VariationalELBO(lik, model, num_data=n)(model(X.to(DEV)), Y.to(DEV))
    out.backward()
    assert abs(float(out.detach()) - float(ref.detach())) < 1e-4 * abs(float(ref.detach())), (float(out), float(ref))
    named = dict(list(model.named_parameters()) + [("lik." + k, v) for k, v in lik.named_parameters()])
    seen = set()
    for name, leaf in sd.items():
        if leaf.grad is None:
            continue
        got, ref_g = named[name].grad.cpu().double(), leaf.grad
        if name.endswith("chol_variational_covar"):
            got, ref_g = got.tril(), ref_g.tril()
        check("variational m=400", name, got, ref_g, bnd, F32)
        seen.add(name)
    assert {"variational_strategy.base_variational_strategy.inducing_points", "covar_module.raw_lengthscale"} <= seen
