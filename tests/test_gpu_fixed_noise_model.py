"""Per-point observation noise at the engine and the model level (FixedNoiseGaussianLikelihood) against the dense fp64
reference tests/_fixed_noise_ref.py, at the tolerances tests/test_gpu_engine.py applies to the same quantities (ref.check_*).
n = 200 throughout (two block rows, the last tile straddled), d = 3, q = 3; n = 250 where a fantasy must cross the 256 edge."""
import copy
import warnings

import pytest
import torch

import _fixed_noise_ref as ref
from _bridge import perturb_

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N, D, Q, NS = 200, 3, 3, 40
NAME = "FixedNoiseGaussianLikelihood"
DTYPES = pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])


@pytest.fixture(autouse=True)
def _nothing_more_after_a_gpu_error():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("HIP error, nothing more is started: %s" % e, returncode=3)


@pytest.fixture(scope="module", autouse=True)
def _release_what_the_module_holds():
    yield
    import gc
    from projectedlmc import _engine
    _engine.free_workspaces()
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def eng():
    from projectedlmc import _engine
    assert torch.cuda.is_available()
    return _engine


def _rounded(dtype, *ts):
    """the values the device sees, in fp64 for the reference"""
    return tuple(None if t is None else t.to(dtype).double() for t in ts)


# ------------------------------------------------------------------------------------------- 1. exactly representable noise
@DTYPES
def test_constant_vector_equals_the_homoskedastic_call_bit_for_bit(eng, dtype):
    """noise 0.25 and a constant vector 0.5 on a unit-diagonal kind without an output scale: 1 + 0.25 + 0.5 and 1 + 0.75 are both exact,
    so value and every gradient are the homoskedastic call's at noise 0.75, as bit patterns."""
    X, y, ell, _, _, _ = ref.problem(N, D, Q, seed=1)
    f = lambda t: t.to(DEV, dtype)

    def run(noise, s):
        Xd, ed, nd, yd = f(X).requires_grad_(), f(ell).requires_grad_(), f(noise).requires_grad_(), f(y).requires_grad_()
        sd = None if s is None else f(s).requires_grad_()
        lp = eng.exact_latent_log_prob("matern52", Xd, ed, None, nd, yd, pnoise=sd)
        lp.sum().backward()
        torch.cuda.synchronize()
        return lp.detach(), Xd.grad, ed.grad, nd.grad, yd.grad, (None if sd is None else sd.grad)

    want = run(torch.full((Q,), 0.75, dtype=torch.float64), None)
    for s in (torch.full((Q, N), 0.5, dtype=torch.float64), torch.full((N,), 0.5, dtype=torch.float64)):
        got = run(torch.full((Q,), 0.25, dtype=torch.float64), s)
        for a, b, name in zip(got[:5], want[:5], ("log-prob", "d/dX", "d/d ell", "d/d noise", "d/dy")):
            assert torch.equal(a, b), (name, float((a - b).abs().max()))
        assert got[5].shape == s.shape
        total = got[5].sum(-1) if s.dim() == 2 else got[5].sum().reshape(1)
        ref.check_gradient(total, want[3].cpu().double() if s.dim() == 2 else want[3].cpu().double().sum().reshape(1), dtype, "sum_i d/ds_i vs d/d noise")


# ------------------------------------------------------------------------------------------- 2. varying noise
@DTYPES
@pytest.mark.parametrize("shared", [False, True], ids=["per-latent", "shared"])
@pytest.mark.parametrize("kind", ["matern52", "rq", "poly2"])
def test_log_prob_and_gradients_against_the_dense_reference(eng, kind, shared, dtype):
    X, y, ell, osc, noise, s = ref.problem(N, D, Q, seed=3, shared=shared)
    table = ref.table_of(kind, ell)
    x_grad = kind != "poly2"                                  # (a dot-product kernel has no input gradient on the engine)
    Xr, yr, tr, orr, nr, sr = _rounded(dtype, X, y, table, osc, noise, s)
    w = torch.linspace(0.5, 1.5, Q, dtype=torch.float64)
    want_lp, want = ref.gradients(kind, Xr, tr, orr, nr, sr, yr, weights=w, wrt_x=x_grad)
    f = lambda t: t.to(DEV, dtype)
    Xd = f(X).requires_grad_(x_grad)
    td, od, nd, yd, sd = (f(t).requires_grad_() for t in (table, osc, noise, y, s))
    lp = eng.exact_latent_log_prob(kind, Xd, td, od, nd, yd, pnoise=sd)
    (lp * w.to(DEV, dtype)).sum().backward()
    torch.cuda.synchronize()
    ref.check_log_prob(lp, want_lp, dtype)
    for name, got in (("table", td.grad), ("oscale", od.grad), ("noise", nd.grad), ("y", yd.grad), ("s", sd.grad)) + ((("X", Xd.grad),) if x_grad else ()):
        print("%s %s d/d %s: err %.3e of %.3e" % (kind, dtype, name, float((got.cpu().double() - want[name]).abs().max()), float(want[name].abs().max())))
        ref.check_gradient(got, want[name], dtype, "d/d " + name)


def test_nothing_is_allocated_for_a_vector_without_a_graph(eng):
    """the kinv_diag buffer exists only when the vector requires a gradient: the saved tensors of the node say so"""
    X, y, ell, osc, noise, s = ref.problem(N, D, Q, seed=3)
    f = lambda t: t.to(DEV)
    for with_graph in (False, True):
        ed, yd = f(ell).requires_grad_(), f(y).requires_grad_()       # (the targets keep the node in the graph in the two-node form too)
        sd = f(s).requires_grad_(with_graph)
        lp = eng.exact_latent_log_prob("matern52", f(X), ed, f(osc), f(noise), yd, pnoise=sd)
        node = lp.grad_fn
        while node is not None and "ExactLatentLogProb" not in type(node).__name__:
            node = next((fn for fn, _ in node.next_functions if fn is not None and "ExactLatentLogProb" in type(fn).__name__), None)
        assert node is not None and (node.saved_tensors[3] is not None) == with_graph
        lp.sum().backward()
        assert ed.grad is not None and (sd.grad is not None) == with_graph


# ------------------------------------------------------------------------------------------- models
def _build(dtype, X, Y, s, extra=True, kernel="matern", batch=True):
    """an ExactGPModel with a FixedNoiseGaussianLikelihood on host tensors; Y (n, p) with batch, (n) without"""
    import projectedlmc as plmc
    p = Y.shape[1] if batch else 1
    torch.manual_seed(0)
    lik = plmc.FixedNoiseGaussianLikelihood(s.to(dtype), learn_additional_noise=extra, batch_shape=torch.Size([p]) if batch else torch.Size())
    kw = {"matern": dict(kernel_type=plmc.MaternKernel), "rq": dict(kernel_type=plmc.RQKernel),
          "poly2": dict(kernel_type=plmc.PolynomialKernel, ker_kwargs={"power": 2})}[kernel]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = plmc.ExactGPModel(X.to(dtype), Y.to(dtype), lik, n_tasks=p, outputscales=True, mean_type=plmc.ZeroMean, **kw)
    return perturb_(m.to(dtype), scale=0.1)


def _data(n, p, seed=5, shared=False):
    g = torch.Generator().manual_seed(seed)
    X = 2 * torch.rand(n, D, generator=g, dtype=torch.float64) - 1
    Y = torch.stack([torch.sin(2.0 * X[:, 0] + k) * torch.cos(X[:, 1] - X[:, 2]) for k in range(p)], 1)
    Y = Y + 0.1 * torch.randn(n, p, generator=g, dtype=torch.float64)
    Xs = 2 * torch.rand(NS, D, generator=g, dtype=torch.float64) - 1
    u = torch.rand(n, generator=g, dtype=torch.float64) if shared else torch.rand(p, n, generator=g, dtype=torch.float64)
    s = torch.pow(10.0, -3 + 4 * u)
    return X, Y, Xs, s


def _ref_inputs(model, kind):
    """(table, oscale, additional noise) of a model as fp64 host tensors, detached"""
    with torch.no_grad():
        lazy = model.covar_module(model.train_inputs[0])
        return lazy.ell.double().cpu(), lazy.oscale.double().cpu(), model._latent_noise().double().cpu()


def _moments(model, Xs, full_cov=False):
    with torch.no_grad():
        out = model(Xs, full_cov=True) if full_cov else model(Xs)
        return out.mean.clone(), out.variance.clone(), (out.covariance_matrix.clone() if full_cov else None)


def _want(model, X, Y, s, Xs, kind="matern52"):
    table, osc, noise = _ref_inputs(model, kind)
    f = lambda t: t.to(model.train_inputs[0].dtype).double().cpu()
    return ref.posterior(kind, f(X), table, osc, noise, f(s), f(Y).T, f(Xs))


# ------------------------------------------------------------------------------------------- 3. predictions, every cache route
def test_predictions_on_the_miss_the_build_and_the_hit_and_a_new_vector_is_a_new_key():
    from projectedlmc import settings
    dtype = torch.float64
    X, Y, Xs, s = _data(N, Q)
    model = _build(dtype, X, Y, s).to(DEV).eval()
    Xd = Xs.to(DEV)
    want = _want(model, X, Y, s, Xs)
    c = model._prediction_cache()
    with settings.prediction_cache("lazy"):
        ref.check_moments(*_moments(model, Xd, full_cov=True), *want)            # a plain miss: nothing is kept
        assert (c.hits, c.misses) == (0, 1) and c.ws is None
    with settings.prediction_cache("eager"):
        model.clear_prediction_cache()
        ref.check_moments(*_moments(model, Xd), *want)                           # the eager build
        assert c.ws is not None and c.hits == 0
        ref.check_moments(*_moments(model, Xd, full_cov=True), *want)            # a hit
        assert c.hits == 1
        misses = c.misses
        # a replaced vector: a miss, and the new vector's predictions
        s2 = s.flip(-1).contiguous()
        model.likelihood.noise = s2.to(DEV)
        ref.check_moments(*_moments(model, Xd), *_want(model, X, Y, s2, Xs))
        assert c.misses == misses + 1 and c.hits == 1
        ref.check_moments(*_moments(model, Xd), *_want(model, X, Y, s2, Xs))
        assert c.hits == 2
        # edited in place: a miss again
        model.likelihood.noise.mul_(3.0)
        ref.check_moments(*_moments(model, Xd), *_want(model, X, Y, 3.0 * s2, Xs))
        assert c.misses == misses + 2 and c.hits == 2
        # the mean-only route and the input derivatives see the vector too
        with settings.skip_posterior_variances(True), torch.no_grad():
            mean = model(Xd).mean
        assert torch.allclose(mean.cpu(), _want(model, X, Y, 3.0 * s2, Xs)[0], rtol=1e-8, atol=1e-10)


def test_fp32_cache_hit_on_the_kept_planes_sees_the_vector():
    """fp32: the eager build keeps the split engine's planes and the hit substitutes on them with eig_lo = noise + min_i s_i.  Build and
    hit against the fp64 reference at the fp32 tolerance of the cached predictions (2e-4 of the largest value, ref.FANTASY_TOL)."""
    from projectedlmc import settings
    dtype = torch.float32
    X, Y, Xs, s = _data(N, Q)
    model = _build(dtype, X, Y, s).to(DEV).eval()
    mu, cov = _want(model, X, Y, s, Xs)
    c = model._prediction_cache()
    with settings.prediction_cache("eager"):
        built = _moments(model, Xs.to(DEV, dtype))
        assert c.ws is not None and c.ws.keep_planes and c.hits == 0
        hit = _moments(model, Xs.to(DEV, dtype))
        assert c.hits == 1
    for got, tag in ((built, "build"), (hit, "hit")):
        ref.check_fantasy(got[0], mu, dtype, tag + " mean")
        ref.check_fantasy(got[1], torch.diagonal(cov, dim1=1, dim2=2), dtype, tag + " variance")


def test_input_gradients_of_the_predictions_see_the_vector():
    """x.requires_grad_() and predictive_gradients against autograd through the reference posterior"""
    dtype = torch.float64
    X, Y, Xs, s = _data(N, Q)
    model = _build(dtype, X, Y, s).to(DEV).eval()
    table, osc, noise = _ref_inputs(model, "matern52")
    xr = Xs.clone().requires_grad_()
    mu, cov = ref.posterior("matern52", X, table, osc, noise, s, Y.T, xr)
    var = torch.diagonal(cov, dim1=1, dim2=2)
    wm, wv = torch.linspace(0.5, 1.5, Q, dtype=dtype)[:, None], torch.linspace(1.5, 0.5, Q, dtype=dtype)[:, None]
    ((mu * wm).sum() + (var * wv).sum()).backward()
    xd = Xs.to(DEV).requires_grad_()
    out = model(xd)
    ((out.mean * wm.to(DEV)).sum() + (out.variance * wv.to(DEV)).sum()).backward()
    ref.check_gradient(xd.grad, xr.grad, dtype, "d (mean, var) / dx")
    Jm, Jv = model.predictive_gradients(Xs.to(DEV))                              # (ns, q, d)
    gm_ = torch.autograd.functional.jacobian(lambda x: ref.posterior("matern52", X, table, osc, noise, s, Y.T, x)[0].sum(-1), Xs[:5])
    assert Jm.shape == (NS, Q, D)
    # d mean_l(x_j) / d x_j: the diagonal blocks of the reference Jacobian of sum_s mean_l(x_s)
    ref.check_gradient(Jm[:5].transpose(0, 1), gm_, dtype, "predictive_gradients, mean")


# ------------------------------------------------------------------------------------------- 4. test-point noise
def test_test_point_noise_keyword_and_the_warning():
    dtype = torch.float64
    X, Y, Xs, s = _data(N, Q)
    for extra in (True, False):
        model = _build(dtype, X, Y, s, extra=extra).to(DEV).eval()
        lik = model.likelihood
        with torch.no_grad():
            latent = model(Xs.to(DEV))
            t = (0.1 + torch.rand(Q, NS, dtype=dtype)).to(DEV)
            add = lik.second_noise.reshape(Q, 1) if extra else 0.0
            assert torch.allclose(lik(latent, noise=t).variance, latent.variance + add + t, rtol=1e-12, atol=0)
            with pytest.warns(UserWarning, match="only the additional noise"):
                got = lik(latent).variance
            assert torch.allclose(got, latent.variance + add, rtol=1e-12, atol=0)
            assert torch.equal(lik(latent, noise=t).mean, latent.mean)


# ------------------------------------------------------------------------------------------- 5. fantasies
@pytest.fixture(autouse=True)
def _eager_cache(request):
    from projectedlmc import settings
    if "fantasy" in request.node.name:
        with settings.prediction_cache("eager"):
            yield
    else:
        yield


def _refit(dtype, base, X, Y, s):
    m = _build(dtype, X, Y, s).to(DEV).eval()
    m.load_state_dict(base.state_dict())
    return m


@DTYPES
@pytest.mark.parametrize("n,m", [(200, 1), (200, 5), (250, 10)])
def test_fantasy_model_equals_the_refit_on_the_concatenated_data(n, m, dtype):
    X, Y, Xs, s = _data(n + m, Q, seed=6)
    f = lambda t: t.to(DEV, dtype)
    base = _build(dtype, X[:n], Y[:n], s[:, :n]).to(DEV).eval()
    _moments(base, f(Xs))
    assert base._prediction_cache().ws is not None
    with pytest.raises(ValueError, match="needs noise="):
        base.get_fantasy_model(f(X[n:]), f(Y[n:]))
    fant = base.get_fantasy_model(f(X[n:]), f(Y[n:]), noise=f(s[:, n:]))
    assert torch.equal(fant.likelihood.noise, f(s)) and fant.train_inputs[0].shape[0] == n + m
    c = fant._prediction_cache()
    assert c.ws is not None and c.ws.n == n + m
    got = _moments(fant, f(Xs), full_cov=True)
    assert (c.hits, c.misses) == (1, 0), (c.hits, c.misses)                      # the extension, not a refit, produced them
    refit = _refit(dtype, base, X, Y, s)
    want = _moments(refit, f(Xs), full_cov=True)
    assert refit._prediction_cache().misses == 1
    for a, b, name in zip(got, want, ("mean", "variance", "full_cov")):
        ref.check_fantasy(a, b, dtype, "n=%d m=%d %s vs refit" % (n, m, name))
    if dtype == torch.float64:
        table, osc, noise = _ref_inputs(base, "matern52")
        mu, cov = ref.bordered_posterior("matern52", X[:n], table, osc, noise, s[:, :n], Y[:n].T, X[n:], s[:, n:], Y[n:].T, Xs)
        ref.check_fantasy(got[0], mu, dtype, "mean vs the bordered reference")
        ref.check_fantasy(got[1], torch.diagonal(cov, dim1=1, dim2=2), dtype, "variance vs the bordered reference")
        ref.check_fantasy(got[2], cov, dtype, "full_cov vs the bordered reference")


@DTYPES
def test_fantasy_of_a_fantasy(dtype):
    n, m = 200, 7
    X, Y, Xs, s = _data(n + m, Q, seed=7, shared=True)                           # one vector shared by the tasks
    f = lambda t: t.to(DEV, dtype)
    base = _build(dtype, X[:n], Y[:n], s[:n]).to(DEV).eval()
    _moments(base, f(Xs))
    one = base.get_fantasy_model(f(X[n:]), f(Y[n:]), noise=f(s[n:]))
    two = base.get_fantasy_model(f(X[n:n + 3]), f(Y[n:n + 3]), noise=f(s[n:n + 3])).get_fantasy_model(f(X[n + 3:]), f(Y[n + 3:]), noise=f(s[n + 3:]))
    a, b = _moments(one, f(Xs)), _moments(two, f(Xs))
    c = two._prediction_cache()
    assert (c.hits, c.misses) == (1, 0) and c.ws.n == n + m and torch.equal(two.likelihood.noise, f(s))
    ref.check_fantasy(b[0], a[0], dtype, "mean")
    ref.check_fantasy(b[1], a[1], dtype, "variance")
    want = _moments(_refit(dtype, base, X, Y, s), f(Xs))
    ref.check_fantasy(b[0], want[0], dtype, "mean vs refit")
    ref.check_fantasy(b[1], want[1], dtype, "variance vs refit")


# ------------------------------------------------------------------------------------------- 6. batched model: loss, gradients, moments
@DTYPES
@pytest.mark.parametrize("shared", [False, True], ids=["vector-(p,n)", "vector-(n)"])
@pytest.mark.parametrize("kernel,kind", [("matern", "matern52"), ("rq", "rq"), ("poly2", "poly2")])
def test_batched_model_loss_gradients_and_moments(kernel, kind, shared, dtype):
    import projectedlmc as plmc
    X, Y, Xs, s = _data(N, Q, seed=8, shared=shared)
    host = _build(dtype, X, Y, s, kernel=kernel)
    model = copy.deepcopy(host).to(DEV).train()
    sd = s.to(DEV, dtype).requires_grad_()
    model.likelihood.noise = sd
    Xd, Yd = model.train_inputs[0], model.train_targets
    mll = plmc.ExactMarginalLogLikelihood(model.likelihood, model)
    loss = -mll(model(Xd), Yd.T if Yd.shape[0] != Q else Yd).sum()
    loss.backward()
    # the reference: the same parameters through the host copy's own transforms, the density in fp64
    ref_model = copy.deepcopy(host).double()
    sr = s.to(dtype).double().requires_grad_()
    lazy = ref_model.covar_module(ref_model.train_inputs[0])
    noise = ref_model.likelihood.additional_noise(Q, lazy.ell)
    lp = ref.log_prob(kind, X.to(dtype).double(), lazy.ell, lazy.oscale, noise, sr, Y.to(dtype).double().T)
    want_loss = -(lp / N).sum()
    want_loss.backward()
    ref.check_log_prob(loss.reshape(1), want_loss.detach().reshape(1), dtype)
    ref.check_gradient(sd.grad, sr.grad, dtype, "d loss / d vector")
    want = dict(ref_model.named_parameters())
    seen = 0
    for name, p_ in model.named_parameters():
        if want[name].grad is None:
            assert p_.grad is None or not p_.grad.any(), name
            continue
        seen += 1
        ref.check_gradient(p_.grad, want[name].grad, dtype, "d loss / d " + name)
    assert seen >= 3                                                             # lengthscales (or variances), output scale, additional noise
    if dtype == torch.float64:
        model.eval()
        model.likelihood.noise = sd.detach()
        table, osc, nz = _ref_inputs(model, kind)
        ref.check_moments(*_moments(model, Xs.to(DEV), full_cov=True), *ref.posterior(kind, X, table, osc, nz, s, Y.T, Xs))


def test_single_output_model():
    """targets (n), no batch: loss, the vector's gradient and the moments"""
    import projectedlmc as plmc
    dtype = torch.float64
    X, Y, Xs, s = _data(N, 1, seed=9, shared=True)
    host = _build(dtype, X, Y[:, 0], s, batch=False)
    model = copy.deepcopy(host).to(DEV).train()
    sd = s.to(DEV).requires_grad_()
    model.likelihood.noise = sd
    mll = plmc.ExactMarginalLogLikelihood(model.likelihood, model)
    loss = -mll(model(model.train_inputs[0]), model.train_targets)
    loss.backward()
    table, osc, nz = _ref_inputs(model, "matern52")
    sr = s.clone().requires_grad_()
    want = -ref.log_prob("matern52", X, table, osc, nz, sr, Y.T).sum() / N
    want.backward()
    ref.check_log_prob(loss.reshape(1), want.detach().reshape(1), dtype)
    ref.check_gradient(sd.grad, sr.grad, dtype, "d loss / d vector")
    model.eval()
    mean, var, cov = _moments(model, Xs.to(DEV), full_cov=True)
    assert mean.shape == (NS,) and cov.shape == (NS, NS)
    mu, wc = ref.posterior("matern52", X, table, osc, nz, s, Y.T, Xs)
    ref.check_moments(mean[None], var[None], cov[None], mu, wc)


# ------------------------------------------------------------------------------------------- 7. a noise model
@DTYPES
def test_a_parametric_noise_model_is_trained_through_the_marginal_likelihood(dtype):
    """s = softplus(a + b x_0): a.grad and b.grad after loss.backward() against fp64 autograd through the reference"""
    import projectedlmc as plmc
    X, Y, Xs, s0 = _data(N, Q, seed=10, shared=True)
    host = _build(dtype, X, Y, s0)
    model = copy.deepcopy(host).to(DEV).train()
    a = torch.tensor(-1.0, dtype=dtype, device=DEV, requires_grad=True)
    b = torch.tensor(0.7, dtype=dtype, device=DEV, requires_grad=True)
    Xd = model.train_inputs[0]
    model.likelihood.noise = torch.nn.functional.softplus(a + b * Xd[:, 0])
    mll = plmc.ExactMarginalLogLikelihood(model.likelihood, model)
    loss = -mll(model(Xd), model.train_targets.T if model.train_targets.shape[0] != Q else model.train_targets).sum()
    loss.backward()
    table, osc, nz = _ref_inputs(model, "matern52")
    ar = torch.tensor(-1.0, dtype=torch.float64, requires_grad=True)
    br = torch.tensor(0.7, dtype=torch.float64, requires_grad=True)
    Xr = X.to(dtype).double()
    sr = torch.nn.functional.softplus(ar + br * Xr[:, 0])
    want = -(ref.log_prob("matern52", Xr, table, osc, nz, sr, Y.to(dtype).double().T) / N).sum()
    want.backward()
    ref.check_log_prob(loss.reshape(1), want.detach().reshape(1), dtype)
    got, exp = torch.stack([a.grad, b.grad]), torch.stack([ar.grad, br.grad])
    print("noise model %s: (a.grad, b.grad) = %s, reference %s" % (dtype, got.tolist(), exp.tolist()))
    ref.check_gradient(got, exp, dtype, "(a.grad, b.grad)")


# ------------------------------------------------------------------------------------------- 8. refusals on the device
def test_device_side_refusals_name_the_class(eng):
    import projectedlmc as plmc
    from projectedlmc import settings
    dtype = torch.float64
    X, Y, Xs, s = _data(N, Q)
    model = _build(dtype, X, Y, s).to(DEV)
    lik = model.likelihood
    Xd = model.train_inputs[0]
    with pytest.raises(NotImplementedError, match=NAME):
        lik(model(Xd)).rsample()
    with pytest.raises(NotImplementedError, match=NAME):
        model.compute_loo()
    with pytest.raises(NotImplementedError, match=NAME):
        plmc.LeaveOneOutPseudoLikelihood(lik, model)
    model.eval()
    with pytest.raises(NotImplementedError, match=NAME):
        model.sample_paths(2)
    with settings.posterior_hyper_grad(True), pytest.raises(NotImplementedError, match=NAME):
        model(Xs.to(DEV))
    # the engine itself refuses a vector under the differentiable-prediction setting instead of dropping it
    f = lambda t: t.to(DEV)
    _, y, ell, osc, noise, sv = ref.problem(N, D, Q, seed=1)
    with settings.posterior_hyper_grad(True), pytest.raises(NotImplementedError, match=NAME):
        eng.exact_posterior("matern52", Xd, f(ell).requires_grad_(), f(osc), f(noise), f(y), f(Xs), pnoise=f(sv))
    with pytest.raises(ValueError, match="per-point noise is"):
        eng.exact_posterior("matern52", Xd, f(ell), f(osc), f(noise), f(y), f(Xs), pnoise=f(sv)[:, :50])
