"""FixedNoiseGaussianLikelihood and per-point noise, the part that runs without a GPU: the class's semantics, every
ValueError, every refusal that fires before a device is needed (matched on the class name), the 32 new symbols and their argument
errors, and the dense reference tests/_fixed_noise_ref.py judged where nothing else judges it."""
import ctypes
import warnings

import pytest
import torch

import _fixed_noise_ref as ref
from oracle import gp_math as gm

NAME = "FixedNoiseGaussianLikelihood"
INFIXES = ("", "_add", "_sm", "_per", "_rq", "_lper", "_sum", "_dot")


def _plmc():
    import projectedlmc
    return projectedlmc


# ---- the class

def test_names_parameters_and_state_dict():
    plmc = _plmc()
    assert plmc.FixedNoiseGaussianLikelihood is plmc.likelihoods.FixedNoiseGaussianLikelihood
    s = torch.rand(7) + 0.1
    lik = plmc.FixedNoiseGaussianLikelihood(s)
    assert lik.noise is s and lik.noise_covar.noise is s
    assert list(lik.state_dict()) == [] and list(lik.parameters()) == []
    assert lik.second_noise_covar is None and lik.second_noise == 0.0
    lik2 = plmc.FixedNoiseGaussianLikelihood(s, learn_additional_noise=True)
    assert list(lik2.state_dict()) == ["second_noise_covar.raw_noise"]
    assert [n for n, _ in lik2.named_parameters()] == ["second_noise_covar.raw_noise"]
    assert tuple(lik2.second_noise_covar.raw_noise.shape) == (1,)
    assert torch.equal(lik2.second_noise, lik2.second_noise_covar.noise) and float(lik2.second_noise.detach()) > 0
    lik3 = plmc.FixedNoiseGaussianLikelihood(torch.rand(3, 7) + 0.1, learn_additional_noise=True, batch_shape=torch.Size([3]))
    assert tuple(lik3.second_noise_covar.raw_noise.shape) == (3, 1)
    t = torch.rand(7) + 0.2
    lik.noise = t
    assert lik.noise is t
    lik2.second_noise = 0.3
    assert abs(float(lik2.second_noise.detach()) - 0.3) < 1e-6
    with pytest.raises(RuntimeError):
        lik.second_noise = 0.3
    assert isinstance(lik, plmc.likelihoods._GaussianLikelihoodBase)       # ExactMarginalLogLikelihood accepts it


def test_the_vector_keeps_its_graph():
    plmc = _plmc()
    a = torch.zeros(1, requires_grad=True)
    s = torch.nn.functional.softplus(a + torch.arange(5.0))
    lik = plmc.FixedNoiseGaussianLikelihood(s)
    assert lik.noise.requires_grad and lik.noise.grad_fn is s.grad_fn
    import copy
    c = copy.deepcopy(lik)                                                  # a fantasy model copies its likelihood: values, no graph
    assert torch.equal(c.noise, s.detach()) and not c.noise.requires_grad


@pytest.mark.parametrize("bad", [torch.tensor([0.1, 0.0, 0.2]), torch.tensor([0.1, -1.0]), torch.tensor([0.1, float("nan")])])
def test_non_positive_values_are_value_errors(bad):
    plmc = _plmc()
    with pytest.raises(ValueError, match="non-positive"):
        plmc.FixedNoiseGaussianLikelihood(bad)
    lik = plmc.FixedNoiseGaussianLikelihood(torch.ones(bad.shape[0]))
    with pytest.raises(ValueError, match="non-positive"):
        lik.noise = bad


def test_batch_shape_that_disagrees_with_the_vector_is_a_value_error():
    plmc = _plmc()
    with pytest.raises(ValueError, match="batch_shape"):
        plmc.FixedNoiseGaussianLikelihood(torch.ones(3, 7), batch_shape=torch.Size([2]))
    with pytest.raises(ValueError, match="batch_shape"):
        plmc.FixedNoiseGaussianLikelihood(torch.ones(3, 7))
    with pytest.raises(ValueError, match="batch_shape"):
        plmc.FixedNoiseGaussianLikelihood(torch.tensor(1.0))
    plmc.FixedNoiseGaussianLikelihood(torch.ones(7), batch_shape=torch.Size([2]))       # one vector shared by the batch


def _model(n=9, d=2, p=None, lik=None, **kw):
    plmc = _plmc()
    g = torch.Generator().manual_seed(0)
    X = torch.rand(n, d, generator=g)
    y = torch.rand(n, generator=g) if p is None else torch.rand(n, p, generator=g)
    lik = lik if lik is not None else plmc.FixedNoiseGaussianLikelihood(torch.rand(n, generator=g) + 0.1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return plmc.ExactGPModel(X, y, lik, n_tasks=1 if p is None else p, **kw), X, y


def test_forward_records_the_vector_on_the_lazy_covariance():
    plmc = _plmc()
    model, X, y = _model()
    lik = model.likelihood
    out = lik(model(X))
    c = out.lazy_covariance_matrix
    assert c.pnoise is lik.noise and torch.equal(c.noise, torch.zeros(1))
    assert torch.allclose(out.variance, model(X).variance + lik.noise)
    t = torch.rand(9) + 0.5
    c2 = lik(model(X), noise=t).lazy_covariance_matrix
    assert c2.pnoise is t
    assert c2.add_noise(torch.ones(1)).pnoise is t                          # add_noise keeps it
    with pytest.raises(ValueError, match="noise= has 4 entries"):
        lik(model(X), noise=torch.ones(4))
    lik2 = plmc.FixedNoiseGaussianLikelihood(lik.noise, learn_additional_noise=True)
    c3 = lik2(model(X)).lazy_covariance_matrix
    assert torch.equal(c3.noise, lik2.second_noise.reshape(-1)) and c3.pnoise is lik.noise


def test_test_point_noise_on_a_dense_predictive_distribution():
    """likelihood(dist, noise=t): variance = latent variance + additional noise + t; without the keyword the warning fires and only the
    additional noise is added."""
    plmc = _plmc()
    s = torch.rand(9) + 0.1
    for extra in (False, True):
        lik = plmc.FixedNoiseGaussianLikelihood(s, learn_additional_noise=extra)
        add = float(lik.second_noise.detach()) if extra else 0.0
        v = torch.rand(4) + 0.3
        dist = plmc.MultivariateNormal(torch.zeros(4), torch.diag_embed(v))
        t = torch.rand(4) + 0.2
        assert torch.allclose(lik(dist, noise=t).variance, v + add + t)
        with pytest.warns(UserWarning, match="only the additional noise"):
            got = lik(dist).variance
        assert torch.allclose(got, v + add)
    lik = plmc.FixedNoiseGaussianLikelihood(torch.rand(2, 9) + 0.1, learn_additional_noise=True, batch_shape=torch.Size([2]))
    v = torch.rand(2, 4) + 0.3
    t = torch.rand(2, 4) + 0.2
    got = lik(plmc.MultivariateNormal(torch.zeros(2, 4), torch.diag_embed(v)), noise=t).variance
    assert torch.allclose(got, v + lik.second_noise.reshape(2, 1) + t)


def test_a_vector_that_does_not_fit_the_training_data_is_a_value_error_at_first_use():
    plmc = _plmc()
    model, X, y = _model(lik=plmc.FixedNoiseGaussianLikelihood(torch.ones(5)))
    with pytest.raises(ValueError, match="does not fit 9 training points"):
        model.eval()(torch.rand(3, 2))
    model, X, y = _model(p=3, lik=plmc.FixedNoiseGaussianLikelihood(torch.ones(2, 9), batch_shape=torch.Size([2])))
    with pytest.raises(ValueError, match="does not fit 9 training points"):
        model.eval()(torch.rand(3, 2))


def test_lazy_kernel_diagonal_and_shape_checks():
    model, X, y = _model()
    c = model(X).lazy_covariance_matrix
    with pytest.raises(ValueError, match="per-point noise is"):
        c.add_point_noise(torch.ones(4))
    with pytest.raises(ValueError, match="per-point noise is"):
        c.add_point_noise(torch.ones(2, 9))
    s = torch.rand(9)
    assert torch.allclose(c.add_point_noise(s).diagonal(), c.diagonal() + s)
    assert torch.allclose(c.add_point_noise(s).add_point_noise(s).pnoise, 2 * s)


# ---- refusals by name, before a device is needed (host tensors throughout)

def test_models_that_do_not_serve_it_refuse_at_construction():
    plmc = _plmc()
    g = torch.Generator().manual_seed(0)
    n, d, p = 12, 2, 3
    X, Y = torch.rand(n, d, generator=g), torch.rand(n, p, generator=g)
    lik = plmc.FixedNoiseGaussianLikelihood(torch.ones(n))
    with pytest.raises(NotImplementedError, match=NAME):
        plmc.ProjectedGPModel(X, Y, p, 2, proj_likelihood=lik)
    with pytest.raises(NotImplementedError, match=NAME):
        plmc.MultitaskGPModel(X, Y, lik, n_tasks=p, n_latents=2)
    with pytest.raises(NotImplementedError, match=NAME):
        plmc.ExactGPModel(X, Y[:, 0], lik, n_inducing_points=4)
    vm = plmc.VariationalMultitaskGPModel(X, 2, p, train_y=Y)
    with pytest.raises(NotImplementedError, match=NAME):
        plmc.VariationalELBO(lik, vm, num_data=n)


def test_objectives_and_methods_that_do_not_serve_it_refuse():
    plmc = _plmc()
    model, X, y = _model()
    lik = model.likelihood
    with pytest.raises(NotImplementedError, match=NAME):
        plmc.LeaveOneOutPseudoLikelihood(lik, model)
    with pytest.raises(NotImplementedError, match=NAME):
        model.compute_loo()
    model.eval()
    with pytest.raises(NotImplementedError, match=NAME):
        model.sample_paths(2)
    with plmc.settings.posterior_hyper_grad(True), pytest.raises(NotImplementedError, match=NAME):
        model(torch.rand(3, 2))
    with pytest.raises(NotImplementedError, match=NAME):
        lik(model.train()(X)).rsample()
    with pytest.raises(NotImplementedError, match=NAME):
        lik(model(X)).sample(torch.Size([2]))
    # the served paths on host tensors reach the device check
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        plmc.ExactMarginalLogLikelihood(lik, model)(model(X), y)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.eval()(torch.rand(3, 2))


def test_fantasy_noise_keyword():
    plmc = _plmc()
    model, X, y = _model()
    model.eval()
    with pytest.raises(ValueError, match="needs noise="):
        model.get_fantasy_model(torch.rand(2, 2), torch.rand(2))
    with pytest.raises(ValueError, match="does not continue"):
        model.get_fantasy_model(torch.rand(2, 2), torch.rand(2), noise=torch.ones(3))
    with pytest.raises(ValueError, match="non-positive"):
        model.get_fantasy_model(torch.rand(2, 2), torch.rand(2), noise=torch.zeros(2))
    homo, _, _ = _model(lik=plmc.GaussianLikelihood())
    with pytest.raises(ValueError, match="homoskedastic"):
        homo.eval().get_fantasy_model(torch.rand(2, 2), torch.rand(2), noise=torch.ones(2))


def test_engine_functions_check_the_vector_and_refuse_what_they_do_not_serve():
    from projectedlmc import _engine
    with pytest.raises(ValueError, match="per-point noise is"):
        _engine.point_noise(torch.ones(5), 2, 9, torch.float64)
    with pytest.raises(ValueError, match="per-point noise is"):
        _engine.point_noise(torch.ones(3, 9), 2, 9, torch.float64)
    assert _engine.point_noise(None, 2, 9, torch.float64) is None
    s = torch.rand(2, 9)
    assert torch.equal(_engine.noise_bound(torch.tensor([0.25, 0.5]), s), torch.tensor([0.25, 0.5]) + s.amin(-1))
    assert torch.equal(_engine.noise_bound(torch.tensor([0.25, 0.5]), s[0]), torch.tensor([0.25, 0.5]) + s[0].min())
    with pytest.raises(NotImplementedError, match="per-point noise"):
        _engine.refuse_point_noise("this path")
    with pytest.raises(ValueError, match="for neither"):
        _engine.extend_cached_factor("rbf", torch.rand(9, 2), torch.ones(1, 2), None, torch.ones(1), torch.rand(1, 9), torch.rand(2, 2), None, None,
                                     pnoise=torch.ones(9))


# ---- the library

def test_the_32_symbols_resolve_and_the_abi_version_is_unchanged():
    from projectedlmc import _hip
    lib = _hip.lib()
    assert lib.cdll.plmc_version() == 4
    names = set(_hip.exported_symbols())
    new = ["plmc_%s%s_%s" % (op, infix, tail) for op, tail in (("assemble", "pn"), ("factorize", "pn_ex")) for infix in INFIXES]
    assert len(new) == 16
    for base in new:
        for suf in ("_f32", "_f64"):
            assert base + suf in names
            getattr(lib.cdll, base + suf)


def test_null_vector_and_short_stride_are_argument_errors_without_a_launch():
    """This runs without a device: the refusal comes before anything is launched."""
    from projectedlmc import _hip
    cd = _hip.lib().cdll
    P = ctypes.c_void_p
    one = P(8)                  # never dereferenced
    n = 100
    # plmc_assemble_pn: kind, X, n, d, ell, oscale, noise, pnoise, stride_pn, A, lda, strideA, q, stream
    assert cd.plmc_assemble_pn_f64(3, one, n, 2, one, None, one, None, 0, one, 128, 128 * 128, 1, None) != 0
    assert b"null pointer" in cd.plmc_last_error() and b"plmc_assemble_pn_f64" in cd.plmc_last_error()
    for stride in (1, n - 1):
        assert cd.plmc_assemble_pn_f32(3, one, n, 2, one, None, one, one, stride, one, 128, 128 * 128, 1, None) != 0
        assert b"bad sizes" in cd.plmc_last_error()
    assert cd.plmc_assemble_rq_pn_f32(one, n, 2, one, one, None, one, None, 0, one, 128, 128 * 128, 1, None) != 0
    assert b"null pointer" in cd.plmc_last_error()
    # plmc_factorize_pn_ex: ..., noise, pnoise, stride_pn, A, n_pad, lda, naug, strideA, Vd, logdet, info, with_inverse, q, eig_lo, stream
    assert cd.plmc_factorize_pn_ex_f64(3, one, n, 2, one, None, one, None, 0, one, 128, 384, 1, 128 * 384, one, one, one, 1, 1, None, None) != 0
    assert b"null pointer" in cd.plmc_last_error() and b"plmc_factorize_pn_ex_f64" in cd.plmc_last_error()
    assert cd.plmc_factorize_dot_pn_ex_f32(one, n, 2, one, one, 2, None, one, one, n - 1, one, 128, 384, 1, 128 * 384, one, one, one, 1, 1, None, None) != 0
    assert b"bad sizes" in cd.plmc_last_error()


# ---- the reference, judged where nothing else judges it

def test_constant_vector_equals_the_oracle_at_noise_plus_c():
    n, d, q, c = 60, 3, 2, 0.37
    X, y, ell, osc, noise, _ = ref.problem(n, d, q, seed=4)
    Xs = 2 * torch.rand(11, d, generator=torch.Generator().manual_seed(9), dtype=torch.float64) - 1
    for s in (torch.full((n,), c, dtype=torch.float64), torch.full((q, n), c, dtype=torch.float64)):
        lp = ref.log_prob("matern52", X, ell, osc, noise, s, y)
        assert torch.allclose(lp, gm.exact_latent_log_prob("matern", X, ell, noise + c, y, osc, 2.5), rtol=1e-12, atol=0)
        want = gm.exact_latent_log_prob_analytic("matern", X, ell, noise + c, y, osc, 2.5)
        _, g = ref.gradients("matern52", X, ell, osc, noise, s, y, wrt_x=False)
        for name, w in (("table", want[1]), ("noise", want[2]), ("oscale", want[3]), ("y", want[4])):
            assert torch.allclose(g[name], w, rtol=1e-8, atol=1e-11), name
        gs = g["s"].sum(0) if s.dim() == 1 else g["s"].sum(-1)
        assert torch.allclose(gs.expand(q) if s.dim() == 1 else gs, want[2].sum().expand(q) if s.dim() == 1 else want[2], rtol=1e-8, atol=1e-11)
        mu, cov = ref.posterior("matern52", X, ell, osc, noise, s, y, Xs)
        wmu, wcov = gm.exact_gp_posterior("matern", X, ell, noise + c, y, Xs, osc, 2.5)
        assert torch.allclose(mu, wmu, rtol=1e-10, atol=1e-12) and torch.allclose(cov, wcov, rtol=1e-9, atol=1e-12)


def test_per_point_gradient_is_half_alpha_squared_minus_the_inverse_diagonal():
    n, d, q = 40, 2, 2
    X, y, ell, osc, noise, s = ref.problem(n, d, q, seed=2)
    for kind in ("matern52", "rq", "poly2"):
        table = ref.table_of(kind, ell)
        _, g = ref.gradients(kind, X, table, osc, noise, s, y, wrt_x=False)
        Kinv = torch.linalg.inv(ref.noisy(ref.kernel(kind, X, X, table, osc), noise, s))
        alpha = (Kinv @ y.unsqueeze(-1)).squeeze(-1)
        assert torch.allclose(g["s"], 0.5 * (alpha ** 2 - torch.diagonal(Kinv, dim1=1, dim2=2)), rtol=1e-8, atol=1e-10), kind
        assert torch.allclose(g["s"].sum(-1), g["noise"], rtol=1e-9, atol=1e-10), kind


def test_bordered_posterior_equals_the_posterior_on_the_concatenated_data():
    n, m, d, q = 30, 4, 2, 2
    X, y, ell, osc, noise, s = ref.problem(n + m, d, q, seed=6)
    Xs = 2 * torch.rand(7, d, generator=torch.Generator().manual_seed(1), dtype=torch.float64) - 1
    a = ref.bordered_posterior("matern52", X[:n], ell, osc, noise, s[:, :n], y[:, :n], X[n:], s[:, n:], y[:, n:], Xs)
    b = ref.posterior("matern52", X, ell, osc, noise, s, y, Xs)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.fixture
def mutation():
    def set_(name):
        ref.MUTATION = name
    yield set_
    ref.MUTATION = None


def test_mutation_vector_on_the_whole_row_fails_the_assembly_assertion(mutation):
    n, n_pad = 5, 8
    for dtype in (torch.float32, torch.float64):
        base = torch.full((2, n_pad, n_pad + 4), float("nan"), dtype=dtype)
        base[:, :, :n_pad] = torch.rand(2, n_pad, n_pad).to(dtype).triu()
        s = torch.logspace(-3, 1, n, dtype=torch.float64)
        good = ref.expected_assembly(base, s, n)
        ref.check_assembly(good.clone(), good)
        assert torch.equal(good[:, n:], base[:, n:]) or torch.isnan(base[:, n:]).any()       # the padding is not touched
        mutation("row")
        bad = ref.expected_assembly(base, s, n)
        with pytest.raises(AssertionError):
            ref.check_assembly(bad, good)
        mutation(None)
        moved = good.clone()
        moved[0, 0, n_pad] = 1.0                                                                 # a NaN position that moved
        with pytest.raises(AssertionError, match="NaN positions"):
            ref.check_assembly(moved, good)


def test_mutation_noise_left_off_the_border_fails_the_fantasy_assertions(mutation):
    n, m, d, q = 60, 5, 3, 2
    X, y, ell, osc, noise, s = ref.problem(n + m, d, q, seed=8)
    Xs = 2 * torch.rand(20, d, generator=torch.Generator().manual_seed(3), dtype=torch.float64) - 1
    args = ("matern52", X[:n], ell, osc, noise, s[:, :n], y[:, :n], X[n:], s[:, n:], y[:, n:], Xs)
    good = ref.bordered_posterior(*args)
    mutation("border")
    bad = ref.bordered_posterior(*args)
    for dtype in (torch.float64, torch.float32):
        ref.check_fantasy(good[0], good[0], dtype)
        with pytest.raises(AssertionError):
            ref.check_fantasy(bad[0], good[0], dtype, "mean")
        with pytest.raises(AssertionError):
            ref.check_fantasy(torch.diagonal(bad[1], dim1=1, dim2=2), torch.diagonal(good[1], dim1=1, dim2=2), dtype, "variance")
    with pytest.raises(AssertionError):
        ref.check_moments(bad[0], torch.diagonal(bad[1], dim1=1, dim2=2), bad[1], good[0], good[1])
