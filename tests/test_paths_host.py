"""Pathwise posterior draws without a device: the spectral sampler of projectedlmc/paths.py, the refusals of sample_paths by name, and
the default of settings.skip_posterior_variances.

Spectral sampler, fixed seed, m = 2^16 frequencies: the mean of cos(2 pi omega . tau) over the drawn frequencies is a Monte-Carlo
estimate of k(tau) whose terms lie in [-1, 1], so its variance is at most 1 / m; it is held to 5 / sqrt(m), five standard deviations,
for the four stationary kinds at six lags each against oracle.gp_math's profile."""
import math
import warnings

import pytest
import torch

from oracle import gp_math as gm

M = 2 ** 16
KINDS = {"rbf": ("rbf", 2.5), "matern12": ("matern", 0.5), "matern32": ("matern", 1.5), "matern52": ("matern", 2.5)}
LAGS = torch.tensor([[0.0, 0.0], [0.3, 0.0], [0.5, -0.5], [1.0, 0.4], [-1.5, 1.0], [2.5, 1.5]], dtype=torch.float64)


@pytest.fixture(scope="module")
def plmc():
    import projectedlmc
    return projectedlmc


@pytest.mark.parametrize("kind", list(KINDS))
def test_mean_cosine_of_the_drawn_frequencies_is_the_kernel(kind):
    from projectedlmc.paths import spectral_frequencies
    g = torch.Generator().manual_seed(1234)
    omega = spectral_frequencies(kind, (M, 2), g)
    assert omega.shape == (M, 2) and omega.dtype == torch.float64
    est = torch.cos(2.0 * math.pi * (omega @ LAGS.T)).mean(0)          # (6)
    okind, nu = KINDS[kind]
    want = gm.kernel_matrix(okind, LAGS, torch.zeros(1, 2, dtype=torch.float64), torch.ones(1, 2, dtype=torch.float64), nu=nu)[0, :, 0]
    err = (est - want).abs()
    print(kind, "largest error %.2e of %.2e allowed" % (float(err.max()), 5 / math.sqrt(M)))
    assert float(est[0]) == 1.0                                        # lag 0
    assert bool((err <= 5.0 / math.sqrt(M)).all()), (kind, err)


def test_draws_follow_the_generator():
    from projectedlmc.paths import spectral_frequencies
    a = spectral_frequencies("matern32", (3, 2, 50, 4), torch.Generator().manual_seed(5))
    b = spectral_frequencies("matern32", (3, 2, 50, 4), torch.Generator().manual_seed(5))
    c = spectral_frequencies("matern32", (3, 2, 50, 4), torch.Generator().manual_seed(6))
    assert torch.equal(a, b) and not torch.equal(a, c)
    with pytest.raises(NotImplementedError, match="periodic"):
        spectral_frequencies("periodic", (4, 2))


def _data(n=40, d=2, p=4):
    g = torch.Generator().manual_seed(0)
    return torch.rand(n, d, generator=g, dtype=torch.float64), torch.randn(n, p, generator=g, dtype=torch.float64)


def _exact(plmc, kernel, **kw):
    X, Y = _data()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return plmc.ExactGPModel(X, Y[:, 0].contiguous(), plmc.GaussianLikelihood(), kernel_type=kernel, **kw).double()


@pytest.mark.parametrize("kernel,word", [("PeriodicKernel", "periodic"), ("RQKernel", "rq"), ("SpectralMixtureKernel", "sm"),
                                         ("LinearKernel", "linear"), ("SplineKernel", "spline")])
def test_other_kernel_kinds_are_refused_by_name(plmc, kernel, word):
    kw = dict(ker_kwargs=dict(num_mixtures=2)) if kernel == "SpectralMixtureKernel" else {}
    m = _exact(plmc, getattr(plmc, kernel), **kw).eval()
    with pytest.raises(NotImplementedError, match=r"sample_paths: kernel kind '%s'" % word):
        m.sample_paths(2, num_features=8)


def test_models_without_an_exact_factor_are_refused_by_name(plmc):
    X, Y = _data()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sgpr = _exact(plmc, plmc.MaternKernel, n_inducing_points=8, mean_type=plmc.ZeroMean).eval()
        with pytest.raises(NotImplementedError, match=r"sample_paths: the inducing-point \(SGPR\) model"):
            sgpr.sample_paths(2)
        psgpr = plmc.ProjectedGPModel(X, Y, 4, 2, mean_type=plmc.ZeroMean, kernel_type=plmc.MaternKernel, n_inducing_points=8).double().eval()
        with pytest.raises(NotImplementedError, match=r"sample_paths: the inducing-point \(SGPR\) model"):
            psgpr.sample_paths(2)
        var = plmc.VariationalMultitaskGPModel(X, n_latents=2, n_tasks=4, train_ind_ratio=2.0, seed=0)
        with pytest.raises(NotImplementedError, match=r"sample_paths: the variational model \(VariationalMultitaskGPModel\)"):
            var.sample_paths(2)
        lmc = plmc.MultitaskGPModel(X, Y, plmc.MultitaskGaussianLikelihood(num_tasks=4, rank=0), n_tasks=4, n_latents=2, model_type="LMC")
        with pytest.raises(NotImplementedError, match=r"sample_paths: the dense LMC model \(MultitaskGPModel\)"):
            lmc.eval().sample_paths(2)
        shard = plmc.ProjectedGPModel(X, Y, 4, 2, mean_type=plmc.ZeroMean, kernel_type=plmc.MaternKernel, latent_shard=(0, 2)).double().eval()
        with pytest.raises(NotImplementedError, match="sample_paths: the latent-sharded ProjectedGPModel"):
            shard.sample_paths(2)


def test_train_mode_is_refused(plmc):
    m = _exact(plmc, plmc.MaternKernel)
    assert m.training
    with pytest.raises(RuntimeError, match="sample_paths is an eval-mode method"):
        m.sample_paths(2)
    with pytest.raises(ValueError, match="num_paths >= 1"):
        m.eval().sample_paths(0)


def test_skip_posterior_variances_defaults_to_off(plmc):
    s = plmc.settings.skip_posterior_variances
    assert s.on() is False
    with s():
        assert s.on() is True
        with s(False):
            assert s.on() is False
        assert s.on() is True
    assert s.on() is False


def test_a_mean_only_prediction_refuses_what_it_cannot_serve(plmc):
    """The refusals come before any device work: gradients with respect to x, full_cov, the inducing-point and the sharded model."""
    X, Y = _data()
    m = _exact(plmc, plmc.MaternKernel).eval()
    xs = torch.rand(5, 2, dtype=torch.float64)
    with plmc.settings.skip_posterior_variances():
        with pytest.raises(NotImplementedError, match="skip_posterior_variances.*require a gradient"):
            m(xs.clone().requires_grad_())
        with pytest.raises(NotImplementedError, match="skip_posterior_variances.*full_cov=True"):
            m(xs, full_cov=True)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sgpr = _exact(plmc, plmc.MaternKernel, n_inducing_points=8, mean_type=plmc.ZeroMean).eval()
            with pytest.raises(NotImplementedError, match=r"skip_posterior_variances.*inducing-point \(SGPR\)"):
                sgpr(xs)
            shard = plmc.ProjectedGPModel(X, Y, 4, 2, mean_type=plmc.ZeroMean, kernel_type=plmc.MaternKernel, latent_shard=(0, 2)).double().eval()
            with pytest.raises(NotImplementedError, match="skip_posterior_variances.*latent-sharded"):
                shard(xs)
            proj = plmc.ProjectedGPModel(X, Y, 4, 2, mean_type=plmc.ZeroMean, kernel_type=plmc.MaternKernel).double().eval()
            with pytest.raises(NotImplementedError, match="skip_posterior_variances.*full_cov=True"):
                proj(xs, full_cov=True)
