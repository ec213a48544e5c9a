"""Gaussian likelihoods with the gpytorch parameter names and semantics the reference uses:
`GaussianLikelihood(batch_shape=[q], noise_constraint=GreaterThan(e^noise_thresh))`
(projected_lmc.py:920-921) and `MultitaskGaussianLikelihood(num_tasks, rank, has_global_noise)`
(:1025, experiments.py:184,190).  Applying a likelihood to a prior only records the noise on the
lazy covariance; the addition itself is fused into the HIP assembly kernel.

[gpytorch-knowledge]: noise = softplus(raw_noise) + lower bound (default 1e-4), raw init 0;
multitask rank 0: Sigma = diag(task_noises) + noise I; rank r > 0: Sigma = F F^T + noise I with
F = task_noise_covar_factor (p x r, randn init); has_global_noise=False drops noise I.
FixedNoiseGaussianLikelihood(noise, learn_additional_noise): a known noise variance per training point (+ a learned scalar).
"""
import torch

from .constraints import GreaterThan
from .distributions import MultivariateNormal, MultitaskMultivariateNormal, KroneckerSumCovariance
from .kernels import LazyKernel


class Likelihood(torch.nn.Module):
    pass


class _GaussianLikelihoodBase(Likelihood):
    pass


class HomoskedasticNoise(torch.nn.Module):
    def __init__(self, noise_constraint=None, batch_shape=torch.Size()):
        super().__init__()
        self.register_parameter("raw_noise", torch.nn.Parameter(torch.zeros(*batch_shape, 1)))
        self.raw_noise_constraint = noise_constraint or GreaterThan(1e-4)

    @property
    def noise(self):
        return self.raw_noise_constraint.transform(self.raw_noise)

    @noise.setter
    def noise(self, value):
        value = torch.as_tensor(value, dtype=self.raw_noise.dtype, device=self.raw_noise.device)
        with torch.no_grad():
            self.raw_noise.copy_(self.raw_noise_constraint.inverse_transform(value).expand_as(self.raw_noise))


class GaussianLikelihood(_GaussianLikelihoodBase):
    def __init__(self, noise_prior=None, noise_constraint=None, batch_shape=torch.Size(), **kwargs):
        super().__init__()
        self.batch_shape = torch.Size(batch_shape)
        self.noise_covar = HomoskedasticNoise(noise_constraint, self.batch_shape)

    @property
    def noise(self):
        return self.noise_covar.noise

    @noise.setter
    def noise(self, value):
        self.noise_covar.noise = value

    @property
    def raw_noise(self):
        return self.noise_covar.raw_noise

    def forward(self, function_dist, *params, **kwargs):
        c = function_dist.lazy_covariance_matrix
        noise = self.noise.reshape(-1)
        if isinstance(c, LazyKernel) or hasattr(c, "log_prob_batch"):
            new = c.add_noise(noise.to(c.ell.dtype))
        elif torch.is_tensor(c):
            eye = torch.eye(c.shape[-1], dtype=c.dtype, device=c.device)
            new = c + noise.reshape(*self.batch_shape, 1, 1) * eye
        else:
            raise NotImplementedError("GaussianLikelihood on %s" % type(c).__name__)
        return MultivariateNormal(function_dist.mean, new)


class FixedNoise(torch.nn.Module):
    """The per-point noise vector of FixedNoiseGaussianLikelihood: a plain tensor (n) or (*batch_shape, n) -- no parameter, not in the
    state_dict.  It may be the output of the user's own noise model and then carries its graph."""

    def __init__(self, noise, batch_shape=torch.Size()):
        super().__init__()
        self.batch_shape = torch.Size(batch_shape)
        self.noise = self._checked(noise)

    def __deepcopy__(self, memo):          # (a vector that carries a graph has no deepcopy of its own: the copy holds its values)
        new = memo[id(self)] = FixedNoise(self.noise.detach().clone(), self.batch_shape)
        return new

    def _checked(self, noise):
        if not torch.is_tensor(noise):
            noise = torch.as_tensor(noise, dtype=torch.get_default_dtype())
        if noise.dim() == 0 or noise.dim() > 1 + len(self.batch_shape) or (noise.dim() > 1 and noise.shape[:-1] != self.batch_shape):
            raise ValueError("FixedNoiseGaussianLikelihood: noise is (n) or (*batch_shape, n) with batch_shape %s, got %s"
                             % (tuple(self.batch_shape), tuple(noise.shape)))
        if not bool((noise.detach() > 0).all()):
            raise ValueError("FixedNoiseGaussianLikelihood: noise has non-positive (or non-finite) values; every entry must be > 0")
        return noise

    def _apply(self, fn, *args, **kwargs):
        self.noise = fn(self.noise) if not self.noise.requires_grad else self.noise
        return super()._apply(fn, *args, **kwargs)


class FixedNoiseGaussianLikelihood(_GaussianLikelihoodBase):
    """Gaussian likelihood with a known (or modelled) noise variance per training point, gpytorch's names and meaning
    [gpytorch-knowledge, unverified offline]: Khat = K + diag(noise) (+ second_noise I with learn_additional_noise=True).
    `noise` (n) or (*batch_shape, n), every entry > 0: replicated runs averaged to sigma^2 / r_i, Monte-Carlo standard errors, the
    output of a noise model sigma^2(x) = g_phi(x) (its graph is kept: the marginal likelihood differentiates into it), or a large value
    that down-weights an observation.  `.noise` gets and sets the vector (`noise_covar.noise`); `.second_noise` is the learned
    homoskedastic part (`second_noise_covar.raw_noise`, (*batch_shape, 1)).  The addition itself is fused into the HIP assembly kernels
    (plmc_assemble*_pn_*, plmc_factorize*_pn_ex_*).
    forward(function_dist, noise=None): the keyword's vector if given; else the stored one if its length is the distribution's; else a
    UserWarning, and only the additional noise is added (zero without one) -- what evaluating the likelihood at test points without
    telling it their noise means.
    Served by ExactGPModel (training with ExactMarginalLogLikelihood, eval-mode predictions, get_fantasy_model(..., noise=)); every other
    model and objective refuses it by name."""

    def __init__(self, noise, learn_additional_noise=False, batch_shape=torch.Size(), noise_constraint=None, **kwargs):
        super().__init__()
        self.batch_shape = torch.Size(batch_shape)
        self.noise_covar = FixedNoise(noise, self.batch_shape)
        self.second_noise_covar = HomoskedasticNoise(noise_constraint, self.batch_shape) if learn_additional_noise else None

    @property
    def noise(self):
        return self.noise_covar.noise

    @noise.setter
    def noise(self, value):
        self.noise_covar.noise = self.noise_covar._checked(value)

    @property
    def second_noise(self):
        if self.second_noise_covar is None:
            return 0.0
        return self.second_noise_covar.noise

    @second_noise.setter
    def second_noise(self, value):
        if self.second_noise_covar is None:
            raise RuntimeError("FixedNoiseGaussianLikelihood: set second_noise with learn_additional_noise=True only")
        self.second_noise_covar.noise = value

    def additional_noise(self, q, like):
        """The homoskedastic part per latent, (q): second_noise, or zeros without one."""
        if self.second_noise_covar is None:
            return torch.zeros(q, dtype=like.dtype, device=like.device)
        return self.second_noise.reshape(-1).to(like.dtype).expand(q)

    def _vector(self, noise, n):
        """The per-point vector for a distribution over n points: the keyword's, the stored one if it fits, or None with a warning."""
        if noise is not None:
            noise = self.noise_covar._checked(noise)
            if noise.shape[-1] != n:
                raise ValueError("FixedNoiseGaussianLikelihood: noise= has %d entries for a distribution over %d points" % (noise.shape[-1], n))
            return noise
        if self.noise.shape[-1] == n:
            return self.noise
        import warnings
        warnings.warn("FixedNoiseGaussianLikelihood: the distribution has %d points and the stored noise %d, and no noise= was given: only "
                      "the additional noise is added (pass noise= for the points' own)" % (n, self.noise.shape[-1]), UserWarning)
        return None

    def forward(self, function_dist, *params, noise=None, **kwargs):
        c = function_dist.lazy_covariance_matrix
        if hasattr(c, "log_prob_batch"):
            raise NotImplementedError("FixedNoiseGaussianLikelihood on the inducing-point (SGPR) covariance of ExactGPModel(n_inducing_points=...) "
                                      "is not implemented: per-point noise runs on the exact engine only")
        if isinstance(c, LazyKernel):
            if not c.is_square:
                raise NotImplementedError("FixedNoiseGaussianLikelihood on a cross-covariance k(X1, X2)")
            q = c.ell.shape[0]
            v = self._vector(noise, c.x1.shape[-2])
            new = c.add_noise(self.additional_noise(q, c.ell))
            if v is not None:
                new = new.add_point_noise(v.to(device=c.ell.device))
            return MultivariateNormal(function_dist.mean, new)
        if torch.is_tensor(c):
            v = self._vector(noise, c.shape[-1])
            extra = self.second_noise if self.second_noise_covar is None else self.second_noise.reshape(*self.batch_shape, 1).to(c.dtype)
            dg = extra if v is None else v.to(c) + extra
            if not torch.is_tensor(dg):
                return MultivariateNormal(function_dist.mean, c)
            return MultivariateNormal(function_dist.mean, c + torch.diag_embed(dg.expand(c.shape[:-1])))
        raise NotImplementedError("FixedNoiseGaussianLikelihood on %s" % type(c).__name__)


def refuse_fixed_noise(likelihood, what):
    """What does not serve per-point noise says so by the likelihood's name instead of dropping the vector."""
    if isinstance(likelihood, FixedNoiseGaussianLikelihood):
        raise NotImplementedError("%s is not implemented for FixedNoiseGaussianLikelihood (per-point noise): it is served by ExactGPModel "
                                  "without inducing points -- ExactMarginalLogLikelihood, eval-mode predictions, get_fantasy_model" % what)


class MultitaskGaussianLikelihood(_GaussianLikelihoodBase):
    def __init__(self, num_tasks, rank=0, task_prior=None, batch_shape=torch.Size(), noise_prior=None,
                 noise_constraint=None, has_global_noise=True, has_task_noise=True, **kwargs):
        super().__init__()
        self.num_tasks, self.rank = num_tasks, rank
        self.has_global_noise, self.has_task_noise = has_global_noise, has_task_noise
        self.raw_noise_constraint = noise_constraint or GreaterThan(1e-4)
        if has_task_noise:
            if rank == 0:
                self.register_parameter("raw_task_noises", torch.nn.Parameter(torch.zeros(num_tasks)))
                self.raw_task_noises_constraint = noise_constraint or GreaterThan(1e-4)
            else:
                self.register_parameter("task_noise_covar_factor", torch.nn.Parameter(torch.randn(num_tasks, rank)))
        if has_global_noise:
            self.register_parameter("raw_noise", torch.nn.Parameter(torch.zeros(1)))

    @property
    def noise(self):
        return self.raw_noise_constraint.transform(self.raw_noise)

    @property
    def task_noises(self):
        if self.rank > 0:
            raise AttributeError("Cannot get diagonal task noises when covariance is rank %d" % self.rank)
        return self.raw_task_noises_constraint.transform(self.raw_task_noises)

    @property
    def task_noise_covar(self):
        if self.rank == 0:
            return torch.diag_embed(self.task_noises)
        return self.task_noise_covar_factor @ self.task_noise_covar_factor.T

    def __getattr__(self, name):
        # `hasattr(lik, "noise")` must be False without global noise (experiments.py:323,333)
        if name == "noise" and not self.__dict__.get("has_global_noise", True):
            raise AttributeError(name)
        return super().__getattr__(name)

    def task_noise_matrix(self, dtype=None):
        """Sigma (p x p)."""
        S = 0.0
        if self.has_task_noise:
            S = self.task_noise_covar
        if self.has_global_noise:
            ref = self.raw_noise
            S = S + self.noise.reshape(()) * torch.eye(self.num_tasks, dtype=ref.dtype, device=ref.device)
        return S if dtype is None else S.to(dtype)

    def expected_log_prob(self, target, input, *params, **kwargs):
        """E_q(f)[log p(y|f)] per data point; like gpytorch's _GaussianLikelihoodBase it uses only the
        marginal variances of q(f) and the DIAGONAL of the task-noise covariance [gpytorch-knowledge]."""
        import math
        mean, variance = input.mean, input.variance
        noise = torch.diagonal(self.task_noise_matrix(mean.dtype)).reshape(1, -1)
        res = ((target - mean).square() + variance) / noise + noise.log() + math.log(2 * math.pi)
        return res.mul(-0.5).sum(-1)

    def forward(self, function_dist, *params, **kwargs):
        c = function_dist.lazy_covariance_matrix
        Sigma = self.task_noise_matrix(function_dist.mean.dtype)
        if hasattr(c, "add_task_noise"):
            return MultitaskMultivariateNormal(function_dist.mean, c.add_task_noise(Sigma))
        ind = getattr(function_dist, "_independent", None)
        if ind is not None and self.rank == 0:
            noisy = ind.lazy_covariance_matrix.add_noise(torch.diagonal(Sigma).to(function_dist.mean.dtype))
            return MultitaskMultivariateNormal.from_batch_mvn(MultivariateNormal(ind.mean, noisy))
        raise NotImplementedError("MultitaskGaussianLikelihood on %s" % type(c).__name__)
