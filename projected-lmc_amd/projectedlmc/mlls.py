"""`ExactMarginalLogLikelihood` with gpytorch's contract (experiments.py:233, README.md:45):
mll(model(X), Y) = likelihood(model(X)).log_prob(Y) / num_data, num_data =
function_dist.event_shape.numel() [gpytorch-knowledge, v1.11 -- the same expression the
reference copies at projected_lmc.py:1194].  `_add_other_terms` adds the model's added-loss terms and
the log-density of every registered lengthscale prior (priors.py)."""
import torch

from .distributions import MultivariateNormal
from .likelihoods import _GaussianLikelihoodBase


class MarginalLogLikelihood(torch.nn.Module):
    def __init__(self, likelihood, model):
        super().__init__()
        self.likelihood = likelihood
        self.model = model

    def _add_other_terms(self, res, params):
        """Added loss terms registered by the model's modules (the SGPR trace term of
        InducingPointKernel), then `prior.log_prob(value).sum()` of every registered prior, added to
        every element of `res` [gpytorch-knowledge: MarginalLogLikelihood._add_other_terms, v1.11]."""
        from .priors import named_priors
        for mod in self.model.modules():
            fn = getattr(mod, "added_loss_term", None)
            if fn is not None:
                term = fn()
                if term is not None:
                    res = res + term.reshape(res.shape)
        for _, _, prior, value in named_priors(self.model):
            res = res + prior.log_prob(value).sum()
        return res


class ExactMarginalLogLikelihood(MarginalLogLikelihood):
    def __init__(self, likelihood, model):
        if not isinstance(likelihood, _GaussianLikelihoodBase):
            raise RuntimeError("Likelihood must be Gaussian for exact inference")
        super().__init__(likelihood, model)

    def forward(self, function_dist, target, *params):
        if not isinstance(function_dist, MultivariateNormal):
            raise RuntimeError("ExactMarginalLogLikelihood can only operate on Gaussian random variables")
        output = self.likelihood(function_dist, *params)
        res = output.log_prob(target)
        res = self._add_other_terms(res, params)
        num_data = function_dist.event_shape.numel()
        return res / num_data


class LeaveOneOutPseudoLikelihood(ExactMarginalLogLikelihood):
    """The leave-one-out cross-validation objective of the reference (projected_lmc.py:86-105; gpytorch ships it under the same name):
    loo(model(X), Y) = [ sum_i log N(y_i; mu_-i, sigma2_-i) + other terms ] / num_data, the predictive density of every training point
    given all the others (Rasmussen & Williams 5.4.2), from diag(Khat^-1) and Khat^-1 y of the factorisation the MLL uses, with the
    analytic gradient (_engine.ExactLooLogProb).  Constructor order as in the reference; train_x / train_y are kept and not used.
    Serves ExactGPModel without inducing points (a batch of independent tasks is summed, as log_prob does)."""

    def __init__(self, likelihood, model, train_x=None, train_y=None):
        from .likelihoods import refuse_fixed_noise
        refuse_fixed_noise(likelihood, "LeaveOneOutPseudoLikelihood")
        super().__init__(likelihood, model)
        self.train_x = train_x
        self.train_y = train_y

    def forward(self, function_dist, target, *params):
        if not isinstance(function_dist, MultivariateNormal):
            raise RuntimeError("LeaveOneOutPseudoLikelihood can only operate on Gaussian random variables")
        from .kernels import LazyKernel, LazyLmcKernel
        from .projected import ProjectedGPModel
        # refusals by the type of the covariance (and of the model that owns it), before anything looks at a device
        c = function_dist.lazy_covariance_matrix
        if isinstance(self.model, ProjectedGPModel):
            raise NotImplementedError("LeaveOneOutPseudoLikelihood is not implemented for ProjectedGPModel (its latent processes see "
                                      "projected data: train it with ProjectedLMCmll)")
        if getattr(self.model, "input_transform", None) is not None:
            raise NotImplementedError("LeaveOneOutPseudoLikelihood is not implemented for a model with an input_transform (the leave-one-out "
                                      "objective has no gradient with respect to the inputs): train it with ExactMarginalLogLikelihood")
        if hasattr(c, "log_prob_batch"):
            raise NotImplementedError("LeaveOneOutPseudoLikelihood is not implemented for the inducing-point (SGPR) covariance of "
                                      "ExactGPModel(n_inducing_points=...)")
        if isinstance(c, LazyLmcKernel):
            raise NotImplementedError("LeaveOneOutPseudoLikelihood is not implemented for MultitaskGPModel (dense LMC / ICM covariance)")
        if not isinstance(c, LazyKernel):
            raise NotImplementedError("LeaveOneOutPseudoLikelihood on %s" % type(c).__name__)
        output = self.likelihood(function_dist, *params)
        ind = getattr(output, "_independent", None)          # independent tasks built from a batch (from_batch_mvn): (n, p) -> (p, n)
        dist, y = (output, target) if ind is None else (ind, target.transpose(-1, -2))
        k = dist.lazy_covariance_matrix
        from . import _engine
        q = k.ell.shape[0]
        diff = (y - dist.mean).reshape(q, -1)
        res = _engine.exact_loo_log_prob(k.kind, k.x1, k.ell, k.oscale, k.noise.reshape(-1), diff)
        res = res.reshape(dist.batch_shape) if ind is None else res.sum(-1)
        res = self._add_other_terms(res, params)
        num_data = function_dist.event_shape.numel()
        return res / num_data
