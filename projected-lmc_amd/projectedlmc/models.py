"""Exact GP model classes: `ExactGPModel` and the helpers it is built from, mirroring the
reference's constructor-and-forward API (projected_lmc.py:107-201, 264-436) on top of the HIP
engine instead of gpytorch.
"""
import warnings

import weakref

import torch

from . import _engine
from . import settings
from . import kernels as _k
from . import means as _m
from .distributions import MultivariateNormal, MultitaskMultivariateNormal, ZeroCovariance
from .likelihoods import FixedNoiseGaussianLikelihood, GaussianLikelihood, refuse_fixed_noise

# model -> (input tensor, version, training input, version) already compared equal (kept outside the module's
# __dict__: weak references do not pickle)
_TRAIN_INPUT_SEEN = weakref.WeakKeyDictionary()


# ---------------------------------------------------------------------------------------- helpers
def handle_covar_(kernel, dim, decomp=None, n_funcs=1, prior_scales=None, prior_width=None, outputscales=True,
                  ker_kwargs=None):
    """Kernel factory with the reference's semantics (projected_lmc.py:107-181): an ARD kernel with
    batch_shape=[n_funcs]; wrapped in a ScaleKernel when `outputscales`.  With `prior_scales` the
    lengthscales get a Normal (one variable) / MultivariateNormal (ARD group) prior -- mean
    prior_scales, deviation resp. covariance diagonal prior_scales * prior_width, exactly as :140-149
    writes them -- and start at the prior mean (:169-179).  `decomp` with several groups builds the
    additive kernel of additive.py (single-output models)."""
    from . import priors as _p
    ker_kwargs = {} if ker_kwargs is None else ker_kwargs
    if decomp is None:
        decomp = [list(range(dim))]
    l_priors = [None] * len(decomp)
    if prior_scales is not None:
        if prior_width is None:
            raise ValueError('A prior width should be provided if a prior mean is')
        if type(prior_scales) is not list:      # one length per variable, or a list with one array per kernel
            prior_scales = [torch.as_tensor(prior_scales)[idx_list] for idx_list in decomp]
        if type(prior_width) is not list:
            prior_width = [torch.as_tensor(prior_width)[idx_list] for idx_list in decomp]
        for i_ker, idx_list in enumerate(decomp):
            sc, wd = torch.as_tensor(prior_scales[i_ker]), torch.as_tensor(prior_width[i_ker])
            if len(idx_list) > 1:
                l_priors[i_ker] = _p.MultivariateNormalPrior(loc=sc, covariance_matrix=torch.diag_embed(sc * wd))
            else:
                l_priors[i_ker] = _p.NormalPrior(loc=sc, scale=sc * wd)

    def init_from_prior(ker, prior):
        if prior is not None and ker.has_lengthscale:
            try:
                ker.lengthscale = prior.mean
            except Exception:
                raise ValueError('Provided prior scales were of the wrong shape')

    if len(decomp) > 1:
        _k.refuse_sm(kernel, "handle_covar_(decomp=...) with several groups (the additive kernel)")
        _k.refuse_periodic(kernel, "handle_covar_(decomp=...) with several groups (the additive kernel)")
        _k.refuse_rq(kernel, "handle_covar_(decomp=...) with several groups (the additive kernel)")
        _k.refuse_dot(kernel, "handle_covar_(decomp=...) with several groups (the additive kernel)")
        # k(x) = sum_g s_g k_g(x[idx_g]): every sub-kernel gets an output scale (:159-162)
        from .additive import AdditiveKernel
        subs = []
        for i_ker, idx_g in enumerate(decomp):
            kg = kernel(ard_num_dims=len(idx_g), active_dims=idx_g, lengthscale_prior=l_priors[i_ker],
                        batch_shape=torch.Size([n_funcs]), **ker_kwargs)
            _k.refuse_product(kg, "handle_covar_(decomp=...) with several groups (the additive kernel)")   # (a factory shows it only now)
            _k.refuse_sum(kg, "handle_covar_(decomp=...) with several groups (the additive kernel)")
            init_from_prior(kg, l_priors[i_ker])
            subs.append(_k.ScaleKernel(kg, batch_shape=torch.Size([n_funcs])))
        return AdditiveKernel(*subs)
    idx = decomp[0]
    ker = kernel(ard_num_dims=len(idx), active_dims=idx, lengthscale_prior=l_priors[0],
                 batch_shape=torch.Size([n_funcs]), **ker_kwargs)
    covar_module = _k.ScaleKernel(ker, batch_shape=torch.Size([n_funcs])) if outputscales else ker
    init_from_prior(ker, l_priors[0])
    return covar_module


def init_lmc_coefficients(train_y, n_latents, QR_form=False):
    """SVD projection of the labels onto the latent task subspace (projected_lmc.py:183-201).

    The reference calls sklearn's randomized_svd(Y^T, q, random_state=0) on the host.  Here the
    p x p Gram matrix Y^T Y is formed on the device and eigendecomposed exactly: U = eigenvectors
    (p x q), S = sqrt(eigenvalues); signs follow sklearn's svd_flip convention for this call
    (largest-magnitude entry of each column of U positive).  Identical to the reference whenever
    its randomised range finder is exact (q + 10 >= p); otherwise equal up to the randomised
    method's approximation error.  Returns (U, S) if QR_form else (U S / sqrt(n-1))^T."""
    n_data, n_tasks = train_y.shape
    dt = train_y.dtype
    Y = train_y.to(torch.float64)
    if n_data >= n_latents:
        G = Y.T @ Y
        evals, evecs = torch.linalg.eigh(G)
        order = torch.argsort(evals, descending=True)[:n_latents]
        S = evals[order].clamp_min(0).sqrt()
        U = evecs[:, order]
        if U.shape[1] < n_latents:                   # asked for more components than tasks
            raise ValueError("n_latents cannot exceed n_tasks in the SVD initialisation")
        piv = U.abs().argmax(dim=0)
        sgn = torch.sign(U[piv, torch.arange(U.shape[1], device=U.device)])
        sgn[sgn == 0] = 1
        U = U * sgn[None, :]
    else:
        Q, R = torch.linalg.qr(Y.T, mode="complete")
        S = 1e-3 * torch.ones(n_latents, dtype=torch.float64, device=Y.device)
        S[:n_data] = torch.diagonal(R)[:n_data]
        U = Q[:, :n_latents]
    U, S = U.to(dt), S.to(dt)
    if QR_form:
        return U, S
    return (U * S / (n_data - 1) ** 0.5).T


def refuse_skip_variances(x, full_cov, model=None):
    """settings.skip_posterior_variances serves the mean of the exact posterior at constant test inputs only."""
    what = "settings.skip_posterior_variances(True) together with "
    if model is not None:
        raise NotImplementedError(what + model + ": the mean-only route serves the exact models")
    if torch.is_grad_enabled() and x.requires_grad:
        raise NotImplementedError(what + "test inputs that require a gradient (x.requires_grad): the mean-only route carries no "
                                  "derivative with respect to x -- detach x, or leave the setting off")
    if full_cov:
        raise NotImplementedError(what + "full_cov=True: there is no covariance to return")


# ------------------------------------------------------------------------------- parametrisations
class ScalarParam(torch.nn.Module):
    """All entries equal to the clamped mean of the raw vector (projected_lmc.py:207-218)."""

    def __init__(self, bounds=(1e-16, 1e16)):
        super().__init__()
        self.bounds = bounds

    def forward(self, X):
        return torch.clamp(X.mean(), *self.bounds) * torch.ones_like(X)

    def right_inverse(self, A):
        return A


class PositiveDiagonalParam(torch.nn.Module):
    """diag(exp(diag X)) (projected_lmc.py:220-227)."""

    def forward(self, X):
        return torch.diag_embed(torch.diagonal(X).exp())

    def right_inverse(self, A):
        return torch.diag_embed(torch.diagonal(A).log())


class UpperTriangularParam(torch.nn.Module):
    """triu(X) with exponentiated diagonal (projected_lmc.py:229-240)."""

    def forward(self, X):
        U = X.triu(1)
        return U + torch.diag_embed(torch.diagonal(X).exp())

    def right_inverse(self, A):
        return A.triu(1) + torch.diag_embed(torch.diagonal(A).log())


class LowerTriangularParam(torch.nn.Module):
    """tril(X) with exp(clamp(diagonal)) (projected_lmc.py:242-258)."""

    def __init__(self, bounds=(1e-16, 1e16)):
        super().__init__()
        self.bounds = bounds

    def forward(self, X):
        L = X.tril(-1)
        return L + torch.diag_embed(torch.clamp(torch.diagonal(X), *self.bounds).exp())

    def right_inverse(self, A):
        return A.tril(-1) + torch.diag_embed(torch.diagonal(A).log())


# ------------------------------------------------------------------------------------- ExactGP base
class ExactGP(torch.nn.Module):
    """The slice of gpytorch.models.ExactGP the reference relies on [gpytorch-knowledge]:
    train_inputs (tuple) / train_targets, `set_train_data`, and `__call__` that returns the prior
    at the training inputs in train mode and the posterior in eval mode."""

    def __init__(self, train_inputs, train_targets, likelihood):
        super().__init__()
        if train_inputs is not None and torch.is_tensor(train_inputs):
            train_inputs = (train_inputs,)
        self.train_inputs = None if train_inputs is None else tuple(
            t.unsqueeze(-1) if t.ndimension() == 1 else t for t in train_inputs)
        self.train_targets = train_targets
        self.likelihood = likelihood

    def _apply(self, fn, *args, **kwargs):
        if self.train_inputs is not None:
            self.train_inputs = tuple(fn(t) for t in self.train_inputs)
            self.train_targets = fn(self.train_targets)
        return super()._apply(fn, *args, **kwargs)

    # ---- eval-mode factorisation cache (gpytorch keeps its prediction strategy between calls; _engine.PosteriorCache)
    def _prediction_cache(self):
        c = self.__dict__.get("_pred_cache")
        if c is None:
            from . import _engine
            c = self.__dict__["_pred_cache"] = _engine.PosteriorCache()
        return c

    def _drop_prediction_cache(self):
        c = self.__dict__.get("_pred_cache")
        if c is not None:
            c.drop()

    def clear_prediction_cache(self):
        """Release the factorisation an eval-mode model keeps between prediction calls.  The cache is keyed on the identity and
        version counter of every parameter, buffer and the training data: an optimiser step, load_state_dict, train() or
        set_train_data drop it by themselves; an edit through `.data` (no version bump) does not -- call this after one."""
        self._drop_prediction_cache()

    def train(self, mode=True):
        if mode:
            self._drop_prediction_cache()             # parameters are about to change: release the cached factor buffer
        return super().train(mode)

    def __deepcopy__(self, memo):
        cache = self.__dict__.pop("_pred_cache", None)   # a copy starts without the (large) cached workspace
        try:
            import copy
            cls = self.__class__
            new = cls.__new__(cls)
            memo[id(self)] = new
            for k, v in self.__dict__.items():
                new.__dict__[k] = copy.deepcopy(v, memo)
            return new
        finally:
            if cache is not None:
                self.__dict__["_pred_cache"] = cache

    def set_train_data(self, inputs=None, targets=None, strict=True):
        self._drop_prediction_cache()
        if inputs is not None:
            if torch.is_tensor(inputs):
                inputs = (inputs,)
            self.train_inputs = tuple(t.unsqueeze(-1) if t.ndimension() == 1 else t for t in inputs)
        if targets is not None:
            self.train_targets = targets

    def _posterior(self, x, full_cov=False):
        raise NotImplementedError

    def __call__(self, *args, **kwargs):
        x = args[0]
        if x.ndimension() == 1:
            x = x.unsqueeze(-1)
        if self.training:
            tx = self.train_inputs[0]
            # same object or same memory: equal without looking.  Otherwise torch.equal -- a host sync that drains the
            # queue at the head of every training step -- is run once per (input tensor, version) pair and remembered:
            # an in-place change of either tensor bumps its version and brings the comparison back.
            same = x is tx or (x.shape == tx.shape and x.dtype == tx.dtype and x.device == tx.device
                               and x.data_ptr() == tx.data_ptr() and x.stride() == tx.stride())
            if not same:
                seen = _TRAIN_INPUT_SEEN.get(self)
                if seen is not None and seen[0]() is x and seen[1] == x._version and seen[2]() is tx and seen[3] == tx._version:
                    same = True
                elif x.shape == tx.shape and torch.equal(x, tx):
                    same = True
                    _TRAIN_INPUT_SEEN[self] = (weakref.ref(x), x._version, weakref.ref(tx), tx._version)
            if not same:
                raise RuntimeError("You must train on the training inputs!")
            return self.forward(x)
        return self._posterior(x, **kwargs)


def refuse_hyper_grad(full_cov, path=None, input_transform=None):
    """What settings.posterior_hyper_grad does not serve says so by name: a silently partial gradient is worse than a refusal."""
    head = "settings.posterior_hyper_grad (predictions differentiable in hyper-parameters, noise and targets): "
    if path is not None:
        raise NotImplementedError(head + "%s is not served -- the exact posterior of ExactGPModel and of the unsharded ProjectedGPModel is" % path)
    if full_cov:
        raise NotImplementedError(head + "full_cov=True is not served: only the marginal moments (mean, variance) carry the gradient")
    if settings.skip_posterior_variances.on():
        raise NotImplementedError(head + "settings.skip_posterior_variances is not served: its mean carries no gradient")
    if input_transform is not None and any(p.requires_grad for p in input_transform.parameters()):
        raise NotImplementedError(head + "an input_transform with parameters that require a gradient is not served -- the gradient with "
                                  "respect to the training inputs through the posterior is not built; freeze the transform's parameters")


def refuse_fantasy(path):
    """What get_fantasy_model does not serve says so by name."""
    raise NotImplementedError("get_fantasy_model (condition a fitted model on new observations without refactorising): %s is not served -- "
                              "the eval-mode ExactGPModel and the unsharded ProjectedGPModel with a prediction cache are" % path)


class ExactGPModel(ExactGP):
    """Standard exact GP; a batch of `n_tasks` independent GPs via batch dimensions
    (projected_lmc.py:264-321)."""

    def __init__(self, train_x, train_y, likelihood, n_tasks=1, prior_scales=None, prior_width=None,
                 mean_type=_m.ConstantMean, decomp=None, outputscales=False, kernel_type=_k.RBFKernel,
                 ker_kwargs=None, n_inducing_points=None, input_transform=None, **kwargs):
        super().__init__(train_x, train_y, likelihood)
        if ker_kwargs is None:
            ker_kwargs = {}
        # input_transform (a torch.nn.Module | None): a learned feature map in front of the mean and the kernel, gpytorch's deep-kernel
        # convention -- a warping, a linear embedding, a network.  Its parameters are the model's; the MLL reaches them through
        # d logp / dX of the engine (_engine.ExactLatentLogProb).  `dim` is the width of the features.
        if input_transform is not None and n_inducing_points is not None:
            raise NotImplementedError("ExactGPModel(input_transform=..., n_inducing_points=...): the inducing-point (SGPR) path has no "
                                      "gradient with respect to the inputs")
        self.input_transform = input_transform
        self.dim = self._features(self.train_inputs[0][:2].detach(), grad=False).shape[-1]
        self.n_tasks = n_tasks
        self.batch_lik = isinstance(likelihood, (GaussianLikelihood, FixedNoiseGaussianLikelihood))
        # per-point noise (FixedNoiseGaussianLikelihood): the vector rides beside the scalar noise through the engine
        self.fixed_noise = isinstance(likelihood, FixedNoiseGaussianLikelihood)
        if n_inducing_points is not None:
            refuse_fixed_noise(likelihood, "ExactGPModel(n_inducing_points=...) (SGPR)")
        self.mean_module = mean_type(input_size=self.dim, batch_shape=torch.Size([n_tasks]))
        self.covar_module = handle_covar_(kernel_type, dim=self.dim, decomp=decomp, prior_scales=prior_scales,
                                          prior_width=prior_width, outputscales=outputscales, n_funcs=n_tasks,
                                          ker_kwargs=ker_kwargs)
        if n_inducing_points is not None:
            _k.refuse_sm(self.covar_module, "ExactGPModel(n_inducing_points=...) (SGPR)")
            _k.refuse_periodic(self.covar_module, "ExactGPModel(n_inducing_points=...) (SGPR)")
            _k.refuse_rq(self.covar_module, "ExactGPModel(n_inducing_points=...) (SGPR)")
            _k.refuse_dot(self.covar_module, "ExactGPModel(n_inducing_points=...) (SGPR)")
            _k.refuse_product(self.covar_module, "ExactGPModel(n_inducing_points=...) (SGPR)")
            _k.refuse_sum(self.covar_module, "ExactGPModel(n_inducing_points=...) (SGPR)")
            from .sgpr import InducingPointKernel
            self.covar_module = InducingPointKernel(self.covar_module, torch.randn(n_inducing_points, self.dim),
                                                    likelihood)
        if input_transform is not None:
            _engine.require_input_grad_kind(self.covar_module(torch.zeros(2, self.dim)).kind)

    def _features(self, x, grad=True):
        """What the mean and the kernel see: x, or input_transform(x)."""
        if self.input_transform is None:
            return x
        if grad:
            return self.input_transform(x)
        with torch.no_grad():
            return self.input_transform(x)

    def _test_features(self, x):
        """The features of eval-mode test points.  Where x requires a gradient the graph is kept, with the transform's parameters and
        buffers detached: the eval-mode posterior is a function of x alone, and a backward pass must not leave a partial gradient on
        them.  Otherwise as _features(x, grad=False)."""
        if not (torch.is_grad_enabled() and x.requires_grad):
            return self._features(x, grad=False)
        if self.input_transform is None:
            return x
        tf = self.input_transform
        frozen = {k: v.detach() for k, v in list(tf.named_parameters()) + list(tf.named_buffers())}
        return torch.func.functional_call(tf, frozen, (x,))

    def forward(self, x):
        x = self._features(x)
        mean_x = self.mean_module(x)
        covar_x = self.covar_module(x)
        if not self.batch_lik and self.n_tasks > 1:
            return MultitaskMultivariateNormal.from_batch_mvn(MultivariateNormal(mean_x, covar_x))
        return MultivariateNormal(mean_x, covar_x)

    # -- eval-mode posterior (gpytorch DefaultPredictionStrategy), one augmented factorization
    def _latent_targets(self):
        y = self.train_targets
        n = self.train_inputs[0].shape[0]
        if y.dim() == 1:
            return y.reshape(1, n)
        return y if y.shape[-1] == n and y.shape[0] == self.n_tasks else y.T

    def _posterior(self, x, full_cov=False):
        raw_tx = self.train_inputs[0]
        tx, x = self._features(raw_tx, grad=False), self._test_features(x)
        lazy = self.covar_module(tx)
        noise, pnoise = self._latent_noise(), self._point_noise()
        prior_mean = self.mean_module(tx).reshape(self.n_tasks, -1)
        resid = self._latent_targets() - prior_mean
        xs = self.covar_module.select(x)
        # settings.posterior_hyper_grad: the posterior keeps the graph of the kernel's table, the noise and y - m(X)
        hyper = settings.posterior_hyper_grad.on() and torch.is_grad_enabled()
        if hyper:
            refuse_fixed_noise(self.likelihood, "settings.posterior_hyper_grad")
            refuse_hyper_grad(full_cov, "an inducing-point (SGPR) model" if hasattr(lazy, "log_prob_batch") else None, self.input_transform)
        if settings.skip_posterior_variances.on():             # the mean alone, K(x*, X) alpha without K(x*, X)
            refuse_skip_variances(x, full_cov, "an inducing-point (SGPR) model" if hasattr(lazy, "log_prob_batch") else None)
            mean = _engine.exact_posterior_mean(lazy.kind, lazy.x1, lazy.ell.detach(), None if lazy.oscale is None else lazy.oscale.detach(),
                                                noise.detach().to(lazy.ell.dtype), resid.detach(), xs, cache=self._prediction_cache(),
                                                key=_engine.model_state_key(self, *self._cache_key_tensors()), pnoise=pnoise)
            with torch.no_grad():
                mean = mean + self.mean_module(x).reshape(self.n_tasks, -1)
            return self._wrap_posterior(mean, ZeroCovariance(mean))
        if hasattr(lazy, "log_prob_batch"):                    # SGPR predictive moments (sgpr.py)
            with torch.no_grad():
                mean, v = lazy.add_noise(noise.detach().to(lazy.ell.dtype)).posterior(resid.detach(), xs, full_cov=full_cov)
            return self._wrap_posterior(mean + self.mean_module(x).reshape(self.n_tasks, -1), v if full_cov else torch.diag_embed(v))
        keep = (lambda t: t) if hyper else (lambda t: t.detach())
        mean, v = _engine.exact_posterior(lazy.kind, lazy.x1, keep(lazy.ell),
                                          None if lazy.oscale is None else keep(lazy.oscale),
                                          keep(noise).to(lazy.ell.dtype), keep(resid), xs, full_cov=full_cov,
                                          cache=self._prediction_cache(), key=_engine.model_state_key(self, *self._cache_key_tensors()),
                                          pnoise=pnoise)
        mean = mean + self.mean_module(x).reshape(self.n_tasks, -1)
        return self._wrap_posterior(mean, v if full_cov else torch.diag_embed(v))

    def sample_paths(self, num_paths, num_features=1024, generator=None):
        """num_paths draws of the posterior AS FUNCTIONS (pathwise conditioning, paths.PosteriorPaths): evaluable at any number of points
        chosen later, consistent across calls, linear in n*.  Eval mode; the stationary kinds and their additive table."""
        refuse_fixed_noise(self.likelihood, "sample_paths")
        from .paths import sample_paths
        return sample_paths(self, num_paths, num_features, generator)

    # -- fantasy models: condition on new observations through a bordered update of the cached factorisation
    def _cache_key_tensors(self):
        """the training tensors the model's cache key is made of beside its parameters and buffers (_posterior); with per-point noise
        the vector is one of them -- a replaced or in-place-edited vector is a new key"""
        return self.train_inputs[0], self.train_targets, (self.likelihood.noise if getattr(self, "fixed_noise", False) else None)

    def _engine_targets(self):
        """the latent targets y (q, n) the engine is given (_posterior)"""
        tx = self._features(self.train_inputs[0], grad=False)
        return self._latent_targets() - self.mean_module(tx).reshape(self.n_tasks, -1)

    def _latent_noise(self):
        """the scalar noise per latent, (n_tasks); with per-point noise its homoskedastic part (zeros without an additional noise)"""
        lik = self.likelihood
        if getattr(self, "fixed_noise", False):
            return lik.additional_noise(self.n_tasks, self.train_inputs[0])
        return lik.noise.reshape(-1) if self.batch_lik else torch.diagonal(lik.task_noise_matrix()).reshape(-1)

    def _point_noise(self):
        """the per-point noise of the training points, (n) or (n_tasks, n), detached | None"""
        if not getattr(self, "fixed_noise", False):
            return None
        v, n = self.likelihood.noise, self.train_inputs[0].shape[0]
        if v.shape[-1] != n or (v.dim() == 2 and v.shape[0] != self.n_tasks):
            raise ValueError("FixedNoiseGaussianLikelihood: noise of shape %s does not fit %d training points (and %d tasks)"
                             % (tuple(v.shape), n, self.n_tasks))
        return v.detach()

    def _append_train_data(self, inputs, targets):
        """[X; X_new] and the targets in the layout of train_targets: (n,), (n_tasks, n) or (n, n_tasks) (_latent_targets)"""
        tx, y = self.train_inputs[0], self.train_targets
        n = tx.shape[0]
        targets = targets.to(y)
        along = 0 if (y.dim() == 1 or not (y.shape[-1] == n and y.shape[0] == self.n_tasks)) else -1
        if y.dim() != targets.dim() or targets.shape[along] != inputs.shape[0]:
            raise ValueError("get_fantasy_model: targets of shape %s do not continue train_targets of shape %s for %d new inputs"
                             % (tuple(targets.shape), tuple(y.shape), inputs.shape[0]))
        self.train_inputs = (torch.cat([tx, inputs.to(tx)]),)
        self.train_targets = torch.cat([y, targets], dim=along)

    def get_fantasy_model(self, inputs, targets, noise=None):
        """noise (m) | (n_tasks, m): the new points' noise variances, required with a FixedNoiseGaussianLikelihood (the copy's likelihood
        holds the concatenated vector; the new diagonal carries additional noise + jitter + these values) and refused without one.
        A new eval-mode model on [X; inputs] / [y; targets] whose cached factorisation was extended by the m new rows in O(n^2 m)
        (plmc_factor_extend) instead of factorised again: gpytorch's get_fantasy_model [gpytorch-knowledge, unverified offline], the step
        a Bayesian-optimisation or active-learning loop takes after choosing a point.  The model itself, its cache and its predictions
        are unchanged; the copy shares no parameter with it.  Every eval-mode path works on the copy; a fantasy model of a fantasy model
        works.  If a pivot of the border is not positive the copy simply has no cache and its first prediction factorises as usual.
        The copy's cache has the capacity of this model's (predict on this model first with as many test points as the copy will see),
        and keeps no planes of the split engine."""
        if self.training:
            raise RuntimeError("get_fantasy_model is an eval-mode method: call .eval() first")
        if hasattr(self.covar_module, "inducing_points"):
            refuse_fantasy("an inducing-point (SGPR) model")
        if settings.prediction_cache.value() == "off":
            refuse_fantasy('settings.prediction_cache("off") (there is no cached factorisation to extend)')
        if inputs.ndimension() == 1:
            inputs = inputs.unsqueeze(-1)
        pnoise = self._point_noise()
        if pnoise is None and noise is not None:
            raise ValueError("get_fantasy_model: noise= is the new points' per-point noise of a FixedNoiseGaussianLikelihood; this model's "
                             "likelihood is homoskedastic")
        if pnoise is not None:
            if noise is None:
                raise ValueError("get_fantasy_model: a model with a FixedNoiseGaussianLikelihood needs noise=, the new points' noise "
                                 "variances (m) or (n_tasks, m)")
            noise = self.likelihood.noise_covar._checked(torch.as_tensor(noise).detach().to(pnoise))
            if noise.shape[-1] != inputs.shape[0] or noise.dim() != pnoise.dim():
                raise ValueError("get_fantasy_model: noise= of shape %s does not continue the likelihood's noise of shape %s for %d new inputs"
                                 % (tuple(noise.shape), tuple(pnoise.shape), inputs.shape[0]))
        import copy
        from torch.nn.utils import parametrize
        with torch.no_grad(), parametrize.cached():
            raw_tx = self.train_inputs[0]
            inputs = inputs.detach().to(raw_tx)
            lazy = self.covar_module(self._features(raw_tx, grad=False))
            xnew = self.covar_module.select(self._features(inputs, grad=False))
            ws = _engine.extend_cached_factor(lazy.kind, lazy.x1, lazy.ell, lazy.oscale, self._latent_noise().to(lazy.ell.dtype),
                                              self._engine_targets(), xnew, self._prediction_cache(),
                                              _engine.model_state_key(self, *self._cache_key_tensors()), pnoise=pnoise, pnoise_new=noise)
        new = copy.deepcopy(self)
        with torch.no_grad():
            new._append_train_data(inputs, targets.detach())
            if pnoise is not None:
                new.likelihood.noise = torch.cat([pnoise, noise], dim=-1)
        if ws is not None:
            cache = new._prediction_cache()
            key = _engine.model_state_key(new, *new._cache_key_tensors())
            cache.key = key + (lazy.kind,) if (_engine.is_sum(lazy.kind) or _engine.is_dot(lazy.kind)) else key
            cache.ws = ws
        return new

    def _plain_test_inputs(self, x, what):
        """predictive_gradients reads d / d(features seen by the kernel) off the engine: x must BE those features, and the prior mean
        must not depend on it."""
        if self.training:
            raise RuntimeError("%s is an eval-mode method: call .eval() first" % what)
        if x.ndimension() == 1:
            x = x.unsqueeze(-1)
        plain_mean = isinstance(self.mean_module, (_m.ZeroMean, _m.ConstantMean))
        if self.input_transform is not None or self.covar_module.select(x) is not x or not plain_mean:
            raise NotImplementedError("%s serves models without an input_transform, with a kernel on all dimensions and a zero or "
                                      "constant mean; otherwise differentiate model(x) with x.requires_grad_()" % what)
        if hasattr(self.covar_module, "inducing_points"):
            raise NotImplementedError("%s: the inducing-point (SGPR) path has no gradient with respect to the inputs" % what)
        return x.detach()

    def predictive_gradients(self, x):
        """(d mean / dx, d variance / dx) of the eval-mode posterior at x (n*, d), shaped (n*, d), or (n*, n_tasks, d) for a batch of
        tasks: test points do not interact in the marginal moments, so this is the whole Jacobian.  Read off the engine's kernel
        (plmc_posterior_dx); no autograd graph is built."""
        x = self._plain_test_inputs(x, "predictive_gradients")
        raw_tx = self.train_inputs[0]
        lazy = self.covar_module(raw_tx)
        noise = self._latent_noise()
        resid = self._latent_targets() - self.mean_module(raw_tx).reshape(self.n_tasks, -1)
        Jm, Jv = _engine.posterior_jacobians(lazy.kind, lazy.x1, lazy.ell.detach(), None if lazy.oscale is None else lazy.oscale.detach(),
                                             noise.detach().to(lazy.ell.dtype), resid.detach(), x, cache=self._prediction_cache(),
                                             key=_engine.model_state_key(self, *self._cache_key_tensors()), pnoise=self._point_noise())
        Jm, Jv = Jm.to(x.dtype), Jv.to(x.dtype)
        if self.n_tasks == 1 and self.train_targets.dim() == 1:
            return Jm[0], Jv[0]
        return Jm.transpose(0, 1), Jv.transpose(0, 1)

    def _wrap_posterior(self, mean, cov):
        if not self.batch_lik and self.n_tasks > 1:
            return MultitaskMultivariateNormal.from_batch_mvn(MultivariateNormal(mean, cov))
        if self.n_tasks == 1 and self.train_targets.dim() == 1:
            return MultivariateNormal(mean[0], cov[0])
        return MultivariateNormal(mean, cov)

    def compute_loo(self, output=None, complex_mean=False, eps=1e-6):
        """Leave-one-out variances and residuals (projected_lmc.py:371-436): returns
        (sigma2, y - mu_loo), shaped like train_y (n,) or (n, n_tasks).  Shares the blocked sweep with
        the MLL; diag(Khat^-1) comes out of the fused K^-1 kernel.  `complex_mean` (basis-function
        means) is not supported."""
        if complex_mean:
            raise ValueError("A complex mean treatment was required, but the model mean function doesn't allow it !")
        refuse_fixed_noise(self.likelihood, "compute_loo")
        tx = self._features(self.train_inputs[0], grad=False)
        lazy = self.covar_module(tx)
        lik = self.likelihood
        if self.batch_lik:
            noise = lik.noise.reshape(-1).clamp_min(eps) if self.n_tasks == 1 else lik.noise.reshape(-1)
        else:
            noise = torch.diagonal(lik.task_noise_matrix()).reshape(-1)
        resid = self._latent_targets() - self.mean_module(tx).reshape(self.n_tasks, -1)
        with torch.no_grad():
            s2, r = _engine.exact_loo(lazy.kind, lazy.x1, lazy.ell, lazy.oscale, noise.to(lazy.ell.dtype), resid)
        if self.train_targets.dim() == 1:
            return s2[0], r[0]
        return s2.T, r.T

    def kernel_cond(self):
        """2-norm condition number of the noisy train covariance K + sigma^2 I (projected_lmc.py:367-369); a
        diagnostic: the matrix is materialised and handed to torch.linalg.cond."""
        tx = self.train_inputs[0]
        lazy = self.likelihood(self.forward(tx)).lazy_covariance_matrix
        return torch.linalg.cond(lazy.to_dense())

    # -- inspection helpers (projected_lmc.py:324-365)
    def _kernel(self):
        """The model's kernel without the inducing-point wrapper (sgpr.InducingPointKernel) around it."""
        cm = self.covar_module
        return cm.base_kernel if hasattr(cm, "inducing_points") else cm

    def _base(self):
        cm = self._kernel()
        return cm.base_kernel if hasattr(cm, "base_kernel") else cm

    def lscales(self, unpacked=True):
        cm = self._kernel()
        if hasattr(cm, "kernels"):                                   # additive decomposition: one entry per sub-kernel
            return [(k.base_kernel if hasattr(k, "base_kernel") else k).lengthscale.data.squeeze() for k in cm.kernels]
        scales = self._base().lengthscale.data.squeeze()
        return scales if unpacked else [scales]

    def outputscale(self, unpacked=False):
        n_funcs = self.n_latents if hasattr(self, "n_latents") else self.n_tasks
        cm = self._kernel()
        if hasattr(cm, "kernels"):
            res = torch.zeros((n_funcs, len(cm.kernels)))
            for i_ker, k in enumerate(cm.kernels):
                res[:, i_ker] = k.outputscale.data.squeeze()
            return res
        res = torch.zeros((n_funcs, 1))
        res[:, 0] = cm.outputscale.data.squeeze()
        return res.squeeze() if unpacked else res
