"""Posterior draws as functions: pathwise conditioning (Matheron's rule),

    f(.) = m(.) + f_prior(.) + K(., X) Khat^-1 (y - m(X) - f_prior(X) - eps),      eps ~ N(0, sigma^2 I),

with f_prior a random-Fourier-feature draw of the prior,  f_prior(x) = sqrt(2 os / m) sum_j w_j cos(2 pi (omega_j . x + b_j)).  A path
is linear in the number of points it is evaluated at, evaluable at points chosen later and consistent across calls; a joint draw
(`model(x).sample()`) is none of these.  Both products run on the engine without a cross-covariance matrix: plmc_rff_matvec for the
prior part, plmc_cross_matvec for the update, whose weights v = Khat^-1 (...) are solved for all paths at once against the model's
cached factor (_engine.solve_cached).

Served kernels: the stationary kinds (rbf, matern12 / 32 / 52), bare or in a ScaleKernel, and their additive table (`decomp`, or a sum
of kernels of one stationary kind).  The spectral draws are made on the host from `generator`:
    RBF         omega = Z / (2 pi ell),                        Z ~ N(0, I)
    Matern-nu   omega = Z sqrt(2 nu / g) / (2 pi ell),         g ~ chi^2(2 nu) as the sum of 2 nu squared normals (1, 3 or 5 of them)
in revolutions per unit of x.  An additive table draws `num_features` features per component -- an infinite lengthscale gives frequency 0
on that dimension -- with the component's output scale in the scale of its features, and concatenates them.
"""
import math

import torch

from . import _engine

NU2 = {"rbf": None, "matern12": 1, "matern32": 3, "matern52": 5}      # 2 nu of the served kinds


def spectral_frequencies(kind, shape, generator=None, device="cpu"):
    """Frequencies in REVOLUTIONS of a unit-lengthscale kernel of `kind`, float64 of shape (*shape, d): the mean of cos(2 pi omega . tau)
    over them is k(tau).  shape = (..., m, d)."""
    if kind not in NU2:
        raise NotImplementedError("spectral draws serve the stationary kinds %s, not %r" % (", ".join(NU2), kind))
    Z = torch.randn(*shape, dtype=torch.float64, generator=generator, device=device)
    k = NU2[kind]
    if k is not None:
        g = torch.randn(*shape[:-1], k, dtype=torch.float64, generator=generator, device=device).square().sum(-1, keepdim=True)
        Z = Z * (k / g).sqrt()
    return Z / (2.0 * math.pi)


def _refuse(model):
    """The models and kernels sample_paths does not serve, by name.  -> (lazy kernel of the training features, is_projected)"""
    from .multitask import MultitaskGPModel
    from .projected import ProjectedGPModel
    name = type(model).__name__
    if isinstance(model, MultitaskGPModel):
        raise NotImplementedError("sample_paths: the dense LMC model (%s) is not served -- its tasks share one joint factorisation" % name)
    if getattr(model, "training", False):
        raise RuntimeError("sample_paths is an eval-mode method: call .eval() first")
    projected = isinstance(model, ProjectedGPModel)
    if projected and model.latent_ids is not None:
        raise NotImplementedError("sample_paths: the latent-sharded ProjectedGPModel (latent_shard / latent_ids) is not served")
    if hasattr(model.covar_module, "inducing_points"):
        raise NotImplementedError("sample_paths: the inducing-point (SGPR) model is not served -- there is no exact factor to condition on")
    lazy = model.covar_module(model._features(model.train_inputs[0], grad=False))
    if hasattr(lazy, "log_prob_batch"):
        raise NotImplementedError("sample_paths: the inducing-point (SGPR) model is not served -- there is no exact factor to condition on")
    if lazy.kind not in NU2 or lazy.ell.dim() not in (2, 3):
        raise NotImplementedError("sample_paths: kernel kind %r has no random-Fourier-feature prior here (served: %s, bare, in a ScaleKernel "
                                  "or as an additive table of one kind)" % (lazy.kind, ", ".join(NU2)))
    return lazy, projected


class PosteriorPaths:
    """num_paths posterior draws of one model as functions (model.sample_paths).  paths(x), x (n*, d), any n* ->
    (num_paths, n*) for a single-output ExactGPModel, (num_paths, n*, n_tasks) for a batch of tasks, (num_paths, n*, p) for
    ProjectedGPModel (latents mixed by H as the posterior mean is, no observation noise added).  Under no_grad;
    paths(x, differentiable=True) attaches the result to the graph of an x that requires a gradient, paths.jacobian(x) returns
    d paths / dx without a graph.
    Read-only tensors: freq (q, M, d) and phase (q, M) in revolutions, feature_scale (q, M) = sqrt(2 os / m) per feature, w (P, q, M),
    eps (P, q, n) and v (q, n, P) = Khat^-1 (y - m(X) - f_prior(X) - eps).  The paths belong to the model's parameters and data at the
    time they were drawn."""

    def __init__(self, model, lazy, projected, freq, phase, feature_scale, w, eps):
        self._model, self._projected = model, projected
        self._kind = lazy.kind
        dt = lazy.ell.dtype
        self._X = lazy.x1.detach().to(dt).contiguous()
        self._ell = lazy.ell.detach().contiguous()
        self._osc = None if lazy.oscale is None else lazy.oscale.detach().contiguous()
        self._freq, self._phase, self._fscale, self._w, self._eps = freq, phase, feature_scale, w, eps
        self._Wt = (w * feature_scale[None]).permute(1, 2, 0).contiguous()          # (q, M, P)
        self._v = self._solve()

    freq = property(lambda self: self._freq)
    phase = property(lambda self: self._phase)
    feature_scale = property(lambda self: self._fscale)
    w = property(lambda self: self._w)
    eps = property(lambda self: self._eps)
    v = property(lambda self: self._v)
    num_paths = property(lambda self: self._w.shape[0])

    def _targets(self):
        """(noise (q), y - m(X) (q, n), state key) of the latent GPs, as the model's posterior takes them."""
        m = self._model
        raw_tx = m.train_inputs[0]
        if self._projected:
            return m.projected_noise(), m.project_data(m.train_y), _engine.model_state_key(m, raw_tx, m.train_y)
        lik = m.likelihood
        noise = lik.noise.reshape(-1) if m.batch_lik else torch.diagonal(lik.task_noise_matrix()).reshape(-1)
        resid = m._latent_targets() - m.mean_module(m._features(raw_tx, grad=False)).reshape(m.n_tasks, -1)
        return noise, resid, _engine.model_state_key(m, raw_tx, m.train_targets)

    def _solve(self):
        from torch.nn.utils import parametrize
        with torch.no_grad(), parametrize.cached():
            noise, resid, key = self._targets()
            dt = self._ell.dtype
            fX = _engine.rff_matvec(self._freq, self._phase, self._X, self._Wt)                          # (q, n, P)
            rhs = resid.to(dt)[:, None, :] - fX.permute(0, 2, 1) - self._eps.permute(1, 0, 2)
            return _engine.solve_cached(self._kind, self._X, self._ell, self._osc, noise.to(dt), rhs.contiguous(),
                                        cache=self._model._prediction_cache(), key=key)

    def with_draws(self, w=None, eps=None):
        """The paths of other prior weights w (P, q, M) and / or noise draws eps (P, q, n) on the same features: v is solved again."""
        w = self._w if w is None else w.to(self._w)
        eps = self._eps if eps is None else eps.to(self._eps)
        if w.shape[1:] != self._w.shape[1:] or eps.shape[1:] != self._eps.shape[1:] or w.shape[0] != eps.shape[0]:
            raise ValueError("with_draws: w (P, q, M) and eps (P, q, n) with the features' q and M and the model's n")
        new = object.__new__(PosteriorPaths)
        new.__dict__.update(self.__dict__)
        new._w, new._eps = w, eps
        new._Wt = (w * self._fscale[None]).permute(1, 2, 0).contiguous()
        new._v = new._solve()
        return new

    def _latents(self, xs):
        """(q, n*, P): the latent draws at the kernel's features xs (n*, d'), the two fused products."""
        lat = _engine.rff_matvec(self._freq, self._phase, xs, self._Wt)
        return lat + _engine.cross_matvec(self._kind, xs, self._X, self._ell, self._osc, self._v)

    def _latents_dx(self, xs, G=None, column=None):
        """(q, n*, d') float64: d _latents / d xs contracted with G (q, n*, P), or the Jacobian of path `column` (G None)."""
        Wt, v = self._Wt, self._v
        if G is None:
            Wt, v = Wt[:, :, column:column + 1], v[:, :, column:column + 1]
        return (_engine.cross_matvec_dx(self._kind, xs, self._X, self._ell, self._osc, v, G)
                + _engine.rff_matvec_dx(self._freq, self._phase, xs, Wt, G))

    def _outputs(self, lat, xf):
        """The latent draws (q, n*, P) as the model's outputs: mixed by H, or with the prior mean of the features xf."""
        m = self._model
        if self._projected:
            Ht = m.lmc_coefficients().detach().to(lat.dtype)
            return torch.einsum("qsc,qp->csp", lat, Ht)
        lat = lat + m.mean_module(xf).reshape(m.n_tasks, -1).to(lat.dtype)[:, :, None]
        if m.n_tasks == 1 and m.train_targets.dim() == 1:
            return lat[0].T
        return lat.permute(2, 1, 0)

    def __call__(self, x, differentiable=False):
        """The paths at x (n*, d).  differentiable=True: where x requires a gradient the result is attached to its graph -- the two
        products and their input derivative (plmc_cross_matvec_dx, plmc_rff_matvec_dx) are one node over the kernel's
        features, the mixing, the prior mean and an input_transform plain autograd around it (the transform's parameters detached, as
        the differentiable prediction takes them).  Same values, bit for bit; once differentiable.  An x that needs no gradient is
        evaluated as without the keyword."""
        m = self._model
        if differentiable and torch.is_grad_enabled() and x.requires_grad:
            if x.ndimension() == 1:
                x = x.unsqueeze(-1)
            _engine.require_input_grad_kind(self._kind)
            xf = m._test_features(x)
            xs = m.covar_module.select(xf).to(self._ell.dtype)
            return self._outputs(_PathLatents.apply(xs, self), xf)
        if x.requires_grad and not differentiable:
            raise NotImplementedError("PosteriorPaths: an x that requires a gradient is not served -- paths carry no derivative with "
                                      "respect to x; detach it")
        with torch.no_grad():
            if x.ndimension() == 1:
                x = x.unsqueeze(-1)
            xf = m._features(x, grad=False)
            xs = m.covar_module.select(xf).to(self._ell.dtype)
            return self._outputs(self._latents(xs), xf)                                                  # (q, n*, P) mixed

    def jacobian(self, x):
        """d paths(x) / dx, shaped paths(x).shape + (d,): test points do not interact in a path, so this is the whole Jacobian.  No graph
        is built.  It COSTS ONE GRADIENT PER PATH -- a G = NULL, r = 1 pair of kernel calls each -- so for a scalar objective of the paths
        paths(x, differentiable=True) and one backward pass is num_paths times cheaper.  x as predictive_gradients takes it: the model has
        no input_transform, a kernel on all dimensions and a zero or constant mean."""
        m = self._model
        x = m._plain_test_inputs(x, "PosteriorPaths.jacobian")
        with torch.no_grad():
            xs = x.to(self._ell.dtype)
            J = torch.stack([self._latents_dx(xs, column=c) for c in range(self.num_paths)])             # (P, q, n*, d) float64
            if self._projected:
                Ht = m.lmc_coefficients().detach().to(J.dtype)
                return torch.einsum("cqsk,qp->cspk", J, Ht).to(x.dtype)
            if m.n_tasks == 1 and m.train_targets.dim() == 1:
                return J[:, 0].to(x.dtype)
            return J.permute(0, 2, 1, 3).to(x.dtype)


class _PathLatents(torch.autograd.Function):
    """PosteriorPaths._latents as a function of the kernel's features: backward is _latents_dx with the upstream gradient as G, summed over
    the latents.  The draws, the weights and the hyper-parameters are constants of this node.  Not twice differentiable."""

    @staticmethod
    def forward(ctx, xs, paths):
        ctx.paths = paths
        ctx.save_for_backward(xs)
        return paths._latents(xs.detach())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (xs,) = ctx.saved_tensors
        return ctx.paths._latents_dx(xs, g.contiguous()).sum(0).to(xs.dtype), None


def sample_paths(model, num_paths, num_features=1024, generator=None):
    """model.sample_paths: draw the features, the prior weights and the noise on the host from `generator` (None: the default one) in
    float64, move them to the model's device and dtype, and condition (PosteriorPaths)."""
    lazy, projected = _refuse(model)
    if num_paths < 1 or num_features < 1:
        raise ValueError("sample_paths: num_paths >= 1 and num_features >= 1")
    P, m = int(num_paths), int(num_features)
    ell = lazy.ell.detach()
    dt, dev = ell.dtype, ell.device
    if ell.dim() == 2:
        ell = ell[:, None, :]
    q, G, d = ell.shape
    osc = lazy.oscale
    osc = torch.ones(q, G, dtype=torch.float64) if osc is None else osc.detach().reshape(q, G).to("cpu", torch.float64)
    n = lazy.x1.shape[0]
    gdev = "cpu" if generator is None else generator.device
    draw = dict(dtype=torch.float64, generator=generator, device=gdev)
    omega = spectral_frequencies(lazy.kind, (q, G, m, d), generator, gdev).cpu()
    freq = (omega / ell.to("cpu", torch.float64)[:, :, None, :]).reshape(q, G * m, d)                 # ell = +inf: frequency 0
    phase = torch.rand(q, G * m, **draw).cpu()
    w = torch.randn(P, q, G * m, **draw).cpu()
    z = torch.randn(P, q, n, **draw).cpu()
    fscale = (2.0 * osc / m).sqrt()[:, :, None].expand(q, G, m).reshape(q, G * m)
    if projected:
        noise = model.projected_noise()
    else:
        lik = model.likelihood
        noise = lik.noise.reshape(-1) if model.batch_lik else torch.diagonal(lik.task_noise_matrix()).reshape(-1)
    eps = z * noise.detach().to("cpu", torch.float64).sqrt()[None, :, None]
    to = lambda t: t.to(dev, dt).contiguous()
    return PosteriorPaths(model, lazy, projected, to(freq), to(phase), to(fscale), to(w), to(eps))
