"""Kernel modules: parameter containers with gpytorch's constructor / attribute surface
(`ard_num_dims`, `active_dims`, `batch_shape`, `lengthscale_prior`, `.lengthscale`,
`ScaleKernel.outputscale`, `.base_kernel`) as used by handle_covar_ (projected_lmc.py:151-179).

Calling a kernel does NOT build an n x n tensor: it returns a `LazyKernel` descriptor that the
HIP engine consumes (fused assembly inside the factorization).  `.evaluate()` / `.to_dense()`
materialise through the HIP cross-assembly kernel when a dense matrix is explicitly asked for.
"""
import torch

from .constraints import Positive

_MATERN_KIND = {0.5: "matern12", 1.5: "matern32", 2.5: "matern52"}


class Kernel(torch.nn.Module):
    has_lengthscale = False
    kind = None

    def __init__(self, ard_num_dims=None, batch_shape=torch.Size(), active_dims=None, lengthscale_prior=None,
                 lengthscale_constraint=None, **kwargs):
        super().__init__()
        self.ard_num_dims = ard_num_dims
        self.batch_shape = torch.Size(batch_shape)
        self.active_dims = None if active_dims is None else tuple(int(a) for a in active_dims)
        self.lengthscale_prior = lengthscale_prior
        if self.has_lengthscale:
            nd = 1 if ard_num_dims is None else ard_num_dims
            self.register_parameter("raw_lengthscale", torch.nn.Parameter(torch.zeros(*self.batch_shape, 1, nd)))
            self.raw_lengthscale_constraint = lengthscale_constraint or Positive()

    @property
    def lengthscale(self):
        return self.raw_lengthscale_constraint.transform(self.raw_lengthscale) if self.has_lengthscale else None

    @lengthscale.setter
    def lengthscale(self, value):
        value = torch.as_tensor(value, dtype=self.raw_lengthscale.dtype, device=self.raw_lengthscale.device)
        raw = self.raw_lengthscale_constraint.inverse_transform(value)
        with torch.no_grad():
            self.raw_lengthscale.copy_(raw.expand_as(self.raw_lengthscale))

    # -- descriptor pieces consumed by the engine
    def _ell(self, d, like=None):
        """(q, d) lengthscales (q = prod(batch_shape) or 1)."""
        ell = self.lengthscale.reshape(-1, self.lengthscale.shape[-1])
        return ell.expand(ell.shape[0], d) if ell.shape[-1] != d else ell

    def _pieces(self, d, like=None):
        return self.kind, self._ell(d, like), None

    def select(self, x):
        if self.active_dims is not None and len(self.active_dims) != x.shape[-1]:
            return x[..., list(self.active_dims)]
        return x

    def forward(self, x1, x2=None, **params):
        x1 = self.select(x1)
        x2 = x1 if x2 is None else self.select(x2)
        kind, ell, osc = self._pieces(x1.shape[-1], x1)
        return LazyKernel(kind, x1, x2, ell, osc, self.batch_shape)

    def __mul__(self, other):
        return ProductKernel(self, other)

    def __add__(self, other):
        """k1 + k2: additive.AdditiveKernel [gpytorch-knowledge: AdditiveKernel, `kernels` ModuleList, unverified offline], flattened."""
        from .additive import AdditiveKernel
        return AdditiveKernel(self, *(other.kernels if isinstance(other, AdditiveKernel) else [other]))


class RBFKernel(Kernel):
    has_lengthscale = True
    kind = "rbf"


class MaternKernel(Kernel):
    has_lengthscale = True

    def __init__(self, nu=2.5, **kwargs):
        if nu not in _MATERN_KIND:
            raise RuntimeError("nu expected to be 0.5, 1.5, or 2.5")
        super().__init__(**kwargs)
        self.nu = nu
        self.kind = _MATERN_KIND[nu]


class SplineKernel(Kernel):
    """The reference's SplineKernel (projected_lmc.py:26-36): k(x, x') = prod_k [1 + m M + m^2 (M - m / 3) / 2] with
    m = min(x_k, x'_k), M = max(x_k, x'_k); no lengthscale, k(x, x) = prod_k (1 + x_k^2 + x_k^3 / 3).  On the HIP path it
    is kernel kind "spline" of the assembly / cross / gradient kernels (exact GP and projected models; the dense-LMC and
    variational engines take the stationary kinds only)."""
    has_lengthscale = False
    kind = "spline"
    is_stationary = True                      # as declared by the reference

    def _ell(self, d, like=None):
        q = max(1, int(self.batch_shape.numel()))
        if like is None:
            return torch.ones(q, d)
        return torch.ones(q, d, dtype=like.dtype, device=like.device)


class SpectralMixtureKernel(Kernel):
    """Spectral-mixture kernel [gpytorch-knowledge: SpectralMixtureKernel; realdata_experiments.py:130-140 runs the tidal study with it]:
        k(x, x') = sum_m w_m exp(-2 pi^2 sum_k s_mk^2 tau_k^2) prod_k cos(2 pi mu_mk tau_k),   tau = x - x'.
    gpytorch's parameter names and shapes, so state dicts line up: raw_mixture_weights (*batch, M), raw_mixture_means and
    raw_mixture_scales (*batch, M, 1, d), zero-initialised, Positive constraints.  No lengthscale.  On the HIP path it is kernel kind
    "sm" of the batched exact engine (include/plmc.h, "Spectral-mixture kernel"); SGPR, the dense LMC / ICM and the variational models
    refuse it."""
    has_lengthscale = False
    kind = "sm"
    is_stationary = True

    def __init__(self, num_mixtures=None, ard_num_dims=1, batch_shape=torch.Size(), active_dims=None, mixture_scales_prior=None,
                 mixture_scales_constraint=None, mixture_means_prior=None, mixture_means_constraint=None,
                 mixture_weights_prior=None, mixture_weights_constraint=None, **kwargs):
        if num_mixtures is None:
            raise RuntimeError("num_mixtures is a required argument")
        kwargs.pop("lengthscale_prior", None)                 # (handle_covar_ passes one to every kernel; this one has no lengthscale)
        super().__init__(ard_num_dims=ard_num_dims, batch_shape=batch_shape, active_dims=active_dims, **kwargs)
        self.num_mixtures = int(num_mixtures)
        M, d = self.num_mixtures, 1 if ard_num_dims is None else int(ard_num_dims)
        self.register_parameter("raw_mixture_weights", torch.nn.Parameter(torch.zeros(*self.batch_shape, M)))
        self.register_parameter("raw_mixture_means", torch.nn.Parameter(torch.zeros(*self.batch_shape, M, 1, d)))
        self.register_parameter("raw_mixture_scales", torch.nn.Parameter(torch.zeros(*self.batch_shape, M, 1, d)))
        self.raw_mixture_weights_constraint = mixture_weights_constraint or Positive()
        self.raw_mixture_means_constraint = mixture_means_constraint or Positive()
        self.raw_mixture_scales_constraint = mixture_scales_constraint or Positive()

    def _get(self, name):
        return getattr(self, "raw_%s_constraint" % name).transform(getattr(self, "raw_" + name))

    def _set(self, name, value):
        raw = getattr(self, "raw_" + name)
        value = torch.as_tensor(value, dtype=raw.dtype, device=raw.device)
        with torch.no_grad():
            raw.copy_(getattr(self, "raw_%s_constraint" % name).inverse_transform(value).expand_as(raw))

    mixture_weights = property(lambda self: self._get("mixture_weights"), lambda self, v: self._set("mixture_weights", v))
    mixture_means = property(lambda self: self._get("mixture_means"), lambda self, v: self._set("mixture_means", v))
    mixture_scales = property(lambda self: self._get("mixture_scales"), lambda self, v: self._set("mixture_scales", v))

    def initialize_from_data(self, train_x, train_y, **kwargs):
        """[gpytorch-knowledge: SpectralMixtureKernel.initialize_from_data] per input dimension: scales = 1 / |N(0, max_dist^2)|, means ~
        U(0, 0.5 / min_dist) with zero gaps between sorted inputs taken as 1e10, weights = std(y) / M."""
        with torch.no_grad():
            if train_x.dim() == 1:
                train_x = train_x.unsqueeze(-1)
            train_x = self.select(train_x)
            srt = train_x.sort(dim=-2)[0]
            max_dist = srt[..., -1, :] - srt[..., 0, :]
            gaps = srt[..., 1:, :] - srt[..., :-1, :]
            gaps = torch.where(gaps.eq(0.0), torch.full_like(gaps, 1.0e10), gaps)
            min_dist = gaps.sort(dim=-2)[0][..., 0, :]
            raw = self.raw_mixture_scales
            like = dict(dtype=raw.dtype, device=raw.device)
            max_dist, min_dist = max_dist.to(**like), min_dist.to(**like)
            self.mixture_scales = (torch.randn_like(raw) * max_dist).abs().reciprocal()
            self.mixture_means = torch.rand_like(self.raw_mixture_means) * (0.5 / min_dist)
            self.mixture_weights = train_y.std().to(**like) / self.num_mixtures

    def _pieces(self, d, like=None):
        M = self.num_mixtures
        scales = self.mixture_scales.reshape(-1, M, self.mixture_scales.shape[-1])
        means = self.mixture_means.reshape(-1, M, self.mixture_means.shape[-1])
        if scales.shape[-1] != d:
            scales, means = scales.expand(-1, M, d), means.expand(-1, M, d)
        return self.kind, torch.stack([scales, means], 1), self.mixture_weights.reshape(-1, M)


class PeriodicKernel(Kernel):
    """Periodic kernel [gpytorch-knowledge: PeriodicKernel.forward, v1.11, unverified offline]:
        k(x, x') = exp(-2 sum_k sin^2(pi (x_k - x'_k) / p_k) / ell_k)            (the lengthscale is not squared).
    gpytorch's parameter names and shapes, so state dicts line up: raw_lengthscale and raw_period_length (*batch, 1, d),
    zero-initialised, Positive constraints.  On the HIP path it is kernel kind "periodic" of the batched exact engine (include/plmc.h,
    "Periodic kernel"); the additive kernel, SGPR, the dense LMC / ICM and the variational models refuse it."""
    has_lengthscale = True
    kind = "periodic"
    is_stationary = True

    def __init__(self, ard_num_dims=None, batch_shape=torch.Size(), active_dims=None, period_length_prior=None,
                 period_length_constraint=None, lengthscale_prior=None, lengthscale_constraint=None, **kwargs):
        super().__init__(ard_num_dims=ard_num_dims, batch_shape=batch_shape, active_dims=active_dims,
                         lengthscale_prior=lengthscale_prior, lengthscale_constraint=lengthscale_constraint, **kwargs)
        nd = 1 if ard_num_dims is None else int(ard_num_dims)
        self.period_length_prior = period_length_prior
        self.register_parameter("raw_period_length", torch.nn.Parameter(torch.zeros(*self.batch_shape, 1, nd)))
        self.raw_period_length_constraint = period_length_constraint or Positive()

    @property
    def period_length(self):
        return self.raw_period_length_constraint.transform(self.raw_period_length)

    @period_length.setter
    def period_length(self, value):
        value = torch.as_tensor(value, dtype=self.raw_period_length.dtype, device=self.raw_period_length.device)
        with torch.no_grad():
            self.raw_period_length.copy_(self.raw_period_length_constraint.inverse_transform(value).expand_as(self.raw_period_length))

    def _pieces(self, d, like=None):
        """The table (q, 2, d) = [lengthscale | period] and no output scale."""
        period = self.period_length.reshape(-1, self.period_length.shape[-1])
        if period.shape[-1] != d:
            period = period.expand(period.shape[0], d)
        return self.kind, torch.stack([self._ell(d, like), period], 1), None


class RQKernel(Kernel):
    """Rational-quadratic kernel [gpytorch-knowledge: RQKernel, unverified offline]:
        k(x, x') = (1 + r^2 / (2 alpha))^(-alpha),   r^2 = sum_k ((x_k - x'_k) / ell_k)^2,
    the scale mixture of RBF kernels (alpha -> inf: the RBF kernel).  gpytorch's parameter names and shapes, so state dicts line up:
    raw_lengthscale (*batch, 1, d) and raw_alpha (*batch, 1), zero-initialised, Positive constraints.  On the HIP path it is kernel kind
    "rq" of the batched exact engine (include/plmc.h, "Rational-quadratic kernel"); the additive kernel, SGPR, the dense LMC / ICM and
    the variational models refuse it."""
    has_lengthscale = True
    kind = "rq"
    is_stationary = True

    def __init__(self, ard_num_dims=None, batch_shape=torch.Size(), active_dims=None, alpha_constraint=None, lengthscale_prior=None,
                 lengthscale_constraint=None, **kwargs):
        super().__init__(ard_num_dims=ard_num_dims, batch_shape=batch_shape, active_dims=active_dims,
                         lengthscale_prior=lengthscale_prior, lengthscale_constraint=lengthscale_constraint, **kwargs)
        self.register_parameter("raw_alpha", torch.nn.Parameter(torch.zeros(*self.batch_shape, 1)))
        self.raw_alpha_constraint = alpha_constraint or Positive()

    @property
    def alpha(self):
        return self.raw_alpha_constraint.transform(self.raw_alpha)

    @alpha.setter
    def alpha(self, value):
        value = torch.as_tensor(value, dtype=self.raw_alpha.dtype, device=self.raw_alpha.device)
        with torch.no_grad():
            self.raw_alpha.copy_(self.raw_alpha_constraint.inverse_transform(value).expand_as(self.raw_alpha))

    def _pieces(self, d, like=None):
        """The table (q, d + 1) = [lengthscales | alpha] and no output scale."""
        return self.kind, torch.cat([self._ell(d, like), self.alpha.reshape(-1, 1)], 1), None


def dot_power(kind):
    """The power P of a dot-product kind -- "linear" (1) or "poly<P>" -- or None for every other kind.  P travels in the kind string, so
    it survives add_noise and tells prediction-cache keys apart."""
    if kind == "linear":
        return 1
    if isinstance(kind, str) and kind.startswith("poly") and kind[4:].isdigit():
        return int(kind[4:])
    return None


class _DotKernel(Kernel):
    """What LinearKernel and PolynomialKernel share: the dot-product family of the batched exact engine (include/plmc.h, "Dot-product
    kernels"),  k(x, x') = (c + sum_k v_k x_k x'_k)^P.  No lengthscale; NOT stationary (k(x, x) depends on x).  SGPR, the dense LMC / ICM,
    the variational models, the additive kernel and the product kernel refuse them."""
    has_lengthscale = False
    is_stationary = False

    def _register(self, name, shape, constraint):
        self.register_parameter("raw_" + name, torch.nn.Parameter(torch.zeros(*shape)))
        setattr(self, "raw_%s_constraint" % name, constraint or Positive())

    def _get(self, name):
        return getattr(self, "raw_%s_constraint" % name).transform(getattr(self, "raw_" + name))

    def _set(self, name, value):
        raw = getattr(self, "raw_" + name)
        value = torch.as_tensor(value, dtype=raw.dtype, device=raw.device)
        with torch.no_grad():
            raw.copy_(getattr(self, "raw_%s_constraint" % name).inverse_transform(value).expand_as(raw))


class LinearKernel(_DotKernel):
    """Linear kernel [gpytorch-knowledge: LinearKernel, unverified offline]: k(x, x') = sum_k v_k x_k x'_k -- Bayesian linear regression
    with prior variance v_k on the k-th weight.  gpytorch's parameter name and shape, so state dicts line up: raw_variance
    (*batch, 1, 1 if ard_num_dims is None else ard_num_dims), zero-initialised, Positive constraint.  Kernel kind "linear".  The prior has
    rank <= d: without noise the matrix is singular for n > d."""
    kind = "linear"

    def __init__(self, ard_num_dims=None, batch_shape=torch.Size(), active_dims=None, variance_prior=None, variance_constraint=None,
                 **kwargs):
        kwargs.pop("lengthscale_prior", None)                 # (handle_covar_ passes one to every kernel; this one has no lengthscale)
        kwargs.pop("lengthscale_constraint", None)
        super().__init__(ard_num_dims=ard_num_dims, batch_shape=batch_shape, active_dims=active_dims, **kwargs)
        self.variance_prior = variance_prior
        self._register("variance", (*self.batch_shape, 1, 1 if ard_num_dims is None else int(ard_num_dims)), variance_constraint)

    variance = property(lambda self: self._get("variance"), lambda self, v: self._set("variance", v))

    def _pieces(self, d, like=None):
        """The table (q, d + 1) = [variances | 0] and no output scale; the offset column is a constant."""
        v = self.variance.reshape(-1, self.variance.shape[-1])
        if v.shape[-1] != d:
            v = v.expand(v.shape[0], d)
        return self.kind, torch.cat([v, torch.zeros_like(v[:, :1])], 1), None


class PolynomialKernel(_DotKernel):
    """Polynomial kernel [gpytorch-knowledge: PolynomialKernel, unverified offline]: k(x, x') = (x . x' + c)^P, P an integer >= 1.
    gpytorch's parameter name and shape: raw_offset (*batch, 1), zero-initialised, Positive constraint.  Kernel kind "poly<P>": the power
    is part of the kind."""

    def __init__(self, power=None, offset_prior=None, offset_constraint=None, batch_shape=torch.Size(), active_dims=None, **kwargs):
        if power is None:
            raise RuntimeError("power is a required argument")
        if isinstance(power, bool) or not isinstance(power, int) or power < 1:
            raise RuntimeError("power expected to be an int >= 1, got %r" % (power,))
        kwargs.pop("lengthscale_prior", None)                 # (see LinearKernel)
        kwargs.pop("lengthscale_constraint", None)
        super().__init__(ard_num_dims=kwargs.pop("ard_num_dims", None), batch_shape=batch_shape, active_dims=active_dims, **kwargs)
        self.power = power
        self.kind = "poly%d" % power
        self.offset_prior = offset_prior
        self._register("offset", (*self.batch_shape, 1), offset_constraint)

    offset = property(lambda self: self._get("offset"), lambda self, v: self._set("offset", v))

    def _pieces(self, d, like=None):
        """The table (q, d + 1) = [1 | offset] and no output scale; the variance columns are constants."""
        c = self.offset.reshape(-1, 1)
        return self.kind, torch.cat([torch.ones(c.shape[0], d, dtype=c.dtype, device=c.device), c], 1), None


class ProductKernel(Kernel):
    """Product of kernels [gpytorch-knowledge: ProductKernel, the elementwise product of its factors, unverified offline] -- what
    `k1 * k2` returns.  One product is served, the LOCALLY PERIODIC kernel PeriodicKernel * RBFKernel (either order):
        k(x, x') = exp(-2 sum_k sin^2(pi tau_k / p_k) / ell_k - 1/2 sum_k (tau_k / lam_k)^2),   tau = x - x',
    the model of a periodicity whose shape drifts.  The factors live in `self.kernels` (gpytorch's layout), so state dicts line up:
    kernels.<i>.raw_lengthscale, kernels.<i>.raw_period_length.  Both factors are bare (no ScaleKernel inside; wrap the product) and
    agree in active_dims, ard_num_dims and batch_shape; anything else raises NotImplementedError.  No lengthscale of its own.  On the
    HIP path it is kernel kind "locally_periodic" of the batched exact engine (include/plmc.h, "Locally periodic kernel"); the additive
    kernel, SGPR, the dense LMC / ICM and the variational models refuse it."""
    has_lengthscale = False
    kind = "locally_periodic"
    is_stationary = True

    def __init__(self, *kernels):
        given = "ProductKernel(%s)" % ", ".join(type(k).__name__ for k in kernels)
        per = [k for k in kernels if type(k) is PeriodicKernel]
        rbf = [k for k in kernels if type(k) is RBFKernel]
        if len(kernels) != 2 or len(per) != 1 or len(rbf) != 1:
            raise NotImplementedError("ProductKernel serves the product of one PeriodicKernel and one RBFKernel only, got %s" % given)
        for name in ("active_dims", "ard_num_dims", "batch_shape"):
            if getattr(per[0], name) != getattr(rbf[0], name):
                raise NotImplementedError("ProductKernel needs factors with equal %s, got %s with %r and %r"
                                          % (name, given, getattr(kernels[0], name), getattr(kernels[1], name)))
        super().__init__(ard_num_dims=per[0].ard_num_dims, batch_shape=per[0].batch_shape, active_dims=per[0].active_dims)
        self.kernels = torch.nn.ModuleList(kernels)
        self._per, self._rbf = (0, 1) if kernels[0] is per[0] else (1, 0)

    def _pieces(self, d, like=None):
        """The table (q, 3, d) = [periodic lengthscale | period | RBF lengthscale] and no output scale."""
        _, table, _ = self.kernels[self._per]._pieces(d, like)
        return self.kind, torch.cat([table, self.kernels[self._rbf]._ell(d, like).unsqueeze(1)], 1), None


def _refuse(cls, name, kernel, model):
    k = kernel
    while k is not None and not isinstance(k, cls):
        k = getattr(k, "base_kernel", None)
    if k is not None or (isinstance(kernel, type) and issubclass(kernel, cls)):
        raise NotImplementedError("%s does not take a %s: it is served by the batched exact engine only "
                                  "(ExactGPModel without inducing points, ProjectedGPModel)" % (model, name))


def refuse_periodic(kernel, model):
    """The periodic kernel runs on the batched exact engine only: name the model that cannot take it."""
    _refuse(PeriodicKernel, "PeriodicKernel", kernel, model)


def refuse_product(kernel, model):
    """The locally periodic kernel (ProductKernel) runs on the batched exact engine only: name the model that cannot take it.  `kernel`
    is an instance, bare or inside a ScaleKernel: `kernel_type` may be a factory function, which only shows its product once called."""
    _refuse(ProductKernel, "ProductKernel (PeriodicKernel * RBFKernel)", kernel, model)


def refuse_rq(kernel, model):
    """The rational-quadratic kernel runs on the batched exact engine only: name the model that cannot take it."""
    _refuse(RQKernel, "RQKernel", kernel, model)


def refuse_dot(kernel, model):
    """The dot-product kernels run on the batched exact engine only: name the model that cannot take them, and the class."""
    _refuse(LinearKernel, "LinearKernel", kernel, model)
    _refuse(PolynomialKernel, "PolynomialKernel", kernel, model)


def refuse_sum(kernel, model):
    """A sum of different kernel families (additive.AdditiveKernel with mixed members, kind "sum(...)") runs on the batched exact engine
    only: name the model that cannot take it, and the members.  A sum of one stationary kind goes wherever it went.  `kernel` is an
    instance, bare or inside a ScaleKernel: `kernel_type` may be a factory function, which only shows its sum once called."""
    from .additive import AdditiveKernel
    k = kernel
    while k is not None and not isinstance(k, AdditiveKernel):
        k = getattr(k, "base_kernel", None)
    if k is not None and k.is_heterogeneous():
        raise NotImplementedError("%s does not take the sum %s: a sum of different kernel families is served by the batched exact engine "
                                  "only (ExactGPModel without inducing points, ProjectedGPModel)" % (model, k.describe()))


def refuse_sm(kernel, model):
    """The spectral-mixture kernel runs on the batched exact engine only: name the model that cannot take it."""
    _refuse(SpectralMixtureKernel, "SpectralMixtureKernel", kernel, model)


def prior_diagonal(kind, x, oscale, q, table=None):
    """k(x, x) per latent, (q, n): 1 for the stationary kinds, prod_k (1 + x_k^2 + x_k^3 / 3) for the spline kernel,
    (c + sum_k v_k x_k^2)^P for a dot-product kind, which needs its `table` (q, d + 1) = [v | c]; no other kind looks at it."""
    if kind == "sm" and oscale is None:                        # unit weights: k(x, x) = M needs the table, not known here
        raise ValueError("prior_diagonal: a spectral mixture needs its weights")
    P = dot_power(kind)
    if P is not None:
        if table is None:
            raise ValueError("prior_diagonal: a dot-product kernel needs its table")
        table = table.to(x.dtype)
        dg = (table[:, -1:] + table[:, :-1] @ (x * x).transpose(-1, -2)) ** P
    elif kind == "spline":
        dg = (1 + x ** 2 + x ** 3 / 3).prod(dim=-1).reshape(1, -1).expand(q, -1)
    else:
        dg = torch.ones(q, x.shape[-2], dtype=x.dtype, device=x.device)
    if oscale is not None and oscale.dim() == 2:              # additive kernel: k(x, x) = sum_g os_g
        oscale = oscale.sum(-1)
    return dg if oscale is None else dg * oscale.reshape(-1, 1)


class ScaleKernel(Kernel):
    def __init__(self, base_kernel, outputscale_prior=None, outputscale_constraint=None, batch_shape=torch.Size(),
                 **kwargs):
        super().__init__(batch_shape=batch_shape, active_dims=base_kernel.active_dims)
        self.base_kernel = base_kernel
        self.register_parameter("raw_outputscale", torch.nn.Parameter(torch.zeros(self.batch_shape)))
        self.raw_outputscale_constraint = outputscale_constraint or Positive()

    @property
    def outputscale(self):
        return self.raw_outputscale_constraint.transform(self.raw_outputscale)

    @outputscale.setter
    def outputscale(self, value):
        value = torch.as_tensor(value, dtype=self.raw_outputscale.dtype, device=self.raw_outputscale.device)
        with torch.no_grad():
            self.raw_outputscale.copy_(self.raw_outputscale_constraint.inverse_transform(value).expand_as(self.raw_outputscale))

    def _pieces(self, d, like=None):
        kind, ell, inner = self.base_kernel._pieces(d, like if like is not None else self.raw_outputscale)
        if kind == "sm":                                       # the output scale folds into the mixture weights (q, M)
            return kind, ell, self.outputscale.reshape(-1, 1) * inner
        if kind.startswith("sum("):                            # ... and into the component output scales (q, G) of a heterogeneous sum
            return kind, ell, self.outputscale.reshape(-1, 1) * inner
        return kind, ell, self.outputscale.reshape(-1)


class LazyKernel:
    """Un-evaluated batched covariance os * k(x1, x2; ell) (+ noise * I once a likelihood was
    applied).  The hot path never materialises it.
    ell (q, d), oscale (q) | None: one ARD kernel per latent.  ell (q, G, d), oscale (q, G): the component table of an additive
    kernel sum_g os_g k(x1, x2; ell_g) (additive.py), +inf on the dimensions a component ignores -- `inv_ell` is 0 there.
    kind "sm": ell (q, 2, M, d) holds the scales and the means of a spectral mixture, oscale (q, M) its weights (`scales`, `means`,
    `weights`).  kind "periodic": ell (q, 2, d) holds the lengthscales and the periods, oscale (q) | None.  kind "rq": ell (q, d + 1) holds
    the lengthscales and, in its last column, alpha; oscale (q) | None.  kind "locally_periodic": ell (q, 3, d) holds the periodic
    lengthscales, the periods and the RBF lengthscales, oscale (q) | None.  kind "sum(<member>,...)": a sum of different families
    (additive.py); the member kinds travel in the kind string (so through add_noise and into the prediction cache's key), ell
    (q, G, 3 d + 1) holds one record [lengthscales | periods | RBF lengthscales | alpha] per member, oscale (q, G).  kind "linear" /
    "poly<P>": ell (q, d + 1) holds the variances and, in its last column, the offset of a dot-product kernel; oscale (q) | None.
    pnoise (n) | (q, n) | None: per-point noise on the diagonal beside `noise` (FixedNoiseGaussianLikelihood): + diag(pnoise)."""

    def __init__(self, kind, x1, x2, ell, oscale, batch_shape, noise=None, pnoise=None):
        self.kind, self.x1, self.x2, self.ell, self.oscale, self.noise, self.pnoise = kind, x1, x2, ell, oscale, noise, pnoise
        self.batch_shape = torch.Size(batch_shape)
        self.is_square = x1 is x2

    @property
    def shape(self):
        return torch.Size([*self.batch_shape, self.x1.shape[-2], self.x2.shape[-2]])

    def size(self, dim=None):
        return self.shape if dim is None else self.shape[dim]

    @property
    def dtype(self):
        return self.x1.dtype

    @property
    def device(self):
        return self.x1.device

    scales = property(lambda self: self.ell[:, 0] if self.kind == "sm" else None)
    means = property(lambda self: self.ell[:, 1] if self.kind == "sm" else None)
    weights = property(lambda self: self.oscale if self.kind == "sm" else None)

    @property
    def inv_ell(self):
        """1 / ell: exactly 0 on the slots of an additive component's table that are outside its group of dimensions."""
        return 1.0 / self.ell

    def add_noise(self, noise):
        return LazyKernel(self.kind, self.x1, self.x2, self.ell, self.oscale, self.batch_shape,
                          noise if self.noise is None else self.noise + noise, self.pnoise)

    def add_point_noise(self, pnoise):
        """+ diag(pnoise), pnoise (n) or (q, n); the scalar noise stays what it is."""
        n, q = self.x1.shape[-2], self.ell.shape[0]
        if not self.is_square or pnoise.dim() not in (1, 2) or pnoise.shape[-1] != n or (pnoise.dim() == 2 and pnoise.shape[0] != q):
            raise ValueError("per-point noise is (n) = (%d) or (q, n) = (%d, %d) on a square kernel matrix, got %s" % (n, q, n, tuple(pnoise.shape)))
        return LazyKernel(self.kind, self.x1, self.x2, self.ell, self.oscale, self.batch_shape, self.noise,
                          pnoise if self.pnoise is None else self.pnoise + pnoise)

    def diagonal(self, *args, **kwargs):
        q = self.ell.shape[0]
        dg = prior_diagonal(self.kind, self.x1.to(self.ell.dtype), self.oscale, q, self.ell)
        if self.noise is not None:
            dg = dg + self.noise.reshape(-1, 1)
        if self.pnoise is not None:
            dg = dg + self.pnoise.to(dg.dtype)
        return dg.reshape(*self.batch_shape, -1)

    def evaluate(self):
        from . import _engine
        K = _engine.dense_cross(self.kind, self.x1.to(self.ell.dtype), self.x2.to(self.ell.dtype), self.ell.detach(),
                                None if self.oscale is None else self.oscale.detach())
        if self.noise is not None and self.is_square:
            K = K + self.noise.detach().reshape(-1, 1, 1) * torch.eye(K.shape[-1], dtype=K.dtype, device=K.device)
        if self.pnoise is not None and self.is_square:
            K = K + torch.diag_embed(self.pnoise.detach().to(K.dtype).expand(K.shape[0], -1))
        return K.reshape(*self.batch_shape, *K.shape[-2:])

    to_dense = evaluate
    evaluate_kernel = lambda self: self  # noqa: E731  (gpytorch idiom used at projected_lmc.py:368)


# ------------------------------------------------------------------------------------------------
# Multitask (Kronecker) kernels of the exact LMC / ICM models (projected_lmc.py:462-466).
class IndexKernel(torch.nn.Module):
    """Task covariance B = F F^T + diag(softplus(raw_var)) [gpytorch-knowledge: IndexKernel;
    covar_factor (p x rank) and raw_var (p) are randn-initialised]."""

    def __init__(self, num_tasks, rank=1, **kwargs):
        super().__init__()
        self.num_tasks, self.rank = num_tasks, rank
        self.register_parameter("covar_factor", torch.nn.Parameter(torch.randn(num_tasks, rank)))
        self.register_parameter("raw_var", torch.nn.Parameter(torch.randn(num_tasks)))
        self.raw_var_constraint = Positive()

    @property
    def var(self):
        return self.raw_var_constraint.transform(self.raw_var)

    @property
    def covar_matrix(self):
        F = self.covar_factor
        return F @ F.transpose(-1, -2) + torch.diag_embed(self.var.to(F.dtype))


class MultitaskKernel(Kernel):
    """K_data(x,x') (x) B (data-major interleaving) [gpytorch-knowledge: MultitaskKernel]."""

    def __init__(self, data_covar_module, num_tasks, rank=1, **kwargs):
        super().__init__()
        self.data_covar_module = data_covar_module
        self.task_covar_module = IndexKernel(num_tasks=num_tasks, rank=rank)
        self.num_tasks = num_tasks

    def _lmc_pieces(self, d):
        kind, ell, osc = self.data_covar_module._pieces(d)
        return kind, ell[:1], None if osc is None else osc[:1], self.task_covar_module.covar_matrix.unsqueeze(0)

    def forward(self, x1, x2=None, **params):
        x1 = self.data_covar_module.select(x1)
        kind, ell, osc, B = self._lmc_pieces(x1.shape[-1])
        return LazyLmcKernel(kind, x1, ell, osc, B)


class LCMKernel(Kernel):
    """sum_i K_i (x) B_i, one MultitaskKernel per latent [gpytorch-knowledge: LCMKernel]."""

    def __init__(self, base_kernels, num_tasks, rank=1, **kwargs):
        super().__init__()
        self.covar_module_list = torch.nn.ModuleList(
            [MultitaskKernel(b, num_tasks=num_tasks, rank=rank) for b in base_kernels])
        self.num_tasks = num_tasks

    def forward(self, x1, x2=None, **params):
        x1 = self.covar_module_list[0].data_covar_module.select(x1)
        pieces = [m._lmc_pieces(x1.shape[-1]) for m in self.covar_module_list]
        kind = pieces[0][0]
        ell = torch.cat([p_[1] for p_ in pieces], 0)
        osc = None if pieces[0][2] is None else torch.cat([p_[2] for p_ in pieces], 0)
        B = torch.cat([p_[3] for p_ in pieces], 0)
        return LazyLmcKernel(kind, x1, ell, osc, B)


class LazyLmcKernel:
    """Un-evaluated sum_i os_i k(X,X; ell_i) (x) B_i (+ I (x) Sigma once a multitask likelihood was
    applied); consumed by the HIP LMC engine."""

    def __init__(self, kind, x, ell, oscale, B, task_noise=None):
        self.kind, self.x, self.ell, self.oscale, self.B, self.task_noise = kind, x, ell, oscale, B, task_noise

    @property
    def shape(self):
        N = self.x.shape[-2] * self.B.shape[-1]
        return torch.Size([N, N])

    def add_task_noise(self, Sigma):
        tn = Sigma if self.task_noise is None else self.task_noise + Sigma
        return LazyLmcKernel(self.kind, self.x, self.ell, self.oscale, self.B, tn)

    def diagonal(self, *a, **k):
        q = self.ell.shape[0]
        os_ = torch.ones(q, dtype=self.B.dtype, device=self.B.device) if self.oscale is None else self.oscale
        dg = (os_[:, None] * torch.diagonal(self.B, dim1=-2, dim2=-1)).sum(0)
        if self.task_noise is not None:
            dg = dg + torch.diagonal(self.task_noise)
        return dg.repeat(self.x.shape[-2])

    def log_prob_flat(self, diff):
        from . import _lmc_engine
        if self.task_noise is None:
            raise RuntimeError("log_prob of a noise-free LMC prior: apply the multitask likelihood first")
        return _lmc_engine.lmc_exact_log_prob(self.kind, self.x, self.ell, self.oscale, self.B, self.task_noise,
                                              diff.reshape(-1))

    def evaluate(self):
        """Dense (np x np) matrix via the HIP cross kernel (small cases / inspection only)."""
        from . import _hip
        L = _hip.lib()
        x = self.x.contiguous()
        n, d = x.shape
        q, p = self.B.shape[0], self.B.shape[-1]
        dt, dev = self.B.dtype, self.B.device
        out = torch.empty(n * p, n * p, dtype=dt, device=dev)
        L.call("plmc_lmc_cross", dt, _hip.KIND[self.kind], _hip.ptr(x.to(dt)), n, _hip.ptr(x.to(dt)), n, d, p, q,
               _hip.ptr(self.ell.detach().to(dt).contiguous()),
               _hip.ptr(None if self.oscale is None else self.oscale.detach().to(dt).contiguous()),
               _hip.ptr(self.B.detach().contiguous()), _hip.ptr(out), n * p, 0, n * p, _hip.stream_ptr(dev))
        if self.task_noise is not None:
            out = out + torch.kron(torch.eye(n, dtype=dt, device=dev), self.task_noise.detach())
        return out

    to_dense = evaluate
