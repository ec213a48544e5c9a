"""Minimal Gaussian distribution types with the attribute surface the reference's drivers and
model code touch: `.mean`, `.variance`, `.stddev`, `.confidence_region()`,
`.lazy_covariance_matrix`, `.covariance_matrix`, `.event_shape`, `.batch_shape`, `.log_prob`,
and the draws `.get_base_samples`, `.rsample`, `.sample` [gpytorch-knowledge, unverified offline: names, argument order and
shapes of gpytorch.distributions.MultivariateNormal] -- the reference's synthetic study begins with
`MultivariateNormal(zeros, kernel(X)).sample()` (experiments.py:150-151).

`covar` may be a dense tensor, a kernels.LazyKernel (prior of a batch of GPs: log_prob goes to
the HIP engine) or one of the structured covariances below (never materialised unless asked).
"""
import math

import torch

from .kernels import LazyKernel


class KroneckerSumCovariance:
    """sum_i C_i (x) h_i h_i^T + eps I, data-major interleaved ((n p) x (n p)) -- the task-space
    covariance ProjectedGPModel.__call__ builds at projected_lmc.py:1149-1153.  Only its diagonal is
    needed by the drivers (experiments.py:329); `evaluate()` materialises for small cases.
    C_i given either as full (q,n,n) `cov` or as diagonal (q,n) `var`."""

    def __init__(self, Ht, cov=None, var=None, eps=0.0, task_noise=None, diag=None):
        self.Ht, self.cov, self.var, self.eps, self.task_noise = Ht, cov, var, eps, task_noise
        self.diag = diag                                    # (n, p) diagonal incl. eps, if already mixed (plmc_mix_posterior)
        self.n = (cov if cov is not None else var).shape[-1]
        self.p = Ht.shape[-1]

    @property
    def shape(self):
        return torch.Size([self.n * self.p, self.n * self.p])

    def add_task_noise(self, Sigma):
        tn = Sigma if self.task_noise is None else self.task_noise + Sigma
        return KroneckerSumCovariance(self.Ht, self.cov, self.var, self.eps, tn, self.diag)

    def diagonal(self, *a, **k):
        if self.diag is not None:
            dg = self.diag
        else:
            v = self.var if self.var is not None else torch.diagonal(self.cov, dim1=-2, dim2=-1)   # (q,n)
            dg = v.T @ (self.Ht * self.Ht) + self.eps                                              # (n,p)
        if self.task_noise is not None:
            dg = dg + torch.diagonal(self.task_noise)[None, :]
        return dg.reshape(-1)

    def log_prob_flat(self, diff):
        """log N(diff; 0, this covariance), diff (n, p), for latent VARIANCES (full_cov=False): the points are independent and each has
        the p x p covariance sum_i var_i(s) h_i h_i^T + eps I (+ task noise) -- n small Cholesky factors, plain torch, differentiable in
        the variances, the mixing matrix and the task noise.  Full latent covariances are not served."""
        if self.cov is not None:
            raise NotImplementedError("log_prob of the task-space posterior is implemented for latent variances (full_cov=False) only")
        Ht = self.Ht.to(diff.dtype)
        C = torch.einsum("qs,qa,qb->sab", self.var, Ht, Ht) + self.eps * torch.eye(self.p, dtype=diff.dtype, device=diff.device)
        if self.task_noise is not None:
            C = C + self.task_noise
        Lc = torch.linalg.cholesky(C)
        z = torch.linalg.solve_triangular(Lc, diff.unsqueeze(-1), upper=False).squeeze(-1)
        return -0.5 * (z * z).sum() - torch.diagonal(Lc, dim1=-2, dim2=-1).log().sum() - 0.5 * diff.numel() * math.log(2.0 * math.pi)

    def evaluate(self):
        if self.cov is None:
            raise RuntimeError("full task covariance requested but only latent variances were computed; "
                               "call the model with full_cov=True")
        q, n, p = self.Ht.shape[0], self.n, self.p
        B = self.Ht[:, :, None] * self.Ht[:, None, :]                                           # (q,p,p)
        C = torch.einsum("qab,qst->asbt", self.cov, B).reshape(n * p, n * p)
        C = C + self.eps * torch.eye(n * p, dtype=C.dtype, device=C.device)
        if self.task_noise is not None:
            C = C + torch.kron(torch.eye(n, dtype=C.dtype, device=C.device), self.task_noise)
        return C

    to_dense = evaluate


class ZeroCovariance:
    """The covariance of a mean-only prediction (settings.skip_posterior_variances): exactly zero, never materialised unless asked.
    `like`: a tensor with the batch shape and the event size of the distribution, (..., n)."""

    def __init__(self, like):
        self.like = like

    @property
    def shape(self):
        return torch.Size([*self.like.shape, self.like.shape[-1]])

    def __getitem__(self, idx):
        return ZeroCovariance(self.like[idx])

    def diagonal(self, *a, **k):
        return torch.zeros_like(self.like)

    def evaluate(self):
        return torch.zeros(self.shape, dtype=self.like.dtype, device=self.like.device)

    to_dense = evaluate


class MultivariateNormal:
    def __init__(self, mean, covariance_matrix, validate_args=False):
        self.loc = mean
        self._covar = covariance_matrix

    # -- shapes
    @property
    def event_shape(self):
        return self.loc.shape[-1:]

    @property
    def batch_shape(self):
        return self.loc.shape[:-1]

    @property
    def mean(self):
        return self.loc

    @property
    def lazy_covariance_matrix(self):
        return self._covar

    @property
    def covariance_matrix(self):
        c = self._covar
        return c if torch.is_tensor(c) else c.evaluate()

    @property
    def variance(self):
        c = self._covar
        if torch.is_tensor(c):
            return torch.diagonal(c, dim1=-2, dim2=-1)
        return c.diagonal().reshape(self.loc.shape)

    @property
    def stddev(self):
        return self.variance.sqrt()

    def confidence_region(self):
        s2 = self.stddev * 2.0
        return self.mean - s2, self.mean + s2

    # -- draws
    sample_jitter = 0.0        # what the last rsample / sample added to the diagonal to factorise the covariance (the largest over its factorisations)

    def _base_sample_event(self):
        return self.loc.shape

    def get_base_samples(self, sample_shape=torch.Size(), generator=None):
        """Standard-normal base samples of shape sample_shape + loc.shape (see MultitaskMultivariateNormal for the one exception), on
        loc's device and dtype.  Obeys torch.manual_seed; `generator` goes to torch.randn."""
        return torch.randn(*sample_shape, *self._base_sample_event(), dtype=self.loc.dtype, device=self.loc.device, generator=generator)

    def _not_served(self, c):
        raise NotImplementedError("draws from a %s covariance are not implemented (served: kernel priors -- LazyKernel, with or without "
                                  "noise -- and dense covariance tensors)" % type(c).__name__)

    def _draw(self, Z):
        """Z (S, *loc.shape) base samples -> draws loc.detach() + U^T z of the same shape, U^T U = covariance per batch
        member, on the engine: the factor is the sweep's, the product plmc_trmm_ut."""
        c = self._covar
        S, n = Z.shape[0], self.loc.shape[-1]
        loc = self.loc.detach()
        if isinstance(c, LazyKernel):
            from . import _engine
            if not c.is_square:
                raise NotImplementedError("draws need a square kernel matrix k(X, X)")
            if getattr(c, "pnoise", None) is not None:
                _engine.refuse_point_noise("rsample / sample of a kernel prior")
            q = c.ell.shape[0]
            Zk = Z.reshape(S, q, n).permute(1, 2, 0)                   # K-major (q, n, S)
            Y, jit = _engine.sample_lazy(c.kind, c.x1, c.ell, c.oscale, None if c.noise is None else c.noise.reshape(-1), Zk,
                                         loc.reshape(q, n))
        elif torch.is_tensor(c):
            from . import _dense
            batch = self.loc.shape[:-1]
            q = 1
            for b in batch:
                q *= b
            M = c.detach().to(loc.dtype).expand(*batch, n, n).reshape(q, n, n)
            Zk = Z.reshape(S, q, n).permute(1, 2, 0)
            Y, jit = _dense.spd_sample(M, Zk, loc.reshape(q, n))
        else:
            self._not_served(c)
        self.sample_jitter = float(jit)
        return Y.permute(2, 0, 1).reshape(Z.shape)

    def rsample(self, sample_shape=torch.Size(), base_samples=None):
        """Draws of shape sample_shape + loc.shape: loc + U^T z per batch member with U^T U = covariance (gpytorch's `L z`) and z =
        `base_samples` (sample_shape + loc.shape; drawn with get_base_samples if None).  The covariance is factorised on the engine
        (with the package's jitter ladder; a noise-free kernel prior gets settings.cholesky_jitter from the first attempt) and what
        was added is left in `sample_jitter`.
        Differentiable through `loc` ONLY: the covariance part is detached -- the Cholesky adjoint for draws is out of scope, so
        kernel hyper-parameters receive no gradient from a draw."""
        sample_shape = torch.Size(sample_shape)
        event = self._base_sample_event()
        if base_samples is None:
            base_samples = self.get_base_samples(sample_shape)
        else:
            if tuple(base_samples.shape[base_samples.dim() - len(event):]) != tuple(event):
                raise ValueError("base_samples must end in %s, got %s" % (tuple(event), tuple(base_samples.shape)))
            sample_shape = base_samples.shape[:base_samples.dim() - len(event)]
        Z = base_samples.detach().to(self.loc.dtype).reshape(-1, *event)
        out = self._draw(Z).reshape(*sample_shape, *self.loc.shape)
        if self.loc.requires_grad and torch.is_grad_enabled():
            out = out + (self.loc - self.loc.detach())             # value unchanged (adds exact zeros), d out / d loc = 1
        return out

    def sample(self, sample_shape=torch.Size(), base_samples=None):
        """rsample under no_grad."""
        with torch.no_grad():
            return self.rsample(sample_shape, base_samples)

    def log_prob(self, value):
        """-1/2 (quad + logdet + n log 2pi).  Lazy kernel covariances run on the HIP engine
        (the call the reference makes at projected_lmc.py:1201)."""
        c = self._covar
        diff = value - self.loc
        if hasattr(c, "log_prob_batch"):                       # SGPR / Nystrom prior (sgpr.py)
            return c.log_prob_batch(diff.reshape(-1, diff.shape[-1])).reshape(self.batch_shape)
        if isinstance(c, LazyKernel):
            from . import _engine
            if c.noise is None:
                raise RuntimeError("log_prob of a noise-free kernel prior: apply the likelihood first")
            q = c.ell.shape[0]
            y = diff.reshape(q, -1)
            lp = _engine.exact_latent_log_prob(c.kind, c.x1, c.ell, c.oscale, c.noise.reshape(-1), y, pnoise=c.pnoise)
            return lp.reshape(self.batch_shape)
        if torch.is_tensor(c):          # a dense predictive covariance (n* x n*, usually diagonal): plain torch, differentiable
            Lc = torch.linalg.cholesky(c)
            z = torch.linalg.solve_triangular(Lc, diff.unsqueeze(-1), upper=False).squeeze(-1)
            return (-0.5 * (z * z).sum(-1) - torch.diagonal(Lc, dim1=-2, dim2=-1).log().sum(-1)
                    - 0.5 * diff.shape[-1] * math.log(2.0 * math.pi))
        raise NotImplementedError("log_prob is implemented for kernel priors (HIP engine) and dense predictive covariances only")


class MultitaskMultivariateNormal(MultivariateNormal):
    """mean (n, p); covariance over the data-major interleaved vector (flat = i_point * p + i_task)
    [gpytorch-knowledge: MultitaskMultivariateNormal, interleaved=True]."""

    def __init__(self, mean, covariance_matrix, validate_args=False, interleaved=True, independent=None):
        super().__init__(mean, covariance_matrix)
        self._independent = independent      # batch MVN it was built from (from_batch_mvn)

    @classmethod
    def from_batch_mvn(cls, batch_mvn, task_dim=-1):
        """Independent tasks from a batch of q MVNs (projected_lmc.py:318-319): mean (q,n)->(n,q)."""
        return cls(batch_mvn.mean.transpose(-1, -2), batch_mvn.lazy_covariance_matrix, independent=batch_mvn)

    @property
    def event_shape(self):
        return self.loc.shape[-2:]

    @property
    def batch_shape(self):
        return self.loc.shape[:-2]

    @property
    def num_tasks(self):
        return self.loc.shape[-1]

    @property
    def variance(self):
        c = self._covar
        if self._independent is not None:
            return self._independent.variance.transpose(-1, -2)
        if torch.is_tensor(c):
            return torch.diagonal(c, dim1=-2, dim2=-1).reshape(self.loc.shape)
        return c.diagonal().reshape(self.loc.shape)

    # -- draws.  Base samples have the shape of the mean, sample_shape + (n, p), except under a KroneckerSumCovariance (the projected
    # model's posterior): sample_shape + (n, q + p) -- the first q columns drive the q latent processes, the last p the eps / task-noise
    # term:   draw = mean + sum_i f_i (x) h_i + sqrt(eps) e  (with task noise: + U_t^T e, U_t^T U_t = eps I + Sigma, one p-vector per point).
    # f_i comes from the latent covariance (_dense.spd_sample) or, when only variances were formed (full_cov=False), from
    # sqrt(var_i) z: the points are then drawn independently -- that is what full_cov=False computes.
    def _base_sample_event(self):
        c = self._covar
        if isinstance(c, KroneckerSumCovariance):
            return torch.Size([c.n, c.Ht.shape[0] + c.p])
        return self.loc.shape

    def _draw(self, Z):
        c = self._covar
        loc = self.loc.detach()
        S = Z.shape[0]
        if self._independent is not None:
            bm = self._independent
            out = MultivariateNormal._draw(bm, Z.transpose(-1, -2)).transpose(-1, -2)      # (its mean is this one transposed)
            self.sample_jitter = bm.sample_jitter
            return out
        if isinstance(c, KroneckerSumCovariance):
            from . import _dense
            Ht = c.Ht.detach().to(loc.dtype)
            q, n, p = Ht.shape[0], c.n, c.p
            Zl, Ze = Z[..., :q], Z[..., q:]                                   # (S, n, q), (S, n, p)
            jit = 0.0
            if c.cov is not None:
                F, jit = _dense.spd_sample(c.cov.detach().to(loc.dtype), Zl.permute(2, 1, 0))       # (q, n, S)
            else:
                F = c.var.detach().to(loc.dtype).clamp_min(0).sqrt()[:, :, None] * Zl.permute(2, 1, 0)
            out = loc + torch.einsum("qns,qp->snp", F, Ht)
            if c.task_noise is not None:
                T = c.task_noise.detach().to(loc.dtype) + c.eps * torch.eye(p, dtype=loc.dtype, device=loc.device)
                E, jt = _dense.spd_sample(T[None], Ze.reshape(1, S * n, p).transpose(-1, -2))         # (1, p, S n)
                out = out + E[0].transpose(0, 1).reshape(S, n, p)
                jit = max(jit, jt)
            else:
                out = out + (float(c.eps) ** 0.5) * Ze
            self.sample_jitter = float(jit)
            return out
        from .projected import _DiagonalTaskCovariance
        if isinstance(c, _DiagonalTaskCovariance):                            # marginal variances only: independent marginals
            self.sample_jitter = 0.0
            return loc + c.diagonal().detach().reshape(loc.shape).clamp_min(0).sqrt() * Z
        if torch.is_tensor(c):
            flat = MultivariateNormal(loc.reshape(*self.batch_shape, -1), c)
            out = flat._draw(Z.reshape(S, *flat.loc.shape)).reshape(Z.shape)
            self.sample_jitter = flat.sample_jitter
            return out
        self._not_served(c)

    def log_prob(self, value):
        if self._independent is not None:
            return self._independent.log_prob(value.transpose(-1, -2)).sum(-1)
        c = self._covar
        if hasattr(c, "log_prob_flat"):
            return c.log_prob_flat((value - self.loc))
        flat = MultivariateNormal(self.loc.reshape(*self.batch_shape, -1), c)
        return flat.log_prob(value.reshape(*self.batch_shape, -1))
