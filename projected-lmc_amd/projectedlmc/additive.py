"""Additive sub-kernel decompositions, `decomp=[[0,1],[1,2]]` -> k(x) = s1 k1(x0,x1) + s2 k2(x1,x2)
(reference: handle_covar_, projected_lmc.py:131-167).

HIP path: the sum of G scaled ARD kernels on subsets of the input dimensions is a kernel kind of the batched exact engine
like any other.  Calling the module returns an ordinary `LazyKernel` whose hyper-parameters are a COMPONENT TABLE -- lengthscales
(q, G, d) with an infinite lengthscale (1 / ell = 0 exactly, `LazyKernel.inv_ell`) on the dimensions a component ignores, output
scales (q, G) -- for batch_shape [1] and [n_funcs] alike (the reference builds the decomposition with batch_shape=[n_funcs],
projected_lmc.py:151-167: batched exact GPs, the latent processes of the projected model).  The assembly, cross-assembly and
gradient kernels evaluate the G components per element (include/plmc.h, "Additive kernels"); the sweep, the pivot checks, the
prediction cache, `full_cov` and latent sharding do not look at the kernel and serve it unchanged.  A sub-kernel owns len(group)
lengthscales: autograd gathers the active slots of the table's gradient back into them (index_copy below).

Sums of DIFFERENT families -- what `k1 + k2` builds, e.g. RBFKernel() + PeriodicKernel() * RBFKernel() + RQKernel() -- are kernel kind
"sum(<member>,...)" of the same engine (include/plmc.h, "Sums of kernel families"): members are the stationary ARD kernels, PeriodicKernel,
RQKernel and the locally periodic ProductKernel, each bare or one ScaleKernel deep.  The table is (q, G, 3 d + 1), one record
[lengthscales | periods | RBF lengthscales: d each | alpha] per member; a member reads only its own slots, the others hold a constant.
Sums whose members are all of one stationary kind keep the component table above, unchanged."""
import torch

from .kernels import Kernel, ScaleKernel, LazyKernel, RBFKernel, MaternKernel, PeriodicKernel, RQKernel, ProductKernel

_SUM_MEMBER_TYPES = (RBFKernel, MaternKernel, PeriodicKernel, RQKernel, ProductKernel)
_OWN_TABLE = ("periodic", "rq", "locally_periodic")        # member kinds that no same-kind component table serves


class AdditiveKernel(Kernel):
    def __init__(self, *kernels):
        super().__init__()
        self.kernels = torch.nn.ModuleList(kernels)

    def __add__(self, other):
        return AdditiveKernel(*self.kernels, *(other.kernels if isinstance(other, AdditiveKernel) else [other]))

    def select(self, x):
        return x

    @staticmethod
    def _base(k):
        return k.base_kernel if isinstance(k, ScaleKernel) else k

    def describe(self):
        return "AdditiveKernel(%s)" % ", ".join(
            ("ScaleKernel(%s)" % type(k.base_kernel).__name__) if isinstance(k, ScaleKernel) else type(k).__name__ for k in self.kernels)

    def is_heterogeneous(self):
        """Whether this is a sum of different families (kind "sum(...)") rather than the component table of one stationary kind."""
        kinds = [getattr(self._base(k), "kind", None) for k in self.kernels]
        return len(set(kinds)) != 1 or kinds[0] in _OWN_TABLE or kinds[0] is None

    def sum_table(self, d):
        """(kind "sum(...)", table (batch, G, 3 d + 1), oscale (batch, G)) of a sum of different families.  An owned lengthscale slot
        outside the member's active_dims holds +inf (1 / ell = 0: that dimension adds exactly 0 to the member's exponent or distance and has
        exactly-0 gradients); slots a member does not own hold 1 and are never read.  Autograd gathers the table's gradient back into the
        members' parameters: index_copy for the active dimensions, a sum over them for a parameter without ARD."""
        from ._engine import sum_kind
        bases = [self._base(k) for k in self.kernels]
        bad = [b for b in bases if type(b) not in _SUM_MEMBER_TYPES]
        if bad:
            raise NotImplementedError("a sum of kernels takes RBFKernel, MaternKernel, PeriodicKernel, RQKernel and PeriodicKernel * RBFKernel "
                                      "members, each bare or inside one ScaleKernel; got %s" % self.describe())
        shapes = {tuple(b.batch_shape) for b in bases}
        if len(shapes) != 1:
            raise NotImplementedError("the members of a sum of kernels must agree in batch_shape; got %s with %s"
                                      % (self.describe(), ", ".join(str(tuple(b.batch_shape)) for b in bases)))
        nb = max(1, int(bases[0].batch_shape.numel()))
        recs, oss, kinds = [], [], []
        for k, b in zip(self.kernels, bases):
            dims = list(b.active_dims) if b.active_dims is not None else list(range(d))
            per = b.kernels[b._per] if isinstance(b, ProductKernel) else (b if isinstance(b, PeriodicKernel) else None)
            lsk = per if isinstance(b, ProductKernel) else b
            like = lsk.raw_lengthscale
            idx = torch.tensor(dims, device=like.device)

            def slot(value, fill):
                v = value.reshape(-1, value.shape[-1])
                v = v.expand(v.shape[0], len(dims)) if v.shape[-1] != len(dims) else v
                full = torch.full((v.shape[0], d), fill, dtype=like.dtype, device=like.device)
                return full.index_copy(1, idx, v).expand(nb, d)

            one = torch.ones(nb, d, dtype=like.dtype, device=like.device)
            ell = slot(lsk.lengthscale, float("inf"))
            period = slot(per.period_length, 1.0) if per is not None else one
            rbf = slot(b.kernels[b._rbf].lengthscale, float("inf")) if isinstance(b, ProductKernel) else one
            alpha = b.alpha.reshape(-1, 1).expand(nb, 1) if isinstance(b, RQKernel) else one[:, :1]
            recs.append(torch.cat([ell, period, rbf, alpha], 1))
            oss.append(k.outputscale.reshape(-1).expand(nb) if isinstance(k, ScaleKernel) else one[:, 0])
            kinds.append(b.kind)
        return sum_kind(kinds), torch.stack(recs, 1), torch.stack(oss, 1)

    def table(self, d):
        """(kind, ell (batch, G, d), oscale (batch, G)) from the sub-kernels' parameters; needs no device.  A sum of different
        families: sum_table."""
        if self.is_heterogeneous():
            return self.sum_table(d)
        kinds, ells, oss = [], [], []
        nb = max(int((k.base_kernel if isinstance(k, ScaleKernel) else k).batch_shape.numel()) for k in self.kernels)
        for k in self.kernels:
            base = k.base_kernel if isinstance(k, ScaleKernel) else k
            dims = list(base.active_dims) if base.active_dims is not None else list(range(d))
            ls = base.lengthscale.reshape(-1, len(dims))                       # (batch, |dims|)
            ell_g = torch.full((ls.shape[0], d), float("inf"), dtype=ls.dtype, device=ls.device)
            ell_g = ell_g.index_copy(1, torch.tensor(dims, device=ls.device), ls)
            kinds.append(base.kind)
            ells.append(ell_g.expand(nb, d))
            os_g = k.outputscale.reshape(-1) if isinstance(k, ScaleKernel) else torch.ones(1, dtype=ls.dtype, device=ls.device)
            oss.append(os_g.expand(nb))
        if len(set(kinds)) != 1:
            raise NotImplementedError("all sub-kernels of a decomposition must be of the same type")
        return kinds[0], torch.stack(ells, 1), torch.stack(oss, 1)

    def _pieces(self, d, like=None):
        """The component table, for the wrappers that ask a kernel for its pieces (sgpr.InducingPointKernel, the variational strategies)."""
        return self.table(d)

    def forward(self, x1, x2=None, **params):
        kind, ell, osc = self.table(x1.shape[-1])
        return LazyKernel(kind, x1, x1 if x2 is None else x2, ell, osc, torch.Size([ell.shape[0]]))
