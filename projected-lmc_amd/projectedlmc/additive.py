"""Additive sub-kernel decompositions, `decomp=[[0,1],[1,2]]` -> k(x) = s1 k1(x0,x1) + s2 k2(x1,x2)
(reference: handle_covar_, projected_lmc.py:131-167).

HIP path: the sum of G scaled ARD kernels on subsets of the input dimensions is a kernel kind of the batched exact engine
like any other.  Calling the module returns an ordinary `LazyKernel` whose hyper-parameters are a COMPONENT TABLE -- lengthscales
(q, G, d) with an infinite lengthscale (1 / ell = 0 exactly, `LazyKernel.inv_ell`) on the dimensions a component ignores, output
scales (q, G) -- for batch_shape [1] and [n_funcs] alike (the reference builds the decomposition with batch_shape=[n_funcs],
projected_lmc.py:151-167: batched exact GPs, the latent processes of the projected model).  The assembly, cross-assembly and
gradient kernels evaluate the G components per element (include/plmc.h, "Additive kernels"); the sweep, the pivot checks, the
prediction cache, `full_cov` and latent sharding do not look at the kernel and serve it unchanged.  A sub-kernel owns len(group)
lengthscales: autograd gathers the active slots of the table's gradient back into them (index_copy below)."""
import torch

from .kernels import Kernel, ScaleKernel, LazyKernel


class AdditiveKernel(Kernel):
    def __init__(self, *kernels):
        super().__init__()
        self.kernels = torch.nn.ModuleList(kernels)

    def __add__(self, other):
        return AdditiveKernel(*self.kernels, *(other.kernels if isinstance(other, AdditiveKernel) else [other]))

    def select(self, x):
        return x

    def table(self, d):
        """(kind, ell (batch, G, d), oscale (batch, G)) from the sub-kernels' parameters; needs no device."""
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
