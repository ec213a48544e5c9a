"""Host side of the additive (`decomp`) kernels on the batched exact engine: the C ABI exports and binds the new entry points,
and the kernel factory builds the component table of include/plmc.h ("Additive kernels") without a device."""
import ctypes

import torch

NEW_TYPED = ["plmc_assemble_add", "plmc_assemble_cross_add", "plmc_factorize_add_ex", "plmc_kinv_grad_add_vd"]


def test_library_exports_and_binds_the_additive_entry_points():
    from projectedlmc import _hip
    cdll = ctypes.CDLL(_hip.LIB_PATH)
    names = [b + s for b in NEW_TYPED for s in ("_f32", "_f64")] + ["plmc_max_components"]
    for name in names:
        assert hasattr(cdll, name), name
        assert name in _hip.exported_symbols(), name
    for b in NEW_TYPED:                                    # the additive form takes one int (the component count) more
        single = b.replace("_add", "")
        assert len(_hip._TYPED[b]) == len(_hip._TYPED[single]) + 1, b
    lib = _hip.lib()
    assert lib.cdll.plmc_max_components() >= 4
    assert lib.cdll.plmc_version() == _hip.ABI_VERSION == 4
    for b in NEW_TYPED:
        for suf in ("_f32", "_f64"):
            assert getattr(lib.cdll, b + suf).argtypes == _hip._TYPED[b]


def _table(n_funcs):
    import projectedlmc as plmc
    from projectedlmc.kernels import LazyKernel
    torch.manual_seed(0)
    k = plmc.handle_covar_(plmc.MaternKernel, 3, decomp=[[0, 1], [2]], n_funcs=n_funcs).double()
    with torch.no_grad():
        for prm in k.parameters():
            prm.add_(0.3 * torch.randn(prm.shape, dtype=prm.dtype))
    x = torch.rand(7, 3, dtype=torch.float64)              # CPU tensors: building the descriptor needs no device
    lazy = k(x)
    assert isinstance(lazy, LazyKernel) and lazy.kind == "matern52" and lazy.x1 is x and lazy.is_square
    return k, lazy


def test_decomp_descriptor_carries_the_component_table():
    for q in (3, 1):
        k, lazy = _table(q)
        table = lazy.inv_ell
        assert table.shape == (q, 2, 3) and lazy.ell.shape == (q, 2, 3) and lazy.oscale.shape == (q, 2)
        assert lazy.shape == (q, 7, 7) and lazy.batch_shape == (q,)
        active = torch.tensor([[True, True, False], [False, False, True]])
        assert bool((table[:, ~active] == 0).all()) and bool((table[:, active] > 0).all())
        assert bool(torch.isinf(lazy.ell[:, ~active]).all())
        for g, idx in enumerate([[0, 1], [2]]):
            sub = k.kernels[g]
            assert torch.equal(lazy.ell[:, g, idx], sub.base_kernel.lengthscale.reshape(q, -1))
            assert torch.equal(lazy.oscale[:, g], sub.outputscale.reshape(q))
        # the prior variance is the sum of the output scales; the noise rides on the descriptor like on any other
        assert torch.allclose(lazy.diagonal(), lazy.oscale.sum(-1, keepdim=True).expand(q, 7))
        noisy = lazy.add_noise(torch.full((q,), 0.5, dtype=torch.float64))
        assert noisy.ell is lazy.ell and torch.allclose(noisy.diagonal(), lazy.diagonal() + 0.5)


def test_table_gradient_reaches_only_the_active_lengthscales():
    """A sub-kernel owns len(group) lengthscales: a gradient on the (q, G, d) table is gathered back into them."""
    k, lazy = _table(3)
    w = 1.0 + torch.arange(18, dtype=torch.float64).reshape(3, 2, 3)
    torch.where(torch.isinf(lazy.ell), torch.zeros_like(lazy.ell), lazy.ell * w).sum().backward()
    g0, g1 = (k.kernels[g].base_kernel.raw_lengthscale.grad for g in (0, 1))
    assert g0.shape == (3, 1, 2) and g1.shape == (3, 1, 1)
    assert bool(torch.isfinite(g0).all()) and bool(torch.isfinite(g1).all()) and bool((g0 != 0).all()) and bool((g1 != 0).all())
