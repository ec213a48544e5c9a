"""Differentiable predictions without a device: the fp64 reference the GPU tests hold plmc_posterior_dx against
(tests/_posterior_dx_dense.py) equals autograd through a dense-Cholesky posterior for every family; the library exports the entry points
and refuses bad arguments through plmc_last_error() before it looks at a device; the backward formula of the autograd node and the
detaching of an input_transform's parameters are exercised with a stand-in for the engine call."""
import ctypes

import pytest
import torch

import _posterior_dx_dense as pdd


@pytest.mark.parametrize("family", pdd.FAMILIES)
def test_reference_equals_autograd_of_the_dense_posterior(family):
    """With alpha = Khat^-1 y and B = Khat^-1 K*^T the two sums ARE d mean / dx* and d var / dx*: the diagonal k(x*, x*) is constant."""
    n, ns, d, q = 40, 7, 3, 2
    p = pdd.problem(family, d, q, seed=3)
    X = pdd.igd.inputs(n, d, seed=3)
    Xs = pdd.query_points(ns, d, seed=3)
    g = torch.Generator().manual_seed(11)
    y = torch.randn(q, n, generator=g, dtype=torch.float64)
    noise = torch.tensor([0.1, 0.3], dtype=torch.float64)
    alpha, B = pdd.solved_operands(p.K, X, y, noise, Xs)
    Jm, Jv, Tm, Tv = pdd.posterior_dx_ref(p.K, X, Xs, alpha, B)
    Xa = Xs.clone().requires_grad_(True)
    mean, var = pdd.dense_posterior(p.K, X, y, noise, Xa)
    for lat in range(q):
        wm, = torch.autograd.grad(mean[lat].sum(), Xa, retain_graph=True)
        wv, = torch.autograd.grad(var[lat].sum(), Xa, retain_graph=True)
        live_m, live_v = Tm[lat] > 0, Tv[lat] > 0
        em = float(((Jm[lat] - wm).abs()[live_m] / Tm[lat][live_m]).max())
        ev = float(((Jv[lat] - wv).abs()[live_v] / Tv[lat][live_v]).max())
        print("%s latent %d: error / sum |terms|: mean %.3e, variance %.3e" % (family, lat, em, ev))
        assert em <= 1e-12 and ev <= 1e-12, (family, lat, em, ev)
        assert bool((wm[~live_m] == 0).all()) and bool((wv[~live_v] == 0).all())
    assert bool((Tm >= Jm.abs() * (1 - 1e-12)).all()) and bool((Tv >= Jv.abs() * (1 - 1e-12)).all())     # a sum of absolute terms bounds the sum
    assert bool((Jm[:, :, p.zero] == 0).all()) and bool((Jv[:, :, p.zero] == 0).all()) and bool((Tm[:, :, p.zero] == 0).all())


def test_library_exports_the_entry_points():
    from projectedlmc import _hip
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for infix in ("", "_add", "_sm", "_per", "_rq", "_lper", "_sum", "_dot"):
        for suf in ("_f32", "_f64"):
            name = "plmc_posterior_dx" + infix + suf
            assert name in _hip.exported_symbols(), name
            assert hasattr(lib, name), name
    for name in ("plmc_posterior_dx_splits", "plmc_posterior_dx_partials_bytes"):
        assert name in _hip.exported_symbols() and hasattr(lib, name), name
    assert lib.plmc_version() == _hip.ABI_VERSION == 4                  # symbols are only added


def test_split_count_is_a_function_of_the_sizes_alone():
    from projectedlmc import _hip
    L = _hip.lib().cdll
    assert L.plmc_posterior_dx_splits(129, 37, 3) == 1 and L.plmc_posterior_dx_partials_bytes(129, 37, 5, 3) == 0
    s = L.plmc_posterior_dx_splits(1100, 3, 3)
    assert s > 1 and L.plmc_posterior_dx_partials_bytes(1100, 3, 5, 3) == 2 * s * 3 * 3 * 5 * 8
    assert L.plmc_posterior_dx_splits(8192, 16, 8) > L.plmc_posterior_dx_splits(8192, 2048, 8) >= 1
    assert L.plmc_posterior_dx_splits(0, 3, 3) == 0 and L.plmc_posterior_dx_splits(5, 0, 3) == 0


def test_argument_errors_come_back_without_a_device():
    """Refused families, d above a family's capacity and ns <= 0 fail through plmc_last_error() before anything is launched: the
    pointers below are host memory that no kernel could read."""
    from projectedlmc import _hip
    L = _hip.lib()
    n, ns, q = 6, 2, 2
    host = (ctypes.c_double * 4096)()
    P = ctypes.cast(host, ctypes.c_void_p)
    fam = (ctypes.c_int * 2)(0, 16)
    tail = (P, n, P, ns, ns, P, P, None, q, None)                       # alpha, n_pad, B, ldb, strideB, Jm, Jv, partials, q, stream

    def refused(base, head, table, word, ns_=ns):
        with pytest.raises(RuntimeError, match=base + r"_f64 failed.*" + word):
            L.call(base, torch.float64, *head, P, n, P, ns_, *table, *tail)

    refused("plmc_posterior_dx", (4,), (3, P, None), "spline")
    refused("plmc_posterior_dx_add", (4,), (3, 2, P, None), "spline")
    refused("plmc_posterior_dx_sum", (), (2, 2, ctypes.cast(fam, ctypes.c_void_p), P, None), "sum")
    refused("plmc_posterior_dx_dot", (), (3, P, P, 1, None), "dot-product")
    refused("plmc_posterior_dx", (3,), (33, P, None), "plmc_max_dim")
    refused("plmc_posterior_dx_add", (3,), (3, 5, P, None), "plmc_max_components")
    refused("plmc_posterior_dx_sm", (), (9, 2, P, P, None), "plmc_sm_max_dim")
    refused("plmc_posterior_dx_sm", (), (2, 9, P, P, None), "plmc_sm_max_mixtures")
    refused("plmc_posterior_dx_per", (), (9, P, P, None), "plmc_per_max_dim")
    refused("plmc_posterior_dx_lper", (), (9, P, P, P, None), "plmc_lper_max_dim")
    refused("plmc_posterior_dx_rq", (), (17, P, P, None), "plmc_rq_max_dim")
    refused("plmc_posterior_dx", (3,), (3, P, None), "ns > 0", ns_=0)
    refused("plmc_posterior_dx", (3,), (3, P, None), "ns > 0", ns_=-1)


@pytest.mark.parametrize("kind", ["spline", "linear", "poly3", "sum(rbf,periodic)"])
def test_refused_kinds_and_full_cov_raise_before_the_device_check(kind):
    from projectedlmc import _engine
    n, ns, d, q = 12, 3, 2, 2
    X, Xs = torch.rand(n, d), torch.rand(ns, d)
    y, noise = torch.randn(q, n), torch.full((q,), 0.1)
    ell = torch.ones(q, 2, 3 * d + 1) if kind.startswith("sum") else torch.ones(q, d + 1) if kind != "spline" else torch.ones(q, d)
    with pytest.raises(NotImplementedError, match=kind.replace("(", r"\(").replace(")", r"\)")):
        _engine.exact_posterior(kind, X, ell, None, noise, y, Xs.clone().requires_grad_())
    with pytest.raises(NotImplementedError, match="full_cov"):
        _engine.exact_posterior("matern52", X, torch.ones(q, d), None, noise, y, Xs.clone().requires_grad_(), full_cov=True)
    # without a gradient for the test inputs nothing changes: host tensors meet the device check
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _engine.exact_posterior(kind, X, ell, None, noise, y, Xs)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        _engine.exact_posterior(kind, X, ell, None, noise, y, Xs.clone().requires_grad_())


def _stand_in(monkeypatch, q, seed=0):
    """Replaces the engine call of the autograd node by one that returns fixed random moments and Jacobians on the host."""
    from projectedlmc import _engine
    made = {}

    def fake(kind, X, ell, oscale, noise, y, Xs, full_cov=False, cache=None, key=None, dx=None):
        g = torch.Generator().manual_seed(seed)
        ns, d = Xs.shape
        made["dx"], made["Xs"] = dx, Xs
        made["Jm"] = torch.randn(q, ns, d, generator=g, dtype=torch.float64)
        made["Jv"] = torch.randn(q, ns, d, generator=g, dtype=torch.float64) if dx == "both" else None
        made["mean"], made["var"] = torch.randn(q, ns, generator=g).to(Xs.dtype), torch.rand(q, ns, generator=g).to(Xs.dtype)
        return (made["mean"], made["var"]) + ((made["Jm"], made["Jv"]) if dx is not None else ())

    monkeypatch.setattr(_engine, "_exact_posterior", fake)
    return made


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["float64", "float32"])
def test_backward_is_the_element_wise_formula(monkeypatch, dt):
    from projectedlmc import _engine, settings
    q, n, ns, d = 3, 9, 5, 4
    made = _stand_in(monkeypatch, q)
    X, ell, noise, y = torch.rand(n, d, dtype=dt), torch.ones(q, d, dtype=dt), torch.full((q,), 0.1, dtype=dt), torch.randn(q, n, dtype=dt)
    Xs = torch.rand(ns, d, dtype=dt).requires_grad_()
    mean, var = _engine.exact_posterior("matern52", X, ell, None, noise, y, Xs)
    assert made["dx"] == "both" and torch.equal(mean, made["mean"]) and torch.equal(var, made["var"])
    assert mean.requires_grad and var.requires_grad
    a, b = torch.randn(q, ns, dtype=dt), torch.randn(q, ns, dtype=dt)
    (a * mean + b * var).sum().backward()
    want = (a.double()[:, :, None] * made["Jm"]).sum(0) + (b.double()[:, :, None] * made["Jv"]).sum(0)      # fp64, one cast
    assert Xs.grad.dtype == dt and torch.allclose(Xs.grad, want.to(dt), rtol=4 * torch.finfo(dt).eps, atol=0)
    # only the mean is used downstream: the variance's upstream gradient is zero or absent
    Xs.grad = None
    mean, var = _engine.exact_posterior("matern52", X, ell, None, noise, y, Xs)
    (a * mean).sum().backward()
    assert torch.equal(Xs.grad, (a.double()[:, :, None] * made["Jm"]).sum(0).to(dt))
    # once differentiable
    mean, var = _engine.exact_posterior("matern52", X, ell, None, noise, y, Xs)
    g, = torch.autograd.grad(mean.sum(), Xs, create_graph=True)
    assert not g.requires_grad
    # mean-only work
    Xs.grad = None
    with settings.predictive_variance_grad(False):
        mean, var = _engine.exact_posterior("matern52", X, ell, None, noise, y, Xs)
    assert made["dx"] == "mean" and made["Jv"] is None and mean.requires_grad and not var.requires_grad
    (a * mean + b * var).sum().backward()
    assert torch.equal(Xs.grad, (a.double()[:, :, None] * made["Jm"]).sum(0).to(dt))
    assert settings.predictive_variance_grad.on()


def test_input_transform_is_applied_with_detached_parameters(monkeypatch):
    """The gradient reaches the raw x through the transform (chain rule), and no parameter of the transform gets a .grad."""
    import projectedlmc as plmc
    q, n, ns = 1, 20, 6
    made = _stand_in(monkeypatch, q, seed=4)
    torch.manual_seed(0)
    tf = torch.nn.Sequential(torch.nn.Linear(5, 3), torch.nn.Tanh()).double()
    X, y = torch.rand(n, 5, dtype=torch.float64), torch.rand(n, dtype=torch.float64)
    m = plmc.ExactGPModel(X, y, plmc.GaussianLikelihood(), input_transform=tf, kernel_type=plmc.MaternKernel).double().eval()
    x = torch.rand(ns, 5, dtype=torch.float64).requires_grad_()
    out = m(x)
    assert made["Xs"].requires_grad and made["Xs"].shape == (ns, 3)
    a, b = torch.randn(ns, dtype=torch.float64), torch.randn(ns, dtype=torch.float64)
    (a * out.mean + b * out.variance).sum().backward()
    assert x.grad is not None and all(prm.grad is None for prm in tf.parameters())
    xr = x.detach().clone().requires_grad_()
    gF = a[:, None] * made["Jm"][0] + b[:, None] * made["Jv"][0]
    (tf(xr) * gF).sum().backward()
    assert torch.allclose(x.grad, xr.grad, rtol=1e-13, atol=1e-15)
    # a test input without a gradient takes the features without a graph, as before
    m(x.detach())
    assert not made["Xs"].requires_grad and made["dx"] is None
