"""d logp / dX of the batched exact engine: `_engine.exact_latent_log_prob` with X.requires_grad_() against fp64 autograd of the dense
Cholesky log density (tests/_input_grad_dense.py), per family, in both forms of the node -- one node, and the two-node form with the
hyper-parameter gradients on the gradient stream -- with PLMC_GRAD_STREAM=0 and the default, under a weighted upstream gradient.  A run
without X.requires_grad is bit for bit what it was: same loss, same hyper-parameter gradients, same sequence of library calls."""
import functools

import pytest
import torch

import _input_grad_dense as igd

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N, D, Q = 300, 3, 2
FAMILIES = tuple(igd.STATIONARY) + ("add", "rq", "periodic", "locally_periodic", "sm3")
WEIGHTS = torch.tensor([0.7, -1.3], dtype=torch.float64)


@pytest.fixture(scope="module")
def eng():
    from projectedlmc import _engine
    assert torch.cuda.is_available()
    return _engine


@functools.lru_cache(maxsize=None)
def _reference(family):
    """(problem, X, y, noise, d logp_l / dX (q, n, d)) at fp32-representable values, once for both element types."""
    p = igd.problem("add_disjoint", D, Q, 21, groups=[[0, 1], [2]]) if family == "add" else igd.problem(family, D, Q, 21)
    X = igd.inputs(N, D, 21)
    g = torch.Generator().manual_seed(22)
    y = torch.randn(Q, N, generator=g, dtype=torch.float64).float().double()
    noise = torch.tensor([0.1, 0.3]).double()
    return p, X, y, noise, igd.mll_input_grad(p.K, X, noise, y)


def _run(eng, family, dt, x_grad=True, hyper_grad=True, weights=WEIGHTS):
    p, X, y, noise, _ = _reference(family)
    f = lambda t, g=False: None if t is None else t.to(DEV, dt).contiguous().requires_grad_(g)
    Xd, ell, osc, nz, yd = f(X, x_grad), f(p.ell, hyper_grad), f(p.oscale, hyper_grad), f(noise, hyper_grad), f(y)
    lp = eng.exact_latent_log_prob(p.kind, Xd, ell, osc, nz, yd)
    (weights.to(DEV, dt) * lp).sum().backward()
    torch.cuda.synchronize()
    return lp.detach(), Xd.grad, ell.grad, nz.grad, (None if osc is None else osc.grad)


def _check(got, want, dt):
    got = got.cpu().double()
    if dt == torch.float64:
        assert torch.allclose(got, want, rtol=1e-7, atol=1e-9), float((got - want).abs().max())
    else:
        err = float((got - want).abs().max() / want.abs().max())
        print("fp32 input gradient: %.2e of the largest magnitude" % err)
        assert err < 2e-3, err


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("family", FAMILIES)
def test_input_gradient_of_the_mll(eng, family, dt):
    """The default form: with a gradient stream and hyper-parameters that require a gradient, the two-node form."""
    want = (WEIGHTS[:, None, None] * _reference(family)[4]).sum(0)
    got = _run(eng, family, dt)[1]
    assert got is not None and got.dtype == dt and got.shape == (N, D)
    _check(got, want, dt)


@pytest.mark.parametrize("env,hyper_grad", [("1", False), ("0", True), ("0", False)], ids=["one-node", "no-stream", "no-stream-x-only"])
@pytest.mark.parametrize("family", ["matern52", "sm3"])
def test_input_gradient_in_the_one_node_form(eng, family, env, hyper_grad, monkeypatch):
    """Only X requires a gradient (no _HyperGrad node), and PLMC_GRAD_STREAM=0 (everything on the caller's stream)."""
    monkeypatch.setenv("PLMC_GRAD_STREAM", env)                     # Python-level knob, read per call
    want = (WEIGHTS[:, None, None] * _reference(family)[4]).sum(0)
    out = _run(eng, family, torch.float64, hyper_grad=hyper_grad)
    _check(out[1], want, torch.float64)
    assert (out[2] is None) == (not hyper_grad)


@pytest.mark.parametrize("env", ["1", "0"], ids=["grad-stream", "no-stream"])
@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["float64", "float32"])
def test_nothing_changes_when_x_requires_no_gradient(eng, dt, env, monkeypatch):
    """Loss and hyper-parameter gradients are the same bits with and without X.requires_grad, and the library sees the same calls plus
    exactly one plmc_input_grad."""
    from projectedlmc import _hip
    monkeypatch.setenv("PLMC_GRAD_STREAM", env)
    L = _hip.lib()
    calls = []
    real = L.call

    def recording(base, dtype, *args):
        calls.append(base)
        return real(base, dtype, *args)

    monkeypatch.setattr(L, "call", recording)
    _run(eng, "matern52", dt, x_grad=False)                              # (workspaces exist from here on)
    del calls[:]
    plain = _run(eng, "matern52", dt, x_grad=False)
    seq_plain = list(calls)
    del calls[:]
    withx = _run(eng, "matern52", dt, x_grad=True)
    seq_x = list(calls)
    assert plain[1] is None and withx[1] is not None
    for a, b in zip(plain[:1] + plain[2:], withx[:1] + withx[2:]):
        assert torch.equal(a, b)
    assert [c for c in seq_x if not c.startswith("plmc_input_grad")] == seq_plain
    assert sum(c.startswith("plmc_input_grad") for c in seq_x) == 1
    assert seq_x.index("plmc_input_grad") == seq_x.index("plmc_kinv_grad_vd") + 1


@pytest.mark.parametrize("kind", ["spline", "linear", "poly3", "sum(rbf,periodic)"])
def test_refused_kinds_do_not_return_a_silent_none(eng, kind):
    d = 2
    X = torch.rand(50, d, dtype=torch.float64, device=DEV).requires_grad_()
    shape = (Q, 2, 3 * d + 1) if kind.startswith("sum") else (Q, d) if kind == "spline" else (Q, d + 1)
    ell = torch.ones(*shape, dtype=torch.float64, device=DEV)
    with pytest.raises(NotImplementedError, match="inputs"):
        eng.exact_latent_log_prob(kind, X, ell, None, torch.full((Q,), 0.1, dtype=torch.float64, device=DEV),
                                  torch.randn(Q, 50, dtype=torch.float64, device=DEV))
