"""The pivot check and the jitter ladder (gpytorch's psd_safe_cholesky [gpytorch-knowledge]) at every site of the host layer that
factorises a possibly non-positive-definite matrix: the exact-GP engine (LOO, eval-mode posterior with and without the
prediction cache, the log-prob outside any deferred_pivot_checks), the dense-LMC log-prob and the K_ZZ factorisations of the
variational path.

A non-PD matrix is ordinary input here (`info != 0` from the sweep), not a fault.  The failing input is the one of
test_gpu_projected._singular_model: fp32, RBF, n = 300 points on U(-1, 1)^2, lengthscales 5, noise e^-40.  That it "needs
jitter" is a property of the input, checked on the host first: an fp32 LAPACK Cholesky of the matrix fails without jitter and at
the first rung 1e-6, and succeeds at a rung <= 1e-1 -- reachable under settings.cholesky_max_tries(8), the reference's training
loop setting (experiments.py:265)."""
import math
import re
import warnings

import pytest
import torch

from oracle import gp_math as gm
from oracle import lmc_dense as ld

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N, D, Q, P = 300, 2, 2, 2
NOISE = math.exp(-40.0)
WARN_FMT = "A not p.d., added jitter of %.1e to the diagonal"
EXHAUSTED = "Matrix not positive definite after repeatedly adding jitter up to 1.0e-06"


@pytest.fixture(scope="module")
def eng():
    import types
    from projectedlmc import _engine, _lmc_engine, _var_engine, settings
    assert torch.cuda.is_available()
    return types.SimpleNamespace(exact=_engine, lmc=_lmc_engine, var=_var_engine, settings=settings)


def _inputs():
    g = torch.Generator().manual_seed(3)
    X = (2 * torch.rand(N, D, generator=g, dtype=torch.float64) - 1).float()
    y = torch.randn(Q, N, generator=g, dtype=torch.float64).float()
    Xs = (2 * torch.rand(40, D, generator=g, dtype=torch.float64) - 1).float()
    Y = torch.randn(N, P, generator=g, dtype=torch.float64).float()
    F = torch.randn(Q, P, 1, generator=g, dtype=torch.float64)
    B = (F @ F.transpose(-1, -2) + 0.2 * torch.eye(P, dtype=torch.float64)).float()
    return X, y, Xs, Y, torch.full((Q, D), 5.0), torch.full((Q,), NOISE), B, NOISE * torch.eye(P)


def _host_rung(K):
    """Index of the first rung 1e-6 * 10^i at which the fp32 LAPACK Cholesky of K + (e^-40 + jitter) I succeeds for every
    matrix of the batch; asserts that it fails without jitter and at rung 0, and that the rung found is <= 1e-1."""
    base = 1e-6
    eye = torch.eye(K.shape[-1])
    ok = lambda jit: not bool(torch.linalg.cholesky_ex(K + (NOISE + jit) * eye)[1].any())
    assert K.dtype == torch.float32 and not ok(0.0) and not ok(base)
    k = next(i for i in range(1, 8) if ok(base * 10 ** i))
    assert base * 10 ** k <= 1e-1
    return k


@pytest.fixture(scope="module")
def problem():
    X, y, Xs, Y, ell, noise, B, S = _inputs()
    _host_rung(gm.kernel_matrix("rbf", X, X, ell))
    _host_rung(ld.lmc_covariance("rbf", X, ell, B, torch.zeros(P, P)))
    f = lambda t: t.to(DEV)
    return dict(X=f(X), y=f(y), Xs=f(Xs), Y=f(Y), ell=f(ell), noise=f(noise), B=f(B), S=f(S))


def _recorded(fn):
    """(result, jitters warned) of fn(); every jitter warning must be a RuntimeWarning with exactly the ladder's text."""
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out = fn()
        torch.cuda.synchronize()
    jit = []
    for w in rec:
        msg = str(w.message)
        if "not p.d." in msg or "added jitter" in msg:
            assert issubclass(w.category, RuntimeWarning), w
            m = re.fullmatch(r"A not p\.d\., added jitter of (\d\.\de[-+]\d\d) to the diagonal", msg)
            assert m is not None and msg == WARN_FMT % float(m.group(1)), msg
            jit.append(msg)
    return out, jit


def _ladder_ok(eng, jit, dtype=torch.float32):
    base = eng.settings.cholesky_jitter.value(dtype)
    assert 1 <= len(jit) <= 8
    assert jit == [WARN_FMT % (base * 10 ** i) for i in range(len(jit))], jit
    return len(jit)


def _finite(out):
    out = out if isinstance(out, (tuple, list)) else (out,)
    return all(bool(torch.isfinite(t).all()) for t in out)


# ------------------------------------------------------------------------------------------------ the sites
def _loo(eng, P_):
    return eng.exact.exact_loo("rbf", P_["X"], P_["ell"], None, P_["noise"], P_["y"])


def _posterior(eng, P_, cache=None, key=None):
    return eng.exact.exact_posterior("rbf", P_["X"], P_["ell"], None, P_["noise"], P_["y"], P_["Xs"], cache=cache, key=key)


def _log_prob(eng, P_, grad=True):
    ell = P_["ell"].clone().requires_grad_(grad)
    lp = eng.exact.exact_latent_log_prob("rbf", P_["X"], ell, None, P_["noise"], P_["y"])
    if grad:
        lp.sum().backward()
        return lp.detach(), ell.grad
    return lp


def _lmc(eng, P_, grad=True):
    ones = torch.ones(Q, device=DEV)
    leaves = [t.clone().requires_grad_(grad) for t in (P_["ell"], ones, P_["B"], P_["S"], P_["Y"].reshape(-1))]
    lp = eng.lmc.lmc_exact_log_prob("rbf", P_["X"], *leaves)
    if grad:
        lp.backward()
        return [lp.detach()] + [t.grad for t in leaves]
    return lp


SITES = {"exact_loo": _loo, "exact_posterior": _posterior, "exact_latent_log_prob": _log_prob, "dense_lmc_log_prob": _lmc}


@pytest.mark.parametrize("site", list(SITES))
def test_ladder_walks_the_rungs_and_returns_finite_values(eng, problem, site):
    with eng.settings.cholesky_max_tries(8):
        out, jit = _recorded(lambda: SITES[site](eng, problem))
    k = _ladder_ok(eng, jit)
    print("%s: left the ladder at rung %d (%s)" % (site, k - 1, jit[-1]))
    assert _finite(out)


@pytest.mark.parametrize("site", list(SITES))
def test_ladder_exhausted_raises_the_final_error(eng, problem, site):
    with eng.settings.cholesky_max_tries(1), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(RuntimeError, match=EXHAUSTED):
            SITES[site](eng, problem)


def test_prediction_cache_build_walks_the_ladder(eng, problem):
    """Two calls with one key under prediction_cache "lazy": the first runs the plain augmented sweep, the second builds the
    cached factorisation (a workspace of its own, inverse factor and kept planes); both go through the ladder."""
    cache, key = eng.exact.PosteriorCache(), ("state", 1)
    with eng.settings.prediction_cache("lazy"), eng.settings.cholesky_max_tries(8):
        out1, jit1 = _recorded(lambda: _posterior(eng, problem, cache, key))
        assert cache.ws is None and cache.seen == key
        out2, jit2 = _recorded(lambda: _posterior(eng, problem, cache, key))
        assert cache.ws is not None and cache.key == key
        out3, jit3 = _recorded(lambda: _posterior(eng, problem, cache, key))          # a hit factorises nothing
    _ladder_ok(eng, jit1)
    _ladder_ok(eng, jit2)
    assert jit3 == [] and cache.hits == 1
    assert _finite(out1) and _finite(out2) and _finite(out3)


def test_prediction_cache_build_exhausted_raises(eng, problem):
    cache, key = eng.exact.PosteriorCache(), ("state", 2)
    with eng.settings.prediction_cache("lazy"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with eng.settings.cholesky_max_tries(8):
            _posterior(eng, problem, cache, key)
        assert cache.ws is None and cache.seen == key
        with eng.settings.cholesky_max_tries(1), pytest.raises(RuntimeError, match=EXHAUSTED):
            _posterior(eng, problem, cache, key)                                          # the build
        assert cache.ws is None


def test_loo_and_log_prob_stop_at_the_same_rung(eng, problem):
    """The eager site (factorize_checked behind exact_loo) and the deferred one (the log-prob with gradients: the same
    workspace shape, the same sweep) see the same `info` words, so they leave the ladder together."""
    with eng.settings.cholesky_max_tries(8):
        _, jit_loo = _recorded(lambda: _loo(eng, problem))
        _, jit_lp = _recorded(lambda: _log_prob(eng, problem))
    assert jit_loo == jit_lp and len(jit_loo) >= 1


@pytest.mark.parametrize("site", list(SITES))
def test_check_off_neither_warns_nor_raises(eng, problem, site):
    """settings.check_cholesky(False): no read-back of `info`, hence no ladder; the value is whatever the failed sweep left."""
    with eng.settings.check_cholesky(False), eng.settings.cholesky_max_tries(1):
        _, jit = _recorded(lambda: SITES[site](eng, problem))
    assert jit == []


# ------------------------------------------------------------------------------------------------ variational sites
KZZ_NOT_PD = r"K_ZZ \+ jitter not positive definite"


@pytest.fixture(scope="module")
def kzz(problem):
    """Duplicate inducing points and jitter 0: K_ZZ is exactly singular (and numerically far from full rank before that)."""
    Z = torch.cat([problem["X"][:N // 2], problem["X"][:N // 2]])
    K = gm.kernel_matrix("rbf", Z.cpu(), Z.cpu(), problem["ell"].cpu())
    assert K.dtype == torch.float32 and bool(torch.linalg.cholesky_ex(K)[1].all())
    g = torch.Generator().manual_seed(5)
    mvar = torch.randn(Q, N, generator=g).to(DEV)
    Ls = (torch.eye(N) + 0.01 * torch.randn(Q, N, N, generator=g).tril()).to(DEV)
    return dict(Z=Z, X=problem["Xs"], ell=problem["ell"], mvar=mvar, Ls=Ls)


def test_prior_cholesky_raises_on_a_singular_kzz(eng, kzz):
    with pytest.raises(RuntimeError, match=KZZ_NOT_PD):
        eng.var.prior_cholesky("rbf", kzz["Z"], kzz["ell"], None, 0.0)


def test_unwhitened_predictive_raises_on_a_singular_kzz(eng, kzz):
    with pytest.raises(RuntimeError, match=KZZ_NOT_PD):
        eng.var.unwhitened_predictive("rbf", kzz["Z"], kzz["X"], kzz["ell"], None, kzz["mvar"], kzz["Ls"], 0.0)


def test_whitened_interp_raises_in_forward_without_gradients(eng, kzz):
    with pytest.raises(RuntimeError, match=KZZ_NOT_PD):
        eng.var.whitened_interp("rbf", kzz["Z"], kzz["X"], kzz["ell"], None, 0.0)


def test_whitened_interp_raises_in_backward_with_gradients(eng, kzz):
    ell = kzz["ell"].clone().requires_grad_()
    A = eng.var.whitened_interp("rbf", kzz["Z"], kzz["X"], ell, None, 0.0)          # the check waits for backward()
    assert A.shape == (Q, N, kzz["X"].shape[0])
    with pytest.raises(RuntimeError, match=KZZ_NOT_PD):
        A.sum().backward()


def test_gaussian_kl_raises_in_forward_without_gradients(eng, kzz):
    with pytest.raises(RuntimeError, match=KZZ_NOT_PD):
        eng.var.gaussian_kl_to_kernel_prior("rbf", kzz["Z"], kzz["ell"], None, kzz["mvar"], kzz["Ls"], 0.0)


def test_gaussian_kl_raises_in_backward_with_gradients(eng, kzz):
    ell = kzz["ell"].clone().requires_grad_()
    kl = eng.var.gaussian_kl_to_kernel_prior("rbf", kzz["Z"], ell, None, kzz["mvar"], kzz["Ls"], 0.0)
    assert kl.shape == (Q,)
    with pytest.raises(RuntimeError, match=KZZ_NOT_PD):
        kl.sum().backward()
