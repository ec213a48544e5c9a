"""The fp16 operand scales of the two-plane split engine (the fp32 default), read from the scale block a sweep leaves in its Vd
scratch (plmc_split_scales_offset) and compared, exactly, with the host restatement of the input matrix (tests/_split_scales.py):
unpadded and padded n, a largest diagonal entry below 1 and a noise above the pivots, the 1e-12 D clamp, zero and large
right-hand sides, latents of very different magnitudes in one call -- under the fused assembly + sweep (plmc_factorize_ex), the
two calls and the one-stream schedule.  Plus: accuracy against the fp64 oracle where the scales differ per latent, and the
scales and bits of the eval-mode cached prediction (plmc_potrs_aug_kept)."""
import contextlib

import numpy as np
import pytest
import torch

import _split_scales as ss
from oracle import gp_math as gm

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32 = torch.float32


@pytest.fixture(scope="module")
def eng():
    from projectedlmc import _engine
    assert torch.cuda.is_available()
    yield _engine
    _engine.free_workspaces()
    torch.cuda.empty_cache()


def _schedule(name):
    """fused: plmc_factorize_ex (the default of _engine.factorize); two-call: plmc_assemble + plmc_potrf_ex; serial: one stream."""
    from projectedlmc import _hip
    if name == "fused":
        return contextlib.nullcontext()
    if name == "two-call":
        return _hip.knob("PLMC_FUSED_ASSEMBLE", "0")
    return _hip.knob("PLMC_SERIAL", "1")


def _problem(n, d, q, osc, noise, seed, yscale=1.0):
    g = torch.Generator().manual_seed(seed)
    X = 2 * torch.rand(n, d, generator=g, dtype=torch.float64) - 1
    y = torch.randn(q, n, generator=g, dtype=torch.float64) * torch.as_tensor(yscale, dtype=torch.float64).reshape(-1, 1)
    ell = 0.4 + 0.5 * torch.rand(q, d, generator=g, dtype=torch.float64)
    osc = torch.as_tensor(osc, dtype=torch.float64).reshape(q)
    noise = torch.as_tensor(noise, dtype=torch.float64).reshape(q)
    return X, y, ell, osc, noise


def _dev(*ts):
    return [t.to(DEV, F32).contiguous() for t in ts]


def scale_block(ws):
    """(q, BLOCK) float32 numpy: every latent's scale block of the sweep's Vd scratch."""
    from projectedlmc import _hip
    off = int(_hip.lib().cdll.plmc_split_scales_offset(ws.n_pad, ws.lda))
    torch.cuda.synchronize()
    return ws.Vd.reshape(ws.q, -1)[:, off:off + ss.BLOCK].cpu().numpy()


def input_matrix(eng, X, ell, osc, noise, y, naug=1, Xs=None):
    """The sweep's input, assembled as plmc_assemble + plmc_write_rhs (+ plmc_assemble_cross) write it, into a workspace of its
    own: (diagonal (q, n_pad), augmented columns (q, n_pad, naug_pad)) as float32 numpy."""
    from projectedlmc import _hip
    L = _hip.lib()
    q, n = y.shape
    ws = eng.Workspace(n, q, naug, F32, DEV, False)
    st = _hip.stream_ptr(DEV)
    L.call("plmc_assemble", F32, _hip.KIND["matern52"], _hip.ptr(X), n, X.shape[1], _hip.ptr(ell), _hip.ptr(osc), _hip.ptr(noise),
           _hip.ptr(ws.A), ws.lda, ws.strideA, q, st)
    L.call("plmc_write_rhs", F32, _hip.ptr(y), 1, n, _hip.ptr(ws.A), ws.lda, ws.strideA, 0, ws.naug_pad, q, st)
    if Xs is not None:
        L.call("plmc_assemble_cross", F32, _hip.KIND["matern52"], _hip.ptr(X), n, _hip.ptr(Xs), Xs.shape[0], X.shape[1], _hip.ptr(ell),
               _hip.ptr(osc), _hip.ptr(ws.A), ws.lda, ws.strideA, ws.n_pad + 1, ws.n_pad, q, st)
    torch.cuda.synchronize()
    diag = torch.diagonal(ws.A[:, :, :ws.n_pad], dim1=1, dim2=2).cpu().numpy()
    aug = ws.A[:, :, ws.n_pad:ws.n_pad + ws.naug_pad].cpu().numpy()
    del ws
    return diag, aug


def factor(eng, ws, X, ell, osc, noise, y, eig_lo=None):
    """_engine.factorize (fused by default; PLMC_FUSED_ASSEMBLE=0: two calls), or with eig_lo the same calls through the C ABI
    with that eigenvalue bound instead of the noise."""
    from projectedlmc import _hip
    import os
    q, n = y.shape
    if eig_lo is None:
        eng.factorize("matern52", X, ell, osc, noise, y.reshape(q, 1, n), ws)
    else:
        L = _hip.lib()
        st = _hip.stream_ptr(DEV)
        k = _hip.KIND["matern52"]
        fused = os.environ.get("PLMC_FUSED_ASSEMBLE", "1") != "0"
        if not fused:
            L.call("plmc_assemble", F32, k, _hip.ptr(X), n, X.shape[1], _hip.ptr(ell), _hip.ptr(osc), _hip.ptr(noise), _hip.ptr(ws.A),
                   ws.lda, ws.strideA, q, st)
        L.call("plmc_write_rhs", F32, _hip.ptr(y), 1, n, _hip.ptr(ws.A), ws.lda, ws.strideA, 0, ws.naug_pad, q, st)
        if fused:
            L.call("plmc_factorize_ex", F32, k, _hip.ptr(X), n, X.shape[1], _hip.ptr(ell), _hip.ptr(osc), _hip.ptr(noise), _hip.ptr(ws.A),
                   ws.n_pad, ws.lda, ws.naug, ws.strideA, _hip.ptr(ws.Vd), _hip.ptr(ws.logdet), _hip.ptr(ws.info), 1, q, _hip.ptr(eig_lo), st)
        else:
            L.call("plmc_potrf_ex", F32, _hip.ptr(ws.A), ws.n_pad, ws.lda, ws.naug, ws.strideA, _hip.ptr(ws.Vd), _hip.ptr(ws.logdet),
                   _hip.ptr(ws.info), 1, q, _hip.ptr(eig_lo), st)
    torch.cuda.synchronize()
    assert not bool(ws.info.any()), ws.info
    assert bool(torch.isfinite(ws.logdet).all())


def assert_block(got, diag, aug, eig_lo, n_pad, vd_blocks, npl=2, what=""):
    for l in range(got.shape[0]):
        want = ss.split_scales(diag[l], aug[l], eig_lo[l], n_pad=n_pad, npl=npl, vd_blocks=vd_blocks)
        g = got[l]
        assert np.array_equal(g[ss.SC_TAG:ss.SC_TAG + 2], want["tag"]), (what, l, g[ss.SC_TAG:ss.SC_TAG + 2], want["tag"])
        bad = [(ss.NAMES[i], float(g[i]), float(want["block"][i])) for i in range(8) if g[i] != want["block"][i]]
        assert not bad, "%s latent %d: scale block differs from the input's restatement (name, sweep, input): %s" % (what, l, bad)


# (n, q, outputscales, noises, right-hand-side scale, eig_lo: None = the noise, 0 = no usable bound)
REGIMES = {
    # largest diagonal entry below 1: the factor's sqrt(pivot) exceeds it (D, RU, RW); 2304 = three groups, the look-ahead runs
    "u2304-small-diag": (2304, 4, [0.55, 0.63, 0.71, 0.8], [0.013, 0.05, 0.11, 0.17], 1.0, None),
    "u8192-small-diag": (8192, 8, np.linspace(0.6, 0.9, 8), np.linspace(0.011, 0.09, 8), 1.0, None),
    # noise above the pivots' square roots (lambda, SW, SA, RA)
    "u8192-noise4": (8192, 4, [1.0, 1.0, 0.7, 1.3], [3.3, 4.1, 4.6, 5.5], 1.0, None),
    # padded: the identity rows give D >= 1 and lambda <= 1 whatever the matrix
    "p2300-small-diag": (2300, 4, [0.55, 0.63, 0.71, 0.8], [0.013, 0.05, 0.11, 0.17], 1.0, None),
    "p2300-noise4": (2300, 4, [1.0, 1.0, 0.7, 1.3], [3.3, 4.1, 4.6, 5.5], 1.0, None),
    # eig_lo = 0: lambda = 1e-12 D (the noise itself keeps the matrix factorisable)
    "u2304-clamp": (2304, 2, [0.75, 1.4], [0.03, 0.2], 1.0, 0.0),
    "u2304-rhs0": (2304, 2, [0.75, 1.4], [0.03, 0.2], 0.0, None),
    "u2304-rhs1e4": (2304, 2, [0.75, 1.4], [0.03, 0.2], 1e4, None),
    # latents of very different magnitudes in one call: per-latent indexing of the scale block
    "u2304-mixed": (2304, 6, [1e-3, 0.05, 1.1, 30.0, 700.0, 4e4], [2.3e-6, 1.3e-4, 0.02, 0.7, 9.0, 80.0], "sqrt-osc", None),
}


def _regime(name, seed=11):
    n, q, osc, noise, ysc, eig_lo = REGIMES[name]
    osc_t = torch.as_tensor(np.asarray(osc, dtype=np.float64))
    if ysc == "sqrt-osc":
        ysc = osc_t.sqrt()
    X, y, ell, osc_t, noise_t = _problem(n, 4, q, osc_t, noise, seed, ysc)
    return X, y, ell, osc_t, noise_t, eig_lo


@pytest.mark.parametrize("sched", ["fused", "two-call", "serial"])
@pytest.mark.parametrize("regime", list(REGIMES))
def test_scales_are_those_of_the_input_matrix(eng, regime, sched):
    X, y, ell, osc, noise, eig_lo = _regime(regime)
    q, n = y.shape
    Xd, yd, elld, oscd, nzd = _dev(X, y, ell, osc, noise)
    diag, aug = input_matrix(eng, Xd, elld, oscd, nzd, yd)
    elo = nzd if eig_lo is None else torch.full_like(nzd, eig_lo)
    ws = eng.Workspace(n, q, 1, F32, DEV, True)
    with _schedule(sched):
        factor(eng, ws, Xd, elld, oscd, nzd, yd, None if eig_lo is None else elo)
    assert_block(scale_block(ws), diag, aug, elo.cpu().numpy(), ws.n_pad, ws.Vd.shape[1], what="%s/%s" % (regime, sched))
    del ws
    torch.cuda.empty_cache()


@pytest.mark.parametrize("regime", ["u2304-small-diag", "u2304-mixed"])
def test_bf16x3_scheme_writes_unit_scales(eng, regime):
    from projectedlmc import _hip
    X, y, ell, osc, noise, _ = _regime(regime)
    q, n = y.shape
    Xd, yd, elld, oscd, nzd = _dev(X, y, ell, osc, noise)
    ws = eng.Workspace(n, q, 1, F32, DEV, True)
    with _hip.knob("PLMC_SPLIT", "3"):
        factor(eng, ws, Xd, elld, oscd, nzd, yd)
    got = scale_block(ws)
    for l in range(q):
        assert np.array_equal(got[l, :8], np.ones(8, dtype=np.float32)), (l, got[l, :8])
        assert np.array_equal(got[l, ss.SC_TAG:ss.SC_TAG + 2], np.array([3, ws.Vd.shape[1]], dtype=np.float32))
    del ws


def test_logprob_and_grads_where_scales_differ_per_latent(eng):
    """One call whose latents span outputscales 1e-3 .. 4e4 and noises 2e-6 .. 80 (so every latent has scales of its own): log-prob
    and every gradient against the fp64 oracle, latent by latent, with the fp32 tolerances (1e-4 relative, 2e-3 of the largest)."""
    X, y, ell, osc, noise, _ = _regime("u2304-mixed", seed=3)
    ref = gm.exact_latent_log_prob_analytic("matern", X, ell, noise, y, osc, 2.5)
    Xd = X.to(DEV, F32)
    ell_d, nz_d, y_d, os_d = [t.to(DEV, F32).requires_grad_() for t in (ell, noise, y, osc)]
    lp = eng.exact_latent_log_prob("matern52", Xd, ell_d, os_d, nz_d, y_d)
    lp.sum().backward()
    torch.cuda.synchronize()
    lp = lp.detach().cpu().double()
    assert torch.isfinite(lp).all()
    rel = (lp - ref[0]).abs() / ref[0].abs()
    assert (rel < 1e-4).all(), rel
    for name, got, want in (("ell", ell_d.grad, ref[1]), ("noise", nz_d.grad, ref[2]), ("outputscale", os_d.grad, ref[3]), ("y", y_d.grad, ref[4])):
        got = got.detach().cpu().double().reshape(y.shape[0], -1)
        want = want.reshape(y.shape[0], -1)
        for l in range(y.shape[0]):
            err = float((got[l] - want[l]).abs().max() / want[l].abs().max())
            assert err < 2e-3, (name, l, err)


def test_kept_factor_prediction_scales_bits_and_mean(eng):
    """Eval-mode cached prediction (plmc_potrs_aug_kept, k_aug_scales) at unpadded n with the largest diagonal entry below 1:
    (a) the caching sweep's scale block is the restatement of its input; the cached call's SA / RA are the restatement with the new
    cross-covariance columns and the sweep's D / lambda; (b) the cached call is bit-identical whether the caching sweep was the fused
    call or the two calls; (c) its mean agrees with the fp64 oracle posterior (fp32 tolerance of test_gpu_prediction_cache.py)."""
    from projectedlmc import settings
    X, y, ell, osc, noise, _ = _regime("u2304-small-diag", seed=5)
    q, n = y.shape
    g = torch.Generator().manual_seed(9)
    Xs1 = 2 * torch.rand(200, X.shape[1], generator=g, dtype=torch.float64) - 1
    Xs2 = 2 * torch.rand(150, X.shape[1], generator=g, dtype=torch.float64) - 1
    y2 = 0.1 * y                                       # new targets too: the new columns' largest entry is a cross-covariance
    Xd, yd, y2d, elld, oscd, nzd, Xs1d, Xs2d = _dev(X, y, y2, ell, osc, noise, Xs1, Xs2)
    diag, aug1 = input_matrix(eng, Xd, elld, oscd, nzd, yd, naug=1 + Xs1.shape[0], Xs=Xs1d)
    _, aug2 = input_matrix(eng, Xd, elld, oscd, nzd, y2d, naug=1 + Xs1.shape[0], Xs=Xs2d)
    eig_lo = noise.float().numpy()
    outs = {}
    for sched in ("fused", "two-call"):
        cache = eng.PosteriorCache()
        with settings.prediction_cache("eager"), _schedule(sched):
            eng.exact_posterior("matern52", Xd, elld, oscd, nzd, yd, Xs1d, cache=cache, key="k")
            torch.cuda.synchronize()
            ws = cache.ws
            assert ws is not None and ws.keep_planes and ws.n_pad == n and (cache.hits, cache.misses) == (0, 1)
            assert_block(scale_block(ws), diag, aug1, eig_lo, ws.n_pad, ws.Vd.shape[1], what="caching sweep/%s" % sched)
            mean, var = eng.exact_posterior("matern52", Xd, elld, oscd, nzd, y2d, Xs2d, cache=cache, key="k")
            torch.cuda.synchronize()
            assert (cache.hits, cache.misses) == (1, 1)
        got = scale_block(ws)
        for l in range(q):
            want = ss.split_scales(diag[l], aug1[l], eig_lo[l], n_pad=ws.n_pad)
            sa, ra = ss.aug_scales(want["D"], want["lam"], aug2[l], ws.n_pad)
            assert (got[l, ss.SC_SA], got[l, ss.SC_RA]) == (sa, ra), (sched, l, got[l, :8], sa, ra)
            assert (got[l, ss.SC_D], got[l, ss.SC_LAM]) == (want["D"], want["lam"]), (sched, l)
        outs[sched] = (mean.clone(), var.clone(), ws.A.clone())
        cache.drop()
        del ws
    for a, b in zip(outs["fused"], outs["two-call"]):      # as bit patterns: a NaN left in a part of the buffer that no launch writes is unequal to itself
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "cached prediction differs between a fused and a two-call caching sweep"
    mu, cov = gm.exact_gp_posterior("matern", X, ell, noise, y2, Xs2, osc, 2.5)
    mean = outs["fused"][0].cpu().double()
    assert (mean - mu).abs().max() < 2e-4 * max(1.0, float(mu.abs().max()))
    del outs
    torch.cuda.empty_cache()
