"""The split engine's main loop (csrc/bf3_engine.hpp: a ring of three LDS stages for the two-plane fp16 scheme, requested two
stages ahead and retired by counted waits) at every stage-count class of the ring, at the depth classes of the updates and
panels, and under memory load that moves the landing times of its DMA pieces.  A stage read too early or overwritten too
early is an error of order 1 / stages in a tile, four orders above the bounds used here."""
import pytest
import torch

from oracle import gp_math as gm

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _problem(n, d, q, seed=0):
    """inputs as tests/test_gpu_engine.py::_problem: noise O(0.1-1)"""
    g = torch.Generator().manual_seed(seed)
    X = 2 * torch.rand(n, d, generator=g, dtype=torch.float64) - 1
    y = torch.randn(q, n, generator=g, dtype=torch.float64)
    ell = 0.3 + 0.5 * torch.rand(q, d, generator=g, dtype=torch.float64)
    noise = 0.05 + 0.5 * torch.rand(q, generator=g, dtype=torch.float64)
    osc = 0.5 + torch.rand(q, generator=g, dtype=torch.float64)
    return X, y, ell, noise, osc


@pytest.fixture(scope="module")
def eng():
    from projectedlmc import _engine
    assert torch.cuda.is_available()
    return _engine


def _sweep_and_kinv(eng, ws, Xd, yd, elld, nzd, n, d, q, want_kinv):
    """assemble + sweep + alpha + K^-1 and gradient (plmc_kinv_grad_ex: its own split pass over W) on workspace `ws`"""
    from projectedlmc import _hip
    L = _hip.lib()
    dt = torch.float32
    st = _hip.stream_ptr(DEV)
    L.call("plmc_assemble", dt, _hip.KIND["matern52"], _hip.ptr(Xd), n, d, _hip.ptr(elld), None, _hip.ptr(nzd), _hip.ptr(ws.A), ws.lda, ws.strideA, q, st)
    L.call("plmc_write_rhs", dt, _hip.ptr(yd), 1, n, _hip.ptr(ws.A), ws.lda, ws.strideA, 0, ws.naug_pad, q, st)
    L.call("plmc_potrf_ex", dt, _hip.ptr(ws.A), ws.n_pad, ws.lda, ws.naug, ws.strideA, _hip.ptr(ws.Vd), _hip.ptr(ws.logdet), _hip.ptr(ws.info), 1, q,
           _hip.ptr(nzd), st)
    L.call("plmc_extract_col", dt, _hip.ptr(ws.A), ws.n_pad, ws.lda, ws.strideA, 0, _hip.ptr(ws.z), _hip.ptr(ws.quad), q, st)
    L.call("plmc_wt_matvec", dt, _hip.ptr(ws.W), ws.n_pad, ws.ldw, ws.strideW, _hip.ptr(ws.z), _hip.ptr(ws.alpha), q, st)
    g = torch.zeros(q, d + 2, dtype=torch.float64, device=DEV)
    kd = torch.zeros(q, ws.n_pad, dtype=dt, device=DEV)
    Kinv = torch.zeros(q, ws.n_pad, ws.n_pad, dtype=dt, device=DEV) if want_kinv else None
    part = torch.empty(int(L.cdll.plmc_grad_scratch_bytes_for(ws.n_pad, q, 4)) // 8, dtype=torch.float64, device=DEV)
    L.call("plmc_kinv_grad_ex", dt, _hip.KIND["matern52"], _hip.ptr(ws.W), ws.n_pad, ws.ldw, ws.strideW, _hip.ptr(ws.alpha), _hip.ptr(Xd), n, d,
           _hip.ptr(elld), None, _hip.ptr(g), _hip.ptr(Kinv) if want_kinv else None, ws.n_pad if want_kinv else 0,
           ws.n_pad * ws.n_pad if want_kinv else 0, _hip.ptr(kd), _hip.ptr(part), q, _hip.ptr(nzd), st)
    torch.cuda.synchronize()
    return g, kd, Kinv


@pytest.mark.parametrize("n", [128, 256, 384, 512, 640, 768, 200, 517])
def test_kinv_tiles_at_every_stage_count_of_the_ring(eng, n):
    """K^-1 = W^T W through the split engine: tile depths 128 ... n_pad, i.e. 4 ... 24 stages of 32 rows -- every residue mod 2
    and mod 3 of the stage count, both halves of a macro tile, the reverse walk of the K range.  Upper triangle against the
    fp64 product of the fp32 W of the same sweep; the rule of test_split_engines_against_fp32_mfma_path:
    e_split < 2 e_plain + 2e-6, both relative to max |K^-1|, e_plain from the same call under PLMC_SPLIT=0."""
    from projectedlmc import _hip
    d, q = 3, 2
    X, y, ell, noise, _ = _problem(n, d, q, seed=n)
    f = lambda t: t.to(DEV, torch.float32).contiguous()
    Xd, yd, elld, nzd = f(X), f(y), f(ell), f(noise)
    ws = eng.Workspace(n, q, 1, torch.float32, DEV, True)

    def err():
        _, _, Kinv = _sweep_and_kinv(eng, ws, Xd, yd, elld, nzd, n, d, q, True)
        assert not bool(ws.info.any())
        # W[k][c] lives in the tiles with k // 128 >= c // 128 (the product of tile (ib, jb) starts at row 128 jb); the sweep never
        # writes the tiles above, and the workspace is not cleared
        blk = torch.arange(ws.n_pad) // 128
        W = ws.W.detach().cpu().double()
        W = torch.where(blk[:, None] >= blk[None, :], W, torch.zeros_like(W))
        want = W.transpose(1, 2) @ W
        got = Kinv.cpu().double()
        assert bool(torch.isfinite(got).all())
        return float(torch.triu(got - want).abs().max() / want.abs().max())

    e_split = err()
    with _hip.knob("PLMC_SPLIT", "0"):
        e_plain = err()
    print("n = %d: e_split %.3e  e_plain %.3e" % (n, e_split, e_plain))
    assert e_split < 2.0 * e_plain + 2e-6, (e_split, e_plain)


_B_N, _B_D, _B_Q = 2100, 4, 2


@pytest.fixture(scope="module")
def depth_problem():
    X, y, ell, noise, _ = _problem(_B_N, _B_D, _B_Q, seed=_B_N + 1)
    ref = gm.exact_latent_log_prob_analytic("matern", X, ell, noise, y, None, 2.5)
    return X, y, ell, noise, ref


@pytest.mark.parametrize("grp", [5, 6, 7, 8])
def test_updates_and_panels_at_every_depth_class(eng, depth_problem, grp):
    """Groups of 5 / 6 / 7 / 8 block rows at n = 2100: trailing updates and group panels 20 / 24 / 28 / 32 stages deep, four or
    three groups.  Both split schemes against the fp64 oracle with the tolerances and the factor-2 rule of
    test_split_engines_against_fp32_mfma_path (plain = PLMC_SPLIT=0 with the same groups)."""
    from projectedlmc import _hip
    X, y, ell, noise, ref = depth_problem
    f = lambda t: t.to(DEV, torch.float32)

    def run():
        ell_d, nz_d, y_d = f(ell).requires_grad_(), f(noise).requires_grad_(), f(y).requires_grad_()
        lp = eng.exact_latent_log_prob("matern52", f(X), ell_d, None, nz_d, y_d)
        lp.sum().backward()
        torch.cuda.synchronize()
        return [t.detach().cpu().double() for t in (lp, ell_d.grad, nz_d.grad, y_d.grad)]

    with _hip.knob("PLMC_GRP", str(grp)):
        with _hip.knob("PLMC_SPLIT", "2"):
            h2 = run()
        with _hip.knob("PLMC_SPLIT", "3"):
            b3 = run()
        with _hip.knob("PLMC_SPLIT", "0"):
            plain = run()
    for name, split in (("fp16x2", h2), ("bf16x3", b3)):
        for got, base, want, tol in ((split[0], plain[0], ref[0], 1e-4), (split[1], plain[1], ref[1], 2e-3),
                                     (split[2], plain[2], ref[2], 2e-3), (split[3], plain[3], ref[4], 2e-3)):
            scale = want.abs().max()
            e_split, e_plain = float((got - want).abs().max() / scale), float((base - want).abs().max() / scale)
            print("PLMC_GRP=%d %s: e_split %.3e  e_plain %.3e" % (grp, name, e_split, e_plain))
            assert bool(torch.isfinite(got).all())
            assert e_split < tol and e_plain < tol, (e_split, e_plain)
            assert e_split < 2.0 * e_plain + 2e-6, (e_split, e_plain)


def test_bits_do_not_move_under_memory_load(eng):
    """n = 2304, q = 2: sweep + K^-1 + gradient four times while a side stream copies a 1 GB buffer device to device in a loop
    (the DMA pieces of the ring land at other times), then once on the one-stream schedule (PLMC_SERIAL=1): the factor buffer,
    log det and gradients are the same bits in all five runs."""
    from projectedlmc import _hip
    n, d, q = 2304, 4, 2
    X, y, ell, noise, _ = _problem(n, d, q, seed=n)
    f = lambda t: t.to(DEV, torch.float32).contiguous()
    Xd, yd, elld, nzd = f(X), f(y), f(ell), f(noise)
    ws = eng.Workspace(n, q, 1, torch.float32, DEV, True)
    src = torch.empty(1 << 28, dtype=torch.float32, device=DEV)            # 1 GB
    dst = torch.empty_like(src)
    side = torch.cuda.Stream(device=DEV)

    def run(load):
        if load:
            with torch.cuda.stream(side):
                for _ in range(8):
                    dst.copy_(src, non_blocking=True)
        g, kd, _ = _sweep_and_kinv(eng, ws, Xd, yd, elld, nzd, n, d, q, False)
        torch.cuda.synchronize()
        return ws.A.view(torch.int32).clone(), ws.logdet.clone(), g.clone(), kd.view(torch.int32).clone()

    runs = [run(True) for _ in range(4)]
    with _hip.knob("PLMC_SERIAL", "1"):
        runs.append(run(False))
    A0, ld0, g0, kd0 = runs[0]
    assert not bool(ws.info.any()) and bool(torch.isfinite(ld0).all()) and bool(torch.isfinite(g0).all()) and float(g0.abs().max()) > 0
    for i, (A, ld, g, kd) in enumerate(runs[1:], 1):
        assert torch.equal(A, A0), "run %d: %d elements of the factor buffer differ" % (i, int((A != A0).sum()))
        assert torch.equal(ld, ld0) and torch.equal(g, g0) and torch.equal(kd, kd0), "run %d" % i
    side.synchronize()
