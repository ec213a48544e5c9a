"""The references and the bound of the reductions (tests/_reduce_ref.py) on their own, without a GPU.

  * a sum carried in fp64 and rounded once, formed from the NaN-laden buffers, is inside the bound at every shape
    tests/test_gpu_reductions.py runs;
  * the same sum carried in fp32 is outside it for most outputs -- the tolerances the suite had for these kernels (rtol 2e-3,
    2e-6 of the largest) let such a kernel pass;
  * four more seeded mistakes leave it: a row of the padding counted (the clamped row of the vector loads), the wrong augmented
    column, var H for var H^2, eps dropped.
"""
import pytest
import torch

import _reduce_ref as rr

F32, F64 = torch.float32, torch.float64


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_moments_carried_in_fp64_are_inside_the_bound(dtype):
    for n in rr.MOMENT_SIZES:
        for q in rr.QS:
            for ns in rr.MOMENT_NS:
                zV = rr.moment_inputs(n, q, ns, dtype)
                A = rr.moment_buffer(zV, dtype)
                n_pad = A.shape[1]
                assert A.shape[2] == rr.moment_lda_min(n_pad, ns, dtype) and bool(torch.isnan(A[:, :, :n_pad]).all())
                mean, vsq = rr.moment_cpu(A, n_pad, ns, dtype)
                rm, rv, mm, mv = rr.moment_reference(zV)
                assert not rr.violations(mean, rm, rr.bound(rm, mm, n_pad, dtype)), (n, q, ns)
                assert not rr.violations(vsq, rv, rr.bound(rv, mv, n_pad, dtype)), (n, q, ns)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_w_sums_carried_in_fp64_are_inside_the_bound(dtype):
    for n in rr.W_SIZES:
        for q in rr.QS:
            W, z = rr.w_inputs(n, q, dtype)
            ws = rr.w_buffer(n, q, dtype, W)
            assert ws.lda > ws.n_pad and bool(torch.isnan(ws.A[:, :, :ws.wcol0]).all())
            alpha, kd = rr.w_cpu(ws, z, dtype)
            ra, ma, rk = rr.w_reference(W, z)
            assert not rr.violations(alpha, ra, rr.bound(ra, ma, ws.n_pad, dtype)), (n, q)
            assert not rr.violations(kd, rk, rr.bound(rk, rk, ws.n_pad, dtype)), (n, q)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_mixing_carried_in_fp64_is_inside_the_bound(dtype):
    for q, ns, p in rr.MIX_CASES:
        for eps in rr.MIX_EPS:
            e = rr.mix_eps(eps, dtype)
            ml, vl, H = rr.mix_inputs(q, ns, p, dtype)
            mean, var = rr.mix_cpu(ml, vl, H, e, dtype)
            rm, rv, mm, mv = rr.mix_reference(ml, vl, H, e)
            assert not rr.violations(mean, rm, rr.bound(rm, mm, q, dtype)), (q, ns, p, eps)
            assert not rr.violations(var, rv, rr.bound(rv, mv, q, dtype)), (q, ns, p, eps)


def test_a_sum_carried_in_fp32_is_outside_the_bound_for_most_columns():
    """L = 384 terms of N(0,1) products: the fp32-carried sum is not the correctly rounded one"""
    n, q, ns = 300, 1, 37
    zV = rr.moment_inputs(n, q, ns, F32)
    A = rr.moment_buffer(zV, F32)
    rm, rv, mm, mv = rr.moment_reference(zV)
    mean, vsq = rr.moment_cpu(A, 384, ns, F32, carry=F32)
    bad = rr.outside(mean, rm, rr.bound(rm, mm, 384, F32))
    print("fp32-carried means outside the bound: %d of %d; |v|^2: %d" % (bad, ns, rr.outside(vsq, rv, rr.bound(rv, mv, 384, F32))))
    assert bad > ns // 2, bad
    # ... and is what the tolerance of the model-level test lets through
    assert torch.allclose(mean.double(), rm, rtol=2e-3, atol=0)
    W, z = rr.w_inputs(n, 3, F32)
    ws = rr.w_buffer(n, 3, F32, W)
    ra, ma, rk = rr.w_reference(W, z)
    alpha, kd = rr.w_cpu(ws, z, F32, carry=F32)
    bad = rr.outside(alpha, ra, rr.bound(ra, ma, 384, F32))
    assert bad > alpha.numel() // 2, bad
    assert float((alpha.double() - ra).abs().max()) <= 2e-6 * float(ra.abs().max())


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_seeded_mutations_leave_the_bound(dtype):
    n, q, ns = 300, 3, 37
    # the wrong augmented column
    zV = rr.moment_inputs(n, q, ns, dtype)
    A = rr.moment_buffer(zV, dtype)
    rm, rv, mm, mv = rr.moment_reference(zV)
    mean, vsq = rr.moment_cpu(A, 384, ns, dtype, mutate="wrong_column")
    assert rr.outside(mean, rm, rr.bound(rm, mm, 384, dtype)) > q * ns // 2
    assert rr.outside(vsq, rv, rr.bound(rv, mv, 384, dtype)) > q * ns // 2
    # a row of the padding counted
    W, z = rr.w_inputs(n, q, dtype)
    ws = rr.w_buffer(n, q, dtype, W)
    ra, ma, rk = rr.w_reference(W, z)
    alpha, kd = rr.w_cpu(ws, z, dtype, mutate="pad_row")
    assert rr.outside(alpha, ra, rr.bound(ra, ma, 384, dtype)) > alpha.numel() // 2
    assert rr.outside(kd, rk, rr.bound(rk, rk, 384, dtype)) > kd.numel() // 2
    # var H for var H^2, eps dropped
    qm, nsm, p = rr.MIX_CASES[1]
    e = rr.mix_eps(1e-3, dtype)
    ml, vl, H = rr.mix_inputs(qm, nsm, p, dtype)
    rmm, rvv, mmm, mvv = rr.mix_reference(ml, vl, H, e)
    for mutate in ("h_for_h2", "no_eps"):
        mean, var = rr.mix_cpu(ml, vl, H, e, dtype, mutate=mutate)
        assert not rr.violations(mean, rmm, rr.bound(rmm, mmm, qm, dtype))
        assert rr.outside(var, rvv, rr.bound(rvv, mvv, qm, dtype)) > var.numel() // 2, mutate


def test_nan_above_the_block_diagonal_reaches_a_sum_that_multiplies_by_zero():
    """why the tiles above the block diagonal must not be loaded: 0 * NaN is NaN"""
    n, q = 300, 1
    W, z = rr.w_inputs(n, q, F32)
    ws = rr.w_buffer(n, q, F32, W)
    Wr = ws.A[:, :, ws.wcol0:ws.wcol0 + ws.n_pad]
    alpha = (Wr * torch.tril(torch.ones(384, 384)) * z.to(F32)[:, :, None]).sum(1)
    assert bool(torch.isnan(alpha).any())
    assert not bool(torch.isnan(rr.w_cpu(ws, z, F32)[0]).any())
