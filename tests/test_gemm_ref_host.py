"""The reference and the bound of the TN tile product (tests/_gemm_ref.py) on their own, without a GPU.

  * a torch-CPU product in the element type, formed from the NaN-laden operands through a select, stays inside the bound at every
    shape x tri x mode x batch x dtype tests/test_gpu_gemm_tn.py runs;
  * eight seeded mistakes a kernel could make leave it on more than one tile's worth of elements: each of A_LOWER, B_LOWER, A_UPPER
    ignored, k_lo one slab late, k_hi one block early, mode 2 applied as mode 1, A used untransposed, the tiles C_LOWER skips
    computed instead of left.  For these the declared-zero blocks hold finite garbage, so a mistake shows as an error, not as NaN;
  * why the mask must be a select: 0 * NaN reaches C.
"""
import pytest
import torch

import _gemm_ref as gr

F32, F64 = torch.float32, torch.float64


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", gr.SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_cpu_product_in_the_element_type_is_inside_the_bound(dtype, shape):
    M, N, K = shape
    worst = {}
    for batch in gr.BATCH:
        for tri in gr.TRIS:
            A, B, C0 = gr.make_inputs(M, N, K, batch, tri, dtype)
            for mode in gr.valid_modes(tri):
                C = gr.cpu_product(A, B, C0, mode, tri, dtype)
                assert not bool(torch.isnan(C).any()), (shape, batch, tri, mode)
                Cref, bnd = gr.reference(A, B, C0, mode, tri), gr.bound(A, B, C0, mode, tri, dtype)
                bad = gr.violations(C, Cref, bnd)
                assert not bad, (shape, batch, gr.tri_name(tri), mode, bad)
                worst[mode] = max(worst.get(mode, 0.0), gr.worst_ratio(C, Cref, bnd)[0])
    print("cpu product, largest error / bound per mode:", shape, {m: "%.3f" % v for m, v in worst.items()})


CASES = {
    # mutation: (shape, tri, mode)
    "ignore_a_lower": ((384, 384, 384), gr.AL, 0),
    "ignore_b_lower": ((384, 384, 384), gr.BL, 0),
    "ignore_a_upper": ((384, 384, 384), gr.AU, 0),
    "k_lo_late": ((384, 384, 384), gr.AL, 0),
    "k_hi_early": ((384, 256, 144), gr.AU, 1),
    "sub_as_add": ((256, 384, 400), 0, 2),
    "untransposed": ((384, 384, 384), 0, 0),
    "c_lower_computed": ((384, 384, 384), gr.CL, 0),
}


def test_every_mutation_has_a_case():
    assert set(CASES) == set(gr.MUTATIONS)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("mutate", gr.MUTATIONS)
def test_seeded_mutations_leave_the_bound(dtype, mutate):
    (M, N, K), tri, mode = CASES[mutate]
    A, B, C0 = gr.make_inputs(M, N, K, 3, tri, dtype, garbage=True)   # finite in the declared-zero blocks
    assert bool(torch.isfinite(A).all()) and bool(torch.isfinite(B).all())
    Cref, bnd = gr.reference(A, B, C0, mode, tri), gr.bound(A, B, C0, mode, tri, dtype)
    assert not gr.violations(gr.cpu_product(A, B, C0, mode, tri, dtype), Cref, bnd)
    bad = gr.outside(gr.cpu_product(A, B, C0, mode, tri, dtype, mutate=mutate), Cref, bnd)
    print(mutate, "elements outside the bound:", bad, "of", 3 * M * N)
    assert bad > gr.NB * gr.NB, (mutate, bad)                         # more than one tile's worth


def test_nan_in_a_declared_zero_block_reaches_a_product_that_multiplies_by_zero():
    """why the mask has to be a select: 0 * NaN is NaN"""
    M, N, K = 384, 256, 144
    A, B, C0 = gr.make_inputs(M, N, K, 1, gr.AL, F32)
    zA, _ = gr.zero_masks(M, N, K, gr.AL)
    assert bool(torch.isnan(A[:, zA]).all()) and not bool(torch.isnan(A[:, ~zA]).any())
    C = (A.to(F32) * (~zA).to(F32)).transpose(1, 2) @ B.to(F32)
    assert bool(torch.isnan(C).any())
    assert not bool(torch.isnan(gr.cpu_product(A, B, C0, 0, gr.AL, F32)).any())


def test_embed_lays_the_operand_at_its_offset_and_fills_the_gap():
    t = torch.arange(2 * 3 * 4, dtype=F64).reshape(2, 3, 4)
    buf = gr.embed(t, 8, 4, float("nan"))
    assert buf.shape == (2, 3, 8) and torch.equal(buf[:, :, 4:], t) and bool(torch.isnan(buf[:, :, :4]).all())
    buf = gr.embed(t, 9, 2, gr.SENTINEL)
    assert torch.equal(buf[:, :, 2:6], t) and bool((buf[:, :, :2] == gr.SENTINEL).all()) and bool((buf[:, :, 6:] == gr.SENTINEL).all())
