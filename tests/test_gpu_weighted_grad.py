"""plmc_weighted_grad* alone, through the raw C ABI, against the dense fp64 reference of _weighted_grad_ref.py:
    G[l][t] = sum_{i <= j < N} c_ij (At_l^T Bt_l)_ij d Khat_l(Z)_ij / d theta_t,   c_ii = 1, c_ij = 2.
Every family form x {fp32, fp64}; N = n + n* with (n, n*) in {(200, 70), (128, 1), (1, 1), (127, 130)} -- one to three block rows, the
train / test boundary inside a tile and on a tile edge, a ragged last tile -- r in {2, n* + 2}, q in {1, 3}, d in {1, 3, 8} and one d > 8
per family that allows it; each family meets every shape, and the other sizes rotate over (family, shape).  NaN stands wherever the
contract says nothing is read; two calls return the same bits; a product that is not symmetric yields the upper-weighted sum; every
argument error is refused before a launch.

Tolerances.  S_t is the sum of absolute terms behind output t (reference).
  fp64: |G_t - ref_t| <= 1e-9 + 1e-7 S_t -- rtol / atol of the fp64 MLL-gradient parity tests (tests/test_gpu_engine.py), relative to S_t.
  fp32: |G_t - ref_t| <= kappa (r + d + 4) 2^-24 S_t.  kappa = the next power of two above twice the worst ratio measured over the cases
  of this file on the GPU against the fp64 reference (profiles/weighted_grad_accuracy.md), per shape class: 8 at N = 2, where an output
  is a single term (worst 2.48), 1/4 from N = 129 on, where it is a sum over the tile product (worst 9.4e-2).
  tests/test_weighted_grad_ref_host.py shows that at these kappa an operand rounded to fp16 and a dropped contraction row both fail, in
  either class."""
import functools

import pytest
import torch

import _posterior_dx_dense as pdd
import _weighted_grad_ref as wgr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FORMULA32 = 2.0            # a draw is taken where the reference's formula in IEEE float32 is within this many units of the bound
SHAPES = ((200, 70), (128, 1), (1, 1), (127, 130))
DS, QS = (1, 3, 8), (1, 3)
DTYPES = [torch.float64, torch.float32]
DT_IDS = ["f64", "f32"]


@pytest.fixture(scope="module")
def eng():
    import projectedlmc  # noqa: F401
    from projectedlmc import _engine, _hip
    assert torch.cuda.is_available()

    class E:
        exact, hip = _engine, _hip
    return E


def _family_d(family, d):
    """the d a family is given: the additive tables need their groups' dimensions, the sum's 3 d + 1 records stay small"""
    if family.startswith("add_"):
        return 3 if d < 8 else 5
    if family == "sum_single":                          # (one member: periodic, d <= 8)
        return d
    if family == "sm8":                                 # 2 x 8 x d table entries, one forward-mode pass each in the reference: d = 8 is sm1's and sm3's
        return min(d, 3)
    return d


def _cases():
    out = []
    for i, f in enumerate(wgr.FAMILIES):
        for j, (n, ns) in enumerate(SHAPES):
            out.append((f, n, ns, bool((i + j // 2) % 2), QS[(i + j) % 2], _family_d(f, DS[(i + j) % 3])))
    # d > 8 where the family allows it: the 16- and 32-dimension instantiations of the plain epilogue (and its spline form), rq, dot
    out += [("matern52", 200, 70, True, 1, 12), ("rbf", 127, 130, False, 3, 20), ("spline", 128, 1, True, 1, 12), ("matern32", 1, 1, True, 3, 32),
            ("rq", 200, 70, True, 1, 16), ("poly2", 127, 130, True, 1, 11)]
    return out


CASES = _cases()
CASE_IDS = ["%s-n%d-ns%d-%s-q%d-d%d" % (f, n, ns, "full" if full else "r2", q, d) for f, n, ns, full, q, d in CASES]


@functools.lru_cache(maxsize=None)
def _reference(case, symmetric=True):
    """problem, inputs, operands and (G, S) of one case, computed once and shared by the element types.  At N = 2, and there only, the
    inputs are the first draw (seed, seed + 1000, ...) at which the reference's own formula, evaluated in IEEE float32 on the host, stays
    within FORMULA32 units of the bound (_weighted_grad_ref.formula_in_float32): an output is then a single term, S_t is its magnitude,
    and a draw at which a factor of the derivative nearly vanishes tests the conditioning of sin or of a difference in float32, not the
    kernel.  Every larger shape takes its one draw as it comes."""
    family, n, ns, full, q, d = case
    seed0 = 100 + CASES.index(case) if case in CASES else 7
    r = ns + 2 if full else 2
    for seed in range(seed0, seed0 + 200000, 1000):
        p = wgr.problem(family, d, q, seed)
        Z = torch.cat([pdd.igd.inputs(n, d, seed), pdd.query_points(ns, d, seed)])
        if family.startswith("sum_"):
            Z = 3.0 * Z
        noise = (0.05 + 0.2 * torch.rand(q, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)).float().double()
        At, Bt = wgr.random_operands(r, n + ns, q, seed, symmetric=symmetric)
        G, S = wgr.weighted_grad_ref(p.kind, p.ell, p.oscale, noise, Z, At, Bt)
        G, S = wgr.flat_table(G), wgr.flat_table(S)
        if n + ns > 2:
            return p, Z, noise, At, Bt, G, S
        e32 = (wgr.formula_in_float32(p.kind, p.ell, p.oscale, noise, Z, At, Bt) - G).abs()
        if bool((e32 <= FORMULA32 * (r + d + 4) * 2.0 ** -24 * S).all()):
            return p, Z, noise, At, Bt, G, S
    raise AssertionError("no well-conditioned draw for %r" % (case,))


def _call(eng, p, Z, At, Bt, dt, ld_extra=8, stride_extra=1):
    """one library call on NaN-guarded buffers -> the gradient table (q, width) on the host"""
    ex, hip = eng.exact, eng.hip
    L = hip.lib()
    q, r, N = At.shape
    A, B, r_pad, N_pad = wgr.padded(At, Bt, dt, ld_extra=ld_extra, stride_extra=stride_extra)
    A, B = A.to(DEV), B.to(DEV)
    Zb = torch.full((N + 3, Z.shape[1]), float("nan"), dtype=dt)                     # rows >= N are not read
    Zb[:N] = Z.to(dt)
    Zb = Zb.to(DEV)
    ell = p.ell.to(DEV, dt).contiguous()
    osc = None if p.oscale is None else p.oscale.to(DEV, dt).contiguous()
    table = torch.full((q, ex.grad_table_width(ell, p.kind)), float("nan"), dtype=torch.float64, device=DEV)
    partials = ex._grad_partials(L, N_pad, q, ell, p.kind, dt, DEV)
    ex._kernel_call(L, "plmc_weighted_grad", dt, (ex.kind_code(p.kind), hip.ptr(A), hip.ptr(B), r_pad, N_pad, A.stride(1), A.stride(0),
                    hip.ptr(Zb), N, Z.shape[1]), ell, (hip.ptr(osc), hip.ptr(table), hip.ptr(partials), q, hip.stream_ptr(DEV)))
    torch.cuda.synchronize()
    return table.cpu()


def _check(got, want, S, r, d, dt, what, N):
    width = want.shape[1]                                                            # (a table without output scales: the library's slots for them stay out)
    got = got[:, :width]
    assert torch.isfinite(got).all(), (what, got)
    err = (got - want).abs()
    if dt == torch.float64:
        bound = 1e-9 + 1e-7 * S
        worst = float((err / bound).max())
        print("weighted_grad %s f64: worst |err| / (1e-9 + 1e-7 S) = %.3e" % (what, worst))
    else:
        unit = (r + d + 4) * 2.0 ** -24 * S
        ratio = torch.where(unit > 0, err / unit.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
        print("weighted_grad %s f32: worst |err| / ((r + d + 4) 2^-24 S) = %.4e   (r = %d, d = %d)" % (what, float(ratio.max()), r, d))
        bound = wgr.kappa(N) * unit
    assert bool((err <= bound).all()), (what, float((err - bound).max()))


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_every_family_form_matches_the_reference(eng, case, dt):
    p, Z, noise, At, Bt, G, S = _reference(case)
    got = _call(eng, p, Z, At, Bt, dt)
    _check(got, G, S, At.shape[1], Z.shape[1], dt, CASE_IDS[CASES.index(case)], Z.shape[0])
    again = _call(eng, p, Z, At, Bt, dt)                                             # fixed-order reductions: the same bits
    assert torch.equal(got, again)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", [("matern52", 200, 70, True, 3, 3), ("poly2", 127, 130, False, 1, 8), ("sm3", 128, 1, True, 1, 3)],
                         ids=["matern52", "poly2", "sm3"])
def test_a_product_that_is_not_symmetric_yields_the_upper_weighted_sum(eng, case, dt):
    p, Z, noise, At, Bt, G, S = _reference(case, symmetric=False)
    _check(_call(eng, p, Z, At, Bt, dt), G, S, At.shape[1], Z.shape[1], dt, "non-symmetric " + case[0], Z.shape[0])


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_tight_buffers_give_the_same_bits_as_guarded_ones(eng, dt):
    """ld = N_pad and no slack behind a latent: what the NaN guards surround is all that is read"""
    p, Z, noise, At, Bt, G, S = _reference(("matern52", 200, 70, True, 3, 3))
    assert torch.equal(_call(eng, p, Z, At, Bt, dt), _call(eng, p, Z, At, Bt, dt, ld_extra=0, stride_extra=0))


def test_bad_arguments_fail_before_any_launch(eng):
    hip = eng.hip
    L = hip.lib()
    dt = torch.float64
    t = torch.ones(256 * 256, dtype=dt, device=DEV)
    g = torch.full((8,), 7.0, dtype=torch.float64, device=DEV)
    st = hip.stream_ptr(DEV)
    # kind, At, Bt, r_pad, N_pad, ld, stride, Z, N, d, ell, oscale, grad, partials, q, stream
    ok = (0, hip.ptr(t), hip.ptr(t), 16, 128, 128, 16 * 128, hip.ptr(t), 100, 2, hip.ptr(t), None, hip.ptr(g), hip.ptr(t), 1, st)

    def bad(i, v, match, base="plmc_weighted_grad", args=ok):
        a = list(args)
        a[i] = v
        with pytest.raises(RuntimeError, match=match or None):
            L.call(base, dt, *a)

    for i in (1, 2, 7, 10, 12, 13):
        bad(i, None, "null pointer")
    bad(8, 0, "N > 0")
    bad(8, -3, "N > 0")
    bad(8, 129, "N_pad")
    bad(3, 24, "r_pad")
    bad(3, 0, "r_pad")
    bad(4, 192, "N_pad")
    bad(5, 64, "ld must be at least N_pad")
    bad(9, 33, "plmc_max_dim")
    bad(0, 9, "unknown kernel kind")
    bad(1, hip._c.c_void_p(t.data_ptr() + 8), "unaligned")
    bad(14, 0, "q>0")
    # the family forms: components, mixtures, dimensions and power beyond the family's limits
    cd = L.cdll
    i32 = (hip._c.c_int * 2)(0, 16)
    add = (0, hip.ptr(t), hip.ptr(t), 16, 128, 128, 16 * 128, hip.ptr(t), 100, 2, 2, hip.ptr(t), None, hip.ptr(g), hip.ptr(t), 1, st)
    bad(10, cd.plmc_max_components() + 1, "", "plmc_weighted_grad_add", add)
    sm = (hip.ptr(t), hip.ptr(t), 16, 128, 128, 16 * 128, hip.ptr(t), 100, 2, 2, hip.ptr(t), hip.ptr(t), None, hip.ptr(g), hip.ptr(t), 1, st)
    bad(9, cd.plmc_sm_max_mixtures() + 1, "", "plmc_weighted_grad_sm", sm)
    bad(8, cd.plmc_sm_max_dim() + 1, "", "plmc_weighted_grad_sm", sm)
    per = (hip.ptr(t), hip.ptr(t), 16, 128, 128, 16 * 128, hip.ptr(t), 100, 2, hip.ptr(t), hip.ptr(t), None, hip.ptr(g), hip.ptr(t), 1, st)
    bad(8, cd.plmc_per_max_dim() + 1, "", "plmc_weighted_grad_per", per)
    bad(8, cd.plmc_rq_max_dim() + 1, "", "plmc_weighted_grad_rq", per)
    lper = per[:11] + (hip.ptr(t),) + per[11:]
    bad(8, cd.plmc_lper_max_dim() + 1, "", "plmc_weighted_grad_lper", lper)
    dot = (hip.ptr(t), hip.ptr(t), 16, 128, 128, 16 * 128, hip.ptr(t), 100, 2, hip.ptr(t), hip.ptr(t), 2, None, hip.ptr(g), hip.ptr(t), 1, st)
    bad(11, cd.plmc_dot_max_power() + 1, "", "plmc_weighted_grad_dot", dot)
    bad(8, cd.plmc_dot_max_dim() + 1, "", "plmc_weighted_grad_dot", dot)
    sm_ = (hip.ptr(t), hip.ptr(t), 16, 128, 128, 16 * 128, hip.ptr(t), 100, 2, 2, hip._c.addressof(i32), hip.ptr(t), hip.ptr(t), hip.ptr(g),
           hip.ptr(t), 1, st)
    bad(9, cd.plmc_sum_max_components() + 1, "", "plmc_weighted_grad_sum", sm_)
    bad(8, cd.plmc_sum_max_dim() + 1, "", "plmc_weighted_grad_sum", sm_)
    torch.cuda.synchronize()
    assert bool((g == 7.0).all())                                                    # nothing was launched: the table is untouched
    L.call("plmc_weighted_grad", dt, *ok)                                            # and the well-formed call goes through
    torch.cuda.synchronize()
    assert bool((g[:4] != 7.0).all()) and bool((g[4:] == 7.0).all())
