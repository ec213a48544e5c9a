"""plmc_rff_matvec_dx (csrc/cross_matvec_dx.hip), the input derivative of the prior part of a pathwise posterior draw, against the fp64 sum
of tests/_cross_matvec_dx_ref.py, whose sines are accurate at any phase.  d in {1, 4, 9}, m in {1, 64, 65, 300} (one feature; a staged
chunk; one more; two segments, split over workgroups where the test points are few), n* in {1, 65}, phases from 0 up to about 10^4
revolutions -- test point 0 is (1, ..., 1), where the last feature stands at 10^4.  Per element
    |Jx - exact| <= |scale| 2 pi [4 (d + 2) u sum_j |f_jk| |w_sj| + (m + 4) 2^-53 sum_j |sin_j f_jk w_sj|],
one sine within 4 (d + 2) u as derived in DESIGN.md 7.13: the bound does not grow with the phase."""
import pytest
import torch

import _cross_matvec_dx_ref as cdx
import _cross_matvec_ref as cm

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MAX_REV = 1.0e4


@pytest.fixture(scope="module")
def eng():
    from projectedlmc import _engine
    assert torch.cuda.is_available()
    return _engine


def _problem(d, m, ns, q=2, r=3):
    seed = 100 * d + m + ns
    freq, phase, Wt, scale = cm.rff_problem(d, m, q, r, seed, MAX_REV)
    _, Xs = cm.inputs("rbf", 2, ns, d, seed)
    Xs[0] = 1.0
    G = cdx.operands(2, ns, r, q, seed)[1]
    return freq, phase, Wt, scale, Xs, G


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("ns", [1, 65])
@pytest.mark.parametrize("m", [1, 64, 65, 300])
@pytest.mark.parametrize("d", [1, 4, 9])
def test_feature_derivative_against_fp64_within_the_derived_bound(eng, d, m, ns, dt):
    freq, phase, Wt, scale, Xs, G = _problem(d, m, ns)
    assert float((freq[:, -1] * Xs[0]).sum(-1).max()) >= MAX_REV - 1.0
    exact, bound = cdx.rff_reference(freq, phase, Xs, Wt, G, scale, dt)
    f = lambda t: t.to(DEV, dt)
    got = eng.rff_matvec_dx(f(freq), f(phase), f(Xs), f(Wt), f(G), f(scale))
    again = eng.rff_matvec_dx(f(freq), f(phase), f(Xs), f(Wt), f(G), f(scale))
    torch.cuda.synchronize()
    assert got.shape == exact.shape and got.dtype == torch.float64
    assert bool(torch.isfinite(got).all())
    print("d=%d m=%d ns=%d %s: largest share of the bound %.3f" % (d, m, ns, dt, cm.worst_share(got.cpu(), exact, bound)))
    assert cdx.rff_violations(got.cpu(), exact, bound) == 0
    assert torch.equal(got, again)
    assert (eng._hip.lib().cdll.plmc_cross_matvec_dx_splits(m, ns, 2) > 1) == (m == 300)


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["float64", "float32"])
def test_one_column_without_g_no_scale_and_wide_weights_in_chunks(eng, dt):
    freq, phase, Wt, scale, Xs, G = _problem(4, 65, 65)
    f = lambda t: t.to(DEV, dt)
    exact, bound = cdx.rff_reference(freq, phase, Xs, Wt[:, :, 1:2], None, None, dt)
    got = eng.rff_matvec_dx(f(freq), f(phase), f(Xs), f(Wt[:, :, 1:2])).cpu()         # G None: the Jacobian of one column; scale None: 1
    assert cdx.rff_violations(got, exact, bound) == 0
    Wt19, G19 = cm.columns(65, 19, 2, 5), cdx.operands(2, 65, 19, 2, 5)[1]
    exact, bound = cdx.rff_reference(freq, phase, Xs, Wt19, G19, scale, dt)
    got = eng.rff_matvec_dx(f(freq), f(phase), f(Xs), f(Wt19), f(G19), f(scale)).cpu()
    assert got.shape == (2, 65, 4) and cdx.rff_violations(got, exact, bound) == 0


def test_an_element_does_not_depend_on_the_split_or_on_its_neighbours(eng):
    freq, phase, Wt, scale, Xs, G = _problem(4, 300, 1)
    g = torch.Generator().manual_seed(2)
    many = torch.cat([Xs, (2 * torch.rand(65600, 4, generator=g, dtype=torch.float64) - 1).float().double()])
    Gmany = torch.cat([G, torch.randn(2, 65600, 3, generator=g, dtype=torch.float64).float().double()], 1)
    f = lambda t: t.to(DEV, torch.float32)
    L = eng._hip.lib().cdll
    assert L.plmc_cross_matvec_dx_splits(300, 1, 2) > 1 and L.plmc_cross_matvec_dx_splits(300, 65601, 2) == 1
    one = eng.rff_matvec_dx(f(freq), f(phase), f(Xs), f(Wt), f(G), f(scale))
    all_ = eng.rff_matvec_dx(f(freq), f(phase), f(many), f(Wt), f(Gmany), f(scale))
    assert torch.equal(one[:, 0], all_[:, 0])
