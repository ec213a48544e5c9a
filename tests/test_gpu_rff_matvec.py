"""plmc_rff_matvec (csrc/cross_matvec.hip), the prior part of a pathwise posterior draw: the cosine sum over m random Fourier features
against the fp64 sum of tests/_cross_matvec_ref.py, whose features are accurate at any phase.  d in {1, 3, 8} (and 32, the largest
capacity), m in {1, 100, 1030} (one feature; less than a segment; five segments, split over workgroups), n* in {1, 130}, phases from 0 up
to about 2000 revolutions -- test point 0 is (1, ..., 1), where the last feature stands at 2000.  Per element
    |Out - exact| <= |scale| sum_j 4 (d + 2) u |Wt_jc| + u |exact| + (m + 4) 2^-53 |scale| sum_j |cos_j Wt_jc|,
the bound of one cosine derived in DESIGN.md 7.12: it does not grow with the phase."""
import pytest
import torch

import _cross_matvec_ref as cm

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MAX_REV = 2000.0


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
    return freq, phase, Wt, scale, Xs


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("ns", [1, 130])
@pytest.mark.parametrize("m", [1, 100, 1030])
@pytest.mark.parametrize("d", [1, 3, 8, 32])
def test_feature_sum_against_fp64_within_the_derived_bound(eng, d, m, ns, dt):
    freq, phase, Wt, scale, Xs = _problem(d, m, ns)
    assert float((freq[:, -1] * Xs[0]).sum(-1).max()) >= MAX_REV - 1.0
    exact, bound = cm.rff_reference(freq, phase, Xs, Wt, scale, dt)
    f = lambda t: t.to(DEV, dt)
    got = eng.rff_matvec(f(freq), f(phase), f(Xs), f(Wt), f(scale))
    again = eng.rff_matvec(f(freq), f(phase), f(Xs), f(Wt), f(scale))
    torch.cuda.synchronize()
    assert got.shape == exact.shape and got.dtype == dt
    print("d=%d m=%d ns=%d %s: largest share of the bound %.3f" % (d, m, ns, dt, cm.worst_share(got.cpu(), exact, bound)))
    assert cm.violations(got.cpu(), exact, bound) == 0
    assert torch.equal(got, again)
    assert (eng.cross_matvec_splits(m, ns, 2) > 1) == (m == 1030)


def test_no_scale_means_one_and_wide_weights_go_in_chunks(eng):
    freq, phase, _, _, Xs = _problem(3, 100, 130)
    Wt = cm.columns(100, 19, 2, 5)
    exact, bound = cm.rff_reference(freq, phase, Xs, Wt, None, torch.float32)
    f = lambda t: t.to(DEV, torch.float32)
    got = eng.rff_matvec(f(freq), f(phase), f(Xs), f(Wt)).cpu()
    assert got.shape == (2, 130, 19) and cm.violations(got, exact, bound) == 0


def test_an_element_does_not_depend_on_the_split_or_on_its_neighbours(eng):
    freq, phase, Wt, scale, Xs = _problem(3, 1030, 1)
    g = torch.Generator().manual_seed(2)
    many = torch.cat([Xs, (2 * torch.rand(65600, 3, generator=g, dtype=torch.float64) - 1).float().double()])
    f = lambda t: t.to(DEV, torch.float32)
    assert eng.cross_matvec_splits(1030, 1, 2) > 1 and eng.cross_matvec_splits(1030, 65601, 2) == 1
    one = eng.rff_matvec(f(freq), f(phase), f(Xs), f(Wt), f(scale))
    all_ = eng.rff_matvec(f(freq), f(phase), f(many), f(Wt), f(scale))
    assert torch.equal(one[:, 0], all_[:, 0])
