"""The border formulas of plmc_factor_extend (tests/_factor_extend_ref.py) without the library: restated in the element type with the
Schur block in fp64, starting from the element-type LAPACK factor of the leading n x n block and laid into the buffer the way the call
leaves it, they pass every assertion the sweep is held to (tests/_factor_ref.py: structure, measures, log det, thresholds untouched) for
Case(family, n + m, ...) at every shape of tests/test_gpu_factor_extend.py; four seeded mutations each fail them."""
import pytest
import torch

import _factor_extend_ref as fx
import _factor_ref as fr

DTYPES = [torch.float32, torch.float64]
FAMILIES = [("wishart", 3), ("graded", 3), ("kernel", 2)]
_cases = {}


def _case(family, n, q, dtype):
    key = (family, n, q, dtype)
    if key not in _cases:
        _cases[key] = fr.Case(family, n, q, dtype)
    return _cases[key]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("family,q", FAMILIES, ids=[f for f, _ in FAMILIES])
@pytest.mark.parametrize("n,m", fx.SHAPES, ids=["%d+%d" % s for s in fx.SHAPES])
def test_border_formulas_in_the_buffer_layout_pass_every_assertion(n, m, family, q, dtype):
    case = _case(family, n + m, q, dtype)
    ws = fx.extended_workspace(case, n)
    bad, meas, _ = fr.check_sweep(case, ws, None)
    thr = fr.plain_thresholds(case, case.__dict__["_ref_meas"][None], list(meas))
    print(family, n, m, {k: "%.2f" % float((meas[k] / thr[k]).max()) for k in meas})
    assert not bad, bad
    assert set(meas) == {"rho_U", "e_U", "rho_W", "e_W"}


def test_source_workspace_is_a_finished_sweep_of_the_leading_block():
    """what the GPU test hands to the call: the leading block's factor passes the sweep's assertions on its own"""
    big = _case("graded", 250 + 10, 3, torch.float32)
    lead = fr.Case("graded", 250, 3, torch.float32)
    lead.K = big.K[:, :250, :250].clone()
    ev = torch.linalg.eigvalsh(lead.K)
    lead.kappa = ev[:, -1] / ev[:, 0]
    ws = fx.source_workspace(big, 250, 128)
    bad, _, _ = fr.check_sweep(lead, ws, None)
    assert not bad, bad


def _caught(bad):
    """a mutation counts as caught by a residual 10 x above its threshold, a tile-wise e above its bound, or an exact property"""
    for v in bad:
        if isinstance(v, str):
            return True
        name, _, value, thr = v
        if name.startswith("e_") or value >= 10.0 * thr:
            return True
    return False


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("which", fx.MUTATIONS)
def test_seeded_mutation_of_the_border_fails_the_assertions(which, dtype):
    case = _case("graded", 250 + 10, 3, dtype)
    ws = fx.extended_workspace(case, 250, mutation=which)
    bad, meas, _ = fr.check_sweep(case, ws, None, logdet=False)
    assert _caught(bad), (which, bad, meas)
