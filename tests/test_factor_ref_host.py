"""The checks of tests/test_gpu_factor.py without the library (tests/_factor_ref.py): a CPU LAPACK factorisation of the
element type, laid into the buffer the way the sweep leaves it, passes every assertion; five seeded mutations of that buffer
each fail them; and the non-positive-definite construction fails at the pivot it names."""
import pytest
import torch

import _factor_ref as fr

DTYPES = [torch.float32, torch.float64]
_cases = {}


def _case(family, n, dtype):
    key = (family, n, dtype)
    if key not in _cases:
        _cases[key] = fr.Case(family, n, 3, dtype)
    return _cases[key]


def _fake_sweep(case, naug, with_inverse=True):
    ws = fr.HostWorkspace(case.n, case.q, naug, case.dtype, with_inverse)
    rhs = case.rhs(naug) if naug > 0 else None
    fr.fill_buffer(ws, case.K, rhs)
    lap = case.lapack()
    fr.write_factor(ws, lap["U"], lap["W"], case.z_lapack(rhs) if naug > 0 else None)
    return ws, rhs


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("family,n", [("wishart", 200), ("graded", 200), ("kernel", 200), ("graded", 384), ("graded", 1100)])
def test_cpu_lapack_in_the_buffer_layout_passes_every_assertion(family, n, dtype):
    """the inputs are within the conditions for the reference alone; also: kappa_2 <= 100 and eig_lo a true bound (asserted
    where the matrices are made), fill_buffer's NaN canaries survive where the contracts say so"""
    case = _case(family, n, dtype)
    for naug, wi in ((130, True), (1, True), (0, False)):
        ws, rhs = _fake_sweep(case, naug, wi)
        bad, meas, _ = fr.check_sweep(case, ws, rhs)
        assert not bad, (naug, wi, bad)
        assert set(meas) == {"rho_U", "e_U"} | ({"rho_W", "e_W"} if wi else set()) | ({"rho_Z", "e_Z"} if naug else set())
    if family == "graded":
        assert float(torch.diagonal(case.K[0]).max()) < 1.0 and float(torch.diagonal(case.K[2]).min()) > 100.0


def _caught(bad):
    """a mutation counts as caught by a residual 10 x above its threshold, a tile-wise e above its bound, or an exact property"""
    for v in bad:
        if isinstance(v, str):
            return True
        name, _, value, thr = v
        if name.startswith("e_") or value >= 10.0 * thr:
            return True
    return False


def _mutations(ws):
    """name -> function that mutates the buffer of a finished (fake) sweep in place; n = 1100: m = 9, 52 padded rows"""
    n_pad, w0, a0 = ws.n_pad, ws.wcol0, ws.n_pad
    A = ws.A

    def scale_u_tile():
        A[1, 256:384, 640:768] *= 1.0 + 2.0 ** -11

    def w_tile_from_neighbour():
        A[1, 512:640, w0 + 128:w0 + 256] = A[2, 512:640, w0 + 128:w0 + 256]

    def transpose_sub_block():
        A[0, 384 + 16:384 + 32, 384 + 48:384 + 64] = A[0, 384 + 16:384 + 32, 384 + 48:384 + 64].transpose(0, 1).clone()

    def zero_last_padded_row():
        A[2, n_pad - 1, :n_pad] = 0

    def shift_aug_column():
        A[0, :, a0 + 77] = torch.roll(A[0, :, a0 + 77], 1)

    return dict(scale_u_tile=scale_u_tile, w_tile_from_neighbour=w_tile_from_neighbour, transpose_sub_block=transpose_sub_block,
                zero_last_padded_row=zero_last_padded_row, shift_aug_column=shift_aug_column)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("which", ["scale_u_tile", "w_tile_from_neighbour", "transpose_sub_block", "zero_last_padded_row",
                                   "shift_aug_column"])
def test_seeded_mutation_fails_the_assertions(which, dtype):
    case = _case("graded", 1100, dtype)
    ws, rhs = _fake_sweep(case, 130)
    before = ws.A.clone()
    _mutations(ws)[which]()
    assert not torch.equal(torch.nan_to_num(ws.A), torch.nan_to_num(before))
    # (log det and info are the fake sweep's own: the mutation has to be seen in what was written)
    bad, meas, tiles = fr.check_sweep(case, ws, rhs, logdet=False)
    assert _caught(bad), (which, bad, meas)
    if which == "scale_u_tile":
        hit = [v for v in bad if not isinstance(v, str) and v[0] == "e_U" and v[1] == 1]
        assert hit and tiles["e_U"][1] == (2, 5), (bad, tiles)          # the bad tile is named


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_non_pd_construction_fails_at_the_pivot_it_names(dtype):
    case = _case("graded", 1100, dtype)
    for k in (5, 48, 127, 130, 1030, case.n - 1):
        K = fr.nonpd_matrix(case, 1, k)
        assert torch.equal(K[0], case.K[0]) and torch.equal(K[2], case.K[2])
        _, info = torch.linalg.cholesky_ex(K.to(dtype))
        assert info.tolist() == [0, k + 1, 0], (k, info.tolist())
