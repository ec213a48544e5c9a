"""CPU tests of projectedlmc._pivot: the one reader of the sweep's `info` words and the one jitter ladder (gpytorch's
psd_safe_cholesky [gpytorch-knowledge]), driven with fabricated host tensors and a fake attempt function -- no GPU, no
library call.  The chain-abort code is only ever fabricated here: nobody provokes one on a device."""
import types
import warnings

import pytest
import torch

from projectedlmc import _pivot, settings

WARN_FMT = "A not p.d., added jitter of %.1e to the diagonal"


def _check(*info):
    """An eager PivotCheck over a fabricated host `info`."""
    return _pivot.PivotCheck.eager(types.SimpleNamespace(info=torch.tensor(info, dtype=torch.int32)))


def _walk(dtype, infos):
    """Walk the ladder after a failed first attempt [7, 0]; attempt i sees infos[i].  -> (jitters tried, warnings, outcome)."""
    first = _check(7, 0)
    assert first.failed() and first.first_bad == [7, 0]
    tried = []

    def attempt(jit):
        tried.append(jit)
        return _check(*infos[len(tried) - 1]), "result %d" % len(tried)

    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        try:
            out = _pivot.walk(dtype, first, attempt)
        except RuntimeError as exc:
            out = exc
    assert all(issubclass(w.category, RuntimeWarning) for w in rec)
    return tried, [str(w.message) for w in rec], out


@pytest.mark.parametrize("dtype,base", [(torch.float32, 1e-6), (torch.float64, 1e-8)])
def test_ladder_rungs_warnings_and_result(dtype, base):
    tried, warned, out = _walk(dtype, [(3, 0), (0, 5), (0, 0)])
    assert tried == [base * 10 ** i for i in range(3)]
    assert warned == [WARN_FMT % j for j in tried]
    assert out == (tried[-1], "result 3")
    tried, warned, out = _walk(dtype, [(0, 0)])                      # the first rung passes: one warning, one attempt
    assert tried == [base] and warned == [WARN_FMT % base] and out == (base, "result 1")


def test_ladder_honours_max_tries_and_jitter_settings():
    with settings.cholesky_max_tries(5), settings.cholesky_jitter(1e-4, 1e-7):
        tried, warned, out = _walk(torch.float32, [(1, 1)] * 4 + [(0, 0)])
        assert tried == [1e-4 * 10 ** i for i in range(5)] and out == (tried[-1], "result 5")
        tried, _, out = _walk(torch.float64, [(1, 1)] * 4 + [(0, 0)])
        assert tried == [1e-7 * 10 ** i for i in range(5)] and out == (tried[-1], "result 5")
    assert settings.cholesky_max_tries.value() == 3


def test_ladder_exhausted_raises_the_final_text_with_the_pivot_list():
    tried, warned, out = _walk(torch.float32, [(3, 0), (0, 5), (0, 129)])          # default cholesky_max_tries = 3
    assert len(tried) == 3 and len(warned) == 3
    assert isinstance(out, RuntimeError)
    assert str(out) == ("Matrix not positive definite after repeatedly adding jitter up to 1.0e-04 "
                        "(first failing pivot per latent: [0, 129])")
    with settings.cholesky_max_tries(1):
        tried, warned, out = _walk(torch.float64, [(2, 2)])
    assert warned == [WARN_FMT % 1e-8]
    assert str(out) == ("Matrix not positive definite after repeatedly adding jitter up to 1.0e-08 "
                        "(first failing pivot per latent: [2, 2])")


def test_ladder_takes_the_pivot_list_of_a_deferred_context():
    """ProjectedLMCmll's attempts return the deferred_pivot_checks context of a whole forward pass: `first_bad` is its list."""
    def attempt(jit):
        with _pivot.deferred_pivot_checks(jit) as dc:
            assert _pivot.deferred_pivot_checks.current.jitter == jit
            dc.pending.append(_check(0, 0))
            dc.pending.append(_check(0, 41))
        return dc, None

    with settings.cholesky_max_tries(2), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(RuntimeError, match=r"up to 1\.0e-05 \(first failing pivot per latent: \[0, 41\]\)"):
            _pivot.walk(torch.float32, _check(1, 0), attempt)


def test_pivot_check_reads_info():
    ok, bad = _check(0, 0, 0), _check(0, 17, 3)
    assert ok.failed() is False and ok.first_bad is None
    assert bad.failed() is True and bad.first_bad == [0, 17, 3]
    assert _pivot.any_pivot_failed(torch.zeros(4, dtype=torch.int32)) is False


def test_chain_abort_is_an_internal_error_on_the_first_attempt():
    assert _pivot.INFO_CHAIN_ABORT == 0x7ffffff0
    with pytest.raises(RuntimeError, match="resident chain kernel .* timed out"):
        _check(0, _pivot.INFO_CHAIN_ABORT).failed()
    with pytest.raises(RuntimeError, match="internal error -- not a property of the matrix"):
        _pivot.any_pivot_failed(torch.tensor([5, _pivot.INFO_CHAIN_ABORT], dtype=torch.int32))
    with _pivot.deferred_pivot_checks() as dc:                      # and through the context a caller collects checks in
        dc.pending.append(_check(_pivot.INFO_CHAIN_ABORT))
    with pytest.raises(RuntimeError, match="resident chain kernel .* timed out"):
        dc.failed()


def test_chain_abort_on_a_retry_is_neither_swallowed_nor_retried():
    tried, warned, out = _walk(torch.float32, [(4, 0), (_pivot.INFO_CHAIN_ABORT, 0), (0, 0)])
    assert len(tried) == 2 and len(warned) == 2                     # the third rung is never reached
    assert isinstance(out, RuntimeError) and "resident chain kernel" in str(out) and "timed out" in str(out)
    assert "not positive definite" not in str(out)
