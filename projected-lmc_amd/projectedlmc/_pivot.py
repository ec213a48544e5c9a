"""What the host does about a factorisation that may not be positive definite -- once, for every model of the package.

The blocked sweep leaves one `info` word per latent (include/plmc.h): 0, 1 + the index of the first failing pivot (tests/test_gpu_factor.py), or
PLMC_INFO_CHAIN_ABORT.  This module owns the reading of those words (`PivotCheck`, at once or behind the kernels that follow
the sweep), the context a caller uses to collect the checks of a forward pass it can redo (`deferred_pivot_checks`), and the
jitter ladder of gpytorch's psd_safe_cholesky [gpytorch-knowledge] (`walk`; reference call sites: experiments.py:265,
projected_lmc.py:416,649).  A site keeps only its *attempt*: what to queue again with a given jitter.  Imports without a GPU.
"""
import warnings

import torch

from . import settings

INFO_CHAIN_ABORT = 0x7ffffff0      # csrc/diag_block.hpp: the sweep's resident chain kernel gave up a bounded wait (never a pivot index)


def any_pivot_failed(info_host):
    """The one reader of a host copy of `info`: True if a pivot failed; a chain abort is an internal error, never a pivot."""
    if bool((info_host == INFO_CHAIN_ABORT).any()):
        raise RuntimeError("projectedlmc: the resident chain kernel of the blocked sweep timed out waiting for another workgroup "
                           "(internal error -- not a property of the matrix); PLMC_CHAIN=0 selects the launch-per-step chain")
    return bool(info_host.any())


class PivotCheck:
    """Pivot check of the factorisation just queued on ws.  PivotCheck(ws) does not stall the stream: `info` is copied to
    pinned host memory right behind the sweep and looked at only after the kernels that follow it have been queued, so the
    GPU runs from the sweep straight into them while the host waits for the copy (not for those kernels).
    PivotCheck.eager(ws) reads `info` now (one synchronising copy).  Either way failed() says whether a pivot failed and
    leaves the `info` words -- 1 + the first failing pivot per latent, 0 for a latent that passed -- in `first_bad`."""
    first_bad = None

    def __init__(self, ws):
        if getattr(ws, "info_host", None) is None:
            ws.info_host = torch.empty(ws.info.shape, dtype=ws.info.dtype, pin_memory=True)
        self.host = ws.info_host
        self.host.copy_(ws.info, non_blocking=True)
        self.event = torch.cuda.Event()
        self.event.record(torch.cuda.current_stream(ws.device))

    @classmethod
    def eager(cls, ws):
        self = object.__new__(cls)
        self.host, self.event = ws.info.cpu(), None
        return self

    def failed(self):
        if self.event is not None:
            self.event.synchronize()
        bad = any_pivot_failed(self.host)
        self.first_bad = self.host.tolist() if bad else None
        return bad


class deferred_pivot_checks:
    """Context manager for a caller that can redo its whole forward pass: inside it the exact log-prob does not wait
    for the pivot check of its factorisation (the host goes on queueing the rest of the forward pass while the sweep
    runs); `failed()` after the block waits for the checks.  `jitter` is added to the noise of every factorisation
    inside the block -- the caller's retry ladder (ProjectedLMCmll.forward) plays psd_safe_cholesky's."""
    current = None

    def __init__(self, jitter=0.0):
        self.jitter = float(jitter)
        self.pending = []
        self.first_bad = None

    def __enter__(self):
        self._outer = deferred_pivot_checks.current
        deferred_pivot_checks.current = self
        return self

    def __exit__(self, *exc):
        deferred_pivot_checks.current = self._outer
        return False

    def failed(self):
        bad = [i for i in self.pending if i.failed()]
        self.first_bad = bad[0].host.tolist() if bad else None
        return bool(bad)


def walk(dtype, check, attempt):
    """The ladder, after the attempt without jitter failed (`check`: its check, failed() already True): retry with
    jitter * 10^i (settings.cholesky_jitter: 1e-6 fp32 / 1e-8 fp64) for i < settings.cholesky_max_tries, warning each time;
    raise if still not positive definite.  attempt(jitter) queues the site's work again with that jitter on the diagonal
    and returns (check, result), check being a PivotCheck or a deferred_pivot_checks.  Returns (jitter, result) of the
    first attempt that passed."""
    base, tries = settings.cholesky_jitter.value(dtype), settings.cholesky_max_tries.value()
    jit = 0.0
    for i in range(tries):
        jit = base * (10 ** i)
        warnings.warn("A not p.d., added jitter of %.1e to the diagonal" % jit, RuntimeWarning)
        check, result = attempt(jit)
        if not check.failed():
            return jit, result
    raise RuntimeError("Matrix not positive definite after repeatedly adding jitter up to %.1e "
                       "(first failing pivot per latent: %s)" % (jit, check.first_bad))
