"""Host side of the exact-GP hot path: torch-owned workspaces + autograd wrappers around the
C ABI (include/plmc.h).  PyTorch is plumbing here (device memory, streams, autograd graph);
all n x n work happens in the HIP library.

What it replaces in the reference: the gpytorch evaluation chain behind
`latent_output.log_prob(proj_target)` (projected_lmc.py:1200-1201), ExactMarginalLogLikelihood
(experiments.py:233) and `loss.backward()` (experiments.py:270); see SURVEY.md 8a rows a1-a4.
"""
import math
import os

import torch

from . import _hip
from . import settings
from .kernels import dot_power
from ._families import FAMILIES, LPER, OPERATIONS, PER, RQ, SUM, Sm, family_of, is_sum, sum_members     # noqa: F401 (re-exported)
from ._pivot import PivotCheck, deferred_pivot_checks, walk      # noqa: F401 (deferred_pivot_checks: re-exported for callers)

LOG2PI = math.log(2.0 * math.pi)


class Workspace:
    """Caller-owned device buffers for q latent GPs on n points with naug augmented columns.
    Layout documented in include/plmc.h."""

    def __init__(self, n, q, naug, dtype, device, with_inverse=True, keep_planes=False, ncomp=1, sm=False, per=False):
        L = _hip.lib()
        self.n, self.q, self.naug, self.dtype, self.device = n, q, naug, dtype, device
        self.ncomp = ncomp               # components of an additive kernel: the gradient kernel writes one row of partial sums per tile and component
        self.with_inverse = bool(with_inverse)
        # keep_planes (fp32, with the inverse factor): the sweep keeps the 16-bit planes of every group's solved rows, so that new
        # augmented columns can be forward-substituted on the split engine (plmc_potrs_aug_kept): the eval-mode cache
        self.keep_planes = bool(keep_planes) and self.with_inverse and dtype == torch.float32
        self.NB = L.cdll.plmc_block()
        self.n_pad = int(L.cdll.plmc_pad(n))
        self.naug_pad = int(L.cdll.plmc_pad(naug)) if naug > 0 else 0
        self.wcol0 = self.n_pad + self.naug_pad
        self.lda = self.wcol0 + (self.n_pad if with_inverse else 0)
        if (self.lda // self.NB) % 2 == 0:
            self.lda += self.NB          # odd number of blocks per row: keeps the row stride off a power of two
        self.strideA = self.n_pad * self.lda
        esz = torch.empty((), dtype=dtype).element_size()
        # scratch sizes depend on (n_pad, lda, element size) only -- never on a dev knob (include/plmc.h, version 3)
        vd_blocks = L.cdll.plmc_vd_blocks_keep(self.n_pad, self.lda) if self.keep_planes else L.cdll.plmc_vd_blocks_for(self.n_pad, self.lda, esz)
        self.Vd = torch.empty(q, int(vd_blocks), self.NB, self.NB, dtype=dtype, device=device)
        self.m = self.n_pad // self.NB
        self.A = torch.empty(q, self.n_pad, self.lda, dtype=dtype, device=device)
        self.logdet = torch.empty(q, dtype=torch.float64, device=device)
        self.quad = torch.empty(q, dtype=torch.float64, device=device)
        self.info = torch.empty(q, dtype=torch.int32, device=device)
        self.z = torch.empty(q, self.n_pad, dtype=dtype, device=device)
        self.W = self.alpha = self.partials = None
        if with_inverse:
            # W = U^-T lives in the same buffer, right of the augmented block (include/plmc.h)
            self.W = self.A[:, :, self.wcol0:self.wcol0 + self.n_pad]
            self.ldw, self.strideW = self.lda, self.strideA
            self.alpha = torch.empty(q, self.n_pad, dtype=dtype, device=device)
            # per-tile partial sums of the gradient kernel; the 16-bit planes of W it multiplies are left in Vd by the sweep
            # (plmc_kinv_grad_vd), except with PLMC_SPLIT=0 / fp64, which need none.  (sm, per) name the family whose size call it is
            self.partials = torch.empty(_partials_bytes(L, self.n_pad, q, esz, ncomp, sm, per) // 8, dtype=torch.float64, device=device)


_ws_cache = {}


def _release(ws):
    """Before a workspace's memory goes back to the caching allocator: the gradient kernel of its last evaluation may
    still read W / alpha and write the partials on the gradient stream -- make the allocating (current) stream wait."""
    pending = getattr(ws, "pending", None)
    if pending is not None:
        torch.cuda.current_stream(ws.device).wait_event(pending)
        ws.pending = None


def _drop_all():
    for ws in _ws_cache.values():
        _release(ws)
    _ws_cache.clear()


def get_workspace(n, q, naug, dtype, device, need_grad, ncomp=1, sm=False, per=False):
    ncomp = ncomp if need_grad else 1                   # (only the partial sums of the gradient kernel depend on it)
    sm = bool(sm) and bool(need_grad)
    per = per if (per and need_grad) else False       # False, PER, LPER or SUM (_per_kind)
    key = (n, q, naug, dtype, device.index, bool(need_grad), ncomp, sm, per)
    ws = _ws_cache.get(key)
    if ws is None:
        if len(_ws_cache) > 3:
            _drop_all()
        ws = Workspace(n, q, naug, dtype, device, need_grad, ncomp=ncomp, sm=sm, per=per)
        _ws_cache[key] = ws
    _release(ws)       # a gradient kernel of the previous evaluation may still be reading this workspace on the gradient stream
    return ws


_grad_streams = {}


def grad_stream(device):
    """Stream the fused K^-1 + gradient kernel runs on (one per device; PLMC_GRAD_STREAM=0: the caller's stream).
    The kernel is the last consumer of the factor and nothing in the forward pass needs its output, so the rest of
    the forward pass and the part of the backward pass ahead of the latent node (the projection terms of
    ProjectedLMCmll) -- dozens of launch-bound torch kernels -- run beside it instead of behind it."""
    if os.environ.get("PLMC_GRAD_STREAM", "1") == "0":
        return None
    s = _grad_streams.get(device.index)
    if s is None:
        s = _grad_streams[device.index] = torch.cuda.Stream(device)
    return s


def free_workspaces():
    _drop_all()


def _contig(t, dtype=None):
    if t is None:
        return None
    t = t.detach()
    if dtype is not None and t.dtype != dtype:
        t = t.to(dtype)
    return t.contiguous()


# ---- the kernel's hyper-parameters.  Every function below takes a kind with its table `ell` and `oscale`: (q, d), (q) | None -- one ARD
# kernel per latent -- or what the kind's covariance family makes of them.  _families has one row per family: its table's layout, the
# form of its entry points, its shape check, its component count and the size call of its gradient partials.  The functions here ask
# the row; everything else (workspaces, pivot checks, streams, caches) does not look at the kernel.

def sum_kind(members):
    """The kind string of a heterogeneous sum of these member kinds."""
    return "%s(%s)" % (SUM, ",".join(members))


def is_dot(kind):
    return dot_power(kind) is not None


def is_sm(ell):
    return ell.dim() == 4


def _per_kind(kind):
    """The kind if its table is a stack of (q, d) rows with one row of partial sums per tile (periodic, locally periodic), SUM for a
    heterogeneous sum (whatever its members: the key of its workspace), else False."""
    return family_of(kind).per_kind


def n_components(ell, kind=None):
    return family_of(kind, ell.dim()).ncomp(ell)


def kind_code(kind):
    """The library's code of a kernel kind.  The families whose entry points take none have no code: the spectral mixture's is None (its
    table's rank names it), the name of every other stands in the code's place and sends _kernel_call to its family."""
    return None if kind == "sm" else (_hip.KIND[kind] if family_of(kind).lead_kind else kind)


def grad_table_width(ell, kind=None):
    """Entries per latent of the gradient table: [d/d table (ell[0].numel()) | d/d noise | d/d oscale (one per component)]."""
    return ell[0].numel() + 1 + n_components(ell, kind)


def _check_kernel_shape(L, ell, kind=None):
    family_of(kind, ell.dim()).check(L, ell, kind)


def _partials_bytes(L, n_pad, q, esz, ncomp=1, sm=False, per=False):
    """Bytes of the per-tile partial sums of the gradient kernels at n_pad, by the size call of the family that a workspace's key names:
    `sm`, else `per` (True, PER, LPER or SUM: _per_kind), else the plain call, which the other families share (one row of partial sums
    per tile, latent and component)."""
    fam = Sm if sm else next(f for f in FAMILIES if f.per_kind == (PER if per is True else per))
    return int(fam.partials_bytes(L.cdll, n_pad, q, ncomp, esz))


def _table_workspace(n, q, naug, dtype, device, need_grad, ell, kind):
    """The workspace of a kind's table: keyed by what its family's gradient partials depend on."""
    return get_workspace(n, q, naug, dtype, device, need_grad, n_components(ell, kind), is_sm(ell), _per_kind(kind))


def _kernel_call(L, base, dt, head, ell, tail, stream=None):
    """Entry point `base`(*head, ell, *tail) in the form of the family that (head[0], ell) belongs to (_families): head[0], the kind's
    code or name, stays in front for the families that take a code and is dropped for the others, and the family's flat arguments stand
    in ell's place.  What a family passes beside the table itself -- contiguous copies of its rows or planes, a sum's host array of member
    codes -- is made once per table and kind and kept on the table: the 3-4 calls of a step share it.
    `stream`: the side stream the call is queued on, if not the current one."""
    kind = head[0]
    fam = family_of(kind, ell.dim())
    kept = ()
    if fam.split is not None:
        cached = getattr(ell, "_family_split", None)
        if cached is None or cached[0] != kind:
            cached = ell._family_split = (kind, fam.split(ell, kind))
        kept = cached[1]
        if stream is not None and fam.split_on_device:
            for t in kept:
                t.record_stream(stream)
    L.call(OPERATIONS[base][0] % fam.infix, dt, *(head if fam.lead_kind else head[1:]), *fam.flat(ell, kept, kind), *tail)


def _split_grad_table(g, ell_shape, os_shape):
    """Views (d/d ell, d/d noise, d/d oscale | None) of a gradient table (q, grad_table_width)."""
    ne = 1
    for s_ in ell_shape[1:]:
        ne *= s_
    return g[:, :ne].reshape(ell_shape), g[:, ne], (None if os_shape is None else g[:, ne + 1:].reshape(os_shape))


# ---- per-point noise.  Beside `noise` (q), one variance per latent, the functions that say so take `pnoise`: (n) -- one vector for every
# latent -- or (q, n), added to the diagonal behind the scalar (include/plmc.h, "Per-point noise").  Jitter goes on the
# scalar part; wherever `noise` is an eigenvalue bound, noise + min_i pnoise stands in its place.  A function of this module that has no
# `pnoise` argument does not serve it, and its callers refuse (refuse_point_noise) instead of dropping the vector.

def point_noise(pnoise, q, n, dtype):
    """The vector as the library takes it: detached, contiguous, of the call's dtype; (n) or (q, n)."""
    if pnoise is None:
        return None
    if pnoise.dim() not in (1, 2) or pnoise.shape[-1] != n or (pnoise.dim() == 2 and pnoise.shape[0] != q):
        raise ValueError("per-point noise is (n) = (%d) or (q, n) = (%d, %d), got %s" % (n, q, n, tuple(pnoise.shape)))
    return _contig(pnoise, dtype)


def _pn_args(pn):
    """(pnoise, stride_pn) of the *_pn entry points: stride 0 shares one vector between the latents"""
    return _hip.ptr(pn), (0 if pn.dim() == 1 else pn.shape[-1])


def noise_bound(noise, pn):
    """What stands where `noise` is passed as a lower bound on the eigenvalues of Khat: noise + min_i pnoise, (q)."""
    return noise if pn is None else (noise + pn.amin(-1)).contiguous()


def refuse_point_noise(what):
    raise NotImplementedError("%s does not serve per-point noise (FixedNoiseGaussianLikelihood): the vector would be dropped from the "
                              "diagonal -- use the marginal likelihood and the eval-mode predictions of ExactGPModel, or a "
                              "GaussianLikelihood" % what)


def factorize(kind, X, ell, oscale, noise, rhs, ws, Xs=None, eig_lo=True, pnoise=None):
    """Assemble Khat (+ rhs / cross-covariance columns) and run the blocked Cholesky.
    rhs: (q, nrhs, n) or None.  Returns nothing; results live in ws (A, Vd, logdet, info).
    eig_lo=False: `noise` is no eigenvalue bound to scale by (a jitter on a noise-free prior, sample_lazy): the fp32 sweep gets
    eig_lo = NULL and takes the three-plane scheme, which needs none (include/plmc.h, plmc_potrf_ex_*).
    pnoise (point_noise()'s result) | None: per-point noise, through the *_pn form of the same entry points."""
    L = _hip.lib()
    dt, dev = ws.dtype, ws.device
    st = _hip.stream_ptr(dev)
    k = kind_code(kind)
    q, n, d = ws.q, ws.n, X.shape[1]
    # round 4: assembly and sweep as ONE library call (plmc_factorize_ex_*): the sweep writes the rows of its first group itself and
    # queues the others beside that group's chain (same kernels, same data: bit-identical; PLMC_FUSED_ASSEMBLE=0: two calls)
    fused = os.environ.get("PLMC_FUSED_ASSEMBLE", "1") != "0"
    pn = () if pnoise is None else _pn_args(pnoise)
    assemble, fact = ("plmc_assemble", "plmc_factorize_ex") if pnoise is None else ("plmc_assemble_pn", "plmc_factorize_pn_ex")
    if not fused:
        _kernel_call(L, assemble, dt, (k, _hip.ptr(X), n, d), ell, (_hip.ptr(oscale), _hip.ptr(noise), *pn,
                     _hip.ptr(ws.A), ws.lda, ws.strideA, q, st))
    nrhs = 0 if rhs is None else rhs.shape[1]
    if ws.naug_pad > 0:
        L.call("plmc_write_rhs", dt, _hip.ptr(rhs), nrhs, n, _hip.ptr(ws.A), ws.lda, ws.strideA, 0, ws.naug_pad, q, st)
    if Xs is not None:
        _kernel_call(L, "plmc_assemble_cross", dt, (k, _hip.ptr(X), n, _hip.ptr(Xs), Xs.shape[0], d), ell,
                     (_hip.ptr(oscale), _hip.ptr(ws.A), ws.lda, ws.strideA, ws.n_pad + nrhs, ws.n_pad, q, st))
    # eig_lo = the noise variances: lambda_min(K + s2 I) >= s2 -- the bound the two-plane fp16 split of the bulk fp32 products
    # scales its operands with (include/plmc.h, plmc_potrf_ex_*); ignored by the fp64 entry point
    flags = (1 | (4 if ws.keep_planes else 0)) if ws.with_inverse else 0
    lo = noise_bound(noise, pnoise) if eig_lo else None           # (kept alive until the call is queued)
    bound = _hip.ptr(lo)
    if fused:
        _kernel_call(L, fact, dt, (k, _hip.ptr(X), n, d), ell, (_hip.ptr(oscale), _hip.ptr(noise), *pn, _hip.ptr(ws.A), ws.n_pad,
                     ws.lda, ws.naug, ws.strideA, _hip.ptr(ws.Vd), _hip.ptr(ws.logdet), _hip.ptr(ws.info), flags, q, bound, st))
    else:
        L.call("plmc_potrf_ex", dt, _hip.ptr(ws.A), ws.n_pad, ws.lda, ws.naug, ws.strideA, _hip.ptr(ws.Vd),
               _hip.ptr(ws.logdet), _hip.ptr(ws.info), flags, q, bound, st)


def factorize_checked(kind, X, ell, oscale, noise, rhs, ws, Xs=None, eig_lo=True, pnoise=None):
    """factorize + the jitter ladder (_pivot.walk) with the check read at once: on a non-PD pivot retry with noise + jitter (the scalar
    part takes it, with or without a per-point vector).  Returns the jitter that was added."""
    factorize(kind, X, ell, oscale, noise, rhs, ws, Xs, eig_lo, pnoise)
    if not settings.check_cholesky.on():
        return 0.0
    check = PivotCheck.eager(ws)
    if not check.failed():
        return 0.0

    def attempt(jit):
        factorize(kind, X, ell, oscale, noise + jit, rhs, ws, Xs, eig_lo, pnoise)
        return PivotCheck.eager(ws), None

    return walk(ws.dtype, check, attempt)[0]


class ExactLatentLogProb(torch.autograd.Function):
    """log N(y_i; 0, os_i k(X,X; ell_i) + noise_i I) for a batch of q independent GPs, with the
    analytic gradient computed in the same pass.

    forward(X (n,d), ell (q,d), oscale (q)|None, noise (q), y (q,n), kind) -> (q,)
    ell (q,G,d), oscale (q,G)|None: the component table of an additive kernel, same value and gradients (d/d ell (q,G,d), d/d oscale (q,G)).
    forward(..., kind, table) with table (q, grad_table_width(ell)) float64: the hyper-parameter gradients are written into `table` and
    NOT returned by this node's backward -- the two-node form exact_latent_log_prob builds when a gradient stream
    exists (see _HyperGrad).
    forward(..., kind, table | None, pnoise) with pnoise (n) | (q, n): per-point noise on the diagonal beside `noise`.  Where it requires a
    gradient, d logp / d pnoise_i = 1/2 (alpha_i^2 - (Khat^-1)_ii) is returned by this node (both forms), from alpha and the `kinv_diag`
    output of the K^-1 + gradient kernel -- a buffer that exists only then; the table's d/d noise stays the gradient of the scalar part.
    """

    @staticmethod
    def forward(ctx, X, ell, oscale, noise, y, kind, table=None, pnoise=None):
        x_grad = ctx.needs_input_grad[0]
        pn_grad = pnoise is not None and ctx.needs_input_grad[7]
        if x_grad:
            require_input_grad_kind(kind)
        _hip.require_device(X, ell, noise, y)
        L = _hip.lib()
        dt, dev = y.dtype, y.device
        if dt not in (torch.float32, torch.float64):
            raise TypeError("projectedlmc hot path supports float32 and float64 tensors")
        q, n = y.shape
        d = X.shape[1]
        _check_kernel_shape(L, ell, kind)
        need_grad = any(ctx.needs_input_grad[1:5]) or table is not None or x_grad or pn_grad
        Xc, ellc, osc, nzc, yc = (_contig(t, dt) for t in (X, ell, oscale, noise, y))
        pnc = point_noise(pnoise, q, n, dt)
        ws = _table_workspace(n, q, 1, dt, dev, need_grad, ell, kind)
        st = _hip.stream_ptr(dev)
        grad = table if table is not None else (torch.empty(q, grad_table_width(ell, kind), dtype=torch.float64, device=dev) if need_grad else None)
        check = settings.check_cholesky.on()
        # d logp / dX, one (n, d) table per latent: the K^-1 + gradient kernel also writes K^-1, plmc_input_grad pulls alpha alpha^T - K^-1
        # back through the kernel's input derivative.  Nothing of this exists when X requires no gradient.
        gX = torch.empty(q, n, d, dtype=torch.float64, device=dev) if x_grad else None
        kd = torch.empty(q, ws.n_pad, dtype=dt, device=dev) if pn_grad else None       # diag(Khat^-1): only for d logp / d pnoise

        def enqueue(noise_eff):
            """factorisation + everything that consumes it; returns (deferred pivot check, logp)."""
            factorize(kind, Xc, ellc, osc, noise_eff, yc.reshape(q, 1, n), ws, pnoise=pnc)
            # (the copy of `info` stays right behind the sweep: the late pivot check of a training step waits for it, and with one
            # latent per rank the host, which then still has the optimiser step and the next projection to queue, is nearly critical)
            info = PivotCheck(ws) if check else None
            L.call("plmc_extract_col", dt, _hip.ptr(ws.A), ws.n_pad, ws.lda, ws.strideA, 0, _hip.ptr(ws.z),
                   _hip.ptr(ws.quad), q, st)
            if need_grad:
                L.call("plmc_wt_matvec", dt, _hip.ptr(ws.W), ws.n_pad, ws.ldw, ws.strideW, _hip.ptr(ws.z),
                       _hip.ptr(ws.alpha), q, st)
                lo = noise_bound(noise_eff, pnc)          # the gradient call's eig_lo (queued in front of the gradient stream's wait)
                gs = grad_stream(dev)
                gst = st
                if gs is not None:
                    gs.wait_stream(torch.cuda.current_stream(dev))
                    gst = _hip.stream_handle(gs, dev)
                    for t in (grad, Xc, ellc, osc, noise_eff, gX, lo, kd):
                        if t is not None:
                            t.record_stream(gs)
                Kinv = _kinv_buffer(ws) if x_grad else None
                ldk = Kinv.shape[2] if x_grad else 0
                _kernel_call(L, "plmc_kinv_grad_vd", dt, (kind_code(kind), _hip.ptr(ws.W), ws.n_pad, ws.ldw, ws.strideW,
                             _hip.ptr(ws.alpha), _hip.ptr(Xc), n, d), ellc, (_hip.ptr(osc), _hip.ptr(grad),
                             _hip.ptr(Kinv), ldk, ws.n_pad * ldk, _hip.ptr(kd), _hip.ptr(ws.partials), q, _hip.ptr(lo), _hip.ptr(ws.Vd), gst),
                             stream=gs)
                if x_grad:
                    _kernel_call(L, "plmc_input_grad", dt, (kind_code(kind), _hip.ptr(Kinv), ws.n_pad, ldk, ws.n_pad * ldk,
                                 _hip.ptr(ws.alpha), _hip.ptr(Xc), n, d), ellc, (_hip.ptr(osc), _hip.ptr(gX), q, gst), stream=gs)
                if gs is not None:
                    ws.pending = torch.cuda.Event()
                    ws.pending.record(gs)
            # (the three small kernels of this line are queued BEHIND the gradient kernel's launch: in front of plmc_wt_matvec they
            # sat on the serial path sweep -> alpha -> gradient kernel)
            lp = -0.5 * (ws.quad + ws.logdet + n * LOG2PI)
            return info, lp

        dc = deferred_pivot_checks.current if check else None
        if dc is not None:                 # the caller owns the ladder and looks at the check after its forward pass
            info, logp = enqueue(nzc + dc.jitter if dc.jitter > 0.0 else nzc)
            dc.pending.append(info)
        else:
            info, logp = enqueue(nzc)
            if check and info.failed():
                def attempt(jit):
                    nonlocal ws
                    ws = _table_workspace(n, q, 1, dt, dev, need_grad, ell, kind)   # waits for the failed attempt's gradient kernel
                    return enqueue(nzc + jit)

                logp = walk(dt, info, attempt)[1]
        if need_grad:
            ctx.save_for_backward(grad, ws.alpha[:, :n].clone(), gX, kd)
        ctx.x_dtype = X.dtype
        ctx.pn_meta = (pnoise.dim(), pnoise.dtype) if pn_grad else None
        ctx.grad_ready = getattr(ws, "pending", None) if need_grad else None
        ctx.ell_shape = ell.shape
        ctx.os_shape = None if oscale is None else oscale.shape
        ctx.table_out = table is not None
        return logp.to(dt)

    @staticmethod
    def backward(ctx, gout):
        grad, alpha, gX, kd = ctx.saved_tensors
        dt = alpha.dtype
        g_X = g_pn = None
        if kd is not None:                 # d logp / d pnoise_i = 1/2 (alpha_i^2 - (Khat^-1)_ii); a shared vector sums the latents
            if ctx.grad_ready is not None:
                torch.cuda.current_stream(alpha.device).wait_event(ctx.grad_ready)
            a = alpha.to(torch.float64)
            g_pn = gout.to(torch.float64)[:, None] * (0.5 * (a * a - kd[:, :alpha.shape[1]].to(torch.float64)))
            g_pn = (g_pn.sum(0) if ctx.pn_meta[0] == 1 else g_pn).to(ctx.pn_meta[1])
        if gX is not None:                 # X is shared by the latents: their tables, weighted, summed in fp64
            if ctx.grad_ready is not None:
                torch.cuda.current_stream(alpha.device).wait_event(ctx.grad_ready)
            g_X = (gout.to(torch.float64)[:, None, None] * gX).sum(0).to(ctx.x_dtype)
        if ctx.table_out:                  # the hyper-parameter gradients flow through _HyperGrad
            return g_X, None, None, None, -(gout[:, None].to(dt) * alpha), None, None, g_pn
        if ctx.grad_ready is not None:
            torch.cuda.current_stream(alpha.device).wait_event(ctx.grad_ready)
        g_ell, g_noise, g_os = _split_grad_table(gout.to(torch.float64)[:, None] * grad, ctx.ell_shape, ctx.os_shape)
        g_y = -(gout[:, None].to(dt) * alpha)
        return g_X, g_ell, g_os, g_noise, g_y, None, None, g_pn


class _HyperGrad(torch.autograd.Function):
    """Second autograd node of the exact log-prob: contributes 0 to the value and carries d logp / d(ell, oscale,
    noise) from the gradient table.  It is applied with the gradient stream current, so autograd runs its backward on
    that stream -- behind the K^-1 + gradient kernel in stream order, no host wait -- and makes the caller's stream wait
    only where the first consumer of these gradients runs (the constraint transforms of the kernel parameters, created
    early in the forward pass and therefore late in the backward pass).  The backward of the projection (d logp / dy
    -> mixing matrix, ~50 launch-bound kernels) is queued ahead of that wait and runs beside the gradient kernel."""

    @staticmethod
    def forward(ctx, ell, oscale, noise, table, zero):
        ctx.save_for_backward(table)
        ctx.ell_shape = ell.shape
        ctx.os_shape = None if oscale is None else oscale.shape
        return zero.detach()

    @staticmethod
    def backward(ctx, gout):
        (table,) = ctx.saved_tensors
        g = (table * gout[:, None]).to(gout.dtype)          # fp64 product, one cast; the three gradients are views
        g_ell, g_noise, g_os = _split_grad_table(g, ctx.ell_shape, ctx.os_shape)
        return g_ell, g_os, g_noise, None, None


_zeros = {}


class HyperGradHandle:
    __slots__ = ("table", "hz")


def prepare_hyper_grad(ell, oscale, noise, kind=None):
    """Create the hyper-parameter gradient node (_HyperGrad) NOW and return a handle for exact_latent_log_prob, or
    None when there is nothing to do (no gradient stream, nothing requires grad, host tensors).
    Autograd runs backward nodes in reverse creation order, and the caller's stream is made to wait for the gradient
    stream as soon as this node has run; a caller that creates it BEFORE the graph that produces y (the projection
    of ProjectedLMCmll: QR, triangular solve, GEMMs) gets that graph's backward queued ahead of the wait."""
    hyper = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (ell, oscale, noise))
    gs = grad_stream(ell.device) if (hyper and ell.is_cuda) else None
    if gs is None:
        return None
    q = ell.shape[0]
    key = (ell.device.index, ell.dtype, q)
    zero = _zeros.get(key)
    if zero is None:
        zero = _zeros[key] = torch.zeros(q, dtype=ell.dtype, device=ell.device)
        torch.cuda.current_stream(ell.device).synchronize()
    h = HyperGradHandle()
    h.table = torch.empty(q, grad_table_width(ell, kind), dtype=torch.float64, device=ell.device)
    with torch.cuda.stream(gs):
        h.hz = _HyperGrad.apply(ell, oscale, noise, h.table, zero)
    return h


def exact_latent_log_prob(kind, X, ell, oscale, noise, y, hyper=None, pnoise=None):
    """pnoise (n) | (q, n) | None: per-point noise beside `noise`; it keeps its graph (ExactLatentLogProb)."""
    if hyper is None:
        hyper = prepare_hyper_grad(ell, oscale, noise, kind)
    if hyper is None:
        return ExactLatentLogProb.apply(X, ell, oscale, noise, y, kind, None, pnoise)
    det = lambda t: None if t is None else t.detach()
    lp = ExactLatentLogProb.apply(X, det(ell), det(oscale), det(noise), y, kind, hyper.table, pnoise)
    return lp + hyper.hz


def exact_loo(kind, X, ell, oscale, noise, y):
    """Leave-one-out moments of q independent exact GPs sharing the factorisation the MLL uses
    (reference: compute_loo, projected_lmc.py:371-436, 1108-1119):
        sigma2_i = 1 / [Khat^-1]_ii ,   (y - mu_loo)_i = [Khat^-1 y]_i * sigma2_i .
    diag(Khat^-1) is a by-product of the fused K^-1 kernel (`kinv_diag` output).  Returns (q,n),(q,n)."""
    _hip.require_device(X, ell, noise, y)
    L = _hip.lib()
    dt, dev = y.dtype, y.device
    q, n = y.shape
    d = X.shape[1]
    Xc, ellc, osc, nzc, yc = (_contig(t, dt) for t in (X, ell, oscale, noise, y))
    _check_kernel_shape(L, ellc, kind)
    ws = _table_workspace(n, q, 1, dt, dev, True, ellc, kind)
    st = _hip.stream_ptr(dev)
    factorize_checked(kind, Xc, ellc, osc, nzc, yc.reshape(q, 1, n), ws)
    L.call("plmc_extract_col", dt, _hip.ptr(ws.A), ws.n_pad, ws.lda, ws.strideA, 0, _hip.ptr(ws.z),
           _hip.ptr(ws.quad), q, st)
    L.call("plmc_wt_matvec", dt, _hip.ptr(ws.W), ws.n_pad, ws.ldw, ws.strideW, _hip.ptr(ws.z),
           _hip.ptr(ws.alpha), q, st)
    grad = torch.empty(q, grad_table_width(ellc, kind), dtype=torch.float64, device=dev)
    kd = torch.empty(q, ws.n_pad, dtype=dt, device=dev)
    _kernel_call(L, "plmc_kinv_grad_vd", dt, (kind_code(kind), _hip.ptr(ws.W), ws.n_pad, ws.ldw, ws.strideW, _hip.ptr(ws.alpha),
                 _hip.ptr(Xc), n, d), ellc, (_hip.ptr(osc), _hip.ptr(grad), None, 0, 0, _hip.ptr(kd),
                 _hip.ptr(ws.partials), q, _hip.ptr(nzc), _hip.ptr(ws.Vd), st))
    sigma2 = 1.0 / kd[:, :n]
    return sigma2, ws.alpha[:, :n] * sigma2


def loo_gradient_operands(kdiag, alpha, u=None, n=None):
    """What the gradient of the leave-one-out objective L = sum_i [1/2 log p_i - 1/2 alpha_i^2 / p_i] is built from (DESIGN.md,
    "Leave-one-out objective"), from p = diag(Khat^-1) and alpha = Khat^-1 y, both (q, n_pad); plain torch on any device.
        c = 1/2 / p + 1/2 alpha^2 / p^2 ,   g = -alpha / p          (u = Khat^-1 g is dL / dy)
    and, given u (q, n_pad), with s = sqrt(|u| / |alpha|) per latent and v+- = s alpha +- u / s:
        beta = v- / sqrt 2 ,   rowscale = sqrt(2 c) ,   extra_row = v+ / sqrt 2 ,
    so that 2 dL / dKhat = beta beta^T - Xop^T Xop for Xop = [diag(rowscale) Khat^-1 ; extra_row^T].  Entries at or beyond n are 0.
    Returns (c, g) or (c, g, beta, rowscale, extra_row)."""
    n = kdiag.shape[-1] if n is None else n
    live = torch.arange(kdiag.shape[-1], device=kdiag.device) < n
    p = torch.where(live, kdiag, torch.ones_like(kdiag))
    a = torch.where(live, alpha, torch.zeros_like(alpha))
    c = torch.where(live, 0.5 / p + 0.5 * a * a / (p * p), torch.zeros_like(p))
    g = -a / p
    if u is None:
        return c, g
    u = torch.where(live, u, torch.zeros_like(u))
    nu, na = u.norm(dim=-1, keepdim=True), a.norm(dim=-1, keepdim=True)
    s = torch.where((nu > 0) & (na > 0), (nu / na.clamp_min(torch.finfo(a.dtype).tiny)).sqrt(), torch.ones_like(nu))
    r = math.sqrt(0.5)
    return c, g, (s * a - u / s) * r, (2.0 * c).sqrt(), (s * a + u / s) * r


def _loo_buffers(ws):
    """K^-1 (n_pad rows of n_pad + NB) and the gradient product's operand (n_pad + NB rows of n_pad; n_pad + 16 are used) of the
    leave-one-out objective, q (n_pad + NB) n_pad elements each, kept with the workspace."""
    buf = getattr(ws, "loo", None)
    if buf is None:
        buf = ws.loo = (_kinv_buffer(ws), torch.empty(ws.q, ws.n_pad + ws.NB, ws.n_pad, dtype=ws.dtype, device=ws.device))
    return buf


def _kinv_buffer(ws):
    """K^-1 as plmc_kinv_grad*_vd writes it through `Kinv` (n_pad rows of n_pad + NB per latent, the upper triangle), kept with the
    workspace and created on first use: the leave-one-out objective and the input gradient of the MLL read it."""
    buf = getattr(ws, "kinv", None)
    if buf is None:
        buf = ws.kinv = torch.empty(ws.q, ws.n_pad, ws.n_pad + ws.NB, dtype=ws.dtype, device=ws.device)
    return buf


def require_input_grad_kind(kind):
    """d logp / dX exists for the kinds whose diagonal k(x, x) does not depend on x (plmc_input_grad*); the others say so."""
    if kind == "spline" or is_dot(kind) or is_sum(kind):
        raise NotImplementedError("kernel kind %r has no gradient with respect to the inputs yet (plmc_input_grad serves the stationary "
                                  "kinds, additive tables, sm, periodic, rq and locally_periodic): detach the inputs, or use "
                                  "one of those kernels behind an input_transform" % (kind,))


def input_grad(kind, X, ell, oscale, Kinv, alpha):
    """plmc_input_grad on caller-owned buffers: Kinv (q, n_pad, ldk) holding K^-1 in its upper triangle, alpha (q, n_pad), X (n, d) and
    the kind's table (ell, oscale) as everywhere in this module -> gX (q, n, d) float64,
        gX[l, i, k] = sum_{j != i} (alpha_li alpha_lj - Kinv_l[min(i, j), max(i, j)]) d k_l(x_i, x_j) / d x_i[k]."""
    _hip.require_device(X, ell, Kinv, alpha)
    L = _hip.lib()
    dt, dev = Kinv.dtype, Kinv.device
    q, n_pad, ldk = Kinv.shape
    n, d = X.shape
    Xc, ellc, osc, ac = (_contig(t, dt) for t in (X, ell, oscale, alpha))
    gX = torch.empty(q, n, d, dtype=torch.float64, device=dev)
    _kernel_call(L, "plmc_input_grad", dt, (kind_code(kind), _hip.ptr(Kinv), n_pad, ldk, Kinv.stride(0), _hip.ptr(ac), _hip.ptr(Xc), n, d),
                 ellc, (_hip.ptr(osc), _hip.ptr(gX), q, _hip.stream_ptr(dev)))
    return gX


class ExactLooLogProb(torch.autograd.Function):
    """Leave-one-out log predictive density sum_i log N(y_i; mu_-i, sigma2_-i) of q independent GPs, with the analytic gradient
    computed in the same pass ("Leave-one-out objective"): from the factorisation the MLL uses,
        L = sum_i [1/2 log p_i - 1/2 alpha_i^2 / p_i] - n/2 log 2 pi ,   p = diag(Khat^-1), alpha = Khat^-1 y.
    forward(X (n,d), ell, oscale, noise (q), y (q,n), kind) -> (q,), ell / oscale as for ExactLatentLogProb.  Everything runs on the
    current stream."""

    @staticmethod
    def forward(ctx, X, ell, oscale, noise, y, kind):
        _hip.require_device(X, ell, noise, y)
        L = _hip.lib()
        dt, dev = y.dtype, y.device
        if dt not in (torch.float32, torch.float64):
            raise TypeError("projectedlmc hot path supports float32 and float64 tensors")
        q, n = y.shape
        d = X.shape[1]
        _check_kernel_shape(L, ell, kind)
        need_grad = any(ctx.needs_input_grad[1:5])
        Xc, ellc, osc, nzc, yc = (_contig(t, dt) for t in (X, ell, oscale, noise, y))
        ws = _table_workspace(n, q, 1, dt, dev, True, ellc, kind)
        st = _hip.stream_ptr(dev)
        factorize_checked(kind, Xc, ellc, osc, nzc, yc.reshape(q, 1, n), ws)
        L.call("plmc_extract_col", dt, _hip.ptr(ws.A), ws.n_pad, ws.lda, ws.strideA, 0, _hip.ptr(ws.z), _hip.ptr(ws.quad), q, st)
        L.call("plmc_wt_matvec", dt, _hip.ptr(ws.W), ws.n_pad, ws.ldw, ws.strideW, _hip.ptr(ws.z), _hip.ptr(ws.alpha), q, st)
        Kinv, Xop = _loo_buffers(ws)
        ldk, ldx, krows = Kinv.shape[2], Xop.shape[2], ws.n_pad + 16
        grad = torch.empty(q, grad_table_width(ellc, kind), dtype=torch.float64, device=dev)
        kd = torch.empty(q, ws.n_pad, dtype=dt, device=dev)
        # K^-1 and its diagonal; the MLL gradient table this call also writes is overwritten below
        _kernel_call(L, "plmc_kinv_grad_vd", dt, (kind_code(kind), _hip.ptr(ws.W), ws.n_pad, ws.ldw, ws.strideW, _hip.ptr(ws.alpha),
                     _hip.ptr(Xc), n, d), ellc, (_hip.ptr(osc), _hip.ptr(grad), _hip.ptr(Kinv), ldk, ws.n_pad * ldk, _hip.ptr(kd),
                     _hip.ptr(ws.partials), q, _hip.ptr(nzc), _hip.ptr(ws.Vd), st))
        p, a = kd[:, :n].double(), ws.alpha[:, :n].double()
        value = (0.5 * p.log() - 0.5 * a * a / p).sum(-1) - 0.5 * n * LOG2PI
        if need_grad:
            c, g = loo_gradient_operands(kd, ws.alpha, n=n)
            rowscale = (2.0 * c).sqrt()
            L.call("plmc_loo_operand", dt, _hip.ptr(Kinv), ws.n_pad, ldk, ws.n_pad * ldk, _hip.ptr(rowscale), _hip.ptr(Xop), krows, ldx,
                   Xop.shape[1] * ldx, n, q, st)
            # u = Khat^-1 g = Xop^T (g / rowscale) over the live block
            u = torch.zeros(q, ws.n_pad, dtype=dt, device=dev)
            u[:, :n] = torch.bmm(Xop[:, :n, :n].transpose(1, 2), (g[:, :n] / rowscale[:, :n]).unsqueeze(-1)).squeeze(-1)
            beta, extra = loo_gradient_operands(kd, ws.alpha, u, n)[2::2]
            Xop[:, ws.n_pad, :] = extra
            beta = beta.contiguous()
            _kernel_call(L, "plmc_loo_grad", dt, (kind_code(kind), _hip.ptr(Xop), ws.n_pad, krows, ldx, Xop.shape[1] * ldx, _hip.ptr(beta),
                         _hip.ptr(Xc), n, d), ellc, (_hip.ptr(osc), _hip.ptr(grad), _hip.ptr(ws.partials), q, st))
            ctx.save_for_backward(grad, u[:, :n].clone())
        ctx.ell_shape = ell.shape
        ctx.os_shape = None if oscale is None else oscale.shape
        return value.to(dt)

    @staticmethod
    def backward(ctx, gout):
        grad, u = ctx.saved_tensors
        g_ell, g_noise, g_os = _split_grad_table(gout.to(torch.float64)[:, None] * grad, ctx.ell_shape, ctx.os_shape)
        return None, g_ell, g_os, g_noise, gout[:, None].to(u.dtype) * u, None


def exact_loo_log_prob(kind, X, ell, oscale, noise, y):
    """(q,) leave-one-out log predictive densities of y (q, n) under q independent exact GPs; see ExactLooLogProb."""
    return ExactLooLogProb.apply(X, ell, oscale, noise, y, kind)


class PosteriorCache:
    """What gpytorch's prediction strategy keeps between eval-mode calls of one model (projected_lmc.py:1133-1134,
    experiments.py:316-331 predicts batch by batch): the factorisation of the training covariance.  Here: a workspace of
    its own holding U, the inverse factor W and room for the augmented columns [y | K*^T].  The first call does the whole
    augmented sweep; while `key` (the model's parameter / data versions) is unchanged, a later call only rewrites the
    augmented columns and forward-substitutes them (plmc_potrs_aug): n^2 n* flops instead of n^3 / 3 + n^2 n*."""

    def __init__(self):
        self.key, self.ws = None, None
        self.seen = None                 # state key of the last uncached call (the cache is built on the SECOND call with one key)
        self.hits = self.misses = 0

    def drop(self):
        self.key, self.ws = None, None
        self.seen = None


def model_state_key(module, *tensors):
    """Cache key of an eval-mode model: identity and version counter of every parameter / buffer and of the given tensors
    (an optimiser step, load_state_dict or an in-place edit bumps a version; a new tensor has a new identity)."""
    items = [(id(t), t._version) for t in list(module.parameters()) + list(module.buffers())]
    items += [(id(t), t._version, tuple(t.shape)) for t in tensors if t is not None]
    return tuple(items)


def exact_posterior(kind, X, ell, oscale, noise, y, Xs, full_cov=False, cache=None, key=None, pnoise=None):
    """Posterior of q zero-mean GPs at Xs from ONE augmented factorization [Khat | y | K*^T]:
    with v = U^-T k*, z = U^-T y:  mean = v^T z,  cov = K** - v^T v.
    (ExactGPModel.__call__ in eval mode -> gpytorch DefaultPredictionStrategy; reached from
    projected_lmc.py:1134.)  Returns (mean (q,ns), var (q,ns) | cov (q,ns,ns)).
    cache / key: a PosteriorCache owned by the calling model and its state key -- see PosteriorCache.  The cache is built
    LAZILY (settings.prediction_cache "lazy", the default): the first call with a given key runs the plain augmented sweep
    (n^3 / 3 flops, a workspace from the shared pool) and only remembers the key; the second call with the same key pays for the
    sweep with the inverse factor and the kept planes (2 n^3 / 3, 13 GB at n = 8192, q = 8; ~50 GB per latent at n = 44 484) that
    every later call then reuses -- a one-shot prediction neither slows down nor holds that memory.  "eager" builds it
    on the first call, "off" never.
    Xs.requires_grad (with gradients enabled): the moments come from the autograd node PosteriorMoments, which carries d mean / dXs and
    d var / dXs; hyper-parameters, noise and training data stay constants.  Without it nothing below changes.
    pnoise (n) | (q, n) | None: per-point noise of the training points (a constant of the prediction); settings.posterior_hyper_grad
    does not serve it."""
    if pnoise is not None and settings.posterior_hyper_grad.on() and torch.is_grad_enabled():
        refuse_point_noise("settings.posterior_hyper_grad (predictions differentiable in hyper-parameters, noise and targets)")
    if settings.posterior_hyper_grad.on() and torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (ell, oscale, noise, y)):
        # hyper-parameters, noise or targets carry a graph: the node that differentiates the moments in them (and in Xs, if it asks)
        if full_cov:
            raise NotImplementedError("full_cov=True under settings.posterior_hyper_grad: only the marginal moments (mean, variance) are "
                                      "differentiable with respect to hyper-parameters, noise and targets -- predict with full_cov=False")
        if Xs.requires_grad:
            require_input_grad_kind(kind)
        return PosteriorHyperMoments.apply(Xs, ell, oscale, noise, y, kind, X, cache, key)
    if torch.is_grad_enabled() and Xs.requires_grad:
        if full_cov:
            raise NotImplementedError("full_cov=True together with test inputs that require a gradient: only the marginal moments "
                                      "(mean, variance) are differentiable with respect to the test inputs -- detach them, or "
                                      "predict with full_cov=False")
        require_input_grad_kind(kind)
        return PosteriorMoments.apply(Xs, kind, X, ell, oscale, noise, y, cache, key, pnoise)
    return _exact_posterior(kind, X, ell, oscale, noise, y, Xs, full_cov, cache, key, **({} if pnoise is None else {"pnoise": pnoise}))


def _exact_posterior(kind, X, ell, oscale, noise, y, Xs, full_cov=False, cache=None, key=None, dx=None, keep=None, pnoise=None):
    """exact_posterior's work.  dx = "mean" | "both": also the Jacobians of the marginal moments with respect to Xs, -> (mean, var, Jm,
    Jv | None) (_posterior_jacobians); they need the inverse factor, so a miss builds the cache at once where there is one (a caller
    who differentiates predictions will call again) and takes a pooled workspace WITH the inverse factor where there is none.
    keep (a dict, PosteriorHyperMoments): the workspace is chosen as for dx and handed back in keep["ws"]."""
    _hip.require_device(X, ell, noise, y, Xs)
    L = _hip.lib()
    dt, dev = y.dtype, y.device
    q, n = y.shape
    ns = Xs.shape[0]
    Xc, Xsc, ellc, osc, nzc = (_contig(t, dt) for t in (X, Xs, ell, oscale, noise))
    pnc = point_noise(pnoise, q, n, dt)
    _check_kernel_shape(L, ellc, kind)
    yc = _contig(y).reshape(q, 1, n)
    st = _hip.stream_ptr(dev)
    mode = settings.prediction_cache.value() if cache is not None else "off"
    if key is not None and (is_sum(kind) or is_dot(kind)):
        key = key + (kind,)                                # the members / the power are part of the state a cached factorisation belongs to
    hit = False
    if cache is not None and mode != "off":
        ws = cache.ws
        hit = (ws is not None and cache.key == key and key is not None and ws.dtype == dt and ws.device == dev and ws.n == n and ws.q == q
               and ws.naug >= 1 + ns)
    # build: eager mode; lazy mode on the second call with one key; or the cached state is the same and only its capacity is short
    same_state = cache is not None and cache.ws is not None and key is not None and cache.key == key
    build = cache is not None and mode != "off" and not hit and (mode == "eager" or same_state or (key is not None and cache.seen == key)
                                                                 or dx is not None or keep is not None)
    if not hit and not build:
        if cache is not None and mode != "off":
            cache.drop()                                   # (a stale factorisation of another state goes now, not at the next build)
            cache.seen = key
            cache.misses += 1
        ws = get_workspace(n, q, 1 + ns, dt, dev, dx is not None or keep is not None)
        factorize_checked(kind, Xc, ellc, osc, nzc, yc, ws, Xs=Xsc, pnoise=pnc)
    else:
        if hit:
            # new right-hand sides into the factorised buffer: y (column 0 shares its tile with the first test points, so it
            # is rewritten raw as well), K*^T behind it; then the forward substitution of those columns only
            cache.hits += 1
            k = kind_code(kind)
            L.call("plmc_write_rhs", dt, _hip.ptr(yc), 1, n, _hip.ptr(ws.A), ws.lda, ws.strideA, 0, ws.naug_pad, q, st)
            _kernel_call(L, "plmc_assemble_cross", dt, (k, _hip.ptr(Xc), n, _hip.ptr(Xsc), ns, Xc.shape[1]), ellc, (_hip.ptr(osc),
                         _hip.ptr(ws.A), ws.lda, ws.strideA, ws.n_pad + 1, ws.n_pad, q, st))
            if ws.keep_planes:
                L.call("plmc_potrs_aug_kept", dt, _hip.ptr(ws.A), ws.n_pad, ws.lda, 1 + ns, ws.wcol0, ws.strideA, _hip.ptr(ws.Vd), q,
                       _hip.ptr(noise_bound(nzc, pnc)), st)
            else:
                L.call("plmc_potrs_aug", dt, _hip.ptr(ws.A), ws.n_pad, ws.lda, 1 + ns, ws.wcol0, ws.strideA, _hip.ptr(ws.Vd), q, st)
        else:
            cache.misses += 1
            cache.drop()
            ws = Workspace(n, q, 1 + ns, dt, dev, with_inverse=True, keep_planes=True)
            ws.jitter = factorize_checked(kind, Xc, ellc, osc, nzc, yc, ws, Xs=Xsc, pnoise=pnc)      # (extend_cached_factor: the new diagonal carries it too)
            cache.key, cache.ws = key, ws
    # mean = V^T z and |v|^2 per test point: one pass over the augmented columns (plmc_posterior_moments)
    mean = torch.empty(q, ns, dtype=dt, device=dev)
    vsq = torch.empty(q, ns, dtype=dt, device=dev)
    L.call("plmc_posterior_moments", dt, _hip.ptr(ws.A), ws.n_pad, ws.lda, ws.strideA, ns, _hip.ptr(mean), _hip.ptr(vsq), q, st)
    if keep is not None:
        keep["ws"] = ws
    if full_cov:
        V = ws.A[:, :, ws.n_pad + 1:ws.n_pad + 1 + ns]             # (q, n_pad, ns) strided view, K-major
        Kss = dense_cross(kind, Xsc, Xsc, ellc, osc)
        from ._dense import gemm_tn
        cov = Kss - gemm_tn(V, V)                                   # V^T V on the library's tile engine (plmc_gemm_tn)
        return mean, cov
    from .kernels import prior_diagonal
    var = prior_diagonal(kind, Xsc, osc, q, ellc) - vsq                # k(x*, x*) = 1 for the stationary kinds (additive: sum_g os_g)
    if dx is not None:
        return (mean, var) + _posterior_jacobians(kind, Xc, Xsc, ellc, osc, ws, dx == "both")
    return mean, var


def _cached_factor(kind, Xc, ellc, osc, nzc, rhs, cache, key, always=False, pnc=None):
    """A factorised workspace WITH the inverse factor whose first augmented columns hold U^-T rhs, rhs (q, P, n): the model's cached one
    where its key matches and it has room for P columns (the new columns are written and forward-substituted, plmc_write_rhs +
    plmc_potrs_aug[_kept]); else a new one, kept in `cache` by the rule of exact_posterior (settings.prediction_cache: eager, the second
    call with one key in lazy mode, or a cached state that is the same and only short of columns; always=True: unless the mode is "off")
    and otherwise taken from the shared pool.  pnc: per-point noise as point_noise() returns it."""
    L = _hip.lib()
    dt, dev = rhs.dtype, rhs.device
    q, P, n = rhs.shape
    st = _hip.stream_ptr(dev)
    mode = settings.prediction_cache.value() if cache is not None else "off"
    if key is not None and (is_sum(kind) or is_dot(kind)):
        key = key + (kind,)
    ws = cache.ws if cache is not None and mode != "off" else None
    same_state = ws is not None and key is not None and cache.key == key
    if same_state and ws.dtype == dt and ws.device == dev and ws.n == n and ws.q == q and ws.naug >= P and ws.with_inverse:
        cache.hits += 1
        L.call("plmc_write_rhs", dt, _hip.ptr(rhs), P, n, _hip.ptr(ws.A), ws.lda, ws.strideA, 0, ws.naug_pad, q, st)
        if ws.keep_planes:
            L.call("plmc_potrs_aug_kept", dt, _hip.ptr(ws.A), ws.n_pad, ws.lda, P, ws.wcol0, ws.strideA, _hip.ptr(ws.Vd), q,
                   _hip.ptr(noise_bound(nzc, pnc)), st)
        else:
            L.call("plmc_potrs_aug", dt, _hip.ptr(ws.A), ws.n_pad, ws.lda, P, ws.wcol0, ws.strideA, _hip.ptr(ws.Vd), q, st)
        ws.alpha_key = None
        return ws
    build = cache is not None and mode != "off" and (always or mode == "eager" or same_state or (key is not None and cache.seen == key))
    if cache is not None and mode != "off":
        cache.misses += 1
        cache.drop()
    if build:
        ws = Workspace(n, q, P, dt, dev, with_inverse=True, keep_planes=True)
    else:
        if cache is not None and mode != "off":
            cache.seen = key
        ws = get_workspace(n, q, P, dt, dev, True)
    ws.jitter = factorize_checked(kind, Xc, ellc, osc, nzc, rhs, ws, pnoise=pnc)
    ws.alpha_key = None
    if build:
        cache.key, cache.ws = key, ws
    return ws


def extend_cached_factor(kind, X, ell, oscale, noise, y, Xnew, cache, key, pnoise=None, pnoise_new=None):
    """The cached factorisation of a model on X (n, d) conditioned on m new inputs Xnew (m, d) without a new sweep: a NEW
    workspace of n + m live rows that meets the sweep's post-condition with the inverse factor (plmc_factor_extend, O(n^2 m)), so that every
    eval-mode path works on it unchanged; the model's own cache (built first through _cached_factor if absent) is read, not changed --
    only its augmented columns are used for V = U^-T K(X, Xnew), as a cached prediction uses them.  Chunks of min(plmc_block(), naug) new
    rows: the first call copies base -> destination, the later ones extend the destination in place on its own augmented columns.  The new
    diagonal carries noise + the jitter the cached factor was built with.  The destination has the capacity (naug) of the base and keeps no
    planes of the split engine.  Returns the workspace, or None if a pivot of a Schur block was not positive (read once): the caller then
    has no extended factor and its first prediction factorises through the usual ladder.
    pnoise (n) | (q, n) with pnoise_new (m) | (q, m): per-point noise of the training points and of the new ones -- the new diagonal carries
    noise + jitter + pnoise_new."""
    if (pnoise is None) != (pnoise_new is None):
        raise ValueError("extend_cached_factor: per-point noise is given for the training points and for the new points, or for neither")
    _hip.require_device(X, ell, noise, y, Xnew)
    L = _hip.lib()
    dt, dev = y.dtype, y.device
    q, n = y.shape
    m = Xnew.shape[0]
    with torch.no_grad():
        Xc, Xn, ellc, osc, nzc = (_contig(t, dt) for t in (X, Xnew, ell, oscale, noise))
        _check_kernel_shape(L, ellc, kind)
        pnc, pnew = point_noise(pnoise, q, n, dt), point_noise(pnoise_new, q, m, dt)
        lo = noise_bound(nzc, pnc)
        base = _cached_factor(kind, Xc, ellc, osc, nzc, _contig(y).reshape(q, 1, n), cache, key, always=True, pnc=pnc)
        if cache is None or cache.ws is not base:
            return None                                    # (settings.prediction_cache "off": there is no cache to extend)
        base.alpha_key = None
        st = _hip.stream_ptr(dev)
        k, d = kind_code(kind), Xc.shape[1]
        dst = Workspace(n + m, q, base.naug, dt, dev, with_inverse=True, keep_planes=False)
        dst.jitter = float(getattr(base, "jitter", 0.0))
        dst.logdet.copy_(base.logdet)
        dst.alpha_key = None
        diag = nzc.reshape(-1) + dst.jitter
        esz = torch.empty((), dtype=dt).element_size()
        scratch = torch.empty(q * int(L.cdll.plmc_factor_extend_scratch_bytes(dst.n_pad, 1, esz)), dtype=torch.uint8, device=dev)
        Xall = torch.cat([Xc, Xn]).contiguous()
        step = min(base.NB, base.naug)
        # (what stands in the other columns of the base's first 128-column strip is substituted along and ignored: plmc_factor_extend
        # reads V from the first c columns only, and the base's next prediction rewrites the block)
        cur, live = base, n
        while live < n + m:
            c = min(step, n + m - live)
            Xl, Xs = Xall[:live], Xall[live:live + c].clone()
            _kernel_call(L, "plmc_assemble_cross", dt, (k, _hip.ptr(Xl), live, _hip.ptr(Xs), c, d), ellc, (_hip.ptr(osc), _hip.ptr(cur.A), cur.lda,
                         cur.strideA, cur.n_pad, cur.n_pad, q, st))
            if cur.keep_planes:
                L.call("plmc_potrs_aug_kept", dt, _hip.ptr(cur.A), cur.n_pad, cur.lda, c, cur.wcol0, cur.strideA, _hip.ptr(cur.Vd), q, _hip.ptr(lo), st)
            else:
                L.call("plmc_potrs_aug", dt, _hip.ptr(cur.A), cur.n_pad, cur.lda, c, cur.wcol0, cur.strideA, _hip.ptr(cur.Vd), q, st)
            K22 = dense_cross(kind, Xs, Xs, ellc, osc)
            K22.diagonal(dim1=1, dim2=2).add_(diag[:, None])
            if pnew is not None:
                K22.diagonal(dim1=1, dim2=2).add_(pnew[..., live - n:live - n + c])
            L.call("plmc_factor_extend", dt, _hip.ptr(cur.A), live, cur.n_pad, cur.lda, cur.wcol0, cur.strideA, c, _hip.ptr(K22), _hip.ptr(dst.A),
                   dst.n_pad, dst.lda, dst.wcol0, dst.strideA, _hip.ptr(dst.logdet), _hip.ptr(dst.info), _hip.ptr(scratch), q, st)
            cur, live = dst, live + c
        if PivotCheck.eager(dst).failed():
            return None
        return dst


def exact_posterior_mean(kind, X, ell, oscale, noise, y, Xs, cache=None, key=None, pnoise=None):
    """Posterior mean of q zero-mean GPs at Xs, (q, ns), as K(Xs, X) alpha with alpha = Khat^-1 y from a factorisation of [Khat | y]
    (settings.skip_posterior_variances): no augmented columns for the test points, so ns is not bounded by a workspace, and K(Xs, X) is
    never written (cross_matvec).  alpha is kept with the model's cached workspace (_cached_factor) and reused while the key is unchanged."""
    _hip.require_device(X, ell, noise, y, Xs)
    L = _hip.lib()
    dt, dev = y.dtype, y.device
    q, n = y.shape
    with torch.no_grad():
        Xc, Xsc, ellc, osc, nzc = (_contig(t, dt) for t in (X, Xs, ell, oscale, noise))
        _check_kernel_shape(L, ellc, kind)
        full_key = key + (kind,) if key is not None and (is_sum(kind) or is_dot(kind)) else key
        ws = cache.ws if cache is not None and settings.prediction_cache.value() != "off" else None
        ready = (ws is not None and full_key is not None and cache.key == full_key and getattr(ws, "alpha_key", None) == full_key
                 and ws.dtype == dt and ws.device == dev and ws.n == n and ws.q == q)
        if ready:
            cache.hits += 1
            alpha = ws.alpha_kept
        else:
            ws = _cached_factor(kind, Xc, ellc, osc, nzc, _contig(y).reshape(q, 1, n), cache, key, pnc=point_noise(pnoise, q, n, dt))
            st = _hip.stream_ptr(dev)
            L.call("plmc_extract_col", dt, _hip.ptr(ws.A), ws.n_pad, ws.lda, ws.strideA, 0, _hip.ptr(ws.z), _hip.ptr(ws.quad), q, st)
            L.call("plmc_wt_matvec", dt, _hip.ptr(ws.W), ws.n_pad, ws.ldw, ws.strideW, _hip.ptr(ws.z), _hip.ptr(ws.alpha), q, st)
            alpha = ws.alpha
            if cache is not None and cache.ws is ws:       # (ws.alpha itself is rewritten by the calls that differentiate predictions)
                ws.alpha_kept, ws.alpha_key = ws.alpha.clone(), full_key
        return cross_matvec(kind, Xsc, Xc, ellc, osc, alpha, n=n, ws=ws)


def solve_cached(kind, X, ell, oscale, noise, rhs, cache=None, key=None):
    """Khat^-1 rhs for q latents against the model's cached factor, rhs (q, P, n) -> (q, n, P) K-major: the columns are forward-substituted
    in the factor buffer (_cached_factor; the cache is built if there is none) and multiplied by W^T on the tile engine as the
    prediction's input derivative does it (_posterior_jacobians)."""
    _hip.require_device(X, ell, noise, rhs)
    L = _hip.lib()
    dt, dev = rhs.dtype, rhs.device
    q, P, n = rhs.shape
    with torch.no_grad():
        Xc, ellc, osc, nzc, rc = (_contig(t, dt) for t in (X, ell, oscale, noise, rhs))
        _check_kernel_shape(L, ellc, kind)
        ws = _cached_factor(kind, Xc, ellc, osc, nzc, rc, cache, key, always=True)
        buf = _wtv_buffer(ws)
        ncols = int(L.cdll.plmc_pad(P))
        L.call("plmc_gemm_tn_tri", dt, 0, 1, ws.n_pad, ncols, ws.n_pad, _hip.ptr(ws.W), ws.ldw, ws.strideW,
               _hip.ptr(ws.A[:, :, ws.n_pad:]), ws.lda, ws.strideA, _hip.ptr(buf), buf.shape[2], buf.stride(0), q, _hip.stream_ptr(dev))
        return buf[:, :n, :P].clone()


def _wtv_buffer(ws):
    """[alpha | B] = W^T [z | V] of the eval-mode posterior (n_pad rows of naug_pad per latent), kept with the workspace and created on
    first use: the variance part of the prediction's input derivative reads B = Khat^-1 K*^T from its columns 1 ..."""
    buf = getattr(ws, "wtv", None)
    if buf is None:
        buf = ws.wtv = torch.empty(ws.q, ws.n_pad, ws.naug_pad, dtype=ws.dtype, device=ws.device)
    return buf


def _posterior_jacobians(kind, Xc, Xsc, ellc, osc, ws, variance):
    """(Jm, Jv | None), (q, ns, d) float64 each: d mean / dXs and d var / dXs from a factorised workspace with the inverse factor whose
    augmented columns hold [z | V] = U^-T [y | K*^T] (plmc_posterior_dx).  alpha = W^T z as the leave-one-out path takes
    it.  variance: B = W^T V on the tile engine, in place on the strided views -- W is the lower triangle of its block of the factor
    buffer (explicit zeros above the diagonal inside the diagonal blocks; PLMC_TRI_A_LOWER skips the blocks above, which are never
    written), rows >= n of the augmented columns are zero and the padded part of W is the identity.  The product starts at the aligned
    column n_pad, so its column 0 is W^T z and test point s stands in column 1 + s; the columns it covers beyond 1 + ns are zeros
    (plmc_write_rhs clears the block)."""
    L = _hip.lib()
    dt, dev, q, n = ws.dtype, ws.device, ws.q, ws.n
    ns, d = Xsc.shape
    st = _hip.stream_ptr(dev)
    L.call("plmc_extract_col", dt, _hip.ptr(ws.A), ws.n_pad, ws.lda, ws.strideA, 0, _hip.ptr(ws.z), _hip.ptr(ws.quad), q, st)
    L.call("plmc_wt_matvec", dt, _hip.ptr(ws.W), ws.n_pad, ws.ldw, ws.strideW, _hip.ptr(ws.z), _hip.ptr(ws.alpha), q, st)
    B = None
    if variance:
        buf = _wtv_buffer(ws)
        ncols = int(L.cdll.plmc_pad(1 + ns))
        L.call("plmc_gemm_tn_tri", dt, 0, 1, ws.n_pad, ncols, ws.n_pad, _hip.ptr(ws.W), ws.ldw, ws.strideW,
               _hip.ptr(ws.A[:, :, ws.n_pad:]), ws.lda, ws.strideA, _hip.ptr(buf), buf.shape[2], buf.stride(0), q, st)     # 1: PLMC_TRI_A_LOWER
        B = buf[:, :, 1:]
    return posterior_dx(kind, Xc, Xsc, ellc, osc, ws.alpha, B, n=n)


def posterior_dx_splits(n, ns, q):
    """Ranges plmc_posterior_dx splits n training rows into for ns test points and q latents (one workgroup each per block of test points)."""
    return int(_hip.lib().cdll.plmc_posterior_dx_splits(n, ns, q))


def posterior_dx(kind, X, Xs, ell, oscale, alpha, B, n=None, Jv=None):
    """plmc_posterior_dx on caller-owned buffers: X (n, d), Xs (ns, d), the kind's table (ell, oscale) as everywhere in this module,
    alpha (q, n_pad) and B (q, rows >= n, ldb >= ns) | None, a view with unit stride along the test points -> (Jm, Jv), (q, ns, d) float64,
        Jm[l, s, k] = sum_i alpha_li d k_l(xs_s, x_i) / d xs_s[k],   Jv[l, s, k] = -2 sum_i B_l[i, s] d k_l(xs_s, x_i) / d xs_s[k].
    B None: Jv is handed back as given (None, or the caller's buffer untouched)."""
    _hip.require_device(X, Xs, ell, alpha, B)
    L = _hip.lib()
    dt, dev = alpha.dtype, alpha.device
    q, n_pad = alpha.shape
    n = X.shape[0] if n is None else n
    ns, d = Xs.shape
    Xc, Xsc, ellc, osc, ac = (_contig(t, dt) for t in (X, Xs, ell, oscale, alpha))
    Jm = torch.empty(q, ns, d, dtype=torch.float64, device=dev)
    ldb = strideB = 0
    if B is not None:
        if B.stride(2) != 1:
            raise ValueError("B must be contiguous along the test points")
        ldb, strideB = B.stride(1), B.stride(0)
        if Jv is None:
            Jv = torch.empty(q, ns, d, dtype=torch.float64, device=dev)
    nbytes = int(L.cdll.plmc_posterior_dx_partials_bytes(n, ns, d, q))
    partials = torch.empty(nbytes // 8, dtype=torch.float64, device=dev) if nbytes else None
    _kernel_call(L, "plmc_posterior_dx", dt, (kind_code(kind), _hip.ptr(Xc), n, _hip.ptr(Xsc), ns, d), ellc,
                 (_hip.ptr(osc), _hip.ptr(ac), n_pad, _hip.ptr(B), ldb, strideB, _hip.ptr(Jm), _hip.ptr(Jv if B is not None else None),
                  _hip.ptr(partials), q, _hip.stream_ptr(dev)))
    return Jm, Jv


def cross_matvec_splits(n, ns, q):
    """Ranges plmc_cross_matvec / plmc_rff_matvec split n rows into for ns test points and q latents."""
    return int(_hip.lib().cdll.plmc_cross_matvec_splits(n, ns, q))


_cm_scratch = {}


def _cross_matvec_scratch(nbytes, dev, ws=None):
    """fp64 scratch of the range split: the caller's workspace lends its gradient partials when they are large enough; else one pooled
    tensor per device, grown on demand.  Calls on one stream use it one after the other."""
    if not nbytes:
        return None
    own = getattr(ws, "partials", None)
    if own is not None and own.numel() * 8 >= nbytes:
        return own
    buf = _cm_scratch.get(dev.index)
    if buf is None or buf.numel() * 8 < nbytes:
        buf = _cm_scratch[dev.index] = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
    buf.record_stream(torch.cuda.current_stream(dev))
    return buf


def cross_matvec(kind, Xs, X, ell, oscale, V, n=None, ws=None):
    """K(Xs, X) V without K(Xs, X) (plmc_cross_matvec): Xs (ns, d), X (n, d), the kind's table (ell, oscale) as everywhere
    in this module, V (q, rows >= n) -- one column, e.g. alpha (q, n_pad) -- or (q, rows >= n, r) with unit stride along r (a view of
    the [alpha | B] buffer is taken as it is) -> (q, ns) or (q, ns, r) of V's dtype,
        out[l, s, c] = sum_{i < n} k_l(xs_s, x_i) V[l, i, c].
    More columns than plmc_cross_matvec_max_cols() go in chunks.  ws: a workspace whose scratch may be borrowed.  Current stream."""
    _hip.require_device(X, Xs, ell, V)
    L = _hip.lib()
    dt, dev = V.dtype, V.device
    vec = V.dim() == 2
    Vv = V.detach().unsqueeze(-1) if vec else V.detach()
    if Vv.shape[2] > 1 and Vv.stride(2) != 1:
        raise ValueError("V must be contiguous along its columns")
    q, r = Vv.shape[0], Vv.shape[2]
    n = X.shape[0] if n is None else n
    ns, d = Xs.shape
    Xc, Xsc, ellc, osc = (_contig(t, dt) for t in (X, Xs, ell, oscale))
    _check_kernel_shape(L, ellc, kind)
    ldv, strideV = Vv.stride(1), Vv.stride(0)
    cap = int(L.cdll.plmc_cross_matvec_max_cols())
    st = _hip.stream_ptr(dev)
    out = torch.empty(q, ns, r, dtype=dt, device=dev)
    for c0 in range(0, r, cap):
        rc = min(cap, r - c0)
        part = _cross_matvec_scratch(int(L.cdll.plmc_cross_matvec_partials_bytes(n, ns, rc, q)), dev, ws)
        dst = out if rc == r else torch.empty(q, ns, rc, dtype=dt, device=dev)
        _kernel_call(L, "plmc_cross_matvec", dt, (kind_code(kind), _hip.ptr(Xc), n, _hip.ptr(Xsc), ns, d), ellc,
                     (_hip.ptr(osc), _hip.ptr(Vv[:, :, c0:]), ldv, strideV, rc, _hip.ptr(dst), _hip.ptr(part), q, st))
        if dst is not out:
            out[:, :, c0:c0 + rc] = dst
    return out[:, :, 0] if vec else out


def rff_matvec(freq, phase, Xs, Wt, scale=None):
    """The prior part of a pathwise draw (plmc_rff_matvec): freq (q, m, d) and phase (q, m) in revolutions, Xs (ns, d), Wt (q, m, r),
    scale (q) | None -> (q, ns, r),  out[l, s, c] = scale_l sum_j cos(2 pi (freq_lj . xs_s + phase_lj)) Wt[l, j, c].  Wider Wt than
    plmc_cross_matvec_max_cols() goes in chunks.  Current stream."""
    _hip.require_device(freq, phase, Xs, Wt)
    L = _hip.lib()
    dt, dev = Wt.dtype, Wt.device
    q, m, r = Wt.shape
    ns, d = Xs.shape
    fc, pc, Xsc, sc = (_contig(t, dt) for t in (freq, phase, Xs, scale))
    cap = int(L.cdll.plmc_cross_matvec_max_cols())
    st = _hip.stream_ptr(dev)
    out = torch.empty(q, ns, r, dtype=dt, device=dev)
    for c0 in range(0, r, cap):
        rc = min(cap, r - c0)
        part = _cross_matvec_scratch(int(L.cdll.plmc_cross_matvec_partials_bytes(m, ns, rc, q)), dev)
        Wc = _contig(Wt[:, :, c0:c0 + rc])
        dst = out if rc == r else torch.empty(q, ns, rc, dtype=dt, device=dev)
        L.call("plmc_rff_matvec", dt, _hip.ptr(fc), _hip.ptr(pc), m, _hip.ptr(Xsc), ns, d, _hip.ptr(Wc), rc, _hip.ptr(sc), _hip.ptr(dst),
               _hip.ptr(part), q, st)
        if dst is not out:
            out[:, :, c0:c0 + rc] = dst
    return out


def cross_matvec_dx(kind, Xs, X, ell, oscale, V, G=None, n=None, ws=None):
    """d (K(Xs, X) V) / dXs contracted with G, without K(Xs, X) (plmc_cross_matvec_dx): Xs (ns, d), X (n, d) raw
    coordinates, the kind's table (ell, oscale) as everywhere in this module, V (q, rows >= n) or (q, rows >= n, r) as cross_matvec takes
    it, G (q, ns, r) the upstream gradient of cross_matvec's result -> (q, ns, d) float64,
        out[l, s, k] = sum_{i < n} (sum_c G[l, s, c] V[l, i, c]) d k_l(xs_s, x_i) / d xs_s[k].
    G None (one column only): the Jacobian of that column.  More columns than plmc_cross_matvec_max_cols() go in chunks whose float64
    results are added in chunk order.  ws: a workspace whose scratch may be borrowed.  Current stream."""
    require_input_grad_kind(kind)
    _hip.require_device(X, Xs, ell, V, G)
    L = _hip.lib()
    dt, dev = V.dtype, V.device
    Vv = V.detach().unsqueeze(-1) if V.dim() == 2 else V.detach()
    if Vv.shape[2] > 1 and Vv.stride(2) != 1:
        raise ValueError("V must be contiguous along its columns")
    q, r = Vv.shape[0], Vv.shape[2]
    n = X.shape[0] if n is None else n
    ns, d = Xs.shape
    if G is None and r != 1:
        raise ValueError("cross_matvec_dx: G=None is the Jacobian of ONE column, V has %d" % r)
    if G is not None and tuple(G.shape) != (q, ns, r):
        raise ValueError("cross_matvec_dx: G is (q, ns, r) = %s, got %s" % ((q, ns, r), tuple(G.shape)))
    Xc, Xsc, ellc, osc = (_contig(t, dt) for t in (X, Xs, ell, oscale))
    _check_kernel_shape(L, ellc, kind)
    ldv, strideV = Vv.stride(1), Vv.stride(0)
    cap = int(L.cdll.plmc_cross_matvec_max_cols())
    st = _hip.stream_ptr(dev)
    part = _cross_matvec_scratch(int(L.cdll.plmc_cross_matvec_dx_partials_bytes(n, ns, d, q)), dev, ws)
    out = None
    for c0 in range(0, r, cap):
        rc = min(cap, r - c0)
        Gc = None if G is None else _contig(G[:, :, c0:c0 + rc], dt)
        dst = torch.empty(q, ns, d, dtype=torch.float64, device=dev)
        _kernel_call(L, "plmc_cross_matvec_dx", dt, (kind_code(kind), _hip.ptr(Xc), n, _hip.ptr(Xsc), ns, d), ellc,
                     (_hip.ptr(osc), _hip.ptr(Vv[:, :, c0:]), ldv, strideV, rc, _hip.ptr(Gc), _hip.ptr(dst), _hip.ptr(part), q, st))
        out = dst if out is None else out + dst
    return out


def rff_matvec_dx(freq, phase, Xs, Wt, G=None, scale=None):
    """d rff_matvec / dXs contracted with G (plmc_rff_matvec_dx): freq (q, m, d) and phase (q, m) in revolutions, Xs (ns, d), Wt (q, m, r),
    G (q, ns, r) | None (r = 1: the Jacobian of the one column), scale (q) | None -> (q, ns, d) float64,
        out[l, s, k] = -2 pi scale_l sum_j sin(2 pi (freq_lj . xs_s + phase_lj)) freq_ljk sum_c G[l, s, c] Wt[l, j, c].
    Wider Wt than plmc_cross_matvec_max_cols() goes in chunks whose float64 results are added in chunk order.  Current stream."""
    _hip.require_device(freq, phase, Xs, Wt, G)
    L = _hip.lib()
    dt, dev = Wt.dtype, Wt.device
    q, m, r = Wt.shape
    ns, d = Xs.shape
    if G is None and r != 1:
        raise ValueError("rff_matvec_dx: G=None is the Jacobian of ONE column, Wt has %d" % r)
    if G is not None and tuple(G.shape) != (q, ns, r):
        raise ValueError("rff_matvec_dx: G is (q, ns, r) = %s, got %s" % ((q, ns, r), tuple(G.shape)))
    fc, pc, Xsc, sc = (_contig(t, dt) for t in (freq, phase, Xs, scale))
    cap = int(L.cdll.plmc_cross_matvec_max_cols())
    st = _hip.stream_ptr(dev)
    part = _cross_matvec_scratch(int(L.cdll.plmc_cross_matvec_dx_partials_bytes(m, ns, d, q)), dev)
    out = None
    for c0 in range(0, r, cap):
        rc = min(cap, r - c0)
        Wc = _contig(Wt[:, :, c0:c0 + rc])
        Gc = None if G is None else _contig(G[:, :, c0:c0 + rc], dt)
        dst = torch.empty(q, ns, d, dtype=torch.float64, device=dev)
        L.call("plmc_rff_matvec_dx", dt, _hip.ptr(fc), _hip.ptr(pc), m, _hip.ptr(Xsc), ns, d, _hip.ptr(Wc), rc, _hip.ptr(Gc), _hip.ptr(sc),
               _hip.ptr(dst), _hip.ptr(part), q, st)
        out = dst if out is None else out + dst
    return out


class PosteriorMoments(torch.autograd.Function):
    """(mean, var) of exact_posterior as a function of the test inputs Xs: forward is _exact_posterior, which also leaves the Jacobians
    Jm, Jv (q, ns, d); test points do not interact in the marginal moments, so backward is element-wise,
        gXs[s, k] = sum_l gmean[l, s] Jm[l, s, k] + gvar[l, s] Jv[l, s, k].
    Hyper-parameters, noise and training data are constants of this node.  settings.predictive_variance_grad(False): Jv is not formed
    and `var` carries no gradient.  Not twice differentiable."""

    @staticmethod
    def forward(ctx, Xs, kind, X, ell, oscale, noise, y, cache, key, pnoise=None):
        variance = settings.predictive_variance_grad.on()
        pn = {} if pnoise is None else {"pnoise": pnoise}
        mean, var, Jm, Jv = _exact_posterior(kind, X, ell, oscale, noise, y, Xs, False, cache, key, dx="both" if variance else "mean", **pn)
        ctx.save_for_backward(Jm, Jv)
        ctx.x_dtype = Xs.dtype
        if not variance:
            ctx.mark_non_differentiable(var)
        return mean, var

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gmean, gvar):
        Jm, Jv = ctx.saved_tensors
        g = (gmean.to(torch.float64)[:, :, None] * Jm).sum(0)
        if Jv is not None and gvar is not None:
            g = g + (gvar.to(torch.float64)[:, :, None] * Jv).sum(0)
        return (g.to(ctx.x_dtype),) + (None,) * 9


def _grad_partials(L, n_pad, q, ell, kind, dtype, device):
    """The per-tile partial sums of the family's gradient kernels at n_pad, by the library's own size calls (as Workspace sizes them)."""
    esz = torch.empty((), dtype=dtype).element_size()
    nbytes = _partials_bytes(L, n_pad, q, esz, n_components(ell, kind), is_sm(ell), _per_kind(kind))
    return torch.empty(nbytes // 8, dtype=torch.float64, device=device)


def weighted_grad(kind, Z, ell, oscale, At, Bt, N):
    """plmc_weighted_grad on caller-owned buffers (include/plmc.h, "Weighted kernel-gradient sum"): Z (N, d), the kind's table (ell, oscale)
    as everywhere in this module, At, Bt (q, r_pad, ld) K-major with unit stride along ld >= plmc_pad(N), zeros in the rows that carry
    nothing and in the columns [N, plmc_pad(N)) -> (d/d ell, d/d noise, d/d oscale | None) float64, shaped like the table,
        g[l][t] = sum_{i <= j < N} c_ij (At_l^T Bt_l)_ij d Khat_l(Z)_ij / d theta_t,   c_ii = 1, c_ij = 2.
    Current stream."""
    _hip.require_device(Z, ell, At, Bt)
    L = _hip.lib()
    dt, dev = At.dtype, At.device
    if At.dim() != 3 or At.shape != Bt.shape or At.stride() != Bt.stride() or At.stride(2) != 1 or Bt.dtype != dt:
        raise ValueError("weighted_grad: At and Bt are (q, r_pad, ld) of one dtype, shape and layout, contiguous along ld")
    q, r_pad, ld = At.shape[0], At.shape[1], At.stride(1)
    N_pad = int(L.cdll.plmc_pad(N))
    Zc, ellc, osc = (_contig(t, dt) for t in (Z, ell, oscale))
    _check_kernel_shape(L, ellc, kind)
    if ellc.shape[0] != q:
        raise ValueError("weighted_grad: the table has %d latents, the operands %d" % (ellc.shape[0], q))
    grad = torch.empty(q, grad_table_width(ellc, kind), dtype=torch.float64, device=dev)
    partials = _grad_partials(L, N_pad, q, ellc, kind, dt, dev)
    _kernel_call(L, "plmc_weighted_grad", dt, (kind_code(kind), _hip.ptr(At), _hip.ptr(Bt), r_pad, N_pad, ld, At.stride(0), _hip.ptr(Zc), N,
                 Zc.shape[1]), ellc, (_hip.ptr(osc), _hip.ptr(grad), _hip.ptr(partials), q, _hip.stream_ptr(dev)))
    return _split_grad_table(grad, ellc.shape, None if osc is None else osc.shape)


_OPERAND_BLOCK, _OPERAND_DEPTH = 128, 16        # plmc_block() and the stage depth of the tile engine (include/plmc.h): the operands' padding


def posterior_hyper_operands(alpha, B, gm, gv, n, ns, u=None):
    """The operands of the weighted kernel-gradient sum behind d L / d theta for a loss L(mean, var) of the posterior moments at ns test
    points; plain torch on any device.  alpha = Khat^-1 y (q, >= n), B = Khat^-1 K(X, X*) (q, >= n, >= ns) | None, gm =
    dL / d mean (q, ns), gv = dL / d var (q, ns) | None.  Over the stacked points Z = [X; X*] (N = n + ns), with u = B gm = dL / dy:
        Qt rows   c < ns: [ b_c^T | -e_c^T ]     ns: [ alpha^T | 0 ]      ns + 1: [ u^T | -gm^T ]
        Pt rows   c < ns: gv_c Qt[c]             ns: -1/2 Qt[ns + 1]      ns + 1: -1/2 Qt[ns]
    so that M = Pt^T Qt = sum_c gv_c q_c q_c^T - 1/2 (a u~^T + u~ a^T) is symmetric, its test x test block is diag(gv), and
        dL / d theta = sum_{i, j < N} M_ij d Khat(Z)_ij / d theta,   dL / d noise = sum_i M_ii - sum_s gv_s
    (the latent variance at a test point carries no noise: the caller subtracts).  gv None or B None: a loss of the mean alone -- only the
    last two rows (r = 2), and u must be given (u = Khat^-1 K(X, X*) gm; B is never formed).
    -> (Pt, Qt, u): Pt, Qt (q, r_pad, N_pad) of alpha's dtype, exact zeros in rows [r, r_pad) and columns [N, N_pad); u (q, n)."""
    q, dt, dev = alpha.shape[0], alpha.dtype, alpha.device
    variance = B is not None and gv is not None
    gm = gm.to(dt)
    if u is None:
        if B is None:
            raise ValueError("posterior_hyper_operands: without B, u = Khat^-1 K(X, X*) gm must be given")
        u = torch.bmm(B[:, :n, :ns], gm.unsqueeze(-1)).squeeze(-1)
    u = u[:, :n].to(dt)
    r, N = (ns + 2 if variance else 2), n + ns
    r_pad = -(-r // _OPERAND_DEPTH) * _OPERAND_DEPTH
    N_pad = -(-N // _OPERAND_BLOCK) * _OPERAND_BLOCK
    Qt = torch.zeros(q, r_pad, N_pad, dtype=dt, device=dev)
    Pt = torch.zeros(q, r_pad, N_pad, dtype=dt, device=dev)
    r0 = ns if variance else 0
    if variance:
        Qt[:, :ns, :n] = B[:, :n, :ns].transpose(1, 2)
        idx = torch.arange(ns, device=dev)
        Qt[:, idx, n + idx] = -1.0
        Pt[:, :ns] = gv.to(dt)[:, :, None] * Qt[:, :ns]
    Qt[:, r0, :n] = alpha[:, :n]
    Qt[:, r0 + 1, :n] = u
    Qt[:, r0 + 1, n:N] = -gm
    Pt[:, r0] = -0.5 * Qt[:, r0 + 1]
    Pt[:, r0 + 1] = -0.5 * Qt[:, r0]
    return Pt, Qt, u


def _vtw_buffer(ws):
    """[alpha^T ; B^T] = [z | V]^T W of the eval-mode posterior (naug_pad rows of n_pad per latent: the test points are the ROWS, as the
    operands of the weighted kernel-gradient sum want them), kept with the workspace and created on first use."""
    buf = getattr(ws, "vtw", None)
    if buf is None:
        buf = ws.vtw = torch.empty(ws.q, ws.naug_pad, ws.n_pad, dtype=ws.dtype, device=ws.device)
    return buf


hyper_grad_counters = {"b_products": 0, "weighted_grad_calls": 0, "mean_only_solves": 0}    # what the differentiable prediction launched (tests)


def _alpha_and_bt(ws, ns, variance):
    """alpha = W^T z into ws.alpha and, with `variance`, [alpha^T ; B^T] = [z | V]^T W on the tile engine, already transposed for
    posterior_hyper_operands: the product of _posterior_jacobians with its operands exchanged -- W, the lower triangle of its block of the
    factor buffer, is now the B operand (PLMC_TRI_B_LOWER skips the blocks above its diagonal, which are never written).  Row 0 is
    alpha^T, test point s stands in row 1 + s.  -> B^T (q, ns, n_pad) view | None."""
    L = _hip.lib()
    dt, q = ws.dtype, ws.q
    st = _hip.stream_ptr(ws.device)
    L.call("plmc_extract_col", dt, _hip.ptr(ws.A), ws.n_pad, ws.lda, ws.strideA, 0, _hip.ptr(ws.z), _hip.ptr(ws.quad), q, st)
    L.call("plmc_wt_matvec", dt, _hip.ptr(ws.W), ws.n_pad, ws.ldw, ws.strideW, _hip.ptr(ws.z), _hip.ptr(ws.alpha), q, st)
    if not variance:
        return None
    buf = _vtw_buffer(ws)
    nrows = int(L.cdll.plmc_pad(1 + ns))
    L.call("plmc_gemm_tn_tri", dt, 0, 2, nrows, ws.n_pad, ws.n_pad, _hip.ptr(ws.A[:, :, ws.n_pad:]), ws.lda, ws.strideA,
           _hip.ptr(ws.W), ws.ldw, ws.strideW, _hip.ptr(buf), buf.shape[2], buf.stride(0), q, st)                          # 2: PLMC_TRI_B_LOWER
    hyper_grad_counters["b_products"] += 1
    return buf[:, 1:1 + ns]


class PosteriorHyperMoments(torch.autograd.Function):
    """(mean, var) of exact_posterior as a function of the kernel's table (ell, oscale), the noise and the targets y as well as of the
    test inputs Xs (settings.posterior_hyper_grad).  Forward is _exact_posterior -- the values are those of the path
    without the setting -- on a workspace with the inverse factor, from which it keeps alpha = Khat^-1 y and, unless
    settings.predictive_variance_grad(False), B^T = K(X*, X) Khat^-1.  Backward builds the operands (posterior_hyper_operands), makes ONE
    plmc_weighted_grad call on Z = [X; Xs] and returns d ell, d oscale, d noise (less sum gvar: the latent variance carries no noise)
    and d y = u = B gmean; d Xs as PosteriorMoments returns it when Xs requires a gradient.  Mean-only: r = 2, B is never formed, u comes
    from one cross_matvec and one solve against the cached factor.  If the factorisation took a jitter, these are the gradients of the
    jittered model.  Not twice differentiable."""

    @staticmethod
    def forward(ctx, Xs, ell, oscale, noise, y, kind, X, cache, key):
        variance = settings.predictive_variance_grad.on()
        x_grad = ctx.needs_input_grad[0]
        keep = {}
        out = _exact_posterior(kind, X, ell, oscale, noise, y, Xs, False, cache, key,
                               dx=("both" if variance else "mean") if x_grad else None, keep=keep)
        mean, var = out[0], out[1]
        Jm, Jv = (out[2], out[3]) if x_grad else (None, None)
        ws = keep["ws"]
        n, ns = ws.n, Xs.shape[0]
        if x_grad:                   # _posterior_jacobians has left alpha and, with `variance`, [alpha | B] = W^T [z | V] in the workspace
            Bt = ws.wtv[:, :n, 1:1 + ns].transpose(1, 2).contiguous() if variance else None
        else:
            Bt = _alpha_and_bt(ws, ns, variance)
            Bt = None if Bt is None else Bt[:, :, :n].clone()
        alpha = ws.alpha[:, :n].clone()
        dt = y.dtype
        ctx.save_for_backward(alpha, Bt, Jm, Jv, *(_contig(t, dt) for t in (X, Xs, ell, oscale, noise)))
        ctx.kind, ctx.cache, ctx.key, ctx.variance = kind, cache, key, variance
        ctx.dtypes = tuple(None if t is None else t.dtype for t in (Xs, ell, oscale, noise, y))
        if not variance:
            ctx.mark_non_differentiable(var)
        return mean, var

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gmean, gvar):
        alpha, Bt, Jm, Jv, X, Xs, ell, oscale, noise = ctx.saved_tensors
        kind, variance = ctx.kind, ctx.variance and gvar is not None
        dt = alpha.dtype
        n, ns = X.shape[0], Xs.shape[0]
        need = ctx.needs_input_grad
        g_Xs = None
        if need[0]:
            g_Xs = (gmean.to(torch.float64)[:, :, None] * Jm).sum(0)
            if Jv is not None and variance:
                g_Xs = g_Xs + (gvar.to(torch.float64)[:, :, None] * Jv).sum(0)
            g_Xs = g_Xs.to(ctx.dtypes[0])
        g_ell = g_os = g_noise = g_y = None
        if any(need[1:5]):
            gm = gmean.to(dt).contiguous()
            u = None
            if not variance:         # u = Khat^-1 (K(X, X*) gm): one column through the cached factor
                hyper_grad_counters["mean_only_solves"] += 1
                rhs = cross_matvec(kind, X, Xs, ell, oscale, gm, n=ns)
                u = solve_cached(kind, X, ell, oscale, noise, rhs.reshape(rhs.shape[0], 1, n), ctx.cache, ctx.key)[:, :, 0]
            Pt, Qt, u = posterior_hyper_operands(alpha, Bt.transpose(1, 2) if variance else None, gm, gvar if variance else None, n, ns, u=u)
            if any(need[1:4]):
                hyper_grad_counters["weighted_grad_calls"] += 1
                t_ell, t_noise, t_os = weighted_grad(kind, torch.cat([X, Xs]), ell, oscale, Pt, Qt, n + ns)
                if variance:
                    t_noise = t_noise - gvar.to(torch.float64).sum(-1)
                g_ell = t_ell.to(ctx.dtypes[1]) if need[1] else None
                g_os = t_os.to(ctx.dtypes[2]) if need[2] and t_os is not None else None
                g_noise = t_noise.to(ctx.dtypes[3]) if need[3] else None
            g_y = u.to(ctx.dtypes[4]) if need[4] else None
        return g_Xs, g_ell, g_os, g_noise, g_y, None, None, None, None


def posterior_jacobians(kind, X, ell, oscale, noise, y, Xs, cache=None, key=None, pnoise=None):
    """(Jm, Jv), (q, ns, d) float64: d mean / dXs and d var / dXs of exact_posterior's marginal moments, read off the kernel's output --
    no autograd graph."""
    require_input_grad_kind(kind)
    with torch.no_grad():
        return _exact_posterior(kind, X, ell, oscale, noise, y, Xs, False, cache, key, dx="both", pnoise=pnoise)[2:]


def trmm_ut(ws, n, Z, shift=None):
    """shift + U^T Z against the factor in ws.A where the sweep left it (plmc_trmm_ut): Z (q, n, ns) K-major, shift (q, n) | None ->
    (q, n, ns).  Only the element-wise upper triangle of the leading n x n of the square part is read."""
    L = _hip.lib()
    q, ns = Z.shape[0], Z.shape[-1]
    Y = torch.empty(q, n, ns, dtype=ws.dtype, device=ws.device)
    L.call("plmc_trmm_ut", ws.dtype, _hip.ptr(ws.A), ws.n_pad, ws.lda, ws.strideA, n, _hip.ptr(Z), ns, ns, n * ns, _hip.ptr(shift),
           _hip.ptr(Y), ns, n * ns, q, _hip.stream_ptr(ws.device))
    return Y


def sample_lazy(kind, X, ell, oscale, noise, Z, shift=None):
    """Draws from q GP priors N(shift_i, os_i k(X, X; ell_i) + noise_i I) given base samples: factorise Khat = U^T U on the engine (any
    kernel family _kernel_call serves), then shift + U^T Z (plmc_trmm_ut) -- the `MultivariateNormal(mean, kernel(X)).sample()` the
    reference's synthetic study begins with (experiments.py:150-151).  Z (q, n, ns), shift (q, n) | None -> (draws (q, n, ns), jitter).
    noise None (the reference's own call, a noise-free prior): settings.cholesky_jitter stands on the diagonal from the first attempt,
    and the fp32 sweep is given no eigenvalue bound -- a jitter of 1e-6 is not one the two-plane fp16 scaling should be fed.  Further
    rungs come from the one ladder (_pivot.walk).  `jitter` is everything that was added to the caller's diagonal.  No gradient."""
    _hip.require_device(X, ell, Z)
    L = _hip.lib()
    dt, dev = Z.dtype, Z.device
    q, n = Z.shape[0], Z.shape[1]
    with torch.no_grad():
        Xc, ellc, osc, nzc, Zc, sh = (_contig(t, dt) for t in (X, ell, oscale, noise, Z, shift))
        _check_kernel_shape(L, ellc, kind)
        ws = get_workspace(n, q, 0, dt, dev, False)
        base = 0.0
        if nzc is None:
            base = settings.cholesky_jitter.value(dt)
            nzc = torch.full((q,), base, dtype=dt, device=dev)
        else:
            nzc = nzc.reshape(-1)
        jitter = base + factorize_checked(kind, Xc, ellc, osc, nzc, None, ws, eig_lo=noise is not None)
        return trmm_ut(ws, n, Zc, sh), jitter


def mix_posterior(mean_lat, var_lat, Ht, eps=0.0):
    """Task-space moments of the projected model (projected_lmc.py:1144, :1152): mean (ns, p) = mean_lat^T Ht,
    var (ns, p) = var_lat^T Ht^2 + eps, from latent moments (q, ns) and the mixing matrix Ht (q, p) -- plmc_mix_posterior."""
    _hip.require_device(mean_lat, var_lat, Ht)
    L = _hip.lib()
    dt, dev = mean_lat.dtype, mean_lat.device
    q, ns = mean_lat.shape
    p = Ht.shape[1]
    ml, vl, H = (_contig(t, dt) for t in (mean_lat, var_lat, Ht))
    mean = torch.empty(ns, p, dtype=dt, device=dev)
    var = torch.empty(ns, p, dtype=dt, device=dev)
    L.call("plmc_mix_posterior", dt, _hip.ptr(ml), _hip.ptr(vl), _hip.ptr(H), q, ns, p, float(eps), _hip.ptr(mean), _hip.ptr(var),
           _hip.stream_ptr(dev))
    return mean, var


class MixPosterior(torch.autograd.Function):
    """mix_posterior as a function of the latent moments (the mixing is linear in them): the values are plmc_mix_posterior's, bit for
    bit; backward is gmean Ht^T and gvar (Ht^2)^T.  eps is a constant, and so is Ht unless it requires a gradient
    (settings.posterior_hyper_grad): then gHt = mean_lat gmean + 2 Ht o (var_lat gvar), plain torch."""

    @staticmethod
    def forward(ctx, mean_lat, var_lat, Ht, eps):
        mean, var = mix_posterior(mean_lat, var_lat, Ht, eps)
        h_grad = ctx.needs_input_grad[2]
        ctx.save_for_backward(Ht.detach().to(mean_lat.dtype), *((mean_lat.detach(), var_lat.detach()) if h_grad else ()))
        ctx.h_dtype = Ht.dtype
        if not (ctx.needs_input_grad[1] or h_grad):
            ctx.mark_non_differentiable(var)
        return mean, var

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gmean, gvar):
        Ht = ctx.saved_tensors[0]
        g_mean = (gmean @ Ht.T).T if ctx.needs_input_grad[0] else None
        g_var = (gvar @ (Ht * Ht).T).T if ctx.needs_input_grad[1] and gvar is not None else None
        g_Ht = None
        if ctx.needs_input_grad[2]:
            mean_lat, var_lat = ctx.saved_tensors[1:]
            g_Ht = mean_lat @ gmean
            if gvar is not None:
                g_Ht = g_Ht + 2.0 * Ht * (var_lat @ gvar)
            g_Ht = g_Ht.to(ctx.h_dtype)
        return g_mean, g_var, g_Ht, None


def dense_cross(kind, X1, X2, ell, oscale):
    """Dense k(X1, X2) per latent via the cross-assembly kernel: (q, n1, n2).  ell, oscale: (q, d), (q) or a component table."""
    L = _hip.lib()
    dt, dev = X1.dtype, X1.device
    q = ell.shape[0]
    n1, n2, d = X1.shape[0], X2.shape[0], X1.shape[1]
    out = torch.empty(q, n1, n2, dtype=dt, device=dev)
    _kernel_call(L, "plmc_assemble_cross", dt, (kind_code(kind), _hip.ptr(X1.contiguous()), n1, _hip.ptr(X2.contiguous()), n2, d),
                 ell.contiguous(), (_hip.ptr(None if oscale is None else oscale.contiguous()), _hip.ptr(out),
                 n2, n1 * n2, 0, n1, q, _hip.stream_ptr(dev)))
    return out
