"""Dense fp64 reference of the weighted kernel-gradient sum (include/plmc.h, plmc_weighted_grad*):
    G[l][t] = sum_{i <= j < N} c_ij (At_l^T Bt_l)_ij d Khat_l(Z)_ij / d theta_t ,   c_ii = 1, c_ij = 2,   Khat = K(Z, Z) + noise I,
by autograd of sum_ij c_ij M_ij Khat_ij on leaf hyper-parameters, and the sum of absolute terms
    S[l][t] = sum_{i <= j < N} c_ij (|At_l|^T |Bt_l|)_ij |d Khat_l(Z)_ij / d theta_t|
behind each output (one forward-mode pass per table entry).  TEST INFRASTRUCTURE ONLY: plain torch on the CPU, nothing from the package.
The dense kernels are those the test tree already has: oracle.gp_math.kernel_matrix (stationary kinds, their additive tables, spline) and
the kernels of _sm_dense, _periodic_dense, _rq_dense, _lper_dense, _dot_dense and _sum_dense, driven by a table in the layout
projectedlmc._engine takes (kind, ell, oscale); the families' values are _input_grad_dense.problem's plus spline, a dot-product kernel and a
mixed sum."""
import math

import torch

import _dot_dense
import _input_grad_dense as igd
import _lper_dense
import _periodic_dense
import _posterior_dx_dense as pdd
import _rq_dense
import _sm_dense
import _sum_dense
from oracle import gp_math as gm

NB, BK = 128, 16
# fp32 bound of the GPU tests, |G_t - ref_t| <= kappa (r + d + 4) 2^-24 S_t, per shape class: the next power of two above twice the worst
# ratio measured on the GPU over that class's cases of tests/test_gpu_weighted_grad.py against this reference
# (profiles/weighted_grad_accuracy.md).  At N = 2 an output is ONE term and the ratio is the relative error of a single derivative
# evaluation (worst 2.48); from N = 128 on it is the error of a sum over the tile product (worst 9.4e-2), and the bound there is the one
# with power against a product formed in lower precision.
KAPPA_SINGLE_TERM, KAPPA_SUM = 8.0, 0.25


def kappa(N):
    return KAPPA_SINGLE_TERM if N <= 2 else KAPPA_SUM
FAMILIES = igd.FAMILIES + ("spline", "poly2", "linear", "sum_mixed", "sum_single")
SUM_MEMBERS = ("matern52", "periodic", "rq")


def _f32(t):
    return None if t is None else t.float().double()


def problem(family, d, q, seed, use_os=True):
    """kind, ell, oscale (fp64, fp32-representable) of `family` as projectedlmc._engine takes them, in an object with .kind, .ell, .oscale."""
    if family in igd.FAMILIES:
        return pdd.problem(family, d, q, seed, use_os)
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    p = igd.Problem()
    p.family, p.d, p.q = family, d, q
    osc = _f32(0.5 + rnd(q)) if use_os else None
    if family == "spline":
        p.kind, p.ell, p.oscale = "spline", torch.ones(q, d, dtype=torch.float64), osc
    elif family in ("poly2", "linear"):
        v, c = _f32((0.3 + rnd(q, d)) / d), _f32(0.2 + rnd(q))
        p.kind, p.ell, p.oscale = family, torch.cat([v, c[:, None]], 1), osc
    elif family in ("sum_mixed", "sum_single"):            # sum_single: a sum of ONE member, the library's route through that member's own kernels
        members = SUM_MEMBERS if family == "sum_mixed" else ("periodic",)
        table, os_ = _sum_dense.make_table(members, d, q, seed)
        p.kind, p.ell, p.oscale = "sum(%s)" % ",".join(members), _f32(table), _f32(os_)
    else:
        raise ValueError(family)
    return p


def dense_kernel(kind, ell, oscale):
    """K(Xa, Xb) -> (q, na, nb) of the table (kind, ell, oscale) in the engine's layout; differentiable in ell and oscale."""
    if kind.startswith("sum("):
        members = kind[4:-1].split(",")
        d = (ell.shape[-1] - 1) // 3
        mask = torch.stack([_sum_dense.owned(m, d) for m in members])[None].expand_as(ell)
        table = torch.where(mask, ell, torch.ones_like(ell))            # the slots a member does not own never enter the graph
        return lambda Xa, Xb: _sum_dense.sum_kernel(members, Xa, Xb, table, oscale)
    if kind in ("linear",) or kind.startswith("poly"):
        P = 1 if kind == "linear" else int(kind[4:])
        d = ell.shape[1] - 1
        return lambda Xa, Xb: _dot_dense.dot_kernel(Xa, Xb, ell[:, :d], ell[:, d], P, oscale)
    if kind == "rq":
        d = ell.shape[1] - 1
        return lambda Xa, Xb: _rq_dense.rq_kernel(Xa, Xb, ell[:, :d], ell[:, d], oscale)
    if kind == "periodic":
        return lambda Xa, Xb: _periodic_dense.per_kernel(Xa, Xb, ell[:, 0], ell[:, 1], oscale)
    if kind == "locally_periodic":
        return lambda Xa, Xb: _lper_dense.lper_kernel(Xa, Xb, ell[:, 0], ell[:, 1], ell[:, 2], oscale)
    if kind == "sm":
        wt = torch.ones(ell.shape[0], ell.shape[2], dtype=ell.dtype) if oscale is None else oscale
        return lambda Xa, Xb: _sm_dense.sm_kernel(Xa, Xb, ell[:, 0], ell[:, 1], wt)
    if kind == "spline":
        return lambda Xa, Xb: gm.kernel_matrix("spline", Xa, Xb, ell, oscale)
    okind, nu = igd.STATIONARY[kind]
    if ell.dim() == 3:                                                   # additive table: +inf switches a dimension off (x / inf = 0)
        def K(Xa, Xb):
            out = 0
            for g in range(ell.shape[1]):
                out = out + gm.kernel_matrix(okind, Xa, Xb, ell[:, g], None if oscale is None else oscale[:, g], nu)
            return out
        return K
    return lambda Xa, Xb: gm.kernel_matrix(okind, Xa, Xb, ell, oscale, nu)


def khat(kind, ell, oscale, noise, Z):
    return dense_kernel(kind, ell, oscale)(Z, Z) + noise[:, None, None] * torch.eye(Z.shape[0], dtype=torch.float64)


def tri_weights(N, mutate=None):
    """c (N, N): 1 on the diagonal, 2 above, 0 below.  mutate: "diag_twice" (c_ii = 2) or "lower" (the lower triangle instead of the
    upper one) -- the seeded mistakes the host test must catch."""
    up = torch.triu(torch.ones(N, N, dtype=torch.float64), 1)
    c = 2.0 * up + torch.eye(N, dtype=torch.float64)
    if mutate == "diag_twice":
        c = c + torch.eye(N, dtype=torch.float64)
    elif mutate == "lower":
        c = c.T.contiguous()
    return c


def weighted_grad_ref(kind, ell, oscale, noise, Z, At, Bt, mutate=None, terms=True):
    """((g_ell, g_noise, g_os | None), (s_ell, s_noise, s_os | None)): the weighted sum and the sums of absolute terms, shaped like the
    table; At, Bt (q, r, >= N) fp64, of which the first N columns enter.  terms=False: the second tuple is None."""
    q, N = At.shape[0], Z.shape[0]
    A, B = At[:, :, :N].double(), Bt[:, :, :N].double()
    c = tri_weights(N, mutate)
    Wm = c * (A.transpose(1, 2) @ B)
    leaves = [ell.detach().clone().requires_grad_(True), noise.detach().clone().requires_grad_(True)]
    if oscale is not None:
        leaves.append(oscale.detach().clone().requires_grad_(True))
    fn = lambda e, nz, *o: khat(kind, e, o[0] if o else None, nz, Z)
    grads = torch.autograd.grad((Wm * fn(*leaves)).sum(), leaves, allow_unused=True)
    grads = [torch.zeros_like(l) if g is None else g for g, l in zip(grads, leaves)]
    if kind.startswith("sum("):                                          # (the NaN of a slot its member does not own: exactly 0)
        grads[0] = torch.nan_to_num(grads[0], nan=0.0)
    G = (grads[0], grads[1], grads[2] if oscale is not None else None)
    if not terms:
        return G, None
    Wa = c * (A.abs().transpose(1, 2) @ B.abs())
    base = [l.detach() for l in leaves]
    S = []
    for k, leaf in enumerate(base):
        flat = torch.zeros(q, leaf[0].numel(), dtype=torch.float64)
        for t in range(leaf[0].numel()):
            tang = [torch.zeros_like(b) for b in base]
            tang[k].reshape(q, -1)[:, t] = 1.0
            dK = torch.func.jvp(fn, tuple(base), tuple(tang))[1]
            flat[:, t] = (Wa * torch.nan_to_num(dK, nan=0.0).abs()).sum((1, 2))
        S.append(flat.reshape(leaf.shape))
    return G, (S[0], S[1], S[2] if oscale is not None else None)


def formula_in_float32(kind, ell, oscale, noise, Z, At, Bt):
    """The flat table G of weighted_grad_ref with the dense formula itself evaluated in IEEE float32 by torch on the host (the weights
    c_ij M_ij from the fp64 product, rounded once): what the number format alone does to the sum.  Where an output is ONE term (N = 2)
    and a factor of the derivative nearly vanishes -- sin at a zero, a difference of nearly equal numbers -- float32 misses the
    S-relative bound by itself; such inputs measure the conditioning of the formula, not the kernel under test, and the GPU test draws
    its inputs where this evaluation meets the bound with KAPPA = 1."""
    N = Z.shape[0]
    f = lambda t: None if t is None else t.detach().float()
    Wm = (tri_weights(N) * (At[:, :, :N].double().transpose(1, 2) @ Bt[:, :, :N].double())).float()
    leaves = [f(ell).requires_grad_(True), f(noise).requires_grad_(True)] + ([] if oscale is None else [f(oscale).requires_grad_(True)])
    Kh = dense_kernel(kind, leaves[0], leaves[2] if oscale is not None else None)(f(Z), f(Z)) + leaves[1][:, None, None] * torch.eye(N)
    grads = torch.autograd.grad((Wm * Kh).sum(), leaves, allow_unused=True)
    grads = [torch.zeros_like(l) if g is None else torch.nan_to_num(g, nan=0.0) for g, l in zip(grads, leaves)]
    return flat_table((grads[0].double(), grads[1].double(), grads[2].double() if oscale is not None else None))


def flat_table(parts):
    """[d ell | d noise | d oscale] per latent, (q, width): the layout of the library's gradient table (without the oscale slots when the
    table has none)."""
    g_ell, g_noise, g_os = parts
    cols = [g_ell.reshape(g_ell.shape[0], -1), g_noise[:, None]]
    if g_os is not None:
        cols.append(g_os.reshape(g_os.shape[0], -1))
    return torch.cat(cols, 1)


def random_operands(r, N, q, seed, symmetric=True):
    """At, Bt (q, r, N), fp32-representable.  symmetric: Bt rows are At's, scaled per row and paired (row 2 k with 2 k + 1 exchanged and
    both scaled alike), so that At^T Bt is symmetric without being a Gram matrix -- the shape of the posterior's operands."""
    g = torch.Generator().manual_seed(seed + 5000)
    At = _f32(torch.randn(q, r, N, generator=g, dtype=torch.float64) / math.sqrt(r))
    if not symmetric:
        return At, _f32(torch.randn(q, r, N, generator=g, dtype=torch.float64))
    Bt = torch.empty_like(At)
    w = _f32(torch.randn(q, r, generator=g, dtype=torch.float64))
    for k in range(0, r - 1, 2):
        Bt[:, k], Bt[:, k + 1] = w[:, k, None] * At[:, k + 1], w[:, k, None] * At[:, k]
    if r % 2:
        Bt[:, r - 1] = w[:, r - 1, None] * At[:, r - 1]
    return At, _f32(Bt)


def padded(At, Bt, dtype, ld_extra=0, stride_extra=0, fill=float("nan")):
    """The operands as the library takes them: (q, r_pad, ld) views of `dtype` with exact zeros in rows [r, r_pad) and columns [N, N_pad),
    and `fill` (NaN) wherever the contract says nothing is read -- the columns [N_pad, ld) and `stride_extra` rows behind every latent's
    r_pad rows (the last latent's included).  Both views have the same strides."""
    q, r, N = At.shape
    r_pad, N_pad = -(-r // BK) * BK, -(-N // NB) * NB
    out = []
    for M in (At, Bt):
        buf = torch.full((q, r_pad + stride_extra, N_pad + ld_extra), fill, dtype=dtype)
        buf[:, :r_pad, :N_pad] = 0
        buf[:, :r, :N] = M.to(dtype)
        out.append(buf)
    return out[0], out[1], r_pad, N_pad
