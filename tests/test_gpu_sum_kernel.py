"""Sums of different kernel families (kind "sum(...)", `k1 + k2`) on the batched exact engine: the `_sum` entry points per element, a
one-member sum against its family's own entry points (bit patterns), the log-prob and every entry of the gradient table (fp64; fp32 on
every arithmetic of the sweep, fused and two-call assembly), switched-off dimensions, the leave-one-out objective, the models
(`ExactGPModel` single and batched, `ProjectedGPModel`, shards, the prediction cache), draws and the argument errors.

Reference values: the dense fp64 formulas of tests/_sum_dense.py (torch CPU, autograd).  Shapes: n = 130 (two blocks of 128, ragged
edge) and n = 257 (3 x 3 tiles), d in {1, 3, 8} (the compile-time capacities 1, 4, 8), q in {1, 3} with different parameters per latent.
The member sets put every family in the first and in a later slot, two members of one non-ARD family and a four-member sum.  Every
table slot a member does not own holds NaN in every library-level test.  fp64 tolerances are those of tests/test_gpu_lper_kernel.py
(named beside each use); the fp32 per-element bound is the sum of the members' derived bounds (_sum_dense.fp32_bound)."""
import copy
import json
import math
import os
import warnings

import pytest
import torch

import _factor_ref as fr
import _sum_dense as sd
from _oracle_params import oracle_dict
from oracle import gp_math as gm
from oracle import projected as pj
from _bridge import perturb_

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
INF = float("inf")
SETS = [("rbf", "periodic"), ("matern52", "locally_periodic", "rq"), ("periodic", "periodic"),
        ("rq", "matern12", "rbf", "locally_periodic"), ("locally_periodic", "matern32")]


def kind_of(members):
    return "sum(%s)" % ",".join(members)


@pytest.fixture(scope="module")
def eng():
    import types
    from projectedlmc import _hip, _engine, settings
    assert torch.cuda.is_available()
    return types.SimpleNamespace(hip=_hip, exact=_engine, settings=settings)


@pytest.fixture(scope="module")
def plmc():
    import projectedlmc
    assert torch.cuda.is_available()
    return projectedlmc


def _problem(members, n, d, q, seed, ns=1, off=None):
    """Inputs on [0, span]^d (span 10, 3, 2 for d = 1, 3, 8: lengthscales of order 1 leave the covariance neither flat nor diagonal),
    the table of _sum_dense.make_table (NaN in unowned slots), noise in [0.05, 0.2]."""
    g = torch.Generator().manual_seed(seed)
    span = {1: 10.0, 3: 3.0, 8: 2.0}[d]
    X, Xs = span * torch.rand(n, d, generator=g, dtype=torch.float64), span * torch.rand(ns, d, generator=g, dtype=torch.float64)
    y = torch.randn(q, n, generator=g, dtype=torch.float64)
    table, os_ = sd.make_table(members, d, q, seed + 1, off=off)
    noise = 0.05 + 0.15 * torch.rand(q, generator=g, dtype=torch.float64)
    return X, Xs, y, table, os_, noise


def _fam(eng, members):
    import ctypes
    codes = [eng.hip.FAM[m] for m in members]
    return (ctypes.c_int * len(codes))(*codes)


def _assemble(eng, members, X, table, os_, noise, dt, fill=0.0):
    """plmc_assemble_sum_*: the whole factor buffer's square part (q, n_pad, n_pad) on the host, pre-filled with `fill`."""
    import ctypes
    hip = eng.hip
    f = lambda t: None if t is None else t.to(DEV, dt).contiguous()
    n, d = X.shape
    q = table.shape[0]
    ws = eng.exact.Workspace(n, q, 0, dt, DEV, with_inverse=False)
    ws.A.fill_(fill)
    Xd, t_, o_, nz = f(X), f(table), f(os_), f(noise)
    fam = _fam(eng, members)
    hip.lib().call("plmc_assemble_sum", dt, hip.ptr(Xd), n, d, len(members), ctypes.addressof(fam), hip.ptr(t_), hip.ptr(o_), hip.ptr(nz),
                   hip.ptr(ws.A), ws.lda, ws.strideA, q, hip.stream_ptr(DEV))
    torch.cuda.synchronize()
    return ws.A[:, :, :ws.n_pad].cpu().double()


def _cross(eng, members, X, Xs, table, os_, dt):
    f = lambda t: None if t is None else t.to(DEV, dt).contiguous()
    K = eng.exact.dense_cross(kind_of(members), f(X), f(Xs), f(table), f(os_))
    torch.cuda.synchronize()
    return K.cpu().double()


# ------------------------------------------------------------------------------------------------ 1. per element
CASES = [(SETS[0], 130, 1, 1), (SETS[1], 257, 3, 3), (SETS[2], 257, 1, 3), (SETS[3], 130, 8, 3), (SETS[4], 257, 8, 1), (SETS[3], 257, 1, 3)]


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("members,n,d,q", CASES, ids=["+".join(c[0]) + "-%d-%d-%d" % c[1:] for c in CASES])
def test_assembly_and_cross_against_the_dense_formula(eng, members, n, d, q, dt):
    """plmc_assemble_sum / plmc_assemble_cross_sum.  fp64: rtol 1e-12 per element.  fp32: _sum_dense.fp32_bound per element against
    the fp64 formula at the fp32-rounded inputs, diagonal (sum_g os_g + noise) included.  Padding rows are the identity; nothing below
    the block diagonal is written (the buffer is pre-filled with NaN)."""
    assert d <= eng.hip.lib().cdll.plmc_sum_max_dim() and len(members) <= eng.hip.lib().cdll.plmc_sum_max_components()
    ns = 70
    X, Xs, _, table, os_, nz = _problem(members, n, d, q, seed=10 * d + n, ns=ns)
    if dt == torch.float32:
        X, Xs, table, os_, nz = (t.float().double() for t in (X, Xs, table, os_, nz))
    ref = sd.khat(members, X, table, os_, nz)
    refx = sd.sum_kernel(members, X, Xs, table, os_)
    A = _assemble(eng, members, X, table, os_, nz, dt, fill=float("nan"))
    got, gotx = A[:, :n, :n], _cross(eng, members, X, Xs, table, os_, dt)
    up = torch.triu(torch.ones(n, n, dtype=torch.bool))
    for name, a, b in (("assemble", got[:, up], ref[:, up]), ("cross", gotx, refx)):
        err = (a - b).abs()
        if dt == torch.float64:
            print("%s f64 %s n=%d d=%d q=%d: max rel err %.3g" % (name, "+".join(members), n, d, q, float((err / b.abs()).max())))
            assert bool((err <= 1e-12 * b.abs()).all()), name
        else:
            bound = sd.fp32_bound(members, d, table, os_)
            bound = bound[:, :, 0] if a.dim() == 2 else bound
            print("%s f32 %s n=%d d=%d q=%d: max err / bound %.3g" % (name, "+".join(members), n, d, q, float((err / bound).max())))
            assert bool((err <= bound).all()), name
    # padding: identity; blocks below the block diagonal: untouched
    NB, n_pad = 128, A.shape[1]
    for ib in range(n_pad // NB):
        for jb in range(n_pad // NB):
            blk = A[:, ib * NB:(ib + 1) * NB, jb * NB:(jb + 1) * NB]
            if jb < ib:
                assert bool(torch.isnan(blk).all()), (ib, jb)
    pad = A[:, n:, n:]
    assert torch.equal(torch.triu(pad), torch.eye(n_pad - n, dtype=torch.float64).expand_as(pad))
    assert bool((torch.triu(A[:, :n, n:]) == 0).all())


# ------------------------------------------------------------------------------------------------ 2. one component is the family itself
def _family_args(member, table, os_):
    """(kind, table, oscale) of the single-family engine call for a one-member sum's record (q, 1, 3 d + 1)."""
    d = (table.shape[-1] - 1) // 3
    rec = table[:, 0]
    ell, per, lam, alpha = rec[:, :d], rec[:, d:2 * d], rec[:, 2 * d:3 * d], rec[:, 3 * d:]
    if member == "periodic":
        return member, torch.stack([ell, per], 1), os_[:, 0]
    if member == "locally_periodic":
        return member, torch.stack([ell, per, lam], 1), os_[:, 0]
    if member == "rq":
        return member, torch.cat([ell, alpha], 1), os_[:, 0]
    return member, ell.contiguous(), os_[:, 0]


def _relay(member, g, d):
    """The family's gradient of its table, re-laid into the sum's record layout (q, 1, 3 d + 1), zeros elsewhere."""
    q = g.shape[0]
    out = torch.zeros(q, 1, 3 * d + 1, dtype=g.dtype)
    if member == "periodic":
        out[:, 0, :2 * d] = g.reshape(q, 2 * d)
    elif member == "locally_periodic":
        out[:, 0, :3 * d] = g.reshape(q, 3 * d)
    elif member == "rq":
        out[:, 0, :d], out[:, 0, 3 * d] = g[:, :d], g[:, d]
    else:
        out[:, 0, :d] = g
    return out


def _logprob(eng, kind, X, y, table, os_, nz, dt, fn=None, wt=None):
    f = lambda t: t.to(DEV, dt)
    tb = f(table).requires_grad_()
    leaves = [None if os_ is None else f(os_).requires_grad_(), f(nz).requires_grad_(), f(y).requires_grad_()]
    fn = eng.exact.exact_latent_log_prob if fn is None else fn
    lp = fn(kind, f(X), tb, leaves[0], leaves[1], leaves[2])
    (lp if wt is None else lp * f(wt)).sum().backward()
    torch.cuda.synchronize()
    return [lp.detach().cpu(), tb.grad.cpu()] + [None if t is None else t.grad.cpu() for t in leaves]


def _factor(eng, kind, X, y, table, os_, nz, dt):
    f = lambda t: t.to(DEV, dt).contiguous()
    n, q = X.shape[0], table.shape[0]
    ws = eng.exact.Workspace(n, q, 1, dt, DEV, with_inverse=True)
    ws.A.zero_()
    ws.Vd.zero_()
    eng.exact.factorize(kind, f(X), f(table), f(os_), f(nz), f(y).reshape(q, 1, n), ws)
    torch.cuda.synchronize()
    return ws.A.cpu(), ws.logdet.cpu()


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("member", ["matern52", "periodic", "rq", "locally_periodic"])
def test_one_component_is_the_family_itself(eng, member, dt):
    """n = 130, d = 3, q = 3.  A sum of one member against that family's own entry points: K, the factor buffer with the inverse factor,
    log det, the log-prob and the leave-one-out value (ExactLooLogProb) with every gradient of both (the family's table gradient re-laid
    into the record) are equal as bit patterns; the unowned slots of the gradients are exactly 0.
    A two-member sum whose second output scale is 0, with a rational-quadratic and with a periodic second member, gives the first
    family's K, fp64 and fp32: 0 x value adds exactly 0, so what is left between the two is the rounding of the first member's value on
    its two routes.  A stationary ARD member of a sum scales the raw difference x - x' (formed once per element for all members) where the
    plain kernel's own assembly scales the inputs; the other members run the source of their family's value function inside the loop over
    components, where the compiler is free to fuse other multiply-adds than in the family's kernel (measured on an MI355X: bit-equal in
    fp64 and for the rational-quadratic member in fp32, up to 1.5e-7, a few units in the last place, for the periodic and the locally
    periodic member in fp32).  fp64: rtol 1e-13, as for the ARD members.
    fp32: each route is within the member's per-element bound of the fp64 formula (_sum_dense.fp32_bound of the one-member sum, the
    bound test 1 applies to either), so the two are within twice that bound of each other."""
    n, d, q = 130, 3, 3
    members = (member,)
    X, _, y, table, os_, nz = _problem(members, n, d, q, seed=5)
    kind, ftab, fos = _family_args(member, table, os_)
    f = lambda t: t.to(DEV, dt).contiguous()
    K_sum = _assemble(eng, members, X, table, os_, nz, dt)[:, :n, :n]
    ws = eng.exact.Workspace(n, q, 0, dt, DEV, with_inverse=False)
    ws.A.zero_()
    hip = eng.hip
    Xd, ft, fo, nzd = f(X), f(ftab), f(fos), f(nz)
    eng.exact._kernel_call(hip.lib(), "plmc_assemble", dt, (eng.exact.kind_code(kind), hip.ptr(Xd), n, d), ft,
                           (hip.ptr(fo), hip.ptr(nzd), hip.ptr(ws.A), ws.lda, ws.strideA, q, hip.stream_ptr(DEV)))
    torch.cuda.synchronize()
    K_fam = ws.A[:, :n, :n].cpu().double()
    assert torch.equal(K_sum, K_fam)
    A1, ld1 = _factor(eng, kind_of(members), X, y, table, os_, nz, dt)
    A2, ld2 = _factor(eng, kind, X, y, ftab, fos, nz, dt)
    assert torch.equal(A1, A2) and torch.equal(ld1, ld2)
    got = _logprob(eng, kind_of(members), X, y, table, os_, nz, dt)
    fam = _logprob(eng, kind, X, y, ftab, fos, nz, dt)
    assert torch.equal(got[0], fam[0])
    assert torch.equal(got[1], _relay(member, fam[1], d))
    assert torch.equal(got[2][:, 0], fam[2]) and torch.equal(got[3], fam[3]) and torch.equal(got[4], fam[4])
    assert bool((got[1][:, 0, ~sd.owned(member, d)] == 0).all())
    loo = eng.exact.exact_loo_log_prob
    got = _logprob(eng, kind_of(members), X, y, table, os_, nz, dt, fn=loo)
    fam = _logprob(eng, kind, X, y, ftab, fos, nz, dt, fn=loo)
    assert torch.equal(got[0], fam[0])
    assert torch.equal(got[1], _relay(member, fam[1], d))
    assert torch.equal(got[2][:, 0], fam[2]) and torch.equal(got[3], fam[3]) and torch.equal(got[4], fam[4])
    assert bool((got[1][:, 0, ~sd.owned(member, d)] == 0).all())
    for second in ("rq", "periodic"):
        two = (member, second)
        t2, o2 = sd.make_table(two, d, q, seed=9)
        t2[:, 0] = table[:, 0]
        o2[:, 0], o2[:, 1] = os_[:, 0], 0.0
        K_two = _assemble(eng, two, X, t2, o2, nz, dt)[:, :n, :n]
        a, b = torch.triu(K_two), torch.triu(K_fam)
        print("%s + 0 x %s: max |K_two - K_family| %.3g" % (member, second, float((a - b).abs().max())))
        if dt == torch.float64:
            assert torch.allclose(a, b, rtol=1e-13, atol=0), second
        else:
            assert bool(((a - b).abs() <= 2 * sd.fp32_bound(members, d, table.float().double(), os_.float().double())).all()), second


# ------------------------------------------------------------------------------------------------ 3. log-prob and every gradient, fp64
GCASES = [(SETS[1], 257, 1, 3, None), (SETS[3], 130, 3, 1, {1: [0], 3: [1]}), (SETS[0], 257, 8, 3, {1: [2, 5]}), (SETS[2], 130, 3, 3, None),
          (SETS[4], 130, 1, 1, None)]


def _check_grads(members, d, got, ref_val, ref_tab, off, rtol, atol):
    q, G = got[1].shape[:2]
    rec = 3 * d + 1
    gt = ref_tab[:, :G * rec].reshape(q, G, rec)
    gn, go = ref_tab[:, G * rec], ref_tab[:, G * rec + 1:]
    for g, m in enumerate(members):
        own = sd.owned(m, d)
        assert bool((got[1][:, g, ~own] == 0).all()), ("unowned slots", m)
        a, b = got[1][:, g, own].double(), gt[:, g, own]
        print("d/d record of %s: max abs err %.3g" % (m, float((a - b).abs().max())))
        assert torch.allclose(a, b, rtol=rtol, atol=atol), (m, float((a - b).abs().max()))
    for g, dims in (off or {}).items():
        for k in dims:
            slots = [k, d + k] + ([2 * d + k] if members[g] == "locally_periodic" else [])
            if members[g] not in ("periodic", "locally_periodic"):
                slots = [k]
            assert bool((got[1][:, g, slots] == 0).all()), ("switched-off dimension", members[g], k, got[1][:, g, slots])
    if got[2] is not None:
        assert torch.allclose(got[2].double(), go, rtol=rtol, atol=atol), "oscale"
    assert torch.allclose(got[3].double(), gn, rtol=rtol, atol=atol), "noise"


@pytest.mark.parametrize("members,n,d,q,off", GCASES, ids=["+".join(c[0]) + "-%d-%d-%d" % c[1:4] for c in GCASES])
def test_logprob_and_every_gradient_fp64(eng, members, n, d, q, off):
    """Tolerances of the test of the same name in tests/test_gpu_lper_kernel.py: log-prob rtol 1e-10; gradients rtol 1e-7 / atol 1e-9.
    Unowned slots of the gradient table are exactly 0.0; a switched-off dimension (+inf) has exactly-0 gradients, its period's included."""
    X, _, y, table, os_, nz = _problem(members, n, d, q, seed=n + d, off=off)
    val, tab = sd.grads(sd.sum_logprob, members, X, y, table, os_, nz)
    got = _logprob(eng, kind_of(members), X, y, table, os_, nz, torch.float64)
    assert torch.allclose(got[0].double(), val, rtol=1e-10, atol=0), (got[0], val)
    _check_grads(members, d, got, val, tab, off, 1e-7, 1e-9)


def test_logprob_without_output_scales_fp64(eng):
    """oscale NULL: unit output scales, no gradient for them."""
    members, n, d, q = SETS[1], 130, 3, 3
    X, _, y, table, _, nz = _problem(members, n, d, q, seed=8)
    val, tab = sd.grads(sd.sum_logprob, members, X, y, table, None, nz)
    got = _logprob(eng, kind_of(members), X, y, table, None, nz, torch.float64)
    assert torch.allclose(got[0].double(), val, rtol=1e-10, atol=0)
    _check_grads(members, d, got, val, tab, None, 1e-7, 1e-9)


# ------------------------------------------------------------------------------------------------ 4. fp32 on every arithmetic
@pytest.mark.parametrize("d", [1, 3])
def test_logprob_fp32_on_every_arithmetic_and_fused_against_two_call_assembly(eng, monkeypatch, d):
    """n = 257, q = 3, fp32 with PLMC_SPLIT unset, 0 and 3, members matern52 + locally_periodic + rq; the tolerances of the test of the same
    name in tests/test_gpu_lper_kernel.py: value 1e-4 relative, gradients 2e-3 of the largest entry.  The fused plmc_factorize_sum_ex and
    PLMC_FUSED_ASSEMBLE=0 give the same factor buffer, log det, value and gradients as bit patterns.  The problem is
    _sum_dense.fp32_problem(d): noise in [0.05, 0.2], sum of output scales of order 1, lengthscales of order 1 on inputs in [0, 10]; the dense
    reference evaluated in fp32 on the CPU stays within half of these tolerances there
    (tests/test_sum_kernel.py::test_the_fp32_problem_leaves_half_of_the_fp32_tolerances)."""
    members = SETS[1]
    X, y, table, os_, nz = sd.fp32_problem(members, d)
    q, n = y.shape
    val, tab = sd.grads(sd.sum_logprob, members, X, y, table, os_, nz)
    monkeypatch.delenv("PLMC_SPLIT", raising=False)
    monkeypatch.delenv("PLMC_FUSED_ASSEMBLE", raising=False)
    eng.hip.lib().cdll.plmc_dev_reload_knobs()
    G, rec = len(members), 3 * d + 1
    mask = torch.stack([sd.owned(m, d) for m in members])[None].expand(q, G, rec)
    gt = tab[:, :G * rec].reshape(q, G, rec)

    def check(tag):
        got = _logprob(eng, kind_of(members), X, y, table, os_, nz, torch.float32)
        monkeypatch.setenv("PLMC_FUSED_ASSEMBLE", "0")
        two = _logprob(eng, kind_of(members), X, y, table, os_, nz, torch.float32)
        A2, ld2 = _factor(eng, kind_of(members), X, y, table, os_, nz, torch.float32)
        monkeypatch.delenv("PLMC_FUSED_ASSEMBLE")
        A1, ld1 = _factor(eng, kind_of(members), X, y, table, os_, nz, torch.float32)
        for a, b in zip(got, two):
            assert torch.equal(a, b), tag
        assert torch.equal(A1, A2) and torch.equal(ld1, ld2), tag
        e = float(((got[0].double() - val) / val).abs().max())
        print("PLMC_SPLIT %s: log-prob rel err %.3g" % (tag, e))
        assert e < 1e-4, (tag, e)
        assert bool((got[1][~mask] == 0).all()), tag
        for name, a, b in (("table", got[1].double()[mask], gt[mask]), ("oscale", got[2].double(), tab[:, G * rec + 1:]),
                           ("noise", got[3].double(), tab[:, G * rec])):
            e = float((a - b).abs().max() / b.abs().max())
            print("PLMC_SPLIT %s: d/d %s err %.3g of the largest" % (tag, name, e))
            assert e < 2e-3, (tag, name, e)

    check("unset")
    for split in ("0", "3"):
        with eng.hip.knob("PLMC_SPLIT", split):
            check(split)


# ------------------------------------------------------------------------------------------------ 5. leave-one-out
@pytest.mark.parametrize("members,d,q", [(SETS[0], 1, 1), (SETS[1], 3, 3)], ids=["rbf+periodic", "matern52+lper+rq"])
def test_exact_loo_value_and_every_gradient_fp64(eng, members, d, q):
    """n = 130, fp64; the tolerances of the test of the same name in tests/test_gpu_lper_kernel.py: value 1e-10 relative, every gradient
    group 1e-8 of the group's largest magnitude; exact_loo's moments to 1e-8 relative."""
    n = 130
    X, _, y, table, os_, nz = _problem(members, n, d, q, seed=50 + d)
    val, tab = sd.grads(sd.sum_loo, members, X, y, table, os_, nz)
    got = _logprob(eng, kind_of(members), X, y, table, os_, nz, torch.float64, fn=eng.exact.exact_loo_log_prob)
    rel = float(((got[0] - val) / val).abs().max())
    assert rel <= 1e-10, rel
    G, rec = len(members), 3 * d + 1
    gt = tab[:, :G * rec].reshape(q, G, rec)
    for name, a, b in (("table", got[1], gt), ("oscale", got[2], tab[:, G * rec + 1:]), ("noise", got[3], tab[:, G * rec])):
        scale, err = float(b.abs().max()), float((a - b).abs().max())
        print("    %s: %.2e of %.3e" % (name, err / scale, scale))
        assert err <= 1e-8 * scale, (name, err, scale)
    f = lambda t: t.to(DEV)
    with torch.no_grad():
        s2, r = eng.exact.exact_loo(kind_of(members), f(X), f(table), f(os_), f(nz), f(y))
    Kinv = torch.linalg.inv(sd.khat(members, X, table, os_, nz))
    dg = torch.diagonal(Kinv, dim1=-2, dim2=-1)
    assert torch.allclose(s2.cpu(), 1.0 / dg, rtol=1e-8, atol=0)
    assert torch.allclose(r.cpu(), (Kinv @ y.unsqueeze(-1)).squeeze(-1) / dg, rtol=1e-8, atol=1e-12)


# ------------------------------------------------------------------------------------------------ 6. models
def factory(first=None, **kw):
    """k = ScaleKernel(RBF) + ScaleKernel(Periodic * RBF) + ScaleKernel(RQ), what `kernel_type` may be; `first`: another first member."""
    import projectedlmc
    K = projectedlmc.kernels
    kw.pop("lengthscale_prior", None)
    B = kw.get("batch_shape", torch.Size())
    sc = lambda k: K.ScaleKernel(k, batch_shape=B)
    return sc((first or K.RBFKernel)(**kw)) + sc(K.PeriodicKernel(**kw) * K.RBFKernel(**kw)) + sc(K.RQKernel(**kw))


def factory2(**kw):
    """The same parameters in the same order with a Matern-5/2 kernel in the place of the RBF kernel."""
    import projectedlmc
    return factory(first=projectedlmc.kernels.MaternKernel, **kw)


def _host_pieces(model, d):
    """(members, table, oscale) in fp64 on the host from a copy of the model's kernel, with autograd to the copy's raw parameters (their
    names are the model's).  The table's layout is the package's (pinned by tests/test_sum_kernel.py); the formulas are _sum_dense's."""
    cm = copy.deepcopy(model.covar_module).cpu().double()
    kind, table, os_ = cm._pieces(d)
    assert kind.startswith("sum(")
    return kind[4:-1].split(","), table, os_, {"covar_module." + k: v for k, v in cm.named_parameters()}


def _dense_model_loss(model, X, Y, q, fn=sd.sum_logprob):
    d = X.shape[1]
    members, table, os_, kraw = _host_pieces(model, d)
    raw = {k: v.detach().cpu().double().requires_grad_() for k, v in model.named_parameters() if not k.startswith("covar_module.")}
    lik = model.likelihood
    noise = lik.noise_covar.raw_noise_constraint.transform(raw["likelihood.noise_covar.raw_noise"]).reshape(-1).expand(q)
    c = raw["mean_module.raw_constant"].reshape(q, 1) if "mean_module.raw_constant" in raw else raw["mean_module.constant"].reshape(q, 1)
    y = (Y.reshape(X.shape[0], -1).T if Y.dim() > 1 else Y.reshape(1, -1)) - c
    lp = fn(members, X, y, table, os_, noise)
    return -(lp.sum() / X.shape[0]), {**raw, **kraw}, (members, table.detach(), os_.detach(), noise.detach(), c.detach())


def _series(n, p, seed, d=1):
    g = torch.Generator().manual_seed(seed)
    X = 4.0 * torch.rand(n, d, generator=g, dtype=torch.float64)
    X[:, 0] = torch.sort(X[:, 0])[0]
    Y = torch.stack([torch.sin(2 * math.pi * (1 + k) * X[:, 0] / 4.0) + 0.2 * X[:, 0] + 0.3 * torch.randn(n, generator=g, dtype=torch.float64)
                     for k in range(p)], 1)
    return X, Y


def test_single_output_exact_model(plmc):
    """ExactGPModel with k = ScaleKernel(RBF) + ScaleKernel(Periodic * RBF) + ScaleKernel(RQ), d = 1, fp64; tolerances of the test of the
    same name in tests/test_gpu_lper_kernel.py: loss 1e-9 relative, every parameter gradient rtol 1e-5 / atol 1e-9, eval-mode mean rtol
    1e-7, variance rtol 1e-6, full covariance likewise, compute_loo 1e-8 / 1e-7, evaluate() rtol 1e-10; and LeaveOneOutPseudoLikelihood
    as in tests/test_gpu_loo_objective.py (value 1e-9, gradients rtol 1e-5 / atol 1e-9)."""
    n, ns = 257, 40
    X, Y = _series(n, 1, seed=1)
    y = Y[:, 0]
    torch.manual_seed(4)
    m = perturb_(plmc.ExactGPModel(X, y, plmc.GaussianLikelihood(), kernel_type=factory).double())
    names = [nm for nm, _ in m.named_parameters()]
    for nm in ("kernels.0.raw_outputscale", "kernels.0.base_kernel.raw_lengthscale", "kernels.1.base_kernel.kernels.0.raw_period_length",
               "kernels.2.base_kernel.raw_alpha"):
        assert "covar_module." + nm in names, nm
    m = m.to(DEV)
    m.train(); m.likelihood.train()
    for objective, fn in ((plmc.ExactMarginalLogLikelihood(m.likelihood, m), sd.sum_logprob),
                          (plmc.LeaveOneOutPseudoLikelihood(m.likelihood, m, X, y), sd.sum_loo)):
        m.zero_grad()
        loss = -objective(m(X.to(DEV)), y.to(DEV)).sum()
        loss.backward()
        ref, raw, (members, table, os_, noise, c) = _dense_model_loss(m, X, y, 1, fn=fn)
        ref.backward()
        scale = 1.0                                                # (both objectives are per data point)
        assert abs(float(loss) - scale * float(ref)) < 1e-9 * abs(scale * float(ref)), (float(loss), float(ref))
        for name, prm in m.named_parameters():
            a, b = prm.grad.cpu().double(), scale * raw[name].grad.reshape(prm.shape)
            assert torch.allclose(a, b, rtol=1e-5, atol=1e-9), (name, float((a - b).abs().max()))
    Xs = 4.0 * torch.rand(ns, 1, dtype=torch.float64)
    m.eval(); m.likelihood.eval()
    with torch.no_grad():
        post = m(Xs.to(DEV))
        full = m._posterior(Xs.to(DEV), full_cov=True)
        s2, r = m.compute_loo()
        dense = m.covar_module(X.to(DEV)).evaluate()
    mean_ref, cov_ref = sd.sum_posterior(members, X, (y - c[0]).reshape(1, n), Xs, table, os_, noise)
    assert torch.allclose(post.mean.cpu(), mean_ref[0] + c[0], rtol=1e-7, atol=1e-9)
    assert torch.allclose(post.variance.cpu(), torch.diagonal(cov_ref[0]), rtol=1e-6, atol=1e-9)
    assert torch.allclose(full.covariance_matrix.cpu(), cov_ref[0], rtol=1e-6, atol=1e-9)
    Kinv = torch.linalg.inv(sd.khat(members, X, table, os_, noise)[0])
    dg = torch.diagonal(Kinv)
    assert torch.allclose(s2.cpu().reshape(-1), 1.0 / dg, rtol=1e-8)
    assert torch.allclose(r.cpu().reshape(-1), (Kinv @ (y - c[0, 0])) / dg, rtol=1e-7, atol=1e-10)
    assert torch.allclose(dense.cpu().reshape(n, n), sd.sum_kernel(members, X, X, table, os_)[0], rtol=1e-10, atol=1e-12)


def test_single_output_exact_model_against_the_scikit_learn_fixture(plmc):
    """The configuration of tests/golden/sum_third_party_v1.json (scikit-learn: C RBF + C ExpSineSquared RBF + C RationalQuadratic + White,
    n = 300 sorted points of [0, 10], d = 1) as an ExactGPModel with k = ScaleKernel(RBF) + ScaleKernel(Periodic * RBF) + ScaleKernel(RQ)
    and a zero mean, fp64, set to the fixture's parameters.  scikit-learn's periodic length l enters as l^2: lengthscale = l^2,
    d/d log l = 2 ell d/d ell.  Tolerances of test_single_output_exact_model: the log marginal likelihood (n x the loss per data point)
    1e-9 relative; every gradient, scikit-learn's d/d log theta carried to the model's raw parameter by the chain rule
    (d loss / d raw = -(d lml / d log theta) / (n theta) x d theta / d raw), rtol 1e-5 / atol 1e-9."""
    D = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sum_third_party_v1.json")))
    P = D["params"]
    X = torch.tensor(D["X"], dtype=torch.float64).reshape(-1, 1)
    y = torch.tensor(D["y"], dtype=torch.float64)
    n = X.shape[0]
    m = plmc.ExactGPModel(X, y, plmc.GaussianLikelihood(), kernel_type=factory, mean_type=plmc.ZeroMean).double()
    trend, drift, irregular = m.covar_module.kernels
    periodic, envelope = drift.base_kernel.kernels
    trend.outputscale, trend.base_kernel.lengthscale = P["os_rbf"], P["ell_rbf"]
    drift.outputscale, periodic.lengthscale, periodic.period_length, envelope.lengthscale = P["os_lper"], P["ell_ess"] ** 2, P["period"], P["ell_drift"]
    irregular.outputscale, irregular.base_kernel.lengthscale, irregular.base_kernel.alpha = P["os_rq"], P["ell_rq"], P["alpha"]
    m.likelihood.noise = torch.tensor(P["noise"], dtype=torch.float64)
    nc = m.likelihood.noise_covar
    # scikit-learn's name -> (module, raw parameter, theta, d log theta_sklearn / d log theta)
    where = {"k1__k1__k1__k1__constant_value": (trend, "raw_outputscale", P["os_rbf"], 1.0),
             "k1__k1__k1__k2__length_scale": (trend.base_kernel, "raw_lengthscale", P["ell_rbf"], 1.0),
             "k1__k1__k2__k1__k1__constant_value": (drift, "raw_outputscale", P["os_lper"], 1.0),
             "k1__k1__k2__k1__k2__length_scale": (periodic, "raw_lengthscale", P["ell_ess"] ** 2, 0.5),
             "k1__k1__k2__k1__k2__periodicity": (periodic, "raw_period_length", P["period"], 1.0),
             "k1__k1__k2__k2__length_scale": (envelope, "raw_lengthscale", P["ell_drift"], 1.0),
             "k1__k2__k1__constant_value": (irregular, "raw_outputscale", P["os_rq"], 1.0),
             "k1__k2__k2__alpha": (irregular.base_kernel, "raw_alpha", P["alpha"], 1.0),
             "k1__k2__k2__length_scale": (irregular.base_kernel, "raw_lengthscale", P["ell_rq"], 1.0),
             "k2__noise_level": (nc, "raw_noise", P["noise"], 1.0)}
    assert list(where) == D["theta_names"] and len(list(m.parameters())) == len(where)
    m = m.to(DEV)
    m.train(); m.likelihood.train()
    lazy = m.covar_module(X.to(DEV))
    assert lazy.kind == kind_of(("rbf", "locally_periodic", "rq")) and lazy.ell.shape == (1, 3, 4)
    loss = -plmc.ExactMarginalLogLikelihood(m.likelihood, m)(m(X.to(DEV)), y.to(DEV)).sum()
    loss.backward()
    lml, ref = -n * float(loss), D["log_marginal_likelihood"]
    print("log marginal likelihood %.12f, scikit-learn %.12f" % (lml, ref))
    assert abs(lml - ref) <= 1e-9 * abs(ref), (lml, ref)
    for name, g_log in zip(D["theta_names"], D["grad_log_theta"]):
        mod, raw_name, theta, log_ratio = where[name]
        prm = getattr(mod, raw_name)
        raw = prm.detach().cpu().double().clone().requires_grad_()
        nat = getattr(mod, raw_name + "_constraint").transform(raw)
        assert abs(float(nat.detach().sum()) - theta) <= 1e-12 * theta, (name, nat, theta)
        (dnat,) = torch.autograd.grad(nat.sum(), raw)
        want = -(g_log * log_ratio / theta) / n * dnat.reshape(prm.shape)
        got = prm.grad.cpu().double()
        print("    %s: d loss / d raw %.6e, from scikit-learn %.6e" % (name, float(got.reshape(-1)[0]), float(want.reshape(-1)[0])))
        assert torch.allclose(got, want, rtol=1e-5, atol=1e-9), (name, got, want)


def test_batched_exact_model_latent_moments_against_dense(plmc):
    """n_tasks = 3 batched ExactGPModel on d = 3 inputs, fp64, the factory under an outer ScaleKernel (outputscales=True: it folds into the
    component output scales); body and tolerances of the test of the same name in tests/test_gpu_lper_kernel.py, and the full covariance
    (rtol 1e-6) and evaluate() (rtol 1e-10) with the tolerances of test_single_output_exact_model: the (q, G, 3 d + 1) table with q > 1
    through both."""
    n, q, ns, d = 200, 3, 30, 3
    X, Y = _series(n, q, seed=2, d=d)
    torch.manual_seed(6)
    m = plmc.ExactGPModel(X, Y, plmc.GaussianLikelihood(batch_shape=torch.Size([q])), n_tasks=q, kernel_type=factory, outputscales=True).double()
    perturb_(m)
    m = m.to(DEV)
    m.train(); m.likelihood.train()
    loss = -plmc.ExactMarginalLogLikelihood(m.likelihood, m)(m(X.to(DEV)), Y.T.contiguous().to(DEV)).sum()
    loss.backward()
    ref, raw, (members, table, os_, noise, _) = _dense_model_loss(m, X, Y, q)
    ref.backward()
    assert "covar_module.raw_outputscale" in raw and os_.shape == (q, 3)
    assert abs(float(loss) - float(ref)) < 1e-9 * abs(float(ref)), (float(loss), float(ref))
    for name, prm in m.named_parameters():
        a, b = prm.grad.cpu().double(), raw[name].grad.reshape(prm.shape)
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-9), (name, float((a - b).abs().max()))
    c = m.mean_module(X.to(DEV)).detach().cpu().double().reshape(q, n)
    Xs = 4.0 * torch.rand(ns, d, dtype=torch.float64)
    cs = m.mean_module(Xs.to(DEV)).detach().cpu().double().reshape(q, ns)
    m.eval(); m.likelihood.eval()
    with torch.no_grad():
        post = m(Xs.to(DEV))
        full = m._posterior(Xs.to(DEV), full_cov=True)
        s2, r = m.compute_loo()
        dense = m.covar_module(X.to(DEV)).evaluate()
    mean_ref, cov_ref = sd.sum_posterior(members, X, Y.T - c, Xs, table, os_, noise)
    assert torch.allclose(post.mean.cpu().reshape(q, ns), mean_ref + cs, rtol=1e-7, atol=1e-9)
    assert torch.allclose(post.variance.cpu().reshape(q, ns), torch.diagonal(cov_ref, dim1=-2, dim2=-1), rtol=1e-6, atol=1e-9)
    assert torch.allclose(full.mean.cpu().reshape(q, ns), mean_ref + cs, rtol=1e-7, atol=1e-9)
    assert torch.allclose(full.covariance_matrix.cpu().reshape(q, ns, ns), cov_ref, rtol=1e-6, atol=1e-9)
    assert torch.allclose(dense.cpu().reshape(q, n, n), sd.sum_kernel(members, X, X, table, os_), rtol=1e-10, atol=1e-12)
    Kinv = torch.linalg.inv(sd.khat(members, X, table, os_, noise))
    dg = torch.diagonal(Kinv, dim1=-2, dim2=-1)
    assert torch.allclose(s2.cpu().T, 1.0 / dg, rtol=1e-8)
    assert torch.allclose(r.cpu().T, (Kinv @ (Y.T - c).unsqueeze(-1)).squeeze(-1) / dg, rtol=1e-7, atol=1e-10)


def _projected(plmc, X, Y, q, seed=5, fac=factory, **kw):
    torch.manual_seed(seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return plmc.ProjectedGPModel(X, Y, Y.shape[1], q, mean_type=plmc.ZeroMean, kernel_type=fac, init_lmc_coeffs=True, **kw)


@pytest.mark.parametrize("bulk", [True, False])
def test_projected_model_loss_gradients_and_eval_mode_against_dense(plmc, bulk):
    """fp64, p = 5, q = 3, d = 1, a factory `kernel_type` that returns a sum; body and tolerances of the test of the same name in
    tests/test_gpu_lper_kernel.py (loss 1e-9 relative; gradients rtol 2e-6 / atol 1e-8; eval mode rtol 1e-8 / 1e-7; compute_loo 1e-8;
    evaluate() rtol 1e-10).  The second eval call hits the prediction cache."""
    from projectedlmc import settings
    n, p, q, ns = 257, 5, 3, 40
    X, Y = _series(n, p, seed=3)
    m = perturb_(_projected(plmc, X, Y, q, bulk=bulk).double())
    P, _, names = oracle_dict(m)                     # (the oracle's parameter dict without kernel keys)
    members, table, os_, kraw = _host_pieces(m, 1)
    leaves = {**{k: P[k] for k in names.values()}, **kraw}
    for k in names.values():
        P[k].requires_grad_(True)
    eye = torch.eye(n, dtype=torch.float64)
    ytil = pj.project_data(P, Y)
    K = sd.sum_kernel(members, X, X, table, os_) + pj.projected_noise(P).reshape(q, 1, 1) * eye
    terms, const = pj.projection_terms(P, Y)
    ref = -(gm.mvn_log_prob(K, ytil).sum() / n + sum(terms) + const)
    ref.backward()

    m = m.to(DEV)
    Xd, Yd = X.to(DEV), Y.to(DEV)
    m.train(); m.likelihood.train()
    loss = -plmc.ProjectedLMCmll(m.likelihood, m)(m(Xd), Yd)
    loss.backward()
    assert abs(float(loss) - float(ref)) < 1e-9 * abs(float(ref)), (float(loss), float(ref))
    checked = 0
    for pname, prm in m.named_parameters():
        g_ref = leaves[names.get(pname, pname)].grad
        assert prm.grad is not None and g_ref is not None, pname
        assert torch.allclose(prm.grad.cpu(), g_ref.reshape(prm.shape), rtol=2e-6, atol=1e-8), (pname, prm.grad.cpu(), g_ref)
        checked += 1
    assert checked == len(names) + len(kraw)

    with torch.no_grad():
        Pd = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in P.items()}
        table, os_, K, ytil = table.detach(), os_.detach(), K.detach(), ytil.detach()
        Xs = 4.0 * torch.rand(ns, 1, dtype=torch.float64)
        Ks, Kss = sd.sum_kernel(members, X, Xs, table, os_), sd.sum_kernel(members, Xs, Xs, table, os_)
        sol = torch.linalg.solve(K, Ks)
        mu_lat = (sol * ytil.unsqueeze(-1)).sum(1)
        cov_lat = Kss - Ks.transpose(-1, -2) @ sol
        Ht = pj.lmc_coefficients(Pd)
        mean_ref = mu_lat.T @ Ht
        var_ref = torch.diagonal(cov_lat, dim1=-2, dim2=-1).T @ (Ht * Ht) + Pd["eps"]
        Kinv = torch.linalg.inv(K)
        kdiag = torch.diagonal(Kinv, dim1=-2, dim2=-1)
        alpha = (Kinv @ ytil.unsqueeze(-1)).squeeze(-1)
    m.eval(); m.likelihood.eval()
    with settings.prediction_cache("eager"), torch.no_grad():
        dist = m(Xs.to(DEV))
        c = m._prediction_cache()
        assert (c.hits, c.misses) == (0, 1) and c.ws is not None and c.ws.with_inverse
        again = m(Xs.to(DEV))
        assert (c.hits, c.misses) == (1, 1)
        lat = m.compute_latent_distrib(Xs.to(DEV), full_cov=True)
        s2, r = m.compute_loo()
        dense = m.covar_module(Xd).evaluate()
    for d_ in (dist, again):
        assert torch.allclose(d_.mean.cpu(), mean_ref, rtol=1e-8, atol=1e-10)
        assert torch.allclose(d_.variance.cpu(), var_ref, rtol=1e-7, atol=1e-10)
    assert torch.allclose(lat.mean.cpu(), mu_lat, rtol=1e-8, atol=1e-10)
    assert torch.allclose(lat.covariance_matrix.cpu(), cov_lat, rtol=1e-7, atol=1e-10)
    assert torch.allclose(s2.cpu(), (1.0 / kdiag).T, rtol=1e-8, atol=0)
    assert torch.allclose(r.cpu(), (alpha / kdiag).T, rtol=1e-8, atol=1e-12)
    assert torch.allclose(dense.cpu(), sd.sum_kernel(members, X, X, table, os_), rtol=1e-10, atol=1e-12)


def test_latent_shards_sum_to_the_unsharded_loss_and_gradients(plmc):
    """The shards of a latent-sharded projected model sum to the unsharded loss (1e-10) and gradients (rtol 1e-8): the table
    (q, G, 3 d + 1) is sliced by latent_ids like ell is (tests/test_gpu_lper_kernel.py, the same name)."""
    n, p, q, world = 257, 6, 3, 2
    X, Y = _series(n, p, seed=21)
    Xd, Yd = X.to(DEV), Y.to(DEV)

    def build(shard):
        m = perturb_(_projected(plmc, X, Y, q, seed=2, latent_shard=shard).double()).to(DEV)
        m.train(); m.likelihood.train()
        return m, plmc.ProjectedLMCmll(m.likelihood, m)

    m0, mll0 = build(None)
    loss0 = -mll0(m0(Xd), Yd)
    loss0.backward()
    total, grads = 0.0, None
    for rank in range(world):
        m1, mll1 = build((rank, world))
        share = -mll1(m1(Xd), Yd)
        share.backward()
        total = total + float(share.detach())
        gs = [torch.zeros_like(prm) if prm.grad is None else prm.grad.clone() for prm in m1.parameters()]
        grads = gs if grads is None else [a + b for a, b in zip(grads, gs)]
    assert abs(total - float(loss0)) < 1e-10 * abs(float(loss0)), (total, float(loss0))
    for (name, prm), g in zip(m0.named_parameters(), grads):
        assert torch.allclose(prm.grad, g, rtol=1e-8, atol=1e-11), (name, (prm.grad - g).abs().max())


def test_sums_that_differ_only_in_members_do_not_share_a_cached_prediction(plmc, eng):
    """Two models with the same parameter values whose sums differ in one member (RBF against Matern-5/2) predict differently, each equal
    to its own dense conditioning, also when one PosteriorCache object serves both with the same state key: the member list is part of
    the key (exact_posterior)."""
    from projectedlmc import settings
    n, ns = 130, 20
    X, Y = _series(n, 1, seed=7)
    y = Y[:, 0]
    Xs = 4.0 * torch.rand(ns, 1, dtype=torch.float64)
    out = []
    cache = eng.exact.PosteriorCache()
    for fac in (factory, factory2):
        torch.manual_seed(4)
        m = perturb_(plmc.ExactGPModel(X, y, plmc.GaussianLikelihood(), kernel_type=fac).double()).to(DEV)
        m.eval(); m.likelihood.eval()
        lazy = m.covar_module(X.to(DEV))
        noise = m.likelihood.noise.reshape(-1).detach()
        with settings.prediction_cache("eager"), torch.no_grad():
            for _ in range(2):
                mean, var = eng.exact.exact_posterior(lazy.kind, lazy.x1, lazy.ell.detach(), lazy.oscale.detach(), noise,
                                                      y.reshape(1, n).to(DEV), Xs.to(DEV), cache=cache, key=("same state",))
        members, table, os_, _ = _host_pieces(m, 1)
        mean_ref, cov_ref = sd.sum_posterior(members, X, y.reshape(1, n), Xs, table.detach(), os_.detach(), noise.cpu())
        assert torch.allclose(mean.cpu(), mean_ref, rtol=1e-7, atol=1e-9), members
        out.append(mean.cpu())
    assert cache.misses == 2 and cache.hits == 2
    assert not torch.allclose(out[0], out[1], rtol=1e-3)


# ------------------------------------------------------------------------------------------------ 7. draws
def test_prior_draws_are_shift_plus_the_dense_factor_times_the_base_samples(plmc):
    """`MultivariateNormal(loc, k(X)).sample()` for a sum kernel, fp64, n = 130, through the likelihood (noise 0.1) and noise-free (the
    reference's call: settings.cholesky_jitter stands on the diagonal).  With identity base samples the draws are the rows of U: exactly
    upper triangular, and U^T U reproduces Khat + the reported jitter by the rho_U rule tests/test_gpu_sampling.py applies to the same call
    with a single-family kernel.  With noise the factor itself equals the dense fp64 one (rtol 1e-8, condition number of order 10) and
    draws for other base samples are shift + U^T z to rounding."""
    n, d, q = 130, 1, 1
    X, _ = _series(n, 1, seed=9)
    torch.manual_seed(4)
    k = perturb_(factory(batch_shape=torch.Size([q])).double())
    members, table, os_, _ = _host_pieces(torch.nn.ModuleDict({"covar_module": k}), d)
    table, os_ = table.detach(), os_.detach()
    kd = k.to(DEV)
    lik = plmc.GaussianLikelihood(batch_shape=torch.Size([q])).double().to(DEV)
    lik.noise = torch.tensor(0.1)
    g = torch.Generator().manual_seed(3)
    loc = torch.randn(q, n, generator=g, dtype=torch.float64)
    eye = torch.eye(n, dtype=torch.float64)
    for noisy in (True, False):
        dist = plmc.MultivariateNormal(loc.to(DEV), kd(X.to(DEV)))
        if noisy:
            dist = lik(dist)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            draws = dist.sample(base_samples=eye.to(DEV)[:, None, :].expand(n, q, n).contiguous())
        jit = dist.sample_jitter
        S = (draws.cpu() - loc).permute(1, 0, 2)                       # S[b][j][i] = U_b[j][i]
        S = torch.triu(S)                                              # (the shift was added and taken off again: one rounding of |loc|)
        low = torch.tril((draws.cpu() - loc).permute(1, 0, 2), -1).abs()
        assert bool((low <= 2 * 2.0 ** -53 * loc.abs()[:, None, :]).all())
        nz = float(dist.lazy_covariance_matrix.noise.reshape(-1)[0]) if noisy else 0.0      # (0.1 through the constraint's round trip)
        assert abs(nz - (0.1 if noisy else 0.0)) < 1e-6
        Kref = sd.sum_kernel(members, X, X, table, os_) + (nz + jit) * eye
        rho = float(torch.linalg.matrix_norm(S.transpose(1, 2) @ S - Kref) / torch.linalg.matrix_norm(Kref))
        print("noisy=%s: jitter %.1e, |U^T U - Khat| / |Khat| = %.3g" % (noisy, jit, rho))
        # the rule of tests/test_gpu_sampling.py for the same call with a single-family kernel (tests/_factor_ref.plain_thresholds): in
        # units of n_pad u |Khat|, rho_U <= (1 + sqrt kappa) max(rho_U of the CPU LAPACK factor, 1)
        unit = fr.pad(n) * fr.UNIT[torch.float64]
        ev = torch.linalg.eigvalsh(Kref)
        kappa = float((ev[:, -1] / ev[:, 0].clamp_min(1e-300)).max())
        Lk = torch.linalg.cholesky(Kref)
        rho_lapack = float(torch.linalg.matrix_norm(Lk @ Lk.transpose(1, 2) - Kref) / torch.linalg.matrix_norm(Kref)) / unit
        thr = (1.0 + math.sqrt(kappa)) * max(rho_lapack, 1.0)
        print("    kappa %.3g, rho_U %.3g, threshold %.3g (units of n_pad u)" % (kappa, rho / unit, thr))
        assert rho / unit <= thr, (rho / unit, thr)
        if noisy:
            assert jit == 0.0
            Lc = torch.linalg.cholesky(Kref)
            assert torch.allclose(S.transpose(1, 2), Lc, rtol=1e-8, atol=1e-11)
            Z = torch.randn(5, q, n, generator=g, dtype=torch.float64)
            more = dist.sample(base_samples=Z.to(DEV)).cpu()
            ref = loc + (Lc @ Z.unsqueeze(-1)).squeeze(-1)
            assert torch.allclose(more, ref, rtol=1e-8, atol=1e-9), float((more - ref).abs().max())


# ------------------------------------------------------------------------------------------------ 8. limits
def test_limits_are_argument_errors(eng):
    """Too many components, d beyond the limit, a spline or unknown member code, null `fam` or `table`: refused on the host by every new
    entry point with the library's error naming the limit or the member; nothing is launched (the buffers of NaN are untouched)."""
    import ctypes
    hip = eng.hip
    L = hip.lib()
    Dx, Gx = L.cdll.plmc_sum_max_dim(), L.cdll.plmc_sum_max_components()
    assert (Dx, Gx) == (8, 4)
    n, q, f64 = 130, 1, torch.float64
    st = hip.stream_ptr(DEV)
    nan = lambda *s: torch.full(s, float("nan"), device=DEV, dtype=f64)
    cases = [(Dx + 1, [0, 16], True, True, "plmc_sum_max_dim"), (2, [0] * (Gx + 1), True, True, "plmc_sum_max_components"),
             (2, [0, 4], True, True, "spline"), (2, [0, 7], True, True, "unknown member family code"),
             (2, [0, 16], False, True, "null pointer"), (2, [0, 16], True, False, "null pointer")]
    for d, codes, with_fam, with_table, word in cases:
        G = len(codes)
        fam = (ctypes.c_int * G)(*codes)
        famp = ctypes.addressof(fam) if with_fam else None
        X = torch.rand(n, d, device=DEV, dtype=f64)
        table = torch.ones(q, G, 3 * d + 1, device=DEV, dtype=f64)
        tp = hip.ptr(table) if with_table else None
        o, nz = torch.ones(q, G, device=DEV, dtype=f64), torch.ones(q, device=DEV, dtype=f64)
        wi = eng.exact.Workspace(n, q, 1, f64, DEV, with_inverse=True, ncomp=min(G, Gx), per=eng.exact.SUM)
        wi.A.fill_(float("nan"))
        out, gt = nan(q, n, n), nan(q, G * (3 * d + 2) + 1)
        with pytest.raises(RuntimeError, match=word):
            L.call("plmc_assemble_sum", f64, hip.ptr(X), n, d, G, famp, tp, hip.ptr(o), hip.ptr(nz), hip.ptr(wi.A), wi.lda, wi.strideA, q, st)
        with pytest.raises(RuntimeError, match=word):
            L.call("plmc_assemble_cross_sum", f64, hip.ptr(X), n, hip.ptr(X), n, d, G, famp, tp, hip.ptr(o), hip.ptr(out), n, n * n, 0, n, q, st)
        with pytest.raises(RuntimeError, match=word):
            L.call("plmc_factorize_sum_ex", f64, hip.ptr(X), n, d, G, famp, tp, hip.ptr(o), hip.ptr(nz), hip.ptr(wi.A), wi.n_pad, wi.lda,
                   wi.naug, wi.strideA, hip.ptr(wi.Vd), hip.ptr(wi.logdet), hip.ptr(wi.info), 1, q, hip.ptr(nz), st)
        with pytest.raises(RuntimeError, match=word):
            L.call("plmc_kinv_grad_sum_vd", f64, hip.ptr(wi.W), wi.n_pad, wi.ldw, wi.strideW, hip.ptr(wi.alpha), hip.ptr(X), n, d, G, famp, tp,
                   hip.ptr(o), hip.ptr(gt), None, 0, 0, None, hip.ptr(wi.partials), q, hip.ptr(nz), hip.ptr(wi.Vd), st)
        Xop = torch.zeros(q, wi.n_pad + wi.NB, wi.n_pad, device=DEV, dtype=f64)
        beta = torch.zeros(q, wi.n_pad, device=DEV, dtype=f64)
        with pytest.raises(RuntimeError, match=word):
            L.call("plmc_loo_grad_sum", f64, hip.ptr(Xop), wi.n_pad, wi.n_pad + 16, wi.n_pad, Xop.shape[1] * wi.n_pad, hip.ptr(beta), hip.ptr(X),
                   n, d, G, famp, tp, hip.ptr(o), hip.ptr(gt), hip.ptr(wi.partials), q, st)
        torch.cuda.synchronize()
        assert bool(torch.isnan(wi.A).all()) and bool(torch.isnan(out).all()) and bool(torch.isnan(gt).all()), word
    # the fp32 split path without the planes of W in Vd: refused, in the words of the other families
    X = torch.rand(n, 1, device=DEV)
    wi = eng.exact.Workspace(n, q, 1, torch.float32, DEV, with_inverse=True, ncomp=2, per=eng.exact.SUM)
    fam = (ctypes.c_int * 2)(0, 16)
    table, o, nz = torch.ones(q, 2, 4, device=DEV), torch.ones(q, 2, device=DEV), torch.ones(q, device=DEV)
    gt = torch.full((q, 2 * 5 + 1), float("nan"), device=DEV, dtype=f64)
    with eng.hip.knob("PLMC_SPLIT", "3"), pytest.raises(RuntimeError, match="planes of W from the sweep's Vd"):
        L.call("plmc_kinv_grad_sum_vd", torch.float32, hip.ptr(wi.W), wi.n_pad, wi.ldw, wi.strideW, hip.ptr(wi.alpha), hip.ptr(X), n, 1, 2,
               ctypes.addressof(fam), hip.ptr(table), hip.ptr(o), hip.ptr(gt), None, 0, 0, None, hip.ptr(wi.partials), q, hip.ptr(nz), None, st)
    torch.cuda.synchronize()
    assert bool(torch.isnan(gt).all())
    # ... and with one member, whose own family's checks refuse: they run before the record is re-laid behind the partial sums
    wi = eng.exact.Workspace(n, q, 1, torch.float32, DEV, with_inverse=True, ncomp=1, per=eng.exact.SUM)
    wi.partials.fill_(7)
    fam = (ctypes.c_int * 1)(16)
    with eng.hip.knob("PLMC_SPLIT", "3"), pytest.raises(RuntimeError, match="planes of W from the sweep's Vd"):
        L.call("plmc_kinv_grad_sum_vd", torch.float32, hip.ptr(wi.W), wi.n_pad, wi.ldw, wi.strideW, hip.ptr(wi.alpha), hip.ptr(X), n, 1, 1,
               ctypes.addressof(fam), hip.ptr(table), hip.ptr(o), hip.ptr(gt), None, 0, 0, None, hip.ptr(wi.partials), q, hip.ptr(nz), None, st)
    with pytest.raises(RuntimeError, match="null pointer"):      # (no alpha)
        L.call("plmc_kinv_grad_sum_vd", torch.float32, hip.ptr(wi.W), wi.n_pad, wi.ldw, wi.strideW, None, hip.ptr(X), n, 1, 1,
               ctypes.addressof(fam), hip.ptr(table), hip.ptr(o), hip.ptr(gt), None, 0, 0, None, hip.ptr(wi.partials), q, hip.ptr(nz), hip.ptr(wi.Vd), st)
    torch.cuda.synchronize()
    assert bool(torch.isnan(gt).all()) and bool((wi.partials == 7).all())
    # the Python layer names the limits too
    Xb = torch.rand(n, Dx + 1, device=DEV, dtype=f64)
    with pytest.raises(ValueError, match="plmc_sum_max_dim"):
        eng.exact.exact_latent_log_prob("sum(rbf,rq)", Xb, torch.ones(q, 2, 3 * (Dx + 1) + 1, device=DEV, dtype=f64), None,
                                        torch.ones(q, device=DEV, dtype=f64), torch.zeros(q, n, device=DEV, dtype=f64))
    with pytest.raises(ValueError, match="spline"):
        eng.exact.exact_latent_log_prob("sum(rbf,spline)", Xb[:, :2].contiguous(), torch.ones(q, 2, 7, device=DEV, dtype=f64), None,
                                        torch.ones(q, device=DEV, dtype=f64), torch.zeros(q, n, device=DEV, dtype=f64))
