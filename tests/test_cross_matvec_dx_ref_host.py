"""The input derivatives of the fused cross-covariance products without a device (tests/_cross_matvec_dx_ref.py), in the pattern of
test_cross_matvec_ref_host.py:

  * the library declares and exports the entry points of every family, their signatures are the value's with `G, Jx` in the place of
    `Out`, the split is a function of the sizes alone, refused kinds raise by name before the device check and every argument error
    comes back through plmc_last_error() with no device present;
  * the references agree with central differences of the dense value formulas;
  * a CPU restatement of the kernel's arithmetic -- the pair in the element type, fp64 sums in segment order -- passes the assertions the
    GPU tests apply, read from buffers with NaN wherever the kernel must not read;
  * seeded mistakes leave them: sums carried in fp32 (shown at the fp64 tolerance: at n = 600 an fp32 sum is off by about sqrt(n) 2^-25 of
    the terms, which the fp32 tolerance 4 (d + 4) 2^-24 admits by design and 1e-10 does not), a dropped last row, G's column order
    swapped, and the sine's phase left unreduced at 10^4 revolutions in fp32."""
import ctypes
import os
import re

import pytest
import torch

import _cross_matvec_dx_ref as cdx
import _cross_matvec_ref as cm
import _posterior_dx_dense as pdd

F32, F64 = torch.float32, torch.float64
INFIXES = ("", "_add", "_sm", "_per", "_rq", "_lper", "_sum", "_dot")


@pytest.fixture(scope="module")
def L():
    from projectedlmc import _hip
    return _hip.lib().cdll


# ---------------------------------------------------------------------------------------------- the library, without a device
def test_symbols_are_declared_and_exported(L, repo_root):
    from projectedlmc import _hip
    header = open(os.path.join(repo_root, "include", "plmc.h")).read()
    declared = set(re.findall(r"\b(plmc_[a-z0-9_]+)\s*\(", header))
    names = ["plmc_cross_matvec_dx" + i + s for i in INFIXES for s in ("_f32", "_f64")]
    names += ["plmc_rff_matvec_dx_f32", "plmc_rff_matvec_dx_f64", "plmc_cross_matvec_dx_splits", "plmc_cross_matvec_dx_partials_bytes"]
    for name in names:
        assert name in declared and name in _hip.exported_symbols() and getattr(L, name) is not None, name
    assert L.plmc_version() == _hip.ABI_VERSION == 4                    # symbols are only added


def test_signatures_are_the_values_with_g_and_jx_for_out(repo_root):
    from projectedlmc import _hip
    P = _hip._P
    for infix in INFIXES:
        val, dx = _hip._TYPED["plmc_cross_matvec" + infix], _hip._TYPED["plmc_cross_matvec_dx" + infix]
        assert dx == val[:-4] + [P, P] + val[-3:], infix               # ..., r | Out -> G, Jx | partials, q, stream
    val, dx = _hip._TYPED["plmc_rff_matvec"], _hip._TYPED["plmc_rff_matvec_dx"]
    assert dx == val[:8] + [P] + val[8:], "G stands in front of scale"   # (freq, phase, m, Xs, ns, d, Wt, r | G | scale, Jx, partials, q, stream)
    header = open(os.path.join(repo_root, "include", "plmc.h")).read()
    flat = re.sub(r"\s+", " ", header)
    for infix in INFIXES:
        for suf, T in (("f32", "float"), ("f64", "double")):
            val = re.search(r"int plmc_cross_matvec%s_%s\((.*?)\);" % (infix, suf), flat).group(1)
            dx = re.search(r"int plmc_cross_matvec_dx%s_%s\((.*?)\);" % (infix, suf), flat).group(1)
            norm = lambda a: re.sub(r"\s*\*\s*", " *", a)
            assert norm(dx) == norm(val).replace("%s *Out" % T, "const %s *G, double *Jx" % T), (infix, suf)


def test_split_is_a_function_of_the_sizes_alone(L):
    assert L.plmc_cross_matvec_dx_splits(129, 37, 3) == 1 and L.plmc_cross_matvec_dx_partials_bytes(129, 37, 5, 3) == 0
    assert L.plmc_cross_matvec_dx_splits(256, 1, 1) == 1                # one segment cannot be split
    s = L.plmc_cross_matvec_dx_splits(1100, 3, 3)
    assert s == 5 and L.plmc_cross_matvec_dx_partials_bytes(1100, 3, 5, 3) == 5 * 3 * 3 * 5 * 8    # one fp64 sum per segment of 256 rows
    for n, ns, q in ((130, 37, 3), (700, 3, 3), (8192, 16, 8), (8192, 2048, 8), (8192, 131072, 8), (40000, 5, 2)):
        assert L.plmc_cross_matvec_dx_splits(n, ns, q) == L.plmc_cross_matvec_splits(n, ns, q)        # the ranges of the values
    assert L.plmc_cross_matvec_dx_splits(8192, 16, 8) > L.plmc_cross_matvec_dx_splits(8192, 2048, 8) >= 1
    assert L.plmc_cross_matvec_dx_splits(0, 3, 3) == 0 and L.plmc_cross_matvec_dx_splits(5, 0, 3) == 0
    assert L.plmc_cross_matvec_dx_partials_bytes(1100, 3, 0, 3) == 0


@pytest.mark.parametrize("kind", ["spline", "linear", "poly3", "sum(rbf,periodic)"])
def test_refused_kinds_raise_by_name_before_the_device_check(kind):
    from projectedlmc import _engine
    n, ns, d, q = 12, 3, 2, 2
    X, Xs, V, G = torch.rand(n, d), torch.rand(ns, d), torch.rand(q, n, 2), torch.rand(q, ns, 2)
    ell = torch.ones(q, 2, 3 * d + 1) if kind.startswith("sum") else torch.ones(q, d + 1) if kind != "spline" else torch.ones(q, d)
    with pytest.raises(NotImplementedError, match=kind.replace("(", r"\(").replace(")", r"\)")):
        _engine.cross_matvec_dx(kind, Xs, X, ell, None, V, G)
    with pytest.raises(RuntimeError, match="no CPU fallback"):        # a served kind meets the device check
        _engine.cross_matvec_dx("matern52", Xs, X, torch.ones(q, d), None, V, G)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _engine.rff_matvec_dx(torch.rand(q, 5, d), torch.rand(q, 5), Xs, torch.rand(q, 5, 2), G)


def test_argument_errors_come_back_without_a_device(L):
    """Pointers are never dereferenced on a refused call: dummy non-null addresses stand in for device memory."""
    P = ctypes.c_void_p(4096)
    cap = L.plmc_cross_matvec_max_cols()

    def refused(word, kind=3, X=P, n=20, Xs=P, ns=4, d=3, ell=P, V=P, ldv=3, strideV=100, r=3, G=P, Jx=P, part=None, q=2):
        rc = L.plmc_cross_matvec_dx_f32(kind, X, n, Xs, ns, d, ell, None, V, ldv, strideV, r, G, Jx, part, q, None)
        msg = L.plmc_last_error().decode()
        assert rc != 0 and word in msg, (word, rc, msg)

    for null in ("X", "Xs", "ell", "V", "Jx"):
        refused("null pointer", **{null: None})
    refused("n > 0", n=0)
    refused("ns > 0", ns=0)
    refused("r > 0", r=0)
    refused("q <= 65535", q=0)
    refused("plmc_cross_matvec_max_cols", r=cap + 1, ldv=cap + 1)
    refused("ldv >= r", ldv=2)
    refused("strideV", strideV=3 * 19 + 2)
    refused("G == NULL takes r == 1", G=None)
    refused("plmc_max_dim", d=33)
    refused("unknown kernel kind", kind=5)
    refused("spline", kind=4)
    refused("partials", n=700, strideV=2100)                           # splits into three ranges, no scratch given
    fam = (ctypes.c_int * 2)(0, 16)
    for name, args, word in (("plmc_cross_matvec_dx_add_f32", (3, P, 20, P, 4, 3, 5, P, None), "plmc_max_components"),
                             ("plmc_cross_matvec_dx_add_f32", (4, P, 20, P, 4, 3, 2, P, None), "spline"),
                             ("plmc_cross_matvec_dx_sm_f32", (P, 20, P, 4, 9, 2, P, P, None), "plmc_sm_max_dim"),
                             ("plmc_cross_matvec_dx_sm_f32", (P, 20, P, 4, 2, 9, P, P, None), "plmc_sm_max_mixtures"),
                             ("plmc_cross_matvec_dx_per_f32", (P, 20, P, 4, 9, P, P, None), "plmc_per_max_dim"),
                             ("plmc_cross_matvec_dx_rq_f32", (P, 20, P, 4, 17, P, P, None), "plmc_rq_max_dim"),
                             ("plmc_cross_matvec_dx_lper_f32", (P, 20, P, 4, 9, P, P, P, None), "plmc_lper_max_dim"),
                             ("plmc_cross_matvec_dx_sum_f32", (P, 20, P, 4, 2, 2, ctypes.cast(fam, ctypes.c_void_p), P, None), "sum"),
                             ("plmc_cross_matvec_dx_dot_f32", (P, 20, P, 4, 3, P, P, 1, None), "dot-product")):
        rc = getattr(L, name)(*args, P, 3, 100, 3, P, P, None, 2, None)
        msg = L.plmc_last_error().decode()
        assert rc != 0 and word in msg, (name, rc, msg)
    # the f64 entry points take the same road
    rc = L.plmc_cross_matvec_dx_f64(3, P, 20, P, 4, 3, P, None, P, 3, 100, 3, None, P, None, 2, None)
    assert rc != 0 and "G == NULL takes r == 1" in L.plmc_last_error().decode()

    def rff_refused(word, freq=P, phase=P, m=10, Xs=P, ns=4, d=3, Wt=P, r=3, G=P, Jx=P, part=None, q=2):
        rc = L.plmc_rff_matvec_dx_f32(freq, phase, m, Xs, ns, d, Wt, r, G, None, Jx, part, q, None)
        msg = L.plmc_last_error().decode()
        assert rc != 0 and word in msg, (word, rc, msg)

    for null in ("freq", "phase", "Xs", "Wt", "Jx"):
        rff_refused("null pointer", **{null: None})
    rff_refused("n > 0", m=0)
    rff_refused("ns > 0", ns=0)
    rff_refused("plmc_cross_matvec_max_cols", r=cap + 1)
    rff_refused("G == NULL takes r == 1", G=None)
    rff_refused("plmc_max_dim", d=33)
    rff_refused("partials", m=1030)


# ---------------------------------------------------------------------------------------------- the references
@pytest.mark.parametrize("family", pdd.FAMILIES)
def test_reference_agrees_with_central_differences_of_the_values(family):
    n, ns, d, q, r = 30, 5, 3, 2, 3
    p = pdd.problem(family, d, q, seed=7)
    X = pdd.igd.inputs(n, d, seed=7)
    Xs = pdd.query_points(ns, d, seed=7)
    V, G = cdx.operands(n, ns, r, q, seed=7)
    Jx, T = cdx.reference(p.K, X, Xs, V, G)
    value = lambda Xa: ((p.K(Xa, X) @ V) * G).sum(-1)                   # (q, ns): sum_c G[s, c] Out[s, c]
    h = 1e-5
    for k in range(d):
        e = torch.zeros(ns, d, dtype=F64)
        e[:, k] = h
        cd = (value(Xs + e) - value(Xs - e)) / (2 * h)
        scale = T[:, :, k].clamp_min(1e-300)
        assert float(((cd - Jx[:, :, k]).abs() / scale).max()) < (2e-4 if family == "matern12" else 1e-7), (family, k)
    assert bool((T >= Jx.abs() * (1 - 1e-12)).all())
    one, _ = cdx.reference(p.K, X, Xs, V[:, :, 1:2], None)              # G None: the Jacobian of one column
    sel = torch.zeros(q, ns, r, dtype=F64)
    sel[:, :, 1] = 1.0
    assert torch.allclose(one, cdx.reference(p.K, X, Xs, V, sel)[0], rtol=1e-13, atol=1e-15)


@pytest.mark.parametrize("d", [1, 4])
def test_feature_reference_agrees_with_central_differences(d):
    freq, phase, Wt, scale = cm.rff_problem(d, 40, 2, 3, seed=d, max_rev=3.0)
    _, Xs = cm.inputs("rbf", 4, 6, d, seed=d)
    G = cdx.operands(4, 6, 3, 2, seed=d)[1]
    exact, bound = cdx.rff_reference(freq, phase, Xs, Wt, G, scale, F64)
    value = lambda Xa: (cm.rff_reference(freq, phase, Xa, Wt, scale, F64)[0] * G).sum(-1)
    h = 1e-6
    for k in range(d):
        e = torch.zeros(6, d, dtype=F64)
        e[:, k] = h
        cd = (value(Xs + e) - value(Xs - e)) / (2 * h)
        assert torch.allclose(cd, exact[:, :, k], rtol=1e-6, atol=1e-6)
    assert bool((bound > 0).all())


def test_path_reference_is_differentiable_in_the_test_inputs():
    p = pdd.problem("matern52", 2, 2, seed=1)
    X = pdd.igd.inputs(20, 2, seed=1)
    freq, phase, Wt, _ = cm.rff_problem(2, 16, 2, 3, seed=1, max_rev=3.0)
    g = torch.Generator().manual_seed(2)
    w, v = torch.randn(3, 2, 16, generator=g, dtype=F64), torch.randn(2, 20, 3, generator=g, dtype=F64)
    fs = torch.full((2, 16), 0.3, dtype=F64)
    Xs = pdd.query_points(4, 2, seed=1).requires_grad_()
    out = cdx.paths_latents(p.K, X, freq, phase, fs, w, v, Xs)
    up = torch.randn(out.shape, generator=g, dtype=F64)
    grad, = torch.autograd.grad((out * up).sum(), Xs)
    Wt = (w * fs[None]).permute(1, 2, 0)
    want = cdx.reference(p.K, X, Xs.detach(), v, up)[0] + cdx.rff_reference(freq, phase, Xs.detach(), Wt, up, None, F64)[0]
    assert torch.allclose(grad, want.sum(0), rtol=1e-12, atol=1e-13)


# ---------------------------------------------------------------------------------------------- the kernel's arithmetic on the CPU
def _setup(family, d, n, ns, q, r, seed, dtype, with_g=True):
    p = pdd.problem(family, d, q, seed)
    X = pdd.igd.inputs(n, d, seed)
    Xs = pdd.query_points(ns, d, seed, X, coincident=True)
    V, G = cdx.operands(n, ns, r, q, seed, with_g)
    return (p, X, Xs, V, G) + cdx.buffers(V, G, dtype)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("family", pdd.FAMILIES)
def test_cpu_restatement_passes_the_gpu_assertions(family, dtype):
    d, n, ns, q, r = 3, 300, 9, 2, 3
    p, X, Xs, V, G, Vbuf, Gbuf = _setup(family, d, n, ns, q, r, 11, dtype)
    want, T = cdx.reference(p.K, X, Xs, V, G)
    got = cdx.cpu_product(p.K, X, Xs, Vbuf, Gbuf, n, r, dtype)
    assert bool(torch.isfinite(got).all())
    print(family, dtype, "worst err / (2^-24 sum |terms|) = %.3f" % cdx.worst_ratio(got, want, T))
    assert cdx.violations(got, want, T, cdx.tolerance(family, d, dtype)) == 0
    assert bool((got[:, :, p.zero] == 0.0).all())


def test_cpu_restatement_of_one_column_without_g():
    p, X, Xs, V, G, Vbuf, Gbuf = _setup("matern52", 3, 130, 5, 2, 1, 3, F32, with_g=False)
    assert G is None and Gbuf is None
    want, T = cdx.reference(p.K, X, Xs, V, None)
    assert cdx.violations(cdx.cpu_product(p.K, X, Xs, Vbuf, None, 130, 1, F32), want, T, cdx.tolerance("matern52", 3, F32)) == 0


@pytest.mark.parametrize("mutate,dtype", [("fp32_sums", F64), ("drop_last_row", F32), ("drop_last_row", F64), ("swap_g_columns", F32),
                                          ("swap_g_columns", F64)])
def test_seeded_mutations_fail_the_gpu_assertions(mutate, dtype):
    d, n, ns, q, r = 3, 600, 8, 2, 3                                   # three segments of 256 rows
    p, X, Xs, V, G, Vbuf, Gbuf = _setup("matern52", d, n, ns, q, r, 5, dtype)
    want, T = cdx.reference(p.K, X, Xs, V, G)
    tol = cdx.tolerance("matern52", d, dtype)
    assert cdx.violations(cdx.cpu_product(p.K, X, Xs, Vbuf, Gbuf, n, r, dtype), want, T, tol) == 0
    bad = cdx.violations(cdx.cpu_product(p.K, X, Xs, Vbuf, Gbuf, n, r, dtype, mutate=mutate), want, T, tol)
    print(mutate, dtype, "elements outside the tolerance:", bad, "of", want.numel())
    assert bad > want.numel() // 2, (mutate, bad)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("d", [1, 4, 9])
def test_feature_derivative_meets_its_bound_at_large_phase(d, dtype):
    freq, phase, Wt, scale = cm.rff_problem(d, 100, 2, 3, seed=d, max_rev=1.0e4)
    _, Xs = cm.inputs("rbf", 4, 33, d, seed=d)
    Xs[0] = 1.0                                                        # the last feature at 10^4 revolutions
    assert float((freq[:, -1] * Xs[0]).sum(-1).max()) >= 9999.0
    G = cdx.operands(4, 33, 3, 2, seed=d)[1]
    exact, bound = cdx.rff_reference(freq, phase, Xs, Wt, G, scale, dtype)
    assert cdx.rff_violations(cdx.rff_cpu_product(freq, phase, Xs, Wt, G, scale, dtype), exact, bound) == 0


def test_unreduced_fp32_phase_fails_the_bound_at_ten_thousand_revolutions():
    freq, phase, Wt, scale = cm.rff_problem(3, 100, 2, 3, seed=3, max_rev=1.0e4)
    _, Xs = cm.inputs("rbf", 4, 33, 3, seed=3)
    G = cdx.operands(4, 33, 3, 2, seed=3)[1]
    exact, bound = cdx.rff_reference(freq, phase, Xs, Wt, G, scale, F32)
    bad = cdx.rff_violations(cdx.rff_cpu_product(freq, phase, Xs, Wt, G, scale, F32, mutate="unreduced_phase"), exact, bound)
    print("unreduced fp32 phase: elements outside the bound:", bad, "of", exact.numel())
    assert bad > exact.numel() // 2


def test_path_reference_is_paths_dense_with_the_weights_handed_in():
    """paths_latents restates _cross_matvec_ref.paths_dense with v given: with paths_dense's own solve for v the two agree."""
    p = pdd.problem("matern52", 2, 2, seed=1)
    X, Xs = pdd.igd.inputs(20, 2, seed=1), pdd.query_points(4, 2, seed=1)
    freq, phase, _, _ = cm.rff_problem(2, 16, 2, 3, seed=1, max_rev=3.0)
    g = torch.Generator().manual_seed(2)
    w, eps = torch.randn(3, 2, 16, generator=g, dtype=F64), 0.1 * torch.randn(3, 2, 20, generator=g, dtype=F64)
    resid, noise, fs = torch.randn(2, 20, generator=g, dtype=F64), torch.tensor([0.1, 0.3], dtype=F64), torch.full((2, 16), 0.3, dtype=F64)
    Wt = (w * fs[None]).permute(1, 2, 0)
    Khat = p.K(X, X) + noise[:, None, None] * torch.eye(20, dtype=F64)
    v = torch.linalg.solve(Khat, resid[:, :, None] - cm.rff_features(freq, phase, X) @ Wt - eps.permute(1, 2, 0))
    want = cm.paths_dense(p.K, X, resid, noise, freq, phase, fs, w, eps, Xs)
    assert torch.allclose(cdx.paths_latents(p.K, X, freq, phase, fs, w, v, Xs), want, rtol=1e-13, atol=1e-13)
