"""The references and the bounds of the cross-covariance products (tests/_cross_matvec_ref.py) on their own, without a GPU, in the
pattern of test_gemm_ref_host.py:

  * an fp64 CPU product whose pair values are rounded to the element type stays inside the bound the GPU test asserts, for every family
    and both element types, read from a V buffer with NaN wherever the kernel must not read;
  * seeded mistakes a kernel could make leave it: the last training row dropped, the output scale omitted, `ldv` taken as `r`, one
    segment's partial sum added twice, and -- for the random-Fourier-feature product -- the fp32 phase formed without reduction at about
    2000 revolutions;
  * the library exports the entry points of every family and refuses bad arguments before any launch (no device is touched)."""
import ctypes

import pytest
import torch

import _cross_matvec_ref as cm

F32, F64 = torch.float32, torch.float64


def _setup(family, d, n, ns, q, r, ldv, seed, dtype):
    p = cm.problem(family, d, q, seed)
    X, Xs = cm.inputs(family, n, ns, d, seed)
    V = cm.columns(n, r, q, seed)
    return p, X, Xs, V, cm.v_buffer(V, n + 5, ldv, dtype)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("family", cm.FAMILIES)
def test_cpu_product_in_the_element_type_is_inside_the_bound(family, dtype):
    d = 3
    p, X, Xs, V, Vbuf = _setup(family, d, 300, 37, 2, 3, 5, 11, dtype)
    exact, bound = cm.reference(p, Xs, X, V, dtype)
    got = cm.cpu_product(p, Xs, X, Vbuf, 300, 3, 5, dtype)
    assert not bool(torch.isnan(got).any())
    print(family, dtype, "largest share of the bound: %.3f" % cm.worst_share(got, exact, bound))
    assert cm.violations(got, exact, bound) == 0


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("mutate", cm.MUTATIONS)
def test_seeded_mutations_leave_the_bound(mutate, dtype):
    n, ns, q, r, ldv = 600, 40, 2, 3, 5                               # three segments of 256 rows
    p = cm.problem("matern52", 3, q, 5)
    X, Xs = cm.inputs("matern52", n, ns, 3, 5)
    V = cm.columns(n, r, q, 5)
    Vbuf = cm.v_buffer(V, n + 5, ldv, dtype)
    if mutate == "ldv_as_r":                                           # (the mistaken stride walks into the padding: finite garbage there)
        Vbuf = torch.where(torch.isnan(Vbuf), torch.full_like(Vbuf, 0.37), Vbuf)
    exact, bound = cm.reference(p, Xs, X, V, dtype)
    assert cm.violations(cm.cpu_product(p, Xs, X, Vbuf, n, r, ldv, dtype), exact, bound) == 0
    bad = cm.violations(cm.cpu_product(p, Xs, X, Vbuf, n, r, ldv, dtype, mutate=mutate), exact, bound)
    print(mutate, dtype, "elements outside the bound:", bad, "of", q * ns * r)
    assert bad > q * ns * r // 2, (mutate, bad)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("d", [1, 3, 8])
def test_feature_product_meets_its_bound_at_large_phase(d, dtype):
    freq, phase, Wt, scale = cm.rff_problem(d, 100, 2, 3, seed=d, max_rev=2000.0)
    _, Xs = cm.inputs("rbf", 4, 33, d, seed=d)
    Xs[0] = 1.0                                                        # the last feature at 2000 revolutions
    assert float((freq[:, -1] * Xs[0]).sum(-1).max()) >= 1999.0
    exact, bound = cm.rff_reference(freq, phase, Xs, Wt, scale, dtype)
    assert cm.violations(cm.rff_cpu_product(freq, phase, Xs, Wt, scale, dtype), exact, bound) == 0


def test_unreduced_fp32_phase_leaves_the_bound():
    freq, phase, Wt, scale = cm.rff_problem(3, 100, 2, 3, seed=3, max_rev=2000.0)
    _, Xs = cm.inputs("rbf", 4, 33, 3, seed=3)
    exact, bound = cm.rff_reference(freq, phase, Xs, Wt, scale, F32)
    bad = cm.violations(cm.rff_cpu_product(freq, phase, Xs, Wt, scale, F32, mutate="unreduced_phase"), exact, bound)
    print("unreduced fp32 phase: elements outside the bound:", bad, "of", exact.numel())
    assert bad > exact.numel() // 2


def test_accurate_features_agree_with_a_wide_evaluation():
    """rff_features against mpmath-free wide arithmetic: the same cosines from integer-exact fractions (Python fractions)."""
    from fractions import Fraction
    import math
    freq, phase, _, _ = cm.rff_problem(2, 5, 1, 1, seed=9, max_rev=2000.0)
    _, Xs = cm.inputs("rbf", 2, 3, 2, seed=9)
    Phi = cm.rff_features(freq, phase, Xs)
    for s in range(3):
        for j in range(5):
            t = sum(Fraction(float(freq[0, j, k])) * Fraction(float(Xs[s, k])) for k in range(2)) + Fraction(float(phase[0, j]))
            frac = float(t - round(t))
            assert abs(float(Phi[0, s, j]) - math.cos(2 * math.pi * frac)) < 1e-14


def test_paths_dense_with_no_prior_draw_is_the_posterior_mean():
    p = cm.problem("matern52", 3, 2, 4)
    X, Xs = cm.inputs("matern52", 50, 7, 3, 4)
    g = torch.Generator().manual_seed(0)
    y = torch.randn(2, 50, generator=g, dtype=F64)
    noise = torch.tensor([0.1, 0.3], dtype=F64)
    freq, phase, _, _ = cm.rff_problem(3, 16, 2, 1, seed=1, max_rev=3.0)
    fs = torch.ones(2, 16, dtype=F64)
    out = cm.paths_dense(p.K, X, y, noise, freq, phase, fs, torch.zeros(4, 2, 16, dtype=F64), torch.zeros(4, 2, 50, dtype=F64), Xs)
    Khat = p.K(X, X) + noise[:, None, None] * torch.eye(50, dtype=F64)
    mean = (p.K(Xs, X) @ torch.linalg.solve(Khat, y[:, :, None]))[:, :, 0]
    assert torch.allclose(out, mean[:, :, None].expand(2, 7, 4), rtol=1e-12, atol=1e-12)


# ---------------------------------------------------------------------------------------------- the library, without a device
INFIXES = ("", "_add", "_sm", "_per", "_rq", "_lper", "_sum", "_dot")


@pytest.fixture(scope="module")
def L():
    from projectedlmc import _hip
    return _hip.lib().cdll


def test_library_exports_the_entry_points_of_every_family(L):
    for infix in INFIXES:
        for suf in ("_f32", "_f64"):
            assert getattr(L, "plmc_cross_matvec" + infix + suf) is not None
    for name in ("plmc_rff_matvec_f32", "plmc_rff_matvec_f64", "plmc_cross_matvec_max_cols", "plmc_cross_matvec_splits",
                 "plmc_cross_matvec_partials_bytes"):
        assert getattr(L, name) is not None
    assert L.plmc_version() == 4


def test_split_is_a_function_of_the_sizes(L):
    cap = L.plmc_cross_matvec_max_cols()
    assert cap in (8, 16)
    assert L.plmc_cross_matvec_splits(130, 37, 3) == 1 and L.plmc_cross_matvec_partials_bytes(130, 37, 3, 3) == 0
    assert L.plmc_cross_matvec_splits(256, 1, 1) == 1                  # one segment cannot be split
    s = L.plmc_cross_matvec_splits(700, 3, 3)
    assert s == 3 and L.plmc_cross_matvec_partials_bytes(700, 3, 2, 3) == 3 * 3 * 3 * 2 * 8   # one fp64 sum per segment of 256 rows
    assert L.plmc_cross_matvec_splits(8192, 16, 8) > L.plmc_cross_matvec_splits(8192, 2048, 8) >= 1
    assert L.plmc_cross_matvec_splits(8192, 131072, 8) == 1
    assert L.plmc_cross_matvec_splits(0, 3, 3) == 0 and L.plmc_cross_matvec_splits(5, 0, 3) == 0


def test_argument_errors_are_refused_before_any_launch(L):
    """Pointers are never dereferenced on a refused call: dummy non-null addresses stand in for device memory."""
    P = ctypes.c_void_p(4096)
    cap = L.plmc_cross_matvec_max_cols()

    def refused(word, kind=3, X=P, n=20, Xs=P, ns=4, d=3, ell=P, V=P, ldv=3, strideV=100, r=3, Out=P, part=None, q=2):
        rc = L.plmc_cross_matvec_f32(kind, X, n, Xs, ns, d, ell, None, V, ldv, strideV, r, Out, part, q, None)
        msg = L.plmc_last_error().decode()
        assert rc != 0 and word in msg, (word, rc, msg)

    for null in ("X", "Xs", "ell", "V", "Out"):
        refused("null pointer", **{null: None})
    refused("n > 0", n=0)
    refused("ns > 0", ns=0)
    refused("r > 0", r=0)
    refused("q <= 65535", q=0)
    refused("plmc_cross_matvec_max_cols", r=cap + 1, ldv=cap + 1)
    refused("ldv >= r", ldv=2)
    refused("strideV", strideV=3 * 19 + 2)
    refused("plmc_max_dim", d=33)
    refused("unknown kernel kind", kind=5)
    refused("partials", n=700, strideV=2100)                           # splits into three ranges, no scratch given
    fam = (ctypes.c_int * 2)(0, 16)
    for name, args, word in (("plmc_cross_matvec_add_f32", (3, P, 20, P, 4, 3, 5, P, None), "plmc_max_components"),
                             ("plmc_cross_matvec_add_f32", (4, P, 20, P, 4, 3, 2, P, None), "spline"),
                             ("plmc_cross_matvec_sm_f32", (P, 20, P, 4, 9, 2, P, P, None), "plmc_sm_max_dim"),
                             ("plmc_cross_matvec_per_f32", (P, 20, P, 4, 9, P, P, None), "plmc_per_max_dim"),
                             ("plmc_cross_matvec_rq_f32", (P, 20, P, 4, 17, P, P, None), "plmc_rq_max_dim"),
                             ("plmc_cross_matvec_lper_f32", (P, 20, P, 4, 9, P, P, P, None), "plmc_lper_max_dim"),
                             ("plmc_cross_matvec_sum_f32", (P, 20, P, 4, 9, 2, ctypes.cast(fam, ctypes.c_void_p), P, None), "plmc_sum_max_dim"),
                             ("plmc_cross_matvec_dot_f32", (P, 20, P, 4, 3, P, P, 9, None), "plmc_dot_max_power")):
        rc = getattr(L, name)(*args, P, 3, 100, 3, P, None, 2, None)
        msg = L.plmc_last_error().decode()
        assert rc != 0 and word in msg, (name, rc, msg)

    def rff_refused(word, freq=P, phase=P, m=10, Xs=P, ns=4, d=3, Wt=P, r=3, Out=P, part=None, q=2):
        rc = L.plmc_rff_matvec_f32(freq, phase, m, Xs, ns, d, Wt, r, None, Out, part, q, None)
        msg = L.plmc_last_error().decode()
        assert rc != 0 and word in msg, (word, rc, msg)

    for null in ("freq", "phase", "Xs", "Wt", "Out"):
        rff_refused("null pointer", **{null: None})
    rff_refused("n > 0", m=0)
    rff_refused("plmc_cross_matvec_max_cols", r=cap + 1)
    rff_refused("plmc_max_dim", d=33)
    rff_refused("partials", m=1030)
