"""CPU tests of the host restatement of the split engine's fp16 scales (tests/_split_scales.py), of the C-ABI query that
locates the scale block in the Vd scratch, and of the library Makefile's header list."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import _split_scales as ss

F = np.float32


def _p2(k):
    return F(2.0 ** k)


def test_scale_for_puts_the_bound_at_two_to_the_13():
    # bound = f 2^e, f in [0.5, 1)  ->  2^(13 - e); the scaled bound lands in [2^12, 2^13)
    for bound, e in ((1.0, 1), (0.75, 0), (0.5, 0), (3.0, 2), (1e-30, -99), (4e4, 16)):
        assert ss.scale_for(bound) == _p2(13 - e), bound
        assert 2.0 ** 12 <= float(F(bound)) * float(ss.scale_for(bound)) < 2.0 ** 13


def test_hand_made_diagonal():
    # D = 3, lam = eig_lo = 0.01, amax = 0.5, n_pad = 256: Rn = 16 * 0.5 = 8
    n = 256
    diag = np.full(n, 2.0, dtype=F)
    diag[17] = 3.0
    aug = np.zeros((n, 128), dtype=F)
    aug[5, 3] = -0.5
    aug[200, 0] = 0.25
    s = ss.split_scales(diag, aug, 0.01)
    assert s["D"] == F(3.0) and s["lam"] == F(0.01) and s["amax"] == F(0.5) and s["Rn"] == F(8.0)
    # SU sqrt 3 = 1.73 (e 1); SW 1 / 0.1 = 10 (e 4); RU 3 (e 2); RW sqrt 300 = 17.3 (e 5); SA 8 / 0.1 = 80 (e 7);
    # RA 8 (1 + 17.3) = 146.6 (e 8)
    want = {"SU": 12, "SW": 9, "RU": 11, "RW": 8, "SA": 6, "RA": 5}
    for k, e in want.items():
        assert s[k] == _p2(e), (k, s[k])
    assert s["block"].dtype == F and s["block"].shape == (8,)
    assert list(s["block"][6:]) == [F(3.0), F(0.01)]


def test_lam_is_the_smaller_of_eig_lo_and_the_smallest_diagonal_entry():
    diag = np.array([5.0, 0.3, 2.0, 7.0], dtype=F)
    assert ss.split_scales(diag, None, 0.01)["lam"] == F(0.01)
    assert ss.split_scales(diag, None, 0.7)["lam"] == F(0.3)           # a diagonal entry below the caller's bound
    assert ss.split_scales(diag, None, 0.7)["D"] == F(7.0)


def test_lam_clamp_at_1e_12_d():
    diag = np.array([0.7, 0.55, 0.9], dtype=F)
    for eig_lo in (0.0, -1.0, 1e-14, float(F(1e-12) * F(0.9))):          # no usable bound, or not above 1e-12 D
        s = ss.split_scales(diag, None, eig_lo)
        assert s["lam"] == F(1e-12) * F(0.9), eig_lo
    s = ss.split_scales(diag, None, 1e-11)                               # a usable one stays
    assert s["lam"] == F(1e-11)
    s = ss.split_scales(diag, None, 0.0)
    # sqrt(D / lam) = 1e6: RW = 2^(13 - 20)
    assert s["RW"] == _p2(13 - 20) and s["SW"] == ss.scale_for(1.0 / math.sqrt(float(s["lam"])))


def test_zero_right_hand_side():
    diag = np.full(384, 1.3, dtype=F)
    for aug in (None, np.zeros((384, 256), dtype=F)):
        s = ss.split_scales(diag, aug, 0.2)
        assert s["amax"] == 0 and s["Rn"] == F(1e-30)
        assert s["SA"] == ss.scale_for(float(F(1e-30)) / math.sqrt(float(F(0.2))))
        assert s["RA"] == ss.scale_for(float(F(1e-30)) * (1 + math.sqrt(1.3 / 0.2)))


def test_padding_rows_count_as_one():
    n, n_pad = 300, 384
    diag = np.full(n, 0.8, dtype=F)                                      # outputscale + noise < 1
    pad = ss.split_scales(diag, None, 0.05, n_pad=n_pad)
    full = ss.split_scales(np.full(n_pad, 0.8, dtype=F), None, 0.05)
    assert pad["D"] == F(1.0) and full["D"] == F(0.8)                    # the identity padding raises D
    assert pad["RU"] == _p2(12) and full["RU"] == _p2(13)
    big = ss.split_scales(np.full(n, 5.0, dtype=F), None, 4.0, n_pad=n_pad)
    assert big["lam"] == F(1.0) and big["D"] == F(5.0)                   # ... and lowers lambda below a noise of 4
    # the padding enters Rn through sqrt(n_pad)
    aug = np.full((n, 1), 0.3, dtype=F)
    assert ss.split_scales(diag, aug, 0.05, n_pad=n_pad)["Rn"] == F(np.sqrt(F(n_pad)) * F(0.3) + F(1e-30))


def test_split_b3_scales_are_ones_and_the_tag_words():
    s = ss.split_scales(np.full(128, 2.0, dtype=F), None, 0.1, npl=3, vd_blocks=1234)
    assert list(s["block"]) == [1.0] * 8 and list(s["tag"]) == [3.0, 1234.0]
    s = ss.split_scales(np.full(128, 2.0, dtype=F), None, 0.1, npl=2, vd_blocks=77)
    assert list(s["tag"]) == [2.0, 77.0]


def test_bounds_near_a_power_of_two_are_refused_unless_exact():
    # D = 4: RU = 4 and SU = sqrt(4) = 2 are exact -- allowed
    s = ss.split_scales(np.full(128, 4.0, dtype=F), None, 0.3)
    assert s["RU"] == _p2(10) and s["SU"] == _p2(11)
    # D one ulp above 4: sqrt(D) is a rounded value within 1e-7 of 2 -- refused
    with pytest.raises(AssertionError, match="power of two"):
        ss.split_scales(np.full(128, np.nextafter(F(4.0), F(8.0)), dtype=F), None, 0.3)
    # 1 / sqrt(lam) within 1e-5 of 8
    with pytest.raises(AssertionError, match="power of two"):
        ss.split_scales(np.full(128, 3.0, dtype=F), None, float(F(1.0 / 64 * (1 + 4e-6))))


def test_aug_scales_restate_the_sweeps_augmented_scales():
    # k_aug_scales with the D and lambda of the sweep and the same augmented columns gives the sweep's SA and RA
    g = np.random.default_rng(0)
    diag = (0.6 + 0.3 * g.random(512)).astype(F)
    aug = (3 * g.standard_normal((512, 129))).astype(F)
    s = ss.split_scales(diag, aug, 0.07)
    assert ss.aug_scales(s["D"], s["lam"], aug, 512) == (s["SA"], s["RA"])
    sa, ra = ss.aug_scales(s["D"], s["lam"], aug * F(1e4), 512)           # 1e4 x the columns: about 13 binades lower
    assert sa < s["SA"] and ra < s["RA"]


def test_split_scales_offset_points_inside_the_scratch(repo_root):
    """plmc_split_scales_offset: 16-byte aligned, the whole 128 x 128-float scale block inside one latent's Vd slice of either size,
    ahead of the full-height planes of W (which sit behind that block when lda leaves room for the inverse factor)."""
    from projectedlmc import _hip
    lib = ctypes.CDLL(_hip.LIB_PATH)
    I64 = ctypes.c_int64
    for name, args in (("plmc_split_scales_offset", [I64, I64]), ("plmc_vd_blocks_for", [I64, I64, ctypes.c_int]),
                       ("plmc_vd_blocks_keep", [I64, I64])):
        getattr(lib, name).restype, getattr(lib, name).argtypes = I64, args
    for n_pad, lda in ((128, 384), (2304, 4864), (2304, 2432), (8192, 16512), (8320, 16768)):
        off = lib.plmc_split_scales_offset(n_pad, lda)
        nb2 = 128 * 128
        assert off % 4 == 0 and off >= (n_pad // 128) * nb2
        wk = (3 * (n_pad // 128) ** 2 + 1) // 2 if lda >= 2 * n_pad else 0       # blocks of the W planes (vd_layout.hpp)
        assert off + nb2 <= (lib.plmc_vd_blocks_for(n_pad, lda, 4) - wk) * nb2, (n_pad, lda)
        assert lib.plmc_vd_blocks_keep(n_pad, lda) >= lib.plmc_vd_blocks_for(n_pad, lda, 4)
    # the layout itself (csrc/vd_layout.hpp) is part of the ABI: these sizes and offsets are pinned
    # (n_pad, lda): vd_blocks_for(., ., 4), vd_blocks_for(., ., 8), vd_blocks_keep, split_scales_offset
    pinned = {(128, 384): (616, 313, 652, 10043392), (1024, 1152): (885, 368, 993, 14483456),
              (1024, 2176): (1333, 432, 1537, 20250624), (2304, 4736): (2613, 602, 3945, 34832384),
              (4096, 8320): (4909, 840, 8029, 55246848), (8192, 8320): (3405, 872, 9645, 55771136),
              (8192, 16512): (12365, 1384, 24749, 101908480)}
    for (n_pad, lda), want in pinned.items():
        got = (lib.plmc_vd_blocks_for(n_pad, lda, 4), lib.plmc_vd_blocks_for(n_pad, lda, 8), lib.plmc_vd_blocks_keep(n_pad, lda),
               lib.plmc_split_scales_offset(n_pad, lda))
        assert got == want, (n_pad, lda, got)


def test_makefile_lists_every_included_header(repo_root):
    """csrc/Makefile rebuilds an object when a header in HDRS changes: a header missing there ships stale objects."""
    csrc = os.path.join(repo_root, "projected-lmc_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    hdrs = set(re.search(r"^HDRS\s*=(.*)$", mk, re.M).group(1).split())
    included = set()
    for f in os.listdir(csrc):
        if f.endswith((".hip", ".hpp", ".inc")):
            included |= set(re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(os.path.join(csrc, f)).read(), re.M))
    assert included, "no quoted includes found"
    for h in included:
        assert os.path.exists(os.path.join(csrc, h)), h
    missing = sorted(included - hdrs)
    assert not missing, "csrc/Makefile HDRS lacks %s" % missing
