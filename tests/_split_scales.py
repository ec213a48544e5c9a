"""Test helper: a host restatement, in numpy float32, of the power-of-two scales the two-plane fp16 split engine gives its
operand families (csrc/potrf.hip: k_scale_scan + k_split_scales, and k_aug_scales for the new augmented columns of a kept
factorisation; csrc/bf3_engine.hpp: b3_scale_for).  A sweep leaves them in a block of its Vd scratch
(plmc_split_scales_offset): [SU, SW, RU, RW, SA, RA, D, lam], and at SC_TAG the scheme's plane count and the per-latent
scratch stride in 128 x 128 blocks.

Only the exponent of each bound enters a scale, and the device's sqrt / division may differ from IEEE by an ulp (and a
multiply-add may be fused), so an input whose bound lies within MARGIN (relative) of a power of two is refused with an
assert -- unless every operation of that bound is exact (e.g. D itself, or sqrt(4)), which any faithful arithmetic
reproduces.  Tests pick their inputs away from those boundaries."""
import math

import numpy as np

F = np.float32
SC_SU, SC_SW, SC_RU, SC_RW, SC_SA, SC_RA, SC_D, SC_LAM = range(8)
SC_N = 8
SC_TAG = SC_N + 3 * 32                  # behind the 32 scan partials (3 floats each)
BLOCK = SC_TAG + 2                      # floats of the scale block the tests read
NAMES = ("SU", "SW", "RU", "RW", "SA", "RA", "D", "lam")
MARGIN = 1e-5
EPS_LAM = F(1e-12)                      # no usable eigenvalue bound: lambda = 1e-12 D
R_FLOOR = F(1e-30)                      # Rn of a zero right-hand side


def scale_for(bound):
    """b3_scale_for: the power of two that puts `bound` (> 0) at 2^13 -- with bound = f 2^e, f in [0.5, 1): 2^(13 - e)."""
    _, e = math.frexp(float(F(bound)))
    return F(math.ldexp(1.0, 13 - e))


class _V:
    """A value as float32 arithmetic computes it (f32), the same expression in float64 (f64) and whether every step so far
    was exact (the float32 result of each step equal to its float64 result)."""

    def __init__(self, f32, f64=None, exact=True):
        self.f32 = F(f32)
        self.f64 = float(self.f32) if f64 is None else float(f64)
        self.exact = exact and float(self.f32) == self.f64

    def _op(self, o, f32, f64):
        return _V(f32, f64, self.exact and (o.exact if isinstance(o, _V) else True))

    def sqrt(self):
        return self._op(None, np.sqrt(self.f32), math.sqrt(self.f64))

    def __truediv__(self, o):
        return self._op(o, self.f32 / o.f32, self.f64 / o.f64)

    def __rtruediv__(self, c):
        return self._op(None, F(c) / self.f32, float(F(c)) / self.f64)

    def __mul__(self, o):
        return self._op(o, self.f32 * o.f32, self.f64 * o.f64)

    def __add__(self, o):
        return self._op(o, self.f32 + o.f32, self.f64 + o.f64)

    def __radd__(self, c):
        return self._op(None, F(c) + self.f32, float(F(c)) + self.f64)


def _checked_scale(name, b):
    """scale_for(b.f32), after refusing a bound whose exponent an ulp could change."""
    assert b.f64 > 0 and math.isfinite(b.f64), (name, b.f64)
    if not b.exact:
        p = 2.0 ** round(math.log2(b.f64))
        assert abs(b.f64 / p - 1.0) > MARGIN, "bound %s = %.9g lies within %g of the power of two %g: pick another input" % (
            name, b.f64, MARGIN, p)
    s = scale_for(b.f32)
    assert s == scale_for(b.f64), (name, b.f32, b.f64)
    return s


def _diag_padded(diag, n_pad):
    d = np.asarray(diag, dtype=F).reshape(-1)
    n_pad = len(d) if n_pad is None else int(n_pad)
    assert len(d) <= n_pad
    return np.concatenate([d, np.ones(n_pad - len(d), dtype=F)]), n_pad      # identity padding: 1 on the diagonal


def _rn(aug, n_pad):
    amax = F(0) if aug is None or np.size(aug) == 0 else F(np.abs(np.asarray(aug, dtype=F)).max())
    return _V(F(n_pad)).sqrt() * _V(amax) + _V(R_FLOOR), amax


def split_scales(diag, aug, eig_lo, n_pad=None, npl=2, vd_blocks=None):
    """The scale block k_split_scales writes for one latent.
    diag: the input matrix's diagonal, n or n_pad entries (rows beyond them are identity padding: 1);
    aug: the augmented columns of the input (any rows / columns; absent ones are zero), None for none;
    eig_lo: the caller's lower bound of the smallest eigenvalue; npl: planes of the scheme (2: SplitH2, 3: SplitB3);
    vd_blocks: the per-latent Vd stride in 128 x 128 blocks (for the tag words).
    Returns a dict: D, lam, amax, Rn, the six scales by name, `block` (8 float32: SU SW RU RW SA RA D lam) and, with
    vd_blocks, `tag` (2 float32: npl, vd_blocks)."""
    d, n_pad = _diag_padded(diag, n_pad)
    out = {}
    if vd_blocks is not None:
        out["tag"] = np.array([npl, vd_blocks], dtype=F)
    if npl == 3:                                          # SplitB3 needs no scales
        out["block"] = np.ones(8, dtype=F)
        return out
    dmax = F(max(F(0), d.max()))
    dmin = F(min(F(3.0e38), d.min()))
    D = dmax if dmax > 0 else F(1)
    lam = F(min(F(eig_lo), dmin))
    if not lam > EPS_LAM * D:
        lam = F(EPS_LAM * D)
    Rn, amax = _rn(aug, n_pad)
    out.update(D=D, lam=lam, amax=amax, Rn=Rn.f32)
    out.update(_scales(_V(D), _V(lam), Rn))
    out["block"] = np.array([out[k] for k in NAMES], dtype=F)
    return out


def _scales(D, lam, Rn):
    sl = lam.sqrt()
    q = (D / lam).sqrt()
    return dict(SU=_checked_scale("SU", D.sqrt()), SW=_checked_scale("SW", 1.0 / sl), RU=_checked_scale("RU", D),
                RW=_checked_scale("RW", q), SA=_checked_scale("SA", Rn / sl), RA=_checked_scale("RA", Rn * (1.0 + q)))


def aug_scales(D, lam, aug, n_pad):
    """k_aug_scales: (SA, RA) for new augmented columns `aug` of a kept factorisation whose scale block holds D and lam."""
    Rn, _ = _rn(aug, n_pad)
    s = _scales(_V(D), _V(lam), Rn)
    return s["SA"], s["RA"]
