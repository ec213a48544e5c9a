// vd_layout.hpp -- the one description of the per-latent `Vd` scratch of the factorisation sweep (potrf.hip): where the sweep
// puts its group scratch, panel buffers, plane buffers and scales, and where the substitutions, the
// gradient (potri_grad.hip) and the C-ABI size queries find them.  No other file computes an offset into Vd; indexing by
// latent or, inside a region, by group is the caller's.
#pragma once
#include <stdint.h>

#include "gemm_core.hpp"

namespace plmc {

constexpr int GMAX = 8;                       // largest group (block rows; 16 was measured: 4 groups at n = 8192 pipeline too coarsely, 36.8 -> 38.8 ms at q = 8)
constexpr int LDG = (GMAX + 1) * NB;          // leading dimension of the group scratch matrices (Wg, Vg, Ph): an odd number of
                                              // 128-blocks, like lda -- a power-of-two row stride camps on a few L2 channels
// per-latent scratch behind the m inverse diagonal blocks of Vd: Wg + two Vg (ping-pong), GMAX^2 blocks each
// + the head panel buffer (GMAX^2 blocks) + the bulk panel buffer (GMAX block rows of lda / NB blocks)
constexpr int VD_FIXED_BLOCKS = 4 * GMAX * (GMAX + 1);

// The scale block of the split engine (one NB x NB block of floats per latent): the scales of the operand families (potrf.hip,
// k_split_scales), D and lambda at [6] [7], the partials of the diagonal / augmented scan (3 SCAN_PARTS floats from SC_N), and
// behind them the tag words: the scheme's planes per element and the per-latent stride in blocks
enum { SC_SU = 0, SC_SW = 1, SC_RU = 2, SC_RW = 3, SC_SA = 4, SC_RA = 5, SC_N = 8, SC_TAG = 8 + 3 * 32 };
constexpr int SCAN_PARTS = 32;
constexpr int VD_W_TAG = SC_TAG - SC_SW;   // floats from the W-family scale (vd_w_planes: *w_scale) to the scheme tag (planes per element) of that scratch

// NB x NB blocks (4-byte elements) of the full-height W planes inside Vd: 3 planes x 2 bytes x n_pad^2 (the three-plane
// scheme's size, whatever the scheme), only for 4-byte elements and a layout with inverse-factor columns (lda >= 2 n_pad)
inline int64_t vd_wk_blocks(int64_t n_pad, int64_t lda, int elem_bytes) {
  const int64_t m = n_pad / NB;
  return (elem_bytes == 4 && lda >= 2 * n_pad) ? (3 * m * m + 1) / 2 : 0;
}

// One latent's slice of Vd, region by region in the order they sit.  Offsets are in NB x NB blocks of elem_bytes-byte elements
// from the start of the slice; -1 = no such region in this layout.  The sizes depend on (n_pad, lda, elem_bytes, keep) only, never
// on a dev knob: for 4-byte elements the plane buffers are there whether or not the split engine runs, laid out for the
// three-plane scheme whatever the scheme.
//   diag     m inverses of the diagonal blocks of U (offset 0)
//   wg       the inverse triangle of the current group (GMAX block rows, leading dimension LDG); the resident chain's control
//            words sit in its pad column (CTR, CTL)
//   vg[2]    its transpose Vgg, ping-pong between groups (ld LDG)
//   ph       panel buffer of the head columns (fp32 / fp64 engine; ld LDG)
//   pbulk    panel buffer of the other columns (GMAX block rows, ld lda)
//   4-byte elements only, 16-bit planes in k8 order (bf3_engine.hpp):
//   pl[2]    rolling two-group buffer of the solved panel rows (128 GMAX rows x lda columns each: `plane_blocks`)
//            A sweep that pairs its tails (potrf.hip, Sweep::pair) rolls over FOUR slots instead, slot = group & 3, laid back to
//            back from the start of pbulk -- the split engine's group panel works in place and never uses pbulk -- so that the
//            rows of a pair of groups are one contiguous run of k8 rows: `slot_room` 16-bit elements in front of praw.  The
//            sizes and offsets of the layout (pinned as part of the ABI) do not change for it.
//   praw     the raw rows of the group whose panel comes next (one such buffer)
//   vgp[2]   planes of Vgg (128 GMAX x 128 GMAX), ping-pong like vg
//   scl      the scale block (SC_*)
//   wk       full-height planes of W (n_pad rows x n_pad columns), lda >= 2 n_pad only
//   uk       keep only: one buffer of `plane_blocks` per GMAX block rows, the solved panel rows of every group
struct VdLayout {
  // element offsets inside wg: row 0 of the pad column holds the chain's 2 GMAX^2 tile counters, row 1 (latent 0 of a chain
  // launch) [0] finished workgroups, [1] abort, [2] tickets
  static constexpr int64_t CTR = (int64_t)GMAX * NB, CTL = LDG + (int64_t)GMAX * NB;

  int elem_bytes;
  int64_t wg, vg[2], ph, pbulk;
  int64_t pl[2] = {-1, -1}, praw = -1, vgp[2] = {-1, -1}, scl = -1, wk = -1, uk = -1;
  int64_t plane_blocks = 0;
  int64_t blocks;                         // the per-latent size

  VdLayout(int64_t n_pad, int64_t lda, int elem_bytes_, bool keep) : elem_bytes(elem_bytes_) {
    const int64_t m = n_pad / NB, ldb = (lda + NB - 1) / NB, grp = GMAX * (GMAX + 1);
    wg = m;
    vg[0] = wg + grp;
    vg[1] = vg[0] + grp;
    ph = vg[1] + grp;
    pbulk = ph + grp;
    int64_t b = pbulk + GMAX * ldb;
    if (elem_bytes == 4) {
      plane_blocks = 3 * GMAX * ldb / 2;                  // 128 GMAX rows x 3 planes x lda x 2 bytes
      const int64_t vgp_blocks = 6 * GMAX * GMAX / 4;     // 3 x (128 GMAX)^2 x 2 bytes
      pl[0] = b;
      pl[1] = pl[0] + plane_blocks;
      praw = pl[1] + plane_blocks;
      vgp[0] = praw + plane_blocks;
      vgp[1] = vgp[0] + vgp_blocks;
      scl = vgp[1] + vgp_blocks;
      b = scl + 1;
      if (vd_wk_blocks(n_pad, lda, 4) > 0) {
        wk = b;
        b += vd_wk_blocks(n_pad, lda, 4);
      }
      if (keep) {
        uk = b;
        b += ((m + GMAX - 1) / GMAX) * plane_blocks;
      }
    }
    blocks = b;
  }
  // 16-bit elements between the start of pbulk and praw: room for the four slots of a sweep that pairs its tails
  int64_t slot_room() const { return praw < 0 ? 0 : (praw - pbulk) * (int64_t)NB * NB * 2; }
  int64_t stride() const { return blocks * NB * NB; }                         // per latent, in elements
  int64_t stride_u16() const { return stride() * (elem_bytes / 2); }           // ... in 16-bit plane elements
  int64_t stride_f32() const { return stride() * elem_bytes / 4; }             // ... in floats
  // region `blk` of latent 0 (V: the element type, elem_bytes wide), as a pointer to U; nullptr for a region the layout lacks
  template <class U, class V> U *at(V *Vd, int64_t blk) const {
    return blk < 0 ? nullptr : reinterpret_cast<U *>(Vd + blk * (int64_t)NB * NB);
  }
};

// Where a sweep of the split engine left the full-height planes of W and the scale of that operand family inside its `Vd`
// (potrf.hip; for kinv_grad_impl, potri_grad.hip).  False when the layout has no such planes.
bool vd_w_planes(const float *Vd, int64_t n_pad, int64_t lda, const unsigned short **wk, int64_t *wk_lat_stride, const float **w_scale,
                 int64_t *w_scale_lat_stride);

}  // namespace plmc
