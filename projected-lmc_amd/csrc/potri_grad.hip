// potri_grad.hip -- K^-1 = W^T W on MFMA with the analytic MLL gradient fused into the epilogue.
//
// Replaces the autograd backward of cholesky + kernel chain that `loss.backward()`
// (experiments.py:270) runs through gpytorch:
//     d logp / d theta = 1/2 tr((alpha alpha^T - Khat^-1) dKhat/dtheta),   d logp / d y = -alpha.
// For each upper tile (ib <= jb) of K^-1 the workgroup accumulates the tile on MFMA, then,
// without writing it to HBM, re-derives dK/dtheta for the same (i,j) from X staged in LDS and
// reduces (alpha_i alpha_j - Kinv_ij) * dK_ij to d+2 partial sums.  A second tiny kernel sums the
// per-tile partials in a fixed order (deterministic, no float atomics).
#include <stdlib.h>
#include "api_common.hpp"
#include "covariance.hpp"
#include "bf3_engine.hpp"
#include "vd_layout.hpp"
#include "../../include/plmc.h"

namespace plmc {

constexpr int GP = MAX_DIM + 2;      // partial-sum slots per tile: d lengthscales, noise, outputscale

// ---- gradient epilogue for d <= 8 (DCAP in {4, 8}): the metric shape and every BASELINE config but the SARCOS one.
// The 64 accumulator registers stay live through the whole epilogue, so at 4 waves per SIMD (128 registers) the
// epilogue itself has to fit ~60: round 1's version kept 16 packed column pairs + 16 packed sums + 8 row values and
// spilled 80 bytes per lane (WRITE_SIZE 3.4 GB per launch for 9 MB of output).  Here the packed pairs are two
// DIMENSIONS of one element instead of two elements: 4 packed sums, 4 packed column values, 4 packed differences
// (kept for the second use: no recomputation), one scalar transcendental per element -- the same number of vector
// instructions per element, half the registers, no scratch (tools/resource_usage.py, profiles/r02_resource_usage.md).
// The loops are real loops: the 16 accumulator registers of one sub-tile row mt are parked in LDS -- each thread reads
// back only what it wrote, no barrier -- so that (nt, r) can be runtime indices.
// LDS plan (T elements), all inside tile_smem_elems():
//   ui [128][DCAP + 4], uj [128][DCAP + 4]   scaled inputs u = x / ell of the tile's rows / columns (0 beyond n and d)
//   ai [128], aj [128]                       alpha of rows / columns
//   accs[4 nt][256 threads][4 r]             the parked accumulator slice
template <int DCAP> struct GradLds {
  static constexpr int LDI = DCAP + 4;
  static constexpr int UI = 0, UJ = UI + NB * LDI, AI = UJ + NB * LDI, AJ = AI + NB, ACCS = AJ + NB, END = ACCS + 4 * NTHREADS * 4;
};

// INTERIOR: tile strictly above the diagonal, no padded rows or columns, nothing stored -- every element is live and
// counts twice, no per-element predicate.  Otherwise (diagonal tiles, ragged edge, K^-1 or its diagonal wanted):
//   weight 2 above the diagonal, 1 on it (where df = 0, so it adds nothing to the lengthscale sums), 0 below / outside n.
//     g[k] += os sum_ij wt w base df_k^2,   g_os += sum wt w val,   g_noise += sum_ii w,   w = alpha_i alpha_j - Kinv_ij.
template <typename T, int DCAP, int KIND, bool INTERIOR>
__device__ __forceinline__ void grad_tile_small(const Acc<T> &acc, T *smem, const int tid, T os, int ib, int jb, int n, int lat, int64_t n_pad,
                                                T *Kinv, int64_t ldk, int64_t strideK, T *kinv_diag, T (&g)[DCAP],
                                                T &g_noise, T &g_os) {
  typedef Pair<T> T2;
  typedef GradLds<DCAP> L;
  constexpr int NP = DCAP / 2;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  T2 g2[NP];
#pragma unroll
  for (int j = 0; j < NP; ++j) g2[j] = T2{T(0), T(0)};
  T gos = T(0), gnz = T(0);
  T *accs = smem + L::ACCS + tid * 4;
#pragma unroll 1
  for (int mt = 0; mt < 4; ++mt) {
    // park acc.v[mt][0..3] (static register indices per case)
#define PLMC_PARK(M)                                                                                    \
  _Pragma("unroll") for (int nt = 0; nt < 4; ++nt) _Pragma("unroll") for (int r = 0; r < 4; ++r)         \
      accs[nt * NTHREADS * 4 + r] = acc.v[M][nt][r];
    if (mt == 0) { PLMC_PARK(0) } else if (mt == 1) { PLMC_PARK(1) } else if (mt == 2) { PLMC_PARK(2) } else { PLMC_PARK(3) }
#undef PLMC_PARK
#pragma unroll 1
    for (int nt = 0; nt < 4; ++nt) {
      const int col = tile_col(wn, nt, lane);
      const T *ujc = smem + L::UJ + col * L::LDI;
      T2 u2[NP];
#pragma unroll
      for (int j = 0; j < NP; ++j) u2[j] = *reinterpret_cast<const T2 *>(ujc + 2 * j);
      const T a_j = smem[L::AJ + col];
      const int gj = jb * NB + col;
#pragma unroll 1
      for (int r = 0; r < 4; ++r) {
        const int row = tile_row<T>(wm, mt, lane, r);
        const T kin = accs[nt * NTHREADS * 4 + r];
        const T *uir = smem + L::UI + row * L::LDI;
        T2 df[NP];
        T2 r2p = {T(0), T(0)};
#pragma unroll
        for (int j = 0; j < NP; ++j) {
          df[j] = *reinterpret_cast<const T2 *>(uir + 2 * j) - u2[j];
          r2p += df[j] * df[j];
        }
        T val, base;
        if constexpr (KIND == K_SPLINE) {                // no lengthscale: the value only feeds the outputscale sum
          val = T(1);
#pragma unroll
          for (int j = 0; j < NP; ++j) {
            const T2 xr = *reinterpret_cast<const T2 *>(uir + 2 * j);
            val *= spline_factor(xr.x, u2[j].x) * spline_factor(xr.y, u2[j].y);
          }
          base = T(0);
        } else {
          kern_value_base_fast(KIND, r2p.x + r2p.y, val, base);
        }
        T w = smem[L::AI + row] * a_j - kin;
        if (!INTERIOR) {
          const int gi = ib * NB + row;
          if (Kinv && gj >= gi) Kinv[(int64_t)lat * strideK + (int64_t)gi * ldk + gj] = kin;
          if (kinv_diag && gi == gj) kinv_diag[(int64_t)lat * n_pad + gi] = kin;
          const bool live = gi < n && gj < n && gj >= gi;
          if (live && gi == gj) gnz += w;
          w = live ? (gj > gi ? T(2) * w : w) : T(0);
        }
        gos += w * val;
        const T c = w * base;
#pragma unroll
        for (int j = 0; j < NP; ++j) g2[j] += (c * df[j]) * df[j];
      }
    }
  }
  const T sc = INTERIOR ? T(2) * os : os;
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    g[2 * j] += sc * g2[j].x;
    g[2 * j + 1] += sc * g2[j].y;
  }
  g_os += INTERIOR ? T(2) * gos : gos;
  g_noise += gnz;
}

// occupancy floor: fp32 with up to 8 input dimensions fits 128 registers (4 waves per SIMD, as the update kernels)
template <typename T, int DCAP> constexpr int KG_MIN_WAVES = sizeof(T) == 8 ? 2 : (DCAP <= 8 ? 4 : (DCAP <= 16 ? 2 : 1));

// ---- gradient epilogue of one 128 x 128 tile (ib, jb) of K^-1 held in `acc` (the accumulator layout of the tile engines),
// as a function: for the halves of the 512-thread macro-tile kernel (tid = threadIdx.x & 255; each half on its own tile with
// its own `smem` of tile_smem_elems<T>() elements).  Both halves execute the same barriers; a half without a tile
// (live = false) stages zeros and writes nothing.  Body: kinv_epilogue.inc.
template <typename T, int DCAP, bool SPLINE>
__device__ __forceinline__ void kinv_tile_epilogue(const Acc<T> &acc, T *smem, const int tid, const bool live, int kind, int ib, int jb, int lat,
                                                   int m, int64_t n_pad, const T *__restrict__ alpha, const T *__restrict__ X, int n, int d,
                                                   const T *__restrict__ ell, const T *__restrict__ oscale, T *Kinv, int64_t ldk,
                                                   int64_t strideK, T *kinv_diag, double *__restrict__ partials) {
  if (!live) { n = 0; Kinv = nullptr; kinv_diag = nullptr; }       // every element predicate below is then false
  // 512 threads = two waves per SIMD = 256 registers: with 32 dimensions the one-pass form does not fit beside the accumulators
#define PLMC_KINV_KEEP (DCAP <= 16)
#include "kinv_epilogue.inc"
#undef PLMC_KINV_KEEP
}

// The part the 256-thread kernels share in front of their epilogue, as text (a function, even always inlined, changed the code of every
// one of them): declares m, the tile (ib, jb) of latent `lat` that this workgroup owns, `smem`, and that tile of K^-1 = W^T W in `acc`.
// Longest tiles first: jb ascending outermost, latent fastest.  A (jb, ib, lat) grid ran the long tiles of the last latent
// at the end of the launch: 112 vs 120 TF at n = 8192, q = 8, 97 vs 118 TF at q = 1, 77 vs 104 TF at n = 4096 (the same
// launch with every tile reading one panel pair ran no faster, so operand locality is not what limits it; an XCD-dealt
// super-tile order was level with the grid).
#define PLMC_KINV_TILE_PRODUCT                                                                                                                 \
  const int m = (int)(n_pad / NB);                                                                                                             \
  const int lat = (int)blockIdx.x % nlat;                                                                                                      \
  int ib, jb;                                                                                                                                  \
  tri_decode((int)blockIdx.x / nlat, ib, jb);                                                                                                  \
  __shared__ __align__(16) T smem[tile_smem_elems<T>()];                                                                                       \
  const T *Wl = W + (int64_t)lat * strideW + (int64_t)jb * NB * ldw;                                                                           \
  Acc<T> acc;                                                                                                                                  \
  acc.zero();                                                                                                                                  \
  tile_mainloop<T, false, true>(acc, Wl + (int64_t)ib * NB, ldw, Wl + (int64_t)jb * NB, ldw, (int)(n_pad - (int64_t)jb * NB), smem)

// SPLINE (general epilogue only): the product-form spline kernel gets its own instantiation, so that its extra live
// values do not raise the register pressure (and the scratch) of the stationary kernels' code.
template <typename T, int DCAP, bool SPLINE = false>
__global__ __launch_bounds__(NTHREADS, (KG_MIN_WAVES<T, DCAP>)) void k_kinv_grad(int kind, const T *__restrict__ W, int64_t n_pad, int64_t ldw,
                                                         int64_t strideW, const T *__restrict__ alpha,
                                                         const T *__restrict__ X, int n, int d,
                                                         const T *__restrict__ ell, const T *__restrict__ oscale,
                                                         T *Kinv, int64_t ldk, int64_t strideK, T *kinv_diag,
                                                         double *__restrict__ partials, int nlat) {
  PLMC_KINV_TILE_PRODUCT;
  // the epilogue body is textually included, not called: as an (always inlined) function it cost k_kinv_grad<float, 8>, which
  // sits at exactly 128 registers, 24 bytes of scratch per lane
  const int tid = threadIdx.x;
  constexpr bool live = true;
#define PLMC_KINV_KEEP (sizeof(T) == 4)
#include "kinv_epilogue.inc"
#undef PLMC_KINV_KEEP
}

// The part the split-engine kernels share in front of their epilogue, as text (see PLMC_KINV_TILE_PRODUCT): declares `lds`, m, the macro
// tile's two products combined in `acc0`, and the tile (ib, jb) of latent `lat` that this `half` (threadIdx.x >> 8) of the workgroup owns;
// returns from a workgroup without a macro tile.
// Latent-major: the ~256 resident workgroups are consecutive macro tiles of ONE matrix (a few block columns jb, all their
// ibm): 16 + 16 operand strips instead of one B and 32 A strips per XCD and latent -- the strips are shared across the XCDs
// through the Infinity Cache (step 18.5 -> 18.1 ms at q = 8 against latent fastest, the fp32 kernel's order)
// Tile order: XCD-dealt super-blocks of 4 macro rows x 8 block columns (= the 32 workgroups an XCD holds; workgroup w lands on
// XCD w % 8), longest K range first, latent by latent.  With the K range walked from its END (every range ends at row n) the
// 32 tiles of a block read their 4 A strips and 8 B strips in lockstep through one L2, and the blocks in flight on the eight
// XCDs belong to one or two matrices (Infinity Cache).  PMC, q = 8: 12.7 GB fetched per launch; the plain orders (latent
// fastest / latent by latent, forward walk) 14.7 / 26.4 GB at 5.1 / 4.7 ms against 4.7 ms here.
// Planes taken over from a sweep (ws_stride > 1): the per-latent stride of that scratch is the one the sweep recorded behind
// its scheme tag -- plmc_vd_blocks_for blocks, or plmc_vd_blocks_keep when the sweep kept its planes (with_inverse | 4).  They must be
// of THIS scheme -- a sweep without eig_lo followed by a K^-1 call with it (or a changed PLMC_SPLIT in between) would read
// three-plane rows as two-plane rows; the scale poisons the result instead.
#define PLMC_KINV_BF3_TILE_PRODUCT                                                                                                             \
  constexpr int LDS_BYTES = b3_lds_bytes<S>() > 2 * tile_smem_elems<float>() * (int)sizeof(float) ? b3_lds_bytes<S>() : 2 * tile_smem_elems<float>() * (int)sizeof(float); \
  __shared__ __align__(16) unsigned char lds[LDS_BYTES];                                                                                       \
  const int m = (int)(n_pad / NB);                                                                                                             \
  const int SJ = (m + 7) / 8, NSB = SJ * (SJ + 1) / 2;                                                                                         \
  const int w = blockIdx.x, xcd = w & 7, slot = w >> 3;                                                                                        \
  const int gb = xcd + 8 * (slot >> 5), in = slot & 31;                                                                                        \
  if (gb >= nlat * NSB) return;                                                                                                                \
  const int lat = gb / NSB;                                                                                                                    \
  int sa, sj;                                                                                                                                  \
  tri_decode(gb - lat * NSB, sa, sj);                                                                                                          \
  const int ibm = 2 * (4 * sa + (in >> 3)), jb = 8 * sj + (in & 7);                                                                            \
  if (jb >= m || ibm > jb) return;                                                                                                             \
  Acc<float> acc0, acc1;                                                                                                                       \
  acc0.zero();                                                                                                                                 \
  acc1.zero();                                                                                                                                 \
  if (ws_stride > 1) {                                                                                                                         \
    ws_stride = (int64_t)wscale[VD_W_TAG + 1] * NB * NB;                                                                                       \
    wp_lat_stride = 2 * ws_stride;                                                                                                             \
  }                                                                                                                                            \
  const unsigned short *Pl = Wp + (int64_t)lat * wp_lat_stride + b3_index<S>((int64_t)jb * NB, 0, 0, n_pad);                                   \
  b3_mainloop<S, 0, B3NoPre, true>(acc0, acc1, Pl + (int64_t)ibm * NB * 8, n_pad, Pl + (int64_t)jb * NB * 8, n_pad, (int)(n_pad - (int64_t)jb * NB), lds); \
  float ws = wscale[(int64_t)lat * ws_stride];                                                                                                 \
  if (ws_stride > 1 && wscale[(int64_t)lat * ws_stride + VD_W_TAG] != (float)S::NPL) ws = __builtin_nanf("");                                  \
  b3_combine<S>(acc0, acc1, 1.0f / (ws * ws));                                                                                                 \
  const int half = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 8);                                                                      \
  const int ib = ibm + half

// The same on the 16-bit matrix cores (fp32 only; bf3_engine.hpp): a workgroup of 512 threads takes the macro tile
// (ib, ib + 1) x jb of K^-1 = W^T W from the k8-ordered planes of W (`Wp`, n_pad columns per plane row, `wp_lat_stride` elements
// per latent: the planes the sweep left in its Vd scratch, or the ones k_split_w writes behind the partials), then each half of
// 256 threads runs the gradient epilogue on its own tile.
// `wscale`: per latent the power-of-two scale the planes of W were written with (SplitH2; SplitB3: ones).
template <class S, int DCAP, bool SPLINE = false>
__global__ __launch_bounds__(B3_NT, 2) void k_kinv_grad_bf3(int kind, int64_t n_pad, const float *__restrict__ alpha, const float *__restrict__ X, int n,
                                                            int d, const float *__restrict__ ell, const float *__restrict__ oscale, float *Kinv,
                                                            int64_t ldk, int64_t strideK, float *kinv_diag, double *__restrict__ partials, int nlat,
                                                            const unsigned short *__restrict__ Wp, const float *__restrict__ wscale,
                                                            int64_t wp_lat_stride, int64_t ws_stride) {
  PLMC_KINV_BF3_TILE_PRODUCT;
  kinv_tile_epilogue<float, DCAP, SPLINE>(acc0, reinterpret_cast<float *>(lds) + half * tile_smem_elems<float>(), (int)threadIdx.x & 255, ib <= jb, kind,
                                          ib, jb, lat, m, n_pad, alpha, X, n, d, ell, oscale, Kinv, ldk, strideK, kinv_diag, partials);
}


// ---- the table families: the two kernels above with the epilogue of their family F.
// COV_ADD (sum of `ncomp` <= MAX_COMP scaled stationary ARD kernels, kinv_epilogue_add.inc): one instantiation per element type / split
// scheme, DC = 0 -- the input dimension and the component count are run-time loop bounds there.  The single kernel (ncomp = 1) never
// comes here (kinv_grad_impl).
// COV_SM: a spectral-mixture kernel of up to DC input dimensions (kinv_epilogue_sm.inc): ncomp = its components, ell = its scales,
// oscale = its weights, `means` its means; `kind` is not looked at.
// COV_PER: a periodic kernel of up to DC input dimensions (kinv_epilogue_per.inc): ell = its lengthscales, `means` its periods, oscale (q)
// or null; `kind` and ncomp (1) are not looked at.
// COV_RQ: a rational-quadratic kernel of up to DC (1, 4, 8, 16) input dimensions (kinv_epilogue_rq.inc): ell = its lengthscales, `means` its alpha (q),
// oscale (q) or null; `kind` and ncomp (1) are not looked at.
// COV_DOT: a dot-product kernel of up to DC (1, 4, 8, 16) input dimensions (kinv_epilogue_dot.inc): ell = its variances, `means` its offset (q),
// oscale (q) or null, ncomp = its power; `kind` is not looked at.
// COV_LPER: a locally periodic kernel of up to DC (1, 4, 8) input dimensions (kinv_epilogue_lper.inc): ell = its periodic lengthscales,
// `means` its periods, `third` its RBF lengthscales, oscale (q) or null; `kind` and ncomp (1) are not looked at.  No other family reads
// `third`.
// COV_SUM: a heterogeneous sum of ncomp (2 .. MAX_COMP) members on up to DC (1, 4, 8) input dimensions (kinv_epilogue_sum.inc): `kind` =
// the members' 4-bit codes, ell = its table (q, ncomp, 3 d + 1), oscale (q, ncomp) or null; `means` and `third` are not looked at.
template <typename T, CovFamily F, int DC>
__device__ __forceinline__ void kinv_tile_epilogue_add(const Acc<T> &acc, T *smem, const int tid, const bool live, int kind, int ncomp, int ib, int jb,
                                                       int lat, int m, int64_t n_pad, const T *__restrict__ alpha, const T *__restrict__ X, int n, int d,
                                                       const T *__restrict__ ell, const T *__restrict__ oscale, T *Kinv, int64_t ldk,
                                                       int64_t strideK, T *kinv_diag, double *__restrict__ partials, const T *__restrict__ means,
                                                       const T *__restrict__ third) {
  if (!live) { n = 0; Kinv = nullptr; kinv_diag = nullptr; }       // every element predicate below is then false
#include "kinv_epilogue_table.inc"
}

template <typename T, CovFamily F, int DC = 0>
__global__ __launch_bounds__(NTHREADS, (table_min_waves<T, F, DC>())) void k_kinv_grad_add(int kind, int ncomp, const T *__restrict__ W, int64_t n_pad, int64_t ldw,
                                                                int64_t strideW, const T *__restrict__ alpha, const T *__restrict__ X, int n, int d,
                                                                const T *__restrict__ ell, const T *__restrict__ oscale, T *Kinv, int64_t ldk,
                                                                int64_t strideK, T *kinv_diag, double *__restrict__ partials, int nlat,
                                                                const T *__restrict__ means, const T *__restrict__ third) {
  PLMC_KINV_TILE_PRODUCT;
  const int tid = threadIdx.x;
  constexpr bool live = true;
#include "kinv_epilogue_table.inc"
}

template <class S, CovFamily F, int DC = 0>
__global__ __launch_bounds__(B3_NT, 2) void k_kinv_grad_add_bf3(int kind, int ncomp, int64_t n_pad, const float *__restrict__ alpha,
                                                                const float *__restrict__ X, int n, int d, const float *__restrict__ ell,
                                                                const float *__restrict__ oscale, float *Kinv, int64_t ldk, int64_t strideK,
                                                                float *kinv_diag, double *__restrict__ partials, int nlat,
                                                                const unsigned short *__restrict__ Wp, const float *__restrict__ wscale,
                                                                int64_t wp_lat_stride, int64_t ws_stride, const float *__restrict__ means,
                                                                const float *__restrict__ third) {
  PLMC_KINV_BF3_TILE_PRODUCT;
  kinv_tile_epilogue_add<float, F, DC>(acc0, reinterpret_cast<float *>(lds) + half * tile_smem_elems<float>(), (int)threadIdx.x & 255, ib <= jb, kind, ncomp,
                                       ib, jb, lat, m, n_pad, alpha, X, n, d, ell, oscale, Kinv, ldk, strideK, kinv_diag, partials, means, third);
}

// The tile walk of the reductions below, as text (see PLMC_KINV_TILE_PRODUCT): declares `lat` = blockIdx.x and leaves in red[grp * GP + slot]
// the sum of that slot of the partial-sum row at `row0` (in doubles) over group grp's share of the latent's upper tiles, the tiles `tstride`
// doubles apart.  1024 threads = 30 groups of GP = 34 slots; every group walks its tiles with 4 independent
// accumulators (the loads are latency-bound); fixed summation order throughout.
constexpr int RED_NT = 1024;
#define PLMC_REDUCE_TILES(tstride, row0)                                                      \
  __shared__ double red[RED_NT];                                                              \
  const int lat = blockIdx.x;                                                                 \
  const int ntile = m * m;                                                                    \
  const int slot = threadIdx.x % GP;                                                          \
  const int grp = threadIdx.x / GP;                                                           \
  constexpr int NG = RED_NT / GP;                                                             \
  double s[4] = {0.0, 0.0, 0.0, 0.0};                                                         \
  if (grp < NG) {                                                                             \
    const double *base = partials + (int64_t)lat * ntile * (tstride) + (row0) + slot;         \
    for (int t0 = grp; t0 < ntile; t0 += 4 * NG) {                                            \
      _Pragma("unroll") for (int u = 0; u < 4; ++u) {                                         \
        const int t = t0 + u * NG;                                                            \
        if (t < ntile) {                                                                      \
          const int ib = t / m, jb = t - ib * m;                                              \
          if (jb >= ib) s[u] += base[(int64_t)t * (tstride)];                                 \
        }                                                                                     \
      }                                                                                       \
    }                                                                                         \
  }                                                                                           \
  red[threadIdx.x] = (s[0] + s[1]) + (s[2] + s[3]);                                           \
  __syncthreads()
// ... and the total of slot threadIdx.x < GP over the groups, in their order
__device__ __forceinline__ double reduce_slot_total(const double *red) {
  double tot = 0.0;
  for (int gq = 0; gq < RED_NT / GP; ++gq) tot += red[gq * GP + threadIdx.x];
  return tot;
}

// grad[lat][k] = 1/2 * sum over upper tiles of partials, with the 1/ell_k factor for lengthscales.  grid (q).
template <typename T>
__global__ __launch_bounds__(RED_NT) void k_reduce_grad(const double *__restrict__ partials, int m, int d,
                                                        const T *__restrict__ ell, double *__restrict__ grad) {
  PLMC_REDUCE_TILES(GP, 0);
  if (threadIdx.x < GP) {
    const double tot = reduce_slot_total(red);
    const int k = threadIdx.x;
    if (k < d) grad[(int64_t)lat * (d + 2) + k] = 0.5 * tot / (double)ell[(int64_t)lat * d + k];
    else if (k == MAX_DIM) grad[(int64_t)lat * (d + 2) + d] = 0.5 * tot;
    else if (k == MAX_DIM + 1) grad[(int64_t)lat * (d + 2) + d + 1] = 0.5 * tot;
  }
}

// The reduction for the additive kernels: the tile's partials are `ncomp` rows of GP slots.  grid (q, ncomp).
// grad[lat]: [ d/d ell (ncomp x d) | d/d noise | d/d oscale (ncomp) ] -- for one component the
// layout of k_reduce_grad.  A dimension outside its component (ell = +inf) gets 0.5 * 0 / inf = 0.
// SM: the rows of kinv_epilogue_sm.inc, grad[lat]: [ d/d scales (ncomp x d) | d/d means (ncomp x d) | d/d noise | d/d weights (ncomp) ]
template <typename T, bool SM = false>
__global__ __launch_bounds__(RED_NT) void k_reduce_grad_add(const double *__restrict__ partials, int m, int d, int ncomp,
                                                            const T *__restrict__ ell, double *__restrict__ grad) {
  const int g = blockIdx.y;
  const int64_t tstride = (int64_t)ncomp * GP;
  PLMC_REDUCE_TILES(tstride, (int64_t)g * GP);
  if (threadIdx.x < GP) {
    const double tot = reduce_slot_total(red);
    const int k = threadIdx.x;
    if constexpr (SM) {
      double *gl = grad + (int64_t)lat * (ncomp * (2 * d + 1) + 1);
      if (k < d) gl[g * d + k] = -2.0 * SM_2PI2 * 0.5 * tot;
      else if (k >= SM_MAX_DIM && k < SM_MAX_DIM + d) gl[(ncomp + g) * d + k - SM_MAX_DIM] = -SM_2PI * 0.5 * tot;
      else if (k == MAX_DIM && g == 0) gl[2 * ncomp * d] = 0.5 * tot;
      else if (k == MAX_DIM + 1) gl[2 * ncomp * d + 1 + g] = 0.5 * tot;
      return;
    }
    double *gl = grad + (int64_t)lat * (ncomp * (d + 1) + 1);
    if (k < d) gl[g * d + k] = 0.5 * tot / (double)ell[((int64_t)lat * ncomp + g) * d + k];
    else if (k == MAX_DIM && g == 0) gl[ncomp * d] = 0.5 * tot;
    else if (k == MAX_DIM + 1) gl[ncomp * d + 1 + g] = 0.5 * tot;
  }
}

// The reduction for the periodic kernel: one row of GP slots per tile (kinv_epilogue_per.inc).  grid (q).
// grad[lat]: [ d/d ell (d) | d/d period (d) | d/d noise | d/d oscale ], with the factors the epilogue left out.
template <typename T>
__global__ __launch_bounds__(RED_NT) void k_reduce_grad_per(const double *__restrict__ partials, int m, int d, const T *__restrict__ ell,
                                                            const T *__restrict__ period, double *__restrict__ grad) {
  PLMC_REDUCE_TILES(GP, 0);
  if (threadIdx.x < GP) {
    const double tot = reduce_slot_total(red);
    const int k = threadIdx.x;
    double *gl = grad + (int64_t)lat * (2 * d + 2);
    if (k < d) {
      const double l = (double)ell[(int64_t)lat * d + k];
      gl[k] = 0.5 * tot / (l * l);
    } else if (k >= PER_MAX_DIM && k < PER_MAX_DIM + d) {
      const int kk = k - PER_MAX_DIM;
      const double l = (double)ell[(int64_t)lat * d + kk], p = (double)period[(int64_t)lat * d + kk];
      gl[d + kk] = 0.5 * tot * SM_2PI / (l * p * p);
    } else if (k == MAX_DIM) gl[2 * d] = 0.5 * tot;
    else if (k == MAX_DIM + 1) gl[2 * d + 1] = 0.5 * tot;
  }
}

// The reduction for the rational-quadratic kernel: one row of GP slots per tile (kinv_epilogue_rq.inc).  grid (q).
// grad[lat]: [ d/d ell (d) | d/d alpha | d/d noise | d/d oscale ], with the factor 1 / ell_k and the sign of d/d alpha the epilogue left out.
template <typename T>
__global__ __launch_bounds__(RED_NT) void k_reduce_grad_rq(const double *__restrict__ partials, int m, int d, const T *__restrict__ ell,
                                                           double *__restrict__ grad) {
  PLMC_REDUCE_TILES(GP, 0);
  if (threadIdx.x < GP) {
    const double tot = reduce_slot_total(red);
    const int k = threadIdx.x;
    double *gl = grad + (int64_t)lat * (d + 3);
    if (k < d) gl[k] = 0.5 * tot / (double)ell[(int64_t)lat * d + k];
    else if (k == RQ_MAX_DIM) gl[d] = -0.5 * tot;
    else if (k == MAX_DIM) gl[d + 1] = 0.5 * tot;
    else if (k == MAX_DIM + 1) gl[d + 2] = 0.5 * tot;
  }
}

// The reduction for the dot-product kernel: one row of GP slots per tile (kinv_epilogue_dot.inc).  grid (q).
// grad[lat]: [ d/d v (d) | d/d c | d/d noise | d/d oscale ]; the epilogue left no factor out.
__global__ __launch_bounds__(RED_NT) void k_reduce_grad_dot(const double *__restrict__ partials, int m, int d, double *__restrict__ grad) {
  PLMC_REDUCE_TILES(GP, 0);
  if (threadIdx.x < GP) {
    const double tot = reduce_slot_total(red);
    const int k = threadIdx.x;
    double *gl = grad + (int64_t)lat * (d + 3);
    if (k < d) gl[k] = 0.5 * tot;
    else if (k == DOT_MAX_DIM) gl[d] = 0.5 * tot;
    else if (k == MAX_DIM) gl[d + 1] = 0.5 * tot;
    else if (k == MAX_DIM + 1) gl[d + 2] = 0.5 * tot;
  }
}

// The reduction for the locally periodic kernel: one row of GP slots per tile (kinv_epilogue_lper.inc).  grid (q).
// grad[lat]: [ d/d ell (d) | d/d period (d) | d/d lam (d) | d/d noise | d/d oscale ], with the factors the epilogue left out.  A factor
// that is switched off (ell = +inf or lam = +inf) gets finite sum / inf = exactly 0.
template <typename T>
__global__ __launch_bounds__(RED_NT) void k_reduce_grad_lper(const double *__restrict__ partials, int m, int d, const T *__restrict__ ell,
                                                             const T *__restrict__ period, const T *__restrict__ rbf_ell,
                                                             double *__restrict__ grad) {
  PLMC_REDUCE_TILES(GP, 0);
  if (threadIdx.x < GP) {
    const double tot = reduce_slot_total(red);
    const int k = threadIdx.x, kk = k % LPER_MAX_DIM;
    double *gl = grad + (int64_t)lat * (3 * d + 2);
    if (k < 3 * LPER_MAX_DIM && kk < d) {
      const double l = (double)ell[(int64_t)lat * d + kk];
      if (k < LPER_MAX_DIM) gl[kk] = 0.5 * tot / (l * l);
      else if (k < 2 * LPER_MAX_DIM) {
        const double p = (double)period[(int64_t)lat * d + kk];
        gl[d + kk] = 0.5 * tot * SM_2PI / (l * p * p);
      } else gl[2 * d + kk] = 0.5 * tot / (double)rbf_ell[(int64_t)lat * d + kk];
    } else if (k == MAX_DIM) gl[3 * d] = 0.5 * tot;
    else if (k == MAX_DIM + 1) gl[3 * d + 1] = 0.5 * tot;
  }
}

// The reduction for the heterogeneous sum: the tile's partials are `ncomp` rows of GP slots, each in the slot layout of its member's
// family (kinv_epilogue_sum.inc; for one component: the row that family's own kernel writes).  grid (q, ncomp).
// grad[lat]: [ d/d table (ncomp x (3 d + 1), in table layout) | d/d noise | d/d oscale (ncomp) ], each entry with the scaling of its
// family's reduction (k_reduce_grad, _per, _rq, _lper); a slot its member does not own is written as exactly 0.
template <typename T>
__global__ __launch_bounds__(RED_NT) void k_reduce_grad_sum(const double *__restrict__ partials, int m, int d, int ncomp, int fams,
                                                            const T *__restrict__ table, double *__restrict__ grad) {
  const int g = blockIdx.y;
  const int64_t tstride = (int64_t)ncomp * GP;
  PLMC_REDUCE_TILES(tstride, (int64_t)g * GP);
  const int f = (fams >> (4 * g)) & 15;
  const int rec = 3 * d + 1, j = threadIdx.x;
  double *gl = grad + (int64_t)lat * (ncomp * (rec + 1) + 1);
  const T *tb = table + ((int64_t)lat * ncomp + g) * rec;
  const auto total = [&](int slot) {
    double tot = 0.0;
    for (int gq = 0; gq < RED_NT / GP; ++gq) tot += red[gq * GP + slot];
    return tot;
  };
  if (j < rec) {                         // one table slot per thread: row 0 ell, 1 period, 2 rbf_ell (d each), then alpha
    const int row = j / d, kk = j - row * d;
    double v = 0.0;
    if (row == 0) {
      const double tot = total(kk), l = (double)tb[kk];
      v = (f == F_PER || f == F_LPER) ? 0.5 * tot / (l * l) : 0.5 * tot / l;
    } else if (row == 1 && (f == F_PER || f == F_LPER)) {
      const double tot = total(SUM_MAX_DIM + kk), l = (double)tb[kk], p = (double)tb[d + kk];
      v = 0.5 * tot * SM_2PI / (l * p * p);
    } else if (row == 2 && f == F_LPER) {
      v = 0.5 * total(2 * SUM_MAX_DIM + kk) / (double)tb[2 * d + kk];
    } else if (row == 3 && f == F_RQ) {
      v = -0.5 * total(RQ_MAX_DIM);
    }
    gl[g * rec + j] = v;
  } else if (j == MAX_DIM) {
    if (g == 0) gl[ncomp * rec] = 0.5 * total(MAX_DIM);
  } else if (j == MAX_DIM + 1) {
    gl[ncomp * rec + 1 + g] = 0.5 * total(MAX_DIM + 1);
  }
}

// Split of the inverse factor for the split-engine gradient kernel: W (fp32, lower block triangle: block (lb, cb) with
// cb <= lb) -> k8-ordered planes Wp[latent][k / 8][plane][n_pad columns][k % 8] (bf3_engine.hpp), every value times the
// latent's scale `wscale` (SplitH2: 2^13 / bound of |W|, written by k_w_scale; SplitB3: 1).
// grid (m, m, q), one 128 x 128 block per workgroup; HBM-bound (4 bytes read, 2 NPL written per element).
template <class S>
__global__ __launch_bounds__(NTHREADS) void k_split_w(const float *__restrict__ W, int64_t n_pad, int64_t ldw, int64_t strideW,
                                                      unsigned short *__restrict__ Wp, const float *__restrict__ wscale) {
  const int cb = blockIdx.x, lb = blockIdx.y, lat = blockIdx.z;
  if (cb > lb) return;
  b3_split_block<S, false>(W + (int64_t)lat * strideW + (int64_t)lb * NB * ldw + (int64_t)cb * NB, ldw,
                           Wp + (int64_t)lat * b3_elems<S>(n_pad, n_pad) + b3_index<S>((int64_t)lb * NB, 0, (int64_t)cb * NB, n_pad), n_pad, wscale[lat],
                           nullptr, 0, threadIdx.x);
}
// wscale[lat] = scale for |W_ij| <= 1 / sqrt(lambda_min(Khat)) <= 1 / sqrt(eig_lo[lat])  (SplitB3 / no bound: 1); the identity
// padding of the rows beyond n has eigenvalue 1 whatever the noise (`padded`).  1 x q threads.
template <class S>
__global__ void k_w_scale(const float *__restrict__ eig_lo, float *__restrict__ wscale, int q, int padded) {
  const int lat = threadIdx.x;
  if (lat >= q) return;
  if constexpr (S::NPL == 3) wscale[lat] = 1.0f;
  else {
    float lam = fmaxf(eig_lo[lat], 1e-30f);
    if (padded) lam = fminf(lam, 1.0f);
    wscale[lat] = b3_scale_for(1.0f / sqrtf(lam));
  }
}

// The family's reduction of the per-tile partial sums (`part`: table.partials_rows() rows of GP slots per tile) into its gradient table
template <typename T>
void launch_reduce_grad(const CovTable &table, const double *part, int m, int q, double *grad, hipStream_t st) {
  const int d = table.d, ncomp = table.ncomp;
  const T *ell = (const T *)table.ell, *second = (const T *)table.second, *third = (const T *)table.third;
  ProfScope ps(PK_REDUCE, st, 0.0, (double)m * m * q * table.partials_rows() * GP * sizeof(double) / 2);
  switch (table.route()) {
    case COV_PER: hipLaunchKernelGGL(k_reduce_grad_per<T>, dim3(q), dim3(RED_NT), 0, st, part, m, d, ell, second, grad); break;
    case COV_LPER: hipLaunchKernelGGL(k_reduce_grad_lper<T>, dim3(q), dim3(RED_NT), 0, st, part, m, d, ell, second, third, grad); break;
    case COV_SUM: hipLaunchKernelGGL(k_reduce_grad_sum<T>, dim3(q, ncomp), dim3(RED_NT), 0, st, part, m, d, ncomp, table.fams, ell, grad); break;
    case COV_RQ: hipLaunchKernelGGL(k_reduce_grad_rq<T>, dim3(q), dim3(RED_NT), 0, st, part, m, d, ell, grad); break;
    case COV_DOT: hipLaunchKernelGGL(k_reduce_grad_dot, dim3(q), dim3(RED_NT), 0, st, part, m, d, grad); break;
    case COV_SM: hipLaunchKernelGGL((k_reduce_grad_add<T, true>), dim3(q, ncomp), dim3(RED_NT), 0, st, part, m, d, ncomp, ell, grad); break;
    case COV_ADD: hipLaunchKernelGGL((k_reduce_grad_add<T, false>), dim3(q, ncomp), dim3(RED_NT), 0, st, part, m, d, ncomp, ell, grad); break;
    case COV_PLAIN: hipLaunchKernelGGL(k_reduce_grad<T>, dim3(q), dim3(RED_NT), 0, st, part, m, d, ell, grad);
  }
}

// `call(member table, its gradient table, check_only)` runs the member family's gradient path, or its argument checks alone (below)
template <typename T, class Call>
int sum_single_member(const CovTable &t, int64_t n_pad, int q, double *grad, void *partials, void *stream, Call call);

// S: split scheme of the W^T W products (void: MFMA of the element type); eig_lo: see potrf_impl.
// `partials` is table.partials_rows() rows of GP slots per tile and `grad` as wide as the family's reduction kernel writes it.
// check_only: return after the argument checks, before the first launch (sum_single_member).
template <typename T, class S>
int kinv_grad_impl(const CovTable &table, const T *W, int64_t n_pad, int64_t ldw, int64_t strideW, const T *alpha, const T *X, int n, double *grad,
                   T *Kinv, int64_t ldk, int64_t strideK, T *kinv_diag, void *partials, int q, const float *eig_lo, void *stream,
                   const float *Vd = nullptr, int64_t lda_vd = 0, bool check_only = false) {
  PLMC_REQUIRE_TABLE(table);
  const CovFamily family = table.route();
  const int kind = table.kernel_kind(), d = table.d, ncomp = table.ncomp, rows = table.partials_rows();
  const T *ell = (const T *)table.ell, *oscale = (const T *)table.oscale, *second = (const T *)table.second, *third = (const T *)table.third;
  PLMC_REQUIRE(table.kind >= 0 && table.kind <= 4, "unknown kernel kind");
  PLMC_REQUIRE(W && alpha && X && ell && grad && partials, "null pointer");
  PLMC_REQUIRE(n_pad > 0 && n_pad % NB == 0 && ldw % NB == 0 && n <= n_pad && n > n_pad - NB, "n_pad must be plmc_pad(n)");
  PLMC_REQUIRE(d > 0 && d <= MAX_DIM && q > 0, "need 0<d<=plmc_max_dim(), q>0");
  PLMC_REQUIRE(!Kinv || (ldk >= n_pad), "ldk too small");
  PLMC_REQUIRE(aligned16(W), "unaligned W");
  hipStream_t st = (hipStream_t)stream;
  const int m = (int)(n_pad / NB);
  double *part = reinterpret_cast<double *>(partials);
  const double np = (double)n_pad;
  // split engine (bf3_engine.hpp): split W into k8-ordered planes behind the partials (and the q scales behind the
  // planes), then the macro-tile kernel
  if constexpr (!std::is_void<S>::value) {
    PLMC_REQUIRE(q <= 1024, "too many latents for one scale launch");
    // the planes of W and the scale of that operand family: the ones the sweep left in its Vd scratch (plmc_kinv_grad_vd_*:
    // same scheme, since both calls see the same knob and the same eig_lo) -- or split W now, behind the partials
    const unsigned short *wp = nullptr;
    const float *wsc = nullptr;
    int64_t wp_lat = b3_elems<S>(n_pad, n_pad), ws_lat = 1;
    const bool from_vd = Vd && vd_w_planes(Vd, n_pad, lda_vd, &wp, &wp_lat, &wsc, &ws_lat);
    if (!from_vd) {
      if (const char *noun = table.vd_noun()) {
        char msg[160];
        snprintf(msg, sizeof(msg), "the %s gradient call takes the planes of W from the sweep's Vd (factorise with the inverse factor)", noun);
        return fail(__func__, msg);
      }
    }
    if (check_only) return 0;
    if (!from_vd) {
      char *pb = reinterpret_cast<char *>(partials) + (int64_t)m * m * q * rows * GP * (int64_t)sizeof(double);
      unsigned short *wpo = reinterpret_cast<unsigned short *>(pb);
      float *wsco = reinterpret_cast<float *>(pb + (int64_t)q * b3_elems<SplitB3>(n_pad, n_pad) * 2);
      hipLaunchKernelGGL((k_w_scale<S>), dim3(1), dim3(q < 64 ? 64 : ((q + 63) / 64) * 64), 0, st, eig_lo, wsco, q, (int)(n < n_pad));
      ProfScope ps(PK_SPLIT, st, 0.0, (double)q * np * np / 2 * (4 + 2 * S::NPL));
      hipLaunchKernelGGL((k_split_w<S>), dim3(m, m, q), dim3(NTHREADS), 0, st, (const float *)W, n_pad, ldw, strideW, wpo, (const float *)wsco);
      wp = wpo;
      wsc = wsco;
      wp_lat = b3_elems<S>(n_pad, n_pad);
      ws_lat = 1;
    }
    const int SJ = (m + 7) / 8, NSB = SJ * (SJ + 1) / 2;
    const dim3 gridb(8 * ((q * NSB + 7) / 8) * 32);                       // XCD-dealt super-blocks of 32 macro tiles (see the kernel)
#define PLMC_LAUNCH_KB(DC, SP) \
  hipLaunchKernelGGL((k_kinv_grad_bf3<S, DC, SP>), gridb, dim3(B3_NT), 0, st, kind, n_pad, alpha, X, n, d, ell, oscale, Kinv, ldk, strideK, kinv_diag, \
                     part, q, wp, wsc, wp_lat, ws_lat)
#define PLMC_LAUNCH_TB(F, DC) \
  hipLaunchKernelGGL((k_kinv_grad_add_bf3<S, F, DC>), gridb, dim3(B3_NT), 0, st, kind, ncomp, n_pad, alpha, X, n, d, ell, oscale, Kinv, ldk, strideK, \
                     kinv_diag, part, q, wp, wsc, wp_lat, ws_lat, (const float *)second, (const float *)third)
    ProfScope ps(PK_KINV_GRAD, st, q * np * np * np / 3.0, q * (np * np / 2) * sizeof(T));
    switch (family) {                                      // (table families first, here and below: the order of the kernels in the code object)
      default:                                             // beside the planes: DC = 1 only, except RQ / DOT beside two (FamilyTraits::split_max_d)
        with_capacity<S::NPL>(family, d, [&](auto f, auto dc) { PLMC_LAUNCH_TB(decltype(f)::value, decltype(dc)::value); });
        break;
      case COV_ADD: PLMC_LAUNCH_TB(COV_ADD, 0); break;
      case COV_PLAIN:
        if (d <= 4) PLMC_LAUNCH_KB(4, false);
        else if (d <= 8) PLMC_LAUNCH_KB(8, false);
        else if (d <= 16) { if (kind == K_SPLINE) PLMC_LAUNCH_KB(16, true); else PLMC_LAUNCH_KB(16, false); }
        else { if (kind == K_SPLINE) PLMC_LAUNCH_KB(32, true); else PLMC_LAUNCH_KB(32, false); }
    }
#undef PLMC_LAUNCH_TB
#undef PLMC_LAUNCH_KB
  } else {
    if (check_only) return 0;
    const dim3 grid(q * (m * (m + 1) / 2)), block(NTHREADS);          // longest tiles first (see the kernel)
#define PLMC_LAUNCH_KG(DC, SP)                                                                                       \
  hipLaunchKernelGGL((k_kinv_grad<T, DC, SP>), grid, block, 0, st, kind, W, n_pad, ldw, strideW, alpha, X, n, d, ell, \
                     oscale, Kinv, ldk, strideK, kinv_diag, part, q)
#define PLMC_LAUNCH_TG(F, DC) \
  hipLaunchKernelGGL((k_kinv_grad_add<T, F, DC>), grid, block, 0, st, kind, ncomp, W, n_pad, ldw, strideW, alpha, X, n, d, ell, oscale, Kinv, ldk, \
                     strideK, kinv_diag, part, q, second, third)
    ProfScope ps(PK_KINV_GRAD, st, q * np * np * np / 3.0, q * (np * np / 2) * sizeof(T));
    switch (family) {
      default: with_capacity<0>(family, d, [&](auto f, auto dc) { PLMC_LAUNCH_TG(decltype(f)::value, decltype(dc)::value); }); break;
      case COV_ADD: PLMC_LAUNCH_TG(COV_ADD, 0); break;
      case COV_PLAIN:
        if (d <= 4) PLMC_LAUNCH_KG(4, false);
        else if (d <= 8) PLMC_LAUNCH_KG(8, false);
        else if (d <= 16) { if (kind == K_SPLINE) PLMC_LAUNCH_KG(16, true); else PLMC_LAUNCH_KG(16, false); }
        else { if (kind == K_SPLINE) PLMC_LAUNCH_KG(32, true); else PLMC_LAUNCH_KG(32, false); }
    }
#undef PLMC_LAUNCH_TG
#undef PLMC_LAUNCH_KG
  }
  launch_reduce_grad<T>(table, part, m, q, grad, st);
  return launch_status(__func__);
}


// ---- leave-one-out pseudo-likelihood: the gradient epilogues above behind another tile product.
// d L_loo / d Khat = G with 2 G = beta beta^T - Xop^T Xop ("Leave-one-out objective"): Xop is the full symmetric Khat^-1 with
// scaled rows and one more row, krows x n_pad per latent, K-major like W.  So the tile (ib, jb) is the product of the two column strips
// over ALL krows rows (W^T W stops at the diagonal block: W is triangular, Xop is not), `beta` is staged where alpha was, and the epilogue
// text reduces (beta_i beta_j - acc_ij) dKhat_ij / dtheta exactly as it does for the marginal likelihood; nothing is stored.
// Every tile has the same depth, so the order is the XCD-dealt one of gemm_core.hpp: the 64 tiles of a super-block stream their 8 + 8
// strips through one L2.  fp32 runs on v_mfma_f32_16x16x4_f32 (no split engine for this product).
#define PLMC_LOO_TILE_PRODUCT                                                                                                                  \
  const int m = (int)(n_pad / NB);                                                                                                             \
  int lat, ib, jb;                                                                                                                             \
  if (!xcd_tri_decode((int)blockIdx.x, m, nlat, lat, ib, jb)) return;                                                                          \
  __shared__ __align__(16) T smem[tile_smem_elems<T>()];                                                                                       \
  const T *Xl = Xop + (int64_t)lat * strideX;                                                                                                  \
  Acc<T> acc;                                                                                                                                  \
  acc.zero();                                                                                                                                  \
  tile_mainloop<T, false, false>(acc, Xl + (int64_t)ib * NB, ldx, Xl + (int64_t)jb * NB, ldx, (int)krows, smem);                               \
  const T *__restrict__ alpha = beta;                                                                                                          \
  T *const Kinv = nullptr, *const kinv_diag = nullptr;                                                                                         \
  constexpr int64_t ldk = 0, strideK = 0;                                                                                                      \
  const int tid = threadIdx.x;                                                                                                                 \
  constexpr bool live = true

// occupancy floor: that of k_kinv_grad, except fp32 with 5..8 dimensions -- k_kinv_grad<float, 8> sits at exactly 128 registers, and behind
// this tile product the same epilogue text needs a few more: at 4 waves per SIMD it would spill 24 bytes per lane, at 3 it does not
template <typename T, int DCAP> constexpr int LOO_MIN_WAVES = (sizeof(T) == 4 && DCAP == 8) ? 3 : KG_MIN_WAVES<T, DCAP>;

template <typename T, int DCAP, bool SPLINE = false>
__global__ __launch_bounds__(NTHREADS, (LOO_MIN_WAVES<T, DCAP>)) void k_loo_grad(int kind, const T *__restrict__ Xop, int64_t n_pad, int64_t krows,
                                                                                int64_t ldx, int64_t strideX, const T *__restrict__ beta,
                                                                                const T *__restrict__ X, int n, int d, const T *__restrict__ ell,
                                                                                const T *__restrict__ oscale, double *__restrict__ partials,
                                                                                int nlat) {
  PLMC_LOO_TILE_PRODUCT;
#define PLMC_KINV_KEEP (sizeof(T) == 4)
#include "kinv_epilogue.inc"
#undef PLMC_KINV_KEEP
}

template <typename T, CovFamily F, int DC = 0>
__global__ __launch_bounds__(NTHREADS, (table_min_waves<T, F, DC>())) void k_loo_grad_add(
    int kind, int ncomp, const T *__restrict__ Xop, int64_t n_pad, int64_t krows, int64_t ldx, int64_t strideX, const T *__restrict__ beta,
    const T *__restrict__ X, int n, int d, const T *__restrict__ ell, const T *__restrict__ oscale, double *__restrict__ partials, int nlat,
    const T *__restrict__ means, const T *__restrict__ third) {
  PLMC_LOO_TILE_PRODUCT;
#include "kinv_epilogue_table.inc"
}

// Xop[k][i] = rowscale[k] P_ki for k, i < n from the upper triangle of P = Khat^-1 that the K^-1 + gradient kernels store (their `Kinv`
// output), mirrored across the diagonal; exact zeros in the rest of [0, krows) x [0, n_pad).  One 64 x 64 tile of Xop per workgroup: the
// source tile (min, max) of the pair goes through LDS with 16-byte loads and is read back straight or transposed.  grid (n_pad / 64,
// ceil(krows / 64), q).  HBM-bound: one read and one write per element.
constexpr int OPT = 64;
template <typename T>
__global__ __launch_bounds__(NTHREADS) void k_loo_operand(const T *__restrict__ Kinv, int64_t ldk, int64_t strideK, const T *__restrict__ rowscale,
                                                          int64_t n_pad, T *__restrict__ Xop, int64_t krows, int64_t ldx, int64_t strideX, int n) {
  using vec_t = typename Traits<T>::vec_t;
  constexpr int EPV = Traits<T>::EPV;
  constexpr int CPR = OPT / EPV;                       // 16-byte chunks per tile row
  constexpr int NCH = OPT * CPR / NTHREADS;            // chunks per thread
  __shared__ T s[OPT][OPT + 1];
  const int cb = blockIdx.x, kb = blockIdx.y, lat = blockIdx.z;
  const int k0 = kb * OPT, i0 = cb * OPT;
  const int tid = threadIdx.x;
  const bool any = k0 < n && i0 < n;                   // (then both tiles lie inside n_pad x n_pad)
  if (any) {
    const int rb = kb < cb ? kb : cb, sb = kb < cb ? cb : kb;
    const T *src = Kinv + (int64_t)lat * strideK + (int64_t)rb * OPT * ldk + (int64_t)sb * OPT;
#pragma unroll
    for (int h = 0; h < NCH; ++h) {
      const int c = tid + h * NTHREADS, r = c / CPR, c0 = (c % CPR) * EPV;
      const vec_t v = *reinterpret_cast<const vec_t *>(src + (int64_t)r * ldk + c0);
#pragma unroll
      for (int e = 0; e < EPV; ++e) s[r][c0 + e] = v[e];
    }
    __syncthreads();
  }
  T *dst = Xop + (int64_t)lat * strideX + (int64_t)k0 * ldx + i0;
#pragma unroll
  for (int h = 0; h < NCH; ++h) {
    const int c = tid + h * NTHREADS, r = c / CPR, c0 = (c % CPR) * EPV;
    const int k = k0 + r;
    if (k >= krows) continue;
    vec_t o;
#pragma unroll
    for (int e = 0; e < EPV; ++e) o[e] = T(0);
    if (any && k < n) {
      const T rs = rowscale[(int64_t)lat * n_pad + k];
#pragma unroll
      for (int e = 0; e < EPV; ++e) {
        const int li = c0 + e;
        const bool straight = kb < cb || (kb == cb && li >= r);
        const T p = straight ? s[r][li] : s[li][r];
        o[e] = i0 + li < n ? rs * p : T(0);
      }
    }
    *reinterpret_cast<vec_t *>(dst + (int64_t)r * ldx + c0) = o;
  }
}

// The sibling of kinv_grad_impl<T, void> for the leave-one-out gradient: the same table, the same partial sums, the same reductions.
template <typename T>
int loo_grad_impl(const CovTable &table, const T *Xop, int64_t n_pad, int64_t krows, int64_t ldx, int64_t strideX, const T *beta, const T *X, int n,
                  double *grad, void *partials, int q, void *stream, bool check_only = false) {
  if (table.single_member())          // a sum of one member IS that member: its family's own path
    return sum_single_member<T>(table, n_pad, q, grad, partials, stream, [&](const CovTable &mt, double *fg, bool check) {
      return loo_grad_impl<T>(mt, Xop, n_pad, krows, ldx, strideX, beta, X, n, fg, partials, q, stream, check);
    });
  PLMC_REQUIRE_TABLE(table);
  const CovFamily family = table.route();
  const int kind = table.kernel_kind(), d = table.d, ncomp = table.ncomp;
  const T *ell = (const T *)table.ell, *oscale = (const T *)table.oscale, *second = (const T *)table.second, *third = (const T *)table.third;
  PLMC_REQUIRE(table.kind >= 0 && table.kind <= 4, "unknown kernel kind");
  PLMC_REQUIRE(Xop && beta && X && ell && grad && partials, "null pointer");
  PLMC_REQUIRE(n_pad > 0 && n_pad % NB == 0 && n > 0 && n <= n_pad && n > n_pad - NB, "n_pad must be plmc_pad(n)");
  PLMC_REQUIRE(krows > 0 && krows % BK == 0 && krows < ((int64_t)1 << 31), "krows must be a positive multiple of 16");
  PLMC_REQUIRE(ldx >= n_pad && ldx % NB == 0, "ldx must be a multiple of the block size, at least n_pad");
  PLMC_REQUIRE(q == 1 || strideX >= krows * ldx, "strideX too small");
  PLMC_REQUIRE(d > 0 && d <= MAX_DIM && q > 0, "need 0<d<=plmc_max_dim(), q>0");
  PLMC_REQUIRE(aligned16(Xop) && strideX % (16 / (int64_t)sizeof(T)) == 0, "unaligned Xop");
  if (check_only) return 0;
  hipStream_t st = (hipStream_t)stream;
  const int m = (int)(n_pad / NB);
  double *part = reinterpret_cast<double *>(partials);
  const double np = (double)n_pad;
  const dim3 grid(xcd_tri_grid(m, q)), block(NTHREADS);
#define PLMC_LAUNCH_LG(DC, SP) \
  hipLaunchKernelGGL((k_loo_grad<T, DC, SP>), grid, block, 0, st, kind, Xop, n_pad, krows, ldx, strideX, beta, X, n, d, ell, oscale, part, q)
#define PLMC_LAUNCH_LT(F, DC) \
  hipLaunchKernelGGL((k_loo_grad_add<T, F, DC>), grid, block, 0, st, kind, ncomp, Xop, n_pad, krows, ldx, strideX, beta, X, n, d, ell, oscale, part, q, \
                     second, third)
  {
    ProfScope ps(PK_KINV_GRAD, st, q * np * np * (double)krows, q * np * (double)krows * sizeof(T));
    switch (family) {
      default: with_capacity<0>(family, d, [&](auto f, auto dc) { PLMC_LAUNCH_LT(decltype(f)::value, decltype(dc)::value); }); break;
      case COV_ADD: PLMC_LAUNCH_LT(COV_ADD, 0); break;
      case COV_PLAIN:
        if (d <= 4) PLMC_LAUNCH_LG(4, false);
        else if (d <= 8) PLMC_LAUNCH_LG(8, false);
        else if (d <= 16) { if (kind == K_SPLINE) PLMC_LAUNCH_LG(16, true); else PLMC_LAUNCH_LG(16, false); }
        else { if (kind == K_SPLINE) PLMC_LAUNCH_LG(32, true); else PLMC_LAUNCH_LG(32, false); }
    }
  }
#undef PLMC_LAUNCH_LT
#undef PLMC_LAUNCH_LG
  launch_reduce_grad<T>(table, part, m, q, grad, st);
  return launch_status(__func__);
}

template <typename T>
int loo_operand_impl(const T *Kinv, int64_t n_pad, int64_t ldk, int64_t strideK, const T *rowscale, T *Xop, int64_t krows, int64_t ldx,
                     int64_t strideX, int n, int q, void *stream) {
  constexpr int64_t EPV = 16 / (int64_t)sizeof(T);
  PLMC_REQUIRE(Kinv && rowscale && Xop, "null pointer");
  PLMC_REQUIRE(n_pad > 0 && n_pad % NB == 0 && n > 0 && n <= n_pad && n > n_pad - NB, "n_pad must be plmc_pad(n)");
  PLMC_REQUIRE(q > 0 && q <= 65535, "need 0 < q <= 65535");
  PLMC_REQUIRE(krows >= n && krows % BK == 0 && krows <= 65535 * (int64_t)OPT, "krows must be a multiple of 16, at least n");
  PLMC_REQUIRE(ldk >= n_pad && ldk % EPV == 0 && strideK % EPV == 0 && aligned16(Kinv), "Kinv: ldk >= n_pad, 16-byte aligned rows");
  PLMC_REQUIRE(ldx >= n_pad && ldx % NB == 0 && strideX % EPV == 0 && aligned16(Xop), "Xop: ldx a multiple of the block size, at least n_pad");
  PLMC_REQUIRE(q == 1 || (strideK >= n_pad * ldk && strideX >= krows * ldx), "batch stride too small");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(n_pad / OPT), (unsigned)((krows + OPT - 1) / OPT), q);
  hipLaunchKernelGGL(k_loo_operand<T>, grid, dim3(NTHREADS), 0, st, Kinv, ldk, strideK, rowscale, n_pad, Xop, krows, ldx, strideX, n);
  return launch_status(__func__);
}

// ---- weighted kernel-gradient sum: the gradient epilogues above behind the product of two GENERAL operands.
//     grad[l][t] = sum_{i <= j < N} c_ij (At_l^T Bt_l)_ij dKhat_l(Z)_ij / dtheta_t,   c_ii = 1, c_ij = 2
// (include/plmc.h, "Weighted kernel-gradient sum"; DESIGN.md 7.14: the gradient of a loss of the posterior moments with respect to the
// hyper-parameters is this sum over the stacked points Z = [X; X*]).  At, Bt: r_pad x N_pad per latent, K-major like W, every row
// contracted -- the tile (ib, jb) is the product of column strip ib of At and column strip jb of Bt over ALL r_pad rows, as for the
// leave-one-out gradient, but of two different operands, so that only the upper tiles of a symmetric At^T Bt are formed.  The epilogue
// text reduces (alpha_i alpha_j - acc_ij) dKhat_ij / dtheta and its reduction halves the sum: `alpha` is a vector of zeros that is never
// read from memory (ZeroVector), so the family's reduction leaves -1/2 of the wanted sum, and k_scale_table multiplies the finished
// table by -2, a power of two: sign and 1/2 of the marginal-likelihood form cancel without a rounding.  (Scaling the tile in front of
// the epilogue instead kept a second copy of the accumulators in registers: 64 / 128 more per lane, scratch in one instantiation.)
// Nothing is stored.
// One upper tile per workgroup in the order of k_kinv_grad (latent fastest); fp32 on v_mfma_f32_16x16x4_f32 (no split engine: the
// operands have no eigenvalue bound to scale by).
template <typename T> struct ZeroVector {
  __device__ __forceinline__ T operator[](int64_t) const { return T(0); }
};
#define PLMC_WEIGHTED_TILE_PRODUCT                                                                                                             \
  const int m = (int)(n_pad / NB);                                                                                                             \
  const int lat = (int)blockIdx.x % nlat;                                                                                                      \
  int ib, jb;                                                                                                                                  \
  tri_decode((int)blockIdx.x / nlat, ib, jb);                                                                                                  \
  __shared__ __align__(16) T smem[tile_smem_elems<T>()];                                                                                       \
  Acc<T> acc;                                                                                                                                  \
  acc.zero();                                                                                                                                  \
  tile_mainloop<T, false, true>(acc, At + (int64_t)lat * strideAB + (int64_t)ib * NB, ldab, Bt + (int64_t)lat * strideAB + (int64_t)jb * NB,   \
                                ldab, (int)r_pad, smem);                                                                                       \
  const ZeroVector<T> alpha;                                                                                                                   \
  T *const Kinv = nullptr, *const kinv_diag = nullptr;                                                                                         \
  constexpr int64_t ldk = 0, strideK = 0;                                                                                                      \
  const int tid = threadIdx.x;                                                                                                                 \
  constexpr bool live = true

// occupancy floor: that of the matching k_kinv_grad / k_kinv_grad_add instantiation, except where the same epilogue text behind this tile
// product needs a few registers more than the floor leaves (as k_loo_grad found, LOO_MIN_WAVES): no instantiation uses scratch
// (profiles/weighted_grad_resource_usage.md)
template <typename T, int DCAP> constexpr int WG_MIN_WAVES = LOO_MIN_WAVES<T, DCAP>;

template <typename T, int DCAP, bool SPLINE = false>
__global__ __launch_bounds__(NTHREADS, (WG_MIN_WAVES<T, DCAP>)) void k_weighted_grad(int kind, const T *__restrict__ At, const T *__restrict__ Bt,
                                                                                    int64_t r_pad, int64_t n_pad, int64_t ldab, int64_t strideAB,
                                                                                    const T *__restrict__ X, int n, int d,
                                                                                    const T *__restrict__ ell, const T *__restrict__ oscale,
                                                                                    double *__restrict__ partials, int nlat) {
  PLMC_WEIGHTED_TILE_PRODUCT;
#define PLMC_KINV_KEEP (sizeof(T) == 4)
#include "kinv_epilogue.inc"
#undef PLMC_KINV_KEEP
}

template <typename T, CovFamily F, int DC = 0>
__global__ __launch_bounds__(NTHREADS, (table_min_waves<T, F, DC>())) void k_weighted_grad_add(
    int kind, int ncomp, const T *__restrict__ At, const T *__restrict__ Bt, int64_t r_pad, int64_t n_pad, int64_t ldab, int64_t strideAB,
    const T *__restrict__ X, int n, int d, const T *__restrict__ ell, const T *__restrict__ oscale, double *__restrict__ partials, int nlat,
    const T *__restrict__ means, const T *__restrict__ third) {
  PLMC_WEIGHTED_TILE_PRODUCT;
#include "kinv_epilogue_table.inc"
}

// table[0 .. count) *= factor, one workgroup (the finished gradient table of a call: q rows of at most a few hundred doubles)
__global__ void k_scale_table(double *__restrict__ table, int count, double factor) {
  for (int e = threadIdx.x; e < count; e += blockDim.x) table[e] *= factor;
}
// entries per latent of the family's gradient table, as its reduction kernel writes it (k_reduce_grad*)
inline int grad_table_width(const CovTable &t) {
  const int d = t.d, g = t.ncomp;
  switch (t.route()) {
    case COV_PER: return 2 * d + 2;
    case COV_LPER: return 3 * d + 2;
    case COV_SUM: return g * (3 * d + 2) + 1;
    case COV_RQ: case COV_DOT: return d + 3;
    case COV_SM: return g * (2 * d + 1) + 1;
    case COV_ADD: return g * (d + 1) + 1;
    case COV_PLAIN: break;
  }
  return d + 2;
}

// The sibling of loo_grad_impl for the weighted sum: the same table, the same partial sums (sized by the same calls, at N_pad), the same
// reductions.  Z: the N points the table's kernel is evaluated on (rows < N are read); operand rows [r, r_pad) and columns [N, N_pad)
// must be zero (the caller's duty); columns [N_pad, ld) are not read.
template <typename T>
int weighted_grad_impl(const CovTable &table, const T *At, const T *Bt, int64_t r_pad, int64_t n_pad, int64_t ld, int64_t stride, const T *Z, int n,
                       double *grad, void *partials, int q, void *stream, bool check_only = false) {
  if (table.single_member())          // a sum of one member IS that member: its family's own path
    return sum_single_member<T>(table, n_pad, q, grad, partials, stream, [&](const CovTable &mt, double *fg, bool check) {
      return weighted_grad_impl<T>(mt, At, Bt, r_pad, n_pad, ld, stride, Z, n, fg, partials, q, stream, check);
    });
  constexpr int64_t EPV = 16 / (int64_t)sizeof(T);
  PLMC_REQUIRE_TABLE(table);
  const CovFamily family = table.route();
  const int kind = table.kernel_kind(), d = table.d, ncomp = table.ncomp;
  const T *ell = (const T *)table.ell, *oscale = (const T *)table.oscale, *second = (const T *)table.second, *third = (const T *)table.third;
  PLMC_REQUIRE(table.kind >= 0 && table.kind <= 4, "unknown kernel kind");
  PLMC_REQUIRE(At && Bt && Z && ell && grad && partials, "null pointer");
  PLMC_REQUIRE(n > 0, "need N > 0");
  PLMC_REQUIRE(n_pad > 0 && n_pad % NB == 0 && n <= n_pad && n_pad < ((int64_t)1 << 31), "N_pad must be a multiple of the block size, at least N");
  PLMC_REQUIRE(r_pad > 0 && r_pad % BK == 0 && r_pad < ((int64_t)1 << 31), "r_pad must be a positive multiple of 16");
  PLMC_REQUIRE(ld >= n_pad && ld % EPV == 0, "ld must be at least N_pad, its rows 16-byte aligned");
  PLMC_REQUIRE(q == 1 || stride >= r_pad * ld, "stride too small");
  PLMC_REQUIRE(d > 0 && d <= MAX_DIM && q > 0, "need 0<d<=plmc_max_dim(), q>0");
  PLMC_REQUIRE(aligned16(At) && aligned16(Bt) && stride % EPV == 0, "unaligned operands");
  const int m = (int)(n_pad / NB);
  PLMC_REQUIRE((int64_t)q * ((int64_t)m * (m + 1) / 2) < ((int64_t)1 << 31), "too many tiles for one launch");
  if (check_only) return 0;
  hipStream_t st = (hipStream_t)stream;
  double *part = reinterpret_cast<double *>(partials);
  const double np = (double)n_pad;
  const dim3 grid(q * (m * (m + 1) / 2)), block(NTHREADS);
#define PLMC_LAUNCH_WG(DC, SP) \
  hipLaunchKernelGGL((k_weighted_grad<T, DC, SP>), grid, block, 0, st, kind, At, Bt, r_pad, n_pad, ld, stride, Z, n, d, ell, oscale, part, q)
#define PLMC_LAUNCH_WT(F, DC) \
  hipLaunchKernelGGL((k_weighted_grad_add<T, F, DC>), grid, block, 0, st, kind, ncomp, At, Bt, r_pad, n_pad, ld, stride, Z, n, d, ell, oscale, part, q, \
                     second, third)
  {
    ProfScope ps(PK_KINV_GRAD, st, q * np * np * (double)r_pad, q * np * (double)r_pad * 2 * sizeof(T));
    switch (family) {
      default: with_capacity<0>(family, d, [&](auto f, auto dc) { PLMC_LAUNCH_WT(decltype(f)::value, decltype(dc)::value); }); break;
      case COV_ADD: PLMC_LAUNCH_WT(COV_ADD, 0); break;
      case COV_PLAIN:
        if (d <= 4) PLMC_LAUNCH_WG(4, false);
        else if (d <= 8) PLMC_LAUNCH_WG(8, false);
        else if (d <= 16) { if (kind == K_SPLINE) PLMC_LAUNCH_WG(16, true); else PLMC_LAUNCH_WG(16, false); }
        else { if (kind == K_SPLINE) PLMC_LAUNCH_WG(32, true); else PLMC_LAUNCH_WG(32, false); }
    }
  }
#undef PLMC_LAUNCH_WT
#undef PLMC_LAUNCH_WG
  launch_reduce_grad<T>(table, part, m, q, grad, st);
  hipLaunchKernelGGL(k_scale_table, dim3(1), dim3(256), 0, st, grad, q * grad_table_width(table), -2.0);
  return launch_status(__func__);
}

// ---- a heterogeneous sum of ONE member is that member's family: its own kernels run on the whole batch, bit for bit.  They read (q, d)
// rows, the sum's records are 3 d + 1 apart, so the owned slots are re-laid behind the partial sums (SUM_TAIL_BYTES per latent, counted
// by plmc_sum_grad_partials_bytes): rows [ell | period | rbf_ell: q x d each | alpha: q], then the family's gradient table, which
// k_sum_member_grad copies into the sum's layout.  A slot the member does not own is neither read nor left unwritten (exactly 0).
constexpr int64_t SUM_TAIL_BYTES = 512;
static_assert((3 * SUM_MAX_DIM + 1) * 8 <= 256 && (3 * SUM_MAX_DIM + 2) * 8 <= 256, "one-member scratch of a sum");
template <typename T>
__global__ void k_sum_member_rows(int f, int d, int q, const T *__restrict__ table, T *__restrict__ rows) {
  const int rec = 3 * d + 1;
  for (int e = threadIdx.x; e < q * rec; e += blockDim.x) {
    const int lat = e / rec, j = e - lat * rec, row = j / d, kk = j - row * d;
    const bool owned = row == 0 || (row == 1 && (f == F_PER || f == F_LPER)) || (row == 2 && f == F_LPER) || (row == 3 && f == F_RQ);
    T *dst = row < 3 ? rows + ((int64_t)row * q + lat) * d + kk : rows + (int64_t)3 * q * d + lat;
    *dst = owned ? table[e] : T(0);
  }
}
// family layouts: [ell: d | noise | os], periodic [ell | period | noise | os], rational quadratic [ell | alpha | noise | os], locally periodic
// [ell | period | rbf_ell | noise | os]  ->  [ell | period | rbf_ell | alpha | noise | os]
__global__ void k_sum_member_grad(int f, int d, int q, const double *__restrict__ fg, double *__restrict__ grad) {
  const int wf = f == F_PER ? 2 * d + 2 : f == F_RQ ? d + 3 : f == F_LPER ? 3 * d + 2 : d + 2, ws = 3 * d + 3;
  for (int e = threadIdx.x; e < q * ws; e += blockDim.x) {
    const int lat = e / ws, j = e - lat * ws;
    int src = -1;
    if (j < d) src = j;
    else if (j < 2 * d) src = (f == F_PER || f == F_LPER) ? j : -1;
    else if (j < 3 * d) src = f == F_LPER ? j : -1;
    else if (j == 3 * d) src = f == F_RQ ? d : -1;
    else src = wf - 2 + (j - (3 * d + 1));
    grad[e] = src >= 0 ? fg[(int64_t)lat * wf + src] : 0.0;
  }
}
// `call(member table, its gradient table, check_only)` runs the member family's gradient path, or its argument checks alone: they run
// first, so a refused call has launched nothing
template <typename T, class Call>
int sum_single_member(const CovTable &t, int64_t n_pad, int q, double *grad, void *partials, void *stream, Call call) {
  PLMC_REQUIRE_TABLE(t);
  PLMC_REQUIRE(grad && partials && q > 0 && n_pad > 0, "null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int f = t.fam_of(0), d = t.d;
  char *tail = reinterpret_cast<char *>(partials) + (n_pad / NB) * (n_pad / NB) * (int64_t)q * GP * (int64_t)sizeof(double);
  T *rows = reinterpret_cast<T *>(tail);
  double *fg = reinterpret_cast<double *>(tail + (SUM_TAIL_BYTES / 2) * q);
  const CovTable mt = t.member(rows, rows + (int64_t)q * d, rows + (int64_t)2 * q * d, rows + (int64_t)3 * q * d, t.oscale);
  if (int rc = call(mt, fg, true)) return rc;
  hipLaunchKernelGGL(k_sum_member_rows<T>, dim3(1), dim3(256), 0, st, f, d, q, (const T *)t.ell, rows);
  if (int rc = call(mt, fg, false)) return rc;
  hipLaunchKernelGGL(k_sum_member_grad, dim3(1), dim3(256), 0, st, f, d, q, (const double *)fg, grad);
  return launch_status(__func__);
}

}  // namespace plmc

// The K^-1 + gradient call of either element type.  fp32 goes by the arithmetic of its products (PLMC_SPLIT) and by what fits beside the
// split engine (api_common.hpp, FamilyTraits::split_max_d); fp64 has one path and looks at neither eig_lo nor Vd.  Vd: the scratch of
// the sweep that produced W, or null.
template <typename T>
static int kinv_grad_any(const plmc::CovTable &table, const T *W, int64_t n_pad, int64_t ldw, int64_t strideW, const T *alpha, const T *X, int n,
                         double *grad, T *Kinv, int64_t ldk, int64_t strideK, T *kinv_diag, void *partials, int q, const T *eig_lo, void *stream,
                         const T *Vd = nullptr, bool check_only = false) {
  if (!table.single_member()) {
    if constexpr (sizeof(T) == 8) {
      return plmc::kinv_grad_impl<double, void>(table, W, n_pad, ldw, strideW, alpha, X, n, grad, Kinv, ldk, strideK, kinv_diag, partials, q, nullptr,
                                                stream, nullptr, 0, check_only);
    } else {
      const int split = plmc::knobs().split;
      const bool three_planes = !(split == 2 && eig_lo);
      if (split == 0 || table.d > plmc::FAMILY[table.family].split_max_d[three_planes])
        return plmc::kinv_grad_impl<float, void>(table, W, n_pad, ldw, strideW, alpha, X, n, grad, Kinv, ldk, strideK, kinv_diag, partials, q, nullptr,
                                                 stream, nullptr, 0, check_only);
      // Vd: the scratch of the sweep that produced W, whose leading dimension is ldw (W lives in the factor buffer's columns)
      if (!three_planes)
        return plmc::kinv_grad_impl<float, plmc::SplitH2>(table, W, n_pad, ldw, strideW, alpha, X, n, grad, Kinv, ldk, strideK, kinv_diag, partials, q,
                                                          eig_lo, stream, Vd, ldw, check_only);
      return plmc::kinv_grad_impl<float, plmc::SplitB3>(table, W, n_pad, ldw, strideW, alpha, X, n, grad, Kinv, ldk, strideK, kinv_diag, partials, q,
                                                        nullptr, stream, Vd, ldw, check_only);
    }
  }
  // a sum of one member IS that member: its family's own path.  (Behind the others in the text, so that the gradient kernels come first
  // in the code object, as they always did: profiles/family_dispatch_kernel_identity.md.)
  return plmc::sum_single_member<T>(table, n_pad, q, grad, partials, stream, [&](const plmc::CovTable &mt, double *fg, bool check) {
    return kinv_grad_any<T>(mt, W, n_pad, ldw, strideW, alpha, X, n, fg, Kinv, ldk, strideK, kinv_diag, partials, q, eig_lo, stream, Vd, check);
  });
}

extern "C" {
// per-tile partial sums + (4-byte elements) the planes of W for the split engine (the entry points without Vd); independent of the knobs
int64_t plmc_grad_scratch_bytes_for(int64_t n_pad, int q, int elem_bytes) {
  int64_t m = n_pad / plmc::NB;
  const int64_t planes = elem_bytes == 4 ? (int64_t)q * plmc::b3_elems<plmc::SplitB3>(n_pad, n_pad) * 2 + 4096 : 0;   // + the q scales
  return m * m * (int64_t)q * plmc::GP * (int64_t)sizeof(double) + planes;
}
int64_t plmc_grad_scratch_bytes(int64_t n_pad, int q) { return plmc_grad_scratch_bytes_for(n_pad, q, 4); }
// what plmc_kinv_grad_vd_* needs when the sweep's scratch supplies the planes of W: the per-tile partial sums only
int64_t plmc_grad_partials_bytes(int64_t n_pad, int q) {
  const int64_t m = n_pad / plmc::NB;
  return m * m * (int64_t)q * plmc::GP * (int64_t)sizeof(double);
}
// The entry points of the families (api_common.hpp, PLMC_FAMILY_ENTRIES): the only place the covariance tables of this file are built from
// flat arguments.  plmc_kinv_grad*_vd_*: `partials` is sized by plmc_grad_partials_bytes, for a spectral mixture, a locally periodic
// kernel and a sum by their own plmc_*_grad_partials_bytes.  plmc_loo_grad*: the leave-one-out pseudo-likelihood (include/plmc.h,
// "Leave-one-out objective"), the family's gradient table of 1/2 (beta beta^T - Xop^T Xop).  plmc_weighted_grad*: the family's gradient
// table weighted by the upper triangle of At^T Bt (include/plmc.h, "Weighted kernel-gradient sum").
#define PLMC_GRAD_ENTRY(SUF, T, INFIX, LEAD, PARAMS, TABLE)                                                                                     \
  int plmc_kinv_grad##INFIX##_vd_##SUF(PLMC_LEAD_##LEAD const T *W, int64_t n_pad, int64_t ldw, int64_t strideW, const T *alpha, const T *X,    \
                                       int n, int d, PLMC_UNPACK PARAMS, double *grad, T *Kinv, int64_t ldk, int64_t strideK, T *kinv_diag,     \
                                       void *partials, int q, const T *eig_lo, const T *Vd, void *stream) {                                     \
    return kinv_grad_any<T>(TABLE, W, n_pad, ldw, strideW, alpha, X, n, grad, Kinv, ldk, strideK, kinv_diag, partials, q, eig_lo, stream, Vd);  \
  }                                                                                                                                             \
  int plmc_loo_grad##INFIX##_##SUF(PLMC_LEAD_##LEAD const T *Xop, int64_t n_pad, int64_t krows, int64_t ldx, int64_t strideX, const T *beta,    \
                                   const T *X, int n, int d, PLMC_UNPACK PARAMS, double *grad, void *partials, int q, void *stream) {           \
    return plmc::loo_grad_impl<T>(TABLE, Xop, n_pad, krows, ldx, strideX, beta, X, n, grad, partials, q, stream);                               \
  }                                                                                                                                             \
  int plmc_weighted_grad##INFIX##_##SUF(PLMC_LEAD_##LEAD const T *At, const T *Bt, int64_t r_pad, int64_t N_pad, int64_t ld, int64_t stride,    \
                                        const T *Z, int N, int d, PLMC_UNPACK PARAMS, double *grad, void *partials, int q, void *stream) {      \
    return plmc::weighted_grad_impl<T>(TABLE, At, Bt, r_pad, N_pad, ld, stride, Z, N, grad, partials, q, stream);                               \
  }
PLMC_FAMILY_ENTRIES(PLMC_GRAD_ENTRY, f32, float)
PLMC_FAMILY_ENTRIES(PLMC_GRAD_ENTRY, f64, double)
#undef PLMC_GRAD_ENTRY
// the plain kernel without the sweep's scratch, with and without eigenvalue bounds
#define PLMC_KINV_GRAD_PLAIN(SUF, T)                                                                                                            \
  int plmc_kinv_grad_##SUF(int kind, const T *W, int64_t n_pad, int64_t ldw, int64_t strideW, const T *alpha, const T *X, int n, int d,         \
                           const T *ell, const T *oscale, double *grad, T *Kinv, int64_t ldk, int64_t strideK, T *kinv_diag, void *partials,    \
                           int q, void *stream) {                                                                                               \
    return kinv_grad_any<T>(plmc::CovTable::plain(kind, d, ell, oscale), W, n_pad, ldw, strideW, alpha, X, n, grad, Kinv, ldk, strideK,         \
                            kinv_diag, partials, q, nullptr, stream);                                                                           \
  }                                                                                                                                             \
  int plmc_kinv_grad_ex_##SUF(int kind, const T *W, int64_t n_pad, int64_t ldw, int64_t strideW, const T *alpha, const T *X, int n, int d,      \
                              const T *ell, const T *oscale, double *grad, T *Kinv, int64_t ldk, int64_t strideK, T *kinv_diag, void *partials, \
                              int q, const T *eig_lo, void *stream) {                                                                           \
    return kinv_grad_any<T>(plmc::CovTable::plain(kind, d, ell, oscale), W, n_pad, ldw, strideW, alpha, X, n, grad, Kinv, ldk, strideK,         \
                            kinv_diag, partials, q, eig_lo, stream);                                                                            \
  }
PLMC_KINV_GRAD_PLAIN(f32, float)
PLMC_KINV_GRAD_PLAIN(f64, double)
#undef PLMC_KINV_GRAD_PLAIN
// one row of fp64 partial sums per tile (and component), whatever the element type
int64_t plmc_sm_grad_partials_bytes(int64_t n_pad, int q, int nmix, int elem_bytes) {
  (void)elem_bytes;
  return plmc_grad_partials_bytes(n_pad, q * nmix);
}
int64_t plmc_per_grad_partials_bytes(int64_t n_pad, int q, int elem_bytes) {
  (void)elem_bytes;
  return plmc_grad_partials_bytes(n_pad, q);
}
int64_t plmc_lper_grad_partials_bytes(int64_t n_pad, int q, int elem_bytes) {
  (void)elem_bytes;
  return plmc_grad_partials_bytes(n_pad, q);
}
// ... and the scratch of a one-member sum behind them (sum_single_member)
int64_t plmc_sum_grad_partials_bytes(int64_t n_pad, int q, int ncomp, int elem_bytes) {
  (void)elem_bytes;
  return plmc_grad_partials_bytes(n_pad, q * ncomp) + plmc::SUM_TAIL_BYTES * q;
}
#define PLMC_LOO_OPERAND(SUF, T)                                                                                                                \
  int plmc_loo_operand_##SUF(const T *Kinv, int64_t n_pad, int64_t ldk, int64_t strideK, const T *rowscale, T *Xop, int64_t krows, int64_t ldx, \
                             int64_t strideX, int n, int q, void *stream) {                                                                    \
    return plmc::loo_operand_impl<T>(Kinv, n_pad, ldk, strideK, rowscale, Xop, krows, ldx, strideX, n, q, stream);                              \
  }
PLMC_LOO_OPERAND(f32, float)
PLMC_LOO_OPERAND(f64, double)
#undef PLMC_LOO_OPERAND
}
