// cross_matvec_order.hpp -- what the products with a never-written cross-covariance share (cross_matvec.hip: the values; cross_matvec_dx.hip:
// their derivatives with respect to the test inputs): the thread map, the ONE fixed summation order -- segments, ranges, splits, functions
// of the sizes alone -- the checks on the sizes, and the phase of a random Fourier feature reduced in revolutions.
#pragma once
#include "api_common.hpp"

namespace plmc {

constexpr int CM_TS = 64;                            // test points per workgroup: one per lane
constexpr int CM_JP = NTHREADS / CM_TS;              // waves, each with its share of a chunk
constexpr int CM_JC = 64;                            // rows per staged chunk
constexpr int CM_JW = CM_JC / CM_JP;                 // of which one wave takes these
constexpr int CM_MIN_ROWS = 256;                     // shortest range of rows worth a workgroup of its own
constexpr int CM_MAX_COLS = 8;                       // most columns of V in one call: 8 fp64 sums per lane beside the widest table's pair
#ifndef PLMC_CM_TARGET_WGS
#define PLMC_CM_TARGET_WGS 2048                      // workgroups wanted: eight per compute unit, i.e. eight waves per SIMD -- the pair values are
                                                     // chains of dependent transcendentals, hidden by other waves only (dev builds: 1 = never split)
#endif
static_assert(CM_TS == 64 && NTHREADS % CM_TS == 0 && CM_JC % CM_JP == 0 && CM_MIN_ROWS % CM_JC == 0, "cross-matvec thread map");

// Rows of one segment of the fixed summation order, a function of n alone: CM_MIN_ROWS, or what keeps n within CM_MAX_SEGS segments.
constexpr int CM_MAX_SEGS = 64;
static int cross_matvec_segment(int n) {
  const int per = ((n + CM_MAX_SEGS - 1) / CM_MAX_SEGS + CM_JC - 1) / CM_JC * CM_JC;
  return per > CM_MIN_ROWS ? per : CM_MIN_ROWS;
}
static int cross_matvec_segments(int n) { return (n + cross_matvec_segment(n) - 1) / cross_matvec_segment(n); }
// Ranges the rows are split into, and the rows of one (whole segments): as many as bring the launch to PLMC_CM_TARGET_WGS workgroups.
static int cross_matvec_rows(int n, int ns, int q) {
  const int64_t wgs = (int64_t)((ns + CM_TS - 1) / CM_TS) * q;
  int64_t want = (PLMC_CM_TARGET_WGS + wgs - 1) / wgs;
  const int64_t nseg = cross_matvec_segments(n);
  want = want < 1 ? 1 : (want > nseg ? nseg : want);
  return (int)((nseg + want - 1) / want) * cross_matvec_segment(n);
}
static int cross_matvec_splits(int n, int ns, int q) {
  const int rows = cross_matvec_rows(n, ns, q);
  return (n + rows - 1) / rows;
}

// The phase of one random Fourier feature against the lane's point, sum_k f_k x_k + b in revolutions, brought into [-1/2, 1/2].  It is
// hundreds to thousands of revolutions for short lengthscales on wide inputs, so it is reduced term by term as sm_phase reduces the
// mixture's: t = f x with its FMA residual, t - rint(t) exact, the running sum brought back into [-1/2, 1/2] after every term (each
// add of two numbers <= 1/2 rounds by <= 2^-25 in fp32), the residuals added at the end, one more reduction.
template <typename T> __device__ __forceinline__ T rff_fold(T s) { return s - __builtin_rint(s); }
template <typename T, int DCAP> __device__ __forceinline__ T rff_phase(const T *fa, T b, const T (&xs)[DCAP]) {
  T s = rff_fold(b), res = T(0);
#pragma unroll
  for (int k = 0; k < DCAP; ++k) {
    const T t = fa[k] * xs[k];
    res += __builtin_fma(fa[k], xs[k], -t);          // f x = t + (this) exactly
    s = rff_fold(s + rff_fold(t));
  }
  return rff_fold(s + res);
}

// what every operation asks of the sizes, V and the scratch (`n`: rows or features)
#define PLMC_CM_REQUIRE_SHAPE(n, ns, r, q, ldv, strideV, partials)                                                                       \
  PLMC_REQUIRE(n > 0 && ns > 0 && r > 0 && q > 0 && q <= 65535, "need n > 0, ns > 0, r > 0, 0 < q <= 65535");                            \
  PLMC_REQUIRE(r <= CM_MAX_COLS, "need r <= plmc_cross_matvec_max_cols()");                                                              \
  PLMC_REQUIRE(ldv >= r, "V: ldv >= r");                                                                                                 \
  PLMC_REQUIRE(q == 1 || strideV >= (int64_t)(n - 1) * ldv + r, "V: strideV >= (n - 1) * ldv + r");                                      \
  PLMC_REQUIRE(cross_matvec_splits(n, ns, q) <= 65535, "too many ranges");                                                               \
  PLMC_REQUIRE(cross_matvec_splits(n, ns, q) == 1 || partials, "null pointer: partials (plmc_cross_matvec_partials_bytes)")

}  // namespace plmc
