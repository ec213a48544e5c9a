// cross_matvec_dx.hip -- derivative of the products of cross_matvec.hip with respect to the test inputs, contracted with weights on the fly
// (DESIGN.md 7.13): for q latents on the training inputs X (n x d, raw coordinates), test inputs Xs (ns x d), r <= CM_MAX_COLS columns V
// (n x r per latent, leading dimension ldv) and upstream weights G (ns x r per latent),
//   Jx[lat][s][k] = sum_{i < n} w_si  d k_lat(xs_s, x_i) / d xs_s[k],     w_si = sum_{c < r} G[lat][s][c] V[lat][i][c]      (plmc_cross_matvec_dx*)
// for the families of posterior_dx.hip (the unit derivative of a pair through dx_pair of input_dx.hpp with g = 1, evaluated once in the
// element type), and for m random Fourier features, frequencies and phases in revolutions,
//   Jx[lat][s][k] = -2 pi scale[lat] sum_{j < m} sin(2 pi (freq[lat][j] . xs_s + phase[lat][j])) freq[lat][j][k] w_sj     (plmc_rff_matvec_dx)
// with w_sj from Wt (m x r) in the place of V.  G == NULL (r = 1 only): w = the one column, the Jacobian of that column.
// One kernel serves both, on the skeleton of k_cross_matvec: one workgroup per (block of CM_TS test points, range of rows, latent); a lane
// owns one test point, its row of G (r fp64 registers) and d fp64 sums; the four waves take a quarter of every staged chunk of rows each,
// whose coordinates, columns of V and the latent's table are LDS broadcasts.  w and every sum are fp64 in the ONE fixed order of
// cross_matvec_order.hpp, a function of the row count alone: w over the columns in order; segments of cross_matvec_segment(n) rows, within
// a segment every wave adds its rows in order and the four waves meet in order through LDS (cmd_kp() dimensions per pass), the segments are
// added in order.  When the call splits (cross_matvec_splits()) the segments' sums go to the caller's `partials` for
// k_cross_matvec_dx_reduce to add in that same order: an output element has the same bits whether or not the call splits, whichever lane
// owns its test point and however many test points the call has.  No atomics, no scratch, every output element written once.
// Indices are clamped into range before the address is formed and the term is selected afterwards: nothing is read from rows >= n of X or
// V, from columns >= r of V or G or from test points >= ns, every load is unconditional, nothing outside Jx[.][< ns][< d] is written.
#include "api_common.hpp"
#include "covariance.hpp"
#include "cross_matvec_order.hpp"
#include "input_dx.hpp"
#include "../../include/plmc.h"

namespace plmc {

template <int DC> constexpr int cmd_kp() { return DC < 4 ? DC : 4; }   // dimensions per pass of the waves' meeting (LDS: 3 x 4 x 64 fp64)

// The unit derivative of a pair for a covariance family: what k_posterior_dx evaluates, the same tables (dx_stage_table), g = 1.
template <typename T, CovFamily F, int DC> struct DxFamily {
  static constexpr bool rff = false;
  static constexpr CovFamily family = F;
  static constexpr int LDS = IG_TAB;
  int kind, ncomp;
  const T *ell, *second, *third, *oscale;
  __device__ __forceinline__ void stage(int lat, int d, T *tab) const {
    dx_stage_table<T, F, DC>(tab, threadIdx.x, lat, d, ncomp, ell, second, third, oscale);
  }
  // acc[k] += w d k(xs, row) / d xs[k]
  __device__ __forceinline__ void add(const T (&xs)[DC], const T *row, T, const T *tab, T os, double w, double (&acc)[DC]) const {
    T u[DC];
#pragma unroll
    for (int k = 0; k < DC; ++k) u[k] = T(0);
    dx_pair<T, F, DC>(kind, ncomp, xs, row, tab, T(1), os, u);
#pragma unroll
    for (int k = 0; k < DC; ++k) acc[k] = __builtin_fma(w, (double)u[k], acc[k]);
  }
};

// One random Fourier feature: d cos(2 pi phi) / d xs[k] = -2 pi sin(2 pi phi) f_k.  The sine of the reduced phase (rff_phase, the value's own
// reduction) is of the element type, from sm_sincos; its product with the weight and with f_k -- exact in fp64 -- and the sums are fp64; the
// factor -2 pi scale multiplies the finished sum once.  One sine is within 4 (d + 2) u of the exact one whatever the phase.
template <typename T, int DC> struct DxRff {
  static constexpr bool rff = true;
  static constexpr int LDS = 1;
  const T *scale;
  __device__ __forceinline__ void stage(int lat, int, T *tab) const {
    if (threadIdx.x == 0) tab[0] = scale ? scale[lat] : T(1);
  }
  __device__ __forceinline__ void add(const T (&xs)[DC], const T *row, T b, const T *, T, double w, double (&acc)[DC]) const {
    T sn, cs;
    sm_sincos(rff_phase<T, DC>(row, b, xs), sn, cs);
    const double ws = w * (double)sn;
#pragma unroll
    for (int k = 0; k < DC; ++k) acc[k] = __builtin_fma(ws, (double)row[k], acc[k]);
  }
};
constexpr double CMD_M2PI = -6.283185307179586476925286766559;

// X: the rows, (n, d) raw, `strideX` elements from one latent's to the next (0: shared by the latents); phase: (q, n), features only.
// RC: capacity of the lane's row of G, 1 or CM_MAX_COLS.  `rows`: rows of this workgroup's range, `seg`: of a segment (rows a multiple of
// seg, seg of CM_JC).  part != null: the segments' sums go there, [segment][lat][s][k], unscaled; else their sum goes to Jx.
template <typename T, int DC, int RC, class P>
__global__ __launch_bounds__(NTHREADS) void k_cross_matvec_dx(const P prm, const T *__restrict__ X, int64_t strideX, const T *__restrict__ phase, int n,
                                                               const T *__restrict__ Xs, int ns, int d, const T *__restrict__ V, int64_t ldv,
                                                               int64_t strideV, int r, const T *__restrict__ G, int rows, int seg,
                                                               double *__restrict__ part, double *__restrict__ Jx) {
  constexpr bool RFF = P::rff;
  constexpr int KP = cmd_kp<DC>();
  __shared__ __align__(16) T sX[CM_JC * DC];         // the chunk's rows (0 beyond d)
  __shared__ T sV[CM_JC * RC];                       // their columns of V (0 beyond r and beyond the range)
  __shared__ T sPh[RFF ? CM_JC : 1];                 // features: their phases
  __shared__ T tab[P::LDS];                          // the latent's table
  __shared__ double sRed[(CM_JP - 1) * KP * CM_TS];  // the other waves' sums, KP dimensions at a time
  __shared__ double sTot[DC * CM_TS];                // wave 0: the segments so far, each lane its own column (registers are the scarce thing)
  const int tid = threadIdx.x, tb = blockIdx.x, sp = blockIdx.y, lat = blockIdx.z, q = gridDim.z;
  const int sl = tid & (CM_TS - 1), jp = tid / CM_TS;
  const int s = tb * CM_TS + sl, cs = s < ns ? s : ns - 1;
  const T *Xl = X + (int64_t)lat * strideX, *Vl = V + (int64_t)lat * strideV;
  const int j_begin = sp * rows, j_end = j_begin + rows < n ? j_begin + rows : n;

  prm.stage(lat, d, tab);
  T os = T(1);
  if constexpr (!RFF) os = dx_oscale<T, P::family>(prm.oscale, lat);

  // ---- this lane's test point and its row of G (no G: the one column itself)
  T xs[DC];
#pragma unroll
  for (int k = 0; k < DC; ++k) {
    const T v = Xs[(int64_t)cs * d + (k < d ? k : d - 1)];
    xs[k] = k < d ? v : T(0);
  }
  double g[RC];
#pragma unroll
  for (int c = 0; c < RC; ++c) g[c] = c == 0 ? 1.0 : 0.0;
  if (G) {
    const T *Gl = G + ((int64_t)lat * ns + cs) * r;
#pragma unroll
    for (int c = 0; c < RC; ++c) {
      const T v = Gl[c < r ? c : r - 1];
      g[c] = c < r ? (double)v : 0.0;
    }
  }
  double acc[DC];                                    // this wave's share of the segment
#pragma unroll
  for (int k = 0; k < DC; ++k) {
    acc[k] = 0.0;
    if (jp == 0) sTot[k * CM_TS + sl] = 0.0;
  }

#pragma unroll 1
  for (int j0 = j_begin; j0 < j_end; j0 += CM_JC) {
    __syncthreads();                                 // the table is staged; the previous chunk and the last meeting are consumed
    for (int e = tid; e < CM_JC * DC; e += NTHREADS) {
      const int jl = e / DC, k = e % DC;
      const int cj = j0 + jl < n ? j0 + jl : n - 1;
      const T v = Xl[(int64_t)cj * d + (k < d ? k : d - 1)];
      sX[e] = k < d ? v : T(0);
    }
    for (int e = tid; e < CM_JC * RC; e += NTHREADS) {
      const int jl = e / RC, c = e % RC;
      const int cj = j0 + jl < n ? j0 + jl : n - 1;
      const T v = Vl[(int64_t)cj * ldv + (c < r ? c : r - 1)];
      sV[e] = (c < r && j0 + jl < j_end) ? v : T(0);
    }
    if constexpr (RFF) {
      if (tid < CM_JC) sPh[tid] = phase[(int64_t)lat * n + (j0 + tid < n ? j0 + tid : n - 1)];
    }
    __syncthreads();
    const int jw = jp * CM_JW;                       // this wave's rows: the same in every lane, so sX, sV and the table are broadcasts
#pragma unroll 1
    for (int jj = 0; jj < CM_JW; ++jj) {
      const int row = jw + jj;
      double w = 0.0;
#pragma unroll
      for (int c = 0; c < RC; ++c) w = __builtin_fma(g[c], (double)sV[row * RC + c], w);
      prm.add(xs, sX + row * DC, RFF ? sPh[row] : T(0), tab, os, j0 + row < j_end ? w : 0.0, acc);
    }
    if ((j0 + CM_JC) % seg != 0 && j0 + CM_JC < j_end) continue;
    // ---- a segment ends: its four waves in a fixed order; wave 0 hands the sums on or adds them to the segments before it
    const int64_t sg = j0 / seg;
#pragma unroll
    for (int k0 = 0; k0 < DC; k0 += KP) {
      if (k0 < d) {                                  // (the same in every thread)
        __syncthreads();
        if (jp > 0) {
#pragma unroll
          for (int kk = 0; kk < KP; ++kk) sRed[((jp - 1) * KP + kk) * CM_TS + sl] = acc[k0 + kk];
        }
        __syncthreads();
        if (jp == 0) {
#pragma unroll
          for (int kk = 0; kk < KP; ++kk) {
            double sum = acc[k0 + kk];
#pragma unroll
            for (int w = 0; w < CM_JP - 1; ++w) sum += sRed[(w * KP + kk) * CM_TS + sl];
            if (part) {
              if (s < ns && k0 + kk < d) part[((sg * q + lat) * ns + s) * d + k0 + kk] = sum;
            } else {
              sTot[(k0 + kk) * CM_TS + sl] += sum;
            }
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < DC; ++k) acc[k] = 0.0;
  }

  if (!part && jp == 0 && s < ns) {
    double scale = 1.0;
    if constexpr (RFF) scale = CMD_M2PI * (double)tab[0];
#pragma unroll
    for (int k = 0; k < DC; ++k)
      if (k < d) Jx[((int64_t)lat * ns + s) * d + k] = sTot[k * CM_TS + sl] * scale;
  }
}

// Jx[e] = (-2 pi scale[latent of e], features; else 1) * the sum over the segments, in their order, of part[segment][e]
template <typename T>
__global__ __launch_bounds__(NTHREADS) void k_cross_matvec_dx_reduce(const double *__restrict__ part, int nseg, int64_t count, int64_t per_latent,
                                                                      bool rff, const T *__restrict__ scale, double *__restrict__ Jx) {
  const int64_t e = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  const int64_t ce = e < count ? e : count - 1;
  const double *p = part + ce;
  double sum = 0.0;
  for (int g = 0; g < nseg; ++g) sum += p[(int64_t)g * count];
  if (rff) {
    T sc = T(1);
    if (scale) sc = scale[ce / per_latent];
    sum *= CMD_M2PI * (double)sc;
  }
  if (e < count) Jx[e] = sum;
}

// the launches of one call, once the arguments are checked
template <typename T, int DC, class P>
int cross_matvec_dx_launch(const char *fn, const P &prm, const T *scale, const T *X, int64_t strideX, const T *phase, int n, const T *Xs, int ns, int d,
                           const T *V, int64_t ldv, int64_t strideV, int r, const T *G, double *Jx, void *partials, int q, hipStream_t st) {
  const int rows = cross_matvec_rows(n, ns, q), nsplit = cross_matvec_splits(n, ns, q), seg = cross_matvec_segment(n);
  double *part = nsplit == 1 ? nullptr : (double *)partials;
  const dim3 grid((unsigned)((ns + CM_TS - 1) / CM_TS), (unsigned)nsplit, (unsigned)q), block(NTHREADS);
  ProfScope ps(PK_CROSS_MATVEC_DX, st, 2.0 * q * n * (double)ns * (r + d), (double)q * (n + (double)ns) * r * sizeof(T));
  if (r == 1)
    hipLaunchKernelGGL((k_cross_matvec_dx<T, DC, 1, P>), grid, block, 0, st, prm, X, strideX, phase, n, Xs, ns, d, V, ldv, strideV, r, G, rows, seg, part,
                       Jx);
  else
    hipLaunchKernelGGL((k_cross_matvec_dx<T, DC, CM_MAX_COLS, P>), grid, block, 0, st, prm, X, strideX, phase, n, Xs, ns, d, V, ldv, strideV, r, G, rows,
                       seg, part, Jx);
  if (nsplit > 1) {
    const int64_t count = (int64_t)q * ns * d;
    hipLaunchKernelGGL(k_cross_matvec_dx_reduce<T>, dim3((unsigned)((count + NTHREADS - 1) / NTHREADS)), block, 0, st, (const double *)partials,
                       cross_matvec_segments(n), count, (int64_t)ns * d, P::rff, scale, Jx);
  }
  return launch_status(fn);
}

template <typename T>
int cross_matvec_dx_impl(const CovTable &t, const T *X, int n, const T *Xs, int ns, const T *V, int64_t ldv, int64_t strideV, int r, const T *G,
                         double *Jx, void *partials, int q, void *stream) {
  // the diagonal of these depends on x: the families plmc_posterior_dx refuses
  if (const char *why = dx_refusal(t)) return fail(__func__, why);
  PLMC_REQUIRE(X && Xs && V && Jx && t.ell, "null pointer");
  PLMC_REQUIRE_TABLE(t);
  const int d = t.d;
  PLMC_REQUIRE((t.family != COV_PLAIN && t.family != COV_ADD) || (t.kind >= 0 && t.kind <= K_MATERN52), "unknown kernel kind");
  PLMC_REQUIRE(d > 0 && d <= MAX_DIM, "need 0 < d <= plmc_max_dim()");
  PLMC_CM_REQUIRE_SHAPE(n, ns, r, q, ldv, strideV, partials);
  PLMC_REQUIRE(G || r == 1, "null pointer: G (G == NULL takes r == 1)");
  hipStream_t st = (hipStream_t)stream;
  int rc = 0;
  const auto go = [&](auto f, auto dc) {
    constexpr CovFamily F = decltype(f)::value;
    constexpr int DC = decltype(dc)::value;
    if constexpr (F != COV_SUM && F != COV_DOT) {
      DxFamily<T, F, DC> prm;
      prm.kind = t.kind, prm.ncomp = t.ncomp;
      prm.ell = (const T *)t.ell, prm.second = (const T *)t.second, prm.third = (const T *)t.third, prm.oscale = (const T *)t.oscale;
      rc = cross_matvec_dx_launch<T, DC>("cross_matvec_dx_impl", prm, (const T *)nullptr, X, 0, (const T *)nullptr, n, Xs, ns, d, V, ldv, strideV, r, G, Jx,
                                         partials, q, st);
    }
  };
  switch (t.family) {
    case COV_PLAIN:
    case COV_ADD: {                                  // (the plain kernel is a table of one component, as in posterior_dx.hip)
      constexpr std::integral_constant<CovFamily, COV_ADD> f{};
      if (d <= 4) go(f, std::integral_constant<int, 4>());
      else if (d <= 8) go(f, std::integral_constant<int, 8>());
      else if (d <= 16) go(f, std::integral_constant<int, 16>());
      else go(f, std::integral_constant<int, 32>());
      break;
    }
    default:
      with_capacity<0>(t.family, d, go);
  }
  return rc;
}

template <typename T>
int rff_matvec_dx_impl(const T *freq, const T *phase, int m, const T *Xs, int ns, int d, const T *Wt, int r, const T *G, const T *scale, double *Jx,
                       void *partials, int q, void *stream) {
  PLMC_REQUIRE(freq && phase && Xs && Wt && Jx, "null pointer");
  PLMC_REQUIRE(d > 0 && d <= MAX_DIM, "need 0 < d <= plmc_max_dim()");
  const int64_t ldw = r, strideW = (int64_t)m * r;
  PLMC_CM_REQUIRE_SHAPE(m, ns, r, q, ldw, strideW, partials);
  PLMC_REQUIRE(G || r == 1, "null pointer: G (G == NULL takes r == 1)");
  hipStream_t st = (hipStream_t)stream;
  const auto go = [&](auto dc) {
    constexpr int DC = decltype(dc)::value;
    return cross_matvec_dx_launch<T, DC>("rff_matvec_dx_impl", DxRff<T, DC>{scale}, scale, freq, (int64_t)m * d, phase, m, Xs, ns, d, Wt, ldw, strideW, r, G,
                                         Jx, partials, q, st);
  };
  if (d <= 4) return go(std::integral_constant<int, 4>());
  if (d <= 8) return go(std::integral_constant<int, 8>());
  if (d <= 16) return go(std::integral_constant<int, 16>());
  return go(std::integral_constant<int, 32>());
}

}  // namespace plmc

extern "C" {
int plmc_cross_matvec_dx_splits(int n, int ns, int q) { return n > 0 && ns > 0 && q > 0 ? plmc::cross_matvec_splits(n, ns, q) : 0; }
int64_t plmc_cross_matvec_dx_partials_bytes(int n, int ns, int d, int q) {
  const int splits = plmc_cross_matvec_dx_splits(n, ns, q);
  return splits > 1 && d > 0 ? (int64_t)plmc::cross_matvec_segments(n) * q * ns * d * (int64_t)sizeof(double) : 0;
}
// the entry points of the families (api_common.hpp, PLMC_FAMILY_ENTRIES)
#define PLMC_CROSS_MATVEC_DX_ENTRY(SUF, T, INFIX, LEAD, PARAMS, TABLE)                                                                         \
  int plmc_cross_matvec_dx##INFIX##_##SUF(PLMC_LEAD_##LEAD const T *X, int n, const T *Xs, int ns, int d, PLMC_UNPACK PARAMS, const T *V,     \
                                          int64_t ldv, int64_t strideV, int r, const T *G, double *Jx, void *partials, int q, void *stream) { \
    return plmc::cross_matvec_dx_impl<T>(TABLE, X, n, Xs, ns, V, ldv, strideV, r, G, Jx, partials, q, stream);                                \
  }
PLMC_FAMILY_ENTRIES(PLMC_CROSS_MATVEC_DX_ENTRY, f32, float)
PLMC_FAMILY_ENTRIES(PLMC_CROSS_MATVEC_DX_ENTRY, f64, double)
#undef PLMC_CROSS_MATVEC_DX_ENTRY
int plmc_rff_matvec_dx_f32(const float *freq, const float *phase, int m, const float *Xs, int ns, int d, const float *Wt, int r, const float *G,
                           const float *scale, double *Jx, void *partials, int q, void *stream) {
  return plmc::rff_matvec_dx_impl<float>(freq, phase, m, Xs, ns, d, Wt, r, G, scale, Jx, partials, q, stream);
}
int plmc_rff_matvec_dx_f64(const double *freq, const double *phase, int m, const double *Xs, int ns, int d, const double *Wt, int r, const double *G,
                           const double *scale, double *Jx, void *partials, int q, void *stream) {
  return plmc::rff_matvec_dx_impl<double>(freq, phase, m, Xs, ns, d, Wt, r, G, scale, Jx, partials, q, stream);
}
}
