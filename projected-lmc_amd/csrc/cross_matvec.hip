// cross_matvec.hip -- products with a cross-covariance that is never written: for q latents on the training inputs
// X (n x d), test inputs Xs (ns x d) and r <= CM_MAX_COLS columns V (n x r per latent, leading dimension ldv),
//   Out[lat][s][c] = sum_{i < n} k_lat(xs_s, x_i) V[lat][i][c]                                          (plmc_cross_matvec*)
// where k_lat is the noise-free value plmc_assemble_cross* writes for the same table: the tables and their value() of cov_tables.hpp,
// the plain kernel (and the spline) on coordinates divided by the lengthscale as k_assemble_cross forms them; and the prior part of a
// pathwise posterior draw from m random Fourier features, frequencies and phases in revolutions,
//   Out[lat][s][c] = scale[lat] sum_{j < m} cos(2 pi (freq[lat][j] . xs_s + phase[lat][j])) Wt[lat][j][c]  (plmc_rff_matvec).
// One kernel serves both: a "row" is a training input or a feature, a "pair" its value against the lane's test point.
// One workgroup per (block of CM_TS test points, range of rows, latent).  A lane owns one test point and its r sums; the four waves
// take a quarter of every staged chunk of rows each, whose coordinates, columns of V and the latent's table are LDS broadcasts.  The
// value of a pair is of the element type; its products with V and the sums are fp64, in ONE fixed order that depends on the row count
// alone: the rows are cut into segments of cross_matvec_segment(n) rows; within a segment every wave adds its rows in order and the
// four waves meet in order through LDS; the segments are added in order, and the sum is rounded once to the element type.  When few
// test points leave the machine idle the segments are dealt to cross_matvec_splits() workgroups (a function of the row count, ns and
// q alone), which write one fp64 sum per segment to the caller's `partials` for k_cross_matvec_reduce to add in that same order: an
// output element has the same bits whether or not the call splits, whichever lane owns its test point and however many test points
// the call has.  No atomics, no scratch, every output element written once, two calls give the same bits.
// Indices are clamped into range before the address is formed and the term is selected afterwards: nothing is read from rows >= n of
// X or V or from columns >= r of V, every load is unconditional, nothing outside Out[.][< ns][< r] is written.
#include "api_common.hpp"
#include "covariance.hpp"
#include "cov_tables.hpp"
#include "cross_matvec_order.hpp"
#include "../../include/plmc.h"

namespace plmc {

// The plain kernel as k_assemble_cross evaluates it: both points divided by the lengthscale (the rows when they are staged, the test
// point once per lane), the squared distance over the DCAP slots in order, the spline from its factors.  In LDS: ell [DCAP] (1 beyond d), os.
template <typename T, int DCAP> struct PlainTable {
  static constexpr int LDS = DCAP + 1;
  int kind, d;
  const T *ell, *oscale;
  __device__ __forceinline__ void stage(int lat, int, T *par) const {
    const int tid = threadIdx.x;
    if (tid < DCAP) {
      const T v = ell[(int64_t)lat * d + (tid < d ? tid : d - 1)];
      par[tid] = tid < d ? v : T(1);
    }
    if (tid == 0) par[DCAP] = oscale ? oscale[lat] : T(1);
  }
  __device__ __forceinline__ T value(const T *xa, const T (&xs)[DCAP], const T *par) const {
    T r2 = T(0), sp = T(1);
#pragma unroll
    for (int k = 0; k < DCAP; ++k) {
      const T df = xa[k] - xs[k];
      r2 += df * df;
      if (kind == K_SPLINE && k < d) sp *= spline_factor(xa[k], xs[k]);
    }
    return par[DCAP] * (kind == K_SPLINE ? sp : kern_value<T>(kind, r2));
  }
};

// One random Fourier feature against the lane's point: cos(2 pi (sum_k f_k x_k + b)), f and b in revolutions, the phase reduced in
// revolutions term by term (rff_phase, cross_matvec_order.hpp), then sm_cos.
template <typename T, int DCAP> struct RffTable {
  static constexpr int LDS = 1;
  const T *scale;
  __device__ __forceinline__ void stage(int lat, int, T *par) const {
    if (threadIdx.x == 0) par[0] = scale ? scale[lat] : T(1);
  }
  __device__ __forceinline__ T value(const T *fa, T b, const T (&xs)[DCAP]) const {
    return sm_cos(rff_phase<T, DCAP>(fa, b, xs));
  }
};
template <class P> struct cm_traits { static constexpr bool plain = false, rff = false; };
template <typename T, int DC> struct cm_traits<PlainTable<T, DC>> { static constexpr bool plain = true, rff = false; };
template <typename T, int DC> struct cm_traits<RffTable<T, DC>> { static constexpr bool plain = false, rff = true; };

// X: the rows, (n, d), `strideX` elements from one latent's to the next (0: shared by the latents); phase: (q, n), features only.
// RC: capacity of the lane's sums, 1 or CM_MAX_COLS.  `rows`: rows of this workgroup's range, `seg`: of a segment (rows a multiple of
// seg, seg of CM_JC).  part != null: the segments' sums go there in fp64, [segment][lat][s][c], unscaled; else their sum goes to Out.
template <typename T, int DC, int RC, class P>
__global__ __launch_bounds__(NTHREADS) void k_cross_matvec(const P prm, const T *__restrict__ X, int64_t strideX, const T *__restrict__ phase, int n,
                                                            const T *__restrict__ Xs, int ns, int d, const T *__restrict__ V, int64_t ldv,
                                                            int64_t strideV, int r, int rows, int seg, double *__restrict__ part, T *__restrict__ Out) {
  constexpr bool PLAIN = cm_traits<P>::plain, RFF = cm_traits<P>::rff;
  __shared__ __align__(16) T sX[CM_JC * DC];         // the chunk's rows (0 beyond d)
  __shared__ T sV[CM_JC * RC];                       // their columns of V (0 beyond r and beyond the range)
  __shared__ T sPh[RFF ? CM_JC : 1];                 // features: their phases
  __shared__ T par[P::LDS];                          // the latent's table
  __shared__ double sRed[(CM_JP - 1) * RC * CM_TS];  // the other waves' sums
  const int tid = threadIdx.x, tb = blockIdx.x, sp = blockIdx.y, lat = blockIdx.z, q = gridDim.z;
  const int sl = tid & (CM_TS - 1), jp = tid / CM_TS;
  const int s = tb * CM_TS + sl, cs = s < ns ? s : ns - 1;
  const T *Xl = X + (int64_t)lat * strideX, *Vl = V + (int64_t)lat * strideV;
  const int j_begin = sp * rows, j_end = j_begin + rows < n ? j_begin + rows : n;

  prm.stage(lat, d, par);

  // ---- this lane's test point
  T xs[DC];
#pragma unroll
  for (int k = 0; k < DC; ++k) {
    const int ck = k < d ? k : d - 1;
    T v = Xs[(int64_t)cs * d + ck];
    if constexpr (PLAIN) v = v / prm.ell[(int64_t)lat * d + ck];
    xs[k] = k < d ? v : T(0);
  }
  double acc[RC], tot[RC];                           // this wave's share of the segment; wave 0: the segments so far
#pragma unroll
  for (int c = 0; c < RC; ++c) acc[c] = tot[c] = 0.0;

#pragma unroll 1
  for (int j0 = j_begin; j0 < j_end; j0 += CM_JC) {
    __syncthreads();                                 // the table is staged; the previous chunk is consumed
    for (int e = tid; e < CM_JC * DC; e += NTHREADS) {
      const int jl = e / DC, k = e % DC, ck = k < d ? k : d - 1;
      const int cj = j0 + jl < n ? j0 + jl : n - 1;
      T v = Xl[(int64_t)cj * d + ck];
      if constexpr (PLAIN) v = v / prm.ell[(int64_t)lat * d + ck];
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
      T kv;
      if constexpr (RFF) kv = prm.value(sX + row * DC, sPh[row], xs);
      else kv = prm.value(sX + row * DC, xs, par);
      const double kd = j0 + row < j_end ? (double)kv : 0.0;
#pragma unroll
      for (int c = 0; c < RC; ++c) acc[c] = __builtin_fma(kd, (double)sV[row * RC + c], acc[c]);
    }
    if ((j0 + CM_JC) % seg != 0 && j0 + CM_JC < j_end) continue;
    // ---- a segment ends: its four waves in a fixed order; wave 0 hands the sum on or adds it to the segments before it
    __syncthreads();
    if (jp > 0) {
#pragma unroll
      for (int c = 0; c < RC; ++c) sRed[((jp - 1) * RC + c) * CM_TS + sl] = acc[c];
    }
    __syncthreads();                                 // (the barrier at the head of the next chunk keeps sRed until wave 0 has read it)
    if (jp == 0) {
      const int64_t sg = j0 / seg;
#pragma unroll
      for (int c = 0; c < RC; ++c) {
        double sum = acc[c];
#pragma unroll
        for (int w = 0; w < CM_JP - 1; ++w) sum += sRed[(w * RC + c) * CM_TS + sl];
        if (part) {
          if (s < ns && c < r) part[((sg * q + lat) * ns + s) * r + c] = sum;
        } else {
          tot[c] += sum;
        }
      }
    }
#pragma unroll
    for (int c = 0; c < RC; ++c) acc[c] = 0.0;
  }

  if (!part && jp == 0 && s < ns) {
    double scale = 1.0;
    if constexpr (RFF) scale = (double)par[0];
#pragma unroll
    for (int c = 0; c < RC; ++c)
      if (c < r) Out[((int64_t)lat * ns + s) * r + c] = (T)(tot[c] * scale);
  }
}

// Out[e] = scale[latent of e] * the sum over the segments, in their order, of part[segment][e], rounded once (scale null: 1)
template <typename T>
__global__ __launch_bounds__(NTHREADS) void k_cross_matvec_reduce(const double *__restrict__ part, int nseg, int64_t count, int64_t per_latent,
                                                                   const T *__restrict__ scale, T *__restrict__ Out) {
  const int64_t e = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  const int64_t ce = e < count ? e : count - 1;
  const double *p = part + ce;
  double sum = 0.0;
  for (int g = 0; g < nseg; ++g) sum += p[(int64_t)g * count];
  if (scale) sum *= (double)scale[ce / per_latent];
  if (e < count) Out[e] = (T)sum;
}

// the launches of one call, once the arguments are checked
template <typename T, int DC, class P>
int cross_matvec_launch(const char *fn, const P &prm, const T *scale, const T *X, int64_t strideX, const T *phase, int n, const T *Xs, int ns, int d, const T *V,
                        int64_t ldv, int64_t strideV, int r, T *Out, void *partials, int q, hipStream_t st) {
  const int rows = cross_matvec_rows(n, ns, q), nsplit = cross_matvec_splits(n, ns, q), seg = cross_matvec_segment(n);
  double *part = nsplit == 1 ? nullptr : (double *)partials;
  const dim3 grid((unsigned)((ns + CM_TS - 1) / CM_TS), (unsigned)nsplit, (unsigned)q), block(NTHREADS);
  ProfScope ps(PK_CROSS_MATVEC, st, 2.0 * q * n * (double)ns * r, (double)q * n * r * sizeof(T));
  if (r == 1)
    hipLaunchKernelGGL((k_cross_matvec<T, DC, 1, P>), grid, block, 0, st, prm, X, strideX, phase, n, Xs, ns, d, V, ldv, strideV, r, rows, seg, part, Out);
  else
    hipLaunchKernelGGL((k_cross_matvec<T, DC, CM_MAX_COLS, P>), grid, block, 0, st, prm, X, strideX, phase, n, Xs, ns, d, V, ldv, strideV, r, rows,
                       seg, part, Out);
  if (nsplit > 1) {
    const int64_t count = (int64_t)q * ns * r;
    hipLaunchKernelGGL(k_cross_matvec_reduce<T>, dim3((unsigned)((count + NTHREADS - 1) / NTHREADS)), block, 0, st, (const double *)partials,
                       cross_matvec_segments(n), count, (int64_t)ns * r, scale, Out);
  }
  return launch_status(fn);
}

template <typename T>
int cross_matvec_impl(const CovTable &t, const T *X, int n, const T *Xs, int ns, const T *V, int64_t ldv, int64_t strideV, int r, T *Out,
                      void *partials, int q, void *stream) {
  PLMC_REQUIRE(X && Xs && V && Out && t.ell, "null pointer");
  PLMC_REQUIRE_TABLE(t);
  const int d = t.d;
  PLMC_REQUIRE(t.kind >= 0 && t.kind <= K_SPLINE, "unknown kernel kind");
  PLMC_REQUIRE(d > 0 && d <= MAX_DIM, "need 0 < d <= plmc_max_dim()");
  PLMC_CM_REQUIRE_SHAPE(n, ns, r, q, ldv, strideV, partials);
  hipStream_t st = (hipStream_t)stream;
  int rc = 0;
  const auto go = [&](const auto &prm, auto dc) {
    rc = cross_matvec_launch<T, decltype(dc)::value>("cross_matvec_impl", prm, (const T *)nullptr, X, 0, (const T *)nullptr, n, Xs, ns, d, V, ldv, strideV, r, Out, partials,
                                                    q, st);
  };
  const auto by_dim = [&](auto make) {               // the capacities of the stationary kinds: every d up to MAX_DIM
    if (d <= 4) make(std::integral_constant<int, 4>());
    else if (d <= 8) make(std::integral_constant<int, 8>());
    else if (d <= 16) make(std::integral_constant<int, 16>());
    else make(std::integral_constant<int, 32>());
  };
  switch (t.route()) {                               // (the routing of assemble_cross_impl: one additive component IS the plain kernel)
    case COV_PLAIN:
      by_dim([&](auto dc) { go(PlainTable<T, decltype(dc)::value>{t.kind, d, (const T *)t.ell, (const T *)t.oscale}, dc); });
      break;
    case COV_ADD:
      by_dim([&](auto dc) { go(device_table<T, COV_ADD, decltype(dc)::value>(t), dc); });
      break;
    default:
      with_capacity<0>(t.family, d, [&](auto f, auto dc) { go(device_table<T, decltype(f)::value, decltype(dc)::value>(t), dc); });
  }
  return rc;
}

template <typename T>
int rff_matvec_impl(const T *freq, const T *phase, int m, const T *Xs, int ns, int d, const T *Wt, int r, const T *scale, T *Out, void *partials,
                    int q, void *stream) {
  PLMC_REQUIRE(freq && phase && Xs && Wt && Out, "null pointer");
  PLMC_REQUIRE(d > 0 && d <= MAX_DIM, "need 0 < d <= plmc_max_dim()");
  const int64_t ldw = r, strideW = (int64_t)m * r;
  PLMC_CM_REQUIRE_SHAPE(m, ns, r, q, ldw, strideW, partials);
  hipStream_t st = (hipStream_t)stream;
  const auto go = [&](auto dc) {
    constexpr int DC = decltype(dc)::value;
    return cross_matvec_launch<T, DC>("rff_matvec_impl", RffTable<T, DC>{scale}, scale, freq, (int64_t)m * d, phase, m, Xs, ns, d, Wt, ldw, strideW, r, Out,
                                      partials, q, st);
  };
  if (d <= 4) return go(std::integral_constant<int, 4>());
  if (d <= 8) return go(std::integral_constant<int, 8>());
  if (d <= 16) return go(std::integral_constant<int, 16>());
  return go(std::integral_constant<int, 32>());
}

}  // namespace plmc

extern "C" {
int plmc_cross_matvec_max_cols(void) { return plmc::CM_MAX_COLS; }
int plmc_cross_matvec_splits(int n, int ns, int q) { return n > 0 && ns > 0 && q > 0 ? plmc::cross_matvec_splits(n, ns, q) : 0; }
int64_t plmc_cross_matvec_partials_bytes(int n, int ns, int r, int q) {
  const int splits = plmc_cross_matvec_splits(n, ns, q);
  return splits > 1 && r > 0 ? (int64_t)plmc::cross_matvec_segments(n) * q * ns * r * (int64_t)sizeof(double) : 0;
}
// the entry points of the families (api_common.hpp, PLMC_FAMILY_ENTRIES)
#define PLMC_CROSS_MATVEC_ENTRY(SUF, T, INFIX, LEAD, PARAMS, TABLE)                                                                         \
  int plmc_cross_matvec##INFIX##_##SUF(PLMC_LEAD_##LEAD const T *X, int n, const T *Xs, int ns, int d, PLMC_UNPACK PARAMS, const T *V,     \
                                       int64_t ldv, int64_t strideV, int r, T *Out, void *partials, int q, void *stream) {                 \
    return plmc::cross_matvec_impl<T>(TABLE, X, n, Xs, ns, V, ldv, strideV, r, Out, partials, q, stream);                                  \
  }
PLMC_FAMILY_ENTRIES(PLMC_CROSS_MATVEC_ENTRY, f32, float)
PLMC_FAMILY_ENTRIES(PLMC_CROSS_MATVEC_ENTRY, f64, double)
#undef PLMC_CROSS_MATVEC_ENTRY
int plmc_rff_matvec_f32(const float *freq, const float *phase, int m, const float *Xs, int ns, int d, const float *Wt, int r, const float *scale,
                        float *Out, void *partials, int q, void *stream) {
  return plmc::rff_matvec_impl<float>(freq, phase, m, Xs, ns, d, Wt, r, scale, Out, partials, q, stream);
}
int plmc_rff_matvec_f64(const double *freq, const double *phase, int m, const double *Xs, int ns, int d, const double *Wt, int r,
                        const double *scale, double *Out, void *partials, int q, void *stream) {
  return plmc::rff_matvec_impl<double>(freq, phase, m, Xs, ns, d, Wt, r, scale, Out, partials, q, stream);
}
}
