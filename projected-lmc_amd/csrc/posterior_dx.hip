// posterior_dx.hip -- derivative of the eval-mode posterior moments with respect to the test inputs: for q latents on the
// training inputs X (n x d), test inputs Xs (ns x d), alpha = Khat^-1 y and B = Khat^-1 K*^T (n x ns per latent, contiguous along s),
//   Jm[lat][s][k] = d mean(s) / d x*_s[k] =      sum_{i < n} alpha_i  d k_lat(x*_s, x_i) / d x*_s[k]
//   Jv[lat][s][k] = d var(s)  / d x*_s[k] = -2 * sum_{i < n} B[i][s]  d k_lat(x*_s, x_i) / d x*_s[k]
// for the families whose diagonal k(x, x) does not depend on x.  Test points do not interact in the marginal moments: this is the whole
// Jacobian.  The unit derivative of a pair is evaluated once (the family's *_dx of covariance.hpp with g = 1, the accurate forms) and
// weighted twice, in fp64.
// One workgroup per (block of PD_TS test points, range of training rows, latent).  A lane owns one test point, so a wave reads a row of B
// coalesced; the four waves take a quarter of every staged chunk of training rows each, whose coordinates, alpha and the latent's table
// are LDS broadcasts.  The four waves' fp64 sums meet in LDS in a fixed order.  With few test points the training range is split over
// posterior_dx_splits() workgroups (a function of n, ns and q alone), whose partial sums go to the caller's `partials` and are added in
// the order of the ranges by k_posterior_dx_reduce; with one range the outputs are written directly.  No atomics, no scratch, every
// output element written once, two calls give the same bits.
// Indices are clamped into range before the address is formed and the term is selected afterwards: nothing is read from rows >= n of B,
// from alpha past n or from columns >= ns, and every load is unconditional (B == NULL: none from B, Jv untouched).
#include "api_common.hpp"
#include "covariance.hpp"
#include "input_dx.hpp"
#include "../../include/plmc.h"

namespace plmc {

constexpr int PD_TS = 64;                            // test points per workgroup: one per lane
constexpr int PD_JP = NTHREADS / PD_TS;              // waves, each with its share of a chunk
constexpr int PD_JC = 64;                            // training rows per staged chunk
constexpr int PD_JW = PD_JC / PD_JP;                 // of which one wave takes these
constexpr int PD_MIN_ROWS = 256;                     // shortest training range worth a workgroup of its own
#ifndef PLMC_PDX_TARGET_WGS
#define PLMC_PDX_TARGET_WGS 512                      // workgroups wanted: two per compute unit (dev builds: 1 = never split)
#endif
static_assert(PD_TS == 64 && NTHREADS % PD_TS == 0 && PD_JC % PD_JP == 0 && PD_MIN_ROWS % PD_JC == 0, "posterior-dx thread map");

// Ranges the training rows are split into, and the rows of one (a multiple of PD_JC): as many as bring the launch to
// PLMC_PDX_TARGET_WGS workgroups, none shorter than PD_MIN_ROWS.
static int posterior_dx_rows(int n, int ns, int q) {
  const int64_t wgs = (int64_t)((ns + PD_TS - 1) / PD_TS) * q;
  int64_t want = (PLMC_PDX_TARGET_WGS + wgs - 1) / wgs;
  const int64_t most = (n + PD_MIN_ROWS - 1) / PD_MIN_ROWS;
  want = want < 1 ? 1 : (want > most ? most : want);
  const int64_t rows = ((n + want - 1) / want + PD_JC - 1) / PD_JC * PD_JC;
  return (int)rows;
}
static int posterior_dx_splits(int n, int ns, int q) {
  const int rows = posterior_dx_rows(n, ns, q);
  return (n + rows - 1) / rows;
}

template <int DC> constexpr int pd_kp() { return DC < 4 ? DC : 4; }   // dimensions per pass of the wave reduction

template <typename T, CovFamily F, int DC>
__global__ __launch_bounds__(NTHREADS) void k_posterior_dx(int kind, int ncomp, const T *__restrict__ X, int n, const T *__restrict__ Xs, int ns,
                                                            int d, const T *__restrict__ ell, const T *__restrict__ second,
                                                            const T *__restrict__ third, const T *__restrict__ oscale,
                                                            const T *__restrict__ alpha, int64_t n_pad, const T *__restrict__ B, int64_t ldb,
                                                            int64_t strideB, int rows, double *__restrict__ outM, double *__restrict__ outV) {
  constexpr int KP = pd_kp<DC>();
  __shared__ __align__(16) T sX[PD_JC * DC];         // raw inputs of the chunk's rows (0 beyond d)
  __shared__ T sA[PD_JC];                            // their alpha
  __shared__ T tab[IG_TAB];                          // the latent's table
  __shared__ double sRed[(PD_JP - 1) * 2 * KP * PD_TS];   // the other waves' sums, KP dimensions at a time
  const int tid = threadIdx.x, tb = blockIdx.x, sp = blockIdx.y, lat = blockIdx.z, q = gridDim.z;
  const int sl = tid & (PD_TS - 1), jp = tid / PD_TS;
  const int s = tb * PD_TS + sl, cs = s < ns ? s : ns - 1;
  const bool hasB = B != nullptr;
  const T *Bl = B + (int64_t)lat * strideB + cs;     // (not dereferenced without B)
  const T *al = alpha + (int64_t)lat * n_pad;
  const int j_begin = sp * rows, j_end = j_begin + rows < n ? j_begin + rows : n;

  dx_stage_table<T, F, DC>(tab, tid, lat, d, ncomp, ell, second, third, oscale);
  const T os = dx_oscale<T, F>(oscale, lat);

  // ---- this lane's test point
  T xs[DC];
#pragma unroll
  for (int k = 0; k < DC; ++k) {
    const T v = Xs[(int64_t)cs * d + (k < d ? k : d - 1)];
    xs[k] = k < d ? v : T(0);
  }
  double sm[DC], sv[DC];
#pragma unroll
  for (int k = 0; k < DC; ++k) sm[k] = sv[k] = 0.0;

#pragma unroll 1
  for (int j0 = j_begin; j0 < j_end; j0 += PD_JC) {
    __syncthreads();                                 // the table is staged; the previous chunk is consumed
    for (int e = tid; e < PD_JC * DC; e += NTHREADS) {
      const int jl = e / DC, k = e % DC;
      const int cj = j0 + jl < n ? j0 + jl : n - 1;
      const T v = X[(int64_t)cj * d + (k < d ? k : d - 1)];
      sX[e] = k < d ? v : T(0);
    }
    if (tid < PD_JC) sA[tid] = al[j0 + tid < n ? j0 + tid : n - 1];
    const int jw = j0 + jp * PD_JW;                  // this wave's rows: the same in every lane, so sX, sA and the table are broadcasts
    T bcur = T(0);
    if (hasB) bcur = Bl[(int64_t)(jw < n ? jw : n - 1) * ldb];
    __syncthreads();
#pragma unroll 1
    for (int jj = 0; jj < PD_JW; ++jj) {
      const int gj = jw + jj;
      T bnext = T(0);                                // the next row's element, ahead of this row's arithmetic
      if (hasB) bnext = Bl[(int64_t)(gj + 1 < n ? gj + 1 : n - 1) * ldb];
      const bool take = gj < j_end;
      T u[DC];
#pragma unroll
      for (int k = 0; k < DC; ++k) u[k] = T(0);
      dx_pair<T, F, DC>(kind, ncomp, xs, sX + (jp * PD_JW + jj) * DC, tab, T(1), os, u);
      const double wa = (double)sA[jp * PD_JW + jj], wb = -2.0 * (double)bcur;
#pragma unroll
      for (int k = 0; k < DC; ++k) {
        const double uk = (double)u[k];
        sm[k] += take ? wa * uk : 0.0;
        sv[k] += take ? wb * uk : 0.0;
      }
      bcur = bnext;
    }
  }

  // ---- the four waves of every test point, in a fixed order, then this range's sums
  double *om = outM + (((int64_t)sp * q + lat) * ns + cs) * d;
  double *ov = outV + (((int64_t)sp * q + lat) * ns + cs) * d;
#pragma unroll
  for (int k0 = 0; k0 < DC; k0 += KP) {
    __syncthreads();
    if (jp > 0) {
#pragma unroll
      for (int kk = 0; kk < KP; ++kk) {
        sRed[((jp - 1) * 2 * KP + kk) * PD_TS + sl] = sm[k0 + kk];
        sRed[((jp - 1) * 2 * KP + KP + kk) * PD_TS + sl] = sv[k0 + kk];
      }
    }
    __syncthreads();
    if (jp == 0 && s < ns) {
#pragma unroll
      for (int kk = 0; kk < KP; ++kk) {
        double m = sm[k0 + kk], v = sv[k0 + kk];
#pragma unroll
        for (int w = 0; w < PD_JP - 1; ++w) {
          m += sRed[(w * 2 * KP + kk) * PD_TS + sl];
          v += sRed[(w * 2 * KP + KP + kk) * PD_TS + sl];
        }
        if (k0 + kk < d) {
          om[k0 + kk] = m;
          if (hasB) ov[k0 + kk] = v;
        }
      }
    }
  }
}

// out[p][e] = sum over the ranges, in their order, of part[p][range][e]; p = 0 (Jm), 1 (Jv, only when the grid has it)
__global__ __launch_bounds__(NTHREADS) void k_posterior_dx_reduce(const double *__restrict__ part, int nsplit, int64_t count, double *__restrict__ Jm,
                                                                   double *__restrict__ Jv) {
  const int64_t e = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  const int64_t ce = e < count ? e : count - 1;
  const double *p = part + (int64_t)blockIdx.y * nsplit * count + ce;
  double sum = 0.0;
  for (int r = 0; r < nsplit; ++r) sum += p[(int64_t)r * count];
  if (e < count) (blockIdx.y ? Jv : Jm)[e] = sum;
}

template <typename T>
int posterior_dx_impl(const CovTable &t, const T *X, int n, const T *Xs, int ns, const T *alpha, int64_t n_pad, const T *B, int64_t ldb,
                      int64_t strideB, double *Jm, double *Jv, void *partials, int q, void *stream) {
  // the diagonal of these depends on x, which the sum over the training points does not cover
  if (const char *why = dx_refusal(t)) return fail(__func__, why);
  PLMC_REQUIRE_TABLE(t);
  const int kind = t.kind, d = t.d, ncomp = t.ncomp;
  const T *ell = (const T *)t.ell, *oscale = (const T *)t.oscale, *second = (const T *)t.second, *third = (const T *)t.third;
  PLMC_REQUIRE((t.family != COV_PLAIN && t.family != COV_ADD) || (kind >= 0 && kind <= K_MATERN52), "unknown kernel kind");
  PLMC_REQUIRE(d > 0 && d <= MAX_DIM && q > 0 && q <= 65535, "need 0<d<=plmc_max_dim(), 0<q<=65535");
  PLMC_REQUIRE(n > 0 && ns > 0, "need n > 0, ns > 0");
  PLMC_REQUIRE(X && Xs && alpha && ell && Jm, "null pointer");
  PLMC_REQUIRE(!B || Jv, "null pointer: B without Jv");
  PLMC_REQUIRE(n_pad >= n, "alpha: n_pad >= n");
  PLMC_REQUIRE(!B || (ldb >= ns && (q == 1 || strideB >= (int64_t)n * ldb)), "B: ldb >= ns, strideB >= n * ldb");
  const int rows = posterior_dx_rows(n, ns, q), nsplit = posterior_dx_splits(n, ns, q);
  PLMC_REQUIRE(nsplit <= 65535, "too many ranges");
  PLMC_REQUIRE(nsplit == 1 || partials, "null pointer: partials (plmc_posterior_dx_partials_bytes)");
  hipStream_t st = (hipStream_t)stream;
  const int64_t count = (int64_t)q * ns * d;
  double *outM = nsplit == 1 ? Jm : (double *)partials;
  double *outV = nsplit == 1 ? Jv : (double *)partials + (int64_t)nsplit * count;
  const dim3 grid((unsigned)((ns + PD_TS - 1) / PD_TS), (unsigned)nsplit, (unsigned)q), block(NTHREADS);
  ProfScope ps(PK_POSTERIOR_DX, st, 0.0, (B ? (double)q * n * ns : 0.0) * sizeof(T));   // B is read once
#define PLMC_LAUNCH_PD(F, DC) \
  hipLaunchKernelGGL((k_posterior_dx<T, F, DC>), grid, block, 0, st, kind, ncomp, X, n, Xs, ns, d, ell, second, third, oscale, alpha, n_pad, B, ldb, \
                     strideB, rows, outM, outV)
  switch (t.family) {
    case COV_PLAIN:
    case COV_ADD:
      if (d <= 4) PLMC_LAUNCH_PD(COV_ADD, 4);
      else if (d <= 8) PLMC_LAUNCH_PD(COV_ADD, 8);
      else if (d <= 16) PLMC_LAUNCH_PD(COV_ADD, 16);
      else PLMC_LAUNCH_PD(COV_ADD, 32);
      break;
    default:
      with_capacity<0>(t.family, d, [&](auto f, auto dc) {
        constexpr CovFamily F = decltype(f)::value;
        if constexpr (F != COV_SUM && F != COV_DOT) PLMC_LAUNCH_PD(F, decltype(dc)::value);
      });
  }
#undef PLMC_LAUNCH_PD
  if (nsplit > 1) {
    const dim3 rgrid((unsigned)((count + NTHREADS - 1) / NTHREADS), B ? 2u : 1u);
    hipLaunchKernelGGL(k_posterior_dx_reduce, rgrid, block, 0, st, (const double *)partials, nsplit, count, Jm, Jv);
  }
  return launch_status(__func__);
}

}  // namespace plmc

extern "C" {
int plmc_posterior_dx_splits(int n, int ns, int q) { return n > 0 && ns > 0 && q > 0 ? plmc::posterior_dx_splits(n, ns, q) : 0; }
int64_t plmc_posterior_dx_partials_bytes(int n, int ns, int d, int q) {
  const int splits = plmc_posterior_dx_splits(n, ns, q);
  return splits > 1 && d > 0 ? 2 * (int64_t)splits * q * ns * d * (int64_t)sizeof(double) : 0;
}
// the entry points of the families (api_common.hpp, PLMC_FAMILY_ENTRIES)
#define PLMC_POSTERIOR_DX_ENTRY(SUF, T, INFIX, LEAD, PARAMS, TABLE)                                                                             \
  int plmc_posterior_dx##INFIX##_##SUF(PLMC_LEAD_##LEAD const T *X, int n, const T *Xs, int ns, int d, PLMC_UNPACK PARAMS, const T *alpha,     \
                                       int64_t n_pad, const T *B, int64_t ldb, int64_t strideB, double *Jm, double *Jv, void *partials, int q, \
                                       void *stream) {                                                                                         \
    return plmc::posterior_dx_impl<T>(TABLE, X, n, Xs, ns, alpha, n_pad, B, ldb, strideB, Jm, Jv, partials, q, stream);                        \
  }
PLMC_FAMILY_ENTRIES(PLMC_POSTERIOR_DX_ENTRY, f32, float)
PLMC_FAMILY_ENTRIES(PLMC_POSTERIOR_DX_ENTRY, f64, double)
#undef PLMC_POSTERIOR_DX_ENTRY
}
