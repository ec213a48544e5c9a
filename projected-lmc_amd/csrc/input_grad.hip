// input_grad.hip -- gradient of log N(y; 0, Khat) with respect to the inputs: the row-wise pull-back of Omega = alpha alpha^T - Khat^-1
// through the kernel's input derivative,
//   gX[lat][i][k] = sum_{j < n, j != i} (alpha_i alpha_j - P_ij) d k_lat(x_i, x_j) / d x_i[k],
// with P = Khat^-1 as plmc_kinv_grad*_vd_* writes it through its `Kinv` argument: the elements gj >= gi only, so P_ij is read at
// Kinv[min(i, j)][max(i, j)].  No factor 1/2: x_i enters row i and column i of Khat.
// One workgroup per (block of 128 rows, latent) walks the columns j < n in chunks of IG_JC.  A chunk of P is staged in LDS transposed,
// sP[j][i], with the global read along the direction the chunk is stored in: for a block column left of the diagonal block that is our
// row index i (tile (jb, ib) as stored), right of it the column index j (tile (ib, jb)); the diagonal block takes each element from its own
// side.  Then every thread owns one row i and one half of the chunk's columns and adds its terms to d fp64 sums of its own; the two
// halves meet once at the end, in a fixed order.  No atomics, no scratch, every output element written once.
// Indices are clamped into [0, n) before the address is formed and the term is selected afterwards: nothing below the diagonal, in the
// identity padding (rows or columns >= n) or in alpha past n is read, and every load is unconditional.
#include "api_common.hpp"
#include "covariance.hpp"
#include "input_dx.hpp"
#include "../../include/plmc.h"

namespace plmc {

constexpr int IG_JC = 32;                            // columns per staged chunk (NB is a multiple: a chunk lies in one block column)
static_assert(NB % IG_JC == 0 && NTHREADS == 2 * NB && IG_JC % (NTHREADS / NB) == 0 && NTHREADS % IG_JC == 0, "input-gradient thread map");

template <typename T, int DC> constexpr int ig_stage_bytes() { return (IG_JC * (NB + 1) + IG_JC * DC + IG_JC + IG_TAB) * (int)sizeof(T); }
template <typename T, int DC> constexpr int ig_lds_bytes() {
  constexpr int red = NB * DC * (int)sizeof(double);
  return ((ig_stage_bytes<T, DC>() > red ? ig_stage_bytes<T, DC>() : red) + 15) / 16 * 16;
}

// F, the table arguments: input_dx.hpp
template <typename T, CovFamily F, int DC>
__global__ __launch_bounds__(NTHREADS) void k_input_grad(int kind, int ncomp, const T *__restrict__ Kinv, int64_t ldk, int64_t strideK,
                                                          const T *__restrict__ alpha, int64_t n_pad, const T *__restrict__ X, int n, int d,
                                                          const T *__restrict__ ell, const T *__restrict__ second,
                                                          const T *__restrict__ third, const T *__restrict__ oscale,
                                                          double *__restrict__ gX) {
  __shared__ __align__(16) unsigned char raw[ig_lds_bytes<T, DC>()];
  T *sP = reinterpret_cast<T *>(raw);                // [IG_JC][NB + 1]: P_ij of the chunk, column-major
  T *sX = sP + IG_JC * (NB + 1);                     // [IG_JC][DC] raw inputs of the chunk's columns (0 beyond d)
  T *sA = sX + IG_JC * DC;                           // [IG_JC] their alpha
  T *tab = sA + IG_JC;                               // the latent's table
  double *sRed = reinterpret_cast<double *>(raw);    // [DC][NB]: the second half's sums, once the walk is over
  const int tid = threadIdx.x, ib = blockIdx.x, lat = blockIdx.y;
  const int il = tid & (NB - 1), half = tid >> 7;
  const int gi = ib * NB + il, ci = gi < n ? gi : n - 1;
  const T *P = Kinv + (int64_t)lat * strideK;
  const T *al = alpha + (int64_t)lat * n_pad;

  // ---- the latent's table, padded with what makes a slot beyond d add exactly 0
  dx_stage_table<T, F, DC>(tab, tid, lat, d, ncomp, ell, second, third, oscale);
  const T os = dx_oscale<T, F>(oscale, lat);

  // ---- this thread's row
  T xi[DC];
#pragma unroll
  for (int k = 0; k < DC; ++k) {
    const T v = X[(int64_t)ci * d + (k < d ? k : d - 1)];
    xi[k] = k < d ? v : T(0);
  }
  const T a_i = al[ci];
  double sum[DC];
#pragma unroll
  for (int k = 0; k < DC; ++k) sum[k] = 0.0;

#pragma unroll 1
  for (int j0 = 0; j0 < n; j0 += IG_JC) {
    const int jb = j0 / NB;
    __syncthreads();                                 // the table is staged; the previous chunk is consumed
    // P of the chunk: element (i, j) from Kinv[min][max] of the clamped indices, read along the stored direction
    if (jb < ib) {                                   // tile (jb, ib): rows j, contiguous in i
#pragma unroll
      for (int s = 0; s < IG_JC / 2; ++s) {
        const int jl = half + 2 * s;
        const int cj = j0 + jl < n ? j0 + jl : n - 1;     // (cj < ci: jb < ib and ci lies in block ib, or cj <= n - 1 = ci)
        const int lo = cj < ci ? cj : ci, hi = cj < ci ? ci : cj;
        sP[jl * (NB + 1) + il] = P[(int64_t)lo * ldk + hi];
      }
    } else {                                         // tile (ib, jb): rows i, contiguous in j; the diagonal block from either side
      const int jl = tid & (IG_JC - 1);
      const int cj = j0 + jl < n ? j0 + jl : n - 1;
#pragma unroll
      for (int s = 0; s < NB / (NTHREADS / IG_JC); ++s) {
        const int r = (tid / IG_JC) + (NTHREADS / IG_JC) * s;
        const int gr = ib * NB + r, cr = gr < n ? gr : n - 1;
        const int lo = cj < cr ? cj : cr, hi = cj < cr ? cr : cj;
        sP[jl * (NB + 1) + r] = P[(int64_t)lo * ldk + hi];
      }
    }
    for (int e = tid; e < IG_JC * DC; e += NTHREADS) {
      const int jl = e / DC, k = e % DC;
      const int cj = j0 + jl < n ? j0 + jl : n - 1;
      const T v = X[(int64_t)cj * d + (k < d ? k : d - 1)];
      sX[e] = k < d ? v : T(0);
    }
    if (tid < IG_JC) sA[tid] = al[j0 + tid < n ? j0 + tid : n - 1];
    __syncthreads();
#pragma unroll 1
    for (int jj = 0; jj < IG_JC / 2; ++jj) {
      const int jl = half * (IG_JC / 2) + jj;        // the same in every lane of a wave: sX, sA and the table are broadcasts
      const int gj = j0 + jl;
      const bool take = gi < n && gj < n && gj != gi;
      const T g = __builtin_fma(a_i, sA[jl], -sP[jl * (NB + 1) + il]);
      const T *xj = sX + jl * DC;
      T gx[DC];
#pragma unroll
      for (int k = 0; k < DC; ++k) gx[k] = T(0);
      dx_pair<T, F, DC>(kind, ncomp, xi, xj, tab, g, os, gx);
#pragma unroll
      for (int k = 0; k < DC; ++k) sum[k] += take ? (double)gx[k] : 0.0;
    }
  }

  // ---- the two halves of every row, in a fixed order
  __syncthreads();
  if (half == 1) {
#pragma unroll
    for (int k = 0; k < DC; ++k) sRed[k * NB + il] = sum[k];
  }
  __syncthreads();
  if (half == 0 && gi < n) {
    double *out = gX + ((int64_t)lat * n + gi) * d;
#pragma unroll
    for (int k = 0; k < DC; ++k)
      if (k < d) out[k] = sum[k] + sRed[k * NB + il];
  }
}

template <typename T>
int input_grad_impl(const CovTable &t, const T *Kinv, int64_t n_pad, int64_t ldk, int64_t strideK, const T *alpha, const T *X, int n, double *gX,
                    int q, void *stream) {
  // the diagonal of these depends on x, which the row sum over j != i does not cover
  if (const char *why = dx_refusal(t)) return fail(__func__, why);
  PLMC_REQUIRE_TABLE(t);
  const int kind = t.kind, d = t.d, ncomp = t.ncomp;
  const T *ell = (const T *)t.ell, *oscale = (const T *)t.oscale, *second = (const T *)t.second, *third = (const T *)t.third;
  PLMC_REQUIRE((t.family != COV_PLAIN && t.family != COV_ADD) || (kind >= 0 && kind <= K_MATERN52), "unknown kernel kind");
  PLMC_REQUIRE(Kinv && alpha && X && ell && gX, "null pointer");
  PLMC_REQUIRE(n_pad > 0 && n_pad % NB == 0 && n > 0 && n <= n_pad && n > n_pad - NB, "n_pad must be plmc_pad(n)");
  PLMC_REQUIRE(ldk >= n_pad && (q == 1 || strideK >= n_pad * ldk), "Kinv: ldk >= n_pad, strideK >= n_pad * ldk");
  PLMC_REQUIRE(d > 0 && d <= MAX_DIM && q > 0 && q <= 65535, "need 0<d<=plmc_max_dim(), 0<q<=65535");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(n_pad / NB), (unsigned)q), block(NTHREADS);
  // every stored element of the live upper triangle is read twice
  ProfScope ps(PK_INPUT_GRAD, st, 0.0, (double)q * n * n * sizeof(T));
#define PLMC_LAUNCH_IG(F, DC) \
  hipLaunchKernelGGL((k_input_grad<T, F, DC>), grid, block, 0, st, kind, ncomp, Kinv, ldk, strideK, alpha, n_pad, X, n, d, ell, second, third, oscale, gX)
  switch (t.family) {
    case COV_PLAIN:
    case COV_ADD:
      if (d <= 4) PLMC_LAUNCH_IG(COV_ADD, 4);
      else if (d <= 8) PLMC_LAUNCH_IG(COV_ADD, 8);
      else if (d <= 16) PLMC_LAUNCH_IG(COV_ADD, 16);
      else PLMC_LAUNCH_IG(COV_ADD, 32);
      break;
    default:
      with_capacity<0>(t.family, d, [&](auto f, auto dc) {
        constexpr CovFamily F = decltype(f)::value;
        if constexpr (F != COV_SUM && F != COV_DOT) PLMC_LAUNCH_IG(F, decltype(dc)::value);
      });
  }
#undef PLMC_LAUNCH_IG
  return launch_status(__func__);
}

}  // namespace plmc

extern "C" {
// the entry points of the families (api_common.hpp, PLMC_FAMILY_ENTRIES)
#define PLMC_INPUT_GRAD_ENTRY(SUF, T, INFIX, LEAD, PARAMS, TABLE)                                                                              \
  int plmc_input_grad##INFIX##_##SUF(PLMC_LEAD_##LEAD const T *Kinv, int64_t n_pad, int64_t ldk, int64_t strideK, const T *alpha, const T *X,  \
                                     int n, int d, PLMC_UNPACK PARAMS, double *gX, int q, void *stream) {                                      \
    return plmc::input_grad_impl<T>(TABLE, Kinv, n_pad, ldk, strideK, alpha, X, n, gX, q, stream);                                             \
  }
PLMC_FAMILY_ENTRIES(PLMC_INPUT_GRAD_ENTRY, f32, float)
PLMC_FAMILY_ENTRIES(PLMC_INPUT_GRAD_ENTRY, f64, double)
#undef PLMC_INPUT_GRAD_ENTRY
}
