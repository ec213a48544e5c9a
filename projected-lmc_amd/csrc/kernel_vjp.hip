// kernel_vjp.hip -- vector-Jacobian product of a dense (cross-)covariance block with respect to its
// inputs and hyper-parameters:  given G = d loss / d K  with  K_i[a][b] = os_i k(|x1_a - x2_b| / ell_i),
//   gX1[i][a][k]  = sum_b G_i[a][b] dK_i[a][b] / d x1_a[k]
//   gEll[i][a][k] = sum_b G_i[a][b] dK_i[a][b] / d ell_i[k]       (row partials; the caller sums over a)
//   gOs[i][a]     = sum_b G_i[a][b] k(...)                         (row partials)
// Used by the variational path: gradients of K_ZZ and K_ZX with respect to the
// learned inducing locations Z and the lengthscales -- what torch autograd derives through gpytorch's
// kernel evaluation chain in `loss.backward()` (experiments.py:270) for VariationalMultitaskGPModel.
// One wave per row a: lanes stride over b with coalesced reads of G; fixed-order reductions, fp64
// accumulation, no atomics.  HBM-bound: reads G once.
#include "api_common.hpp"
#include "covariance.hpp"
#include "../../include/plmc.h"

namespace plmc {

template <typename T, int DCAP>
__global__ __launch_bounds__(NTHREADS) void k_kernel_vjp(int kind, const T *__restrict__ X1, int n1,
                                                          const T *__restrict__ X2, int n2, int d,
                                                          const T *__restrict__ ell, const T *__restrict__ oscale,
                                                          const T *__restrict__ G, int64_t ldg, int64_t strideG,
                                                          double *__restrict__ gX1, double *__restrict__ gEll,
                                                          double *__restrict__ gOs) {
  const int lat = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int a = blockIdx.x * 4 + wave;
  if (a >= n1) return;
  const T *el = ell + (int64_t)lat * d;
  const T os = oscale ? oscale[lat] : T(1);
  T x1[DCAP], il[DCAP];
#pragma unroll
  for (int k = 0; k < DCAP; ++k) {
    il[k] = k < d ? T(1) / el[k] : T(0);
    x1[k] = k < d ? X1[(int64_t)a * d + k] : T(0);
  }
  double sx[DCAP], sl[DCAP], so = 0.0;
#pragma unroll
  for (int k = 0; k < DCAP; ++k) { sx[k] = 0.0; sl[k] = 0.0; }
  const T *Grow = G + (int64_t)lat * strideG + (int64_t)a * ldg;
  for (int b = lane; b < n2; b += 64) {
    const T g = Grow[b];
    T df[DCAP];
    T r2 = T(0);
    // difference of the raw inputs, then scaled: exactly 0 at coincident points.  (x1 il - x2 il contracts to an fma
    // whose result there is the rounding error of x1 il; the Matern-1/2 factor exp(-r) / r turned it into an O(1) term.)
#pragma unroll
    for (int k = 0; k < DCAP; ++k) {
      df[k] = k < d ? (x1[k] - X2[(int64_t)b * d + k]) * il[k] : T(0);
      r2 += df[k] * df[k];
    }
    T val, base;
    kern_value_base<T>(kind, r2, val, base);
    so += (double)(g * val);
    const T c = g * os * base;
#pragma unroll
    for (int k = 0; k < DCAP; ++k) {
      sl[k] += (double)(c * df[k] * df[k]);           // * 1/ell_k below
      sx[k] -= (double)(c * df[k]);                   // dK/dx1_k = -os base (x1-x2)_k / ell_k^2 = -os base du_k / ell_k
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    so += __shfl_down(so, off, 64);
#pragma unroll
    for (int k = 0; k < DCAP; ++k) {
      sx[k] += __shfl_down(sx[k], off, 64);
      sl[k] += __shfl_down(sl[k], off, 64);
    }
  }
  if (lane == 0) {
    const int64_t o = ((int64_t)lat * n1 + a) * d;
#pragma unroll
    for (int k = 0; k < DCAP; ++k)
      if (k < d) {
        gX1[o + k] = sx[k] * (double)il[k];
        gEll[o + k] = sl[k] * (double)il[k];
      }
    gOs[(int64_t)lat * n1 + a] = so;
  }
}

// Component-table form (an additive kernel, include/plmc.h "Additive kernels"):  K_i[a][b] = sum_g os_ig k(|(x1_a - x2_b) / ell_ig|).
//   gX1[i][a][k]     = sum_b G_i[a][b] sum_g dK_ig[a][b] / d x1_a[k]       (summed over the components)
//   gEll[i][a][g][k] = sum_b G_i[a][b] dK_ig[a][b] / d ell_ig[k]           (row partials per component)
//   gOs[i][a][g]     = sum_b G_i[a][b] k_g(...)                            (row partials per component)
// The plain kernel's structure: one wave per row a, lanes stride over b with coalesced reads of G, fp64 sums in registers, the same
// fixed-order shuffle, no atomics.  x1 - x2 is formed once per element from the raw inputs and scaled per component by 1 / ell_g, which
// is exactly 0 on a slot the component ignores (ell = +inf) and beyond d: that slot's df, its gEll entry and its share of gX1 are
// exactly 0, and nothing is divided by ell.  A component whose own scaled distance is 0 has base = 0 for Matern-1/2 (kern_value_base):
// nothing to gX1 / gEll, its value still to gOs -- also where the points differ in dimensions outside its group.
// The 1 / ell and output-scale table of the latent is staged in LDS (every lane reads the same address: a broadcast).  GC components are
// evaluated per pass over the row of G; d + GC d + GC fp64 sums are live.  ncomp <= GC: G is read once.
template <typename T, int DCAP, int GC>
__global__ __launch_bounds__(NTHREADS) void k_kernel_vjp_add(int kind, const T *__restrict__ X1, int n1, const T *__restrict__ X2,
                                                              int n2, int d, int ncomp, const T *__restrict__ ell,
                                                              const T *__restrict__ oscale, const T *__restrict__ G, int64_t ldg,
                                                              int64_t strideG, double *__restrict__ gX1, double *__restrict__ gEll,
                                                              double *__restrict__ gOs) {
  __shared__ T s_il[MAX_COMP * DCAP];
  __shared__ T s_os[MAX_COMP];
  const int lat = blockIdx.y;
  for (int i = threadIdx.x; i < MAX_COMP * DCAP; i += NTHREADS) {
    const int g = i / DCAP, k = i % DCAP;
    s_il[i] = (g < ncomp && k < d) ? T(1) / ell[((int64_t)lat * ncomp + g) * d + k] : T(0);
  }
  if (threadIdx.x < MAX_COMP)
    s_os[threadIdx.x] = (int)threadIdx.x < ncomp ? (oscale ? oscale[(int64_t)lat * ncomp + threadIdx.x] : T(1)) : T(0);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int a = blockIdx.x * 4 + wave;
  if (a >= n1) return;
  // slots beyond d re-read the last coordinate (an unconditional, in-bounds load); their 1 / ell is 0
  int col[DCAP];
  T x1[DCAP];
#pragma unroll
  for (int k = 0; k < DCAP; ++k) {
    col[k] = k < d ? k : d - 1;
    x1[k] = X1[(int64_t)a * d + col[k]];
  }
  double sx[DCAP];
#pragma unroll
  for (int k = 0; k < DCAP; ++k) sx[k] = 0.0;
  const T *Grow = G + (int64_t)lat * strideG + (int64_t)a * ldg;
  const int64_t orow = (int64_t)lat * n1 + a;
  for (int g0 = 0; g0 < ncomp; g0 += GC) {
    double sl[GC][DCAP], so[GC];
#pragma unroll
    for (int j = 0; j < GC; ++j) {
      so[j] = 0.0;
#pragma unroll
      for (int k = 0; k < DCAP; ++k) sl[j][k] = 0.0;
    }
    for (int b = lane; b < n2; b += 64) {
      const T g = Grow[b];
      const T *x2 = X2 + (int64_t)b * d;
      T diff[DCAP], wx[DCAP];
#pragma unroll
      for (int k = 0; k < DCAP; ++k) {
        diff[k] = x1[k] - x2[col[k]];
        wx[k] = T(0);
      }
#pragma unroll
      for (int j = 0; j < GC; ++j) {
        if (g0 + j < ncomp) {                               // the same in every lane
          const T *il = s_il + (g0 + j) * DCAP;
          T df[DCAP];
          T r2 = T(0);
#pragma unroll
          for (int k = 0; k < DCAP; ++k) {
            df[k] = diff[k] * il[k];
            r2 += df[k] * df[k];
          }
          T val, base;
          kern_value_base<T>(kind, r2, val, base);
          so[j] += (double)(g * val);
          const T c = g * s_os[g0 + j] * base;
#pragma unroll
          for (int k = 0; k < DCAP; ++k) {
            const T t = c * df[k];
            sl[j][k] += (double)(t * df[k]);                // * 1/ell_gk below
            wx[k] += t * il[k];                             // dK_g/dx1_k = -os_g base df_k / ell_gk
          }
        }
      }
#pragma unroll
      for (int k = 0; k < DCAP; ++k) sx[k] -= (double)wx[k];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
      for (int j = 0; j < GC; ++j) {
        so[j] += __shfl_down(so[j], off, 64);
#pragma unroll
        for (int k = 0; k < DCAP; ++k) sl[j][k] += __shfl_down(sl[j][k], off, 64);
      }
    }
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < GC; ++j)
        if (g0 + j < ncomp) {
          const int64_t o = (orow * ncomp + g0 + j) * d;
#pragma unroll
          for (int k = 0; k < DCAP; ++k)
            if (k < d) gEll[o + k] = sl[j][k] * (double)s_il[(g0 + j) * DCAP + k];
          gOs[orow * ncomp + g0 + j] = so[j];
        }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int k = 0; k < DCAP; ++k) sx[k] += __shfl_down(sx[k], off, 64);
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < DCAP; ++k)
      if (k < d) gX1[orow * d + k] = sx[k];
  }
}

template <typename T>
int kernel_vjp_impl(const CovTable &t, const T *X1, int n1, const T *X2, int n2, const T *G, int64_t ldg, int64_t strideG, double *gX1,
                    double *gEll, double *gOs, int q, void *stream) {
  PLMC_REQUIRE_TABLE(t);
  const int kind = t.kind, d = t.d;
  const T *ell = (const T *)t.ell, *oscale = (const T *)t.oscale;
  PLMC_REQUIRE(kind >= 0 && kind <= 3, "unknown kernel kind");
  PLMC_REQUIRE(X1 && X2 && ell && G && gX1 && gEll && gOs, "null pointer");
  PLMC_REQUIRE(n1 > 0 && n2 > 0 && q > 0 && d > 0 && d <= MAX_DIM && ldg >= n2, "bad sizes");
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((n1 + 3) / 4, q), block(NTHREADS);
  ProfScope ps(PK_VJP, st, 0.0, (double)q * n1 * n2 * sizeof(T));
#define PLMC_LAUNCH_VJP(DC)                                                                                         \
  hipLaunchKernelGGL((k_kernel_vjp<T, DC>), grid, block, 0, st, kind, X1, n1, X2, n2, d, ell, oscale, G, ldg, strideG, \
                     gX1, gEll, gOs)
#define PLMC_LAUNCH_VJP_ADD(DC, GC)                                                                                          \
  hipLaunchKernelGGL((k_kernel_vjp_add<T, DC, GC>), grid, block, 0, st, kind, X1, n1, X2, n2, d, t.ncomp, ell, oscale, G, ldg, \
                     strideG, gX1, gEll, gOs)
  // d > 16: the sums of all components do not fit the register file -- fp32 takes two components per pass over G, fp64 one
  constexpr int GC32 = sizeof(T) == 4 ? 2 : 1;
  switch (t.route()) {
    case COV_PLAIN:
      if (d <= 4) PLMC_LAUNCH_VJP(4);
      else if (d <= 8) PLMC_LAUNCH_VJP(8);
      else if (d <= 16) PLMC_LAUNCH_VJP(16);
      else PLMC_LAUNCH_VJP(32);
      break;
    case COV_ADD:
      if (d <= 4) PLMC_LAUNCH_VJP_ADD(4, 4);
      else if (d <= 8) PLMC_LAUNCH_VJP_ADD(8, 4);
      else if (d <= 16) PLMC_LAUNCH_VJP_ADD(16, 4);
      else PLMC_LAUNCH_VJP_ADD(32, GC32);
      break;
    default:
      return fail(__func__, "the kernel VJP takes the plain and the additive family only");
  }
#undef PLMC_LAUNCH_VJP
#undef PLMC_LAUNCH_VJP_ADD
  return launch_status(__func__);
}

}  // namespace plmc

extern "C" {
int plmc_kernel_vjp_f32(int kind, const float *X1, int n1, const float *X2, int n2, int d, const float *ell,
                        const float *oscale, const float *G, int64_t ldg, int64_t strideG, double *gX1, double *gEll,
                        double *gOs, int q, void *stream) {
  return plmc::kernel_vjp_impl<float>(plmc::CovTable::plain(kind, d, ell, oscale), X1, n1, X2, n2, G, ldg, strideG, gX1, gEll, gOs, q, stream);
}
int plmc_kernel_vjp_f64(int kind, const double *X1, int n1, const double *X2, int n2, int d, const double *ell,
                        const double *oscale, const double *G, int64_t ldg, int64_t strideG, double *gX1, double *gEll,
                        double *gOs, int q, void *stream) {
  return plmc::kernel_vjp_impl<double>(plmc::CovTable::plain(kind, d, ell, oscale), X1, n1, X2, n2, G, ldg, strideG, gX1, gEll, gOs, q, stream);
}
int plmc_kernel_vjp_add_f32(int kind, const float *X1, int n1, const float *X2, int n2, int d, int ncomp, const float *ell,
                            const float *oscale, const float *G, int64_t ldg, int64_t strideG, double *gX1, double *gEll,
                            double *gOs, int q, void *stream) {
  return plmc::kernel_vjp_impl<float>(plmc::CovTable::add(kind, d, ncomp, ell, oscale), X1, n1, X2, n2, G, ldg, strideG, gX1, gEll, gOs, q,
                                      stream);
}
int plmc_kernel_vjp_add_f64(int kind, const double *X1, int n1, const double *X2, int n2, int d, int ncomp, const double *ell,
                            const double *oscale, const double *G, int64_t ldg, int64_t strideG, double *gX1, double *gEll,
                            double *gOs, int q, void *stream) {
  return plmc::kernel_vjp_impl<double>(plmc::CovTable::add(kind, d, ncomp, ell, oscale), X1, n1, X2, n2, G, ldg, strideG, gX1, gEll, gOs, q,
                                       stream);
}
}
