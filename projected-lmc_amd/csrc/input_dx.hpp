// input_dx.hpp -- what the kernels that differentiate a covariance with respect to an input row share (input_grad.hip: d logp / dX of the
// training inputs; posterior_dx.hip: d mean / dx*, d var / dx* of the test inputs): the latent's table staged in LDS, padded so that a
// slot beyond d adds exactly 0, and the derivative of one pair through the family's *_dx of covariance.hpp.
#pragma once
#include "api_common.hpp"
#include "covariance.hpp"

namespace plmc {

constexpr int IG_TAB = 2 * SM_MAX_MIX * SM_MAX_DIM + SM_MAX_MIX;   // the largest table of one latent: the mixture's
static_assert(IG_TAB >= MAX_COMP * MAX_DIM + MAX_COMP && IG_TAB >= 4 * LPER_MAX_DIM && IG_TAB >= RQ_MAX_DIM + 2, "input-derivative table");

// F: COV_ADD serves the plain kernel too (one component; ell (q, d) is ell (q, 1, d)).  `second`, `third`: the family's rows (CovTable).
// Every thread of the workgroup calls it; the caller's barrier publishes the table.
template <typename T, CovFamily F, int DC>
__device__ __forceinline__ void dx_stage_table(T *tab, int tid, int lat, int d, int ncomp, const T *__restrict__ ell,
                                               const T *__restrict__ second, const T *__restrict__ third, const T *__restrict__ oscale) {
  if constexpr (F == COV_ADD) {                      // [MAX_COMP][DC] 1 / ell | [MAX_COMP] os
    for (int e = tid; e < MAX_COMP * DC; e += NTHREADS) {
      const int g = e / DC, k = e % DC;
      const bool used = g < ncomp && k < d;
      const T v = ell[((int64_t)lat * ncomp + (g < ncomp ? g : 0)) * d + (k < d ? k : 0)];
      tab[e] = used ? T(1) / v : T(0);
    }
    if (tid < MAX_COMP) {
      const T v = oscale ? oscale[(int64_t)lat * ncomp + (tid < ncomp ? tid : 0)] : T(1);
      tab[MAX_COMP * DC + tid] = tid < ncomp ? v : T(0);
    }
  } else if constexpr (F == COV_SM) {                // [M][DC] scales | [M][DC] means | [M] weights
    for (int e = tid; e < SM_MAX_MIX * DC; e += NTHREADS) {
      const int g = e / DC, k = e % DC;
      const bool used = g < ncomp && k < d;
      const int64_t o = ((int64_t)lat * ncomp + (g < ncomp ? g : 0)) * d + (k < d ? k : 0);
      const T s = ell[o], m = second[o];
      tab[e] = used ? s : T(0);
      tab[SM_MAX_MIX * DC + e] = used ? m : T(0);
    }
    if (tid < SM_MAX_MIX) {
      const T v = oscale ? oscale[(int64_t)lat * ncomp + (tid < ncomp ? tid : 0)] : T(1);
      tab[2 * SM_MAX_MIX * DC + tid] = tid < ncomp ? v : T(0);
    }
  } else if constexpr (F == COV_PER || F == COV_LPER) {   // [DC] 1 / p | its residual | 1 / ell | 1 / lam
    if (tid < DC) {
      const int64_t o = (int64_t)lat * d + (tid < d ? tid : 0);
      T ip, ipr;
      per_inv_period(second[o], ip, ipr);
      const T w = T(1) / ell[o];
      tab[tid] = tid < d ? ip : T(0);
      tab[DC + tid] = tid < d ? ipr : T(0);
      tab[2 * DC + tid] = tid < d ? w : T(0);
      if constexpr (F == COV_LPER) {
        const T v = T(1) / third[o];
        tab[3 * DC + tid] = tid < d ? v : T(0);
      }
    }
  } else if constexpr (F == COV_RQ) {                // [DC] 1 / ell | alpha | 1 / (2 alpha)
    if (tid < DC) {
      const T w = T(1) / ell[(int64_t)lat * d + (tid < d ? tid : 0)];
      tab[tid] = tid < d ? w : T(0);
    }
    if (tid == 0) {
      const T a = second[lat];
      tab[DC] = a;
      tab[DC + 1] = T(1) / (T(2) * a);
    }
  }
}

// the output scale of the families that carry one per latent beside the table (the others keep theirs in the table)
template <typename T, CovFamily F> __device__ __forceinline__ T dx_oscale(const T *__restrict__ oscale, int lat) {
  if constexpr (F == COV_PER || F == COV_LPER || F == COV_RQ) return oscale ? oscale[lat] : T(1);
  return T(1);
}

// gx[k] += g os d k(a, b) / d a_k, k < DC, from the staged table: a in registers, b a row of DC raw coordinates (0 beyond d)
template <typename T, CovFamily F, int DC>
__device__ __forceinline__ void dx_pair(int kind, int ncomp, const T (&a)[DC], const T *b, const T *tab, T g, T os, T (&gx)[DC]) {
  if constexpr (F == COV_ADD) {
#pragma unroll 1
    for (int c = 0; c < ncomp; ++c) kern_dx<T, DC>(kind, a, b, tab + c * DC, g, tab[MAX_COMP * DC + c], gx);
  } else if constexpr (F == COV_SM) {
    sm_dx<T, DC>(a, b, tab, tab + SM_MAX_MIX * DC, tab + 2 * SM_MAX_MIX * DC, ncomp, g, gx);
  } else if constexpr (F == COV_PER) {
    per_dx<T, DC>(a, b, tab, tab + DC, tab + 2 * DC, g, os, gx);
  } else if constexpr (F == COV_LPER) {
    lper_dx<T, DC>(a, b, tab, tab + DC, tab + 2 * DC, tab + 3 * DC, g, os, gx);
  } else if constexpr (F == COV_RQ) {
    rq_dx<T, DC>(a, b, tab, tab[DC], tab[DC + 1], g, os, gx);
  }
}

// The families these kernels refuse, by name: their diagonal k(x, x) depends on x, which a sum over pairs of distinct points does not cover
// (null: served).
inline const char *dx_refusal(const CovTable &t) {
  if (t.family == COV_SUM) return "a heterogeneous sum (_sum) has no input gradient yet";
  if (t.family == COV_DOT) return "the dot-product family (_dot: linear, polynomial) has no input gradient yet: its diagonal depends on x";
  if ((t.family == COV_PLAIN || t.family == COV_ADD) && t.kind == K_SPLINE)
    return "the spline kernel has no input gradient yet: its diagonal depends on x";
  return nullptr;
}

}  // namespace plmc
