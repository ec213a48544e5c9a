// cov_tables.hpp -- the covariance tables of the families as the kernels see them: what a table stages in LDS for one latent, the value of
// one pair from it (value(): one training row against one test point; the *PairValue functors: one row against two columns of a tile) and
// the tile walk the assembly kernels share.  assemble.hip (Khat, cross-covariances) and cross_matvec.hip (K(X*, X) V without K*) include
// it, so both evaluate a pair with the same code.
#pragma once
#include "api_common.hpp"
#include "covariance.hpp"

namespace plmc {

// ---- the noise on the diagonal as the tile walks take it (NZ): the latent's scalar `T` -- the code of the entry points without a per-point
// vector, as it was -- or PointNoise, the scalar and the latent's per-point vector (plmc_assemble*_pn_*): A_ii = (a_ii + nz) + pn[i], a_ii
// in the rounding of the scalar form.  The vector is read in diagonal tiles only (a workgroup-uniform condition), once per row: an
// unconditional load at the index clamped into the vector, and the element-wise select the scalar form already has -- no predicated load.
template <typename T> struct PointNoise { T nz; const T *pn; };
template <typename T> struct RowNoise { T nz, pv; };
template <typename T> __device__ __forceinline__ T row_noise(T nz, int, int, bool) { return nz; }
template <typename T> __device__ __forceinline__ RowNoise<T> row_noise(const PointNoise<T> &z, int gi, int n, bool diag_tile) {
  RowNoise<T> r{z.nz, T(0)};
  if (diag_tile) r.pv = z.pn[gi < n ? gi : n - 1];
  return r;
}
// what a kernel hands to its tile walk for latent `lat`
template <typename T, bool PN>
__device__ __forceinline__ auto diag_noise_of(const T *noise, const T *pnoise, int64_t stride_pn, int lat) {
  if constexpr (PN) return PointNoise<T>{noise[lat], pnoise + (int64_t)lat * stride_pn};
  else return noise[lat];
}
template <typename T> __device__ __forceinline__ T add_noise(T v, T nz) { return v + nz; }
template <typename T> __device__ __forceinline__ T add_noise(T v, const RowNoise<T> &z) { return (v + z.nz) + z.pv; }

// ---- additive kernels: K = sum_{g < G} os_g k(|(x - x') / ell_g|) + noise I, G <= MAX_COMP components of one stationary kind, each with
// its own d lengthscales; ell_g[k] = +inf (1 / ell = 0) takes dimension k out of component g.  The inputs are staged RAW, once: the
// differences x - x' are formed once per element and scaled per component (one rounding each), so a component costs d multiplies,
// d multiply-adds and one kernel profile.  Same tiling, padding and row-range interface as the kernels above.
// The tile walk is shared by every kernel that is a table of components (additive, spectral mixture): `value(xr, xc)` is the noise-free
// covariance of one row against a pair of columns, from their raw coordinates.
template <typename T, int DCAP, class F, class NZ>
__device__ __forceinline__ void assemble_tile_table(const T *xi, const T *xj, int ldu, const F value, NZ nz, T *Al, int64_t lda,
                                                    int ib, int jb, int n, bool edge) {
  typedef Pair<T> T2;
  const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
  const int c0 = tx * 4;
  T2 x2[2][DCAP];                                         // [pair][k]
#pragma unroll
  for (int pp = 0; pp < 2; ++pp)
#pragma unroll
    for (int k = 0; k < DCAP; ++k) x2[pp][k] = T2{xj[(c0 + 2 * pp) * ldu + k], xj[(c0 + 2 * pp + 1) * ldu + k]};
#pragma unroll 1
  for (int rr = 0; rr < 16; ++rr) {
    const int r = ty + 8 * rr;
    const int gi = ib * NB + r;
    T xr[DCAP];
#pragma unroll
    for (int k = 0; k < DCAP; ++k) xr[k] = xi[r * ldu + k];
    T2 v[2];
#pragma unroll
    for (int pp = 0; pp < 2; ++pp) v[pp] = value(xr, x2[pp]);
    T o[4] = {v[0].x, v[0].y, v[1].x, v[1].y};
    if (edge) {
      const auto rn = row_noise<T>(nz, gi, n, ib == jb);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int gj = jb * NB + c0 + c;
        if (gi < n && gj < n) { if (gi == gj) o[c] = add_noise<T>(o[c], rn); }
        else o[c] = (gi == gj) ? T(1) : T(0);             // identity padding keeps the padded factor trivial
      }
    }
    T *dst = Al + (int64_t)gi * lda + jb * NB + c0;
    using vec_t = typename Traits<T>::vec_t;
    constexpr int EPV = Traits<T>::EPV;
#pragma unroll
    for (int c = 0; c < 4; c += EPV) {
      vec_t o4;
#pragma unroll
      for (int e = 0; e < EPV; ++e) o4[e] = o[c + e];
      *reinterpret_cast<vec_t *>(dst + c) = o4;
    }
  }
}

// The additive table: per latent ell (G, d), oscale (G) | null.  In LDS: w = 1 / ell [G][DCAP] (0 beyond d), os [G].
template <typename T, int DCAP, int KIND> struct AddPairValue {
  const T *w, *osl;
  int G;
  __device__ __forceinline__ Pair<T> operator()(const T (&xr)[DCAP], const Pair<T> (&xc)[DCAP]) const {
    typedef Pair<T> T2;
    T2 df[DCAP];
#pragma unroll
    for (int k = 0; k < DCAP; ++k) df[k] = xr[k] - xc[k];
    T2 sum = {T(0), T(0)};
#pragma unroll 1
    for (int g = 0; g < G; ++g) {
      T2 r2 = {T(0), T(0)};
#pragma unroll
      for (int k = 0; k < DCAP; ++k) {
        const T2 sd = df[k] * w[g * DCAP + k];
        r2 += sd * sd;
      }
      sum += osl[g] * kern_value_pair<T>(KIND, r2);
    }
    return sum;
  }
};
template <typename T, int DCAP> struct AddTable {
  static constexpr int LDS = MAX_COMP * DCAP + MAX_COMP;
  int kind, G;
  const T *ell, *oscale;
  __device__ __forceinline__ void stage(int lat, int d, T *par) const {
    const int tid = threadIdx.x;
    if (tid < G * DCAP) {
      const int g = tid / DCAP, k = tid % DCAP;
      par[tid] = k < d ? T(1) / ell[((int64_t)lat * G + g) * d + k] : T(0);
    }
    if (tid < G) par[MAX_COMP * DCAP + tid] = oscale ? oscale[(int64_t)lat * G + tid] : T(1);
  }
  template <class NZ>
  __device__ __forceinline__ void tile(const T *xi, const T *xj, int ldu, const T *par, NZ nz, T *Al, int64_t lda, int ib, int jb, int n,
                                       bool edge) const {
    const T *w = par, *osl = par + MAX_COMP * DCAP;
    if (kind == K_RBF) assemble_tile_table<T, DCAP>(xi, xj, ldu, AddPairValue<T, DCAP, K_RBF>{w, osl, G}, nz, Al, lda, ib, jb, n, edge);
    else if (kind == K_MATERN12) assemble_tile_table<T, DCAP>(xi, xj, ldu, AddPairValue<T, DCAP, K_MATERN12>{w, osl, G}, nz, Al, lda, ib, jb, n, edge);
    else if (kind == K_MATERN32) assemble_tile_table<T, DCAP>(xi, xj, ldu, AddPairValue<T, DCAP, K_MATERN32>{w, osl, G}, nz, Al, lda, ib, jb, n, edge);
    else assemble_tile_table<T, DCAP>(xi, xj, ldu, AddPairValue<T, DCAP, K_MATERN52>{w, osl, G}, nz, Al, lda, ib, jb, n, edge);
  }
  // one value of the cross kernel: xa a row of raw coordinates in LDS, xs the thread's test point
  __device__ __forceinline__ T value(const T *xa, const T (&xs)[DCAP], const T *par) const {
    const T *w = par, *osl = par + MAX_COMP * DCAP;
    T df[DCAP];
#pragma unroll
    for (int k = 0; k < DCAP; ++k) df[k] = xa[k] - xs[k];
    T val = T(0);
#pragma unroll 1
    for (int g = 0; g < G; ++g) {
      T r2 = T(0);
#pragma unroll
      for (int k = 0; k < DCAP; ++k) {
        const T sd = df[k] * w[g * DCAP + k];
        r2 += sd * sd;
      }
      val += osl[g] * kern_value<T>(kind, r2);
    }
    return val;
  }
};

// The spectral-mixture table (covariance.hpp): per latent scales, means (M, d), weights (M) | null.  In LDS: sc, mu [M][DCAP] (0 beyond
// d: that factor is exactly 1), wt [M].
template <typename T, int DCAP> struct SmPairValue {
  const T *sc, *mu, *wt;
  int M;
  __device__ __forceinline__ Pair<T> operator()(const T (&xr)[DCAP], const Pair<T> (&xc)[DCAP]) const {
    T b0[DCAP], b1[DCAP];
#pragma unroll
    for (int k = 0; k < DCAP; ++k) { b0[k] = xc[k].x; b1[k] = xc[k].y; }
    return Pair<T>{sm_value<T, DCAP>(xr, b0, sc, mu, wt, M), sm_value<T, DCAP>(xr, b1, sc, mu, wt, M)};
  }
};
template <typename T, int DCAP> struct SmTable {
  static constexpr int LDS = SM_MAX_MIX * (2 * DCAP + 1);
  int M;
  const T *scales, *means, *weights;
  __device__ __forceinline__ void stage(int lat, int d, T *par) const {
    const int tid = threadIdx.x;
    if (tid < M * DCAP) {
      const int g = tid / DCAP, k = tid % DCAP;
      par[tid] = k < d ? scales[((int64_t)lat * M + g) * d + k] : T(0);
      par[SM_MAX_MIX * DCAP + tid] = k < d ? means[((int64_t)lat * M + g) * d + k] : T(0);
    }
    if (tid < M) par[2 * SM_MAX_MIX * DCAP + tid] = weights ? weights[(int64_t)lat * M + tid] : T(1);
  }
  template <class NZ>
  __device__ __forceinline__ void tile(const T *xi, const T *xj, int ldu, const T *par, NZ nz, T *Al, int64_t lda, int ib, int jb, int n,
                                       bool edge) const {
    assemble_tile_table<T, DCAP>(xi, xj, ldu, SmPairValue<T, DCAP>{par, par + SM_MAX_MIX * DCAP, par + 2 * SM_MAX_MIX * DCAP, M}, nz, Al, lda,
                                 ib, jb, n, edge);
  }
  __device__ __forceinline__ T value(const T *xa, const T (&xs)[DCAP], const T *par) const {
    T a[DCAP];
#pragma unroll
    for (int k = 0; k < DCAP; ++k) a[k] = xa[k];
    return sm_value<T, DCAP>(a, xs, par, par + SM_MAX_MIX * DCAP, par + 2 * SM_MAX_MIX * DCAP, M);
  }
};

// The periodic table (covariance.hpp): per latent lengthscales, periods (d), output scale | null.  In LDS: ip = 1 / p, its residual ipr,
// w = 1 / ell [DCAP] each (0 beyond d: that dimension adds exactly 0 to the exponent), os.
template <typename T, int DCAP> struct PerPairValue {
  const T *ip, *ipr, *w;
  T os;
  __device__ __forceinline__ Pair<T> operator()(const T (&xr)[DCAP], const Pair<T> (&xc)[DCAP]) const {
    T b0[DCAP], b1[DCAP];
#pragma unroll
    for (int k = 0; k < DCAP; ++k) { b0[k] = xc[k].x; b1[k] = xc[k].y; }
    return Pair<T>{os * per_value<T, DCAP>(xr, b0, ip, ipr, w), os * per_value<T, DCAP>(xr, b1, ip, ipr, w)};
  }
};
template <typename T, int DCAP> struct PerTable {
  static constexpr int LDS = 3 * DCAP + 1;
  const T *ell, *period, *oscale;
  __device__ __forceinline__ void stage(int lat, int d, T *par) const {
    const int tid = threadIdx.x;
    if (tid < DCAP) {
      T ip = T(0), ipr = T(0);
      if (tid < d) per_inv_period(period[(int64_t)lat * d + tid], ip, ipr);
      par[tid] = ip;
      par[DCAP + tid] = ipr;
      par[2 * DCAP + tid] = tid < d ? T(1) / ell[(int64_t)lat * d + tid] : T(0);
    }
    if (tid == 0) par[3 * DCAP] = oscale ? oscale[lat] : T(1);
  }
  template <class NZ>
  __device__ __forceinline__ void tile(const T *xi, const T *xj, int ldu, const T *par, NZ nz, T *Al, int64_t lda, int ib, int jb, int n,
                                       bool edge) const {
    assemble_tile_table<T, DCAP>(xi, xj, ldu, PerPairValue<T, DCAP>{par, par + DCAP, par + 2 * DCAP, par[3 * DCAP]}, nz, Al, lda, ib, jb, n,
                                 edge);
  }
  __device__ __forceinline__ T value(const T *xa, const T (&xs)[DCAP], const T *par) const {
    T a[DCAP];
#pragma unroll
    for (int k = 0; k < DCAP; ++k) a[k] = xa[k];
    return par[3 * DCAP] * per_value<T, DCAP>(a, xs, par, par + DCAP, par + 2 * DCAP);
  }
};

// The rational-quadratic table (covariance.hpp): per latent lengthscales (d), alpha, output scale | null.  In LDS: w = 1 / ell [DCAP]
// (0 beyond d: that dimension adds exactly 0 to r^2), alpha, 1 / (2 alpha), os.
template <typename T, int DCAP> struct RqPairValue {
  const T *w;
  T alpha, i2a, os;
  __device__ __forceinline__ Pair<T> operator()(const T (&xr)[DCAP], const Pair<T> (&xc)[DCAP]) const {
    typedef Pair<T> T2;
    T2 r2 = {T(0), T(0)};
#pragma unroll
    for (int k = 0; k < DCAP; ++k) {
      const T2 sd = (xr[k] - xc[k]) * w[k];
      r2 += sd * sd;
    }
    return os * T2{rq_profile(r2.x, alpha, i2a), rq_profile(r2.y, alpha, i2a)};
  }
};
template <typename T, int DCAP> struct RqTable {
  static constexpr int LDS = DCAP + 3;
  const T *ell, *alpha, *oscale;
  __device__ __forceinline__ void stage(int lat, int d, T *par) const {
    const int tid = threadIdx.x;
    if (tid < DCAP) par[tid] = tid < d ? T(1) / ell[(int64_t)lat * d + tid] : T(0);
    if (tid == 0) {
      const T a = alpha[lat];
      par[DCAP] = a;
      par[DCAP + 1] = T(0.5) / a;
      par[DCAP + 2] = oscale ? oscale[lat] : T(1);
    }
  }
  template <class NZ>
  __device__ __forceinline__ void tile(const T *xi, const T *xj, int ldu, const T *par, NZ nz, T *Al, int64_t lda, int ib, int jb, int n,
                                       bool edge) const {
    assemble_tile_table<T, DCAP>(xi, xj, ldu, RqPairValue<T, DCAP>{par, par[DCAP], par[DCAP + 1], par[DCAP + 2]}, nz, Al, lda, ib, jb, n, edge);
  }
  __device__ __forceinline__ T value(const T *xa, const T (&xs)[DCAP], const T *par) const {
    T a[DCAP];
#pragma unroll
    for (int k = 0; k < DCAP; ++k) a[k] = xa[k];
    return par[DCAP + 2] * rq_value<T, DCAP>(a, xs, par, par[DCAP], par[DCAP + 1]);
  }
};

// The dot-product table (covariance.hpp): per latent variances v (d), offset c, output scale | null; the power P is the same for every
// latent.  In LDS: v [DCAP] (0 beyond d: that dimension adds exactly 0 to s), c, os.  The diagonal is a value like any other
// (k(x, x) = os (c + sum_k v_k x_k^2)^P); the tile walk adds the noise to it and writes the identity padding.
template <typename T, int DCAP> struct DotPairValue {
  const T *v;
  T c, os;
  int P;
  __device__ __forceinline__ Pair<T> operator()(const T (&xr)[DCAP], const Pair<T> (&xc)[DCAP]) const {
    T ta[DCAP], b0[DCAP], b1[DCAP];
#pragma unroll
    for (int k = 0; k < DCAP; ++k) { ta[k] = v[k] * xr[k]; b0[k] = xc[k].x; b1[k] = xc[k].y; }
    return Pair<T>{os * dot_value<T, DCAP>(ta, b0, c, P), os * dot_value<T, DCAP>(ta, b1, c, P)};
  }
};
template <typename T, int DCAP> struct DotTable {
  static constexpr int LDS = DCAP + 2;
  int P;
  const T *var, *offset, *oscale;
  __device__ __forceinline__ void stage(int lat, int d, T *par) const {
    const int tid = threadIdx.x;
    if (tid < DCAP) par[tid] = tid < d ? var[(int64_t)lat * d + tid] : T(0);
    if (tid == 0) {
      par[DCAP] = offset[lat];
      par[DCAP + 1] = oscale ? oscale[lat] : T(1);
    }
  }
  template <class NZ>
  __device__ __forceinline__ void tile(const T *xi, const T *xj, int ldu, const T *par, NZ nz, T *Al, int64_t lda, int ib, int jb, int n,
                                       bool edge) const {
    assemble_tile_table<T, DCAP>(xi, xj, ldu, DotPairValue<T, DCAP>{par, par[DCAP], par[DCAP + 1], P}, nz, Al, lda, ib, jb, n, edge);
  }
  // the training row is the scaled side, as the tile's row is
  __device__ __forceinline__ T value(const T *xa, const T (&xs)[DCAP], const T *par) const {
    T ta[DCAP];
#pragma unroll
    for (int k = 0; k < DCAP; ++k) ta[k] = par[k] * xa[k];
    return par[DCAP + 1] * dot_value<T, DCAP>(ta, xs, par[DCAP], P);
  }
};

// The locally periodic table (covariance.hpp): per latent periodic lengthscales, periods, RBF lengthscales (d each), output scale | null.
// In LDS: ip = 1 / p, its residual ipr, w = 1 / ell, v = 1 / lam [DCAP] each (0 beyond d: that dimension adds exactly 0 to both
// exponents), os.
template <typename T, int DCAP> struct LperPairValue {
  const T *ip, *ipr, *w, *v;
  T os;
  __device__ __forceinline__ Pair<T> operator()(const T (&xr)[DCAP], const Pair<T> (&xc)[DCAP]) const {
    T b0[DCAP], b1[DCAP];
#pragma unroll
    for (int k = 0; k < DCAP; ++k) { b0[k] = xc[k].x; b1[k] = xc[k].y; }
    return Pair<T>{os * lper_value<T, DCAP>(xr, b0, ip, ipr, w, v), os * lper_value<T, DCAP>(xr, b1, ip, ipr, w, v)};
  }
};
template <typename T, int DCAP> struct LperTable {
  static constexpr int LDS = 4 * DCAP + 1;
  const T *ell, *period, *rbf_ell, *oscale;
  __device__ __forceinline__ void stage(int lat, int d, T *par) const {
    const int tid = threadIdx.x;
    if (tid < DCAP) {
      T ip = T(0), ipr = T(0);
      if (tid < d) per_inv_period(period[(int64_t)lat * d + tid], ip, ipr);
      par[tid] = ip;
      par[DCAP + tid] = ipr;
      par[2 * DCAP + tid] = tid < d ? T(1) / ell[(int64_t)lat * d + tid] : T(0);
      par[3 * DCAP + tid] = tid < d ? T(1) / rbf_ell[(int64_t)lat * d + tid] : T(0);
    }
    if (tid == 0) par[4 * DCAP] = oscale ? oscale[lat] : T(1);
  }
  template <class NZ>
  __device__ __forceinline__ void tile(const T *xi, const T *xj, int ldu, const T *par, NZ nz, T *Al, int64_t lda, int ib, int jb, int n,
                                       bool edge) const {
    assemble_tile_table<T, DCAP>(xi, xj, ldu, LperPairValue<T, DCAP>{par, par + DCAP, par + 2 * DCAP, par + 3 * DCAP, par[4 * DCAP]}, nz, Al,
                                 lda, ib, jb, n, edge);
  }
  __device__ __forceinline__ T value(const T *xa, const T (&xs)[DCAP], const T *par) const {
    T a[DCAP];
#pragma unroll
    for (int k = 0; k < DCAP; ++k) a[k] = xa[k];
    return par[4 * DCAP] * lper_value<T, DCAP>(a, xs, par, par + DCAP, par + 2 * DCAP, par + 3 * DCAP);
  }
};

// The heterogeneous sum (CovTable SUM): per latent and component one record [ell | period | rbf_ell: d each | alpha] and an output scale |
// null; `fams` holds the members' 4-bit codes.  A member reads only the slots it owns (ARD kinds: ell; rational quadratic: ell, alpha;
// periodic: ell, period; locally periodic: ell, period, rbf_ell), the others may hold anything.  In LDS, per component (stride REC):
// ip = 1 / p, its residual ipr, w = 1 / ell, v = 1 / rbf_ell [DCAP] each (0 where not owned and beyond d), alpha, 1 / (2 alpha), os.
// Every component's value comes from its own family's function (kern_value*, rq_profile, per_value, lper_value); the components are added
// in table order.
template <typename T, int DCAP> struct SumPairValue {
  static constexpr int REC = 4 * DCAP + 3;
  const T *par;
  int fams, G;
  __device__ __forceinline__ Pair<T> operator()(const T (&xr)[DCAP], const Pair<T> (&xc)[DCAP]) const {
    typedef Pair<T> T2;
    T2 sum = {T(0), T(0)};
#pragma unroll 1
    for (int g = 0; g < G; ++g) {
      const int f = (fams >> (4 * g)) & 15;
      const T *pg = par + g * REC;
      const T os = pg[4 * DCAP + 2];
      if (f == F_PER || f == F_LPER) {
        T b0[DCAP], b1[DCAP];
#pragma unroll
        for (int k = 0; k < DCAP; ++k) { b0[k] = xc[k].x; b1[k] = xc[k].y; }
        if (f == F_PER) sum += os * T2{per_value<T, DCAP>(xr, b0, pg, pg + DCAP, pg + 2 * DCAP), per_value<T, DCAP>(xr, b1, pg, pg + DCAP, pg + 2 * DCAP)};
        else sum += os * T2{lper_value<T, DCAP>(xr, b0, pg, pg + DCAP, pg + 2 * DCAP, pg + 3 * DCAP),
                            lper_value<T, DCAP>(xr, b1, pg, pg + DCAP, pg + 2 * DCAP, pg + 3 * DCAP)};
      } else {
        T2 r2 = {T(0), T(0)};
#pragma unroll
        for (int k = 0; k < DCAP; ++k) {
          const T2 sd = (xr[k] - xc[k]) * pg[2 * DCAP + k];
          r2 += sd * sd;
        }
        if (f == F_RQ) sum += os * T2{rq_profile(r2.x, pg[4 * DCAP], pg[4 * DCAP + 1]), rq_profile(r2.y, pg[4 * DCAP], pg[4 * DCAP + 1])};
        else sum += os * kern_value_pair<T>(f, r2);
      }
    }
    return sum;
  }
};
template <typename T, int DCAP> struct SumTable {
  static constexpr int REC = 4 * DCAP + 3;
  static constexpr int LDS = MAX_COMP * REC;
  int fams, G;
  const T *table, *oscale;
  __device__ __forceinline__ void stage(int lat, int d, T *par) const {
    const int tid = threadIdx.x;
    if (tid < G * DCAP) {
      const int g = tid / DCAP, k = tid % DCAP;
      const int f = (fams >> (4 * g)) & 15;
      const T *rec = table + ((int64_t)lat * G + g) * (3 * d + 1);
      T ip = T(0), ipr = T(0);
      if (k < d && (f == F_PER || f == F_LPER)) per_inv_period(rec[d + k], ip, ipr);
      T *pg = par + g * REC;
      pg[k] = ip;
      pg[DCAP + k] = ipr;
      pg[2 * DCAP + k] = k < d ? T(1) / rec[k] : T(0);
      pg[3 * DCAP + k] = (k < d && f == F_LPER) ? T(1) / rec[2 * d + k] : T(0);
      if (k == 0) {
        const T a = f == F_RQ ? rec[3 * d] : T(1);
        pg[4 * DCAP] = a;
        pg[4 * DCAP + 1] = T(0.5) / a;
        pg[4 * DCAP + 2] = oscale ? oscale[(int64_t)lat * G + g] : T(1);
      }
    }
  }
  template <class NZ>
  __device__ __forceinline__ void tile(const T *xi, const T *xj, int ldu, const T *par, NZ nz, T *Al, int64_t lda, int ib, int jb, int n,
                                       bool edge) const {
    assemble_tile_table<T, DCAP>(xi, xj, ldu, SumPairValue<T, DCAP>{par, fams, G}, nz, Al, lda, ib, jb, n, edge);
  }
  __device__ __forceinline__ T value(const T *xa, const T (&xs)[DCAP], const T *par) const {
    T a[DCAP];
#pragma unroll
    for (int k = 0; k < DCAP; ++k) a[k] = xa[k];
    T val = T(0);
#pragma unroll 1
    for (int g = 0; g < G; ++g) {
      const int f = (fams >> (4 * g)) & 15;
      const T *pg = par + g * REC;
      T v;
      if (f == F_PER) v = per_value<T, DCAP>(a, xs, pg, pg + DCAP, pg + 2 * DCAP);
      else if (f == F_LPER) v = lper_value<T, DCAP>(a, xs, pg, pg + DCAP, pg + 2 * DCAP, pg + 3 * DCAP);
      else if (f == F_RQ) v = rq_value<T, DCAP>(a, xs, pg + 2 * DCAP, pg[4 * DCAP], pg[4 * DCAP + 1]);
      else {
        T r2 = T(0);
#pragma unroll
        for (int k = 0; k < DCAP; ++k) {
          const T sd = (a[k] - xs[k]) * pg[2 * DCAP + k];
          r2 += sd * sd;
        }
        v = kern_value<T>(f, r2);
      }
      val += pg[4 * DCAP + 2] * v;
    }
    return val;
  }
};

// the device-side table of family F from a descriptor
template <typename T, CovFamily F, int DC>
auto device_table(const CovTable &t) {
  const T *ell = (const T *)t.ell, *second = (const T *)t.second, *oscale = (const T *)t.oscale;
  if constexpr (F == COV_ADD) return AddTable<T, DC>{t.kind, t.ncomp, ell, oscale};
  else if constexpr (F == COV_SM) return SmTable<T, DC>{t.ncomp, ell, second, oscale};
  else if constexpr (F == COV_PER) return PerTable<T, DC>{ell, second, oscale};
  else if constexpr (F == COV_RQ) return RqTable<T, DC>{ell, second, oscale};
  else if constexpr (F == COV_LPER) return LperTable<T, DC>{ell, second, (const T *)t.third, oscale};
  else if constexpr (F == COV_SUM) return SumTable<T, DC>{t.fams, t.ncomp, ell, oscale};
  else if constexpr (F == COV_DOT) return DotTable<T, DC>{t.power(), ell, second, oscale};
}

}  // namespace plmc
