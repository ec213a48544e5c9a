// covariance.hpp -- stationary ARD kernel profiles shared by assembly and gradient kernels.
// Restates the kernels handle_covar_ builds (projected_lmc.py:151-167): gpytorch RBFKernel and
// MaternKernel(nu in {1/2,3/2,5/2}) on scaled inputs u = x / ell  [gpytorch-knowledge].
#pragma once
#include <hip/hip_runtime.h>

namespace plmc {

enum { K_RBF = 0, K_MATERN12 = 1, K_MATERN32 = 2, K_MATERN52 = 3, K_SPLINE = 4 };

// One factor of the reference's SplineKernel (projected_lmc.py:26-36): k(x, x') = prod_k [1 + m M + m^2 (M - m / 3) / 2],
// m = min(x_k, x'_k), M = max(x_k, x'_k).  Not a function of the distance and without a lengthscale: the kernels that
// take a `kind` evaluate it from the staged inputs themselves (callers pass ell = 1) instead of through r2.
template <typename T> __device__ __forceinline__ T spline_factor(T a, T b) {
  const T mn = a < b ? a : b, mx = a < b ? b : a;
  return T(1) + mn * mx + T(0.5) * mn * mn * (mx - mn * T(1.0 / 3.0));
}

__device__ __forceinline__ float  dexp(float x) { return expf(x); }
__device__ __forceinline__ double dexp(double x) { return exp(x); }
__device__ __forceinline__ float  dsqrt(float x) { return sqrtf(x); }
__device__ __forceinline__ double dsqrt(double x) { return sqrt(x); }

// k(r2) for unit output scale, r2 = |u - u'|^2.
template <typename T> __device__ __forceinline__ T kern_value(int kind, T r2) {
  if (kind == K_RBF) return dexp(T(-0.5) * r2);
  T r = dsqrt(r2 > T(0) ? r2 : T(0));
  if (kind == K_MATERN12) return dexp(-r);
  if (kind == K_MATERN32) { T s = T(1.7320508075688772) * r; return (T(1) + s) * dexp(-s); }
  T s = T(2.23606797749979) * r;
  return (T(1) + s + T(5.0 / 3.0) * r2) * dexp(-s);
}

// value and "base" such that  d k / d ell_k = base * (u_k - u'_k)^2 / ell_k   (unit output scale).
template <typename T> __device__ __forceinline__ void kern_value_base(int kind, T r2, T &val, T &base) {
  if (kind == K_RBF) { val = dexp(T(-0.5) * r2); base = val; return; }
  T r = dsqrt(r2 > T(0) ? r2 : T(0));
  if (kind == K_MATERN12) {
    val = dexp(-r);
    base = r > T(1e-15) ? val / r : T(0);
    return;
  }
  if (kind == K_MATERN32) {
    T s = T(1.7320508075688772) * r, e = dexp(-s);
    val = (T(1) + s) * e; base = T(3) * e; return;
  }
  T s = T(2.23606797749979) * r, e = dexp(-s);
  val = (T(1) + s + T(5.0 / 3.0) * r2) * e;
  base = T(5.0 / 3.0) * (T(1) + s) * e;
}

// ---- d k / d x (input_grad.hip).  Every family's *_dx adds  g os d k(a, b) / d a_k  to gx[k], k < DCAP, for one pair of raw input
// rows a (registers) and b, with its table rows padded so that a slot beyond d adds exactly 0.  Coincident rows give exactly 0 for
// every family.
// stationary kinds, one component: il = 1 / ell [DCAP] (0 beyond d and on a slot the component ignores, ell = +inf).  The arithmetic
// of k_kernel_vjp_add: the raw difference scaled, kern_value_base (Matern-1/2: base = 0 at r = 0), -g os base df_k / ell_k.
template <typename T, int DCAP>
__device__ __forceinline__ void kern_dx(int kind, const T (&a)[DCAP], const T *b, const T *il, T g, T os, T (&gx)[DCAP]) {
  T df[DCAP];
  T r2 = T(0);
#pragma unroll
  for (int k = 0; k < DCAP; ++k) {
    df[k] = (a[k] - b[k]) * il[k];
    r2 += df[k] * df[k];
  }
  T val, base;
  kern_value_base<T>(kind, r2, val, base);
  const T c = g * os * base;
#pragma unroll
  for (int k = 0; k < DCAP; ++k) gx[k] -= (c * df[k]) * il[k];
}

// Gradient-epilogue variant: for fp32 the transcendental pair is taken from the hardware units
// (v_sqrt_f32 / v_exp_f32, ~1-2 ulp) instead of the ~35-instruction IEEE expansions; the values only
// weight a reduction whose fp32 tolerance is 1e-3, the covariance ASSEMBLY keeps the accurate forms.
__device__ __forceinline__ void kern_value_base_fast(int kind, float r2, float &val, float &base) {
  if (kind == K_RBF) { val = __expf(-0.5f * r2); base = val; return; }
  const float r = __builtin_amdgcn_sqrtf(r2 > 0.f ? r2 : 0.f);
  if (kind == K_MATERN12) { val = __expf(-r); base = r > 1e-15f ? val / r : 0.f; return; }
  if (kind == K_MATERN32) { const float s = 1.7320508075688772f * r, e = __expf(-s); val = (1.f + s) * e; base = 3.f * e; return; }
  const float s = 2.23606797749979f * r, e = __expf(-s);
  val = (1.f + s + (5.0f / 3.0f) * r2) * e;
  base = (5.0f / 3.0f) * (1.f + s) * e;
}
__device__ __forceinline__ void kern_value_base_fast(int kind, double r2, double &val, double &base) {
  kern_value_base<double>(kind, r2, val, base);
}


// Two elements at a time (fp32: the polynomial parts compile to packed v_pk_* instructions; only the square root and
// the exponential stay scalar).  Same values as kern_value_base_fast.
__device__ __forceinline__ float  fast_exp(float x) { return __expf(x); }
__device__ __forceinline__ double fast_exp(double x) { return exp(x); }
__device__ __forceinline__ float  fast_sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
__device__ __forceinline__ double fast_sqrt(double x) { return sqrt(x); }
template <typename T> using Pair = T __attribute__((ext_vector_type(2)));
template <typename T> __device__ __forceinline__ void kern_value_base_pair(int kind, Pair<T> r2, Pair<T> &val, Pair<T> &base) {
  if (kind == K_RBF) {
    const Pair<T> a = T(-0.5) * r2;
    val = Pair<T>{fast_exp(a.x), fast_exp(a.y)};
    base = val;
    return;
  }
  const Pair<T> r = {fast_sqrt(r2.x > T(0) ? r2.x : T(0)), fast_sqrt(r2.y > T(0) ? r2.y : T(0))};
  if (kind == K_MATERN12) {
    val = Pair<T>{fast_exp(-r.x), fast_exp(-r.y)};
    base = Pair<T>{r.x > T(1e-15) ? val.x / r.x : T(0), r.y > T(1e-15) ? val.y / r.y : T(0)};
    return;
  }
  if (kind == K_MATERN32) {
    const Pair<T> s = T(1.7320508075688772) * r, e = {fast_exp(-s.x), fast_exp(-s.y)};
    val = (T(1) + s) * e;
    base = T(3) * e;
    return;
  }
  const Pair<T> s = T(2.23606797749979) * r, e = {fast_exp(-s.x), fast_exp(-s.y)};
  const Pair<T> ope = (T(1) + s) * e;
  val = ope + T(5.0 / 3.0) * r2 * e;
  base = T(5.0 / 3.0) * ope;
}

// exp / sqrt of the packed assembly path.  fp32: the hardware exp2 on x log2(e) with the rounding error of that
// product carried along (t + e = x log2(e) to ~2^-45; exp2(t) is good to 1 ulp), so the result is within ~1.5 ulp
// for every argument -- the plain __expf loses |x| 2^-24 -- at 6 instructions instead of the ~20 of expf; v_sqrt_f32
// is 1 ulp.  fp64 keeps the library forms.
__device__ __forceinline__ float asm_exp(float x) {
  const float L = 1.44269504088896340736f, Ll = 1.9259629911266175e-8f;   // log2(e) = L + Ll
  const float t = x * L;
  const float e = __builtin_fmaf(x, L, -t) + x * Ll;
  const float r = __builtin_amdgcn_exp2f(t);
  return __builtin_fmaf(r, e * 0.6931471805599453f, r);
}
__device__ __forceinline__ double asm_exp(double x) { return exp(x); }
__device__ __forceinline__ float asm_sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
__device__ __forceinline__ double asm_sqrt(double x) { return sqrt(x); }
#define dexp asm_exp
#define dsqrt asm_sqrt
// Two covariance values at a time (assembly kernels).
template <typename T> __device__ __forceinline__ Pair<T> kern_value_pair(int kind, Pair<T> r2) {
  if (kind == K_RBF) {
    const Pair<T> a = T(-0.5) * r2;
    return Pair<T>{dexp(a.x), dexp(a.y)};
  }
  const Pair<T> r = {dsqrt(r2.x > T(0) ? r2.x : T(0)), dsqrt(r2.y > T(0) ? r2.y : T(0))};
  if (kind == K_MATERN12) return Pair<T>{dexp(-r.x), dexp(-r.y)};
  if (kind == K_MATERN32) {
    const Pair<T> s = T(1.7320508075688772) * r;
    return (T(1) + s) * Pair<T>{dexp(-s.x), dexp(-s.y)};
  }
  const Pair<T> s = T(2.23606797749979) * r;
  return (T(1) + s + T(5.0 / 3.0) * r2) * Pair<T>{dexp(-s.x), dexp(-s.y)};
}

// ---- spectral mixture [gpytorch-knowledge: SpectralMixtureKernel.forward]:
//     k(x, x') = sum_m w_m exp(-2 pi^2 sum_k s_mk^2 tau_k^2) prod_k cos(2 pi mu_mk tau_k),   tau = x - x'.
// The carrier's phase mu tau is hundreds to thousands of revolutions at the sizes this library is built for (mu up to 0.5 / the
// smallest spacing), so it is reduced IN REVOLUTIONS before the cosine: tau = a - b with its rounding residual (TwoSum), t = mu tau
// with its FMA residual, f = t - rint(t) (exact) with the residuals added back; |f| <= 1/2 + a few ulp carries an absolute error of a
// few 2^-25 whatever the phase was ("Spectral mixture: the phase in fp32").
template <typename T> __device__ __forceinline__ T sm_phase(T a, T b, T mu) {
  const T tau = a - b;
  const T bv = tau - a;
  const T te = (a - (tau - bv)) - (b + bv);               // a - b = tau + te exactly
  const T t = mu * tau;
  const T tr = __builtin_fma(mu, tau, -t);                // mu tau = t + tr exactly
  return (t - __builtin_rint(t)) + __builtin_fma(mu, te, tr);
}
// cos / sin of 2 pi f.  Assembly: the library's cospi (fp32: ~1 ulp); gradient epilogue (fp32): the hardware forms, which take revolutions
__device__ __forceinline__ float  sm_cos(float f) { return cospif(2.0f * f); }
__device__ __forceinline__ double sm_cos(double f) { return cospi(2.0 * f); }
__device__ __forceinline__ void sm_sincos_fast(float f, float &s, float &c) { s = __builtin_amdgcn_sinf(f); c = __builtin_amdgcn_cosf(f); }
__device__ __forceinline__ void sm_sincos_fast(double f, double &s, double &c) { sincospi(2.0 * f, &s, &c); }
constexpr double SM_2PI2 = 19.739208802178716;             // 2 pi^2
constexpr double SM_2PI = 6.283185307179586;
// one covariance value (unit noise-free): rows of DCAP raw coordinates a, b; sc, mu [M][DCAP] (0 beyond d: factor exactly 1), wt [M]
template <typename T, int DCAP>
__device__ __forceinline__ T sm_value(const T (&a)[DCAP], const T (&b)[DCAP], const T *sc, const T *mu, const T *wt, int M) {
  T sum = T(0);
#pragma unroll 1
  for (int m = 0; m < M; ++m) {
    T e = T(0), c = T(1);
#pragma unroll
    for (int k = 0; k < DCAP; ++k) {
      const T st = sc[m * DCAP + k] * (a[k] - b[k]);
      e += st * st;
      c *= sm_cos(sm_phase(a[k], b[k], mu[m * DCAP + k]));
    }
    sum += wt[m] * (dexp(T(-SM_2PI2) * e) * c);
  }
  return sum;
}
__device__ __forceinline__ void sm_sincos(float f, float &s, float &c) { s = sinpif(2.0f * f); c = cospif(2.0f * f); }
__device__ __forceinline__ void sm_sincos(double f, double &s, double &c) { sincospi(2.0 * f, &s, &c); }
// d k / d a_k, summed over the M components (sm_value's tables):
//     w env [-4 pi^2 s_k^2 tau_k prod_l cos_l - 2 pi mu_k sin_k prod_{l != k} cos_l],
// the product of the other cosines from prefix and suffix products (kinv_epilogue_sm.inc): no division, finite where a cosine is 0.
// A dimension with s = mu = 0 gives exactly 0.
template <typename T, int DCAP>
__device__ __forceinline__ void sm_dx(const T (&a)[DCAP], const T *b, const T *sc, const T *mu, const T *wt, int M, T g, T (&gx)[DCAP]) {
#pragma unroll 1
  for (int m = 0; m < M; ++m) {
    T tau[DCAP], sn[DCAP], cs[DCAP], ex[DCAP];
    T e = T(0), pre = T(1);
#pragma unroll
    for (int k = 0; k < DCAP; ++k) {
      tau[k] = a[k] - b[k];
      const T st = sc[m * DCAP + k] * tau[k];
      e += st * st;
      sm_sincos(sm_phase(a[k], b[k], mu[m * DCAP + k]), sn[k], cs[k]);
      ex[k] = pre;
      pre *= cs[k];
    }
    T suf = T(1);
#pragma unroll
    for (int k = DCAP - 1; k >= 0; --k) { ex[k] *= suf; suf *= cs[k]; }
    const T cw = g * wt[m] * dexp(T(-SM_2PI2) * e);
#pragma unroll
    for (int k = 0; k < DCAP; ++k) {
      const T s = sc[m * DCAP + k];
      gx[k] -= cw * (T(2 * SM_2PI2) * (s * s * tau[k]) * pre + T(SM_2PI) * (mu[m * DCAP + k] * sn[k]) * ex[k]);
    }
  }
}

// ---- periodic [gpytorch-knowledge: PeriodicKernel.forward, v1.11, unverified offline]:
//     k(x, x') = exp(-2 sum_k sin^2(pi (x_k - x'_k) / p_k) / ell_k)            (the lengthscale is not squared).
// The phase f_k = tau_k / p_k is reduced in revolutions like the spectral mixture's (sm_phase) with the inverse period as the frequency.
// 1 / p is staged as TWO terms, ip = fl(1 / p) and ipr = fl(fl(1 - ip p) ip) ~ 1 / p - ip (the FMA's 1 - ip p is exact), so that the
// rounding of 1 / p does not cost f 2^-24 revolutions: tau ipr, at most f 2^-24, is added to the reduced phase.  sin^2(pi f) has period 1
// in f, sin(2 pi f) too, so the reduction to |f| <= 1/2 changes neither ("Periodic kernel: the phase in fp32").
template <typename T> __device__ __forceinline__ void per_inv_period(T p, T &ip, T &ipr) {
  ip = T(1) / p;
  ipr = __builtin_fma(-ip, p, T(1)) * ip;
}
template <typename T> __device__ __forceinline__ T per_phase(T a, T b, T ip, T ipr) {
  return sm_phase(a, b, ip) + (a - b) * ipr;
}
// sin(pi f).  Assembly: the library's sinpi (fp32: ~1 ulp)
__device__ __forceinline__ float  per_sinpi(float f) { return sinpif(f); }
__device__ __forceinline__ double per_sinpi(double f) { return sinpi(f); }
// gradient epilogue: s2 = sin(2 pi f) and omc = 1 - cos(2 pi f) = 2 sin^2(pi f), the latter from sin(pi f) (no cancellation at small f).
// fp32: the hardware sine, which takes revolutions
__device__ __forceinline__ void per_sin_fast(float f, float &s2, float &omc) {
  const float s1 = __builtin_amdgcn_sinf(0.5f * f);
  s2 = __builtin_amdgcn_sinf(f);
  omc = 2.0f * s1 * s1;
}
__device__ __forceinline__ void per_sin_fast(double f, double &s2, double &omc) {
  double s1, c1;
  sincospi(f, &s1, &c1);
  s2 = 2.0 * s1 * c1;
  omc = 2.0 * s1 * s1;
}
// one covariance value (unit output scale): rows of DCAP raw coordinates a, b; ip, ipr, w = 1 / ell [DCAP] (all 0 beyond d: that
// dimension adds exactly 0 to the exponent)
template <typename T, int DCAP>
__device__ __forceinline__ T per_value(const T (&a)[DCAP], const T (&b)[DCAP], const T *ip, const T *ipr, const T *w) {
  T e = T(0);
#pragma unroll
  for (int k = 0; k < DCAP; ++k) {
    const T s = per_sinpi(per_phase(a[k], b[k], ip[k], ipr[k]));
    e += (s * s) * w[k];
  }
  return dexp(T(-2) * e);
}
// sin(pi f), cos(pi f): sin(2 pi f) = 2 s c
__device__ __forceinline__ void per_sincospi(float f, float &s, float &c) { s = sinpif(f); c = cospif(f); }
__device__ __forceinline__ void per_sincospi(double f, double &s, double &c) { sincospi(f, &s, &c); }
constexpr double PER_2PI = 6.283185307179586;
// d k / d a_k = -k (2 / ell_k) (pi / p_k) sin(2 pi f_k)                                    (per_value's tables)
template <typename T, int DCAP>
__device__ __forceinline__ void per_dx(const T (&a)[DCAP], const T *b, const T *ip, const T *ipr, const T *w, T g, T os, T (&gx)[DCAP]) {
  T s2[DCAP];
  T e = T(0);
#pragma unroll
  for (int k = 0; k < DCAP; ++k) {
    T s, c;
    per_sincospi(per_phase(a[k], b[k], ip[k], ipr[k]), s, c);
    e += (s * s) * w[k];
    s2[k] = T(2) * s * c;
  }
  const T cw = g * os * dexp(T(-2) * e);
#pragma unroll
  for (int k = 0; k < DCAP; ++k) gx[k] -= cw * (T(PER_2PI) * (w[k] * ip[k]) * s2[k]);
}

// ---- rational quadratic [gpytorch-knowledge: RQKernel, unverified offline]:
//     k(x, x') = (1 + r^2 / (2 alpha))^(-alpha),   r^2 = sum_k ((x_k - x'_k) / ell_k)^2,   alpha > 0 one scalar per latent.
// The value is exp(-alpha log1p(u)), u = r^2 fl(1 / (2 alpha)): pow(1 + u, -alpha) and log(1 + u) lose the low bits of u in the sum
// 1 + u, which alpha then multiplies (alpha 2^-24 absolute in fp32; a trained alpha is 10^3 .. 10^6 when the data are RBF-like).  With the
// library's log1p (accurate at small u) the exponent a = alpha log1p(u) <= r^2 / 2 carries a few ulp RELATIVE whatever alpha is
// ("Rational-quadratic kernel: fp32 numerics").  u = 0 gives exactly 1.
__device__ __forceinline__ float  rq_log1p(float u) { return log1pf(u); }
__device__ __forceinline__ double rq_log1p(double u) { return log1p(u); }
__device__ __forceinline__ float  rq_rcp(float x) { return __builtin_amdgcn_rcpf(x); }        // 1 ulp; weights a reduction only
__device__ __forceinline__ double rq_rcp(double x) { return 1.0 / x; }
template <typename T> __device__ __forceinline__ T rq_profile(T r2, T alpha, T i2a) { return dexp(-alpha * rq_log1p(r2 * i2a)); }
// h(u) = log1p(u) - u / (1 + u) >= 0, the factor of d k / d alpha = -k h(u); h ~ u^2 / 2, and the two terms agree to u / 2 of their
// size.  Below u = 1/8 the series sum_{k >= 2} (-1)^k (k - 1) / k u^k, through u^9 (fp32) / u^19 (fp64): the first term left out is
// below 1.9 u^(K - 1) of h, i.e. 1.9 2^-24 / 1.9 2^-54.  From 1/8 on the direct form from `l1p` = log1p(u) and `rc` = 1 / (1 + u): its two
// terms carry ~5 roundings of size u, h >= 0.43 u^2 there, so <= ~12 / u <= 96 roundings = 48 ulp relative.
template <typename T> __device__ __forceinline__ T rq_h(T u, T l1p, T rc) {
  constexpr int KMAX = sizeof(T) == 4 ? 9 : 19;
  T p = T((KMAX & 1 ? -1.0 : 1.0) * (KMAX - 1) / KMAX);
#pragma unroll
  for (int k = KMAX - 1; k >= 2; --k) p = __builtin_fma(p, u, T((k & 1 ? -1.0 : 1.0) * (k - 1) / k));
  return u < T(0.125) ? p * (u * u) : __builtin_fma(-u, rc, l1p);
}
// gradient epilogue: value, base = val / (1 + u) (d k / d ell_k = base df_k^2 / ell_k, the library's convention) and val h(u), unit
// output scale.  The accurate exponential here too: d / d alpha at large alpha is a sum of terms ~ u^2 that the error of __expf
// (|a| 2^-24) would be weighed against.
template <typename T> __device__ __forceinline__ void rq_value_base_h(T r2, T alpha, T i2a, T &val, T &base, T &vh) {
  const T u = r2 * i2a, l1p = rq_log1p(u), rc = rq_rcp(T(1) + u);
  val = dexp(-alpha * l1p);
  base = val * rc;
  vh = val * rq_h(u, l1p, rc);
}
// one covariance value (unit output scale): rows of DCAP raw coordinates a, b; w = 1 / ell [DCAP] (0 beyond d).  The difference is
// taken from the RAW inputs and then scaled (k_kernel_vjp_add): no |x| / ell term in the error, exactly 0 at coincident points.
template <typename T, int DCAP>
__device__ __forceinline__ T rq_value(const T (&a)[DCAP], const T (&b)[DCAP], const T *w, T alpha, T i2a) {
  T r2 = T(0);
#pragma unroll
  for (int k = 0; k < DCAP; ++k) {
    const T sd = (a[k] - b[k]) * w[k];
    r2 += sd * sd;
  }
  return rq_profile(r2, alpha, i2a);
}
// d k / d a_k = -base df_k / ell_k with rq_value_base_h's base = k / (1 + u)                 (rq_value's tables)
template <typename T, int DCAP>
__device__ __forceinline__ void rq_dx(const T (&a)[DCAP], const T *b, const T *w, T alpha, T i2a, T g, T os, T (&gx)[DCAP]) {
  T df[DCAP];
  T r2 = T(0);
#pragma unroll
  for (int k = 0; k < DCAP; ++k) {
    df[k] = (a[k] - b[k]) * w[k];
    r2 += df[k] * df[k];
  }
  T val, base, vh;
  rq_value_base_h(r2, alpha, i2a, val, base, vh);
  const T c = g * os * base;
#pragma unroll
  for (int k = 0; k < DCAP; ++k) gx[k] -= (c * df[k]) * w[k];
}

// ---- locally periodic [gpytorch-knowledge: ProductKernel of PeriodicKernel and RBFKernel, unverified offline]:
//     k(x, x') = exp(-2 sum_k sin^2(pi tau_k / p_k) / ell_k - 1/2 sum_k (tau_k / lam_k)^2),   tau = x - x'
// (ell the periodic lengthscale, not squared; lam the RBF lengthscale).  The periodic exponent is per_value's: the phase reduced in
// revolutions, 1 / p as two terms.  The RBF exponent is rq_value's r^2: the RAW difference scaled by v = 1 / lam, exactly 0 at coincident
// points and beyond d.  ONE accurate exponential of the summed exponent ("Locally periodic kernel: fp32 numerics"); with
// v = 0 the sum is per_value's exponent bit for bit, with w = 0 it is -r^2 / 2.
template <typename T> __device__ __forceinline__ T lper_exp(T e, T r2) { return dexp(__builtin_fma(T(-0.5), r2, T(-2) * e)); }
// one covariance value (unit output scale): rows of DCAP raw coordinates a, b; ip, ipr, w = 1 / ell, v = 1 / lam [DCAP] (all 0 beyond d:
// that dimension adds exactly 0 to both exponents)
template <typename T, int DCAP>
__device__ __forceinline__ T lper_value(const T (&a)[DCAP], const T (&b)[DCAP], const T *ip, const T *ipr, const T *w, const T *v) {
  T e = T(0), r2 = T(0);
#pragma unroll
  for (int k = 0; k < DCAP; ++k) {
    const T s = per_sinpi(per_phase(a[k], b[k], ip[k], ipr[k]));
    e += (s * s) * w[k];
    const T sd = (a[k] - b[k]) * v[k];
    r2 += sd * sd;
  }
  return lper_exp(e, r2);
}
// d k / d a_k = -k [(2 / ell_k) (pi / p_k) sin(2 pi f_k) + tau_k / lam_k^2]: the periodic term (per_dx) plus the RBF one, sharing
// the one exponential                                                                        (lper_value's tables)
template <typename T, int DCAP>
__device__ __forceinline__ void lper_dx(const T (&a)[DCAP], const T *b, const T *ip, const T *ipr, const T *w, const T *v, T g, T os,
                                        T (&gx)[DCAP]) {
  T s2[DCAP], sd[DCAP];
  T e = T(0), r2 = T(0);
#pragma unroll
  for (int k = 0; k < DCAP; ++k) {
    T s, c;
    per_sincospi(per_phase(a[k], b[k], ip[k], ipr[k]), s, c);
    e += (s * s) * w[k];
    s2[k] = T(2) * s * c;
    sd[k] = (a[k] - b[k]) * v[k];
    r2 += sd[k] * sd[k];
  }
  const T cw = g * os * lper_exp(e, r2);
#pragma unroll
  for (int k = 0; k < DCAP; ++k) gx[k] -= cw * (T(PER_2PI) * (w[k] * ip[k]) * s2[k] + sd[k] * v[k]);
}

// ---- dot product [gpytorch-knowledge: LinearKernel, PolynomialKernel, unverified offline]:
//     k(x, x') = (c + sum_k v_k x_k x'_k)^P,   v_k > 0, c >= 0, P an integer >= 1
// (LinearKernel: P = 1, c = 0; PolynomialKernel: v = 1).  NOT stationary: k(x, x) = (c + sum_k v_k x_k^2)^P is a value like any other, so
// the diagonal goes through these functions too.  s is one FMA chain over the raw inputs that starts from c, with the row's coordinates
// scaled once (t_k = v_k a_k, one rounding); s^P is P - 1 multiplications -- no pow, exp or log, so a negative s keeps its sign under an
// odd P and s = 0 gives exactly 0 (P = 1: exactly s).  fp32: |error| <= P (d + 2) 2^-24 S^P to first order, S = c + sum_k |v_k a_k b_k|
// ("Dot-product kernels: fp32 numerics").
__device__ __forceinline__ float  dot_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double dot_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
// s^P and, in `pm1`, s^(P - 1) from the same chain: 1 * s * s ... (the first product is exact)
template <typename T> __device__ __forceinline__ T dot_pow(T s, int P, T &pm1) {
  T p = T(1);
#pragma unroll 1
  for (int i = 1; i < P; ++i) p *= s;
  pm1 = p;
  return p * s;
}
// one covariance value (unit output scale): ta = v a [DCAP] (0 beyond d: that dimension adds exactly 0 to s), b raw
template <typename T, int DCAP>
__device__ __forceinline__ T dot_value(const T (&ta)[DCAP], const T (&b)[DCAP], T c, int P) {
  T s = c;
#pragma unroll
  for (int k = 0; k < DCAP; ++k) s = dot_fma(ta[k], b[k], s);
  T pm1;
  return dot_pow(s, P, pm1);
}
// gradient epilogue: value s^P and P s^(P - 1) (d k / d c; d k / d v_k = P s^(P - 1) a_k b_k), unit output scale.  pr = a b [DCAP]
// (the products the d / d v sums need anyway), v [DCAP] (0 beyond d)
template <typename T, int DCAP>
__device__ __forceinline__ void dot_value_deriv(const T (&pr)[DCAP], const T (&v)[DCAP], T c, int P, T &val, T &dval) {
  T s = c;
#pragma unroll
  for (int k = 0; k < DCAP; ++k) s = dot_fma(v[k], pr[k], s);
  T pm1;
  val = dot_pow(s, P, pm1);
  dval = T(P) * pm1;
}
#undef dexp
#undef dsqrt

}  // namespace plmc
