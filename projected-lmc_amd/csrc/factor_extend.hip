// factor_extend.hip -- bordered update of a finished factorisation (plmc_factor_extend_*): condition a factor buffer with the inverse
// factor on m <= 128 new rows without a new sweep.
//
// Per latent, Khat = U^T U, W = U^-T (lower), V = W K12 already in the first m augmented columns of the source:
//     Bt = V^T W = (Khat^-1 K12)^T   (128 x n_pad, tile engine, the W tiles above the block diagonal are never loaded)
//     G  = V^T V                     (128 x 128, tile engine)
//     S  = K22 - G in fp64, U22 = chol(S)^T, W22 = U22^-T: k_diag<double> (diag_block.hpp) on S padded to 128 with the identity
//     W21 = -W22 Bt                  (128 x n_pad, tile engine; rows >= m are not used)
//     U' = [[U, V], [0, U22]],  W' = [[W, 0], [W21, W22]],  log det' = log det + 2 sum log diag U22.
// The only O(n^2) part is the tile copy source -> destination (k_fx_copy, HBM-bound); with A_dst == A_src it is skipped.
// Everything runs on the caller's stream; sums have a fixed order, there are no atomics.
#include "api_common.hpp"
#include "diag_block.hpp"
#include "../../include/plmc.h"

namespace plmc {

// Per-latent scratch, in bytes from its start: Bt | Tm (128 x n_pad elements each) | G | W22t (128 x 128 elements each) |
// S64 | V64 | W64 (128 x 128 doubles each: the block k_diag<double> factors in place, its W_kk^T and W_kk outputs).
struct FxScratch {
  int64_t bt, tm, g, w22t, s64, v64, w64, bytes;
  FxScratch(int64_t n_pad, int esz) {
    bt = 0;
    tm = bt + (int64_t)NB * n_pad * esz;
    g = tm + (int64_t)NB * n_pad * esz;
    w22t = g + (int64_t)NB * NB * esz;
    s64 = w22t + (int64_t)NB * NB * esz;
    v64 = s64 + (int64_t)NB * NB * 8;
    w64 = v64 + (int64_t)NB * NB * 8;
    bytes = w64 + (int64_t)NB * NB * 8;
  }
};

// Tile copy of the U upper / W lower 128-tiles of the source into the destination (another row stride, another W column, more block
// rows).  grid (mbd * mbd, 2, q): tile (ib, jb) of the square part (y = 0, ib <= jb) or of the W columns (y = 1, ib >= jb).  An element is
// LIVE when row and column are both < n: it is the source's; every other element is the identity (1 on the diagonal, 0 elsewhere) -- the
// source's own padding identity is never copied, the border kernels then write rows / columns [n, n + m).  Eight 16-byte loads per thread
// are in flight; the tiles that straddle n are masked by a select on unconditional loads (a tile without any live element loads nothing:
// the branch is uniform over the workgroup).
template <typename T>
__global__ __launch_bounds__(NTHREADS) void k_fx_copy(const T *__restrict__ S, int64_t lds, int64_t wcs, int64_t strideS, int mbs,
                                                      T *__restrict__ D, int64_t ldd, int64_t wcd, int64_t strideD, int mbd, int n) {
  using vec_t = typename Traits<T>::vec_t;
  constexpr int EPV = Traits<T>::EPV, CPR = NB / EPV, RPP = NTHREADS / CPR, UNR = 8;
  const int ib = blockIdx.x / mbd, jb = blockIdx.x % mbd, which = blockIdx.y, lat = blockIdx.z;
  if (which == 0 ? ib > jb : ib < jb) return;
  const bool has_src = ib < mbs && jb < mbs && ib * NB < n && jb * NB < n;
  const int r0 = threadIdx.x / CPR, c = (threadIdx.x % CPR) * EPV;
  const T *sp = S + (int64_t)lat * strideS + (which ? wcs : 0) + (int64_t)(has_src ? ib : 0) * NB * lds + (int64_t)(has_src ? jb : 0) * NB + c;
  T *dp = D + (int64_t)lat * strideD + (which ? wcd : 0) + (int64_t)ib * NB * ldd + (int64_t)jb * NB + c;
  for (int rr = r0; rr < NB; rr += RPP * UNR) {
    vec_t v[UNR];
    if (has_src) {
#pragma unroll
      for (int u = 0; u < UNR; ++u) v[u] = *reinterpret_cast<const vec_t *>(sp + (int64_t)(rr + u * RPP) * lds);
    } else {
#pragma unroll
      for (int u = 0; u < UNR; ++u)
#pragma unroll
        for (int e = 0; e < EPV; ++e) v[u][e] = T(0);
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int i = ib * NB + rr + u * RPP;
      vec_t o;
#pragma unroll
      for (int e = 0; e < EPV; ++e) {
        const int j = jb * NB + c + e;
        o[e] = (i < n && j < n) ? v[u][e] : (i == j ? T(1) : T(0));
      }
      *reinterpret_cast<vec_t *>(dp + (int64_t)(rr + u * RPP) * ldd) = o;
    }
  }
}

// S64 = K22 - G in fp64 (symmetric from the upper triangles, padded to 128 with the identity), V64 = W64 = 0 (k_diag writes only the
// 16 x 16 tiles on and below the diagonal), and rows >= m of Bt = 0 (what stands in augmented columns >= m of the source is not V).
// grid (n_pad / 128, q); workgroup 0 of a latent also prepares the three 128 x 128 blocks.
template <typename T>
__global__ __launch_bounds__(NTHREADS) void k_fx_prep(const T *__restrict__ K22, int m, const T *__restrict__ G, double *__restrict__ S64,
                                                      double *__restrict__ V64, double *__restrict__ W64, T *__restrict__ Bt, int64_t n_pad,
                                                      int64_t stride_bytes) {
  const int lat = blockIdx.y, tid = threadIdx.x;
  const int64_t off = (int64_t)lat * stride_bytes;
  T *bt = reinterpret_cast<T *>(reinterpret_cast<char *>(Bt) + off);
  for (int e = tid; e < (NB - m) * NB; e += NTHREADS) {
    const int r = m + e / NB, c = e % NB;
    bt[(int64_t)r * n_pad + (int64_t)blockIdx.x * NB + c] = T(0);
  }
  if (blockIdx.x != 0) return;
  const T *g = reinterpret_cast<const T *>(reinterpret_cast<const char *>(G) + off);
  double *s = reinterpret_cast<double *>(reinterpret_cast<char *>(S64) + off);
  double *v = reinterpret_cast<double *>(reinterpret_cast<char *>(V64) + off);
  double *w = reinterpret_cast<double *>(reinterpret_cast<char *>(W64) + off);
  const T *k22 = K22 + (int64_t)lat * m * m;
  for (int e = tid; e < NB * NB; e += NTHREADS) {
    const int i = e / NB, j = e % NB;
    const int a = i < j ? i : j, b = i < j ? j : i;
    // clamped, unconditional loads; the select keeps what lies outside the m x m block out of S
    const int ac = a < m ? a : m - 1, bc = b < m ? b : m - 1;
    const double kv = (double)k22[ac * m + bc], gv = (double)g[ac * NB + bc];
    s[e] = b < m ? kv - gv : (i == j ? 1.0 : 0.0);
    v[e] = 0.0;
    w[e] = 0.0;
  }
}

// After k_diag<double>: S64 holds U22 (upper), W64 holds W22 (lower, zeros above the diagonal).  One workgroup per latent:
//   info / log det from the fp64 pivots (thread 0, fixed order): the first k whose pivot is not a positive finite number -- in fp64, and
//     rounded to the element type -- gives info = 1 + n + k;
//   W22t[k][i] = W22[i][k] in the element type, zero outside the m x m block: the K-major operand of W21 = -W22 Bt;
//   U22 into the destination's square part (element-wise upper triangle of rows / columns [n, n + m)), W22 into its W columns: the
//     lower triangle, and explicit zeros above the diagonal where row and column share a 128-block (a W tile above the block diagonal
//     is never touched).
template <typename T>
__global__ __launch_bounds__(NTHREADS) void k_fx_fin(const double *__restrict__ S64, const double *__restrict__ W64, T *__restrict__ W22t,
                                                     int64_t stride_bytes, T *__restrict__ D, int64_t ldd, int64_t wcd, int64_t strideD, int n, int m,
                                                     double *__restrict__ logdet, int *__restrict__ info) {
  const int lat = blockIdx.x, tid = threadIdx.x;
  const int64_t off = (int64_t)lat * stride_bytes;
  const double *s = reinterpret_cast<const double *>(reinterpret_cast<const char *>(S64) + off);
  const double *w = reinterpret_cast<const double *>(reinterpret_cast<const char *>(W64) + off);
  T *wt = reinterpret_cast<T *>(reinterpret_cast<char *>(W22t) + off);
  T *d = D + (int64_t)lat * strideD;
  if (tid == 0) {
    double lg = 0.0;
    int bad = 0;
    for (int k = 0; k < m; ++k) {
      const double p = s[k * NB + k];
      const T pt = (T)p;
      const bool ok = p > 0.0 && p < 1.0e300 && pt > T(0) && pt < T(3.0e38);
      if (ok) lg += 2.0 * log(p);
      else if (bad == 0) bad = 1 + n + k;
    }
    logdet[lat] += lg;
    info[lat] = bad;
  }
  for (int e = tid; e < NB * NB; e += NTHREADS) {
    const int k = e / NB, i = e % NB;
    wt[e] = (k <= i && i < m) ? (T)w[i * NB + k] : T(0);
  }
  for (int e = tid; e < m * m; e += NTHREADS) {
    const int i = e / m, j = e % m;
    const int64_t gi = n + i, gj = n + j;
    if (i <= j) d[gi * ldd + gj] = (T)s[i * NB + j];
    if (j <= i) d[gi * ldd + wcd + gj] = (T)w[i * NB + j];
    else if (gi / NB == gj / NB) d[gi * ldd + wcd + gj] = T(0);
  }
}

// The border: V (the first m augmented columns of the source, rows < n) into columns [n, n + m) of the destination's square part, and
// W21 = -Tm (rows < m, columns < n) into rows [n, n + m) of its W columns.  Grid-stride over the 2 n m elements, grid (x, q).
template <typename T>
__global__ __launch_bounds__(NTHREADS) void k_fx_border(const T *__restrict__ S, int64_t lds, int64_t nps, int64_t strideS, const T *__restrict__ Tm,
                                                        int64_t stride_bytes, T *D, int64_t ldd, int64_t wcd, int64_t strideD, int n, int m) {
  const int lat = blockIdx.y;
  const T *v = S + (int64_t)lat * strideS + nps;
  const T *tm = reinterpret_cast<const T *>(reinterpret_cast<const char *>(Tm) + (int64_t)lat * stride_bytes);
  T *d = D + (int64_t)lat * strideD;
  const int64_t total = (int64_t)n * m;
  for (int64_t e = (int64_t)blockIdx.x * NTHREADS + threadIdx.x; e < total; e += (int64_t)gridDim.x * NTHREADS) {
    const int64_t i = e / m, c = e % m;
    d[i * ldd + n + c] = v[i * lds + c];
    const int64_t r = e / n, cc = e % n;
    d[(n + r) * ldd + wcd + cc] = -tm[r * nps + cc];
  }
}

// Zero the destination's augmented block, columns [n_pad, wcol0) of every row: the next plmc_write_rhs finds padded rows that are 0.
// grid (n_pad, q); 16-byte stores.
template <typename T>
__global__ __launch_bounds__(NTHREADS) void k_fx_zero_aug(T *__restrict__ D, int64_t ldd, int64_t npd, int64_t wcd, int64_t strideD) {
  using vec_t = typename Traits<T>::vec_t;
  constexpr int EPV = Traits<T>::EPV;
  T *row = D + (int64_t)blockIdx.y * strideD + (int64_t)blockIdx.x * ldd + npd;
  vec_t z;
#pragma unroll
  for (int e = 0; e < EPV; ++e) z[e] = T(0);
  for (int64_t c = (int64_t)threadIdx.x * EPV; c < wcd - npd; c += (int64_t)NTHREADS * EPV) *reinterpret_cast<vec_t *>(row + c) = z;
}

template <typename T> struct FxGemm;
template <> struct FxGemm<float> {
  static int tn(int tri, int M, int N, int K, const float *A, int64_t lda, int64_t sa, const float *B, int64_t ldb, int64_t sb, float *C, int64_t ldc,
                int64_t sc, int q, void *st) {
    return plmc_gemm_tn_tri_f32(0, tri, M, N, K, A, lda, sa, B, ldb, sb, C, ldc, sc, q, st);
  }
};
template <> struct FxGemm<double> {
  static int tn(int tri, int M, int N, int K, const double *A, int64_t lda, int64_t sa, const double *B, int64_t ldb, int64_t sb, double *C, int64_t ldc,
                int64_t sc, int q, void *st) {
    return plmc_gemm_tn_tri_f64(0, tri, M, N, K, A, lda, sa, B, ldb, sb, C, ldc, sc, q, st);
  }
};

template <typename T>
int factor_extend_impl(const T *A_src, int n, int64_t nps, int64_t lds, int64_t wcs, int64_t strideS, int m, const T *K22, T *A_dst, int64_t npd,
                       int64_t ldd, int64_t wcd, int64_t strideD, double *logdet, int *info, void *scratch, int q, void *stream) {
  constexpr int EPV = Traits<T>::EPV;
  PLMC_REQUIRE(A_src && K22 && A_dst && logdet && info && scratch, "null pointer");
  PLMC_REQUIRE(q > 0 && n > 0 && m >= 1 && m <= NB, "q > 0, n > 0, 1 <= m <= plmc_block() (the caller loops for more rows)");
  PLMC_REQUIRE(nps > 0 && nps % NB == 0 && lds % NB == 0 && wcs % NB == 0 && n <= nps, "source: n <= n_pad, n_pad / lda / wcol0 multiples of NB");
  PLMC_REQUIRE(nps + NB <= wcs && wcs + nps <= lds, "source: one block of augmented columns (V) between the square part and the W columns");
  PLMC_REQUIRE(npd > 0 && npd % NB == 0 && ldd % NB == 0 && wcd % NB == 0 && npd <= wcd && wcd + npd <= ldd,
               "destination: n_pad / lda / wcol0 multiples of NB, W columns inside lda");
  PLMC_REQUIRE(npd >= plmc_pad((int64_t)n + m), "destination: n_pad < plmc_pad(n + m)");
  PLMC_REQUIRE(aligned16(A_src) && aligned16(A_dst) && aligned16(scratch) && strideS % EPV == 0 && strideD % EPV == 0, "16-byte alignment");
  PLMC_REQUIRE(q == 1 || (strideS >= nps * lds && strideD >= npd * ldd), "batch stride smaller than one latent's buffer");
  const bool in_place = A_dst == A_src;
  if (in_place) {
    PLMC_REQUIRE(npd == nps && ldd == lds && wcd == wcs && strideD == strideS, "A_dst == A_src needs identical geometry");
  } else {
    const char *s0 = reinterpret_cast<const char *>(A_src), *d0 = reinterpret_cast<const char *>(A_dst);
    const char *s1 = s0 + ((int64_t)(q - 1) * strideS + nps * lds) * (int64_t)sizeof(T), *d1 = d0 + ((int64_t)(q - 1) * strideD + npd * ldd) * (int64_t)sizeof(T);
    PLMC_REQUIRE(s1 <= d0 || d1 <= s0, "source and destination overlap (only A_dst == A_src with identical geometry may alias)");
  }
  const FxScratch L(nps, (int)sizeof(T));
  char *sc = reinterpret_cast<char *>(scratch);
  T *Bt = reinterpret_cast<T *>(sc + L.bt), *Tm = reinterpret_cast<T *>(sc + L.tm), *G = reinterpret_cast<T *>(sc + L.g), *W22t = reinterpret_cast<T *>(sc + L.w22t);
  double *S64 = reinterpret_cast<double *>(sc + L.s64), *V64 = reinterpret_cast<double *>(sc + L.v64), *W64 = reinterpret_cast<double *>(sc + L.w64);
  const int64_t sstr = L.bytes / (int64_t)sizeof(T);             // per-latent scratch stride in elements (bytes is a multiple of 16)
  hipStream_t st = (hipStream_t)stream;
  const T *V = A_src + nps, *W = A_src + wcs;
  // Bt = V^T W: A operand V (K x 128), B operand W (K x n_pad, lower: only k >= 128 jb is walked)
  int rc = FxGemm<T>::tn(PLMC_TRI_B_LOWER, NB, (int)nps, (int)nps, V, lds, strideS, W, lds, strideS, Bt, nps, sstr, q, stream);
  if (rc != 0) return rc;
  rc = FxGemm<T>::tn(0, NB, NB, (int)nps, V, lds, strideS, V, lds, strideS, G, NB, sstr, q, stream);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(k_fx_prep<T>, dim3((unsigned)(nps / NB), q), dim3(NTHREADS), 0, st, K22, m, (const T *)G, S64, V64, W64, Bt, nps, L.bytes);
  hipLaunchKernelGGL((k_diag<double>), dim3(q), dim3(DIAG_NT), 0, st, S64, (int64_t)NB, L.bytes / 8, 0, V64, L.bytes / 8, W64, (int64_t)NB, L.bytes / 8);
  if (!in_place) {
    const int mbd = (int)(npd / NB);
    hipLaunchKernelGGL(k_fx_copy<T>, dim3((unsigned)(mbd * mbd), 2, q), dim3(NTHREADS), 0, st, A_src, lds, wcs, strideS, (int)(nps / NB), A_dst, ldd, wcd,
                       strideD, mbd, n);
  }
  hipLaunchKernelGGL(k_fx_fin<T>, dim3(q), dim3(NTHREADS), 0, st, (const double *)S64, (const double *)W64, W22t, L.bytes, A_dst, ldd, wcd, strideD, n, m,
                     logdet, info);
  rc = launch_status(__func__);
  if (rc != 0) return rc;
  // Tm = W22 Bt: A operand W22t (K = 128 x 128), B operand Bt (K = 128 x n_pad)
  rc = FxGemm<T>::tn(0, NB, (int)nps, NB, W22t, NB, sstr, Bt, nps, sstr, Tm, nps, sstr, q, stream);
  if (rc != 0) return rc;
  const int64_t total = (int64_t)n * m;
  const unsigned gx = (unsigned)((total + NTHREADS - 1) / NTHREADS < 2048 ? (total + NTHREADS - 1) / NTHREADS : 2048);
  hipLaunchKernelGGL(k_fx_border<T>, dim3(gx, q), dim3(NTHREADS), 0, st, A_src, lds, nps, strideS, (const T *)Tm, L.bytes, A_dst, ldd, wcd, strideD, n, m);
  if (wcd > npd) hipLaunchKernelGGL(k_fx_zero_aug<T>, dim3((unsigned)npd, q), dim3(NTHREADS), 0, st, A_dst, ldd, npd, wcd, strideD);
  return launch_status(__func__);
}

}  // namespace plmc

extern "C" {
int64_t plmc_factor_extend_scratch_bytes(int64_t n_pad, int m, int elem_bytes) {
  if (n_pad <= 0 || n_pad % plmc::NB != 0 || m < 1 || m > plmc::NB || (elem_bytes != 4 && elem_bytes != 8)) return -1;
  return plmc::FxScratch(n_pad, elem_bytes).bytes;
}
int plmc_factor_extend_f32(const float *A_src, int n, int64_t n_pad_src, int64_t lda_src, int64_t wcol0_src, int64_t strideA_src, int m, const float *K22,
                           float *A_dst, int64_t n_pad_dst, int64_t lda_dst, int64_t wcol0_dst, int64_t strideA_dst, double *logdet, int *info,
                           void *scratch, int q, void *stream) {
  return plmc::factor_extend_impl<float>(A_src, n, n_pad_src, lda_src, wcol0_src, strideA_src, m, K22, A_dst, n_pad_dst, lda_dst, wcol0_dst, strideA_dst,
                                         logdet, info, scratch, q, stream);
}
int plmc_factor_extend_f64(const double *A_src, int n, int64_t n_pad_src, int64_t lda_src, int64_t wcol0_src, int64_t strideA_src, int m, const double *K22,
                           double *A_dst, int64_t n_pad_dst, int64_t lda_dst, int64_t wcol0_dst, int64_t strideA_dst, double *logdet, int *info,
                           void *scratch, int q, void *stream) {
  return plmc::factor_extend_impl<double>(A_src, n, n_pad_src, lda_src, wcol0_src, strideA_src, m, K22, A_dst, n_pad_dst, lda_dst, wcol0_dst, strideA_dst,
                                          logdet, info, scratch, q, stream);
}
}
