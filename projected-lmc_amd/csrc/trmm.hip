// trmm.hip -- draws from a factorised covariance: the product of the factor's transpose with a block of base samples,
//     Y[b][i][j] = shift[b][i] + sum_{k <= i} U[b][k][i] Z[b][k][j],     i < n, j < ns, b < q          (plmc_trmm_ut_*)
// against the factor WHERE THE SWEEP LEFT IT.  U is the element-wise upper triangle of columns [0, n_pad) of a factor buffer; the part
// of a diagonal block below its diagonal holds whatever the input held, the tiles below the block diagonal were never written, rows and
// columns >= n hold padding: none of that is read.  Every element load goes to an address clamped INTO the live triangle
// (thin path: along the row, column max(i', k); wide path: along the column, row min(k, i'); i' = min(i, n - 1)) and the value is SELECTED (?:), never multiplied by a 0 mask, so a NaN in any of those
// places cannot reach Y.  Z and Y are K-major (q, n, ns) with arbitrary leading dimensions; Y is written for i < n, j < ns only.
//   thin (ns <= 16)  HBM-bound, the walk of k_wt_matvec (potrf.hip) on the other triangle: U is read once for all ns columns.
//   wide (ns > 16)   the tile engine's slab / fragment layout and MFMA loop (gemm_core.hpp tile_mainloop) behind element loaders.
// Both are deterministic: fixed summation order, no atomics.  The split engine does not serve this product.
#include "api_common.hpp"
#include "../../include/plmc.h"

namespace plmc {

// ---- thin path ------------------------------------------------------------------------------------------------------------------
// grid (n_cols / CW, q).  A workgroup takes CW columns of U and the rows k <= its last column; its 16 (CW = 128) or 8 waves are the
// row groups.  One wave
// reads 64 VW consecutive elements of ONE row per step when CW = 128 (VW = 2: a lane owns columns c and c + 64, two coalesced 4- or
// 8-byte loads) and 32 elements of TWO rows when CW = 32 (VW = 1, the half-waves take neighbouring rows), so the row index is
// wave-uniform: row k of Z -- one contiguous read of ns values -- comes through the scalar cache into SGPRs, not through a vector
// load per lane, and costs the vector memory path nothing.
// R rows of U are in flight per thread (64 bytes, what a thread of k_wt_matvec keeps in flight): unconditional loads from CLAMPED
// addresses -- row min(k, klast), column max(i', k) with i' = min(i, n - 1), always inside the live triangle -- and the value
// selected: a predicated load is a branch with a full wait behind it (README, round 4).  fp64 accumulators, VW x NSB per thread (ns rounded up to a power of two;
// the surplus columns repeat column ns - 1 and are not written).
// Rows go to the row groups in chunks of TRMM_C: group rg owns the rows k with (k / TRMM_C) % TRMM_NRG == rg, so the rows of Z a wave
// needs for one 128-row block are TRMM_C (CW = 32: 2 TRMM_C) CONSECUTIVE rows -- with ns = 1 that is one scalar-cache line, not one line
// per row (a group striding through the rows missed the scalar cache on every load).  FULL (ns == NSB, the usual case): the ns values
// of a row are read without the clamp on j, which lets the compiler merge them into wide scalar loads.
// CW = 128, or 32 where q * n_pad / 128 workgroups would leave CUs idle.  Either way a column's sum is built by the same TRMM_NRG row
// groups, each adding its rows in increasing order, and then added up in order: bit-identical results.
constexpr int TRMM_NRG = 16;
constexpr int TRMM_C = 8;
// keeps a wave-uniform value in an SGPR (an empty statement the optimiser cannot look through): without it the select between the two
// rows of a wave below becomes a select between their ADDRESSES and Z goes through a vector load per lane after all
template <typename T> __device__ __forceinline__ T in_sgpr(T x) {
  asm("" : "+s"(x));
  return x;
}
// The value of a load that has been issued, made opaque: the mask below is a select on the VALUE, and a value that is only used under a
// condition lets the optimiser sink its load into a branch on that condition -- a predicated load, one full round trip each (it did:
// 16 `s_cbranch_execz` / `s_waitcnt vmcnt(0)` pairs per pass, 12 to 48 times k_wt_matvec's time).  Placed where the value is consumed,
// behind the issue of every load of the pass, it costs the partial wait the consumer needs anyway.
template <typename T> __device__ __forceinline__ T loaded(T x) {
  asm volatile("" : "+v"(x));
  return x;
}
template <int CW> constexpr int TRMM_THREADS = CW == NB ? 64 * TRMM_NRG : 32 * TRMM_NRG;
template <typename T, int CW, int NSB, bool FULL>
__global__ __launch_bounds__(TRMM_THREADS<CW>) void k_trmm_ut_thin(const T *__restrict__ A, int64_t lda, int64_t strideA, int n,
                                                                   const T *__restrict__ Z, int ns, int64_t ldz, int64_t strideZ,
                                                                   const T *__restrict__ shift, T *__restrict__ Y, int64_t ldy,
                                                                   int64_t strideY) {
  static_assert(CW == NB || CW == 32, "column widths");
  constexpr int RW = CW == NB ? 1 : 2;             // rows one wave reads per step
  constexpr int VW = CW == NB ? 2 : 1;             // columns per lane
  // rows in flight per thread: 8 (64 bytes in fp32, what a thread of k_wt_matvec keeps in flight), 32 / 16 in the narrow workgroups
  // (128 bytes), whose longest column is walked by half the threads
  constexpr int R = CW == NB ? TRMM_C : 128 / (int)sizeof(T);
  static_assert(R % TRMM_C == 0, "whole chunks");
  constexpr int JC = CW == NB ? 2 : 8;             // columns of Y reduced per pass (32 KB of LDS either way)
  __shared__ double red[JC][TRMM_NRG][CW];
  const int lat = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int sub = RW == 2 ? lane >> 5 : 0;         // which of the wave's rows this lane reads
  const int c0 = RW == 2 ? lane & 31 : lane;
  const int rg = wave * RW + sub;
  const int colw = (gridDim.x - 1 - blockIdx.x) * CW;      // the longest columns are dispatched first
  const int klast = min(colw + CW - 1, n - 1);     // last row any column of this workgroup contracts
  const T *Ul = A + (int64_t)lat * strideA;
  const T *Zl = Z + (int64_t)lat * strideZ;
  int icol[VW];
  bool live[VW];
#pragma unroll
  for (int e = 0; e < VW; ++e) {
    const int i = colw + c0 + 64 * e;
    live[e] = i < n;
    icol[e] = live[e] ? i : n - 1;                 // clamped column: always inside the live triangle
  }
  double s[VW][NSB];
#pragma unroll
  for (int e = 0; e < VW; ++e)
#pragma unroll
    for (int j = 0; j < NSB; ++j) s[e][j] = 0.0;
  for (int k0 = 0; k0 <= klast; k0 += R * TRMM_NRG) {
    T v[R][VW];
#pragma unroll
    for (int u = 0; u < R; ++u) {
      // address = the wave's row (uniform, 64 bits, scalar registers) + a 32-bit byte offset per lane: one address register per load
      // instead of two (16 loads in flight: the difference between 128 registers and a spill at ns = 16).  Clamped along the ROW:
      // column max(i', k) of row k is on or right of the diagonal and, as k <= klast < n, inside the live triangle
      const int kw = k0 + (u / TRMM_C) * (TRMM_C * TRMM_NRG) + wave * RW * TRMM_C + u % TRMM_C;
      const int krow = min(kw, klast), k = min(kw + sub * TRMM_C, klast);      // krow <= k <= klast: never a row past the live ones
      const char *row = reinterpret_cast<const char *>(Ul + (int64_t)krow * lda);
#pragma unroll
      for (int e = 0; e < VW; ++e) {
        const unsigned off = ((unsigned)(k - krow) * (unsigned)lda + (unsigned)max(icol[e], k)) * (unsigned)sizeof(T);
        v[u][e] = *reinterpret_cast<const T *>(row + off);
      }
    }
#pragma unroll
    for (int u = 0; u < R; ++u) {
      const int kw = k0 + (u / TRMM_C) * (TRMM_C * TRMM_NRG) + wave * RW * TRMM_C + u % TRMM_C;   // wave-uniform: the row of sub = 0
      const T *z0 = Zl + (int64_t)min(kw, n - 1) * ldz, *z1 = Zl + (int64_t)min(kw + (RW - 1) * TRMM_C, n - 1) * ldz;
      T x[VW];
#pragma unroll
      for (int e = 0; e < VW; ++e) {
        const T raw = loaded(v[u][e]);
        x[e] = (live[e] && kw + sub * TRMM_C <= icol[e]) ? raw : T(0);     // a select: what lies outside k <= i < n never enters
      }
#pragma unroll
      for (int j = 0; j < NSB; ++j) {
        const int jc = FULL ? j : (j < ns ? j : ns - 1);
        T zz = z0[jc];
        if (RW == 2) {
          const T za = in_sgpr(zz), zb = in_sgpr(z1[jc]);
          zz = sub ? zb : za;
        }
#pragma unroll
        for (int e = 0; e < VW; ++e) s[e][j] += (double)x[e] * (double)zz;
      }
    }
  }
  // reduction over the row groups in order, JC columns of Y per pass; thread t adds up column t % CW of Y column j0 + t / CW
  const int rc = threadIdx.x % CW, rj = threadIdx.x / CW;
  const int ri = colw + rc;
  const double sh = (shift && ri < n) ? (double)shift[(int64_t)lat * n + ri] : 0.0;
#pragma unroll
  for (int j0 = 0; j0 < NSB; j0 += JC) {
    if (j0) __syncthreads();
#pragma unroll
    for (int jj = 0; jj < JC; ++jj)
      if (j0 + jj < NSB) {
#pragma unroll
        for (int e = 0; e < VW; ++e) red[jj][rg][c0 + 64 * e] = s[e][j0 + jj];
      }
    __syncthreads();
    const int j = j0 + rj;
    if (rj < JC && ri < n && j < ns) {
      double t = 0.0;
#pragma unroll
      for (int g = 0; g < TRMM_NRG; ++g) t += red[rj][g][rc];
      Y[(int64_t)lat * strideY + (int64_t)ri * ldy + j] = (T)(t + sh);
    }
  }
}

// ---- wide path ------------------------------------------------------------------------------------------------------------------
// grid (ceil(ns / 128), ceil(n / 128), q); tile (ib, jb) of Y contracts k in [0, 128 (ib + 1)) cut at n, as PLMC_TRI_A_UPPER does.
// The LDS slab layout, the fragment reads and the MFMA order are tile_mainloop's (gemm_core.hpp); only the way a slab reaches the
// registers differs -- tile_mainloop streams whole 128-column rows with buffer loads, which would read below the diagonal of the
// diagonal block and past n, and Z has neither the alignment nor the padding for them.  Here both operands come element by element
// from clamped addresses, without a branch (a "whole chunk is live: one 16-byte load" fast path cost a divergent branch and a full
// wait per chunk), and the values are selected on their way into LDS.  ns is padded to 128 in LDS, never in memory.
template <typename T>
__global__ __launch_bounds__(NTHREADS, TILE_MIN_WAVES<T>) void k_trmm_ut_wide(const T *__restrict__ A, int64_t lda, int64_t strideA, int n,
                                                                              const T *__restrict__ Z, int ns, int64_t ldz, int64_t strideZ,
                                                                              const T *__restrict__ shift, T *__restrict__ Y, int64_t ldy,
                                                                              int64_t strideY) {
  using Tr = Traits<T>;
  using vec_t = typename Tr::vec_t;
  constexpr int EPV = Tr::EPV;
  constexpr int CPR = NB / EPV;                    // 16-byte chunks per slab row
  constexpr int NCH = BK * CPR / NTHREADS;         // chunks per thread and operand (2 / 4)
  constexpr int RSTEP = NTHREADS / CPR;            // rows between a thread's chunks
  __shared__ __align__(16) T smem[tile_smem_elems<T>()];
  const int jb = blockIdx.x, ib = blockIdx.y, lat = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const T *Ul = A + (int64_t)lat * strideA;
  const T *Zl = Z + (int64_t)lat * strideZ;
  const int kend = min((ib + 1) * NB, n);          // contraction rows [0, kend)
  const int nkt = (kend + BK - 1) / BK;
  T *sA = smem, *sB = smem + SB_OFF;
  const int row0 = tid / CPR, col0 = (tid % CPR) * EPV;
  const int i0 = ib * NB + col0, j0 = jb * NB + col0;    // first column of this thread's chunks in U / in Z
  vec_t ra[NCH], rb[NCH];
  auto gload = [&](int kt) {
#pragma unroll
    for (int h = 0; h < NCH; ++h) {
      const int k = kt * BK + row0 + h * RSTEP;
#pragma unroll
      for (int e = 0; e < EPV; ++e) {
        const int i = i0 + e, ic = i < n ? i : n - 1, kc = k < ic ? k : ic;
        ra[h][e] = Ul[(int64_t)kc * lda + ic];
      }
      const T *zr = Zl + (int64_t)(k < n ? k : n - 1) * ldz;
#pragma unroll
      for (int e = 0; e < EPV; ++e) {
        const int j = j0 + e;
        rb[h][e] = zr[j < ns ? j : ns - 1];
      }
    }
  };
  // the masks, applied to the VALUES on their way into LDS (`loaded`: see the thin path): a select, never a product with 0
  auto mask = [&](int kt) {
#pragma unroll
    for (int h = 0; h < NCH; ++h) {
      const int k = kt * BK + row0 + h * RSTEP;
#pragma unroll
      for (int e = 0; e < EPV; ++e) {
        const T a = loaded(ra[h][e]), b = loaded(rb[h][e]);
        ra[h][e] = (k <= i0 + e && i0 + e < n) ? a : T(0);
        rb[h][e] = (k < n && j0 + e < ns) ? b : T(0);
      }
    }
  };
  // contraction row r = 4 ks + fk of a slab is LDS row 4 fk + ks, stride LDT (tile_mainloop)
  const int rp0 = (row0 & 3) * 4 + (row0 >> 2);
  T *swA = sA + rp0 * LDT + col0, *swB = sB + rp0 * LDT + col0;
  auto sstore = [&](int buf) {
#pragma unroll
    for (int h = 0; h < NCH; ++h) {
      *reinterpret_cast<vec_t *>(swA + buf * (BK * LDT) + h * (RSTEP / 4) * LDT) = ra[h];
      *reinterpret_cast<vec_t *>(swB + buf * (BK * LDT) + h * (RSTEP / 4) * LDT) = rb[h];
    }
  };
  const int fk = lane >> 4, fm = lane & 15;
  const T *pa0 = sA + fk * 4 * LDT + wm * 64 + fm, *pb0 = sB + fk * 4 * LDT + wn * 64 + fm;
  Acc<T> acc;
  acc.zero();
  gload(0);
  mask(0);
  sstore(0);
  __syncthreads();
  for (int kt = 0; kt < nkt; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nkt) gload(kt + 1);
    const T *pa = pa0 + buf * (BK * LDT), *pb = pb0 + buf * (BK * LDT);
#pragma unroll
    for (int ks = 0; ks < BK / 4; ++ks) {
      T a[4], b[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) a[t] = pa[ks * LDT + t * 16];
#pragma unroll
      for (int t = 0; t < 4; ++t) b[t] = pb[ks * LDT + t * 16];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc.v[mt][nt] = Tr::mfma(a[mt], b[nt], acc.v[mt][nt]);
    }
    if (kt + 1 < nkt) {
      mask(kt + 1);
      sstore(buf ^ 1);
    }
    __syncthreads();
  }
  // epilogue: + shift, the live part of the tile only
  T *Yl = Y + (int64_t)lat * strideY;
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = ib * NB + tile_row<T>(wm, mt, lane, r);
      if (i < n) {
        const T sh = shift ? shift[(int64_t)lat * n + i] : T(0);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          const int j = jb * NB + tile_col(wn, nt, lane);
          if (j < ns) Yl[(int64_t)i * ldy + j] = acc.v[mt][nt][r] + sh;
        }
      }
    }
}

template <typename T, int CW>
static void launch_thin(int nsb, dim3 grid, hipStream_t st, const T *A, int64_t lda, int64_t strideA, int n, const T *Z, int ns, int64_t ldz,
                        int64_t strideZ, const T *shift, T *Y, int64_t ldy, int64_t strideY) {
  const dim3 block(TRMM_THREADS<CW>);
#define PLMC_TRMM_THIN(NSB) \
  do { \
    if (ns == NSB) hipLaunchKernelGGL((k_trmm_ut_thin<T, CW, NSB, true>), grid, block, 0, st, A, lda, strideA, n, Z, ns, ldz, strideZ, shift, Y, ldy, strideY); \
    else hipLaunchKernelGGL((k_trmm_ut_thin<T, CW, NSB, false>), grid, block, 0, st, A, lda, strideA, n, Z, ns, ldz, strideZ, shift, Y, ldy, strideY); \
  } while (0)
  if (nsb == 1) PLMC_TRMM_THIN(1);
  else if (nsb == 2) PLMC_TRMM_THIN(2);
  else if (nsb == 4) PLMC_TRMM_THIN(4);
  else if (nsb == 8) PLMC_TRMM_THIN(8);
  else PLMC_TRMM_THIN(16);
#undef PLMC_TRMM_THIN
}

constexpr int TRMM_THIN_MAX = 16;                  // widest block of base samples the thin path takes

template <typename T>
int trmm_ut_impl(const T *A, int64_t n_pad, int64_t lda, int64_t strideA, int n, const T *Z, int ns, int64_t ldz, int64_t strideZ,
                 const T *shift, T *Y, int64_t ldy, int64_t strideY, int q, void *stream) {
  PLMC_REQUIRE(A && Z && Y, "null pointer");
  PLMC_REQUIRE(n >= 1 && ns >= 1 && q >= 1, "need n >= 1, ns >= 1, q >= 1");
  PLMC_REQUIRE(n_pad > 0 && n_pad % NB == 0 && n <= n_pad && lda >= n_pad, "need n <= n_pad, n_pad a multiple of plmc_block(), lda >= n_pad");
  PLMC_REQUIRE(ldz >= ns && ldy >= ns, "ldz and ldy must be at least ns");
  PLMC_REQUIRE(q == 1 || (strideA >= 0 && strideZ >= 0 && strideY >= (int64_t)(n - 1) * ldy + ns), "batch strides");
  {
    // the product is not in-place safe: a workgroup reads rows of Z that another has already overwritten
    const int64_t ez = (int64_t)(q - 1) * strideZ + (int64_t)(n - 1) * ldz + ns, ey = (int64_t)(q - 1) * strideY + (int64_t)(n - 1) * ldy + ns;
    const uintptr_t z0 = reinterpret_cast<uintptr_t>(Z), y0 = reinterpret_cast<uintptr_t>(Y);
    PLMC_REQUIRE(z0 + (uintptr_t)ez * sizeof(T) <= y0 || y0 + (uintptr_t)ey * sizeof(T) <= z0, "Y overlaps Z (the product is not in-place safe)");
  }
  hipStream_t st = (hipStream_t)stream;
  const int m = (n + NB - 1) / NB;                 // live block rows
  ProfScope ps(PK_TRMM, st, q * (double)n * n * ns, q * ((double)n * n / 2 + 2.0 * n * ns) * sizeof(T));
  if (ns <= TRMM_THIN_MAX) {
    int nsb = 1;
    while (nsb < ns) nsb *= 2;
    int cus = 0, dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 256;
    if ((int64_t)q * (n_pad / NB) < cus)
      launch_thin<T, 32>(nsb, dim3((unsigned)((n + 31) / 32), q), st, A, lda, strideA, n, Z, ns, ldz, strideZ, shift, Y, ldy, strideY);
    else
      launch_thin<T, NB>(nsb, dim3((unsigned)m, q), st, A, lda, strideA, n, Z, ns, ldz, strideZ, shift, Y, ldy, strideY);
  } else {
    hipLaunchKernelGGL(k_trmm_ut_wide<T>, dim3((unsigned)((ns + NB - 1) / NB), (unsigned)m, q), dim3(NTHREADS), 0, st, A, lda, strideA, n, Z, ns,
                       ldz, strideZ, shift, Y, ldy, strideY);
  }
  return launch_status(__func__);
}

}  // namespace plmc

extern "C" {
int plmc_trmm_ut_f32(const float *A, int64_t n_pad, int64_t lda, int64_t strideA, int n, const float *Z, int ns, int64_t ldz,
                     int64_t strideZ, const float *shift, float *Y, int64_t ldy, int64_t strideY, int q, void *stream) {
  return plmc::trmm_ut_impl<float>(A, n_pad, lda, strideA, n, Z, ns, ldz, strideZ, shift, Y, ldy, strideY, q, stream);
}
int plmc_trmm_ut_f64(const double *A, int64_t n_pad, int64_t lda, int64_t strideA, int n, const double *Z, int ns, int64_t ldz,
                     int64_t strideZ, const double *shift, double *Y, int64_t ldy, int64_t strideY, int q, void *stream) {
  return plmc::trmm_ut_impl<double>(A, n_pad, lda, strideA, n, Z, ns, ldz, strideZ, shift, Y, ldy, strideY, q, stream);
}
}
