// kinv_epilogue.inc -- body of the gradient epilogue of one 128 x 128 tile (ib, jb) of K^-1 held in `acc`; textually included
// by k_kinv_grad (256 threads, potri_grad.hip) and by kinv_tile_epilogue (the halves of the 512-thread macro-tile kernel).
// Names it expects in scope: T, DCAP, SPLINE, acc, smem, tid (0..255), live, kind, ib, jb, lat, m, n_pad, alpha, X, n, d, ell,
// oscale, Kinv, ldk, strideK, kinv_diag, partials; and the macro PLMC_KINV_KEEP (bool expression: one pass over the tile with every
// lengthscale sum in registers, or one pass per 8 dimensions).
  // stage scaled inputs u = x / ell and alpha for the tile's rows and columns
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const T *el = ell + (int64_t)lat * d;
  const T os = oscale ? oscale[lat] : T(1);
  // per-lane partial sums over the lane's 64 tile elements stay in T (fp32 on the fp32 path: 64 terms,
  // relative error ~4e-6, far inside the fp32 gradient tolerance); everything across lanes, waves and
  // tiles is reduced in fp64.
  T g_noise = T(0), g_os = T(0);
  auto wave_sum = [&](double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
  };
  double *red;                                         // [4][GP] per-wave sums, reduced across waves at the end

  if constexpr (DCAP <= 8) {
    typedef GradLds<DCAP> L;
    T g[DCAP];
#pragma unroll
    for (int k = 0; k < DCAP; ++k) g[k] = T(0);
    static_assert(L::END <= tile_smem_elems<T>(), "gradient epilogue LDS plan");
    for (int e = tid; e < NB * DCAP; e += NTHREADS) {     // unused dimensions and rows beyond n are staged as zeros
      const int r = e / DCAP, k = e % DCAP;
      const int gi = ib * NB + r, gj = jb * NB + r;
      const T inv = k < d ? T(1) / el[k] : T(0);
      smem[L::UI + r * L::LDI + k] = (k < d && gi < n) ? X[(int64_t)gi * d + k] * inv : T(0);
      smem[L::UJ + r * L::LDI + k] = (k < d && gj < n) ? X[(int64_t)gj * d + k] * inv : T(0);
    }
    if (tid < NB) {
      smem[L::AI + tid] = live ? alpha[(int64_t)lat * n_pad + ib * NB + tid] : T(0);
      smem[L::AJ + tid] = live ? alpha[(int64_t)lat * n_pad + jb * NB + tid] : T(0);
    }
    __syncthreads();
    // `Kinv` alone (the input gradient of the MLL, input_grad.hip) does not change which instantiation sums a tile: the gradient
    // table is the same bits with and without it.  The interior instantiation does not look at Kinv, and every element of such a
    // tile lies above the diagonal: the tile is written here.
    const bool interior = ib < jb && (jb + 1) * NB <= n && !kinv_diag;
    if (interior && Kinv) {
      T *Kt = Kinv + (int64_t)lat * strideK + (int64_t)ib * NB * ldk + (int64_t)jb * NB;
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
          for (int r = 0; r < 4; ++r) Kt[(int64_t)tile_row<T>(wm, mt, lane, r) * ldk + tile_col(wn, nt, lane)] = acc.v[mt][nt][r];
    }
#define PLMC_GRAD_TILE(KIND, INT) \
  grad_tile_small<T, DCAP, KIND, INT>(acc, smem, tid, os, ib, jb, n, lat, n_pad, Kinv, ldk, strideK, kinv_diag, g, g_noise, g_os)
    if (interior) {
      if (kind == K_RBF) PLMC_GRAD_TILE(K_RBF, true);
      else if (kind == K_MATERN12) PLMC_GRAD_TILE(K_MATERN12, true);
      else if (kind == K_MATERN32) PLMC_GRAD_TILE(K_MATERN32, true);
      else if (kind == K_MATERN52) PLMC_GRAD_TILE(K_MATERN52, true);
      else PLMC_GRAD_TILE(K_SPLINE, false);            // rare kernel: one (predicated) instantiation serves all tiles
    } else {
      if (kind == K_RBF) PLMC_GRAD_TILE(K_RBF, false);
      else if (kind == K_MATERN12) PLMC_GRAD_TILE(K_MATERN12, false);
      else if (kind == K_MATERN32) PLMC_GRAD_TILE(K_MATERN32, false);
      else if (kind == K_MATERN52) PLMC_GRAD_TILE(K_MATERN52, false);
      else PLMC_GRAD_TILE(K_SPLINE, false);
    }
#undef PLMC_GRAD_TILE
    __syncthreads();                                   // the sums reuse the staging area
    red = reinterpret_cast<double *>(smem);
#pragma unroll
    for (int k = 0; k < DCAP; ++k) {
      const double s = wave_sum((double)g[k]);
      if (lane == 0) red[wave * GP + k] = s;
    }
  } else {
  // d > 8: general tile code.  mt / nt are unrolled (static accumulator indices); the register r inside an MFMA tile
  // is picked with a select chain -- a runtime-indexed accumulator would be demoted to scratch memory.
  // fp32 keeps the row's inputs, the squared differences and all DCAP lengthscale sums in registers (one pass over the
  // tile).  fp64 (64 accumulator doubles = 128 registers at 2 waves per SIMD) walks the tile once per group of GH = 8
  // dimensions with 8 sums live and reads the inputs from LDS where they are needed; the covariance value is
  // recomputed per pass.  Either way nothing is spilled.
  constexpr bool KEEP = PLMC_KINV_KEEP;
  constexpr int GH = KEEP ? DCAP : 8;
  constexpr int KD = KEEP ? DCAP : 1;
  const int ldu = d + 1;
  T *ui = smem;                        // [128][ldu]
  T *uj = ui + NB * ldu;               // [128][ldu]
  T *ai = uj + NB * ldu;               // [128]
  T *aj = ai + NB;                     // [128]
  red = reinterpret_cast<double *>(aj + NB);           // own area: filled pass by pass
  static_assert((2 * NB * (MAX_DIM + 1) + 2 * NB) * sizeof(T) + 4 * GP * sizeof(double) <= tile_smem_elems<T>() * sizeof(T),
                "general gradient epilogue LDS plan");
  for (int e = tid; e < NB * d; e += NTHREADS) {
    int r = e / d, k = e % d;
    int gi = ib * NB + r, gj = jb * NB + r;
    T inv = T(1) / el[k];
    ui[r * ldu + k] = gi < n ? X[(int64_t)gi * d + k] * inv : T(0);
    uj[r * ldu + k] = gj < n ? X[(int64_t)gj * d + k] * inv : T(0);
  }
  if (tid < NB) {
    ai[tid] = live ? alpha[(int64_t)lat * n_pad + ib * NB + tid] : T(0);
    aj[tid] = live ? alpha[(int64_t)lat * n_pad + jb * NB + tid] : T(0);
  }
  __syncthreads();
#pragma unroll 1
  for (int k0 = 0; k0 < DCAP; k0 += GH) {
    T g[GH];
#pragma unroll
    for (int k = 0; k < GH; ++k) g[k] = T(0);
    const bool first = k0 == 0;
    if (first || (k0 < d && !SPLINE)) {
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
#pragma unroll 1
        for (int r = 0; r < 4; ++r) {
          const int row = tile_row<T>(wm, mt, lane, r);
          const int gi = ib * NB + row;
          T xi[KD];
          const T *uir = ui + row * ldu;
          if constexpr (KEEP) {
#pragma unroll
            for (int k = 0; k < DCAP; ++k) xi[k] = k < d ? uir[k] : T(0);
          }
          const T a_i = ai[row];
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) {
            const int col = tile_col(wn, nt, lane);
            const int gj = jb * NB + col;
            const auto &av = acc.v[mt][nt];
            const T kin = r == 0 ? av[0] : (r == 1 ? av[1] : (r == 2 ? av[2] : av[3]));
            if (first) {
              if (Kinv && gj >= gi) Kinv[(int64_t)lat * strideK + (int64_t)gi * ldk + gj] = kin;
              if (kinv_diag && gi == gj) kinv_diag[(int64_t)lat * n_pad + gi] = kin;
            }
            if (gi < n && gj < n && gj >= gi) {
              const T wij = a_i * aj[col] - kin;
              const T *ujc = uj + col * ldu;
              T df2[KD];
              T r2 = T(0);
              if constexpr (KEEP) {
#pragma unroll
                for (int k = 0; k < DCAP; ++k) {
                  T df = k < d ? xi[k] - ujc[k] : T(0);
                  df2[k] = df * df;
                  r2 += df2[k];
                }
              } else {
#pragma unroll 4
                for (int k = 0; k < d; ++k) { const T df = uir[k] - ujc[k]; r2 += df * df; }
              }
              T val, base;
              if constexpr (SPLINE) {
                val = T(1);
                if constexpr (KEEP) {
#pragma unroll
                  for (int k = 0; k < DCAP; ++k) val *= k < d ? spline_factor(xi[k], ujc[k]) : T(1);
                } else {
#pragma unroll 4
                  for (int k = 0; k < d; ++k) val *= spline_factor(uir[k], ujc[k]);
                }
                base = T(0);
              } else {
                kern_value_base_fast(kind, r2, val, base);
              }
              if (gi == gj) {
                if (first) { g_noise += wij; g_os += wij * val; }
              } else {
                const T c = T(2) * wij * os * base;          // symmetric pair (i,j),(j,i)
                if constexpr (KEEP) {
#pragma unroll
                  for (int k = 0; k < DCAP; ++k) g[k] += c * df2[k];
                } else if constexpr (!SPLINE) {
#pragma unroll
                  for (int k = 0; k < GH; ++k) {
                    const T df = k0 + k < d ? uir[k0 + k] - ujc[k0 + k] : T(0);
                    g[k] += c * df * df;
                  }
                }
                if (first) g_os += T(2) * wij * val;
              }
            }
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < GH; ++k) {
      const double s = wave_sum((double)g[k]);
      if (lane == 0) red[wave * GP + k0 + k] = s;
    }
  }
  }

  // ---- noise / outputscale sums, then the reduction across the 4 waves
  {
    double s = wave_sum((double)g_noise);
    if (lane == 0) red[wave * GP + MAX_DIM] = s;
    s = wave_sum((double)g_os);
    if (lane == 0) red[wave * GP + MAX_DIM + 1] = s;
  }
  __syncthreads();
  double *out = partials + (((int64_t)lat * m + ib) * m + jb) * GP;
  if (live && tid < GP) {
    const bool used = tid < DCAP || tid >= MAX_DIM;
    out[tid] = used ? red[tid] + red[GP + tid] + red[2 * GP + tid] + red[3 * GP + tid] : 0.0;
  }
