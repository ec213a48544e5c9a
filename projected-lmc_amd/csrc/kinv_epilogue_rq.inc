// kinv_epilogue_rq.inc -- gradient epilogue of one 128 x 128 tile (ib, jb) of K^-1 held in `acc` for a RATIONAL-QUADRATIC kernel
//     K = os (1 + r^2 / (2 alpha))^(-alpha) + noise I,   r^2 = sum_k ((x_k - x'_k) / ell_k)^2                       (covariance.hpp);
// textually included where kinv_epilogue_add.inc is (k_kinv_grad_add, kinv_tile_epilogue_add) when their family F is COV_RQ.
// Names it expects in scope: those of kinv_epilogue_add.inc with ell = the lengthscales (q, d), `means` = alpha (q), oscale (q) or null,
// plus the compile-time dimension capacity DC (1, 4, 8 or 16; d <= DC).  ncomp is 1 and not looked at.
// Per element, with u = r^2 / (2 alpha) and df_k = (x_k - x'_k) / ell_k from the RAW difference:
//     d k / d ell_k = k / (1 + u) df_k^2 / ell_k,     d k / d alpha = -k h(u),  h(u) = log1p(u) - u / (1 + u) (rq_h),     d k / d os = k / os.
// Sums of the tile, in its row of GP slots:
//     [0, RQ_MAX_DIM) d/d ell_k | [RQ_MAX_DIM] d/d alpha | [MAX_DIM] d/d noise | [MAX_DIM + 1] d/d os
// without the factor 1 / ell_k and the sign of d/d alpha (k_reduce_grad_rq).  The diagonal element has u = 0: noise and os only.
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  auto wave_sum = [&](double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
  };
  constexpr int ldu = DC + 1;
  T *xi = smem;                        // [128][ldu] raw inputs of the tile's rows, staged once
  T *xj = xi + NB * ldu;               // [128][ldu] ... and columns
  T *ai = xj + NB * ldu;               // [128]
  T *aj = ai + NB;                     // [128]
  T *pw = aj + NB;                     // [RQ_MAX_DIM] 1 / ell (0 beyond d)
  double *red = reinterpret_cast<double *>(pw + RQ_MAX_DIM);   // [4][GP] per-wave sums: d + 3 of the GP slots
  static_assert(RQ_MAX_DIM + 1 <= MAX_DIM && DC <= RQ_MAX_DIM, "rational-quadratic gradient slots");
  static_assert((2 * NB * (RQ_MAX_DIM + 1) + 2 * NB + RQ_MAX_DIM) * sizeof(T) + 4 * GP * sizeof(double) <=
                    tile_smem_elems<T>() * sizeof(T) && ((2 * NB * (DC + 1) + 2 * NB + RQ_MAX_DIM) * sizeof(T)) % 8 == 0,
                "rational-quadratic gradient epilogue LDS plan");
  __syncthreads();                     // every wave is done with the main loop's operands in `smem`
  for (int e = tid; e < NB * DC; e += NTHREADS) {
    const int r = e / DC, k = e % DC;
    const int gi = ib * NB + r, gj = jb * NB + r;
    xi[r * ldu + k] = (k < d && gi < n) ? X[(int64_t)gi * d + k] : T(0);
    xj[r * ldu + k] = (k < d && gj < n) ? X[(int64_t)gj * d + k] : T(0);
  }
  if (tid < NB) {
    ai[tid] = live ? alpha[(int64_t)lat * n_pad + ib * NB + tid] : T(0);
    aj[tid] = live ? alpha[(int64_t)lat * n_pad + jb * NB + tid] : T(0);
  }
  if (tid < RQ_MAX_DIM) pw[tid] = tid < d ? T(1) / ell[(int64_t)lat * d + tid] : T(0);
  __syncthreads();
  {
    T w[DC], gl[DC];
#pragma unroll
    for (int k = 0; k < DC; ++k) { w[k] = pw[k]; gl[k] = T(0); }
    const T os = oscale ? oscale[lat] : T(1);
    const T shape = means[lat], i2a = T(0.5) / shape;      // alpha of the kernel (`alpha` in scope is K^-1 y)
    T g_noise = T(0), g_os = T(0), g_al = T(0);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
#pragma unroll 1
      for (int r = 0; r < 4; ++r) {
        const int row = tile_row<T>(wm, mt, lane, r);
        const int gi = ib * NB + row;
        const T *xir = xi + row * ldu;
        const T a_i = ai[row];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          const int col = tile_col(wn, nt, lane);
          const int gj = jb * NB + col;
          const auto &av = acc.v[mt][nt];
          const T kin = r == 0 ? av[0] : (r == 1 ? av[1] : (r == 2 ? av[2] : av[3]));
          if (Kinv && gj >= gi) Kinv[(int64_t)lat * strideK + (int64_t)gi * ldk + gj] = kin;
          if (kinv_diag && gi == gj) kinv_diag[(int64_t)lat * n_pad + gi] = kin;
          if (gi < n && gj < n && gj >= gi) {
            const T wij = a_i * aj[col] - kin;
            if (gi == gj) {                                  // u = 0: value os, every derivative but d/d os and d/d noise 0
              g_noise += wij;
              g_os += wij;
            } else {
              const T *xjc = xj + col * ldu;
              T df2[DC];
              T r2 = T(0);
#pragma unroll
              for (int k = 0; k < DC; ++k) {
                const T sd = (xir[k] - xjc[k]) * w[k];
                df2[k] = sd * sd;
                r2 += df2[k];
              }
              T val, base, vh;
              rq_value_base_h(r2, shape, i2a, val, base, vh);
              const T w2 = T(2) * wij;                       // symmetric pair (i,j),(j,i)
              g_os += w2 * val;
              const T cw = w2 * os;
              g_al += cw * vh;
              const T cb = cw * base;
#pragma unroll
              for (int k = 0; k < DC; ++k) gl[k] += cb * df2[k];
            }
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < RQ_MAX_DIM; ++k) {
      const double s0 = wave_sum(k < DC ? (double)gl[k < DC ? k : 0] : 0.0);
      if (lane == 0) red[wave * GP + k] = s0;
    }
    {
      double s = wave_sum((double)g_al);
      if (lane == 0) red[wave * GP + RQ_MAX_DIM] = s;
      s = wave_sum((double)g_noise);
      if (lane == 0) red[wave * GP + MAX_DIM] = s;
      s = wave_sum((double)g_os);
      if (lane == 0) red[wave * GP + MAX_DIM + 1] = s;
    }
    __syncthreads();
    if (live && tid < GP) {
      const bool used = tid <= RQ_MAX_DIM || tid >= MAX_DIM;           // the slots written above
      double *out = partials + (((int64_t)lat * m + ib) * m + jb) * GP;
      out[tid] = used ? red[tid] + red[GP + tid] + red[2 * GP + tid] + red[3 * GP + tid] : 0.0;
    }
  }
