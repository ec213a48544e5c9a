// kinv_epilogue_dot.inc -- gradient epilogue of one 128 x 128 tile (ib, jb) of K^-1 held in `acc` for a DOT-PRODUCT kernel
//     K = os (c + sum_k v_k x_k x'_k)^P + noise I                                                                    (covariance.hpp);
// textually included where kinv_epilogue_add.inc is (k_kinv_grad_add, kinv_tile_epilogue_add) when their family F is COV_DOT.
// Names it expects in scope: those of kinv_epilogue_add.inc with ell = the variances v (q, d), `means` = the offset c (q), oscale (q) or
// null, ncomp = the power P, plus the compile-time dimension capacity DC (1, 4, 8 or 16; d <= DC).
// Per element, with s = c + sum_k v_k x_k x'_k:
//     d k / d v_k = os P s^(P - 1) x_k x'_k,     d k / d c = os P s^(P - 1),     d k / d os = s^P.
// The kernel is NOT stationary: the diagonal element (weight 1, the others of the upper triangle 2) carries k(x, x) = os s^P with
// s = c + sum_k v_k x_k^2 and contributes to EVERY sum, not to noise and os only.  No transcendental per element.
// Sums of the tile, in its row of GP slots:
//     [0, DOT_MAX_DIM) d/d v_k | [DOT_MAX_DIM] d/d c | [MAX_DIM] d/d noise | [MAX_DIM + 1] d/d os
// (k_reduce_grad_dot halves them).
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
  T *pv = aj + NB;                     // [DOT_MAX_DIM] v (0 beyond d)
  double *red = reinterpret_cast<double *>(pv + DOT_MAX_DIM);   // [4][GP] per-wave sums: d + 3 of the GP slots
  static_assert(DOT_MAX_DIM + 1 <= MAX_DIM && DC <= DOT_MAX_DIM, "dot-product gradient slots");
  static_assert((2 * NB * (DOT_MAX_DIM + 1) + 2 * NB + DOT_MAX_DIM) * sizeof(T) + 4 * GP * sizeof(double) <=
                    tile_smem_elems<T>() * sizeof(T) && ((2 * NB * (DC + 1) + 2 * NB + DOT_MAX_DIM) * sizeof(T)) % 8 == 0,
                "dot-product gradient epilogue LDS plan");
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
  if (tid < DOT_MAX_DIM) pv[tid] = tid < d ? ell[(int64_t)lat * d + tid] : T(0);
  __syncthreads();
  {
    T v[DC], gv[DC];
#pragma unroll
    for (int k = 0; k < DC; ++k) { v[k] = pv[k]; gv[k] = T(0); }
    const T os = oscale ? oscale[lat] : T(1);
    const T off = means[lat];
    const int P = ncomp;
    T g_noise = T(0), g_os = T(0), g_c = T(0);
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
            const T *xjc = xj + col * ldu;
            T pr[DC];
#pragma unroll
            for (int k = 0; k < DC; ++k) pr[k] = xir[k] * xjc[k];
            T val, dval;
            dot_value_deriv<T, DC>(pr, v, off, P, val, dval);
            const bool diag = gi == gj;
            const T wt = diag ? wij : T(2) * wij;            // the diagonal once, a symmetric pair (i,j),(j,i) twice
            g_noise += diag ? wij : T(0);
            g_os += wt * val;
            const T cb = wt * os * dval;
            g_c += cb;
#pragma unroll
            for (int k = 0; k < DC; ++k) gv[k] += cb * pr[k];
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < DOT_MAX_DIM; ++k) {
      const double s0 = wave_sum(k < DC ? (double)gv[k < DC ? k : 0] : 0.0);
      if (lane == 0) red[wave * GP + k] = s0;
    }
    {
      double s = wave_sum((double)g_c);
      if (lane == 0) red[wave * GP + DOT_MAX_DIM] = s;
      s = wave_sum((double)g_noise);
      if (lane == 0) red[wave * GP + MAX_DIM] = s;
      s = wave_sum((double)g_os);
      if (lane == 0) red[wave * GP + MAX_DIM + 1] = s;
    }
    __syncthreads();
    if (live && tid < GP) {
      const bool used = tid <= DOT_MAX_DIM || tid >= MAX_DIM;          // the slots written above
      double *out = partials + (((int64_t)lat * m + ib) * m + jb) * GP;
      out[tid] = used ? red[tid] + red[GP + tid] + red[2 * GP + tid] + red[3 * GP + tid] : 0.0;
    }
  }
