// kinv_epilogue_sm.inc -- gradient epilogue of one 128 x 128 tile (ib, jb) of K^-1 held in `acc` for a SPECTRAL-MIXTURE kernel
//     K = sum_m w_m exp(-2 pi^2 sum_k s_mk^2 tau_k^2) prod_k cos(2 pi mu_mk tau_k) + noise I          (covariance.hpp);
// textually included where kinv_epilogue_add.inc is (k_kinv_grad_add, kinv_tile_epilogue_add) when their family F is COV_SM.
// Names it expects in scope: those of kinv_epilogue_add.inc with ncomp = the number of mixture components, ell = the scales and oscale =
// the weights (or null), plus `means` and the compile-time dimension capacity DC (1, 4 or 8; d <= DC).
// Per element and component: the d phases are reduced in revolutions (sm_phase) and go through the hardware sine / cosine; the
// derivative of the cosine product with respect to mu_k is sin_k times the product of the OTHER cosines, formed from prefix and suffix
// products -- no division, finite where a cosine is exactly 0.  Sums of one component, in the tile's row of GP slots:
//     [0, SM_MAX_DIM) d/d s_k | [SM_MAX_DIM, 2 SM_MAX_DIM) d/d mu_k | [MAX_DIM] d/d noise (component 0) | [MAX_DIM + 1] d/d w
// without the constant factors -4 pi^2 and -2 pi (k_reduce_grad_add<T, true>).
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
  T *psc = aj + NB;                    // [SM_MAX_MIX][DC] scales (0 beyond d)
  T *pmu = psc + SM_MAX_MIX * DC;      // [SM_MAX_MIX][DC] means (0 beyond d)
  T *pwt = pmu + SM_MAX_MIX * DC;      // [SM_MAX_MIX] weights
  double *red = reinterpret_cast<double *>(pwt + SM_MAX_MIX);   // [4][GP] per-wave sums of the current component: 2 d + 2 of the GP slots
  static_assert(2 * SM_MAX_DIM + 2 <= GP && 2 * SM_MAX_DIM <= MAX_DIM && DC <= SM_MAX_DIM, "spectral-mixture gradient slots");
  static_assert((2 * NB * (SM_MAX_DIM + 1) + 2 * NB + SM_MAX_MIX * (2 * SM_MAX_DIM + 1)) * sizeof(T) + 4 * GP * sizeof(double) <=
                    tile_smem_elems<T>() * sizeof(T) && ((2 * NB * (DC + 1) + 2 * NB + SM_MAX_MIX * (2 * DC + 1)) * sizeof(T)) % 8 == 0,
                "spectral-mixture gradient epilogue LDS plan");
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
  if (tid < ncomp * DC) {
    const int g = tid / DC, k = tid % DC;
    psc[tid] = k < d ? ell[((int64_t)lat * ncomp + g) * d + k] : T(0);
    pmu[tid] = k < d ? means[((int64_t)lat * ncomp + g) * d + k] : T(0);
  }
  if (tid < ncomp) pwt[tid] = oscale ? oscale[(int64_t)lat * ncomp + tid] : T(1);
  double *out = partials + ((((int64_t)lat * m + ib) * m + jb) * ncomp) * GP;
#pragma unroll 1
  for (int g = 0; g < ncomp; ++g) {
    __syncthreads();                                   // staging done; the previous component's sums are out of `red`
    T sc[DC], mu[DC], gs[DC], gm[DC];
#pragma unroll
    for (int k = 0; k < DC; ++k) { sc[k] = psc[g * DC + k]; mu[k] = pmu[g * DC + k]; gs[k] = T(0); gm[k] = T(0); }
    const T wt = pwt[g];
    T g_noise = T(0), g_w = T(0);
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
          if (g == 0) {
            if (Kinv && gj >= gi) Kinv[(int64_t)lat * strideK + (int64_t)gi * ldk + gj] = kin;
            if (kinv_diag && gi == gj) kinv_diag[(int64_t)lat * n_pad + gi] = kin;
          }
          if (gi < n && gj < n && gj >= gi) {
            const T wij = a_i * aj[col] - kin;
            if (gi == gj) {                                  // tau = 0: value 1, every derivative but d/d w and d/d noise 0
              if (g == 0) g_noise += wij;
              g_w += wij;
            } else {
              const T *xjc = xj + col * ldu;
              T tau[DC], sn[DC], cs[DC], ex[DC];
              T e = T(0), pre = T(1);
#pragma unroll
              for (int k = 0; k < DC; ++k) {
                tau[k] = xir[k] - xjc[k];
                const T st = sc[k] * tau[k];
                e += st * st;
                sm_sincos_fast(sm_phase(xir[k], xjc[k], mu[k]), sn[k], cs[k]);
                ex[k] = pre;
                pre *= cs[k];
              }
              T suf = T(1);
#pragma unroll
              for (int k = DC - 1; k >= 0; --k) { ex[k] *= suf; suf *= cs[k]; }
              const T w2 = T(2) * wij;                       // symmetric pair (i,j),(j,i)
              const T env = fast_exp(T(-SM_2PI2) * e);
              g_w += w2 * (env * pre);
              const T cw = w2 * wt * env;
#pragma unroll
              for (int k = 0; k < DC; ++k) {
                gs[k] += (cw * pre) * (sc[k] * tau[k] * tau[k]);
                gm[k] += cw * (tau[k] * sn[k] * ex[k]);
              }
            }
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < SM_MAX_DIM; ++k) {
      const double s0 = wave_sum(k < DC ? (double)gs[k < DC ? k : 0] : 0.0), s1 = wave_sum(k < DC ? (double)gm[k < DC ? k : 0] : 0.0);
      if (lane == 0) { red[wave * GP + k] = s0; red[wave * GP + SM_MAX_DIM + k] = s1; }
    }
    {
      double s = wave_sum((double)g_noise);
      if (lane == 0) red[wave * GP + MAX_DIM] = s;
      s = wave_sum((double)g_w);
      if (lane == 0) red[wave * GP + MAX_DIM + 1] = s;
    }
    __syncthreads();
    if (live && tid < GP) {
      const bool used = tid < 2 * SM_MAX_DIM || tid >= MAX_DIM;       // the slots written above
      out[g * GP + tid] = used ? red[tid] + red[GP + tid] + red[2 * GP + tid] + red[3 * GP + tid] : 0.0;
    }
  }
