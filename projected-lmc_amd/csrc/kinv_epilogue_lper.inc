// kinv_epilogue_lper.inc -- gradient epilogue of one 128 x 128 tile (ib, jb) of K^-1 held in `acc` for a LOCALLY PERIODIC kernel
//     K = os exp(-2 sum_k sin^2(pi tau_k / p_k) / ell_k - 1/2 sum_k (tau_k / lam_k)^2) + noise I                    (covariance.hpp);
// textually included where kinv_epilogue_add.inc is (k_kinv_grad_add, kinv_tile_epilogue_add) when their family F is COV_LPER.
// Names it expects in scope: those of kinv_epilogue_add.inc with ell = the periodic lengthscales, `means` = the periods, `third` = the RBF
// lengthscales (q, d each), oscale (q) or null, plus the compile-time dimension capacity DC (1, 4 or 8; d <= DC).  ncomp is 1 and not
// looked at.
// Per element the d phases f_k = tau_k / p_k are reduced in revolutions (per_phase) and go through the hardware sine; the RBF exponent
// comes from the raw differences scaled by 1 / lam_k, and the summed exponent goes through ONE accurate exponential: unlike the periodic
// exponent (<= 2 d / ell) it is not bounded, and d / d lam weighs every term by the exponent once more, which is the case the
// rational-quadratic epilogue makes for dexp over __expf (error |a| 2^-24).
//     d k / d ell_k = k (1 - cos 2 pi f_k) / ell_k^2,     d k / d p_k = k 2 pi sin(2 pi f_k) tau_k / (ell_k p_k^2),
//     d k / d lam_k = k (tau_k / lam_k)^2 / lam_k,        d k / d os = k / os.
// Sums of the tile, in its row of GP slots:
//     [0, 8) d/d ell_k | [8, 16) d/d p_k | [16, 24) d/d lam_k | [MAX_DIM] d/d noise | [MAX_DIM + 1] d/d os
// without the factors 1 / ell_k^2, 2 pi / (ell_k p_k^2) and 1 / lam_k (k_reduce_grad_lper).  The diagonal element has tau = 0: noise and
// os only.
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
  T *pip = aj + NB;                    // [LPER_MAX_DIM] 1 / p (0 beyond d)
  T *pir = pip + LPER_MAX_DIM;         // [LPER_MAX_DIM] its residual (0 beyond d)
  T *pw = pir + LPER_MAX_DIM;          // [LPER_MAX_DIM] 1 / ell (0 beyond d)
  T *pv = pw + LPER_MAX_DIM;           // [LPER_MAX_DIM] 1 / lam (0 beyond d)
  double *red = reinterpret_cast<double *>(pv + LPER_MAX_DIM);  // [4][GP] per-wave sums: 3 d + 2 of the GP slots
  static_assert(LPER_MAX_DIM == 8 && 3 * LPER_MAX_DIM <= MAX_DIM && MAX_DIM + 2 <= GP && DC <= LPER_MAX_DIM,
                "locally periodic gradient slots");
  static_assert((2 * NB * (LPER_MAX_DIM + 1) + 2 * NB + 4 * LPER_MAX_DIM) * sizeof(T) + 4 * GP * sizeof(double) <=
                    tile_smem_elems<T>() * sizeof(T) && ((2 * NB * (DC + 1) + 2 * NB + 4 * LPER_MAX_DIM) * sizeof(T)) % 8 == 0,
                "locally periodic gradient epilogue LDS plan");
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
  if (tid < LPER_MAX_DIM) {
    T ip = T(0), ipr = T(0);
    if (tid < d) per_inv_period(means[(int64_t)lat * d + tid], ip, ipr);
    pip[tid] = ip;
    pir[tid] = ipr;
    pw[tid] = tid < d ? T(1) / ell[(int64_t)lat * d + tid] : T(0);
    pv[tid] = tid < d ? T(1) / third[(int64_t)lat * d + tid] : T(0);
  }
  __syncthreads();
  {
    T ip[DC], ipr[DC], w[DC], v[DC], gl[DC], gp[DC], gr[DC];
#pragma unroll
    for (int k = 0; k < DC; ++k) { ip[k] = pip[k]; ipr[k] = pir[k]; w[k] = pw[k]; v[k] = pv[k]; gl[k] = T(0); gp[k] = T(0); gr[k] = T(0); }
    const T os = oscale ? oscale[lat] : T(1);
    T g_noise = T(0), g_os = T(0);
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
            if (gi == gj) {                                  // tau = 0: value os, every derivative but d/d os and d/d noise 0
              g_noise += wij;
              g_os += wij;
            } else {
              const T *xjc = xj + col * ldu;
              T s2[DC], omc[DC], df2[DC];
              T e = T(0), r2 = T(0);
#pragma unroll
              for (int k = 0; k < DC; ++k) {
                per_sin_fast(per_phase(xir[k], xjc[k], ip[k], ipr[k]), s2[k], omc[k]);
                e += omc[k] * w[k];
                const T sd = (xir[k] - xjc[k]) * v[k];
                df2[k] = sd * sd;
                r2 += df2[k];
              }
              // symmetric pair (i,j),(j,i); k / os = exp(-sum_k (1 - cos 2 pi f_k) / ell_k - r2 / 2), omc = 2 sin^2(pi f)
              const T kw = (T(2) * wij) * lper_exp(T(0.5) * e, r2);
              g_os += kw;
              const T cw = kw * os;
#pragma unroll
              for (int k = 0; k < DC; ++k) {
                gl[k] += cw * omc[k];
                gp[k] += cw * (s2[k] * (xir[k] - xjc[k]));
                gr[k] += cw * df2[k];
              }
            }
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < LPER_MAX_DIM; ++k) {
      const double s0 = wave_sum(k < DC ? (double)gl[k < DC ? k : 0] : 0.0), s1 = wave_sum(k < DC ? (double)gp[k < DC ? k : 0] : 0.0),
                   s2 = wave_sum(k < DC ? (double)gr[k < DC ? k : 0] : 0.0);
      if (lane == 0) {
        red[wave * GP + k] = s0;
        red[wave * GP + LPER_MAX_DIM + k] = s1;
        red[wave * GP + 2 * LPER_MAX_DIM + k] = s2;
      }
    }
    {
      double s = wave_sum((double)g_noise);
      if (lane == 0) red[wave * GP + MAX_DIM] = s;
      s = wave_sum((double)g_os);
      if (lane == 0) red[wave * GP + MAX_DIM + 1] = s;
    }
    __syncthreads();
    if (live && tid < GP) {
      const bool used = tid < 3 * LPER_MAX_DIM || tid >= MAX_DIM;      // the slots written above
      double *out = partials + (((int64_t)lat * m + ib) * m + jb) * GP;
      out[tid] = used ? red[tid] + red[GP + tid] + red[2 * GP + tid] + red[3 * GP + tid] : 0.0;
    }
  }
