// kinv_epilogue_sum.inc -- gradient epilogue of one 128 x 128 tile (ib, jb) of K^-1 held in `acc` for a HETEROGENEOUS SUM
//     K = sum_g os_g k_{fam[g]}(x, x'; theta_g) + noise I                                                  (api_common.hpp, CovTable SUM);
// textually included where kinv_epilogue_add.inc is (k_kinv_grad_add, kinv_tile_epilogue_add, k_loo_grad_add) when their family F is
// COV_SUM.  Names it expects in scope: those of kinv_epilogue_add.inc with `kind` = the members' 4-bit codes (component g in bits
// 4 g .. 4 g + 3), ell = the table (q, ncomp, 3 d + 1) of records [ell | period | rbf_ell: d each | alpha], oscale (q, ncomp) or null,
// plus the compile-time dimension capacity DC (1, 4 or 8; d <= DC).  A one-component sum never comes here (it is its member's family).
// The weight w_ij = alpha_i alpha_j - Kinv_ij, the tile in `acc` and the RAW inputs of its rows and columns (staged once) are shared by
// all components.  The tile is walked once per component (a real loop: the registers are those of the largest body, not their sum) with
// a wave-uniform switch between two bodies:
//   radial    the stationary ARD kinds and the rational quadratic: r^2 from the raw differences scaled by 1 / ell (exactly 0 for a
//             dimension with ell = +inf); value and base from kern_value_base_fast resp. rq_value_base_h, as their own epilogues
//   periodic  the periodic and the locally periodic kernel: the body of kinv_epilogue_lper.inc, with 1 / rbf_ell = 0 and the fast
//             exponential of kinv_epilogue_per.inc for the periodic kernel (its exponent is bounded), the accurate one for the product
// Each pass writes its family's slot layout into the component's row of GP partial sums (k_reduce_grad_sum):
//   radial    [0, 8) d/d ell_k | [RQ_MAX_DIM] d/d alpha | [MAX_DIM] d/d noise | [MAX_DIM + 1] d/d os
//   periodic  [0, 8) d/d ell_k | [8, 16) d/d p_k | [16, 24) d/d rbf_ell_k | [MAX_DIM] d/d noise | [MAX_DIM + 1] d/d os
// without the factors the families' reductions apply.  K^-1 and its diagonal are stored by the first pass only; d/d noise is read from
// the first row only.  The diagonal element has tau = 0: every member's value is 1 there, noise and os only.
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
  T *pip = aj + NB;                    // [SUM_MAX_DIM] 1 / p of the current component (0 beyond d and for a radial member)
  T *pir = pip + SUM_MAX_DIM;          // [SUM_MAX_DIM] its residual
  T *pw = pir + SUM_MAX_DIM;           // [SUM_MAX_DIM] 1 / ell (0 beyond d)
  T *pv = pw + SUM_MAX_DIM;            // [SUM_MAX_DIM] 1 / rbf_ell (0 beyond d and for every member but the locally periodic one)
  double *red = reinterpret_cast<double *>(pv + SUM_MAX_DIM);  // [4][GP] per-wave sums of the current component
  static_assert(SUM_MAX_DIM == 8 && 3 * SUM_MAX_DIM <= MAX_DIM && RQ_MAX_DIM + 1 <= MAX_DIM && MAX_DIM + 2 <= GP && DC <= SUM_MAX_DIM,
                "sum gradient slots");
  static_assert((2 * NB * (SUM_MAX_DIM + 1) + 2 * NB + 4 * SUM_MAX_DIM) * sizeof(T) + 4 * GP * sizeof(double) <=
                    tile_smem_elems<T>() * sizeof(T) && ((2 * NB * (DC + 1) + 2 * NB + 4 * SUM_MAX_DIM) * sizeof(T)) % 8 == 0,
                "sum gradient epilogue LDS plan");
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
  double *out = partials + ((((int64_t)lat * m + ib) * m + jb) * ncomp) * GP;
#pragma unroll 1
  for (int g = 0; g < ncomp; ++g) {
    const int f = (kind >> (4 * g)) & 15;
    const bool periodic = f == F_PER || f == F_LPER;
    const T *rec = ell + ((int64_t)lat * ncomp + g) * (3 * d + 1);
    const T os = oscale ? oscale[(int64_t)lat * ncomp + g] : T(1);
    const bool store = g == 0;
    __syncthreads();                   // the previous component's walk and its sums are done with the parameters and `red`
    if (tid < SUM_MAX_DIM) {
      T ip = T(0), ipr = T(0);
      if (tid < d && periodic) per_inv_period(rec[d + tid], ip, ipr);
      pip[tid] = ip;
      pir[tid] = ipr;
      pw[tid] = tid < d ? T(1) / rec[tid] : T(0);
      pv[tid] = (tid < d && f == F_LPER) ? T(1) / rec[2 * d + tid] : T(0);
    }
    __syncthreads();
    T g_noise = T(0), g_os = T(0);
    if (periodic) {
      T ip[DC], ipr[DC], w[DC], v[DC], gl[DC], gp[DC], gr[DC];
#pragma unroll
      for (int k = 0; k < DC; ++k) { ip[k] = pip[k]; ipr[k] = pir[k]; w[k] = pw[k]; v[k] = pv[k]; gl[k] = T(0); gp[k] = T(0); gr[k] = T(0); }
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
            if (store) {
              if (Kinv && gj >= gi) Kinv[(int64_t)lat * strideK + (int64_t)gi * ldk + gj] = kin;
              if (kinv_diag && gi == gj) kinv_diag[(int64_t)lat * n_pad + gi] = kin;
            }
            if (gi < n && gj < n && gj >= gi) {
              const T wij = a_i * aj[col] - kin;
              if (gi == gj) {
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
                // symmetric pair (i,j),(j,i); omc = 2 sin^2(pi f)
                const T kw = (T(2) * wij) * (f == F_LPER ? lper_exp(T(0.5) * e, r2) : fast_exp(-e));
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
      for (int k = 0; k < SUM_MAX_DIM; ++k) {
        const double s0 = wave_sum(k < DC ? (double)gl[k < DC ? k : 0] : 0.0), s1 = wave_sum(k < DC ? (double)gp[k < DC ? k : 0] : 0.0),
                     s2 = wave_sum(k < DC ? (double)gr[k < DC ? k : 0] : 0.0);
        if (lane == 0) {
          red[wave * GP + k] = s0;
          red[wave * GP + SUM_MAX_DIM + k] = s1;
          red[wave * GP + 2 * SUM_MAX_DIM + k] = s2;
        }
      }
    } else {
      T w[DC], gl[DC];
#pragma unroll
      for (int k = 0; k < DC; ++k) { w[k] = pw[k]; gl[k] = T(0); }
      const bool is_rq = f == F_RQ;
      const T shape = is_rq ? rec[3 * d] : T(1), i2a = T(0.5) / shape;       // alpha of the kernel (`alpha` in scope is K^-1 y)
      T g_al = T(0);
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
            if (store) {
              if (Kinv && gj >= gi) Kinv[(int64_t)lat * strideK + (int64_t)gi * ldk + gj] = kin;
              if (kinv_diag && gi == gj) kinv_diag[(int64_t)lat * n_pad + gi] = kin;
            }
            if (gi < n && gj < n && gj >= gi) {
              const T wij = a_i * aj[col] - kin;
              if (gi == gj) {
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
                T val, base, vh = T(0);
                if (is_rq) rq_value_base_h(r2, shape, i2a, val, base, vh);
                else kern_value_base_fast(f, r2, val, base);
                const T w2 = T(2) * wij;                     // symmetric pair (i,j),(j,i)
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
      for (int k = 0; k < SUM_MAX_DIM; ++k) {
        const double s0 = wave_sum(k < DC ? (double)gl[k < DC ? k : 0] : 0.0);
        if (lane == 0) {
          red[wave * GP + k] = s0;
          red[wave * GP + SUM_MAX_DIM + k] = 0.0;
          red[wave * GP + 2 * SUM_MAX_DIM + k] = 0.0;
        }
      }
      const double s = wave_sum((double)g_al);
      if (lane == 0) red[wave * GP + RQ_MAX_DIM] = s;
    }
    {
      double s = wave_sum((double)g_noise);
      if (lane == 0) red[wave * GP + MAX_DIM] = s;
      s = wave_sum((double)g_os);
      if (lane == 0) red[wave * GP + MAX_DIM + 1] = s;
    }
    __syncthreads();
    if (live && tid < GP) {
      const bool used = tid < 3 * SUM_MAX_DIM || tid >= MAX_DIM;       // the slots written above
      out[g * GP + tid] = used ? red[tid] + red[GP + tid] + red[2 * GP + tid] + red[3 * GP + tid] : 0.0;
    }
  }
