// kinv_epilogue_add.inc -- gradient epilogue of one 128 x 128 tile (ib, jb) of K^-1 held in `acc` for an ADDITIVE kernel
// K = sum_g os_g k(|(x - x') / ell_g|) + noise I; textually included by k_kinv_grad_add (256 threads) and by kinv_tile_epilogue_add (the
// halves of the 512-thread macro-tile kernel), as kinv_epilogue.inc is by their single-kernel forms.
// Names it expects in scope: T, acc, smem, tid (0..255), live, kind (stationary), ncomp, ib, jb, lat, m, n_pad, alpha, X, n, d, ell
// (q, ncomp, d), oscale (q, ncomp) or null, Kinv, ldk, strideK, kinv_diag, partials (ncomp rows of GP doubles per tile).
// The weight w_ij = alpha_i alpha_j - Kinv_ij and the tile in `acc` are shared by all components; value, base and the squared
// differences are per component.  The tile is walked once per component and per 8 dimensions with 8 lengthscale sums live (the
// schedule of the fp64 path of kinv_epilogue.inc: nothing is spilled beside the 64 accumulator registers); the scaled inputs
// u = x / ell_g are restaged per component, so the element loop is the one of the single kernel.  1 / ell = 0 (a dimension outside the
// component) stages zeros: it adds nothing to the distance and its lengthscale sum is exactly 0.
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  auto wave_sum = [&](double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
  };
  const int ldu = d + 1;
  T *ui = smem;                        // [128][ldu]
  T *uj = ui + NB * ldu;               // [128][ldu]
  T *ai = uj + NB * ldu;               // [128]
  T *aj = ai + NB;                     // [128]
  double *red = reinterpret_cast<double *>(aj + NB);   // [4][GP] per-wave sums of the current component
  static_assert((2 * NB * (MAX_DIM + 1) + 2 * NB) * sizeof(T) + 4 * GP * sizeof(double) <= tile_smem_elems<T>() * sizeof(T),
                "additive gradient epilogue LDS plan");
  if (tid < NB) {
    ai[tid] = live ? alpha[(int64_t)lat * n_pad + ib * NB + tid] : T(0);
    aj[tid] = live ? alpha[(int64_t)lat * n_pad + jb * NB + tid] : T(0);
  }
  double *out = partials + ((((int64_t)lat * m + ib) * m + jb) * ncomp) * GP;
#pragma unroll 1
  for (int g = 0; g < ncomp; ++g) {
    const T *el = ell + ((int64_t)lat * ncomp + g) * d;
    const T os = oscale ? oscale[(int64_t)lat * ncomp + g] : T(1);
    __syncthreads();                                   // the previous component's walk and its sums are done with ui / uj / red
    for (int e = tid; e < NB * d; e += NTHREADS) {
      const int r = e / d, k = e % d;
      const int gi = ib * NB + r, gj = jb * NB + r;
      const T inv = T(1) / el[k];
      ui[r * ldu + k] = gi < n ? X[(int64_t)gi * d + k] * inv : T(0);
      uj[r * ldu + k] = gj < n ? X[(int64_t)gj * d + k] * inv : T(0);
    }
    __syncthreads();
    T g_noise = T(0), g_os = T(0);
#pragma unroll 1
    for (int k0 = 0; k0 < d; k0 += 8) {
      T gs[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) gs[k] = T(0);
      const bool first = k0 == 0;
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
#pragma unroll 1
        for (int r = 0; r < 4; ++r) {
          const int row = tile_row<T>(wm, mt, lane, r);
          const int gi = ib * NB + row;
          const T *uir = ui + row * ldu;
          const T a_i = ai[row];
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) {
            const int col = tile_col(wn, nt, lane);
            const int gj = jb * NB + col;
            const auto &av = acc.v[mt][nt];
            const T kin = r == 0 ? av[0] : (r == 1 ? av[1] : (r == 2 ? av[2] : av[3]));
            if (first && g == 0) {
              if (Kinv && gj >= gi) Kinv[(int64_t)lat * strideK + (int64_t)gi * ldk + gj] = kin;
              if (kinv_diag && gi == gj) kinv_diag[(int64_t)lat * n_pad + gi] = kin;
            }
            if (gi < n && gj < n && gj >= gi) {
              const T wij = a_i * aj[col] - kin;
              const T *ujc = uj + col * ldu;
              T r2 = T(0);
#pragma unroll 4
              for (int k = 0; k < d; ++k) { const T df = uir[k] - ujc[k]; r2 += df * df; }
              T val, base;
              kern_value_base_fast(kind, r2, val, base);
              if (gi == gj) {
                if (first) { g_noise += wij; g_os += wij * val; }
              } else {
                const T c = T(2) * wij * os * base;          // symmetric pair (i,j),(j,i)
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                  const T df = k0 + k < d ? uir[k0 + k] - ujc[k0 + k] : T(0);
                  gs[k] += c * df * df;
                }
                if (first) g_os += T(2) * wij * val;
              }
            }
          }
        }
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const double s = wave_sum((double)gs[k]);
        if (lane == 0) red[wave * GP + k0 + k] = s;
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
      const bool used = tid < ((d + 7) & ~7) || tid >= MAX_DIM;      // the slots this component's passes wrote
      out[g * GP + tid] = used ? red[tid] + red[GP + tid] + red[2 * GP + tid] + red[3 * GP + tid] : 0.0;
    }
  }
