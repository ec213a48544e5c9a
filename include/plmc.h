/*
 * plmc.h -- C ABI of the MI355X-native exact-GP hot path behind the projectedlmc model API.
 *
 * The reference (QWERTY6191/projected-lmc) has no FFI: its hot path is reached through
 * gpytorch calls made by its Python classes.  Each entry point below replaces the named
 * reference call site (file:line in /root/reference/projectedlmc/projected_lmc.py unless
 * stated) and the third-party kernels that call site triggers.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch types.  All pointers are DEVICE pointers
 *     owned by the caller (workspace included); the library allocates nothing and keeps no
 *     pointer after return.  Every call is asynchronous on `stream` (a hipStream_t passed as
 *     void*).  Return value: 0 = launched, <0 = argument / HIP error (see plmc_last_error()).
 *   - dtype by suffix: _f32 / _f64.  Everything row-major.
 *   - Blocked algorithms use NB = 128 (plmc_block()).  n_pad = plmc_pad(n) = n rounded up to NB.
 *   - "Factor buffer" A, one per latent GP (batch stride strideA elements):
 *        n_pad rows x lda columns, lda >= n_pad + naug_pad (+ n_pad when the inverse factor is
 *        requested), naug_pad = plmc_pad(naug) >= 0, lda a multiple of NB.
 *        columns [0, n_pad)               : UPPER triangle holds Khat = K + noise*I, then its factor U
 *                                           (Khat = U^T U); padded rows/cols hold the identity.
 *        columns [n_pad, n_pad+naug_pad)  : augmented right-hand sides (targets, cross-covariances);
 *                                           potrf turns each column c into U^-T c (forward solve for free).
 *        columns [n_pad+naug_pad, +n_pad) : (with_inverse) W = U^-T, LOWER triangle, produced by the same
 *                                           sweep (explicit zeros above the diagonal inside diagonal
 *                                           blocks; blocks strictly above the diagonal are never touched).
 *     The strictly lower triangle of the square part is never read.
 *   - Vd: per latent plmc_vd_blocks(n_pad, lda) blocks of NB x NB: the first n_pad/NB are the inverses of the diagonal
 *     blocks of U (upper), the rest is workspace of the sweep (the inverse triangle of the current group of block
 *     rows, its transposed copies and the panel buffers of the group's block rows).
 *   - "W, ldw, strideW" arguments below: pointer to the first W column of latent 0 inside the factor
 *     buffer (A + n_pad + naug_pad), ldw = lda, strideW = strideA -- or any buffer of that layout.
 *   - kernel kinds: PLMC_RBF, PLMC_MATERN12, PLMC_MATERN32, PLMC_MATERN52 (stationary ARD kernels on x / ell) and
 *     PLMC_SPLINE (the reference's SplineKernel, projected_lmc.py:26-36: no lengthscale -- pass ell = 1; accepted by
 *     plmc_assemble_*, plmc_assemble_cross_* and plmc_kinv_grad_* only).
 */
#ifndef PLMC_H
#define PLMC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { PLMC_RBF = 0, PLMC_MATERN12 = 1, PLMC_MATERN32 = 2, PLMC_MATERN52 = 3, PLMC_SPLINE = 4 };

/* Library identification / geometry. */
int         plmc_version(void);
int         plmc_block(void);                 /* NB (128) */
int64_t     plmc_pad(int64_t n);              /* n rounded up to a multiple of NB */
int         plmc_max_dim(void);               /* largest input dimension d accepted by the fused kernels */
const char *plmc_last_error(void);            /* text of the last error on the calling thread */
/* NB x NB blocks per latent the `Vd` argument of plmc_potrf_* must hold, for elements of `elem_bytes` (4 or 8) bytes.  The
 * sizes depend on (n_pad, lda, elem_bytes) only, never on the dev knobs (version 3: for 4-byte elements they always include
 * the plane buffers of the split engine, on or off; version 4: and, when lda has room for the inverse factor
 * (lda >= 2 n_pad), the full-height planes of W that plmc_kinv_grad_vd_* reads, 6 n_pad^2 bytes).
 * plmc_vd_blocks(n_pad, lda) = the 4-byte count (the larger one: safe for both).
 * ABI note: versions 1-3 sized Vd smaller -- a caller built against them must re-query (check plmc_version() == 4). */
int64_t     plmc_vd_blocks_for(int64_t n_pad, int64_t lda, int elem_bytes);
int64_t     plmc_vd_blocks(int64_t n_pad, int64_t lda);
/* ... for a plmc_potrf_ex_f32 call with with_inverse | 4 (the sweep KEEPS the 16-bit planes of every group's solved rows
 * instead of rolling over two buffers: plmc_potrs_aug_kept_f32 needs them); 4-byte elements only.  Such a sweep always works
 * in groups of 8 block rows (it ignores the dev knob PLMC_GRP: one kept buffer per 8 block rows is what this size reserves and
 * what plmc_potrs_aug_kept_f32 walks).  plmc_kinv_grad_vd_f32 accepts either scratch: the sweep records its per-latent stride. */
int64_t     plmc_vd_blocks_keep(int64_t n_pad, int64_t lda);
/* Offset, in floats from the start of one latent's Vd slice, of the block of scales a plmc_potrf_ex_f32 / plmc_factorize_ex_f32
 * sweep leaves there (4-byte elements; either Vd size above; per-latent stride = that latent's Vd blocks x NB^2 floats):
 *   [0..5]  the power-of-two scales of the split engine's six operand families (SU, SW, RU, RW, SA, RA; all 1 under PLMC_SPLIT=3),
 *   [6] [7] the largest diagonal entry D of the input and lambda = max(min(eig_lo, smallest diagonal entry), 1e-12 D),
 *   [104]   the number of planes of the scheme that wrote them (2 or 3), [105] the per-latent Vd stride in NB x NB blocks.
 * Read-only, for tests and diagnostics; plmc_potrs_aug_kept_f32 rewrites [4] and [5] for its new augmented columns. */
int64_t     plmc_split_scales_offset(int64_t n_pad, int64_t lda);
/* Bytes of the `partials` scratch plmc_kinv_grad_* needs for (n_pad, q): per-tile partial sums, and for 4-byte elements the
 * bf16 planes of W (6 q n_pad^2 bytes).  plmc_grad_scratch_bytes = the 4-byte size. */
int64_t     plmc_grad_scratch_bytes_for(int64_t n_pad, int q, int elem_bytes);
int64_t     plmc_grad_scratch_bytes(int64_t n_pad, int q);
/* ... and what plmc_kinv_grad_vd_* needs (the partial sums only: the planes of W come from the sweep's Vd). */
int64_t     plmc_grad_partials_bytes(int64_t n_pad, int q);

/*
 * Covariance assembly.  Replaces `self.covar_module(x)` (:316, :1090; kernels built by
 * handle_covar_ :151-167) fused with `likelihood(dist)` = +noise*I (:1200):
 *   A[i][j] = oscale * k(|x_i - x_j| / ell) + noise * (i==j)   for i <= j < n  (upper tiles)
 * X: n x d, ell: q x d, oscale: q or NULL, noise: q.
 */
int plmc_assemble_f32(int kind, const float *X, int n, int d, const float *ell, const float *oscale,
                      const float *noise, float *A, int64_t lda, int64_t strideA, int q, void *stream);
int plmc_assemble_f64(int kind, const double *X, int n, int d, const double *ell, const double *oscale,
                      const double *noise, double *A, int64_t lda, int64_t strideA, int q, void *stream);

/*
 * Write right-hand sides into the augmented block: A[i][n_pad + c0 + r] = rhs[latent][r][i]
 * (rhs: q x nrhs x n, e.g. the projected targets of project_data :1014-1021, which are q x n).
 * Rows >= n are zero.  With clear_cols > 0 the other columns of [n_pad, n_pad + clear_cols) are
 * zeroed too (pass naug_pad to reset the whole augmented block).
 */
int plmc_write_rhs_f32(const float *rhs, int nrhs, int n, float *A, int64_t lda, int64_t strideA,
                       int c0, int clear_cols, int q, void *stream);
int plmc_write_rhs_f64(const double *rhs, int nrhs, int n, double *A, int64_t lda, int64_t strideA,
                       int c0, int clear_cols, int q, void *stream);

/*
 * Cross-covariance block (prediction, ProjectedGPModel.__call__ eval branch :1133-1134 -> gpytorch
 * prediction strategy):  Out[i][col0 + j] = oscale * k(x_i, xs_j)  for i < n, j < ns; rows
 * n <= i < n_rows are zero-filled.  To fill the augmented block of a factor buffer pass Out = A,
 * ldo = lda, col0 = n_pad + c0, n_rows = n_pad; any other dense (n_rows x ldo) buffer works too.
 */
int plmc_assemble_cross_f32(int kind, const float *X, int n, const float *Xs, int ns, int d,
                            const float *ell, const float *oscale, float *Out, int64_t ldo,
                            int64_t strideO, int64_t col0, int64_t n_rows, int q, void *stream);
int plmc_assemble_cross_f64(int kind, const double *X, int n, const double *Xs, int ns, int d,
                            const double *ell, const double *oscale, double *Out, int64_t ldo,
                            int64_t strideO, int64_t col0, int64_t n_rows, int q, void *stream);

/*
 * Blocked right-looking Cholesky of the augmented buffer, Khat = U^T U, in place.
 * Replaces torch.linalg.cholesky_ex + the forward triangular solve behind
 * `latent_output.log_prob(proj_target)` (:1201) / ExactMarginalLogLikelihood (experiments.py:233).
 *   logdet[latent] = log det Khat   (double), info[latent] = 0 or 1 + index of first non-PD pivot
 *   (PLMC_INFO_CHAIN_ABORT: the resident chain kernel of the sweep gave up a bounded wait for another workgroup -- an internal
 *   error, never a property of the matrix; the results are then undefined.  Never observed; PLMC_CHAIN=0 selects the
 *   launch-per-step chain).
 * naug = number of live augmented columns (0 allowed).
 * with_inverse != 0: also produce W = U^-T in columns [n_pad + naug_pad, n_pad + naug_pad + n_pad)
 * (the identity rides along as further right-hand sides) -- the first half of the Khat^-1 that
 * `loss.backward()` needs (experiments.py:270).  No initialisation of those
 * columns is required.
 * with_inverse with bit 1 set (2, 3, ...) is refused before anything is launched: Khat^-1 and the gradient come from
 * plmc_kinv_grad_* behind the sweep.
 * The square part after the sweep: U is the ELEMENT-WISE upper triangle (i <= j) of columns [0, n_pad), padded rows i >= n
 * included -- those hold the identity exactly (1 on the diagonal, 0 right of it), and the padded rows of every augmented column
 * hold exactly 0.  Everything below the diagonal is unspecified: the 128 x 128 tiles strictly below the block diagonal are neither
 * read nor written, and the part of a diagonal block below its diagonal is loaded with the block (give it finite values: plmc_assemble_* fills the
 * whole block symmetrically) and left with whatever the input held -- W_kk, the inverse of a diagonal block, goes to Vd and to the W columns, never there.  W: tiles on
 * and below the block diagonal are written (zeros above the diagonal inside a diagonal block), the tiles above are never touched.
 * tests/test_gpu_factor.py pins all of this against an fp64 CPU factorisation.
 */
#define PLMC_INFO_CHAIN_ABORT 0x7ffffff0
int plmc_potrf_f32(float *A, int64_t n_pad, int64_t lda, int naug, int64_t strideA, float *Vd,
                   double *logdet, int *info, int with_inverse, int q, void *stream);
int plmc_potrf_f64(double *A, int64_t n_pad, int64_t lda, int naug, int64_t strideA, double *Vd,
                   double *logdet, int *info, int with_inverse, int q, void *stream);
/* The same with `eig_lo`: q lower bounds of the smallest eigenvalue of the input matrices (device pointer; for a GP
 * covariance K + s2 I the noise variances s2, since K is positive semi-definite).  Arithmetic of the BULK fp32 products
 * (tail / head updates, group panel; environment PLMC_SPLIT, default 2):
 *   2  two fp16 planes per operand, s x = h0 + 2^-11 h1 (22 bits), three plane products on v_mfma_f32_16x16x32_f16 into two
 *      fp32 accumulator levels.  Every operand family is scaled by a power of two that puts a rigorous bound of its
 *      magnitude -- from the largest diagonal entry D and eig_lo: sqrt(D), D, 1/sqrt(eig_lo), sqrt(D/eig_lo) -- at 2^13, so fp16
 *      cannot overflow; the augmented columns (no a-priori bound) stay on the fp32 MFMAs.  Needs eig_lo; without it ->
 *   3  three bf16 planes (x = hi + mid + lo exactly), six plane products, two accumulator levels: any data, no scaling.
 *   0  v_mfma_f32_16x16x4_f32 everywhere.
 * Either split has 0.3-0.45 x the error of the fp32 MFMA chain against fp64 (profiles/r03_split_numerics.txt).  The chain
 * (diagonal blocks, rank-128 updates), the panel columns of the next group and every fp64 product use the MFMA of the
 * element type.  A wrong (too large) eig_lo can overflow fp16: the result is then inf / nan and `info` reports it. */
int plmc_potrf_ex_f32(float *A, int64_t n_pad, int64_t lda, int naug, int64_t strideA, float *Vd, double *logdet,
                      int *info, int with_inverse, int q, const float *eig_lo, void *stream);
int plmc_potrf_ex_f64(double *A, int64_t n_pad, int64_t lda, int naug, int64_t strideA, double *Vd, double *logdet,
                      int *info, int with_inverse, int q, const double *eig_lo, void *stream);

/* Assembly + factorisation in one call (round 4): plmc_assemble_* followed by plmc_potrf_ex_* on the same buffers, with the
 * assembly overlapped with the sweep -- the sweep writes the rows of its first group of block rows on the caller's stream and
 * queues the other rows (and the scan of their diagonal for the fp16 scales; the first group's rows are scanned before its chain) on a helper stream beside that
 * group's chain; nothing reads them before.  The augmented columns must be in place BEFORE the call (plmc_write_rhs_*,
 * plmc_assemble_cross_*).  n_pad = plmc_pad(n).  Same kernels on the same data as the two separate calls: bit-identical results
 * (tests/test_gpu_engine.py).  Replaces, like them: `self.covar_module(x)` + `likelihood(dist)` + the Cholesky inside `log_prob`
 * (projected_lmc.py:316,:1090,:1200-1201). */
int plmc_factorize_ex_f32(int kind, const float *X, int n, int d, const float *ell, const float *oscale, const float *noise,
                          float *A, int64_t n_pad, int64_t lda, int naug, int64_t strideA, float *Vd, double *logdet, int *info,
                          int with_inverse, int q, const float *eig_lo, void *stream);
int plmc_factorize_ex_f64(int kind, const double *X, int n, int d, const double *ell, const double *oscale, const double *noise,
                          double *A, int64_t n_pad, int64_t lda, int naug, int64_t strideA, double *Vd, double *logdet, int *info,
                          int with_inverse, int q, const double *eig_lo, void *stream);

/*
 * Forward substitution of NEW augmented columns against a buffer that plmc_potrf_* already factorised with
 * with_inverse != 0 (and has not been modified since):  columns [n_pad, n_pad + naug) <- U^-T columns.  wcol0 = first
 * inverse-factor column of that factorisation (n_pad + plmc_pad(naug of the factorisation)); naug here may be smaller.
 * What an eval-mode model does on its second and later calls (projected_lmc.py:1133-1134: gpytorch's prediction strategy
 * keeps the factorisation across calls): n^2 naug flops instead of a new sweep.  Vd: the scratch of the factorisation
 * (its group workspace is reused).
 */
int plmc_potrs_aug_f32(float *A, int64_t n_pad, int64_t lda, int naug, int64_t wcol0, int64_t strideA, float *Vd, int q, void *stream);
int plmc_potrs_aug_f64(double *A, int64_t n_pad, int64_t lda, int naug, int64_t wcol0, int64_t strideA, double *Vd, int q, void *stream);
/* The same against a factorisation that kept its planes -- plmc_potrf_ex_f32(..., with_inverse | 4, ...) into a Vd of
 * plmc_vd_blocks_keep(n_pad, lda) blocks per latent: the group panels and the depth-1024 updates of the substitution then run on
 * the split engine too (A operand = the kept planes of the factor's rows; 2-3 x the fp32 MFMA rate of plmc_potrs_aug_f32).
 * eig_lo: NULL or not as in the factorising call (it selects the scheme; the values are not used).  fp64 and PLMC_SPLIT=0:
 * exactly plmc_potrs_aug_*. */
int plmc_potrs_aug_kept_f32(float *A, int64_t n_pad, int64_t lda, int naug, int64_t wcol0, int64_t strideA, float *Vd, int q,
                            const float *eig_lo, void *stream);
int plmc_potrs_aug_kept_f64(double *A, int64_t n_pad, int64_t lda, int naug, int64_t wcol0, int64_t strideA, double *Vd, int q,
                            const double *eig_lo, void *stream);

/*
 * Bordered update of a finished factorisation: condition a factor buffer WITH the inverse factor on m new rows without a new sweep
 * (gpytorch's get_fantasy_model [gpytorch-knowledge, unverified offline]).  Per latent, with Khat = U^T U, W = U^-T and the
 * bordered matrix [[Khat, K12], [K12^T, K22]]:
 *     V = W K12,  S = K22 - V^T V,  U22 = chol(S)^T,  W22 = U22^-T,  W21 = -W22 (W^T V)^T,
 *     U' = [[U, V], [0, U22]],  W' = [[W, 0], [W21, W22]],  logdet' = logdet + 2 sum log diag U22.
 * The caller has already run plmc_assemble_cross_* + plmc_potrs_aug[_kept]_* on the source, as a cached prediction does: the first m
 * augmented columns of the source hold V (rows >= n zero).  n <= n_pad_src live rows (n < n_pad_src: a factor inside a larger buffer
 * with identity padding).  K22: (q, m, m) dense, symmetric, noise and jitter on its diagonal.  1 <= m <= plmc_block(); the caller loops
 * for more.  n_pad_dst >= plmc_pad(n + m).  logdet: q doubles, in: that of the source, out: extended.  info: q ints, out: 0, or
 * 1 + n + k for the first pivot k of S that is not positive (that latent's new rows are then undefined; the others are not affected).
 * S and its pivots are carried in fp64 for both element types (k_diag<double> on the 128 x 128 block) and rounded once.
 * scratch: q * plmc_factor_extend_scratch_bytes(n_pad_src, m, element bytes) bytes, 16-byte aligned (it holds (W^T V)^T, V^T V, the
 * fp64 block and W21 before its sign); the size call returns -1 for arguments the entry point would refuse.
 * A_dst == A_src is allowed with identical geometry and n + m <= n_pad: the copy is skipped and rows [n, n + m) are written in place.
 * Any other overlap of the two buffers is refused.
 * Effect: A_dst satisfies the with-inverse post-condition of plmc_potrf_* for n + m live rows -- the element-wise upper triangle of
 * columns [0, n_pad_dst) is U' with exactly the identity on the padded rows; the W' tiles on and below the block diagonal are all
 * written, explicit zeros above the diagonal inside the diagonal blocks, the identity on its padded part; W tiles above the block
 * diagonal are never touched.  Of the source only the U tiles on and above and the W tiles on and below the block diagonal and the first
 * 128 augmented columns are read; its padding identity is not copied.  The destination's augmented block [n_pad_dst, wcol0_dst) is
 * zeroed (ready for plmc_write_rhs_*); its Vd is not an input of later plmc_potrs_aug_* calls and stays caller-allocated scratch (the
 * kept planes of plmc_potrs_aug_kept_f32 do NOT exist for an extended factor).  Everything runs on `stream`; fixed-order sums, no
 * atomics.  The O(n^2) part is the tile copy (HBM-bound, skipped in place); the rest is 3 products of one 128-column tile.
 */
int64_t plmc_factor_extend_scratch_bytes(int64_t n_pad, int m, int elem_bytes);
int plmc_factor_extend_f32(const float *A_src, int n, int64_t n_pad_src, int64_t lda_src, int64_t wcol0_src, int64_t strideA_src, int m,
                           const float *K22, float *A_dst, int64_t n_pad_dst, int64_t lda_dst, int64_t wcol0_dst, int64_t strideA_dst,
                           double *logdet, int *info, void *scratch, int q, void *stream);
int plmc_factor_extend_f64(const double *A_src, int n, int64_t n_pad_src, int64_t lda_src, int64_t wcol0_src, int64_t strideA_src, int m,
                           const double *K22, double *A_dst, int64_t n_pad_dst, int64_t lda_dst, int64_t wcol0_dst, int64_t strideA_dst,
                           double *logdet, int *info, void *scratch, int q, void *stream);

/*
 * Gather augmented column c of every latent into a contiguous vector z (q x n_pad) and return
 * quad[latent] = sum z^2 in double (the inv_quad term of MVN.log_prob, :1201).  All n_pad rows are copied; the sum is carried
 * in fp64.  Refused before anything is launched: a null pointer, q < 1, n_pad not a positive multiple of plmc_block(),
 * lda < n_pad, c < 0 or n_pad + c >= lda.
 */
int plmc_extract_col_f32(const float *A, int64_t n_pad, int64_t lda, int64_t strideA, int c,
                         float *z, double *quad, int q, void *stream);
int plmc_extract_col_f64(const double *A, int64_t n_pad, int64_t lda, int64_t strideA, int c,
                         double *z, double *quad, int q, void *stream);

/* alpha = W^T z = Khat^-1 y  (q x n_pad).  d logp / d y = -alpha.  Only the tiles of W on and below the block diagonal are read
 * (16-byte vector loads); each sum is carried in fp64 and rounded once.  Refused before anything is launched: a null pointer, q < 1,
 * n_pad not a positive multiple of plmc_block(), ldw < n_pad, W not 16-byte aligned, ldw or strideW not a multiple of 16 bytes. */
int plmc_wt_matvec_f32(const float *W, int64_t n_pad, int64_t ldw, int64_t strideW, const float *z,
                       float *alpha, int q, void *stream);
int plmc_wt_matvec_f64(const double *W, int64_t n_pad, int64_t ldw, int64_t strideW, const double *z,
                       double *alpha, int q, void *stream);

/*
 * Draws from a factorised covariance: Y = shift + U^T Z against the factor where the sweep left it -- the `L z` behind
 * `MultivariateNormal.rsample` [gpytorch-knowledge, unverified offline], which the reference's synthetic study begins with
 * (experiments.py:150-151, `MultivariateNormal(zeros, kernel(X)).sample()`):
 *     Y[b][i][j] = shift[b][i] + sum_{k <= i} U[b][k][i] Z[b][k][j]     for i < n, j < ns, b < q.
 * A: a factor buffer after plmc_potrf* / plmc_factorize*_ex (n_pad a multiple of plmc_block(), n <= n_pad <= lda); U is the ELEMENT-WISE
 *   upper triangle of its columns [0, n_pad).  Only U[k][i] with k <= i < n is read: nothing below the diagonal of a diagonal block
 *   (the sweep leaves the input there), nothing in the tiles below the block diagonal (never written), nothing in the augmented or W
 *   columns, nothing in rows or columns >= n.  The mask is a select on loads from addresses clamped into the live triangle, not a
 *   multiplication by 0: a NaN in any of those places does not reach Y.
 * Z, Y: K-major (q, n, ns) with leading dimensions ldz, ldy >= ns and batch strides strideZ, strideY (strideZ = 0 shares one Z); no
 *   alignment or padding is asked of them -- ns is padded to the tile inside the call.  Exactly Y[b][i][j] with i < n, j < ns is written.
 *   Y must not overlap Z (the product is not in-place safe).  shift: (q, n) contiguous, or NULL for 0.
 * Two paths, chosen from ns alone, both deterministic (fixed summation order, no atomics):
 *   ns <= 16  HBM-bound, the walk of plmc_wt_matvec_* on the other triangle: U is read once for all ns columns, fp64 accumulators;
 *   ns > 16   128 x 128 tiles on the matrix instructions of the element type, contraction range [0, 128 (ib + 1)) cut at n.
 * Per element |Y - exact| <= (i + 4) u (sum_{k <= i} |U_ki| |Z_kj| + |shift_i|), u = 2^-24 / 2^-53 (tests/_trmm_ref.py).
 * Argument errors (null A, Z or Y; n < 1, n > n_pad, ns < 1, q < 1; ldz < ns or ldy < ns; Y overlapping Z; a batch stride of Y that
 * lets two latents share elements) fail through plmc_last_error() before anything is launched.  q n^2 ns flop.
 */
int plmc_trmm_ut_f32(const float *A, int64_t n_pad, int64_t lda, int64_t strideA, int n, const float *Z, int ns, int64_t ldz,
                     int64_t strideZ, const float *shift, float *Y, int64_t ldy, int64_t strideY, int q, void *stream);
int plmc_trmm_ut_f64(const double *A, int64_t n_pad, int64_t lda, int64_t strideA, int n, const double *Z, int ns, int64_t ldz,
                     int64_t strideZ, const double *shift, double *Y, int64_t ldy, int64_t strideY, int q, void *stream);

/*
 * Batched "TN" product on the tile engine:  C[b] (=, +=, -=) A[b]^T B[b]  with A: K x M and B: K x N, both stored
 * K-major (row index = contraction index), C: M x N; mode 0 store / 1 add / 2 subtract.  M, N multiples of plmc_block(),
 * K a multiple of 16 (callers pad with zeros), 16-byte aligned pointers / leading dimensions / strides, lda >= M, ldb >= N,
 * ldc >= N.  strideA or strideB may be 0 (one operand shared by the batch); with batch > 1 the members of C must not share
 * elements: |strideC| >= (M - 1) ldc + N, anything else is refused before the launch like every other argument error.  Exactly
 * the M x N window of every C[b] is written.  Per element |C - exact| <= (K + 4) u (sum_k |A_ki| |B_kj| + |C0_ij|), u = 2^-24 / 2^-53,
 * the C0 term in modes 1 and 2 (tests/_gemm_ref.py).  Replaces the torch.matmul (rocBLAS)
 * calls of the Cholesky adjoint of the inducing-point interpolation (VariationalMultitaskGPModel :672-683, SGPR :302-303).
 */
int plmc_gemm_tn_f32(int mode, int M, int N, int K, const float *A, int64_t lda, int64_t strideA, const float *B,
                     int64_t ldb, int64_t strideB, float *C, int64_t ldc, int64_t strideC, int batch, void *stream);
int plmc_gemm_tn_f64(int mode, int M, int N, int K, const double *A, int64_t lda, int64_t strideA, const double *B,
                     int64_t ldb, int64_t strideB, double *C, int64_t ldc, int64_t strideC, int batch, void *stream);
/* The same for operands with TRIANGULAR structure (the factors W = L^-1, L^T = U, Ls and the triangular adjoints of the
 * Cholesky adjoint): `tri` = OR of the bits below; a tile then only walks the contraction range in which both operands have
 * entries -- the skipped terms are exact zeros, the result is the same number at a half to a sixth of the flops.  Structure is
 * declared per 128-block (entries inside a diagonal block may be anything).
 *   PLMC_TRI_A_LOWER  A[k][i] = 0 for k < 128 (i / 128)        PLMC_TRI_B_LOWER  B[k][j] = 0 for k < 128 (j / 128)
 *   PLMC_TRI_A_UPPER  A[k][i] = 0 for k >= 128 (i / 128 + 1)
 *   PLMC_TRI_C_LOWER  only tiles with i / 128 >= j / 128 are computed; the others are left untouched, or, with PLMC_TRI_C_ZERO
 *                     as well (mode 0 only), written as zeros.
 * The skipped range of a declared-zero block is never loaded: what stands there (the never-written W tiles above the block
 * diagonal of a factor buffer, NaN included) does not reach C.  tests/test_gpu_gemm_tn.py pins this. */
#define PLMC_TRI_A_LOWER 1
#define PLMC_TRI_B_LOWER 2
#define PLMC_TRI_A_UPPER 4
#define PLMC_TRI_C_LOWER 8
#define PLMC_TRI_C_ZERO 16
int plmc_gemm_tn_tri_f32(int mode, int tri, int M, int N, int K, const float *A, int64_t lda, int64_t strideA, const float *B,
                         int64_t ldb, int64_t strideB, float *C, int64_t ldc, int64_t strideC, int batch, void *stream);
int plmc_gemm_tn_tri_f64(int mode, int tri, int M, int N, int K, const double *A, int64_t lda, int64_t strideA, const double *B,
                         int64_t ldb, int64_t strideB, double *C, int64_t ldc, int64_t strideC, int batch, void *stream);

/*
 * Eval-mode posterior, the reductions behind the augmented sweep (ProjectedGPModel.__call__, projected_lmc.py:1133-1155;
 * gpytorch's DefaultPredictionStrategy behind ExactGPModel.__call__ :1134).
 * plmc_posterior_moments: from the factor buffer after plmc_potrf_*(with_inverse = 0) on [ Khat | y | K*^T ]
 *   (naug = 1 + ns): mean[latent][s] = v(s)^T z and vsq[latent][s] = |v(s)|^2 with z = column n_pad, v(s) = column
 *   n_pad + 1 + s; the latent posterior is (mean, k(x*, x*) - vsq).  mean, vsq: q x ns, contiguous.
 * plmc_mix_posterior: task-space moments of :1144 / :1152, mean[s][t] = sum_i mean_lat[i][s] Ht[i][t],
 *   var[s][t] = sum_i var_lat[i][s] Ht[i][t]^2 + eps.  mean_lat, var_lat: q x ns; Ht: q x p; outputs ns x p.  With latent
 *   sharding a rank passes its local latents (q = their number) and eps = 0, and adds eps after the all-reduce.
 * Both HBM-bound; sums carried in fp64 and rounded once: |got - exact| <= u |exact| + (L + 4) 2^-53 sum |terms| for a sum of L terms
 * (tests/_reduce_ref.py).
 * plmc_posterior_moments loads the augmented columns as 16-byte vectors: A 16-byte aligned, lda and strideA multiples of 16 bytes,
 *   and lda >= n_pad + (1 + ns rounded up to the 16-byte vector: 4 fp32 / 2 fp64 elements) -- columns n_pad + 1 + ns up to that
 *   boundary are loaded and not used.  n_pad a positive multiple of plmc_block(), ns >= 1, q >= 1.  Anything else is refused before
 *   the launch.
 */
int plmc_posterior_moments_f32(const float *A, int64_t n_pad, int64_t lda, int64_t strideA, int ns, float *mean,
                               float *vsq, int q, void *stream);
int plmc_posterior_moments_f64(const double *A, int64_t n_pad, int64_t lda, int64_t strideA, int ns, double *mean,
                               double *vsq, int q, void *stream);
int plmc_mix_posterior_f32(const float *mean_lat, const float *var_lat, const float *Ht, int q, int ns, int p,
                           double eps, float *mean, float *var, void *stream);
int plmc_mix_posterior_f64(const double *mean_lat, const double *var_lat, const double *Ht, int q, int ns, int p,
                           double eps, double *mean, double *var, void *stream);

/*
 * kinv_diag = diag(Khat^-1) = column sums of squares of W (q x n_pad): the leave-one-out variances
 * sigma2_i = 1 / [Khat^-1]_ii of `MultitaskGPModel.compute_loo` (:642-656) on the dense (n p) x (n p) system, where
 * the fused gradient kernel (single ARD kernel per matrix) does not apply.  HBM-bound, reads W once (the tiles on and below the
 * block diagonal, 16-byte vector loads), sums carried in fp64.  Refused before anything is launched: a null pointer, q < 1, n_pad
 * not a positive multiple of plmc_block(), ldw < n_pad, W not 16-byte aligned, ldw or strideW not a multiple of 16 bytes.
 */
int plmc_w_diag_f32(const float *W, int64_t n_pad, int64_t ldw, int64_t strideW, float *kinv_diag, int q,
                    void *stream);
int plmc_w_diag_f64(const double *W, int64_t n_pad, int64_t ldw, int64_t strideW, double *kinv_diag, int q,
                    void *stream);

/*
 * Fused K^-1 = W^T W (MFMA) + analytic MLL gradient reduction: for every upper tile of K^-1 the
 * epilogue forms (alpha alpha^T - K^-1) o dKhat/dtheta from X staged in LDS and reduces it.
 *   grad[latent][0..d-1] = d logp / d ell_k,  [d] = d/d noise,  [d+1] = d/d oscale   (double)
 * Optional outputs (may be NULL): Kinv (n_pad x ldk upper tiles, batch stride strideK),
 * kinv_diag (q x n_pad: diagonal of K^-1, for leave-one-out, compute_loo :1108-1119).
 * partials: scratch of plmc_grad_scratch_bytes_for(n_pad, q, sizeof element) bytes.
 * fp32 entry point, PLMC_SPLIT != 0: the W^T W products run on the 16-bit matrix cores from a split copy of W (planes
 * behind the partials; arithmetic as documented at plmc_potrf_ex_f32).
 */
int plmc_kinv_grad_f32(int kind, const float *W, int64_t n_pad, int64_t ldw, int64_t strideW,
                       const float *alpha, const float *X, int n, int d, const float *ell,
                       const float *oscale, double *grad, float *Kinv, int64_t ldk, int64_t strideK,
                       float *kinv_diag, void *partials, int q, void *stream);
int plmc_kinv_grad_f64(int kind, const double *W, int64_t n_pad, int64_t ldw, int64_t strideW,
                       const double *alpha, const double *X, int n, int d, const double *ell,
                       const double *oscale, double *grad, double *Kinv, int64_t ldk, int64_t strideK,
                       double *kinv_diag, void *partials, int q, void *stream);
/* The same with `eig_lo`: q lower bounds of the smallest eigenvalue of Khat (device pointer; for a GP covariance K + s2 I
 * the noise variances s2).  With them the fp32 entry point may run its W^T W products as the two-plane fp16 split (see
 * plmc_potrf_ex_f32); NULL or the plain entry point: three-plane bf16 split.  The fp64 entry point ignores it. */
int plmc_kinv_grad_ex_f32(int kind, const float *W, int64_t n_pad, int64_t ldw, int64_t strideW,
                          const float *alpha, const float *X, int n, int d, const float *ell,
                          const float *oscale, double *grad, float *Kinv, int64_t ldk, int64_t strideK,
                          float *kinv_diag, void *partials, int q, const float *eig_lo, void *stream);
int plmc_kinv_grad_ex_f64(int kind, const double *W, int64_t n_pad, int64_t ldw, int64_t strideW,
                          const double *alpha, const double *X, int n, int d, const double *ell,
                          const double *oscale, double *grad, double *Kinv, int64_t ldk, int64_t strideK,
                          double *kinv_diag, void *partials, int q, const double *eig_lo, void *stream);
/* The same for a W that is still where its sweep left it: W = the inverse-factor columns of the factor buffer (ldw = that
 * buffer's lda), Vd = the scratch of that plmc_potrf_ex_* call (with_inverse != 0), untouched since.  The sweep's
 * epilogues have already written the 16-bit planes of W into Vd (the rows of a group the moment they are final), so the
 * split pass over W of the entry points above is skipped (0.6 ms of the 19 ms step at the metric shape) and `partials`
 * only needs plmc_grad_partials_bytes(n_pad, q).  Both calls must see the same PLMC_SPLIT and both or neither an eig_lo:
 * the scratch records which scheme wrote it and a mismatch yields NaN gradients, not silently wrong ones.  Vd = NULL, fp64,
 * PLMC_SPLIT=0 or a layout without inverse-factor columns: exactly plmc_kinv_grad_ex_* (then `partials` must have the
 * full plmc_grad_scratch_bytes_for size). */
int plmc_kinv_grad_vd_f32(int kind, const float *W, int64_t n_pad, int64_t ldw, int64_t strideW,
                          const float *alpha, const float *X, int n, int d, const float *ell,
                          const float *oscale, double *grad, float *Kinv, int64_t ldk, int64_t strideK,
                          float *kinv_diag, void *partials, int q, const float *eig_lo, const float *Vd, void *stream);
int plmc_kinv_grad_vd_f64(int kind, const double *W, int64_t n_pad, int64_t ldw, int64_t strideW,
                          const double *alpha, const double *X, int n, int d, const double *ell,
                          const double *oscale, double *grad, double *Kinv, int64_t ldk, int64_t strideK,
                          double *kinv_diag, void *partials, int q, const double *eig_lo, const double *Vd, void *stream);

/*
 * Additive kernels: a sum of `ncomp` scaled ARD sub-kernels of ONE stationary kind (the reference's `decomp` constructor argument,
 * handle_covar_ :131-167: k(x, x') = sum_g s_g k_g(x[idx_g], x'[idx_g]), batch_shape = [n_funcs]) on the batched exact engine:
 *     Khat_i = sum_{g < ncomp} oscale[i][g] k(|(x - x') / ell[i][g][:]|) + noise[i] I,     1 <= ncomp <= plmc_max_components().
 * Component table, per latent i:  ell (q x ncomp x d, contiguous) holds d lengthscale slots per component; a dimension k outside
 *   component g has ell[i][g][k] = +inf, i.e. 1 / ell = 0 exactly: it adds nothing to that component's distance.  oscale
 *   (q x ncomp) or NULL (all ones).  noise: q.  Stationary kinds only; PLMC_SPLINE is an argument error.
 * Every entry point takes the arguments of its single-kernel form with `ncomp` in front of `ell`, and does what that form does:
 *   plmc_assemble_add_*        plmc_assemble_*        (upper tiles of Khat, identity padding)
 *   plmc_assemble_cross_add_*  plmc_assemble_cross_*  (prediction columns; the dense K** of a full posterior covariance)
 *   plmc_factorize_add_ex_*    plmc_factorize_ex_*    (assembly overlapped with the sweep; bit-identical to the two calls)
 *   plmc_kinv_grad_add_vd_*    plmc_kinv_grad_vd_*    (K^-1 = W^T W with the gradient reduced in the epilogue)
 * The inputs are staged raw; x - x' is formed once per element and scaled per component.  ncomp = 1 IS the single-kernel entry point:
 * the same kernel instantiations on ell (q x 1 x d) = (q x d), bit-identical output and the gradient layout below with ncomp = 1.
 * Gradient table of plmc_kinv_grad_add_vd_* (double), ncomp (d + 1) + 1 entries per latent:
 *     grad[latent] = [ d logp / d ell: ncomp x d | d / d noise | d / d oscale: ncomp ]
 *   with d / d ell[g][k] = 0 exactly where ell[g][k] = +inf.  `partials`: the scratch of plmc_kinv_grad_vd_* for q * ncomp latents
 *   (plmc_grad_partials_bytes(n_pad, q * ncomp), resp. plmc_grad_scratch_bytes_for(n_pad, q * ncomp, elem_bytes) where the planes of W
 *   are not taken from Vd): one row of partial sums per tile AND component.
 * plmc_kernel_vjp_add_* is plmc_kernel_vjp_* (below) for a component table: the pull-back of the adjoint G of a dense block
 *   K_i[a][b] = sum_g oscale[i][g] k(|(x1_a - x2_b) / ell[i][g][:]|) -- K_ZZ and K_ZX of the inducing-point (SGPR) and variational models.
 *   gX1 [q][n1][d] sums over the components; gEll [q][n1][ncomp][d] and gOs [q][n1][ncomp] are row partials per component (the caller
 *   sums over rows).  gEll is exactly 0 where ell = +inf, gX1 exactly 0 on a dimension no component uses; a component whose own scaled
 *   distance is 0 follows the convention of the plain kernel (Matern-1/2: nothing to gX1 / gEll, its value to gOs), also where the two
 *   points differ outside its group.  G is read once for d <= 16; for d > 16 the components are split over passes (fp32: two per pass,
 *   fp64: one).  The spline kind and ncomp > plmc_max_components() are argument errors.
 */
int plmc_max_components(void);                /* most components of an additive kernel (4) */
int plmc_assemble_add_f32(int kind, const float *X, int n, int d, int ncomp, const float *ell, const float *oscale,
                          const float *noise, float *A, int64_t lda, int64_t strideA, int q, void *stream);
int plmc_assemble_add_f64(int kind, const double *X, int n, int d, int ncomp, const double *ell, const double *oscale,
                          const double *noise, double *A, int64_t lda, int64_t strideA, int q, void *stream);
int plmc_assemble_cross_add_f32(int kind, const float *X, int n, const float *Xs, int ns, int d, int ncomp,
                                const float *ell, const float *oscale, float *Out, int64_t ldo,
                                int64_t strideO, int64_t col0, int64_t n_rows, int q, void *stream);
int plmc_assemble_cross_add_f64(int kind, const double *X, int n, const double *Xs, int ns, int d, int ncomp,
                                const double *ell, const double *oscale, double *Out, int64_t ldo,
                                int64_t strideO, int64_t col0, int64_t n_rows, int q, void *stream);
int plmc_factorize_add_ex_f32(int kind, const float *X, int n, int d, int ncomp, const float *ell, const float *oscale,
                              const float *noise, float *A, int64_t n_pad, int64_t lda, int naug, int64_t strideA, float *Vd,
                              double *logdet, int *info, int with_inverse, int q, const float *eig_lo, void *stream);
int plmc_factorize_add_ex_f64(int kind, const double *X, int n, int d, int ncomp, const double *ell, const double *oscale,
                              const double *noise, double *A, int64_t n_pad, int64_t lda, int naug, int64_t strideA, double *Vd,
                              double *logdet, int *info, int with_inverse, int q, const double *eig_lo, void *stream);
int plmc_kinv_grad_add_vd_f32(int kind, const float *W, int64_t n_pad, int64_t ldw, int64_t strideW,
                              const float *alpha, const float *X, int n, int d, int ncomp, const float *ell,
                              const float *oscale, double *grad, float *Kinv, int64_t ldk, int64_t strideK,
                              float *kinv_diag, void *partials, int q, const float *eig_lo, const float *Vd, void *stream);
int plmc_kinv_grad_add_vd_f64(int kind, const double *W, int64_t n_pad, int64_t ldw, int64_t strideW,
                              const double *alpha, const double *X, int n, int d, int ncomp, const double *ell,
                              const double *oscale, double *grad, double *Kinv, int64_t ldk, int64_t strideK,
                              double *kinv_diag, void *partials, int q, const double *eig_lo, const double *Vd, void *stream);
int plmc_kernel_vjp_add_f32(int kind, const float *X1, int n1, const float *X2, int n2, int d, int ncomp,
                            const float *ell, const float *oscale, const float *G, int64_t ldg,
                            int64_t strideG, double *gX1, double *gEll, double *gOs, int q, void *stream);
int plmc_kernel_vjp_add_f64(int kind, const double *X1, int n1, const double *X2, int n2, int d, int ncomp,
                            const double *ell, const double *oscale, const double *G, int64_t ldg,
                            int64_t strideG, double *gX1, double *gEll, double *gOs, int q, void *stream);

/*
 * Spectral-mixture kernel [gpytorch-knowledge: SpectralMixtureKernel; the reference's tidal study, realdata_experiments.py:130-140, runs
 * every model with it] on the batched exact engine:
 *     Khat_i = sum_{m < nmix} w[i][m] exp(-2 pi^2 sum_k s[i][m][k]^2 tau_k^2) prod_k cos(2 pi mu[i][m][k] tau_k) + noise[i] I,   tau = x - x',
 *     1 <= nmix <= plmc_sm_max_mixtures(),  1 <= d <= plmc_sm_max_dim().  Exceeding a limit is an argument error (plmc_last_error()).
 * Table, per latent i:  scales s and means mu (q x nmix x d, contiguous), weights w (q x nmix) or NULL (all ones).  A dimension a
 *   component ignores carries s = mu = 0: its factor is exactly 1 and its gradients are exactly 0.  noise: q.
 * Every entry point takes the arguments of its `_add` form with (kind, ..., ncomp, ell, oscale, ...) replaced by
 * (..., nmix, scales, means, weights, ...) and does what that form does:
 *   plmc_assemble_sm_*        plmc_assemble_add_*        (upper tiles of Khat, identity padding)
 *   plmc_assemble_cross_sm_*  plmc_assemble_cross_add_*  (prediction columns; the dense K** of a full posterior covariance)
 *   plmc_factorize_sm_ex_*    plmc_factorize_add_ex_*    (assembly overlapped with the sweep; bit-identical to plmc_assemble_sm_* followed
 *                                                         by plmc_potrf_ex_*)
 *   plmc_kinv_grad_sm_vd_*    plmc_kinv_grad_add_vd_*    (K^-1 = W^T W with the gradient reduced in the epilogue)
 * The carrier's phase mu tau is reduced in revolutions before the cosine (difference and product with their rounding residuals), so
 * the fp32 assembly is within 32 d 2^-24 sum_m w_m of the fp64 formula at the fp32 inputs per element, at any phase.
 * The fp16 split scales of the sweep take eig_lo as for every other kernel; |K_ij| <= sum_m w_m + noise, the diagonal, here too.
 * Gradient table of plmc_kinv_grad_sm_vd_* (double), 2 nmix d + 1 + nmix entries per latent:
 *     grad[latent] = [ d logp / d scales: nmix x d | d / d means: nmix x d | d / d noise | d / d weights: nmix ]
 *   finite also where a cosine factor is exactly 0 (the product's derivative is formed without a division).
 *   plmc_kinv_grad_sm_vd_f32 with d > 1 forms K^-1 with the fp32 matrix instructions whatever PLMC_SPLIT says (the knob and eig_lo
 *   are not looked at; no planes of W are needed); d = 1 follows the knob like every other kernel.
 * Scratch.  `Vd`: the scratch of the sweep, sized as for plmc_potrf_ex_* / plmc_factorize_ex_* (plmc_vd_blocks_for(n_pad, lda, elem
 *   bytes), resp. plmc_vd_blocks_keep) -- the kernel does not change it.  `partials`: plmc_sm_grad_partials_bytes(n_pad, q, nmix, elem
 *   bytes) bytes, one row of partial sums per tile and component; a function of its arguments only, never of a dev knob.  The fp32 split
 *   engine takes the planes of W from the Vd of the sweep that produced W (with_inverse on an lda >= 2 n_pad layout) and refuses a call
 *   without them; fp64 and PLMC_SPLIT=0 need no planes.
 */
int plmc_sm_max_mixtures(void);               /* most components of a spectral-mixture kernel (8) */
int plmc_sm_max_dim(void);                    /* largest input dimension of a spectral-mixture kernel (8) */
int64_t plmc_sm_grad_partials_bytes(int64_t n_pad, int q, int nmix, int elem_bytes);
int plmc_assemble_sm_f32(const float *X, int n, int d, int nmix, const float *scales, const float *means, const float *weights,
                         const float *noise, float *A, int64_t lda, int64_t strideA, int q, void *stream);
int plmc_assemble_sm_f64(const double *X, int n, int d, int nmix, const double *scales, const double *means, const double *weights,
                         const double *noise, double *A, int64_t lda, int64_t strideA, int q, void *stream);
int plmc_assemble_cross_sm_f32(const float *X, int n, const float *Xs, int ns, int d, int nmix, const float *scales, const float *means,
                               const float *weights, float *Out, int64_t ldo, int64_t strideO, int64_t col0, int64_t n_rows, int q,
                               void *stream);
int plmc_assemble_cross_sm_f64(const double *X, int n, const double *Xs, int ns, int d, int nmix, const double *scales, const double *means,
                               const double *weights, double *Out, int64_t ldo, int64_t strideO, int64_t col0, int64_t n_rows, int q,
                               void *stream);
int plmc_factorize_sm_ex_f32(const float *X, int n, int d, int nmix, const float *scales, const float *means, const float *weights,
                             const float *noise, float *A, int64_t n_pad, int64_t lda, int naug, int64_t strideA, float *Vd, double *logdet,
                             int *info, int with_inverse, int q, const float *eig_lo, void *stream);
int plmc_factorize_sm_ex_f64(const double *X, int n, int d, int nmix, const double *scales, const double *means, const double *weights,
                             const double *noise, double *A, int64_t n_pad, int64_t lda, int naug, int64_t strideA, double *Vd, double *logdet,
                             int *info, int with_inverse, int q, const double *eig_lo, void *stream);
int plmc_kinv_grad_sm_vd_f32(const float *W, int64_t n_pad, int64_t ldw, int64_t strideW, const float *alpha, const float *X, int n, int d,
                             int nmix, const float *scales, const float *means, const float *weights, double *grad, float *Kinv, int64_t ldk,
                             int64_t strideK, float *kinv_diag, void *partials, int q, const float *eig_lo, const float *Vd, void *stream);
int plmc_kinv_grad_sm_vd_f64(const double *W, int64_t n_pad, int64_t ldw, int64_t strideW, const double *alpha, const double *X, int n, int d,
                             int nmix, const double *scales, const double *means, const double *weights, double *grad, double *Kinv, int64_t ldk,
                             int64_t strideK, double *kinv_diag, void *partials, int q, const double *eig_lo, const double *Vd, void *stream);

/*
 * Periodic kernel [gpytorch-knowledge: PeriodicKernel.forward, v1.11, unverified offline] on the batched exact engine:
 *     Khat_i = os[i] exp(-2 sum_k sin^2(pi tau_k / p[i][k]) / ell[i][k]) + noise[i] I,   tau = x - x'   (the lengthscale is not squared),
 *     1 <= d <= plmc_per_max_dim().  Exceeding the limit or a null `period` is an argument error (plmc_last_error()); nothing is launched.
 * Table, per latent i:  lengthscales ell and periods p (q x d each, contiguous), output scale os (q) or NULL (all ones).  noise: q.
 * Every entry point takes the arguments of its plain form with (kind, ..., ell, oscale, ...) replaced by (..., ell, period, oscale, ...)
 * and does what that form does:
 *   plmc_assemble_per_*        plmc_assemble_*        (upper tiles of Khat, identity padding)
 *   plmc_assemble_cross_per_*  plmc_assemble_cross_*  (prediction columns; the dense K** of a full posterior covariance)
 *   plmc_factorize_per_ex_*    plmc_factorize_ex_*    (assembly overlapped with the sweep; bit-identical to plmc_assemble_per_* followed
 *                                                      by plmc_potrf_ex_*)
 *   plmc_kinv_grad_per_vd_*    plmc_kinv_grad_vd_*    (K^-1 = W^T W with the gradient reduced in the epilogue)
 * The phase tau / p is reduced in revolutions before the sine (difference and product with their rounding residuals, 1 / p as two
 * terms), so the fp32 assembly is within 24 d 2^-24 os (1 + 1 / min_k ell_k) of the fp64 formula at the fp32 inputs per element, at any
 * phase below 2^20 revolutions.  |K_ij| <= os + noise, the diagonal.
 * Gradient table of plmc_kinv_grad_per_vd_* (double), 2 d + 2 entries per latent:
 *     grad[latent] = [ d logp / d ell: d | d / d period: d | d / d noise | d / d os ]
 *   The diagonal (tau = 0) contributes to noise and os only; an off-diagonal sine that is exactly 0 gives exactly 0.
 *   plmc_kinv_grad_per_vd_f32 with d > 1 forms K^-1 with the fp32 matrix instructions whatever PLMC_SPLIT says (the knob and eig_lo
 *   are not looked at; no planes of W are needed); d = 1 follows the knob like every other kernel.
 * Scratch.  `Vd`: as for plmc_kinv_grad_vd_*.  `partials`: plmc_per_grad_partials_bytes(n_pad, q, elem bytes) bytes, one row of partial
 *   sums per tile; a function of its arguments only, never of a dev knob.  The fp32 split engine takes the planes of W from the Vd of
 *   the sweep that produced W and refuses a call without them; fp64 and PLMC_SPLIT=0 need no planes.
 */
int plmc_per_max_dim(void);                   /* largest input dimension of a periodic kernel (8) */
int64_t plmc_per_grad_partials_bytes(int64_t n_pad, int q, int elem_bytes);
int plmc_assemble_per_f32(const float *X, int n, int d, const float *ell, const float *period, const float *oscale, const float *noise,
                          float *A, int64_t lda, int64_t strideA, int q, void *stream);
int plmc_assemble_per_f64(const double *X, int n, int d, const double *ell, const double *period, const double *oscale, const double *noise,
                          double *A, int64_t lda, int64_t strideA, int q, void *stream);
int plmc_assemble_cross_per_f32(const float *X, int n, const float *Xs, int ns, int d, const float *ell, const float *period,
                                const float *oscale, float *Out, int64_t ldo, int64_t strideO, int64_t col0, int64_t n_rows, int q,
                                void *stream);
int plmc_assemble_cross_per_f64(const double *X, int n, const double *Xs, int ns, int d, const double *ell, const double *period,
                                const double *oscale, double *Out, int64_t ldo, int64_t strideO, int64_t col0, int64_t n_rows, int q,
                                void *stream);
int plmc_factorize_per_ex_f32(const float *X, int n, int d, const float *ell, const float *period, const float *oscale, const float *noise,
                              float *A, int64_t n_pad, int64_t lda, int naug, int64_t strideA, float *Vd, double *logdet, int *info,
                              int with_inverse, int q, const float *eig_lo, void *stream);
int plmc_factorize_per_ex_f64(const double *X, int n, int d, const double *ell, const double *period, const double *oscale, const double *noise,
                              double *A, int64_t n_pad, int64_t lda, int naug, int64_t strideA, double *Vd, double *logdet, int *info,
                              int with_inverse, int q, const double *eig_lo, void *stream);
int plmc_kinv_grad_per_vd_f32(const float *W, int64_t n_pad, int64_t ldw, int64_t strideW, const float *alpha, const float *X, int n, int d,
                              const float *ell, const float *period, const float *oscale, double *grad, float *Kinv, int64_t ldk,
                              int64_t strideK, float *kinv_diag, void *partials, int q, const float *eig_lo, const float *Vd, void *stream);
int plmc_kinv_grad_per_vd_f64(const double *W, int64_t n_pad, int64_t ldw, int64_t strideW, const double *alpha, const double *X, int n, int d,
                              const double *ell, const double *period, const double *oscale, double *grad, double *Kinv, int64_t ldk,
                              int64_t strideK, double *kinv_diag, void *partials, int q, const double *eig_lo, const double *Vd, void *stream);

/*
 * Rational-quadratic kernel [gpytorch-knowledge: RQKernel, unverified offline] on the batched exact engine:
 *     Khat_i = os[i] (1 + r^2 / (2 alpha[i]))^(-alpha[i]) + noise[i] I,   r^2 = sum_k ((x_k - x'_k) / ell[i][k])^2,
 *     1 <= d <= plmc_rq_max_dim().  Exceeding the limit, d <= 0 or a null `alpha` is an argument error (plmc_last_error()); nothing is
 *     launched.
 * Table, per latent i:  lengthscales ell (q x d, contiguous), alpha (q) > 0, output scale os (q) or NULL (all ones).  noise: q.
 * Every entry point takes the arguments of its periodic form with (ell, period) replaced by (ell, alpha) and does what that form does:
 *   plmc_assemble_rq_*        plmc_assemble_*        (upper tiles of Khat, identity padding)
 *   plmc_assemble_cross_rq_*  plmc_assemble_cross_*  (prediction columns; the dense K** of a full posterior covariance)
 *   plmc_factorize_rq_ex_*    plmc_factorize_ex_*    (assembly overlapped with the sweep; bit-identical to plmc_assemble_rq_* followed
 *                                                     by plmc_potrf_ex_*)
 *   plmc_kinv_grad_rq_vd_*    plmc_kinv_grad_vd_*    (K^-1 = W^T W with the gradient reduced in the epilogue)
 *   plmc_loo_grad_rq_*        plmc_loo_grad_*        (the gradient table of the leave-one-out objective, below)
 * The value is exp(-alpha log1p(u)), u = r^2 fl(1 / (2 alpha)), with r^2 from the raw differences x - x' scaled by 1 / ell: the fp32
 * assembly is within (d + 8) 2^-24 os of the fp64 formula at the fp32 inputs per element WHATEVER alpha is (pow(1 + u, -alpha) loses
 * alpha 2^-24).  The diagonal is os + noise with one rounding, a coincident pair off the diagonal gives exactly os.
 * Gradient table of plmc_kinv_grad_rq_vd_* and plmc_loo_grad_rq_* (double), d + 3 entries per latent:
 *     grad[latent] = [ d logp / d ell: d | d / d alpha | d / d noise | d / d os ]
 *   d k / d alpha = -k h(u), h(u) = log1p(u) - u / (1 + u), evaluated without cancellation (a series below u = 1/8).  The diagonal
 *   (u = 0) contributes to noise and os only.
 *   plmc_kinv_grad_rq_vd_f32 with d = 1 follows PLMC_SPLIT like every other kernel.  With d > 1 it follows the knob where that selects
 *   the two fp16 planes (the default with eig_lo given); where the three bf16 planes would run (PLMC_SPLIT=3, or no eig_lo) it forms
 *   K^-1 with the fp32 matrix instructions instead (the knob and eig_lo are not looked at; no planes of W are needed).
 * Scratch.  `Vd`: as for plmc_kinv_grad_vd_*.  `partials`: plmc_grad_partials_bytes(n_pad, q) bytes, one row of partial sums per tile.
 *   The fp32 split engine takes the planes of W from the Vd of the sweep that produced W and refuses a call without them; fp64 and
 *   PLMC_SPLIT=0 need no planes.
 */
int plmc_rq_max_dim(void);                    /* largest input dimension of a rational-quadratic kernel (16) */
int plmc_assemble_rq_f32(const float *X, int n, int d, const float *ell, const float *alpha, const float *oscale, const float *noise,
                         float *A, int64_t lda, int64_t strideA, int q, void *stream);
int plmc_assemble_rq_f64(const double *X, int n, int d, const double *ell, const double *alpha, const double *oscale, const double *noise,
                         double *A, int64_t lda, int64_t strideA, int q, void *stream);
int plmc_assemble_cross_rq_f32(const float *X, int n, const float *Xs, int ns, int d, const float *ell, const float *alpha,
                               const float *oscale, float *Out, int64_t ldo, int64_t strideO, int64_t col0, int64_t n_rows, int q,
                               void *stream);
int plmc_assemble_cross_rq_f64(const double *X, int n, const double *Xs, int ns, int d, const double *ell, const double *alpha,
                               const double *oscale, double *Out, int64_t ldo, int64_t strideO, int64_t col0, int64_t n_rows, int q,
                               void *stream);
int plmc_factorize_rq_ex_f32(const float *X, int n, int d, const float *ell, const float *alpha, const float *oscale, const float *noise,
                             float *A, int64_t n_pad, int64_t lda, int naug, int64_t strideA, float *Vd, double *logdet, int *info,
                             int with_inverse, int q, const float *eig_lo, void *stream);
int plmc_factorize_rq_ex_f64(const double *X, int n, int d, const double *ell, const double *alpha, const double *oscale, const double *noise,
                             double *A, int64_t n_pad, int64_t lda, int naug, int64_t strideA, double *Vd, double *logdet, int *info,
                             int with_inverse, int q, const double *eig_lo, void *stream);
/* (`shape` is the kernel's alpha; `alpha` is Khat^-1 y, as in every plmc_kinv_grad* call) */
int plmc_kinv_grad_rq_vd_f32(const float *W, int64_t n_pad, int64_t ldw, int64_t strideW, const float *alpha, const float *X, int n, int d,
                             const float *ell, const float *shape, const float *oscale, double *grad, float *Kinv, int64_t ldk,
                             int64_t strideK, float *kinv_diag, void *partials, int q, const float *eig_lo, const float *Vd, void *stream);
int plmc_kinv_grad_rq_vd_f64(const double *W, int64_t n_pad, int64_t ldw, int64_t strideW, const double *alpha, const double *X, int n, int d,
                             const double *ell, const double *shape, const double *oscale, double *grad, double *Kinv, int64_t ldk,
                             int64_t strideK, double *kinv_diag, void *partials, int q, const double *eig_lo, const double *Vd, void *stream);
int plmc_loo_grad_rq_f32(const float *Xop, int64_t n_pad, int64_t krows, int64_t ldx, int64_t strideX, const float *beta, const float *X,
                         int n, int d, const float *ell, const float *alpha, const float *oscale, double *grad, void *partials, int q,
                         void *stream);
int plmc_loo_grad_rq_f64(const double *Xop, int64_t n_pad, int64_t krows, int64_t ldx, int64_t strideX, const double *beta, const double *X,
                         int n, int d, const double *ell, const double *alpha, const double *oscale, double *grad, void *partials, int q,
                         void *stream);

/*
 * Locally periodic kernel [gpytorch-knowledge: ProductKernel of PeriodicKernel and RBFKernel, the elementwise product of its factors,
 * unverified offline] on the batched exact engine, the model of a periodicity whose shape drifts:
 *     Khat_i = os[i] exp(-2 sum_k sin^2(pi tau_k / p[i][k]) / ell[i][k] - 1/2 sum_k (tau_k / lam[i][k])^2) + noise[i] I,   tau = x - x'
 *     (ell the periodic lengthscale, not squared; p the period; lam = `rbf_ell` the RBF lengthscale),   1 <= d <= plmc_lper_max_dim().
 *     Exceeding the limit, d <= 0 or a null `period` or `rbf_ell` is an argument error (plmc_last_error()); nothing is launched.
 * Table, per latent i:  ell, p and lam (q x d each, contiguous), output scale os (q) or NULL (all ones).  noise: q.
 * Every entry point takes the arguments of its periodic form with (ell, period, oscale) replaced by (ell, period, rbf_ell, oscale) and
 * does what that form does:
 *   plmc_assemble_lper_*        plmc_assemble_per_*        (upper tiles of Khat, identity padding)
 *   plmc_assemble_cross_lper_*  plmc_assemble_cross_per_*  (prediction columns; the dense K** of a full posterior covariance)
 *   plmc_factorize_lper_ex_*    plmc_factorize_per_ex_*    (assembly overlapped with the sweep; bit-identical to plmc_assemble_lper_*
 *                                                           followed by plmc_potrf_ex_*)
 *   plmc_kinv_grad_lper_vd_*    plmc_kinv_grad_per_vd_*    (K^-1 = W^T W with the gradient reduced in the epilogue)
 *   plmc_loo_grad_lper_*        plmc_loo_grad_per_*        (the gradient table of the leave-one-out objective, below)
 * The periodic exponent is the periodic kernel's (phase reduced in revolutions, 1 / p as two terms), the RBF exponent comes from the raw
 * differences x - x' scaled by 1 / lam, and ONE accurate exponential takes their sum: the fp32 assembly is within
 *     [24 d (1 + 1 / min_k ell_k) + (d + 8)] 2^-24 os
 * of the fp64 formula at the fp32 inputs per element, at any phase below 2^20 revolutions.  The diagonal is os + noise
 * with one rounding, a coincident pair off the diagonal gives exactly os.
 * Limits.  lam = +inf (1 / lam = 0) gives the value of plmc_assemble_per_* and ell = +inf that of the RBF kernel with lengthscales lam;
 *   the gradient entries of the factor that is switched off are then EXACTLY 0 (finite tile sums divided by +inf), all others finite.
 * Gradient table of plmc_kinv_grad_lper_vd_* and plmc_loo_grad_lper_* (double), 3 d + 2 entries per latent:
 *     grad[latent] = [ d logp / d ell: d | d / d period: d | d / d rbf_ell: d | d / d noise | d / d os ]
 *   The diagonal (tau = 0) contributes to noise and os only; an off-diagonal sine that is exactly 0 gives exactly 0 for ell and period.
 *   plmc_kinv_grad_lper_vd_f32 with d > 1 forms K^-1 with the fp32 matrix instructions whatever PLMC_SPLIT says, as the periodic kernel
 *   does (the knob and eig_lo are not looked at; no planes of W are needed): the split-engine epilogue is instantiated for d = 1 only,
 *   which follows the knob like every other kernel.
 * Scratch.  `Vd`: as for plmc_kinv_grad_vd_*.  `partials`: plmc_lper_grad_partials_bytes(n_pad, q, elem bytes) bytes, one row of
 *   partial sums per tile (the size plmc_per_grad_partials_bytes gives); a function of its arguments only, never of a dev knob.  The
 *   fp32 split engine takes the planes of W from the Vd of the sweep that produced W and refuses a call without them; fp64 and
 *   PLMC_SPLIT=0 need no planes.
 */
int plmc_lper_max_dim(void);                  /* largest input dimension of a locally periodic kernel (8) */
int64_t plmc_lper_grad_partials_bytes(int64_t n_pad, int q, int elem_bytes);
int plmc_assemble_lper_f32(const float *X, int n, int d, const float *ell, const float *period, const float *rbf_ell, const float *oscale,
                           const float *noise, float *A, int64_t lda, int64_t strideA, int q, void *stream);
int plmc_assemble_lper_f64(const double *X, int n, int d, const double *ell, const double *period, const double *rbf_ell, const double *oscale,
                           const double *noise, double *A, int64_t lda, int64_t strideA, int q, void *stream);
int plmc_assemble_cross_lper_f32(const float *X, int n, const float *Xs, int ns, int d, const float *ell, const float *period,
                                 const float *rbf_ell, const float *oscale, float *Out, int64_t ldo, int64_t strideO, int64_t col0,
                                 int64_t n_rows, int q, void *stream);
int plmc_assemble_cross_lper_f64(const double *X, int n, const double *Xs, int ns, int d, const double *ell, const double *period,
                                 const double *rbf_ell, const double *oscale, double *Out, int64_t ldo, int64_t strideO, int64_t col0,
                                 int64_t n_rows, int q, void *stream);
int plmc_factorize_lper_ex_f32(const float *X, int n, int d, const float *ell, const float *period, const float *rbf_ell, const float *oscale,
                               const float *noise, float *A, int64_t n_pad, int64_t lda, int naug, int64_t strideA, float *Vd, double *logdet,
                               int *info, int with_inverse, int q, const float *eig_lo, void *stream);
int plmc_factorize_lper_ex_f64(const double *X, int n, int d, const double *ell, const double *period, const double *rbf_ell, const double *oscale,
                               const double *noise, double *A, int64_t n_pad, int64_t lda, int naug, int64_t strideA, double *Vd, double *logdet,
                               int *info, int with_inverse, int q, const double *eig_lo, void *stream);
int plmc_kinv_grad_lper_vd_f32(const float *W, int64_t n_pad, int64_t ldw, int64_t strideW, const float *alpha, const float *X, int n, int d,
                               const float *ell, const float *period, const float *rbf_ell, const float *oscale, double *grad, float *Kinv,
                               int64_t ldk, int64_t strideK, float *kinv_diag, void *partials, int q, const float *eig_lo, const float *Vd,
                               void *stream);
int plmc_kinv_grad_lper_vd_f64(const double *W, int64_t n_pad, int64_t ldw, int64_t strideW, const double *alpha, const double *X, int n, int d,
                               const double *ell, const double *period, const double *rbf_ell, const double *oscale, double *grad, double *Kinv,
                               int64_t ldk, int64_t strideK, double *kinv_diag, void *partials, int q, const double *eig_lo, const double *Vd,
                               void *stream);
int plmc_loo_grad_lper_f32(const float *Xop, int64_t n_pad, int64_t krows, int64_t ldx, int64_t strideX, const float *beta, const float *X,
                           int n, int d, const float *ell, const float *period, const float *rbf_ell, const float *oscale, double *grad,
                           void *partials, int q, void *stream);
int plmc_loo_grad_lper_f64(const double *Xop, int64_t n_pad, int64_t krows, int64_t ldx, int64_t strideX, const double *beta, const double *X,
                           int n, int d, const double *ell, const double *period, const double *rbf_ell, const double *oscale, double *grad,
                           void *partials, int q, void *stream);

/*
 * Dot-product kernels [gpytorch-knowledge: LinearKernel, PolynomialKernel, unverified offline] on the batched exact engine:
 *     Khat_i = os[i] (c[i] + sum_k v[i][k] x_k x'_k)^P + noise[i] I,   v > 0, c >= 0, P an integer,
 *     1 <= d <= plmc_dot_max_dim(), 1 <= P <= plmc_dot_max_power()   (LinearKernel: P = 1, c = 0; PolynomialKernel: v = 1).
 *     Exceeding a limit, d <= 0, P <= 0 or a null `offset` is an argument error (plmc_last_error()); nothing is launched.
 * Table, per latent i:  variances v (q x d, contiguous), offset c (q), output scale os (q) or NULL (all ones); ONE power for the batch,
 * a host int.  noise: q.
 * Every entry point takes the arguments of its rational-quadratic form with (ell, alpha) replaced by (var, offset, power) and does what
 * that form does:
 *   plmc_assemble_dot_*        plmc_assemble_rq_*        (upper tiles of Khat, identity padding)
 *   plmc_assemble_cross_dot_*  plmc_assemble_cross_rq_*  (prediction columns; the dense K** of a full posterior covariance)
 *   plmc_factorize_dot_ex_*    plmc_factorize_rq_ex_*    (assembly overlapped with the sweep; bit-identical to plmc_assemble_dot_*
 *                                                         followed by plmc_potrf_ex_*)
 *   plmc_kinv_grad_dot_vd_*    plmc_kinv_grad_rq_vd_*    (K^-1 = W^T W with the gradient reduced in the epilogue)
 *   plmc_loo_grad_dot_*        plmc_loo_grad_rq_*        (the gradient table of the leave-one-out objective, below)
 * NOT stationary: k(x, x) = os (c + sum_k v_k x_k^2)^P depends on x.  The diagonal of Khat is that value plus the noise, an all-zero input
 * row gives os c^P + noise (P = 1, c = 0: a row of exact zeros and the noise), and the prior variance at a test point is NOT os.
 * The matrix is positive semi-definite of rank <= C(d + P, P), so Khat >= noise I as for every other family; without noise it is
 * singular as soon as n exceeds that rank.
 * The value is an FMA chain s = c + sum_k (v_k x_k) x'_k over the raw inputs and P - 1 multiplications; no pow, exp or log, so a negative s
 * keeps its sign under an odd P.  The fp32 assembly is within P (d + 3) 2^-24 os S^P, S = c + sum_k |v_k x_k x'_k|, of the fp64 formula at
 * the fp32 inputs per element.
 * Gradient table of plmc_kinv_grad_dot_vd_* and plmc_loo_grad_dot_* (double), d + 3 entries per latent:
 *     grad[latent] = [ d logp / d v: d | d / d c | d / d noise | d / d os ]
 *   with d k / d v_k = os P s^(P - 1) x_k x'_k, d k / d c = os P s^(P - 1), d k / d os = s^P.  The diagonal element contributes to EVERY
 *   entry (weight 1; the pairs off the diagonal 2).
 *   plmc_kinv_grad_dot_vd_f32 follows the rule of plmc_kinv_grad_rq_vd_f32: d = 1 follows PLMC_SPLIT; d > 1 runs on the two fp16 planes
 *   where the knob selects them (the default with eig_lo given) and on the fp32 matrix instructions where the three bf16 planes would
 *   run (PLMC_SPLIT=3, or no eig_lo).
 * Scratch.  `Vd`: as for plmc_kinv_grad_vd_*.  `partials`: plmc_grad_partials_bytes(n_pad, q) bytes, one row of partial sums per tile.
 *   The fp32 split engine takes the planes of W from the Vd of the sweep that produced W and refuses a call without them; fp64 and
 *   PLMC_SPLIT=0 need no planes.
 */
int plmc_dot_max_dim(void);                   /* largest input dimension of a dot-product kernel (16) */
int plmc_dot_max_power(void);                 /* largest power of a dot-product kernel (8) */
int plmc_assemble_dot_f32(const float *X, int n, int d, const float *var, const float *offset, int power, const float *oscale,
                          const float *noise, float *A, int64_t lda, int64_t strideA, int q, void *stream);
int plmc_assemble_dot_f64(const double *X, int n, int d, const double *var, const double *offset, int power, const double *oscale,
                          const double *noise, double *A, int64_t lda, int64_t strideA, int q, void *stream);
int plmc_assemble_cross_dot_f32(const float *X, int n, const float *Xs, int ns, int d, const float *var, const float *offset, int power,
                                const float *oscale, float *Out, int64_t ldo, int64_t strideO, int64_t col0, int64_t n_rows, int q,
                                void *stream);
int plmc_assemble_cross_dot_f64(const double *X, int n, const double *Xs, int ns, int d, const double *var, const double *offset, int power,
                                const double *oscale, double *Out, int64_t ldo, int64_t strideO, int64_t col0, int64_t n_rows, int q,
                                void *stream);
int plmc_factorize_dot_ex_f32(const float *X, int n, int d, const float *var, const float *offset, int power, const float *oscale,
                              const float *noise, float *A, int64_t n_pad, int64_t lda, int naug, int64_t strideA, float *Vd, double *logdet,
                              int *info, int with_inverse, int q, const float *eig_lo, void *stream);
int plmc_factorize_dot_ex_f64(const double *X, int n, int d, const double *var, const double *offset, int power, const double *oscale,
                              const double *noise, double *A, int64_t n_pad, int64_t lda, int naug, int64_t strideA, double *Vd, double *logdet,
                              int *info, int with_inverse, int q, const double *eig_lo, void *stream);
int plmc_kinv_grad_dot_vd_f32(const float *W, int64_t n_pad, int64_t ldw, int64_t strideW, const float *alpha, const float *X, int n, int d,
                              const float *var, const float *offset, int power, const float *oscale, double *grad, float *Kinv, int64_t ldk,
                              int64_t strideK, float *kinv_diag, void *partials, int q, const float *eig_lo, const float *Vd, void *stream);
int plmc_kinv_grad_dot_vd_f64(const double *W, int64_t n_pad, int64_t ldw, int64_t strideW, const double *alpha, const double *X, int n, int d,
                              const double *var, const double *offset, int power, const double *oscale, double *grad, double *Kinv, int64_t ldk,
                              int64_t strideK, double *kinv_diag, void *partials, int q, const double *eig_lo, const double *Vd, void *stream);
int plmc_loo_grad_dot_f32(const float *Xop, int64_t n_pad, int64_t krows, int64_t ldx, int64_t strideX, const float *beta, const float *X,
                          int n, int d, const float *var, const float *offset, int power, const float *oscale, double *grad, void *partials,
                          int q, void *stream);
int plmc_loo_grad_dot_f64(const double *Xop, int64_t n_pad, int64_t krows, int64_t ldx, int64_t strideX, const double *beta, const double *X,
                          int n, int d, const double *var, const double *offset, int power, const double *oscale, double *grad, void *partials,
                          int q, void *stream);

/*
 * Sums of kernel families (what `k1 + k2` builds: trend + a seasonality that drifts + medium-term irregularity, two periodicities, ...)
 * on the batched exact engine, the heterogeneous sum
 *     Khat_i = sum_{g < ncomp} os[i][g] k_{fam[g]}(x, x'; table[i][g]) + noise[i] I,
 *     1 <= ncomp <= plmc_sum_max_components() (4),   1 <= d <= plmc_sum_max_dim() (8, the smallest of the members' limits).
 * Members.  `fam`: a HOST array of ncomp ints, read during the call and shared by the q latents: the kind codes 0 .. 3 (RBF, Matern 1/2,
 *   3/2, 5/2) or one of the three codes below, which are disjoint from the kind codes.  The spline kind (4: not stationary, no bound
 *   |K_ij| <= diagonal for the fp16 scales) and the spectral mixture (already a sum with its own weights) are not members.
 * Table.  `table`: q x ncomp x (3 d + 1), contiguous, one record per latent and component:
 *     [ ell: d | period: d | rbf_ell: d | alpha: 1 ]
 *   A member reads only the slots it owns -- the ARD kinds ell; rational quadratic ell and alpha; periodic ell and period; locally periodic
 *   ell, period and rbf_ell -- with the meaning they have in that family's own section above.  The other slots are NEVER READ (they may
 *   hold NaN).  An owned lengthscale of +inf (1 / ell = 0 exactly) switches that dimension off for that component, as in the additive
 *   table: it adds exactly 0 to the exponent or distance and its gradient entries are exactly 0, its period's included (for the locally
 *   periodic member set ell and rbf_ell of that dimension).  `oscale`: q x ncomp, or NULL for all ones.  noise: q.
 * Every entry point takes the arguments of its `_add` form with (kind, ..., ncomp, ell, oscale, ...) replaced by
 * (..., ncomp, fam, table, oscale, ...) and does what that form does:
 *   plmc_assemble_sum_*        plmc_assemble_cross_sum_*        plmc_factorize_sum_ex_*  (bit-identical to plmc_assemble_sum_* followed by
 *   plmc_potrf_ex_*: factor buffer, log det, info)              plmc_kinv_grad_sum_vd_*  plmc_loo_grad_sum_*
 * Values.  Each component's value comes from its family's own function (so the phase reduction, the raw-difference scaling and the single
 *   accurate exponential of those sections carry over; x - x' is formed once per element) and the components are added in table order in
 *   the element type: the fp32 assembly is within the sum of the members' bounds, each times its os, plus (ncomp - 1) 2^-24 sum_g os_g, of
 *   the fp64 formula at the fp32 inputs.  The diagonal is sum_g os_g + noise, which is also the bound the sweep's fp16
 *   scales need; eig_lo is treated as for every other family.
 * One component.  ncomp = 1 IS the member's family: its own kernels run, so K, the factor buffer, values and gradients are bit-identical to
 *   the single-family entry point (the gradient after the slots are re-laid), and the arithmetic of the fp32 gradient call is that
 *   family's.
 * Gradient table of plmc_kinv_grad_sum_vd_* and plmc_loo_grad_sum_* (double), ncomp (3 d + 2) + 1 entries per latent:
 *     grad[latent] = [ d / d table: ncomp x (3 d + 1), in table layout | d / d noise | d / d oscale: ncomp ]
 *   Every slot a member does not own is exactly 0.
 *   plmc_kinv_grad_sum_vd_f32 with ncomp > 1 and d > 1 forms K^-1 with the fp32 matrix instructions whatever PLMC_SPLIT says, because the
 *   periodic-phase members do (the knob and eig_lo are not looked at; no planes of W are needed); d = 1 follows the knob.
 * Scratch.  `Vd`: as for plmc_kinv_grad_vd_*.  `partials`: plmc_sum_grad_partials_bytes(n_pad, q, ncomp, elem bytes) bytes, one row of
 *   partial sums per tile and component plus 512 bytes per latent (the re-laid rows of a one-member sum); a function of its arguments
 *   only, never of a dev knob.  The fp32 split engine takes the planes of W from the Vd of the sweep that produced W and refuses a call
 *   without them; fp64 and PLMC_SPLIT=0 need no planes.
 * Argument errors (plmc_last_error(), nothing is launched): ncomp or d beyond the limits, an unknown or spline member code, null `fam` or
 *   `table`.
 */
#define PLMC_FAM_PERIODIC 16                  /* member codes of a sum beside the kind codes 0 .. 3 */
#define PLMC_FAM_RQ 17
#define PLMC_FAM_LPER 18
int plmc_sum_max_components(void);            /* most members of a sum (4) */
int plmc_sum_max_dim(void);                   /* largest input dimension of a sum (8) */
int64_t plmc_sum_grad_partials_bytes(int64_t n_pad, int q, int ncomp, int elem_bytes);
int plmc_assemble_sum_f32(const float *X, int n, int d, int ncomp, const int *fam, const float *table, const float *oscale, const float *noise,
                          float *A, int64_t lda, int64_t strideA, int q, void *stream);
int plmc_assemble_sum_f64(const double *X, int n, int d, int ncomp, const int *fam, const double *table, const double *oscale,
                          const double *noise, double *A, int64_t lda, int64_t strideA, int q, void *stream);
int plmc_assemble_cross_sum_f32(const float *X, int n, const float *Xs, int ns, int d, int ncomp, const int *fam, const float *table,
                                const float *oscale, float *Out, int64_t ldo, int64_t strideO, int64_t col0, int64_t n_rows, int q,
                                void *stream);
int plmc_assemble_cross_sum_f64(const double *X, int n, const double *Xs, int ns, int d, int ncomp, const int *fam, const double *table,
                                const double *oscale, double *Out, int64_t ldo, int64_t strideO, int64_t col0, int64_t n_rows, int q,
                                void *stream);
int plmc_factorize_sum_ex_f32(const float *X, int n, int d, int ncomp, const int *fam, const float *table, const float *oscale, const float *noise,
                              float *A, int64_t n_pad, int64_t lda, int naug, int64_t strideA, float *Vd, double *logdet, int *info,
                              int with_inverse, int q, const float *eig_lo, void *stream);
int plmc_factorize_sum_ex_f64(const double *X, int n, int d, int ncomp, const int *fam, const double *table, const double *oscale,
                              const double *noise, double *A, int64_t n_pad, int64_t lda, int naug, int64_t strideA, double *Vd, double *logdet,
                              int *info, int with_inverse, int q, const double *eig_lo, void *stream);
int plmc_kinv_grad_sum_vd_f32(const float *W, int64_t n_pad, int64_t ldw, int64_t strideW, const float *alpha, const float *X, int n, int d,
                              int ncomp, const int *fam, const float *table, const float *oscale, double *grad, float *Kinv, int64_t ldk,
                              int64_t strideK, float *kinv_diag, void *partials, int q, const float *eig_lo, const float *Vd, void *stream);
int plmc_kinv_grad_sum_vd_f64(const double *W, int64_t n_pad, int64_t ldw, int64_t strideW, const double *alpha, const double *X, int n, int d,
                              int ncomp, const int *fam, const double *table, const double *oscale, double *grad, double *Kinv, int64_t ldk,
                              int64_t strideK, double *kinv_diag, void *partials, int q, const double *eig_lo, const double *Vd, void *stream);
int plmc_loo_grad_sum_f32(const float *Xop, int64_t n_pad, int64_t krows, int64_t ldx, int64_t strideX, const float *beta, const float *X,
                          int n, int d, int ncomp, const int *fam, const float *table, const float *oscale, double *grad, void *partials,
                          int q, void *stream);
int plmc_loo_grad_sum_f64(const double *Xop, int64_t n_pad, int64_t krows, int64_t ldx, int64_t strideX, const double *beta, const double *X,
                          int n, int d, int ncomp, const int *fam, const double *table, const double *oscale, double *grad, void *partials,
                          int q, void *stream);

/*
 * Leave-one-out objective (LeaveOneOutPseudoLikelihood, projected_lmc.py:86-105): with P = Khat^-1, alpha = P y, p_i = P_ii,
 *     L = sum_i [ 1/2 log p_i - 1/2 alpha_i^2 / p_i ] - n/2 log 2 pi,
 *     c_i = 1/2 / p_i + 1/2 alpha_i^2 / p_i^2,   g_i = -alpha_i / p_i,   u = P g = dL / dy,
 *     dL / dKhat = G = -[ P diag(c) P + 1/2 (alpha u^T + u alpha^T) ].
 * For any s > 0 and v+- = s alpha +- u / s:  2 G = beta beta^T - Xop^T Xop  with  beta = v- / sqrt 2  and
 *     Xop = [ diag(sqrt(2 c)) P ; v+^T / sqrt 2 ],
 * the full symmetric P with scaled rows and one more row.  That is the form (a a^T - X^T X) whose contraction with dKhat / dtheta the
 * epilogues of plmc_kinv_grad*_vd_* reduce, so the gradient of L is those epilogues behind another tile product.
 *
 * plmc_loo_grad*_: the arguments of the family's plmc_kinv_grad*_vd_* with (W, n_pad, ldw, strideW, alpha) replaced by
 *   (Xop, n_pad, krows, ldx, strideX, beta) and without Kinv, ldk, strideK, kinv_diag, eig_lo and Vd.
 *     grad[latent] = the family's gradient table (same layout, same reductions) of
 *                    1/2 sum_{i, j < n} (beta_i beta_j - [Xop^T Xop]_ij) dKhat_ij / dtheta.
 *   Xop: krows x n_pad per latent, K-major (row = contraction index), leading dimension ldx, batch stride strideX; every row in
 *   [0, krows) is contracted, so rows that carry nothing must be zero.  krows a multiple of 16, ldx a multiple of plmc_block() and >=
 *   n_pad, the pointer 16-byte aligned.  beta: q x n_pad.  `partials`: plmc_grad_partials_bytes(n_pad, q * ncomp),
 *   plmc_sm_grad_partials_bytes, plmc_per_grad_partials_bytes, plmc_lper_grad_partials_bytes as for the `_vd` calls.  With Xop = W (the inverse factor with zeros above
 *   its diagonal, krows = n_pad) and beta = alpha the call returns what plmc_kinv_grad*_vd_* returns.  Both element types form the
 *   product with the matrix instructions of that type (fp32: v_mfma_f32_16x16x4_f32 whatever PLMC_SPLIT says).  q n_pad^2 krows
 *   flop (upper tiles only).
 * plmc_loo_operand_*: Xop[k][i] = rowscale[k] P_ki for k, i < n from the upper triangle that plmc_kinv_grad*_vd_* writes into `Kinv`
 *   (n_pad x ldk per latent; what lies below the diagonal is not read), mirrored across the diagonal; exact zeros everywhere else in
 *   [0, krows) x [0, n_pad).  rowscale: q x n_pad.  krows >= n, a multiple of 16.  The caller writes the extra row afterwards.
 * Bad arguments fail through plmc_last_error() before anything is launched.
 */
int plmc_loo_grad_f32(int kind, const float *Xop, int64_t n_pad, int64_t krows, int64_t ldx, int64_t strideX, const float *beta,
                      const float *X, int n, int d, const float *ell, const float *oscale, double *grad, void *partials, int q,
                      void *stream);
int plmc_loo_grad_f64(int kind, const double *Xop, int64_t n_pad, int64_t krows, int64_t ldx, int64_t strideX, const double *beta,
                      const double *X, int n, int d, const double *ell, const double *oscale, double *grad, void *partials, int q,
                      void *stream);
int plmc_loo_grad_add_f32(int kind, const float *Xop, int64_t n_pad, int64_t krows, int64_t ldx, int64_t strideX, const float *beta,
                          const float *X, int n, int d, int ncomp, const float *ell, const float *oscale, double *grad, void *partials,
                          int q, void *stream);
int plmc_loo_grad_add_f64(int kind, const double *Xop, int64_t n_pad, int64_t krows, int64_t ldx, int64_t strideX, const double *beta,
                          const double *X, int n, int d, int ncomp, const double *ell, const double *oscale, double *grad, void *partials,
                          int q, void *stream);
int plmc_loo_grad_sm_f32(const float *Xop, int64_t n_pad, int64_t krows, int64_t ldx, int64_t strideX, const float *beta, const float *X,
                         int n, int d, int nmix, const float *scales, const float *means, const float *weights, double *grad,
                         void *partials, int q, void *stream);
int plmc_loo_grad_sm_f64(const double *Xop, int64_t n_pad, int64_t krows, int64_t ldx, int64_t strideX, const double *beta, const double *X,
                         int n, int d, int nmix, const double *scales, const double *means, const double *weights, double *grad,
                         void *partials, int q, void *stream);
int plmc_loo_grad_per_f32(const float *Xop, int64_t n_pad, int64_t krows, int64_t ldx, int64_t strideX, const float *beta, const float *X,
                          int n, int d, const float *ell, const float *period, const float *oscale, double *grad, void *partials, int q,
                          void *stream);
int plmc_loo_grad_per_f64(const double *Xop, int64_t n_pad, int64_t krows, int64_t ldx, int64_t strideX, const double *beta, const double *X,
                          int n, int d, const double *ell, const double *period, const double *oscale, double *grad, void *partials, int q,
                          void *stream);
int plmc_loo_operand_f32(const float *Kinv, int64_t n_pad, int64_t ldk, int64_t strideK, const float *rowscale, float *Xop, int64_t krows,
                         int64_t ldx, int64_t strideX, int n, int q, void *stream);
int plmc_loo_operand_f64(const double *Kinv, int64_t n_pad, int64_t ldk, int64_t strideK, const double *rowscale, double *Xop, int64_t krows,
                         int64_t ldx, int64_t strideX, int n, int q, void *stream);

/*
 * Weighted kernel-gradient sum: the gradient epilogues and reductions of plmc_kinv_grad*_vd_* behind the product of two general
 * operands.  For q latents with N points Z (N x d) each and the family's table theta,
 *     grad[latent][t] = sum_{i <= j < N} c_ij (At^T Bt)_ij dKhat(Z)_ij / dtheta_t ,   c_ii = 1, c_ij = 2 for i < j,
 * Khat(Z) = K(Z, Z) + noise I.  For a symmetric At^T Bt this is the full sum over i, j < N; for any other product it is the sum over the
 * upper triangle with these weights (what lies below the diagonal of At^T Bt is not formed).  The noise slot is sum_{i < N} (At^T Bt)_ii.
 * Use: the gradient of a loss of the posterior moments with respect to hyper-parameters and noise is this sum over the stacked points
 * Z = [X; X*] with a product of rank n* + 2 (or 2 for a loss of the mean alone), DESIGN.md 7.14.
 *
 * plmc_weighted_grad*_: the arguments of the family's plmc_kinv_grad*_vd_* with (W, n_pad, ldw, strideW, alpha, X, n) replaced by
 *   (At, Bt, r_pad, N_pad, ld, stride, Z, N) and without Kinv, ldk, strideK, kinv_diag, eig_lo and Vd.
 *   At, Bt: r_pad x N_pad per latent, K-major (row = contraction index), leading dimension ld, batch stride `stride` (elements); every
 *   row in [0, r_pad) is contracted and every column in [0, N_pad) enters a tile.  ZERO PADDING IS THE CALLER'S DUTY: rows that carry
 *   nothing and the columns [N, N_pad) of both operands must hold exact zeros (a NaN there reaches the sums of the last block row).
 *   Columns [N_pad, ld) and whatever lies behind the last latent's r_pad rows are not read; Z is read for rows < N only.
 *   r_pad a positive multiple of 16, N_pad a multiple of plmc_block() and >= N > 0, ld >= N_pad with 16-byte aligned rows, both pointers
 *   and `stride` 16-byte aligned, stride >= r_pad ld when q > 1.
 *   grad: the family's gradient table, same layout and width as plmc_kinv_grad*_vd_* writes it (double):
 *     plain [d ell: d | d noise | d oscale]; _add [ncomp x d | noise | ncomp]; _sm [scales: nmix x d | means: nmix x d | noise | weights:
 *     nmix]; _per [ell: d | period: d | noise | oscale]; _rq [ell: d | alpha | noise | oscale]; _lper [ell: d | period: d | rbf_ell: d |
 *     noise | oscale]; _sum [table: ncomp x (3 d + 1) | noise | oscale: ncomp]; _dot [var: d | offset | noise | oscale].
 *   partials: the family's size call evaluated at N_pad -- plmc_grad_partials_bytes(N_pad, q * ncomp), plmc_sm_grad_partials_bytes,
 *   plmc_per_grad_partials_bytes, plmc_lper_grad_partials_bytes, plmc_sum_grad_partials_bytes -- as for the `_vd` calls.
 *   Both element types form the product with the matrix instructions of that type (fp32: v_mfma_f32_16x16x4_f32 whatever PLMC_SPLIT
 *   says: the operands have no eigenvalue bound to scale a 16-bit split by).  Per-tile sums in fp64, reduced in a fixed order: two calls
 *   with the same arguments return the same bits.  q N_pad^2 r_pad flop (upper tiles only).
 * Bad arguments -- a null pointer, N <= 0, r_pad or N_pad off their granularity, ld < N_pad, d, components or power beyond the family's
 * plmc_*_max_* -- fail through plmc_last_error() before anything is launched.
 */
int plmc_weighted_grad_f32(int kind, const float *At, const float *Bt, int64_t r_pad, int64_t N_pad, int64_t ld, int64_t stride,
                           const float *Z, int N, int d, const float *ell, const float *oscale, double *grad, void *partials, int q,
                           void *stream);
int plmc_weighted_grad_f64(int kind, const double *At, const double *Bt, int64_t r_pad, int64_t N_pad, int64_t ld, int64_t stride,
                           const double *Z, int N, int d, const double *ell, const double *oscale, double *grad, void *partials, int q,
                           void *stream);
int plmc_weighted_grad_add_f32(int kind, const float *At, const float *Bt, int64_t r_pad, int64_t N_pad, int64_t ld, int64_t stride,
                               const float *Z, int N, int d, int ncomp, const float *ell, const float *oscale, double *grad, void *partials,
                               int q, void *stream);
int plmc_weighted_grad_add_f64(int kind, const double *At, const double *Bt, int64_t r_pad, int64_t N_pad, int64_t ld, int64_t stride,
                               const double *Z, int N, int d, int ncomp, const double *ell, const double *oscale, double *grad,
                               void *partials, int q, void *stream);
int plmc_weighted_grad_sm_f32(const float *At, const float *Bt, int64_t r_pad, int64_t N_pad, int64_t ld, int64_t stride, const float *Z,
                              int N, int d, int nmix, const float *scales, const float *means, const float *weights, double *grad,
                              void *partials, int q, void *stream);
int plmc_weighted_grad_sm_f64(const double *At, const double *Bt, int64_t r_pad, int64_t N_pad, int64_t ld, int64_t stride, const double *Z,
                              int N, int d, int nmix, const double *scales, const double *means, const double *weights, double *grad,
                              void *partials, int q, void *stream);
int plmc_weighted_grad_per_f32(const float *At, const float *Bt, int64_t r_pad, int64_t N_pad, int64_t ld, int64_t stride, const float *Z,
                               int N, int d, const float *ell, const float *period, const float *oscale, double *grad, void *partials,
                               int q, void *stream);
int plmc_weighted_grad_per_f64(const double *At, const double *Bt, int64_t r_pad, int64_t N_pad, int64_t ld, int64_t stride, const double *Z,
                               int N, int d, const double *ell, const double *period, const double *oscale, double *grad, void *partials,
                               int q, void *stream);
int plmc_weighted_grad_rq_f32(const float *At, const float *Bt, int64_t r_pad, int64_t N_pad, int64_t ld, int64_t stride, const float *Z,
                              int N, int d, const float *ell, const float *alpha, const float *oscale, double *grad, void *partials, int q,
                              void *stream);
int plmc_weighted_grad_rq_f64(const double *At, const double *Bt, int64_t r_pad, int64_t N_pad, int64_t ld, int64_t stride, const double *Z,
                              int N, int d, const double *ell, const double *alpha, const double *oscale, double *grad, void *partials,
                              int q, void *stream);
int plmc_weighted_grad_lper_f32(const float *At, const float *Bt, int64_t r_pad, int64_t N_pad, int64_t ld, int64_t stride, const float *Z,
                                int N, int d, const float *ell, const float *period, const float *rbf_ell, const float *oscale,
                                double *grad, void *partials, int q, void *stream);
int plmc_weighted_grad_lper_f64(const double *At, const double *Bt, int64_t r_pad, int64_t N_pad, int64_t ld, int64_t stride,
                                const double *Z, int N, int d, const double *ell, const double *period, const double *rbf_ell,
                                const double *oscale, double *grad, void *partials, int q, void *stream);
int plmc_weighted_grad_sum_f32(const float *At, const float *Bt, int64_t r_pad, int64_t N_pad, int64_t ld, int64_t stride, const float *Z,
                               int N, int d, int ncomp, const int *fam, const float *table, const float *oscale, double *grad,
                               void *partials, int q, void *stream);
int plmc_weighted_grad_sum_f64(const double *At, const double *Bt, int64_t r_pad, int64_t N_pad, int64_t ld, int64_t stride, const double *Z,
                               int N, int d, int ncomp, const int *fam, const double *table, const double *oscale, double *grad,
                               void *partials, int q, void *stream);
int plmc_weighted_grad_dot_f32(const float *At, const float *Bt, int64_t r_pad, int64_t N_pad, int64_t ld, int64_t stride, const float *Z,
                               int N, int d, const float *var, const float *offset, int power, const float *oscale, double *grad,
                               void *partials, int q, void *stream);
int plmc_weighted_grad_dot_f64(const double *At, const double *Bt, int64_t r_pad, int64_t N_pad, int64_t ld, int64_t stride, const double *Z,
                               int N, int d, const double *var, const double *offset, int power, const double *oscale, double *grad,
                               void *partials, int q, void *stream);

/*
 * Input gradients of the exact log density: d log N(y; 0, Khat) / dX for q latents that share the inputs X (n x d), the row-wise
 * pull-back of Omega = alpha alpha^T - Khat^-1 through the kernel's input derivative:
 *     gX[lat][i][k] = sum_{j < n, j != i} (alpha_i alpha_j - P_ij) d k_lat(x_i, x_j) / d x_i[k]          (gX: q x n x d doubles, contiguous)
 * -- no factor 1/2: x_i enters row i and column i of Khat.  The diagonal of these families does not depend on x.
 *   Kinv: P = Khat^-1 as plmc_kinv_grad*_vd_* writes it through its `Kinv` argument (n_pad x ldk per latent, batch stride strideK): P_ij is
 *   read at Kinv[min(i, j)][max(i, j)].  Nothing below the diagonal, no row or column at or beyond n (the identity padding) and nothing
 *   of alpha (q x n_pad) at or beyond n is read; those may hold anything.
 *   The table arguments are the family's, as in its plmc_kinv_grad*_vd_*; every family but the two named below is served: the stationary
 *   kinds 0..3 and their component table (a slot with ell = +inf gets exactly 0), the spectral mixture (a dimension with scale = mean = 0
 *   gets exactly 0), the periodic, the rational-quadratic and the locally periodic kernel, each up to its own limit on d.  Two
 *   coincident rows of X contribute nothing to each other (Matern-1/2: the convention of plmc_kernel_vjp_*).
 *   Every element of gX is written exactly once (no zero-initialised buffer), sums are fp64 in a fixed order without atomics (two calls
 *   give the same bits), no scratch.  Every stored element is read twice: q n^2 kernel-derivative evaluations.
 * Refused as argument errors: the spline kind, plmc_input_grad_sum_* and plmc_input_grad_dot_* (the diagonal of the spline and the
 * dot-product kernels depends on x); they exist because the families' entry points come from one list.
 * Bad arguments fail through plmc_last_error() before anything is launched.
 */
int plmc_input_grad_f32(int kind, const float *Kinv, int64_t n_pad, int64_t ldk, int64_t strideK, const float *alpha, const float *X, int n,
                        int d, const float *ell, const float *oscale, double *gX, int q, void *stream);
int plmc_input_grad_f64(int kind, const double *Kinv, int64_t n_pad, int64_t ldk, int64_t strideK, const double *alpha, const double *X, int n,
                        int d, const double *ell, const double *oscale, double *gX, int q, void *stream);
int plmc_input_grad_add_f32(int kind, const float *Kinv, int64_t n_pad, int64_t ldk, int64_t strideK, const float *alpha, const float *X,
                            int n, int d, int ncomp, const float *ell, const float *oscale, double *gX, int q, void *stream);
int plmc_input_grad_add_f64(int kind, const double *Kinv, int64_t n_pad, int64_t ldk, int64_t strideK, const double *alpha, const double *X,
                            int n, int d, int ncomp, const double *ell, const double *oscale, double *gX, int q, void *stream);
int plmc_input_grad_sm_f32(const float *Kinv, int64_t n_pad, int64_t ldk, int64_t strideK, const float *alpha, const float *X, int n, int d,
                           int nmix, const float *scales, const float *means, const float *weights, double *gX, int q, void *stream);
int plmc_input_grad_sm_f64(const double *Kinv, int64_t n_pad, int64_t ldk, int64_t strideK, const double *alpha, const double *X, int n, int d,
                           int nmix, const double *scales, const double *means, const double *weights, double *gX, int q, void *stream);
int plmc_input_grad_per_f32(const float *Kinv, int64_t n_pad, int64_t ldk, int64_t strideK, const float *alpha, const float *X, int n, int d,
                            const float *ell, const float *period, const float *oscale, double *gX, int q, void *stream);
int plmc_input_grad_per_f64(const double *Kinv, int64_t n_pad, int64_t ldk, int64_t strideK, const double *alpha, const double *X, int n, int d,
                            const double *ell, const double *period, const double *oscale, double *gX, int q, void *stream);
int plmc_input_grad_rq_f32(const float *Kinv, int64_t n_pad, int64_t ldk, int64_t strideK, const float *alpha, const float *X, int n, int d,
                           const float *ell, const float *shape, const float *oscale, double *gX, int q, void *stream);
int plmc_input_grad_rq_f64(const double *Kinv, int64_t n_pad, int64_t ldk, int64_t strideK, const double *alpha, const double *X, int n, int d,
                           const double *ell, const double *shape, const double *oscale, double *gX, int q, void *stream);
int plmc_input_grad_lper_f32(const float *Kinv, int64_t n_pad, int64_t ldk, int64_t strideK, const float *alpha, const float *X, int n, int d,
                             const float *ell, const float *period, const float *rbf_ell, const float *oscale, double *gX, int q,
                             void *stream);
int plmc_input_grad_lper_f64(const double *Kinv, int64_t n_pad, int64_t ldk, int64_t strideK, const double *alpha, const double *X, int n, int d,
                             const double *ell, const double *period, const double *rbf_ell, const double *oscale, double *gX, int q,
                             void *stream);
int plmc_input_grad_sum_f32(const float *Kinv, int64_t n_pad, int64_t ldk, int64_t strideK, const float *alpha, const float *X, int n, int d,
                            int ncomp, const int *fam, const float *table, const float *oscale, double *gX, int q, void *stream);
int plmc_input_grad_sum_f64(const double *Kinv, int64_t n_pad, int64_t ldk, int64_t strideK, const double *alpha, const double *X, int n, int d,
                            int ncomp, const int *fam, const double *table, const double *oscale, double *gX, int q, void *stream);
int plmc_input_grad_dot_f32(const float *Kinv, int64_t n_pad, int64_t ldk, int64_t strideK, const float *alpha, const float *X, int n, int d,
                            const float *var, const float *offset, int power, const float *oscale, double *gX, int q, void *stream);
int plmc_input_grad_dot_f64(const double *Kinv, int64_t n_pad, int64_t ldk, int64_t strideK, const double *alpha, const double *X, int n, int d,
                            const double *var, const double *offset, int power, const double *oscale, double *gX, int q, void *stream);

/*
 * Derivative of the eval-mode posterior moments with respect to the test inputs, for q latents on the training inputs X (n x d) and the
 * test inputs Xs (ns x d):
 *     Jm[lat][s][k] = d mean(s) / d x*_s[k] =      sum_{i < n} alpha_i d k_lat(x*_s, x_i) / d x*_s[k]
 *     Jv[lat][s][k] = d var(s)  / d x*_s[k] = -2 * sum_{i < n} B_is    d k_lat(x*_s, x_i) / d x*_s[k]         (Jm, Jv: q x ns x d doubles, contiguous)
 * with alpha = Khat^-1 y and B = Khat^-1 K*^T.  The diagonal of these families does not depend on x, and test points do not interact in
 * the marginal moments: Jm and Jv are the whole Jacobian.
 *   alpha: q x n_pad (n_pad >= n; any padding).  B: row i a training point, column s a test point, contiguous in s, ldb >= ns elements
 *   between rows, strideB between latents -- what a plmc_gemm_tn* call leaves.  B = NULL: only Jm is written, Jv is not touched (and may be
 *   NULL).  Nothing of alpha at or beyond n, no row of B at or beyond n and no column at or beyond ns is read; those may hold anything.
 *   The table arguments are the family's, as in its plmc_input_grad*, and so are the families served and their limits on d, the exact
 *   zeros (a slot with ell = +inf; a mixture dimension with scale = mean = 0) and the coincident points: a test point that coincides with a
 *   training point gets nothing from that pair (Matern-1/2: the convention of plmc_kernel_vjp_*).
 *   The unit derivative of a pair is evaluated once, with the accurate transcendental forms, and weighted by alpha_i and by -2 B_is in
 *   fp64.  Sums are fp64 in a fixed order without atomics (two calls give the same bits); every element of Jm (and Jv) is written exactly
 *   once; no private scratch.
 *   With few test points the training rows are split into plmc_posterior_dx_splits(n, ns, q) ranges, one workgroup each per block of 64
 *   test points and latent, a function of (n, ns, q) alone; their partial sums go through `partials`,
 *   plmc_posterior_dx_partials_bytes(n, ns, d, q) bytes (0 with one range: `partials` may then be NULL), and are added in the order of
 *   the ranges.  q n ns kernel-derivative evaluations; B is read once.
 * Refused as argument errors: the spline kind, plmc_posterior_dx_sum_* and plmc_posterior_dx_dot_* (the diagonal of the spline and the
 * dot-product kernels depends on x); they exist because the families' entry points come from one list.
 * Bad arguments (those, d beyond the family's limit, n < 1, ns < 1, a null pointer, ldb < ns) fail through plmc_last_error() before
 * anything is launched.
 */
int     plmc_posterior_dx_splits(int n, int ns, int q);
int64_t plmc_posterior_dx_partials_bytes(int n, int ns, int d, int q);
int plmc_posterior_dx_f32(int kind, const float *X, int n, const float *Xs, int ns, int d, const float *ell, const float *oscale, const float *alpha,
                          int64_t n_pad, const float *B, int64_t ldb, int64_t strideB, double *Jm, double *Jv, void *partials, int q, void *stream);
int plmc_posterior_dx_f64(int kind, const double *X, int n, const double *Xs, int ns, int d, const double *ell, const double *oscale, const double
                          *alpha, int64_t n_pad, const double *B, int64_t ldb, int64_t strideB, double *Jm, double *Jv, void *partials, int q, void
                          *stream);
int plmc_posterior_dx_add_f32(int kind, const float *X, int n, const float *Xs, int ns, int d, int ncomp, const float *ell, const float *oscale, const
                              float *alpha, int64_t n_pad, const float *B, int64_t ldb, int64_t strideB, double *Jm, double *Jv, void *partials, int
                              q, void *stream);
int plmc_posterior_dx_add_f64(int kind, const double *X, int n, const double *Xs, int ns, int d, int ncomp, const double *ell, const double *oscale,
                              const double *alpha, int64_t n_pad, const double *B, int64_t ldb, int64_t strideB, double *Jm, double *Jv, void
                              *partials, int q, void *stream);
int plmc_posterior_dx_sm_f32(const float *X, int n, const float *Xs, int ns, int d, int nmix, const float *scales, const float *means, const float
                             *weights, const float *alpha, int64_t n_pad, const float *B, int64_t ldb, int64_t strideB, double *Jm, double *Jv, void
                             *partials, int q, void *stream);
int plmc_posterior_dx_sm_f64(const double *X, int n, const double *Xs, int ns, int d, int nmix, const double *scales, const double *means, const
                             double *weights, const double *alpha, int64_t n_pad, const double *B, int64_t ldb, int64_t strideB, double *Jm, double
                             *Jv, void *partials, int q, void *stream);
int plmc_posterior_dx_per_f32(const float *X, int n, const float *Xs, int ns, int d, const float *ell, const float *period, const float *oscale, const
                              float *alpha, int64_t n_pad, const float *B, int64_t ldb, int64_t strideB, double *Jm, double *Jv, void *partials, int
                              q, void *stream);
int plmc_posterior_dx_per_f64(const double *X, int n, const double *Xs, int ns, int d, const double *ell, const double *period, const double *oscale,
                              const double *alpha, int64_t n_pad, const double *B, int64_t ldb, int64_t strideB, double *Jm, double *Jv, void
                              *partials, int q, void *stream);
int plmc_posterior_dx_rq_f32(const float *X, int n, const float *Xs, int ns, int d, const float *ell, const float *shape, const float *oscale, const
                             float *alpha, int64_t n_pad, const float *B, int64_t ldb, int64_t strideB, double *Jm, double *Jv, void *partials, int q,
                             void *stream);
int plmc_posterior_dx_rq_f64(const double *X, int n, const double *Xs, int ns, int d, const double *ell, const double *shape, const double *oscale,
                             const double *alpha, int64_t n_pad, const double *B, int64_t ldb, int64_t strideB, double *Jm, double *Jv, void
                             *partials, int q, void *stream);
int plmc_posterior_dx_lper_f32(const float *X, int n, const float *Xs, int ns, int d, const float *ell, const float *period, const float *rbf_ell,
                               const float *oscale, const float *alpha, int64_t n_pad, const float *B, int64_t ldb, int64_t strideB, double *Jm,
                               double *Jv, void *partials, int q, void *stream);
int plmc_posterior_dx_lper_f64(const double *X, int n, const double *Xs, int ns, int d, const double *ell, const double *period, const double
                               *rbf_ell, const double *oscale, const double *alpha, int64_t n_pad, const double *B, int64_t ldb, int64_t strideB,
                               double *Jm, double *Jv, void *partials, int q, void *stream);
int plmc_posterior_dx_sum_f32(const float *X, int n, const float *Xs, int ns, int d, int ncomp, const int *fam, const float *table, const float
                              *oscale, const float *alpha, int64_t n_pad, const float *B, int64_t ldb, int64_t strideB, double *Jm, double *Jv, void
                              *partials, int q, void *stream);
int plmc_posterior_dx_sum_f64(const double *X, int n, const double *Xs, int ns, int d, int ncomp, const int *fam, const double *table, const double
                              *oscale, const double *alpha, int64_t n_pad, const double *B, int64_t ldb, int64_t strideB, double *Jm, double *Jv, void
                              *partials, int q, void *stream);
int plmc_posterior_dx_dot_f32(const float *X, int n, const float *Xs, int ns, int d, const float *var, const float *offset, int power, const float
                              *oscale, const float *alpha, int64_t n_pad, const float *B, int64_t ldb, int64_t strideB, double *Jm, double *Jv, void
                              *partials, int q, void *stream);
int plmc_posterior_dx_dot_f64(const double *X, int n, const double *Xs, int ns, int d, const double *var, const double *offset, int power, const
                              double *oscale, const double *alpha, int64_t n_pad, const double *B, int64_t ldb, int64_t strideB, double *Jm, double
                              *Jv, void *partials, int q, void *stream);

/*
 * Products with a cross-covariance that is never written, for q latents on the training inputs X (n x d), the test inputs
 * Xs (ns x d) and r <= plmc_cross_matvec_max_cols() (8) columns V per latent:
 *     Out[lat][s][c] = sum_{i < n} k_lat(xs_s, x_i) V[lat][i][c]                      (Out: q x ns x r of the element type, contiguous)
 * k_lat is the noise-free value plmc_assemble_cross* writes for the same table arguments: the same value functions with the accurate
 * transcendental forms, the output scale included (oscale == NULL: 1), PLMC_SPLINE accepted by the plain entry point.  The posterior mean
 * at ns points is this with V = alpha = Khat^-1 y, at O(n ns) instead of a sweep over ns augmented columns; a pathwise posterior draw is
 * this with V = Khat^-1 (y - f_prior(X) - eps) beside plmc_rff_matvec.
 *   V: row i a training point, ldv >= r elements between rows, strideV between latents.  alpha (q x n_pad) is r = 1, ldv = 1,
 *   strideV = n_pad; the [alpha | B] rows the W^T product leaves are taken as they are.  No row of V or X at or beyond n and no column of V
 *   at or beyond r is read; those may hold anything.  Nothing outside Out[.][< ns][< r] is written.
 *   The value of a pair is of the element type; its products with V and the sums are fp64 in a fixed order without atomics (two calls give
 *   the same bits), rounded once.  Per element, u = 2^-24 / 2^-53 and b_F the family's bound on one value of plmc_assemble_cross*:
 *       |Out - exact| <= sum_i b_F |V_ic|  +  u |exact|  +  (n + 4) 2^-53 sum_i |k_i V_ic|.
 *   With few test points the training rows are split into plmc_cross_matvec_splits(n, ns, q) ranges, one workgroup each per block of 64
 *   test points and latent, a function of (n, ns, q) alone; their fp64 partial sums go through `partials`,
 *   plmc_cross_matvec_partials_bytes(n, ns, r, q) bytes (0 with one range: `partials` may then be NULL), and are added in the order of the
 *   ranges.  The order of the sums is a function of n alone -- segments of 256 rows (n > 16384: n / 64 rounded up to a multiple of 64),
 *   each summed by its four waves in a fixed order, the segments added in order; `partials` holds one fp64 sum per segment -- so an
 *   output element has the same bits whether or not the call splits and whatever other test points the call has.  q n ns kernel
 *   evaluations; no private scratch.
 * plmc_rff_matvec_*: the prior part of such a draw from m random Fourier features per latent,
 *     Out[lat][s][c] = scale[lat] sum_{j < m} cos(2 pi (sum_k freq[lat][j][k] xs_s[k] + phase[lat][j])) Wt[lat][j][c]
 * freq (q x m x d) and phase (q x m) IN REVOLUTIONS, Wt (q x m x r) and Out (q x ns x r) contiguous, scale (q) or NULL for 1, any m > 0,
 * d <= plmc_max_dim().  The phase is reduced in revolutions term by term (a product with its FMA residual, t - rint(t) exact, the running
 * sum folded back after every term), so one cosine is within 4 (d + 2) 2^-24 (fp32; 2^-53 for fp64) of the exact one of the same inputs
 * whatever the phase is, up to 2^18 revolutions per term.  Same skeleton, split (plmc_cross_matvec_splits(m, ns, q),
 * plmc_cross_matvec_partials_bytes(m, ns, r, q)), fixed-order fp64 sums and refusals.
 * Bad arguments (a null pointer, n, ns, r or q < 1, r over the cap, ldv < r, strideV < (n - 1) ldv + r with q > 1, the family's limits,
 * `partials` missing when the call splits) fail through plmc_last_error() before anything is launched.
 */
int     plmc_cross_matvec_max_cols(void);
int     plmc_cross_matvec_splits(int n, int ns, int q);
int64_t plmc_cross_matvec_partials_bytes(int n, int ns, int r, int q);
int plmc_cross_matvec_f32(int kind, const float *X, int n, const float *Xs, int ns, int d, const float *ell, const float *oscale, const float *V,
                          int64_t ldv, int64_t strideV, int r, float *Out, void *partials, int q, void *stream);
int plmc_cross_matvec_f64(int kind, const double *X, int n, const double *Xs, int ns, int d, const double *ell, const double *oscale, const double *V,
                          int64_t ldv, int64_t strideV, int r, double *Out, void *partials, int q, void *stream);
int plmc_cross_matvec_add_f32(int kind, const float *X, int n, const float *Xs, int ns, int d, int ncomp, const float *ell, const float *oscale, const
                              float *V, int64_t ldv, int64_t strideV, int r, float *Out, void *partials, int q, void *stream);
int plmc_cross_matvec_add_f64(int kind, const double *X, int n, const double *Xs, int ns, int d, int ncomp, const double *ell, const double *oscale,
                              const double *V, int64_t ldv, int64_t strideV, int r, double *Out, void *partials, int q, void *stream);
int plmc_cross_matvec_sm_f32(const float *X, int n, const float *Xs, int ns, int d, int nmix, const float *scales, const float *means, const float
                             *weights, const float *V, int64_t ldv, int64_t strideV, int r, float *Out, void *partials, int q, void *stream);
int plmc_cross_matvec_sm_f64(const double *X, int n, const double *Xs, int ns, int d, int nmix, const double *scales, const double *means, const
                             double *weights, const double *V, int64_t ldv, int64_t strideV, int r, double *Out, void *partials, int q, void *stream);
int plmc_cross_matvec_per_f32(const float *X, int n, const float *Xs, int ns, int d, const float *ell, const float *period, const float *oscale, const
                              float *V, int64_t ldv, int64_t strideV, int r, float *Out, void *partials, int q, void *stream);
int plmc_cross_matvec_per_f64(const double *X, int n, const double *Xs, int ns, int d, const double *ell, const double *period, const double *oscale,
                              const double *V, int64_t ldv, int64_t strideV, int r, double *Out, void *partials, int q, void *stream);
int plmc_cross_matvec_rq_f32(const float *X, int n, const float *Xs, int ns, int d, const float *ell, const float *shape, const float *oscale, const
                             float *V, int64_t ldv, int64_t strideV, int r, float *Out, void *partials, int q, void *stream);
int plmc_cross_matvec_rq_f64(const double *X, int n, const double *Xs, int ns, int d, const double *ell, const double *shape, const double *oscale,
                             const double *V, int64_t ldv, int64_t strideV, int r, double *Out, void *partials, int q, void *stream);
int plmc_cross_matvec_lper_f32(const float *X, int n, const float *Xs, int ns, int d, const float *ell, const float *period, const float *rbf_ell,
                               const float *oscale, const float *V, int64_t ldv, int64_t strideV, int r, float *Out, void *partials, int q, void
                               *stream);
int plmc_cross_matvec_lper_f64(const double *X, int n, const double *Xs, int ns, int d, const double *ell, const double *period, const double
                               *rbf_ell, const double *oscale, const double *V, int64_t ldv, int64_t strideV, int r, double *Out, void *partials, int
                               q, void *stream);
int plmc_cross_matvec_sum_f32(const float *X, int n, const float *Xs, int ns, int d, int ncomp, const int *fam, const float *table, const float
                              *oscale, const float *V, int64_t ldv, int64_t strideV, int r, float *Out, void *partials, int q, void *stream);
int plmc_cross_matvec_sum_f64(const double *X, int n, const double *Xs, int ns, int d, int ncomp, const int *fam, const double *table, const double
                              *oscale, const double *V, int64_t ldv, int64_t strideV, int r, double *Out, void *partials, int q, void *stream);
int plmc_cross_matvec_dot_f32(const float *X, int n, const float *Xs, int ns, int d, const float *var, const float *offset, int power, const float
                              *oscale, const float *V, int64_t ldv, int64_t strideV, int r, float *Out, void *partials, int q, void *stream);
int plmc_cross_matvec_dot_f64(const double *X, int n, const double *Xs, int ns, int d, const double *var, const double *offset, int power, const
                              double *oscale, const double *V, int64_t ldv, int64_t strideV, int r, double *Out, void *partials, int q, void *stream);
int plmc_rff_matvec_f32(const float *freq, const float *phase, int m, const float *Xs, int ns, int d, const float *Wt, int r, const float *scale,
                        float *Out, void *partials, int q, void *stream);
int plmc_rff_matvec_f64(const double *freq, const double *phase, int m, const double *Xs, int ns, int d, const double *Wt, int r, const double *scale,
                        double *Out, void *partials, int q, void *stream);

/*
 * Derivative of those products with respect to the test inputs, contracted with weights on the fly: what the gradient of
 * a pathwise posterior draw f_c(x) needs, without a cross-covariance-sized buffer.  plmc_cross_matvec_dx*_*: arguments as the value's
 * entry point of the same family, with `const T *G, double *Jx` in the place of `T *Out`,
 *     Jx[lat][s][k] = sum_{i < n} w_si  d k_lat(xs_s, x_i) / d xs_s[k],      w_si = sum_{c < r} G[lat][s][c] V[lat][i][c]
 * X (n x d) and Xs (ns x d) raw coordinates as plmc_posterior_dx_* takes them; V as above (ldv, strideV, r <= the cap); G (q x ns x r)
 * contiguous, the upstream gradient of Out; G == NULL is allowed with r == 1 only and means w_si = V[lat][i][0], the Jacobian of that one
 * column; Jx (q x ns x d) fp64 like Jm / Jv.  The unit derivative of a pair is evaluated once in the element type: the code and tables of
 * plmc_posterior_dx_* (accurate forms, a test point on a training point gets nothing from that pair); w_si and every sum are fp64.
 * Families: those of plmc_posterior_dx_*; the spline kind, the _sum and the _dot entry points are refused by name.
 *   Summation order: the contract of the values above, not the looser one of plmc_posterior_dx_*.  w over the columns in order; the rows
 *   in the same segments (256 rows; n > 16384: n / 64 rounded up to a multiple of 64), each summed by its four waves in a fixed order, the
 *   segments added in order.  The ranges are those of the values: plmc_cross_matvec_dx_splits(n, ns, q) of them, whose fp64 sums -- one
 *   per segment -- go through `partials`, plmc_cross_matvec_dx_partials_bytes(n, ns, d, q) bytes (0 with one range: `partials` may then be
 *   NULL).  An element of Jx has the same bits whether or not the call splits, whichever lane owns its test point and however many test
 *   points the call has; two calls give the same bits.  No atomics, no private scratch; nothing is read from rows >= n of X or V, columns
 *   >= r or test points >= ns, nothing outside Jx[.][< ns][< d] is written.  q n ns kernel-derivative evaluations.
 * plmc_rff_matvec_dx_*: the same for the prior part, arguments as plmc_rff_matvec_* with G in front of scale,
 *     Jx[lat][s][k] = -2 pi scale[lat] sum_{j < m} sin(2 pi (sum_k' freq[lat][j][k'] xs_s[k'] + phase[lat][j])) freq[lat][j][k] w_sj,
 *     w_sj = sum_{c < r} G[lat][s][c] Wt[lat][j][c]      (G == NULL, r == 1: Wt[lat][j][0])
 * The phase is reduced in revolutions exactly as the value's; the sine is the accurate one of the element type, within 4 (d + 2) u of the
 * exact one whatever the phase; its products with w_sj and freq are fp64.  Per element, u = 2^-24 / 2^-53:
 *     |Jx - exact| <= |scale| 2 pi [4 (d + 2) u sum_j |f_jk| |w_sj|  +  (m + 4) 2^-53 sum_j |sin_j f_jk w_sj|].
 * Bad arguments (a null pointer, n, ns, r or q < 1, r over the cap, ldv < r, strideV < (n - 1) ldv + r with q > 1, G == NULL with r > 1,
 * the family's limits, a refused family, `partials` missing when the call splits) fail through plmc_last_error() before anything is launched.
 */
int     plmc_cross_matvec_dx_splits(int n, int ns, int q);
int64_t plmc_cross_matvec_dx_partials_bytes(int n, int ns, int d, int q);
int plmc_cross_matvec_dx_f32(int kind, const float *X, int n, const float *Xs, int ns, int d, const float *ell, const float *oscale, const float *V,
                             int64_t ldv, int64_t strideV, int r, const float *G, double *Jx, void *partials, int q, void *stream);
int plmc_cross_matvec_dx_f64(int kind, const double *X, int n, const double *Xs, int ns, int d, const double *ell, const double *oscale,
                             const double *V, int64_t ldv, int64_t strideV, int r, const double *G, double *Jx, void *partials, int q, void *stream);
int plmc_cross_matvec_dx_add_f32(int kind, const float *X, int n, const float *Xs, int ns, int d, int ncomp, const float *ell, const float *oscale,
                                 const float *V, int64_t ldv, int64_t strideV, int r, const float *G, double *Jx, void *partials, int q,
                                 void *stream);
int plmc_cross_matvec_dx_add_f64(int kind, const double *X, int n, const double *Xs, int ns, int d, int ncomp, const double *ell, const double *oscale,
                                 const double *V, int64_t ldv, int64_t strideV, int r, const double *G, double *Jx, void *partials, int q,
                                 void *stream);
int plmc_cross_matvec_dx_sm_f32(const float *X, int n, const float *Xs, int ns, int d, int nmix, const float *scales, const float *means,
                                const float *weights, const float *V, int64_t ldv, int64_t strideV, int r, const float *G, double *Jx, void *partials,
                                int q, void *stream);
int plmc_cross_matvec_dx_sm_f64(const double *X, int n, const double *Xs, int ns, int d, int nmix, const double *scales, const double *means,
                                const double *weights, const double *V, int64_t ldv, int64_t strideV, int r, const double *G, double *Jx,
                                void *partials, int q, void *stream);
int plmc_cross_matvec_dx_per_f32(const float *X, int n, const float *Xs, int ns, int d, const float *ell, const float *period, const float *oscale,
                                 const float *V, int64_t ldv, int64_t strideV, int r, const float *G, double *Jx, void *partials, int q,
                                 void *stream);
int plmc_cross_matvec_dx_per_f64(const double *X, int n, const double *Xs, int ns, int d, const double *ell, const double *period,
                                 const double *oscale, const double *V, int64_t ldv, int64_t strideV, int r, const double *G, double *Jx,
                                 void *partials, int q, void *stream);
int plmc_cross_matvec_dx_rq_f32(const float *X, int n, const float *Xs, int ns, int d, const float *ell, const float *shape, const float *oscale,
                                const float *V, int64_t ldv, int64_t strideV, int r, const float *G, double *Jx, void *partials, int q, void *stream);
int plmc_cross_matvec_dx_rq_f64(const double *X, int n, const double *Xs, int ns, int d, const double *ell, const double *shape, const double *oscale,
                                const double *V, int64_t ldv, int64_t strideV, int r, const double *G, double *Jx, void *partials, int q,
                                void *stream);
int plmc_cross_matvec_dx_lper_f32(const float *X, int n, const float *Xs, int ns, int d, const float *ell, const float *period, const float *rbf_ell,
                                  const float *oscale, const float *V, int64_t ldv, int64_t strideV, int r, const float *G, double *Jx, void *partials,
                                  int q, void *stream);
int plmc_cross_matvec_dx_lper_f64(const double *X, int n, const double *Xs, int ns, int d, const double *ell, const double *period,
                                  const double *rbf_ell, const double *oscale, const double *V, int64_t ldv, int64_t strideV, int r, const double *G,
                                  double *Jx, void *partials, int q, void *stream);
int plmc_cross_matvec_dx_sum_f32(const float *X, int n, const float *Xs, int ns, int d, int ncomp, const int *fam, const float *table,
                                 const float *oscale, const float *V, int64_t ldv, int64_t strideV, int r, const float *G, double *Jx, void *partials,
                                 int q, void *stream);
int plmc_cross_matvec_dx_sum_f64(const double *X, int n, const double *Xs, int ns, int d, int ncomp, const int *fam, const double *table,
                                 const double *oscale, const double *V, int64_t ldv, int64_t strideV, int r, const double *G, double *Jx,
                                 void *partials, int q, void *stream);
int plmc_cross_matvec_dx_dot_f32(const float *X, int n, const float *Xs, int ns, int d, const float *var, const float *offset, int power,
                                 const float *oscale, const float *V, int64_t ldv, int64_t strideV, int r, const float *G, double *Jx, void *partials,
                                 int q, void *stream);
int plmc_cross_matvec_dx_dot_f64(const double *X, int n, const double *Xs, int ns, int d, const double *var, const double *offset, int power,
                                 const double *oscale, const double *V, int64_t ldv, int64_t strideV, int r, const double *G, double *Jx,
                                 void *partials, int q, void *stream);
int plmc_rff_matvec_dx_f32(const float *freq, const float *phase, int m, const float *Xs, int ns, int d, const float *Wt, int r, const float *G,
                           const float *scale, double *Jx, void *partials, int q, void *stream);
int plmc_rff_matvec_dx_f64(const double *freq, const double *phase, int m, const double *Xs, int ns, int d, const double *Wt, int r, const double *G,
                           const double *scale, double *Jx, void *partials, int q, void *stream);

/*
 * The one exchange of the sharded path, for a host without torch.distributed (the Python layer's default
 * is torch.distributed "nccl" = RCCL, `projectedlmc/parallel.py`, which can be switched to these with PLMC_COMM=rccl):
 * a direct RCCL all-reduce (sum, in place) of the fused [loss share | parameter gradients] buffer after backward
 * (experiments.py:270-272 on every rank) and of the (2, n*, p) partial prediction sums (projected_lmc.py:1144,1152).
 * RCCL is opened at run time (dlopen; no link-time dependency).  One communicator per process, bound to the device that is
 * current at plmc_comm_init.  Bootstrap: rank 0 calls plmc_comm_unique_id (128 bytes) and the host's launcher carries the
 * bytes to the other ranks (environment, file, MPI, a torch.distributed broadcast); then every rank calls plmc_comm_init.
 * plmc_comm_allreduce_sum_* is asynchronous on `stream`.  Returns 0 or a negative code (plmc_last_error()).
 */
int plmc_comm_unique_id(void *id128);
int plmc_comm_init(const void *id128, int rank, int world);
int plmc_comm_world(void);                    /* 0 without a communicator */
int plmc_comm_rank(void);                     /* -1 without a communicator */
int plmc_comm_allreduce_sum_f32(float *buf, int64_t count, void *stream);
int plmc_comm_allreduce_sum_f64(double *buf, int64_t count, void *stream);
int plmc_comm_destroy(void);

/*
 * Exact (dense) LMC / ICM: Kronecker-structured coregionalisation.
 * Replaces `MultitaskGPModel.forward` -> gpytorch LCMKernel / MultitaskKernel (:462-466, :586-589)
 * + MultitaskGaussianLikelihood (experiments.py:184) and their autograd backward:
 *     K_full = sum_i oscale_i k(X, X; ell_i) (x) B_i  +  I_n (x) Sigma      N = n*p rows, data-major
 *     interleaved (flat index = i_point * p + i_task), B: q x p x p, Sigma: p x p (both symmetric).
 * plmc_lmc_assemble_*  writes the upper tiles (identity padding up to plmc_pad(N)) of ONE factor buffer
 *                      (batch 1); it is then factorised by plmc_potrf_* like any other matrix.
 * plmc_lmc_cross_*     writes K_full(X, X*) (without Sigma) into columns [col0, col0 + ns*p).
 * plmc_lmc_kinv_grad_* fused K_full^-1 = W^T W + gradient reduction; grad (fp64) has
 *                      plmc_lmc_grad_len(p,q,d) entries laid out as
 *                        [ dB: q*p*p | d ell: q*d | d oscale: q | d Sigma: p*p ]
 *                      where dB / dSigma are accumulated over the UPPER triangle of K_full only
 *                      (weight 2 off the diagonal): the caller symmetrises them, (G + G^T) / 2.
 *                      partials: scratch of plmc_lmc_grad_scratch_bytes(N_pad, p, q, d) bytes.
 */
int64_t plmc_lmc_grad_len(int p, int q, int d);
int64_t plmc_lmc_grad_scratch_bytes(int64_t N_pad, int p, int q, int d);
int plmc_lmc_assemble_f32(int kind, const float *X, int n, int d, int p, int q, const float *ell,
                          const float *oscale, const float *B, const float *Sigma, float *A,
                          int64_t lda, void *stream);
int plmc_lmc_assemble_f64(int kind, const double *X, int n, int d, int p, int q, const double *ell,
                          const double *oscale, const double *B, const double *Sigma, double *A,
                          int64_t lda, void *stream);
int plmc_lmc_cross_f32(int kind, const float *X, int n, const float *Xs, int ns, int d, int p, int q,
                       const float *ell, const float *oscale, const float *B, float *Out, int64_t ldo,
                       int64_t col0, int64_t n_rows, void *stream);
int plmc_lmc_cross_f64(int kind, const double *X, int n, const double *Xs, int ns, int d, int p, int q,
                       const double *ell, const double *oscale, const double *B, double *Out,
                       int64_t ldo, int64_t col0, int64_t n_rows, void *stream);
int plmc_lmc_kinv_grad_f32(int kind, const float *W, int64_t N_pad, int64_t ldw, const float *alpha,
                           const float *X, int n, int d, int p, int q, const float *ell,
                           const float *oscale, const float *B, double *grad, void *partials,
                           void *stream);
int plmc_lmc_kinv_grad_f64(int kind, const double *W, int64_t N_pad, int64_t ldw, const double *alpha,
                           const double *X, int n, int d, int p, int q, const double *ell,
                           const double *oscale, const double *B, double *grad, void *partials,
                           void *stream);

/*
 * Vector-Jacobian product of a dense (cross-)covariance block K_i[a][b] = oscale_i k(|x1_a - x2_b| / ell_i)
 * given G = d loss / d K (q x n1 x n2, row stride ldg, batch stride strideG).  Row partials in fp64:
 *   gX1 [q][n1][d] = sum_b G dK/dx1_a,   gEll[q][n1][d] = sum_b G dK/d ell  (caller sums over rows),
 *   gOs [q][n1]    = sum_b G dK/d oscale.
 * Variational path: gradients of K_ZZ / K_ZX w.r.t. the learned inducing
 * locations and lengthscales of VariationalMultitaskGPModel (projected_lmc.py:686-766), which the
 * reference obtains from torch autograd through gpytorch's kernel evaluation (experiments.py:270).
 */
int plmc_kernel_vjp_f32(int kind, const float *X1, int n1, const float *X2, int n2, int d,
                        const float *ell, const float *oscale, const float *G, int64_t ldg,
                        int64_t strideG, double *gX1, double *gEll, double *gOs, int q, void *stream);
int plmc_kernel_vjp_f64(int kind, const double *X1, int n1, const double *X2, int n2, int d,
                        const double *ell, const double *oscale, const double *G, int64_t ldg,
                        int64_t strideG, double *gX1, double *gEll, double *gOs, int q, void *stream);

/*
 * Per-point noise: Khat = K + diag(noise[lat] + pnoise[lat][i]) -- a known or modelled observation variance per training point beside the
 * latent's scalar one (replicated simulator runs, Monte-Carlo standard errors, a parametric noise model, down-weighted observations).
 * Two operations, in the form of every family (PLMC_FAMILY_ENTRIES) and both element types:
 *   plmc_assemble<infix>_pn_*      the arguments of plmc_assemble<infix>_* with `pnoise, stride_pn` behind `noise`;
 *   plmc_factorize<infix>_pn_ex_*  the arguments of plmc_factorize<infix>_ex_* with `pnoise, stride_pn` behind `noise`: the fused call, same
 *                                  schedule (the first group's rows in front of the chain, the rest on the helper stream); the scan for
 *                                  the scales of the split engine reads the assembled diagonal, so it sees the per-point values.
 * Contract.  For i < n: A_ii = fl(a_ii + pnoise[lat * stride_pn + i]), where a_ii is exactly the value the entry point without `_pn`
 * writes (the kernel's k(x_i, x_i) and noise[lat] in their existing rounding) -- ONE further IEEE addition.  Every other element the call
 * writes is bit-identical to that entry point's output, the identity padding (rows and columns >= n, diagonal 1) included.
 * stride_pn = 0 shares one vector (n values) between the latents; otherwise stride_pn >= n and latent `lat` reads pnoise + lat * stride_pn.
 * pnoise == NULL ("null pointer") or 0 < stride_pn < n ("bad sizes") is an argument error, reported through plmc_last_error before anything
 * is launched.  The values must be finite and >= 0; the kernels do not look.
 * Eigenvalue bound: lambda_min(Khat) >= noise[lat] + min_i pnoise[lat][i], so for plmc_factorize*_pn_ex_* eig_lo[lat] must not exceed
 * noise[lat] + min_i pnoise[lat * stride_pn + i] (the callers of plmc_potrf_ex_* / plmc_potrs_aug_kept_* behind plmc_assemble*_pn_* pass
 * the same bound).  The sweep, the gradient kernels and every other entry point are unchanged: d logp / d pnoise_i =
 * 1/2 (alpha_i^2 - (Khat^-1)_ii) comes from alpha and the `kinv_diag` output of plmc_kinv_grad*_vd_*.
 */
int plmc_assemble_pn_f32(int kind, const float *X, int n, int d, const float *ell, const float *oscale, const float *noise, const float *pnoise,
                         int64_t stride_pn, float *A, int64_t lda, int64_t strideA, int q, void *stream);
int plmc_assemble_pn_f64(int kind, const double *X, int n, int d, const double *ell, const double *oscale, const double *noise, const double *pnoise,
                         int64_t stride_pn, double *A, int64_t lda, int64_t strideA, int q, void *stream);
int plmc_factorize_pn_ex_f32(int kind, const float *X, int n, int d, const float *ell, const float *oscale, const float *noise, const float *pnoise,
                             int64_t stride_pn, float *A, int64_t n_pad, int64_t lda, int naug, int64_t strideA, float *Vd, double *logdet,
                             int *info, int with_inverse, int q, const float *eig_lo, void *stream);
int plmc_factorize_pn_ex_f64(int kind, const double *X, int n, int d, const double *ell, const double *oscale, const double *noise,
                             const double *pnoise, int64_t stride_pn, double *A, int64_t n_pad, int64_t lda, int naug, int64_t strideA, double *Vd,
                             double *logdet, int *info, int with_inverse, int q, const double *eig_lo, void *stream);
int plmc_assemble_add_pn_f32(int kind, const float *X, int n, int d, int ncomp, const float *ell, const float *oscale, const float *noise,
                             const float *pnoise, int64_t stride_pn, float *A, int64_t lda, int64_t strideA, int q, void *stream);
int plmc_assemble_add_pn_f64(int kind, const double *X, int n, int d, int ncomp, const double *ell, const double *oscale, const double *noise,
                             const double *pnoise, int64_t stride_pn, double *A, int64_t lda, int64_t strideA, int q, void *stream);
int plmc_factorize_add_pn_ex_f32(int kind, const float *X, int n, int d, int ncomp, const float *ell, const float *oscale, const float *noise,
                                 const float *pnoise, int64_t stride_pn, float *A, int64_t n_pad, int64_t lda, int naug, int64_t strideA, float *Vd,
                                 double *logdet, int *info, int with_inverse, int q, const float *eig_lo, void *stream);
int plmc_factorize_add_pn_ex_f64(int kind, const double *X, int n, int d, int ncomp, const double *ell, const double *oscale, const double *noise,
                                 const double *pnoise, int64_t stride_pn, double *A, int64_t n_pad, int64_t lda, int naug, int64_t strideA,
                                 double *Vd, double *logdet, int *info, int with_inverse, int q, const double *eig_lo, void *stream);
int plmc_assemble_sm_pn_f32(const float *X, int n, int d, int nmix, const float *scales, const float *means, const float *weights,
                            const float *noise, const float *pnoise, int64_t stride_pn, float *A, int64_t lda, int64_t strideA, int q, void *stream);
int plmc_assemble_sm_pn_f64(const double *X, int n, int d, int nmix, const double *scales, const double *means, const double *weights,
                            const double *noise, const double *pnoise, int64_t stride_pn, double *A, int64_t lda, int64_t strideA, int q,
                            void *stream);
int plmc_factorize_sm_pn_ex_f32(const float *X, int n, int d, int nmix, const float *scales, const float *means, const float *weights,
                                const float *noise, const float *pnoise, int64_t stride_pn, float *A, int64_t n_pad, int64_t lda, int naug,
                                int64_t strideA, float *Vd, double *logdet, int *info, int with_inverse, int q, const float *eig_lo, void *stream);
int plmc_factorize_sm_pn_ex_f64(const double *X, int n, int d, int nmix, const double *scales, const double *means, const double *weights,
                                const double *noise, const double *pnoise, int64_t stride_pn, double *A, int64_t n_pad, int64_t lda, int naug,
                                int64_t strideA, double *Vd, double *logdet, int *info, int with_inverse, int q, const double *eig_lo, void *stream);
int plmc_assemble_per_pn_f32(const float *X, int n, int d, const float *ell, const float *period, const float *oscale, const float *noise,
                             const float *pnoise, int64_t stride_pn, float *A, int64_t lda, int64_t strideA, int q, void *stream);
int plmc_assemble_per_pn_f64(const double *X, int n, int d, const double *ell, const double *period, const double *oscale, const double *noise,
                             const double *pnoise, int64_t stride_pn, double *A, int64_t lda, int64_t strideA, int q, void *stream);
int plmc_factorize_per_pn_ex_f32(const float *X, int n, int d, const float *ell, const float *period, const float *oscale, const float *noise,
                                 const float *pnoise, int64_t stride_pn, float *A, int64_t n_pad, int64_t lda, int naug, int64_t strideA, float *Vd,
                                 double *logdet, int *info, int with_inverse, int q, const float *eig_lo, void *stream);
int plmc_factorize_per_pn_ex_f64(const double *X, int n, int d, const double *ell, const double *period, const double *oscale, const double *noise,
                                 const double *pnoise, int64_t stride_pn, double *A, int64_t n_pad, int64_t lda, int naug, int64_t strideA,
                                 double *Vd, double *logdet, int *info, int with_inverse, int q, const double *eig_lo, void *stream);
int plmc_assemble_rq_pn_f32(const float *X, int n, int d, const float *ell, const float *alpha, const float *oscale, const float *noise,
                            const float *pnoise, int64_t stride_pn, float *A, int64_t lda, int64_t strideA, int q, void *stream);
int plmc_assemble_rq_pn_f64(const double *X, int n, int d, const double *ell, const double *alpha, const double *oscale, const double *noise,
                            const double *pnoise, int64_t stride_pn, double *A, int64_t lda, int64_t strideA, int q, void *stream);
int plmc_factorize_rq_pn_ex_f32(const float *X, int n, int d, const float *ell, const float *alpha, const float *oscale, const float *noise,
                                const float *pnoise, int64_t stride_pn, float *A, int64_t n_pad, int64_t lda, int naug, int64_t strideA, float *Vd,
                                double *logdet, int *info, int with_inverse, int q, const float *eig_lo, void *stream);
int plmc_factorize_rq_pn_ex_f64(const double *X, int n, int d, const double *ell, const double *alpha, const double *oscale, const double *noise,
                                const double *pnoise, int64_t stride_pn, double *A, int64_t n_pad, int64_t lda, int naug, int64_t strideA,
                                double *Vd, double *logdet, int *info, int with_inverse, int q, const double *eig_lo, void *stream);
int plmc_assemble_lper_pn_f32(const float *X, int n, int d, const float *ell, const float *period, const float *rbf_ell, const float *oscale,
                              const float *noise, const float *pnoise, int64_t stride_pn, float *A, int64_t lda, int64_t strideA, int q,
                              void *stream);
int plmc_assemble_lper_pn_f64(const double *X, int n, int d, const double *ell, const double *period, const double *rbf_ell, const double *oscale,
                              const double *noise, const double *pnoise, int64_t stride_pn, double *A, int64_t lda, int64_t strideA, int q,
                              void *stream);
int plmc_factorize_lper_pn_ex_f32(const float *X, int n, int d, const float *ell, const float *period, const float *rbf_ell, const float *oscale,
                                  const float *noise, const float *pnoise, int64_t stride_pn, float *A, int64_t n_pad, int64_t lda, int naug,
                                  int64_t strideA, float *Vd, double *logdet, int *info, int with_inverse, int q, const float *eig_lo, void *stream);
int plmc_factorize_lper_pn_ex_f64(const double *X, int n, int d, const double *ell, const double *period, const double *rbf_ell,
                                  const double *oscale, const double *noise, const double *pnoise, int64_t stride_pn, double *A, int64_t n_pad,
                                  int64_t lda, int naug, int64_t strideA, double *Vd, double *logdet, int *info, int with_inverse, int q,
                                  const double *eig_lo, void *stream);
int plmc_assemble_sum_pn_f32(const float *X, int n, int d, int ncomp, const int *fam, const float *table, const float *oscale, const float *noise,
                             const float *pnoise, int64_t stride_pn, float *A, int64_t lda, int64_t strideA, int q, void *stream);
int plmc_assemble_sum_pn_f64(const double *X, int n, int d, int ncomp, const int *fam, const double *table, const double *oscale,
                             const double *noise, const double *pnoise, int64_t stride_pn, double *A, int64_t lda, int64_t strideA, int q,
                             void *stream);
int plmc_factorize_sum_pn_ex_f32(const float *X, int n, int d, int ncomp, const int *fam, const float *table, const float *oscale,
                                 const float *noise, const float *pnoise, int64_t stride_pn, float *A, int64_t n_pad, int64_t lda, int naug,
                                 int64_t strideA, float *Vd, double *logdet, int *info, int with_inverse, int q, const float *eig_lo, void *stream);
int plmc_factorize_sum_pn_ex_f64(const double *X, int n, int d, int ncomp, const int *fam, const double *table, const double *oscale,
                                 const double *noise, const double *pnoise, int64_t stride_pn, double *A, int64_t n_pad, int64_t lda, int naug,
                                 int64_t strideA, double *Vd, double *logdet, int *info, int with_inverse, int q, const double *eig_lo, void *stream);
int plmc_assemble_dot_pn_f32(const float *X, int n, int d, const float *var, const float *offset, int power, const float *oscale, const float *noise,
                             const float *pnoise, int64_t stride_pn, float *A, int64_t lda, int64_t strideA, int q, void *stream);
int plmc_assemble_dot_pn_f64(const double *X, int n, int d, const double *var, const double *offset, int power, const double *oscale,
                             const double *noise, const double *pnoise, int64_t stride_pn, double *A, int64_t lda, int64_t strideA, int q,
                             void *stream);
int plmc_factorize_dot_pn_ex_f32(const float *X, int n, int d, const float *var, const float *offset, int power, const float *oscale,
                                 const float *noise, const float *pnoise, int64_t stride_pn, float *A, int64_t n_pad, int64_t lda, int naug,
                                 int64_t strideA, float *Vd, double *logdet, int *info, int with_inverse, int q, const float *eig_lo, void *stream);
int plmc_factorize_dot_pn_ex_f64(const double *X, int n, int d, const double *var, const double *offset, int power, const double *oscale,
                                 const double *noise, const double *pnoise, int64_t stride_pn, double *A, int64_t n_pad, int64_t lda, int naug,
                                 int64_t strideA, double *Vd, double *logdet, int *info, int with_inverse, int q, const double *eig_lo, void *stream);

/*
 * Reduced Householder QR of ONE small matrix A (m x n row-major, plmc_qr_max() >= m >= n >= 1) in a single
 * launch: Q (m x n, orthonormal columns), R (n x n upper triangular, the lower part is written as zeros).
 * Replaces `torch.linalg.qr(self.H)` of LMCMixingMatrix.QR in bulk mode (projected_lmc.py:864-875, called at
 * :1015 and :1208) -- on the device ~45 dependent rocSOLVER launches per training step.  LAPACK xGEQR2 / xORG2R
 * sign convention (R_kk = -sign(a_kk) |a_k:m,k|; a column that is already zero below the diagonal keeps its sign),
 * i.e. the factors the reference's torch.linalg.qr returns, to rounding.
 */
int plmc_qr_max(void);
int plmc_qr_small_f32(const float *A, int m, int n, int64_t lda, float *Q, int64_t ldq, float *R, int64_t ldr,
                      void *stream);
int plmc_qr_small_f64(const double *A, int m, int n, int64_t lda, double *Q, int64_t ldq, double *R, int64_t ldr,
                      void *stream);

/*
 * Optional per-kernel profiler (measurement only; the reference's counterpart is the wall-clock
 * `time.time()` around its loops, experiments.py:261,284).  While enabled, kernel launches are
 * bracketed by two hipEvents on their launch stream: `on` = 0 none, 1 every kernel class, any other
 * value = (bit mask of class indices) << 1, so that a timed run can bracket the few heavy kernels
 * only (each bracket costs ~10 us of stream time, which matters on the latency-bound chain).  plmc_prof_collect() waits for the recorded
 * events, then returns per kernel class (index < plmc_prof_kernels(), name plmc_prof_name(i)):
 * total milliseconds, number of launches, and the ALGORITHMIC flops / bytes of those launches;
 * it clears the record.
 * Process-global state of the library (all of it): this profiler record; per device, TWO sets of two helper streams and
 * sixteen ordering events for the look-ahead in plmc_potrf_* (created on first use, never destroyed), each bound to the
 * caller stream that used it last.  Sweeps queued on one stream share a set (stream order protects it); sweeps from two
 * streams get a set each and may overlap on the device (their buffers must differ); a third stream takes over the least
 * recently used set and waits (stream-side, an event) for that set's last sweep.  Calls from several host THREADS are
 * serialised by one library-wide lock while they enqueue (the kernels overlap on the device as their streams allow); each
 * thread keeps its own choice of sweep set.  The Python layer calls from one thread per process.
 * Dev knobs are environment variables read once per process (PLMC_HALF_TILES, PLMC_GRP,
 * PLMC_SERIAL, PLMC_BULK_LDS, PLMC_CHAIN, PLMC_CHAIN_NW, PLMC_CHAIN_EDGE, PLMC_TAIL_PAIR); plmc_dev_reload_knobs() re-reads them (tests and bench.py change one and reload).  They change
 * schedules; PLMC_GRP and PLMC_TAIL_PAIR (1 = default: the split engines apply the far part of two consecutive trailing updates as one
 * product of twice the depth; 0 = one per group) also change the depth of the updates and with it the rounding.  PLMC_SPLIT (0, 2, 3) selects the
 * arithmetic of the bulk fp32 products (see plmc_potrf_ex_f32).  Buffer sizes do not depend on any knob.
 * plmc_prof_mfma_rate: dense MFMA rate (TFLOP/s) of the current device measured with a bare instruction stream
 * (v_mfma_f32_16x16x4_f32, _f64_16x16x4_f64 or v_mfma_f32_16x16x32_bf16, 4 waves per SIMD, no memory traffic); synchronous; `sink` = caller-owned
 * device scratch of at least 4 * CUs * 256 * sizeof(element) bytes.
 */
int         plmc_prof_enable(int on);         /* returns the previous setting */
int         plmc_prof_kernels(void);
const char *plmc_prof_name(int id);
int         plmc_prof_collect(double *ms, int64_t *launches, double *flops, double *bytes);
int         plmc_prof_mfma_rate(int kind, void *sink, int64_t sink_bytes, double *tflops);   /* kind: 0 f32, 1 f64, 2 bf16 (16x16x32) */
int         plmc_dev_reload_knobs(void);

#ifdef __cplusplus
}
#endif
#endif /* PLMC_H */
