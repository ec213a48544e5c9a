// api_common.hpp -- argument checking and error reporting shared by the extern "C" entry points.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "gemm_core.hpp"
#include "covariance.hpp"

namespace plmc {

constexpr int MAX_DIM = 32;          // largest input dimension handled by the fused kernels
constexpr int MAX_COMP = 4;          // most components of an additive kernel (plmc_max_components())
constexpr int SM_MAX_MIX = 8;        // most components of a spectral-mixture kernel (plmc_sm_max_mixtures())
constexpr int SM_MAX_DIM = 8;        // largest input dimension of a spectral-mixture kernel (plmc_sm_max_dim())
constexpr int PER_MAX_DIM = 8;       // largest input dimension of a periodic kernel (plmc_per_max_dim())
constexpr int RQ_MAX_DIM = 16;       // largest input dimension of a rational-quadratic kernel (plmc_rq_max_dim())
constexpr int LPER_MAX_DIM = 8;      // largest input dimension of a locally periodic kernel (plmc_lper_max_dim())
constexpr int DOT_MAX_DIM = 16;      // largest input dimension of a dot-product kernel (plmc_dot_max_dim())
constexpr int DOT_MAX_POWER = 8;     // largest power of a dot-product kernel (plmc_dot_max_power())
constexpr int SUM_MAX_DIM = 8;       // largest input dimension of a heterogeneous sum (plmc_sum_max_dim()): the smallest of its members' limits
// member families of a heterogeneous sum beside the stationary kinds K_RBF .. K_MATERN52: the public codes of include/plmc.h
// (PLMC_FAM_*) and the 4-bit codes the kernels get, packed one nibble per component
constexpr int FAM_PUBLIC_BASE = 16;  // PLMC_FAM_PERIODIC; PLMC_FAM_RQ and PLMC_FAM_LPER follow
enum { F_PER = 5, F_RQ = 6, F_LPER = 7 };

char *err_buf();                     // thread-local, defined in api.hip

inline int fail(const char *fn, const char *msg) {
  snprintf(err_buf(), 256, "%s: %s", fn, msg);
  return -1;
}

inline int launch_status(const char *fn) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    snprintf(err_buf(), 256, "%s: HIP launch failed: %s", fn, hipGetErrorString(e));
    return -2;
  }
  return 0;
}

#define PLMC_REQUIRE(cond, msg) \
  do { if (!(cond)) return plmc::fail(__func__, msg); } while (0)

// kernel classes known to the optional profiler (api.hip)
enum ProfKernel { PK_ASSEMBLE, PK_WRITE_RHS, PK_CROSS, PK_DIAG, PK_PANEL, PK_TRAIL, PK_WDIAG, PK_TRTRI, PK_EXTRACT,
                  PK_WTMV, PK_KINV_GRAD, PK_REDUCE, PK_VJP, PK_SWEEP, PK_TRAIL_ROW, PK_TRAIL_HEAD, PK_GPANEL, PK_SPLIT, PK_POST, PK_TRMM, PK_COUNT };

// Brackets the launches made while it is alive with two hipEvents (no-op unless its class is enabled, plmc_prof_enable).
// flops / bytes = ALGORITHMIC work of the bracketed launch (DESIGN.md gives the formulas).
struct ProfScope {
  ProfScope(int id, hipStream_t st, double flops, double bytes);
  ~ProfScope();
  long idx_;
  hipStream_t st_;
};

// Dev knobs (environment variables), read ONCE per process on first use; plmc_dev_reload_knobs() re-reads them (the
// tests and bench.py change a knob and reload).  They change schedules; PLMC_GRP and PLMC_TAIL_PAIR also change the depth of the
// updates (and with it the rounding), PLMC_SPLIT selects the arithmetic of the bulk fp32 products.
struct Knobs {
  double half_tiles;   // PLMC_HALF_TILES: 0 never, 1 always, N > 1 = tile-count threshold (default 640)
  int grp;             // PLMC_GRP: fixed group size of the sweep (default 0 = 8)
  bool serial;         // PLMC_SERIAL: one stream, no look-ahead
  int bulk_lds;        // PLMC_BULK_LDS: extra dynamic LDS bytes per bulk workgroup (caps bulk occupancy); -1 = default by q
  int split;           // PLMC_SPLIT: arithmetic of the bulk fp32 products (tail / head updates, group panel, K^-1): 0 = v_mfma_f32_16x16x4_f32
                       // everywhere; 3 = three bf16 planes, six products (bf3_engine.hpp SplitB3); 2 (default) = two fp16 planes, three
                       // products (SplitH2) where the caller gives eigenvalue bounds (plmc_*_ex_f32), SplitB3 otherwise
  int bulk_streams;    // PLMC_BULK_STREAMS: 2 = group panel + head rows on their own helper stream beside the tail, 1 = in front of the tail on the caller's stream
  int chain;           // PLMC_CHAIN: 1 (default) = the chain of a group as one resident launch (k_chain), 0 = three launches per block row
  int chain_edge;      // PLMC_CHAIN_EDGE: pool size for the first and the last two groups of a sweep (<= 0: as the others)
  int tail_pair;       // PLMC_TAIL_PAIR: 1 (default) = the split engines apply the far part of every second tail together with the next one, as one
                       // product of twice the depth (potrf.hip, Sweep::pair); 0 = one tail per group
  int chain_nw;        // PLMC_CHAIN_NW: pool workgroups of the resident chain beside the q critical ones (0 = by the number of latents)
};
const Knobs &knobs();

// One covariance table: what a kernel family hands to the host layer, and the ONE place a family is declared to it.  Only the extern "C"
// wrappers build one (from their flat arguments); assemble_impl, assemble_cross_impl, the sweep's AssembleJob and kinv_grad_impl take it.
//   PLAIN  one ARD kernel of `kind` (covariance.hpp): ell (q, d), oscale (q) | null
//   ADD    ncomp <= MAX_COMP stationary kernels of `kind` summed: ell (q, ncomp, d), oscale (q, ncomp) | null
//   SM     spectral mixture of ncomp components: ell = its scales, second = its means (q, ncomp, d), oscale = its weights (q, ncomp) | null
//   PER    periodic: ell = its lengthscales, second = its periods (q, d), oscale (q) | null
//   RQ     rational quadratic: ell = its lengthscales (q, d), second = its alpha (q), oscale (q) | null
//   LPER   locally periodic (periodic x RBF): ell = its periodic lengthscales, second = its periods, third = its RBF lengthscales (q, d
//          each), oscale (q) | null
//   SUM    heterogeneous sum of ncomp <= MAX_COMP members: ell = its table (q, ncomp, 3 d + 1), one record [ell | period | rbf_ell: d each |
//          alpha] per component, oscale (q, ncomp) | null; `fams` = the members' 4-bit codes (K_RBF .. K_MATERN52, F_PER, F_RQ, F_LPER), component g
//          in bits 4 g .. 4 g + 3, read from the caller's host array when the table is built (CovTable::sum)
//   DOT    dot product (linear / polynomial): ell = its variances v (q, d), second = its offset c (q), oscale (q) | null; ncomp = its
//          power P (power()), 1 <= P <= DOT_MAX_POWER -- one component, so the slot is free
// `kind` is not looked at for SM, PER, RQ, LPER, SUM and DOT; the pointers are of the call's element type.  `third` is null for every other family.
enum CovFamily { COV_PLAIN, COV_ADD, COV_SM, COV_PER, COV_RQ, COV_LPER, COV_SUM, COV_DOT };
struct CovTable {
  CovFamily family;
  int kind, d, ncomp;
  const void *ell, *second, *oscale;
  const void *third = nullptr;
  int fams = 0;                      // SUM only; < 0: the member list was refused (check()): -1 unknown code, -2 spline, -3 no list
  bool of_sum = false;               // the one member of a one-component sum, routed to its own family (member()): its gradient calls keep
                                     // scratch behind the partial sums, so they take the planes of W from the sweep's Vd only
  static CovTable plain(int kind, int d, const void *ell, const void *oscale) { return {COV_PLAIN, kind, d, 1, ell, nullptr, oscale}; }
  static CovTable add(int kind, int d, int ncomp, const void *ell, const void *oscale) { return {COV_ADD, kind, d, ncomp, ell, nullptr, oscale}; }
  static CovTable sm(int d, int nmix, const void *scales, const void *means, const void *weights) { return {COV_SM, 0, d, nmix, scales, means, weights}; }
  static CovTable per(int d, const void *ell, const void *period, const void *oscale) { return {COV_PER, 0, d, 1, ell, period, oscale}; }
  static CovTable rq(int d, const void *ell, const void *alpha, const void *oscale) { return {COV_RQ, 0, d, 1, ell, alpha, oscale}; }
  static CovTable lper(int d, const void *ell, const void *period, const void *rbf_ell, const void *oscale) {
    return {COV_LPER, 0, d, 1, ell, period, oscale, rbf_ell};
  }
  static CovTable dot(int d, int power, const void *v, const void *c, const void *oscale) { return {COV_DOT, 0, d, power, v, c, oscale}; }
  int power() const { return ncomp; }                             // DOT only
  // `fam`: HOST array of ncomp public codes (kind codes 0 .. 3, PLMC_FAM_PERIODIC, PLMC_FAM_RQ, PLMC_FAM_LPER)
  static CovTable sum(int d, int ncomp, const int *fam, const void *table, const void *oscale) {
    CovTable t{COV_SUM, 0, d, ncomp, table, nullptr, oscale};
    if (!fam) t.fams = -3;
    if (!fam || ncomp < 1 || ncomp > MAX_COMP) return t;          // (check() names what is wrong)
    for (int g = 0; g < ncomp; ++g) {
      const int f = fam[g];
      int code;
      if (f >= K_RBF && f <= K_MATERN52) code = f;
      else if (f >= FAM_PUBLIC_BASE && f <= FAM_PUBLIC_BASE + 2) code = F_PER + (f - FAM_PUBLIC_BASE);
      else { t.fams = f == K_SPLINE ? -2 : -1; return t; }
      t.fams |= code << (4 * g);
    }
    return t;
  }
  int fam_of(int g) const { return (fams >> (4 * g)) & 15; }
  // a one-component sum IS its member: that family's table for q latents whose rows are `stride` elements apart -- (q, d) contiguous rows
  // need stride = d, so the sum's own records (stride 3 d + 1) serve one latent at a time (lat0, q = 1) and re-laid rows serve all
  CovTable member(const void *ell_, const void *period_, const void *rbf_, const void *alpha_, const void *os_) const {
    const int f = fam_of(0);
    CovTable t = f == F_PER ? per(d, ell_, period_, os_) : f == F_RQ ? rq(d, ell_, alpha_, os_) : f == F_LPER ? lper(d, ell_, period_, rbf_, os_)
                                                                                                          : plain(f, d, ell_, os_);
    t.of_sum = true;
    return t;
  }
  template <typename T> CovTable member_of_latent(int lat) const {
    const T *rec = (const T *)ell + (int64_t)lat * (3 * d + 1);
    return member(rec, rec + d, rec + 2 * d, rec + 3 * d, oscale ? (const T *)oscale + lat : nullptr);
  }
  bool single_member() const { return family == COV_SUM && ncomp == 1; }
  // the family's limits: the message of the first one missed, or null
  const char *check() const {
    if (family == COV_SUM) {
      if (ncomp < 1 || ncomp > MAX_COMP) return "need 1 <= components <= plmc_sum_max_components()";
      if (d <= 0 || d > SUM_MAX_DIM) return "need 0 < d <= plmc_sum_max_dim()";
      if (fams == -3 || !ell) return "null pointer";
      if (fams == -2) return "the spline kernel is not a member of a sum (members: the stationary kinds 0..3, PLMC_FAM_PERIODIC, PLMC_FAM_RQ, PLMC_FAM_LPER)";
      if (fams < 0) return "unknown member family code (members: the stationary kinds 0..3, PLMC_FAM_PERIODIC, PLMC_FAM_RQ, PLMC_FAM_LPER; no spectral mixture)";
      return nullptr;
    }
    if (family == COV_ADD) {
      if (kind < 0 || kind > K_MATERN52) return "additive kernels take the stationary kinds only (no spline kernel)";
      if (ncomp < 1 || ncomp > MAX_COMP) return "need 1 <= components <= plmc_max_components()";
    } else if (family == COV_SM) {
      if (ncomp < 1 || ncomp > SM_MAX_MIX) return "need 1 <= mixtures <= plmc_sm_max_mixtures()";
      if (d <= 0 || d > SM_MAX_DIM) return "need 0 < d <= plmc_sm_max_dim()";
    } else if (family == COV_PER) {
      if (d <= 0 || d > PER_MAX_DIM) return "need 0 < d <= plmc_per_max_dim()";
    } else if (family == COV_RQ) {
      if (d <= 0 || d > RQ_MAX_DIM) return "need 0 < d <= plmc_rq_max_dim()";
    } else if (family == COV_LPER) {
      if (d <= 0 || d > LPER_MAX_DIM) return "need 0 < d <= plmc_lper_max_dim()";
      if (!third) return "null pointer";
    } else if (family == COV_DOT) {
      if (d <= 0 || d > DOT_MAX_DIM) return "need 0 < d <= plmc_dot_max_dim()";
      if (ncomp < 1 || ncomp > DOT_MAX_POWER) return "need 1 <= power <= plmc_dot_max_power()";
    }
    return (family == COV_SM || family == COV_PER || family == COV_RQ || family == COV_LPER || family == COV_DOT) && !second ? "null pointer" : nullptr;
  }
  // the family whose kernels run: an additive table of one component IS the plain kernel (ell (q, 1, d) is ell (q, d)) and takes the
  // plain instantiations, bit for bit
  CovFamily route() const { return family == COV_ADD && ncomp == 1 ? COV_PLAIN : family; }
  // rows of GP partial-sum slots per tile that the K^-1 + gradient kernels write (potri_grad.hip)
  int partials_rows() const { return family == COV_ADD || family == COV_SM || family == COV_SUM ? ncomp : 1; }
};
#define PLMC_REQUIRE_TABLE(t) \
  do { if (const char *why_ = (t).check()) return plmc::fail(__func__, why_); } while (0)

// Covariance assembly handed to the sweep (plmc_factorize*_ex_*): the sweep queues the rows of its first group on the caller's stream and
// the rest on a helper stream beside the first group's chain, instead of the caller assembling the whole matrix in front of the sweep.
// The sweep does not look at the table.
struct AssembleJob {
  CovTable table;
  int n;
  const void *X, *noise;
};
// block rows ib0 .. ib0 + nrows - 1 of the covariance matrices (assemble.hip), the first ncols block columns (< 0: all) without the
// leading skip x skip block triangle; elem_bytes 4 / 8
int assemble_rows(const AssembleJob &job, int elem_bytes, void *A, int64_t lda, int64_t strideA, int q, int ib0, int nrows, void *stream,
                  int ncols = -1, int skip = 0);

hipStream_t side_stream(int which = 0);   // per-device helper streams (api.hip), which in {0, 1}; nullptr on failure
hipEvent_t sync_event(int idx);     // per-device ordering events, idx in [0,16)
void bind_sweep_ctx(hipStream_t caller, int e_prev_idx);   // select the stream / event set of this caller stream (api.hip)

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace plmc
