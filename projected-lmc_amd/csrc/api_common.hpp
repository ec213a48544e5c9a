// api_common.hpp -- argument checking and error reporting shared by the extern "C" entry points.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <type_traits>

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
                  PK_WTMV, PK_KINV_GRAD, PK_REDUCE, PK_VJP, PK_SWEEP, PK_TRAIL_ROW, PK_TRAIL_HEAD, PK_GPANEL, PK_SPLIT, PK_POST, PK_TRMM, PK_INPUT_GRAD,
                  PK_POSTERIOR_DX, PK_CROSS_MATVEC, PK_CROSS_MATVEC_DX,
                  PK_COUNT };

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
// wrappers build one (from their flat arguments, PLMC_FAMILY_ENTRIES below); assemble_impl, assemble_cross_impl, the sweep's AssembleJob,
// kinv_grad_impl and loo_grad_impl take it.
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

// What the host layer knows about a family beside its table, one row per CovFamily in the order of the enumerators: CovTable::check(), the
// capacity ladder (with_capacity), the routing of the fp32 gradient call (potri_grad.hip, kinv_grad_any) and the occupancy floor of the
// gradient kernels (table_min_waves) read it; nothing else lists the families.
constexpr int EVERY_D = 1 << 30, NEVER = 1 << 30;
struct FamilyTraits {
  int max_dim;                       // the family's own limit on d (0: none, MAX_DIM by the entry points' checks) ...
  const char *dim_text;              // ... and the refusal
  int max_count;                     // largest ncomp -- components, mixtures or power (0: not looked at) ...
  const char *count_text;            // ... and the refusal
  bool count_first;                  // which of the two is checked first
  bool needs_second, needs_third;    // `second` / `third` must not be null
  bool rows_per_comp;                // the gradient kernels write one row of partial sums per component (else one)
  int max_dc;                        // largest capacity DC of its table kernels: the ladder is 1, 4, 8 [, 16]
  // largest d whose gradient epilogue runs beside the split engine's two fp16 / three bf16 planes without spilling (above it the fp32
  // products take the call whatever PLMC_SPLIT says): index NPL - 2.  The mixture keeps d sines, cosines and partial products per element
  // live beside the accumulators, the periodic kernel d sines, cosine complements and 2 d sums, the locally periodic one 3 d sums: that fits
  // the registers of the 256-thread fp32 kernel, not those of the 512-thread split-engine kernel, so d = 1 only (the reference's use).  A
  // heterogeneous sum may hold a periodic or a locally periodic member and follows their rule whatever its members are.  The
  // rational-quadratic and the dot-product epilogue fit beside the two planes at every d; beside the three (PLMC_SPLIT=3, or no eig_lo)
  // DC = 4, 8, 16 would spill.
  int split_max_d[2];
  const char *vd_noun;               // its split-engine gradient call takes the planes of W from the sweep's Vd only, and is refused by this
                                     // name otherwise (null: it may split W itself)
  int one_wave_dc[2];                // smallest DC at which k_kinv_grad_add / k_loo_grad_add ask for one wave per SIMD, not two: fp32, fp64
};
constexpr FamilyTraits FAMILY[] = {
    /* PLAIN */ {0, nullptr, 0, nullptr, false, false, false, false, 0, {EVERY_D, EVERY_D}, nullptr, {NEVER, NEVER}},
    /* ADD   */ {0, nullptr, MAX_COMP, "need 1 <= components <= plmc_max_components()", true, false, false, true, 0, {EVERY_D, EVERY_D}, nullptr,
                 {NEVER, NEVER}},
    /* SM    */ {SM_MAX_DIM, "need 0 < d <= plmc_sm_max_dim()", SM_MAX_MIX, "need 1 <= mixtures <= plmc_sm_max_mixtures()", true, true, false, true, 8,
                 {1, 1}, "spectral-mixture", {NEVER, 1}},
    /* PER   */ {PER_MAX_DIM, "need 0 < d <= plmc_per_max_dim()", 0, nullptr, false, true, false, false, 8, {1, 1}, "periodic", {NEVER, 2}},
    /* RQ    */ {RQ_MAX_DIM, "need 0 < d <= plmc_rq_max_dim()", 0, nullptr, false, true, false, false, 16, {EVERY_D, 1}, "rational-quadratic", {NEVER, 1}},
    /* LPER  */ {LPER_MAX_DIM, "need 0 < d <= plmc_lper_max_dim()", 0, nullptr, false, true, true, false, 8, {1, 1}, "locally periodic", {NEVER, 2}},
    /* SUM   */ {SUM_MAX_DIM, "need 0 < d <= plmc_sum_max_dim()", MAX_COMP, "need 1 <= components <= plmc_sum_max_components()", true, false, false, true,
                 8, {1, 1}, "sum", {5, 1}},
    /* DOT   */ {DOT_MAX_DIM, "need 0 < d <= plmc_dot_max_dim()", DOT_MAX_POWER, "need 1 <= power <= plmc_dot_max_power()", false, true, false, false, 16,
                 {EVERY_D, 1}, "dot-product", {NEVER, 1}},
};
static_assert(sizeof(FAMILY) / sizeof(FAMILY[0]) == COV_DOT + 1, "one row per CovFamily");

// occupancy floor (the second __launch_bounds__ argument) of the table families' gradient kernels
template <typename T, CovFamily F, int DC> constexpr int table_min_waves() { return DC >= FAMILY[F].one_wave_dc[sizeof(T) == 8] ? 1 : 2; }

// The ONE capacity ladder of the table families (COV_SM .. COV_DOT): call(F, DC) with the family and the smallest capacity DC in {1, 4, 8
// [, 16]} that holds d, both as std::integral_constant -- the callable is the launch of its site.  PLANES = 0: every d up to the family's
// limit; PLANES = 2 / 3: the kernels that run beside that many planes of the split engine, i.e. DC = 1 alone where
// FamilyTraits::split_max_d says so (no other instance exists there: it would spill, and the routing keeps d > 1 away).  COV_PLAIN and
// COV_ADD have their own kernels and rules at every site and do not come here.
template <int PLANES, CovFamily F, class Call>
void with_capacity_of(int d, Call &&call) {
  constexpr std::integral_constant<CovFamily, F> f{};
  constexpr int top = PLANES != 0 && FAMILY[F].split_max_d[PLANES == 3] == 1 ? 1 : FAMILY[F].max_dc;   // 1, 8 or 16
  if constexpr (top == 1) call(f, std::integral_constant<int, 1>());
  else {
    if (d == 1) call(f, std::integral_constant<int, 1>());
    else if (d <= 4) call(f, std::integral_constant<int, 4>());
    else if (top == 8 || d <= 8) call(f, std::integral_constant<int, 8>());
    else call(f, std::integral_constant<int, top>());
  }
}
template <int PLANES, class Call>
void with_capacity(CovFamily family, int d, Call &&call) {
  switch (family) {                  // (in the order the gradient kernels have in the code object: potri_grad.hip, kinv_grad_any)
    case COV_PER: with_capacity_of<PLANES, COV_PER>(d, call); break;
    case COV_LPER: with_capacity_of<PLANES, COV_LPER>(d, call); break;
    case COV_SUM: with_capacity_of<PLANES, COV_SUM>(d, call); break;
    case COV_RQ: with_capacity_of<PLANES, COV_RQ>(d, call); break;
    case COV_DOT: with_capacity_of<PLANES, COV_DOT>(d, call); break;
    case COV_SM: with_capacity_of<PLANES, COV_SM>(d, call); break;
    case COV_PLAIN: case COV_ADD: break;
  }
}

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
    const FamilyTraits &f = FAMILY[family];
    if (family == COV_ADD && (kind < 0 || kind > K_MATERN52)) return "additive kernels take the stationary kinds only (no spline kernel)";
    const char *count = f.max_count && (ncomp < 1 || ncomp > f.max_count) ? f.count_text : nullptr;
    const char *dim = f.max_dim && (d <= 0 || d > f.max_dim) ? f.dim_text : nullptr;
    if (count || dim) return f.count_first ? (count ? count : dim) : (dim ? dim : count);
    if (family == COV_SUM) {
      if (fams == -3 || !ell) return "null pointer";
      if (fams == -2) return "the spline kernel is not a member of a sum (members: the stationary kinds 0..3, PLMC_FAM_PERIODIC, PLMC_FAM_RQ, PLMC_FAM_LPER)";
      if (fams < 0) return "unknown member family code (members: the stationary kinds 0..3, PLMC_FAM_PERIODIC, PLMC_FAM_RQ, PLMC_FAM_LPER; no spectral mixture)";
    }
    return (f.needs_third && !third) || (f.needs_second && !second) ? "null pointer" : nullptr;
  }
  // the family whose kernels run: an additive table of one component IS the plain kernel (ell (q, 1, d) is ell (q, d)) and takes the
  // plain instantiations, bit for bit
  CovFamily route() const { return family == COV_ADD && ncomp == 1 ? COV_PLAIN : family; }
  // rows of GP partial-sum slots per tile that the K^-1 + gradient kernels write (potri_grad.hip)
  int partials_rows() const { return FAMILY[family].rows_per_comp ? ncomp : 1; }
  // what the gradient kernels get as `kind`: a sum's carries its members
  int kernel_kind() const { return family == COV_SUM ? fams : kind; }
  // FamilyTraits::vd_noun of the call: the one member of a sum keeps scratch behind the partial sums (of_sum), so it follows the sum
  const char *vd_noun() const { return FAMILY[of_sum ? COV_SUM : route()].vd_noun; }
};
#define PLMC_REQUIRE_TABLE(t) \
  do { if (const char *why_ = (t).check()) return plmc::fail(__func__, why_); } while (0)

// The ONE list of the families' extern "C" entry points (include/plmc.h declares them by hand; every .hip file includes it, so the compiler
// holds each generated wrapper against its declaration).  X(SUF, T, infix, LEAD, (flat table arguments), table): the entry points of a
// family are plmc_<operation><infix>..._<SUF>, their first argument is `int kind` where LEAD is KIND, and where the plain entry point has
// `int d, const T *ell, const T *oscale` they have `int d` and the flat table arguments, from which `table` builds the CovTable.  Each
// operation defines its wrappers for both element types with one body:
//   PLMC_FAMILY_ENTRIES(MY_ENTRY, f32, float) PLMC_FAMILY_ENTRIES(MY_ENTRY, f64, double)
// (`shape` is the rational-quadratic alpha: `alpha` is K^-1 y in the gradient entry points.)
#define PLMC_LEAD_KIND int kind,
#define PLMC_LEAD_NO_KIND
#define PLMC_UNPACK(...) __VA_ARGS__
#define PLMC_FAMILY_ENTRIES(X, SUF, T)                                                                                                        \
  X(SUF, T, , KIND, (const T *ell, const T *oscale), plmc::CovTable::plain(kind, d, ell, oscale))                                             \
  X(SUF, T, _add, KIND, (int ncomp, const T *ell, const T *oscale), plmc::CovTable::add(kind, d, ncomp, ell, oscale))                         \
  X(SUF, T, _sm, NO_KIND, (int nmix, const T *scales, const T *means, const T *weights), plmc::CovTable::sm(d, nmix, scales, means, weights)) \
  X(SUF, T, _per, NO_KIND, (const T *ell, const T *period, const T *oscale), plmc::CovTable::per(d, ell, period, oscale))                     \
  X(SUF, T, _rq, NO_KIND, (const T *ell, const T *shape, const T *oscale), plmc::CovTable::rq(d, ell, shape, oscale))                         \
  X(SUF, T, _lper, NO_KIND, (const T *ell, const T *period, const T *rbf_ell, const T *oscale),                                               \
    plmc::CovTable::lper(d, ell, period, rbf_ell, oscale))                                                                                    \
  X(SUF, T, _sum, NO_KIND, (int ncomp, const int *fam, const T *table, const T *oscale), plmc::CovTable::sum(d, ncomp, fam, table, oscale))   \
  X(SUF, T, _dot, NO_KIND, (const T *var, const T *offset, int power, const T *oscale), plmc::CovTable::dot(d, power, var, offset, oscale))

// Covariance assembly handed to the sweep (plmc_factorize*_ex_*): the sweep queues the rows of its first group on the caller's stream and
// the rest on a helper stream beside the first group's chain, instead of the caller assembling the whole matrix in front of the sweep.
// The sweep does not look at the table.
struct AssembleJob {
  CovTable table;
  int n;
  const void *X, *noise;
  const void *pnoise = nullptr;      // per-point noise (plmc_factorize*_pn_ex_*): stride_pn elements between the latents' vectors, 0 = one for all
  int64_t stride_pn = 0;
};
// the per-point arguments of the *_pn entry points, checked before anything is launched
#define PLMC_REQUIRE_POINT_NOISE(pnoise, stride_pn, n)                                                                                        \
  do {                                                                                                                                        \
    PLMC_REQUIRE((pnoise) != nullptr, "null pointer");                                                                                        \
    PLMC_REQUIRE((stride_pn) == 0 || (stride_pn) >= (n), "bad sizes (stride_pn is 0, one vector for every latent, or >= n)");                 \
  } while (0)
// block rows ib0 .. ib0 + nrows - 1 of the covariance matrices (assemble.hip), the first ncols block columns (< 0: all) without the
// leading skip x skip block triangle; elem_bytes 4 / 8
int assemble_rows(const AssembleJob &job, int elem_bytes, void *A, int64_t lda, int64_t strideA, int q, int ib0, int nrows, void *stream,
                  int ncols = -1, int skip = 0);

hipStream_t side_stream(int which = 0);   // per-device helper streams (api.hip), which in {0, 1}; nullptr on failure
hipEvent_t sync_event(int idx);     // per-device ordering events, idx in [0,16)
void bind_sweep_ctx(hipStream_t caller, int e_prev_idx);   // select the stream / event set of this caller stream (api.hip)

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace plmc
