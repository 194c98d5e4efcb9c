// spamtree_hip.hip -- gfx950 kernels + C-ABI for spamtree's per-Gibbs-sweep DAG-node linear algebra.
//
// What each kernel replaces in the reference (paths relative to /root/reference/src):
//   k_factor<MODE_FACTOR>  spamtree_model.cpp:834-998  get_loglik_comps_w_std  (phase A)  + covariance_functions.cpp:95-111, 213-286
//   k_factor<MODE_PREDICT> spamtree_model.cpp:1234-1358 predict_std            (phase P)
//   k_sample               spamtree_model.cpp:1011-1226 gibbs_sample_w_std     (phase B)
//   k_loglik               spamtree_model.cpp:781-826  get_loglik_w_std        (phase C)
//   k_stats / k_xb         spamtree_model.cpp:1374-1375, 1382, 1397-1400       (beta / tausq sufficient statistics)
//
// Design (DESIGN.md has the derivation): the reference materialises, per block u with ancestor rows PI_u,
// H_u = K_{u,pa} K_{pa,pa}^{-1}, the dense (P+m)^2 inverse Cholesky of K_{[pa,u]} and its Gram matrix.  The inverse
// Cholesky of an ancestor set is block lower triangular and its row panel for block a is [-Ri_a H_a | Ri_a]
// (tree_utils.cpp:204-206), so this build stores exactly ONE array per block, that panel ("Linv panel",
// m x (P+m), row-major), and every phase works from the chain of ancestor panels:
//   V = Linv_pa * K_{pa,u}            (one pass over the chain, ancestors last-to-first so V overwrites K in place)
//   T = V' * Linv_pa = H_u            (accumulated in the same pass)
//   R = K_uu - V'V,  Ri = chol(R)^{-1},  panel_u = [-Ri*T | Ri]
// Messages to ancestors are pushed as per-ancestor (m_a x m_a, m_a) pairs and summed hierarchically through
// direct children in a fixed order (no FP64 atomics -> bit-reproducible for any launch geometry).
//
// This translation unit is the HOST side: handle (st_handle.hpp) and its lifecycle, the iteration's C-ABI with every launch of
// the fit, inspection, measurement and st_cross_covariance_ag10.  The feature families have their C-ABI and their state in host
// units of their own: new-point prediction in st_points.hip, the criteria over the fit's rows, leave-one-out and Pareto smoothing
// in st_rows.hip, prior simulation in st_simulate.hip, the running summaries in st_summary.hip.  tree_layout.cpp builds the launch
// structures without a device call (the handle derives from its TreeLayout).  The kernels live in one translation unit per family
// (k_factor_*.hip, k_sample.hip, k_misc.hip); the headers included here give their argument structures, constants and prototypes.

#include "st_handle.hpp"
#include "misc_kernels.hpp"
#include <new>

// ===============================================================================================================
// host side
// ===============================================================================================================
static thread_local std::string g_create_error;

// route codes (st_route_info): written by the launch sites themselves; st_route_name spells them as the source does
enum RouteCode : int {
  R_NONE = ST_ROUTE_NONE,
  R_MARGINAL_INVCHOL_WAVE, R_MARGINAL_INVCHOL,
  R_FACTOR_LDS, R_FACTOR_SCRATCH, R_PREDICT_LDS, R_PREDICT_SCRATCH,
  R_QUAD32_REF_WCH, R_QUAD32_REF, R_QUAD32_LEAF, R_QUAD38_REF_WCH, R_QUAD38_REF, R_QUAD38_LEAF,
  R_QUAD44_REF_WCH, R_QUAD44_REF, R_QUAD44_LEAF, R_QUAD50_REF_WCH, R_QUAD50_REF, R_QUAD50_LEAF,
  R_FACTOR_MFMA, R_LCHAIN96, R_LCHAIN136, R_REF_FINISH, R_LCHAIN_SCALARS, R_FACTOR_WIDE, R_BIGMFMA3, R_BIGMFMA4, R_BIGMFMA5,
  R_GRAM, R_GRAM_DIRECT, R_GRAM_BIG,
  R_SAMPLE_MFMA, R_LEAF_SEG4, R_LEAF_SEG6, R_SAMPLE_LEAF, R_SAMPLE_WAVE, R_SAMPLE_LEAN_LAT, R_SAMPLE_LEAN,
  R_SAMPLE_BIG_REF, R_SAMPLE_LEAF_WIDE, R_SAMPLE_BIG_LEAF, R_SAMPLE_SMALL,
  R_COUNT
};
static const char *const k_route_names[R_COUNT] = {
  "",
  "k_marginal_invchol_wave", "k_marginal_invchol",
  "k_factor<false, MODE_FACTOR>", "k_factor<true, MODE_FACTOR>", "k_factor<false, MODE_PREDICT>", "k_factor<true, MODE_PREDICT>",
  "k_factor_quad<4, 32, 8, true, true>", "k_factor_quad<4, 32, 8, true, false>", "k_factor_quad<4, 32, 8, false, true>",
  "k_factor_quad<4, 38, 10, true, true>", "k_factor_quad<4, 38, 10, true, false>", "k_factor_quad<4, 38, 10, false, true>",
  "k_factor_quad<4, 44, 11, true, true>", "k_factor_quad<4, 44, 11, true, false>", "k_factor_quad<4, 44, 11, false, true>",
  "k_factor_quad<4, 50, 13, true, true>", "k_factor_quad<4, 50, 13, true, false>", "k_factor_quad<4, 50, 13, false, true>",
  "k_factor_mfma", "k_factor_lchain<96>", "k_factor_lchain<136>", "k_factor_ref_finish", "k_lchain_scalars", "k_factor_wide<WG_JT>",
  "k_factor_bigmfma<3, 5, 34>", "k_factor_bigmfma<4, 5, 34>", "k_factor_bigmfma<5, 3, 24>",
  "k_gram", "k_gram_direct", "k_gram_big",
  "k_sample_mfma", "k_sample_leaf_seg<4>", "k_sample_leaf_seg<6>", "k_sample_leaf", "k_sample_wave", "k_sample_lean<true>",
  "k_sample_lean<false>", "k_sample<true, false>", "k_sample_leaf_wide", "k_sample<true, true>", "k_sample<false>",
};

static int fail_create(st_handle_s *h, int code, const std::string &msg) {
  g_create_error = msg;
  if (h) {
    st_destroy(h);
  }
  return code;
}

// The statistics kernel for q outcomes: k_stats<q, false> (xty and ssq), or k_stats<q, true> (the row weight is a column of X).
typedef void (*StatsKernel)(const double *, const double *, const double *, const double *, const int *, const unsigned char *,
                            const long long *, const double *, long long, int, double *);
static StatsKernel stats_kernel(int q, bool xtx) {
  static const StatsKernel tab[2][QMAX] = {
      {k_stats<1, false>, k_stats<2, false>, k_stats<3, false>, k_stats<4, false>, k_stats<5, false>, k_stats<6, false>},
      {k_stats<1, true>, k_stats<2, true>, k_stats<3, true>, k_stats<4, true>, k_stats<5, true>, k_stats<6, true>}};
  return tab[xtx ? 1 : 0][q - 1];
}
// ... over all rows into d_partial: one slice of eight columns of X per grid row.  wt: the weight column (XtX), or null.
static void launch_stats(st_handle_s *h, hipStream_t st, const double *wt) {
  const StatsKernel k_stats = stats_kernel(h->q, wt != nullptr);
  hipLaunchKernelGGL(k_stats, dim3(STATS_WG, (h->p + 7) / 8), dim3(NT), 0, st, h->d_X.p, h->d_y.p, h->d_w.p, h->d_xb.p, h->d_mv.p,
                     h->d_obs.p, h->d_partner.p, wt, h->n_all, h->p, h->d_partial.p);
}

// The instantiations of k_factor_quad, in the order of their route codes: chain rows nkx = 32 / 38 / 44 / 50 (`size` 0 .. 3), each as
// <.., true, true> (reference level, wave Cholesky), <.., true, false> (reference level) and <.., false, true> (leaf) (`kind` 0 .. 2).
typedef void (*QuadKernel)(QuadArgs, CovPar);
constexpr int QUAD_SIZES = 4, QUAD_KINDS = 3;
static QuadKernel quad_kernel(int size, int kind) {
  static const QuadKernel tab[QUAD_SIZES][QUAD_KINDS] = {
      {k_factor_quad<4, 32, 8, true, true>, k_factor_quad<4, 32, 8, true, false>, k_factor_quad<4, 32, 8, false, true>},
      {k_factor_quad<4, 38, 10, true, true>, k_factor_quad<4, 38, 10, true, false>, k_factor_quad<4, 38, 10, false, true>},
      {k_factor_quad<4, 44, 11, true, true>, k_factor_quad<4, 44, 11, true, false>, k_factor_quad<4, 44, 11, false, true>},
      {k_factor_quad<4, 50, 13, true, true>, k_factor_quad<4, 50, 13, true, false>, k_factor_quad<4, 50, 13, false, true>}};
  return tab[size][kind];
}
// One launch of k_factor_quad: `nquad` workgroups of four units; returns the route code of the instantiation it took.
static int launch_quad(int nkx, bool isref, bool wave_chol, int nquad, size_t lds, hipStream_t st, const QuadArgs &F, const CovPar &cp) {
  const int size = nkx == 32 ? 0 : nkx == 38 ? 1 : nkx == 44 ? 2 : 3, kind = isref ? (wave_chol ? 0 : 1) : 2;
  hipLaunchKernelGGL(quad_kernel(size, kind), dim3(nquad), dim3(128 * 4), lds, st, F, cp);
  return R_QUAD32_REF_WCH + QUAD_KINDS * size + kind;
}

// w or XB is about to change: the cached statistics die; a reduction still in flight on the second stream finishes first
static void invalidate_stats(st_handle_s *h) {
  if (h->stats_on_stream2) {
    (void)hipSetDevice(h->device);
    (void)hipStreamWaitEvent(h->stream, h->ev_stats, 0);
    h->stats_on_stream2 = false;
  }
  h->stats_valid = false; h->host_stats_valid = false;
}


extern "C" const char *st_last_error(st_handle h) { return h ? h->err.c_str() : g_create_error.c_str(); }
extern "C" void st_set_create_error(const char *msg) { g_create_error = msg ? msg : ""; }   // other translation units of the library

extern "C" int st_destroy(st_handle h) {
  if (!h) return ST_OK;
  (void)hipSetDevice(h->device);
  if (h->ev_top) (void)hipEventDestroy(h->ev_top);
  if (h->ev_main) (void)hipEventDestroy(h->ev_main);
  if (h->ev_stats) (void)hipEventDestroy(h->ev_stats);
  if (h->stream2) (void)hipStreamDestroy(h->stream2);
  prof_harvest(h);
  for (auto e : h->ev_free) (void)hipEventDestroy(e);
  if (h->comm) (void)ncclCommDestroy(h->comm);
  if (h->pin) (void)hipHostFree(h->pin);
  if (h->pin_up) (void)hipHostFree(h->pin_up);
  for (int i = 0; i < 2; ++i) if (h->ev_up[i]) (void)hipEventDestroy(h->ev_up[i]);
  if (h->ev_factor) (void)hipEventDestroy(h->ev_factor);
  points_free(h); rows_free(h); loo_free(h); sim_free(h);   // the feature families' state (st_handle.hpp)
  if (h->stream && !h->ext_stream) (void)hipStreamDestroy(h->stream);
  delete h;   // the device buffers free themselves (DevBuf)
  return ST_OK;
}

// Pure host: which rank owns each block (0-based block id) when `world` processes share one problem; -1 = replicated
// on every rank (the levels above the cut).  No GPU needed: lets the sharding plan be tested on CPU.
extern "C" int st_shard_plan_opt(const st_problem *pb, const st_options *opt_in, int32_t world, int64_t *owner, int32_t *cut_level) {
  st_options opt = {0, 1, 0, world, 0, 0};   // rank / device of `opt_in` are ignored; it is there for a problem that needs options
  // to be read at all (limited_tree: st_options.reserved bit 1)
  if (opt_in) { opt.reference_quirks = opt_in->reference_quirks; opt.force_generic = opt_in->force_generic; opt.reserved = opt_in->reserved; }
  TreeLayout t;
  if (int rc = layout_order(pb, &opt, t, g_create_error)) return rc;
  if (owner) for (size_t i = 0; i < t.blks.size(); ++i) owner[t.blks[i].model_id] = t.blk_owner[i];
  if (cut_level) *cut_level = t.cut;
  return ST_OK;
}
extern "C" int st_shard_plan(const st_problem *pb, int32_t world, int64_t *owner, int32_t *cut_level) {
  return st_shard_plan_opt(pb, nullptr, world, owner, cut_level);
}

// ---- st_create, the device step ("st_create in three steps"): what the layout needs to know of the device,
// then, with the layout built, the handle's streams, buffers and kernel attributes.  A failing HIP call leaves its text in
// g_create_error and returns; st_create destroys the half-built handle, whose buffers free themselves.
#define CCHK(call)                                                                                            \
  do {                                                                                                        \
    hipError_t e_ = (call);                                                                                   \
    if (e_ != hipSuccess) { g_create_error = std::string(#call) + ": " + hipGetErrorString(e_); return ST_ERR_HIP; } \
  } while (0)

static bool query_device(int device, DeviceLimits &dl) {
  hipDeviceProp_t prop;
  if (hipSetDevice(device) != hipSuccess || hipGetDeviceProperties(&prop, device) != hipSuccess) return false;
  dl.sm_count = prop.multiProcessorCount;
  int v = 0;
  if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, device) == hipSuccess && v > 0) dl.lds_limit = (size_t)v;
  hipFuncAttributes fa;
  // a build whose unrolling failed keeps K in scratch memory (localSizeBytes > 0): never use that
  const void *lc[2] = {(const void *)k_factor_lchain<96>, (const void *)k_factor_lchain<136>};
  for (int i = 0; i < 2; ++i)
    if (hipFuncGetAttributes(&fa, lc[i]) == hipSuccess) { dl.lchain_static[i] = fa.sharedSizeBytes; dl.lchain_no_scratch[i] = fa.localSizeBytes == 0; }
  if (hipFuncGetAttributes(&fa, (const void *)quad_kernel(QUAD_SIZES - 1, 2)) == hipSuccess) dl.quad_static = fa.sharedSizeBytes;
  for (int kind = 0; kind < 2; ++kind)
    if (hipFuncGetAttributes(&fa, (const void *)quad_kernel(QUAD_SIZES - 1, kind)) == hipSuccess) dl.quad_static = std::max(dl.quad_static, (size_t)fa.sharedSizeBytes);
  return true;
}

// stream, events, pinned buffers; the row data in device order
static int create_rows(st_handle_s *h, const st_problem *pb) {
  const long long n = h->n_all;
  std::vector<double> cx(n), cy(n), y(n), X((size_t)n * pb->p);
  std::vector<int> mv(n);
  std::vector<unsigned char> obs(n);
  h->n_obs_q.assign(pb->q, 0);
  for (long long i = 0; i < n; ++i) {
    const long long r = h->dev2model[i];
    cx[i] = pb->coords[r]; cy[i] = pb->coords[n + r];
    const long long v = pb->mv_id[r] - 1;   // (in range: layout_levels has checked)
    mv[i] = (int)v;
    const bool ok = std::isfinite(pb->y[r]);
    obs[i] = ok ? 1 : 0;
    y[i] = ok ? pb->y[r] : 0.0;                                  // spamtree_model.cpp:146
    if (ok) { h->n_obs_q[v]++; h->n_obs++; }
    for (int j = 0; j < pb->p; ++j) X[(size_t)j * n + i] = pb->X[(size_t)j * n + r];
  }
  // Q3 partner rows (spamtree_model.cpp:1375): the t-th available row is paired with w[t]
  std::vector<long long> partner(n), rank_av(n, -1);
  long long t = 0;
  for (long long r = 0; r < n; ++r)
    if (std::isfinite(pb->y[r])) rank_av[r] = t++;
  for (long long i = 0; i < n; ++i) {
    const long long r = h->dev2model[i];
    partner[i] = (h->quirks && rank_av[r] >= 0) ? h->model2dev[rank_av[r]] : i;
  }
  // XtX(j) over observed rows of outcome j (:151-155).  p <= 8: this serial host loop stays, because its order of additions
  // fixes the last bits of every existing chain; p > 8: k_stats<q, true> on the device copy of X (create_state)
  h->xtx.assign((size_t)pb->p * pb->p * pb->q, 0.0);
  for (long long r = 0; pb->p <= 8 && r < n; ++r) {
    if (!std::isfinite(pb->y[r])) continue;
    const int v = (int)(pb->mv_id[r] - 1);
    for (int a = 0; a < pb->p; ++a)
      for (int b2 = 0; b2 < pb->p; ++b2)
        h->xtx[(size_t)v * pb->p * pb->p + (size_t)b2 * pb->p + a] += pb->X[(size_t)a * n + r] * pb->X[(size_t)b2 * n + r];
  }
  CCHK(hipStreamCreate(&h->stream));
  CCHK(hipHostMalloc((void **)&h->pin, sizeof(PinnedArea), hipHostMallocDefault));
  new (h->pin) PinnedArea();
  h->pin_up_len = QMAX + std::max(1, h->p * h->q);
  CCHK(hipHostMalloc((void **)&h->pin_up, (size_t)2 * h->pin_up_len * sizeof(double), hipHostMallocDefault));
  for (int i = 0; i < 2; ++i) CCHK(hipEventCreateWithFlags(&h->ev_up[i], hipEventDisableTiming));
  CCHK(hipEventCreateWithFlags(&h->ev_factor, hipEventDisableTiming));
  CCHK(h->d_cx.upload(cx)); CCHK(h->d_cy.upload(cy)); CCHK(h->d_y.upload(y)); CCHK(h->d_X.upload(X));
  CCHK(h->d_mv.upload(mv)); CCHK(h->d_obs.upload(obs)); CCHK(h->d_partner.upload(partner));
  CCHK(h->d_dev2model.upload(h->dev2model));
  return ST_OK;
}

// the layout's lists on the device
static int create_layout_buffers(st_handle_s *h) {
  {
    // device copy: acc_len = where, inside a child's record, the part FOR this block starts (after the block's own
    // ancestors in the full tree; at 0 when every block has a single parent)
    std::vector<Blk> db = h->blks;
    if (h->limited) for (Blk &B : db) B.acc_len = 0;
    CCHK(h->d_blks.upload(db));
    if (h->limited) CCHK(upload_or_dummy(h->d_twin, h->twin_list));
  }
  CCHK(upload_or_dummy(h->d_anc, h->anc_idx)); CCHK(upload_or_dummy(h->d_dch, h->dch_idx));
  CCHK(h->d_lvl.upload(h->lvl_list));
  CCHK(upload_or_dummy(h->d_grps, h->grps)); CCHK(h->d_gdesc.upload(h->gdesc));
  CCHK(upload_or_dummy(h->d_qrec, h->qrec)); std::vector<long long>().swap(h->qrec);   // (qrec_bytes keeps the size)
  CCHK(upload_or_dummy(h->d_wgrps, h->wgrps));
  if (!h->lcslabs.empty()) { CCHK(h->d_lcslabs.upload(h->lcslabs)); CCHK(h->d_lcrow.alloc((size_t)2 * h->n_all)); }
  if (!h->rfvoff.empty()) { CCHK(h->d_rfvoff.upload(h->rfvoff)); CCHK(h->d_vscr.alloc(h->vscr_need + (size_t)2 * RF_BUFD)); }   // (+ what a chunk's DMA reads past the last block)
  CCHK(h->d_s0off.upload(h->s0off));
  CCHK(h->d_s0.alloc(std::max(h->s0_total, (size_t)1)));
  CCHK(upload_or_dummy(h->d_pred, h->pred_list));
  CCHK(h->d_allobs.upload(h->all_obs_list));
  CCHK(upload_or_dummy(h->d_ownobs, h->own_obs_list));
  CCHK(upload_or_dummy(h->d_owngrp, h->own_grp_list)); CCHK(upload_or_dummy(h->d_ownslow, h->own_obs_slow));
  CCHK(h->d_rowmask.upload(h->rowmask)); CCHK(h->d_blkmask.upload(h->blkmask));
  CCHK(h->d_comm.alloc((size_t)2 * h->n_blocks + ST_MAX_RANKS));
  CCHK(h->d_gidx.upload(h->gidx));
  CCHK(h->d_gather.alloc(h->gidx.size()));
  CCHK(h->d_gerr.alloc(ST_MAX_RANKS));
  CCHK(upload_or_dummy(h->d_toplist, h->top_list));
  CCHK(h->d_err2.alloc(2));
  if (h->scratch_stride) CCHK(h->d_scratch.alloc((size_t)h->scratch_wgs * h->scratch_stride));
  if (h->vleaf_total) CCHK(h->d_vleaf.alloc(h->vleaf_total));
  return ST_OK;
}

// the chain's state: w, XB, z, the two panel arenas, the message arena, the statistics
static int create_state(st_handle_s *h) {
  const size_t n = (size_t)h->n_all, nb = (size_t)h->n_blocks;
  CCHK(h->d_w.alloc(n)); CCHK(h->d_xb.alloc(n)); CCHK(h->d_z.alloc(n)); CCHK(h->d_tmp_n.alloc(n + 64));
  CCHK(hipMemset(h->d_w.p, 0, n * sizeof(double)));
  CCHK(hipMemset(h->d_xb.p, 0, n * sizeof(double)));
  CCHK(hipMemset(h->d_z.p, 0, n * sizeof(double)));
  CCHK(h->d_resid.alloc(n));
  CCHK(hipMemset(h->d_resid.p, 0, n * sizeof(double)));
  CCHK(h->d_B.alloc((size_t)h->p * h->q));
  CCHK(h->d_tsq.alloc(QMAX));
  for (int s = 0; s < 2; ++s) {
    // + 128: k_factor_lchain stages chain rows in whole 128-double LDS-DMA pieces and may read up to 127 doubles past a row's
    // end (the other kernels: one double, an odd row's 16-byte piece); the padding is zeroed with the arena
    CCHK(h->d_panels[s].alloc(h->panel_total + 128));
    CCHK(hipMemset(h->d_panels[s].p, 0, (h->panel_total + 128) * sizeof(double)));
    CCHK(h->d_logdet[s].alloc(nb)); CCHK(h->d_loglik[s].alloc(nb));
    CCHK(hipMemset(h->d_logdet[s].p, 0, nb * sizeof(double)));
    CCHK(hipMemset(h->d_loglik[s].p, 0, nb * sizeof(double)));
  }
  CCHK(h->d_acc.alloc(std::max<size_t>(h->acc_total, 1)));
  CCHK(hipMemset(h->d_acc.p, 0, std::max<size_t>(h->acc_total, 1) * sizeof(double)));
  CCHK(h->d_scalars.alloc(8 + 2 * SUM2_WG));
  CCHK(h->d_err.alloc(2));
  CCHK(h->d_partial.alloc((size_t)STATS_WG * (h->p * h->q + h->q)));
  CCHK(h->d_stats.alloc((size_t)h->p * h->q + h->q));
  if (h->p <= 8) return ST_OK;
  // XtX(v)[a, b] is the statistic xty[a, v] with the row weight X[i, b]: one pass of k_stats per weight column b over the
  // observed rows, reduced like every statistic (fixed shape, deterministic).  Entries [a, b] and [b, a] add the same
  // products x_a x_b in the same order: the result is symmetric to the bit.
  const int p = h->p, pq = p * h->q;
  CCHK(h->d_xtx.alloc((size_t)p * pq));
  for (int b2 = 0; b2 < p; ++b2) {
    launch_stats(h, h->stream, h->d_X.p + (size_t)b2 * n);
    hipLaunchKernelGGL(k_stats_final, dim3(pq), dim3(NT), 0, h->stream, h->d_partial.p, STATS_WG, pq + h->q, h->d_xtx.p + (size_t)b2 * pq);
  }
  CCHK(hipGetLastError());
  std::vector<double> t((size_t)p * pq);
  CCHK(hipMemcpyAsync(t.data(), h->d_xtx.p, t.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  CCHK(hipStreamSynchronize(h->stream));
  h->d_xtx.free();
  for (int v = 0; v < h->q; ++v)
    for (int b2 = 0; b2 < p; ++b2)
      for (int a = 0; a < p; ++a) h->xtx[(size_t)v * p * p + (size_t)b2 * p + a] = t[(size_t)b2 * pq + v * p + a];
  return ST_OK;
}

// opt in to > 64 KiB dynamic LDS; the second stream of the ahead-of-time top levels
static int create_attributes(st_handle_s *h, const DeviceLimits &dl) {
  const int lim = (int)h->lds_limit, cu = (int)DeviceLimits::CU_LDS;
  auto dyn = [](const void *f, int bytes) { (void)hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, bytes); };
  for (const void *f : {(const void *)k_factor<false, MODE_FACTOR>, (const void *)k_factor<true, MODE_FACTOR>, (const void *)k_factor<false, MODE_PREDICT>,
                        (const void *)k_factor<true, MODE_PREDICT>, (const void *)k_sample<false>, (const void *)k_sample<true>,
                        (const void *)k_sample<true, true>, (const void *)k_loglik, (const void *)k_factor_mfma, (const void *)k_factor_wide<WG_JT>,
                        (const void *)k_factor_ref_finish, (const void *)k_factor_bigmfma<5, 3, 24>, (const void *)k_factor_bigmfma<3, 5, 34>,
                        (const void *)k_factor_bigmfma<4, 5, 34>, (const void *)k_sample_mfma, (const void *)k_sample_wave,
                        (const void *)k_marginal_invchol, (const void *)k_marginal_invchol_wave})
    dyn(f, lim);
  dyn((const void *)k_factor_lchain<96>, (int)(lc_dyn_doubles(96) * 8));
  dyn((const void *)k_factor_lchain<136>, (int)(lc_dyn_doubles(136) * 8));
  for (int size = QUAD_SIZES - 1; size >= 0; --size)
    for (int kind = 0; kind < QUAD_KINDS; ++kind) dyn((const void *)quad_kernel(size, kind), cu - (int)dl.quad_static);
  // the top levels are a fixed cost (0.19 ms at n = 1e6: a quarter of a rank's phase A on 8 GPUs, 40 % of phase A at
  // n = 1e5); at n = 1e6 on one GPU the sweep fills the chip and the gain is 1.5 % (SPAMTREE_ASYNC_TOP=0 turns it off)
  h->async_top = h->g_top > 0 && h->sw.async_top;
  if (h->async_top) {
    CCHK(hipStreamCreateWithFlags(&h->stream2, hipStreamNonBlocking));
    CCHK(hipEventCreateWithFlags(&h->ev_top, hipEventDisableTiming));
    CCHK(hipEventCreateWithFlags(&h->ev_main, hipEventDisableTiming));
    CCHK(hipEventCreateWithFlags(&h->ev_stats, hipEventDisableTiming));
  }
  (void)hipGetLastError();
  return ST_OK;
}
#undef CCHK

// st_create in three steps: the order of the blocks (layout_order), what the device allows (query_device), the launch
// structures (layout_levels); then the handle's device side
extern "C" int st_create(const st_problem *pb, const st_options *opt, st_handle *out) {
  if (!pb || !out) { g_create_error = "st_create: null argument"; return ST_ERR_USAGE; }
  *out = nullptr;
  st_handle_s *h = new st_handle_s();
  h->device = opt ? opt->device : 0;
  h->quirks = opt ? opt->reference_quirks : 1;
  h->cache_gram = !(opt && (opt->reserved & 1));
  for (int j = 0; j < QMAX; ++j) h->tausq_inv[j] = 1.0;
  std::string msg;
  DeviceLimits dl;
  int rc = layout_order(pb, opt, *h, msg);
  if (rc == ST_OK && !query_device(h->device, dl)) { rc = ST_ERR_HIP; msg = "no usable HIP device (the product path has no CPU fallback)"; }
  if (rc == ST_OK) rc = layout_levels(pb, read_switches(), dl, *h, msg);
  if (rc != ST_OK) return fail_create(h, rc, msg);
  const int n_actual = h->n_actual_groups;
  h->route_a.assign((size_t)n_actual * ST_ROUTE_A_SLOTS, R_NONE);
  h->route_b.assign((size_t)n_actual * 2, R_NONE);
  h->s0_valid.assign((size_t)std::max(n_actual, 1), 0);
  h->prof_level_ms.assign(2 * n_actual, 0.0);
  h->prof_level_n.assign(2 * n_actual, 0);
  if ((rc = create_rows(h, pb)) || (rc = create_layout_buffers(h)) || (rc = create_state(h)) || (rc = create_attributes(h, dl)))
    return fail_create(h, rc, std::string(g_create_error));
  *out = h;
  return ST_OK;
}

// ---- simple state accessors ---------------------------------------------------------------------------------
static int upload_rows(st_handle h, const double *src, double *dst) {
  std::vector<double> tmp(h->n_all);
  for (long long i = 0; i < h->n_all; ++i) tmp[i] = src[h->dev2model[i]];
  HCHK(h, hipMemcpyAsync(dst, tmp.data(), h->n_all * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HCHK(h, hipStreamSynchronize(h->stream));
  return ST_OK;
}
int download_rows(st_handle h, const double *src, double *dst) {
  std::vector<double> tmp(h->n_all);
  HCHK(h, hipMemcpyAsync(tmp.data(), src, h->n_all * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HCHK(h, hipStreamSynchronize(h->stream));
  for (long long i = 0; i < h->n_all; ++i) dst[h->dev2model[i]] = tmp[i];
  return ST_OK;
}

// The call contract of the two split operations (include/spamtree_hip.h, next to st_factor_enqueue and st_sample_w_loglik_begin):
// what would read or replace state that the open half is still producing is refused BEFORE it changes anything on the handle.
// Checked at the C-ABI entry points only: the library's own compositions (st_factor = _enqueue + _finish, ...) call the inner
// steps while neither flag is set.  slot < 0: whatever the slot.
int refuse_factor_open(st_handle h, const char *who, int slot) {
  if (!h->factor_open || (slot >= 0 && slot != h->factor_open_slot)) return ST_OK;
  h->err = std::string(who) + " between st_factor_enqueue and st_factor_finish";
  if (slot >= 0) h->err += " on the slot being factorised";
  return ST_ERR_USAGE;
}
int refuse_sweep_pending(st_handle h, const char *who) {
  if (!h->c_pending) return ST_OK;
  h->err = std::string(who) + " between st_sample_w_loglik_begin and st_sample_w_loglik_end";
  return ST_ERR_USAGE;
}

extern "C" int st_set_w(st_handle h, const double *w) {
  if (!h || !w) return ST_ERR_USAGE;
  if (const int rc = refuse_sweep_pending(h, "st_set_w")) return rc;
  invalidate_stats(h);
  HCHK(h, hipSetDevice(h->device));
  return upload_rows(h, w, h->d_w.p);
}
extern "C" int st_get_w(st_handle h, double *w) {
  if (!h || !w) return ST_ERR_USAGE;
  if (const int rc = refuse_sweep_pending(h, "st_get_w")) return rc;
  HCHK(h, hipSetDevice(h->device));
  return download_rows(h, h->d_w.p, w);
}
// inspection: the reference blocks' whitened residuals as the last factorisation (either slot) left them -- what the leaf
// quads gather as the g of their chains (limited trees: chol(K_uu)^{-1} w_u of the blocks with children); rows of other blocks: 0
extern "C" int st_get_resid(st_handle h, double *out, int64_t n) {
  if (!h || !out || n != h->n_all) return ST_ERR_USAGE;
  HCHK(h, hipSetDevice(h->device));
  if (h->top_pending) HCHK(h, hipStreamWaitEvent(h->stream, h->ev_top, 0));   // (settle_top: the second stream may be writing top rows)
  return download_rows(h, h->d_resid.p, out);
}
extern "C" int st_get_xb(st_handle h, double *xb) {
  if (!h || !xb) return ST_ERR_USAGE;
  HCHK(h, hipSetDevice(h->device));
  return download_rows(h, h->d_xb.p, xb);
}
extern "C" int st_set_beta(st_handle h, const double *Bcoeff) {
  if (!h || !Bcoeff) return ST_ERR_USAGE;
  invalidate_stats(h);
  HCHK(h, hipSetDevice(h->device));
  // through the handle's pinned staging (the caller's buffer is free on return; a slot is rewritten only after its last copy
  // has run): NO host synchronisation -- the C++ driver calls the setters while the proposal's factorisation is still running
  // (st_factor_enqueue / st_factor_finish), so that the new XB is in place the moment phase A ends
  h->pin_up_slot ^= 1;
  HCHK(h, hipEventSynchronize(h->ev_up[h->pin_up_slot]));
  double *stg = h->pin_up + (size_t)h->pin_up_slot * h->pin_up_len + QMAX;
  std::memcpy(stg, Bcoeff, (size_t)h->p * h->q * sizeof(double));
  HCHK(h, hipMemcpyAsync(h->d_B.p, stg, (size_t)h->p * h->q * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HCHK(h, hipEventRecord(h->ev_up[h->pin_up_slot], h->stream));
  {
    ProfScope ps(h, 4);
    const int grid = (int)((h->n_all + NT - 1) / NT);
    hipLaunchKernelGGL(k_xb, dim3(grid), dim3(NT), 0, h->stream, h->d_X.p, h->d_mv.p, h->d_B.p, h->n_all, h->p, h->d_xb.p);
  }
  HCHK(h, hipGetLastError());
  return ST_OK;
}
extern "C" int st_set_tausq_inv(st_handle h, const double *t) {
  if (!h || !t) return ST_ERR_USAGE;
  for (int j = 0; j < h->q; ++j) h->tausq_inv[j] = t[j];
  HCHK(h, hipSetDevice(h->device));
  h->pin_up_slot ^= 1;                                      // (pinned staging, no host synchronisation: st_set_beta)
  HCHK(h, hipEventSynchronize(h->ev_up[h->pin_up_slot]));
  double *stg = h->pin_up + (size_t)h->pin_up_slot * h->pin_up_len;
  std::memcpy(stg, h->tausq_inv, QMAX * sizeof(double));
  HCHK(h, hipMemcpyAsync(h->d_tsq.p, stg, QMAX * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HCHK(h, hipEventRecord(h->ev_up[h->pin_up_slot], h->stream));
  return ST_OK;
}
// readers of a slot's arena while st_factor_begin's launches may still be writing it on the second stream: order the
// main stream behind them (top_pending stays set: the next st_factor still picks the result up)
int settle_top(st_handle h) {
  if (h->top_pending) { HCHK(h, hipSetDevice(h->device)); HCHK(h, hipStreamWaitEvent(h->stream, h->ev_top, 0)); }
  return ST_OK;
}
// What every launch of k_factor_quad is given alike: `nquad` quads of the groups from grp_first, their records (qr_off < 0: none)
// of qr_words words, the arena `phys`.  The sites add their own: the component arrays, wave_chol, mode / vscr / vtiles, predict / z / w_out.
static QuadArgs quad_args(st_handle h, int grp_first, long long qr_off, int qr_words, int nquad, int ldS, int phys, int *errflag) {
  QuadArgs F;
  std::memset(&F, 0, sizeof(F));
  F.blks = h->d_blks.p; F.anc_idx = h->d_anc.p; F.grps = h->d_grps.p + grp_first;
  F.qrec = qr_off >= 0 ? h->d_qrec.p + qr_off : nullptr; F.qrec_stride = qr_words; F.nquad = nquad;
  F.cx = h->d_cx.p; F.cy = h->d_cy.p; F.mv = h->d_mv.p; F.w = h->d_w.p; F.panels = h->d_panels[phys].p;
  F.errflag = errflag; F.ldS = ldS;
  F.g_in = h->d_resid.p;   // leaf bodies (not phase P, not QM_TFROMV): the g of the chain rows, gathered like w
  return F;
}
// A slot whose leaf levels ran QM_VONLY gets its leaf panels here (QM_TFROMV, on the launch stream), before anything reads
// them.  The time counts as phase A: the levels' launch slots (mean per phase-A launch) and the phase bracket, no launch added.
int complete_leaf(st_handle h, int slot) {
  const int phys = h->slot_map[slot];
  if (!h->leaf_pending[phys]) return ST_OK;
  HCHK(h, hipSetDevice(h->device));
  const CovPar &cp = h->leaf_cp[phys];
  ProfScope phase(h, 0, -2, 0);
  for (int g = 0; g < h->n_actual_groups; ++g) {
    const LevelInfo &L = h->levels[g];
    if (L.vl_off < 0) continue;
    QuadArgs F = quad_args(h, L.grp_first, L.qr_off, L.qr_words, L.qown_n, L.q_ldS, phys, h->d_err.p);
    F.wave_chol = L.maxM <= 27 ? 1 : 0;
    F.mode = QM_TFROMV; F.vscr = h->d_vleaf.p + L.vl_off; F.vtiles = quad_vtiles(L.q_nkx);
    ProfScope ps(h, 0, g, 0);
    (void)launch_quad(L.q_nkx, false, true, L.qown_n, L.lds_quad, h->stream, F, cp);   // (the route stays that of the level's launch)
    HCHK(h, hipGetLastError());
  }
  h->leaf_pending[phys] = false;   // (only once every launch is in: after an error the slot still counts as unfinished)
  return ST_OK;
}
extern "C" int st_swap(st_handle h) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = refuse_factor_open(h, "st_swap")) return rc;
  if (const int rc = refuse_sweep_pending(h, "st_swap")) return rc;
  if (h->top_pending) {   // the proposal's top levels are being written into the arena that would become the accepted slot
    h->err = "st_swap between st_factor_begin and the st_factor / st_factor_local that picks its result up";
    return ST_ERR_USAGE;
  }
  { const int rc = complete_leaf(h, 1); if (rc) return rc; }   // the only way a slot becomes the sweep's
  std::swap(h->slot_map[0], h->slot_map[1]);
  std::swap(h->theta[0], h->theta[1]);
  h->gram_valid = false;
  std::fill(h->s0_valid.begin(), h->s0_valid.end(), 0);
  return ST_OK;
}
extern "C" int st_synchronize(st_handle h) {
  if (!h) return ST_ERR_USAGE;
  HCHK(h, hipSetDevice(h->device));
  HCHK(h, hipStreamSynchronize(h->stream));
  return ST_OK;
}
extern "C" void *st_stream(st_handle h) { return h ? (void *)h->stream : nullptr; }
// run every kernel on the caller's stream (e.g. the stream RCCL collectives are enqueued on): no host synchronisation
// is then needed between the library's kernels and the exchanges
extern "C" int st_set_stream(st_handle h, void *stream) {
  if (!h) return ST_ERR_USAGE;
  HCHK(h, hipSetDevice(h->device));
  HCHK(h, hipStreamSynchronize(h->stream));
  prof_harvest(h);
  if (h->stream && !h->ext_stream) (void)hipStreamDestroy(h->stream);
  h->stream = (hipStream_t)stream;
  h->ext_stream = true;
  return ST_OK;
}
extern "C" int st_shard_info(st_handle h, int32_t *rank, int32_t *world, int32_t *cut_level, int64_t *owned_blocks, int64_t *owned_rows) {
  if (!h) return ST_ERR_USAGE;
  if (rank) *rank = h->rank;
  if (world) *world = h->world;
  if (cut_level) *cut_level = h->cut;
  long long ob = 0, orow = 0;
  for (size_t i = 0; i < h->blks.size(); ++i) if (h->blk_owner[i] == h->rank) { ++ob; orow += h->blks[i].m; }
  if (owned_blocks) *owned_blocks = ob;
  if (owned_rows) *owned_rows = orow;
  return ST_OK;
}

// CovarianceParams::transform (covariance_functions.cpp:34-75) + vec_to_symmat (:77-92)
int make_covpar(st_handle h, const double *theta, int ntheta, CovPar *cp) {
  const int q = h->q, ncb = q > 2 ? 3 : 1, npars = 3 * q + ncb, k = q * (q - 1) / 2;
  if (ntheta != npars + k) { h->err = "theta has the wrong length"; return ST_ERR_USAGE; }
  std::memset(cp, 0, sizeof(*cp));
  cp->q = q; cp->ncb = ncb;
  for (int j = 0; j < q; ++j) { cp->ai1[j] = theta[j]; cp->ai2[j] = theta[q + j]; cp->phi[j] = theta[2 * q + j]; }
  for (int j = 0; j < ncb; ++j) cp->tmv[j] = theta[3 * q + j];
  int ix = 0;
  for (int j = 0; j < q; ++j)
    for (int i = j + 1; i < q; ++i) { cp->D[i * q + j] = theta[npars + ix]; cp->D[j * q + i] = theta[npars + ix]; ++ix; }
  finish_covpar(cp);
  return ST_OK;
}

template <bool BIG, int MODE>
static void launch_factor(st_handle h, const LevelInfo &L, FactorArgs &A, const CovPar &cp, hipStream_t st = nullptr) {
  int grid = A.nlist;
  if (BIG) {
    grid = std::min(grid, h->scratch_wgs);
    A.scratch = h->d_scratch.p; A.scratch_stride = h->scratch_stride;
  }
  hipLaunchKernelGGL((k_factor<BIG, MODE>), dim3(grid), dim3(NT), L.lds_factor, st ? st : h->stream, A, cp);
}

// ---- the read-back protocol (st_protocol.hpp): every result of the iteration comes back as a Landing --------------------------
static bool uses_exchange(st_handle h) { return h->world > 1 || h->comm; }   // an attached communicator selects the exchange protocol even with one rank (tests)
// ... without a communicator: the refusal; `alternatives`: the entry points that leave the exchanges to the caller
static int refuse_without_comm(st_handle h, const char *alternatives) {
  h->err = std::string("world > 1: call st_comm_init first, or use ") + alternatives;
  return ST_ERR_USAGE;
}
// The sums of a and b (n entries each) on the launch stream, and their copy into dst.
static int enqueue_result(st_handle h, const double *a, const double *b, int n, Landing *dst) {
  {
    ProfScope ps(h, 3);
    launch_sum2(h->stream, a, b, n, h->d_scalars.p + 8, h->d_scalars.p);
  }
  HCHK(h, hipGetLastError());
  HCHK(h, hipMemcpyAsync(dst->sums, h->d_scalars.p, 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  return ST_OK;
}
// ... of a slot's component arrays
static int enqueue_slot_result(st_handle h, int slot, Landing *dst) {
  const int phys = h->slot_map[slot];
  return enqueue_result(h, h->d_logdet[phys].p, h->d_loglik[phys].p, (int)h->n_blocks, dst);
}
// ... of the exchanged components (st_mg_pack_comps + all-reduce), with the ranks' failure words behind them
static int enqueue_comm_result(st_handle h, Landing *dst, double *rank_words) {
  const int nb = (int)h->n_blocks;
  if (const int rc = enqueue_result(h, h->d_comm.p, h->d_comm.p + nb, nb, dst)) return rc;
  HCHK(h, hipMemcpyAsync(rank_words, h->d_comm.p + 2 * (size_t)nb, h->world * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  return ST_OK;
}
// The failure word's copy into dst.  On its own because a sweep's word has to leave EARLIER in stream order than the sums: phase C
// (st_loglik_local) resets it.
static int enqueue_fail_word(st_handle h, Landing *dst) {
  HCHK(h, hipMemcpyAsync(dst->err, h->d_err.p, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  return ST_OK;
}
static int reset_err(st_handle h) {
  const int init[2] = {INT_MAX, 0};
  HCHK(h, hipMemcpyAsync(h->d_err.p, init, 2 * sizeof(int), hipMemcpyHostToDevice, h->stream));
  return ST_OK;
}

// sum-with-zeros exchange buffers: every entry is contributed by exactly one rank (replicated blocks by rank 0), so
// an all-reduce(sum) reproduces the single-GPU arrays bit for bit, for any number of ranks and any reduction order
// all-gather form of the exchange of w: a rank's slice of the gather buffer = its owned rows + its failure word

// levels [g_lo, g_hi); `st` / `errflag`: the launch stream and failure word (st_factor_begin: the second stream, d_err2)
// vonly: the deferrable leaf levels take QM_VONLY (*deferred = true when one did)
static int factor_launch(st_handle h, int phys, const CovPar &cp, int g_lo = 0, int g_hi = INT_MAX, hipStream_t st = nullptr, int *errflag = nullptr,
                         bool vonly = false, bool *deferred = nullptr) {
  g_hi = std::min(g_hi, h->n_actual_groups);
  if (!st) st = h->stream;
  if (!errflag) errflag = h->d_err.p;
  int n_launch = 0;
  for (int g = g_lo; g < g_hi; ++g) n_launch += ((h->levels[g].fast ? h->levels[g].gown_n : h->levels[g].own_n) != 0);
  ProfScope phase(h, 0, -2, n_launch, st);   // profile mode 2: the phase's launches between ONE pair of events (mean launch = total / launches)
  for (int g = g_lo; g < g_hi; ++g) std::fill_n(h->route_a.begin() + (size_t)g * ST_ROUTE_A_SLOTS, ST_ROUTE_A_SLOTS, (int)R_NONE);
  auto route = [&](int g, int code) {   // the next free phase-A slot of level g
    int *r = h->route_a.data() + (size_t)g * ST_ROUTE_A_SLOTS;
    for (int i = 0; i < ST_ROUTE_A_SLOTS; ++i) if (r[i] == R_NONE) { r[i] = code; return; }
  };
  if (g_lo == 0 && h->limited && !h->twin_list.empty()) {
    MarginalArgs M;
    M.blks = h->d_blks.p; M.list = h->d_twin.p; M.nlist = (int)h->twin_list.size(); M.cx = h->d_cx.p; M.cy = h->d_cy.p; M.mv = h->d_mv.p;
    M.panels = h->d_panels[phys].p; M.errflag = errflag; M.maxM = h->twin_maxM;
    M.w = h->d_w.p; M.resid = h->d_resid.p;   // the g of the marginal chains (the conditional residuals below are not stored)
    const size_t lds = (size_t)2 * h->twin_maxM * h->twin_maxM * sizeof(double);
    if (h->twin_maxM <= 27 && !h->force_generic) {   // one block per wave, blocked DPP / MFMA elimination
      route(0, R_MARGINAL_INVCHOL_WAVE);
      hipLaunchKernelGGL(k_marginal_invchol_wave, dim3(std::min((M.nlist + NT / 64 - 1) / (NT / 64), 8 * h->sm_count)), dim3(NT),
                         (size_t)(NT / 64) * 64 * CH_LD * sizeof(double), st, M, cp);
    } else {
      route(0, R_MARGINAL_INVCHOL);
      hipLaunchKernelGGL(k_marginal_invchol, dim3(std::min(M.nlist, 8 * h->sm_count)), dim3(NT), lds, st, M, cp);
    }
  }
  // the reference blocks' residuals, for the leaf quads below them (limited trees: their chains are marginal factors, see above)
  double *resid = h->limited ? nullptr : h->d_resid.p;
  for (int g = g_lo; g < g_hi; ++g) {
    const LevelInfo &L = h->levels[g];
    if ((L.fast ? L.gown_n : L.own_n) == 0) continue;
    FactorArgs A;
    std::memset(&A, 0, sizeof(A));
    A.blks = h->d_blks.p; A.anc_idx = h->d_anc.p; A.list = h->d_lvl.p + L.first + L.own_lo; A.nlist = L.own_n;
    A.cx = h->d_cx.p; A.cy = h->d_cy.p; A.mv = h->d_mv.p; A.w_in = h->d_w.p; A.w_out = nullptr; A.z = nullptr;
    A.panels = h->d_panels[phys].p; A.logdet_c = h->d_logdet[phys].p; A.loglik_c = h->d_loglik[phys].p;
    A.resid = resid;
    A.errflag = errflag; A.maxP = L.maxP; A.maxM = L.maxM; A.maxMa = L.maxMa; A.SR = L.big_factor ? 4 : 8;
    {
      ProfScope ps(h, 0, g, 1, st);
      if (L.fast && h->sw.factor_gen == 3 && L.q_nkx > 0) {
        QuadArgs F = quad_args(h, L.grp_first, L.qr_off, L.qr_words, L.qown_n, L.q_ldS, phys, errflag);
        F.logdet_c = h->d_logdet[phys].p; F.loglik_c = h->d_loglik[phys].p; F.resid = resid;
        F.wave_chol = L.maxM <= 27 ? 1 : 0;
        if (!L.isref && vonly && L.vl_off >= 0) { F.mode = QM_VONLY; F.vscr = h->d_vleaf.p + L.vl_off; F.vtiles = quad_vtiles(L.q_nkx); *deferred = true; }
        route(g, launch_quad(L.q_nkx, L.isref != 0, F.wave_chol != 0, L.qown_n, L.lds_quad, st, F, cp));
      } else if (L.fast) {
        FastArgs F;
        std::memset(&F, 0, sizeof(F));
        F.blks = h->d_blks.p; F.anc_idx = h->d_anc.p; F.grps = h->d_grps.p + L.grp_first + L.gown_lo; F.ngrp = L.gown_n;
        F.cx = h->d_cx.p; F.cy = h->d_cy.p; F.mv = h->d_mv.p; F.w = h->d_w.p; F.panels = h->d_panels[phys].p;
        F.logdet_c = h->d_logdet[phys].p; F.loglik_c = h->d_loglik[phys].p; F.resid = resid; F.errflag = errflag;
        F.Pm4 = L.Pm4; F.ldKV = L.ldKV; F.ldS = L.ldS; F.SRm = L.SRm; F.stage_dbl = L.stage_dbl;
        F.gdesc = h->d_gdesc.p + (size_t)(L.grp_first + L.gown_lo) * h->gd_stride; F.gd_stride = h->gd_stride;
        route(g, R_FACTOR_MFMA);
        hipLaunchKernelGGL(k_factor_mfma, dim3(L.gown_n), dim3(NT), L.lds_fast, st, F, cp);
      } else if (L.bigmfma && h->sw.factor_gen == 3 && L.lchain) {
        LcArgs C;
        std::memset(&C, 0, sizeof(C));
        C.blks = h->d_blks.p; C.anc_idx = h->d_anc.p; C.slabs = h->d_lcslabs.p + L.lc_first; C.nslab = L.lc_count;
        C.cx = h->d_cx.p; C.cy = h->d_cy.p; C.mv = h->d_mv.p; C.w_in = h->d_w.p; C.panels = h->d_panels[phys].p;
        C.rowtmp = h->d_lcrow.p; C.n_rows = h->n_all; C.errflag = errflag;
        C.errcode = L.lchain_ref ? 2 : 3;
        C.vscr = L.lchain_ref ? h->d_vscr.p : nullptr;
        if (L.lchain == 96) { route(g, R_LCHAIN96); hipLaunchKernelGGL((k_factor_lchain<96>), dim3(L.lc_count), dim3(LC_NT), lc_dyn_doubles(96) * 8, st, C, cp); }
        else { route(g, R_LCHAIN136); hipLaunchKernelGGL((k_factor_lchain<136>), dim3(L.lc_count), dim3(LC_NT), lc_dyn_doubles(136) * 8, st, C, cp); }
        if (L.lchain_ref) {   // the panels hold [ -r_j T_j | r_j ] per column: finish the blocks (Schur complement, factorisation, -Ri T in place)
          A.vscr = h->d_vscr.p; A.voff = h->d_rfvoff.p + L.rf_first; A.hvrow = h->d_lcrow.p;
          route(g, R_REF_FINISH);
          hipLaunchKernelGGL(k_factor_ref_finish, dim3(std::min(A.nlist, 2 * h->sm_count)), dim3(BM_NT), L.lds_ref_finish, st, A, cp);
        } else {
          route(g, R_LCHAIN_SCALARS);
          hipLaunchKernelGGL(k_lchain_scalars, dim3((A.nlist + 255) / 256), dim3(256), 0, st, h->d_blks.p, A.list, A.nlist, h->d_lcrow.p, h->n_all,
                             h->d_logdet[phys].p, h->d_loglik[phys].p);
        }
      } else if (L.bigmfma && h->sw.factor_gen == 3 && L.wide_count > 0) {
        WideArgs W;
        std::memset(&W, 0, sizeof(W));
        W.blks = h->d_blks.p; W.anc_idx = h->d_anc.p; W.list = h->d_lvl.p + L.first + L.own_lo; W.groups = h->d_wgrps.p + L.wide_first;
        W.ngroups = L.wide_count; W.cx = h->d_cx.p; W.cy = h->d_cy.p; W.mv = h->d_mv.p; W.w_in = h->d_w.p; W.panels = h->d_panels[phys].p;
        W.logdet_c = h->d_logdet[phys].p; W.loglik_c = h->d_loglik[phys].p; W.resid = resid; W.errflag = errflag; W.scratch = h->d_scratch.p;
        W.scratch_stride = h->scratch_stride; W.maxP = L.maxP; W.maxN = L.wide_maxN; W.maxM = L.maxM; W.maxMa = L.maxMa; W.ldS = L.bm_ldS;
        route(g, R_FACTOR_WIDE);
        hipLaunchKernelGGL((k_factor_wide<WG_JT>), dim3(std::min(L.wide_count, h->sm_count)), dim3(WG_NT), L.lds_wide, st, W, cp);
      } else if (L.bigmfma && h->sw.factor_gen == 3) {
        A.scratch = h->d_scratch.p; A.scratch_stride = h->scratch_stride; A.SR = L.bm_ldS;
        if (L.maxM <= 48) { route(g, R_BIGMFMA3); hipLaunchKernelGGL((k_factor_bigmfma<3, 5, 34>), dim3(std::min(A.nlist, h->sm_count)), dim3(BM_NT), L.lds_bigmfma, st, A, cp); }
        else if (L.maxM <= 64) { route(g, R_BIGMFMA4); hipLaunchKernelGGL((k_factor_bigmfma<4, 5, 34>), dim3(std::min(A.nlist, h->sm_count)), dim3(BM_NT), L.lds_bigmfma, st, A, cp); }
        else { route(g, R_BIGMFMA5); hipLaunchKernelGGL((k_factor_bigmfma<5, 3, 24>), dim3(std::min(A.nlist, h->sm_count)), dim3(BM_NT), L.lds_bigmfma, st, A, cp); }
      } else if (L.big_factor) { route(g, R_FACTOR_SCRATCH); launch_factor<true, MODE_FACTOR>(h, L, A, cp, st); }
      else { route(g, R_FACTOR_LDS); launch_factor<false, MODE_FACTOR>(h, L, A, cp, st); }
    }
    HCHK(h, hipGetLastError());
  }
  return ST_OK;
}


// Phase A of the top levels ahead of time, on the second stream: call before the sweep with the theta st_factor /
// st_factor_local will be given next for the same slot.  A no-op when the tree does not qualify (or SPAMTREE_ASYNC_TOP=0).
extern "C" int st_factor_ahead_levels(st_handle h) { return (h && h->async_top && !h->async_top_off) ? h->g_top : 0; }
// measurement: switch the ahead-of-time path off / on at run time (bench.py's per-level pass runs every level of phase A back
// to back on ONE stream; on the second stream, under the sweep, the top levels' launch times are not their own)
extern "C" int st_factor_ahead_enable(st_handle h, int enable) {
  if (!h) return ST_ERR_USAGE;
  h->async_top_off = !enable;
  return ST_OK;
}
extern "C" int st_factor_begin(st_handle h, int slot, const double *theta, int ntheta) {
  if (!h || !theta || slot < 0 || slot > 1) return ST_ERR_USAGE;
  if (const int rc = refuse_factor_open(h, "st_factor_begin")) return rc;
  if (!h->async_top || h->async_top_off) return ST_OK;
  HCHK(h, hipSetDevice(h->device));
  CovPar cp;
  int rc = make_covpar(h, theta, ntheta, &cp);
  if (rc) return rc;
  if (h->top_pending) HCHK(h, hipStreamWaitEvent(h->stream2, h->ev_top, 0));
  HCHK(h, hipEventRecord(h->ev_main, h->stream));          // everything issued so far (the previous iteration) comes first
  HCHK(h, hipStreamWaitEvent(h->stream2, h->ev_main, 0));
  const int init[2] = {INT_MAX, 0};
  HCHK(h, hipMemcpyAsync(h->d_err2.p, init, 2 * sizeof(int), hipMemcpyHostToDevice, h->stream2));
  const int phys = h->slot_map[slot];
  h->leaf_pending[phys] = false;   // the slot is being re-factorised: its deferred half is void
  h->prof_suspend = true;   // not timed: the launches overlap the sweep on another stream
  rc = factor_launch(h, phys, cp, 0, h->g_top, h->stream2, h->d_err2.p);
  h->prof_suspend = false;
  if (rc) return rc;
  HCHK(h, hipEventRecord(h->ev_top, h->stream2));
  h->top_pending = true; h->top_phys = phys; h->top_theta.assign(theta, theta + ntheta);
  return ST_OK;
}
static int fix_top_comps(st_handle h, int phys);
static int run_stats(st_handle h, hipStream_t st);
// The beta / tausq statistics of the iteration need the sweep's w and the current XB only: when a proposal is about to be
// factorised they start on the second stream and run under phase A (the driver asks for them after the Metropolis step).
static int stats_begin(st_handle h) {
  if (!h->stream2 || h->stats_valid) return ST_OK;
  HCHK(h, hipEventRecord(h->ev_main, h->stream));           // w of the sweep is final at this point of the main stream
  HCHK(h, hipStreamWaitEvent(h->stream2, h->ev_main, 0));
  int rc = run_stats(h, h->stream2);
  if (rc) return rc;
  // the results travel to pinned host memory on the same stream: when the driver asks (after the Metropolis step) they are
  // there, and fetching them costs an event query instead of a copy + a synchronisation of the main stream
  const size_t nq = (size_t)h->p * h->q + h->q;
  h->stats_prefetched = nq <= (size_t)ST_PIN_STATS;
  if (h->stats_prefetched) HCHK(h, hipMemcpyAsync(h->pin->stats, h->d_stats.p, nq * sizeof(double), hipMemcpyDeviceToHost, h->stream2));
  HCHK(h, hipEventRecord(h->ev_stats, h->stream2));
  h->stats_on_stream2 = true;
  return ST_OK;
}

static int factor_local(st_handle h, int slot, const double *theta, int ntheta, bool vonly);
extern "C" int st_factor_local(st_handle h, int slot, const double *theta, int ntheta) {
  if (h) { if (const int rc = refuse_factor_open(h, "st_factor_local")) return rc; }
  return factor_local(h, slot, theta, ntheta, false);
}
static int factor_local(st_handle h, int slot, const double *theta, int ntheta, bool vonly) {
  if (!h || !theta || slot < 0 || slot > 1) return ST_ERR_USAGE;
  HCHK(h, hipSetDevice(h->device));
  CovPar cp;
  int rc = make_covpar(h, theta, ntheta, &cp);
  if (rc) return rc;
  h->theta[slot].assign(theta, theta + ntheta);
  if (slot == 0) { h->gram_valid = false; std::fill(h->s0_valid.begin(), h->s0_valid.end(), 0); }
  rc = reset_err(h);
  if (rc) return rc;
  const int phys = h->slot_map[slot];
  h->leaf_pending[phys] = false;
  if (slot == 1) { rc = stats_begin(h); if (rc) return rc; }
  bool reuse = false;
  if (h->top_pending) {
    HCHK(h, hipStreamWaitEvent(h->stream, h->ev_top, 0));   // the top levels are done (or at least out of the way) before anything below
    reuse = h->top_phys == phys && (int)h->top_theta.size() == ntheta && std::equal(theta, theta + ntheta, h->top_theta.begin());
    h->top_pending = false;
  }
  // the top levels ran ahead of time with the w of the sweep's start: their quadratic forms AND the residuals the leaf quads
  // below gather are redone with the current w before those levels are launched (outside factor_launch's phase bracket)
  if (reuse) { rc = fix_top_comps(h, phys); if (rc) return rc; }
  bool deferred = false;
  rc = factor_launch(h, phys, cp, reuse ? h->g_top : 0, INT_MAX, nullptr, nullptr, vonly, &deferred);
  if (deferred) { h->leaf_pending[phys] = true; h->leaf_cp[phys] = cp; }
  if (rc || !reuse) return rc;
  hipLaunchKernelGGL(k_merge_err, dim3(1), dim3(64), 0, h->stream, h->d_err.p, h->d_err2.p);
  HCHK(h, hipGetLastError());
  return ST_OK;
}

extern "C" int st_mg_pack_comps(st_handle h, int slot, void **dev_ptr, int64_t *len) {
  if (!h || slot < 0 || slot > 1) return ST_ERR_USAGE;
  HCHK(h, hipSetDevice(h->device));
  { const int rc0 = settle_top(h); if (rc0) return rc0; }
  const int phys = h->slot_map[slot], nb = (int)h->n_blocks;
  {
    ProfScope ps(h, 3);
    hipLaunchKernelGGL(k_pack_comps, dim3((std::max(nb, h->world) + NT - 1) / NT), dim3(NT), 0, h->stream, h->d_logdet[phys].p,
                       h->d_loglik[phys].p, h->d_blkmask.p, nb, h->d_err.p, h->rank, h->world, h->d_comm.p);
  }
  HCHK(h, hipGetLastError());
  if (dev_ptr) *dev_ptr = h->d_comm.p;
  if (len) *len = 2 * (int64_t)nb + h->world;
  return ST_OK;
}

// after the exchange of the packed components: deterministic sum + failure code agreed by all ranks
extern "C" int st_mg_finish(st_handle h, double *loglik) {
  if (!h) return ST_ERR_USAGE;
  HCHK(h, hipSetDevice(h->device));
  Landing res;
  double errc[ST_MAX_RANKS];
  if (const int rc = enqueue_comm_result(h, &res, errc)) return rc;
  HCHK(h, hipStreamSynchronize(h->stream));
  if (const int code = rank_failure(errc, h->world)) return code;
  return landing_code(res, loglik);
}

#define NCHK(h, call)                                                                                        \
  do {                                                                                                        \
    ncclResult_t r_ = (call);                                                                                 \
    if (r_ != ncclSuccess) { (h)->err = std::string(#call) + ": " + ncclGetErrorString(r_); return ST_ERR_HIP; } \
  } while (0)

// pack -> RCCL all-reduce(sum) on the launch stream -> deterministic finish (native path of the multi-GPU protocol)
static int exchange_comps_and_finish(st_handle h, int slot, double *loglik) {
  void *ptr = nullptr;
  int64_t len = 0;
  int rc = st_mg_pack_comps(h, slot, &ptr, &len);
  if (rc) return rc;
  {
    ProfScope ps(h, 7);
    NCHK(h, ncclAllReduce(ptr, ptr, (size_t)len, ncclDouble, ncclSum, h->comm, h->stream));
  }
  return st_mg_finish(h, loglik);
}

extern "C" int st_comm_unique_id(void *out, int32_t cap) {
  if (!out || cap < (int32_t)sizeof(ncclUniqueId)) return ST_ERR_USAGE;
  ncclUniqueId id;
  if (ncclGetUniqueId(&id) != ncclSuccess) return ST_ERR_HIP;
  std::memcpy(out, &id, sizeof(id));
  return (int)sizeof(id);
}
extern "C" int st_comm_init(st_handle h, const void *unique_id) {
  if (!h || !unique_id) return ST_ERR_USAGE;
  HCHK(h, hipSetDevice(h->device));
  ncclUniqueId id;
  std::memcpy(&id, unique_id, sizeof(id));
  NCHK(h, ncclCommInitRank(&h->comm, h->world, id, h->rank));
  return ST_OK;
}

static int factor_enqueue(st_handle h, int slot, const double *theta, int ntheta, bool vonly);
extern "C" int st_factor(st_handle h, int slot, const double *theta, int ntheta, double *loglik) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = refuse_factor_open(h, "st_factor")) return rc;
  if (uses_exchange(h)) {
    if (!h->comm) return refuse_without_comm(h, "st_factor_local / st_mg_pack_comps / (all-reduce) / st_mg_finish");
    int rc = st_factor_local(h, slot, theta, ntheta);
    if (rc) return rc;
    return exchange_comps_and_finish(h, slot, loglik);
  }
  int rc = factor_enqueue(h, slot, theta, ntheta, false);
  if (rc) return rc;
  return st_factor_finish(h, loglik);
}
// st_factor in two halves (one GPU): everything is ENQUEUED by the first -- the levels, the two sums, the copies of the sums and of
// the failure word to pinned memory, an event behind them -- and the second waits for that event and reads them.  In between the
// host may enqueue work that does not touch the proposal's slot: the C++ driver draws tausq and beta from the sweep's statistics
// (ready early in phase A: they run on the second stream) and uploads them, so that XB is current when phase A ends instead of
// two host round trips later.  With a communicator attached the first half enqueues nothing and the second does all of st_factor.
extern "C" int st_factor_is_async(st_handle h) { return (h && !uses_exchange(h)) ? 1 : 0; }
// the proposal's slot (1) defers its leaf levels' T (unless st_options.reserved bit 2); synchronous st_factor never does
extern "C" int st_factor_enqueue(st_handle h, int slot, const double *theta, int ntheta) {
  return factor_enqueue(h, slot, theta, ntheta, h && h->defer_leaf && slot == 1);
}
static int factor_enqueue(st_handle h, int slot, const double *theta, int ntheta, bool vonly) {
  if (!h || !theta || slot < 0 || slot > 1) return ST_ERR_USAGE;
  if (h->factor_open) { h->err = "st_factor_enqueue: the previous one has not been finished"; return ST_ERR_USAGE; }
  if (uses_exchange(h)) {
    h->factor_open = true; h->factor_open_slot = slot; h->top_theta_open.assign(theta, theta + ntheta);
    return ST_OK;
  }
  int rc = factor_local(h, slot, theta, ntheta, vonly);
  if (rc) return rc;
  // the failure word and the two sums come back in ONE synchronisation (the sums are meaningless after a failure)
  if ((rc = enqueue_slot_result(h, slot, &h->pin->factor)) || (rc = enqueue_fail_word(h, &h->pin->factor))) return rc;
  HCHK(h, hipEventRecord(h->ev_factor, h->stream));
  h->factor_open = true; h->factor_open_slot = slot; h->top_theta_open.clear();
  return ST_OK;
}
extern "C" int st_factor_finish(st_handle h, double *loglik) {
  if (!h) return ST_ERR_USAGE;
  if (!h->factor_open) { h->err = "st_factor_finish without st_factor_enqueue"; return ST_ERR_USAGE; }
  h->factor_open = false;
  if (uses_exchange(h)) {
    if (!h->comm) return refuse_without_comm(h, "st_factor_local / st_mg_pack_comps / (all-reduce) / st_mg_finish");
    int rc = st_factor_local(h, h->factor_open_slot, h->top_theta_open.data(), (int)h->top_theta_open.size());
    if (rc) return rc;
    return exchange_comps_and_finish(h, h->factor_open_slot, loglik);
  }
  HCHK(h, hipSetDevice(h->device));
  HCHK(h, hipEventSynchronize(h->ev_factor));
  return landing_code(h->pin->factor, loglik);   // a code: the reference's `return false` (:971-982)
}

// The sweep and the log-density of its w (one GPU), ENQUEUED with their read-back into dst: the sweep's failure word travels with
// the sums, so that ONE synchronisation brings both.  10 / 11: the reference stops with "Error at gibbs_sample_w" (:1215-1217).
static int enqueue_sweep_loglik(st_handle h, const double *z, uint64_t seed, uint32_t iter, int slot, Landing *dst) {
  int rc = st_sample_w_local(h, z, seed, iter);
  if (rc) return rc;
  rc = st_sample_w_top(h);
  if (rc) return rc;
  rc = enqueue_fail_word(h, dst);
  if (rc) return rc;
  rc = st_loglik_local(h, slot);   // resets the failure word after the copy above (stream order)
  if (rc) return rc;
  return enqueue_slot_result(h, slot, dst);
}

// The sweep's exchange (communicator attached) up to the gather-pack: this rank's subtrees, all-reduce of the cut level's message
// records, the replicated top levels, then the rank's own rows of w and its failure word packed for the all-gather.
static int gather_w_scatter(st_handle h);
static int sweep_exchange(st_handle h, const double *z, uint64_t seed, uint32_t iter, void **send, void **recv, int64_t *count) {
  int rc = st_sample_w_local(h, z, seed, iter);
  if (rc) return rc;
  if (h->top_len > 0) {
    ProfScope ps(h, 7);
    NCHK(h, ncclAllReduce(h->d_acc.p + h->top_off, h->d_acc.p + h->top_off, (size_t)h->top_len, ncclDouble, ncclSum, h->comm, h->stream));
  }
  rc = st_sample_w_top(h);
  if (rc) return rc;
  return st_mg_gather_w_pack(h, send, recv, count);
}

// st_sample_w followed by st_loglik_w(slot) with ONE synchronisation.
extern "C" int st_sample_w_loglik(st_handle h, const double *z, uint64_t seed, uint32_t iter, int slot, double *loglik) {
  if (!h || slot < 0 || slot > 1) return ST_ERR_USAGE;
  if (const int rc = refuse_factor_open(h, "st_sample_w_loglik")) return rc;
  if (const int rc = refuse_sweep_pending(h, "st_sample_w_loglik")) return rc;
  { const int rc0 = complete_leaf(h, slot); if (rc0) return rc0; }
  if (!uses_exchange(h)) {
    const int rc = enqueue_sweep_loglik(h, z, seed, iter, slot, &h->pin->sweep);
    if (rc) return rc;
    HCHK(h, hipStreamSynchronize(h->stream));
    return landing_code(h->pin->sweep, loglik);
  }
  if (!h->comm) {
    int rc = st_sample_w(h, z, seed, iter);   // reports the missing communicator
    if (rc) return rc;
    return st_loglik_w(h, slot, loglik);
  }
  // Fused exchange: the log-density of a rank's own blocks needs w of its own subtrees and of the replicated top only,
  // both current BEFORE the other ranks' rows arrive -- so phase C runs ahead of the exchange of w, and w and the
  // log-density components travel in ONE grouped RCCL call, followed by ONE host synchronisation.
  void *pw = nullptr, *pr = nullptr, *pc = nullptr;
  int64_t lw = 0, lc = 0;
  int rc = sweep_exchange(h, z, seed, iter, &pw, &pr, &lw);   // own rows of w + this rank's failure word of the sweep
  if (rc) return rc;
  rc = st_loglik_local(h, slot);          // resets the failure word after the pack above (stream order)
  if (rc) return rc;
  rc = st_mg_pack_comps(h, slot, &pc, &lc);
  if (rc) return rc;
  {
    ProfScope ps(h, 7);
    NCHK(h, ncclGroupStart());
    NCHK(h, ncclAllGather(pw, pr, (size_t)lw, ncclDouble, h->comm, h->stream));
    NCHK(h, ncclAllReduce(pc, pc, (size_t)lc, ncclDouble, ncclSum, h->comm, h->stream));
    NCHK(h, ncclGroupEnd());
  }
  rc = gather_w_scatter(h);
  if (rc) return rc;
  invalidate_stats(h);
  Landing res;
  double errw[ST_MAX_RANKS], errc[ST_MAX_RANKS];
  rc = enqueue_comm_result(h, &res, errc);
  if (rc) return rc;
  HCHK(h, hipMemcpyAsync(errw, h->d_gerr.p, h->world * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HCHK(h, hipStreamSynchronize(h->stream));
  if (const int code = rank_failure(errw, h->world)) return code;   // the sweep's words first, then the components'
  if (const int code = rank_failure(errc, h->world)) return code;
  return landing_code(res, loglik);
}

// The same pair WITHOUT the host synchronisation: the log-density of the sweep's w is not needed on the host before the
// Metropolis step, i.e. after the proposal's factorisation -- whose own synchronisation then brings it along.  One round trip
// and one idle gap of the GPU less per iteration (the driver enqueues phase A right behind phase C).  _end returns what the
// synchronous call would have returned (failure code of the sweep / the log-density); it synchronises only if nobody has yet.
// With a communicator attached (multi-GPU) _begin simply runs the synchronous protocol and _end hands its result over.
extern "C" int st_sample_w_loglik_begin(st_handle h, const double *z, uint64_t seed, uint32_t iter, int slot) {
  if (!h || slot < 0 || slot > 1) return ST_ERR_USAGE;
  if (const int rc = refuse_factor_open(h, "st_sample_w_loglik_begin")) return rc;
  if (const int rc = refuse_sweep_pending(h, "st_sample_w_loglik_begin")) return rc;
  { const int rc0 = complete_leaf(h, slot); if (rc0) return rc0; }
  if (uses_exchange(h)) {
    h->c_ll = 0.0;
    h->c_rc = st_sample_w_loglik(h, z, seed, iter, slot, &h->c_ll);
    if (h->c_rc < 0) return h->c_rc;   // a HIP / RCCL / usage error: nothing is pending, the caller must not call _end
    h->c_pending = true;
    return ST_OK;
  }
  const int rc = enqueue_sweep_loglik(h, z, seed, iter, slot, &h->pin->deferred);
  if (rc) return rc;
  h->c_rc = INT_MIN;   // not known yet
  h->c_pending = true;
  return ST_OK;
}
extern "C" int st_sample_w_loglik_end(st_handle h, double *loglik) {
  if (!h) return ST_ERR_USAGE;
  if (!h->c_pending) { h->err = "st_sample_w_loglik_end without st_sample_w_loglik_begin"; return ST_ERR_USAGE; }
  h->c_pending = false;
  if (h->c_rc != INT_MIN) {   // the synchronous protocol ran in _begin
    if (h->c_rc == ST_OK && loglik) *loglik = h->c_ll;
    return h->c_rc;
  }
  HCHK(h, hipStreamSynchronize(h->stream));   // returns at once when a later call (st_factor) has synchronised already
  return landing_code(h->pin->deferred, loglik);
}

int gen_or_upload_z(st_handle h, const double *z, uint64_t seed, uint32_t iter, unsigned stream_id, double *dst) {
  if (z) return upload_rows(h, z, dst);
  {
    ProfScope ps(h, 5);
    const int grid = (int)((h->n_all + NT - 1) / NT);
    hipLaunchKernelGGL(k_normals, dim3(grid), dim3(NT), 0, h->stream, dst, h->d_dev2model.p, h->n_all, iter, stream_id,
                       (unsigned long long)seed);
  }
  HCHK(h, hipGetLastError());
  return ST_OK;
}

static int sample_launch(st_handle h, int g_hi, int g_lo) {   // levels g_hi-1 ... g_lo
  const int phys = h->slot_map[0];
  for (int g = g_hi - 1; g >= g_lo; --g) {
    const LevelInfo &L = h->levels[g];
    int *route = h->route_b.data() + 2 * (size_t)g;   // [0]: the Gram kernel, [1]: the sweep kernel
    route[0] = route[1] = R_NONE;
    if ((L.fast ? L.gown_n : L.own_n) == 0) continue;
    SampleArgs A;
    std::memset(&A, 0, sizeof(A));
    A.blks = h->d_blks.p; A.anc_idx = h->d_anc.p; A.dch_idx = h->d_dch.p; A.list = h->d_lvl.p + L.first + L.own_lo; A.nlist = L.own_n;
    A.panels = h->d_panels[phys].p; A.w = h->d_w.p; A.y = h->d_y.p; A.xb = h->d_xb.p; A.z = h->d_z.p; A.mv = h->d_mv.p;
    A.obs = h->d_obs.p; A.acc = h->d_acc.p; A.errflag = h->d_err.p; A.maxP = L.maxP; A.maxM = L.maxM; A.maxLd = L.maxLd;
    for (int j = 0; j < QMAX; ++j) A.tausq_inv[j] = h->tausq_inv[j];
    A.do_gram = (h->gram_valid && h->cache_gram) ? 0 : 1;
    A.no_fwd = h->limited ? 1 : 0;
    A.lds_sq = (L.big_sample && L.sample_sq) ? 2 : 0;
    A.s0 = h->d_s0.p; A.s0off = h->d_s0off.p;
    {
      ProfScope ps(h, 1, h->n_actual_groups + g);   // per-level slots of phase B follow those of phase A
      if (L.fast) {
        SampleFastArgs F;
        std::memset(&F, 0, sizeof(F));
        F.do_gram = A.do_gram; F.no_fwd = A.no_fwd;
        F.blks = h->d_blks.p; F.anc_idx = h->d_anc.p; F.dch_idx = h->d_dch.p; F.grps = h->d_grps.p + L.grp_first + L.gown_lo; F.ngrp = L.gown_n;
        F.panels = h->d_panels[phys].p; F.w = h->d_w.p; F.y = h->d_y.p; F.xb = h->d_xb.p; F.z = h->d_z.p; F.mv = h->d_mv.p;
        F.acc = h->d_acc.p; F.errflag = h->d_err.p; F.ldN = L.ldN; F.Mr4 = L.Mr4; F.Mrows = L.Mrows; F.maxP = L.maxP; F.av_dbl = L.av_dbl;
        F.gdesc = h->d_gdesc.p + (size_t)(L.grp_first + L.gown_lo) * h->gd_stride; F.gd_stride = h->gd_stride;
        for (int j = 0; j < QMAX; ++j) F.tausq_inv[j] = h->tausq_inv[j];
        const bool lean_ok = h->sw.sample_lean && !(!L.isref && L.maxP > 255);
        F.gdesc_all = h->d_gdesc.p;
        // does level `gq` take k_gram + the lean kernels on a rebuild sweep?  (the same test for the level itself, below)
        auto splits = [&](int gq) {
          const LevelInfo &Lq = h->levels[gq];
          const bool lean_q = h->sw.sample_lean && !(!Lq.isref && Lq.maxP > 255);
          return Lq.fast && lean_q && h->sw.split_gram && (h->sw.split_gram == 2 || (Lq.isref && Lq.gown_n >= 32 * h->sm_count));
        };
        // the leaf level of a rebuild sweep writes NO Gram parts when its parents form them from the leaf panels (k_gram_direct)
        const bool direct_parent = F.do_gram && h->gram_direct_level == g && splits(g) && h->levels[g + 1].gown_n > 0;
        if (F.do_gram && lean_ok && g == h->gram_direct_level + 1 && h->gram_direct_level >= 0 && splits(g - 1) && h->levels[g - 1].gown_n > 0) F.do_gram = 0;
        // the theta-only Gram parts on their own (k_gram), then the lean sweep kernels: pays on big reference levels (n = 1e6,
        // level 7: 0.84 -> 0.72 ms averaged over a run's sweeps), loses on leaf levels and on smaller reference levels, where
        // the staged Gram of k_sample_mfma is cheaper (SPAMTREE_SPLIT_GRAM=2: every level; records identical either way)
        if (F.do_gram && lean_ok && h->sw.split_gram && (h->sw.split_gram == 2 || (L.isref && L.gown_n >= 32 * h->sm_count))) {
          if (direct_parent) { route[0] = R_GRAM_DIRECT; hipLaunchKernelGGL(k_gram_direct, dim3(L.gown_n), dim3(NT), 0, h->stream, F); }
          else { route[0] = R_GRAM; hipLaunchKernelGGL(k_gram, dim3(L.gown_n), dim3(NT), 0, h->stream, F); }
          F.do_gram = 0;
        }
        // reference levels on the lean kernels: the theta-only part of the posterior precision (Ri' Ri + the children's Gram parts)
        // is stored by the first such sweep after the records were rebuilt and loaded by the following ones (same bits either way)
        if (!(F.do_gram || !lean_ok) && L.isref) {
          F.s0 = h->d_s0.p; F.s0off = h->d_s0off.p;
          F.s0_mode = !h->cache_gram ? 0 : (h->s0_valid[g] ? 2 : 1);
          if (h->cache_gram) h->s0_valid[g] = 1;
        }
        if (F.do_gram || !lean_ok) { route[1] = R_SAMPLE_MFMA; hipLaunchKernelGGL(k_sample_mfma, dim3(L.gown_n), dim3(NT), L.lds_sfast, h->stream, F); }
        else if (!L.isref) {
          // segment-aligned lanes where the level's chains have at most 12 ancestors of at most 32 rows (SPAMTREE_LEAF_SEG=0: the
          // column-aligned kernel)
          const int need = (L.maxJ + 1) / 2;
          if (h->sw.leaf_seg && need <= 4 && L.maxMa <= 32) { route[1] = R_LEAF_SEG4; hipLaunchKernelGGL((k_sample_leaf_seg<4>), dim3(L.gown_n), dim3(NT), ((size_t)4 * 64 * 4 + 3 * 32) * 8, h->stream, F); }
          else if (h->sw.leaf_seg && need <= 6 && L.maxMa <= 32) { route[1] = R_LEAF_SEG6; hipLaunchKernelGGL((k_sample_leaf_seg<6>), dim3(L.gown_n), dim3(NT), ((size_t)4 * 64 * 6 + 3 * 32) * 8, h->stream, F); }
          else { route[1] = R_SAMPLE_LEAF; hipLaunchKernelGGL(k_sample_leaf, dim3(L.gown_n), dim3(NT), ((size_t)L.maxP + 32 + 4 * 256 + 3 * 32) * 8, h->stream, F); }
        }
        else if (h->sw.sample_wave && L.maxM <= 27 && (h->sw.sample_wave == 2 || L.gown_n >= 8 * h->sm_count)) {   // one block per wave: faster on a level
          // that keeps every CU busy for several rounds (n = 1e6 after the row-wise panel pass: level 7 0.44 -> 0.35 ms, level 6 -- 4096 blocks --
          // 0.151 -> 0.117), a wash at 1024 blocks (0.050 -> 0.046 there, 0.034 -> 0.039 at config #5), slower on latency-bound small levels (256 blocks: 0.029 -> 0.040): gd | wv | seg | tv, ev | Ri, per wave
          const size_t per = (((size_t)h->gd_stride + L.maxP + 32 + L.av_dbl + 64 + (size_t)std::max(L.maxM, 1) * CH_LD + 1) & ~(size_t)1);
          F.ldN = (int)per; F.Mrows = L.maxM;
          route[1] = R_SAMPLE_WAVE;
          hipLaunchKernelGGL(k_sample_wave, dim3((L.gown_n + NT / 64 - 1) / (NT / 64)), dim3(NT), per * 8 * (NT / 64), h->stream, F);
        } else {
          // levels that do not fill the chip (fewer groups than 2 x CUs x the five workgroups the occupancy variant fits): the
          // latency variant -- every descriptor-only load of a block in one round trip (SPAMTREE_SAMPLE_LAT=0: never; identical draws)
          F.av_dbl = L.av_dbl + 224;
          if (h->sw.sample_lat && L.gown_n <= 2 * h->sm_count) { route[1] = R_SAMPLE_LEAN_LAT; hipLaunchKernelGGL((k_sample_lean<true>), dim3(L.gown_n), dim3(NT), L.lds_slean, h->stream, F); }
          else { route[1] = R_SAMPLE_LEAN; hipLaunchKernelGGL((k_sample_lean<false>), dim3(L.gown_n), dim3(NT), L.lds_slean, h->stream, F); }
        }
      } else {
        if (A.do_gram && L.big_sample && h->sw.gram_big) {
          // the theta-only parts first, on the matrix cores (k_gram_big); the sweep kernel then takes its cached branch
          GramBigArgs Gb;
          std::memset(&Gb, 0, sizeof(Gb));
          Gb.blks = h->d_blks.p; Gb.anc_idx = h->d_anc.p; Gb.dch_idx = h->d_dch.p; Gb.list = A.list; Gb.nlist = A.nlist;
          Gb.panels = A.panels; Gb.acc = A.acc; Gb.s0 = A.s0; Gb.s0off = A.s0off; Gb.no_fwd = A.no_fwd;
          // both triangles unless every level of the tree is read by k_gram_big / the generic sweep's cached branch (tiles it >= jt /
          // the lower triangle only)
          bool all_big = true;
          for (const auto &L2 : h->levels) all_big = all_big && (L2.count == 0 || L2.big_sample);
          Gb.mirror = all_big ? 0 : 1;
          route[0] = R_GRAM_BIG;
          hipLaunchKernelGGL(k_gram_big, dim3(A.nlist), dim3(NT), 0, h->stream, Gb);
          A.do_gram = 0;
        }
        if (L.big_sample) {
          A.scratch = h->d_scratch.p; A.scratch_stride = h->scratch_stride;
          if (L.isref) { route[1] = R_SAMPLE_BIG_REF; hipLaunchKernelGGL((k_sample<true, false>), dim3(std::min(L.own_n, h->scratch_wgs)), dim3(NT), L.lds_sample, h->stream, A); }
          else if (h->sw.leaf_wide && !A.do_gram && L.maxM <= 64 && L.maxMa <= 96 && L.maxJ <= 8) {   // one coalesced pass, segment-aligned lanes
            route[1] = R_SAMPLE_LEAF_WIDE;
            hipLaunchKernelGGL(k_sample_leaf_wide, dim3(std::min(L.own_n, 16 * h->sm_count)), dim3(NT), ((size_t)4 * 64 * 12 + 3 * 64) * 8, h->stream, A);
          } else { route[1] = R_SAMPLE_BIG_LEAF; hipLaunchKernelGGL((k_sample<true, true>), dim3(std::min(L.own_n, h->scratch_wgs)), dim3(NT), L.lds_sample, h->stream, A); }
        } else {
          route[1] = R_SAMPLE_SMALL;
          hipLaunchKernelGGL((k_sample<false>), dim3(L.own_n), dim3(NT), L.lds_sample, h->stream, A);
        }
      }
    }
    HCHK(h, hipGetLastError());
  }
  return ST_OK;
}

// levels below the cut (this rank's subtrees); then the cut level's message records of the other ranks are zeroed so
// that an all-reduce(sum) over st_mg_top_region() completes them
extern "C" int st_sample_w_local(st_handle h, const double *z, uint64_t seed, uint32_t iter) {
  if (!h) return ST_ERR_USAGE;
  invalidate_stats(h);
  HCHK(h, hipSetDevice(h->device));
  int rc = gen_or_upload_z(h, z, seed, iter, 0u, h->d_z.p);
  if (rc) return rc;
  h->z_valid = true;
  rc = reset_err(h);
  if (rc) return rc;
  rc = sample_launch(h, h->n_actual_groups, std::min(h->cut, h->n_actual_groups));
  if (rc) return rc;
  for (auto &zr : h->top_zero) HCHK(h, hipMemsetAsync(h->d_acc.p + zr.first, 0, (size_t)zr.second * sizeof(double), h->stream));
  return ST_OK;
}
extern "C" int st_mg_top_region(st_handle h, void **dev_ptr, int64_t *len) {
  if (!h) return ST_ERR_USAGE;
  if (dev_ptr) *dev_ptr = h->d_acc.p + h->top_off;
  if (len) *len = h->top_len;
  return ST_OK;
}
extern "C" int st_sample_w_top(st_handle h) {   // the replicated levels above the cut
  if (!h) return ST_ERR_USAGE;
  invalidate_stats(h);
  HCHK(h, hipSetDevice(h->device));
  const int rc = sample_launch(h, std::min(h->cut, h->n_actual_groups), 0);
  if (rc == ST_OK) h->gram_valid = true;   // every record now carries the Gram sums of the accepted theta
  return rc;
}
extern "C" int st_mg_pack_w(st_handle h, void **dev_ptr, int64_t *len) {
  if (!h) return ST_ERR_USAGE;
  HCHK(h, hipSetDevice(h->device));
  const long long nn = std::max<long long>(h->n_all, h->world);
  hipLaunchKernelGGL(k_pack_w, dim3((unsigned)((nn + NT - 1) / NT)), dim3(NT), 0, h->stream, h->d_w.p, h->d_rowmask.p, h->n_all, h->d_err.p,
                     h->rank, h->world, h->d_tmp_n.p);
  HCHK(h, hipGetLastError());
  if (dev_ptr) *dev_ptr = h->d_tmp_n.p;
  if (len) *len = h->n_all + h->world;
  return ST_OK;
}
extern "C" int st_mg_unpack_w(st_handle h) {
  if (!h) return ST_ERR_USAGE;
  invalidate_stats(h);
  HCHK(h, hipSetDevice(h->device));
  double errw[ST_MAX_RANKS];
  HCHK(h, hipMemcpyAsync(h->d_w.p, h->d_tmp_n.p, (size_t)h->n_all * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  HCHK(h, hipMemcpyAsync(errw, h->d_tmp_n.p + h->n_all, h->world * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HCHK(h, hipStreamSynchronize(h->stream));
  return rank_failure(errw, h->world);
}

// all-gather form (half the traffic of the all-reduce of n doubles): pack -> all-gather(recv, count per rank) -> unpack
extern "C" int st_mg_gather_w_pack(st_handle h, void **send_ptr, void **recv_ptr, int64_t *count_per_rank) {
  if (!h) return ST_ERR_USAGE;
  HCHK(h, hipSetDevice(h->device));
  const int cnt = h->gather_cnt;
  double *mine = h->d_gather.p + (size_t)h->rank * cnt;
  hipLaunchKernelGGL(k_gather_pack, dim3((cnt + NT - 1) / NT), dim3(NT), 0, h->stream, h->d_w.p, h->d_gidx.p + (size_t)h->rank * cnt, cnt,
                     h->d_err.p, mine);
  HCHK(h, hipGetLastError());
  if (send_ptr) *send_ptr = mine;
  if (recv_ptr) *recv_ptr = h->d_gather.p;
  if (count_per_rank) *count_per_rank = cnt;
  return ST_OK;
}
static int gather_w_scatter(st_handle h) {   // launches only: rows into w, failure words into d_gerr
  const long long total = (long long)h->world * h->gather_cnt;
  hipLaunchKernelGGL(k_gather_unpack, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, h->stream, h->d_gather.p, h->d_gidx.p, h->gather_cnt,
                     total, h->d_w.p, h->d_gerr.p);
  HCHK(h, hipGetLastError());
  return ST_OK;
}
extern "C" int st_mg_gather_w_unpack(st_handle h) {
  if (!h) return ST_ERR_USAGE;
  invalidate_stats(h);
  HCHK(h, hipSetDevice(h->device));
  int rc = gather_w_scatter(h);
  if (rc) return rc;
  double errw[ST_MAX_RANKS];
  HCHK(h, hipMemcpyAsync(errw, h->d_gerr.p, h->world * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HCHK(h, hipStreamSynchronize(h->stream));
  return rank_failure(errw, h->world);
}

extern "C" int st_sample_w(st_handle h, const double *z, uint64_t seed, uint32_t iter) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = refuse_factor_open(h, "st_sample_w")) return rc;
  if (const int rc = refuse_sweep_pending(h, "st_sample_w")) return rc;
  if (uses_exchange(h)) {
    if (!h->comm) return refuse_without_comm(h, "st_sample_w_local / st_mg_top_region / st_sample_w_top / st_mg_pack_w / st_mg_unpack_w");
    void *snd = nullptr, *rcv = nullptr;
    int64_t cnt = 0;
    int rc = sweep_exchange(h, z, seed, iter, &snd, &rcv, &cnt);
    if (rc) return rc;
    {
      ProfScope ps(h, 7);
      NCHK(h, ncclAllGather(snd, rcv, (size_t)cnt, ncclDouble, h->comm, h->stream));
    }
    return st_mg_gather_w_unpack(h);
  }
  int rc = st_sample_w_local(h, z, seed, iter);
  if (rc) return rc;
  rc = st_sample_w_top(h);
  if (rc) return rc;
  Landing res;
  rc = enqueue_fail_word(h, &res);
  if (rc) return rc;
  HCHK(h, hipStreamSynchronize(h->stream));
  return landing_code(res, nullptr);  // 10 / 11: the reference stops with "Error at gibbs_sample_w" (:1215-1217)
}

extern "C" int st_loglik_local(st_handle h, int slot) {
  if (!h || slot < 0 || slot > 1) return ST_ERR_USAGE;
  HCHK(h, hipSetDevice(h->device));
  if (slot == 1) { const int rc0 = settle_top(h); if (rc0) return rc0; }
  { const int rc0 = complete_leaf(h, slot); if (rc0) return rc0; }
  const int phys = h->slot_map[slot];
  int maxP = 0, maxM = 0;
  for (auto &L : h->levels) { maxP = std::max(maxP, L.maxP); maxM = std::max(maxM, L.maxM); }
  const size_t lds = lds_loglik_bytes(maxP, maxM);
  LoglikArgs A;
  A.blks = h->d_blks.p; A.anc_idx = h->d_anc.p; A.list = h->d_ownslow.p; A.nlist = (int)h->own_obs_slow.size();
  A.panels = h->d_panels[phys].p; A.w = h->d_w.p; A.loglik_c = h->d_loglik[phys].p; A.resid = nullptr; A.maxP = maxP; A.maxM = maxM;
  {
    ProfScope ps(h, 2);
    if (A.nlist > 0) hipLaunchKernelGGL(k_loglik, dim3(A.nlist), dim3(NT), lds, h->stream, A);
    if (!h->own_grp_list.empty()) {
      LoglikGrpArgs Gr;
      Gr.blks = h->d_blks.p; Gr.anc_idx = h->d_anc.p; Gr.grps = h->d_grps.p; Gr.list = h->d_owngrp.p; Gr.nlist = (int)h->own_grp_list.size();
      Gr.panels = h->d_panels[phys].p; Gr.w = h->d_w.p; Gr.loglik_c = h->d_loglik[phys].p; Gr.maxP = maxP;
      Gr.gdesc = h->d_gdesc.p; Gr.gd_stride = h->gd_stride;
      hipLaunchKernelGGL(k_loglik_grp, dim3(Gr.nlist), dim3(NT), (size_t)(maxP + 32) * sizeof(double), h->stream, Gr);
    }
  }
  HCHK(h, hipGetLastError());
  HCHK(h, reset_err(h) == ST_OK ? hipSuccess : hipErrorUnknown);
  return ST_OK;
}
// the quadratic forms and the residuals of the top blocks with the CURRENT w (st_factor_begin ran them with the w of the sweep's start)
static int fix_top_comps(st_handle h, int phys) {
  if (h->n_toplist == 0) return ST_OK;
  int maxP = 0, maxM = 0;
  for (int g = 0; g < h->g_top; ++g) { maxP = std::max(maxP, h->levels[g].maxP); maxM = std::max(maxM, h->levels[g].maxM); }
  LoglikArgs A;
  A.blks = h->d_blks.p; A.anc_idx = h->d_anc.p; A.list = h->d_toplist.p; A.nlist = h->n_toplist;
  A.panels = h->d_panels[phys].p; A.w = h->d_w.p; A.loglik_c = h->d_loglik[phys].p; A.resid = h->d_resid.p; A.maxP = maxP; A.maxM = maxM;
  {
    ProfScope ps(h, 0, h->g_top > 0 ? h->g_top - 1 : 0);
    hipLaunchKernelGGL(k_loglik, dim3(A.nlist), dim3(NT), lds_loglik_bytes(maxP, maxM), h->stream, A);
  }
  HCHK(h, hipGetLastError());
  return ST_OK;
}
extern "C" int st_loglik_w(st_handle h, int slot, double *loglik) {
  if (!h) return ST_ERR_USAGE;
  if (slot >= 0 && slot <= 1) { if (const int rc = refuse_factor_open(h, "st_loglik_w", slot)) return rc; }
  if (const int rc = refuse_sweep_pending(h, "st_loglik_w")) return rc;
  if (slot >= 0 && slot <= 1) { const int rc0 = complete_leaf(h, slot); if (rc0) return rc0; }
  if (uses_exchange(h)) {
    if (!h->comm) return refuse_without_comm(h, "st_loglik_local / st_mg_pack_comps / (all-reduce) / st_mg_finish");
    int rc = st_loglik_local(h, slot);
    if (rc) return rc;
    return exchange_comps_and_finish(h, slot, loglik);
  }
  int rc = st_loglik_local(h, slot);
  if (rc) return rc;
  Landing res;
  rc = enqueue_slot_result(h, slot, &res);
  if (rc) return rc;
  HCHK(h, hipStreamSynchronize(h->stream));
  return landing_code(res, loglik);
}

extern "C" int st_predict(st_handle h, int theta_changed) {
  (void)theta_changed;  // H of a prediction block is rebuilt from the ancestor chain every call: same values as the cache
  if (!h) return ST_ERR_USAGE;
  if (const int rc = refuse_factor_open(h, "st_predict")) return rc;
  if (const int rc = refuse_sweep_pending(h, "st_predict")) return rc;
  if (h->pred_list.empty()) return ST_OK;
  invalidate_stats(h);
  if (!h->z_valid) { h->err = "st_predict needs the normals of a preceding st_sample_w (spamtree_model.cpp:1325)"; return ST_ERR_USAGE; }
  if (h->theta[0].empty()) { h->err = "st_predict before st_factor(slot 0)"; return ST_ERR_USAGE; }
  HCHK(h, hipSetDevice(h->device));
  CovPar cp;
  int rc = make_covpar(h, h->theta[0].data(), (int)h->theta[0].size(), &cp);
  if (rc) return rc;
  const LevelInfo &L = h->pred_info;
  if (h->pred_nkx > 0 && h->pred_quad_count > 0) {
    // (the records exist: layout_levels appends them under this very condition)
    QuadArgs F = quad_args(h, h->pred_grp_first, h->pred_qr_off, h->pred_qr_words, h->pred_quad_count, quad_lds_stride(h->pred_nkx), h->slot_map[0], h->d_err.p);
    F.wave_chol = 1; F.predict = 1; F.z = h->d_z.p; F.w_out = h->d_w.p;
    {
      ProfScope ps(h, 6);
      h->route_p = launch_quad(h->pred_nkx, false, true, h->pred_quad_count, h->pred_lds, h->stream, F, cp);
    }
    HCHK(h, hipGetLastError());
    HCHK(h, hipStreamSynchronize(h->stream));
    return ST_OK;
  }
  FactorArgs A;
  std::memset(&A, 0, sizeof(A));
  A.blks = h->d_blks.p; A.anc_idx = h->d_anc.p; A.list = h->d_pred.p; A.nlist = (int)h->pred_list.size();
  A.cx = h->d_cx.p; A.cy = h->d_cy.p; A.mv = h->d_mv.p; A.w_in = h->d_w.p; A.w_out = h->d_w.p; A.z = h->d_z.p;
  A.panels = h->d_panels[h->slot_map[0]].p; A.logdet_c = nullptr; A.loglik_c = nullptr; A.errflag = h->d_err.p;
  A.maxP = L.maxP; A.maxM = L.maxM; A.maxMa = L.maxMa; A.SR = L.big_factor ? 4 : 8;
  {
    ProfScope ps(h, 6);
    if (L.big_factor) { h->route_p = R_PREDICT_SCRATCH; launch_factor<true, MODE_PREDICT>(h, L, A, cp); }
    else { h->route_p = R_PREDICT_LDS; launch_factor<false, MODE_PREDICT>(h, L, A, cp); }
  }
  HCHK(h, hipGetLastError());
  HCHK(h, hipStreamSynchronize(h->stream));
  return ST_OK;
}

static int run_stats(st_handle h, hipStream_t st = nullptr) {
  const int nq = h->p * h->q + h->q;
  if (h->stats_valid) return ST_OK;   // w and XB unchanged since the last reduction: both statistics are still current
  if (!st) st = h->stream;
  {
    ProfScope ps(h, 4, -1, 1, st);
    launch_stats(h, st, nullptr);
    hipLaunchKernelGGL(k_stats_final, dim3(nq), dim3(NT), 0, st, h->d_partial.p, STATS_WG, nq, h->d_stats.p);
  }
  HCHK(h, hipGetLastError());
  h->stats_valid = true;
  return ST_OK;
}
// both statistics travel to the host together; a second request for the same (w, XB) is served from the host copy
static int fetch_stats(st_handle h) {
  if (h->stats_valid && h->host_stats_valid) return ST_OK;
  int rc = run_stats(h);
  if (rc) return rc;
  const size_t nq = (size_t)h->p * h->q + h->q;
  h->host_stats.resize(nq);
  if (h->stats_on_stream2) {   // started under phase A (stats_begin)
    if (h->stats_prefetched) {   // ... and already copied to pinned memory behind them on the second stream
      HCHK(h, hipEventSynchronize(h->ev_stats));
      HCHK(h, hipStreamWaitEvent(h->stream, h->ev_stats, 0));   // later work on the main stream stays ordered behind the reduction
      h->stats_on_stream2 = false;
      for (size_t i = 0; i < nq; ++i) h->host_stats[i] = h->pin->stats[i];
      h->host_stats_valid = true;
      return ST_OK;
    }
    HCHK(h, hipStreamWaitEvent(h->stream, h->ev_stats, 0));   // its results before the copy
    h->stats_on_stream2 = false;
  }
  HCHK(h, hipMemcpyAsync(h->host_stats.data(), h->d_stats.p, nq * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HCHK(h, hipStreamSynchronize(h->stream));
  h->host_stats_valid = true;
  return ST_OK;
}
extern "C" int st_beta_stats(st_handle h, double *xty) {
  if (!h || !xty) return ST_ERR_USAGE;
  HCHK(h, hipSetDevice(h->device));
  int rc = fetch_stats(h);
  if (rc) return rc;
  for (int i = 0; i < h->p * h->q; ++i) xty[i] = h->host_stats[i];
  return ST_OK;
}
extern "C" int st_tausq_stats(st_handle h, double *ssq, int64_t *n_obs_by_q) {
  if (!h || !ssq) return ST_ERR_USAGE;
  HCHK(h, hipSetDevice(h->device));
  int rc = fetch_stats(h);
  if (rc) return rc;
  for (int j = 0; j < h->q; ++j) ssq[j] = h->host_stats[(size_t)h->p * h->q + j];
  if (n_obs_by_q)
    for (int j = 0; j < h->q; ++j) n_obs_by_q[j] = h->n_obs_q[j];
  return ST_OK;
}
extern "C" int st_xtx(st_handle h, double *xtx) {
  if (!h || !xtx) return ST_ERR_USAGE;
  std::memcpy(xtx, h->xtx.data(), h->xtx.size() * sizeof(double));
  return ST_OK;
}

extern "C" int st_yhat(st_handle h, const double *noise, uint64_t seed, uint32_t iter, double *yhat) {
  if (!h || !yhat) return ST_ERR_USAGE;
  if (const int rc = refuse_sweep_pending(h, "st_yhat")) return rc;
  HCHK(h, hipSetDevice(h->device));
  int rc = gen_or_upload_z(h, noise, seed, iter, 5u, h->d_tmp_n.p);
  if (rc) return rc;
  const int grid = (int)((h->n_all + NT - 1) / NT);
  hipLaunchKernelGGL(k_yhat, dim3(grid), dim3(NT), 0, h->stream, h->d_xb.p, h->d_w.p, h->d_tmp_n.p, h->d_mv.p, h->n_all, h->d_tsq.p,
                     h->d_tmp_n.p);
  HCHK(h, hipGetLastError());
  return download_rows(h, h->d_tmp_n.p, yhat);
}

// ---- inspection ---------------------------------------------------------------------------------------------
extern "C" int st_block_dims(st_handle h, int64_t u, int64_t *m, int64_t *P, int32_t *is_ref, int32_t *n_obs) {
  if (!h || u < 0 || u >= h->n_blocks) return ST_ERR_USAGE;
  const Blk &B = h->blks[h->blk_model2dev[u]];
  if (m) *m = B.m;
  if (P) *P = B.P;
  if (is_ref) *is_ref = B.isref;
  if (n_obs) *n_obs = B.nobs;
  return ST_OK;
}
extern "C" int st_get_block(st_handle h, int slot, int64_t u, double *negRiH, double *Ri) {
  if (!h || u < 0 || u >= h->n_blocks || slot < 0 || slot > 1) return ST_ERR_USAGE;
  if (const int rc = refuse_factor_open(h, "st_get_block", slot)) return rc;
  const Blk &B = h->blks[h->blk_model2dev[u]];
  if (B.panel_off < 0) { h->err = "block has no observations, hence no cache"; return ST_ERR_USAGE; }
  HCHK(h, hipSetDevice(h->device));
  { const int rc0 = settle_top(h); if (rc0) return rc0; }
  { const int rc0 = complete_leaf(h, slot); if (rc0) return rc0; }
  std::vector<double> pan((size_t)B.m * B.ld);
  HCHK(h, hipMemcpyAsync(pan.data(), h->d_panels[h->slot_map[slot]].p + B.panel_off, pan.size() * sizeof(double), hipMemcpyDeviceToHost,
                         h->stream));
  HCHK(h, hipStreamSynchronize(h->stream));
  if (negRiH)
    for (int i = 0; i < B.m; ++i)
      for (int k = 0; k < B.P; ++k) negRiH[(size_t)k * B.m + i] = pan[(size_t)i * B.ld + k];
  if (Ri) {
    if (B.isref) {
      for (int i = 0; i < B.m; ++i)
        for (int j = 0; j < B.m; ++j) Ri[(size_t)j * B.m + i] = pan[(size_t)i * B.ld + B.P + j];
    } else {
      for (int i = 0; i < B.m; ++i) Ri[i] = pan[(size_t)i * B.ld + B.P];
    }
  }
  return ST_OK;
}
extern "C" int st_get_comps(st_handle h, int slot, double *logdet_c, double *loglik_c) {
  if (!h || slot < 0 || slot > 1) return ST_ERR_USAGE;
  if (const int rc = refuse_factor_open(h, "st_get_comps", slot)) return rc;
  HCHK(h, hipSetDevice(h->device));
  { const int rc0 = settle_top(h); if (rc0) return rc0; }
  const int phys = h->slot_map[slot];
  std::vector<double> a(h->n_blocks), b(h->n_blocks);
  HCHK(h, hipMemcpyAsync(a.data(), h->d_logdet[phys].p, h->n_blocks * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HCHK(h, hipMemcpyAsync(b.data(), h->d_loglik[phys].p, h->n_blocks * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HCHK(h, hipStreamSynchronize(h->stream));
  for (long long i = 0; i < h->n_blocks; ++i) {
    const int u = h->blks[i].model_id;
    if (logdet_c) logdet_c[u] = a[i];
    if (loglik_c) loglik_c[u] = b[i];
  }
  return ST_OK;
}

// ---- measurement --------------------------------------------------------------------------------------------
extern "C" int st_algorithmic_bytes(st_handle h, double *out5, double *flops3) {
  if (!h || !out5) return ST_ERR_USAGE;
  double a = 0, b = 0, c = 0, msg = 0, fa = 0, fb = 0, fc = 0;
  for (auto &L : h->levels) { a += L.alg_bytes_A; b += L.alg_bytes_B; c += L.alg_bytes_C; msg += L.alg_bytes_msg; fa += L.flops_A; fb += L.flops_B; fc += L.flops_C; }
  out5[0] = a; out5[1] = b; out5[2] = c; out5[3] = msg; out5[4] = 40.0 * (double)h->n_obs;
  if (flops3) { flops3[0] = fa; flops3[1] = fb; flops3[2] = fc; }
  return ST_OK;
}
extern "C" int st_profile_enable(st_handle h, int enable) {
  if (!h) return ST_ERR_USAGE;
  h->prof = enable == 2 ? 2 : (enable != 0 ? 1 : 0);
  return ST_OK;
}
extern "C" int st_profile_get(st_handle h, double *ms_total, int64_t *launches) {
  if (!h) return ST_ERR_USAGE;
  HCHK(h, hipSetDevice(h->device));
  prof_harvest(h);
  for (int f = 0; f < ST_N_KERNEL_FAMILIES; ++f) {
    if (ms_total) ms_total[f] = h->prof_ms[f];
    if (launches) launches[f] = h->prof_n[f];
    h->prof_ms[f] = 0; h->prof_n[f] = 0;
  }
  return ST_OK;
}
extern "C" int st_profile_levels(st_handle h, int32_t *n_levels, double *ms_by_level, double *bytes_by_level, int32_t cap) {
  if (!h || !n_levels) return ST_ERR_USAGE;
  HCHK(h, hipSetDevice(h->device));
  prof_harvest(h);
  *n_levels = h->n_actual_groups;
  // entries [0, n_levels): phase A; when cap >= 2 n_levels, entries [n_levels, 2 n_levels): phase B (k_sample*)
  const int ng = h->n_actual_groups;
  for (int g = 0; g < 2 * ng && g < cap; ++g) {
    if (ms_by_level) ms_by_level[g] = h->prof_level_n[g] ? h->prof_level_ms[g] / (double)h->prof_level_n[g] : 0.0;  // mean per launch
    if (bytes_by_level) bytes_by_level[g] = g < ng ? h->levels[g].alg_bytes_A : h->levels[g - ng].alg_bytes_B + h->levels[g - ng].alg_bytes_msg;
    h->prof_level_ms[g] = 0.0; h->prof_level_n[g] = 0;
  }
  return ST_OK;
}

// which phase-A kernel each observed level takes and the sizes that decide it (tests prove the branch they mean to reach)
extern "C" int st_level_info(st_handle h, int32_t *n_levels, int32_t *kernel, int32_t *max_m, int32_t *max_P, int32_t *n_blocks, int32_t cap) {
  if (!h || !n_levels) return ST_ERR_USAGE;
  *n_levels = h->n_actual_groups;
  for (int g = 0; g < h->n_actual_groups && g < cap; ++g) {
    const LevelInfo &L = h->levels[g];
    int k = L.big_factor ? ST_KERNEL_GENERIC_SCRATCH : ST_KERNEL_GENERIC_LDS;
    if (L.fast && h->sw.factor_gen == 3 && L.q_nkx > 0) k = ST_KERNEL_QUAD;
    else if (L.fast) k = ST_KERNEL_MFMA;
    else if (L.bigmfma && h->sw.factor_gen == 3) k = L.lchain ? (L.lchain_ref ? ST_KERNEL_LCHAIN_REF : ST_KERNEL_LCHAIN) : (L.wide_count > 0 ? ST_KERNEL_WIDE : ST_KERNEL_BIGMFMA);
    if (kernel) kernel[g] = k;
    if (max_m) max_m[g] = L.maxM;
    if (max_P) max_P[g] = L.maxP;
    if (n_blocks) n_blocks[g] = L.count;
  }
  return ST_OK;
}

extern "C" int st_route_info(st_handle h, int32_t *n_levels, int32_t *phase_a, int32_t *phase_b, int32_t *phase_p, int32_t cap) {
  if (!h || !n_levels) return ST_ERR_USAGE;
  *n_levels = h->n_actual_groups;
  for (int g = 0; g < h->n_actual_groups && g < cap; ++g) {
    for (int i = 0; i < ST_ROUTE_A_SLOTS && phase_a; ++i) phase_a[ST_ROUTE_A_SLOTS * g + i] = h->route_a[(size_t)ST_ROUTE_A_SLOTS * g + i];
    for (int i = 0; i < 2 && phase_b; ++i) phase_b[2 * g + i] = h->route_b[2 * (size_t)g + i];
  }
  if (phase_p) *phase_p = h->route_p;
  return ST_OK;
}
extern "C" const char *st_route_name(int32_t code) { return (code >= 0 && code < R_COUNT) ? k_route_names[code] : nullptr; }

// ---- CrossCovarianceAG10 (covariance_functions.cpp:301-355): dense n1 x n2 cross-covariance, column-major output.
// mv1 / mv2 are 1-based (as in R).  Like the reference it refuses a 1 x 1 Dmat ("Invalid Dmat for multivariate data").
extern "C" int st_cross_covariance_ag10(const double *coords1, const int64_t *mv1, int64_t n1, const double *coords2, const int64_t *mv2,
                                        int64_t n2, const double *ai1, const double *ai2, const double *phi_i, const double *thetamv,
                                        const double *Dmat, int32_t q, int32_t device, double *out) {
  if (!coords1 || !coords2 || !mv1 || !mv2 || !out || !Dmat || q < 2 || q > QMAX) {
    g_create_error = q < 2 ? "Invalid Dmat for multivariate data" : "st_cross_covariance_ag10: bad argument";
    return ST_ERR_USAGE;
  }
  if (n1 < 0 || n2 < 0) { g_create_error = "st_cross_covariance_ag10: negative extent"; return ST_ERR_USAGE; }
  if (n1 == 0 || n2 == 0) return ST_OK;   // the reference's empty matrix: nothing to compute, nothing written
  if (hipSetDevice(device) != hipSuccess) { g_create_error = "no usable HIP device"; return ST_ERR_HIP; }
  CovPar cp;
  std::memset(&cp, 0, sizeof(cp));
  cp.q = q; cp.ncb = q > 2 ? 3 : 1;
  for (int j = 0; j < q; ++j) { cp.ai1[j] = ai1[j]; cp.ai2[j] = ai2[j]; cp.phi[j] = phi_i[j]; }
  for (int j = 0; j < cp.ncb; ++j) cp.tmv[j] = thetamv[j];
  for (int i = 0; i < q * q; ++i) cp.D[i] = Dmat[i];   // symmetric: layout irrelevant
  finish_covpar(&cp);
  std::vector<int> m1(n1), m2(n2);
  for (int64_t i = 0; i < n1; ++i) { m1[i] = (int)mv1[i] - 1; if (m1[i] < 0 || m1[i] >= q) { g_create_error = "mv1 out of range"; return ST_ERR_USAGE; } }
  for (int64_t i = 0; i < n2; ++i) { m2[i] = (int)mv2[i] - 1; if (m2[i] < 0 || m2[i] >= q) { g_create_error = "mv2 out of range"; return ST_ERR_USAGE; } }
  DevBuf<double> d1, d2, dout;
  DevBuf<int> dm1, dm2;
  int rc = ST_OK;
  auto bad = [&](hipError_t e) { if (e != hipSuccess) { g_create_error = hipGetErrorString(e); rc = ST_ERR_HIP; } return e != hipSuccess; };
  if (!bad(d1.alloc(2 * n1)) && !bad(d2.alloc(2 * n2)) && !bad(dout.alloc((size_t)n1 * n2)) && !bad(dm1.upload(m1)) && !bad(dm2.upload(m2)) &&
      !bad(hipMemcpy(d1.p, coords1, 2 * n1 * sizeof(double), hipMemcpyHostToDevice)) &&
      !bad(hipMemcpy(d2.p, coords2, 2 * n2 * sizeof(double), hipMemcpyHostToDevice))) {
    // gridDim.y is bounded (a grid's y extent is limited to 65535 workgroups): k_cross_cov strides over the columns beyond it
    const unsigned gy = (unsigned)std::min<int64_t>(n2, 4096);
    hipLaunchKernelGGL(k_cross_cov, dim3((unsigned)((n1 + NT - 1) / NT), gy), dim3(NT), 0, 0, d1.p, dm1.p, (long long)n1, d2.p, dm2.p,
                       (long long)n2, cp, dout.p);
    if (!bad(hipGetLastError())) bad(hipMemcpy(out, dout.p, (size_t)n1 * n2 * sizeof(double), hipMemcpyDeviceToHost));
  }
  return rc;
}
