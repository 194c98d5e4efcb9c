// spamtree_hip.hip -- the handle of the gfx950 library: its lifecycle, its accessors, what the host units of the iteration share,
// inspection and measurement.
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
// The HOST side is one translation unit per job (st_handle.hpp lists what they share).  This one: st_create with its device
// steps and st_destroy, the sharding plan, the stream and row accessors (st_set_w, st_get_w, st_get_resid), the refusals of the
// split operations, the read-back helpers every phase ends with (enqueue_result, enqueue_slot_result, enqueue_fail_word,
// reset_err), inspection (st_get_block, st_get_comps, st_level_info, st_route_*), measurement (st_profile_*) and
// st_cross_covariance_ag10.  It launches no per-level kernel: phases A and P and the proposal protocol are st_factor.hip, phases B
// and C st_sweep.hip, the exchanges between ranks st_shard.hip, the statistics and the outputs that read w and XB st_stats.hip.
// The feature families have their C-ABI and their state in host units of their own: new-point prediction in st_points.hip, the
// criteria over the fit's rows, leave-one-out and Pareto smoothing in st_rows.hip, prior simulation in st_simulate.hip, the
// running summaries in st_summary.hip.  tree_layout.cpp builds the launch structures without a device call (the handle derives
// from its TreeLayout).  The kernels live in one translation unit per family (k_factor_*.hip, k_sample.hip, k_misc.hip); the
// headers included here give the prototypes st_create reads and sets attributes of.

#include "st_handle.hpp"
#include "st_routes.hpp"
#include "misc_kernels.hpp"
#include <new>

// ===============================================================================================================
// host side
// ===============================================================================================================
static thread_local std::string g_create_error;

static int fail_create(st_handle_s *h, int code, const std::string &msg) {
  g_create_error = msg;
  if (h) {
    st_destroy(h);
  }
  return code;
}

extern "C" const char *st_last_error(st_handle h) { return h ? h->err.c_str() : g_create_error.c_str(); }
extern "C" void st_set_create_error(const char *msg) { g_create_error = msg ? msg : ""; }   // other translation units of the library

extern "C" int st_destroy(st_handle h) {
  if (!h) return ST_OK;
  (void)hipSetDevice(h->device);
  if (h->ahead.ev_top) (void)hipEventDestroy(h->ahead.ev_top);
  if (h->ev_main) (void)hipEventDestroy(h->ev_main);
  if (h->stats.ev) (void)hipEventDestroy(h->stats.ev);
  if (h->stream2) (void)hipStreamDestroy(h->stream2);
  prof_harvest(h);
  for (auto e : h->prof.ev_free) (void)hipEventDestroy(e);
  comm_free(h);
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
  if (hipFuncGetAttributes(&fa, quad_kernel_address(QUAD_SIZES - 1, 2)) == hipSuccess) dl.quad_static = fa.sharedSizeBytes;
  for (int kind = 0; kind < 2; ++kind)
    if (hipFuncGetAttributes(&fa, quad_kernel_address(QUAD_SIZES - 1, kind)) == hipSuccess) dl.quad_static = std::max(dl.quad_static, (size_t)fa.sharedSizeBytes);
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
  CCHK(upload_or_dummy(h->xch.d_ownobs, h->own_obs_list));
  CCHK(upload_or_dummy(h->d_owngrp, h->own_grp_list)); CCHK(upload_or_dummy(h->d_ownslow, h->own_obs_slow));
  CCHK(h->xch.d_rowmask.upload(h->rowmask)); CCHK(h->xch.d_blkmask.upload(h->blkmask));
  CCHK(h->xch.d_comm.alloc((size_t)2 * h->n_blocks + ST_MAX_RANKS));
  CCHK(h->xch.d_gidx.upload(h->gidx));
  CCHK(h->xch.d_gather.alloc(h->gidx.size()));
  CCHK(h->xch.d_gerr.alloc(ST_MAX_RANKS));
  CCHK(upload_or_dummy(h->ahead.d_toplist, h->top_list));
  CCHK(h->ahead.d_err2.alloc(2));
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
    for (int kind = 0; kind < QUAD_KINDS; ++kind) dyn(quad_kernel_address(size, kind), cu - (int)dl.quad_static);
  // the top levels are a fixed cost (0.19 ms at n = 1e6: a quarter of a rank's phase A on 8 GPUs, 40 % of phase A at
  // n = 1e5); at n = 1e6 on one GPU the sweep fills the chip and the gain is 1.5 % (SPAMTREE_ASYNC_TOP=0 turns it off)
  h->ahead.async_top = h->g_top > 0 && h->sw.async_top;
  if (h->ahead.async_top) {
    CCHK(hipStreamCreateWithFlags(&h->stream2, hipStreamNonBlocking));
    CCHK(hipEventCreateWithFlags(&h->ahead.ev_top, hipEventDisableTiming));
    CCHK(hipEventCreateWithFlags(&h->ev_main, hipEventDisableTiming));
    CCHK(hipEventCreateWithFlags(&h->stats.ev, hipEventDisableTiming));
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
  h->prof.level_ms.assign(2 * n_actual, 0.0);
  h->prof.level_n.assign(2 * n_actual, 0);
  if ((rc = create_rows(h, pb)) || (rc = create_layout_buffers(h)) || (rc = create_state(h)) || (rc = create_attributes(h, dl)))
    return fail_create(h, rc, std::string(g_create_error));
  *out = h;
  return ST_OK;
}

// ---- simple state accessors ---------------------------------------------------------------------------------
int upload_rows(st_handle h, const double *src, double *dst) {
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
  { const int rc0 = settle_top(h); if (rc0) return rc0; }   // (the second stream may be writing top rows)
  return download_rows(h, h->d_resid.p, out);
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

// ---- the read-back protocol (st_protocol.hpp): every result of the iteration comes back as a Landing --------------------------
// The sums of a and b (n entries each) on the launch stream, and their copy into dst.
int enqueue_result(st_handle h, const double *a, const double *b, int n, Landing *dst) {
  {
    ProfScope ps(h, 3);
    launch_sum2(h->stream, a, b, n, h->d_scalars.p + 8, h->d_scalars.p);
  }
  HCHK(h, hipGetLastError());
  HCHK(h, hipMemcpyAsync(dst->sums, h->d_scalars.p, 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  return ST_OK;
}
// ... of a slot's component arrays
int enqueue_slot_result(st_handle h, int slot, Landing *dst) {
  const int phys = h->slot_map[slot];
  return enqueue_result(h, h->d_logdet[phys].p, h->d_loglik[phys].p, (int)h->n_blocks, dst);
}
// The failure word's copy into dst.  On its own because a sweep's word has to leave EARLIER in stream order than the sums: phase C
// (st_loglik_local) resets it.
int enqueue_fail_word(st_handle h, Landing *dst) {
  HCHK(h, hipMemcpyAsync(dst->err, h->d_err.p, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  return ST_OK;
}
int reset_err(st_handle h) {
  const int init[2] = {INT_MAX, 0};
  HCHK(h, hipMemcpyAsync(h->d_err.p, init, 2 * sizeof(int), hipMemcpyHostToDevice, h->stream));
  return ST_OK;
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
  h->prof.mode = enable == 2 ? 2 : (enable != 0 ? 1 : 0);
  return ST_OK;
}
extern "C" int st_profile_get(st_handle h, double *ms_total, int64_t *launches) {
  if (!h) return ST_ERR_USAGE;
  HCHK(h, hipSetDevice(h->device));
  prof_harvest(h);
  for (int f = 0; f < ST_N_KERNEL_FAMILIES; ++f) {
    if (ms_total) ms_total[f] = h->prof.ms[f];
    if (launches) launches[f] = h->prof.n[f];
    h->prof.ms[f] = 0; h->prof.n[f] = 0;
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
    if (ms_by_level) ms_by_level[g] = h->prof.level_n[g] ? h->prof.level_ms[g] / (double)h->prof.level_n[g] : 0.0;  // mean per launch
    if (bytes_by_level) bytes_by_level[g] = g < ng ? h->levels[g].alg_bytes_A : h->levels[g - ng].alg_bytes_B + h->levels[g - ng].alg_bytes_msg;
    h->prof.level_ms[g] = 0.0; h->prof.level_n[g] = 0;
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
