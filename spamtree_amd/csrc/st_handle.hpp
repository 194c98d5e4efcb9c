// st_handle.hpp -- what the host translation units of the library share: the handle behind st_handle, its self-freeing device
// buffers, the HIP error checks of the C-ABI functions, the launch timing, and the functions one host unit defines for another.
// The iteration's host code is one unit per phase: spamtree_hip.hip owns the handle's lifecycle (st_create, st_destroy), its
// accessors, the read-back helpers, inspection and measurement; st_factor.hip phases A and P with the proposal protocol;
// st_sweep.hip phases B and C; st_shard.hip everything that needs a communicator or serves a caller-run exchange; st_stats.hip
// the statistics and the outputs that read w and XB.  A feature family has a host unit of its own, which defines the family's
// state; the handle only points to it: st_points.hip new-point prediction, st_rows.hip the criteria over the fit's rows with
// leave-one-out and Pareto smoothing, st_simulate.hip prior simulation, st_summary.hip the running summaries (state: the handle's).  Above the C-ABI, spamtree_fit.cpp
// is the whole-fit driver; fit_plan.cpp works out its request without a device, as tree_layout.cpp and points_layout.cpp do theirs.
// Members that one unit alone reads and writes are a member structure named after their job (the lifecycle sets them up and
// tears them down); what several units read is flat in the handle, under a heading.
#pragma once
#include "tree_layout.hpp"
#include "st_protocol.hpp"
#include "draw_store.hpp"

// A device allocation that frees itself; a null buffer makes no HIP call.  (The owner has the device current when it goes.)
template <typename T>
struct DevBuf {
  T *p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  DevBuf(DevBuf &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
  DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { free(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; } return *this; }
  ~DevBuf() { free(); }
  hipError_t alloc(size_t count) {
    n = count;
    if (count == 0) { p = nullptr; return hipSuccess; }
    return hipMalloc((void **)&p, count * sizeof(T));
  }
  hipError_t upload(const std::vector<T> &v) {
    hipError_t e = alloc(v.size());
    if (e != hipSuccess || v.empty()) return e;
    return hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
  }
  void free() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
};

// st_factor.hip: phase A of the latency-bound top levels ahead of time (st_factor_begin).  They depend on theta only -- except
// for the blocks' quadratic forms, redone with the current w afterwards -- and run on the second stream under the sweep.
struct AheadTop {
  hipEvent_t ev_top = nullptr;                // behind the top levels' launches on the second stream
  DevBuf<int> d_err2, d_toplist;              // their failure word (merged into d_err when they are picked up); the top blocks
  bool async_top = false, async_top_off = false, top_pending = false;
  int top_phys = -1;                          // what was factorised ahead: the arena ...
  std::vector<double> top_theta;              // ... and the theta
};

// st_shard.hip: the buffers of the exchanges between ranks, and the communicator
struct Exchange {
  DevBuf<int> d_ownobs;                       // this rank's observed blocks
  DevBuf<unsigned char> d_rowmask, d_blkmask; // 1 = this rank contributes the entry to a sum-with-zeros exchange
  DevBuf<double> d_comm;                      // 2*n_blocks + 64 doubles
  DevBuf<double> d_gather;                    // all-gather of w: world x gather_cnt (a rank's owned rows in device order + its failure word)
  DevBuf<int> d_gidx;                         // device row of every slot of d_gather (-1: padding / the failure word)
  DevBuf<double> d_gerr;                      // the ranks' failure words after the all-gather (64)
  ncclComm_t comm = nullptr;                  // native RCCL communicator (st_comm_init); null = exchanges are the caller's
};

// st_stats.hip: what is known of the beta / tausq statistics of the current (w, XB)
struct StatsCache {
  bool valid = false;                         // d_stats matches the current w and XB
  bool host_valid = false;                    // ... and `host` holds a copy of it
  std::vector<double> host;
  bool on_stream2 = false;                    // the statistics kernels of the current (w, XB) are in flight on the second stream
  bool prefetched = false;                    // ... and their results follow them to pin->stats on that stream
  hipEvent_t ev = nullptr;                    // ... with this event behind them
};

// spamtree_hip.hip (st_profile_*), through ProfScope below: the launch timing
struct Profile {
  int mode = 0;   // 0 off, 1 every kernel family, 2 phase A only (the roofline measurement at the lowest cost)
  double ms[ST_N_KERNEL_FAMILIES] = {0};
  long long n[ST_N_KERNEL_FAMILIES] = {0};
  std::vector<double> level_ms;   // phase-A time per level, accumulated
  std::vector<long long> level_n;
  struct Rec { hipEvent_t a, b; int fam, level, count; };   // count: kernel launches inside the bracket
  std::vector<Rec> pending;
  std::vector<hipEvent_t> ev_free;
};

struct st_handle_s : TreeLayout {
  // ---- the device, the streams, errors
  std::string err;
  int device = 0;
  hipStream_t stream = nullptr;
  bool ext_stream = false;
  hipStream_t stream2 = nullptr;              // the second stream: the ahead-of-time top levels (st_factor.hip) and the statistics
  hipEvent_t ev_main = nullptr;               // under phase A (st_stats.hip); ev_main orders it behind the main stream
  bool prof_suspend = false;                  // st_factor_begin: launches that overlap the sweep on the second stream are not timed
  int quirks = 1;
  // ---- the rows and the chain's state
  long long n_obs = 0;
  std::vector<long long> n_obs_q;
  std::vector<double> xtx;
  DevBuf<double> d_cx, d_cy, d_y, d_X, d_w, d_xb, d_z, d_B, d_panels[2], d_acc, d_logdet[2], d_loglik[2], d_scalars, d_partial,
      d_stats, d_xtx, d_scratch, d_tmp_n, d_tsq;
  DevBuf<int> d_mv, d_anc, d_dch, d_lvl, d_pred, d_allobs, d_err;
  DevBuf<unsigned char> d_obs;
  DevBuf<long long> d_dev2model, d_partner;
  int slot_map[2] = {0, 1};    // logical slot (0 param, 1 alter) -> physical arena
  double tausq_inv[QMAX];
  std::vector<double> theta[2];
  bool z_valid = false;
  // ---- the device copies of the layout's lists (tree_layout.hpp)
  DevBuf<Blk> d_blks;
  DevBuf<Grp> d_grps;
  DevBuf<long long> d_qrec;                   // the quad records (TreeLayout::qrec): k_factor_quad's workgroups start from them
  DevBuf<WideGrp> d_wgrps;
  DevBuf<LcSlab> d_lcslabs;
  DevBuf<long long> d_rfvoff, d_gdesc;
  DevBuf<int> d_twin;
  DevBuf<int> d_owngrp, d_ownslow;            // this rank's observed blocks (phase C): column groups of the fast levels / blocks of the others
  DevBuf<double> d_vscr;                      // V = Linv_pa K_pa,u of ONE such level (the largest): written by k_factor_lchain, read by k_factor_ref_finish
  DevBuf<double> d_lcrow;                     // per-row e^2 | log r of the lchain levels (2 n)
  // ---- what a sweep caches for the accepted theta
  DevBuf<double> d_s0;                        // Ri' Ri of the reference blocks on the generic phase-B path (theta-only, cached with the Gram parts)
  DevBuf<long long> d_s0off;                  // per block: offset into d_s0, -1 = none
  std::vector<char> s0_valid;                 // per level: d_s0 holds the theta-only precision parts of the accepted theta (column-group levels)
  bool gram_valid = false;                    // message Gram parts in `acc` match the accepted theta (slot 0)
  bool cache_gram = true;
  // ---- the read-back protocol and the split operations (st_protocol.hpp)
  PinnedArea *pin = nullptr;                  // pinned host memory of the small device-to-host reads, one member per request (st_protocol.hpp)
  double *pin_up = nullptr;                   // pinned staging of the small per-iteration uploads (beta, tausq_inv): two slots taken in turn,
  int pin_up_slot = 0, pin_up_len = 0;        // so that the copy is truly asynchronous and the setters need no host synchronisation
  hipEvent_t ev_up[2] = {nullptr, nullptr};   // recorded behind a slot's copy: a slot is rewritten only after its last copy has run
  bool c_pending = false;                     // st_sample_w_loglik_begin: the sweep's failure word and log-density are on their way to pin->deferred
  int c_rc = 0; double c_ll = 0.0;            // ... or (multi-GPU / communicator attached) already here
  bool factor_open = false; int factor_open_slot = 0;   // st_factor_enqueue without its st_factor_finish yet
  std::vector<double> top_theta_open;                   // ... its theta where the work itself waits for st_factor_finish (communicator attached)
  hipEvent_t ev_factor = nullptr;                       // behind the copies of an enqueued factorisation's sums and failure word
  // ---- a proposal's quad leaf levels (st_factor_enqueue on slot 1): QM_VONLY, their panels finished by QM_TFROMV from d_vleaf when
  // the slot is read (st_swap, st_get_block, st_loglik_*); re-factorising the slot drops the pending half
  bool leaf_pending[2] = {false, false};   // per physical arena
  CovPar leaf_cp[2];
  DevBuf<double> d_vleaf;
  // The whitened residuals e = Ri (w_u - H_u w_pa) of the reference blocks, per device row (n_all): every phase-A route stores
  // what it squares for the block's loglik_w component, and the leaf bodies of k_factor_quad gather them as the g = Linv_pa w_pa
  // of their chain (limited trees: k_marginal_invchol stores chol(K_uu)^{-1} w_u instead, the g of the marginal chain).  ONE
  // buffer for both slots: it is read only by the leaf launch of the factorisation that wrote it, on the same stream; the top
  // levels st_factor_begin runs ahead of time on the second stream are ordered behind everything issued before them, nothing on
  // the main stream reads the buffer until factor_local has waited for them, and their (stale) rows are rewritten by
  // fix_top_comps before the levels below are launched.
  DevBuf<double> d_resid;
  // ---- inspection: per level, ST_ROUTE_A_SLOTS phase-A / 2 phase-B route codes of the last launch (st_routes.hpp)
  std::vector<int> route_a, route_b;
  int route_p = ST_ROUTE_NONE;                // ... and of the last st_predict
  // ---- what one unit alone reads and writes (above)
  AheadTop ahead;
  Exchange xch;
  StatsCache stats;
  Profile prof;
  // ---- The running summaries (st_summary.hip), always present: the criteria over the rows read the stored draws and their epoch
  DevBuf<double> d_sum_w, d_sum_yhat;         // running sums over saved iterations (st_summary_*)
  long long n_summary = 0;
  DevBuf<double> d_draws_w, d_draws_yhat;     // st_summary_reserve: the saved draws themselves, [keep][n_all] (quantiles)
  long long draws_cap = 0, n_draws = 0;
  long long draws_epoch = 0;                  // advances whenever the stored draws of st_summary_reserve change
  // ---- The state of a feature family is defined in the family's host unit and owned here; null: not set.  st_destroy drops each.
  struct PointSet *pts = nullptr;             // st_points.hip: new locations to predict at
  struct RowsScore *rows = nullptr;           // st_rows.hip: the criteria over the fit's own rows
  struct RowsLoo *loo = nullptr;              // st_rows.hip: the leave-one-out criteria and their Pareto store
  struct SimState *sim = nullptr;             // st_simulate.hip: the level plan and the draws' buffers
};

#define HCHK(h, call)                                                                                         \
  do {                                                                                                        \
    hipError_t e_ = (call);                                                                                   \
    if (e_ != hipSuccess) {                                                                                   \
      (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                                           \
      return ST_ERR_HIP;                                                                                      \
    }                                                                                                         \
  } while (0)

// Launch timing with HIP events on the launch stream, harvested lazily (no host sync inside the measured region).
inline hipEvent_t prof_event(st_handle_s *h) {
  if (!h->prof.ev_free.empty()) { hipEvent_t e = h->prof.ev_free.back(); h->prof.ev_free.pop_back(); return e; }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}
inline void prof_harvest(st_handle_s *h) {
  for (auto &r : h->prof.pending) {
    float ms = 0.f;
    if (hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
      h->prof.ms[r.fam] += ms;
      h->prof.n[r.fam] += r.count;
      // (count 0: the deferred half of a level's launch -- its time, not another launch)
      if (r.level >= 0 && r.level < (int)h->prof.level_ms.size()) { h->prof.level_ms[r.level] += ms; h->prof.level_n[r.level] += r.count > 0; }
    }
    h->prof.ev_free.push_back(r.a);
    h->prof.ev_free.push_back(r.b);
  }
  h->prof.pending.clear();
}
struct ProfScope {
  st_handle_s *h;
  Profile::Rec r;
  // mode 1: every launch is bracketed; mode 2: only the whole-phase bracket of phase A (level == -2), one pair of events
  hipStream_t st;
  ProfScope(st_handle_s *h_, int fam, int level = -1, int count = 1, hipStream_t st_ = nullptr) : h(h_), st(st_ ? st_ : h_->stream) {
    r.fam = fam; r.level = level; r.count = count; r.a = r.b = nullptr;
    const bool on = level == -2 ? (h->prof.mode == 2 && !h->prof_suspend) : h->prof.mode == 1;
    if (on) { r.a = prof_event(h); r.b = prof_event(h); (void)hipEventRecord(r.a, st); }
  }
  ~ProfScope() {
    if (r.a && r.b) {
      (void)hipEventRecord(r.b, st);
      h->prof.pending.push_back(r);
      if (h->prof.pending.size() > 8192) prof_harvest(h);
    }
  }
};

// A launcher's failure (the HIP error it returns as an int) as the entry point's: "<what> launch: <HIP's text>"
inline int launch_failed(st_handle_s *h, const std::string &what, int e) { h->err = what + " launch: " + hipGetErrorString((hipError_t)e); return ST_ERR_HIP; }

// The one read-back of a store's per-series outputs (draw_store.hpp): rows x s.n values at the device address src, store order, into
// the caller's dst through s.perm.  A part without dst, src or rows is skipped -- only what the caller asked for comes to the host.
// The copies go on h->stream behind whatever the caller issued there, then one synchronise, then the scatters.
template <typename T> struct StorePart { T *dst; const T *src; long long rows; };
inline int store_read_back(st_handle_s *h, const DrawStore &s, const std::vector<StorePart<double>> &pd, const std::vector<StorePart<int32_t>> &pi) {
  std::vector<std::vector<double>> td(pd.size());
  std::vector<std::vector<int32_t>> ti(pi.size());
  const auto issue = [&](const auto &parts, auto &tmp) {
    for (size_t k = 0; k < parts.size(); ++k) {
      if (!parts[k].dst || !parts[k].src || parts[k].rows == 0) continue;
      tmp[k].resize((size_t)parts[k].rows * s.n);
      HCHK(h, hipMemcpyAsync(tmp[k].data(), parts[k].src, tmp[k].size() * sizeof(tmp[k][0]), hipMemcpyDeviceToHost, h->stream));
    }
    return (int)ST_OK;
  };
  const auto land = [&](const auto &parts, const auto &tmp) {
    for (size_t k = 0; k < parts.size(); ++k)
      if (!tmp[k].empty()) scatter_rows(parts[k].dst, tmp[k].data(), parts[k].rows, s.n, s.perm);
  };
  if (const int rc = issue(pd, td)) return rc;
  if (const int rc = issue(pi, ti)) return rc;
  HCHK(h, hipStreamSynchronize(h->stream));
  land(pd, td);
  land(pi, ti);
  return ST_OK;
}

template <typename T>
inline hipError_t upload_or_dummy(DevBuf<T> &d, const std::vector<T> &v) {   // an empty list still gets one (zero) element to point at
  return v.empty() ? d.upload(std::vector<T>(1)) : d.upload(v);
}

// ---- what one host unit defines for the others, under the name of the defining unit
// spamtree_hip.hip
int upload_rows(st_handle h, const double *src, double *dst);     // n_all doubles, model row order -> device row order
int download_rows(st_handle h, const double *src, double *dst);   // ... and back
int refuse_factor_open(st_handle h, const char *who, int slot = -1);
int refuse_sweep_pending(st_handle h, const char *who);
int enqueue_result(st_handle h, const double *a, const double *b, int n, Landing *dst);   // the read-back protocol (st_protocol.hpp)
int enqueue_slot_result(st_handle h, int slot, Landing *dst);
int enqueue_fail_word(st_handle h, Landing *dst);
int reset_err(st_handle h);
// st_factor.hip
constexpr int QUAD_SIZES = 4, QUAD_KINDS = 3;
const void *quad_kernel_address(int size, int kind);   // the instantiations of k_factor_quad, for the attributes st_create reads and sets
int make_covpar(st_handle h, const double *theta, int ntheta, CovPar *cp);
int settle_top(st_handle h);
int complete_leaf(st_handle h, int slot);
// st_sweep.hip
int gen_or_upload_z(st_handle h, const double *z, uint64_t seed, uint32_t iter, unsigned stream_id, double *dst);
struct LoglikArgs;   // (misc_kernels.hpp) k_loglik over `list` with the maxima of the levels below n_levels; the caller launches
void loglik_args(st_handle h, int phys, int n_levels, const int *list, int nlist, double *resid, LoglikArgs *A);
// st_shard.hip: whether the exchange protocol applies, and the exchange branch of each entry point of the iteration
bool uses_exchange(st_handle h);
void comm_free(st_handle_s *h);   // st_destroy: the communicator, if one is attached
int shard_factor(st_handle h, int slot, const double *theta, int ntheta, double *loglik);
int shard_factor_enqueue(st_handle h, int slot, const double *theta, int ntheta);
int shard_factor_finish(st_handle h, double *loglik);
int shard_sample_w(st_handle h, const double *z, uint64_t seed, uint32_t iter);
int shard_sample_w_loglik(st_handle h, const double *z, uint64_t seed, uint32_t iter, int slot, double *loglik);
int shard_sample_w_loglik_begin(st_handle h, const double *z, uint64_t seed, uint32_t iter, int slot);
int shard_loglik_w(st_handle h, int slot, double *loglik);
// st_stats.hip
void launch_stats(st_handle_s *h, hipStream_t st, const double *wt);   // k_stats over all rows into d_partial (wt: the weight column of XtX, or null)
void invalidate_stats(st_handle_s *h);                                 // w or XB is about to change
int stats_begin(st_handle h);                                          // the statistics on the second stream, under a proposal's phase A
// each drops its unit's state of the handle (st_destroy, and the unit's own clear and set): st_points.hip, st_rows.hip, st_simulate.hip
void points_free(st_handle_s *h); void rows_free(st_handle_s *h); void loo_free(st_handle_s *h); void sim_free(st_handle_s *h);
