// st_handle.hpp -- what the host translation units of the library share: the handle behind st_handle, its self-freeing device
// buffers, the HIP error checks of the C-ABI functions and the launch timing.  spamtree_hip.hip owns the handle (st_create,
// st_destroy) and everything the Gibbs sweep launches.  A feature family has a host unit of its own, which defines the family's
// state; the handle only points to it: st_points.hip new-point prediction, st_rows.hip the criteria over the fit's rows with
// leave-one-out and Pareto smoothing, st_simulate.hip prior simulation, st_summary.hip the running summaries (state: the handle's).
#pragma once
#include "tree_layout.hpp"
#include "st_protocol.hpp"

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

struct st_handle_s : TreeLayout {
  std::string err;
  int device = 0;
  hipStream_t stream = nullptr;
  int quirks = 1;
  long long n_obs = 0;
  DevBuf<Grp> d_grps;                         // the device copies of the layout's lists (tree_layout.hpp)
  DevBuf<long long> d_qrec;                   // the quad records (TreeLayout::qrec): k_factor_quad's workgroups start from them
  DevBuf<WideGrp> d_wgrps;
  DevBuf<LcSlab> d_lcslabs;
  DevBuf<long long> d_rfvoff, d_gdesc;
  DevBuf<double> d_vscr;                      // V = Linv_pa K_pa,u of ONE such level (the largest): written by k_factor_lchain, read by k_factor_ref_finish
  DevBuf<double> d_lcrow;                     // per-row e^2 | log r of the lchain levels (2 n)
  DevBuf<double> d_s0;                        // Ri' Ri of the reference blocks on the generic phase-B path (theta-only, cached with the Gram parts)
  DevBuf<long long> d_s0off;                  // per block: offset into d_s0, -1 = none
  bool c_pending = false;                     // st_sample_w_loglik_begin: the sweep's failure word and log-density are on their way to pin->deferred
  int c_rc = 0; double c_ll = 0.0;            // ... or (multi-GPU / communicator attached) already here
  // multi-GPU sharding
  DevBuf<int> d_ownobs, d_owngrp, d_ownslow;  // this rank's observed blocks; the same set split: column groups of the fast levels / blocks of the others
  DevBuf<unsigned char> d_rowmask, d_blkmask; // 1 = this rank contributes the entry to a sum-with-zeros exchange
  DevBuf<double> d_comm;                      // 2*n_blocks + 64 doubles
  DevBuf<double> d_gather;                    // all-gather of w: world x gather_cnt (a rank's owned rows in device order + its failure word)
  DevBuf<int> d_gidx;                         // device row of every slot of d_gather (-1: padding / the failure word)
  DevBuf<double> d_gerr;                      // the ranks' failure words after the all-gather (64)
  // phase A of the latency-bound top levels ahead of time (st_factor_begin): they depend on theta only -- except for the
  // blocks' quadratic forms, redone with the current w afterwards -- and run on a second stream under the sweep
  hipStream_t stream2 = nullptr;
  hipEvent_t ev_top = nullptr, ev_main = nullptr;
  DevBuf<int> d_err2, d_toplist;
  bool async_top = false, top_pending = false, prof_suspend = false, async_top_off = false;
  hipEvent_t ev_stats = nullptr;
  bool stats_on_stream2 = false;   // the statistics kernels of the current (w, XB) are in flight on the second stream
  bool stats_prefetched = false;   // ... and their results follow them to pin->stats on that stream
  int top_phys = -1;
  std::vector<double> top_theta;
  bool ext_stream = false;
  // The running summaries (st_summary.hip), always present: the criteria over the rows read the stored draws and their epoch
  DevBuf<double> d_sum_w, d_sum_yhat;         // running sums over saved iterations (st_summary_*)
  long long n_summary = 0;
  DevBuf<double> d_draws_w, d_draws_yhat;     // st_summary_reserve: the saved draws themselves, [keep][n_all] (quantiles)
  long long draws_cap = 0, n_draws = 0;
  long long draws_epoch = 0;                  // advances whenever the stored draws of st_summary_reserve change
  bool stats_valid = false;                   // d_stats matches the current w and XB
  bool host_stats_valid = false;              // ... and host_stats holds a copy of it
  std::vector<double> host_stats;
  PinnedArea *pin = nullptr;                  // pinned host memory of the small device-to-host reads, one member per request (st_protocol.hpp)
  double *pin_up = nullptr;                   // pinned staging of the small per-iteration uploads (beta, tausq_inv): two slots taken in turn,
  int pin_up_slot = 0, pin_up_len = 0;        // so that the copy is truly asynchronous and the setters need no host synchronisation
  hipEvent_t ev_up[2] = {nullptr, nullptr};   // recorded behind a slot's copy: a slot is rewritten only after its last copy has run
  bool factor_open = false; int factor_open_slot = 0;   // st_factor_enqueue without its st_factor_finish yet
  std::vector<double> top_theta_open;                   // ... its theta where the work itself waits for st_factor_finish (communicator attached)
  hipEvent_t ev_factor = nullptr;                       // behind the copies of an enqueued factorisation's sums and failure word
  std::vector<char> s0_valid;                 // per level: d_s0 holds the theta-only precision parts of the accepted theta (column-group levels)
  bool gram_valid = false;                    // message Gram parts in `acc` match the accepted theta (slot 0)
  bool cache_gram = true;
  // a proposal's quad leaf levels (st_factor_enqueue on slot 1): QM_VONLY, their panels finished by QM_TFROMV from d_vleaf when
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
  DevBuf<int> d_twin;
  ncclComm_t comm = nullptr;                  // native RCCL communicator (st_comm_init); null = exchanges are the caller's
  std::vector<int> route_a, route_b;          // per level: ST_ROUTE_A_SLOTS phase-A / 2 phase-B route codes of the last launch
  int route_p = ST_ROUTE_NONE;                // ... and of the last st_predict
  std::vector<double> xtx;
  std::vector<long long> n_obs_q;
  // The state of a feature family is defined in the family's host unit and owned here; null: not set.  st_destroy drops each.
  struct PointSet *pts = nullptr;             // st_points.hip: new locations to predict at
  struct RowsScore *rows = nullptr;           // st_rows.hip: the criteria over the fit's own rows
  struct RowsLoo *loo = nullptr;              // st_rows.hip: the leave-one-out criteria and their Pareto store
  struct SimState *sim = nullptr;             // st_simulate.hip: the level plan and the draws' buffers

  DevBuf<double> d_cx, d_cy, d_y, d_X, d_w, d_xb, d_z, d_B, d_panels[2], d_acc, d_logdet[2], d_loglik[2], d_scalars, d_partial,
      d_stats, d_xtx, d_scratch, d_tmp_n, d_tsq;
  DevBuf<int> d_mv, d_anc, d_dch, d_lvl, d_pred, d_allobs, d_err;
  DevBuf<unsigned char> d_obs;
  DevBuf<long long> d_dev2model, d_partner;
  DevBuf<Blk> d_blks;
  int slot_map[2] = {0, 1};    // logical slot (0 param, 1 alter) -> physical arena
  double tausq_inv[QMAX];
  std::vector<double> theta[2];
  bool z_valid = false;

  // profiling
  int prof = 0;   // 0 off, 1 every kernel family, 2 phase A only (the roofline measurement at the lowest cost)
  double prof_ms[ST_N_KERNEL_FAMILIES] = {0};
  long long prof_n[ST_N_KERNEL_FAMILIES] = {0};
  std::vector<double> prof_level_ms;   // phase-A time per level, accumulated
  std::vector<long long> prof_level_n;
  struct ProfRec { hipEvent_t a, b; int fam, level, count; };   // count: kernel launches inside the bracket
  std::vector<ProfRec> prof_pending;
  std::vector<hipEvent_t> ev_free;
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
  if (!h->ev_free.empty()) { hipEvent_t e = h->ev_free.back(); h->ev_free.pop_back(); return e; }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}
inline void prof_harvest(st_handle_s *h) {
  for (auto &r : h->prof_pending) {
    float ms = 0.f;
    if (hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
      h->prof_ms[r.fam] += ms;
      h->prof_n[r.fam] += r.count;
      // (count 0: the deferred half of a level's launch -- its time, not another launch)
      if (r.level >= 0 && r.level < (int)h->prof_level_ms.size()) { h->prof_level_ms[r.level] += ms; h->prof_level_n[r.level] += r.count > 0; }
    }
    h->ev_free.push_back(r.a);
    h->ev_free.push_back(r.b);
  }
  h->prof_pending.clear();
}
struct ProfScope {
  st_handle_s *h;
  st_handle_s::ProfRec r;
  // mode 1: every launch is bracketed; mode 2: only the whole-phase bracket of phase A (level == -2), one pair of events
  hipStream_t st;
  ProfScope(st_handle_s *h_, int fam, int level = -1, int count = 1, hipStream_t st_ = nullptr) : h(h_), st(st_ ? st_ : h_->stream) {
    r.fam = fam; r.level = level; r.count = count; r.a = r.b = nullptr;
    const bool on = level == -2 ? (h->prof == 2 && !h->prof_suspend) : h->prof == 1;
    if (on) { r.a = prof_event(h); r.b = prof_event(h); (void)hipEventRecord(r.a, st); }
  }
  ~ProfScope() {
    if (r.a && r.b) {
      (void)hipEventRecord(r.b, st);
      h->prof_pending.push_back(r);
      if (h->prof_pending.size() > 8192) prof_harvest(h);
    }
  }
};

// A launcher's failure (the HIP error it returns as an int) as the entry point's: "<what> launch: <HIP's text>"
inline int launch_failed(st_handle_s *h, const std::string &what, int e) { h->err = what + " launch: " + hipGetErrorString((hipError_t)e); return ST_ERR_HIP; }

template <typename T>
inline hipError_t upload_or_dummy(DevBuf<T> &d, const std::vector<T> &v) {   // an empty list still gets one (zero) element to point at
  return v.empty() ? d.upload(std::vector<T>(1)) : d.upload(v);
}

// defined in spamtree_hip.hip
int make_covpar(st_handle h, const double *theta, int ntheta, CovPar *cp);
int download_rows(st_handle h, const double *src, double *dst);   // n_all doubles, device row order -> model row order
int refuse_factor_open(st_handle h, const char *who, int slot = -1);
int refuse_sweep_pending(st_handle h, const char *who);
int settle_top(st_handle h);
int complete_leaf(st_handle h, int slot);
int gen_or_upload_z(st_handle h, const double *z, uint64_t seed, uint32_t iter, unsigned stream_id, double *dst);
// each drops its unit's state of the handle (st_destroy, and the unit's own clear and set): st_points.hip, st_rows.hip, st_simulate.hip
void points_free(st_handle_s *h); void rows_free(st_handle_s *h); void loo_free(st_handle_s *h); void sim_free(st_handle_s *h);
