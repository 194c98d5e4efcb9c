// st_points.hip -- the C-ABI of new-point prediction (st_points_*): the device step of st_points_set / st_points_set_joint, predict,
// accumulate, the running summaries, the linear functionals of the predictions (st_points_functionals_*) and the scores of
// held-out observations (st_points_score_*) and the Rao-Blackwellised exceedance probabilities (st_points_exceed_*).  The summaries of the stored draws -- quantiles, diagnostics, excursions, rank
// diagnostics of the points and of the functionals -- are a resolver each (points_store, fun_store) and the store_* calls of
// draw_store.hpp, which the fit's rows go through too.
// predict_points.hpp, predict_joint.hpp, points_fun.hpp, points_score.hpp and points_exceed.hpp have the model; the launch structures of a point set and the term lists
// of its functionals are built without a device call in points_layout.cpp; the kernels and their launchers live in k_predict.hip,
// k_predict_joint.hip, k_points_acc.hip, k_points_fun.hip, k_points_score.hip and k_points_exceed.hip.
#include <memory>

#include "st_handle.hpp"
#include "misc_kernels.hpp"
#include "draw_store.hpp"
#include "points_layout.hpp"
#include "points_score.hpp"
#include "points_exceed.hpp"
#include "points_mixture.hpp"
#include "norm_quantile.hpp"

// The functionals of a point set (st_points_functionals_set): the term lists and chunks on the device, their accumulators, the
// values of the last iteration and, with a reservation, the draws F_w and F_y, [keep][n_fun] each
struct FunSet {
  long long n_fun = 0, nnz = 0, n_var_terms = 0, n_lin_chunks = 0, n_var_chunks = 0;
  double alg_bytes = 0.0;
  DevBuf<FunTerm> d_lin, d_var;
  DevBuf<FunChunk> d_lin_chunks, d_var_chunks;
  DevBuf<long long> d_lin_cptr, d_var_cptr;
  DevBuf<double> d_part, d_acc, d_last, d_keep_w, d_keep_yhat, d_q;
  long long n_acc = 0, n_kept = 0;
};

// The scores of held-out observations at the point set (st_points_score_set): y on the device, the running state of every point
// (SC_NACC x n) and joint group ([n_joint][2]), the counter of degenerate factorisations and room for the CRPS
struct ScoreSet {
  long long n_scored = 0, n_acc = 0;
  int gmax = 0;                    // the largest joint group
  std::vector<char> pt_obs, grp_obs;   // per point / joint group: scored (a group: any member observed)
  DevBuf<double> d_y, d_acc, d_jacc, d_crps;
  DevBuf<unsigned long long> d_ndeg;
};

// The thresholds of the Rao-Blackwellised exceedance probabilities (st_points_exceed_set): the values on the device, n_thr x q for
// the points and, with a functional part, n_thr x n_fun; the running state of every point ([targets][n_thr][2][n], targets = 2
// with X) and functional ([n_thr][2][n_fun])
struct ExceedSet {
  int n_thr = 0;
  unsigned side_neg = 0;           // bit t: s_t = -1
  bool fun = false;                // thr_fun given
  long long n_acc = 0;
  DevBuf<double> d_thr, d_acc, d_thr_fun, d_facc;
};

// The store of per-draw moments behind the mixture quantiles and the exact CRPS (st_points_mixture_reserve): [keep][n] columns of
// m, v and, with X, mu; tau2 [keep][q]; the functionals' F_m and F_v [keep][n_fun] with a count of their own (functionals set
// later start empty); the outputs' room on the device
struct MixSet {
  long long keep = 0, n_kept = 0, fn_kept = 0, n_fun = 0;
  long long passes = 0, solved = 0;   // of the last st_points_mixture_quantiles: evaluations of F, and series x probabilities
  DevBuf<double> d_m, d_v, d_mu, d_tau2, d_fm, d_fv, d_q, d_crps;
  DevBuf<long long> d_idx;
  DevBuf<unsigned long long> d_cnt;
};

struct PointSet : PointsCounts {
  long long n = 0;
  bool has_X = false;
  int route_mask = 0;
  DevBuf<double> d_px, d_py, d_X, d_z, d_out, d_scratch;
  DevBuf<int> d_pmv, d_chain_blk, d_pt_chain, d_gen;
  DevBuf<long long> d_order;
  DevBuf<PtChain> d_chains;
  DevBuf<PtTile> d_tiles;
  // st_points_accumulate: PA_NACC x n accumulators, and with st_points_summary_reserve the draws themselves, [keep][n] each
  DevBuf<double> d_acc, d_keep_w, d_keep_yhat;
  long long n_acc = 0, keep_cap = 0, n_kept = 0;
  // st_points_set_joint: the joint groups in layout order (first appearance), their packing into slots and the pair accumulators
  bool joint = false;
  std::vector<int64_t> j_off, j_mptr, j_mem;   // packed block offsets (n_joint + 1), member list pointers (n_joint + 1), members
  std::vector<int> pt_grp, pt_a;               // per point, caller order: its group and member index (functionals_layout reads them)
  DevBuf<PtJoint> d_jgroups;
  DevBuf<long long> d_jmem;
  DevBuf<PtCol> d_jcols;
  DevBuf<PtTile> d_jtiles;
  DevBuf<int> d_jgen, d_pt_grp, d_pt_a;
  DevBuf<double> d_jout, d_jscratch, d_pacc;   // cov and chol of the last call (2 x cov_total); scratch; pair accumulators
  std::unique_ptr<FunSet> fun;                 // st_points_functionals_set; leaves with the point set
  std::unique_ptr<ScoreSet> score;             // st_points_score_set; leaves with the point set
  std::unique_ptr<ExceedSet> exceed;           // st_points_exceed_set; leaves with the point set
  std::unique_ptr<MixSet> mix;                 // st_points_mixture_reserve; leaves with the point set
};

void points_free(st_handle_s *h) {
  delete h->pts;   // its device buffers free themselves
  h->pts = nullptr;
}

// ---- st_points_set, the device step ("st_points_set in two steps"): the layout's lists go to the device, its counts
// into the point set; of the lists only j_off, j_mptr and j_mem stay on the host
static int points_upload(st_handle h, PointSet *ps, const PointsLayout &L, const double *coords, const int64_t *mv, const double *X) {
  const long long n_new = ps->n;
  std::vector<double> px(coords, coords + n_new), py(coords + n_new, coords + 2 * n_new);
  std::vector<int> pmv(n_new);
  for (long long i = 0; i < n_new; ++i) pmv[i] = (int)(mv[i] - 1);
  HCHK(h, ps->d_px.upload(px)); HCHK(h, ps->d_py.upload(py)); HCHK(h, ps->d_pmv.upload(pmv));
  HCHK(h, ps->d_order.upload(L.order)); HCHK(h, ps->d_pt_chain.upload(L.pt_chain)); HCHK(h, ps->d_chains.upload(L.chains));
  HCHK(h, upload_or_dummy(ps->d_chain_blk, L.chain_blk)); HCHK(h, upload_or_dummy(ps->d_tiles, L.tiles)); HCHK(h, upload_or_dummy(ps->d_gen, L.gen));
  HCHK(h, ps->d_z.alloc(n_new));
  HCHK(h, ps->d_out.alloc((size_t)4 * n_new));
  if (ps->grid_generic > 0) HCHK(h, ps->d_scratch.alloc((size_t)ps->grid_generic * 2 * ps->scratch_stride));
  if (X) {
    std::vector<double> xv(X, X + (size_t)n_new * h->p);
    HCHK(h, ps->d_X.upload(xv));
    ps->has_X = true;
  }
  return ST_OK;
}

static int points_upload_joint(st_handle h, PointSet *ps, const PointsLayout &L) {
  std::vector<long long> jmem_ll(ps->j_mem.begin(), ps->j_mem.end());
  HCHK(h, ps->d_jgroups.upload(L.groups)); HCHK(h, ps->d_jmem.upload(jmem_ll)); HCHK(h, upload_or_dummy(ps->d_jtiles, L.jtiles));
  HCHK(h, ps->d_jcols.upload(L.jcols)); HCHK(h, upload_or_dummy(ps->d_jgen, L.jgen)); HCHK(h, ps->d_pt_grp.upload(L.pt_grp)); HCHK(h, ps->d_pt_a.upload(L.pt_a));
  HCHK(h, ps->d_jout.alloc((size_t)2 * ps->cov_total));
  if (ps->jgrid_generic > 0) HCHK(h, ps->d_jscratch.alloc((size_t)ps->jgrid_generic * PJ_SCRATCH_COLS * ps->scratch_stride));
  return ST_OK;
}

// st_points_set (joint_id NULL) and st_points_set_joint: a refusal of the layout leaves the previous point set in place, a
// failing HIP call none
static int points_set_impl(st_handle h, int64_t n_new, const double *coords, const int64_t *mv, const int64_t *anchor, const double *X,
                           const int64_t *joint_id) {
  if (!h) return ST_ERR_USAGE;
  PointsLayout L;
  if (const int rc = points_layout(*h, n_new, coords, mv, anchor, joint_id, L, h->err)) return rc;
  HCHK(h, hipSetDevice(h->device));
  points_free(h);
  std::unique_ptr<PointSet> ps(new PointSet());   // the handle takes it once every upload has succeeded
  static_cast<PointsCounts &>(*ps) = L;
  ps->n = n_new;
  ps->joint = joint_id != nullptr;
  ps->j_off = std::move(L.j_off); ps->j_mptr = std::move(L.j_mptr); ps->j_mem = std::move(L.j_mem);
  if (n_new > 0) {
    if (const int rc = points_upload(h, ps.get(), L, coords, mv, X)) return rc;
    if (joint_id)
      if (const int rc = points_upload_joint(h, ps.get(), L)) return rc;
  }
  ps->pt_grp = std::move(L.pt_grp); ps->pt_a = std::move(L.pt_a);
  h->pts = ps.release();
  return ST_OK;
}

extern "C" int st_points_set(st_handle h, int64_t n_new, const double *coords, const int64_t *mv, const int64_t *anchor, const double *X) {
  return points_set_impl(h, n_new, coords, mv, anchor, X, nullptr);
}

extern "C" int st_points_set_joint(st_handle h, int64_t n_new, const double *coords, const int64_t *mv, const int64_t *anchor, const double *X,
                                   const int64_t *joint_id) {
  return points_set_impl(h, n_new, coords, mv, anchor, X, joint_id);
}

extern "C" int st_points_joint_layout(st_handle h, int64_t *n_joint, int64_t *offsets, int64_t *member_ptr, int64_t *members) {
  if (!h) return ST_ERR_USAGE;
  const PointSet *ps = h->pts;
  if (!ps || !ps->joint) { h->err = "st_points_joint_layout before st_points_set_joint"; return ST_ERR_USAGE; }
  if (n_joint) *n_joint = ps->n_joint;
  if (offsets) std::copy(ps->j_off.begin(), ps->j_off.end(), offsets);
  if (member_ptr) std::copy(ps->j_mptr.begin(), ps->j_mptr.end(), member_ptr);
  if (members) std::copy(ps->j_mem.begin(), ps->j_mem.end(), members);
  return ST_OK;
}

// What every entry point that works on the point set refuses first.  need_factor: it reads slot 0; joint: the set must be one of
// st_points_set_joint
static int points_refuse(st_handle h, const char *who, bool need_factor = false, bool joint = false) {
  if (h->limited || h->world > 1) {
    h->err = std::string(who) + ": limited_tree and multi-GPU handles are not supported (out of scope)";
    return ST_ERR_UNSUPPORTED;
  }
  if (!h->pts || (joint && !h->pts->joint)) { h->err = std::string(who) + (joint ? " before st_points_set_joint" : " before st_points_set"); return ST_ERR_USAGE; }
  if (need_factor && h->theta[0].empty()) { h->err = std::string(who) + " before st_factor(slot 0)"; return ST_ERR_USAGE; }
  if (need_factor && h->factor_open) { h->err = std::string(who) + " between st_factor_enqueue and st_factor_finish"; return ST_ERR_USAGE; }
  return ST_OK;
}

// The outputs of the last launch to the caller: dst[k] from the k-th n doubles of d_out, the packed cov and chol from d_jout
// (any may be NULL); waits for the stream if it copied anything, or if `always`
static int points_copy_out(st_handle h, PointSet *ps, double *const dst[4], double *cond_cov, double *cond_chol, bool always) {
  const long long n = ps->n;
  bool copied = always;
  for (int k = 0; k < 4; ++k)
    if (dst[k]) { HCHK(h, hipMemcpyAsync(dst[k], ps->d_out.p + (size_t)k * n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream)); copied = true; }
  const size_t cb = (size_t)ps->cov_total * sizeof(double);
  if (cond_cov) { HCHK(h, hipMemcpyAsync(cond_cov, ps->d_jout.p, cb, hipMemcpyDeviceToHost, h->stream)); copied = true; }
  if (cond_chol) { HCHK(h, hipMemcpyAsync(cond_chol, ps->d_jout.p + ps->cov_total, cb, hipMemcpyDeviceToHost, h->stream)); copied = true; }
  if (copied) HCHK(h, hipStreamSynchronize(h->stream));
  return ST_OK;
}

// launches the k_points_* routes of the point set on slot 0 and the current w / beta / tausq_inv into ps->d_out (w, mean, var,
// yhat: n doubles each, caller order; out[k] false: that output is not written).  No synchronisation.
static void points_args(st_handle h, PointSet *ps, int mode, bool use_z, uint64_t seed, uint32_t iter, const bool out[4], PointsArgs &A) {
  const long long n = ps->n;
  double *o = ps->d_out.p;
  std::memset(&A, 0, sizeof(A));
  A.blks = h->d_blks.p; A.chain_blk = ps->d_chain_blk.p; A.chains = ps->d_chains.p; A.tiles = ps->d_tiles.p; A.ntiles = 0;
  A.gen_list = ps->d_gen.p; A.ngen = ps->grid_generic > 0 ? (int)(ps->d_gen.n) : 0;
  A.pt_chain = ps->d_pt_chain.p; A.order = ps->d_order.p; A.px = ps->d_px.p; A.py = ps->d_py.p; A.pmv = ps->d_pmv.p;
  A.cx = h->d_cx.p; A.cy = h->d_cy.p; A.mv = h->d_mv.p; A.w = h->d_w.p; A.panels = h->d_panels[h->slot_map[0]].p;
  A.z = use_z ? ps->d_z.p : nullptr; A.seed = seed; A.iter = iter; A.mode = mode;
  A.X = ps->has_X ? ps->d_X.p : nullptr; A.B = h->d_B.p; A.tsq_inv = h->d_tsq.p; A.p = h->p; A.n_new = n;
  A.w_new = out[0] ? o : nullptr; A.mean = out[1] ? o + n : nullptr; A.var = out[2] ? o + 2 * n : nullptr;
  A.yhat = out[3] ? o + 3 * n : nullptr;
  A.scratch = ps->d_scratch.p; A.scratch_stride = ps->scratch_stride;
}

static int points_run(st_handle h, PointSet *ps, int mode, bool use_z, uint64_t seed, uint32_t iter, const bool out[4], const char *who) {
  CovPar cp;
  int rc = make_covpar(h, h->theta[0].data(), (int)h->theta[0].size(), &cp);
  if (rc) return rc;
  PointsArgs A;
  points_args(h, ps, mode, use_z, seed, iter, out, A);
  PointsLaunch L;
  L.ntile128 = ps->ntile128; L.ntile256 = ps->ntile256; L.grid_generic = ps->grid_generic;
  ProfScope pscope(h, 6);
  if (const int e = points_launch(L, A, cp, h->stream, &ps->route_mask)) return launch_failed(h, who, e);
  return ST_OK;
}

extern "C" int st_points_predict(st_handle h, int mode, const double *z, uint64_t seed, uint32_t iter, double *w_new, double *cond_mean,
                                 double *cond_var, double *yhat_new) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = points_refuse(h, "st_points_predict", true)) return rc;
  if (mode != 0 && mode != 1) { h->err = "st_points_predict: mode must be 0 (draw) or 1 (conditional mean)"; return ST_ERR_USAGE; }
  PointSet *ps = h->pts;
  if (yhat_new && !ps->has_X) { h->err = "st_points_predict: yhat_new needs the regressors X of st_points_set"; return ST_ERR_USAGE; }
  ps->route_mask = 0;
  if (ps->n == 0) return ST_OK;
  HCHK(h, hipSetDevice(h->device));
  const long long n = ps->n;
  if (z && mode == 0) HCHK(h, hipMemcpyAsync(ps->d_z.p, z, (size_t)n * sizeof(double), hipMemcpyHostToDevice, h->stream));
  double *const dst[4] = {w_new, cond_mean, cond_var, yhat_new};
  const bool out[4] = {w_new != nullptr, cond_mean != nullptr, cond_var != nullptr, yhat_new != nullptr};
  const int rc = points_run(h, ps, mode, z && mode == 0, seed, iter, out, "st_points_predict");
  if (rc) return rc;
  return points_copy_out(h, ps, dst, nullptr, nullptr, true);
}

// the joint routes of the point set (st_points_set_joint) into ps->d_out as points_run, plus cov and chol into ps->d_jout
static int points_run_joint(st_handle h, PointSet *ps, int mode, bool use_z, uint64_t seed, uint32_t iter, const bool out[4], bool want_cov,
                            bool want_chol, const char *who) {
  CovPar cp;
  int rc = make_covpar(h, h->theta[0].data(), (int)h->theta[0].size(), &cp);
  if (rc) return rc;
  JointArgs J;
  std::memset(&J, 0, sizeof(J));
  points_args(h, ps, mode, use_z, seed, iter, out, J.P);
  J.P.tiles = ps->d_jtiles.p;
  J.P.scratch = ps->d_jscratch.p;
  J.groups = ps->d_jgroups.p; J.members = ps->d_jmem.p; J.cols = ps->d_jcols.p;
  J.gen_groups = ps->d_jgen.p; J.ngen_groups = ps->jgrid_generic > 0 ? (int)ps->d_jgen.n : 0;
  J.cov = want_cov ? ps->d_jout.p : nullptr; J.chol = want_chol ? ps->d_jout.p + ps->cov_total : nullptr;
  JointLaunch L;
  L.ntile128 = ps->jtile128; L.ntile256 = ps->jtile256; L.grid_generic = ps->jgrid_generic;
  ProfScope pscope(h, 6);
  if (const int e = points_joint_launch(L, J, cp, h->stream, &ps->route_mask)) return launch_failed(h, who, e);
  return ST_OK;
}

extern "C" int st_points_predict_joint(st_handle h, int mode, const double *z, uint64_t seed, uint32_t iter, double *w_new, double *cond_mean,
                                       double *cond_cov, double *cond_chol, double *yhat_new) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = points_refuse(h, "st_points_predict_joint", true, true)) return rc;
  if (mode != 0 && mode != 1) { h->err = "st_points_predict_joint: mode must be 0 (draw) or 1 (conditional mean)"; return ST_ERR_USAGE; }
  PointSet *ps = h->pts;
  if (yhat_new && !ps->has_X) { h->err = "st_points_predict_joint: yhat_new needs the regressors X of st_points_set_joint"; return ST_ERR_USAGE; }
  ps->route_mask = 0;
  if (ps->n == 0) return ST_OK;
  HCHK(h, hipSetDevice(h->device));
  const long long n = ps->n;
  if (z && mode == 0) HCHK(h, hipMemcpyAsync(ps->d_z.p, z, (size_t)n * sizeof(double), hipMemcpyHostToDevice, h->stream));
  const bool out[4] = {w_new != nullptr, cond_mean != nullptr, false, yhat_new != nullptr};
  const int rc = points_run_joint(h, ps, mode, z && mode == 0, seed, iter, out, cond_cov != nullptr, cond_chol != nullptr, "st_points_predict_joint");
  if (rc) return rc;
  double *const dst[4] = {w_new, cond_mean, nullptr, yhat_new};
  return points_copy_out(h, ps, dst, cond_cov, cond_chol, true);
}

extern "C" int st_points_info(st_handle h, int32_t *route, int64_t *n_groups, double *alg_bytes, double *flops) {
  if (!h) return ST_ERR_USAGE;
  const PointSet *ps = h->pts;
  const bool jr = ps && (ps->route_mask >> (PP_ROUTE_JOINT_MFMA128 - 1)) != 0;   // the last call took the joint routes
  if (route) *route = ps ? ps->route_mask : 0;
  if (n_groups) *n_groups = ps ? ps->n_chains : 0;
  if (alg_bytes) *alg_bytes = ps ? (jr ? ps->j_alg_bytes : ps->alg_bytes) : 0.0;
  if (flops) *flops = ps ? (jr ? ps->j_flops : ps->flops) : 0.0;
  return ST_OK;
}

extern "C" const char *st_points_route_name(int32_t code) {
  return code < PP_ROUTE_COUNT ? points_route_name(code) : points_joint_route_name(code);
}

// ---- the functionals' share of reset, reserve and accumulate (the entry points follow the summaries) ----
static int fun_reset(st_handle h, FunSet *fs) {
  HCHK(h, hipMemsetAsync(fs->d_acc.p, 0, (size_t)PA_NACC * fs->n_fun * sizeof(double), h->stream));
  fs->n_acc = 0; fs->n_kept = 0;
  return ST_OK;
}

// room for the functional draws of the point set's reservation (keep_cap)
static int fun_reserve(st_handle h, const PointSet *ps, FunSet *fs) {
  fs->d_keep_w.free(); fs->d_keep_yhat.free();
  fs->n_kept = 0;
  if (ps->keep_cap == 0) return ST_OK;
  HCHK(h, fs->d_keep_w.alloc((size_t)ps->keep_cap * fs->n_fun));
  if (ps->has_X) HCHK(h, fs->d_keep_yhat.alloc((size_t)ps->keep_cap * fs->n_fun));
  return ST_OK;
}

// the functional step of one saved iteration: after k_points_acc, on the same stream, from d_out / d_jout
static int fun_step(st_handle h, PointSet *ps) {
  FunSet *fs = ps->fun.get();
  const long long n = ps->n, nf = fs->n_fun;
  const double *o = ps->d_out.p;
  FunArgs A;
  A.lin = fs->d_lin.p; A.var = fs->d_var.p; A.lin_chunks = fs->d_lin_chunks.p; A.var_chunks = fs->d_var_chunks.p;
  A.lin_cptr = fs->d_lin_cptr.p; A.var_cptr = fs->d_var_cptr.p;
  A.n_lin_chunks = fs->n_lin_chunks; A.n_var_chunks = fs->n_var_chunks; A.n_fun = nf;
  A.w = o; A.mean = o + n; A.yhat = ps->has_X ? o + 3 * n : nullptr;
  A.vsrc = ps->joint ? ps->d_jout.p : o + 2 * n;
  A.part = fs->d_part.p; A.acc = fs->d_acc.p; A.last = fs->d_last.p;
  const bool keep = fs->n_kept < ps->keep_cap && fs->d_keep_w.p;
  A.keep_w = keep ? fs->d_keep_w.p + (size_t)fs->n_kept * nf : nullptr;
  A.keep_yhat = (keep && ps->has_X) ? fs->d_keep_yhat.p + (size_t)fs->n_kept * nf : nullptr;
  A.count = (double)(fs->n_acc + 1);
  {
    ProfScope pscope(h, 6);
    if (const int e = points_fun_launch(A, h->stream)) return launch_failed(h, "st_points_accumulate", e);
  }
  fs->n_acc += 1;
  if (keep) fs->n_kept += 1;
  return ST_OK;
}

// ---- the scores' share of reset and accumulate (the entry points follow the functionals) ----
static int score_reset(st_handle h, ScoreSet *sc) {
  if (sc->d_acc.p) HCHK(h, hipMemsetAsync(sc->d_acc.p, 0, sc->d_acc.n * sizeof(double), h->stream));
  if (sc->d_jacc.p) HCHK(h, hipMemsetAsync(sc->d_jacc.p, 0, sc->d_jacc.n * sizeof(double), h->stream));
  HCHK(h, hipMemsetAsync(sc->d_ndeg.p, 0, sizeof(unsigned long long), h->stream));
  sc->n_acc = 0;
  return ST_OK;
}

// the score step of one saved iteration: after k_points_acc, on the same stream, from d_out / d_jout, d_X, d_B and d_tsq
static int score_step(st_handle h, PointSet *ps) {
  ScoreSet *sc = ps->score.get();
  const long long n = ps->n;
  sc->n_acc += 1;
  if (n == 0 || sc->n_scored == 0) return ST_OK;
  const double *o = ps->d_out.p;
  ProfScope pscope(h, 6, -1, ps->joint ? 2 : 1);
  ScoreArgs A;
  A.y = sc->d_y.p; A.mean = o + n; A.var = o + 2 * n; A.X = ps->d_X.p; A.B = h->d_B.p; A.tsq_inv = h->d_tsq.p; A.pmv = ps->d_pmv.p;
  A.p = h->p; A.n = n; A.acc = sc->d_acc.p;
  int e = points_score_launch(A, h->stream);
  if (!e && ps->joint) {
    ScoreJointArgs J;
    J.y = A.y; J.mean = A.mean; J.cov = ps->d_jout.p; J.X = A.X; J.B = A.B; J.tsq_inv = A.tsq_inv; J.pmv = A.pmv; J.p = A.p; J.n = n;
    J.n_joint = ps->n_joint; J.groups = ps->d_jgroups.p; J.members = ps->d_jmem.p; J.jacc = sc->d_jacc.p; J.n_degenerate = sc->d_ndeg.p;
    e = points_score_joint_launch(J, sc->gmax, h->stream);
  }
  if (e) return launch_failed(h, "st_points_accumulate", e);
  return ST_OK;
}

// ---- the exceedance probabilities' share of reset and accumulate (the entry points follow the scores) ----
static int exceed_reset(st_handle h, ExceedSet *ex) {
  if (ex->d_acc.p) HCHK(h, hipMemsetAsync(ex->d_acc.p, 0, ex->d_acc.n * sizeof(double), h->stream));
  if (ex->d_facc.p) HCHK(h, hipMemsetAsync(ex->d_facc.p, 0, ex->d_facc.n * sizeof(double), h->stream));
  ex->n_acc = 0;
  return ST_OK;
}

// the exceedance step of one saved iteration: after fun_step, on the same stream, from d_out, d_X, d_B, d_tsq and the
// functionals' d_last.  An empty set counts the iteration and launches nothing.
static int exceed_step(st_handle h, PointSet *ps) {
  ExceedSet *ex = ps->exceed.get();
  const long long n = ps->n;
  ex->n_acc += 1;
  if (n == 0) return ST_OK;
  const double *o = ps->d_out.p;
  ProfScope pscope(h, 6);
  ExceedArgs A;
  A.mean = o + n; A.var = o + 2 * n; A.X = ps->has_X ? ps->d_X.p : nullptr; A.B = h->d_B.p; A.tsq_inv = h->d_tsq.p; A.pmv = ps->d_pmv.p;
  A.thr = ex->d_thr.p; A.side_neg = ex->side_neg; A.n_thr = ex->n_thr; A.p = h->p; A.q = h->q; A.n = n;
  A.count = (double)ex->n_acc; A.acc = ex->d_acc.p;
  int e = points_exceed_launch(A, h->stream);
  if (!e && ex->fun && ps->fun) {
    ExceedFunArgs F;
    F.last = ps->fun->d_last.p; F.thr = ex->d_thr_fun.p; F.side_neg = ex->side_neg; F.n_thr = ex->n_thr; F.n_fun = ps->fun->n_fun;
    F.count = A.count; F.acc = ex->d_facc.p;
    e = points_exceed_fun_launch(F, h->stream);
  }
  if (e) return launch_failed(h, "st_points_accumulate", e);
  return ST_OK;
}

// ---- the mixture store's share of reserve and accumulate (the entry points follow the exceedance probabilities) ----
// room for the functional columns of the store (none without functionals)
static int mix_reserve_fun(st_handle h, const PointSet *ps, MixSet *mx) {
  mx->d_fm.free(); mx->d_fv.free();
  mx->fn_kept = 0;
  mx->n_fun = (ps->fun && ps->n > 0) ? ps->fun->n_fun : 0;
  if (mx->n_fun == 0) return ST_OK;
  HCHK(h, mx->d_fm.alloc((size_t)mx->keep * mx->n_fun)); HCHK(h, mx->d_fv.alloc((size_t)mx->keep * mx->n_fun));
  return ST_OK;
}

// the store's step of one saved iteration: after exceed_step, on the same stream, from d_out, d_X, d_B, d_tsq and the functionals'
// d_last.  A full store and an empty set launch nothing.
static int mix_step(st_handle h, PointSet *ps) {
  MixSet *mx = ps->mix.get();
  const long long n = ps->n, c = mx->n_kept;
  if (c >= mx->keep) return ST_OK;
  mx->n_kept += 1;
  if (n == 0) return ST_OK;
  const double *o = ps->d_out.p;
  const bool fun = mx->n_fun > 0 && ps->fun && mx->fn_kept < mx->keep;
  MixStoreArgs A;
  A.mean = o + n; A.var = o + 2 * n; A.X = ps->has_X ? ps->d_X.p : nullptr; A.B = h->d_B.p; A.tsq_inv = h->d_tsq.p; A.pmv = ps->d_pmv.p;
  A.last = fun ? ps->fun->d_last.p : nullptr; A.p = h->p; A.q = h->q; A.n = n; A.n_fun = fun ? mx->n_fun : 0;
  A.m = mx->d_m.p + (size_t)c * n; A.v = mx->d_v.p + (size_t)c * n; A.mu = ps->has_X ? mx->d_mu.p + (size_t)c * n : nullptr;
  A.tau2 = mx->d_tau2.p + (size_t)c * h->q;
  A.fm = fun ? mx->d_fm.p + (size_t)mx->fn_kept * mx->n_fun : nullptr; A.fv = fun ? mx->d_fv.p + (size_t)mx->fn_kept * mx->n_fun : nullptr;
  ProfScope pscope(h, 6);
  if (const int e = points_mix_store_launch(A, h->stream)) return launch_failed(h, "st_points_accumulate", e);
  if (fun) mx->fn_kept += 1;
  return ST_OK;
}

// ---- predictive summaries of the point set over saved iterations (st_points_accumulate; the kernel lives in k_points_acc.hip) ----
extern "C" int st_points_summary_reset(st_handle h) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = points_refuse(h, "st_points_summary_reset")) return rc;
  PointSet *ps = h->pts;
  HCHK(h, hipSetDevice(h->device));
  const size_t cnt = (size_t)PA_NACC * ps->n;
  if (cnt > 0 && !ps->d_acc.p) HCHK(h, ps->d_acc.alloc(cnt));
  if (cnt > 0) HCHK(h, hipMemsetAsync(ps->d_acc.p, 0, cnt * sizeof(double), h->stream));
  const size_t pcnt = (size_t)2 * ps->cov_total;
  if (pcnt > 0 && !ps->d_pacc.p) HCHK(h, ps->d_pacc.alloc(pcnt));
  if (pcnt > 0) HCHK(h, hipMemsetAsync(ps->d_pacc.p, 0, pcnt * sizeof(double), h->stream));
  ps->n_acc = 0; ps->n_kept = 0;
  if (ps->score)
    if (const int rc = score_reset(h, ps->score.get())) return rc;
  if (ps->exceed)
    if (const int rc = exceed_reset(h, ps->exceed.get())) return rc;
  if (ps->mix) { ps->mix->n_kept = 0; ps->mix->fn_kept = 0; }
  if (ps->fun) return fun_reset(h, ps->fun.get());
  return ST_OK;
}

extern "C" int st_points_summary_reserve(st_handle h, int64_t keep) {
  if (!h || keep < 0) return ST_ERR_USAGE;
  if (const int rc = points_refuse(h, "st_points_summary_reserve")) return rc;
  if (keep > STORE_MAX_DRAWS) {
    h->err = "st_points_summary_reserve: at most " + std::to_string(STORE_MAX_DRAWS) + " saved draws (one point's draws are sorted in one workgroup's LDS)";
    return ST_ERR_UNSUPPORTED;
  }
  PointSet *ps = h->pts;
  HCHK(h, hipSetDevice(h->device));
  HCHK(h, hipStreamSynchronize(h->stream));
  ps->d_keep_w.free(); ps->d_keep_yhat.free();
  ps->keep_cap = 0; ps->n_kept = 0;
  if (ps->fun) { ps->fun->d_keep_w.free(); ps->fun->d_keep_yhat.free(); ps->fun->n_kept = 0; }
  if (keep == 0 || ps->n == 0) return ST_OK;
  HCHK(h, ps->d_keep_w.alloc((size_t)keep * ps->n));
  if (ps->has_X) HCHK(h, ps->d_keep_yhat.alloc((size_t)keep * ps->n));
  ps->keep_cap = keep;
  if (ps->fun) return fun_reserve(h, ps, ps->fun.get());
  return ST_OK;
}

// st_points_accumulate and st_points_accumulate_joint (cond_cov, cond_chol: a joint set's packed outputs, NULL otherwise)
static int points_accumulate(st_handle h, uint64_t seed, uint32_t iter, double *w_new, double *cond_mean, double *cond_var, double *yhat_new,
                             double *cond_cov, double *cond_chol) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = points_refuse(h, "st_points_accumulate", true)) return rc;
  PointSet *ps = h->pts;
  if (yhat_new && !ps->has_X) { h->err = "st_points_accumulate: yhat_new needs the regressors X of st_points_set"; return ST_ERR_USAGE; }
  if (!ps->d_acc.p && ps->n > 0) { const int rc0 = st_points_summary_reset(h); if (rc0) return rc0; }
  ps->route_mask = 0;
  if (ps->n == 0) {   // functionals of an empty set have no term: zeros
    ps->n_acc += 1;
    if (ps->score) (void)score_step(h, ps);   // counts the iteration; an empty set launches nothing
    if (ps->exceed) (void)exceed_step(h, ps); // likewise
    if (ps->mix) (void)mix_step(h, ps);       // likewise
    if (!ps->fun) return ST_OK;
    HCHK(h, hipSetDevice(h->device));
    return fun_step(h, ps);
  }
  HCHK(h, hipSetDevice(h->device));
  const long long n = ps->n;
  const bool out[4] = {true, true, true, ps->has_X};
  int rc = ps->joint ? points_run_joint(h, ps, 0, false, seed, iter, out, true, cond_chol != nullptr, "st_points_accumulate")
                     : points_run(h, ps, 0, false, seed, iter, out, "st_points_accumulate");
  if (rc) return rc;
  const double *o = ps->d_out.p;
  if (ps->joint) {   // the pair accumulators, before k_points_acc moves the Welford means
    PointsPairArgs B;
    B.mean = o + n; B.cov = ps->d_jout.p; B.acc = ps->d_acc.p; B.pacc = ps->d_pacc.p; B.groups = ps->d_jgroups.p; B.members = ps->d_jmem.p;
    B.pt_grp = ps->d_pt_grp.p; B.pt_a = ps->d_pt_a.p; B.count = (double)(ps->n_acc + 1); B.n = n; B.cov_total = ps->cov_total;
    ProfScope pscope(h, 6);
    if (const int e = points_pair_acc_launch(B, h->stream)) return launch_failed(h, "st_points_accumulate", e);
  }
  PointsAccArgs A;
  A.w = o; A.mean = o + n; A.var = o + 2 * n; A.yhat = ps->has_X ? o + 3 * n : nullptr;
  A.acc = ps->d_acc.p;
  const bool keep = ps->n_kept < ps->keep_cap;
  A.keep_w = keep ? ps->d_keep_w.p + (size_t)ps->n_kept * n : nullptr;
  A.keep_yhat = (keep && ps->has_X) ? ps->d_keep_yhat.p + (size_t)ps->n_kept * n : nullptr;
  A.count = (double)(ps->n_acc + 1);
  A.n = n;
  {
    ProfScope pscope(h, 6);
    if (const int e = points_acc_launch(A, h->stream)) return launch_failed(h, "st_points_accumulate", e);
  }
  ps->n_acc += 1;
  if (keep) ps->n_kept += 1;
  if (ps->score)
    if (const int rcs = score_step(h, ps)) return rcs;
  if (ps->fun)
    if (const int rcf = fun_step(h, ps)) return rcf;
  if (ps->exceed)
    if (const int rce = exceed_step(h, ps)) return rce;
  if (ps->mix)
    if (const int rcm = mix_step(h, ps)) return rcm;
  double *const dst[4] = {w_new, cond_mean, cond_var, yhat_new};
  return points_copy_out(h, ps, dst, cond_cov, cond_chol, false);
}

extern "C" int st_points_accumulate(st_handle h, uint64_t seed, uint32_t iter, double *w_new, double *cond_mean, double *cond_var,
                                    double *yhat_new) {
  return points_accumulate(h, seed, iter, w_new, cond_mean, cond_var, yhat_new, nullptr, nullptr);
}

extern "C" int st_points_accumulate_joint(st_handle h, uint64_t seed, uint32_t iter, double *w_new, double *cond_mean, double *cond_cov,
                                          double *cond_chol, double *yhat_new) {
  if (!h) return ST_ERR_USAGE;
  if (h->pts && !h->pts->joint) { h->err = "st_points_accumulate_joint before st_points_set_joint"; return ST_ERR_USAGE; }
  return points_accumulate(h, seed, iter, w_new, cond_mean, nullptr, yhat_new, cond_cov, cond_chol);
}

extern "C" int st_points_summary_get_cov(st_handle h, double *cov) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = points_refuse(h, "st_points_summary_get_cov")) return rc;
  PointSet *ps = h->pts;
  if (!ps->joint) { h->err = "st_points_summary_get_cov before st_points_set_joint"; return ST_ERR_USAGE; }
  if (ps->n_acc == 0) { h->err = "st_points_summary_get_cov: no iteration accumulated"; return ST_ERR_USAGE; }
  if (ps->cov_total == 0 || !cov) return ST_OK;
  HCHK(h, hipSetDevice(h->device));
  const long long tot = ps->cov_total;
  std::vector<double> acc((size_t)2 * tot);
  HCHK(h, hipMemcpyAsync(acc.data(), ps->d_pacc.p, acc.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HCHK(h, hipStreamSynchronize(h->stream));
  const double cnt = (double)ps->n_acc;
  for (long long k = 0; k < ps->n_joint; ++k) {
    const long long o = ps->j_off[k], g = ps->j_mptr[k + 1] - ps->j_mptr[k];
    for (long long a = 0; a < g; ++a)
      for (long long b = 0; b <= a; ++b) {
        const long long e = o + a + b * g;
        const double v = acc[e] / cnt + acc[tot + e] / cnt;   // mean conditional covariance + covariance of the conditional means
        cov[e] = v; cov[o + b + a * g] = v;
      }
  }
  return ST_OK;
}

// The Welford accumulators d_acc (PA_NACC x n) after `count` iterations, read out into the caller's arrays (any may be NULL)
static int pa_read_out(st_handle h, const double *d_acc, long long n, long long count, double *mean, double *var, double *w_mean, double *yhat_mean) {
  if (n == 0) return ST_OK;
  HCHK(h, hipSetDevice(h->device));
  std::vector<double> acc((size_t)PA_NACC * n);
  HCHK(h, hipMemcpyAsync(acc.data(), d_acc, acc.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HCHK(h, hipStreamSynchronize(h->stream));
  const double cnt = (double)count;
  const double *a = acc.data();
  for (long long i = 0; i < n; ++i) {
    if (mean) mean[i] = a[PA_MEAN * n + i];
    if (var) var[i] = a[PA_VAR * n + i] / cnt + a[PA_M2 * n + i] / cnt;   // mean conditional variance + variance of the conditional means
    if (w_mean) w_mean[i] = a[PA_W * n + i] / cnt;
    if (yhat_mean) yhat_mean[i] = a[PA_YHAT * n + i] / cnt;
  }
  return ST_OK;
}

extern "C" int st_points_summary_get(st_handle h, double *mean, double *var, double *w_mean, double *yhat_mean, int64_t *n_accumulated) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = points_refuse(h, "st_points_summary_get")) return rc;
  PointSet *ps = h->pts;
  if (n_accumulated) *n_accumulated = ps->n_acc;
  if (ps->n_acc == 0) { h->err = "st_points_summary_get: no iteration accumulated"; return ST_ERR_USAGE; }
  if (yhat_mean && !ps->has_X) { h->err = "st_points_summary_get: yhat_mean needs the regressors X of st_points_set"; return ST_ERR_USAGE; }
  return pa_read_out(h, ps->d_acc.p, ps->n, ps->n_acc, mean, var, w_mean, yhat_mean);
}

// ---- the summaries of stored draws (draw_store.hpp).  The point set as a store: caller order, the domains and thresholds go by
// outcome (d_pmv); d_out serves as the quantile's scratch, the next st_points_accumulate rewrites it anyway
static DrawStore points_store(st_handle h, const char *who) {
  DrawStore s;
  s.rc = h ? points_refuse(h, who) : ST_ERR_USAGE;
  if (s.rc) return s;
  const PointSet *ps = h->pts;
  s.w = ps->d_keep_w.p; s.yhat = ps->d_keep_yhat.p; s.n = ps->n; s.K = ps->n_kept;
  s.d_outcome = ps->d_pmv.p; s.G = h->q; s.d_scratch = ps->d_out.p;
  s.reserve = "st_points_summary_reserve"; s.yhat_needs_X = !ps->has_X;
  return s;
}
extern "C" int st_points_summary_quantile(st_handle h, double q, double *w_q, double *yhat_q) {
  return store_quantile(h, __func__, points_store(h, __func__), q, w_q, yhat_q);
}
extern "C" int st_points_summary_diagnostics(st_handle h, int32_t max_lag, const st_series_diag *w, const st_series_diag *yhat) {
  return store_diagnostics(h, __func__, points_store(h, __func__), max_lag, w, yhat);
}
extern "C" int st_points_summary_excursions(st_handle h, const st_excursion_spec *spec, const st_excursion_out *w, const st_excursion_out *yhat) {
  return store_excursions(h, __func__, points_store(h, __func__), spec, w, yhat);
}
extern "C" int st_points_summary_rank_diagnostics(st_handle h, const st_rank_spec *spec, const st_rank_out *w, const st_rank_out *yhat) {
  return store_rank_diagnostics(h, __func__, points_store(h, __func__), spec, w, yhat);
}
extern "C" int st_points_summary_chain_diagnostics(st_handle h, int32_t n_chains, int32_t max_lag, const st_series_diag *w,
                                                   const st_series_diag *yhat) {
  return store_chain_diagnostics(h, __func__, points_store(h, __func__), n_chains, max_lag, w, yhat);
}
extern "C" int st_points_summary_chain_rank_diagnostics(st_handle h, int32_t n_chains, const st_rank_spec *spec, const st_rank_out *w,
                                                        const st_rank_out *yhat) {
  return store_chain_rank_diagnostics(h, __func__, points_store(h, __func__), n_chains, spec, w, yhat);
}

// ---- linear functionals of the predictions (points_fun.hpp): the term lists come from functionals_layout, without a device call
extern "C" int st_points_functionals_set(st_handle h, int64_t n_fun, const int64_t *ptr, const int64_t *idx, const double *wt) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = points_refuse(h, "st_points_functionals_set")) return rc;
  PointSet *ps = h->pts;
  FunFacts F;
  F.n = ps->n; F.joint = ps->joint;
  F.j_off = ps->j_off.data(); F.j_mptr = ps->j_mptr.data(); F.pt_grp = ps->pt_grp.data(); F.pt_a = ps->pt_a.data();
  FunLayout L;
  if (const int rc = functionals_layout(F, n_fun, ptr, idx, wt, L, h->err)) return rc;   // the previous functionals stay
  HCHK(h, hipSetDevice(h->device));
  HCHK(h, hipStreamSynchronize(h->stream));
  if (ps->exceed) {   // thresholds per functional belong to the functionals they were given for
    ps->exceed->fun = false;
    ps->exceed->d_thr_fun.free(); ps->exceed->d_facc.free();
  }
  if (n_fun == 0) {
    ps->fun.reset();
    if (ps->mix) return mix_reserve_fun(h, ps, ps->mix.get());
    return ST_OK;
  }
  std::unique_ptr<FunSet> fs(new FunSet());   // the point set takes it once every upload has succeeded
  fs->n_fun = L.n_fun; fs->nnz = L.nnz; fs->n_var_terms = L.n_var_terms;
  fs->n_lin_chunks = (long long)L.lin_chunks.size(); fs->n_var_chunks = (long long)L.var_chunks.size();
  fs->alg_bytes = L.alg_bytes(ps->has_X);
  HCHK(h, upload_or_dummy(fs->d_lin, L.lin)); HCHK(h, upload_or_dummy(fs->d_var, L.var));
  HCHK(h, upload_or_dummy(fs->d_lin_chunks, L.lin_chunks)); HCHK(h, upload_or_dummy(fs->d_var_chunks, L.var_chunks));
  HCHK(h, fs->d_lin_cptr.upload(L.lin_cptr)); HCHK(h, fs->d_var_cptr.upload(L.var_cptr));
  HCHK(h, fs->d_part.alloc((size_t)4 * std::max<long long>(1, fs->n_lin_chunks + fs->n_var_chunks)));
  HCHK(h, fs->d_acc.alloc((size_t)PA_NACC * fs->n_fun)); HCHK(h, fs->d_last.alloc((size_t)4 * fs->n_fun)); HCHK(h, fs->d_q.alloc((size_t)fs->n_fun));
  if (const int rc = fun_reset(h, fs.get())) return rc;
  if (const int rc = fun_reserve(h, ps, fs.get())) return rc;
  ps->fun = std::move(fs);
  if (ps->mix) return mix_reserve_fun(h, ps, ps->mix.get());   // the store's functional columns belong to the functionals they were written for
  return ST_OK;
}

// what the functional outputs refuse first
static int fun_refuse(st_handle h, const char *who, bool need_acc) {
  if (const int rc = points_refuse(h, who)) return rc;
  if (!h->pts->fun) { h->err = std::string(who) + " before st_points_functionals_set"; return ST_ERR_USAGE; }
  if (need_acc && h->pts->fun->n_acc == 0) { h->err = std::string(who) + ": no iteration accumulated"; return ST_ERR_USAGE; }
  return ST_OK;
}

extern "C" int st_points_functionals_info(st_handle h, int64_t *n_fun, int64_t *nnz, int64_t *n_chunks, int64_t *n_var_terms, double *alg_bytes) {
  if (!h) return ST_ERR_USAGE;
  const FunSet *fs = h->pts ? h->pts->fun.get() : nullptr;
  if (n_fun) *n_fun = fs ? fs->n_fun : 0;
  if (nnz) *nnz = fs ? fs->nnz : 0;
  if (n_chunks) *n_chunks = fs ? fs->n_lin_chunks + fs->n_var_chunks : 0;
  if (n_var_terms) *n_var_terms = fs ? fs->n_var_terms : 0;
  if (alg_bytes) *alg_bytes = fs ? fs->alg_bytes : 0.0;
  return ST_OK;
}

extern "C" int st_points_functionals_last(st_handle h, double *f_w, double *f_cond_mean, double *f_cond_var, double *f_yhat) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = fun_refuse(h, "st_points_functionals_last", true)) return rc;
  const PointSet *ps = h->pts;
  FunSet *fs = ps->fun.get();
  if (f_yhat && !ps->has_X) { h->err = "st_points_functionals_last: f_yhat needs the regressors X of st_points_set"; return ST_ERR_USAGE; }
  HCHK(h, hipSetDevice(h->device));
  double *const dst[4] = {f_w, f_cond_mean, f_cond_var, f_yhat};
  for (int k = 0; k < 4; ++k)
    if (dst[k]) HCHK(h, hipMemcpyAsync(dst[k], fs->d_last.p + (size_t)k * fs->n_fun, (size_t)fs->n_fun * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HCHK(h, hipStreamSynchronize(h->stream));
  return ST_OK;
}

extern "C" int st_points_functionals_get(st_handle h, double *mean, double *var, double *w_mean, double *yhat_mean, int64_t *n_accumulated) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = fun_refuse(h, "st_points_functionals_get", false)) return rc;
  const PointSet *ps = h->pts;
  FunSet *fs = ps->fun.get();
  if (n_accumulated) *n_accumulated = fs->n_acc;
  if (fs->n_acc == 0) { h->err = "st_points_functionals_get: no iteration accumulated"; return ST_ERR_USAGE; }
  if (yhat_mean && !ps->has_X) { h->err = "st_points_functionals_get: yhat_mean needs the regressors X of st_points_set"; return ST_ERR_USAGE; }
  return pa_read_out(h, fs->d_acc.p, fs->n_fun, fs->n_acc, mean, var, w_mean, yhat_mean);
}

// The functionals as a store: caller order, one domain, a threshold value per functional.  The functionals of an empty point set
// store no draw: an empty store.
static DrawStore fun_store(st_handle h, const char *who) {
  DrawStore s;
  s.rc = h ? fun_refuse(h, who, false) : ST_ERR_USAGE;
  if (s.rc) return s;
  const PointSet *ps = h->pts;
  const FunSet *fs = ps->fun.get();
  s.w = fs->d_keep_w.p; s.yhat = fs->d_keep_yhat.p; s.n = ps->n == 0 ? 0 : fs->n_fun; s.K = fs->n_kept;
  s.thr_per_series = true; s.d_scratch = fs->d_q.p;
  s.reserve = "st_points_summary_reserve"; s.yhat_needs_X = !ps->has_X;
  return s;
}
extern "C" int st_points_functionals_quantile(st_handle h, double q, double *w_q, double *yhat_q) {
  return store_quantile(h, __func__, fun_store(h, __func__), q, w_q, yhat_q);
}
extern "C" int st_points_functionals_diagnostics(st_handle h, int32_t max_lag, const st_series_diag *w, const st_series_diag *yhat) {
  return store_diagnostics(h, __func__, fun_store(h, __func__), max_lag, w, yhat);
}
extern "C" int st_points_functionals_excursions(st_handle h, const st_excursion_spec *spec, const st_excursion_out *w, const st_excursion_out *yhat) {
  return store_excursions(h, __func__, fun_store(h, __func__), spec, w, yhat);
}
extern "C" int st_points_functionals_rank_diagnostics(st_handle h, const st_rank_spec *spec, const st_rank_out *w, const st_rank_out *yhat) {
  return store_rank_diagnostics(h, __func__, fun_store(h, __func__), spec, w, yhat);
}
extern "C" int st_points_functionals_chain_diagnostics(st_handle h, int32_t n_chains, int32_t max_lag, const st_series_diag *w,
                                                       const st_series_diag *yhat) {
  return store_chain_diagnostics(h, __func__, fun_store(h, __func__), n_chains, max_lag, w, yhat);
}
extern "C" int st_points_functionals_chain_rank_diagnostics(st_handle h, int32_t n_chains, const st_rank_spec *spec, const st_rank_out *w,
                                                            const st_rank_out *yhat) {
  return store_chain_rank_diagnostics(h, __func__, fun_store(h, __func__), n_chains, spec, w, yhat);
}

// ---- scores of held-out observations at the point set (points_score.hpp)
extern "C" int st_points_score_set(st_handle h, const double *y_new) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = points_refuse(h, "st_points_score_set")) return rc;
  PointSet *ps = h->pts;
  const long long n = ps->n;
  if (y_new) {   // a refusal leaves the previous scores in place
    if (!ps->has_X) { h->err = "st_points_score_set: the scores need the regressors X of st_points_set"; return ST_ERR_USAGE; }
    for (long long i = 0; i < n; ++i)
      if (std::isinf(y_new[i])) { h->err = "st_points_score_set: y_new[" + std::to_string(i) + "] is infinite (NaN marks a point that is not scored)"; return ST_ERR_USAGE; }
  }
  HCHK(h, hipSetDevice(h->device));
  HCHK(h, hipStreamSynchronize(h->stream));
  if (!y_new) { ps->score.reset(); return ST_OK; }
  std::unique_ptr<ScoreSet> sc(new ScoreSet());   // the point set takes it once every upload has succeeded
  sc->pt_obs.resize((size_t)n);
  for (long long i = 0; i < n; ++i) { sc->pt_obs[i] = !std::isnan(y_new[i]); sc->n_scored += sc->pt_obs[i]; }
  if (ps->joint) {
    sc->grp_obs.assign((size_t)ps->n_joint, 0);
    for (long long k = 0; k < ps->n_joint; ++k) {
      sc->gmax = std::max(sc->gmax, (int)(ps->j_mptr[k + 1] - ps->j_mptr[k]));
      for (int64_t a = ps->j_mptr[k]; a < ps->j_mptr[k + 1]; ++a) sc->grp_obs[k] |= sc->pt_obs[ps->j_mem[a]];
    }
  }
  HCHK(h, sc->d_y.upload(std::vector<double>(y_new, y_new + n)));
  HCHK(h, sc->d_acc.alloc((size_t)SC_NACC * n)); HCHK(h, sc->d_crps.alloc((size_t)n));
  if (ps->joint) HCHK(h, sc->d_jacc.alloc((size_t)2 * ps->n_joint));
  HCHK(h, sc->d_ndeg.alloc(1));
  if (const int rc = score_reset(h, sc.get())) return rc;
  ps->score = std::move(sc);
  return ST_OK;
}

extern "C" int st_points_score_get(st_handle h, double *lpd, double *pit, double *crps, double *lpd_joint, int64_t *n_scored,
                                   int64_t *n_degenerate) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = points_refuse(h, "st_points_score_get")) return rc;
  PointSet *ps = h->pts;
  ScoreSet *sc = ps->score.get();
  if (!sc) { h->err = "st_points_score_get before st_points_score_set"; return ST_ERR_USAGE; }
  if (n_scored) *n_scored = sc->n_scored;
  if (sc->n_scored == 0) { h->err = "st_points_score_get: no point is scored (every y_new is NaN)"; return ST_ERR_USAGE; }
  if (sc->n_acc == 0) { h->err = "st_points_score_get: no iteration accumulated"; return ST_ERR_USAGE; }
  if (crps && ps->n_kept == 0) { h->err = "st_points_score_get: crps needs a stored draw (call st_points_summary_reserve before the saved iterations)"; return ST_ERR_USAGE; }
  if (lpd_joint && !ps->joint) { h->err = "st_points_score_get: lpd_joint before st_points_set_joint"; return ST_ERR_USAGE; }
  HCHK(h, hipSetDevice(h->device));
  const long long n = ps->n;
  const double S = (double)sc->n_acc, nan = std::nan("");
  std::vector<double> acc, jacc;
  unsigned long long ndeg = 0;
  if (lpd || pit) {
    acc.resize((size_t)SC_NACC * n);
    HCHK(h, hipMemcpyAsync(acc.data(), sc->d_acc.p, acc.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  }
  if (lpd_joint) {
    jacc.resize((size_t)2 * ps->n_joint);
    HCHK(h, hipMemcpyAsync(jacc.data(), sc->d_jacc.p, jacc.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  }
  if (n_degenerate) HCHK(h, hipMemcpyAsync(&ndeg, sc->d_ndeg.p, sizeof(ndeg), hipMemcpyDeviceToHost, h->stream));
  if (crps) {
    ScoreCrpsArgs A;
    A.draws = ps->d_keep_yhat.p; A.y = sc->d_y.p; A.n = n; A.keep = (int)ps->n_kept;
    qtile_plan(ps->n_kept, &A.Kpad, &A.R);
    A.out = sc->d_crps.p;
    if (const int e = points_score_crps_launch(A, h->lds_limit, h->stream)) return launch_failed(h, "st_points_score_get", e);
    HCHK(h, hipMemcpyAsync(crps, sc->d_crps.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  }
  HCHK(h, hipStreamSynchronize(h->stream));
  // lpd = M + log(A / S); no draw of positive density: log 0
  auto lme = [&](double M, double A) { return A > 0.0 ? M + std::log(A / S) : -HUGE_VAL; };
  for (long long i = 0; i < n && (lpd || pit); ++i) {
    if (lpd) lpd[i] = sc->pt_obs[i] ? lme(acc[SC_M * n + i], acc[SC_A * n + i]) : nan;
    if (pit) pit[i] = sc->pt_obs[i] ? acc[SC_PIT * n + i] / S : nan;
  }
  for (long long k = 0; lpd_joint && k < ps->n_joint; ++k) lpd_joint[k] = sc->grp_obs[k] ? lme(jacc[2 * k], jacc[2 * k + 1]) : nan;
  if (n_degenerate) *n_degenerate = (int64_t)ndeg;
  return ST_OK;
}

// ---- Rao-Blackwellised exceedance probabilities at the point set (points_exceed.hpp)
extern "C" int st_points_exceed_set(st_handle h, int32_t n_thr, const double *thr, const int32_t *side, const double *thr_fun) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = points_refuse(h, "st_points_exceed_set")) return rc;
  PointSet *ps = h->pts;
  const bool remove = n_thr == 0 || !thr;
  const long long nf = ps->fun ? ps->fun->n_fun : 0;
  if (!remove)   // a refusal leaves the previous thresholds in place
    if (const int rc = check_exceed_spec("st_points_exceed_set: ", n_thr, thr, side, thr_fun, h->q, ps->fun ? nf : -1, h->err)) return rc;
  HCHK(h, hipSetDevice(h->device));
  HCHK(h, hipStreamSynchronize(h->stream));
  if (remove) { ps->exceed.reset(); return ST_OK; }
  std::unique_ptr<ExceedSet> ex(new ExceedSet());   // the point set takes it once every upload has succeeded
  ex->n_thr = n_thr;
  for (int t = 0; side && t < n_thr; ++t) ex->side_neg |= (side[t] < 0 ? 1u : 0u) << t;
  ex->fun = thr_fun != nullptr;
  HCHK(h, ex->d_thr.upload(std::vector<double>(thr, thr + (size_t)n_thr * h->q)));
  HCHK(h, ex->d_acc.alloc((size_t)(ps->has_X ? 2 : 1) * n_thr * 2 * ps->n));
  if (thr_fun) {
    HCHK(h, ex->d_thr_fun.upload(std::vector<double>(thr_fun, thr_fun + (size_t)n_thr * nf)));
    HCHK(h, ex->d_facc.alloc((size_t)n_thr * 2 * nf));
  }
  if (const int rc = exceed_reset(h, ex.get())) return rc;
  ps->exceed = std::move(ex);
  return ST_OK;
}

// prob and prob_var of one target from its [n_thr][2][m] state after S draws (either output may be NULL)
static void exceed_read_out(const double *acc, int n_thr, long long m, double S, const st_rb_out *out) {
  for (int t = 0; t < n_thr; ++t)
    for (long long i = 0; i < m; ++i) {
      if (out->prob) out->prob[(size_t)t * m + i] = acc[((size_t)t * 2 + EX_MEAN) * m + i];
      if (out->prob_var) out->prob_var[(size_t)t * m + i] = acc[((size_t)t * 2 + EX_M2) * m + i] / S;
    }
}

extern "C" int st_points_exceed_get(st_handle h, const st_rb_out *w, const st_rb_out *yhat, const st_rb_out *fun_w, int64_t *n_accumulated) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = points_refuse(h, "st_points_exceed_get")) return rc;
  PointSet *ps = h->pts;
  ExceedSet *ex = ps->exceed.get();
  if (!ex) { h->err = "st_points_exceed_get before st_points_exceed_set"; return ST_ERR_USAGE; }
  if (n_accumulated) *n_accumulated = ex->n_acc;
  if (ex->n_acc == 0) { h->err = "st_points_exceed_get: no iteration accumulated"; return ST_ERR_USAGE; }
  if (yhat && !ps->has_X) { h->err = "st_points_exceed_get: the yhat target needs the regressors X of st_points_set"; return ST_ERR_USAGE; }
  if (fun_w && !(ex->fun && ps->fun)) { h->err = "st_points_exceed_get: fun_w without functional thresholds (thr_fun of st_points_exceed_set)"; return ST_ERR_USAGE; }
  const long long n = ps->n;
  if (n == 0) return ST_OK;   // nothing to write: the functionals of an empty set have no term either
  HCHK(h, hipSetDevice(h->device));
  const int T = ex->n_thr;
  const double S = (double)ex->n_acc;
  const size_t per = (size_t)T * 2 * n;
  std::vector<double> acc, facc;
  const bool want_w = any_out(w), want_y = any_out(yhat), want_f = any_out(fun_w);
  if (want_w || want_y) {
    acc.resize(ex->d_acc.n);
    HCHK(h, hipMemcpyAsync(acc.data(), ex->d_acc.p, acc.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  }
  if (want_f) {
    facc.resize(ex->d_facc.n);
    HCHK(h, hipMemcpyAsync(facc.data(), ex->d_facc.p, facc.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  }
  HCHK(h, hipStreamSynchronize(h->stream));
  if (want_w) exceed_read_out(acc.data(), T, n, S, w);
  if (want_y) exceed_read_out(acc.data() + per, T, n, S, yhat);
  if (want_f) exceed_read_out(facc.data(), T, ps->fun->n_fun, S, fun_w);
  return ST_OK;
}

// ---- quantiles and the exact CRPS of the mixture predictive at the point set (points_mixture.hpp)
extern "C" int st_points_mixture_reserve(st_handle h, int64_t keep) {
  if (!h || keep < 0) return ST_ERR_USAGE;
  if (const int rc = points_refuse(h, "st_points_mixture_reserve")) return rc;
  if (keep > ST_MIX_MAX_DRAWS) {
    h->err = "st_points_mixture_reserve: keep = " + std::to_string(keep) + " beyond ST_MIX_MAX_DRAWS = " + std::to_string(ST_MIX_MAX_DRAWS) +
             " (one series' components are staged in one workgroup's LDS)";
    return ST_ERR_UNSUPPORTED;
  }
  PointSet *ps = h->pts;
  HCHK(h, hipSetDevice(h->device));
  HCHK(h, hipStreamSynchronize(h->stream));
  ps->mix.reset();
  if (keep == 0) return ST_OK;
  std::unique_ptr<MixSet> mx(new MixSet());   // the point set takes it once every allocation has succeeded
  mx->keep = keep;
  const size_t n = (size_t)ps->n;
  if (n > 0) {
    HCHK(h, mx->d_m.alloc((size_t)keep * n)); HCHK(h, mx->d_v.alloc((size_t)keep * n));
    if (ps->has_X) HCHK(h, mx->d_mu.alloc((size_t)keep * n));
    HCHK(h, mx->d_tau2.alloc((size_t)keep * h->q));
    HCHK(h, mx->d_cnt.alloc(3));
    if (const int rc = mix_reserve_fun(h, ps, mx.get())) return rc;
  }
  ps->mix = std::move(mx);
  return ST_OK;
}

// what the store's outputs refuse first
static int mix_refuse(st_handle h, const char *who) {
  if (const int rc = points_refuse(h, who)) return rc;
  if (!h->pts->mix) { h->err = std::string(who) + " before st_points_mixture_reserve"; return ST_ERR_USAGE; }
  return ST_OK;
}

extern "C" int st_points_mixture_draws(st_handle h, double *m, double *v, double *mu, double *tau2, int64_t *n_stored) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = mix_refuse(h, "st_points_mixture_draws")) return rc;
  PointSet *ps = h->pts;
  MixSet *mx = ps->mix.get();
  if (n_stored) *n_stored = mx->n_kept;
  if (mu && !ps->has_X) { h->err = "st_points_mixture_draws: mu needs the regressors X of st_points_set"; return ST_ERR_USAGE; }
  if (ps->n == 0 || mx->n_kept == 0) return ST_OK;
  HCHK(h, hipSetDevice(h->device));
  const size_t cb = (size_t)mx->n_kept * ps->n * sizeof(double);
  if (m) HCHK(h, hipMemcpyAsync(m, mx->d_m.p, cb, hipMemcpyDeviceToHost, h->stream));
  if (v) HCHK(h, hipMemcpyAsync(v, mx->d_v.p, cb, hipMemcpyDeviceToHost, h->stream));
  if (mu) HCHK(h, hipMemcpyAsync(mu, mx->d_mu.p, cb, hipMemcpyDeviceToHost, h->stream));
  if (tau2) HCHK(h, hipMemcpyAsync(tau2, mx->d_tau2.p, (size_t)mx->n_kept * h->q * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HCHK(h, hipStreamSynchronize(h->stream));
  return ST_OK;
}

// one target's quantiles: the launch over its n series of K components, the copies and the wait
static int mix_quantile_target(st_handle h, MixSet *mx, MixQuantileArgs &A, const st_mix_out *out) {
  MixPlan P;
  if (!mix_quantile_plan(A.K, A.n, h->lds_limit, &P)) {
    h->err = "st_points_mixture_quantiles: " + std::to_string(A.K) + " components do not fit the device's LDS";
    return ST_ERR_UNSUPPORTED;
  }
  const size_t cnt = (size_t)A.T * A.n;
  if (mx->d_q.n < cnt) { mx->d_q.free(); HCHK(h, mx->d_q.alloc(cnt)); }
  A.R = P.R; A.out = mx->d_q.p; A.counters = mx->d_cnt.p;
  HCHK(h, hipMemsetAsync(mx->d_cnt.p, 0, 2 * sizeof(unsigned long long), h->stream));
  if (const int e = points_mix_quantile_launch(A, P, h->lds_limit, h->stream)) return launch_failed(h, "st_points_mixture_quantiles", e);
  unsigned long long unc[2] = {0, 0};
  if (out->q) HCHK(h, hipMemcpyAsync(out->q, mx->d_q.p, cnt * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HCHK(h, hipMemcpyAsync(unc, mx->d_cnt.p, sizeof(unc), hipMemcpyDeviceToHost, h->stream));
  HCHK(h, hipStreamSynchronize(h->stream));
  if (out->n_unconverged) *out->n_unconverged = (int64_t)unc[MIX_CNT_UNCONVERGED];
  mx->passes += (long long)unc[MIX_CNT_PASSES]; mx->solved += (long long)cnt;
  return ST_OK;
}

extern "C" int st_points_mixture_quantiles(st_handle h, int32_t n_probs, const double *probs, const st_mix_out *w, const st_mix_out *yhat,
                                           const st_mix_out *fun_w) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = mix_refuse(h, "st_points_mixture_quantiles")) return rc;
  PointSet *ps = h->pts;
  MixSet *mx = ps->mix.get();
  if (const int rc = check_mixture_probs("st_points_mixture_quantiles: ", n_probs, probs, h->err)) return rc;
  if (yhat && !ps->has_X) { h->err = "st_points_mixture_quantiles: the yhat target needs the regressors X of st_points_set"; return ST_ERR_USAGE; }
  if (fun_w && !ps->fun) { h->err = "st_points_mixture_quantiles: fun_w before st_points_functionals_set"; return ST_ERR_USAGE; }
  if (mx->n_kept == 0 || (fun_w && ps->n > 0 && mx->fn_kept == 0)) { h->err = "st_points_mixture_quantiles: no stored draw"; return ST_ERR_USAGE; }
  mx->passes = 0; mx->solved = 0;
  if (ps->n == 0) return ST_OK;   // nothing to write: the functionals of an empty set have no term either
  HCHK(h, hipSetDevice(h->device));
  MixQuantileArgs A;
  std::memset(&A, 0, sizeof(A));
  A.T = n_probs; A.q = h->q;
  std::vector<int> ord(n_probs);
  for (int t = 0; t < n_probs; ++t) ord[t] = t;
  std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return probs[a] < probs[b]; });
  for (int t = 0; t < n_probs; ++t) { A.p[t] = probs[ord[t]]; A.z[t] = st_norm_quantile_f(A.p[t]); A.slot[t] = ord[t]; }
  if (any_out(w)) {
    A.m = mx->d_m.p; A.v = mx->d_v.p; A.tau2 = nullptr; A.pmv = nullptr; A.K = (int)mx->n_kept; A.n = ps->n;
    if (const int rc = mix_quantile_target(h, mx, A, w)) return rc;
  }
  if (any_out(yhat)) {
    A.m = mx->d_mu.p; A.v = mx->d_v.p; A.tau2 = mx->d_tau2.p; A.pmv = ps->d_pmv.p; A.K = (int)mx->n_kept; A.n = ps->n;
    if (const int rc = mix_quantile_target(h, mx, A, yhat)) return rc;
  }
  if (any_out(fun_w)) {
    A.m = mx->d_fm.p; A.v = mx->d_fv.p; A.tau2 = nullptr; A.pmv = nullptr; A.K = (int)mx->fn_kept; A.n = mx->n_fun;
    if (const int rc = mix_quantile_target(h, mx, A, fun_w)) return rc;
  }
  return ST_OK;
}

extern "C" int st_points_mixture_info(st_handle h, int64_t *keep, int64_t *n_stored, double *store_bytes, int64_t *n_solved, int64_t *n_passes) {
  if (!h) return ST_ERR_USAGE;
  const PointSet *ps = h->pts;
  const MixSet *mx = ps ? ps->mix.get() : nullptr;
  if (keep) *keep = mx ? mx->keep : 0;
  if (n_stored) *n_stored = mx ? mx->n_kept : 0;
  if (store_bytes) *store_bytes = mx ? (double)mx->keep * mix_store_bytes(ps->n, ps->has_X, h->q, mx->n_fun) : 0.0;
  if (n_solved) *n_solved = mx ? mx->solved : 0;
  if (n_passes) *n_passes = mx ? mx->passes : 0;
  return ST_OK;
}

extern "C" int st_points_mixture_crps(st_handle h, double *crps, double *spread, int64_t *n_scored) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = mix_refuse(h, "st_points_mixture_crps")) return rc;
  PointSet *ps = h->pts;
  MixSet *mx = ps->mix.get();
  ScoreSet *sc = ps->score.get();
  if (!sc) { h->err = "st_points_mixture_crps before st_points_score_set"; return ST_ERR_USAGE; }
  if (n_scored) *n_scored = sc->n_scored;
  if (ps->n == 0) return ST_OK;
  if (sc->n_scored == 0) { h->err = "st_points_mixture_crps: no point is scored (every y_new is NaN)"; return ST_ERR_USAGE; }
  if (mx->n_kept == 0) { h->err = "st_points_mixture_crps: no stored draw"; return ST_ERR_USAGE; }
  if (!crps && !spread) return ST_OK;
  HCHK(h, hipSetDevice(h->device));
  const long long n = ps->n;
  MixPlan P;
  if (!mix_crps_plan(mx->n_kept, sc->n_scored, h->lds_limit, &P)) {
    h->err = "st_points_mixture_crps: " + std::to_string(mx->n_kept) + " components do not fit the device's LDS";
    return ST_ERR_UNSUPPORTED;
  }
  std::vector<long long> idx;
  idx.reserve((size_t)sc->n_scored);
  for (long long i = 0; i < n; ++i)
    if (sc->pt_obs[i]) idx.push_back(i);
  HCHK(h, hipStreamSynchronize(h->stream));   // a previous call's kernel may still read d_idx
  HCHK(h, mx->d_idx.upload(idx));
  if (!mx->d_crps.p) HCHK(h, mx->d_crps.alloc((size_t)2 * n));
  MixCrpsArgs A;
  A.mu = mx->d_mu.p; A.v = mx->d_v.p; A.tau2 = mx->d_tau2.p; A.y = sc->d_y.p; A.pmv = ps->d_pmv.p; A.idx = mx->d_idx.p;
  A.n = n; A.n_scored = sc->n_scored; A.q = h->q; A.K = (int)mx->n_kept; A.R = P.R; A.G = P.G;
  A.crps = mx->d_crps.p; A.spread = mx->d_crps.p + n;
  {
    ProfScope pscope(h, 6);
    if (const int e = points_mix_crps_launch(A, P, h->lds_limit, h->stream)) return launch_failed(h, "st_points_mixture_crps", e);
  }
  std::vector<double> out((size_t)2 * n);
  HCHK(h, hipMemcpyAsync(out.data(), mx->d_crps.p, out.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HCHK(h, hipStreamSynchronize(h->stream));
  const double nan = std::nan("");
  for (long long i = 0; i < n; ++i) {
    if (crps) crps[i] = sc->pt_obs[i] ? out[i] : nan;
    if (spread) spread[i] = sc->pt_obs[i] ? out[n + i] : nan;
  }
  return ST_OK;
}
