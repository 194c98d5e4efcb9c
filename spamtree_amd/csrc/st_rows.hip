// st_rows.hip -- the C-ABI of the criteria over the fit's own rows: WAIC, DIC and the held-out scores (st_rows_score_*), the
// leave-one-out criteria (st_rows_loo_*) and the Pareto smoothing of their stored ratios (st_rows_loo_reserve / _draws / _psis*,
// st_psis*).  The kernels and their launchers live in k_rows_score.hip, k_rows_loo.hip and k_psis.hip; loo_layout.cpp builds the
// leave-one-out launch structures.  The state is a RowsScore and a RowsLoo that the handle points to (st_handle.hpp): set = the
// pointer is there.  Of the summaries' state the CRPS reads the stored draws of st_summary_reserve and their epoch.
#include <memory>

#include "st_handle.hpp"
#include "misc_kernels.hpp"
#include "draw_store.hpp"
#include "rows_score.hpp"
#include "loo_layout.hpp"
#include "loo_kernels.hpp"
#include "psis_kernels.hpp"
#include "lgo_layout.hpp"
#include "lgo_kernels.hpp"

struct RowsScore {   // st_rows_score_set; device row order throughout
  DevBuf<double> d_tgt, d_hold;               // the targets; the same with NaN off the held-out rows (k_score_crps's y)
  DevBuf<double> d_acc, d_rows, d_crps, d_partial, d_tot;
  long long n_acc = 0, n_tgt = 0, n_held = 0;
  std::vector<long long> nheld_q;
  long long crps_epoch = -1;                  // d_crps holds the CRPS of the stored draws of that epoch (-1: none)
  long long fin_acc = -1, fin_crps = -2;      // d_rows / d_tot are those of fin_acc draws, with the CRPS of that epoch summed (-1: without)
  double tau2_sum[ST_MAX_Q] = {0};            // sum over the accumulated draws of 1 / tausq_inv_j, added in call order
};

// st_rows_loo_reserve: the accumulated draws' (t, Phi, mu), [3][keep][n_all] in device row order, and st_rows_loo_psis' outputs
// of fin_acc draws (PSIS_NOUT x n doubles; tail_len, n_draws; q x PSIS_NSUM totals)
struct PsisStore {
  DevBuf<double> d_store, d_rows, d_tot;
  DevBuf<int> d_int;
  long long keep = 0, fin_acc = -1;
};

// st_rows_loo_groups_set: the groups' index structures (lgo_layout.hpp), the sweep's vectors with their pair part, the groups'
// state and the last draw's matrices
struct LooGroups {
  LgoLayout lay;
  DevBuf<int> d_prptr, d_pra, d_prb, d_prfin, d_grpptr, d_gpptr, d_gpidx, d_sqptr, d_memgrp;
  DevBuf<long long> d_voff, d_memrow;
  DevBuf<double> d_S, d_pairval, d_lastq, d_lastv, d_lastc, d_lastm, d_gacc, d_macc, d_gout, d_rows, d_tot;
  std::vector<int> sq_ptr;
  long long fin_acc = -1;                     // d_gout / d_rows / d_tot are those of fin_acc draws
  // with a store reserved (st_rows_loo_reserve, before or after the groups): the draws' group log ratios [keep][n_groups] and
  // st_rows_loo_groups_psis' outputs of psis_acc draws (PSIS_NOUT x n_groups doubles; tail_len, n_draws)
  DevBuf<double> d_store, d_prow;
  DevBuf<int> d_pint;
  long long keep = 0, psis_acc = -1;
};

struct RowsLoo {   // st_rows_loo_set; device row order throughout
  std::unique_ptr<LooGroups> grp;             // leaves with the state, or with st_rows_loo_groups_clear
  DevBuf<int> d_list, d_chptr, d_chidx;
  DevBuf<long long> d_voff;
  DevBuf<double> d_S, d_last, d_acc, d_rows, d_tot;
  std::vector<LooLevelLaunch> levels;
  long long arena = 0;                        // doubles of d_S; while groups are set their own arena (with the pair parts) stands in and d_S is released
  double bytes = 0, flops = 0;
  int mask = 0;
  long long n_acc = 0, fin_acc = -1;          // d_rows / d_tot are those of fin_acc draws
  std::unique_ptr<PsisStore> psis;            // leaves with the state, or with st_rows_loo_reserve(0)
  long long keep() const { return psis ? psis->keep : 0; }
};

void rows_free(st_handle_s *h) { delete h->rows; h->rows = nullptr; }   // the device buffers free themselves
void loo_free(st_handle_s *h) { delete h->loo; h->loo = nullptr; }

// `count` planes of n_all rows each, `stride` apart on the device: the k-th into dst[k] + at in model row order, a NULL one skipped
static int download_planes(st_handle h, const double *src, size_t stride, int count, double *const *dst, size_t at = 0) {
  for (int k = 0; k < count; ++k)
    if (dst[k])
      if (const int rc = download_rows(h, src + k * stride, dst[k] + at)) return rc;
  return ST_OK;
}
// `count` doubles (totals: q x their number) to the host, complete on return
static int download_host(st_handle h, const double *src, size_t count, std::vector<double> &t) {
  t.resize(count);
  HCHK(h, hipMemcpyAsync(t.data(), src, count * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HCHK(h, hipStreamSynchronize(h->stream));
  return ST_OK;
}

// ---- criteria over the fit's own rows (rows_score.hpp; the kernels and their launchers live in k_rows_score.hip) ----
static int rows_refuse(st_handle h, const char *who, bool need_set = true, bool need_draw = false) {
  if (h->world > 1) { h->err = std::string(who) + ": multi-GPU handles are not supported"; return ST_ERR_UNSUPPORTED; }
  if (need_set && !h->rows) { h->err = std::string(who) + " before st_rows_score_set"; return ST_ERR_USAGE; }
  if (need_draw && h->rows->n_acc == 0) { h->err = std::string(who) + ": no iteration accumulated"; return ST_ERR_USAGE; }
  return ST_OK;
}
extern "C" int st_rows_score_set(st_handle h, const double *y_holdout) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = rows_refuse(h, "st_rows_score_set", false)) return rc;
  HCHK(h, hipSetDevice(h->device));
  const long long n = h->n_all;
  std::vector<double> y(n), tgt(n), hold(n);
  std::vector<unsigned char> obs(n);
  std::vector<int> mv(n);
  HCHK(h, hipMemcpyAsync(y.data(), h->d_y.p, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HCHK(h, hipMemcpyAsync(obs.data(), h->d_obs.p, n * sizeof(unsigned char), hipMemcpyDeviceToHost, h->stream));
  HCHK(h, hipMemcpyAsync(mv.data(), h->d_mv.p, n * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HCHK(h, hipStreamSynchronize(h->stream));
  // a refusal leaves the previous state in place: every check comes before the first change
  for (long long r = 0; y_holdout && r < n; ++r) {
    const double v = y_holdout[r];
    if (std::isinf(v)) { h->err = "st_rows_score_set: y_holdout[" + std::to_string(r) + "] is infinite (NaN marks a row without a held-out value)"; return ST_ERR_USAGE; }
    if (!std::isnan(v) && obs[h->model2dev[r]]) { h->err = "st_rows_score_set: y_holdout[" + std::to_string(r) + "] is finite at an observed row (held-out values belong to NA rows)"; return ST_ERR_USAGE; }
  }
  std::unique_ptr<RowsScore> rs(new RowsScore());   // the handle takes it once every allocation has succeeded
  rs->nheld_q.assign(h->q, 0);                      // (the observed rows per outcome are the handle's n_obs_q)
  const double nan = std::nan("");
  for (long long i = 0; i < n; ++i) {
    const double v = y_holdout ? y_holdout[h->dev2model[i]] : nan;
    hold[i] = obs[i] ? nan : v;
    tgt[i] = obs[i] ? y[i] : v;
    if (!obs[i] && !std::isnan(v)) { rs->nheld_q[mv[i]]++; ++rs->n_held; }
    rs->n_tgt += !std::isnan(tgt[i]);
  }
  HCHK(h, rs->d_tgt.upload(tgt)); HCHK(h, rs->d_hold.upload(hold));
  HCHK(h, rs->d_acc.alloc((size_t)RS_NACC * n)); HCHK(h, rs->d_rows.alloc((size_t)RS_NOUT * n)); HCHK(h, rs->d_crps.alloc((size_t)n));
  HCHK(h, rs->d_partial.alloc((size_t)STATS_WG * h->q * RS_NSUM)); HCHK(h, rs->d_tot.alloc((size_t)h->q * RS_NSUM));
  HCHK(h, hipMemsetAsync(rs->d_acc.p, 0, (size_t)RS_NACC * n * sizeof(double), h->stream));
  HCHK(h, hipStreamSynchronize(h->stream));
  rows_free(h);
  h->rows = rs.release();
  return ST_OK;
}
extern "C" int st_rows_score_clear(st_handle h) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = rows_refuse(h, "st_rows_score_clear", false)) return rc;
  HCHK(h, hipSetDevice(h->device));
  HCHK(h, hipStreamSynchronize(h->stream));
  rows_free(h);
  return ST_OK;
}
extern "C" int st_rows_score_accumulate(st_handle h) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = rows_refuse(h, "st_rows_score_accumulate")) return rc;
  HCHK(h, hipSetDevice(h->device));
  RowsScore &R = *h->rows;
  RowsScoreArgs A;
  A.tgt = R.d_tgt.p; A.obs = h->d_obs.p; A.xb = h->d_xb.p; A.w = h->d_w.p; A.tsq_inv = h->d_tsq.p; A.mv = h->d_mv.p;
  A.n = h->n_all; A.S = (double)(R.n_acc + 1); A.acc = R.d_acc.p;
  if (const int e = rows_score_launch(A, h->stream)) return launch_failed(h, "st_rows_score_accumulate", e);
  for (int j = 0; j < h->q; ++j) R.tau2_sum[j] += 1.0 / h->tausq_inv[j];
  R.n_acc += 1;
  return ST_OK;
}
// The per-row outputs and the sums, enqueued on the handle's stream; with need_crps (and draws stored, and a held-out row) first
// the CRPS of the held-out rows.  Each is computed once per state: the CRPS per epoch of the stored draws, the outputs and sums per
// (draws accumulated, CRPS summed), so st_rows_score_get followed by st_rows_score_totals sorts the draws once.
static int rows_finish(st_handle h, bool need_crps, bool *have_crps) {
  RowsScore &R = *h->rows;
  const bool can = h->n_draws > 0 && R.n_held > 0;
  if (need_crps && can && R.crps_epoch != h->draws_epoch) {
    ScoreCrpsArgs C;
    C.draws = h->d_draws_yhat.p; C.y = R.d_hold.p; C.n = h->n_all; C.keep = (int)h->n_draws;
    qtile_plan(h->n_draws, &C.Kpad, &C.R);
    C.out = R.d_crps.p;
    if (const int e = points_score_crps_launch(C, h->lds_limit, h->stream)) return launch_failed(h, "st_rows_score crps", e);
    R.crps_epoch = h->draws_epoch;
  }
  *have_crps = can && R.crps_epoch == h->draws_epoch;
  const long long with = *have_crps ? h->draws_epoch : -1;
  if (R.fin_acc == R.n_acc && R.fin_crps == with) return ST_OK;
  RowsTotalsArgs T;
  T.tgt = R.d_tgt.p; T.obs = h->d_obs.p; T.mv = h->d_mv.p; T.acc = R.d_acc.p; T.crps = *have_crps ? R.d_crps.p : nullptr;
  T.n = h->n_all; T.S = (double)R.n_acc; T.rows = R.d_rows.p; T.partial = R.d_partial.p;
  for (int j = 0; j < QMAX; ++j) T.tau2bar[j] = j < h->q ? R.tau2_sum[j] / (double)R.n_acc : 1.0;
  if (const int e = rows_score_totals_launch(T, h->q, R.d_tot.p, h->stream)) return launch_failed(h, "st_rows_score totals", e);
  R.fin_acc = R.n_acc; R.fin_crps = with;
  return ST_OK;
}
extern "C" int st_rows_score_get(st_handle h, double *lppd, double *p_waic, double *mean_ll, double *mu_mean, double *pit, double *crps,
                                 int64_t *n_accumulated) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = rows_refuse(h, "st_rows_score_get")) return rc;
  if (n_accumulated) *n_accumulated = h->rows->n_acc;
  if (const int rc = rows_refuse(h, "st_rows_score_get", true, true)) return rc;
  if (crps && h->n_draws == 0) { h->err = "st_rows_score_get: crps needs a stored draw (st_summary_reserve before the st_summary_accumulate calls)"; return ST_ERR_USAGE; }
  HCHK(h, hipSetDevice(h->device));
  bool have_crps = false;
  if (const int rc = rows_finish(h, crps != nullptr, &have_crps)) return rc;
  double *const dst[RS_NOUT] = {lppd, mean_ll, p_waic, mu_mean, pit};   // RS_OUT_* order
  if (const int rc = download_planes(h, h->rows->d_rows.p, h->n_all, RS_NOUT, dst)) return rc;
  if (crps) {
    if (have_crps) { if (const int rc = download_rows(h, h->rows->d_crps.p, crps)) return rc; }
    else for (long long i = 0; i < h->n_all; ++i) crps[i] = std::nan("");   // (no held-out row)
  }
  return ST_OK;
}
extern "C" int st_rows_score_totals(st_handle h, double *obs, double *held, int64_t *n_obs, int64_t *n_held) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = rows_refuse(h, "st_rows_score_totals", true, true)) return rc;
  HCHK(h, hipSetDevice(h->device));
  bool have_crps = false;
  if (const int rc = rows_finish(h, held != nullptr, &have_crps)) return rc;
  std::vector<double> t;
  if (const int rc = download_host(h, h->rows->d_tot.p, (size_t)h->q * RS_NSUM, t)) return rc;
  for (int j = 0; j < h->q; ++j) {
    const double *s = t.data() + (size_t)j * RS_NSUM;
    if (n_obs) n_obs[j] = h->n_obs_q[j];
    if (n_held) n_held[j] = h->rows->nheld_q[j];
    if (obs) {
      double *o = obs + (size_t)j * ST_ROWS_OBS_N;
      o[ST_ROWS_OBS_LPPD] = s[RS_SUM_O_LPPD];
      o[ST_ROWS_OBS_P_WAIC] = s[RS_SUM_O_PWAIC];
      o[ST_ROWS_OBS_WAIC] = -2.0 * (o[ST_ROWS_OBS_LPPD] - o[ST_ROWS_OBS_P_WAIC]);
      o[ST_ROWS_OBS_DBAR] = -2.0 * s[RS_SUM_O_MEANLL];
      o[ST_ROWS_OBS_DHAT] = -2.0 * s[RS_SUM_O_LOGN];
      o[ST_ROWS_OBS_P_D] = o[ST_ROWS_OBS_DBAR] - o[ST_ROWS_OBS_DHAT];
      o[ST_ROWS_OBS_DIC] = o[ST_ROWS_OBS_DBAR] + o[ST_ROWS_OBS_P_D];
      if (h->n_obs_q[j] == 0) for (int k = 0; k < ST_ROWS_OBS_N; ++k) o[k] = 0.0;   // (not -0)
    }
    if (held) {
      double *o = held + (size_t)j * ST_ROWS_HELD_N;
      o[ST_ROWS_HELD_LPPD] = s[RS_SUM_H_LPPD];
      o[ST_ROWS_HELD_PIT] = s[RS_SUM_H_PIT];
      o[ST_ROWS_HELD_CRPS] = s[RS_SUM_H_CRPS];
      o[ST_ROWS_HELD_SQERR] = s[RS_SUM_H_SQERR];
    }
  }
  return ST_OK;
}
// from shapes: every row reads its target; a targeted row also obs, mv, xb, w (21 B) and reads and writes five doubles of
// state, a held-out row six
extern "C" int st_rows_score_info(st_handle h, double *alg_bytes) {
  if (!h || !alg_bytes) return ST_ERR_USAGE;
  *alg_bytes = h->rows ? 8.0 * (double)h->n_all + (21.0 + 80.0) * (double)h->rows->n_tgt + 16.0 * (double)h->rows->n_held : 0.0;
  return ST_OK;
}

// ---- leave-one-out criteria with w_i integrated out (loo_kernels.hpp; the kernels and their launchers live in k_rows_loo.hip) ----
static int loo_refuse(st_handle h, const char *who, bool need_set = true, bool need_draw = false) {
  if (h->limited) { h->err = std::string(who) + ": limited_tree handles are not supported"; return ST_ERR_UNSUPPORTED; }
  if (h->world > 1) { h->err = std::string(who) + ": multi-GPU handles are not supported"; return ST_ERR_UNSUPPORTED; }
  if (need_set && !h->loo) { h->err = std::string(who) + " before st_rows_loo_set"; return ST_ERR_USAGE; }
  if (need_draw && h->loo->n_acc == 0) { h->err = std::string(who) + ": no iteration accumulated"; return ST_ERR_USAGE; }
  return ST_OK;
}
extern "C" int st_rows_loo_set(st_handle h) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = loo_refuse(h, "st_rows_loo_set", false)) return rc;
  LooLayout lay;
  std::string msg;
  if (const int rc = loo_layout(*h, lay, msg)) { h->err = "st_rows_loo_set: " + msg; return rc; }
  HCHK(h, hipSetDevice(h->device));
  const long long n = h->n_all;
  std::unique_ptr<RowsLoo> lo(new RowsLoo());   // the handle takes it once every allocation has succeeded
  HCHK(h, upload_or_dummy(lo->d_list, lay.list)); HCHK(h, lo->d_chptr.upload(lay.ch_ptr)); HCHK(h, upload_or_dummy(lo->d_chidx, lay.ch_idx));
  HCHK(h, lo->d_voff.upload(lay.voff));
  HCHK(h, lo->d_S.alloc((size_t)std::max(lay.arena, 1ll)));
  HCHK(h, lo->d_last.upload(std::vector<double>((size_t)LOO_NLAST * n, std::nan(""))));
  HCHK(h, lo->d_acc.alloc((size_t)LOO_NACC * n)); HCHK(h, lo->d_rows.alloc((size_t)LOO_NOUT * n)); HCHK(h, lo->d_tot.alloc((size_t)h->q * LOO_NSUM));
  HCHK(h, hipMemsetAsync(lo->d_acc.p, 0, (size_t)LOO_NACC * n * sizeof(double), h->stream));
  HCHK(h, hipStreamSynchronize(h->stream));
  for (const LooLevel &V : lay.levels) {
    lo->levels.push_back(LooLevelLaunch{V.first, V.count, V.isref, V.maxLen, V.maxM});
    lo->mask |= 1 << ((V.isref ? LOO_ROUTE_REF : LOO_ROUTE_LEAF) - 1);
  }
  lo->bytes = lay.alg_bytes; lo->flops = lay.flops; lo->arena = std::max(lay.arena, 1ll);
  loo_free(h);
  h->loo = lo.release();
  return ST_OK;
}
extern "C" int st_rows_loo_clear(st_handle h) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = loo_refuse(h, "st_rows_loo_clear")) return rc;
  HCHK(h, hipSetDevice(h->device));
  HCHK(h, hipStreamSynchronize(h->stream));
  loo_free(h);
  return ST_OK;
}
extern "C" int st_rows_loo_accumulate(st_handle h) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = loo_refuse(h, "st_rows_loo_accumulate")) return rc;
  if (const int rc = refuse_factor_open(h, "st_rows_loo_accumulate", 0)) return rc;
  if (const int rc = refuse_sweep_pending(h, "st_rows_loo_accumulate")) return rc;
  if (h->theta[0].empty()) { h->err = "st_rows_loo_accumulate before st_factor(slot 0)"; return ST_ERR_USAGE; }
  RowsLoo &L = *h->loo;
  for (const LooLevelLaunch &V : L.levels)
    if (LOO_LDS(V.maxLen, V.maxM) > h->lds_limit) { h->err = "st_rows_loo_accumulate: a chain too long for the kernel's LDS"; return ST_ERR_UNSUPPORTED; }
  if (const int rc = psis_check_column("st_rows_loo_accumulate", L.n_acc, L.keep(), h->err)) return rc;
  HCHK(h, hipSetDevice(h->device));
  if (const int rc = settle_top(h)) return rc;
  if (const int rc = complete_leaf(h, 0)) return rc;
  LooArgs A;
  std::memset(&A, 0, sizeof(A));
  A.blks = h->d_blks.p; A.anc_idx = h->d_anc.p; A.list = L.d_list.p;
  A.panels = h->d_panels[h->slot_map[0]].p;
  A.w = h->d_w.p; A.xb = h->d_xb.p; A.y = h->d_y.p; A.tsq_inv = h->d_tsq.p; A.obs = h->d_obs.p; A.mv = h->d_mv.p;
  A.voff = L.d_voff.p; A.ch_ptr = L.d_chptr.p; A.ch_idx = L.d_chidx.p;
  A.S = L.d_S.p; A.last = L.d_last.p; A.acc = L.d_acc.p; A.n = h->n_all;
  if (L.grp) {   // the vectors with their pair part
    LooGroups &G = *L.grp;
    A.voff = G.d_voff.p; A.S = G.d_S.p;
    A.pr_ptr = G.d_prptr.p; A.pr_a = G.d_pra.p; A.pr_b = G.d_prb.p; A.pr_fin = G.d_prfin.p; A.pairval = G.d_pairval.p;
  }
  if (L.keep()) {   // this draw's column of the store
    const size_t plane = (size_t)L.keep() * h->n_all, col = (size_t)L.n_acc * h->n_all;
    A.st_t = L.psis->d_store.p + col; A.st_phi = L.psis->d_store.p + plane + col; A.st_mu = L.psis->d_store.p + 2 * plane + col;
  }
  int mask = 0;
  if (const int e = loo_launch(L.levels.data(), (int)L.levels.size(), A, h->stream, &mask)) return launch_failed(h, "st_rows_loo_accumulate", e);
  if (L.grp) {   // after the root level's launch: d, c and every pair are there
    LooGroups &G = *L.grp;
    LgoArgs B;
    std::memset(&B, 0, sizeof(B));
    B.G = (int)G.lay.n_groups; B.n = h->n_all;
    B.grp_ptr = G.d_grpptr.p; B.mem_row = G.d_memrow.p; B.gp_ptr = G.d_gpptr.p; B.gp_idx = G.d_gpidx.p; B.sq_ptr = G.d_sqptr.p;
    B.pairval = G.d_pairval.p; B.last = L.d_last.p;
    B.w = h->d_w.p; B.xb = h->d_xb.p; B.y = h->d_y.p; B.tsq_inv = h->d_tsq.p; B.obs = h->d_obs.p; B.mv = h->d_mv.p;
    B.last_q = G.d_lastq.p; B.last_v = G.d_lastv.p; B.last_c = G.d_lastc.p; B.last_m = G.d_lastm.p;
    B.gacc = G.d_gacc.p; B.macc = G.d_macc.p;
    if (G.keep) B.st_t = G.d_store.p + (size_t)L.n_acc * G.lay.n_groups;
    if (const int e = lgo_groups_launch(B, h->stream)) return launch_failed(h, "st_rows_loo_accumulate groups", e);
  }
  L.n_acc += 1;
  return ST_OK;
}
extern "C" int st_rows_loo_last(st_handle h, double *q_diag, double *qw, double *cond_mean, double *cond_var) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = loo_refuse(h, "st_rows_loo_last", true, true)) return rc;
  HCHK(h, hipSetDevice(h->device));
  double *const dst[LOO_NLAST] = {q_diag, qw, cond_mean, cond_var};   // LOO_LAST_* order
  return download_planes(h, h->loo->d_last.p, h->n_all, LOO_NLAST, dst);
}
// the per-row outputs and the totals, once per number of accumulated draws
static int loo_finish(st_handle h) {
  RowsLoo &L = *h->loo;
  if (L.fin_acc == L.n_acc) return ST_OK;
  LooFinishArgs F;
  F.y = h->d_y.p; F.obs = h->d_obs.p; F.mv = h->d_mv.p; F.acc = L.d_acc.p; F.n = h->n_all; F.S = (double)L.n_acc; F.q = h->q;
  F.rows = L.d_rows.p; F.tot = L.d_tot.p;
  if (const int e = loo_finish_launch(F, h->stream)) return launch_failed(h, "st_rows_loo finish", e);
  L.fin_acc = L.n_acc;
  return ST_OK;
}
extern "C" int st_rows_loo_get(st_handle h, double *elpd_loo, double *pit_loo, double *mu_loo, double *weight_ess, int64_t *n_accumulated,
                               int64_t *n_skipped) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = loo_refuse(h, "st_rows_loo_get")) return rc;
  if (n_accumulated) *n_accumulated = h->loo->n_acc;
  if (const int rc = loo_refuse(h, "st_rows_loo_get", true, true)) return rc;
  HCHK(h, hipSetDevice(h->device));
  if (const int rc = loo_finish(h)) return rc;
  double *const dst[LOO_NOUT] = {elpd_loo, pit_loo, mu_loo, weight_ess};   // LOO_OUT_* order
  if (const int rc = download_planes(h, h->loo->d_rows.p, h->n_all, LOO_NOUT, dst)) return rc;
  if (n_skipped) {
    std::vector<double> ns;
    if (const int rc = download_host(h, h->loo->d_acc.p + (size_t)LOO_NS * h->n_all, h->n_all, ns)) return rc;
    long long tot = 0;
    for (double v : ns) tot += (long long)v;
    *n_skipped = tot;
  }
  return ST_OK;
}
extern "C" int st_rows_loo_totals(st_handle h, double *tot, int64_t *n_obs) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = loo_refuse(h, "st_rows_loo_totals", true, true)) return rc;
  HCHK(h, hipSetDevice(h->device));
  if (const int rc = loo_finish(h)) return rc;
  std::vector<double> t;
  if (const int rc = download_host(h, h->loo->d_tot.p, (size_t)h->q * LOO_NSUM, t)) return rc;
  for (int j = 0; j < h->q; ++j) {
    const double *s = t.data() + (size_t)j * LOO_NSUM;
    if (n_obs) n_obs[j] = h->n_obs_q[j];
    if (!tot) continue;
    double *o = tot + (size_t)j * ST_ROWS_LOO_N;
    o[ST_ROWS_LOO_ELPD] = s[LOO_SUM_ELPD];
    o[ST_ROWS_LOO_LOOIC] = -2.0 * s[LOO_SUM_ELPD];
    o[ST_ROWS_LOO_SQERR] = s[LOO_SUM_SQERR];
    o[ST_ROWS_LOO_PIT] = s[LOO_SUM_PIT];
    o[ST_ROWS_LOO_MIN_ESS] = s[LOO_MIN_ESS];
    o[ST_ROWS_LOO_COUNT] = (double)h->n_obs_q[j];
    if (h->n_obs_q[j] == 0) { o[ST_ROWS_LOO_ELPD] = o[ST_ROWS_LOO_LOOIC] = 0.0; o[ST_ROWS_LOO_MIN_ESS] = std::nan(""); }
  }
  return ST_OK;
}
extern "C" int st_rows_loo_info(st_handle h, int32_t *route_mask, double *alg_bytes, double *flops) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = loo_refuse(h, "st_rows_loo_info")) return rc;
  if (route_mask) *route_mask = h->loo->mask;
  if (alg_bytes) *alg_bytes = h->loo->bytes + (h->loo->grp ? h->loo->grp->lay.alg_bytes : 0.0);
  if (flops) *flops = h->loo->flops + (h->loo->grp ? h->loo->grp->lay.flops : 0.0);
  return ST_OK;
}
extern "C" const char *st_rows_loo_route_name(int32_t code) { return loo_route_name(code); }

// ---- leave-group-out criteria (lgo_kernels.hpp; the kernels and their launchers live in k_rows_loo.hip and k_rows_lgo.hip) ----
// the groups' store of `keep` draws (0: none), NaN until written; a failed allocation is refused with its size
static int lgo_store(st_handle h, const char *who, LooGroups &G, long long keep) {
  DevBuf<double> store, prow;   // the groups keep what they have until every allocation has succeeded
  DevBuf<int> pint;
  if (keep > 0) {
    const size_t ng = (size_t)std::max(G.lay.n_groups, 1ll), cnt = (size_t)keep * ng;
    if (store.alloc(cnt) != hipSuccess || prow.alloc((size_t)PSIS_NOUT * ng) != hipSuccess || pint.alloc(2 * ng) != hipSuccess) {
      (void)hipGetLastError();
      h->err = std::string(who) + ": the store of " + std::to_string(keep) + " draws x " + std::to_string(G.lay.n_groups) + " groups could not be allocated";
      return ST_ERR_HIP;
    }
    HCHK(h, hipMemsetAsync(store.p, 0xff, cnt * sizeof(double), h->stream));   // all bits set: a NaN
    HCHK(h, hipStreamSynchronize(h->stream));
  }
  G.d_store = std::move(store); G.d_prow = std::move(prow); G.d_pint = std::move(pint);
  G.keep = keep; G.psis_acc = -1;
  return ST_OK;
}
static int lgo_refuse(st_handle h, const char *who, bool need_draw = false) {
  if (const int rc = loo_refuse(h, who)) return rc;
  if (!h->loo->grp) { h->err = std::string(who) + " before st_rows_loo_groups_set"; return ST_ERR_USAGE; }
  return loo_refuse(h, who, true, need_draw);
}
extern "C" int st_rows_loo_groups_set(st_handle h, const int64_t *labels) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = loo_refuse(h, "st_rows_loo_groups_set")) return rc;
  if (h->loo->n_acc > 0) { h->err = "st_rows_loo_groups_set after " + std::to_string(h->loo->n_acc) + " accumulated iterations (set the groups right after st_rows_loo_set)"; return ST_ERR_USAGE; }
  if (!labels) { h->err = "st_rows_loo_groups_set: no labels"; return ST_ERR_USAGE; }
  HCHK(h, hipSetDevice(h->device));
  const long long n = h->n_all;
  std::vector<unsigned char> obs(n);
  HCHK(h, hipMemcpyAsync(obs.data(), h->d_obs.p, n * sizeof(unsigned char), hipMemcpyDeviceToHost, h->stream));
  HCHK(h, hipStreamSynchronize(h->stream));
  LooLayout lay;
  std::string msg;
  if (const int rc = loo_layout(*h, lay, msg)) { h->err = "st_rows_loo_groups_set: " + msg; return rc; }
  std::vector<long long> lab(labels, labels + n);
  std::unique_ptr<LooGroups> gp(new LooGroups());   // the state takes it once every allocation has succeeded
  LgoLayout &G = gp->lay;
  if (const int rc = lgo_layout(*h, lay, lab.data(), obs.data(), G, msg)) { h->err = "st_rows_loo_groups_set: " + msg; return rc; }
  std::vector<int> mem_grp;
  gp->sq_ptr.assign(1, 0);
  for (long long g = 0; g < G.n_groups; ++g) {
    const int gm = G.grp_ptr[g + 1] - G.grp_ptr[g];
    gp->sq_ptr.push_back(gp->sq_ptr.back() + gm * gm);
    mem_grp.insert(mem_grp.end(), gm, (int)g);
  }
  const size_t ng = (size_t)std::max(G.n_groups, 1ll), nm = (size_t)std::max(G.n_members, 1ll), nsq = (size_t)std::max(gp->sq_ptr.back(), 1);
  HCHK(h, gp->d_prptr.upload(G.pr_ptr)); HCHK(h, upload_or_dummy(gp->d_pra, G.pr_a)); HCHK(h, upload_or_dummy(gp->d_prb, G.pr_b));
  HCHK(h, upload_or_dummy(gp->d_prfin, G.pr_fin)); HCHK(h, gp->d_grpptr.upload(G.grp_ptr)); HCHK(h, gp->d_gpptr.upload(G.gp_ptr));
  HCHK(h, upload_or_dummy(gp->d_gpidx, G.gp_idx)); HCHK(h, gp->d_sqptr.upload(gp->sq_ptr)); HCHK(h, upload_or_dummy(gp->d_memgrp, mem_grp));
  HCHK(h, gp->d_voff.upload(G.voff)); HCHK(h, upload_or_dummy(gp->d_memrow, G.mem_row));
  HCHK(h, gp->d_S.alloc((size_t)std::max(G.arena, 1ll))); HCHK(h, gp->d_pairval.alloc((size_t)std::max(G.n_pairs, 1ll)));
  HCHK(h, gp->d_lastq.alloc(nsq)); HCHK(h, gp->d_lastv.alloc(nsq)); HCHK(h, gp->d_lastc.alloc(nm)); HCHK(h, gp->d_lastm.alloc(nm));
  HCHK(h, gp->d_gacc.alloc((size_t)LGO_NGACC * ng)); HCHK(h, gp->d_macc.alloc((size_t)LGO_NMACC * nm));
  HCHK(h, gp->d_gout.alloc(2 * ng)); HCHK(h, gp->d_rows.alloc(2 * (size_t)n)); HCHK(h, gp->d_tot.alloc((size_t)LGO_NTOT + (size_t)h->q * LGO_NOUTC));
  HCHK(h, hipMemsetAsync(gp->d_gacc.p, 0, (size_t)LGO_NGACC * ng * sizeof(double), h->stream));
  HCHK(h, hipMemsetAsync(gp->d_macc.p, 0, (size_t)LGO_NMACC * nm * sizeof(double), h->stream));
  HCHK(h, hipMemsetAsync(gp->d_rows.p, 0xff, 2 * (size_t)n * sizeof(double), h->stream));   // all bits set: a NaN
  HCHK(h, hipStreamSynchronize(h->stream));
  if (const int rc = lgo_store(h, "st_rows_loo_groups_set", *gp, h->loo->keep())) return rc;
  h->loo->grp = std::move(gp);
  h->loo->d_S = DevBuf<double>();   // the sweep runs on the groups' arena: the vectors are held once
  return ST_OK;
}
extern "C" int st_rows_loo_groups_clear(st_handle h) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = lgo_refuse(h, "st_rows_loo_groups_clear")) return rc;
  if (h->loo->n_acc > 0) { h->err = "st_rows_loo_groups_clear after " + std::to_string(h->loo->n_acc) + " accumulated iterations (st_rows_loo_set starts anew)"; return ST_ERR_USAGE; }
  HCHK(h, hipSetDevice(h->device));
  HCHK(h, hipStreamSynchronize(h->stream));
  if (!h->loo->d_S.p) HCHK(h, h->loo->d_S.alloc((size_t)h->loo->arena));   // the rows' own arena again, before the groups' leaves
  h->loo->grp.reset();
  return ST_OK;
}
extern "C" int st_rows_loo_groups_count(st_handle h, int64_t *n_groups, int64_t *n_members, int64_t *n_pairs, int64_t *n_matrix) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = lgo_refuse(h, "st_rows_loo_groups_count")) return rc;
  const LooGroups &G = *h->loo->grp;
  if (n_groups) *n_groups = G.lay.n_groups;
  if (n_members) *n_members = G.lay.n_members;
  if (n_pairs) *n_pairs = G.lay.n_pairs;
  if (n_matrix) *n_matrix = G.sq_ptr.back();
  return ST_OK;
}
extern "C" int st_rows_loo_groups_index(st_handle h, int64_t *label, int64_t *ptr, int64_t *rows) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = lgo_refuse(h, "st_rows_loo_groups_index")) return rc;
  const LgoLayout &G = h->loo->grp->lay;
  if (label) std::copy(G.label.begin(), G.label.end(), label);
  if (ptr) std::copy(G.grp_ptr.begin(), G.grp_ptr.end(), ptr);
  if (rows) std::copy(G.mem_model.begin(), G.mem_model.end(), rows);
  return ST_OK;
}
static int download_to(st_handle h, const double *src, size_t count, double *dst) {
  if (!dst || count == 0) return ST_OK;
  HCHK(h, hipMemcpyAsync(dst, src, count * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HCHK(h, hipStreamSynchronize(h->stream));
  return ST_OK;
}
extern "C" int st_rows_loo_groups_last(st_handle h, double *q_gg, double *qw, double *cond_mean, double *cond_cov) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = lgo_refuse(h, "st_rows_loo_groups_last", true)) return rc;
  HCHK(h, hipSetDevice(h->device));
  const LooGroups &G = *h->loo->grp;
  const size_t nsq = (size_t)G.sq_ptr.back(), nm = (size_t)G.lay.n_members;
  if (const int rc = download_to(h, G.d_lastq.p, nsq, q_gg)) return rc;
  if (const int rc = download_to(h, G.d_lastc.p, nm, qw)) return rc;
  if (const int rc = download_to(h, G.d_lastm.p, nm, cond_mean)) return rc;
  return download_to(h, G.d_lastv.p, nsq, cond_cov);
}
// the groups' and members' outputs and the totals, once per number of accumulated draws
static int lgo_finish(st_handle h) {
  RowsLoo &L = *h->loo;
  LooGroups &G = *L.grp;
  if (G.fin_acc == L.n_acc) return ST_OK;
  LgoFinishArgs F;
  std::memset(&F, 0, sizeof(F));
  F.G = (int)G.lay.n_groups; F.q = h->q; F.n = h->n_all; F.n_members = G.lay.n_members; F.S = (double)L.n_acc;
  F.mem_grp = G.d_memgrp.p; F.mem_row = G.d_memrow.p; F.y = h->d_y.p; F.obs = h->d_obs.p; F.mv = h->d_mv.p;
  F.gacc = G.d_gacc.p; F.macc = G.d_macc.p; F.gout = G.d_gout.p; F.rows = G.d_rows.p; F.tot = G.d_tot.p;
  if (const int e = lgo_finish_launch(F, h->stream)) return launch_failed(h, "st_rows_loo_groups finish", e);
  G.fin_acc = L.n_acc;
  return ST_OK;
}
extern "C" int st_rows_loo_groups_get(st_handle h, double *elpd_lgo, double *weight_ess, int64_t *n_skipped, double *mu_lgo, double *pit_lgo,
                                      int64_t *n_accumulated) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = lgo_refuse(h, "st_rows_loo_groups_get")) return rc;
  if (n_accumulated) *n_accumulated = h->loo->n_acc;
  if (const int rc = lgo_refuse(h, "st_rows_loo_groups_get", true)) return rc;
  HCHK(h, hipSetDevice(h->device));
  if (const int rc = lgo_finish(h)) return rc;
  const LooGroups &G = *h->loo->grp;
  const size_t ng = (size_t)G.lay.n_groups;
  if (const int rc = download_to(h, G.d_gout.p, ng, elpd_lgo)) return rc;
  if (const int rc = download_to(h, G.d_gout.p + ng, ng, weight_ess)) return rc;
  if (n_skipped && ng) {
    std::vector<double> ns;
    if (const int rc = download_host(h, G.d_gacc.p + (size_t)LGO_NS * ng, ng, ns)) return rc;
    for (size_t g = 0; g < ng; ++g) n_skipped[g] = (int64_t)ns[g];
  }
  double *const dst[2] = {mu_lgo, pit_lgo};
  return download_planes(h, G.d_rows.p, h->n_all, 2, dst);
}
extern "C" int st_rows_loo_groups_totals(st_handle h, double *tot, double *by_outcome) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = lgo_refuse(h, "st_rows_loo_groups_totals", true)) return rc;
  HCHK(h, hipSetDevice(h->device));
  if (const int rc = lgo_finish(h)) return rc;
  std::vector<double> t;
  if (const int rc = download_host(h, h->loo->grp->d_tot.p, (size_t)LGO_NTOT + (size_t)h->q * LGO_NOUTC, t)) return rc;
  if (tot) {
    const double cnt = t[LGO_TOT_COUNT], sum = t[LGO_TOT_ELPD];
    tot[ST_ROWS_LGO_ELPD] = sum;
    tot[ST_ROWS_LGO_IC] = -2.0 * sum;
    tot[ST_ROWS_LGO_SE] = cnt > 1.0 ? std::sqrt(cnt * t[LGO_TOT_ELPD_SQ] / (cnt - 1.0)) : std::nan("");   // the centred sum of squares
    tot[ST_ROWS_LGO_MIN_ESS] = cnt > 0.0 ? t[LGO_TOT_MIN_ESS] : std::nan("");
    tot[ST_ROWS_LGO_COUNT] = cnt;
  }
  if (by_outcome) std::copy(t.begin() + LGO_NTOT, t.end(), by_outcome);   // LGO_OUT_* = ST_ROWS_LGO_OUT_*
  return ST_OK;
}

// ---- Pareto smoothing of the stored leave-one-out ratios (psis_kernels.hpp; the kernels and their launchers live in k_psis.hip) ----
extern "C" int st_rows_loo_reserve(st_handle h, int64_t keep) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = loo_refuse(h, "st_rows_loo_reserve")) return rc;
  if (h->loo->n_acc > 0) { h->err = "st_rows_loo_reserve after " + std::to_string(h->loo->n_acc) + " accumulated iterations (reserve right after st_rows_loo_set)"; return ST_ERR_USAGE; }
  if (keep != 0)
    if (const int rc = psis_check_draws("st_rows_loo_reserve", "keep", keep, h->err)) return rc;
  HCHK(h, hipSetDevice(h->device));
  HCHK(h, hipStreamSynchronize(h->stream));
  if (keep == 0) {
    h->loo->psis.reset();
    if (h->loo->grp) return lgo_store(h, "st_rows_loo_reserve", *h->loo->grp, 0);
    return ST_OK;
  }
  const size_t n = (size_t)h->n_all, cnt = 3 * (size_t)keep * n;
  std::unique_ptr<PsisStore> ps(new PsisStore());   // the state takes it once every allocation has succeeded
  if (ps->d_store.alloc(cnt) != hipSuccess || ps->d_rows.alloc((size_t)PSIS_NOUT * n) != hipSuccess || ps->d_int.alloc(2 * n) != hipSuccess ||
      ps->d_tot.alloc((size_t)h->q * PSIS_NSUM) != hipSuccess) {
    (void)hipGetLastError();
    char buf[160];
    std::snprintf(buf, sizeof(buf), "st_rows_loo_reserve: the store of %lld draws x %lld rows (%.0f bytes) could not be allocated",
                  (long long)keep, (long long)h->n_all, psis_store_bytes(keep, h->n_all));
    h->err = buf;
    return ST_ERR_HIP;
  }
  HCHK(h, hipMemsetAsync(ps->d_store.p, 0xff, cnt * sizeof(double), h->stream));   // all bits set: a NaN
  HCHK(h, hipStreamSynchronize(h->stream));
  if (h->loo->grp)
    if (const int rc = lgo_store(h, "st_rows_loo_reserve", *h->loo->grp, keep)) return rc;
  ps->keep = keep;
  h->loo->psis = std::move(ps);
  return ST_OK;
}
static int psis_refuse(st_handle h, const char *who) {
  if (const int rc = loo_refuse(h, who)) return rc;
  if (h->loo->keep() == 0) { h->err = std::string(who) + ": no store reserved (st_rows_loo_reserve before the first accumulate)"; return ST_ERR_USAGE; }
  return loo_refuse(h, who, true, true);
}
extern "C" int st_rows_loo_draws(st_handle h, double *t, double *phi, double *mu) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = psis_refuse(h, "st_rows_loo_draws")) return rc;
  HCHK(h, hipSetDevice(h->device));
  double *const dst[3] = {t, phi, mu};
  const size_t n = (size_t)h->n_all, plane = (size_t)h->loo->keep() * n;
  for (long long d = 0; d < h->loo->n_acc; ++d)
    if (const int rc = download_planes(h, h->loo->psis->d_store.p + (size_t)d * n, plane, 3, dst, (size_t)d * n)) return rc;
  return ST_OK;
}
// one pass of k_loo_psis over a [K][n] device store into device outputs (PSIS_NOUT x n doubles; tail_len, n_draws: n each)
static int psis_run(st_handle h, const char *who, long long n, long long K, const double *t, const double *phi, const double *mu,
                    double *rows, int *ints) {
  PsisArgs A = {};
  if (!psis_plan(K, h->lds_limit, &A.R, &A.Kpad)) {
    h->err = std::string(who) + ": the sorted copy of " + std::to_string(K) + " stored draws of one series does not fit one workgroup's LDS";
    return ST_ERR_UNSUPPORTED;
  }
  A.t = t; A.phi = phi; A.mu = mu; A.n = n; A.K = (int)K; A.out = rows; A.tail_len = ints; A.n_draws = ints + n;
  if (const int e = psis_launch(A, h->stream)) return launch_failed(h, who, e);
  return ST_OK;
}
// after `who`'s refusals: the rows' own outputs and totals, once per number of accumulated draws
static int psis_finish(st_handle h, const char *who) {
  if (const int rc = psis_refuse(h, who)) return rc;
  HCHK(h, hipSetDevice(h->device));
  const RowsLoo &L = *h->loo;
  PsisStore &P = *L.psis;
  if (P.fin_acc == L.n_acc) return ST_OK;
  const size_t plane = (size_t)P.keep * h->n_all;
  if (const int rc = psis_run(h, who, h->n_all, L.n_acc, P.d_store.p, P.d_store.p + plane, P.d_store.p + 2 * plane, P.d_rows.p, P.d_int.p)) return rc;
  PsisFinishArgs F = {};
  F.y = h->d_y.p; F.obs = h->d_obs.p; F.mv = h->d_mv.p; F.rows = P.d_rows.p; F.n_draws = P.d_int.p + h->n_all;
  F.n = h->n_all; F.q = h->q; F.tot = P.d_tot.p;
  F.thr = L.n_acc > 1 ? std::min(1.0 - 1.0 / std::log10((double)L.n_acc), 0.7) : -HUGE_VAL;
  if (const int e = psis_finish_launch(F, h->stream)) return launch_failed(h, std::string(who) + " finish", e);
  P.fin_acc = L.n_acc;
  return ST_OK;
}
// the device outputs of a pass to the caller's arrays; perm (device row -> model row) or NULL
static int psis_download(st_handle h, long long n, const double *rows, const int *ints, const long long *perm, const st_psis_out *out,
                         bool have_phi, bool have_mu) {
  if (!out || n == 0) return ST_OK;
  double *const dst[PSIS_NOUT] = {out->khat, out->elpd_psis, have_phi ? out->pit_psis : nullptr, have_mu ? out->mu_psis : nullptr,
                                  out->weight_ess_psis};   // PSIS_OUT_* order
  int32_t *const idst[2] = {out->tail_len, out->n_draws};
  std::vector<double> tmp((size_t)PSIS_NOUT * n);
  std::vector<int> itmp(2 * (size_t)n);
  HCHK(h, hipMemcpyAsync(tmp.data(), rows, tmp.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HCHK(h, hipMemcpyAsync(itmp.data(), ints, itmp.size() * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HCHK(h, hipStreamSynchronize(h->stream));
  for (int k = 0; k < PSIS_NOUT; ++k)
    if (dst[k]) scatter_rows(dst[k], tmp.data() + (size_t)k * n, 1, n, perm);
  for (int k = 0; k < 2; ++k)
    if (idst[k]) scatter_rows(idst[k], itmp.data() + (size_t)k * n, 1, n, perm);
  return ST_OK;
}
extern "C" int st_rows_loo_psis(st_handle h, const st_psis_out *out) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = psis_finish(h, "st_rows_loo_psis")) return rc;
  return psis_download(h, h->n_all, h->loo->psis->d_rows.p, h->loo->psis->d_int.p, h->dev2model.data(), out, true, true);
}
extern "C" int st_rows_loo_psis_totals(st_handle h, double *tot, int64_t *n_obs) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = psis_finish(h, "st_rows_loo_psis_totals")) return rc;
  std::vector<double> t;
  if (const int rc = download_host(h, h->loo->psis->d_tot.p, (size_t)h->q * PSIS_NSUM, t)) return rc;
  for (int j = 0; j < h->q; ++j) {
    double *s = t.data() + (size_t)j * PSIS_NSUM;
    if (n_obs) n_obs[j] = h->n_obs_q[j];
    if (s[ST_ROWS_PSIS_COUNT] == 0.0) s[ST_ROWS_PSIS_MIN_ESS] = s[ST_ROWS_PSIS_MAX_KHAT] = std::nan("");
    if (tot) std::copy(s, s + PSIS_NSUM, tot + (size_t)j * ST_ROWS_PSIS_N);
  }
  return ST_OK;
}
// the groups' stored log ratios through the same kernel: one series per group, no companions
static int lgo_psis_refuse(st_handle h, const char *who) {
  if (const int rc = lgo_refuse(h, who)) return rc;
  if (h->loo->grp->keep == 0) { h->err = std::string(who) + ": no store reserved (st_rows_loo_reserve before the first accumulate)"; return ST_ERR_USAGE; }
  return lgo_refuse(h, who, true);
}
extern "C" int st_rows_loo_groups_draws(st_handle h, double *t) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = lgo_psis_refuse(h, "st_rows_loo_groups_draws")) return rc;
  HCHK(h, hipSetDevice(h->device));
  const LooGroups &G = *h->loo->grp;
  return download_to(h, G.d_store.p, (size_t)h->loo->n_acc * (size_t)G.lay.n_groups, t);
}
extern "C" int st_rows_loo_groups_psis(st_handle h, double *khat, double *elpd_psis, double *weight_ess_psis, int32_t *tail_len, int32_t *n_draws) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = lgo_psis_refuse(h, "st_rows_loo_groups_psis")) return rc;
  HCHK(h, hipSetDevice(h->device));
  const RowsLoo &L = *h->loo;
  LooGroups &G = *L.grp;
  const long long ng = G.lay.n_groups;
  if (G.psis_acc != L.n_acc) {
    if (const int rc = psis_run(h, "st_rows_loo_groups_psis", ng, L.n_acc, G.d_store.p, nullptr, nullptr, G.d_prow.p, G.d_pint.p)) return rc;
    G.psis_acc = L.n_acc;
  }
  const st_psis_out out = {khat, elpd_psis, nullptr, nullptr, weight_ess_psis, tail_len, n_draws};
  return psis_download(h, ng, G.d_prow.p, G.d_pint.p, nullptr, &out, false, false);
}
extern "C" int st_psis(st_handle h, int64_t n, int64_t K, const double *t, const double *phi, const double *mu, const st_psis_out *out) {
  if (!h) return ST_ERR_USAGE;
  if (n < 0) { h->err = "st_psis: n = " + std::to_string(n) + " must not be negative"; return ST_ERR_USAGE; }
  if (const int rc = psis_check_draws("st_psis", "K", K, h->err)) return rc;
  if (n == 0) return ST_OK;
  if (!t) { h->err = "st_psis: no log ratios"; return ST_ERR_USAGE; }
  HCHK(h, hipSetDevice(h->device));
  const size_t cnt = (size_t)n * K;
  DevBuf<double> d_t, d_phi, d_mu, d_rows;
  DevBuf<int> d_int;
  HCHK(h, d_t.alloc(cnt)); HCHK(h, d_rows.alloc((size_t)PSIS_NOUT * n)); HCHK(h, d_int.alloc(2 * (size_t)n));
  HCHK(h, hipMemcpyAsync(d_t.p, t, cnt * sizeof(double), hipMemcpyHostToDevice, h->stream));
  if (phi) { HCHK(h, d_phi.alloc(cnt)); HCHK(h, hipMemcpyAsync(d_phi.p, phi, cnt * sizeof(double), hipMemcpyHostToDevice, h->stream)); }
  if (mu) { HCHK(h, d_mu.alloc(cnt)); HCHK(h, hipMemcpyAsync(d_mu.p, mu, cnt * sizeof(double), hipMemcpyHostToDevice, h->stream)); }
  int rc = psis_run(h, "st_psis", n, K, d_t.p, d_phi.p, d_mu.p, d_rows.p, d_int.p);
  if (rc == ST_OK) rc = psis_download(h, n, d_rows.p, d_int.p, nullptr, out, phi != nullptr, mu != nullptr);
  const hipError_t es = hipStreamSynchronize(h->stream);   // the buffers go with this scope
  if (rc == ST_OK && es != hipSuccess) { h->err = std::string("st_psis: ") + hipGetErrorString(es); rc = ST_ERR_HIP; }
  return rc;
}
extern "C" int st_psis_info(st_handle h, int64_t n, int64_t K, int32_t n_comp, int32_t *R, int32_t *Kpad, int64_t *lds_bytes, double *alg_bytes) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = psis_check_draws("st_psis_info", "K", K, h->err)) return rc;
  int r = 0, kp = 0;
  if (!psis_plan(K, h->lds_limit, &r, &kp)) {
    h->err = "st_psis_info: the sorted copy of " + std::to_string(K) + " stored draws of one series does not fit one workgroup's LDS";
    return ST_ERR_UNSUPPORTED;
  }
  if (R) *R = r;
  if (Kpad) *Kpad = kp;
  if (lds_bytes) *lds_bytes = (int64_t)psis_lds_bytes(r, kp);
  if (alg_bytes) *alg_bytes = (double)n * ((double)K * 8.0 * (2.0 + (double)std::max(0, std::min(n_comp, 2))) + 8.0 * PSIS_NOUT + 8.0);
  return ST_OK;
}
