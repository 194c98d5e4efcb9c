// st_summary.hip -- the C-ABI of the running summaries of the fit's rows (st_summary_*), the rows as a draw store (rows_store)
// and the quantile that every draw store goes through (store_quantile, draw_store.hpp).  The state is the handle's own
// (st_handle.hpp): it is always present, and the criteria over the rows (st_rows.hip) read the stored draws and their epoch.
#include "st_handle.hpp"
#include "misc_kernels.hpp"
#include "draw_store.hpp"

// ---- running posterior means on device: call st_summary_accumulate on every saved iteration
extern "C" int st_summary_reset(st_handle h) {
  if (!h) return ST_ERR_USAGE;
  HCHK(h, hipSetDevice(h->device));
  if (!h->d_sum_w.p) { HCHK(h, h->d_sum_w.alloc(h->n_all)); HCHK(h, h->d_sum_yhat.alloc(h->n_all)); }
  HCHK(h, hipMemsetAsync(h->d_sum_w.p, 0, h->n_all * sizeof(double), h->stream));
  HCHK(h, hipMemsetAsync(h->d_sum_yhat.p, 0, h->n_all * sizeof(double), h->stream));
  h->n_summary = 0; h->n_draws = 0; h->draws_epoch += 1;
  return ST_OK;
}
extern "C" int st_summary_accumulate(st_handle h, uint64_t seed, uint32_t iter) {   // yhat noise: device stream 5 (spamtree_fit.cpp:384)
  if (!h) return ST_ERR_USAGE;
  if (!h->d_sum_w.p) { const int rc0 = st_summary_reset(h); if (rc0) return rc0; }
  HCHK(h, hipSetDevice(h->device));
  int rc = gen_or_upload_z(h, nullptr, seed, iter, 5u, h->d_tmp_n.p);
  if (rc) return rc;
  const int grid = (int)((h->n_all + NT - 1) / NT);
  hipLaunchKernelGGL(k_yhat, dim3(grid), dim3(NT), 0, h->stream, h->d_xb.p, h->d_w.p, h->d_tmp_n.p, h->d_mv.p, h->n_all, h->d_tsq.p, h->d_tmp_n.p);
  hipLaunchKernelGGL(k_axpy_sum, dim3(grid), dim3(NT), 0, h->stream, h->d_sum_yhat.p, h->d_tmp_n.p, h->n_all);
  hipLaunchKernelGGL(k_axpy_sum, dim3(grid), dim3(NT), 0, h->stream, h->d_sum_w.p, h->d_w.p, h->n_all);
  HCHK(h, hipGetLastError());
  if (h->n_draws < h->draws_cap) {   // keep the draw itself for the quantiles (device order, one contiguous row per draw)
    HCHK(h, hipMemcpyAsync(h->d_draws_w.p + (size_t)h->n_draws * h->n_all, h->d_w.p, h->n_all * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    HCHK(h, hipMemcpyAsync(h->d_draws_yhat.p + (size_t)h->n_draws * h->n_all, h->d_tmp_n.p, h->n_all * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    h->n_draws += 1; h->draws_epoch += 1;
  }
  h->n_summary += 1;
  return ST_OK;
}
extern "C" int st_summary_reserve(st_handle h, int64_t keep) {
  if (!h || keep < 0) return ST_ERR_USAGE;
  HCHK(h, hipSetDevice(h->device));
  HCHK(h, hipStreamSynchronize(h->stream));
  h->d_draws_w.free(); h->d_draws_yhat.free();
  h->draws_cap = 0; h->n_draws = 0; h->draws_epoch += 1;
  if (keep == 0) return ST_OK;
  if (keep > STORE_MAX_DRAWS) {
    h->err = "st_summary_reserve: at most " + std::to_string(STORE_MAX_DRAWS) + " saved draws (one row's draws are sorted in one workgroup's LDS)";
    return ST_ERR_UNSUPPORTED;
  }
  HCHK(h, h->d_draws_w.alloc((size_t)keep * h->n_all));
  HCHK(h, h->d_draws_yhat.alloc((size_t)keep * h->n_all));
  h->draws_cap = keep;
  return ST_OK;
}
// ---- the summaries of stored draws (draw_store.hpp).  The fit's rows as a store: device row order, the domains and thresholds
// go by outcome (d_mv), the outputs come back in model row order (dev2model)
static DrawStore rows_store(st_handle h) {
  DrawStore s;
  if (!h) { s.rc = ST_ERR_USAGE; return s; }
  s.w = h->d_draws_w.p; s.yhat = h->d_draws_yhat.p; s.n = h->n_all; s.K = h->n_draws;
  s.d_outcome = h->d_mv.p; s.G = h->q; s.perm = h->dev2model.data(); s.d_scratch = h->d_tmp_n.p;
  s.reserve = "st_summary_reserve";
  return s;
}
// k_qtile (misc_kernels.hpp) over the stored draws of w and yhat into w_q and yhat_q (NULL: skipped), through the store's scratch
int store_quantile(st_handle_s *h, const char *who, const DrawStore &s, double q, double *w_q, double *yhat_q) {
  if (s.rc) return s.rc;
  if (!(q >= 0.0 && q <= 1.0)) { h->err = std::string(who) + ": q must lie in [0, 1]"; return ST_ERR_USAGE; }
  if (s.K == 0) { h->err = std::string(who) + ": no draw stored (call " + s.reserve + " before the saved iterations)"; return ST_ERR_USAGE; }
  if (yhat_q && s.yhat_needs_X) { h->err = std::string(who) + ": yhat_q needs the regressors X of st_points_set"; return ST_ERR_USAGE; }
  HCHK(h, hipSetDevice(h->device));
  QtArgs A;
  A.n = s.n; A.keep = (int)s.K; A.q = q; A.out = s.d_scratch;
  qtile_plan(s.K, &A.Kpad, &A.R);
  const size_t lds = (size_t)A.R * A.Kpad * sizeof(double);
  (void)hipFuncSetAttribute((const void *)k_qtile, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds_limit);
  std::vector<double> tmp(s.perm ? (size_t)s.n : 0);
  for (int which = 0; which < 2; ++which) {
    double *dst = which ? yhat_q : w_q;
    if (!dst) continue;
    A.draws = which ? s.yhat : s.w;
    hipLaunchKernelGGL(k_qtile, dim3((unsigned)((s.n + A.R - 1) / A.R)), dim3(NT), lds, h->stream, A);
    HCHK(h, hipGetLastError());
    HCHK(h, hipMemcpyAsync(s.perm ? tmp.data() : dst, s.d_scratch, (size_t)s.n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HCHK(h, hipStreamSynchronize(h->stream));
    if (s.perm) scatter_rows(dst, tmp.data(), 1, s.n, s.perm);
  }
  return ST_OK;
}
extern "C" int st_summary_quantile(st_handle h, double q, double *w_q, double *yhat_q) {
  return store_quantile(h, __func__, rows_store(h), q, w_q, yhat_q);
}
extern "C" int st_summary_diagnostics(st_handle h, int32_t max_lag, const st_series_diag *w, const st_series_diag *yhat) {
  return store_diagnostics(h, __func__, rows_store(h), max_lag, w, yhat);
}
extern "C" int st_summary_excursions(st_handle h, const st_excursion_spec *spec, const st_excursion_out *w, const st_excursion_out *yhat) {
  return store_excursions(h, __func__, rows_store(h), spec, w, yhat);
}
extern "C" int st_summary_rank_diagnostics(st_handle h, const st_rank_spec *spec, const st_rank_out *w, const st_rank_out *yhat) {
  return store_rank_diagnostics(h, __func__, rows_store(h), spec, w, yhat);
}
extern "C" int st_summary_chain_diagnostics(st_handle h, int32_t n_chains, int32_t max_lag, const st_series_diag *w, const st_series_diag *yhat) {
  return store_chain_diagnostics(h, __func__, rows_store(h), n_chains, max_lag, w, yhat);
}
extern "C" int st_summary_chain_rank_diagnostics(st_handle h, int32_t n_chains, const st_rank_spec *spec, const st_rank_out *w,
                                                 const st_rank_out *yhat) {
  return store_chain_rank_diagnostics(h, __func__, rows_store(h), n_chains, spec, w, yhat);
}
extern "C" int st_summary_get(st_handle h, double *w_mean, double *yhat_mean, int64_t *n_accumulated) {
  if (!h) return ST_ERR_USAGE;
  if (n_accumulated) *n_accumulated = h->n_summary;
  if (h->n_summary == 0 || !h->d_sum_w.p) { h->err = "no iteration accumulated"; return ST_ERR_USAGE; }
  HCHK(h, hipSetDevice(h->device));
  const double inv = 1.0 / (double)h->n_summary;
  if (w_mean) { int rc = download_rows(h, h->d_sum_w.p, w_mean); if (rc) return rc; for (long long i = 0; i < h->n_all; ++i) w_mean[i] *= inv; }
  if (yhat_mean) { int rc = download_rows(h, h->d_sum_yhat.p, yhat_mean); if (rc) return rc; for (long long i = 0; i < h->n_all; ++i) yhat_mean[i] *= inv; }
  return ST_OK;
}
