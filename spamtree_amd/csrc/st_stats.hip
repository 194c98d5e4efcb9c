// st_stats.hip -- the beta / tausq sufficient statistics of the current (w, XB) with their cache, and the outputs that read w and
// XB: st_set_beta (XB itself), st_set_tausq_inv, st_get_xb, st_yhat, st_xtx.  The state is the handle's StatsCache (st_handle.hpp).
#include "st_handle.hpp"
#include "misc_kernels.hpp"

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
void launch_stats(st_handle_s *h, hipStream_t st, const double *wt) {
  const StatsKernel k_stats = stats_kernel(h->q, wt != nullptr);
  hipLaunchKernelGGL(k_stats, dim3(STATS_WG, (h->p + 7) / 8), dim3(NT), 0, st, h->d_X.p, h->d_y.p, h->d_w.p, h->d_xb.p, h->d_mv.p,
                     h->d_obs.p, h->d_partner.p, wt, h->n_all, h->p, h->d_partial.p);
}

// w or XB is about to change: the cached statistics die; a reduction still in flight on the second stream finishes first
void invalidate_stats(st_handle_s *h) {
  if (h->stats.on_stream2) {
    (void)hipSetDevice(h->device);
    (void)hipStreamWaitEvent(h->stream, h->stats.ev, 0);
    h->stats.on_stream2 = false;
  }
  h->stats.valid = false; h->stats.host_valid = false;
}

static int run_stats(st_handle h, hipStream_t st = nullptr) {
  const int nq = h->p * h->q + h->q;
  if (h->stats.valid) return ST_OK;   // w and XB unchanged since the last reduction: both statistics are still current
  if (!st) st = h->stream;
  {
    ProfScope ps(h, 4, -1, 1, st);
    launch_stats(h, st, nullptr);
    hipLaunchKernelGGL(k_stats_final, dim3(nq), dim3(NT), 0, st, h->d_partial.p, STATS_WG, nq, h->d_stats.p);
  }
  HCHK(h, hipGetLastError());
  h->stats.valid = true;
  return ST_OK;
}
// The beta / tausq statistics of the iteration need the sweep's w and the current XB only: when a proposal is about to be
// factorised they start on the second stream and run under phase A (the driver asks for them after the Metropolis step).
int stats_begin(st_handle h) {
  if (!h->stream2 || h->stats.valid) return ST_OK;
  HCHK(h, hipEventRecord(h->ev_main, h->stream));           // w of the sweep is final at this point of the main stream
  HCHK(h, hipStreamWaitEvent(h->stream2, h->ev_main, 0));
  int rc = run_stats(h, h->stream2);
  if (rc) return rc;
  // the results travel to pinned host memory on the same stream: when the driver asks (after the Metropolis step) they are
  // there, and fetching them costs an event query instead of a copy + a synchronisation of the main stream
  const size_t nq = (size_t)h->p * h->q + h->q;
  h->stats.prefetched = nq <= (size_t)ST_PIN_STATS;
  if (h->stats.prefetched) HCHK(h, hipMemcpyAsync(h->pin->stats, h->d_stats.p, nq * sizeof(double), hipMemcpyDeviceToHost, h->stream2));
  HCHK(h, hipEventRecord(h->stats.ev, h->stream2));
  h->stats.on_stream2 = true;
  return ST_OK;
}
// both statistics travel to the host together; a second request for the same (w, XB) is served from the host copy
static int fetch_stats(st_handle h) {
  if (h->stats.valid && h->stats.host_valid) return ST_OK;
  int rc = run_stats(h);
  if (rc) return rc;
  const size_t nq = (size_t)h->p * h->q + h->q;
  h->stats.host.resize(nq);
  if (h->stats.on_stream2) {   // started under phase A (stats_begin)
    if (h->stats.prefetched) {   // ... and already copied to pinned memory behind them on the second stream
      HCHK(h, hipEventSynchronize(h->stats.ev));
      HCHK(h, hipStreamWaitEvent(h->stream, h->stats.ev, 0));   // later work on the main stream stays ordered behind the reduction
      h->stats.on_stream2 = false;
      for (size_t i = 0; i < nq; ++i) h->stats.host[i] = h->pin->stats[i];
      h->stats.host_valid = true;
      return ST_OK;
    }
    HCHK(h, hipStreamWaitEvent(h->stream, h->stats.ev, 0));   // its results before the copy
    h->stats.on_stream2 = false;
  }
  HCHK(h, hipMemcpyAsync(h->stats.host.data(), h->d_stats.p, nq * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HCHK(h, hipStreamSynchronize(h->stream));
  h->stats.host_valid = true;
  return ST_OK;
}
extern "C" int st_beta_stats(st_handle h, double *xty) {
  if (!h || !xty) return ST_ERR_USAGE;
  HCHK(h, hipSetDevice(h->device));
  int rc = fetch_stats(h);
  if (rc) return rc;
  for (int i = 0; i < h->p * h->q; ++i) xty[i] = h->stats.host[i];
  return ST_OK;
}
extern "C" int st_tausq_stats(st_handle h, double *ssq, int64_t *n_obs_by_q) {
  if (!h || !ssq) return ST_ERR_USAGE;
  HCHK(h, hipSetDevice(h->device));
  int rc = fetch_stats(h);
  if (rc) return rc;
  for (int j = 0; j < h->q; ++j) ssq[j] = h->stats.host[(size_t)h->p * h->q + j];
  if (n_obs_by_q)
    for (int j = 0; j < h->q; ++j) n_obs_by_q[j] = h->n_obs_q[j];
  return ST_OK;
}
extern "C" int st_xtx(st_handle h, double *xtx) {
  if (!h || !xtx) return ST_ERR_USAGE;
  std::memcpy(xtx, h->xtx.data(), h->xtx.size() * sizeof(double));
  return ST_OK;
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
extern "C" int st_get_xb(st_handle h, double *xb) {
  if (!h || !xb) return ST_ERR_USAGE;
  HCHK(h, hipSetDevice(h->device));
  return download_rows(h, h->d_xb.p, xb);
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
