// draw_store.hpp -- one view of a store of saved draws for the summaries of the stored draws (quantiles, diagnostics, excursions,
// rank diagnostics).  Draws are kept in three places: the fit's rows (rows_store, st_summary.hip), the new points and their
// functionals (points_store, fun_store, st_points.hip).  A C-ABI entry point is one store_* call on its resolver's view.
// No HIP header: store_spec.cpp, the pure host helpers declared at the end, is compiled and checked without a device.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "spamtree_hip.h"

// Owns nothing, allocates nothing.  A store is draws[d * n + i], d < K, i < n.
struct DrawStore {
  int rc = ST_OK;                               // the resolver's refusal (its text is in the handle): nothing else is looked at
  const double *w = nullptr, *yhat = nullptr;   // device; yhat NULL: the store has none
  long long n = 0, K = 0;                       // series and stored draws (n = 0: an empty store, ST_OK with nothing written)
  const int *d_outcome = nullptr;               // the series' domains on the device, store order; NULL: one domain
  int G = 1;                                    // domains
  bool thr_per_series = false;                  // a spec holds n_thr x n thresholds in output order, else n_thr x G
  const long long *perm = nullptr;              // element i of the store is element perm[i] of every per-series array; NULL: i
  double *d_scratch = nullptr;                  // n doubles on the device that the quantile writes through
  const char *reserve = "";                     // the call that makes room for the draws, for the refusals' texts
  bool yhat_needs_X = false;                    // the point set came without X: a yhat output is refused
  long long n_thr_values() const { return thr_per_series ? n : G; }
};

// Each refuses what does not depend on the store, returns ST_OK on an empty store (not the quantile: it refuses "no draw stored"),
// checks the spec and K, refuses yhat without X, and runs its worker on w and on yhat.
struct st_handle_s;
int store_quantile(st_handle_s *h, const char *who, const DrawStore &s, double q, double *w_q, double *yhat_q);
int store_diagnostics(st_handle_s *h, const char *who, const DrawStore &s, int32_t max_lag, const st_series_diag *w, const st_series_diag *yhat);
int store_excursions(st_handle_s *h, const char *who, const DrawStore &s, const st_excursion_spec *spec, const st_excursion_out *w,
                     const st_excursion_out *yhat);
int store_rank_diagnostics(st_handle_s *h, const char *who, const DrawStore &s, const st_rank_spec *spec, const st_rank_out *w,
                           const st_rank_out *yhat);

// The multi-chain forms: the K stored draws are n_chains chains of K / n_chains draws laid end to end.  The same refusals in the
// same order, with check_chains beside the count of stored draws; n_chains = 1 is the call above, bit for bit.
int store_chain_diagnostics(st_handle_s *h, const char *who, const DrawStore &s, int32_t n_chains, int32_t max_lag, const st_series_diag *w,
                            const st_series_diag *yhat);
int store_chain_rank_diagnostics(st_handle_s *h, const char *who, const DrawStore &s, int32_t n_chains, const st_rank_spec *spec,
                                 const st_rank_out *w, const st_rank_out *yhat);

// The most draws a store holds: one series' draws are sorted in one workgroup's LDS (st_summary_reserve, st_points_summary_reserve)
constexpr int STORE_MAX_DRAWS = 16384;

// What an output struct asks for; NULL asks for nothing
inline bool any_out(const st_series_diag *o) { return o && (o->ess || o->mcse || o->sd || o->rhat || o->lags); }
inline bool exc_thr_out(const st_excursion_out *o) { return o && (o->count || o->prob || o->excur || o->joint_all); }
inline bool exc_band_out(const st_excursion_out *o) { return o && (o->mean || o->sd || o->maxdev || o->n_flat); }
inline bool any_out(const st_excursion_out *o) { return exc_thr_out(o) || exc_band_out(o) || (o && o->n_draws); }
inline bool rank_q_out(const st_rank_out *o) { return o && o->ess_q; }
inline bool rank_exc_out(const st_rank_out *o) { return o && (o->ess_exc || o->mcse_prob || o->prob); }
inline bool any_out(const st_rank_out *o) {
  return o && (o->rhat_rank || o->rhat_bulk || o->rhat_fold || o->ess_bulk || o->ess_tail || o->lags_bulk || o->ess_q || rank_exc_out(o));
}
inline bool any_out(const st_rb_out *o) { return o && (o->prob || o->prob_var); }
inline bool any_out(const st_mix_out *o) { return o && (o->q || o->n_unconverged); }

// ---- store_spec.cpp
// The one copy of each spec's checks, for the st_* calls on a handle and for the whole fit's plan (fit_plan.cpp) before a chain
// exists: an excursion and a rank spec with their outputs, K draws stored and n_thr_values thresholds per t, and the thresholds of
// st_points_exceed_set (thr n_thr x q, not NULL; thr_fun n_thr x n_fun or NULL; n_fun < 0: no functionals are set)
// the probabilities of st_points_mixture_quantiles and of the whole fit's mix: n_probs in 1 .. ST_MIX_MAX_PROBS, each strictly inside
// (0, 1) (a NaN is not); the text names the index
int check_mixture_probs(const std::string &W, int n_probs, const double *probs, std::string &msg);
int check_excursion_spec(const std::string &W, const st_excursion_spec *spec, long long K, long long n_thr_values, const st_excursion_out *w,
                         const st_excursion_out *yhat, std::string &msg);
int check_rank_spec(const std::string &W, const st_rank_spec *spec, long long K, long long n_thr_values, const st_rank_out *w,
                    const st_rank_out *yhat, std::string &msg);
int check_exceed_spec(const std::string &W, int n_thr, const double *thr, const int32_t *side, const double *thr_fun, long long q,
                      long long n_fun, std::string &msg);
// n_chains in 1 .. ST_DIAG_MAX_CHAINS, K a multiple of it, K / n_chains >= ST_DIAG_MIN_DRAWS: ST_OK, or ST_ERR_USAGE with W, the
// numbers and the first failing check in msg
int check_chains(const std::string &W, int n_chains, long long K, std::string &msg);
// n_thr in min_thr .. ST_EXC_MAX_THRESHOLDS, thr given with n_thr > 0, n_thr x n_values finite values, sides +1 / -1 (NULL: all +1):
// ST_OK, or ST_ERR_USAGE with W and the first failing check in msg
int check_thresholds(const std::string &W, int n_thr, int min_thr, const double *thr, const int32_t *side, long long n_values, std::string &msg);
// T x stride thresholds in store order into out -- column j from perm[j] where they go per series and the store has a perm;
// returns the mask of the sides: bit t set for side -1
unsigned thresholds_in_store_order(const double *thr, const int32_t *side, int T, long long stride, bool per_series, const long long *perm,
                                   std::vector<double> &out);
// out[i] = mask[perm ? perm[i] : i] != 0
void mask_in_store_order(const uint8_t *mask, long long n, const long long *perm, std::vector<unsigned char> &out);
// dst[r * n + (perm ? perm[i] : i)] = src[r * n + i], r < rows: device results in store order into the caller's arrays
void scatter_rows(double *dst, const double *src, long long rows, long long n, const long long *perm);
void scatter_rows(int32_t *dst, const int32_t *src, long long rows, long long n, const long long *perm);
void scatter_rows(int64_t *dst, const int64_t *src, long long rows, long long n, const long long *perm);
