// store_spec.cpp -- the pure host helpers of the summaries of the stored draws (draw_store.hpp): the checks of the excursion, the
// rank and the exceedance spec, the small inputs brought into store order and the device results scattered into the caller's
// arrays.  No device call and no HIP header: tests/store_spec_check.cpp checks them on the CPU.
#include <cmath>

#include "draw_store.hpp"

int check_thresholds(const std::string &W, int n_thr, int min_thr, const double *thr, const int32_t *side, long long n_values, std::string &msg) {
  if (n_thr < min_thr || n_thr > ST_EXC_MAX_THRESHOLDS) {
    msg = W + "n_thr = " + std::to_string(n_thr) + " must lie in " + std::to_string(min_thr) + " .. " + std::to_string(ST_EXC_MAX_THRESHOLDS);
    return ST_ERR_USAGE;
  }
  if (n_thr > 0 && !thr) { msg = W + "n_thr = " + std::to_string(n_thr) + " without thr"; return ST_ERR_USAGE; }
  for (long long k = 0; k < (long long)n_thr * n_values; ++k)
    if (!std::isfinite(thr[k])) { msg = W + "threshold " + std::to_string(k) + " is not finite"; return ST_ERR_USAGE; }
  for (int t = 0; side && t < n_thr; ++t)
    if (side[t] != 1 && side[t] != -1) { msg = W + "side " + std::to_string(t) + " must be +1 or -1"; return ST_ERR_USAGE; }
  return ST_OK;
}

int check_excursion_spec(const std::string &W, const st_excursion_spec *spec, long long K, long long n_thr_values, const st_excursion_out *w,
                         const st_excursion_out *yhat, std::string &msg) {
  if (!spec) { msg = W + "no spec"; return ST_ERR_USAGE; }
  const bool band = spec->want_band || exc_band_out(w) || exc_band_out(yhat);
  if (!spec->thr && !band) { msg = W + "the spec holds neither thresholds nor a band request"; return ST_ERR_USAGE; }
  if (spec->thr) {
    if (const int rc = check_thresholds(W, spec->n_thr, 1, spec->thr, spec->side, n_thr_values, msg)) return rc;
  } else if (exc_thr_out(w) || exc_thr_out(yhat)) {
    msg = W + "count, prob, excur and joint_all need thresholds";
    return ST_ERR_USAGE;
  }
  if (K < 1) { msg = W + "no draw stored (reserve room before the saved iterations)"; return ST_ERR_USAGE; }
  if (band && K < 2) { msg = W + "the band needs at least 2 stored draws, " + std::to_string(K) + " stored"; return ST_ERR_USAGE; }
  return ST_OK;
}

int check_rank_spec(const std::string &W, const st_rank_spec *spec, long long K, long long n_thr_values, const st_rank_out *w,
                    const st_rank_out *yhat, std::string &msg) {
  if (!spec) { msg = W + "no spec"; return ST_ERR_USAGE; }
  if (spec->max_lag < 0) { msg = W + "max_lag must not be negative (0: the default cap)"; return ST_ERR_USAGE; }
  if (spec->n_prob < 0 || spec->n_prob > ST_RANK_MAX_PROBS) {
    msg = W + "n_prob = " + std::to_string(spec->n_prob) + " must lie in 0 .. " + std::to_string(ST_RANK_MAX_PROBS);
    return ST_ERR_USAGE;
  }
  if (spec->n_prob > 0 && !spec->prob) { msg = W + "n_prob = " + std::to_string(spec->n_prob) + " without prob"; return ST_ERR_USAGE; }
  for (int k = 0; k < spec->n_prob; ++k)
    if (!(spec->prob[k] > 0.0 && spec->prob[k] < 1.0)) { msg = W + "prob " + std::to_string(k) + " must lie strictly inside (0, 1)"; return ST_ERR_USAGE; }
  if (const int rc = check_thresholds(W, spec->n_thr, 0, spec->thr, spec->side, n_thr_values, msg)) return rc;
  if (spec->n_prob == 0 && (rank_q_out(w) || rank_q_out(yhat))) { msg = W + "ess_q needs prob"; return ST_ERR_USAGE; }
  if (spec->n_thr == 0 && (rank_exc_out(w) || rank_exc_out(yhat))) { msg = W + "ess_exc, mcse_prob and prob need thresholds"; return ST_ERR_USAGE; }
  if (K < ST_DIAG_MIN_DRAWS) {
    msg = W + std::to_string(K) + " draws stored, the diagnostics need at least " + std::to_string(ST_DIAG_MIN_DRAWS) +
          " (reserve room before the saved iterations)";
    return ST_ERR_USAGE;
  }
  return ST_OK;
}

// Its own texts (thr[k], side[t] = v, thr_fun before st_points_functionals_set: the callers of st_points_exceed_set read them), so
// not check_thresholds
int check_exceed_spec(const std::string &W, int n_thr, const double *thr, const int32_t *side, const double *thr_fun, long long q,
                      long long n_fun, std::string &msg) {
  if (n_thr < 1 || n_thr > ST_EXC_MAX_THRESHOLDS) {
    msg = W + "n_thr = " + std::to_string(n_thr) + " must lie in 1 .. " + std::to_string(ST_EXC_MAX_THRESHOLDS);
    return ST_ERR_USAGE;
  }
  for (long long k = 0; k < (long long)n_thr * q; ++k)
    if (!std::isfinite(thr[k])) { msg = W + "thr[" + std::to_string(k) + "] is not finite"; return ST_ERR_USAGE; }
  for (int t = 0; side && t < n_thr; ++t)
    if (side[t] != 1 && side[t] != -1) { msg = W + "side[" + std::to_string(t) + "] = " + std::to_string(side[t]) + " is neither +1 nor -1"; return ST_ERR_USAGE; }
  if (thr_fun && n_fun < 0) { msg = W + "thr_fun before st_points_functionals_set"; return ST_ERR_USAGE; }
  for (long long k = 0; thr_fun && k < (long long)n_thr * n_fun; ++k)
    if (!std::isfinite(thr_fun[k])) { msg = W + "thr_fun[" + std::to_string(k) + "] is not finite"; return ST_ERR_USAGE; }
  return ST_OK;
}

int check_chains(const std::string &W, int n_chains, long long K, std::string &msg) {
  if (n_chains < 1 || n_chains > ST_DIAG_MAX_CHAINS) {
    msg = W + "n_chains = " + std::to_string(n_chains) + " must lie in 1 .. " + std::to_string(ST_DIAG_MAX_CHAINS);
    return ST_ERR_USAGE;
  }
  if (K % n_chains != 0) {
    msg = W + std::to_string(K) + " draws stored are not a multiple of n_chains = " + std::to_string(n_chains);
    return ST_ERR_USAGE;
  }
  if (K / n_chains < ST_DIAG_MIN_DRAWS) {
    msg = W + std::to_string(K) + " draws stored in " + std::to_string(n_chains) + " chains are " + std::to_string(K / n_chains) +
          " per chain, the diagnostics need at least " + std::to_string(ST_DIAG_MIN_DRAWS);
    return ST_ERR_USAGE;
  }
  return ST_OK;
}

unsigned thresholds_in_store_order(const double *thr, const int32_t *side, int T, long long stride, bool per_series, const long long *perm,
                                   std::vector<double> &out) {
  unsigned neg = 0;
  out.resize((size_t)T * stride);
  for (int t = 0; t < T; ++t) {
    for (long long j = 0; j < stride; ++j) out[(size_t)t * stride + j] = thr[(size_t)t * stride + ((per_series && perm) ? perm[j] : j)];
    if (side && side[t] < 0) neg |= 1u << t;
  }
  return neg;
}

void mask_in_store_order(const uint8_t *mask, long long n, const long long *perm, std::vector<unsigned char> &out) {
  out.resize((size_t)n);
  for (long long i = 0; i < n; ++i) out[i] = mask[perm ? perm[i] : i] ? 1 : 0;
}

template <typename T>
static void scatter(T *dst, const T *src, long long rows, long long n, const long long *perm) {
  for (long long r = 0; r < rows; ++r)
    for (long long i = 0; i < n; ++i) dst[(size_t)r * n + (perm ? perm[i] : i)] = src[(size_t)r * n + i];
}
void scatter_rows(double *dst, const double *src, long long rows, long long n, const long long *perm) { scatter(dst, src, rows, n, perm); }
void scatter_rows(int32_t *dst, const int32_t *src, long long rows, long long n, const long long *perm) { scatter(dst, src, rows, n, perm); }
void scatter_rows(int64_t *dst, const int64_t *src, long long rows, long long n, const long long *perm) { scatter(dst, src, rows, n, perm); }

int check_mixture_probs(const std::string &W, int n_probs, const double *probs, std::string &msg) {
  if (n_probs < 1 || n_probs > ST_MIX_MAX_PROBS || !probs) {
    msg = W + "n_probs = " + std::to_string(n_probs) + " must lie in 1 .. " + std::to_string(ST_MIX_MAX_PROBS);
    return ST_ERR_USAGE;
  }
  for (int t = 0; t < n_probs; ++t)
    if (!(probs[t] > 0.0 && probs[t] < 1.0)) {   // NaN fails both comparisons
      msg = W + "probs[" + std::to_string(t) + "] = " + std::to_string(probs[t]) + " is not strictly inside (0, 1)";
      return ST_ERR_USAGE;
    }
  return ST_OK;
}
