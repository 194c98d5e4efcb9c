// store_spec.cpp -- the pure host helpers of the summaries of the stored draws (draw_store.hpp): what the excursion and the rank
// spec share of their checks, the small inputs brought into store order and the device results scattered into the caller's
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
