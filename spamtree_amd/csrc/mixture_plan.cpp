// mixture_plan.hpp's functions: host only, no HIP.
#include "mixture_plan.hpp"

#include <algorithm>

static bool mix_shape_ok(long long K, long long n) { return K >= 1 && K <= MIX_MAX_DRAWS && n >= 1; }

bool mix_quantile_plan(long long K, long long n, size_t lds_limit, MixPlan *P) {
  if (!mix_shape_ok(K, n)) return false;
  const size_t per = (size_t)K * 2 * sizeof(double);
  if (per > lds_limit) return false;
  size_t r = std::min<size_t>(MIX_Q_MAX_R, std::max<size_t>(MIX_NT / 64, MIX_Q_TILE / per));
  r = std::min(r, lds_limit / per);
  P->R = (int)r;
  P->G = 64;
  P->lds = r * per;
  P->grid = (n + (long long)r - 1) / (long long)r;
  return true;
}

bool mix_crps_plan(long long K, long long n, size_t lds_limit, MixPlan *P) {
  if (!mix_shape_ok(K, n)) return false;
  const int G = K <= 64 ? 64 : K <= 128 ? 128 : MIX_NT;
  const int R = MIX_NT / G;
  const size_t lds = (size_t)R * K * 2 * sizeof(double) + MIX_C_RED;
  if (lds > lds_limit) return false;
  P->R = R;
  P->G = G;
  P->lds = lds;
  P->grid = (n + R - 1) / R;
  return true;
}

double mix_crps_pairs(long long K) { return 0.5 * (double)K * (double)(K - 1); }

double mix_store_bytes(long long n, bool has_X, int q, long long n_fun) {
  return (has_X ? 24.0 : 16.0) * (double)n + 8.0 * (double)q + 16.0 * (double)n_fun;
}
