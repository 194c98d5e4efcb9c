// psis_plan.hpp's functions: host only, no HIP.
#include "psis_plan.hpp"
#include "series_tile.hpp"

#include <algorithm>

int psis_tail_length(long long S) {
  if (S <= 0) return 0;
  long long m = 0;
  while (m * m < 9 * S) ++m;   // S <= 16384: at most 384 steps, integers only
  return (int)std::min(S / 5, m);
}

size_t psis_lds_bytes(int R, int Kpad) { return (size_t)R * ((size_t)Kpad + PSIS_MAX_TAIL) * sizeof(double); }

bool psis_plan(long long K, size_t lds_limit, int *R, int *Kpad) {
  if (K < 1 || K > PSIS_MAX_DRAWS) return false;
  const size_t kpad = (size_t)tile_pow2(K);
  const size_t lim = lds_limit > PSIS_LDS_STATIC ? lds_limit - PSIS_LDS_STATIC : 0;
  const size_t per = psis_lds_bytes(1, (int)kpad);
  size_t r = std::min<size_t>(lim, PSIS_TILE) / per;
  if (r < 1) r = lim / per;   // a long series: what the device allows
  if (r < 1) return false;
  *R = (int)std::min<size_t>(r, PSIS_MAX_R);
  *Kpad = (int)kpad;
  return true;
}

long long psis_grid(long long n, int R) {
  const long long ntiles = (n + R - 1) / R;
  return std::max(1ll, std::min<long long>(ntiles, PSIS_MAX_WGS));
}

int psis_check_draws(const char *who, const char *what, long long K, std::string &msg) {
  if (K >= 1 && K <= PSIS_MAX_DRAWS) return ST_OK;
  msg = std::string(who) + ": " + what + " = " + std::to_string(K) + " must lie in 1 .. " + std::to_string(PSIS_MAX_DRAWS);
  return ST_ERR_UNSUPPORTED;
}

int psis_check_column(const char *who, long long col, long long keep, std::string &msg) {
  if (keep == 0 || col < keep) return ST_OK;
  msg = std::string(who) + ": the store of st_rows_loo_reserve holds " + std::to_string(keep) + " draws and " + std::to_string(col) +
        " are accumulated";
  return ST_ERR_USAGE;
}

double psis_store_bytes(long long keep, long long n) { return 3.0 * 8.0 * (double)keep * (double)n; }
