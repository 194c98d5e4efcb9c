// Host-only check of spamtree_amd/csrc/psis_plan.cpp (no GPU): the tile plan of k_loo_psis, the tail length and the refusals of the
// store's bookkeeping.  Prints "OK <n checks>" or the first failure.  tests/test_psis_cpu.py compiles and runs it.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "psis_plan.hpp"

static int n_checks = 0;
#define CHECK(c)                                                            \
  do {                                                                      \
    ++n_checks;                                                             \
    if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); return 1; } \
  } while (0)

int main(int argc, char **argv) {
  const size_t lds_limit = argc > 1 ? (size_t)std::atoll(argv[1]) : 160 * 1024;
  // the tail length against the defining inequality, every S
  for (long long S = 1; S <= PSIS_MAX_DRAWS; ++S) {
    const int M = psis_tail_length(S);
    long long m = 0;
    while (m * m < 9 * S) ++m;
    CHECK(m * m >= 9 * S && (m == 0 || (m - 1) * (m - 1) < 9 * S));
    CHECK(M == (S / 5 < m ? S / 5 : m));
    CHECK(M <= PSIS_MAX_TAIL && M < S);
    int g = 0;
    while ((g + 1) * (g + 1) <= M) ++g;   // isqrt(M): the grid of the fit
    CHECK(30 + g <= PSIS_MAX_GRID);
  }
  CHECK(psis_tail_length(PSIS_MAX_DRAWS) == PSIS_MAX_TAIL && psis_tail_length(24) == 4 && psis_tail_length(25) == 5 && psis_tail_length(0) == 0);
  // the plan: every K fits the limit it is planned under, R rows of Kpad and R tails, Kpad the power of two at or above K
  for (long long K = 1; K <= PSIS_MAX_DRAWS; ++K) {
    int R = -1, Kpad = -1;
    const bool ok = psis_plan(K, lds_limit, &R, &Kpad);
    size_t kp = 2;
    while ((long long)kp < K) kp <<= 1;
    if (psis_lds_bytes(1, (int)kp) + PSIS_LDS_STATIC > lds_limit) { CHECK(!ok); continue; }
    CHECK(ok && Kpad == (int)kp && R >= 1 && R <= PSIS_MAX_R);
    CHECK(psis_lds_bytes(R, Kpad) + PSIS_LDS_STATIC <= lds_limit);
    CHECK(psis_lds_bytes(R, Kpad) == (size_t)R * ((size_t)Kpad + PSIS_MAX_TAIL) * 8);
    CHECK(R == PSIS_MAX_R || psis_lds_bytes(R + 1, Kpad) > PSIS_TILE || psis_lds_bytes(R + 1, Kpad) + PSIS_LDS_STATIC > lds_limit);
  }
  {
    int R = 0, Kpad = 0;
    CHECK(!psis_plan(0, lds_limit, &R, &Kpad) && !psis_plan(PSIS_MAX_DRAWS + 1, lds_limit, &R, &Kpad) && !psis_plan(100, 512, &R, &Kpad));
    CHECK(psis_plan(64, 160 * 1024, &R, &Kpad) && R == PSIS_MAX_R && Kpad == 64);
    CHECK(psis_plan(16384, 160 * 1024, &R, &Kpad) && R == 1 && Kpad == 16384);
    CHECK(!psis_plan(16384, 64 * 1024, &R, &Kpad));
  }
  // the grid: every tile has a workgroup until the cap
  CHECK(psis_grid(1, 8) == 1 && psis_grid(8, 8) == 1 && psis_grid(9, 8) == 2 && psis_grid(300, 8) == 38);
  CHECK(psis_grid(100000000ll, 1) == PSIS_MAX_WGS && psis_grid(0, 4) == 1);
  // the refusals carry both numbers
  std::string msg;
  CHECK(psis_check_draws("who", "keep", 1, msg) == ST_OK && psis_check_draws("who", "keep", PSIS_MAX_DRAWS, msg) == ST_OK && msg.empty());
  CHECK(psis_check_draws("who", "keep", 16385, msg) == ST_ERR_UNSUPPORTED);
  CHECK(msg.find("16385") != std::string::npos && msg.find("16384") != std::string::npos && msg.find("who") == 0);
  CHECK(psis_check_draws("who", "K", 0, msg) == ST_ERR_UNSUPPORTED && psis_check_draws("who", "K", -3, msg) == ST_ERR_UNSUPPORTED);
  msg.clear();
  CHECK(psis_check_column("acc", 5, 0, msg) == ST_OK && psis_check_column("acc", 29, 30, msg) == ST_OK && msg.empty());
  CHECK(psis_check_column("acc", 30, 30, msg) == ST_ERR_USAGE && msg.find("30") != std::string::npos);
  CHECK(psis_store_bytes(1000, 1000000) == 24e9);
  std::printf("OK %d\n", n_checks);
  return 0;
}
