// Stand-alone host check of spamtree_amd/csrc/mixture_plan.cpp: mixture_plan_check [lds_limit].  For every K in 1 .. ST_MIX_MAX_DRAWS
// and a list of n, both kernels' plans: R >= 1, the LDS within the limit, every staged row inside the allocation, the grid covers n
// with no empty workgroup; k_mix_crps's group is a whole number of waves that depends on K alone; the refusals of the shape and, from store_spec.cpp,
// of the probabilities.  Built plain and with -fsanitize=address,undefined (tests/test_mixture_cpu.py); no device.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>

#include "draw_store.hpp"
#include "mixture_plan.hpp"

#define REQUIRE(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s (K=%lld n=%lld)\n", __FILE__, __LINE__, #c, K, n); return 1; } } while (0)

int main(int argc, char **argv) {
  const size_t lim = argc > 1 ? (size_t)std::atoll(argv[1]) : 163840;
  const long long ns[] = {1, 2, 3, 5, 7, 8, 9, 63, 64, 65, 301, 1000000, 5000000000ll};
  long long checked = 0, K = 0, n = 0;
  for (K = 1; K <= ST_MIX_MAX_DRAWS; ++K) {
    const size_t row = (size_t)K * 16;
    for (long long nn : ns) {
      n = nn;
      MixPlan Q, C;
      const bool okq = mix_quantile_plan(K, n, lim, &Q);
      REQUIRE(okq == (row <= lim));
      if (okq) {
        REQUIRE(Q.R >= 1 && Q.R <= MIX_Q_MAX_R && Q.G == 64);
        REQUIRE(Q.lds == (size_t)Q.R * row && Q.lds <= lim);
        REQUIRE(Q.grid >= 1 && Q.grid * Q.R >= n && (Q.grid - 1) * Q.R < n);
        REQUIRE(Q.R >= MIX_NT / 64 || (size_t)(Q.R + 1) * row > lim);   // fewer rows than waves only where the limit forces it
      }
      const bool okc = mix_crps_plan(K, n, lim, &C);
      const int G = K <= 64 ? 64 : K <= 128 ? 128 : 256;
      REQUIRE(okc == ((size_t)(MIX_NT / G) * row + MIX_C_RED <= lim));
      if (okc) {
        REQUIRE(C.G == G && C.G % 64 == 0 && C.R * C.G == MIX_NT && C.R >= 1);
        REQUIRE(C.lds == (size_t)C.R * row + MIX_C_RED && C.lds <= lim);
        REQUIRE((size_t)(MIX_NT / 64) * 3 * sizeof(double) <= MIX_C_RED);
        REQUIRE(C.grid >= 1 && C.grid * C.R >= n && (C.grid - 1) * C.R < n);
      }
      ++checked;
    }
  }
  {
    MixPlan P;
    K = 0; n = 1;
    REQUIRE(!mix_quantile_plan(0, 1, lim, &P) && !mix_crps_plan(0, 1, lim, &P));
    REQUIRE(!mix_quantile_plan(ST_MIX_MAX_DRAWS + 1, 1, lim, &P) && !mix_crps_plan(ST_MIX_MAX_DRAWS + 1, 1, lim, &P));
    REQUIRE(!mix_quantile_plan(5, 0, lim, &P) && !mix_crps_plan(5, 0, lim, &P));
    REQUIRE(mix_crps_pairs(1) == 0.0 && mix_crps_pairs(1000) == 499500.0);
    REQUIRE(mix_store_bytes(10, true, 2, 3) == 240.0 + 16.0 + 48.0 && mix_store_bytes(10, false, 1, 0) == 168.0);
    std::string msg;
    const double good[8] = {0.5, 1e-6, 0.975, 0.025, 0.999999, 0.1, 0.2, 0.3};
    REQUIRE(check_mixture_probs("w: ", 8, good, msg) == ST_OK && check_mixture_probs("w: ", 1, good, msg) == ST_OK);
    REQUIRE(check_mixture_probs("w: ", 0, good, msg) == ST_ERR_USAGE && check_mixture_probs("w: ", 9, good, msg) == ST_ERR_USAGE);
    REQUIRE(check_mixture_probs("w: ", 1, nullptr, msg) == ST_ERR_USAGE);
    const double bad[] = {0.0, 1.0, -0.1, 1.5, std::nan(""), std::numeric_limits<double>::infinity()};
    for (double b : bad) {
      const double pr[3] = {0.5, 0.25, b};
      REQUIRE(check_mixture_probs("w: ", 3, pr, msg) == ST_ERR_USAGE && msg.find("probs[2]") != std::string::npos);
    }
  }
  std::printf("OK %lld plans under an LDS limit of %zu\n", checked, lim);
  return 0;
}
