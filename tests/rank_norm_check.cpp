// CPU check of the normal quantile function the rank-normalised diagnostics use (spamtree_amd/csrc/norm_quantile.hpp): built by the
// host compiler alone, it prints, for every K given on the command line (default 4 5 64 1000 16384) and every r2 = 2 .. 2K,
//   K r2 p z
// with p = (4 r2 - 3) / (8 K + 2) and z = st_rank_score(r2, K) as hexadecimal floating-point literals (exact).
// tests/test_rank_diagnostics_cpu.py compares z with 50-digit arithmetic.  A last line "edge" prints the function at 0, 1, 1/2, the
// two region boundaries and outside [0, 1].
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "norm_quantile.hpp"

int main(int argc, char **argv) {
  std::vector<int> Ks;
  for (int a = 1; a < argc; ++a) Ks.push_back(std::atoi(argv[a]));
  if (Ks.empty()) Ks = {4, 5, 64, 1000, 16384};
  for (const int K : Ks) {
    if (K < 1 || K > (1 << 20)) { std::fprintf(stderr, "K = %d out of range\n", K); return 2; }
    for (int r2 = 2; r2 <= 2 * K; ++r2) {
      const double p = (double)(4 * r2 - 3) / (double)(8 * K + 2);
      std::printf("%d %d %a %a\n", K, r2, p, st_rank_score(r2, K));
    }
  }
  const double edge[] = {0.0, 1.0, 0.5, 0.075, 0.925, 1e-20, 1e-12, 1.0 - 1e-12, -0.1, 1.1, 1e-11, 1e-15, 1e-30, 1e-60, 1e-120, 1e-300};
  std::printf("edge");
  for (const double p : edge) std::printf(" %a", st_norm_quantile_f(p));
  std::printf("\n");
  return 0;
}
