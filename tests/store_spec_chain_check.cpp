// store_spec_chain_check.cpp -- check_chains (spamtree_amd/csrc/store_spec.cpp) against the rule restated here, on the CPU: every
// n_chains in -2 .. 19 with every K in 0 .. 300 and the store's limits (16380 .. 16384), the code, and for a refusal the check
// that failed first and the numbers in its text.  Prints "OK accepted=.. refused=.. ranges=.. multiples=.. short=.."; with the
// argument "late" the rule restated here lets N = 3 through, which must be reported (the check can fail).
#include <cstdio>
#include <cstring>
#include <string>

#include "draw_store.hpp"

static bool has(const std::string &s, const std::string &part) { return s.find(part) != std::string::npos; }

int main(int argc, char **argv) {
  const int min_draws = (argc > 1 && !std::strcmp(argv[1], "late")) ? ST_DIAG_MIN_DRAWS - 1 : ST_DIAG_MIN_DRAWS;
  long long accepted = 0, refused = 0, ranges = 0, multiples = 0, shorts = 0;
  for (int M = -2; M <= ST_DIAG_MAX_CHAINS + 3; ++M) {
    for (long long K = 0; K <= 16384; K = (K == 300 ? 16380 : K + 1)) {
      std::string msg = "untouched";
      const int rc = check_chains("who: ", M, K, msg);
      int want = ST_OK;
      std::string part;
      if (M < 1 || M > ST_DIAG_MAX_CHAINS) { want = ST_ERR_USAGE; part = "n_chains = " + std::to_string(M) + " must lie in 1 .. 16"; ++ranges; }
      else if (K % M) { want = ST_ERR_USAGE; part = std::to_string(K) + " draws stored are not a multiple of n_chains = " + std::to_string(M); ++multiples; }
      else if (K / M < min_draws) {
        want = ST_ERR_USAGE;
        part = std::to_string(K) + " draws stored in " + std::to_string(M) + " chains are " + std::to_string(K / M) + " per chain";
        ++shorts;
      }
      if (rc != want) { std::printf("VIOLATED code: n_chains %d K %lld gives %d, not %d\n", M, K, rc, want); return 1; }
      if (want == ST_OK) {
        if (msg != "untouched") { std::printf("VIOLATED text: n_chains %d K %lld is accepted with a text\n", M, K); return 1; }
        ++accepted;
      } else {
        if (!has(msg, "who: ") || !has(msg, part)) { std::printf("VIOLATED text: n_chains %d K %lld says '%s'\n", M, K, msg.c_str()); return 1; }
        ++refused;
      }
    }
  }
  std::printf("OK accepted=%lld refused=%lld ranges=%lld multiples=%lld short=%lld\n", accepted, refused, ranges, multiples, shorts);
  return 0;
}
