// Stand-alone check of spamtree_amd/csrc/st_protocol.hpp (the landing area of the iteration's read-backs and the decoding of the
// failure words) with hand-written known answers.  Built and run by tests/test_protocol_cpu.py; the header includes no HIP header,
// so this is host code only and may also be built with -fsanitize=address,undefined.  Prints the first failed check and exits 1;
// prints "protocol ok <count>" and exits 0 otherwise.
#include <cstdio>
#include <vector>

#include "st_protocol.hpp"

// the members of the pinned area do not overlap: a request landing on another's bytes would silently corrupt a Metropolis decision
static_assert(sizeof(Landing) >= 2 * sizeof(double) + 2 * sizeof(int), "a Landing holds two sums and the failure word");
static_assert(offsetof(Landing, err) >= offsetof(Landing, sums) + 2 * sizeof(double), "the failure word lies behind the sums");
static_assert(offsetof(Landing, err) % 4 == 0 && alignof(Landing) % 4 == 0, "the failure word is 4-byte aligned");
static_assert(offsetof(PinnedArea, deferred) >= offsetof(PinnedArea, sweep) + sizeof(Landing), "sweep | deferred");
static_assert(offsetof(PinnedArea, factor) >= offsetof(PinnedArea, deferred) + sizeof(Landing), "deferred | factor");
static_assert(offsetof(PinnedArea, stats) >= offsetof(PinnedArea, factor) + sizeof(Landing), "factor | stats");
static_assert(sizeof(PinnedArea) >= offsetof(PinnedArea, stats) + ST_PIN_STATS * sizeof(double), "stats end inside the area");
static_assert(offsetof(PinnedArea, sweep) % 8 == 0 && offsetof(PinnedArea, deferred) % 8 == 0 && offsetof(PinnedArea, factor) % 8 == 0 &&
                  offsetof(PinnedArea, stats) % 8 == 0, "the sums and the statistics are 8-byte aligned");
static_assert(ST_MAX_RANKS == 64 && ST_PIN_STATS == 40, "the bounds the handle was built with");

static int checks = 0;
#define CHECK(cond)                                                           \
  do {                                                                        \
    checks++;                                                                 \
    if (!(cond)) {                                                            \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);                   \
      return 1;                                                               \
    }                                                                         \
  } while (0)

static Landing landing(int word, double a, double b) {
  Landing L;
  L.err[0] = word; L.sums[0] = a; L.sums[1] = b;
  return L;
}

// rank_failure over `world` ranks, all words zero but words[at[k]] = val[k]
static int ranks(int world, int at0 = -1, double v0 = 0.0, int at1 = -1, double v1 = 0.0) {
  std::vector<double> w(world, 0.0);   // (exactly `world` entries: the sanitizers see a read past them)
  if (at0 >= 0) w[at0] = v0;
  if (at1 >= 0) w[at1] = v1;
  return rank_failure(w.data(), world);
}

int main() {
  // ---- a fresh Landing reports no failure and no sum
  {
    Landing L;
    double ll = -7.0;
    CHECK(L.err[0] == INT_MAX && landing_code(L, &ll) == 0 && ll == 0.0);
  }
  // ---- no failure (INT_MAX): code 0, loglik = sums[0] + sums[1]; a null loglik is allowed
  {
    double ll = 0.0;
    CHECK(landing_code(landing(INT_MAX, 1.5, -4.25), &ll) == 0 && ll == -2.75);
    CHECK(landing_code(landing(INT_MAX, 1.5, -4.25), nullptr) == 0);
  }
  // ---- a failure: the code is the word's low four bits, whatever the level above them; loglik is left alone
  for (int code : {1, 2, 3, 10, 11}) {
    double ll = 123.0;
    CHECK(landing_code(landing(code, 1.0, 2.0), &ll) == code && ll == 123.0);          // level 0
    CHECK(landing_code(landing(7 * 16 + code, 1.0, 2.0), &ll) == code && ll == 123.0);   // level 7
    CHECK(landing_code(landing(code, 1.0, 2.0), nullptr) == code);
  }
  CHECK(landing_code(landing((1 << 20) + 5 * 16 + 3, 0.0, 0.0), nullptr) == 3);   // bits far above the low four
  CHECK(landing_code(landing(0x7ffffff0 + 11, 0.0, 0.0), nullptr) == 11);

  // ---- the ranks' words: none, one, two different ones (the smaller word -- the shallower level -- wins), for 1, 3 and 64 ranks
  for (int world : {1, 3, ST_MAX_RANKS}) {
    const int last = world - 1, mid = world / 2;
    CHECK(ranks(world) == 0);
    CHECK(ranks(world, last, 3 * 16 + 2) == 2);
    CHECK(ranks(world, 0, 5 * 16 + 11) == 11);
    CHECK(ranks(world, mid, 1.0) == 1);                                   // level 0, code 1: the smallest word there is
    if (world == 1) continue;
    CHECK(ranks(world, 0, 6 * 16 + 3, last, 5 * 16 + 2) == 2);            // the smaller word is the later rank's
    CHECK(ranks(world, 0, 5 * 16 + 2, last, 6 * 16 + 3) == 2);            // ... the earlier rank's
    CHECK(ranks(world, mid, 2 * 16 + 11, last, 2 * 16 + 10) == 10);       // same level, two codes
    CHECK(ranks(world, 0, 4 * 16 + 10, mid, 4 * 16 + 10) == 10);          // the same word twice
  }
  std::printf("protocol ok %d\n", checks);
  return 0;
}
