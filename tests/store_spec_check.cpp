// store_spec_check -- a stand-alone CPU program: the pure host helpers of the summaries of the stored draws
// (spamtree_amd/csrc/store_spec.cpp) against plain loops written here.  The loops go the other way round: the helpers gather by
// perm, the checks walk the caller's indices c and look at the store position inv[c], inv built here.  Every input array has
// exactly the size its helper may read, so the sanitizer build sees any step past an end.
// Prints "OK key=value ..." or the first violated property (exit status 1).
//
//   store_spec_check [swap]
//
// swap: the negative case -- two thresholds of one store-order array exchanged before it is checked; the checks must name it.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>

#include "draw_store.hpp"

[[noreturn]] static void violated(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  printf("VIOLATED ");
  vprintf(fmt, ap);
  printf("\n");
  va_end(ap);
  exit(1);
}
#define REQUIRE(cond, ...) do { if (!(cond)) violated(__VA_ARGS__); } while (0)

static long long n_thr_cases = 0, n_mask_cases = 0, n_scatter_cases = 0, n_neg_cases = 0, n_refusals = 0;

// kind 0: no perm; 1: identity; 2: reversal; 3: random
static std::vector<long long> make_perm(int kind, long long n) {
  std::vector<long long> p((size_t)n);
  for (long long i = 0; i < n; ++i) p[i] = kind == 2 ? n - 1 - i : i;
  if (kind == 3) {
    std::mt19937_64 rng(1234 + (unsigned)n);
    for (long long i = n - 1; i > 0; --i) std::swap(p[i], p[(long long)(rng() % (unsigned long long)(i + 1))]);
  }
  return p;
}

static void check_thresholds_in_order(long long n, int T, int G, int kind, bool per_series, bool swap) {
  const std::vector<long long> perm = make_perm(kind, n);
  const long long *pp = kind ? perm.data() : nullptr;
  std::vector<long long> inv((size_t)n);
  for (long long i = 0; i < n; ++i) inv[kind ? perm[i] : i] = i;
  const long long stride = per_series ? n : G;
  std::vector<double> thr((size_t)T * stride);
  for (size_t k = 0; k < thr.size(); ++k) thr[k] = 0.5 + (double)k;   // all different
  // the sides: none given, all +1, and exactly one -1 at every t in turn
  for (int tneg = -2; tneg < T; ++tneg) {
    std::vector<int32_t> side((size_t)T, 1);
    if (tneg >= 0) side[tneg] = -1;
    std::vector<double> out(3, -1.0);   // (whatever it held goes)
    const unsigned neg = thresholds_in_store_order(thr.data(), tneg == -2 ? nullptr : side.data(), T, stride, per_series, pp, out);
    REQUIRE(neg == (tneg >= 0 ? 1u << tneg : 0u), "neg: n %lld T %d G %d perm %d per_series %d tneg %d: mask %u", n, T, G, kind, (int)per_series, tneg, neg);
    REQUIRE(out.size() == thr.size(), "thresholds: n %lld T %d: %zu values for %zu", n, T, out.size(), thr.size());
    if (swap && n == 5 && T == 8 && kind == 2 && per_series && tneg == 0) std::swap(out[0], out[1]);
    for (int t = 0; t < T; ++t)
      for (long long c = 0; c < stride; ++c) {
        const long long at = per_series ? inv[c] : c;   // thresholds per domain stay where they are
        REQUIRE(out[(size_t)t * stride + at] == thr[(size_t)t * stride + c],
                "thresholds: n %lld T %d G %d perm %d per_series %d: threshold %d of caller index %lld not at store position %lld", n, T, G, kind,
                (int)per_series, t, c, at);
      }
    ++n_neg_cases;
  }
  ++n_thr_cases;
}

static void check_mask(long long n, int kind) {
  const std::vector<long long> perm = make_perm(kind, n);
  std::vector<uint8_t> mask((size_t)n);
  const uint8_t vals[3] = {0, 1, 255};
  for (long long c = 0; c < n; ++c) mask[c] = vals[(c * 7 + 3) % 3];
  std::vector<unsigned char> out(2, 9);
  mask_in_store_order(mask.data(), n, kind ? perm.data() : nullptr, out);
  REQUIRE((long long)out.size() == n, "mask: n %lld: %zu entries", n, out.size());
  for (long long i = 0; i < n; ++i) {
    const long long c = kind ? perm[i] : i;
    REQUIRE(out[i] == (mask[c] ? 1 : 0), "mask: n %lld perm %d: store position %lld holds %d, caller index %lld holds %d", n, kind, i, (int)out[i], c, (int)mask[c]);
  }
  ++n_mask_cases;
}

template <typename V>
static void check_scatter(long long n, long long rows, int kind, const char *type) {
  const std::vector<long long> perm = make_perm(kind, n);
  const long long *pp = kind ? perm.data() : nullptr;
  const V sentinel = (V)-7;
  std::vector<V> src((size_t)(rows * n)), dst((size_t)(rows * n), sentinel);
  for (size_t k = 0; k < src.size(); ++k) src[k] = (V)(k + 1);   // all different, none the sentinel
  if (rows == 0) {   // nothing may be touched: n entries stand behind the pointers
    std::vector<V> s0((size_t)n, (V)3), d0((size_t)n, sentinel);
    scatter_rows(d0.data(), s0.data(), 0, n, pp);
    for (long long i = 0; i < n; ++i) REQUIRE(d0[i] == sentinel, "scatter %s: rows 0 wrote index %lld", type, i);
  } else {
    scatter_rows(dst.data(), src.data(), rows, n, pp);
  }
  // every destination holds the one source value that belongs there: rows * n different values on rows * n places, so each place
  // was written exactly once
  std::vector<char> seen(src.size() + 1, 0);
  for (long long r = 0; r < rows; ++r)
    for (long long i = 0; i < n; ++i) {
      const long long c = kind ? perm[i] : i;
      const V v = dst[(size_t)(r * n + c)];
      REQUIRE(v == src[(size_t)(r * n + i)], "scatter %s: n %lld rows %lld perm %d: row %lld, store position %lld not at index %lld", type, n, rows, kind, r, i, c);
      REQUIRE(!seen[(size_t)v], "scatter %s: value %lld twice", type, (long long)v);
      seen[(size_t)v] = 1;
    }
  ++n_scatter_cases;
}

static void refused(int rc, const std::string &msg, const char *text) {
  REQUIRE(rc == ST_ERR_USAGE && msg.find(text) != std::string::npos && msg.rfind("who: ", 0) == 0, "refusal \"%s\": code %d, text \"%s\"", text, rc, msg.c_str());
  ++n_refusals;
}

static void check_refusals() {
  const double nan = std::nan(""), inf = std::numeric_limits<double>::infinity();
  const std::string W = "who: ";
  std::string msg = "untouched";
  const double good[6] = {0.0, 1.0, -2.0, 3.5, 1e300, -1e300};
  const int32_t sides[3] = {1, -1, 1};
  REQUIRE(check_thresholds(W, 3, 1, good, sides, 2, msg) == ST_OK && msg == "untouched", "a good spec is refused: %s", msg.c_str());
  REQUIRE(check_thresholds(W, 3, 1, good, nullptr, 2, msg) == ST_OK, "no sides is refused: %s", msg.c_str());
  REQUIRE(check_thresholds(W, 0, 0, nullptr, nullptr, 2, msg) == ST_OK, "no thresholds where none are needed is refused: %s", msg.c_str());
  REQUIRE(check_thresholds(W, ST_EXC_MAX_THRESHOLDS, 1, std::vector<double>(ST_EXC_MAX_THRESHOLDS * 3, 0.25).data(), nullptr, 3, msg) == ST_OK, "the largest count is refused");
  for (int at = 0; at < 6; ++at)
    for (const double bad : {nan, inf, -inf}) {
      double v[6];
      std::memcpy(v, good, sizeof(v));
      v[at] = bad;
      refused(check_thresholds(W, 3, 1, v, sides, 2, msg), msg, ("threshold " + std::to_string(at) + " is not finite").c_str());
    }
  for (int at = 0; at < 3; ++at)
    for (const int32_t bad : {0, 2, -2}) {
      int32_t s[3] = {1, -1, 1};
      s[at] = bad;
      refused(check_thresholds(W, 3, 1, good, s, 2, msg), msg, ("side " + std::to_string(at) + " must be +1 or -1").c_str());
    }
  refused(check_thresholds(W, -1, 0, good, sides, 2, msg), msg, "n_thr = -1 must lie in 0 .. 8");
  refused(check_thresholds(W, -1, 1, good, sides, 2, msg), msg, "n_thr = -1 must lie in 1 .. 8");
  refused(check_thresholds(W, 0, 1, good, sides, 2, msg), msg, "n_thr = 0 must lie in 1 .. 8");
  refused(check_thresholds(W, ST_EXC_MAX_THRESHOLDS + 1, 0, good, sides, 2, msg), msg, "n_thr = 9 must lie in 0 .. 8");   // (before any value is read)
  refused(check_thresholds(W, ST_EXC_MAX_THRESHOLDS + 1, 1, good, sides, 2, msg), msg, "n_thr = 9 must lie in 1 .. 8");
  refused(check_thresholds(W, 2, 0, nullptr, sides, 2, msg), msg, "n_thr = 2 without thr");
  // the count before the values, the values before the sides
  double v[6];
  std::memcpy(v, good, sizeof(v));
  v[5] = nan;
  const int32_t s0[3] = {0, 1, 1};
  refused(check_thresholds(W, 3, 1, v, s0, 2, msg), msg, "threshold 5 is not finite");
}

// the whole texts of the three spec checkers, each refusal in its order; every buffer holds exactly n_thr x n_values values
static void exact(int rc, const std::string &msg, int code, const std::string &text) {
  REQUIRE(rc == code && msg == "who: " + text, "refusal \"%s\": code %d, text \"%s\"", text.c_str(), rc, msg.c_str());
  ++n_refusals;
}

static void check_spec_refusals() {
  const double nan = std::nan("");
  const std::string W = "who: ";
  std::string msg = "untouched";
  double sink[1];
  int32_t isink[1];
  const std::vector<double> thr6 = {0.0, 1.0, 2.0, 3.0, 4.0, 5.0};   // 3 thresholds x 2 values
  const int32_t sides[3] = {1, -1, 1};
  {   // the excursion spec
    st_excursion_spec sp{};
    st_excursion_out w{}, y{};
    exact(check_excursion_spec(W, nullptr, 5, 2, &w, &y, msg), msg, ST_ERR_USAGE, "no spec");
    exact(check_excursion_spec(W, &sp, 5, 2, &w, nullptr, msg), msg, ST_ERR_USAGE, "the spec holds neither thresholds nor a band request");
    w.count = isink;
    sp.want_band = 1;
    exact(check_excursion_spec(W, &sp, 5, 2, nullptr, &w, msg), msg, ST_ERR_USAGE, "count, prob, excur and joint_all need thresholds");
    sp.thr = thr6.data();
    sp.side = sides;
    sp.n_thr = 0;
    exact(check_excursion_spec(W, &sp, 5, 2, &w, &y, msg), msg, ST_ERR_USAGE, "n_thr = 0 must lie in 1 .. 8");
    sp.n_thr = ST_EXC_MAX_THRESHOLDS + 1;   // (refused before any of the 9 x 2 values is read)
    exact(check_excursion_spec(W, &sp, 5, 2, &w, &y, msg), msg, ST_ERR_USAGE, "n_thr = 9 must lie in 1 .. 8");
    sp.n_thr = 3;
    std::vector<double> bad = thr6;
    bad[4] = nan;
    sp.thr = bad.data();
    exact(check_excursion_spec(W, &sp, 0, 2, &w, &y, msg), msg, ST_ERR_USAGE, "threshold 4 is not finite");   // (before the count of draws)
    sp.thr = thr6.data();
    const int32_t s0[3] = {1, 1, 0};
    sp.side = s0;
    exact(check_excursion_spec(W, &sp, 0, 2, &w, &y, msg), msg, ST_ERR_USAGE, "side 2 must be +1 or -1");
    sp.side = sides;
    exact(check_excursion_spec(W, &sp, 0, 2, &w, &y, msg), msg, ST_ERR_USAGE, "no draw stored (reserve room before the saved iterations)");
    exact(check_excursion_spec(W, &sp, 1, 2, &w, &y, msg), msg, ST_ERR_USAGE, "the band needs at least 2 stored draws, 1 stored");
    sp.want_band = 0;
    y.maxdev = sink;   // a band output asks for the band as want_band does
    exact(check_excursion_spec(W, &sp, 1, 2, &w, &y, msg), msg, ST_ERR_USAGE, "the band needs at least 2 stored draws, 1 stored");
    msg = "untouched";
    REQUIRE(check_excursion_spec(W, &sp, 2, 2, &w, &y, msg) == ST_OK && msg == "untouched", "a good excursion spec is refused: %s", msg.c_str());
    y.maxdev = nullptr;
    REQUIRE(check_excursion_spec(W, &sp, 1, 2, &w, &y, msg) == ST_OK, "thresholds alone on one draw are refused: %s", msg.c_str());
  }
  {   // the rank spec
    st_rank_spec sp{};
    st_rank_out w{}, y{};
    const long long K = ST_DIAG_MIN_DRAWS;
    exact(check_rank_spec(W, nullptr, K, 2, &w, &y, msg), msg, ST_ERR_USAGE, "no spec");
    sp.max_lag = -1;
    exact(check_rank_spec(W, &sp, K, 2, &w, &y, msg), msg, ST_ERR_USAGE, "max_lag must not be negative (0: the default cap)");
    sp.max_lag = 0;
    for (const int n : {-1, ST_RANK_MAX_PROBS + 1}) {
      sp.n_prob = n;
      exact(check_rank_spec(W, &sp, K, 2, &w, &y, msg), msg, ST_ERR_USAGE, "n_prob = " + std::to_string(n) + " must lie in 0 .. " + std::to_string(ST_RANK_MAX_PROBS));
    }
    sp.n_prob = 2;
    exact(check_rank_spec(W, &sp, K, 2, &w, &y, msg), msg, ST_ERR_USAGE, "n_prob = 2 without prob");
    for (const double bad : {0.0, 1.0, nan}) {
      const double prob[2] = {0.5, bad};
      sp.prob = prob;
      sp.n_thr = ST_EXC_MAX_THRESHOLDS + 1;   // all of prob before the thresholds
      exact(check_rank_spec(W, &sp, K, 2, &w, &y, msg), msg, ST_ERR_USAGE, "prob 1 must lie strictly inside (0, 1)");
    }
    const double prob[2] = {0.05, 0.95};
    sp.prob = prob;
    sp.thr = thr6.data();
    exact(check_rank_spec(W, &sp, K, 2, &w, &y, msg), msg, ST_ERR_USAGE, "n_thr = 9 must lie in 0 .. 8");
    sp.n_thr = -1;
    exact(check_rank_spec(W, &sp, K, 2, &w, &y, msg), msg, ST_ERR_USAGE, "n_thr = -1 must lie in 0 .. 8");
    sp.n_thr = 3;
    sp.thr = nullptr;
    exact(check_rank_spec(W, &sp, K, 2, &w, &y, msg), msg, ST_ERR_USAGE, "n_thr = 3 without thr");
    std::vector<double> bad = thr6;
    bad[5] = nan;
    sp.thr = bad.data();
    exact(check_rank_spec(W, &sp, K, 2, &w, &y, msg), msg, ST_ERR_USAGE, "threshold 5 is not finite");
    sp.thr = thr6.data();
    const int32_t s0[3] = {-2, 1, 1};
    sp.side = s0;
    exact(check_rank_spec(W, &sp, K, 2, &w, &y, msg), msg, ST_ERR_USAGE, "side 0 must be +1 or -1");
    sp.side = sides;
    sp.n_prob = 0;
    y.ess_q = sink;
    exact(check_rank_spec(W, &sp, K, 2, &w, &y, msg), msg, ST_ERR_USAGE, "ess_q needs prob");
    sp.n_prob = 2;
    sp.n_thr = 0;
    for (int which = 0; which < 3; ++which) {
      st_rank_out o{};
      (which == 0 ? o.ess_exc : which == 1 ? o.mcse_prob : o.prob) = sink;
      exact(check_rank_spec(W, &sp, K, 2, &o, &y, msg), msg, ST_ERR_USAGE, "ess_exc, mcse_prob and prob need thresholds");
    }
    sp.n_thr = 3;
    exact(check_rank_spec(W, &sp, K - 1, 2, &w, &y, msg), msg, ST_ERR_USAGE,
          std::to_string(K - 1) + " draws stored, the diagnostics need at least " + std::to_string(K) + " (reserve room before the saved iterations)");
    msg = "untouched";
    REQUIRE(check_rank_spec(W, &sp, K, 2, &w, &y, msg) == ST_OK && msg == "untouched", "a good rank spec is refused: %s", msg.c_str());
    const st_rank_spec none{};
    REQUIRE(check_rank_spec(W, &none, K, 2, &w, nullptr, msg) == ST_OK, "an empty rank spec is refused: %s", msg.c_str());
  }
  {   // the exceedance spec: thr 3 x q = 2, thr_fun 3 x n_fun = 1
    const std::vector<double> tf3 = {0.5, 1.5, 2.5};
    for (const int n : {-1, 0, ST_EXC_MAX_THRESHOLDS + 1})   // (before any of the n x 2 values is read)
      exact(check_exceed_spec(W, n, thr6.data(), sides, tf3.data(), 2, 1, msg), msg, ST_ERR_USAGE, "n_thr = " + std::to_string(n) + " must lie in 1 .. 8");
    std::vector<double> bad = thr6;
    bad[3] = nan;
    const int32_t s0[3] = {1, 0, 1};
    exact(check_exceed_spec(W, 3, bad.data(), s0, tf3.data(), 2, -1, msg), msg, ST_ERR_USAGE, "thr[3] is not finite");
    exact(check_exceed_spec(W, 3, thr6.data(), s0, tf3.data(), 2, -1, msg), msg, ST_ERR_USAGE, "side[1] = 0 is neither +1 nor -1");
    exact(check_exceed_spec(W, 3, thr6.data(), sides, tf3.data(), 2, -1, msg), msg, ST_ERR_USAGE, "thr_fun before st_points_functionals_set");
    std::vector<double> badf = tf3;
    badf[2] = std::numeric_limits<double>::infinity();
    exact(check_exceed_spec(W, 3, thr6.data(), sides, badf.data(), 2, 1, msg), msg, ST_ERR_USAGE, "thr_fun[2] is not finite");
    msg = "untouched";
    REQUIRE(check_exceed_spec(W, 3, thr6.data(), sides, tf3.data(), 2, 1, msg) == ST_OK && msg == "untouched", "a good exceedance spec is refused: %s", msg.c_str());
    REQUIRE(check_exceed_spec(W, 3, thr6.data(), nullptr, nullptr, 2, -1, msg) == ST_OK, "no sides and no thr_fun are refused: %s", msg.c_str());
  }
}

int main(int argc, char **argv) {
  const bool swap = argc > 1 && !strcmp(argv[1], "swap");
  for (const long long n : {1ll, 5ll, 64ll, 65ll})
    for (int kind = 0; kind < 4; ++kind) {
      for (const int T : {0, 1, 8}) {   // T = 0, the band-only excursions: no threshold array, the mask and the scatter alone
        for (const int G : {1, 3})
          for (int per = 0; per < 2 && T > 0; ++per) check_thresholds_in_order(n, T, G, kind, per != 0, swap);
        for (const long long rows : {(long long)T, 1ll}) {
          check_scatter<double>(n, rows, kind, "double");
          check_scatter<int32_t>(n, rows, kind, "int32");
          check_scatter<int64_t>(n, rows, kind, "int64");
        }
      }
      check_mask(n, kind);
    }
  check_refusals();
  check_spec_refusals();
  printf("OK thresholds=%lld sides=%lld masks=%lld scatters=%lld refusals=%lld\n", n_thr_cases, n_neg_cases, n_mask_cases, n_scatter_cases, n_refusals);
  return 0;
}
