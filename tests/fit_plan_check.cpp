// fit_plan_check -- a stand-alone CPU program: the plan step of stm_mcmc_fit (spamtree_amd/csrc/fit_plan.cpp with the spec
// checkers of store_spec.cpp) on requests built here.  It needs no device: the plan reads the request alone.  Every array has
// exactly the size the plan may read, so the sanitizer build sees any step past an end, and a NULL pb any read through it.
// Prints "OK key=value ..." or the first violated property (exit status 1).
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fit_plan.hpp"

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

static long long n_accepted = 0, n_refused = 0, n_null_pb = 0, n_texts = 0;
static double sink[4];   // where an output pointer points: the plan never writes through one

// A run of q outcomes that keeps `keep` draws; pb only carries q
static st_problem g_pb;
static const double g_theta[2] = {1.0, 0.5};
static stm_fit request(int q, int keep) {
  g_pb = st_problem{};
  g_pb.q = q;
  stm_fit f{};
  f.run.pb = &g_pb;
  f.run.theta = g_theta;
  f.run.ntheta = 2;
  f.run.mcmc_keep = keep;
  f.run.mcmc_thin = 1;
  return f;
}
// A point set of one point (coords only)
static const double g_coords[2] = {0.25, 0.75};
static const int64_t g_mv[1] = {1};
static stm_new_points one_point() {
  stm_new_points p{};
  p.n_new = 1;
  p.coords_new = g_coords;
  p.mv_new = g_mv;
  return p;
}

struct Got {
  int rc;
  std::string text, which;
};
static Got plan(const stm_fit &f, FitPlan &pl) {
  Got g;
  g.text = g.which = "stale";
  g.rc = fit_plan(f, pl, g.text, g.which);
  return g;
}
static void accepted(const char *name, const Got &g) {
  REQUIRE(g.rc == ST_OK && g.text.empty() && g.which.empty(), "%s: refused with %d, \"%s\", \"%s\"", name, g.rc, g.text.c_str(), g.which.c_str());
  ++n_accepted;
}
// refused with `code`; which begins with `which`; text is the reported text: "" or, with loud, the rest of which after its part
static void refused(const char *name, const stm_fit &f, int code, const char *which, bool loud = false) {
  FitPlan pl;
  const Got g = plan(f, pl);
  ++n_refused;
  REQUIRE(g.rc == code && g.which.rfind(which, 0) == 0, "%s: code %d for %d, \"%s\" does not begin with \"%s\"", name, g.rc, code, g.which.c_str(), which);
  if (loud) {
    const size_t at = g.which.find(": ");
    REQUIRE(!g.text.empty() && at != std::string::npos && g.which.substr(at + 2) == g.text, "%s: text \"%s\" beside \"%s\"", name, g.text.c_str(), g.which.c_str());
    ++n_texts;
  } else {
    REQUIRE(g.text.empty(), "%s: a text where none is reported: \"%s\"", name, g.text.c_str());
  }
}

static void check_accepted() {
  {   // the plain fit
    const stm_fit f = request(2, 5);
    FitPlan pl;
    accepted("plain", plan(f, pl));
    REQUIRE(pl.M == 1 && pl.total == 5 && !pl.f.pts && !pl.f.fun && !pl.f.scores && !pl.rb && !pl.crps && !pl.store_rows && pl.cov_len == 0,
            "plain: M %d total %lld", pl.M, pl.total);
    REQUIRE(!pl.d.any() && !pl.e.any() && !pl.k.any(), "plain: something is wanted");
  }
  for (int with_coords = 0; with_coords < 2; ++with_coords) {   // a rows summary beside an empty point argument
    stm_fit f = request(1, ST_DIAG_MIN_DRAWS);
    stm_diagnostics dg{};
    dg.want_rows = 1;
    dg.rows_w.ess = sink;
    stm_new_points p{};
    if (with_coords) p.coords_new = g_coords;
    f.diag = &dg;
    f.pts = &p;
    FitPlan pl;
    accepted("rows diag", plan(f, pl));
    REQUIRE(pl.d.rows && !pl.d.pts && !pl.d.fun && pl.store_rows, "rows diag: wanted rows %d store_rows %d", (int)pl.d.rows, (int)pl.store_rows);
    REQUIRE(with_coords ? pl.f.pts == &pl.p : pl.f.pts == nullptr, "rows diag: coords_new %d, pts %s", with_coords, pl.f.pts ? "kept" : "dropped");
  }
  {   // a point summary raises keep_draws to the stored draws of both chains
    stm_fit f = request(1, 4);
    stm_diagnostics dg{};
    dg.new_w.rhat = sink;
    stm_new_points p = one_point();
    const uint64_t seeds[2] = {1, 2};
    stm_chains ch{};
    ch.n_chains = 2;
    ch.seeds = seeds;
    f.diag = &dg;
    f.pts = &p;
    f.ch = &ch;
    FitPlan pl;
    accepted("point diag", plan(f, pl));
    REQUIRE(pl.M == 2 && pl.total == 8 && pl.p.keep_draws == 8 && p.keep_draws == 0 && pl.d.pts && !pl.store_rows, "point diag: keep_draws %lld", (long long)pl.p.keep_draws);
  }
  {   // several chains: a point store that is reserved at all holds every chain's draws
    stm_fit f = request(1, 3);
    stm_new_points p = one_point();
    p.keep_draws = 2;
    const uint64_t seeds[3] = {1, 2, 3};
    stm_chains ch{};
    ch.n_chains = 3;
    ch.seeds = seeds;
    f.pts = &p;
    f.ch = &ch;
    FitPlan pl;
    accepted("chains", plan(f, pl));
    REQUIRE(pl.total == 9 && pl.p.keep_draws == 9, "chains: keep_draws %lld", (long long)pl.p.keep_draws);
  }
  {   // an exc whose only content is rb: no store is read, nothing reserved
    stm_fit f = request(2, 0);
    stm_new_points p = one_point();
    p.keep_draws = 1;
    const std::vector<double> thr(3 * 2, 0.5);
    const int32_t side[3] = {1, -1, 1};
    stm_rb_exceed rb{};
    rb.n_thr = 3;
    rb.thr = thr.data();
    rb.side = side;
    rb.new_w.prob = sink;
    stm_excursions ex{};
    ex.rb = &rb;
    f.exc = &ex;
    f.pts = &p;
    FitPlan pl;
    accepted("rb alone", plan(f, pl));
    REQUIRE(pl.rb == &rb && !pl.e.any() && !pl.store_rows && pl.p.keep_draws == 1 && pl.f.pts == &pl.p, "rb alone: keep_draws %lld", (long long)pl.p.keep_draws);
    // without thresholds it is no part, whatever else it holds
    const int32_t bad_side[1] = {0};
    rb.side = bad_side;
    rb.n_thr = 0;
    FitPlan pl0;
    accepted("rb n_thr 0", plan(f, pl0));
    rb.n_thr = ST_EXC_MAX_THRESHOLDS + 1;
    rb.thr = nullptr;
    FitPlan pl1;
    accepted("rb thr NULL", plan(f, pl1));
    REQUIRE(!pl0.rb && !pl1.rb, "rb without thresholds is kept");
  }
  {   // fun with n_fun = 0 is no part, and a functional output is then without fun
    stm_fit f = request(1, ST_DIAG_MIN_DRAWS);
    stm_new_points p = one_point();
    stm_functionals fn{};
    f.pts = &p;
    f.fun = &fn;
    FitPlan pl;
    accepted("fun 0", plan(f, pl));
    REQUIRE(!pl.f.fun && pl.f.pts == &pl.p, "fun 0: kept");
    stm_diagnostics dg{};
    dg.fun_w.ess = sink;
    f.diag = &dg;
    refused("fun 0 with a functional output", f, ST_ERR_USAGE, "diag: functional outputs without fun");
  }
  {   // scores without y_new are no part: nothing of theirs is asked of the point set
    stm_fit f = request(1, 2);
    stm_new_points p = one_point();
    stm_scores sc{};
    sc.crps = sink;
    f.pts = &p;
    f.scores = &sc;
    FitPlan pl;
    accepted("scores without y_new", plan(f, pl));
    REQUIRE(!pl.f.scores, "scores without y_new: kept");
  }
  for (int want = 0; want < 2; ++want)   // the criteria's CRPS
    for (int held = 0; held < 2; ++held) {
      stm_fit f = request(1, 2);
      const double y[1] = {0.0};
      stm_criteria cr{};
      cr.want_crps = want;
      cr.y_holdout = held ? y : nullptr;
      f.criteria = &cr;
      FitPlan pl;
      accepted("criteria", plan(f, pl));
      REQUIRE(pl.crps == (want && held), "criteria: want_crps %d y_holdout %d: crps %d", want, held, (int)pl.crps);
      cr.crps = sink;
      if (!(want && held)) refused("crps output", f, ST_ERR_USAGE, "criteria: crps without");
    }
}

// two faults in one request: the earlier check is the one reported
static void check_orders() {
  const double nan = std::nan("");
  {   // parts of both families beside too many chains
    stm_fit f = request(1, 4);
    stm_criteria cr{};
    stm_chains ch{};
    ch.n_chains = ST_DIAG_MAX_CHAINS + 1;
    f.criteria = &cr;
    f.ch = &ch;
    refused("families before chains", f, ST_ERR_USAGE, "fit: stm_mcmc_fit: criteria and loo do not go with", true);
    f.criteria = nullptr;
    refused("chains", f, ST_ERR_USAGE, ("ch: stm_mcmc_chains: n_chains = " + std::to_string(ST_DIAG_MAX_CHAINS + 1) + " must lie in 1 .. ").c_str(), true);
  }
  {   // too many stored draws beside a bad spec
    stm_fit f = request(1, 16385);
    const double prob[1] = {1.5};
    stm_rank_diagnostics rk{};
    rk.want_rows = 1;
    rk.rows_spec.n_prob = 1;
    rk.rows_spec.prob = prob;
    rk.rows_w.ess_q = sink;
    f.rk = &rk;
    refused("limit before spec", f, ST_ERR_UNSUPPORTED, "rk: stm_mcmc_chains: 1 chains x mcmc_keep = 16385 are 16385 stored draws, at most 16384", true);
    f.run.mcmc_keep = 16384;
    refused("spec at the limit", f, ST_ERR_USAGE, "rk.rows_spec: prob 0 must lie strictly inside (0, 1)");
  }
  {   // a point store of several chains beyond the limit, with no summary of the stored draws
    stm_fit f = request(1, 8193);
    stm_new_points p = one_point();
    p.keep_draws = 1;
    const uint64_t seeds[2] = {1, 2};
    stm_chains ch{};
    ch.n_chains = 2;
    ch.seeds = seeds;
    f.pts = &p;
    f.ch = &ch;
    refused("point store of two chains", f, ST_ERR_UNSUPPORTED, "pts: stm_mcmc_chains: 2 chains x mcmc_keep = 8193 are 16386 stored draws, at most 16384", true);
  }
  {   // diag: max_lag before the shared four
    stm_fit f = request(1, ST_DIAG_MIN_DRAWS);
    stm_diagnostics dg{};
    dg.max_lag = -1;
    dg.rows_w.ess = sink;
    f.diag = &dg;
    refused("max_lag before want_rows", f, ST_ERR_USAGE, "diag: max_lag");
    dg.max_lag = 0;
    refused("want_rows", f, ST_ERR_USAGE, "diag: row outputs without want_rows");
    dg.want_rows = 1;
    f.run.mcmc_keep = ST_DIAG_MIN_DRAWS - 1;
    refused("too few draws", f, ST_ERR_USAGE, "diag: mcmc_keep = ");
  }
  {   // exc: the spec before the count of stored draws
    stm_fit f = request(2, 0);
    const std::vector<double> thr = {0.0, 1.0, 2.0, nan};   // n_thr x q
    stm_excursions ex{};
    ex.want_rows = 1;
    ex.rows_spec.n_thr = 2;
    ex.rows_spec.thr = thr.data();
    ex.rows_w.prob = sink;
    f.exc = &ex;
    refused("exc spec before no draw", f, ST_ERR_USAGE, "exc.rows_spec: threshold 3 is not finite");
    const std::vector<double> good = {0.0, 1.0, 2.0, 3.0};
    ex.rows_spec.thr = good.data();
    refused("exc no draw", f, ST_ERR_USAGE, "exc.rows_spec: no draw stored");
    f.run.mcmc_keep = 1;
    ex.rows_w.sd = sink;
    refused("exc band of one draw", f, ST_ERR_USAGE, "exc.rows_spec: the band needs at least 2 stored draws, 1 stored");
  }
  {   // rk: all of prob before the thresholds
    stm_fit f = request(1, ST_DIAG_MIN_DRAWS);
    const double prob[2] = {0.5, 0.0}, thr[1] = {nan};
    stm_rank_diagnostics rk{};
    rk.want_rows = 1;
    rk.rows_spec.n_prob = 2;
    rk.rows_spec.prob = prob;
    rk.rows_spec.n_thr = 1;
    rk.rows_spec.thr = thr;
    rk.rows_w.rhat_rank = sink;
    f.rk = &rk;
    refused("rk prob before thr", f, ST_ERR_USAGE, "rk.rows_spec: prob 1 must lie strictly inside (0, 1)");
    rk.rows_spec.n_prob = 1;
    refused("rk thr", f, ST_ERR_USAGE, "rk.rows_spec: threshold 0 is not finite");
  }
  {   // rb: the parts it needs before its spec
    stm_fit f = request(1, 2);
    const double thr[1] = {0.0};
    stm_rb_exceed rb{};
    rb.n_thr = ST_EXC_MAX_THRESHOLDS + 1;   // (refused before any of the 9 x q values is read)
    rb.thr = thr;
    rb.new_w.prob = sink;
    stm_excursions ex{};
    ex.rb = &rb;
    f.exc = &ex;
    refused("rb point set before n_thr", f, ST_ERR_USAGE, "exc.rb: no point set");
    stm_new_points p = one_point();
    f.pts = &p;
    refused("rb n_thr", f, ST_ERR_USAGE, "exc.rb: n_thr = 9 must lie in 1 .. 8");
    rb.n_thr = 1;
    const int32_t side[1] = {2};
    rb.side = side;
    refused("rb side", f, ST_ERR_USAGE, "exc.rb: side[0] = 2 is neither +1 nor -1");
    rb.side = nullptr;
    rb.thr_fun = thr;
    refused("rb thr_fun", f, ST_ERR_USAGE, "exc.rb: thr_fun before st_points_functionals_set");
  }
  {   // psis: its text, after the criteria's refusals
    stm_fit f = request(1, 0);
    stm_loo_psis ps{};
    stm_loo lo{};
    lo.psis = &ps;
    f.loo = &lo;
    refused("psis", f, ST_ERR_UNSUPPORTED, "loo.psis: stm_mcmc_fit: psis keeps every saved draw, mcmc_keep = 0 must lie in 1 .. 16384", true);
  }
}

// where the plan needs q and the run has no problem, it refuses; nothing is read through the pointer
static void check_null_pb() {
  const double thr[1] = {0.0};
  {
    stm_fit f = request(1, 2);
    f.run.pb = nullptr;
    stm_excursions ex{};
    ex.want_rows = 1;
    ex.rows_spec.n_thr = 1;
    ex.rows_spec.thr = thr;
    ex.rows_w.count = reinterpret_cast<int32_t *>(sink);
    f.exc = &ex;
    refused("exc rows without pb", f, ST_ERR_USAGE, "exc: the run's pb is NULL");
    ++n_null_pb;
  }
  {
    stm_fit f = request(1, ST_DIAG_MIN_DRAWS);
    f.run.pb = nullptr;
    stm_rank_diagnostics rk{};
    rk.want_rows = 1;
    rk.rows_spec.n_thr = 1;
    rk.rows_spec.thr = thr;
    rk.rows_w.prob = sink;
    f.rk = &rk;
    refused("rk rows without pb", f, ST_ERR_USAGE, "rk: the run's pb is NULL");
    ++n_null_pb;
  }
  {
    stm_fit f = request(1, 2);
    f.run.pb = nullptr;
    stm_new_points p = one_point();
    stm_rb_exceed rb{};
    rb.n_thr = 1;
    rb.thr = thr;
    rb.new_w.prob = sink;
    stm_excursions ex{};
    ex.rb = &rb;
    f.exc = &ex;
    f.pts = &p;
    refused("rb without pb", f, ST_ERR_USAGE, "exc.rb: the run's pb is NULL");
    ++n_null_pb;
  }
}

int main() {
  check_accepted();
  check_orders();
  check_null_pb();
  printf("OK accepted=%lld refused=%lld null_pb=%lld texts=%lld\n", n_accepted, n_refused, n_null_pb, n_texts);
  return 0;
}
