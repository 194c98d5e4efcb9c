// fit_plan.hpp -- a whole-fit request (include/spamtree_fit.h, stm_fit) as stm_mcmc_fit runs it, worked out without a device: what
// stm_mcmc_fit refuses before a chain exists, and the request with every part that does not apply dropped.  No HIP header and no
// st_* or stm_* call: tests/fit_plan_check.cpp checks it on the CPU.
#pragma once
#include <string>

#include "spamtree_fit.h"

struct Wanted {   // which stores one summary of the stored draws (diag, exc, rk: the same six members) reads
  bool rows = false, pts = false, fun = false;
  bool any() const { return rows || pts || fun; }
};
struct FitPlan {
  stm_fit f;                 // the request; a part that does not apply is NULL: fun of no functional, scores without y_new, pts of a plain chain
  stm_new_points p;          // what f.pts points to: keep_draws raised to the stored draws, new_cond_cov where the packed blocks go
  int M = 1;                 // chains, one after another on one handle
  long long total = 0;       // the stored draws, M mcmc_keep: the columns of every per-draw output
  Wanted d, e, k;            // what diag, exc and rk read
  const stm_rb_exceed *rb = nullptr;   // exc's rb; NULL without thresholds
  const stm_mixture *mix = nullptr;    // stm_fit_more's mix
  bool mix_q = false, mix_crps = false;   // ... asks for a quantile output; for crps or spread
  bool crps = false;         // the criteria's CRPS: want_crps with a y_holdout
  bool store_rows = false;   // diag, exc or rk read the rows' stores: st_summary_accumulate on every saved iteration
  int64_t cov_len = 0;       // the packed length of st_points_joint_layout (the setup step's: it needs the device)
  FitPlan() = default;
  FitPlan(const FitPlan &) = delete;   // f.pts points into the plan
};
// Fills a fresh pl.  The refusals come in the order of include/spamtree_fit.h's step 1 and the first failing check decides the
// code.  text: what stm_mcmc_chains_last_error() reports, "" for most refusals; which: the failing check of every refusal, a
// checker's own message after the part it came from ("exc.rows_spec: threshold 3 is not finite").
// more: the parts of stm_fit_run beside the request (NULL: none); their refusals come after all of the request's.
int fit_plan(const stm_fit &fit, FitPlan &pl, std::string &text, std::string &which, const stm_fit_more *more = nullptr);
