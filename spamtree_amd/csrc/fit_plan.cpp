// fit_plan.cpp -- step 1 of stm_mcmc_fit up to stm_create (fit_plan.hpp): the request's refusals and its normalisation.  It reads
// the request alone.  The specs go through the checkers the st_* calls use (store_spec.cpp), so a spec is refused here for what
// its call would refuse after the chain, by the same code.
#include <algorithm>

#include "draw_store.hpp"
#include "fit_plan.hpp"

// The four refusals diag, exc and rk share, in their order: the first that applies, or NULL with *out filled
template <class Part>
static const char *wanted_of(const Part *t, bool have_pts, const stm_functionals *fun, const double *X_new, Wanted *out) {
  if (!t) return nullptr;
  Wanted w;
  w.rows = any_out(&t->rows_w) || any_out(&t->rows_yhat);
  w.pts = any_out(&t->new_w) || any_out(&t->new_yhat);
  w.fun = any_out(&t->fun_w) || any_out(&t->fun_yhat);
  if (w.rows && !t->want_rows) return "row outputs without want_rows";
  if (w.pts && !have_pts) return "point outputs without a point set";
  if (w.fun && !fun) return "functional outputs without fun";
  if ((any_out(&t->new_yhat) || any_out(&t->fun_yhat)) && !X_new) return "yhat outputs without X_new";
  *out = w;
  return nullptr;
}

int fit_plan(const stm_fit &fit, FitPlan &pl, std::string &text, std::string &which, const stm_fit_more *more) {
  text.clear(); which.clear();
  const auto refuse = [&](int code, const std::string &part, const std::string &what) { which = part + ": " + what; return code; };
  const auto no = [&](const char *part, const std::string &what) { return refuse(ST_ERR_USAGE, part, what); };
  const auto aloud = [&](int code, const char *part, const std::string &msg) { text = msg; return refuse(code, part, msg); };
  pl.f = fit;
  stm_fit &f = pl.f;
  stm_new_points &p = pl.p;
  const stm_run &r = f.run;
  if ((f.criteria || f.loo) && (f.pts || f.fun || f.scores || f.diag || f.exc || f.rk || f.ch))
    return aloud(ST_ERR_USAGE, "fit", "stm_mcmc_fit: criteria and loo do not go with pts, fun, scores, diag, exc, rk or ch in one request");
  if (f.fun && f.fun->n_fun <= 0) f.fun = nullptr;
  p = f.pts ? *f.pts : stm_new_points{};
  const stm_functionals *const fun = f.fun;
  const stm_diagnostics *const diag = f.diag;
  const stm_excursions *const exc = f.exc;
  const stm_rank_diagnostics *const rk = f.rk;
  const stm_chains *const ch = f.ch;
  const int mcmc_keep = r.mcmc_keep;
  // M chains; chain c's saved draws are columns c keep .. (c + 1) keep - 1 of every per-draw output and of the stores
  const int M = pl.M = ch ? ch->n_chains : 1;
  const std::string W = "stm_mcmc_chains: ";
  if (ch && (M < 1 || M > ST_DIAG_MAX_CHAINS))
    return aloud(ST_ERR_USAGE, "ch", W + "n_chains = " + std::to_string(M) + " must lie in 1 .. " + std::to_string(ST_DIAG_MAX_CHAINS));
  if (ch && !ch->seeds) return aloud(ST_ERR_USAGE, "ch", W + "seeds is NULL: one seed per chain (" + std::to_string(M) + ")");
  if (M > 1 && mcmc_keep < 1)
    return aloud(ST_ERR_USAGE, "ch", W + "mcmc_keep = " + std::to_string(mcmc_keep) + ": " + std::to_string(M) + " chains need at least one saved draw each");
  if (M > 1 && !r.theta) return aloud(ST_ERR_USAGE, "ch", W + "theta is NULL");
  if (M > 1 && r.opt && r.opt->world > 1)
    return aloud(ST_ERR_UNSUPPORTED, "ch", W + "world = " + std::to_string(r.opt->world) + ": several chains run on one GPU");
  const long long total = pl.total = (long long)M * mcmc_keep;
  const auto too_many = [&](const char *part) {
    return aloud(ST_ERR_UNSUPPORTED, part, W + std::to_string(M) + " chains x mcmc_keep = " + std::to_string(mcmc_keep) + " are " + std::to_string(total) +
                                               " stored draws, at most " + std::to_string(STORE_MAX_DRAWS));
  };
  // the plain chain: no point argument, and either a summary of the rows (an empty set without one reaches stm_points_set_joint)
  // or several chains
  const bool plain = (diag || exc || rk || M > 1) && p.n_new == 0 && !p.coords_new && !p.mv_new && !p.anchor_new;
  f.pts = (f.pts && !plain) ? &p : nullptr;
  const bool have_pts = f.pts != nullptr;
  // diag, exc, rk: the shared refusals, the stores' limit, the minimum of draws (exc: per spec, below), the spec; a part that reads
  // the point set's stores raises keep_draws to the stored draws.  Thresholds go per outcome: a spec of the rows or the points needs
  // the problem's q
  int rc;
  Wanted &d = pl.d, &e = pl.e, &k = pl.k;
  const auto stored = [&](const char *part, const Wanted &w, int min_draws) {
    if (total > STORE_MAX_DRAWS) return too_many(part);
    if (mcmc_keep < min_draws) return no(part, "mcmc_keep = " + std::to_string(mcmc_keep) + ", at least " + std::to_string(min_draws) + " draws per chain");
    if (w.pts || w.fun) p.keep_draws = std::max<int64_t>(p.keep_draws, total);
    return 0;
  };
  if (diag && diag->max_lag < 0) return no("diag", "max_lag must not be negative");
  if (const char *what = wanted_of(diag, have_pts, fun, p.X_new, &d)) return no("diag", what);
  if (d.any() && (rc = stored("diag", d, ST_DIAG_MIN_DRAWS)) != 0) return rc;
  if (const char *what = wanted_of(exc, have_pts, fun, p.X_new, &e)) return no("exc", what);
  if (e.any()) {
    if ((rc = stored("exc", e, 0)) != 0) return rc;
    if ((e.rows || e.pts) && !r.pb) return no("exc", "the run's pb is NULL");
    if (e.rows && (rc = check_excursion_spec("exc.rows_spec: ", &exc->rows_spec, total, r.pb->q, &exc->rows_w, &exc->rows_yhat, which)) != 0) return rc;
    if (e.pts && (rc = check_excursion_spec("exc.new_spec: ", &exc->new_spec, total, r.pb->q, &exc->new_w, &exc->new_yhat, which)) != 0) return rc;
    if (e.fun && (rc = check_excursion_spec("exc.fun_spec: ", &exc->fun_spec, total, fun->n_fun, &exc->fun_w, &exc->fun_yhat, which)) != 0) return rc;
  }
  // rb reads no store: no reservation, no limit, no minimum of draws.  (thr NULL or n_thr = 0: no part, as scores without y_new)
  const stm_rb_exceed *const rb = pl.rb = (exc && exc->rb && exc->rb->thr && exc->rb->n_thr != 0) ? exc->rb : nullptr;
  if (rb) {   // the parts it needs, then what st_points_exceed_set would refuse of the spec
    if (!r.pb) return no("exc.rb", "the run's pb is NULL");
    if (!have_pts) return no("exc.rb", "no point set");
    if (any_out(&rb->new_yhat) && !p.X_new) return no("exc.rb", "new_yhat without X_new");
    if (any_out(&rb->fun_w) && (!fun || !rb->thr_fun)) return no("exc.rb", "fun_w without fun or without thr_fun");
    if ((rc = check_exceed_spec("exc.rb: ", rb->n_thr, rb->thr, rb->side, rb->thr_fun, r.pb->q, fun ? fun->n_fun : -1, which)) != 0) return rc;
  }
  if (const char *what = wanted_of(rk, have_pts, fun, p.X_new, &k)) return no("rk", what);
  if (k.any()) {
    if ((rc = stored("rk", k, ST_DIAG_MIN_DRAWS)) != 0) return rc;
    if ((k.rows || k.pts) && !r.pb) return no("rk", "the run's pb is NULL");
    if (k.rows && (rc = check_rank_spec("rk.rows_spec: ", &rk->rows_spec, total, r.pb->q, &rk->rows_w, &rk->rows_yhat, which)) != 0) return rc;
    if (k.pts && (rc = check_rank_spec("rk.new_spec: ", &rk->new_spec, total, r.pb->q, &rk->new_w, &rk->new_yhat, which)) != 0) return rc;
    if (k.fun && (rc = check_rank_spec("rk.fun_spec: ", &rk->fun_spec, total, fun->n_fun, &rk->fun_w, &rk->fun_yhat, which)) != 0) return rc;
  }
  pl.store_rows = d.rows || e.rows || k.rows;   // one reservation serves all three
  if (M > 1 && p.keep_draws > 0) {   // a point store that is reserved at all holds every chain's draws
    if (total > STORE_MAX_DRAWS) return too_many("pts");
    p.keep_draws = total;
  }
  // the point set, its functionals, scores and quantiles
  if (!have_pts && (fun || (f.scores && f.scores->y_new) || p.joint_id_new || p.X_new || p.n_quantiles != 0)) return no("pts", "point arguments without a point set");
  if (f.scores && !f.scores->y_new) f.scores = nullptr;
  const stm_scores *const scores = f.scores;
  if (scores && !p.X_new) return no("scores", "without X_new");
  if (scores && scores->lpd_joint && !p.joint_id_new) return no("scores", "lpd_joint without joint_id_new");
  if (scores && scores->crps && p.keep_draws < 1) return no("scores", "crps without keep_draws");
  if (fun && (fun->fun_yhat || fun->fun_yhat_mean || fun->fun_yhat_q) && !p.X_new) return no("fun", "yhat outputs without X_new");
  if ((p.new_cond_cov || p.new_cov) && !p.joint_id_new) return no("pts", "new_cond_cov or new_cov without joint_id_new");
  if (p.n_quantiles < 0 || (p.n_quantiles > 0 && (!p.quantiles || p.keep_draws < 1))) return no("pts", "quantiles need their levels and keep_draws");
  for (int32_t i = 0; i < p.n_quantiles; ++i) if (!(p.quantiles[i] >= 0.0 && p.quantiles[i] <= 1.0)) return no("pts", "a quantile outside [0, 1]");
  if ((p.new_yhat || p.new_yhat_mean || p.new_yhat_q) && !p.X_new) return no("pts", "yhat outputs without X_new");
  // the criteria over the fit's own rows
  const stm_criteria *const cr = f.criteria;
  pl.crps = cr && cr->want_crps && cr->y_holdout;
  if (cr && cr->crps && !pl.crps) return no("criteria", "crps without want_crps or without y_holdout");
  if (pl.crps && mcmc_keep > STORE_MAX_DRAWS) return refuse(ST_ERR_UNSUPPORTED, "criteria", "want_crps with too many saved draws for the rows' store");
  if (cr && cr->y_holdout && r.flags && (!r.flags->sample_predicts || !r.flags->sample_w)) return no("criteria", "y_holdout: the NA rows' w would be stale");
  if (f.loo && f.loo->psis && (mcmc_keep < 1 || mcmc_keep > ST_PSIS_MAX_DRAWS))   // st_rows_loo_reserve's limits
    return aloud(ST_ERR_UNSUPPORTED, "loo.psis", "stm_mcmc_fit: psis keeps every saved draw, mcmc_keep = " + std::to_string(mcmc_keep) + " must lie in 1 .. " +
                                                     std::to_string(ST_PSIS_MAX_DRAWS));
  // more's mix: the parts it needs, what st_points_mixture_quantiles would refuse of the probabilities, the store's limit
  if (const stm_mixture *const mix = pl.mix = more ? more->mix : nullptr) {
    pl.mix_q = any_out(&mix->new_w) || any_out(&mix->new_yhat) || any_out(&mix->fun_w);
    pl.mix_crps = mix->crps || mix->spread;
    if (!have_pts) return no("mix", "no point set");
    if ((any_out(&mix->new_yhat) || pl.mix_crps) && !p.X_new) return no("mix", "new_yhat, crps or spread without X_new");
    if (pl.mix_crps && !scores) return no("mix", "crps or spread without scores");
    if (pl.mix_crps && p.n_new > 0) {   // what st_points_mixture_crps would refuse after the last chain: the host knows it now
      bool any = false;
      for (int64_t i = 0; i < p.n_new && !any; ++i) any = scores->y_new[i] == scores->y_new[i];
      if (!any) return no("mix", "crps or spread with no scored point (every y_new is NaN)");
    }
    if (any_out(&mix->fun_w) && !fun) return no("mix", "fun_w without fun");
    if ((pl.mix_q || mix->n_probs != 0) && (rc = check_mixture_probs("mix: ", mix->n_probs, mix->probs, which)) != 0) return rc;
    if (total > ST_MIX_MAX_DRAWS)
      return aloud(ST_ERR_UNSUPPORTED, "mix", "stm_fit_run: " + std::to_string(M) + " chains x mcmc_keep = " + std::to_string(mcmc_keep) + " are " +
                                                  std::to_string(total) + " stored components, at most " + std::to_string(ST_MIX_MAX_DRAWS));
  }
  return ST_OK;
}
