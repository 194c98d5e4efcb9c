/* spamtree_fit.h -- C-ABI of the C++ host MCMC driver (spamtree_amd/csrc/spamtree_fit.cpp), the counterpart of the
 * reference's Rcpp-exported `spamtree_mv_mcmc` (/root/reference/src/spamtree_fit.cpp:5-54, registered at
 * /root/reference/src/RcppExports.cpp:112-154, 239).  It sits ABOVE include/spamtree_hip.h and contains no kernels.
 *
 * Random draws: the reference uses R's generator through Rcpp (arma::randn, R::runif, R::rgamma), which does not exist
 * outside R.  Contract here: Philox4x32-10, key = seed, counter = (index_lo, index_hi | outcome, iteration, stream);
 *   stream 0  sweep normals z (device, counter index = row)          spamtree_model.cpp:1018
 *   stream 1  theta proposal normals (index = component)             spamtree_fit.cpp:211
 *   stream 2  Metropolis uniform                                     mh_adapt.h:30
 *   stream 3  gamma draws (Marsaglia-Tsang; index = 2*attempt [+1])  spamtree_model.cpp:1405
 *   stream 4  beta normals (index = component, hi = outcome)         spamtree_model.cpp:1378
 *   stream 5  yhat noise (device)                                    spamtree_fit.cpp:384
 *   stream 6  new-point normals z of st_points_predict (device, index = point in the caller's order)
 *   stream 7  new-point yhat noise of st_points_predict (device, same index)
 * (st_points_accumulate in stm_mcmc_fit draws streams 6 and 7 with iteration counter = saved index, as predict_new.)
 * normal = sqrt(-2 ln u1) cos(2 pi u2), u from 53 bits of two 32-bit words.  Draws are identical for any GPU count.
 */
#ifndef SPAMTREE_FIT_H
#define SPAMTREE_FIT_H

#include "spamtree_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define STM_ERR_NAN (-10) /* "At nan loglik: error." -- the reference's `throw 1` (spamtree_fit.cpp:234-237) */

typedef struct stm_chain_s *stm_chain;

typedef struct stm_flags {   /* the reference's boolean arguments (spamtree_fit.cpp:44-54) */
  int32_t adapting, sample_beta, sample_tausq, sample_theta, sample_w, sample_predicts;
} stm_flags;

/* One chain = SpamTreeMV + RAMAdapt + the loop state of spamtree_fit.cpp:93-165.  set_unif_bounds: k x 2 column-major;
 * mcmcsd: k x k; beta: p (copied to every outcome, spamtree_model.cpp:124-129); w starts at 0 (start_w is ignored, :95). */
int stm_create(const st_problem *pb, const st_options *opt, const double *set_unif_bounds, const double *mcmcsd, const double *theta,
               int ntheta, const double *beta, double tausq, uint64_t seed, const stm_flags *flags, stm_chain *out);
int stm_init(stm_chain c);  /* the two initial factorisations (spamtree_fit.cpp:110-111); stm_step calls it when needed.  With
                              world > 1 attach the communicator first: st_comm_init(stm_handle(c), id) */
int stm_destroy(stm_chain c);
const char *stm_last_error(stm_chain c);
st_handle stm_handle(stm_chain c);
/* n_iters bodies of the loop spamtree_fit.cpp:167-391 without prediction and saving (B, C, theta MH with phase A, tausq, beta) */
int stm_step(stm_chain c, int n_iters);
int stm_state(stm_chain c, double *theta, double *Bcoeff, double *tausq_inv, double *loglik, double *accept_ratio, int64_t *iteration,
              double *paramsd);

/* What a stepped chain can be given before its first iteration, each the st_* call of the same name on the chain's handle
 * (include/spamtree_hip.h).  stm_points_set(_joint): the point set of st_points_set(_joint) (joint_id one label per point or NULL) and
 * room on the device for the first keep_draws saved draws (quantiles; at most 16384, else ST_ERR_UNSUPPORTED); limited_tree and
 * world > 1 chains are refused (ST_ERR_UNSUPPORTED).  stm_points_functionals_set and stm_points_score_set come after it. */
int stm_points_set(stm_chain c, int64_t n_new, const double *coords, const int64_t *mv, const int64_t *anchor, const double *X,
                   int64_t keep_draws);
int stm_points_set_joint(stm_chain c, int64_t n_new, const double *coords, const int64_t *mv, const int64_t *anchor, const double *X,
                         const int64_t *joint_id, int64_t keep_draws);
int stm_points_functionals_set(stm_chain c, int64_t n_fun, const int64_t *ptr, const int64_t *idx, const double *wt);
int stm_points_score_set(stm_chain c, const double *y_new);
int stm_rows_score_set(stm_chain c, const double *y_holdout);
/* st_points_mixture_reserve on the chain's handle: room for the per-draw moments of the first `keep` saved draws (at most
 * ST_MIX_MAX_DRAWS, else ST_ERR_UNSUPPORTED; 0 releases it).  After the point set, its functionals and scores. */
int stm_points_mixture_reserve(stm_chain c, int64_t keep);

/* ---- The whole fit: one request, stm_mcmc_fit ------------------------------------------------------------------------------------
 * A request is the run (the chain of spamtree_mv_mcmc) and up to nine optional parts, each a pointer that is NULL when the part is
 * not asked for.  Every array a part names is optional (NULL: not wanted) unless said otherwise; all are column-major.
 *
 * No part changes the chain: the points draw Philox streams 6 / 7 only, the stores of the rows stream 5 with the iteration's
 * counter (the yhat st_yhat(seed, m) returns), the rest draws nothing.  So every output of a request is, bit for bit, what the
 * same request without some other part writes there.
 *
 * Two families of parts: pts, fun, scores, diag, exc, rk, ch (the points family) and criteria, loo (the rows' criteria).  A request
 * with a part of each is refused (ST_ERR_USAGE); a request with neither is the plain fit. */

/* The run: beta_mcmc p x keep x q, tausq_mcmc q x keep, theta_mcmc k x keep, w_mcmc / yhat_mcmc n_all x keep, paramsd k x k,
 * mcmc_time seconds. */
typedef struct stm_run {
  const st_problem *pb;  const st_options *opt;
  const double *set_unif_bounds, *theta;  int ntheta;
  const double *beta;  double tausq;  const double *mcmcsd;
  int mcmc_keep, mcmc_burn, mcmc_thin;  uint64_t seed;  const stm_flags *flags;
  double *w_mcmc, *yhat_mcmc, *beta_mcmc, *tausq_mcmc, *theta_mcmc, *paramsd, *mcmc_time;
} stm_run;

/* New locations predicted on every saved iteration: after tausq and beta are drawn and before the next sweep, whatever
 * sample_predicts is, st_points_accumulate(_joint)(seed, saved index) on the saved theta's factor (slot 0) and the saved w, beta and
 * tausq.  Inputs as stm_points_set_joint (X_new n_new x p or NULL; joint_id_new one label per point or NULL: a plain set);
 * quantiles: n_quantiles levels in [0, 1], which need keep_draws >= 1.  Outputs: new_w, new_cond_mean, new_cond_var, new_yhat n_new
 * x keep; new_mean, new_var, new_w_mean, new_yhat_mean n_new (st_points_summary_get); new_w_q, new_yhat_q n_new x n_quantiles;
 * new_route st_points_info's route bit set; the yhat outputs need X_new.  Joint sets only, packed by st_points_joint_layout (the
 * packed length is the sum of g_k^2 over the groups): new_cond_cov (packed length x keep, the conditional covariance of every saved
 * draw; new_cond_var is then max(diag, 0) of it) and new_cov (st_points_summary_get_cov).
 * n_new = 0 with NULL coords_new, mv_new and anchor_new is no point set when the request has diag, exc, rk or several chains, and
 * must then name no other point argument; otherwise it reaches stm_points_set_joint as the empty set. */
typedef struct stm_new_points {
  int64_t n_new;  const double *coords_new;  const int64_t *mv_new, *anchor_new;  const double *X_new;
  const int64_t *joint_id_new;
  int64_t keep_draws;  const double *quantiles;  int32_t n_quantiles;
  double *new_w, *new_cond_mean, *new_cond_var, *new_yhat;
  double *new_mean, *new_var, *new_w_mean, *new_yhat_mean;
  double *new_w_q, *new_yhat_q;
  int32_t *new_route;
  double *new_cond_cov, *new_cov;
} stm_new_points;

/* Linear functionals of the new-point predictions (include/spamtree_hip.h, st_points_functionals_*), in CSR form; n_fun <= 0 is no
 * part.  Per saved draw fun_w, fun_cond_mean, fun_cond_var, fun_yhat (n_fun x keep, st_points_functionals_last); fun_mean, fun_var,
 * fun_w_mean, fun_yhat_mean (n_fun, st_points_functionals_get); fun_w_q, fun_yhat_q (n_fun x n_quantiles).  The yhat outputs need
 * X_new. */
typedef struct stm_functionals {
  int64_t n_fun;
  const int64_t *ptr, *idx;
  const double *wt;
  double *fun_w, *fun_cond_mean, *fun_cond_var, *fun_yhat;
  double *fun_mean, *fun_var, *fun_w_mean, *fun_yhat_mean;
  double *fun_w_q, *fun_yhat_q;
} stm_functionals;

/* Scores of held-out observations at the new points (include/spamtree_hip.h, st_points_score_*).  y_new: n_new values, NaN = not
 * scored; NULL is no part.  lpd, pit, crps (n_new), lpd_joint (one per joint group; needs joint_id_new), n_scored, n_degenerate (one
 * each).  crps needs keep_draws >= 1, the scores X_new. */
typedef struct stm_scores {
  const double *y_new;
  double *lpd, *pit, *crps, *lpd_joint;
  int64_t *n_scored, *n_degenerate;
} stm_scores;

/* The three summaries of the stored draws -- diag, exc, rk -- share one shape: outputs for the rows (n_all series, model row
 * order; only with want_rows), the new points (n_new series, caller order) and the functionals (n_fun series).  A part with row
 * outputs makes the driver reserve the stored draws of the rows (st_summary_reserve, one reservation for all three) and call
 * st_summary_accumulate(seed, m) on every saved iteration; one with point or functional outputs raises keep_draws to the stored
 * draws.  The stored draws are mcmc_keep per chain.  After the last iteration each part reads its stores.
 * Refused, in this order for each part: row outputs without want_rows, point outputs without a point set, functional outputs
 * without fun, yhat outputs without X_new (ST_ERR_USAGE); more than 16384 stored draws (ST_ERR_UNSUPPORTED); too few draws and what
 * the part's st_* calls refuse of a spec (ST_ERR_USAGE).
 *
 * diag: ESS, MCSE, sd and split-R-hat (st_*_chain_diagnostics with max_lag; max_lag < 0 is refused first).  At least
 * ST_DIAG_MIN_DRAWS draws per chain. */
typedef struct stm_diagnostics {
  int32_t max_lag, want_rows;
  st_series_diag rows_w, rows_yhat;   /* n_all each, model row order */
  st_series_diag new_w, new_yhat;     /* n_new each, caller order */
  st_series_diag fun_w, fun_yhat;     /* n_fun each */
} stm_diagnostics;

/* exc: exceedance maps, excursion functions and simultaneous bands (st_summary_excursions(rows_spec), st_points_summary_excursions
 * (new_spec), st_points_functionals_excursions(fun_spec)).  rows_spec and new_spec carry n_thr x q thresholds, fun_spec n_thr x
 * n_fun; their masks have n_all, n_new and n_fun bytes.  At least 1 stored draw, 2 with a band.
 *
 * rb: the Rao-Blackwellised exceedance probabilities at the new points (include/spamtree_hip.h, st_points_exceed_*): thr n_thr x q,
 * side (NULL: all +1), thr_fun n_thr x n_fun (NULL: no functional part); new_w, new_yhat n_thr x n_new, fun_w n_thr x n_fun,
 * n_accumulated one value; thr NULL or n_thr = 0 is no part.  It reads no store: it reserves nothing and raises no keep_draws, the stores' limit and minimum of draws
 * do not apply to it, and an exc whose only content is rb is valid.  Refused before a chain exists (ST_ERR_USAGE): rb without a
 * point set, a new_yhat output without X_new, fun_w without fun or without thr_fun, and what st_points_exceed_set refuses of the
 * spec.  The thresholds are set once, after the point set and the functionals, and read out after the last chain: with several
 * chains the state runs across them, pooled like the point summaries.  The chain is draw for draw the same with and without rb. */
typedef struct stm_rb_exceed {
  int32_t n_thr;
  const double *thr;
  const int32_t *side;
  const double *thr_fun;
  st_rb_out new_w, new_yhat, fun_w;
  int64_t *n_accumulated;
} stm_rb_exceed;

typedef struct stm_excursions {
  int32_t want_rows;
  st_excursion_spec rows_spec, new_spec, fun_spec;
  st_excursion_out rows_w, rows_yhat;   /* n_all series, model row order */
  st_excursion_out new_w, new_yhat;     /* n_new series, caller order */
  st_excursion_out fun_w, fun_yhat;     /* n_fun series */
  const stm_rb_exceed *rb;              /* NULL: none */
} stm_excursions;

/* rk: rank-normalised R-hat, bulk, tail, quantile and exceedance ESS (st_*_chain_rank_diagnostics).  rows_spec and new_spec carry
 * n_thr x q thresholds, fun_spec n_thr x n_fun.  At least ST_DIAG_MIN_DRAWS draws per chain. */
typedef struct stm_rank_diagnostics {
  int32_t want_rows;
  st_rank_spec rows_spec, new_spec, fun_spec;
  st_rank_out rows_w, rows_yhat;   /* n_all series, model row order */
  st_rank_out new_w, new_yhat;     /* n_new series, caller order */
  st_rank_out fun_w, fun_yhat;     /* n_fun series */
} stm_rank_diagnostics;

/* Several chains in one fit (n_chains = 1 with seeds[0] = seed: the request without ch, bit for bit).  M = n_chains chains run
 * one after another on ONE handle.  Each chain is the fit from scratch: w = 0, the caller's beta and tausq, theta0[c] (or `theta`),
 * the RAM adaptation restarted from mcmcsd, both slots factorised, then mcmc_burn + mcmc_thin mcmc_keep iterations with seeds[c];
 * the run's `seed` is not used.  Philox counters are the chain's own: the rows' streams take the iteration m, the point draws of
 * streams 6 / 7 the chain's own saved index -- so chain c's columns of every per-draw output are, bit for bit, those of the
 * single-chain request with seed = seeds[c] and theta = theta0[c].
 * Every per-draw output has M mcmc_keep columns, chain-major: chain c at columns c mcmc_keep .. (c + 1) mcmc_keep - 1 (beta_mcmc:
 * p x M mcmc_keep x q).  The stores hold the M mcmc_keep draws in the same order; a point store that is reserved at all (keep_draws
 * > 0, or any stored-draw output) holds all of them.  The running sums are never reset between chains -- the Welford accumulators
 * of the points and functionals, the score mixtures -- so means, variances, quantiles, excursions and scores are those of the pooled
 * draws, and diag and rk are the multi-chain diagnostics with n_chains = M.  The run's paramsd receives the last chain's factor,
 * ch->paramsd every chain's; mcmc_time the sum, ch->chain_time each.
 * Refused: n_chains outside 1 .. ST_DIAG_MAX_CHAINS or seeds NULL (ST_ERR_USAGE); with n_chains > 1, mcmc_keep < 1 (ST_ERR_USAGE),
 * world > 1, and stored draws with M mcmc_keep > 16384 (ST_ERR_UNSUPPORTED). */
typedef struct stm_chains {
  int32_t n_chains;
  const uint64_t *seeds;     /* M */
  const double *theta0;      /* k x M, or NULL: every chain starts at `theta` */
  double *paramsd;           /* k x k x M, or NULL */
  double *chain_time;        /* M, or NULL */
} stm_chains;

/* Criteria over the fit's own rows (include/spamtree_hip.h, st_rows_score_*): WAIC and DIC over the observed rows and the scores
 * of held-out values at NA rows, conditional on w.  On every saved iteration, once tausq and beta are drawn and st_predict has run,
 * st_rows_score_accumulate and, with want_crps and a y_holdout, st_summary_accumulate(seed, m) into a reservation of mcmc_keep draws.
 * y_holdout: n_all values in model row order, NaN = none, or NULL (criteria over the observed rows only).  lppd, p_waic, mean_ll,
 * mu_mean, pit, crps (n_all each, st_rows_score_get); obs (ST_ROWS_OBS_N x q), held (ST_ROWS_HELD_N x q), n_obs, n_held (q each,
 * st_rows_score_totals); n_accumulated.
 * Refused, in this order: crps without want_crps or without y_holdout (ST_ERR_USAGE); want_crps with more than 16384 saved draws
 * (ST_ERR_UNSUPPORTED); a y_holdout with sample_predicts = 0 or sample_w = 0 (ST_ERR_USAGE: the NA rows' w would be stale); then
 * st_rows_score_set's own refusals. */
typedef struct stm_criteria {
  const double *y_holdout;
  int32_t want_crps;
  double *lppd, *p_waic, *mean_ll, *mu_mean, *pit, *crps;
  double *obs, *held;
  int64_t *n_obs, *n_held, *n_accumulated;
} stm_criteria;

/* Leave-one-out criteria with the latent field integrated out (include/spamtree_hip.h, st_rows_loo_*): st_rows_loo_set before
 * the first factorisation, st_rows_loo_accumulate on every saved iteration right after st_rows_score_accumulate.  With or without
 * criteria.  The outputs of st_rows_loo_get (n_all each; n_accumulated, n_skipped: one count each) and of st_rows_loo_totals (tot:
 * ST_ROWS_LOO_N x q; n_obs: q).  limited_tree problems are refused (ST_ERR_UNSUPPORTED). */
typedef struct stm_loo_psis stm_loo_psis;
typedef struct stm_loo_groups stm_loo_groups;
typedef struct stm_loo {
  double *elpd_loo, *pit_loo, *mu_loo, *weight_ess;
  double *tot;
  int64_t *n_obs, *n_accumulated, *n_skipped;
  const stm_loo_psis *psis;   /* NULL: the raw weights alone */
  const stm_loo_groups *groups;   /* NULL: rows alone */
} stm_loo;

/* Leave-group-out criteria (include/spamtree_hip.h, st_rows_loo_groups_*): a part of loo, so it cannot be asked for without it, and
 * no entry point of its own: a request that leaves the pointer NULL runs bit for bit as before.  st_rows_loo_groups_set(labels)
 * comes right after st_rows_loo_set (and loo's st_rows_loo_reserve), so its refusals come in step 1 after loo's; the read-out after
 * loo's and psis' in step 3.  labels: n_all values, model row order.  The caller sizes the per-group outputs for n_all groups (there
 * cannot be more) and reads n_groups and n_members: label, elpd_lgo, weight_ess, n_skipped, khat, elpd_psis, weight_ess_psis
 * (n_groups used), ptr (n_groups + 1), rows (n_members); mu_lgo, pit_lgo: n_all; tot: ST_ROWS_LGO_N; by_outcome: ST_ROWS_LGO_OUT_N x q.
 * khat, elpd_psis and weight_ess_psis are written only when loo has its psis part (the store); any pointer but labels may be NULL. */
struct stm_loo_groups {
  const int64_t *labels;
  int64_t *n_groups, *n_members, *n_pairs;
  int64_t *label, *ptr, *rows;
  double *elpd_lgo, *weight_ess;
  int64_t *n_skipped;
  double *mu_lgo, *pit_lgo;
  double *tot, *by_outcome;
  double *khat, *elpd_psis, *weight_ess_psis;
};

/* Pareto smoothing of the leave-one-out weights (include/spamtree_hip.h, st_rows_loo_reserve / _psis / _psis_totals / _draws): a
 * part of loo, so it cannot be asked for without it, and no entry point of its own: a request (or stm_mcmc_loo's loo) that leaves
 * the pointer NULL runs as before.  mcmc_keep outside 1 .. ST_PSIS_MAX_DRAWS is refused in step 1, after the criteria's refusals
 * (ST_ERR_UNSUPPORTED).  st_rows_loo_reserve(mcmc_keep) comes right after st_rows_loo_set; the read-out after loo's in step 3:
 * out (n_all each), tot (ST_ROWS_PSIS_N x q) and n_obs (q) of st_rows_loo_psis and st_rows_loo_psis_totals, and the stored columns
 * t, phi, mu of st_rows_loo_draws ([mcmc_keep][n_all] each).  Any pointer may be NULL.  The chain and every other output are bit
 * for bit those of the same request without the part. */
struct stm_loo_psis {
  st_psis_out out;
  double *tot;
  int64_t *n_obs;
  double *t, *phi, *mu;
};

/* The request.  stm_mcmc_fit runs it in three steps whose order is part of the contract:
 *  1. Before a chain exists, the refusals; the first failing check decides the return code.  Parts of both families; then the
 *     chains' (with a text, below), diag's, exc's, rk's (each in the order given above), the point set's, the scores', the
 *     quantiles'; then the criteria's.  Then stm_create, the point set, the rows' reservation, functionals, scores, the joint
 *     layout, stm_rows_score_set, st_rows_loo_set (with loo's psis: st_rows_loo_reserve; with loo's groups: st_rows_loo_groups_set) and stm_init: every refusal of those comes before the first sweep.
 *  2. Chain after chain; on every saved iteration st_get_w, st_yhat, the points' accumulate, st_points_functionals_last,
 *     st_rows_score_accumulate and its st_summary_accumulate, st_rows_loo_accumulate, the stores' st_summary_accumulate.
 *  3. After the last chain the read-outs, each only for a part that is there and only once a draw was saved: new_cond_var from
 *     the packed blocks, the points' summaries, covariance, quantiles and routes, the functionals' summaries and quantiles, the
 *     scores, diag (rows, points, functionals), exc, rk, the criteria, loo, loo's psis, loo's groups. */
typedef struct stm_fit {
  stm_run run;
  const stm_new_points *pts;   /* NULL: no point set */
  const stm_functionals *fun;
  const stm_scores *scores;
  const stm_diagnostics *diag;
  const stm_excursions *exc;
  const stm_rank_diagnostics *rk;
  const stm_chains *ch;
  const stm_criteria *criteria;
  const stm_loo *loo;
} stm_fit;
int stm_mcmc_fit(const stm_fit *fit);

/* Parts added after the request's layout was pinned travel beside it: stm_fit_run(fit, more) is stm_mcmc_fit(fit) with the parts of
 * `more`, and stm_fit_run(fit, NULL) is stm_mcmc_fit(fit) bit for bit (stm_mcmc_fit is that call).
 * mix: quantiles and the exact CRPS of the mixture predictive at the new points (st_points_mixture_*, include/spamtree_hip.h).
 * probs: n_probs probabilities strictly inside (0, 1), at most ST_MIX_MAX_PROBS; new_w and new_yhat take n_probs x n_new quantiles
 * (probability-major, caller order), fun_w n_probs x n_fun; crps and spread n_new each, NaN where the scores' y_new is; n_stored the
 * components the store held.  Any output may be NULL; probs are read only when a quantile output (or n_probs != 0) is there.
 * Refused before a chain exists, in this order, after every refusal of the request itself: ST_ERR_USAGE for mix without a point
 * set, a new_yhat output or crps / spread without X_new, crps / spread without scores or with every y_new NaN, fun_w without fun, and what
 * st_points_mixture_quantiles refuses of the probabilities; ST_ERR_UNSUPPORTED for chains x mcmc_keep beyond ST_MIX_MAX_DRAWS.  The
 * store is reserved once for chains x mcmc_keep draws, after the point set, the functionals, the scores and rb's thresholds, and read
 * out after the last chain, behind rb: with several chains it runs across them, pooled like the point summaries.  The chain and
 * every other output are draw for draw the same with and without mix. */
typedef struct stm_mixture {
  const double *probs;
  int32_t n_probs;
  st_mix_out new_w, new_yhat, fun_w;
  double *crps, *spread;
  int64_t *n_stored;
} stm_mixture;
typedef struct stm_fit_more { const stm_mixture *mix; } stm_fit_more;
int stm_fit_run(const stm_fit *fit, const stm_fit_more *more);
/* The text, with the numbers, of what the calling thread's last stm_mcmc_fit refused of its chains or of parts of both families,
 * before a chain existed to carry it; "" otherwise.  Every stm_mcmc_fit clears it first, and so does every entry point below,
 * stm_mcmc_criteria and stm_mcmc_loo included. */
const char *stm_mcmc_chains_last_error(void);

/* ---- The positional entry points: each fills a request from its arguments and calls stm_mcmc_fit --------------------------------
 * spamtree_mv_mcmc_c: the run, its twenty fields in their order. */
int spamtree_mv_mcmc_c(const st_problem *pb, const st_options *opt, const double *set_unif_bounds, const double *theta, int ntheta,
                       const double *beta, double tausq, const double *mcmcsd, int mcmc_keep, int mcmc_burn, int mcmc_thin, uint64_t seed,
                       const stm_flags *flags, double *w_mcmc, double *yhat_mcmc, double *beta_mcmc, double *tausq_mcmc,
                       double *theta_mcmc, double *paramsd, double *mcmc_time);
/* stm_mcmc_points: run and pts, without joint_id_new, new_cond_cov and new_cov (a plain set) */
int stm_mcmc_points(const st_problem *pb, const st_options *opt, const double *set_unif_bounds, const double *theta,
                              int ntheta, const double *beta, double tausq, const double *mcmcsd, int mcmc_keep, int mcmc_burn,
                              int mcmc_thin, uint64_t seed, const stm_flags *flags, double *w_mcmc, double *yhat_mcmc, double *beta_mcmc,
                              double *tausq_mcmc, double *theta_mcmc, double *paramsd, double *mcmc_time, int64_t n_new,
                              const double *coords_new, const int64_t *mv_new, const int64_t *anchor_new, const double *X_new,
                              int64_t keep_draws, const double *quantiles, int32_t n_quantiles, double *new_w, double *new_cond_mean,
                              double *new_cond_var, double *new_yhat, double *new_mean, double *new_var, double *new_w_mean,
                              double *new_yhat_mean, double *new_w_q, double *new_yhat_q, int32_t *new_route);
/* stm_mcmc_points_joint: run and every field of pts, in their order */
int stm_mcmc_points_joint(const st_problem *pb, const st_options *opt, const double *set_unif_bounds, const double *theta,
                          int ntheta, const double *beta, double tausq, const double *mcmcsd, int mcmc_keep, int mcmc_burn,
                          int mcmc_thin, uint64_t seed, const stm_flags *flags, double *w_mcmc, double *yhat_mcmc, double *beta_mcmc,
                          double *tausq_mcmc, double *theta_mcmc, double *paramsd, double *mcmc_time, int64_t n_new,
                          const double *coords_new, const int64_t *mv_new, const int64_t *anchor_new, const double *X_new,
                          const int64_t *joint_id_new, int64_t keep_draws, const double *quantiles, int32_t n_quantiles, double *new_w,
                          double *new_cond_mean, double *new_cond_var, double *new_yhat, double *new_mean, double *new_var,
                          double *new_w_mean, double *new_yhat_mean, double *new_w_q, double *new_yhat_q, int32_t *new_route,
                          double *new_cond_cov, double *new_cov);
/* stm_mcmc_functionals: run, pts, fun */
int stm_mcmc_functionals(const st_problem *pb, const st_options *opt, const double *set_unif_bounds, const double *theta,
                         int ntheta, const double *beta, double tausq, const double *mcmcsd, int mcmc_keep, int mcmc_burn,
                         int mcmc_thin, uint64_t seed, const stm_flags *flags, double *w_mcmc, double *yhat_mcmc, double *beta_mcmc,
                         double *tausq_mcmc, double *theta_mcmc, double *paramsd, double *mcmc_time, int64_t n_new,
                         const double *coords_new, const int64_t *mv_new, const int64_t *anchor_new, const double *X_new,
                         const int64_t *joint_id_new, int64_t keep_draws, const double *quantiles, int32_t n_quantiles, double *new_w,
                         double *new_cond_mean, double *new_cond_var, double *new_yhat, double *new_mean, double *new_var,
                         double *new_w_mean, double *new_yhat_mean, double *new_w_q, double *new_yhat_q, int32_t *new_route,
                         double *new_cond_cov, double *new_cov, const stm_functionals *fun);
/* stm_mcmc_scored: run, pts, fun, scores */
int stm_mcmc_scored(const st_problem *pb, const st_options *opt, const double *set_unif_bounds, const double *theta,
                    int ntheta, const double *beta, double tausq, const double *mcmcsd, int mcmc_keep, int mcmc_burn,
                    int mcmc_thin, uint64_t seed, const stm_flags *flags, double *w_mcmc, double *yhat_mcmc, double *beta_mcmc,
                    double *tausq_mcmc, double *theta_mcmc, double *paramsd, double *mcmc_time, int64_t n_new,
                    const double *coords_new, const int64_t *mv_new, const int64_t *anchor_new, const double *X_new,
                    const int64_t *joint_id_new, int64_t keep_draws, const double *quantiles, int32_t n_quantiles, double *new_w,
                    double *new_cond_mean, double *new_cond_var, double *new_yhat, double *new_mean, double *new_var,
                    double *new_w_mean, double *new_yhat_mean, double *new_w_q, double *new_yhat_q, int32_t *new_route,
                    double *new_cond_cov, double *new_cov, const stm_functionals *fun, const stm_scores *scores);
/* stm_mcmc_diagnosed: run, pts, fun, scores, diag */
int stm_mcmc_diagnosed(const st_problem *pb, const st_options *opt, const double *set_unif_bounds, const double *theta,
                       int ntheta, const double *beta, double tausq, const double *mcmcsd, int mcmc_keep, int mcmc_burn,
                       int mcmc_thin, uint64_t seed, const stm_flags *flags, double *w_mcmc, double *yhat_mcmc, double *beta_mcmc,
                       double *tausq_mcmc, double *theta_mcmc, double *paramsd, double *mcmc_time, int64_t n_new,
                       const double *coords_new, const int64_t *mv_new, const int64_t *anchor_new, const double *X_new,
                       const int64_t *joint_id_new, int64_t keep_draws, const double *quantiles, int32_t n_quantiles, double *new_w,
                       double *new_cond_mean, double *new_cond_var, double *new_yhat, double *new_mean, double *new_var,
                       double *new_w_mean, double *new_yhat_mean, double *new_w_q, double *new_yhat_q, int32_t *new_route,
                       double *new_cond_cov, double *new_cov, const stm_functionals *fun, const stm_scores *scores,
                       const stm_diagnostics *diag);
/* stm_mcmc_excursions: run, pts, fun, scores, diag, exc */
int stm_mcmc_excursions(const st_problem *pb, const st_options *opt, const double *set_unif_bounds, const double *theta,
                        int ntheta, const double *beta, double tausq, const double *mcmcsd, int mcmc_keep, int mcmc_burn,
                        int mcmc_thin, uint64_t seed, const stm_flags *flags, double *w_mcmc, double *yhat_mcmc, double *beta_mcmc,
                        double *tausq_mcmc, double *theta_mcmc, double *paramsd, double *mcmc_time, int64_t n_new,
                        const double *coords_new, const int64_t *mv_new, const int64_t *anchor_new, const double *X_new,
                        const int64_t *joint_id_new, int64_t keep_draws, const double *quantiles, int32_t n_quantiles, double *new_w,
                        double *new_cond_mean, double *new_cond_var, double *new_yhat, double *new_mean, double *new_var,
                        double *new_w_mean, double *new_yhat_mean, double *new_w_q, double *new_yhat_q, int32_t *new_route,
                        double *new_cond_cov, double *new_cov, const stm_functionals *fun, const stm_scores *scores,
                        const stm_diagnostics *diag, const stm_excursions *exc);
/* stm_mcmc_ranked: run, pts, fun, scores, diag, exc, rk */
int stm_mcmc_ranked(const st_problem *pb, const st_options *opt, const double *set_unif_bounds, const double *theta,
                    int ntheta, const double *beta, double tausq, const double *mcmcsd, int mcmc_keep, int mcmc_burn,
                    int mcmc_thin, uint64_t seed, const stm_flags *flags, double *w_mcmc, double *yhat_mcmc, double *beta_mcmc,
                    double *tausq_mcmc, double *theta_mcmc, double *paramsd, double *mcmc_time, int64_t n_new,
                    const double *coords_new, const int64_t *mv_new, const int64_t *anchor_new, const double *X_new,
                    const int64_t *joint_id_new, int64_t keep_draws, const double *quantiles, int32_t n_quantiles, double *new_w,
                    double *new_cond_mean, double *new_cond_var, double *new_yhat, double *new_mean, double *new_var,
                    double *new_w_mean, double *new_yhat_mean, double *new_w_q, double *new_yhat_q, int32_t *new_route,
                    double *new_cond_cov, double *new_cov, const stm_functionals *fun, const stm_scores *scores,
                    const stm_diagnostics *diag, const stm_excursions *exc, const stm_rank_diagnostics *rk);
/* stm_mcmc_chains: run, pts, fun, scores, diag, exc, rk, ch */
int stm_mcmc_chains(const st_problem *pb, const st_options *opt, const double *set_unif_bounds, const double *theta,
                    int ntheta, const double *beta, double tausq, const double *mcmcsd, int mcmc_keep, int mcmc_burn,
                    int mcmc_thin, uint64_t seed, const stm_flags *flags, double *w_mcmc, double *yhat_mcmc, double *beta_mcmc,
                    double *tausq_mcmc, double *theta_mcmc, double *paramsd, double *mcmc_time, int64_t n_new,
                    const double *coords_new, const int64_t *mv_new, const int64_t *anchor_new, const double *X_new,
                    const int64_t *joint_id_new, int64_t keep_draws, const double *quantiles, int32_t n_quantiles, double *new_w,
                    double *new_cond_mean, double *new_cond_var, double *new_yhat, double *new_mean, double *new_var,
                    double *new_w_mean, double *new_yhat_mean, double *new_w_q, double *new_yhat_q, int32_t *new_route,
                    double *new_cond_cov, double *new_cov, const stm_functionals *fun, const stm_scores *scores,
                    const stm_diagnostics *diag, const stm_excursions *exc, const stm_rank_diagnostics *rk, const stm_chains *ch);
/* stm_mcmc_criteria: run, criteria */
int stm_mcmc_criteria(const st_problem *pb, const st_options *opt, const double *set_unif_bounds, const double *theta, int ntheta,
                      const double *beta, double tausq, const double *mcmcsd, int mcmc_keep, int mcmc_burn, int mcmc_thin, uint64_t seed,
                      const stm_flags *flags, double *w_mcmc, double *yhat_mcmc, double *beta_mcmc, double *tausq_mcmc,
                      double *theta_mcmc, double *paramsd, double *mcmc_time, const stm_criteria *criteria);
/* stm_mcmc_loo: run, criteria, loo */
int stm_mcmc_loo(const st_problem *pb, const st_options *opt, const double *set_unif_bounds, const double *theta, int ntheta,
                 const double *beta, double tausq, const double *mcmcsd, int mcmc_keep, int mcmc_burn, int mcmc_thin, uint64_t seed,
                 const stm_flags *flags, double *w_mcmc, double *yhat_mcmc, double *beta_mcmc, double *tausq_mcmc,
                 double *theta_mcmc, double *paramsd, double *mcmc_time, const stm_criteria *criteria, const stm_loo *loo);

#ifdef __cplusplus
}
#endif
#endif
