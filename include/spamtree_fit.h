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
 * (st_points_accumulate in stm_mcmc_points draws streams 6 and 7 with iteration counter = saved index, as predict_new.)
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

/* The whole fit.  Outputs (caller buffers, column-major, any may be NULL): w_mcmc, yhat_mcmc n_all x keep;
 * beta_mcmc p x keep x q; tausq_mcmc q x keep; theta_mcmc k x keep; paramsd k x k; mcmc_time seconds. */
int spamtree_mv_mcmc_c(const st_problem *pb, const st_options *opt, const double *set_unif_bounds, const double *theta, int ntheta,
                       const double *beta, double tausq, const double *mcmcsd, int mcmc_keep, int mcmc_burn, int mcmc_thin, uint64_t seed,
                       const stm_flags *flags, double *w_mcmc, double *yhat_mcmc, double *beta_mcmc, double *tausq_mcmc,
                       double *theta_mcmc, double *paramsd, double *mcmc_time);

/* New locations predicted during the fit (include/spamtree_hip.h, st_points_*).  stm_points_set: the point set of st_points_set
 * and room on the device for the first keep_draws saved draws (quantiles; at most 16384, else ST_ERR_UNSUPPORTED).  Call it
 * before the first iteration.  limited_tree and world > 1 chains are refused (ST_ERR_UNSUPPORTED). */
int stm_points_set(stm_chain c, int64_t n_new, const double *coords, const int64_t *mv, const int64_t *anchor, const double *X,
                   int64_t keep_draws);
/* spamtree_mv_mcmc_c plus prediction at n_new new locations on every saved iteration: after tausq and beta are drawn and before the
 * next sweep, whatever sample_predicts is, st_points_accumulate(seed, saved index) on the saved theta's factor (slot 0) and the
 * saved w, beta and tausq.  It consumes no draw of streams 0-5 and changes no chain state: every output of spamtree_mv_mcmc_c is
 * the same bit for bit.  Inputs as stm_points_set (X_new n_new x p or NULL); quantiles: n_quantiles levels in [0, 1], which need
 * keep_draws >= 1.  Outputs (column-major, any may be NULL): new_w, new_cond_mean, new_cond_var, new_yhat n_new x keep;
 * new_mean, new_var, new_w_mean, new_yhat_mean n_new (st_points_summary_get); new_w_q, new_yhat_q n_new x n_quantiles;
 * new_route st_points_info's route bit set.  Inconsistent requests and every refusal return before the first factorisation. */
int stm_mcmc_points(const st_problem *pb, const st_options *opt, const double *set_unif_bounds, const double *theta,
                              int ntheta, const double *beta, double tausq, const double *mcmcsd, int mcmc_keep, int mcmc_burn,
                              int mcmc_thin, uint64_t seed, const stm_flags *flags, double *w_mcmc, double *yhat_mcmc, double *beta_mcmc,
                              double *tausq_mcmc, double *theta_mcmc, double *paramsd, double *mcmc_time, int64_t n_new,
                              const double *coords_new, const int64_t *mv_new, const int64_t *anchor_new, const double *X_new,
                              int64_t keep_draws, const double *quantiles, int32_t n_quantiles, double *new_w, double *new_cond_mean,
                              double *new_cond_var, double *new_yhat, double *new_mean, double *new_var, double *new_w_mean,
                              double *new_yhat_mean, double *new_w_q, double *new_yhat_q, int32_t *new_route);

/* The joint forms (st_points_set_joint): joint_id one label per point or NULL.  stm_mcmc_points_joint is stm_mcmc_points on a
 * joint set, with two more outputs packed by st_points_joint_layout: new_cond_cov (packed length x keep, the conditional covariance
 * of every saved draw) and new_cov (st_points_summary_get_cov).  new_cond_var is then max(diag, 0) of new_cond_cov.  The packed
 * length is the sum of g_k^2 over the groups, known to the caller from the labels.  The chain is again the same bit for bit. */
int stm_points_set_joint(stm_chain c, int64_t n_new, const double *coords, const int64_t *mv, const int64_t *anchor, const double *X,
                         const int64_t *joint_id, int64_t keep_draws);
int stm_mcmc_points_joint(const st_problem *pb, const st_options *opt, const double *set_unif_bounds, const double *theta,
                          int ntheta, const double *beta, double tausq, const double *mcmcsd, int mcmc_keep, int mcmc_burn,
                          int mcmc_thin, uint64_t seed, const stm_flags *flags, double *w_mcmc, double *yhat_mcmc, double *beta_mcmc,
                          double *tausq_mcmc, double *theta_mcmc, double *paramsd, double *mcmc_time, int64_t n_new,
                          const double *coords_new, const int64_t *mv_new, const int64_t *anchor_new, const double *X_new,
                          const int64_t *joint_id_new, int64_t keep_draws, const double *quantiles, int32_t n_quantiles, double *new_w,
                          double *new_cond_mean, double *new_cond_var, double *new_yhat, double *new_mean, double *new_var,
                          double *new_w_mean, double *new_yhat_mean, double *new_w_q, double *new_yhat_q, int32_t *new_route,
                          double *new_cond_cov, double *new_cov);

/* Linear functionals of the new-point predictions (include/spamtree_hip.h, st_points_functionals_*).  stm_points_functionals_set:
 * st_points_functionals_set on the chain's point set; call it after stm_points_set(_joint) and before the first iteration.
 * stm_mcmc_functionals is stm_mcmc_points_joint (joint_id_new NULL: a plain set; new_cond_cov and new_cov then NULL) plus the
 * functionals in CSR form and their outputs, column-major, any of which may be NULL: per saved draw fun_w, fun_cond_mean,
 * fun_cond_var, fun_yhat (n_fun x keep, st_points_functionals_last); fun_mean, fun_var, fun_w_mean, fun_yhat_mean (n_fun,
 * st_points_functionals_get); fun_w_q, fun_yhat_q (n_fun x n_quantiles).  The yhat outputs need X_new.  It consumes no draw of
 * any stream and changes no chain state: every output stm_mcmc_points(_joint) also produces is the same bit for bit. */
typedef struct stm_functionals {
  int64_t n_fun;
  const int64_t *ptr, *idx;
  const double *wt;
  double *fun_w, *fun_cond_mean, *fun_cond_var, *fun_yhat;
  double *fun_mean, *fun_var, *fun_w_mean, *fun_yhat_mean;
  double *fun_w_q, *fun_yhat_q;
} stm_functionals;
int stm_points_functionals_set(stm_chain c, int64_t n_fun, const int64_t *ptr, const int64_t *idx, const double *wt);
int stm_mcmc_functionals(const st_problem *pb, const st_options *opt, const double *set_unif_bounds, const double *theta,
                         int ntheta, const double *beta, double tausq, const double *mcmcsd, int mcmc_keep, int mcmc_burn,
                         int mcmc_thin, uint64_t seed, const stm_flags *flags, double *w_mcmc, double *yhat_mcmc, double *beta_mcmc,
                         double *tausq_mcmc, double *theta_mcmc, double *paramsd, double *mcmc_time, int64_t n_new,
                         const double *coords_new, const int64_t *mv_new, const int64_t *anchor_new, const double *X_new,
                         const int64_t *joint_id_new, int64_t keep_draws, const double *quantiles, int32_t n_quantiles, double *new_w,
                         double *new_cond_mean, double *new_cond_var, double *new_yhat, double *new_mean, double *new_var,
                         double *new_w_mean, double *new_yhat_mean, double *new_w_q, double *new_yhat_q, int32_t *new_route,
                         double *new_cond_cov, double *new_cov, const stm_functionals *fun);

/* Scores of held-out observations at the new points (include/spamtree_hip.h, st_points_score_*).  stm_points_score_set:
 * st_points_score_set on the chain's point set; call it after stm_points_set(_joint) and before the first iteration.
 * stm_mcmc_scored is stm_mcmc_functionals plus the scores: y_new (n_new, NaN = not scored; NULL: no scores, the call is
 * stm_mcmc_functionals itself) and their outputs, any of which may be NULL: lpd, pit, crps (n_new), lpd_joint (one per joint group;
 * needs joint_id_new), n_scored, n_degenerate (one each).  crps needs keep_draws >= 1, the scores X_new.  It consumes no draw of any
 * stream and changes no chain state: every output stm_mcmc_functionals also produces is the same bit for bit. */
typedef struct stm_scores {
  const double *y_new;
  double *lpd, *pit, *crps, *lpd_joint;
  int64_t *n_scored, *n_degenerate;
} stm_scores;
int stm_points_score_set(stm_chain c, const double *y_new);
int stm_mcmc_scored(const st_problem *pb, const st_options *opt, const double *set_unif_bounds, const double *theta,
                    int ntheta, const double *beta, double tausq, const double *mcmcsd, int mcmc_keep, int mcmc_burn,
                    int mcmc_thin, uint64_t seed, const stm_flags *flags, double *w_mcmc, double *yhat_mcmc, double *beta_mcmc,
                    double *tausq_mcmc, double *theta_mcmc, double *paramsd, double *mcmc_time, int64_t n_new,
                    const double *coords_new, const int64_t *mv_new, const int64_t *anchor_new, const double *X_new,
                    const int64_t *joint_id_new, int64_t keep_draws, const double *quantiles, int32_t n_quantiles, double *new_w,
                    double *new_cond_mean, double *new_cond_var, double *new_yhat, double *new_mean, double *new_var,
                    double *new_w_mean, double *new_yhat_mean, double *new_w_q, double *new_yhat_q, int32_t *new_route,
                    double *new_cond_cov, double *new_cov, const stm_functionals *fun, const stm_scores *scores);

/* Convergence diagnostics of the stored draws (include/spamtree_hip.h, st_*_diagnostics): ESS, MCSE, sd and split-R-hat per row,
 * new point and functional.  stm_mcmc_diagnosed is stm_mcmc_scored plus one stm_diagnostics, every array of which is optional; n_new = 0
 * with NULL coords_new, mv_new and anchor_new (and no other point argument) is the plain chain, spamtree_mv_mcmc_c.
 * With want_rows the driver reserves mcmc_keep draws (st_summary_reserve) before the first iteration and calls
 * st_summary_accumulate(seed, m) on every saved iteration -- stream 5 with the iteration's counter, the yhat st_yhat(seed, m)
 * returns; with point or functional outputs it reserves mcmc_keep draws on the point set.  After the last iteration it calls
 * st_summary_diagnostics / st_points_summary_diagnostics / st_points_functionals_diagnostics with max_lag.  It consumes no draw of
 * streams 0-4, 6, 7 and changes no chain state: every output stm_mcmc_scored also produces is the same bit for bit.
 * Refused before the first factorisation: any diagnostics output with mcmc_keep > 16384 (ST_ERR_UNSUPPORTED) or mcmc_keep <
 * ST_DIAG_MIN_DRAWS, max_lag < 0, row outputs without want_rows, point or functional outputs without their set, yhat outputs
 * without X_new (ST_ERR_USAGE). */
typedef struct stm_diagnostics {
  int32_t max_lag, want_rows;
  st_series_diag rows_w, rows_yhat;   /* n_all each, model row order */
  st_series_diag new_w, new_yhat;     /* n_new each, caller order */
  st_series_diag fun_w, fun_yhat;     /* n_fun each */
} stm_diagnostics;
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

/* Exceedance maps, excursion functions and simultaneous bands of the stored draws (include/spamtree_hip.h, st_*_excursions).
 * stm_mcmc_excursions is stm_mcmc_diagnosed plus one stm_excursions, every array of which is optional: with want_rows it reserves
 * mcmc_keep draws of the rows (one reservation, shared with diag when both are given), with point or functional outputs mcmc_keep
 * draws on the point set, and after the last iteration it calls st_summary_excursions(rows_spec), st_points_summary_excursions
 * (new_spec) and st_points_functionals_excursions(fun_spec).  rows_spec and new_spec carry n_thr x q thresholds, fun_spec n_thr x
 * n_fun; their masks have n_all, n_new and n_fun bytes.  It consumes no draw of streams 0-4, 6, 7 and changes no chain state:
 * every output stm_mcmc_diagnosed also produces is the same bit for bit.  Refused before the first factorisation: any excursion
 * output with mcmc_keep > 16384 (ST_ERR_UNSUPPORTED); what the st_*_excursions calls refuse of a spec, mcmc_keep < 1 (< 2 with a
 * band), row outputs without want_rows, point or functional outputs without their set, yhat outputs without X_new (ST_ERR_USAGE). */
typedef struct stm_excursions {
  int32_t want_rows;
  st_excursion_spec rows_spec, new_spec, fun_spec;
  st_excursion_out rows_w, rows_yhat;   /* n_all series, model row order */
  st_excursion_out new_w, new_yhat;     /* n_new series, caller order */
  st_excursion_out fun_w, fun_yhat;     /* n_fun series */
} stm_excursions;
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

/* Rank-normalised R-hat, bulk, tail, quantile and exceedance ESS of the stored draws (include/spamtree_hip.h,
 * st_*_rank_diagnostics).  stm_mcmc_ranked is stm_mcmc_excursions plus one stm_rank_diagnostics, every array of which is
 * optional: with want_rows it reserves mcmc_keep draws of the rows (one reservation, shared with diag and exc when several are
 * given), with point or functional outputs mcmc_keep draws on the point set, and after the last iteration it calls
 * st_summary_rank_diagnostics(rows_spec), st_points_summary_rank_diagnostics(new_spec) and
 * st_points_functionals_rank_diagnostics(fun_spec).  rows_spec and new_spec carry n_thr x q thresholds, fun_spec n_thr x n_fun.
 * It consumes no draw of streams 0-4, 6, 7 and changes no chain state: every output stm_mcmc_excursions also produces is the same
 * bit for bit.  Refused before the first factorisation: any rank output with mcmc_keep > 16384 (ST_ERR_UNSUPPORTED); what the
 * st_*_rank_diagnostics calls refuse of a spec, mcmc_keep < ST_DIAG_MIN_DRAWS, row outputs without want_rows, point or functional
 * outputs without their set, yhat outputs without X_new (ST_ERR_USAGE). */
typedef struct stm_rank_diagnostics {
  int32_t want_rows;
  st_rank_spec rows_spec, new_spec, fun_spec;
  st_rank_out rows_w, rows_yhat;   /* n_all series, model row order */
  st_rank_out new_w, new_yhat;     /* n_new series, caller order */
  st_rank_out fun_w, fun_yhat;     /* n_fun series */
} stm_rank_diagnostics;
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

/* Several chains in one fit.  stm_mcmc_chains is stm_mcmc_ranked plus one stm_chains (ch = NULL: stm_mcmc_ranked itself; n_chains = 1
 * with seeds[0] = seed: the same, bit for bit).  It runs M = n_chains chains one after another on ONE handle.  Each chain is the
 * fit from scratch: w = 0, the caller's beta and tausq, theta0[c] (or `theta`), the RAM adaptation restarted from mcmcsd, both slots
 * factorised, then mcmc_burn + mcmc_thin mcmc_keep iterations with seeds[c]; the `seed` argument is not used when ch is given.
 * Philox counters are the chain's own: the rows' streams take the iteration m, the point draws of streams 6 / 7 the chain's own
 * saved index -- so chain c's columns of every per-draw output are, bit for bit, those of the single-chain call with seed = seeds[c]
 * and theta = theta0[c].
 * Every per-draw output has M mcmc_keep columns, chain-major: chain c at columns c mcmc_keep .. (c + 1) mcmc_keep - 1 (beta_mcmc:
 * p x M mcmc_keep x q).  The stores hold the M mcmc_keep draws in the same order; a point store that is reserved at all (keep_draws
 * > 0, or any stored-draw output) holds all of them.  The running sums are never reset between chains -- the Welford accumulators
 * of the points and functionals, the score mixtures -- so means, variances, quantiles, excursions and scores are those of the pooled
 * draws.  After the last chain the diagnostics are st_*_chain_diagnostics and st_*_chain_rank_diagnostics with n_chains = M.
 * paramsd receives the last chain's factor, ch->paramsd every chain's; mcmc_time the sum, ch->chain_time each.
 * Refused before the first factorisation: n_chains outside 1 .. ST_DIAG_MAX_CHAINS or seeds NULL (ST_ERR_USAGE); with n_chains > 1,
 * mcmc_keep < 1 (ST_ERR_USAGE), world > 1, and stored draws with M mcmc_keep > 16384 (ST_ERR_UNSUPPORTED).  No chain exists yet to
 * carry a text for these: stm_mcmc_chains_last_error() returns it, with the numbers, for the calling thread's last call ("" if that
 * call refused nothing of its chains).  With n_chains > 1 and no point argument (n_new = 0, coords_new, mv_new, anchor_new NULL)
 * the call is the plain chain, whether or not a summary of the rows is asked for. */
typedef struct stm_chains {
  int32_t n_chains;
  const uint64_t *seeds;     /* M */
  const double *theta0;      /* k x M, or NULL: every chain starts at `theta` */
  double *paramsd;           /* k x k x M, or NULL */
  double *chain_time;        /* M, or NULL */
} stm_chains;
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
const char *stm_mcmc_chains_last_error(void);

/* Criteria over the fit's own rows (include/spamtree_hip.h, st_rows_score_*): WAIC and DIC over the observed rows and the scores
 * of held-out values at NA rows, conditional on w.  stm_rows_score_set: st_rows_score_set on the chain's handle; call it before the
 * first iteration.  stm_mcmc_criteria is spamtree_mv_mcmc_c plus one stm_criteria: on every saved iteration, once tausq and beta are
 * drawn and st_predict has run, st_rows_score_accumulate and, with want_crps and a y_holdout, st_summary_accumulate(seed, m) into a
 * reservation of mcmc_keep draws (Philox stream 5 with the iteration's counter: the yhat that st_yhat(seed, m) returns).  It consumes
 * no draw of streams 0-4 and changes no chain state: every output of spamtree_mv_mcmc_c is the same bit for bit.
 * y_holdout: n_all values in model row order, NaN = none, or NULL (criteria over the observed rows only).  Outputs, any of which may
 * be NULL: lppd, p_waic, mean_ll, mu_mean, pit, crps (n_all each, st_rows_score_get); obs (ST_ROWS_OBS_N x q), held
 * (ST_ROWS_HELD_N x q), n_obs, n_held (q each, st_rows_score_totals); n_accumulated.
 * Refused before the first factorisation: want_crps with more than 16384 saved draws (ST_ERR_UNSUPPORTED); a y_holdout with
 * sample_predicts = 0 or sample_w = 0 (ST_ERR_USAGE: the NA rows' w would be stale); crps without want_crps or without y_holdout
 * (ST_ERR_USAGE); st_rows_score_set's own refusals. */
typedef struct stm_criteria {
  const double *y_holdout;
  int32_t want_crps;
  double *lppd, *p_waic, *mean_ll, *mu_mean, *pit, *crps;
  double *obs, *held;
  int64_t *n_obs, *n_held, *n_accumulated;
} stm_criteria;
int stm_rows_score_set(stm_chain c, const double *y_holdout);
int stm_mcmc_criteria(const st_problem *pb, const st_options *opt, const double *set_unif_bounds, const double *theta, int ntheta,
                      const double *beta, double tausq, const double *mcmcsd, int mcmc_keep, int mcmc_burn, int mcmc_thin, uint64_t seed,
                      const stm_flags *flags, double *w_mcmc, double *yhat_mcmc, double *beta_mcmc, double *tausq_mcmc,
                      double *theta_mcmc, double *paramsd, double *mcmc_time, const stm_criteria *criteria);

/* Leave-one-out criteria with the latent field integrated out (include/spamtree_hip.h, st_rows_loo_*).  stm_mcmc_loo is
 * stm_mcmc_criteria plus one stm_loo: st_rows_loo_set before the first factorisation, and on every saved iteration
 * st_rows_loo_accumulate at the point where st_rows_score_accumulate runs.  It draws nothing: every output of spamtree_mv_mcmc_c and
 * of stm_mcmc_criteria is the same bit for bit.  criteria may be NULL (no conditional criteria); loo NULL: stm_mcmc_criteria itself.
 * stm_loo carries the outputs of st_rows_loo_get (n_all each; n_accumulated, n_skipped: one count each) and of st_rows_loo_totals
 * (tot: ST_ROWS_LOO_N x q column-major; n_obs: q); any may be NULL.  limited_tree problems are refused (ST_ERR_UNSUPPORTED). */
typedef struct stm_loo {
  double *elpd_loo, *pit_loo, *mu_loo, *weight_ess;
  double *tot;
  int64_t *n_obs, *n_accumulated, *n_skipped;
} stm_loo;
int stm_mcmc_loo(const st_problem *pb, const st_options *opt, const double *set_unif_bounds, const double *theta, int ntheta,
                 const double *beta, double tausq, const double *mcmcsd, int mcmc_keep, int mcmc_burn, int mcmc_thin, uint64_t seed,
                 const stm_flags *flags, double *w_mcmc, double *yhat_mcmc, double *beta_mcmc, double *tausq_mcmc,
                 double *theta_mcmc, double *paramsd, double *mcmc_time, const stm_criteria *criteria, const stm_loo *loo);

#ifdef __cplusplus
}
#endif
#endif
