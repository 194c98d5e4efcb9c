// Criteria over the fit's own rows (st_rows_score_*; kernels and launchers in k_rows_score.hip): WAIC and DIC over the observed
// rows and the scores of held-out values at NA rows, all CONDITIONAL ON w -- nothing here integrates the latent field out.
//
// Row i (model row order) has margin j = mv_i and a target t_i: y_i when the row is observed; y_holdout_i when the row is NA and
// the caller gave a finite held-out value; none otherwise (the row's state is never touched, its outputs are NaN).
// Saved draw s gives a targeted row
//   mu_s = xb_i + w_i     (the device's XB and w as they stand when the step runs),
//   tau2_j = 1 / tausq_inv_j,  sigma = sqrt(tau2_j),  r_s = (t_i - mu_s) / sigma,
//   l_s = fma(-r_s / 2, r_s, -log sigma) - log(2 pi) / 2        (k_score_acc's expression with cond_var = 0).
// Per-row state, RS_NACC arrays of n doubles in device row order (structure of arrays); all zero = no draw yet; S = draws so far:
//   (M, A)       the streaming log-sum-exp of points_score.hpp (sc_lse: the one copy)
//   (LM, LM2)    Welford mean and M2 of l_s:   d = l - LM;  LM += d / S;  LM2 = fma(d, l - LM, LM2)
//   MU           Welford mean of mu_s:         MU += (mu - MU) / S
//   PHI          held-out rows only: the running sum of Phi(r_s) = erfc(-r_s / sqrt 2) / 2
// Per-row outputs after S draws:
//   lppd = M + log(A / S),  mean_ll = LM,  p_waic = LM2 / (S - 1) (0 when S = 1),  mu_mean = MU,  pit = PHI / S (held-out rows),
//   crps (held-out rows): points_score.hpp's formula over the K stored yhat draws of the row (st_summary_reserve's store).
// Per-outcome totals j = 0..q-1, with tau2bar_j = the mean over the S draws of 1 / tausq_inv_j (host, added in call order):
//   observed rows:  sum lppd,  sum p_waic,  sum mean_ll,  sum log N(y_i; mu_mean_i, tau2bar_j)
//                   -> waic = -2 (lppd - p_waic),  Dbar = -2 sum mean_ll,  Dhat = -2 sum log N,  p_D = Dbar - Dhat,  dic = Dbar + p_D
//   held-out rows:  sum lppd (the log score),  sum pit,  sum crps,  sum (t_i - mu_mean_i)^2.
// Degenerate draws: a draw whose r is 0 / 0 counts as a density of 0 -- (M, A) stay, as for l = -inf -- and adds nothing to PHI; a
// draw whose l is not finite (tausq_inv of 0 or infinity) leaves (LM, LM2) alone while S counts it: it enters the moments at their
// running mean (d = 0), so mean_ll and p_waic are then those of that imputed sequence, not of the draws.  Nothing is ever NaN, and
// lppd stays finite when every exp l_s underflows.
//
// The order of every operation is fixed (k_rows_score.hip states it with each kernel): a row's values depend on its own inputs in
// saved order only, not on the other rows or the launch shape; a total depends on n_all through its fixed reduction shape only.
#pragma once
#include "points_score.hpp"

#define RS_M 0
#define RS_A 1
#define RS_LM 2
#define RS_LM2 3
#define RS_MU 4
#define RS_PHI 5
#define RS_NACC 6

#define RS_OUT_LPPD 0      // the per-row outputs, RS_NOUT arrays of n doubles in device row order; NaN where a row has no target
#define RS_OUT_MEANLL 1
#define RS_OUT_PWAIC 2
#define RS_OUT_MUMEAN 3
#define RS_OUT_PIT 4       // NaN off the held-out rows
#define RS_NOUT 5

#define RS_SUM_O_LPPD 0    // the sums of k_rows_score_totals, per outcome v: partial[wg][v * RS_NSUM + k]
#define RS_SUM_O_PWAIC 1
#define RS_SUM_O_MEANLL 2
#define RS_SUM_O_LOGN 3
#define RS_SUM_H_LPPD 4
#define RS_SUM_H_PIT 5
#define RS_SUM_H_CRPS 6
#define RS_SUM_H_SQERR 7
#define RS_NSUM 8

struct RowsScoreArgs {             // k_rows_score_acc
  const double *tgt;               // n, device row order; NaN: no target
  const unsigned char *obs;        // 1: observed row (its target is y), 0: NA row (its target, if any, is the held-out value)
  const double *xb, *w, *tsq_inv;  // n; n; q
  const int *mv;                   // 0-based margin
  long long n;
  double S;                        // the number of this draw, 1-based
  double *acc;                     // RS_NACC x n
};

struct RowsTotalsArgs {            // k_rows_score_totals
  const double *tgt;
  const unsigned char *obs;
  const int *mv;
  const double *acc;               // RS_NACC x n
  const double *crps;              // n (k_score_crps's output over the held-out targets), or null: the crps sums are 0
  long long n;
  double S;
  double tau2bar[QMAX];
  double *rows;                    // RS_NOUT x n
  double *partial;                 // STATS_WG x (q RS_NSUM)
};

int rows_score_launch(const RowsScoreArgs &A, hipStream_t st);
// per-row outputs, the STATS_WG partial sums and their fixed-shape tree into out (q RS_NSUM doubles)
int rows_score_totals_launch(const RowsTotalsArgs &A, int q, double *out, hipStream_t st);
