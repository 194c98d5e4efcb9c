// Scores of held-out observations at the new points (st_points_score_*; kernels and launchers in k_points_score.hip).
//
// A scored point i has margin j, an observed y_i and regressors x_i.  Saved draw s gives it the Gaussian predictive
//   mu_s = x_i'beta_j + cond_mean_s(i),   sigma2_s = cond_var_s(i) + tau2_j        (cond_var: the clamped value of k_points_*,
//   tau2_j = 1 / tausq_inv_j),   r_s = (y_i - mu_s) / sigma_s,   l_s = -r_s^2 / 2 - log sigma_s - log(2 pi) / 2
// and over the S draws accumulated since the scores were set
//   lpd_i  = log((1 / S) sum_s exp l_s)    kept as (M, A): M = max l, A = sum exp(l_s - M), rescaled when a new maximum arrives, so
//                                          A >= 1 once a draw is in and lpd = M + log(A / S) is finite when every exp l_s underflows
//   pit_i  = (1 / S) sum_s Phi(r_s),       Phi(r) = erfc(-r / sqrt 2) / 2
//   crps_i = (1 / K) sum_k |d_(k)| - (1 / K^2) sum_k (2 k - K - 1) d_(k),  k = 1..K, d_k = yhat*_k - y_i sorted ascending over the K
//            stored yhat* draws of the point (st_points_summary_reserve's store): the CRPS of their empirical distribution.  The
//            weights 2 k - K - 1 sum to zero, so centring at y_i costs nothing and removes the cancellation against the level of y.
// On a joint set a group G with observed members o (g_o >= 1 of its g, in member order) also has
//   l^G_s = log N_{g_o}(y_o; mu_o, Sigma_oo + diag tau2_{j(a)}) = -r'r / 2 - sum_a log L_aa - (g_o / 2) log(2 pi),  L r = y_o - mu_o
// with Sigma the draw's packed cond_cov read from its lower triangle (off + a + b g, a >= b, not clamped) and L its unpivoted
// Cholesky factor; lpd_joint_G is the same log-mean-exp over the draws.  A pivot that is not > 0 (the rounding of Sigma exceeds
// tau2) gives that draw density 0 for that group -- (M, A) stay as they are -- and adds one to the counter n_degenerate.
//
// The order of every operation is fixed (k_points_score.hip states it with each kernel), so a point's or group's values depend on
// its own inputs in saved order only: not on the other points or groups, their order, the labels or the launch shape.
#pragma once
#include "predict_joint.hpp"

#define SC_M 0        // the per-point state: 3 arrays of n doubles, caller order; all zero = no draw yet (A >= 1 afterwards)
#define SC_A 1
#define SC_PIT 2
#define SC_NACC 3
#define SC_GROUPS_PER_WG (NT / 16)               // k_score_joint_acc: 16 lanes a group

// One draw's log density l into the running (M, A) of log sum exp: A == 0 marks "no draw yet" (afterwards A >= 1: the maximum
// itself contributes exp(0)); a tie takes the first branch.  A density of 0 (l = -inf) leaves the state alone.  The one copy:
// k_score_acc, k_score_joint_acc and k_rows_score_acc (rows_score.hpp) all update through it.
__device__ __forceinline__ void sc_lse(double l, double &M, double &A) {
  if (!(l >= -__DBL_MAX__)) return;
  if (A == 0.0) { M = l; A = 1.0; }
  else if (l <= M) A += exp(l - M);
  else { A = fma(A, exp(M - l), 1.0); M = l; }
}

struct ScoreArgs {                 // k_score_acc
  const double *y;                 // n, caller order; NaN: not scored
  const double *mean, *var;        // this iteration's cond_mean and clamped cond_var (d_out)
  const double *X, *B, *tsq_inv;   // n x p column-major; p x q; q
  const int *pmv;                  // 0-based margin
  int p;
  long long n;
  double *acc;                     // SC_NACC x n
};

struct ScoreJointArgs {            // k_score_joint_acc
  const double *y, *mean, *cov;    // cov: the packed cond_cov of this iteration (d_jout)
  const double *X, *B, *tsq_inv;
  const int *pmv;
  int p;
  long long n, n_joint;
  const PtJoint *groups;
  const long long *members;
  double *jacc;                    // [n_joint][2]: M, A
  unsigned long long *n_degenerate;
};

struct ScoreCrpsArgs {             // k_score_crps
  const double *draws;             // [keep][n] stored yhat*
  const double *y;
  long long n;
  int keep, Kpad, R;
  double *out;                     // n; NaN where y is
};

int points_score_launch(const ScoreArgs &A, hipStream_t st);
// gmax: the largest group of the set (selects the 4-, 8- or 16-column instantiation; a group's bits are the same in each)
int points_score_joint_launch(const ScoreJointArgs &A, int gmax, hipStream_t st);
int points_score_crps_launch(const ScoreCrpsArgs &A, size_t lds_limit, hipStream_t st);
