// Rao-Blackwellised exceedance probabilities at the new points (st_points_exceed_*; kernels and launchers in k_points_exceed.hip).
//
// THE DEFINITION.  T <= ST_EXC_MAX_THRESHOLDS thresholds, each with a side s_t = +1 / -1 and a value per outcome, c = thr[t q + j]
// for a point of margin j, and thr_fun[t n_fun + f] for functional f.  Saved draw s gives every target its p_s:
//   point, target w:     m = cond_mean_s(i), v = cond_var_s(i) as k_points_* leave it in d_out (clamped at 0; on a joint set
//                        max(Sigma_aa, 0)).  v > 0: z = s_t (m - c) / sqrt(v), p_s = Phi(z) = erfc(-z / sqrt 2) / 2.
//                        v == 0 (the draw equals m, e.g. a point on a conditioning row): p_s = 1 if s_t (m - c) > 0, else 0 -- strict,
//                        like the event E_t of the stored-draw excursions.
//   point, target yhat:  (needs X)  mu = x_i'beta_j + m (k_score_acc's fma chain k = 0..p-1, then one add), sigma2 = v + 1 / tausq_inv_j,
//                        z = s_t (mu - c) / sqrt(sigma2), p_s = Phi(z); sigma > 0 always.
//   functional, target w only:  m = F_m, v = F_v, the per-draw values fun_step leaves in the functionals' d_last; the same two
//                        rules, so an empty functional (m = v = 0) takes the strict indicator.
// Over the S draws accumulated since the thresholds were set, in call order, the Welford mean and M2 of p_s, in the form of
// k_points_acc's conditional mean with the host's count (d = p - mean; mean += d / count; M2 += d (p - mean)):
//   prob = mean,   prob_var = M2 / S  (the population variance of p_s over the draws; the caller's MCSE is sqrt(prob_var / ESS)).
// 0 <= p_s <= 1, so 0 <= mean <= 1 and M2 >= 0 in floating point too (the rounded new mean lies between the old one and p_s);
// nothing is NaN for a finite threshold, and a target whose every p_s is exactly 0 (or 1) has prob exactly 0 (or 1) and prob_var 0.
//
// THE STATE is laid out [target][t][{mean, M2}][n] (targets: w, then yhat when the set has X), the functionals' [t][{mean, M2}][n_fun]:
// every access of a wave is contiguous.  One thread per point (or functional) does everything in the fixed order above, so its
// values depend on its own inputs in saved order only: not on the other points, their order or the launch shape.
#pragma once
#include "predict_points.hpp"

#define EX_MEAN 0
#define EX_M2 1

struct ExceedArgs {                // k_exceed_acc
  const double *mean, *var;        // this iteration's cond_mean and clamped cond_var (d_out)
  const double *X, *B, *tsq_inv;   // n x p column-major (NULL: no yhat target); p x q; q
  const int *pmv;                  // 0-based margin
  const double *thr;               // n_thr x q on the device, threshold-major
  unsigned side_neg;               // bit t set: s_t = -1
  int n_thr, p, q;
  long long n;
  double count;                    // iterations accumulated including this one
  double *acc;                     // [1 or 2][n_thr][2][n]
};

struct ExceedFunArgs {             // k_exceed_fun_acc
  const double *last;              // 4 x n_fun of this iteration: F_w, F_m, F_v, F_y
  const double *thr;               // n_thr x n_fun on the device
  unsigned side_neg;
  int n_thr;
  long long n_fun;
  double count;
  double *acc;                     // [n_thr][2][n_fun]
};

int points_exceed_launch(const ExceedArgs &A, hipStream_t st);
int points_exceed_fun_launch(const ExceedFunArgs &A, hipStream_t st);
