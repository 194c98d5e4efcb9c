// Pareto-smoothed importance sampling of stored log ratios: khat and the smoothed leave-one-out estimates (st_psis,
// st_rows_loo_psis, st_rows_loo_psis_totals; the kernels and their launchers live in k_psis.hip).  spamtree_amd/psis.py has the
// definition; this header restates it in the order the kernel evaluates it.
//
// A store is t[d * n + i], d < K <= PSIS_MAX_DRAWS, i < n, optionally with phi and mu of the same shape.  A workgroup of PSIS_NT
// threads takes tiles of R consecutive series, one tile after another (k_series_rank's plan).  Per tile, with barriers between:
//   1  stage: the R values of one draw are contiguous in memory.  Series r goes to the LDS row A_r (Kpad = 2^k >= K doubles); a
//      value that is not finite (NaN, +-inf: a skipped draw) and the padding go in as +inf.
//   2  sort A_r ascending, all R rows by one bitonic network over the workgroup: the S finite values come first.
//   3  one wave per series, lane l of 64:
//      S = #{a < +inf} (a binary search).  S == 0: every double output NaN, tail_len = n_draws = 0.
//      c = A[S - 1].   M = min(S / 5, m*), m* the smallest integer with m*^2 >= 9 S (integers).   smooth = M >= 5.
//      cutv = A[S - M - 1], tmin = A[S - M];  ecut = exp(cutv - c);  smooth = smooth && c != tmin.
//      x_j = exp(A[S - M + j - 1] - c) - ecut into X_r[j - 1] (LDS, PSIS_MAX_TAIL doubles), j = 1 .. M.
//      x* = X[(M + 2) / 4 - 1];  smooth = smooth && x* != 0.
//      fit, lane j - 1 keeps grid point j <= G = 30 + isqrt(M) <= 49:
//        theta_j = 1 / x_M + (1 - sqrt(G / (j - 0.5))) / (3 x*)
//        k_j = (sum_i log1p(-theta_j x_i)) / M         the lane's own chain of additions, i = 1 .. M ascending, from 0
//        l_j = M (log(-theta_j / k_j) - k_j - 1)
//        omega_j = 1 / sum_i exp(l_i - l_j)            the lane's own chain, i = 1 .. G ascending (l_i by __shfl), from 0
//        theta^ = sum_j theta_j omega_j                one chain, j = 1 .. G ascending (the products by __shfl), from 0
//        k = (sum_i log1p(-theta^ x_i)) / M            lane l adds i - 1 = l, l + 64, ... ascending from 0, then wave_allsum
//                                                      (st_device.hpp: rotate-and-add in rows of 16 lanes, then the four row sums)
//        sigma = -k / theta^,  khat = (k M + 5) / (M + 10);   smooth = smooth && both finite
//      smoothing (smooth only): p_j = (j - 0.5) / M,  q_j = sigma expm1(-khat log1p(-p_j)) / khat  (khat == 0: -sigma log1p(-p_j)),
//        X_r[j - 1] = fmin(log(q_j + ecut), 0): the lw' of the draw at sorted position S - M + j - 1.
//      estimates: lane l walks the draws s = l, l + 64, ... ascending and reads t_s (phi_s, mu_s) from the store again.  A finite
//        t_s has lw = t_s - c.  With smooth and t_s >= tmin the draw's sorted position is pos = lo + e, lo = #{a < t_s} (binary
//        search), e = 0 when t_s occurs once (hi - lo == 1, hi = #{a <= t_s}) and otherwise e = #{s' < s : t_s' == t_s}, counted
//        by the whole wave over the store (integers: ballots and popcounts), one tied draw after another: ties go by draw index.
//        pos >= S - M: lw' = X_r[pos - (S - M)], else lw' = lw.   ew = exp(lw'),
//        W1 += ew;  W2 += exp(2 lw');  U += exp(lw' - lw);  P += ew phi_s;  Q += ew mu_s      (products, then additions; from 0)
//        then wave_allsum of each.
//        elpd_psis = (-c + log U) - log W1,  pit_psis = P / W1,  mu_psis = Q / W1,  weight_ess_psis = W1 W1 / W2,
//        khat (+inf when not smooth),  tail_len = smooth ? M : 0,  n_draws = S.
// The outputs of a series are bitwise a function of its K values (and companions): the sort gives the same values in any
// network, S, M, pos and e are integers, and every floating-point sum above has one fixed order that involves neither n, the
// series' position, R nor the grid.  No atomics, no inline assembly; fp contraction off, no fma in the definition.
//
// TOTALS (k_psis_finish) per outcome over its rows with an observed y and n_draws > 0, PSIS_NSUM values: the count, sum elpd_psis,
// sum elpd_psis^2 (fma), sum (y - mu_psis)^2 (fma), sum pit_psis, min weight_ess_psis, max khat, #{khat > 0.7}, #{khat > thr}; one workgroup
// per outcome, thread t walks rows t, t + NT, ... ascending, then a fixed binary tree over the NT threads in LDS (k_loo_finish's).
#pragma once
#include "st_device.hpp"
#include "psis_plan.hpp"         // the tile plan and its constants (host only)

#define PSIS_OUT_KHAT 0          // the per-series double outputs, PSIS_NOUT arrays of n
#define PSIS_OUT_ELPD 1
#define PSIS_OUT_PIT 2
#define PSIS_OUT_MU 3
#define PSIS_OUT_ESS 4
#define PSIS_NOUT 5

#define PSIS_NSUM ST_ROWS_PSIS_N

struct PsisArgs {
  const double *t, *phi, *mu;    // [K][n]; phi, mu may be NULL
  long long n;
  int K, Kpad, R;
  double *out;                   // PSIS_NOUT x n
  int *tail_len, *n_draws;       // n each
};

struct PsisFinishArgs {
  const double *y;
  const unsigned char *obs;
  const int *mv;
  const double *rows;            // PSIS_NOUT x n
  const int *n_draws;
  long long n;
  int q;
  double thr;
  double *tot;                   // q x PSIS_NSUM
};

// one pass over the store on `st` (no synchronisation); A.R and A.Kpad from psis_plan
int psis_launch(const PsisArgs &A, hipStream_t st);
int psis_finish_launch(const PsisFinishArgs &A, hipStream_t st);
