// Quantiles and the exact CRPS of the mixture predictive at the new points (st_points_mixture_*; kernels and launchers in
// k_points_mixture.hip, the launch shapes in mixture_plan.hpp).
//
// THE MIXTURE.  Saved draw s gives point i of margin j exactly the quantities of points_exceed.hpp:
//   m_s = cond_mean_s(i),  v_s = cond_var_s(i) as k_points_* leave it in d_out (clamped at 0; on a joint set max(Sigma_aa, 0));
//   with X: mu_s = x_i'beta_j + m_s (k_score_acc's fma chain k = 0..p-1, then one add),  sigma2_s = v_s + tau2_s(j), tau2 = 1 / tausq_inv_j;
//   functional f, target w only: m_s = F_m, v_s = F_v of the functionals' d_last.
// The predictive of a target is the equal-weight mixture of its K stored components N(m_s, v_s) (target yhat: N(mu_s, sigma2_s)).
//   CDF       F(x) = (1 / K) sum_s Phi_s(x),  Phi_s(x) = erfc(-(x - m_s) / (sd_s sqrt 2)) / 2,  sd_s = sqrt(v_s);  a component with
//             v_s == 0 is the right-continuous step 1(x >= m_s).
//   quantile  q(p) = inf{x : F(x) >= p} for p strictly inside (0, 1).
//   CRPS at y A(d, s2) = d erf(d / (s sqrt 2)) + s sqrt(2 / pi) exp(-d^2 / (2 s2)), s = sqrt(s2), and A(d, 0) = |d|  (= E|N(d, s2)|;
//             erf, not 1 - erfc: small arguments do not cancel).  Both terms are >= 0 and A >= max(|d|, s sqrt(2 / pi)).
//             crps   = (1 / K) sum_s A(y - mu_s, sigma2_s) - spread,
//             spread = (1 / (2 K^2)) sum_s sum_t A(mu_s - mu_t, sigma2_s + sigma2_t)      (Grimit et al. 2006)
//             the double sum formed as its diagonal (A(0, 2 sigma2) = sqrt(2 sigma2) sqrt(2 / pi)) plus twice the pairs s < t.  Every
//             term is >= 0: the only cancellation is the final subtraction.  spread does not depend on y: the sharpness.
//
// THE STORE (st_points_mixture_reserve) holds the first `keep` saved draws, [keep][n] per field like the stored draws of
// st_points_summary_reserve: m, v and with X mu (24 B per point and draw, 16 B without), tau2 [keep][q], and F_m, F_v [keep][n_fun].
// k_mix_store writes one column per saved iteration from d_out, d_X, d_B, d_tsq and d_last; sigma2 is re-formed as v + tau2, the
// bits of k_score_acc's s2.  keep <= ST_MIX_MAX_DRAWS = 8192: one series' K pairs of doubles are 128 KB of a workgroup's 160 KB LDS.
//
// k_mix_quantile.  A wave per series; the workgroup stages R series (mixture_plan.hpp) as (m, sd) pairs into LDS once and serves all
// T probabilities from them, in ascending order of p.  One evaluation ("pass") of F and the density f at x: lane l takes the
// components s = l, l + 64, ... in ascending order -- z = (x - m_s) / sd_s, S += erfc(-z / sqrt 2) / 2, D += exp(-z^2 / 2) / sd_s; a
// point mass adds 1(x >= m_s) to S and nothing to D -- then the 64 lane sums go through the six-level xor butterfly (offsets 32 .. 1),
// F = S / K.  A series' result depends on its own components in stored order only: not on the other series, R or the launch shape.
//   bracket   lo0 = min_s (m_s + z_p sd_s), hi0 = max_s (m_s + z_p sd_s), z_p = st_norm_quantile_f(p) formed on the host: at hi0 every
//             component's CDF is >= p, so F >= p; lo0 mirrors it.  M = max(|lo0|, |hi0|).
//   iteration x = the midpoint; each pass moves lo (F < p) or hi (F > p) to x, so F(lo) < p < F(hi) of the evaluated ends; a pass
//             with F == p ends the search at its x.  The next x comes from the evaluated point closest to p, (xb, Fb, fb): its
//             Newton point on the probit scale, xn = xb - (Phi^-1(Fb) - z_p) phi(Phi^-1(Fb)) / fb -- on that scale the CDF of a
//             near-normal mixture is near-linear, in the tails too.  Newton closes in from one side, so once its step |xn - xb| is
//             down to 64 w (w the stopping width: the rounding noise of F over f is of that order) the next x is a probe beyond the
//             root, xn pushed by 2 |xn - xb| + 0.4 w toward the far end, and twice as far every time a pass brings no point closer
//             to p; with hi - lo <= 256 w the rest is bisection.  The midpoint also replaces a candidate that is not finite (f == 0:
//             a gap between modes) or not strictly inside (lo, hi) (a jump of a point mass), and every third pass, which halves the
//             bracket whatever the shape.
//   stop      hi - lo <= w = 2^-51 M, or no double lies strictly between lo and hi.  The result is hi (clamped from below by the result
//             of the previous, smaller p: the quantiles of a series never decrease in p).  At most MIX_Q_MAX_PASSES passes per
//             probability (the forced midpoints need at most 3 x 53 of them); a series that reaches the cap counts in n_unconverged.
//   delta     = 2^-50 M, the width the callers and tests hold the result to: F(x + delta) >= p - eps_F and F(x - delta) <= p + eps_F.
//             Half of it is the stopping width, the other half covers the rounding of the bracket ends themselves (the ends are
//             each off by at most 3 u M = 0.75 x 2^-51 M) where an end was never evaluated.  The two evaluations that decide the
//             result lie in [x - delta, x + delta]: eps_F is taken as the largest of its values at x - delta, x and x + delta.
//   eps_F     the first-order rounding bound of one evaluation of F at a double x, u = 2^-53.  The argument of erfc is behind the
//             subtraction, the root (target yhat: the addition v + tau2 before it), the division and the product with the rounded
//             1 / sqrt 2: dz <= 6 u |z|.  Through Phi that is phi(max(|z| - dz, 0)) dz; erfc itself at 5 ulp (10 u relative, sections 19
//             and 30), the halving exact; the K-term sum of non-negative terms has ceil(K / 64) + 6 additions on its longest chain,
//             and S / K rounds once:
//               eps_F = (1 / K) sum_s [phi(max(|z_s| - dz_s, 0)) dz_s + 10 u Phi_s] + (ceil(K / 64) + 8) u F + 6 x 2^-1074.
//
// k_mix_crps.  G threads per scored point (64 up to K = 64, 128 up to K = 128, else 256; R = 256 / G points a workgroup); points
// whose y_new is NaN are not in the launch's list and cost nothing.  The point's (mu_s, sigma2_s) are staged into two LDS rows.
// Thread g owns the components s = g, g + G, ... in ascending order; the owned component sits in registers and meets, in the
// circulant order, the partners t = (s + j) mod K for j = 1 .. floor((K - 1) / 2), and for even K also j = K / 2 when s < K / 2: each
// unordered pair exactly once, neighbouring lanes read neighbouring LDS words.  Per pair one sqrt, one division, one erf, one exp.
//   order     four accumulators per thread: pair j of an owned s goes to accumulator (j - 1) mod 4 (the loop is unrolled by four, so
//             four independent erf / exp chains are in flight), the j = K / 2 pair to accumulator 0; owned s ascending, j ascending
//             within it.  P = (a0 + a1) + (a2 + a3).  T1 (the terms A(y - mu_s, sigma2_s)) and the diagonal D each in one accumulator,
//             owned s ascending.  Then the xor butterfly (32 .. 1) within each wave, and the G / 64 wave sums added in ascending wave
//             order by the group's first thread:  spread = (D + 2 P) / (2 K^2),  crps = T1 / K - spread.
//   bound     one A: s behind an addition and a root (1.5 u), d (u), the quotient (3.5 u), the product with 1 / sqrt 2 (5.5 u); erf
//             moves by at most the relative error of its argument and is itself taken at 5 ulp (10 u): the first term is off by
//             18 u of itself.  The exponent d^2 / (2 s2) = e is off by 8 u e, and e exp(-e) <= 0.37, so the second term is off by 14.5 u
//             of itself plus 3 u s sqrt(2 / pi) <= 3 u A; one addition: |A^ - A| <= 24 u A.  The sums add non-negative terms: a chain
//             of c additions costs c u of the sum, c1 = ceil(K / G) + 10 for T1 and D, c2 = ceil(K / G) (floor(K / 8) + 2) + 12 for P:
//               |crps^ - crps| <= (27 + c1) u T1 / K + (27 + c2) u spread,     |spread^ - spread| <= (27 + c2) u spread
//             (27 = 24 + the two divisions and the final subtraction): absolute, and small beside crps unless the forecast is far
//             sharper than its error.
#pragma once
#include "predict_points.hpp"
#include "mixture_plan.hpp"

#define MIX_Q_MAX_PASSES 200
#define MIX_CNT_UNCONVERGED 0         // k_mix_quantile's two counters of a launch
#define MIX_CNT_PASSES 1

struct MixStoreArgs {              // k_mix_store: one column of the store
  const double *mean, *var;        // this iteration's cond_mean and clamped cond_var (d_out)
  const double *X, *B, *tsq_inv;   // n x p column-major (NULL: no mu); p x q; q
  const int *pmv;
  const double *last;              // the functionals' 4 x n_fun of this iteration (NULL: none)
  int p, q;
  long long n, n_fun;
  double *m, *v, *mu, *tau2, *fm, *fv;   // the column's n, n, n (NULL without X), q, n_fun, n_fun doubles
};

struct MixQuantileArgs {           // k_mix_quantile
  const double *m, *v;             // [K][n]; target yhat: m = the stored mu
  const double *tau2;              // [K][q], target yhat only (NULL: sd = sqrt(v))
  const int *pmv;                  // margin per series (target yhat)
  int q, K, R, T;
  long long n;
  double p[MIX_MAX_PROBS], z[MIX_MAX_PROBS];   // ascending probabilities and their normal quantiles
  int slot[MIX_MAX_PROBS];         // the caller's index of each: the result goes to out[slot n + i]
  double *out;                     // T x n
  unsigned long long *counters;    // [MIX_CNT_UNCONVERGED]: the series that hit the cap; [MIX_CNT_PASSES]: the passes of the launch
};

struct MixCrpsArgs {               // k_mix_crps
  const double *mu, *v, *tau2;     // [K][n], [K][n], [K][q]
  const double *y;                 // n
  const int *pmv;
  const long long *idx;            // the scored points, ascending
  long long n, n_scored;
  int q, K, R, G;
  double *crps, *spread;           // n each; only the scored points are written
};

int points_mix_store_launch(const MixStoreArgs &A, hipStream_t st);
int points_mix_quantile_launch(const MixQuantileArgs &A, const MixPlan &P, size_t lds_limit, hipStream_t st);
int points_mix_crps_launch(const MixCrpsArgs &A, const MixPlan &P, size_t lds_limit, hipStream_t st);
