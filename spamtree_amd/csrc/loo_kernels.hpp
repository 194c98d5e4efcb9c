// Leave-one-out criteria with the latent field integrated out (st_rows_loo_*; kernels and launchers in k_rows_loo.hip, the
// launch structures in loo_layout.hpp).
//
// THE DENSITY.  w ranges over the blocks that take part in the density the sampler targets: the blocks with observed rows;
// blocks that hold only NA rows (prediction blocks) are left out.  For block u, L_u is its m x (P + m) panel of slot 0, placed at
// the columns [rows of parents(u) in chain order ; rows of u]: [-Ri H | Ri] for a reference block (Ri lower triangular), and for a
// non-reference row i [-r_i H_i | r_i] with r_i at its own column.  Q = sum_u L_u' L_u is the prior precision of w.
//
// PER SAVED DRAW s, from the current w, XB, tausq_inv and slot 0, for row i of margin j:
//   d_i = Q_ii = sum_u sum_r L_u[r,i]^2,   e_u = L_u [w_pa(u); w_u],   c_i = (Qw)_i = sum_u sum_r L_u[r,i] e_u[r],
//   v_i = 1 / d_i,   m_i = w_i - c_i / d_i       (w_i | w_-i, theta ~ N(m_i, v_i); a non-reference row: H_i w_pa and 1 / r_i^2),
// and when the row has an observed y_i:
//   mu_s = XB_i + m_i,  sigma2_s = v_i + 1 / tausq_inv_j,  sigma = sqrt(sigma2_s),  z = (y_i - mu_s) / sigma,
//   l_s = fma(-z / 2, z, -log sigma) + HL2PI,   Phi_s = erfc(-z / sqrt 2) / 2.
// OVER THE S DRAWS, with weights r_s = exp(-l_s):
//   elpd_loo = -log((1/S) sum r_s),  pit_loo = sum r_s Phi_s / sum r_s,  mu_loo = sum r_s mu_s / sum r_s,
//   weight_ess = (sum r_s)^2 / sum r_s^2.
// E_post[1 / p(y_i | w_-i, theta, beta, tau2)] = 1 / p(y_i | y_-i), so elpd_loo estimates log p(y_i | y_-i).  These are the raw
// weights, with weight_ess as their diagnostic; with a store reserved (st_rows_loo_reserve) every draw's (t, Phi, mu) is kept as
// well -- NaN in all three where the draw is skipped -- and psis_kernels.hpp smooths the tail and gives khat.  The store changes
// nothing of what is described here.
//
// STREAMING STATE, LOO_NACC arrays of n doubles in device row order, all zero = no draw yet.  With t = -l_s:
//   no draw yet (A1 == 0):  M = t;  A1 = 1;  A2 = 1;  AP = Phi;  AM = mu
//   t <= M:   x = exp(t - M);            A1 = A1 + x;  A2 = fma(x, x, A2);  AP = fma(x, Phi, AP);  AM = fma(x, mu, AM)
//   t >  M:   x = exp(M - t);  x2 = x x; A1 = fma(A1, x, 1);  A2 = fma(A2, x2, 1);  AP = fma(AP, x, Phi);  AM = fma(AM, x, mu);  M = t
// A draw whose l_s is not finite (tausq_inv of 0 or infinity, a NaN in w) is skipped: the five values stay bit for bit and NS, the
// sixth array, counts it (st_rows_score_* instead counts such a draw in S; here S_i = S - NS_i is the number of weights in the sums).
//   elpd_loo = -(M + log(A1 / S_i)),  pit_loo = AP / A1,  mu_loo = AM / A1,  weight_ess = A1 A1 / A2       (NaN when S_i = 0)
// TOTALS per outcome over its observed rows, LOO_NSUM values: sum elpd_loo, sum (y - mu_loo)^2 (fma), sum pit_loo, min weight_ess;
// one workgroup per outcome, thread t walks rows t, t + NT, ... ascending, then a fixed binary tree over the NT threads in LDS.
//
// THE KERNEL.  One launch per level from the deepest to the root; k_loo_block<REF, PAIRS>: one workgroup of NT threads per block
// (PAIRS: the pair part of the leave-group-out criteria behind step 5, lgo_kernels.hpp; it changes nothing of steps 0 - 5).
//   0. x[k], k < P + m: the w of the chain's rows, then the block's own, into LDS.
//   1. e[r], wave r mod 4 of the workgroup: lane l adds the terms L[r,k] x[k] of the columns k = l, l + 64, ... in ascending order
//      by fma from 0 (a reference row r has the columns k <= P + r; a non-reference row its P chain columns and then, as column
//      P, r_i x[P + r]), then wave_allsum (st_device.hpp: rotate-and-add in rows of 16 lanes by 8, 4, 2, 1, then the four row sums in
//      lane order).  e stays in LDS.
//   2. thread per column k: own_d = fma(L[r,k], L[r,k], own_d), own_c = fma(L[r,k], e[r], own_c), both from 0, over the rows r in
//      ascending order that hold the column (a chain column: every row; own column P + i: rows r >= i of a reference block, row i
//      alone of a non-reference one).  The panel's second read comes from L2: a block's panel is at most a few hundred KB.
//   3. the children's prefixes are added one after another in list order (ascending device block id): d += S_ch.d[k], c += S_ch.c[k].
//   4. S_u is written.
//   5. the thread of an own column P + i finishes row i: d_i, c_i -> v_i, m_i -> q_diag, qw, cond_mean, cond_var of _last and, on
//      a row with an observed y, the update above.
// No FP64 atomics; nothing depends on the launch geometry: a row's values are a function of the tree, the panels and w.
//
// ROUNDING.  d_i and c_i are sums of products in one documented chain of additions.  With u = 2^-53, first order:
//   |d_i - exact| <= (T_i + 1) u sum |L[r,i]|^2
//   |c_i - exact| <= (T_i + E + 1) u sum_u sum_r |L_u[r,i]| sum_k |L_u[r,k] x[k]|
// T_i = the number of additions the earliest term can pass = the non-zero entries of column i over all panels + the child vectors
// added on the way up (at most the column's entries again);  E = ceil((P + m) / 64) + 7, the additions of one e[r] (lane chain,
// four rotate-and-adds, three row sums), taken at the longest chain that holds the column.
#pragma once
#include "st_device.hpp"

#define LOO_M 0
#define LOO_A1 1
#define LOO_A2 2
#define LOO_AP 3
#define LOO_AM 4
#define LOO_NS 5
#define LOO_NACC 6

#define LOO_LAST_QD 0     // the last draw's per-row values, LOO_NLAST arrays of n doubles in device row order
#define LOO_LAST_QW 1
#define LOO_LAST_MEAN 2
#define LOO_LAST_VAR 3
#define LOO_NLAST 4

#define LOO_OUT_ELPD 0    // the per-row outputs, LOO_NOUT arrays of n; NaN where a row has no observed y
#define LOO_OUT_PIT 1
#define LOO_OUT_MU 2
#define LOO_OUT_ESS 3
#define LOO_NOUT 4

#define LOO_SUM_ELPD 0
#define LOO_SUM_SQERR 1
#define LOO_SUM_PIT 2
#define LOO_MIN_ESS 3
#define LOO_NSUM 4

#define LOO_ROUTE_REF 1   // route codes of st_rows_loo_info (a bit set: bit code - 1 = that kernel runs on some level)
#define LOO_ROUTE_LEAF 2
#define LOO_ROUTE_COUNT 3

struct LooArgs {
  const Blk *blks;
  const int *anc_idx;
  const int *list;               // this level's device block ids
  int nlist;
  const double *panels;          // slot 0 arena
  const double *w, *xb, *y, *tsq_inv;
  const unsigned char *obs;
  const int *mv;
  const long long *voff;         // per device block, into S
  const int *ch_ptr, *ch_idx;
  double *S;                     // the upward vectors
  double *last;                  // LOO_NLAST x n
  double *acc;                   // LOO_NACC x n
  long long n;
  double *st_t, *st_phi, *st_mu; // this draw's column of st_rows_loo_reserve's store (n each), or all NULL: no store
  // the pair part of the leave-group-out criteria (lgo_kernels.hpp), or all NULL: k_loo_block<REF, false>
  const int *pr_ptr, *pr_a, *pr_b, *pr_fin;   // per device block (CSR) its pair list; the slot in pairval where a pair finishes, or -1
  double *pairval;
};

struct LooFinishArgs {
  const double *y;
  const unsigned char *obs;
  const int *mv;
  const double *acc;
  long long n;
  double S;
  int q;
  double *rows;                  // LOO_NOUT x n
  double *tot;                   // q x LOO_NSUM
};

#define LOO_LDS(maxLen, maxM) (((size_t)(maxLen) + (size_t)(maxM)) * sizeof(double))

struct LooLevelLaunch { int first, count, isref, maxLen, maxM; };
// the whole upward sweep on `st` (no synchronisation); *route_mask gets bit code - 1 of each route taken.  With A.pr_ptr set the
// instantiations with the pair part run (voff then counts the p part of every S_u)
int loo_launch(const LooLevelLaunch *lv, int nlev, const LooArgs &A, hipStream_t st, int *route_mask);
int loo_finish_launch(const LooFinishArgs &A, hipStream_t st);
const char *loo_route_name(int code);
