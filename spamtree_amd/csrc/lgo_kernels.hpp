// Leave-group-out criteria with a group's rows of the latent field integrated out jointly (st_rows_loo_groups_*; the pair part
// of the upward sweep lives in k_loo_block<REF, true> of k_rows_loo.hip, k_lgo_groups and k_lgo_finish in k_rows_lgo.hip, the
// index structures in lgo_layout.hpp).  loo_kernels.hpp defines the density, the panels L_u, d_i = Q_ii and c_i = (Qw)_i.
//
// A GROUP G is 1 .. LGO_MAX_MEMBERS rows of the density with one label, in ascending model row; o are its members with an observed y.
// PER SAVED DRAW, after the sweep that gives d and c:
//   A = Q_GG:  A_ii = d_i,  A_ij = p_ij = sum_u sum_r L_u[r,i] L_u[r,j]  (0 where no panel holds both columns),
//   c_G = (Qw)_G,   V = A^-1,   m_G = w_G - V c_G                  (w_G | w_-G, theta ~ N(m_G, V)),
//   mu_o = XB_o + m_o,   Sigma = V_oo + diag(1 / tausq_inv_{j(a)}),
//   l_s = log N(y_o; mu_o, Sigma) = -z'z / 2 - sum_a log L_aa + g_o HL2PI,  L L' = Sigma,  L z = y_o - mu_o,
//   Phi_a = erfc(-(y_a - mu_a) / sqrt(Sigma_aa) / sqrt 2) / 2   per observed member.
// A member without an observed y is integrated out with the group and not scored.
// OVER THE DRAWS, r_s = exp(-l_s):  elpd_lgo = -log mean r_s,  weight_ess = (sum r)^2 / sum r^2,  mu_lgo_a and pit_lgo_a weighted by
// r_s.  E_post[1 / p(y_G | w_-G, theta, beta, tau2)] = 1 / p(y_G | y_-G), so elpd_lgo estimates log p(y_G | y_-G).
//
// THE PAIR PART OF THE SWEEP (k_loo_block<REF, true>, after steps 2 - 5 of loo_kernels.hpp; d, c and the rows' state are computed
// by the same instructions with and without it).  S_u has a third part of n_pairs_u doubles behind d and c.  One thread per pair
// slot t = (a, b), a < b:
//   p = fma(L[r,a], L[r,b], p) from 0 over the rows r ascending that hold both columns: every row when b < P; the rows r >= b - P of
//   a reference block when b >= P; the single product L[b - P, a] r_{b-P} of a non-reference block (a < P);
//   then p += S_ch.p[t] over the children in list order (a child's first n_pairs_u slots are this block's pairs);
//   S_u.p[t] = p, and where the pair finishes here (b >= P) the per-pair array gets p.
// No FP64 atomics; a pair's value is a function of the tree, the panels and the labels.
//   |p_ij - exact| <= (T_ij + 1) u sum |L[r,i] L[r,j]|,  T_ij = the rows over all panels that hold both columns + the child vectors
//   added on the way up (at most those rows again).
//
// k_lgo_groups: 16 lanes per group, four groups per workgroup of one wave; lane i owns row i of the group's matrices in LDS.
//   1. gather A (lower triangle and diagonal), c, w.
//   2. chol16, the unpivoted right-looking Cholesky A = L L': for k ascending: s = sqrt(A_kk); L_ik = A_ik / s (i > k);
//      A_ij = fma(-L_ik, L_jk, A_ij) for k < j <= i.  A pivot that is not > 0 marks the draw.
//   3. lane j solves A v = e_j: z_i = (e_i - sum_{k<i} L_ik z_k) / L_ii for i ascending, k ascending by fma;
//      v_i = (z_i - sum_{k>i} L_ki v_k) / L_ii for i descending, k ascending by fma.  V[., j] = v.
//   4. m_i = w_i - sum_j V[i,j] c_j, j ascending by fma from 0.
//   5. Sigma's lower triangle from row i of V over the observed members before it, 1 / tausq_inv added on the diagonal; chol16;
//      lane 0: z by forward substitution (as 3.), quad = fma(z_a, z_a, quad), ld = ld + log L_aa, both from 0 in member order,
//      l = fma(-0.5, quad, -ld) + g_o HL2PI.
//   6. the streaming update of loo_kernels.hpp (STREAMING STATE) with t = -l: (M, A1, A2) per group, (AP, AM) per observed member.
//      A pivot of either Cholesky that is not > 0, or an l that is not finite, skips the draw for the group: its values stay bit
//      for bit and NS counts it.
// With a store (st_rows_loo_reserve) the draw's log ratio t = -l of every group is kept as well, NaN where the draw is skipped, for
// the Pareto smoothing of psis_kernels.hpp (one series per group, no companions); the store changes nothing else.
// The last draw's A, c_G, m_G and V are kept for st_rows_loo_groups_last (written also on a skipped draw).
//
// ROUNDING of one draw, given A and c.  g the group's size, g_o its observed members, u = 2^-53, kappa_A and kappa_S the 2-norm
// condition numbers of A and Sigma, lam the smallest eigenvalue of Sigma.  The Cholesky solves are backward stable (Higham, Accuracy
// and Stability of Numerical Algorithms, Th. 10.4: (A + dA) x = b with |dA| <= gamma_{3g+1} |L||L'|); to first order, with a factor
// 4 for the norm of |L||L'| and the g solves behind V,
//   ||V - A^-1||_2 <= eV ||V||_2,   eV = 4 g (3 g + 1) u kappa_A
//   |m_i - exact| <= dm = (eV + (g + 2) u) ||V||_2 ||c||_1 + u max |w_G|,    |mu_a - exact| <= dmu = dm + 2 u max |mu|
//   Sigma's perturbation relative to lam:  eS = eV ||V||_2 / lam + 4 g_o (3 g_o + 1) u kappa_S
//   |l - exact| <= dl = eS (z'z + g_o) / 2 + sqrt(z'z / lam) sqrt(g_o) dmu + u (|l| + 4 g_o + 4)
//   a member's standardised residual (at most sqrt(z'z) in size):  dz = dmu / min sqrt(Sigma_aa) + (eS + 4 u) sqrt(z'z),  dPhi <= 0.4 dz + 4 u
// tests/test_gpu_rows_lgo.py evaluates these from the long-double reference's own kappa_A, kappa_S, V and z'z at the device's A and c;
// the outputs over the draws then follow as for the rows (each update adds one rounding per sum).
//
// FINISH (k_lgo_finish, q + 1 workgroups).  Workgroup q: thread t walks the groups t, t + NT, ... ascending: elpd_lgo =
// -(M + log(A1 / S_G)), weight_ess = A1 A1 / A2 (NaN when S_G = S - NS = 0), and sums elpd, the minimum of weight_ess and the count,
// then in a second pass over the same groups (elpd - mean)^2 by fma, the centred sum of squares behind the standard error;
// workgroup v < q walks the members of outcome v: mu_lgo = AM / A1, pit_lgo = AP / A1 into the row arrays and sums
// (y - mu_lgo)^2 (fma), pit_lgo and the count.  Then a fixed binary tree over the NT threads in LDS.
#pragma once
#include "loo_kernels.hpp"

#define LGO_MAXG 16       // = LGO_MAX_MEMBERS of lgo_layout.hpp
#define LGO_WG 64         // threads of a k_lgo_groups workgroup: four groups

#define LGO_M 0           // the groups' state, LGO_NGACC arrays of n_groups doubles
#define LGO_A1 1
#define LGO_A2 2
#define LGO_NS 3
#define LGO_NGACC 4
#define LGO_AP 0          // the members' state, LGO_NMACC arrays of n_members doubles
#define LGO_AM 1
#define LGO_NMACC 2

#define LGO_TOT_ELPD 0    // workgroup q's sums
#define LGO_TOT_ELPD_SQ 1  // centred: sum (elpd - mean)^2
#define LGO_TOT_MIN_ESS 2
#define LGO_TOT_COUNT 3
#define LGO_NTOT 4
#define LGO_OUT_SQERR 0   // per outcome
#define LGO_OUT_PIT 1
#define LGO_OUT_COUNT 2
#define LGO_NOUTC 3

struct LgoArgs {
  int G;
  long long n;
  const int *grp_ptr;            // G + 1
  const long long *mem_row;      // device rows
  const int *gp_ptr, *gp_idx;    // per group g (g - 1) / 2 slots of pairval, -1: a structural zero
  const int *sq_ptr;             // G + 1: where a group's g x g matrices start in last_q / last_v
  const double *pairval;
  const double *last;            // LOO_NLAST x n of this draw's sweep
  const double *w, *xb, *y, *tsq_inv;
  const unsigned char *obs;
  const int *mv;
  double *last_q, *last_v;       // row-major g x g per group
  double *last_c, *last_m;       // n_members
  double *gacc;                  // LGO_NGACC x G
  double *macc;                  // LGO_NMACC x n_members
  double *st_t;                  // this draw's column of the groups' store (G log ratios t = -l, NaN where skipped), or NULL: no store
};

struct LgoFinishArgs {
  int G, q;
  long long n, n_members;
  double S;
  const int *mem_grp;            // member -> group
  const long long *mem_row;
  const double *y;
  const unsigned char *obs;
  const int *mv;
  const double *gacc, *macc;
  double *gout;                  // 2 x G: elpd_lgo, weight_ess
  double *rows;                  // 2 x n: mu_lgo, pit_lgo; NaN off the observed members (filled at set)
  double *tot;                   // LGO_NTOT, then q x LGO_NOUTC
};

int lgo_groups_launch(const LgoArgs &A, hipStream_t st);
int lgo_finish_launch(const LgoFinishArgs &A, hipStream_t st);
