// Joint new-point prediction (st_points_set_joint, st_points_predict_joint): a joint group G is 1..PJ_MAXG new points that share
// one conditioning chain S and are predicted together.  With V = Linv_S K(S, G) and u = Linv_S w_S (predict_points.hpp):
//   mean = V'u (per point, as k_points_*),  Sigma = K(G, G) - V'V,  L = lower Cholesky factor of Sigma in member order,
//   w_G = mean + L z_G,  yhat = x'beta_j + w + sqrt(tausq_j) eps         (z, eps: Philox streams 6 / 7, per-point counters)
// A pivot d_j that is not above (P + g) 2^-52 K(x_j, x_j) (P chain rows: the rounding bound of the P + g products behind it) counts
// as zero: L_jj = 0 and the column below it is zero, so z_j is not used; row j keeps what the earlier pivots explain (a duplicate
// of an earlier member repeats that member's draw, a point on a conditioning row gets its conditional mean to rounding).
//
//   k_points_joint_mfma<PMAX>  k_points_mfma's pass over the chain, on 16-column slots that the host fills with whole groups
//                              (padding columns repeat a member's coordinates and write nothing).  Each wave also accumulates the
//                              16 x 16 Gram V'V of its slot: in the accumulator layout c[r] of a lane is element (point l15,
//                              k = l4) of A = V' and element (k = l4, point l15) of B = V for chain rows l4 + 4 r, so four
//                              v_mfma_f64_16x16x4_f64 per sub-panel, rows beyond the sub-panel masked to zero.  Epilogue per
//                              wave in the (then free) staging LDS: the lane of a group's first column forms Sigma, factorises it
//                              in place and draws; then every column writes its point's outputs.
//   k_points_joint_generic     any chain: one workgroup per joint group, K(S, G), V (g columns), w_S and u in a global scratch
//                              slice, one wave per chain row, the Gram by one thread per pair a >= b in chain-row order.
// A group's mean, Sigma, L and draws from a caller's z depend on its chain and its own members only: the Gram entry (a, b) is a
// fixed-order sum over the chain rows of products of columns a and b, whatever else shares the slot, workgroup or point set.
#pragma once
#include "predict_points.hpp"

#define PJ_MAXG ST_POINTS_MAX_JOINT
#define PJ_LD 17                   // row stride of a 16 x 16 Gram in LDS
#define PJ_WAVE_LDS 400            // doubles of epilogue LDS per wave: Gram, member coordinates, mean, draw, work, margins
#define PJ_SCRATCH_COLS (2 * PJ_MAXG + 2)   // k_points_joint_generic: K(S, G), V, w_S, u -- scratch_stride doubles each

struct PtJoint {       // one joint group, in layout order (first appearance in the caller's order)
  long long cov_off;   // its g x g column-major block in the packed cov / chol outputs
  int first;           // into JointArgs::members
  int g;               // members
  int chain, pad;
};
struct PtCol {         // a column of a k_points_joint_mfma slot: member a of group grp; a < 0: padding (grp lends its first member)
  int grp, a;
};

struct JointArgs {
  PointsArgs P;                  // tiles: 4 slots of 16 columns, one chain (np: slots in use)
  const PtJoint *groups;
  const long long *members;      // caller indices, group by group in member order
  const PtCol *cols;             // k_points_joint_mfma: 64 per tile of this launch
  const int *gen_groups;         // k_points_joint_generic: its groups
  int ngen_groups;
  double *cov, *chol;            // packed by PtJoint::cov_off, either may be NULL
};

// route codes of st_points_info for the joint kernels, after predict_points.hpp's (same bit set: bit code - 1)
#define PP_ROUTE_JOINT_MFMA128 (PP_ROUTE_COUNT + 0)
#define PP_ROUTE_JOINT_MFMA256 (PP_ROUTE_COUNT + 1)
#define PP_ROUTE_JOINT_GENERIC (PP_ROUTE_COUNT + 2)
#define PP_ROUTE_JOINT_END (PP_ROUTE_COUNT + 3)
const char *points_joint_route_name(int code);   // NULL outside [PP_ROUTE_JOINT_MFMA128, PP_ROUTE_JOINT_END)

struct JointLaunch {
  int ntile128, ntile256;        // tiles (and 64 cols each) [0, ntile128) take <128>, the next ntile256 <256>
  int grid_generic;
};
int points_joint_launch(const JointLaunch &L, const JointArgs &J, const CovPar &cp, hipStream_t st, int *route_mask);

// pair accumulators of st_points_accumulate on a joint set (k_points_pair_acc in k_predict_joint.hip): pacc holds two arrays packed as
// cov -- the running sum of Sigma_ab and the Welford co-moment of the conditional means -- for a >= b; launched BEFORE k_points_acc
// of the same iteration, whose Welford means (PA_MEAN) it reads as the previous iteration's.
struct PointsPairArgs {
  const double *mean, *cov;      // this iteration's conditional means (caller order) and packed Sigma
  const double *acc;             // PA_NACC x n of PointsAccArgs
  double *pacc;                  // 2 x cov_total
  const PtJoint *groups;
  const long long *members;
  const int *pt_grp, *pt_a;      // per point, caller order: its group and member index
  double count;
  long long n, cov_total;
};
int points_pair_acc_launch(const PointsPairArgs &A, hipStream_t st);
