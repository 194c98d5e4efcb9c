// points_fun.hpp -- linear functionals F = sum_k a_k value[i_k] of the new-point predictions (st_points_functionals_*), formed on the
// device after every saved iteration from what st_points_accumulate left there: d_out (w*, conditional mean, conditional
// variance, yhat; caller order) and, on a joint set, the packed conditional covariances d_jout.  The term lists are built on the
// host without a HIP call (functionals_layout in points_layout.cpp); the kernels and their launcher live in k_points_fun.hip.
//
// Every functional has two term lists in one format, (coefficient, source index): the linear list -- the caller's terms in the
// caller's order, read once for F_w = a'w*, F_m = a'cond_mean and F_y = a'yhat -- and the variance list, whose sum is
// Var(a'w* | w, theta): (a_i^2, i) into cond_var on a plain set; on a joint set, per group the functional touches (layout
// order) the pairs a >= b of its members there in column-major order, (a_a a_b, doubled off the diagonal; j_off[g] + a + b g)
// into the packed Sigma.  Each list is cut into chunks of FUN_CHUNK terms; a chunk never spans two functionals.
//
// THE SUMMATION ORDER (part of the contract; the tests' rounding bound is derived from it).  For one list of one functional:
//   1. chunk c holds terms [FUN_CHUNK c, FUN_CHUNK (c + 1)) of the list.  One wave takes it; lane l adds its terms
//      l, l + 64, l + 128, ... in that order into s_l, starting from 0, as s_l = fma(coefficient, value, s_l): one rounding a term.
//   2. the 64 lane sums are combined by the xor butterfly s_l += s_(l xor o) for o = 32, 16, 8, 4, 2, 1: six roundings, every lane
//      ends with the same bits.
//   3. one thread adds the functional's chunk sums in chunk order, starting from 0, and clamps F_v at 0.
// So a term passes through at most ceil(min(terms, FUN_CHUNK) / 64) + 6 + chunks roundings of partial sums that are each at most
// sum |coefficient value| in magnitude: |F - exact| <= (that count) 2^-53 sum |coefficient value|, first order.  No atomics; a
// functional's values depend on its own term lists and the source vectors only -- not on the other functionals, their order or
// the launch shape.  A functional without terms has no chunk and is 0.
#pragma once
#include "predict_points.hpp"

#define FUN_CHUNK 1024             // terms per chunk (one wave: 16 per lane)

struct alignas(16) FunTerm {
  double c;                        // coefficient
  long long src;                   // index into the source vector
};
struct FunChunk {
  long long t0;                    // first term, in its list
  int nt, fun;                     // terms (1..FUN_CHUNK); the functional they belong to -- no kernel reads it (the host checker
                                   // does): it fills what would be padding of the 16-byte record
};

// per-functional accumulators: PA_NACC arrays of n_fun doubles, laid out and updated as PointsAccArgs::acc
struct FunArgs {
  const FunTerm *lin, *var;              // the two term lists
  const FunChunk *lin_chunks, *var_chunks;
  const long long *lin_cptr, *var_cptr;  // n_fun + 1 each: the chunks of functional f in its list
  long long n_lin_chunks, n_var_chunks, n_fun;
  const double *w, *mean, *yhat;         // sources of the linear list, caller order (yhat NULL: no regressors)
  const double *vsrc;                    // source of the variance list: cond_var, or the packed Sigma of a joint set
  double *part;                          // [n_lin_chunks + n_var_chunks][4]: w, mean, yhat of a linear chunk; [3] of a variance chunk
  double *acc;                           // PA_NACC x n_fun
  double *last;                          // 4 x n_fun: F_w, F_m, F_v, F_y of this iteration
  double *keep_w, *keep_yhat;            // row of this draw in the [keep][n_fun] stores, or NULL
  double count;                          // iterations accumulated including this one
};
int points_fun_launch(const FunArgs &A, hipStream_t st);
