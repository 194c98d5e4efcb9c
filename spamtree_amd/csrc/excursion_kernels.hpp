// Exceedance probabilities, excursion functions and simultaneous bands of the stored draws (st_summary_excursions,
// st_points_summary_excursions, st_points_functionals_excursions; the kernels and their launcher live in k_excursions.hip).
// include/spamtree_hip.h has the definition; k_excursions.hip restates it beside the code that evaluates it.
//
// A store is draws[d * n + i], d < K <= 16384, i < n: a draw is one contiguous row of n doubles, and both passes read it as such.
//   pass 1  k_store_colstats     a thread owns one series and walks d ascending, EXC_UNROLL draws' loads in flight; every load
//                                instruction of a wave is one contiguous 512 B segment of a draw's row.  count_t for all T
//                                thresholds and, with the band, the Welford mean / sd, in one read of the store.
//   pass 2  k_store_drawreduce   a workgroup takes a tile of EXC_NT x S series and a chunk of draws; count_t, c_t, the domain, the
//                                mean and 1 / sd of its series stay in registers across the chunk.  Per draw and (t, g) the
//                                int32 max m_{t,g} and per g the double max maxdev_g over the tile: count + 1 <= 16385 fits 16
//                                bits (0: no failing series), so two thresholds share a register and one packed 16-bit max
//                                serves both; four DPP steps (row_ror 8, 4, 2, 1) inside each row of 16 lanes, one LDS slot per
//                                row, and after EXC_BATCH draws one integer atomicMax per (t, g, d) of the tile into m[t][g][d]
//                                (maxdev: its bit pattern as an unsigned 64-bit integer, order-preserving for non-negative
//                                doubles).  With G > 1 the series of a tile belong to different domains: the row reduction is
//                                made once per domain, ceil(T / 2) G packed and G double reductions per draw and wave (T = 8,
//                                G = 6: 24 + 6 of them, eight and twelve VALU instructions each, and 6 masked LDS writes; about
//                                350 VALU instructions per draw and wave beside the S loads per lane).
//   finish  k_exc_hist, k_exc_scan, k_exc_apply: per (t, g) the histogram of m(d) by integer atomicAdd, its running sum
//                                H[c] = #{d : m(d) < c}, c = 0 .. K, in place, joint_all = H[0] / K, then
//                                excur_t(i) = H[count_t(i)] / K and prob_t(i) = count_t(i) / K per series.
// Every reduction over series is an integer max, an integer sum or a max of non-negative doubles: its value does not depend on the
// tiles, the chunks or the order of the atomics.  No floating-point atomics, no scratch, no inline assembly.
#pragma once
#include "st_device.hpp"

#define EXC_NT 256        // threads of a workgroup, both passes
#define EXC_UNROLL 8      // pass 1: draws in flight per thread
#define EXC_BATCH 16      // pass 2: draws between two workgroup barriers
#define EXC_MAX_G 6       // ST_MAX_Q domains at most
#define EXC_MIN_WGS 2048  // pass 2 splits the draws into chunks until the grid has about this many workgroups

struct ExcArgs {
  const double *draws;          // [K][n]
  long long n;
  int K, T, G;
  const int *outcome;           // n, store order; NULL: all 0
  const unsigned char *mask;    // n, store order, 0 = out of every domain; NULL: all in
  const double *thr;            // c_t(i) = thr[t * thr_stride + (per_series ? i : outcome(i))]
  long long thr_stride;
  int per_series;
  unsigned neg;                 // bit t: side -1
  const double *rinv;           // K: 1 / (d + 1)
  int *count;                   // [T][n]
  double *mean, *sd;            // n each
  unsigned long long *n_flat;   // G
  int *m;                       // [T G][K], starts at -1
  unsigned long long *dev;      // [G][K], bit patterns of non-negative doubles, starts at 0
  int chunk;                    // draws per workgroup of pass 2, a multiple of EXC_BATCH
  int *hist;                    // [T G][K + 2]: bin m + 1, then in place H[c]
  double *prob, *excur;         // [T][n]
  double *joint_all;            // [T G]
};
