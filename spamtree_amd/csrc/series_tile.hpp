// The series tile: what the kernels over a store of saved draws share (k_qtile, k_score_crps, k_series_rank, k_loo_psis,
// k_series_diag).  A store is draws[d * n + i], d < K, i < n; a workgroup stages the draws of R consecutive series into R LDS rows,
// transposed, and the four sorting kernels pad each row to Kpad = 2^k with +inf and sort it.  The functions below hold loads, stores,
// compares and integer index arithmetic only -- no floating-point arithmetic, so every includer gets the same bits from them whatever
// its fp-contraction setting (k_psis.hip compiles with contraction off, the others with the default).
// Not shared, on purpose: the three LDS budget rules (qtile_plan, psis_plan, series_rank_plan: each keeps other arrays beside the
// sorted rows) and the wave sums (diag_allsum, wave_allsum, k_score_crps's loop: each adds in an order of its own, which its header
// documents as part of the result).
// The plain part needs no HIP header (psis_plan.cpp is compiled and checked without a device).
#pragma once

// the smallest power of two >= max(K, 2): the row length of a bitonic sort of K values
static inline long long tile_pow2(long long K) {
  long long kpad = 2;
  while (kpad < K) kpad <<= 1;
  return kpad;
}

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

// R rows of Kpad = 2^k doubles each in LDS (row r at lds + r Kpad), every row sorted ascending by a bitonic network over the nt
// threads of the workgroup.  The rows are in LDS behind a barrier on entry and sorted behind one on return.
__device__ __forceinline__ void tile_sort_rows(double *lds, int R, int Kpad, int tid, int nt) {
  const int half = Kpad >> 1;
  for (int k = 2; k <= Kpad; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int p = tid; p < R * half; p += nt) {
        const int r = p / half, i = p - r * half;
        const int i1 = 2 * j * (i / j) + (i % j), i2 = i1 + j;
        double *a = lds + (size_t)r * Kpad;
        const double x = a[i1], y = a[i2];
        const bool up = (i1 & k) == 0;
        if ((x > y) == up) { a[i1] = y; a[i2] = x; }
      }
      __syncthreads();
    }
  }
}

// Columns d < fill of the rows r < R (row r at lds + r ld): load(d, r) where d < K and r < nr, +inf elsewhere.  nr <= R series of
// the tile exist; load(d, r) reads draw d of series r and may do more (a loader's side effects happen once per staged element).
// No barrier: the caller's follows.
template <typename Load>
__device__ __forceinline__ void tile_stage(double *lds, int R, int ld, int fill, int K, int nr, int tid, int nt, Load load) {
  for (int idx = tid; idx < R * fill; idx += nt) {
    const int d = idx / R, r = idx - d * R;   // R consecutive series of one draw: contiguous in memory
    lds[(size_t)r * ld + d] = (d < K && r < nr) ? load(d, r) : __builtin_inf();
  }
}

// #{a[0 .. K) < v} of the ascending a, and #{a[0 .. K) <= v} given lo = #{a < v}: binary searches (indices stay in [0, K))
__device__ __forceinline__ int sorted_count_below(const double *a, int K, double v) {
  int lo = 0, n = K;
  while (n > 0) {
    const int half = n >> 1;
    if (a[lo + half] < v) { lo += half + 1; n -= half + 1; }
    else n = half;
  }
  return lo;
}
__device__ __forceinline__ int sorted_count_upto(const double *a, int K, double v, int lo) {
  int hi = lo, n = K - lo;
  while (n > 0) {
    const int half = n >> 1;
    if (a[hi + half] <= v) { hi += half + 1; n -= half + 1; }
    else n = half;
  }
  return hi;
}
#endif
