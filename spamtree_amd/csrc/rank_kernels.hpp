// Rank-normalised R-hat, bulk, tail, quantile and exceedance ESS of the stored draws (st_summary_rank_diagnostics,
// st_points_summary_rank_diagnostics, st_points_functionals_rank_diagnostics; the kernel and its launcher live in k_rank.hip).
// include/spamtree_hip.h has the definition; this header restates it in the order the kernel evaluates it.
//
// A store is draws[d * n + i], d < K <= 16384, i < n.  A workgroup of RANK_NT threads takes tiles of R consecutive series, one tile
// after another (the grid is capped: the global slice below is sized by the grid, never by n K).  Per tile, with barriers between
// the steps:
//   1  stage: the R values of one draw are contiguous in memory (k_series_diag's gather).  Series r goes to the workgroup's global
//      slice X (row r at X + r K, read back at unit stride) and to the LDS row S_r (Kpad = 2^k >= K doubles, padded with +inf).
//      A NaN draw marks its series: every double output NaN, lags 0, no further work on it.
//   2  sort S_r ascending, all R rows by one bitonic network over the workgroup.
//      med_r and the quantile thresholds xs[j] (j from the host: one multiplication, ceil, the two clamps) are read off S_r.
//      (Skipped when only exceedance outputs are asked for: they read X alone.)
//   3  ranks: lo_s, hi_s by two binary searches of x_s in S_r (no index array is sorted along);  r2 = lo + hi + 1;
//      z_s = st_rank_score(r2, K) (norm_quantile.hpp) into Z_r.  Z_r is an LDS row (stride K | 1) while K <= RANK_LDS_Z_MAX_K and
//      both fit; beyond that (the padded sorted copy alone is 128 KB at K > 8192) Z_r is a second row of the global slice.
//   4  bulk: one wave per series runs diag_series_wave<true> (diag_kernels.hpp: P1 .. P4 and the lag pairs, k_series_diag's text
//      and order) on Z_r: rhat_bulk, ess_bulk, lags_bulk.
//   5  folded: S_r <- |x_s - med_r| (+inf padding), the sort, the ranks of the same expression, Z_r <- zf, then
//      diag_series_wave<false> (moments only, no lag pass): rhat_fold;  rhat_rank = fmax(rhat_bulk, rhat_fold).
//   6  indicators, one wave per series, one indicator after another (n_prob quantiles, the two tails 0.05 and 0.95, n_thr
//      exceedances): the series as a bit mask, 64 draws per word by __ballot, into the first ceil(K / 64) words of S_r; c = the
//      popcounts.  Lags 64 at a time, lane l takes t = t0 + l and walks the words once:
//        n11_t = sum_w popc(B_w & (B >> t)_w),  first_t = #{s < t : I_s},  last_t = #{s >= K - t : I_s}  (masked popcounts),
//        head_t = c - last_t, tail_t = c - first_t,  A_t = K^2 n11_t - K c (head_t + tail_t) + (K - t) c^2   (int64)
//      then the pairs in order, every lane the same, on the integer numerators: N_k = A_2k + A_2k+1 (Gamma_k = N_k / A_0), stop at
//      !(N_k > 0), N_k <- min(N_k, N_k-1), sum;  tau = max((double)(2 sum N_k - A_0) / (double)A_0, 1 / log10 K), ess = K / tau:
//      diag_kernels.hpp's rules, with integers up to tau's one quotient: no reduction order, no rounding per lag.
// With M >= 2 chains (st_*_chain_rank_diagnostics, k_series_rank<true>; chain c is the draws c N .. (c + 1) N - 1, N = K / M) steps
// 1 to 3 and the folded scores are unchanged -- ranks, scores, the median and xs[j] are those of the pooled K draws -- and
//   4, 5  run diag_chain_wave (diag_kernels.hpp) on Z_r in place of diag_series_wave;
//   6     every chain is balloted into words of its own, ceil(N / 64) per chain, chain c from word c ceil(N / 64) on with the bits
//         at and beyond N clear, so that the lag walk of a chain is the single-chain walk with K -> N on its own words and no mask
//         ever straddles a boundary;  c_c = the chain's popcount, kept in lane c;  C = sum c_c, D = sum (M c_c - C)^2.
//         Lane l takes t = t0 + l and walks chain after chain:  S_t = sum_c A_{c,t} (int64),  Num_t = N D + M (M - 1) S_t
//         (= (M - 1) M^2 N^3 (B' + gbar_t) of the indicator; Num_0 from A_{c,0} = N c_c (N - c_c)), then the pairs on the integers
//         as above: N_k = Num_2k + Num_2k+1, tau = max((double)(2 sum N_k - Num_0) / (double)Num_0, 1 / log10 K), ess = K / tau.
//         N D <= K^3 / 4 and |M (M - 1) S_t| < K^3 / 4 (|A_{c,t}| <= N^3 / 4 by Cauchy-Schwarz), so |Num_t| < K^3 / 2 <= 2^41, a pair
//         is below 2^42, and with at most 2^13 pairs |2 sum N_k - Num_0| < 2^57.  C == 0 or C == K: ess NaN, lags 0.
// The outputs of a series are bitwise a function of its K values and the spec: the sort gives the same values in any network, the
// ranks and the A_t are integers, and the moments of z follow diag_series_wave's fixed order.  No atomics; no inline assembly
// (diag_allsum's DPP moves are st_device.hpp's group_xor_sum).
#pragma once
#include "st_device.hpp"

#define RANK_NT 256              // four waves: the sort wants threads, the moments one wave per series
#define RANK_MAX_R 8             // series per tile at most
#define RANK_TILE (64 * 1024)    // the LDS a workgroup aims for (two workgroups per CU); a longer series takes what the device allows
#define RANK_LDS_Z_MAX_K 8192    // up to here z lives in LDS beside the sorted copy
#define RANK_LDS_STATIC 2048     // room left for the kernel's static LDS (medians, thresholds, flags)
#define RANK_MAX_WGS 1024        // grid cap: four workgroups per CU
#define RANK_SCRATCH_BYTES (64ll << 20)   // and the global slices together stay within this (255 workgroups at K = 16384)
#define RANK_NQ 10               // quantile indicators at most: ST_RANK_MAX_PROBS and the two tails

struct RankArgs {
  const double *draws;   // [K][n]
  long long n;
  int K, Kpad, Kz, R;
  int M;                 // chains the K draws are cut into (1: the single-chain definition and kernel)
  int L;                 // min(max_lag, K / M - 2), max_lag = 0 resolved
  int z_global;          // Z rows in the global slice instead of LDS
  double *scratch;       // gridDim.x slices of `slice` doubles: X (R K) and, with z_global, Z (R Kz)
  long long slice;
  int want_bulk, want_fold;
  int n_prob, want_tail; // indicators 0 .. n_prob - 1: the caller's quantiles; then, with want_tail, 0.05 and 0.95
  int jq[RANK_NQ];       // their order statistics j (jq[8], jq[9]: the tails)
  int n_thr;             // then the exceedances
  unsigned neg;          // bit t: side -1
  const double *thr;     // c_t(i) = thr[t * thr_stride + (per_series ? i : outcome(i))], store order
  long long thr_stride;
  int per_series;
  const int *outcome;    // n, store order; NULL: all 0
  double *rhat_rank, *rhat_bulk, *rhat_fold, *ess_bulk, *ess_tail;   // n each (device), store order; NULL: not wanted
  int *lags_bulk;
  double *ess_q;                       // n_prob x n
  double *ess_exc, *mcse_prob, *prob;  // n_thr x n
};

// R, Kpad, Kz and the route of a store of K draws under a per-workgroup LDS limit; false: the sorted copy of one series does not fit
bool series_rank_plan(long long K, size_t lds_limit, int *R, int *Kpad, int *Kz, int *z_global);
// the order statistic of a probability: min(max(ceil(prob K), 1), K - 1) - 1
int series_rank_order(double prob, long long K);
