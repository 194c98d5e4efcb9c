// Kernel translation unit of libspamtree_hip.so: the criteria over the fit's own rows (rows_score.hpp has the definitions).
// k_rows_score_acc reads the target vector, d_obs, d_mv, d_xb, d_w and d_tsq, draws nothing and writes only the criteria's state;
// k_rows_score_totals reads that state and writes the per-row outputs and the partial sums: no other step reads what they write.
#include "rows_score.hpp"
#include "misc_kernels.hpp"

// One thread per row, device row order; every array is read and written at index i: coalesced.  A row without a target returns
// after reading tgt[i] (8 B).  A targeted row reads tgt, obs, mv, xb, w (29 B) and five state values (40 B; a held-out row six, 48 B)
// and writes them back.  No atomics, no LDS, no private array.  In order:
//   mu = xb + w;  sigma = sqrt(1 / tausq_inv_j);  r = (t - mu) / sigma;  l = fma(-r / 2, r, -log sigma) + HL2PI;
//   MU += (mu - MU) / S;  sc_lse(l, M, A);
//   when l is finite:  d = l - LM;  LM += d / S;  LM2 = fma(d, l - LM, LM2);
//   on a held-out row, when r is a number:  PHI += erfc(-r / sqrt 2) / 2.
__global__ __launch_bounds__(NT) void k_rows_score_acc(RowsScoreArgs A) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  const double t = A.tgt[i];
  if (!(t == t)) return;   // no target
  const long long n = A.n;
  const double mu = A.xb[i] + A.w[i];
  const double sig = sqrt(1.0 / A.tsq_inv[A.mv[i]]);
  const double r = (t - mu) / sig;
  const double l = fma(-0.5 * r, r, -log(sig)) + HL2PI;
  const double MU = A.acc[RS_MU * n + i];
  A.acc[RS_MU * n + i] = MU + (mu - MU) / A.S;
  double M = A.acc[RS_M * n + i], Sa = A.acc[RS_A * n + i];
  sc_lse(l, M, Sa);
  A.acc[RS_M * n + i] = M;
  A.acc[RS_A * n + i] = Sa;
  if (l >= -__DBL_MAX__ && l <= __DBL_MAX__) {   // (a density of 0, or r = 0 / 0: the moments of l stay)
    double LM = A.acc[RS_LM * n + i];
    const double d = l - LM;
    LM += d / A.S;
    A.acc[RS_LM * n + i] = LM;
    A.acc[RS_LM2 * n + i] = fma(d, l - LM, A.acc[RS_LM2 * n + i]);
  }
  if (!A.obs[i] && r == r) A.acc[RS_PHI * n + i] += 0.5 * erfc(-r * 0.70710678118654752440);
}

// The per-row outputs and the per-outcome sums, in the manner of k_stats: workgroup g owns the rows of chunk g of ceil(n / STATS_WG)
// rows, a thread walks every NT-th row of it serially, then block_sum; k_stats_final adds the STATS_WG partial sums in its fixed
// tree.  A row of margin v adds to s[v][.] only, under the predicate v == vv of a fully unrolled loop: every accumulator has a
// compile-time index (a register; no private array indexed at run time), and a skipped accumulator keeps its bits.
// Per targeted row, in order: lppd = M + log(A / S);  p_waic = S > 1 ? LM2 / (S - 1) : 0;  e = t - MU;
//   observed:  sb = sqrt(tau2bar_v);  rb = e / sb;  logn = fma(-rb / 2, rb, -log sb) + HL2PI;
//              s[v][0..3] += lppd, p_waic, LM, logn
//   held out:  pit = PHI / S;  s[v][4..6] += lppd, pit, crps_i (0 without stored draws);  s[v][7] = fma(e, e, s[v][7]).
// A row without a target writes NaN to its outputs and adds nothing.
template <int Q>
__global__ __launch_bounds__(NT) void k_rows_score_totals(RowsTotalsArgs A) {
  __shared__ double s_red[NT / 64];
  const long long n = A.n;
  const double nan = __builtin_nan("");
  double s[Q][RS_NSUM];
#pragma unroll
  for (int vv = 0; vv < Q; ++vv) {
#pragma unroll
    for (int k = 0; k < RS_NSUM; ++k) s[vv][k] = 0.0;
  }
  const long long chunk = (n + gridDim.x - 1) / gridDim.x;
  const long long lo = (long long)blockIdx.x * chunk, hi = min(n, lo + chunk);
  for (long long i = lo + threadIdx.x; i < hi; i += NT) {
    const double t = A.tgt[i];
    if (!(t == t)) {
#pragma unroll
      for (int k = 0; k < RS_NOUT; ++k) A.rows[k * n + i] = nan;
      continue;
    }
    const int v = A.mv[i];
    const bool ob = A.obs[i] != 0;
    const double LM = A.acc[RS_LM * n + i], MU = A.acc[RS_MU * n + i];
    const double lppd = A.acc[RS_M * n + i] + log(A.acc[RS_A * n + i] / A.S);
    const double pw = A.S > 1.0 ? A.acc[RS_LM2 * n + i] / (A.S - 1.0) : 0.0;
    const double e = t - MU;
    double pit = nan, logn = 0.0, cr = 0.0;
    if (ob) {
      double sb = 1.0;
#pragma unroll
      for (int vv = 0; vv < Q; ++vv)
        if (v == vv) sb = A.tau2bar[vv];
      sb = sqrt(sb);
      const double rb = e / sb;
      logn = fma(-0.5 * rb, rb, -log(sb)) + HL2PI;
    } else {
      pit = A.acc[RS_PHI * n + i] / A.S;
      if (A.crps) cr = A.crps[i];
    }
    A.rows[RS_OUT_LPPD * n + i] = lppd;
    A.rows[RS_OUT_MEANLL * n + i] = LM;
    A.rows[RS_OUT_PWAIC * n + i] = pw;
    A.rows[RS_OUT_MUMEAN * n + i] = MU;
    A.rows[RS_OUT_PIT * n + i] = pit;
#pragma unroll
    for (int vv = 0; vv < Q; ++vv) {
      if (v == vv) {
        if (ob) {
          s[vv][RS_SUM_O_LPPD] += lppd;
          s[vv][RS_SUM_O_PWAIC] += pw;
          s[vv][RS_SUM_O_MEANLL] += LM;
          s[vv][RS_SUM_O_LOGN] += logn;
        } else {
          s[vv][RS_SUM_H_LPPD] += lppd;
          s[vv][RS_SUM_H_PIT] += pit;
          s[vv][RS_SUM_H_CRPS] += cr;
          s[vv][RS_SUM_H_SQERR] = fma(e, e, s[vv][RS_SUM_H_SQERR]);
        }
      }
    }
  }
#pragma unroll
  for (int vv = 0; vv < Q; ++vv) {
#pragma unroll
    for (int k = 0; k < RS_NSUM; ++k) {
      const double r = block_sum(s[vv][k], s_red);
      if (threadIdx.x == 0) A.partial[(size_t)blockIdx.x * (Q * RS_NSUM) + vv * RS_NSUM + k] = r;
    }
  }
}

int rows_score_launch(const RowsScoreArgs &A, hipStream_t st) {
  if (A.n <= 0) return 0;
  hipLaunchKernelGGL(k_rows_score_acc, dim3((unsigned)((A.n + NT - 1) / NT)), dim3(NT), 0, st, A);
  return launch_rc();
}

int rows_score_totals_launch(const RowsTotalsArgs &A, int q, double *out, hipStream_t st) {
  typedef void (*Kernel)(RowsTotalsArgs);
  static const Kernel tab[QMAX] = {k_rows_score_totals<1>, k_rows_score_totals<2>, k_rows_score_totals<3>,
                                   k_rows_score_totals<4>, k_rows_score_totals<5>, k_rows_score_totals<6>};
  if (A.n <= 0 || q < 1 || q > QMAX) return 0;
  hipLaunchKernelGGL(tab[q - 1], dim3(STATS_WG), dim3(NT), 0, st, A);
  hipLaunchKernelGGL(k_stats_final, dim3(q * RS_NSUM), dim3(NT), 0, st, A.partial, STATS_WG, q * RS_NSUM, out);
  return launch_rc();
}
