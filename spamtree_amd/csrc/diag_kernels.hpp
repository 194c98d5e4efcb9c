// Convergence diagnostics of the stored draws (st_summary_diagnostics, st_points_summary_diagnostics,
// st_points_functionals_diagnostics; the kernel and its launcher live in k_diag.hip): per series of K stored draws the effective
// sample size, the Monte-Carlo standard error of the mean, the posterior sd of the draws and the split-R-hat of the one chain.
// include/spamtree_hip.h has the definition; this header restates it in the order the kernel evaluates it.
//
// A store is draws[d * n + i], d < K <= 16384, i < n.  A workgroup stages the K draws of R consecutive series into LDS, transposed
// (series r at lds + r Kp; Kp = K | 1 when R > 1, so that the R values of one draw land on different banks), and wave w takes the
// series w, w + nw, ... of the tile, one at a time.  Every sum below is taken the same way: lane l adds the terms s = l, l + 64,
// l + 128, ... in ascending order into one accumulator (products by fma), then the 64 accumulators are added by the xor butterfly
// with partners 8, 4, 2, 1 (DPP moves inside a row of 16 lanes), then 16 and 32 -- the order depends on K and the term's index only, not on n, R, the series' place in the
// store or the workgroup, so the outputs of a series are bitwise a function of its K values and max_lag.  In order:
//   P1  a = sum x_s;  m0 = a / K
//   P2  c = sum (x_s - m0);  m = m0 + c / K               (the mean to the rounding of the data's spread, not of its offset:
//                                                           a constant series gets m = x_0 and d = 0 exactly)
//   P3  d_s = x_s - m, in place;  g0 = sum d_s^2;  b1 = sum_{s < h} d_s;  b2 = sum_{s >= K - h} d_s;  h = K / 2
//       mu1 = b1 / h, mu2 = b2 / h                         (the half means less m)
//   P4  v1 = sum_{s < h} (d_s - mu1)^2;  v2 = sum_{s >= K - h} (d_s - mu2)^2
//       sd = sqrt(g0 / (K - 1));  W = (v1 / (h - 1) + v2 / (h - 1)) / 2;  mb = (mu1 + mu2) / 2;
//       B = h ((mu1 - mb)^2 + (mu2 - mb)^2);  rhat = sqrt(((h - 1) / h W + B / h) / W)
//   lags, DIAG_NL = 4 at a time (two pairs per pass over d):  a_t = sum_{s < K - t} d_s d_{s + t},  rho_t = a_t / g0
//       (a_0 is g0's own chain: rho_0 = 1 exactly);  pair k: G = rho_2k + rho_2k+1;  stop at !(G > 0);  G = min(G, G_prev);
//       tsum += G, in pair order.  A pass is made only while no pair has stopped.
//   tau = max(-1 + 2 tsum, 1 / log10 K);  ess = K / tau;  mcse = sd / sqrt(ess);  lags = 2 pairs.
// g0 == 0: ess = NaN, mcse = 0, sd = 0, rhat = NaN, lags = 0.  W == 0: rhat = NaN.
// LDS: unit stride across lanes in every pass (d[s] and d[s + t] alike): no bank conflict.  No atomics, no scratch.
// Several chains in one store (st_*_chain_diagnostics, k_series_diag<true>): diag_chain_wave below, with its own order of operations.
#pragma once
#include "st_device.hpp"

#define DIAG_NL 4              // lags per pass over the centred series
#define DIAG_MAX_R 8           // series per workgroup at most
#define DIAG_NT 512            // one wave per series of the tile: 64 min(R, 8) threads
#define DIAG_TILE (64 * 1024)  // the tile a workgroup aims for (two workgroups per CU); a longer series takes what the device allows

struct DiagArgs {
  const double *draws;   // [K][n]
  long long n;
  int K, Kp, R;
  int M;                 // chains the K draws are cut into (1: the single-chain definition and kernel)
  int L;                 // min(max_lag, K / M - 2), max_lag = 0 resolved
  double *ess, *mcse, *sd, *rhat;   // n each (device), store order
  int *lags;
};

#ifdef __HIPCC__
// the sum of v over the wave, in every lane: the xor butterfly with partners 8, 4, 2, 1 inside each row of 16 lanes by DPP moves
// (st_device.hpp: group_xor_sum), then partners 16 and 32 across the rows.  a + b == b + a bit for bit, so all lanes agree.
__device__ __forceinline__ double diag_allsum(double v) {
  v = group_xor_sum<16>(v);
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

// The diagnostics of one series by one wave: x[0 .. K) (LDS, or global memory that only this wave touches) is centred in place.
// P1 .. P4 and, with LAGS, the lag pairs, in the order of the header; every lane returns the same values.  Without LAGS only sd
// and rhat are formed (ess = NaN, mcse = 0, pairs = 0).  k_series_diag and the rank-normalised kernel (k_rank.hip) share this text.
struct DiagOut { double ess, mcse, sd, rhat; int pairs; };
template <bool LAGS>
__device__ __forceinline__ DiagOut diag_series_wave(double *x, int K, int L, int lane) {
  const int h = K / 2;
  const double dK = (double)K, dh = (double)h;
  // P1, P2: the mean
  double a = 0.0;
  for (int s = lane; s < K; s += 64) a += x[s];
  const double m0 = diag_allsum(a) / dK;
  double c = 0.0;
  for (int s = lane; s < K; s += 64) c += x[s] - m0;
  const double m = m0 + diag_allsum(c) / dK;
  // P3: centre in place; g0 and the half sums
  double g0 = 0.0, b1 = 0.0, b2 = 0.0;
  for (int s = lane; s < K; s += 64) {
    const double d = x[s] - m;
    x[s] = d;
    g0 = fma(d, d, g0);
    if (s < h) b1 += d;
    if (s >= K - h) b2 += d;
  }
  g0 = diag_allsum(g0);
  const double mu1 = diag_allsum(b1) / dh, mu2 = diag_allsum(b2) / dh;
  wave_lds_sync();
  // P4: the half variances
  double v1 = 0.0, v2 = 0.0;
  for (int s = lane; s < K; s += 64) {
    const double d = x[s];
    if (s < h) { const double e = d - mu1; v1 = fma(e, e, v1); }
    if (s >= K - h) { const double e = d - mu2; v2 = fma(e, e, v2); }
  }
  v1 = diag_allsum(v1);
  v2 = diag_allsum(v2);
  const double nan = __builtin_nan("");
  double ess = nan, mcse = 0.0, sd = 0.0, rhat = nan;
  int pairs = 0;
  if (g0 != 0.0) {   // (a NaN series goes through the formulas)
    sd = sqrt(g0 / (dK - 1.0));
    const double W = (v1 / (dh - 1.0) + v2 / (dh - 1.0)) / 2.0;
    const double mb = (mu1 + mu2) / 2.0;
    const double e1 = mu1 - mb, e2 = mu2 - mb;
    const double B = dh * fma(e1, e1, e2 * e2);
    if (W != 0.0) rhat = sqrt(((dh - 1.0) / dh * W + B / dh) / W);
    // the lag pairs
    const int kmax = (L - 1) / 2;
    double tsum = 0.0, prev = __builtin_inf();
    bool stop = !LAGS;
    for (int k0 = 0; k0 <= kmax && !stop; k0 += DIAG_NL / 2) {
      const int t0 = 2 * k0, len = K - t0;   // len >= 2: t0 <= L - 1 <= K - 3
      double acc[DIAG_NL];
#pragma unroll
      for (int j = 0; j < DIAG_NL; ++j) acc[j] = 0.0;
      for (int s = lane; s < len; s += 64) {
        const double ds = x[s];
        const double *y = x + s + t0;
#pragma unroll
        for (int j = 0; j < DIAG_NL; ++j)
          if (s + j < len) acc[j] = fma(ds, y[j], acc[j]);   // s + t0 + j < K
      }
#pragma unroll
      for (int j = 0; j < DIAG_NL; ++j) acc[j] = diag_allsum(acc[j]);
#pragma unroll
      for (int j = 0; j < DIAG_NL / 2; ++j) {
        if (!stop && k0 + j <= kmax) {
          double G = acc[2 * j] / g0 + acc[2 * j + 1] / g0;
          if (!(G > 0.0)) stop = true;
          else {
            G = fmin(G, prev);
            prev = G;
            tsum += G;
            ++pairs;
          }
        }
      }
    }
    if (LAGS) {
      const double tau = fmax(2.0 * tsum - 1.0, 1.0 / log10(dK));
      ess = dK / tau;
      mcse = sd / sqrt(ess);
    }
  }
  DiagOut o;
  o.ess = ess; o.mcse = mcse; o.sd = sd; o.rhat = rhat; o.pairs = pairs;
  return o;
}

// The multi-chain diagnostics of one series by one wave (st_*_chain_diagnostics, M >= 2 chains; M = 1 runs diag_series_wave):
// x[0 .. K), K = M N, is chain c at x[c N .. (c + 1) N), centred in place about its chain's mean.  Sums are taken as above (lane l
// adds its terms in ascending order, then diag_allsum); "over a chain" means lane l takes s = l, l + 64, ... of that chain, and
// "over the chains" means chain 0's terms of the lane, then chain 1's, ... into the one accumulator before the one butterfly.
// A value per chain or per segment lives in one lane (chain c in lane c, its halves in lanes 2c and 2c + 1; the other lanes hold
// 0) and is summed by diag_allsum: M <= ST_DIAG_MAX_CHAINS = 16 keeps the 2M segments inside the wave.  In order:
//   Q1  a = sum x_s over all K;  m0 = a / K;  c = sum (x_s - m0);  m = m0 + c / K                  (P1, P2: the pooled mean)
//   Q2  y_s = x_s - m, in place;  g0 = sum y_s^2 over all K;  sd = sqrt(g0 / (K - 1))              (P3's chain: the sd of the
//       single-chain call on the same store, bit for bit)
//   per chain c = 0 .. M - 1, on y, h = N / 2:
//   C1  a = sum y over the chain;  n0 = a / N;  e = sum (y - n0);  nu_c = n0 + e / N               (the chain's mean less m)
//   C2  d_s = y_s - nu_c, in place;  b1 = sum_{s < h} d_s;  b2 = sum_{s >= N - h} d_s;  mu1 = b1 / h, mu2 = b2 / h;
//       the lane's share of a_0 = sum d_s^2 over the chains grows here, chain after chain (no pass of its own)
//   C3  v1 = sum_{s < h} (d_s - mu1)^2;  v2 = sum_{s >= N - h} (d_s - mu2)^2
//       lane c keeps nu_c;  lane 2c keeps (nu_c + mu1, v1), lane 2c + 1 keeps (nu_c + mu2, v2)    (segment means less m)
//   R   S = 2M;  W = (sum of the lanes' v) / (h - 1) / S;  mb = (sum of the lanes' segment means) / S;
//       B = h / (S - 1) sum (m_j - mb)^2;  rhat = sqrt(((h - 1) / h W + B / h) / W)
//   E   nb = (sum nu_c) / M;  Q = K sum (nu_c - nb)^2 / (M - 1)                                    (= K B')
//       a_0 = sum d_s^2 over the chains;  den = Q + a_0                                             (= K (B' + gbar_0))
//   lags, DIAG_NL = 4 at a time:  a_t = sum_{s < N - t} d_{c,s} d_{c,s+t} over the chains (no product crosses a chain boundary: the
//       inner loop ends at N - t in every chain);  rho_t = (Q + a_t) / den  (a_0 is den's own chain: rho_0 = 1 exactly);
//       the pairs, the stop rule, the monotone rule, tau, its floor, ess, mcse and lags as above, with K = M N in the floor and ess.
// den == 0: ess = NaN, mcse = 0, sd = 0, rhat = NaN, lags = 0.  W == 0: rhat = NaN.  Without LAGS, E and the lags are left out.
// The multiply-adds of a lag pass are the single-chain pass's less the pairs that straddle a boundary; what M adds is C1 .. C3's
// seven butterflies per chain and R's and E's six.
template <bool LAGS>
__device__ __forceinline__ DiagOut diag_chain_wave(double *x, int K, int M, int L, int lane) {
  const int N = K / M, h = N / 2;
  const double dK = (double)K, dN = (double)N, dh = (double)h;
  // Q1, Q2: the pooled mean and sd
  double a = 0.0;
  for (int s = lane; s < K; s += 64) a += x[s];
  const double m0 = diag_allsum(a) / dK;
  double c = 0.0;
  for (int s = lane; s < K; s += 64) c += x[s] - m0;
  const double m = m0 + diag_allsum(c) / dK;
  double g0 = 0.0;
  for (int s = lane; s < K; s += 64) {
    const double y = x[s] - m;
    x[s] = y;
    g0 = fma(y, y, g0);
  }
  g0 = diag_allsum(g0);
  wave_lds_sync();
  // C1 .. C3 per chain; the lanes' keepsakes
  double nuL = 0.0, mL = 0.0, vL = 0.0;
  double a0 = 0.0;   // a_0's lane sums, over the chains: formed in C2, as the d_s are (the lag pass's own order at t = 0)
  for (int ch = 0; ch < M; ++ch) {
    double *xc = x + (size_t)ch * N;
    double s1 = 0.0;
    for (int s = lane; s < N; s += 64) s1 += xc[s];
    const double n0 = diag_allsum(s1) / dN;
    double s2 = 0.0;
    for (int s = lane; s < N; s += 64) s2 += xc[s] - n0;
    const double nu = n0 + diag_allsum(s2) / dN;
    double b1 = 0.0, b2 = 0.0;
    for (int s = lane; s < N; s += 64) {
      const double d = xc[s] - nu;
      xc[s] = d;
      if (LAGS) a0 = fma(d, d, a0);
      if (s < h) b1 += d;
      if (s >= N - h) b2 += d;
    }
    const double mu1 = diag_allsum(b1) / dh, mu2 = diag_allsum(b2) / dh;
    wave_lds_sync();
    double v1 = 0.0, v2 = 0.0;
    for (int s = lane; s < N; s += 64) {
      const double d = xc[s];
      if (s < h) { const double e = d - mu1; v1 = fma(e, e, v1); }
      if (s >= N - h) { const double e = d - mu2; v2 = fma(e, e, v2); }
    }
    v1 = diag_allsum(v1);
    v2 = diag_allsum(v2);
    if (lane == ch) nuL = nu;
    if (lane == 2 * ch) { mL = nu + mu1; vL = v1; }
    if (lane == 2 * ch + 1) { mL = nu + mu2; vL = v2; }
  }
  // R: the 2M segments
  const double dS = (double)(2 * M), dM = (double)M;
  const double W = diag_allsum(vL) / (dh - 1.0) / dS;
  const double mb = diag_allsum(mL) / dS;
  const double eb = lane < 2 * M ? mL - mb : 0.0;
  const double B = dh / (dS - 1.0) * diag_allsum(eb * eb);
  // E: between and within
  double Q = 0.0, den = g0;   // (without LAGS only den's zero matters, and g0 == 0 is den == 0: all K values equal)
  if (LAGS) {
    const double nb = diag_allsum(nuL) / dM;
    const double en = lane < M ? nuL - nb : 0.0;
    Q = dK * diag_allsum(en * en) / (dM - 1.0);
    den = Q + diag_allsum(a0);
  }
  const double nan = __builtin_nan("");
  double ess = nan, mcse = 0.0, sd = 0.0, rhat = nan;
  int pairs = 0;
  if (den != 0.0) {   // (a NaN series goes through the formulas)
    sd = sqrt(g0 / (dK - 1.0));
    if (W != 0.0) rhat = sqrt(((dh - 1.0) / dh * W + B / dh) / W);
    const int kmax = (L - 1) / 2;
    double tsum = 0.0, prev = __builtin_inf();
    bool stop = !LAGS;
    for (int k0 = 0; k0 <= kmax && !stop; k0 += DIAG_NL / 2) {
      const int t0 = 2 * k0, len = N - t0;   // len >= 2: t0 <= L - 1 <= N - 3
      double acc[DIAG_NL];
#pragma unroll
      for (int j = 0; j < DIAG_NL; ++j) acc[j] = 0.0;
      for (int ch = 0; ch < M; ++ch) {
        const double *xc = x + (size_t)ch * N;
        for (int s = lane; s < len; s += 64) {
          const double ds = xc[s];
          const double *y = xc + s + t0;
#pragma unroll
          for (int j = 0; j < DIAG_NL; ++j)
            if (s + j < len) acc[j] = fma(ds, y[j], acc[j]);   // s + t0 + j < N: inside the chain
        }
      }
#pragma unroll
      for (int j = 0; j < DIAG_NL; ++j) acc[j] = diag_allsum(acc[j]);
#pragma unroll
      for (int j = 0; j < DIAG_NL / 2; ++j) {
        if (!stop && k0 + j <= kmax) {
          double G = (Q + acc[2 * j]) / den + (Q + acc[2 * j + 1]) / den;
          if (!(G > 0.0)) stop = true;
          else {
            G = fmin(G, prev);
            prev = G;
            tsum += G;
            ++pairs;
          }
        }
      }
    }
    if (LAGS) {
      const double tau = fmax(2.0 * tsum - 1.0, 1.0 / log10(dK));
      ess = dK / tau;
      mcse = sd / sqrt(ess);
    }
  }
  DiagOut o;
  o.ess = ess; o.mcse = mcse; o.sd = sd; o.rhat = rhat; o.pairs = pairs;
  return o;
}
#endif

// R and Kp of a store of K draws under a per-workgroup LDS limit; false: one series does not fit
bool series_diag_plan(long long K, size_t lds_limit, int *R, int *Kp);
int series_diag_launch(const DiagArgs &A, size_t lds_limit, hipStream_t st);
