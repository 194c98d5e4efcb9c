// Kernel translation unit of libspamtree_hip.so: the mixture store's step of st_points_accumulate and the two kernels over the
// store, k_mix_quantile and k_mix_crps (points_mixture.hpp has the definitions, the summation orders and the rounding bounds).
// k_mix_store reads d_out, d_pmv, d_X, d_B, d_tsq and the functionals' d_last, draws nothing and writes only the store: no other
// step reads what it writes.
#include "points_mixture.hpp"
#include "series_tile.hpp"
#include "norm_quantile.hpp"

#define MIX_RSQRT2 0.70710678118654752440
#define MIX_SQRT_2_OVER_PI 0.79788456080286535588
#define MIX_W_STOP 4.440892098500626e-16     // 2^-51

static_assert(MIX_NT == NT, "the mixture kernels run the library's workgroup size");

// One thread per point, then one per functional: the point's m, v and, with X, mu = xb + m (k_score_acc's chain: p fma, k = 0..p-1,
// then one add); the first thread also writes tau2_j = 1 / tausq_inv_j, j < q; the functional's F_m, F_v from d_last.
__global__ __launch_bounds__(NT) void k_mix_store(MixStoreArgs A) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long n = A.n;
  if (i < n) {
    const double m = A.mean[i];
    A.m[i] = m;
    A.v[i] = A.var[i];
    if (A.X) {
      const double *bj = A.B + (size_t)A.p * A.pmv[i];
      double xb = 0.0;
      for (int k = 0; k < A.p; ++k) xb = fma(A.X[(size_t)k * n + i], bj[k], xb);
      A.mu[i] = xb + m;
    }
    if (i == 0)
      for (int j = 0; j < A.q; ++j) A.tau2[j] = 1.0 / A.tsq_inv[j];
  } else if (i < n + A.n_fun) {
    const long long f = i - n;
    A.fm[f] = A.last[A.n_fun + f];
    A.fv[f] = A.last[2 * A.n_fun + f];
  }
}

// the xor butterfly the other kernels use: every lane ends with the same bits
__device__ __forceinline__ double mix_wave_sum(double x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}
__device__ __forceinline__ double mix_wave_min(double x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = fmin(x, __shfl_xor(x, o, 64));
  return x;
}
__device__ __forceinline__ double mix_wave_max(double x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = fmax(x, __shfl_xor(x, o, 64));
  return x;
}

// One pass: F(x) and the density sum over the K components of a series (ms, sds: its LDS rows), the same bits in every lane
__device__ __forceinline__ void mix_pass(const double *ms, const double *sds, int K, int lane, double x, double &F, double &D) {
  double s = 0.0, d = 0.0;
  for (int k = lane; k < K; k += 64) {
    const double m = ms[k], sd = sds[k];
    if (sd > 0.0) {
      const double z = (x - m) / sd;
      s += 0.5 * erfc(-z * MIX_RSQRT2);
      d += exp(-0.5 * z * z) / sd;
    } else {
      s += x >= m ? 1.0 : 0.0;
    }
  }
  F = mix_wave_sum(s) / (double)K;
  D = mix_wave_sum(d) * (0.39894228040143267794 / (double)K);
}

// A workgroup stages R series as (m, sd) rows -- row r: m at lds + 2 r K, sd behind it -- through series_tile.hpp's loader (the fill
// is K: no padding column), then wave w serves the series r = w, w + 4, ...: points_mixture.hpp has the iteration.
__global__ __launch_bounds__(NT) void k_mix_quantile(MixQuantileArgs A) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, R = A.R, K = A.K;
  const long long row0 = (long long)blockIdx.x * R, n = A.n;
  const int nr = (int)(n - row0 < R ? n - row0 : R);
  tile_stage(lds, R, 2 * K, K, K, nr, tid, NT, [&](int d, int r) { return A.m[(size_t)d * n + row0 + r]; });
  tile_stage(lds + K, R, 2 * K, K, K, nr, tid, NT, [&](int d, int r) {
    const double v = A.v[(size_t)d * n + row0 + r];
    return sqrt(A.tau2 ? v + A.tau2[(size_t)d * A.q + A.pmv[row0 + r]] : v);
  });
  __syncthreads();
  unsigned long long passes = 0;   // of this wave's series, all probabilities
  for (int r = wid; r < nr; r += NT / 64) {
    const double *ms = lds + (size_t)r * 2 * K, *sds = ms + K;
    double prev = -__builtin_inf();
    bool capped = false;
    for (int t = 0; t < A.T; ++t) {
      const double p = A.p[t], zp = A.z[t];
      double lo = __builtin_inf(), hi = -__builtin_inf();
      for (int k = lane; k < K; k += 64) {
        const double e = ms[k] + zp * sds[k];
        lo = fmin(lo, e); hi = fmax(hi, e);
      }
      lo = mix_wave_min(lo); hi = mix_wave_max(hi);
      const double w = MIX_W_STOP * fmax(fabs(lo), fabs(hi));
      int pass = 0;
      double x = lo + 0.5 * (hi - lo);
      double best = __builtin_inf(), xn = x, step = __builtin_inf();   // the evaluated point closest to p, its Newton point and step
      bool bup = false;
      while (hi - lo > w && x > lo && x < hi) {   // x == an end: no double strictly between them
        if (pass == MIX_Q_MAX_PASSES) { capped = true; break; }
        double F, D;
        mix_pass(ms, sds, K, lane, x, F, D);
        ++pass;
        if (F == p) { hi = x; break; }                          // both conditions of the result hold at x itself
        const bool up = F > p;
        if (up) hi = x; else lo = x;
        const double mid = lo + 0.5 * (hi - lo);
        if (hi - lo <= 256.0 * w) { x = mid; continue; }        // both ends are in: bisect to the width
        double cand;
        if (fabs(F - p) < best) {                               // Newton on the probit scale from the best point so far
          best = fabs(F - p); bup = up;
          const double zF = st_norm_quantile_f(F);
          xn = x - (zF - zp) * (0.39894228040143267794 * exp(-0.5 * zF * zF)) / D;
          step = fabs(xn - x);
          cand = xn;
          if (step <= 64.0 * w) cand = up ? xn - (2.0 * step + 0.4 * w) : xn + (2.0 * step + 0.4 * w);   // at the noise of F: look beyond the root
        } else {                                                // no improvement (a midpoint, a probe): look beyond again, twice as far
          cand = bup ? xn - (2.0 * step + 0.4 * w) : xn + (2.0 * step + 0.4 * w);
          step *= 2.0;
        }
        x = (pass % 3 != 0 && cand > lo && cand < hi) ? cand : mid;   // a NaN or infinite candidate fails the comparisons
      }
      passes += (unsigned)pass;
      const double res = fmax(hi, prev);
      prev = res;
      if (lane == 0) A.out[(size_t)A.slot[t] * n + row0 + r] = res;
    }
    if (capped && lane == 0) atomicAdd(A.counters + MIX_CNT_UNCONVERGED, 1ull);
  }
  if (lane == 0 && passes) atomicAdd(A.counters + MIX_CNT_PASSES, passes);   // one per wave
}

// A(d, s2) of points_mixture.hpp: one sqrt, one division, one erf, one exp
__device__ __forceinline__ double mix_A(double d, double s2) {
  const double s = sqrt(s2);
  const double r = d / s;
  const double a = d * erf(r * MIX_RSQRT2) + s * MIX_SQRT_2_OVER_PI * exp(-0.5 * r * r);
  return s2 > 0.0 ? a : fabs(d);
}

// G threads per scored point, R = NT / G points a workgroup: the point's rows mu and sigma2 at lds + 2 K r, the cross-wave sums behind
// all rows.  points_mixture.hpp has the pair order and the order of every sum.
__global__ __launch_bounds__(NT) void k_mix_crps(MixCrpsArgs A) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x, G = A.G, K = A.K, R = A.R;
  const int r = tid / G, g = tid - r * G, lane = tid & 63;
  const long long slot = (long long)blockIdx.x * R + r;
  const bool live = slot < A.n_scored;          // whole waves: G is a multiple of 64
  const long long i = live ? A.idx[slot] : 0;
  const long long n = A.n;
  double *mus = lds + (size_t)r * 2 * K, *s2s = mus + K;
  double *red = lds + (size_t)R * 2 * K;        // [NT / 64][3]
  if (live) {
    const int j = A.pmv[i];
    for (int s = g; s < K; s += G) {
      mus[s] = A.mu[(size_t)s * n + i];
      s2s[s] = A.v[(size_t)s * n + i] + A.tau2[(size_t)s * A.q + j];
    }
  }
  __syncthreads();
  double t1 = 0.0, dg = 0.0, a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  if (live) {
    const double y = A.y[i];
    const int J = (K - 1) >> 1, J4 = J & ~3;
    const bool even = (K & 1) == 0;
    for (int s = g; s < K; s += G) {
      const double mu = mus[s], s2 = s2s[s];
      t1 += mix_A(y - mu, s2);
      dg += sqrt(s2 + s2) * MIX_SQRT_2_OVER_PI;
      int t = s + 1;                            // the partner of j = 1; kept in [0, K)
      if (t >= K) t -= K;
      int j = 1;
      for (; j <= J4; j += 4) {
        int tb = t + 1; if (tb >= K) tb -= K;
        int tc = tb + 1; if (tc >= K) tc -= K;
        int td = tc + 1; if (td >= K) td -= K;
        a0 += mix_A(mu - mus[t], s2 + s2s[t]);
        a1 += mix_A(mu - mus[tb], s2 + s2s[tb]);
        a2 += mix_A(mu - mus[tc], s2 + s2s[tc]);
        a3 += mix_A(mu - mus[td], s2 + s2s[td]);
        t = td + 1; if (t >= K) t -= K;
      }
      if (j <= J) { a0 += mix_A(mu - mus[t], s2 + s2s[t]); ++j; ++t; if (t >= K) t -= K; }
      if (j <= J) { a1 += mix_A(mu - mus[t], s2 + s2s[t]); ++j; ++t; if (t >= K) t -= K; }
      if (j <= J) { a2 += mix_A(mu - mus[t], s2 + s2s[t]); ++j; ++t; if (t >= K) t -= K; }
      if (even && s < (K >> 1)) a0 += mix_A(mu - mus[s + (K >> 1)], s2 + s2s[s + (K >> 1)]);
    }
  }
  const double pr = mix_wave_sum((a0 + a1) + (a2 + a3));
  t1 = mix_wave_sum(t1);
  dg = mix_wave_sum(dg);
  const int wid = tid >> 6;
  if (lane == 0) { red[3 * wid] = t1; red[3 * wid + 1] = dg; red[3 * wid + 2] = pr; }
  __syncthreads();
  if (live && g == 0) {
    const int w0 = tid >> 6, nw = G >> 6;
    double T1 = 0.0, D = 0.0, P = 0.0;
    for (int w = w0; w < w0 + nw; ++w) { T1 += red[3 * w]; D += red[3 * w + 1]; P += red[3 * w + 2]; }
    const double Kd = (double)K;
    const double spread = (D + 2.0 * P) / (2.0 * Kd * Kd);
    A.spread[i] = spread;
    A.crps[i] = T1 / Kd - spread;
  }
}

int points_mix_store_launch(const MixStoreArgs &A, hipStream_t st) {
  const long long tot = A.n + A.n_fun;
  if (tot <= 0) return 0;
  hipLaunchKernelGGL(k_mix_store, dim3((unsigned)((tot + NT - 1) / NT)), dim3(NT), 0, st, A);
  return launch_rc();
}

int points_mix_quantile_launch(const MixQuantileArgs &A, const MixPlan &P, size_t lds_limit, hipStream_t st) {
  if (A.n <= 0 || A.T <= 0) return 0;
  (void)hipFuncSetAttribute((const void *)k_mix_quantile, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_limit);
  hipLaunchKernelGGL(k_mix_quantile, dim3((unsigned)P.grid), dim3(NT), P.lds, st, A);
  return launch_rc();
}

int points_mix_crps_launch(const MixCrpsArgs &A, const MixPlan &P, size_t lds_limit, hipStream_t st) {
  if (A.n_scored <= 0) return 0;
  (void)hipFuncSetAttribute((const void *)k_mix_crps, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_limit);
  hipLaunchKernelGGL(k_mix_crps, dim3((unsigned)P.grid), dim3(NT), P.lds, st, A);
  return launch_rc();
}
