// Kernel translation unit of libspamtree_hip.so: Pareto-smoothed importance sampling of stored log ratios (psis_kernels.hpp has the
// evaluation order, spamtree_amd/psis.py the definition).  k_loo_psis reads a store and writes only its own outputs; k_psis_finish
// reduces them per outcome.  Neither draws anything nor touches any state of the chain.
#include "psis_kernels.hpp"
#include "series_tile.hpp"       // stage, sort and the searches of a sorted row: no floating-point arithmetic in them
#pragma clang fp contract(off)

__device__ __forceinline__ bool psis_finite(double v) { return v >= -__DBL_MAX__ && v <= __DBL_MAX__; }

// the smallest integer m with m m >= v (v < 2^31)
__device__ __forceinline__ int psis_ceil_sqrt(int v) {
  int m = (int)sqrt((double)v);
  while (m * m < v) ++m;
  while (m > 0 && (m - 1) * (m - 1) >= v) --m;
  return m;
}

// step 3 of psis_kernels.hpp for series i by one wave (all 64 lanes): a = its sorted row, X = its PSIS_MAX_TAIL tail values
__device__ __forceinline__ void psis_series_wave(const PsisArgs &A, long long i, const double *a, double *X, int lane) {
  const long long n = A.n;
  const int K = A.K;
  const double inf = __builtin_inf(), nan = __builtin_nan("");
  const int S = sorted_count_below(a, K, inf);
  if (S == 0) {
    if (lane == 0) {
      for (int k = 0; k < PSIS_NOUT; ++k) A.out[(size_t)k * n + i] = nan;
      A.tail_len[i] = 0; A.n_draws[i] = 0;
    }
    return;
  }
  const double c = a[S - 1];
  const int M = min(S / 5, psis_ceil_sqrt(9 * S));
  bool smooth = M >= 5;
  double khat = inf, tmin = inf, ecut = 0.0;
  if (smooth) {   // wave-uniform: S and M are
    tmin = a[S - M];
    ecut = exp(a[S - M - 1] - c);
    smooth = c != tmin;
  }
  if (smooth) {
    for (int j = lane; j < M; j += 64) X[j] = exp(a[S - M + j] - c) - ecut;
    wave_lds_sync();
    const double xs = X[(M + 2) / 4 - 1], xN = X[M - 1];
    smooth = xs != 0.0;
    if (smooth) {
      const double dM = (double)M;
      int G = 30 + psis_ceil_sqrt(M);
      if ((G - 30) * (G - 30) > M) --G;   // isqrt
      const double theta = 1.0 / xN + (1.0 - sqrt((double)G / ((double)lane + 0.5))) / (3.0 * xs);
      double kj = 0.0;
      for (int m = 0; m < M; ++m) kj += log1p(-theta * X[m]);
      kj = kj / dM;
      const double lj = dM * (log(-theta / kj) - kj - 1.0);
      double den = 0.0;
      for (int g = 0; g < G; ++g) den += exp(__shfl(lj, g, 64) - lj);
      const double tw = theta * (1.0 / den);
      double th = 0.0;
      for (int g = 0; g < G; ++g) th += __shfl(tw, g, 64);
      double ks = 0.0;
      for (int m = lane; m < M; m += 64) ks += log1p(-th * X[m]);
      const double k = wave_allsum(ks) / dM;
      const double sigma = -k / th;
      khat = (k * dM + 5.0) / (dM + 10.0);
      smooth = psis_finite(khat) && psis_finite(sigma);
      wave_lds_sync();   // every lane has read x before the smoothed values replace it
      if (smooth) {
        for (int j = lane; j < M; j += 64) {
          const double l1p = log1p(-((double)j + 0.5) / dM);
          const double q = khat == 0.0 ? -sigma * l1p : sigma * expm1(-khat * l1p) / khat;
          X[j] = fmin(log(q + ecut), 0.0);
        }
        wave_lds_sync();
      } else khat = inf;
    }
  }
  // the estimates, over the draws in ascending index
  double W1 = 0.0, W2 = 0.0, U = 0.0, P = 0.0, Q = 0.0;
  for (int base = 0; base < K; base += 64) {
    const int s = base + lane;
    double tv = nan;
    if (s < K) tv = A.t[(size_t)s * n + i];
    const bool fin = psis_finite(tv);
    const bool cand = smooth && fin && tv >= tmin;
    int lo = 0;
    bool tied = false;
    if (cand) {
      lo = sorted_count_below(a, S, tv);
      tied = sorted_count_upto(a, S, tv, lo) - lo > 1;
    }
    int e = 0;
    unsigned long long tm = __ballot(tied);
    while (tm) {   // wave-uniform: one tied draw after another, its earlier equals counted by the whole wave
      const int L = __ffsll((long long)tm) - 1;
      tm &= tm - 1;
      const double v = __shfl(tv, L, 64);
      const int sL = base + L;
      int cnt = 0;
      for (int b2 = 0; b2 < sL; b2 += 64) {
        const int s2 = b2 + lane;
        const bool p = s2 < sL && A.t[(size_t)s2 * n + i] == v;
        cnt += __popcll(__ballot(p));
      }
      if (lane == L) e = cnt;
    }
    if (fin) {
      const double lw = tv - c;
      double lwp = lw;
      if (cand) {
        const int pos = lo + e;   // <= S - 1
        if (pos >= S - M) lwp = X[pos - (S - M)];
      }
      const double ew = exp(lwp);
      W1 += ew;
      W2 += exp(2.0 * lwp);
      U += exp(lwp - lw);
      if (A.phi) { const double pr = ew * A.phi[(size_t)s * n + i]; P += pr; }
      if (A.mu) { const double pr = ew * A.mu[(size_t)s * n + i]; Q += pr; }
    }
  }
  W1 = wave_allsum(W1); W2 = wave_allsum(W2); U = wave_allsum(U); P = wave_allsum(P); Q = wave_allsum(Q);
  if (lane == 0) {
    A.out[(size_t)PSIS_OUT_KHAT * n + i] = khat;
    A.out[(size_t)PSIS_OUT_ELPD * n + i] = (-c + log(U)) - log(W1);
    A.out[(size_t)PSIS_OUT_PIT * n + i] = A.phi ? P / W1 : nan;
    A.out[(size_t)PSIS_OUT_MU * n + i] = A.mu ? Q / W1 : nan;
    A.out[(size_t)PSIS_OUT_ESS * n + i] = W1 * W1 / W2;
    A.tail_len[i] = smooth ? M : 0;
    A.n_draws[i] = S;
  }
}

__global__ __launch_bounds__(PSIS_NT) void k_loo_psis(PsisArgs A) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int K = A.K, Kpad = A.Kpad, R = A.R;
  double *Srt = lds, *Xt = lds + (size_t)R * Kpad;
  const double inf = __builtin_inf();
  const long long ntiles = (A.n + R - 1) / R;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long row0 = tile * R;
    const int nr = (int)(A.n - row0 < R ? A.n - row0 : R);
    // 1: stage
    tile_stage(Srt, R, Kpad, Kpad, K, nr, tid, PSIS_NT, [&](int d, int r) {
      const double v = A.t[(size_t)d * A.n + row0 + r];
      return psis_finite(v) ? v : inf;
    });
    __syncthreads();
    // 2: sort
    tile_sort_rows(Srt, R, Kpad, tid, PSIS_NT);
    // 3: one wave per series
    for (int r = wid; r < nr; r += PSIS_NT / 64) psis_series_wave(A, row0 + r, Srt + (size_t)r * Kpad, Xt + (size_t)r * PSIS_MAX_TAIL, lane);
    __syncthreads();   // the next tile restages the rows
  }
}

// The per-outcome totals: workgroup v takes outcome v.  Thread t walks the rows t, t + NT, ... ascending, then the NT partial values
// meet in a fixed binary tree in LDS (sums; the minimum for weight_ess_psis, the maximum for khat).
__global__ __launch_bounds__(NT) void k_psis_finish(PsisFinishArgs A) {
  __shared__ double sm[PSIS_NSUM][NT];
  const int v = blockIdx.x, tid = threadIdx.x;
  const long long n = A.n;
  double s[PSIS_NSUM];
  for (int k = 0; k < PSIS_NSUM; ++k) s[k] = 0.0;
  s[ST_ROWS_PSIS_MIN_ESS] = __builtin_inf();
  s[ST_ROWS_PSIS_MAX_KHAT] = -__builtin_inf();
  for (long long i = tid; i < n; i += NT) {
    if (A.mv[i] != v || !A.obs[i] || A.n_draws[i] <= 0) continue;
    const double khat = A.rows[(size_t)PSIS_OUT_KHAT * n + i], elpd = A.rows[(size_t)PSIS_OUT_ELPD * n + i];
    const double r = A.y[i] - A.rows[(size_t)PSIS_OUT_MU * n + i];
    s[ST_ROWS_PSIS_COUNT] += 1.0;
    s[ST_ROWS_PSIS_ELPD] += elpd;
    s[ST_ROWS_PSIS_ELPD_SQ] = fma(elpd, elpd, s[ST_ROWS_PSIS_ELPD_SQ]);
    s[ST_ROWS_PSIS_SQERR] = fma(r, r, s[ST_ROWS_PSIS_SQERR]);
    s[ST_ROWS_PSIS_PIT] += A.rows[(size_t)PSIS_OUT_PIT * n + i];
    s[ST_ROWS_PSIS_MIN_ESS] = fmin(s[ST_ROWS_PSIS_MIN_ESS], A.rows[(size_t)PSIS_OUT_ESS * n + i]);
    s[ST_ROWS_PSIS_MAX_KHAT] = fmax(s[ST_ROWS_PSIS_MAX_KHAT], khat);
    if (khat > 0.7) s[ST_ROWS_PSIS_N_BAD] += 1.0;
    if (khat > A.thr) s[ST_ROWS_PSIS_N_ABOVE] += 1.0;
  }
  for (int k = 0; k < PSIS_NSUM; ++k) sm[k][tid] = s[k];
  __syncthreads();
  for (int o = NT / 2; o > 0; o >>= 1) {
    if (tid < o) {
      for (int k = 0; k < PSIS_NSUM; ++k) {
        const double x = sm[k][tid], y = sm[k][tid + o];
        sm[k][tid] = k == ST_ROWS_PSIS_MIN_ESS ? fmin(x, y) : k == ST_ROWS_PSIS_MAX_KHAT ? fmax(x, y) : x + y;
      }
    }
    __syncthreads();
  }
  if (tid < PSIS_NSUM) A.tot[v * PSIS_NSUM + tid] = sm[tid][0];
}

int psis_launch(const PsisArgs &A, hipStream_t st) {
  if (A.n <= 0) return 0;
  const size_t lds = psis_lds_bytes(A.R, A.Kpad);
  const hipError_t ea = hipFuncSetAttribute((const void *)k_loo_psis, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (ea != hipSuccess) return (int)ea;
  hipLaunchKernelGGL(k_loo_psis, dim3((unsigned)psis_grid(A.n, A.R)), dim3(PSIS_NT), lds, st, A);
  return launch_rc();
}

int psis_finish_launch(const PsisFinishArgs &A, hipStream_t st) {
  if (A.n <= 0 || A.q < 1) return 0;
  hipLaunchKernelGGL(k_psis_finish, dim3(A.q), dim3(NT), 0, st, A);
  return launch_rc();
}
