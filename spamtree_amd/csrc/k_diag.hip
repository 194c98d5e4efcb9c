// Kernel translation unit of libspamtree_hip.so: the convergence diagnostics of the stored draws (diag_kernels.hpp has the
// evaluation order, include/spamtree_hip.h the definition).  k_series_diag reads a store of saved draws and writes only its own
// outputs; it draws nothing and touches no state of the chain.
#include "st_handle.hpp"
#include "diag_kernels.hpp"

// the sum of v over the wave, in every lane: the xor butterfly with partners 8, 4, 2, 1 inside each row of 16 lanes by DPP moves
// (st_device.hpp: group_xor_sum), then partners 16 and 32 across the rows.  a + b == b + a bit for bit, so all lanes agree.
__device__ __forceinline__ double diag_allsum(double v) {
  v = group_xor_sum<16>(v);
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

// LDS written by one lane of the wave and read by another: order the wave's own LDS traffic (no workgroup barrier: a series belongs
// to one wave)
__device__ __forceinline__ void diag_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(DIAG_NT) void k_series_diag(DiagArgs A) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, nw = blockDim.x >> 6;
  const int K = A.K, Kp = A.Kp, R = A.R;
  const long long row0 = (long long)blockIdx.x * R;
  for (int idx = tid; idx < R * K; idx += blockDim.x) {
    const int d = idx / R, r = idx - d * R;   // R consecutive series of one draw: contiguous in memory
    if (row0 + r < A.n) lds[(size_t)r * Kp + d] = A.draws[(size_t)d * A.n + row0 + r];
  }
  __syncthreads();
  const int h = K / 2;
  const double dK = (double)K, dh = (double)h;
  for (int r = wid; r < R && row0 + r < A.n; r += nw) {
    double *x = lds + (size_t)r * Kp;
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
    diag_wave_sync();
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
      const int kmax = (A.L - 1) / 2;
      double tsum = 0.0, prev = __builtin_inf();
      bool stop = false;
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
      const double tau = fmax(2.0 * tsum - 1.0, 1.0 / log10(dK));
      ess = dK / tau;
      mcse = sd / sqrt(ess);
    }
    if (lane == 0) {
      const long long i = row0 + r;
      if (A.ess) A.ess[i] = ess;
      if (A.mcse) A.mcse[i] = mcse;
      if (A.sd) A.sd[i] = sd;
      if (A.rhat) A.rhat[i] = rhat;
      if (A.lags) A.lags[i] = 2 * pairs;
    }
  }
}

bool series_diag_plan(long long K, size_t lds_limit, int *R, int *Kp) {
  const size_t kp = (size_t)(K | 1);
  size_t r = std::min<size_t>(lds_limit, DIAG_TILE) / (kp * sizeof(double));
  if (r < 2) r = lds_limit / (kp * sizeof(double));   // a long series: what the device allows
  if (r >= 2) { *R = (int)std::min<size_t>(r, DIAG_MAX_R); *Kp = (int)kp; return true; }
  if ((size_t)K * sizeof(double) > lds_limit) return false;
  *R = 1; *Kp = (int)K;
  return true;
}

int series_diag_launch(const DiagArgs &A, size_t lds_limit, hipStream_t st) {
  if (A.n <= 0) return 0;
  const size_t lds = (size_t)A.R * A.Kp * sizeof(double);
  (void)hipFuncSetAttribute((const void *)k_series_diag, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_limit);
  hipLaunchKernelGGL(k_series_diag, dim3((unsigned)((A.n + A.R - 1) / A.R)), dim3(64 * std::min(A.R, DIAG_NT / 64)), lds, st, A);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

int series_diag_store(st_handle_s *h, const char *who, const double *draws, long long n, long long K, int32_t max_lag,
                      const long long *perm, const st_series_diag *out) {
  if (!out || n <= 0 || !(out->ess || out->mcse || out->sd || out->rhat || out->lags)) return ST_OK;
  DiagArgs A;
  A.draws = draws; A.n = n; A.K = (int)K;
  A.L = (int)std::min<long long>(max_lag == 0 ? ST_DIAG_DEFAULT_MAX_LAG : max_lag, K - 2);
  if (!series_diag_plan(K, h->lds_limit, &A.R, &A.Kp)) {
    h->err = std::string(who) + ": " + std::to_string(K) + " stored draws of one series do not fit one workgroup's LDS";
    return ST_ERR_UNSUPPORTED;
  }
  HCHK(h, hipSetDevice(h->device));
  DevBuf<double> d_out;
  DevBuf<int> d_lags;
  HCHK(h, d_out.alloc((size_t)4 * n));
  HCHK(h, d_lags.alloc((size_t)n));
  A.ess = d_out.p; A.mcse = d_out.p + n; A.sd = d_out.p + 2 * n; A.rhat = d_out.p + 3 * n; A.lags = d_lags.p;
  {
    ProfScope pscope(h, 3);
    const int e = series_diag_launch(A, h->lds_limit, h->stream);
    if (e) { h->err = std::string(who) + " launch: " + hipGetErrorString((hipError_t)e); return ST_ERR_HIP; }
  }
  // only what the caller asked for comes to the host
  double *const dst[4] = {out->ess, out->mcse, out->sd, out->rhat};
  std::vector<double> tmp((size_t)4 * n);
  std::vector<int> tl(out->lags ? (size_t)n : 0);
  for (int k = 0; k < 4; ++k)
    if (dst[k]) HCHK(h, hipMemcpyAsync(tmp.data() + (size_t)k * n, d_out.p + (size_t)k * n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (out->lags) HCHK(h, hipMemcpyAsync(tl.data(), d_lags.p, tl.size() * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HCHK(h, hipStreamSynchronize(h->stream));
  for (int k = 0; k < 4; ++k)
    if (dst[k])
      for (long long i = 0; i < n; ++i) dst[k][perm ? perm[i] : i] = tmp[(size_t)k * n + i];
  if (out->lags)
    for (long long i = 0; i < n; ++i) out->lags[perm ? perm[i] : i] = tl[i];
  return ST_OK;
}
