// Kernel translation unit of libspamtree_hip.so: exceedance probabilities, excursion functions and simultaneous bands of the
// stored draws (excursion_kernels.hpp has the plan of the passes, include/spamtree_hip.h the definition).  The kernels read a store
// of saved draws and write only their own outputs; they draw nothing and touch no state of the chain.
//
// The definition, as evaluated here.  X[d][i], d < K, i < n; g(i) the domain (-1: masked out); thresholds c_t(i), sides s_t:
//   E_t(d,i)      X[d][i] > c_t(i) (s_t = +1) or X[d][i] < c_t(i) (s_t = -1), strict; false for a NaN draw
//   count_t(i)    #{d : E_t(d,i)};  prob_t(i) = count_t(i) / K
//   m_{t,g}(d)    max{count_t(i) : g(i) = g, not E_t(d,i)}, -1 if no series of the domain fails
//   excur_t(i)    #{d : m_{t,g(i)}(d) < count_t(i)} / K, NaN for g(i) = -1;  joint_all[t][g] = #{d : m_{t,g}(d) < 0} / K
//   mean, sd      Welford over ascending d: delta = x - m; m = fma(delta, r_d, m), r_d = 1 / (d + 1); M2 = fma(delta, x - m, M2);
//                 sd = sqrt(M2 / (K - 1))
//   maxdev[g][d]  max{|X[d][i] - mean_i| (1 / sd_i) : g(i) = g, sd_i > 0 and finite}, 0 without such a series; the others of the
//                 domain are counted in n_flat[g]
#include "st_handle.hpp"
#include "excursion_kernels.hpp"
#include "draw_store.hpp"
#include <cmath>

__device__ __forceinline__ bool exc_event(double x, double c, bool neg) { return neg ? x < c : x > c; }

// ---- pass 1: per series count_t and the Welford mean / sd.  TT: the thresholds the registers hold (T <= TT; the others compare
// against +inf on side +1 and never count)
template <int TT, bool BAND>
__global__ __launch_bounds__(EXC_NT) void k_store_colstats(ExcArgs A) {
  constexpr int TTm = TT ? TT : 1;
  const long long i = (long long)blockIdx.x * EXC_NT + threadIdx.x;
  const bool in = i < A.n;
  const long long ii = in ? i : A.n - 1;   // a lane past the end walks the last series and writes nothing: every load stays inside the store
  const int oc = A.outcome ? A.outcome[ii] : 0;
  double c[TTm];
  int cnt[TTm];
#pragma unroll
  for (int t = 0; t < TT; ++t) {
    c[t] = t < A.T ? A.thr[(size_t)t * A.thr_stride + (A.per_series ? ii : (long long)oc)] : __builtin_inf();
    cnt[t] = 0;
  }
  const unsigned neg = A.neg;
  const int K = A.K;
  const size_t n = (size_t)A.n;
  const double *p = A.draws + ii;
  double m = 0.0, M2 = 0.0;
  auto step = [&](double x, int d) {
#pragma unroll
    for (int t = 0; t < TT; ++t) cnt[t] += exc_event(x, c[t], (neg >> t) & 1u) ? 1 : 0;
    if (BAND) {
      const double delta = x - m;
      m = fma(delta, A.rinv[d], m);
      M2 = fma(delta, x - m, M2);
    }
  };
  int d = 0;
  for (; d + EXC_UNROLL <= K; d += EXC_UNROLL) {
    double x[EXC_UNROLL];
#pragma unroll
    for (int u = 0; u < EXC_UNROLL; ++u) x[u] = p[(size_t)(d + u) * n];
#pragma unroll
    for (int u = 0; u < EXC_UNROLL; ++u) step(x[u], d + u);
  }
  for (; d < K; ++d) step(p[(size_t)d * n], d);
  if (in) {
#pragma unroll
    for (int t = 0; t < TT; ++t)
      if (t < A.T) A.count[(size_t)t * n + i] = cnt[t];
  }
  if (BAND) {
    const double sd = sqrt(M2 / (double)(K - 1));
    if (in) { A.mean[i] = m; A.sd[i] = sd; }
    const int g = (in && !(A.mask && !A.mask[ii])) ? oc : -1;
    const bool flat = g >= 0 && !(sd > 0.0 && sd < __builtin_inf());
    for (int k = 0; k < A.G; ++k) {   // integer sums: one atomicAdd per wave and domain that has any
      const unsigned long long b = __ballot(flat && g == k);
      if (b && (threadIdx.x & 63) == 0) atomicAdd(&A.n_flat[k], (unsigned long long)__popcll(b));
    }
  }
}

// ---- pass 2: per draw m_{t,g} and maxdev_g over a tile of EXC_NT x S series, for a chunk of draws.
// A count is at most K <= 16384, so count + 1 fits 16 bits with 0 for "no failing series": the thresholds travel in pairs, two
// 16-bit fields per register, and one packed unsigned max (v_pk_max_u16) reduces both.  Per draw and domain a lane folds its S
// series into NP = ceil(TT / 2) packed words, four DPP steps leave every row of 16 lanes with its maximum, and the first lane of
// each row writes the row's words to LDS; the 4 NW rows of the workgroup meet in the flush after EXC_BATCH draws.
typedef unsigned short exc_us2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned exc_pkmax(unsigned a, unsigned b) {
  return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(exc_us2, a), __builtin_bit_cast(exc_us2, b)));
}
template <int CTRL>
__device__ __forceinline__ unsigned exc_ror(unsigned v) { return (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, 0xf, 0xf, false); }
__device__ __forceinline__ unsigned exc_row_pkmax(unsigned v) {   // the row's maximum in every lane of the row; all lanes active
  v = exc_pkmax(v, exc_ror<0x128>(v));
  v = exc_pkmax(v, exc_ror<0x124>(v));
  v = exc_pkmax(v, exc_ror<0x122>(v));
  return exc_pkmax(v, exc_ror<0x121>(v));
}
__device__ __forceinline__ double exc_row_max(double v) {   // v >= 0, no NaN
  v = fmax(v, dpp_mov_f64<0x128, 0xf>(v, v));
  v = fmax(v, dpp_mov_f64<0x124, 0xf>(v, v));
  v = fmax(v, dpp_mov_f64<0x122, 0xf>(v, v));
  return fmax(v, dpp_mov_f64<0x121, 0xf>(v, v));
}

// dynamic LDS of k_store_drawreduce: per draw of the batch and row of 16 lanes, G x NP packed words, then G doubles with the band
static size_t exc_pass2_lds(int TT, bool band, int G) {
  const size_t np = (size_t)(TT + 1) / 2, rows = EXC_NT / 16;
  return (size_t)EXC_BATCH * rows * G * (np * sizeof(unsigned) + (band ? sizeof(double) : 0));
}

template <int TT, bool BAND, int S>
__global__ __launch_bounds__(EXC_NT) void k_store_drawreduce(ExcArgs A) {
  constexpr int NP = (TT + 1) / 2, NPm = NP ? NP : 1, TTm = TT ? TT : 1, ROWS = EXC_NT / 16;
  extern __shared__ double exc_lds[];
  const int tid = threadIdx.x, lane = tid & 63, row = tid >> 4;
  const int K = A.K, G = A.G, T = A.T;
  double *s_dev = exc_lds;                                                          // [EXC_BATCH][ROWS][G], with the band
  unsigned *s_m = (unsigned *)(exc_lds + (BAND ? (size_t)EXC_BATCH * ROWS * G : 0));   // [EXC_BATCH][ROWS][G][NP]
  const size_t n = (size_t)A.n;
  const long long tile0 = (long long)blockIdx.x * (EXC_NT * S);
  const int d_lo = blockIdx.y * A.chunk, d_hi = min(K, d_lo + A.chunk);
  // the side data of the thread's S series: read once per chunk
  const double *p[S];
  int g[S];
  unsigned cp[S][NPm];   // count + 1 of thresholds 2 j and 2 j + 1 in the low and high half
  double c[S][TTm], mean[S], isd[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const long long i = tile0 + (long long)s * EXC_NT + tid;
    const bool in = i < A.n;
    const long long ii = in ? i : A.n - 1;   // past the end: the last series' loads, no domain
    const int oc = A.outcome ? A.outcome[ii] : 0;
    g[s] = (in && !(A.mask && !A.mask[ii])) ? oc : -1;
    p[s] = A.draws + ii;
#pragma unroll
    for (int j = 0; j < NP; ++j) cp[s][j] = 0;
#pragma unroll
    for (int t = 0; t < TT; ++t) {
      if (t < T) cp[s][t >> 1] |= (unsigned)(A.count[(size_t)t * n + ii] + 1) << (16 * (t & 1));   // t >= T: the field stays 0
      c[s][t] = t < T ? A.thr[(size_t)t * A.thr_stride + (A.per_series ? ii : (long long)oc)] : __builtin_inf();
    }
    mean[s] = 0.0; isd[s] = -1.0;
    if (BAND) {
      const double sd = A.sd[ii];
      mean[s] = A.mean[ii];
      isd[s] = (sd > 0.0 && sd < __builtin_inf()) ? 1.0 / sd : -1.0;   // -1: left out of maxdev
    }
  }
  const unsigned neg = A.neg;
  double xn[S];
  if (d_lo < d_hi) {
#pragma unroll
    for (int s = 0; s < S; ++s) xn[s] = p[s][(size_t)d_lo * n];
  }
  for (int d0 = d_lo; d0 < d_hi; d0 += EXC_BATCH) {
    const int nb = min(EXC_BATCH, d_hi - d0);
    for (int dd = 0; dd < nb; ++dd) {
      const int d = d0 + dd;
      double x[S];
#pragma unroll
      for (int s = 0; s < S; ++s) x[s] = xn[s];
      if (d + 1 < d_hi) {   // the next draw's loads go out before this draw's reductions
#pragma unroll
        for (int s = 0; s < S; ++s) xn[s] = p[s][(size_t)(d + 1) * n];
      }
      unsigned fw[S][NPm];   // the packed counts of the thresholds whose event fails at this draw, 0 in the other fields
      double dev[S];
#pragma unroll
      for (int s = 0; s < S; ++s) {
#pragma unroll
        for (int j = 0; j < NP; ++j) {
          unsigned keep = exc_event(x[s], c[s][2 * j], (neg >> (2 * j)) & 1u) ? 0u : 0xffffu;
          if (2 * j + 1 < TT) keep |= exc_event(x[s], c[s][(2 * j + 1) % TTm], (neg >> (2 * j + 1)) & 1u) ? 0u : 0xffff0000u;
          fw[s][j] = cp[s][j] & keep;
        }
        dev[s] = (BAND && isd[s] > 0.0) ? fabs(x[s] - mean[s]) * isd[s] : 0.0;
      }
      for (int k = 0; k < G; ++k) {
        unsigned v[NPm];
#pragma unroll
        for (int j = 0; j < NP; ++j) {
          unsigned a = 0;
#pragma unroll
          for (int s = 0; s < S; ++s) a = exc_pkmax(a, g[s] == k ? fw[s][j] : 0u);
          v[j] = exc_row_pkmax(a);
        }
        double dv = 0.0;
        if (BAND) {
#pragma unroll
          for (int s = 0; s < S; ++s) dv = g[s] == k ? fmax(dv, dev[s]) : dv;
          dv = exc_row_max(dv);
        }
        if ((lane & 15) == 0) {
          const size_t slot = ((size_t)dd * ROWS + row) * G + k;
#pragma unroll
          for (int j = 0; j < NP; ++j) s_m[slot * NPm + j] = v[j];
          if (BAND) s_dev[slot] = dv;
        }
      }
    }
    __syncthreads();
    // one value per tile, (t, g) and draw: integer atomicMax (the tiles of a draw meet here; the max does not depend on their order)
    const int TG = T * G;
    for (int idx = tid; idx < nb * TG; idx += EXC_NT) {
      const int dd = idx / TG, tg = idx - dd * TG, t = tg / G, k = tg - t * G;
      unsigned v = 0;
      for (int r = 0; r < ROWS; ++r) v = max(v, (s_m[(((size_t)dd * ROWS + r) * G + k) * NPm + (t >> 1)] >> (16 * (t & 1))) & 0xffffu);
      if (v > 0) atomicMax(&A.m[(size_t)tg * K + d0 + dd], (int)v - 1);
    }
    if (BAND) {
      for (int idx = tid; idx < nb * G; idx += EXC_NT) {
        const int dd = idx / G, k = idx - dd * G;
        double v = 0.0;
        for (int r = 0; r < ROWS; ++r) v = fmax(v, s_dev[((size_t)dd * ROWS + r) * G + k]);
        if (v > 0.0) atomicMax(&A.dev[(size_t)k * K + d0 + dd], (unsigned long long)__double_as_longlong(v));
      }
    }
    __syncthreads();
  }
}

// ---- the finish: histogram of m(d) per (t, g), its running sum H[c] = #{d : m(d) < c}, then excur and prob per series
__global__ __launch_bounds__(EXC_NT) void k_exc_hist(ExcArgs A) {
  const long long idx = (long long)blockIdx.x * EXC_NT + threadIdx.x;
  const long long tot = (long long)A.T * A.G * A.K;
  if (idx >= tot) return;
  const long long k = idx / A.K;
  atomicAdd(&A.hist[k * (A.K + 2) + A.m[idx] + 1], 1);   // m in -1 .. K: bin 0 .. K + 1
}

__global__ __launch_bounds__(EXC_NT) void k_exc_scan(ExcArgs A) {
  __shared__ int s_part[EXC_NT];
  const int tid = threadIdx.x, L = A.K + 2;
  int *hst = A.hist + (size_t)blockIdx.x * L;
  const int seg = (L + EXC_NT - 1) / EXC_NT, lo = min(L, tid * seg), hi = min(L, lo + seg);
  int sum = 0;
  for (int j = lo; j < hi; ++j) sum += hst[j];
  s_part[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int j = 0; j < EXC_NT; ++j) { const int v = s_part[j]; s_part[j] = run; run += v; }
  }
  __syncthreads();
  int run = s_part[tid];
  for (int j = lo; j < hi; ++j) { run += hst[j]; hst[j] = run; }   // H[j] = #{d : m(d) + 1 <= j}
  __syncthreads();
  if (tid == 0 && A.joint_all) A.joint_all[blockIdx.x] = (double)hst[0] / (double)A.K;
}

__global__ __launch_bounds__(EXC_NT) void k_exc_apply(ExcArgs A) {
  const long long idx = (long long)blockIdx.x * EXC_NT + threadIdx.x;
  if (idx >= (long long)A.T * A.n) return;
  const long long t = idx / A.n, i = idx - t * A.n;
  const int cnt = A.count[idx];
  A.prob[idx] = (double)cnt / (double)A.K;
  if (A.excur) {
    const int g = (A.mask && !A.mask[i]) ? -1 : (A.outcome ? A.outcome[i] : 0);
    A.excur[idx] = g >= 0 ? (double)A.hist[(t * A.G + g) * (A.K + 2) + cnt] / (double)A.K : __builtin_nan("");
  }
}

// ---- host side
template <int TT, bool BAND>
static void exc_launch_passes(const ExcArgs &A, bool pass2, dim3 g1, dim3 g2, hipStream_t st) {
  hipLaunchKernelGGL((k_store_colstats<TT, BAND>), g1, dim3(EXC_NT), 0, st, A);
  if (pass2) hipLaunchKernelGGL((k_store_drawreduce<TT, BAND, (TT > 1 ? 2 : 4)>), g2, dim3(EXC_NT), exc_pass2_lds(TT, BAND, A.G), st, A);
}

// The outputs out asks for, of one of the store's two sets of draws, into out's host arrays; element i of the store at position
// perm ? perm[i] : i of every per-series array, and spec->mask read there too.  store_excursions has checked spec and K.
static int series_exc_store(st_handle_s *h, const char *who, const DrawStore &s, const double *draws, const st_excursion_spec *spec,
                            const st_excursion_out *out) {
  const long long n = s.n, K = s.K;
  const int G = s.G;
  if (!out) return ST_OK;
  if (out->n_draws) *out->n_draws = K;
  const bool thr = exc_thr_out(out), band = exc_band_out(out);
  if (!thr && !band) return ST_OK;
  const int T = thr ? spec->n_thr : 0, TG = T * G;
  const bool joint = out->excur || out->joint_all, pass2 = joint || out->maxdev;
  HCHK(h, hipSetDevice(h->device));
  ExcArgs A = {};
  A.draws = draws; A.n = n; A.K = (int)K; A.T = T; A.G = G; A.outcome = s.d_outcome; A.per_series = s.thr_per_series ? 1 : 0;
  A.thr_stride = s.n_thr_values();
  // the small inputs, in store order
  DevBuf<unsigned char> d_mask;
  DevBuf<double> d_thr, d_rinv;
  if (spec->mask) {
    std::vector<unsigned char> mk;
    mask_in_store_order(spec->mask, n, s.perm, mk);
    HCHK(h, d_mask.upload(mk));
    A.mask = d_mask.p;
  }
  if (T) {
    std::vector<double> tv;
    A.neg = thresholds_in_store_order(spec->thr, spec->side, T, A.thr_stride, s.thr_per_series, s.perm, tv);
    HCHK(h, d_thr.upload(tv));
    A.thr = d_thr.p;
  }
  if (band) {
    std::vector<double> rv((size_t)K);
    for (long long d = 0; d < K; ++d) rv[d] = 1.0 / (double)(d + 1);
    HCHK(h, d_rinv.upload(rv));
    A.rinv = d_rinv.p;
  }
  DevBuf<int> d_count, d_m, d_hist;
  DevBuf<double> d_ms, d_pe, d_joint;
  DevBuf<unsigned long long> d_flat, d_dev;
  if (T) { HCHK(h, d_count.alloc((size_t)T * n)); A.count = d_count.p; }
  if (band) {
    HCHK(h, d_ms.alloc((size_t)2 * n)); A.mean = d_ms.p; A.sd = d_ms.p + n;
    HCHK(h, d_flat.alloc((size_t)G)); A.n_flat = d_flat.p;
    HCHK(h, hipMemsetAsync(d_flat.p, 0, (size_t)G * sizeof(unsigned long long), h->stream));
  }
  if (pass2 && T) {
    HCHK(h, d_m.alloc((size_t)TG * K)); A.m = d_m.p;
    HCHK(h, hipMemsetAsync(d_m.p, 0xff, (size_t)TG * K * sizeof(int), h->stream));   // -1
    HCHK(h, d_hist.alloc((size_t)TG * (K + 2))); A.hist = d_hist.p;
    HCHK(h, hipMemsetAsync(d_hist.p, 0, (size_t)TG * (K + 2) * sizeof(int), h->stream));
    HCHK(h, d_joint.alloc((size_t)TG)); A.joint_all = d_joint.p;
  }
  if (pass2 && band) {
    HCHK(h, d_dev.alloc((size_t)G * K)); A.dev = d_dev.p;
    HCHK(h, hipMemsetAsync(d_dev.p, 0, (size_t)G * K * sizeof(unsigned long long), h->stream));
  }
  if (T && (out->prob || out->excur)) {
    HCHK(h, d_pe.alloc((size_t)2 * T * n)); A.prob = d_pe.p;
    if (out->excur) A.excur = d_pe.p + (size_t)T * n;
  }
  // the grids: pass 1 one thread per series; pass 2 tiles of EXC_NT x S series times chunks of draws
  const int S = T > 1 ? 2 : 4;
  const long long tiles = (n + (long long)EXC_NT * S - 1) / ((long long)EXC_NT * S);
  long long nch = std::max<long long>(1, std::min<long long>((EXC_MIN_WGS + tiles - 1) / tiles, (K + EXC_BATCH - 1) / EXC_BATCH));
  long long chunk = (K + nch - 1) / nch;
  chunk = (chunk + EXC_BATCH - 1) / EXC_BATCH * EXC_BATCH;
  nch = (K + chunk - 1) / chunk;
  A.chunk = (int)chunk;
  const dim3 g1((unsigned)((n + EXC_NT - 1) / EXC_NT)), g2((unsigned)tiles, (unsigned)nch);
  {
    ProfScope pscope(h, 3);
    if (T == 0) exc_launch_passes<0, true>(A, pass2, g1, g2, h->stream);
    else if (T == 1 && band) exc_launch_passes<1, true>(A, pass2, g1, g2, h->stream);
    else if (T == 1) exc_launch_passes<1, false>(A, pass2, g1, g2, h->stream);
    else if (band) exc_launch_passes<8, true>(A, pass2, g1, g2, h->stream);
    else exc_launch_passes<8, false>(A, pass2, g1, g2, h->stream);
    if (pass2 && T) {
      hipLaunchKernelGGL(k_exc_hist, dim3((unsigned)(((long long)TG * K + EXC_NT - 1) / EXC_NT)), dim3(EXC_NT), 0, h->stream, A);
      hipLaunchKernelGGL(k_exc_scan, dim3((unsigned)TG), dim3(EXC_NT), 0, h->stream, A);
    }
    if (A.prob) hipLaunchKernelGGL(k_exc_apply, dim3((unsigned)(((long long)T * n + EXC_NT - 1) / EXC_NT)), dim3(EXC_NT), 0, h->stream, A);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { h->err = std::string(who) + " launch: " + hipGetErrorString(e); return ST_ERR_HIP; }
  }
  // only what the caller asked for comes to the host
  // the three that are not per series first: the read-back's one synchronise covers them
  std::vector<unsigned long long> hf(out->n_flat ? (size_t)G : 0);
  const auto d2h = [&](void *dst, const void *src, size_t bytes) { return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream); };
  if (out->joint_all) HCHK(h, d2h(out->joint_all, A.joint_all, (size_t)TG * sizeof(double)));
  if (out->maxdev) HCHK(h, d2h(out->maxdev, A.dev, (size_t)G * K * sizeof(double)));   // the bit patterns are the doubles
  if (out->n_flat) HCHK(h, d2h(hf.data(), A.n_flat, hf.size() * sizeof(unsigned long long)));
  if (const int rc = store_read_back(h, s, {{out->prob, A.prob, T}, {out->excur, A.excur, T}, {out->mean, A.mean, 1}, {out->sd, A.sd, 1}},
                                     {{out->count, A.count, T}})) return rc;
  for (int k = 0; out->n_flat && k < G; ++k) out->n_flat[k] = (int64_t)hf[k];
  return ST_OK;
}

int store_excursions(st_handle_s *h, const char *who, const DrawStore &s, const st_excursion_spec *spec, const st_excursion_out *w,
                     const st_excursion_out *yhat) {
  if (s.rc || s.n == 0) return s.rc;
  if (const int rc = check_excursion_spec(std::string(who) + ": ", spec, s.K, s.n_thr_values(), w, yhat, h->err)) return rc;
  if (yhat && s.yhat_needs_X) { h->err = std::string(who) + ": yhat needs the regressors X of st_points_set"; return ST_ERR_USAGE; }
  for (int which = 0; which < 2; ++which)
    if (const int rc = series_exc_store(h, who, s, which ? s.yhat : s.w, spec, which ? yhat : w)) return rc;
  return ST_OK;
}
