// Kernel translation unit of libspamtree_hip.so: rank-normalised R-hat, bulk, tail, quantile and exceedance ESS of the stored
// draws (rank_kernels.hpp has the evaluation order, include/spamtree_hip.h the definition).  k_series_rank reads a store of saved
// draws and writes only its own outputs and its own global slice; it draws nothing and touches no state of the chain.
#include "st_handle.hpp"
#include "diag_kernels.hpp"
#include "norm_quantile.hpp"
#include "rank_kernels.hpp"
#include "draw_store.hpp"
#include "series_tile.hpp"

// r2 = lo + hi + 1 of v among the sorted a[0 .. K): lo = #{a < v}, hi = #{a <= v}
__device__ __forceinline__ int rank_twice(const double *a, int K, double v) {
  const int lo = sorted_count_below(a, K, v);
  return lo + sorted_count_upto(a, K, v, lo) + 1;
}

// the bits of a word whose draw index base + b lies below `limit`
__device__ __forceinline__ unsigned long long rank_mask_below(int limit, int base) {
  const int nb = limit - base;
  return nb <= 0 ? 0ull : nb >= 64 ? ~0ull : (1ull << nb) - 1ull;
}

// A_t of the bit mask B (W = ceil(K / 64) words, bits at and beyond K clear, c bits set), t <= K - 2, by one lane
__device__ __forceinline__ long long rank_lag_numerator(const unsigned long long *B, int W, int K, int c, int t) {
  const long long Kl = K, cl = c;
  const int q = t >> 6, sh = t & 63;
  int n11 = 0, first = 0, last = 0;
  for (int w = 0; w < W; ++w) {
    const unsigned long long b = B[w];
    const unsigned long long u0 = w + q < W ? B[w + q] : 0ull, u1 = w + q + 1 < W ? B[w + q + 1] : 0ull;
    const unsigned long long shifted = sh ? (u0 >> sh) | (u1 << (64 - sh)) : u0;   // bit s: I_{s + t}
    n11 += __popcll(b & shifted);
    first += __popcll(b & rank_mask_below(t, 64 * w));
    last += __popcll(b & ~rank_mask_below(K - t, 64 * w));
  }
  const long long head = c - last, tail = c - first;
  return Kl * Kl * n11 - Kl * cl * (head + tail) + (Kl - t) * cl * cl;
}

// The indicator ESS of the bit mask B (W = ceil(K / 64) words, bits at and beyond K clear, c bits set), by one wave; every lane
// returns the same values.  Integers up to tau's one quotient.
__device__ __forceinline__ double rank_indicator_ess(const unsigned long long *B, int W, int K, int c, int L, int lane, int *lags) {
  *lags = 0;
  if (c == 0 || c == K) return __builtin_nan("");
  const long long Kl = K, cl = c;
  const long long A0 = Kl * cl * (Kl - cl);
  const double dK = (double)K;
  const int kmax = (L - 1) / 2, tmax = 2 * kmax + 1;   // tmax <= L <= K - 2
  long long nsum = 0, prev = 0x7fffffffffffffffll;     // the pairs' numerators: |N_k| <= 2^43, at most 2^13 of them
  int pairs = 0;
  bool stop = false;
  for (int t0 = 0; t0 <= tmax && !stop; t0 += 64) {
    const int t = t0 + lane;
    const long long At = t <= tmax ? rank_lag_numerator(B, W, K, c, t) : 0;
    for (int j = 0; j < 32 && !stop && t0 / 2 + j <= kmax; ++j) {
      const long long a0 = __shfl(At, 2 * j, 64), a1 = __shfl(At, 2 * j + 1, 64);
      long long N = a0 + a1;   // Gamma_k = N / A_0
      if (!(N > 0)) stop = true;
      else {
        N = N < prev ? N : prev;
        prev = N;
        nsum += N;
        ++pairs;
      }
    }
  }
  const double tau = fmax((double)(2 * nsum - A0) / (double)A0, 1.0 / log10(dK));
  *lags = 2 * pairs;
  return dK / tau;
}

// The multi-chain indicator ESS (rank_kernels.hpp, step 6 with M >= 2): chain c's mask is B + c Wc (Wc = ceil(N / 64) words, bits at
// and beyond N clear), its count is lane c's cL; every lane returns the same values.  Integers up to tau's one quotient.
__device__ __forceinline__ double rank_chain_indicator_ess(const unsigned long long *B, int Wc, int N, int M, int cL, int L, int lane,
                                                           int *lags) {
  *lags = 0;
  const long long Nl = N, Ml = M, K = Nl * Ml;
  long long C = 0;
  for (int ch = 0; ch < M; ++ch) C += __shfl(cL, ch, 64);
  if (C == 0 || C == K) return __builtin_nan("");
  long long D = 0, S0 = 0;
  for (int ch = 0; ch < M; ++ch) {
    const long long cc = __shfl(cL, ch, 64), e = Ml * cc - C;
    D += e * e;
    S0 += Nl * cc * (Nl - cc);
  }
  const long long ND = Nl * D, MM = Ml * (Ml - 1), Num0 = ND + MM * S0;   // > 0: 0 < C < K
  const int kmax = (L - 1) / 2, tmax = 2 * kmax + 1;   // tmax <= L <= N - 2
  long long nsum = 0, prev = 0x7fffffffffffffffll;     // the pairs' numerators: |N_k| < 2^42, at most 2^13 of them
  int pairs = 0;
  bool stop = false;
  for (int t0 = 0; t0 <= tmax && !stop; t0 += 64) {
    const int t = t0 + lane;
    long long St = 0;
    for (int ch = 0; ch < M; ++ch) {
      const int cc = __shfl(cL, ch, 64);   // (every lane takes part: the shuffle stands outside the lane's own condition)
      if (t <= tmax) St += rank_lag_numerator(B + (size_t)ch * Wc, Wc, N, cc, t);
    }
    const long long Nt = ND + MM * St;
    for (int j = 0; j < 32 && !stop && t0 / 2 + j <= kmax; ++j) {
      const long long a0 = __shfl(Nt, 2 * j, 64), a1 = __shfl(Nt, 2 * j + 1, 64);
      long long Np = a0 + a1;   // Gamma_k = Np / Num_0
      if (!(Np > 0)) stop = true;
      else {
        Np = Np < prev ? Np : prev;
        prev = Np;
        nsum += Np;
        ++pairs;
      }
    }
  }
  const double tau = fmax((double)(2 * nsum - Num0) / (double)Num0, 1.0 / log10((double)K));
  *lags = 2 * pairs;
  return (double)K / tau;
}

// steps 3 and 4 / 5 for the rows of one tile: the scores of v_s (x_s, or |x_s - med_r| with FOLD) among the sorted S_r into Z_r,
// then one wave per series over Z_r (LDS rows or rows of the global slice: each call site is inlined with its own address space).
// Returns through s_out[r] (LDS), written by lane 0.  CHAINS: the moments are diag_chain_wave's, of A.M chains.
template <bool FOLD, bool CHAINS>
__device__ __forceinline__ void rank_scores_and_moments(const RankArgs &A, const double *S, double *Z, const double *X, int nr,
                                                        const double *s_med, const int *s_nan, DiagOut *s_out, int tid) {
  const int K = A.K, lane = tid & 63, wid = tid >> 6;
  for (int idx = tid; idx < nr * K; idx += RANK_NT) {
    const int r = idx / K, s = idx - r * K;
    if (s_nan[r]) continue;
    double v = X[(size_t)r * K + s];
    if (FOLD) v = fabs(v - s_med[r]);
    Z[(size_t)r * A.Kz + s] = st_rank_score(rank_twice(S + (size_t)r * A.Kpad, K, v), K);
  }
  __syncthreads();
  for (int r = wid; r < nr; r += RANK_NT / 64) {
    if (s_nan[r]) continue;
    double *z = Z + (size_t)r * A.Kz;
    const DiagOut o = CHAINS ? diag_chain_wave<!FOLD>(z, K, A.M, A.L, lane) : diag_series_wave<!FOLD>(z, K, A.L, lane);
    if (lane == 0) s_out[r] = o;
  }
  __syncthreads();
}

// CHAINS: the multi-chain definition (A.M >= 2 chains) in steps 4 to 6; staging, sort and ranks are the same
template <bool CHAINS>
__global__ __launch_bounds__(RANK_NT) void k_series_rank(RankArgs A) {
  extern __shared__ double lds[];
  __shared__ double s_med[RANK_MAX_R], s_cq[RANK_MAX_R][RANK_NQ];
  __shared__ int s_nan[RANK_MAX_R];
  __shared__ DiagOut s_bulk[RANK_MAX_R], s_fold[RANK_MAX_R];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int K = A.K, Kpad = A.Kpad, R = A.R, W = (K + 63) >> 6;
  double *S = lds, *Zl = lds + (size_t)R * Kpad;
  double *X = A.scratch + (size_t)blockIdx.x * A.slice, *Zg = X + (size_t)R * K;
  const double inf = __builtin_inf(), nan = __builtin_nan("");
  const int nquant = A.n_prob + (A.want_tail ? 2 : 0), nind = nquant + A.n_thr;
  const bool need_sort = A.want_bulk || A.want_fold || nquant > 0;
  const long long ntiles = (A.n + R - 1) / R;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long row0 = tile * R;
    const int nr = (int)(A.n - row0 < R ? A.n - row0 : R);
    if (tid < RANK_MAX_R) s_nan[tid] = 0;
    __syncthreads();
    // 1: stage
    tile_stage(S, R, Kpad, Kpad, K, nr, tid, RANK_NT, [&](int d, int r) {
      const double v = A.draws[(size_t)d * A.n + row0 + r];
      X[(size_t)r * K + d] = v;
      if (v != v) s_nan[r] = 1;   // (every writer stores the same value)
      return v;
    });
    __syncthreads();
    // 2: sort; the median and the quantile thresholds (exceedances alone need neither: they read X)
    if (need_sort) tile_sort_rows(S, R, Kpad, tid, RANK_NT);
    if (need_sort && tid < 16 * nr) {
      const int r = tid >> 4, k = tid & 15;
      const double *a = S + (size_t)r * Kpad;
      if (k == 15) s_med[r] = (K & 1) ? a[(K - 1) / 2] : 0.5 * (a[K / 2 - 1] + a[K / 2]);
      else if (k < RANK_NQ) {
        const int which = k < A.n_prob ? k : k - A.n_prob + ST_RANK_MAX_PROBS;   // the caller's, then the tails
        if (k < nquant) s_cq[r][k] = a[A.jq[which]];
      }
    }
    __syncthreads();
    // 3, 4: bulk
    if (A.want_bulk) {
      if (A.z_global) rank_scores_and_moments<false, CHAINS>(A, S, Zg, X, nr, s_med, s_nan, s_bulk, tid);
      else rank_scores_and_moments<false, CHAINS>(A, S, Zl, X, nr, s_med, s_nan, s_bulk, tid);
    }
    // 5: folded
    if (A.want_fold) {
      for (int idx = tid; idx < R * Kpad; idx += RANK_NT) {
        const int r = idx / Kpad, s = idx - r * Kpad;
        S[idx] = (s < K && r < nr) ? fabs(X[(size_t)r * K + s] - s_med[r]) : inf;
      }
      __syncthreads();
      tile_sort_rows(S, R, Kpad, tid, RANK_NT);
      if (A.z_global) rank_scores_and_moments<true, CHAINS>(A, S, Zg, X, nr, s_med, s_nan, s_fold, tid);
      else rank_scores_and_moments<true, CHAINS>(A, S, Zl, X, nr, s_med, s_nan, s_fold, tid);
    }
    if (tid < nr) {
      const long long i = row0 + tid;
      const bool bad = s_nan[tid] != 0;
      const double rb = bad || !A.want_bulk ? nan : s_bulk[tid].rhat, rf = bad || !A.want_fold ? nan : s_fold[tid].rhat;
      if (A.rhat_bulk) A.rhat_bulk[i] = rb;
      if (A.ess_bulk) A.ess_bulk[i] = bad ? nan : s_bulk[tid].ess;
      if (A.lags_bulk) A.lags_bulk[i] = bad ? 0 : 2 * s_bulk[tid].pairs;
      if (A.rhat_fold) A.rhat_fold[i] = rf;
      if (A.rhat_rank) A.rhat_rank[i] = fmax(rb, rf);
    }
    // 6: the indicators, one wave per series; the masks go where the sorted copy was
    if (nind > 0) {
      __syncthreads();
      for (int r = wid; r < nr; r += RANK_NT / 64) {
        const long long i = row0 + r;
        const bool bad = s_nan[r] != 0;
        unsigned long long *B = (unsigned long long *)(S + (size_t)r * Kpad);   // W <= Kpad words
        const double *x = X + (size_t)r * K;
        double e05 = nan;
        for (int v = 0; v < nind; ++v) {
          const int t = v - nquant;   // >= 0: an exceedance
          int mode = 0;               // 0: x <= c;  1: x > c;  2: x < c
          double c;
          if (t < 0) c = s_cq[r][v];
          else {
            c = A.thr[(size_t)t * A.thr_stride + (A.per_series ? i : (A.outcome ? A.outcome[i] : 0))];
            mode = (A.neg >> t) & 1u ? 2 : 1;
          }
          double ess = nan;
          int cnt = 0, lags = 0;
          if (!bad && CHAINS) {   // every chain into words of its own: M ceil(N / 64) <= K / 64 + M < Kpad words
            const int N = K / A.M, Wc = (N + 63) >> 6;
            int cL = 0;
            for (int ch = 0; ch < A.M; ++ch) {
              int cc = 0;
              for (int base = 0; base < N; base += 64) {
                const int s = base + lane;
                bool p = false;
                if (s < N) {
                  const double xv = x[ch * N + s];
                  p = mode == 0 ? xv <= c : mode == 1 ? xv > c : xv < c;
                }
                const unsigned long long word = __ballot(p);
                if (lane == 0) B[ch * Wc + (base >> 6)] = word;
                cc += __popcll(word);
              }
              if (lane == ch) cL = cc;
              cnt += cc;
            }
            wave_lds_sync();
            ess = rank_chain_indicator_ess(B, Wc, N, A.M, cL, A.L, lane, &lags);
            wave_lds_sync();   // the next indicator overwrites the masks
          } else if (!bad) {
            for (int base = 0; base < K; base += 64) {
              const int s = base + lane;
              bool p = false;
              if (s < K) {
                const double xv = x[s];
                p = mode == 0 ? xv <= c : mode == 1 ? xv > c : xv < c;
              }
              const unsigned long long word = __ballot(p);
              if (lane == 0) B[base >> 6] = word;
              cnt += __popcll(word);
            }
            wave_lds_sync();
            ess = rank_indicator_ess(B, W, K, cnt, A.L, lane, &lags);
            wave_lds_sync();   // the next indicator overwrites the mask
          }
          if (v == A.n_prob && t < 0) e05 = ess;
          if (lane == 0) {
            if (v < A.n_prob) { if (A.ess_q) A.ess_q[(size_t)v * A.n + i] = ess; }
            else if (t < 0) { if (v == A.n_prob + 1 && A.ess_tail) A.ess_tail[i] = fmin(e05, ess); }
            else {
              const double pr = bad ? nan : (double)cnt / (double)K;
              if (A.ess_exc) A.ess_exc[(size_t)t * A.n + i] = ess;
              if (A.prob) A.prob[(size_t)t * A.n + i] = pr;
              if (A.mcse_prob) A.mcse_prob[(size_t)t * A.n + i] = bad ? nan : (cnt == 0 || cnt == K) ? 0.0 : sqrt(pr * (1.0 - pr) / ess);
            }
          }
        }
      }
    }
    __syncthreads();   // the next tile restages X and S
  }
}

// ---- host side
int series_rank_order(double prob, long long K) {
  const long long c = (long long)std::ceil(prob * (double)K);
  return (int)(std::min(std::max(c, 1ll), K - 1) - 1);
}

bool series_rank_plan(long long K, size_t lds_limit, int *R, int *Kpad, int *Kz, int *z_global) {
  const size_t kpad = (size_t)tile_pow2(K);
  const size_t kz = (size_t)(K | 1), lim = lds_limit > RANK_LDS_STATIC ? lds_limit - RANK_LDS_STATIC : 0;
  *Kpad = (int)kpad; *Kz = (int)kz;
  for (int zg = K > RANK_LDS_Z_MAX_K ? 1 : 0; zg < 2; ++zg) {   // z in LDS where it fits beside the sorted copy, else in the slice
    const size_t per = (kpad + (zg ? 0 : kz)) * sizeof(double);
    size_t r = std::min<size_t>(lim, RANK_TILE) / per;
    if (r < 1) r = lim / per;   // a long series: what the device allows
    if (r >= 1) { *R = (int)std::min<size_t>(r, RANK_MAX_R); *z_global = zg; return true; }
  }
  return false;
}

// The outputs out asks for, of one of the store's two sets of draws, into out's host arrays (any may be NULL), element i of the
// store at out[perm ? perm[i] : i].  store_chain_rank_diagnostics has checked the spec, K and n_chains.
static int series_rank_store(st_handle_s *h, const char *who, const DrawStore &s, const double *draws, int32_t n_chains,
                             const st_rank_spec *spec, const st_rank_out *out) {
  const long long n = s.n, K = s.K;
  if (!any_out(out)) return ST_OK;
  const bool bulk = out->rhat_rank || out->rhat_bulk || out->ess_bulk || out->lags_bulk, fold = out->rhat_rank || out->rhat_fold;
  const int n_prob = out->ess_q ? spec->n_prob : 0, n_thr = rank_exc_out(out) ? spec->n_thr : 0;   // (checked: positive where wanted)
  RankArgs A = {};
  A.draws = draws; A.n = n; A.K = (int)K; A.M = n_chains;
  A.L = (int)std::min<long long>(spec->max_lag == 0 ? ST_DIAG_DEFAULT_MAX_LAG : spec->max_lag, K / n_chains - 2);
  if (!series_rank_plan(K, h->lds_limit, &A.R, &A.Kpad, &A.Kz, &A.z_global)) {
    h->err = std::string(who) + ": the sorted copy of " + std::to_string(K) + " stored draws of one series does not fit one workgroup's LDS";
    return ST_ERR_UNSUPPORTED;
  }
  A.want_bulk = bulk; A.want_fold = fold; A.n_prob = n_prob; A.want_tail = out->ess_tail ? 1 : 0; A.n_thr = n_thr;
  for (int k = 0; k < n_prob; ++k) A.jq[k] = series_rank_order(spec->prob[k], K);
  A.jq[ST_RANK_MAX_PROBS] = series_rank_order(0.05, K);
  A.jq[ST_RANK_MAX_PROBS + 1] = series_rank_order(0.95, K);
  A.outcome = s.d_outcome; A.per_series = s.thr_per_series ? 1 : 0; A.thr_stride = s.n_thr_values();
  HCHK(h, hipSetDevice(h->device));
  DevBuf<double> d_thr, d_scr, d_out;
  DevBuf<int> d_lags;
  if (n_thr) {
    std::vector<double> tv;
    A.neg = thresholds_in_store_order(spec->thr, spec->side, n_thr, A.thr_stride, s.thr_per_series, s.perm, tv);
    HCHK(h, d_thr.upload(tv));
    A.thr = d_thr.p;
  }
  // the grid and its global slices
  A.slice = (long long)A.R * K + (A.z_global ? (long long)A.R * A.Kz : 0);
  const long long ntiles = (n + A.R - 1) / A.R;
  const long long by_bytes = std::max<long long>(1, RANK_SCRATCH_BYTES / (A.slice * (long long)sizeof(double)));
  const long long grid = std::min<long long>(ntiles, std::min<long long>(RANK_MAX_WGS, by_bytes));
  HCHK(h, d_scr.alloc((size_t)grid * A.slice));
  A.scratch = d_scr.p;
  // the outputs, device side: the five per-series doubles, ess_q, the three exceedance arrays
  const size_t n_dbl = (size_t)(5 + n_prob + 3 * n_thr) * n;
  HCHK(h, d_out.alloc(n_dbl));
  HCHK(h, d_lags.alloc((size_t)n));
  double *p = d_out.p;
  const auto take = [&](bool want, size_t rows) { double *q = want ? p : nullptr; p += rows * n; return q; };
  A.rhat_rank = take(out->rhat_rank, 1); A.rhat_bulk = take(out->rhat_bulk, 1); A.rhat_fold = take(out->rhat_fold, 1);
  A.ess_bulk = take(out->ess_bulk, 1); A.ess_tail = take(out->ess_tail, 1);
  A.ess_q = take(n_prob > 0, n_prob);
  A.ess_exc = take(n_thr && out->ess_exc, n_thr); A.mcse_prob = take(n_thr && out->mcse_prob, n_thr); A.prob = take(n_thr && out->prob, n_thr);
  A.lags_bulk = out->lags_bulk ? d_lags.p : nullptr;
  {
    ProfScope pscope(h, 3);
    const size_t lds = ((size_t)A.R * A.Kpad + (A.z_global ? 0 : (size_t)A.R * A.Kz)) * sizeof(double);
    const auto kernel = A.M > 1 ? k_series_rank<true> : k_series_rank<false>;
    HCHK(h, hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));   // (beside RANK_LDS_STATIC)
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(RANK_NT), lds, h->stream, A);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { h->err = std::string(who) + " launch: " + hipGetErrorString(e); return ST_ERR_HIP; }
  }
  // only what the caller asked for comes to the host
  return store_read_back(h, s,
                         {{out->rhat_rank, A.rhat_rank, 1}, {out->rhat_bulk, A.rhat_bulk, 1}, {out->rhat_fold, A.rhat_fold, 1},
                          {out->ess_bulk, A.ess_bulk, 1}, {out->ess_tail, A.ess_tail, 1}, {out->ess_q, A.ess_q, n_prob},
                          {out->ess_exc, A.ess_exc, n_thr}, {out->mcse_prob, A.mcse_prob, n_thr}, {out->prob, A.prob, n_thr}},
                         {{out->lags_bulk, A.lags_bulk, 1}});
}

// the single-chain call is the multi-chain one with one chain: the same refusals in the same order, the same kernel as before
int store_rank_diagnostics(st_handle_s *h, const char *who, const DrawStore &s, const st_rank_spec *spec, const st_rank_out *w,
                           const st_rank_out *yhat) {
  return store_chain_rank_diagnostics(h, who, s, 1, spec, w, yhat);
}

int store_chain_rank_diagnostics(st_handle_s *h, const char *who, const DrawStore &s, int32_t n_chains, const st_rank_spec *spec,
                                 const st_rank_out *w, const st_rank_out *yhat) {
  if (s.rc || s.n == 0) return s.rc;
  if (const int rc = check_rank_spec(std::string(who) + ": ", spec, s.K, s.n_thr_values(), w, yhat, h->err)) return rc;
  if (const int rc = check_chains(std::string(who) + ": ", n_chains, s.K, h->err)) return rc;
  if (yhat && s.yhat_needs_X) { h->err = std::string(who) + ": yhat needs the regressors X of st_points_set"; return ST_ERR_USAGE; }
  for (int which = 0; which < 2; ++which)
    if (const int rc = series_rank_store(h, who, s, which ? s.yhat : s.w, n_chains, spec, which ? yhat : w)) return rc;
  return ST_OK;
}

extern "C" int st_norm_quantile(const double *p, double *z, int64_t n) {
  if (n > 0 && (!p || !z)) return ST_ERR_USAGE;
  for (int64_t i = 0; i < n; ++i) z[i] = st_norm_quantile_f(p[i]);
  return ST_OK;
}
