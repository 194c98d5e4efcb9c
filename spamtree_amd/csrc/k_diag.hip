// Kernel translation unit of libspamtree_hip.so: the convergence diagnostics of the stored draws (diag_kernels.hpp has the
// evaluation order, include/spamtree_hip.h the definition).  k_series_diag reads a store of saved draws and writes only its own
// outputs; it draws nothing and touches no state of the chain.
#include "st_handle.hpp"
#include "diag_kernels.hpp"
#include "draw_store.hpp"
#include "series_tile.hpp"

// CHAINS: the multi-chain definition (A.M >= 2 chains, diag_chain_wave); staging, tiles and outputs are the same
template <bool CHAINS>
__global__ __launch_bounds__(DIAG_NT) void k_series_diag(DiagArgs A) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, nw = blockDim.x >> 6;
  const int K = A.K, Kp = A.Kp, R = A.R;
  const long long row0 = (long long)blockIdx.x * R;
  const int nr = (int)(A.n - row0 < R ? A.n - row0 : R);
  // (no padding column: fill = K; the rows >= nr of the R Kp doubles get +inf, and nothing reads them)
  tile_stage(lds, R, Kp, K, K, nr, tid, blockDim.x, [&](int d, int r) { return A.draws[(size_t)d * A.n + row0 + r]; });
  __syncthreads();
  for (int r = wid; r < R && row0 + r < A.n; r += nw) {
    double *x = lds + (size_t)r * Kp;
    const DiagOut o = CHAINS ? diag_chain_wave<true>(x, K, A.M, A.L, lane) : diag_series_wave<true>(x, K, A.L, lane);
    if (lane == 0) {
      const long long i = row0 + r;
      if (A.ess) A.ess[i] = o.ess;
      if (A.mcse) A.mcse[i] = o.mcse;
      if (A.sd) A.sd[i] = o.sd;
      if (A.rhat) A.rhat[i] = o.rhat;
      if (A.lags) A.lags[i] = 2 * o.pairs;
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
  const auto kernel = A.M > 1 ? k_series_diag<true> : k_series_diag<false>;
  (void)hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_limit);
  hipLaunchKernelGGL(kernel, dim3((unsigned)((A.n + A.R - 1) / A.R)), dim3(64 * std::min(A.R, DIAG_NT / 64)), lds, st, A);
  return launch_rc();
}

// diagnostics of one of the store's two sets of draws into out's host arrays (any may be NULL), element i of the store at
// out[perm ? perm[i] : i]; store_chain_diagnostics has checked K, n_chains and max_lag
static int series_diag_store(st_handle_s *h, const char *who, const DrawStore &s, const double *draws, int32_t n_chains, int32_t max_lag,
                             const st_series_diag *out) {
  const long long n = s.n, K = s.K;
  if (!any_out(out)) return ST_OK;
  DiagArgs A;
  A.draws = draws; A.n = n; A.K = (int)K; A.M = n_chains;
  A.L = (int)std::min<long long>(max_lag == 0 ? ST_DIAG_DEFAULT_MAX_LAG : max_lag, K / n_chains - 2);
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
  return store_read_back(h, s, {{out->ess, A.ess, 1}, {out->mcse, A.mcse, 1}, {out->sd, A.sd, 1}, {out->rhat, A.rhat, 1}}, {{out->lags, A.lags, 1}});
}

// the single-chain call is the multi-chain one with one chain: the same refusals in the same order, the same kernel as before
int store_diagnostics(st_handle_s *h, const char *who, const DrawStore &s, int32_t max_lag, const st_series_diag *w, const st_series_diag *yhat) {
  return store_chain_diagnostics(h, who, s, 1, max_lag, w, yhat);
}

int store_chain_diagnostics(st_handle_s *h, const char *who, const DrawStore &s, int32_t n_chains, int32_t max_lag, const st_series_diag *w,
                            const st_series_diag *yhat) {
  if (s.rc) return s.rc;
  if (max_lag < 0) { h->err = std::string(who) + ": max_lag must not be negative (0: the default cap)"; return ST_ERR_USAGE; }
  if (s.n == 0) return ST_OK;
  if (s.K < ST_DIAG_MIN_DRAWS) {
    h->err = std::string(who) + ": " + std::to_string(s.K) + " draws stored, the diagnostics need at least " + std::to_string(ST_DIAG_MIN_DRAWS) +
             " (call " + s.reserve + " before the saved iterations)";
    return ST_ERR_USAGE;
  }
  if (const int rc = check_chains(std::string(who) + ": ", n_chains, s.K, h->err)) return rc;
  if (yhat && s.yhat_needs_X) { h->err = std::string(who) + ": yhat needs the regressors X of st_points_set"; return ST_ERR_USAGE; }
  for (int which = 0; which < 2; ++which)
    if (const int rc = series_diag_store(h, who, s, which ? s.yhat : s.w, n_chains, max_lag, which ? yhat : w)) return rc;
  return ST_OK;
}
