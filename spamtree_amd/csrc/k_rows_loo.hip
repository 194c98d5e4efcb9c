// Kernel translation unit of libspamtree_hip.so: the leave-one-out criteria with the latent field integrated out
// (loo_kernels.hpp has the definitions, the order of every sum and the rounding bound).  The kernels read slot 0's panels, w, XB, y
// and tausq_inv and write only the upward vectors and the criteria's own state: no other step reads what they write.
#include "loo_kernels.hpp"
#pragma clang fp contract(off)

static const char *const k_loo_route_names[LOO_ROUTE_COUNT] = {"", "k_loo_block<ref>", "k_loo_block<leaf>"};
const char *loo_route_name(int code) { return (code >= 0 && code < LOO_ROUTE_COUNT) ? k_loo_route_names[code] : nullptr; }

// step 5 of a row: the conditional moments and the streaming update (loo_kernels.hpp, STREAMING STATE)
__device__ __forceinline__ void loo_row(const LooArgs &A, long long i, double wi, double d, double c) {
  const long long n = A.n;
  const double v = 1.0 / d;
  const double mi = wi - c / d;
  A.last[LOO_LAST_QD * n + i] = d;
  A.last[LOO_LAST_QW * n + i] = c;
  A.last[LOO_LAST_MEAN * n + i] = mi;
  A.last[LOO_LAST_VAR * n + i] = v;
  if (!A.obs[i]) return;
  const double mu = A.xb[i] + mi;
  const double sig = sqrt(v + 1.0 / A.tsq_inv[A.mv[i]]);
  const double z = (A.y[i] - mu) / sig;
  const double l = fma(-0.5 * z, z, -log(sig)) + HL2PI;
  if (!(l >= -__DBL_MAX__ && l <= __DBL_MAX__)) {
    A.acc[LOO_NS * n + i] += 1.0;
    if (A.st_t) { const double nan = __builtin_nan(""); A.st_t[i] = nan; A.st_phi[i] = nan; A.st_mu[i] = nan; }
    return;
  }
  const double phi = 0.5 * erfc(-z * 0.70710678118654752440);
  const double t = -l;
  if (A.st_t) { A.st_t[i] = t; A.st_phi[i] = phi; A.st_mu[i] = mu; }
  double M = A.acc[LOO_M * n + i], A1 = A.acc[LOO_A1 * n + i], A2 = A.acc[LOO_A2 * n + i], AP = A.acc[LOO_AP * n + i],
         AM = A.acc[LOO_AM * n + i];
  if (A1 == 0.0) { M = t; A1 = 1.0; A2 = 1.0; AP = phi; AM = mu; }
  else if (t <= M) {
    const double x = exp(t - M);
    A1 = A1 + x; A2 = fma(x, x, A2); AP = fma(x, phi, AP); AM = fma(x, mu, AM);
  } else {
    const double x = exp(M - t), x2 = x * x;
    A1 = fma(A1, x, 1.0); A2 = fma(A2, x2, 1.0); AP = fma(AP, x, phi); AM = fma(AM, x, mu); M = t;
  }
  A.acc[LOO_M * n + i] = M; A.acc[LOO_A1 * n + i] = A1; A.acc[LOO_A2 * n + i] = A2; A.acc[LOO_AP * n + i] = AP;
  A.acc[LOO_AM * n + i] = AM;
}

template <bool REF, bool PAIRS>
__global__ __launch_bounds__(NT) void k_loo_block(LooArgs A) {
  extern __shared__ double lds[];                   // x[P + m], e[m]
  __shared__ int s_am[MAXJ], s_ao[MAXJ + 1];
  __shared__ long long s_arow[MAXJ];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int li = blockIdx.x;
  if (li >= A.nlist) return;
  const int b = A.list[li];
  const Blk B = A.blks[b];
  const int m = B.m, P = B.P, J = B.nanc, ld = B.ld, len = P + m;
  const double *pan = A.panels + B.panel_off;
  double *x = lds, *e = lds + len;
  if (tid < J) {
    const Blk Ba = A.blks[A.anc_idx[B.anc_ptr + tid]];
    s_am[tid] = Ba.m;
    s_arow[tid] = Ba.row0;
  }
  __syncthreads();
  if (tid == 0) {
    int o = 0;
    for (int t = 0; t < J; ++t) { s_ao[t] = o; o += s_am[t]; }
    s_ao[J] = o;                                    // = P
  }
  __syncthreads();
  // 0. the chain's w and the block's own
  for (int k = tid; k < len; k += NT) {
    long long row;
    if (k < P) { const int t = anc_of(s_ao, J, k); row = s_arow[t] + (k - s_ao[t]); }
    else row = B.row0 + (k - P);
    x[k] = A.w[row];
  }
  __syncthreads();
  // 1. e = L x, one wave per row
  for (int r = wid; r < m; r += NT / 64) {
    const double *lr = pan + (size_t)r * ld;
    const int ncol = REF ? P + r + 1 : P + 1;
    double acc = 0.0;
    for (int k = lane; k < ncol; k += 64) acc = fma(lr[k], (!REF && k == P) ? x[P + r] : x[k], acc);
    acc = wave_allsum(acc);
    if (lane == 0) e[r] = acc;
  }
  __syncthreads();
  // 2. - 5. one thread per column
  const long long vo = A.voff[b];
  const int c0 = A.ch_ptr[b], c1 = A.ch_ptr[b + 1];
  for (int k = tid; k < len; k += NT) {
    double d = 0.0, c = 0.0;
    if (k < P) {
      for (int r = 0; r < m; ++r) { const double v = pan[(size_t)r * ld + k]; d = fma(v, v, d); c = fma(v, e[r], c); }
    } else if (REF) {
      for (int r = k - P; r < m; ++r) { const double v = pan[(size_t)r * ld + k]; d = fma(v, v, d); c = fma(v, e[r], c); }
    } else {
      const double v = pan[(size_t)(k - P) * ld + P];
      d = fma(v, v, d); c = fma(v, e[k - P], c);
    }
    for (int j = c0; j < c1; ++j) {
      const int ch = A.ch_idx[j];
      const Blk Bc = A.blks[ch];
      const double *Sc = A.S + A.voff[ch];
      d += Sc[k];
      c += Sc[Bc.P + Bc.m + k];
    }
    A.S[vo + k] = d;
    A.S[vo + len + k] = c;
    if (k >= P) loo_row(A, B.row0 + (k - P), x[k], d, c);
  }
  // the pair part (lgo_kernels.hpp): one thread per pair slot of S_u
  if (PAIRS) {
    const int p0 = A.pr_ptr[b], np = A.pr_ptr[b + 1] - p0;
    for (int t = tid; t < np; t += NT) {
      const int ca = A.pr_a[p0 + t], cb = A.pr_b[p0 + t];
      double p = 0.0;
      if (REF || cb < P) {
        for (int r = cb < P ? 0 : cb - P; r < m; ++r) p = fma(pan[(size_t)r * ld + ca], pan[(size_t)r * ld + cb], p);
      } else {
        p = fma(pan[(size_t)(cb - P) * ld + ca], pan[(size_t)(cb - P) * ld + P], p);
      }
      for (int j = c0; j < c1; ++j) {
        const int ch = A.ch_idx[j];
        const Blk Bc = A.blks[ch];
        p += A.S[A.voff[ch] + 2ll * (Bc.P + Bc.m) + t];
      }
      A.S[vo + 2ll * len + t] = p;
      const int fin = A.pr_fin[p0 + t];
      if (fin >= 0) A.pairval[fin] = p;
    }
  }
}

// Per-row outputs and the per-outcome totals: workgroup v takes outcome v; every workgroup writes the outputs of its own
// outcome's rows and NaN at the rows without an observed y of that outcome.  Thread t walks the rows t, t + NT, ... ascending,
// then the NT partial values meet in a fixed binary tree in LDS (sums; the minimum for weight_ess).
__global__ __launch_bounds__(NT) void k_loo_finish(LooFinishArgs A) {
  __shared__ double sm[LOO_NSUM][NT];
  const int v = blockIdx.x, tid = threadIdx.x;
  const long long n = A.n;
  const double nan = __builtin_nan("");
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = __builtin_inf();
  for (long long i = tid; i < n; i += NT) {
    if (A.mv[i] != v) continue;
    double elpd = nan, pit = nan, mu = nan, ess = nan;
    if (A.obs[i]) {
      const double Si = A.S - A.acc[LOO_NS * n + i];
      const double A1 = A.acc[LOO_A1 * n + i];
      if (Si > 0.0) {
        elpd = -(A.acc[LOO_M * n + i] + log(A1 / Si));
        pit = A.acc[LOO_AP * n + i] / A1;
        mu = A.acc[LOO_AM * n + i] / A1;
        ess = A1 * A1 / A.acc[LOO_A2 * n + i];
        const double r = A.y[i] - mu;
        s0 += elpd; s1 = fma(r, r, s1); s2 += pit; s3 = fmin(s3, ess);
      }
    }
    A.rows[LOO_OUT_ELPD * n + i] = elpd; A.rows[LOO_OUT_PIT * n + i] = pit; A.rows[LOO_OUT_MU * n + i] = mu;
    A.rows[LOO_OUT_ESS * n + i] = ess;
  }
  sm[0][tid] = s0; sm[1][tid] = s1; sm[2][tid] = s2; sm[3][tid] = s3;
  __syncthreads();
  for (int o = NT / 2; o > 0; o >>= 1) {
    if (tid < o) {
      sm[0][tid] += sm[0][tid + o]; sm[1][tid] += sm[1][tid + o]; sm[2][tid] += sm[2][tid + o];
      sm[3][tid] = fmin(sm[3][tid], sm[3][tid + o]);
    }
    __syncthreads();
  }
  if (tid < LOO_NSUM) A.tot[v * LOO_NSUM + tid] = sm[tid][0];
}

template <bool REF, bool PAIRS>
static void loo_launch_level(int count, size_t lds, hipStream_t st, const LooArgs &A) {
  (void)hipFuncSetAttribute((const void *)k_loo_block<REF, PAIRS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL((k_loo_block<REF, PAIRS>), dim3(count), dim3(NT), lds, st, A);
}

int loo_launch(const LooLevelLaunch *lv, int nlev, const LooArgs &A0, hipStream_t st, int *route_mask) {
  int mask = 0;
  for (int g = 0; g < nlev; ++g) {
    const LooLevelLaunch &L = lv[g];
    if (L.count == 0) continue;
    LooArgs A = A0;
    A.list = A0.list + L.first;
    A.nlist = L.count;
    const size_t lds = LOO_LDS(L.maxLen, L.maxM);
    const bool pairs = A.pr_ptr != nullptr;
    if (L.isref && pairs) loo_launch_level<true, true>(L.count, lds, st, A);
    else if (L.isref) loo_launch_level<true, false>(L.count, lds, st, A);
    else if (pairs) loo_launch_level<false, true>(L.count, lds, st, A);
    else loo_launch_level<false, false>(L.count, lds, st, A);
    mask |= 1 << ((L.isref ? LOO_ROUTE_REF : LOO_ROUTE_LEAF) - 1);
    if (const int e = launch_rc()) { *route_mask = mask; return e; }
  }
  *route_mask = mask;
  return 0;
}

int loo_finish_launch(const LooFinishArgs &A, hipStream_t st) {
  if (A.n <= 0 || A.q < 1) return 0;
  hipLaunchKernelGGL(k_loo_finish, dim3(A.q), dim3(NT), 0, st, A);
  return launch_rc();
}
