// Kernel translation unit of libspamtree_hip.so: the leave-group-out criteria (lgo_kernels.hpp has the definitions, the order of
// every operation and the rounding bound).  The kernels read what the upward sweep of k_rows_loo.hip left (d, c, the per-pair
// array), w, XB, y and tausq_inv and write only the groups' own state.
#include "lgo_kernels.hpp"
#pragma clang fp contract(off)

// The unpivoted right-looking Cholesky of the g x g lower triangle in a (LDS, row i owned by lane i; an idle lane passes
// i >= g), the diagonal of the factor into sd.  Every thread of the workgroup calls it: the barriers are uniform.
// Returns whether a pivot was not > 0.
__device__ __forceinline__ bool chol16(double (*a)[LGO_MAXG + 1], double *sd, int g, int i) {
  bool bad = false;
  for (int k = 0; k < LGO_MAXG; ++k) {
    __syncthreads();
    if (k < g) {
      const double piv = a[k][k];
      bad |= !(piv > 0.0);
      const double s = sqrt(piv);
      if (i == k) sd[k] = s;
      if (i > k && i < g) a[i][k] = a[i][k] / s;
    }
    __syncthreads();
    if (k < g && i > k && i < g) {
      const double lik = a[i][k];
      for (int j = k + 1; j <= i; ++j) a[i][j] = fma(-lik, a[j][k], a[i][j]);
    }
  }
  __syncthreads();
  return bad;
}

__global__ __launch_bounds__(LGO_WG) void k_lgo_groups(LgoArgs A) {
  constexpr int NG = LGO_WG / LGO_MAXG;
  __shared__ double sA[NG][LGO_MAXG][LGO_MAXG + 1], sV[NG][LGO_MAXG][LGO_MAXG + 1];
  __shared__ double sD[NG][LGO_MAXG], sC[NG][LGO_MAXG], sR[NG][LGO_MAXG], sZ[NG][LGO_MAXG], sL[NG];
  __shared__ int sO[NG][LGO_MAXG];
  const int sub = threadIdx.x / LGO_MAXG, i = threadIdx.x % LGO_MAXG;
  const int gi = blockIdx.x * NG + sub;
  const long long n = A.n;
  int g = 0, m0 = 0, gp0 = 0, sq0 = 0;
  if (gi < A.G) { m0 = A.grp_ptr[gi]; g = A.grp_ptr[gi + 1] - m0; gp0 = A.gp_ptr[gi]; sq0 = A.sq_ptr[gi]; }
  const bool mine = i < g;
  const long long row = mine ? A.mem_row[m0 + i] : 0;
  double (*a)[LGO_MAXG + 1] = sA[sub], (*v)[LGO_MAXG + 1] = sV[sub];
  double *sd = sD[sub];
  // 1. gather
  double wi = 0.0, ci = 0.0;
  if (mine) {
    const double d = A.last[LOO_LAST_QD * n + row];
    ci = A.last[LOO_LAST_QW * n + row];
    wi = A.w[row];
    a[i][i] = d;
    A.last_q[sq0 + i * g + i] = d;
    for (int j = 0; j < i; ++j) {
      const int slot = A.gp_idx[gp0 + i * (i - 1) / 2 + j];
      const double p = slot >= 0 ? A.pairval[slot] : 0.0;
      a[i][j] = p;
      A.last_q[sq0 + i * g + j] = p;
      A.last_q[sq0 + j * g + i] = p;
    }
    sC[sub][i] = ci;
    A.last_c[m0 + i] = ci;
  }
  // 2. A = L L'
  bool bad = chol16(a, sd, g, mine ? i : LGO_MAXG);
  // 3. column i of V = A^-1
  if (mine) {
    for (int r = 0; r < i; ++r) v[r][i] = 0.0;
    for (int r = i; r < g; ++r) {
      double s = r == i ? 1.0 : 0.0;
      for (int k = i; k < r; ++k) s = fma(-a[r][k], v[k][i], s);
      v[r][i] = s / sd[r];
    }
    for (int r = g - 1; r >= 0; --r) {
      double s = v[r][i];
      for (int k = r + 1; k < g; ++k) s = fma(-a[k][r], v[k][i], s);
      v[r][i] = s / sd[r];
    }
    for (int r = 0; r < g; ++r) A.last_v[sq0 + r * g + i] = v[r][i];
  }
  __syncthreads();
  // 4. the conditional mean
  double mi = 0.0;
  if (mine) {
    double s = 0.0;
    for (int j = 0; j < g; ++j) s = fma(v[i][j], sC[sub][j], s);
    mi = wi - s;
    A.last_m[m0 + i] = mi;
  }
  // 5. the observed members, Sigma and the joint log density
  const bool ob = mine && A.obs[row] != 0;
  sO[sub][i] = ob ? 1 : 0;
  __syncthreads();
  int ro = 0, go = 0;
  for (int j = 0; j < LGO_MAXG; ++j) { ro += (j < i && sO[sub][j]) ? 1 : 0; go += sO[sub][j]; }
  __syncthreads();
  double mu = 0.0, yi = 0.0, sii = 1.0;
  if (ob) {
    sO[sub][ro] = i;           // the observed members in member order (entries below go)
    mu = A.xb[row] + mi;
    yi = A.y[row];
    sR[sub][ro] = yi - mu;
  }
  __syncthreads();               // (also: every lane has left L in `a`)
  if (ob) {
    for (int k = 0; k < ro; ++k) a[ro][k] = v[i][sO[sub][k]];
    sii = v[i][i] + 1.0 / A.tsq_inv[A.mv[row]];
    a[ro][ro] = sii;
  }
  bad |= chol16(a, sd, go, ob ? ro : LGO_MAXG);
  if (i == 0) {
    double quad = 0.0, ld = 0.0;
    for (int r = 0; r < go; ++r) {
      double s = sR[sub][r];
      for (int k = 0; k < r; ++k) s = fma(-a[r][k], sZ[sub][k], s);
      const double z = s / sd[r];
      sZ[sub][r] = z;
      quad = fma(z, z, quad);
      ld = ld + log(sd[r]);
    }
    sL[sub] = fma(-0.5, quad, -ld) + (double)go * HL2PI;
  }
  __syncthreads();
  // 6. the streaming update
  const double l = sL[sub];
  const bool skip = bad || !(l >= -__DBL_MAX__ && l <= __DBL_MAX__);
  double M = 0.0, A1 = 0.0, A2 = 0.0, NS = 0.0, AP = 0.0, AM = 0.0;
  if (gi < A.G) {
    M = A.gacc[LGO_M * A.G + gi]; A1 = A.gacc[LGO_A1 * A.G + gi]; A2 = A.gacc[LGO_A2 * A.G + gi]; NS = A.gacc[LGO_NS * A.G + gi];
  }
  __syncthreads();
  if (gi >= A.G) return;
  if (skip) {
    if (i == 0) { A.gacc[LGO_NS * A.G + gi] = NS + 1.0; if (A.st_t) A.st_t[gi] = __builtin_nan(""); }
    return;
  }
  if (i == 0 && A.st_t) A.st_t[gi] = -l;
  const long long nm = A.grp_ptr[A.G];
  double phi = 0.0;
  if (ob) {
    const double z = (yi - mu) / sqrt(sii);
    phi = 0.5 * erfc(-z * 0.70710678118654752440);
    AP = A.macc[LGO_AP * nm + m0 + i]; AM = A.macc[LGO_AM * nm + m0 + i];
  }
  const double t = -l;
  if (A1 == 0.0) { M = t; A1 = 1.0; A2 = 1.0; AP = phi; AM = mu; }
  else if (t <= M) {
    const double x = exp(t - M);
    A1 = A1 + x; A2 = fma(x, x, A2); AP = fma(x, phi, AP); AM = fma(x, mu, AM);
  } else {
    const double x = exp(M - t), x2 = x * x;
    A1 = fma(A1, x, 1.0); A2 = fma(A2, x2, 1.0); AP = fma(AP, x, phi); AM = fma(AM, x, mu); M = t;
  }
  if (i == 0) { A.gacc[LGO_M * A.G + gi] = M; A.gacc[LGO_A1 * A.G + gi] = A1; A.gacc[LGO_A2 * A.G + gi] = A2; }
  if (ob) { A.macc[LGO_AP * nm + m0 + i] = AP; A.macc[LGO_AM * nm + m0 + i] = AM; }
}

// lgo_kernels.hpp, FINISH
__global__ __launch_bounds__(NT) void k_lgo_finish(LgoFinishArgs A) {
  __shared__ double sm[LGO_NTOT][NT];
  const int v = blockIdx.x, tid = threadIdx.x;
  const int G = A.G;
  const double nan = __builtin_nan("");
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  if (v == A.q) {
    s2 = __builtin_inf();
    for (int g = tid; g < G; g += NT) {
      const double Sg = A.S - A.gacc[LGO_NS * G + g], A1 = A.gacc[LGO_A1 * G + g];
      double elpd = nan, ess = nan;
      if (Sg > 0.0) {
        elpd = -(A.gacc[LGO_M * G + g] + log(A1 / Sg));
        ess = A1 * A1 / A.gacc[LGO_A2 * G + g];
        s0 += elpd; s2 = fmin(s2, ess); s3 += 1.0;
      }
      A.gout[g] = elpd; A.gout[G + g] = ess;
    }
  } else {
    const long long nm = A.n_members;
    for (long long k = tid; k < nm; k += NT) {
      const long long row = A.mem_row[k];
      if (A.mv[row] != v || !A.obs[row]) continue;
      const int g = A.mem_grp[k];
      const double Sg = A.S - A.gacc[LGO_NS * G + g], A1 = A.gacc[LGO_A1 * G + g];
      double mu = nan, pit = nan;
      if (Sg > 0.0) {
        mu = A.macc[LGO_AM * nm + k] / A1;
        pit = A.macc[LGO_AP * nm + k] / A1;
        const double r = A.y[row] - mu;
        s0 = fma(r, r, s0); s1 += pit; s2 += 1.0;
      }
      A.rows[row] = mu; A.rows[A.n + row] = pit;
    }
  }
  sm[0][tid] = s0; sm[1][tid] = s1; sm[2][tid] = s2; sm[3][tid] = s3;
  __syncthreads();
  for (int o = NT / 2; o > 0; o >>= 1) {
    if (tid < o) {
      sm[0][tid] += sm[0][tid + o]; sm[1][tid] += sm[1][tid + o]; sm[3][tid] += sm[3][tid + o];
      sm[2][tid] = v == A.q ? fmin(sm[2][tid], sm[2][tid + o]) : sm[2][tid] + sm[2][tid + o];
    }
    __syncthreads();
  }
  if (v == A.q) {
    // the centred sum of squares in a second pass over the thread's own groups: no cancellation of sum e^2 against (sum e)^2 / G
    const double sum = sm[0][0], ess = sm[2][0], cnt = sm[3][0];
    const double mean = sum / cnt;
    __syncthreads();
    double c = 0.0;
    for (int g = tid; g < G; g += NT) {
      const double e = A.gout[g];
      if (e == e) { const double dlt = e - mean; c = fma(dlt, dlt, c); }
    }
    sm[1][tid] = c;
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
      if (tid < o) sm[1][tid] += sm[1][tid + o];
      __syncthreads();
    }
    if (tid == 0) { A.tot[LGO_TOT_ELPD] = sum; A.tot[LGO_TOT_ELPD_SQ] = sm[1][0]; A.tot[LGO_TOT_MIN_ESS] = ess; A.tot[LGO_TOT_COUNT] = cnt; }
  } else if (tid < LGO_NOUTC) A.tot[LGO_NTOT + v * LGO_NOUTC + tid] = sm[tid][0];
}

int lgo_groups_launch(const LgoArgs &A, hipStream_t st) {
  if (A.G <= 0) return 0;
  constexpr int NG = LGO_WG / LGO_MAXG;
  hipLaunchKernelGGL(k_lgo_groups, dim3((A.G + NG - 1) / NG), dim3(LGO_WG), 0, st, A);
  return launch_rc();
}

int lgo_finish_launch(const LgoFinishArgs &A, hipStream_t st) {
  if (A.G <= 0 || A.q < 1) return 0;
  hipLaunchKernelGGL(k_lgo_finish, dim3(A.q + 1), dim3(NT), 0, st, A);
  return launch_rc();
}
