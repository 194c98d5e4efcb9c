// Kernel translation unit of libspamtree_hip.so: the exceedance step of st_points_accumulate (points_exceed.hpp has the
// definition).  It reads d_out, d_pmv, d_X, d_B, d_tsq and the functionals' d_last, draws nothing and writes only the exceedance
// state: no other step reads what it writes.
#include "points_exceed.hpp"

#define EX_RSQRT2 0.70710678118654752440

// One draw's probability of the event s (m - c) > 0 for a Gaussian of mean m and standard deviation sd = sqrt(v), d = s (m - c):
// Phi(d / sd) as k_score_acc forms it (one division, one multiplication, erfc, one halving -- the last exact), or the strict
// indicator when the Gaussian is a point mass.  d / sd = +-inf gives erfc's limits 0 and 2: never NaN for d finite or infinite.
__device__ __forceinline__ double ex_prob(double d, double v, double sd) {
  if (v > 0.0) return 0.5 * erfc(-(d / sd) * EX_RSQRT2);
  return d > 0.0 ? 1.0 : 0.0;
}

// k_points_acc's Welford update of (mean, M2) with the host's count, on one slot of a state [...][{mean, M2}][n]
__device__ __forceinline__ void ex_welford(double *slot, long long n, long long i, double x, double count) {
  const double m0 = slot[EX_MEAN * n + i];
  const double d = x - m0;
  const double m1 = m0 + d / count;
  slot[EX_MEAN * n + i] = m1;
  slot[EX_M2 * n + i] += d * (x - m1);
}

// One thread per point: reads cond_mean, cond_var, the margin (20 B) and, for the yhat target, p regressors (8 p B); per threshold
// and target the two state values (16 B), written back (16 B).  In order: sd = sqrt(v); with X: xb (p fma, k = 0..p-1), mu = xb + m,
// s2 = v + 1 / tausq_inv, sigma = sqrt(s2); then t = 0..T-1: c = thr[t q + j], d = s (m - c) (one subtraction; the sign is exact),
// p = ex_prob, the Welford update of target w; d = s (mu - c), p, the update of target yhat.
__global__ __launch_bounds__(NT) void k_exceed_acc(ExceedArgs A) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  const long long n = A.n;
  const int j = A.pmv[i], T = A.n_thr;
  const double m = A.mean[i], v = A.var[i];
  const double sd = sqrt(v);
  double mu = 0.0, s2 = 1.0, sig = 1.0;
  if (A.X) {
    const double *bj = A.B + (size_t)A.p * j;
    double xb = 0.0;
    for (int k = 0; k < A.p; ++k) xb = fma(A.X[(size_t)k * n + i], bj[k], xb);
    mu = xb + m;
    s2 = v + 1.0 / A.tsq_inv[j];
    sig = sqrt(s2);
  }
  for (int t = 0; t < T; ++t) {
    const double c = A.thr[t * A.q + j];
    const bool neg = (A.side_neg >> t) & 1u;
    const double dw = neg ? c - m : m - c;
    ex_welford(A.acc + (size_t)t * 2 * n, n, i, ex_prob(dw, v, sd), A.count);
    if (A.X) {
      const double dy = neg ? c - mu : mu - c;
      ex_welford(A.acc + ((size_t)T + t) * 2 * n, n, i, ex_prob(dy, s2, sig), A.count);
    }
  }
}

// One thread per functional, over d_last: F_m and F_v (16 B), per threshold the value c (8 B) and the state (16 B read, 16 B written)
__global__ __launch_bounds__(NT) void k_exceed_fun_acc(ExceedFunArgs A) {
  const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= A.n_fun) return;
  const long long nf = A.n_fun;
  const double m = A.last[nf + f], v = A.last[2 * nf + f];
  const double sd = sqrt(v);
  for (int t = 0; t < A.n_thr; ++t) {
    const double c = A.thr[(size_t)t * nf + f];
    const double d = ((A.side_neg >> t) & 1u) ? c - m : m - c;
    ex_welford(A.acc + (size_t)t * 2 * nf, nf, f, ex_prob(d, v, sd), A.count);
  }
}

int points_exceed_launch(const ExceedArgs &A, hipStream_t st) {
  if (A.n <= 0 || A.n_thr <= 0) return 0;
  hipLaunchKernelGGL(k_exceed_acc, dim3((unsigned)((A.n + NT - 1) / NT)), dim3(NT), 0, st, A);
  return launch_rc();
}

int points_exceed_fun_launch(const ExceedFunArgs &A, hipStream_t st) {
  if (A.n_fun <= 0 || A.n_thr <= 0) return 0;
  hipLaunchKernelGGL(k_exceed_fun_acc, dim3((unsigned)((A.n_fun + NT - 1) / NT)), dim3(NT), 0, st, A);
  return launch_rc();
}
