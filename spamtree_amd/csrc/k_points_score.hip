// Kernel translation unit of libspamtree_hip.so: the score step of st_points_accumulate and the CRPS of st_points_score_get
// (points_score.hpp has the definitions).  It reads d_out, d_jout, d_X, d_B and d_tsq, draws nothing and writes only the score
// state: no other step reads what it writes.
#include "points_score.hpp"
#include "misc_kernels.hpp"

// x_i'beta_j: one fused multiply-add chain k = 0..p-1 (p roundings)
__device__ __forceinline__ double sc_xb(const double *X, const double *B, long long n, int p, long long i, int j) {
  const double *bj = B + (size_t)p * j;
  double xb = 0.0;
  for (int k = 0; k < p; ++k) xb = fma(X[(size_t)k * n + i], bj[k], xb);
  return xb;
}

// One thread per point: reads y, cond_mean, cond_var, the margin and p regressors (28 + 8 p B) and the three state values (24 B),
// writes the state back (24 B).  In order: xb (p fma), mu = xb + cond_mean, e = y - mu, s2 = cond_var + 1 / tausq_inv, sigma =
// sqrt(s2), r = e / sigma, l = fma(-r / 2, r, -log sigma) + HL2PI, the (M, A) update, pit += erfc(-r / sqrt 2) / 2.
__global__ __launch_bounds__(NT) void k_score_acc(ScoreArgs A) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  const double y = A.y[i];
  if (!(y == y)) return;   // not scored
  const long long n = A.n;
  const int j = A.pmv[i];
  const double mu = sc_xb(A.X, A.B, n, A.p, i, j) + A.mean[i];
  const double s2 = A.var[i] + 1.0 / A.tsq_inv[j];
  const double sig = sqrt(s2);
  const double r = (y - mu) / sig;
  const double l = fma(-0.5 * r, r, -log(sig)) + HL2PI;
  double M = A.acc[SC_M * n + i], S = A.acc[SC_A * n + i];
  sc_lse(l, M, S);
  A.acc[SC_M * n + i] = M;
  A.acc[SC_A * n + i] = S;
  if (r == r) A.acc[SC_PIT * n + i] += 0.5 * erfc(-r * 0.70710678118654752440);   // (0 / 0 at sigma = 0, y = mu: as a density of 0)
}

// Moves inside a 16-lane row for k_score_joint_acc: lane J's value to every lane of the row, and d -= (lane J's l) * l.  As 64-bit
// DPP row broadcasts (v_mov_b32_dpp row_newbcast pairs; the fused v_fmac_f64_dpp of chol_blocked.hpp) they stay in the VALU; with
// SC_JOINT_SHFL defined they are the __shfl(., J, 16) they replace, a ds_bpermute_b32 pair through the LDS crossbar each -- the same
// bits either way (profiles/micro/score_joint_ab.py builds and times both).  Every lane of a row must be active or none.
// the inline asm of fmac_bcast is not covered by the hazard recogniser: two wait states between a VALU write and a DPP read of it
#ifdef SC_JOINT_SHFL
__device__ __forceinline__ double sc_bcast(double x, int j) { return __shfl(x, j, 16); }
__device__ __forceinline__ int sc_bcast_i(int x, int j) { return __shfl(x, j, 16); }
__device__ __forceinline__ void sc_fnma(double &d, const double l, int j) { d = fma(-l, __shfl(l, j, 16), d); }
__device__ __forceinline__ void sc_dpp_settle() {}
#else
__device__ __forceinline__ void sc_dpp_settle() { asm volatile("s_nop 1" ::: "memory"); }
// j is a compile-time constant after unrolling: one case survives
#define SC_CASES(OP) OP(0) OP(1) OP(2) OP(3) OP(4) OP(5) OP(6) OP(7) OP(8) OP(9) OP(10) OP(11) OP(12) OP(13) OP(14) OP(15)
__device__ __forceinline__ double sc_bcast(double x, int j) {
  switch (j) {
#define SC_OP(J_) case J_: return dpp_mov_f64<0x150 + J_, 0xf>(x, x);
    SC_CASES(SC_OP)
#undef SC_OP
  }
  return x;
}
__device__ __forceinline__ int sc_bcast_i(int x, int j) {
  switch (j) {
#define SC_OP(J_) case J_: return __builtin_amdgcn_update_dpp(x, x, 0x150 + J_, 0xf, 0xf, false);
    SC_CASES(SC_OP)
#undef SC_OP
  }
  return x;
}
__device__ __forceinline__ void sc_fnma(double &d, const double l, int j) {
  switch (j) {
#define SC_OP(J_) case J_: fmac_bcast<J_>(d, l, -l); break;
    SC_CASES(SC_OP)
#undef SC_OP
  }
}
#endif

// 16 lanes per joint group, four groups per wave.  The observed members are compacted in member order (lane a takes the a-th
// observed member), lane a holds row a of Sigma_oo + diag tau2 in registers (columns 0..a; lanes beyond g_o hold a unit row, which
// the elimination passes through exactly) and its residual e_a = y - (xb + cond_mean).  Right-looking Cholesky, column c = 0..GM-1
// unrolled: the pivot, the residual and the column travel by the row moves above; L_cc = sqrt(pivot), L_ac = row_a[c] / L_cc,
// z_c = e_c / L_cc, e_a = fma(-L_ac, z_c, e_a) for a > c, row_a[b] = fma(-L_ac, L_bc, row_a[b]) for c < b <= a (the instruction runs
// for the whole wave whatever a lane needs, so it is not predicated: a lane's entries b > a are never read), and, the same in
// every lane, q = fma(z_c, z_c, q), ld += log L_cc.  l = fma(g_o, HL2PI, fma(-1/2, q, -ld)).  Nothing depends on GM beyond the
// unit rows, nor on the other groups of the wave.
template <int GM>
__global__ __launch_bounds__(NT) void k_score_joint_acc(ScoreJointArgs A) {
  const int tid = threadIdx.x, a = tid & 15, row = (tid & 63) >> 4;
  const long long k = (long long)blockIdx.x * SC_GROUPS_PER_WG + (tid >> 4);
  if (k >= A.n_joint) return;   // the whole 16-lane row leaves
  const PtJoint G = A.groups[k];
  const int g = G.g;
  const bool obs = a < g && A.y[A.members[G.first + min(a, g - 1)]] == A.y[A.members[G.first + min(a, g - 1)]];
  const unsigned rm = (unsigned)(__ballot(obs) >> (16 * row)) & 0xffffu;
  const int go = __popc(rm);
  if (go == 0) return;
  int src = 0, cnt = 0;         // member behind compact index a: the a-th set bit
#pragma unroll
  for (int b = 0; b < GM; ++b)
    if ((rm >> b) & 1u) { if (cnt == a) src = b; ++cnt; }
  const bool act = a < go;
  const long long cs = A.members[G.first + src];
  const int j = A.pmv[cs];
  const double mu = sc_xb(A.X, A.B, A.n, A.p, cs, j) + A.mean[cs];
  double e = act ? A.y[cs] - mu : 0.0;
  const double tau2 = 1.0 / A.tsq_inv[j];
  const double *S = A.cov + G.cov_off;
  double rw[GM];
#pragma unroll
  for (int b = 0; b < GM; ++b) {
    const int sb = sc_bcast_i(src, b);
    double v = 0.0;
    if (act && b < a) v = S[src + (size_t)sb * g];
    if (b == a) v = act ? S[src + (size_t)src * g] + tau2 : 1.0;
    rw[b] = v;
  }
  double q = 0.0, ld = 0.0;
  bool bad = false;
#pragma unroll
  for (int c = 0; c < GM; ++c) {
    sc_dpp_settle();            // rw[c] may come from the previous column's fused multiply-adds
    const double piv = sc_bcast(rw[c], c);
    const bool ok = piv > 0.0;
    bad |= !ok;
    const double lcc = ok ? sqrt(piv) : 1.0;
    const double lac = (a > c) ? rw[c] / lcc : 0.0;
    const double zc = sc_bcast(e, c) / lcc;
    q = fma(zc, zc, q);
    ld += log(lcc);
    e = fma(-lac, zc, e);
    sc_dpp_settle();            // lac is read through DPP next
#pragma unroll
    for (int b = c + 1; b < GM; ++b) sc_fnma(rw[b], lac, b);
  }
  if (a != 0) return;
  if (bad) { atomicAdd(A.n_degenerate, 1ull); return; }
  const double l = fma((double)go, HL2PI, fma(-0.5, q, -ld));
  double M = A.jacc[2 * k], Sa = A.jacc[2 * k + 1];
  sc_lse(l, M, Sa);
  A.jacc[2 * k] = M;
  A.jacc[2 * k + 1] = Sa;
}

// A workgroup takes R points: d = yhat* - y of their stored draws into R LDS rows (padded to Kpad with +inf), series_tile.hpp's sort, then
// one wave per row: lane l adds the terms k = l, l + 64, ... in ascending order -- s1 += |d_(k)|, s2 = fma(2 k - K - 1, d_(k), s2)
// -- the 64 lane sums go through a six-level xor butterfly, and crps = s1 / K - s2 / K^2.
__global__ __launch_bounds__(NT) void k_score_crps(ScoreCrpsArgs A) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, R = A.R, K = A.Kpad;
  const long long row0 = (long long)blockIdx.x * R;
  const int nr = (int)(A.n - row0 < R ? A.n - row0 : R);
  tile_stage(lds, R, K, K, A.keep, nr, tid, NT, [&](int d, int r) {
    const double y = A.y[row0 + r];
    return y == y ? A.draws[(size_t)d * A.n + row0 + r] - y : __builtin_inf();
  });
  __syncthreads();
  tile_sort_rows(lds, R, K, tid, NT);
  for (int r = wid; r < R; r += NT / 64) {
    if (row0 + r >= A.n) break;
    const double *a = lds + (size_t)r * K;
    double s1 = 0.0, s2 = 0.0;
    for (int k = lane; k < A.keep; k += 64) {
      const double d = a[k];
      s1 += fabs(d);
      s2 = fma((double)(2 * (k + 1) - A.keep - 1), d, s2);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s1 += __shfl_xor(s1, o, 64); s2 += __shfl_xor(s2, o, 64); }
    if (lane == 0) {
      const double y = A.y[row0 + r], Kd = (double)A.keep;
      A.out[row0 + r] = (y == y) ? s1 / Kd - s2 / (Kd * Kd) : __builtin_nan("");
    }
  }
}

int points_score_launch(const ScoreArgs &A, hipStream_t st) {
  if (A.n <= 0) return 0;
  hipLaunchKernelGGL(k_score_acc, dim3((unsigned)((A.n + NT - 1) / NT)), dim3(NT), 0, st, A);
  return launch_rc();
}

int points_score_joint_launch(const ScoreJointArgs &A, int gmax, hipStream_t st) {
  if (A.n_joint <= 0) return 0;
  const dim3 grid((unsigned)((A.n_joint + SC_GROUPS_PER_WG - 1) / SC_GROUPS_PER_WG));
  if (gmax <= 4) hipLaunchKernelGGL(k_score_joint_acc<4>, grid, dim3(NT), 0, st, A);
  else if (gmax <= 8) hipLaunchKernelGGL(k_score_joint_acc<8>, grid, dim3(NT), 0, st, A);
  else hipLaunchKernelGGL(k_score_joint_acc<16>, grid, dim3(NT), 0, st, A);
  return launch_rc();
}

int points_score_crps_launch(const ScoreCrpsArgs &A, size_t lds_limit, hipStream_t st) {
  if (A.n <= 0) return 0;
  (void)hipFuncSetAttribute((const void *)k_score_crps, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_limit);
  hipLaunchKernelGGL(k_score_crps, dim3((unsigned)((A.n + A.R - 1) / A.R)), dim3(NT), (size_t)A.R * A.Kpad * sizeof(double), st, A);
  return launch_rc();
}
