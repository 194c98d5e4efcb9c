// Kernel translation unit of libspamtree_hip.so: the functional step of st_points_accumulate (FunArgs in points_fun.hpp, which
// has the summation order).  By its byte count bandwidth-bound: 16 B a term, read once and coalesced, plus the values it gathers
// (DESIGN.md section 18 has the model and what was measured).
#include "points_fun.hpp"

// the 64 lane sums of a wave, in one fixed order; every lane ends with the same bits
__device__ __forceinline__ double fun_butterfly(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// One wave per chunk, NT / 64 chunks per workgroup: linear chunks first, then the variance chunks.  Lane l takes the chunk's terms
// l, l + 64, ...; a linear chunk forms its three sums in one pass over the terms.
__global__ __launch_bounds__(NT) void k_fun_chunks(FunArgs A) {
  const long long c = (long long)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);   // the same for the whole wave
  if (c >= A.n_lin_chunks + A.n_var_chunks) return;
  const int lane = threadIdx.x & 63;
  if (c < A.n_lin_chunks) {
    const FunChunk C = A.lin_chunks[c];
    const FunTerm *t = A.lin + C.t0;
    double sw = 0.0, sm = 0.0, sy = 0.0;
    for (int k = lane; k < C.nt; k += 64) {
      const FunTerm T = t[k];
      sw = fma(T.c, A.w[T.src], sw);
      sm = fma(T.c, A.mean[T.src], sm);
      if (A.yhat) sy = fma(T.c, A.yhat[T.src], sy);
    }
    sw = fun_butterfly(sw); sm = fun_butterfly(sm); sy = fun_butterfly(sy);
    if (lane == 0) { A.part[4 * c] = sw; A.part[4 * c + 1] = sm; A.part[4 * c + 2] = sy; }
  } else {
    const FunChunk C = A.var_chunks[c - A.n_lin_chunks];
    const FunTerm *t = A.var + C.t0;
    double sv = 0.0;
    for (int k = lane; k < C.nt; k += 64) {
      const FunTerm T = t[k];
      sv = fma(T.c, A.vsrc[T.src], sv);
    }
    sv = fun_butterfly(sv);
    if (lane == 0) A.part[4 * c + 3] = sv;
  }
}

// One thread per functional: its chunk sums in chunk order, then the updates of k_points_acc, expression for expression
__global__ __launch_bounds__(NT) void k_fun_finish(FunArgs A) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n_fun) return;
  const long long n = A.n_fun;
  double w = 0.0, x = 0.0, y = 0.0, v = 0.0;
  for (long long c = A.lin_cptr[i]; c < A.lin_cptr[i + 1]; ++c) { w += A.part[4 * c]; x += A.part[4 * c + 1]; y += A.part[4 * c + 2]; }
  for (long long c = A.var_cptr[i]; c < A.var_cptr[i + 1]; ++c) v += A.part[4 * (A.n_lin_chunks + c) + 3];
  v = fmax(v, 0.0);
  double *acc = A.acc;
  const double m0 = acc[PA_MEAN * n + i];
  const double d = x - m0;
  const double m1 = m0 + d / A.count;
  acc[PA_MEAN * n + i] = m1;
  acc[PA_M2 * n + i] = fma(d, x - m1, acc[PA_M2 * n + i]);   // the fused multiply-add that k_points_acc's += d * (x - m1) compiles to
  acc[PA_VAR * n + i] += v;
  acc[PA_W * n + i] += w;
  if (A.keep_w) A.keep_w[i] = w;
  A.last[i] = w; A.last[n + i] = x; A.last[2 * n + i] = v;
  if (A.yhat) {
    acc[PA_YHAT * n + i] += y;
    if (A.keep_yhat) A.keep_yhat[i] = y;
    A.last[3 * n + i] = y;
  }
}

int points_fun_launch(const FunArgs &A, hipStream_t st) {
  if (A.n_fun <= 0) return 0;
  const long long nc = A.n_lin_chunks + A.n_var_chunks;
  if (nc > 0) hipLaunchKernelGGL(k_fun_chunks, dim3((unsigned)((nc + NT / 64 - 1) / (NT / 64))), dim3(NT), 0, st, A);
  hipLaunchKernelGGL(k_fun_finish, dim3((unsigned)((A.n_fun + NT - 1) / NT)), dim3(NT), 0, st, A);
  return launch_rc();
}
