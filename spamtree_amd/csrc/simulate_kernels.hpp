// Prior simulation from slot 0 (st_simulate): exact draws of w ~ N(0, C_DAG) and y = XB + w + tau * eps, root to leaves.
// Slot 0 holds one row panel [N | Ri] = [-Ri H | Ri] per block (non-reference rows: [-r_j H_j | r_j]), so for every block u,
// in level order,
//   Ri w_u = z_u - N w_pa(u)          (forward substitution; Ri is lower triangular, diagonal r_j on non-reference levels)
// which is w_u = H w_pa + chol(R_u) z_u.  Only N and Ri are read: every panel once per call.
//
// Draws live on the device row-major, [row][ND] (ND = 1, 2, 4, 8 or 16 >= the call's nd, unused columns zero), so a row's
// draws are one contiguous run and the ancestor gathers and outputs coalesce.  Every draw column is computed by the same
// scalar sequence of fma / division / lane broadcasts whatever ND is (no reassociation across columns, explicit fma, no
// contraction): a draw does not depend on the batch it rode in.
//
//   k_sim_wave<MM, ND>   reference levels, blocks of <= MM rows (MM = 32, 64): one wave per block, four independent blocks per
//                        workgroup, no workgroup barrier.  Lane i owns row i.  N is staged by rows (256-byte runs) into a
//                        wave-private LDS tile of 32 columns, which lane i then walks along its row; the ancestors' w are
//                        wave-uniform loads.  Ri's row i is then held in registers and the substitution broadcasts r_j and
//                        Ri[j][j] by v_readlane: one fma per lane and column per step.
//   k_sim_leaf<ND>       non-reference levels: every row is independent given the chain, w_j = (z_j - N_j w_pa) / r_j.  One wave
//                        per row, lanes along each ancestor's segment of the row (contiguous), the sum by wave_allsum.
//   k_sim_generic<ND>    any m and P (blocks wider than 64 rows, force_generic handles): one workgroup per block, one wave per
//                        row for N w_pa, the substitution column-parallel through LDS with a barrier per pivot.
#pragma once
#include "st_device.hpp"

#define SIM_NT 256
#define SIM_TW 32                 // columns of k_sim_wave's staged tile
#define SIM_MAX_ND 16
#define SIM_NOISE_Z 8u            // Philox streams (rng.py): z of the draw, eps of the outcome
#define SIM_NOISE_EPS 9u

struct SimArgs {
  const Blk *blks;
  const int *anc_idx;
  const int *list;               // this level's device block ids
  int nlist;
  const double *panels;          // slot 0 arena
  const double *z;               // [row][ND]
  const double *eps;             // [row][ND] (used when y != NULL)
  const double *xb;              // XB of the handle's beta, device rows
  const int *mv;                 // 0-based outcome of every row
  const double *tsq_inv;         // q
  double *w;                     // [row][ND]: ancestors read, this level's rows written
  double *y;                     // [row][ND] or NULL
  const int *rowblk;             // k_sim_leaf: device block of every device row
  long long row_lo, row_hi;      // k_sim_leaf: the level's rows (contiguous in device order)
};

// LDS of the launches
#define SIM_WAVE_LDS(MM) ((size_t)4 * (MM) * (SIM_TW + 1) * sizeof(double))
#define SIM_GEN_LDS(maxM, ND) ((size_t)(maxM) * (ND) * sizeof(double))

#ifdef ST_DEFS_SIMULATE
#pragma clang fp contract(off)

// y = XB + w + sqrt(tau^2_j) eps of one row, the same in every route
template <int ND>
__device__ __forceinline__ void sim_store_row(const SimArgs &A, long long row, const double *wv) {
  double *w = A.w + row * ND;
#pragma unroll
  for (int d = 0; d < ND; ++d) w[d] = wv[d];
  if (A.y) {
    const double s = sqrt(1.0 / A.tsq_inv[A.mv[row]]), xb = A.xb[row];
    const double *e = A.eps + row * ND;
    double *y = A.y + row * ND;
#pragma unroll
    for (int d = 0; d < ND; ++d) y[d] = fma(s, e[d], xb + wv[d]);
  }
}

// the chain of block B: lane t < J holds ancestor t's first row and row count (ONE round trip for the whole chain; J <= MAXJ
// <= 64), read back wave-uniform by v_readlane inside the ancestor loops
__device__ __forceinline__ void sim_chain(const SimArgs &A, const Blk &B, int lane, long long &arow, int &am) {
  arow = 0; am = 0;
  if (lane < B.nanc) {
    const Blk Ba = A.blks[A.anc_idx[B.anc_ptr + lane]];
    arow = Ba.row0; am = Ba.m;
  }
}
__device__ __forceinline__ long long readlane_i64(long long v, int l) {
  const int lo = __builtin_amdgcn_readlane((int)(unsigned)(v & 0xffffffffll), l), hi = __builtin_amdgcn_readlane((int)(v >> 32), l);
  return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}

__global__ void k_sim_normals(double *out, const long long *dev2model, long long n, int nd, int ND, unsigned iter0,
                              unsigned stream, unsigned long long seed) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * ND) return;
  const long long i = e / ND;
  const int d = (int)(e - i * ND);
  out[e] = d < nd ? philox_normal((unsigned long long)dev2model[i], iter0 + (unsigned)d, stream, seed) : 0.0;
}

template <int MM, int ND>
__global__ __launch_bounds__(SIM_NT, 1) void k_sim_wave(SimArgs A) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = blockIdx.x * (SIM_NT / 64) + wid;
  if (li >= A.nlist) return;                      // a whole wave; no workgroup barrier below
  double *tile = lds + (size_t)wid * MM * (SIM_TW + 1);
  const Blk B = A.blks[A.list[li]];
  const int m = B.m, P = B.P, ld = B.ld, J = B.nanc;
  const double *pan = A.panels + B.panel_off;
  const bool own = lane < m;
  const long long row = B.row0 + lane;
  double r[ND];
#pragma unroll
  for (int d = 0; d < ND; ++d) r[d] = own ? A.z[row * ND + d] : 0.0;

  // r = z - N w_pa, ancestor by ancestor, 32 columns at a time; summation order: chain order
  long long arow_l;
  int am_l;
  sim_chain(A, B, lane, arow_l, am_l);
  int ao = 0;
  for (int t = 0; t < J; ++t) {
    const long long arow = readlane_i64(arow_l, t);
    const int am = __builtin_amdgcn_readlane(am_l, t);
    for (int c0 = 0; c0 < am; c0 += SIM_TW) {
      const int cw = min(SIM_TW, am - c0);
      for (int e = lane; e < m * SIM_TW; e += 64) {
        const int i = e / SIM_TW, c = e % SIM_TW;
        tile[i * (SIM_TW + 1) + c] = c < cw ? pan[(size_t)i * ld + ao + c0 + c] : 0.0;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const double *wa = A.w + (arow + c0) * ND;
      for (int c = 0; c < cw; ++c) {
        const double nic = own ? tile[lane * (SIM_TW + 1) + c] : 0.0;
#pragma unroll
        for (int d = 0; d < ND; ++d) r[d] = fma(-nic, wa[c * ND + d], r[d]);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    ao += am;
  }

  // row `lane` of Ri into registers (zero above the diagonal and beyond m), staged by rows like N
  double ri[MM];
#pragma unroll
  for (int j0 = 0; j0 < MM; j0 += SIM_TW) {
    if (j0 < m) {
      const int cw = min(SIM_TW, m - j0);
      for (int e = lane; e < m * SIM_TW; e += 64) {
        const int i = e / SIM_TW, c = e % SIM_TW;
        tile[i * (SIM_TW + 1) + c] = (c < cw && j0 + c <= i) ? pan[(size_t)i * ld + P + j0 + c] : 0.0;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
      for (int c = 0; c < SIM_TW; ++c) ri[j0 + c] = own ? tile[lane * (SIM_TW + 1) + c] : 0.0;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else {
#pragma unroll
      for (int c = 0; c < SIM_TW; ++c) ri[j0 + c] = 0.0;
    }
  }

  // forward substitution: w_j = r_j / Ri[j][j], then r_i -= Ri[i][j] w_j for every row i
  double wv[ND];
#pragma unroll
  for (int d = 0; d < ND; ++d) wv[d] = 0.0;
#pragma unroll
  for (int j = 0; j < MM; ++j) {
    if (j < m) {                                  // wave-uniform
      const double djj = readlane_f64(ri[j], j);
#pragma unroll
      for (int d = 0; d < ND; ++d) {
        const double wj = readlane_f64(r[d], j) / djj;
        r[d] = fma(-ri[j], wj, r[d]);
        wv[d] = lane == j ? wj : wv[d];
      }
    }
  }
  if (own) sim_store_row<ND>(A, row, wv);
}

template <int ND>
__global__ __launch_bounds__(SIM_NT) void k_sim_leaf(SimArgs A) {
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long row = A.row_lo + (long long)blockIdx.x * (SIM_NT / 64) + wid;
  if (row >= A.row_hi) return;
  const Blk B = A.blks[A.rowblk[row]];
  const int i = (int)(row - B.row0), P = B.P, J = B.nanc;
  const double *nrow = A.panels + B.panel_off + (size_t)i * B.ld;
  double acc[ND];
#pragma unroll
  for (int d = 0; d < ND; ++d) acc[d] = 0.0;
  long long arow_l;
  int am_l;
  sim_chain(A, B, lane, arow_l, am_l);
  int ao = 0;
  for (int t = 0; t < J; ++t) {
    const long long arow = readlane_i64(arow_l, t);
    const int am = __builtin_amdgcn_readlane(am_l, t);
    for (int c = lane; c < am; c += 64) {
      const double nv = nrow[ao + c];
      const double *wa = A.w + (arow + c) * ND;
#pragma unroll
      for (int d = 0; d < ND; ++d) acc[d] = fma(nv, wa[d], acc[d]);
    }
    ao += am;
  }
  const double rj = nrow[P];
  const double *z = A.z + row * ND;
  double wv[ND];
#pragma unroll
  for (int d = 0; d < ND; ++d) wv[d] = (z[d] - wave_allsum(acc[d])) / rj;
  if (lane == 0) sim_store_row<ND>(A, row, wv);
}

template <int ND>
__global__ __launch_bounds__(SIM_NT) void k_sim_generic(SimArgs A) {
  extern __shared__ double rr[];                    // [m][ND]: r, then w
  __shared__ int s_am[MAXJ], s_ao[MAXJ + 1];
  __shared__ long long s_arow[MAXJ];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  for (int li = blockIdx.x; li < A.nlist; li += gridDim.x) {
    const Blk B = A.blks[A.list[li]];
    const int m = B.m, P = B.P, J = B.nanc, ld = B.ld;
    const double *pan = A.panels + B.panel_off;
    __syncthreads();
    if (tid < J) {
      const Blk Ba = A.blks[A.anc_idx[B.anc_ptr + tid]];
      s_am[tid] = Ba.m;
      s_arow[tid] = Ba.row0;
    }
    __syncthreads();
    if (tid == 0) {
      int o = 0;
      for (int t = 0; t < J; ++t) { s_ao[t] = o; o += s_am[t]; }
      s_ao[J] = o;
    }
    __syncthreads();
    for (int i = wid; i < m; i += SIM_NT / 64) {
      double acc[ND];
#pragma unroll
      for (int d = 0; d < ND; ++d) acc[d] = 0.0;
      int t = 0;
      for (int k = lane; k < P; k += 64) {
        while (k >= s_ao[t + 1]) ++t;
        const double nv = pan[(size_t)i * ld + k];
        const double *wa = A.w + (s_arow[t] + k - s_ao[t]) * ND;
#pragma unroll
        for (int d = 0; d < ND; ++d) acc[d] = fma(nv, wa[d], acc[d]);
      }
      const double *z = A.z + (B.row0 + i) * ND;
#pragma unroll
      for (int d = 0; d < ND; ++d) {
        const double s = wave_allsum(acc[d]);
        if (lane == 0) rr[i * ND + d] = z[d] - s;
      }
    }
    __syncthreads();
    if (B.isref) {
      for (int j = 0; j < m; ++j) {
        if (tid < ND) rr[j * ND + tid] = rr[j * ND + tid] / pan[(size_t)j * ld + P + j];
        __syncthreads();
        for (int e = (j + 1) * ND + tid; e < m * ND; e += SIM_NT) {
          const int i = e / ND, d = e - i * ND;
          rr[e] = fma(-pan[(size_t)i * ld + P + j], rr[j * ND + d], rr[e]);
        }
        __syncthreads();
      }
    } else {
      for (int e = tid; e < m * ND; e += SIM_NT) rr[e] = rr[e] / pan[(size_t)(e / ND) * ld + P];
      __syncthreads();
    }
    for (int i = tid; i < m; i += SIM_NT) sim_store_row<ND>(A, B.row0 + i, rr + i * ND);
  }
}
#endif   // ST_DEFS_SIMULATE

// route codes of st_simulate_info (a bit set: bit code - 1 = that kernel runs on some level)
#define SIM_ROUTE_WAVE32 1
#define SIM_ROUTE_WAVE64 2
#define SIM_ROUTE_LEAF 3
#define SIM_ROUTE_GENERIC 4
#define SIM_ROUTE_COUNT 5

// one level of the sweep as the host hands it to the launcher
struct SimLevel {
  int first, count;              // into the level list (device block ids)
  int route;                     // SIM_ROUTE_*
  int maxM;
  long long row_lo, row_hi;      // the level's device rows
};
int simulate_route(bool isref, int maxM, bool force_generic);
// Launches the whole sweep, root level first, on `st` (no synchronisation); *route_mask gets bit code - 1 of each route taken.
int simulate_launch(const SimLevel *lv, int nlev, const SimArgs &A, int nd_pad, hipStream_t st, int *route_mask);
int simulate_normals(double *out, const long long *dev2model, long long n, int nd, int nd_pad, unsigned iter0, unsigned stream,
                     unsigned long long seed, hipStream_t st);
const char *simulate_route_name(int code);
