// New-point prediction from a fitted state (st_points_*): the predictive of a location x* that is not a row of the problem,
// the way the model treats an NA row (make_tree's missing level + predict_std, spamtree_model.cpp:1234-1358) but without
// rebuilding the tree.  A point of margin j anchored at block b conditions on S = the reference blocks on b's path, which is
// the whole chain root .. r of ONE reference block r (r = b for a reference anchor, else b's last parent).  Slot 0 holds the
// inverse Cholesky factor of that chain as the row panels [-Ri H | Ri] of its blocks, so with k = K(S, x*):
//   v = Linv_S k,  u = Linv_S w_S,  mean = v'u,  var = max(K(x*, x*) - v'v, 0)
// V-only: unlike phase P (k_factor<., MODE_PREDICT>, k_factor_quad's leaf path) no T = H is formed.
//
//   k_points_mfma<PMAX>   chains of <= PMAX rows; one workgroup (4 waves) per tile of <= PP_NCOL points that share r.  The chain
//                         panels stream through LDS in sub-panels of <= 16 rows (LDS-DMA, double buffer); each wave keeps
//                         K(S, x*) of its 16 points in registers as the B operands of v_mfma_f64_16x16x4_f64, u of the
//                         sub-panel comes from the same staged rows, and the V tile is reduced into v'v and v'u in registers.
//   k_points_generic      any chain (and the force_generic handles): one workgroup per point, k and w_S in a global scratch
//                         slice, one wave per chain row.
// Both kernels give every point a result that depends on its chain and its own coordinates only (fixed accumulation order),
// so mean, var and a draw from a caller-supplied z do not depend on which points share a workgroup or on the input order.
#pragma once
#include "st_device.hpp"

#define PP_NT 256
#define PP_NCOL 64                 // points per workgroup of k_points_mfma: 16 per wave
#define PP_MAXB (MAXJ + 1)         // blocks in a chain
#define PP_MAXT 64                 // sub-panels of a chain of <= 256 rows: sum ceil(m_t / 16) <= 256 / 16 + PP_MAXB

struct PtChain {      // one conditioning chain: the reference block r and its ancestors, root first
  int first;          // into PointsArgs::chain_blk
  int nblk;           // blocks (0: empty conditioning set)
  int rows;           // chain rows
  int pad;
};
struct PtTile {       // a workgroup of k_points_mfma: np <= PP_NCOL consecutive points of the sorted list, one chain
  int chain, p0, np, pad;
};

struct PointsArgs {
  const Blk *blks;
  const int *chain_blk;          // device block ids of every chain, root first
  const PtChain *chains;
  const PtTile *tiles;           // k_points_mfma: this launch's tiles
  int ntiles;
  const int *gen_list;           // k_points_generic: sorted point indices
  int ngen;
  const int *pt_chain;           // per sorted point: its chain
  const long long *order;        // sorted point -> index in the caller's order
  const double *px, *py;         // new points, caller order
  const int *pmv;                // 0-based margin
  const double *cx, *cy;         // problem rows, device order
  const int *mv;
  const double *w;
  const double *panels;          // slot 0 arena
  const double *z;               // caller order; NULL: Philox stream 6
  unsigned long long seed;
  unsigned iter;
  int mode;                      // 0 draw, 1 conditional mean only
  const double *X;               // n_new x p column-major, caller order; NULL: no yhat
  const double *B;               // p x q
  const double *tsq_inv;         // q
  int p;
  long long n_new;
  double *w_new, *mean, *var, *yhat;   // caller order, any may be NULL
  double *scratch;               // k_points_generic: 2 x scratch_stride doubles per workgroup
  long long scratch_stride;
};

// launch constants and LDS of k_points_mfma<PMAX>
#define PP_LDS_STRIDE(PMAX) ((PMAX) + 8)
#define PP_LDS_BYTES(PMAX) ((size_t)(2 * 16 * PP_LDS_STRIDE(PMAX) + 4 * (PMAX)) * sizeof(double) + (size_t)(PMAX) * sizeof(int))

#ifdef ST_DEFS_PREDICT_POINTS
// the per-point outputs: mean, var, the draw and yhat (spamtree_model.cpp:1306-1326 for a one-row block; spamtree_fit.cpp:384)
__device__ __forceinline__ void pt_finish(const PointsArgs &A, long long ci, double vu, double vv, double kss) {
  const double mean = vu;
  const double var = fmax(kss - vv, 0.0);
  double w = mean;
  if (A.mode == 0) {
    const double z = A.z ? A.z[ci] : philox_normal((unsigned long long)ci, A.iter, 6u, A.seed);
    w = mean + ((var > 0.0) ? sqrt(var) : 0.0) * z;
  }
  if (A.mean) A.mean[ci] = mean;
  if (A.var) A.var[ci] = var;
  if (A.w_new) A.w_new[ci] = w;
  if (A.yhat && A.X) {
    const int j = A.pmv[ci];
    const double *bj = A.B + (size_t)A.p * j;
    double xb = 0.0;
    for (int k = 0; k < A.p; ++k) xb += A.X[(size_t)k * A.n_new + ci] * bj[k];
    const double e = (A.mode == 0) ? philox_normal((unsigned long long)ci, A.iter, 7u, A.seed) / sqrt(A.tsq_inv[j]) : 0.0;
    A.yhat[ci] = xb + w + e;
  }
}

template <int PMAX>
__global__ __launch_bounds__(PP_NT) void k_points_mfma(PointsArgs A, CovPar cp) {
  constexpr int LDS_ = PP_LDS_STRIDE(PMAX);
  constexpr int NS = PMAX / 4;                  // K-steps of a full chain
  extern __shared__ double lds[];
  double *const stage0 = lds;                   // 2 x 16 x LDS_: the double-buffered sub-panel
  double *const s_x = lds + 2 * 16 * LDS_, *const s_y = s_x + PMAX, *const s_w = s_y + PMAX, *const s_u = s_w + PMAX;
  int *const s_mv = (int *)(s_u + PMAX);
  __shared__ int s_m[PP_MAXB], s_off[PP_MAXB + 1];
  __shared__ long long s_row0[PP_MAXB], s_pan[PP_MAXB];
  __shared__ int s_tt[PP_MAXT], s_tr[PP_MAXT];  // sub-panel k: chain block, first row inside it
  __shared__ int s_nt;

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
  const PtTile T = A.tiles[blockIdx.x];
  const PtChain C = A.chains[T.chain];
  const int J = C.nblk, Ptot = C.rows;
  if (tid < J) {
    const Blk b = A.blks[A.chain_blk[C.first + tid]];
    s_m[tid] = b.m; s_row0[tid] = b.row0; s_pan[tid] = b.chain_off;
  }
  __syncthreads();
  if (tid == 0) {
    int o = 0, nt = 0;
    for (int t = 0; t < J; ++t) {
      s_off[t] = o;
      for (int r0 = 0; r0 < s_m[t]; r0 += 16) { s_tt[nt] = t; s_tr[nt] = r0; ++nt; }
      o += s_m[t];
    }
    s_off[J] = o;
    s_nt = nt;
  }
  __syncthreads();
  for (int t = 0; t < J; ++t) {
    const long long r0 = s_row0[t];
    const int o = s_off[t];
    for (int i = tid; i < s_m[t]; i += PP_NT) {
      s_x[o + i] = A.cx[r0 + i]; s_y[o + i] = A.cy[r0 + i]; s_mv[o + i] = A.mv[r0 + i]; s_w[o + i] = A.w[r0 + i];
    }
  }
  const int nt = s_nt;

  // stage sub-panel k into buffer `buf` (rows wid, wid + 4, ... of it): LDS-DMA, 2 doubles per lane
  auto issue = [&](int k, double *buf) {
    const int t = s_tt[k], r0 = s_tr[k], sr = min(16, s_m[t] - r0), Kb = s_off[t] + s_m[t];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int row = wid + 4 * rr;
      if (row < sr) {
        const double *src = A.panels + s_pan[t] + (size_t)(r0 + row) * Kb;
#pragma unroll
        for (int c = 0; c < (PMAX + 127) / 128; ++c)
          if (128 * c + 2 * lane < Kb)
            __builtin_amdgcn_global_load_lds((q_glb_void *)(src + 128 * c + 2 * lane), (q_lds_void *)(buf + (size_t)row * LDS_ + 128 * c), 16, 0, 0);
      }
    }
  };
  if (nt > 0) issue(0, stage0);
  __syncthreads();   // chain coordinates in LDS

  // this lane's point and its K(S, x*) as B operands: element (k = 4 s + l4, point l15 of the wave's 16)
  const int jl = wid * 16 + l15;
  const long long ci = A.order[T.p0 + min(jl, T.np - 1)];
  const double pxv = A.px[ci], pyv = A.py[ci];
  const int pmv = A.pmv[ci];
  double Kreg[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int k = 4 * s + l4;
    Kreg[s] = (k < Ptot) ? cov_entry(cp, s_x[k], s_y[k], s_mv[k], pxv, pyv, pmv) : 0.0;
  }

  double vv = 0.0, vu = 0.0;       // this lane's part of v'v and v'u (rows l4 + 4 r of every sub-panel)
  d4 cprev = (d4){0.0, 0.0, 0.0, 0.0};
  int prev_base = 0, prev_sr = 0;  // rows of the previous sub-panel (its epilogue waits for its u behind the next barrier)
  for (int k = 0; k < nt; ++k) {
    double *buf = stage0 + (size_t)(k & 1) * 16 * LDS_;
    const int t = s_tt[k], r0 = s_tr[k], sr = min(16, s_m[t] - r0), Kb = s_off[t] + s_m[t];
    const int base = s_off[t] + r0, Kbe = min(Kb, base + sr);   // the chain factor is lower triangular: zeros beyond Kbe
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int row = wid + 4 * rr;
      if (row < sr && lane < 4) buf[(size_t)row * LDS_ + Kb + lane] = 0.0;   // the K-step overshoot reads zeros
    }
    __syncthreads();   // sub-panel k is in LDS, sub-panel k - 1 and u of k - 1 are complete
    if (k + 1 < nt) issue(k + 1, stage0 + (size_t)((k + 1) & 1) * 16 * LDS_);
    // epilogue of sub-panel k - 1
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = l4 + 4 * r;
      if (i < prev_sr) { vv += cprev[r] * cprev[r]; vu += cprev[r] * s_u[prev_base + i]; }
    }
    // u of this sub-panel: 16 threads per row, strided over the columns, butterfly sum (identical in every lane)
    {
      const int i = tid >> 4, g = tid & 15;
      double a = 0.0;
      if (i < sr)
        for (int c = g; c < Kbe; c += 16) a += buf[(size_t)i * LDS_ + c] * s_w[c];
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) a += __shfl_xor(a, o, 16);
      if (i < sr && g == 0) s_u[base + i] = a;
    }
    // V tile = Linv[rows, 0:Kbe] K[0:Kbe, points]
    d4 c = (d4){0.0, 0.0, 0.0, 0.0};
    const double *ap = buf + (size_t)l15 * LDS_ + l4;
#pragma unroll
    for (int s = 0; s < NS; ++s)
      if (4 * s < Kbe) c = __builtin_amdgcn_mfma_f64_16x16x4f64(ap[4 * s], Kreg[s], c, 0, 0, 0);
    cprev = c; prev_base = base; prev_sr = sr;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = l4 + 4 * r;
    if (i < prev_sr) { vv += cprev[r] * cprev[r]; vu += cprev[r] * s_u[prev_base + i]; }
  }
  // the four row groups of a column, in order
  const double vv1 = __shfl(vv, l15 + 16, 64), vv2 = __shfl(vv, l15 + 32, 64), vv3 = __shfl(vv, l15 + 48, 64);
  const double vu1 = __shfl(vu, l15 + 16, 64), vu2 = __shfl(vu, l15 + 32, 64), vu3 = __shfl(vu, l15 + 48, 64);
  if (l4 == 0 && jl < T.np) {
    const double kss = cov_entry(cp, pxv, pyv, pmv, pxv, pyv, pmv);
    pt_finish(A, ci, ((vu + vu1) + vu2) + vu3, ((vv + vv1) + vv2) + vv3, kss);
  }
}

__global__ __launch_bounds__(PP_NT) void k_points_generic(PointsArgs A, CovPar cp) {
  __shared__ int s_m[PP_MAXB], s_off[PP_MAXB + 1];
  __shared__ long long s_row0[PP_MAXB], s_pan[PP_MAXB];
  __shared__ double s_vv[PP_NT / 64], s_vu[PP_NT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  double *kv = A.scratch + (size_t)blockIdx.x * 2 * A.scratch_stride, *ws = kv + A.scratch_stride;
  for (int li = blockIdx.x; li < A.ngen; li += gridDim.x) {
    const int sp = A.gen_list[li];
    const long long ci = A.order[sp];
    const PtChain C = A.chains[A.pt_chain[sp]];
    const int J = C.nblk, Ptot = C.rows;
    __syncthreads();   // the previous point is done with the metadata and the scratch slice
    if (tid < J) {
      const Blk b = A.blks[A.chain_blk[C.first + tid]];
      s_m[tid] = b.m; s_row0[tid] = b.row0; s_pan[tid] = b.chain_off;
    }
    __syncthreads();
    if (tid == 0) {
      int o = 0;
      for (int t = 0; t < J; ++t) { s_off[t] = o; o += s_m[t]; }
      s_off[J] = o;
    }
    __syncthreads();
    const double pxv = A.px[ci], pyv = A.py[ci];
    const int pmv = A.pmv[ci];
    for (int k = tid; k < Ptot; k += PP_NT) {
      int t = 0;
      while (k >= s_off[t + 1]) ++t;
      const long long r = s_row0[t] + (k - s_off[t]);
      kv[k] = cov_entry(cp, A.cx[r], A.cy[r], A.mv[r], pxv, pyv, pmv);
      ws[k] = A.w[r];
    }
    __syncthreads();
    // one wave per chain row: v_k = Linv[k, 0:k] k, u_k = Linv[k, 0:k] w_S
    double vv = 0.0, vu = 0.0;
    int t = 0;
    for (int k = wid; k < Ptot; k += PP_NT / 64) {
      while (k >= s_off[t + 1]) ++t;
      const int Kb = s_off[t + 1];
      const double *row = A.panels + s_pan[t] + (size_t)(k - s_off[t]) * Kb;
      double a = 0.0, b = 0.0;
      for (int c = lane; c <= k; c += 64) { const double l = row[c]; a += l * kv[c]; b += l * ws[c]; }
      a = wave_sum(a); b = wave_sum(b);
      vv += a * a; vu += a * b;
    }
    if (lane == 0) { s_vv[wid] = vv; s_vu[wid] = vu; }
    __syncthreads();
    if (tid == 0) {
      double tv = 0.0, tu = 0.0;
      for (int i = 0; i < PP_NT / 64; ++i) { tv += s_vv[i]; tu += s_vu[i]; }
      pt_finish(A, ci, tu, tv, cov_entry(cp, pxv, pyv, pmv, pxv, pyv, pmv));
    }
  }
}

template __global__ void k_points_mfma<128>(PointsArgs, CovPar);
template __global__ void k_points_mfma<256>(PointsArgs, CovPar);
#else   // host side: prototypes only (the kernels are compiled in k_predict.hip)
template <int PMAX> __global__ void k_points_mfma(PointsArgs A, CovPar cp);
__global__ void k_points_generic(PointsArgs A, CovPar cp);
#endif

// route codes of st_points_info (a bit set: bit code - 1 = that kernel ran in the last st_points_predict)
#define PP_ROUTE_MFMA128 1
#define PP_ROUTE_MFMA256 2
#define PP_ROUTE_GENERIC 3
#define PP_ROUTE_COUNT 4

// what st_points_predict hands the launcher: the tiles of each k_points_mfma instantiation, contiguous in `tiles`
struct PointsLaunch {
  int ntile128, ntile256;        // tiles [0, ntile128) take <128>, the next ntile256 <256>
  int grid_generic;              // workgroups of k_points_generic (0: none)
};
int points_launch(const PointsLaunch &L, const PointsArgs &A, const CovPar &cp, hipStream_t st, int *route_mask);
const char *points_route_name(int code);

// ---- per-point predictive summaries over saved iterations (st_points_accumulate; kernel and launcher in k_points_acc.hip) -----
// acc holds PA_NACC arrays of n_new doubles, caller order: the Welford mean and M2 of the conditional mean, and the running sums
// of the conditional variance, the draw w* and yhat*.  One element-wise update per saved iteration, in saved order.
#define PA_MEAN 0
#define PA_M2 1
#define PA_VAR 2
#define PA_W 3
#define PA_YHAT 4
#define PA_NACC 5
struct PointsAccArgs {
  const double *w, *mean, *var, *yhat;   // this iteration's outputs of k_points_*, caller order (yhat NULL: no regressors)
  double *acc;                           // PA_NACC x n
  double *keep_w, *keep_yhat;            // row of this draw in the [keep][n] stores, or NULL
  double count;                          // iterations accumulated including this one
  long long n;
};
int points_acc_launch(const PointsAccArgs &A, hipStream_t st);
