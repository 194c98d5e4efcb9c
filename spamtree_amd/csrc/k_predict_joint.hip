// Kernel translation unit of libspamtree_hip.so: the joint new-point routes of predict_joint.hpp and their launcher.  Kept apart
// from k_predict.hip so that the per-point k_points_* kernels compile exactly as they did.
#include "predict_joint.hpp"

// the outputs of one member (pt_finish of predict_points.hpp with the draw already made)
__device__ __forceinline__ void pj_write(const PointsArgs &A, long long ci, double mean, double var, double w) {
  if (A.mean) A.mean[ci] = mean;
  if (A.var) A.var[ci] = fmax(var, 0.0);
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

// One thread finishes one joint group.  S (row stride PJ_LD, LDS) holds (V'V)_ab for a >= b on entry and L on return; mx, my, mmv
// the members' coordinates and margins, mean their conditional means; wk 3 x 16 doubles of work space at stride 16: K(x_a, x_a),
// z_a and (kept for the caller) Sigma_aa.  Writes the group's blocks of cov and chol and the draws wd.
__device__ void joint_finish(const JointArgs &J, const CovPar &cp, const PtJoint G, int Prows, double *S, const double *mx,
                             const double *my, const int *mmv, const double *mean, double *wd, double *wk) {
  const PointsArgs &A = J.P;
  const int g = G.g;
  double *const kd = wk, *const zz = wk + 16, *const sd = wk + 32;
  double *const cov = J.cov ? J.cov + G.cov_off : nullptr, *const chol = J.chol ? J.chol + G.cov_off : nullptr;
  for (int a = 0; a < g; ++a)
    for (int b = 0; b <= a; ++b) {
      const double kab = cov_entry(cp, mx[a], my[a], mmv[a], mx[b], my[b], mmv[b]);
      const double s = kab - S[a * PJ_LD + b];
      S[a * PJ_LD + b] = s;
      if (a == b) { kd[a] = kab; sd[a] = s; }
      if (cov) { cov[a + (size_t)b * g] = s; cov[b + (size_t)a * g] = s; }
    }
  const double eps = (double)(Prows + g) * 0x1p-52;
  for (int i = 0; i < g; ++i)
    for (int j = 0; j <= i; ++j) {
      double s = S[i * PJ_LD + j];
      for (int k = 0; k < j; ++k) s -= S[i * PJ_LD + k] * S[j * PJ_LD + k];
      if (j < i) {
        const double ljj = S[j * PJ_LD + j];
        S[i * PJ_LD + j] = (ljj > 0.0) ? s / ljj : 0.0;
      } else {
        S[i * PJ_LD + i] = (s > eps * kd[i]) ? sqrt(s) : 0.0;
      }
    }
  if (chol)
    for (int a = 0; a < g; ++a)
      for (int b = 0; b < g; ++b) chol[a + (size_t)b * g] = (b <= a) ? S[a * PJ_LD + b] : 0.0;
  if (A.mode == 0) {
    for (int a = 0; a < g; ++a) {
      const long long ci = J.members[G.first + a];
      zz[a] = A.z ? A.z[ci] : philox_normal((unsigned long long)ci, A.iter, 6u, A.seed);
    }
    for (int a = 0; a < g; ++a) {
      double w = mean[a];
      for (int b = 0; b <= a; ++b) w += S[a * PJ_LD + b] * zz[b];
      wd[a] = w;
    }
  } else {
    for (int a = 0; a < g; ++a) wd[a] = mean[a];
  }
}

template <int PMAX>
__global__ __launch_bounds__(PP_NT) void k_points_joint_mfma(JointArgs J, CovPar cp) {
  const PointsArgs &A = J.P;
  constexpr int LDS_ = PP_LDS_STRIDE(PMAX);
  constexpr int NS = PMAX / 4;                  // K-steps of a full chain
  static_assert(4 * PJ_WAVE_LDS <= 2 * 16 * LDS_, "the epilogue reuses the staging buffers");
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
  const int J_ = C.nblk, Ptot = C.rows;
  if (tid < J_) {
    const Blk b = A.blks[A.chain_blk[C.first + tid]];
    s_m[tid] = b.m; s_row0[tid] = b.row0; s_pan[tid] = b.chain_off;
  }
  __syncthreads();
  if (tid == 0) {
    int o = 0, nt = 0;
    for (int t = 0; t < J_; ++t) {
      s_off[t] = o;
      for (int r0 = 0; r0 < s_m[t]; r0 += 16) { s_tt[nt] = t; s_tr[nt] = r0; ++nt; }
      o += s_m[t];
    }
    s_off[J_] = o;
    s_nt = nt;
  }
  __syncthreads();
  for (int t = 0; t < J_; ++t) {
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

  // this lane's column: member pc.a of group pc.grp (padding: that group's first member, nothing written)
  const PtCol pc = J.cols[(size_t)blockIdx.x * PP_NCOL + wid * 16 + l15];
  const PtJoint G = J.groups[pc.grp];
  const long long ci = J.members[G.first + max(pc.a, 0)];
  const double pxv = A.px[ci], pyv = A.py[ci];
  const int pmv = A.pmv[ci];
  double Kreg[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int k = 4 * s + l4;
    Kreg[s] = (k < Ptot) ? cov_entry(cp, s_x[k], s_y[k], s_mv[k], pxv, pyv, pmv) : 0.0;
  }

  double vu = 0.0;                 // this lane's part of v'u (rows l4 + 4 r of every sub-panel)
  d4 gram = (d4){0.0, 0.0, 0.0, 0.0};   // (V'V)[l4 + 4 r][l15] of this wave's 16 columns
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
      if (i < prev_sr) vu += cprev[r] * s_u[prev_base + i];
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
    // Gram of the slot: rows at or beyond sr came from stale staging rows and count as zero
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double v = (l4 + 4 * r < sr) ? c[r] : 0.0;
      gram = __builtin_amdgcn_mfma_f64_16x16x4f64(v, v, gram, 0, 0, 0);
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = l4 + 4 * r;
    if (i < prev_sr) vu += cprev[r] * s_u[prev_base + i];
  }
  // the four row groups of a column, in order
  const double vu1 = __shfl(vu, l15 + 16, 64), vu2 = __shfl(vu, l15 + 32, 64), vu3 = __shfl(vu, l15 + 48, 64);

  // epilogue: the staging buffers are free behind the barrier above (s_u lies beyond them)
  double *const S = stage0 + (size_t)wid * PJ_WAVE_LDS;
  double *const mx = S + 16 * PJ_LD, *const my = mx + 16, *const mean = my + 16, *const wd = mean + 16, *const wk = wd + 16;
  int *const mmv = (int *)(wk + 48);
#pragma unroll
  for (int r = 0; r < 4; ++r) S[(l4 + 4 * r) * PJ_LD + l15] = gram[r];
  if (l4 == 0) { mx[l15] = pxv; my[l15] = pyv; mmv[l15] = pmv; mean[l15] = ((vu + vu1) + vu2) + vu3; }
  __syncthreads();
  if (l4 == 0 && pc.a == 0)
    joint_finish(J, cp, G, Ptot, S + l15 * (PJ_LD + 1), mx + l15, my + l15, mmv + l15, mean + l15, wd + l15, wk + l15);
  __syncthreads();
  if (l4 == 0 && pc.a >= 0) pj_write(A, ci, mean[l15], wk[32 + l15], wd[l15]);
}

__global__ __launch_bounds__(PP_NT) void k_points_joint_generic(JointArgs J, CovPar cp) {
  const PointsArgs &A = J.P;
  __shared__ int s_m[PP_MAXB], s_off[PP_MAXB + 1];
  __shared__ long long s_row0[PP_MAXB], s_pan[PP_MAXB];
  __shared__ double S[16 * PJ_LD], mx[16], my[16], mean[16], wd[16], wk[48];
  __shared__ int mmv[16];
  __shared__ long long s_ci[16];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const long long ld = A.scratch_stride;
  double *const kv = A.scratch + (size_t)blockIdx.x * PJ_SCRATCH_COLS * ld, *const vv = kv + PJ_MAXG * ld;
  double *const ws = vv + PJ_MAXG * ld, *const us = ws + ld;
  for (int li = blockIdx.x; li < J.ngen_groups; li += gridDim.x) {
    const PtJoint G = J.groups[J.gen_groups[li]];
    const PtChain C = A.chains[G.chain];
    const int J_ = C.nblk, Ptot = C.rows, g = G.g;
    __syncthreads();   // the previous group is done with the metadata and the scratch slice
    if (tid < J_) {
      const Blk b = A.blks[A.chain_blk[C.first + tid]];
      s_m[tid] = b.m; s_row0[tid] = b.row0; s_pan[tid] = b.chain_off;
    }
    if (tid >= 64 && tid - 64 < g) {
      const int a = tid - 64;
      const long long ci = J.members[G.first + a];
      s_ci[a] = ci; mx[a] = A.px[ci]; my[a] = A.py[ci]; mmv[a] = A.pmv[ci];
    }
    __syncthreads();
    if (tid == 0) {
      int o = 0;
      for (int t = 0; t < J_; ++t) { s_off[t] = o; o += s_m[t]; }
      s_off[J_] = o;
    }
    __syncthreads();
    for (int k = tid; k < Ptot; k += PP_NT) {
      int t = 0;
      while (k >= s_off[t + 1]) ++t;
      const long long r = s_row0[t] + (k - s_off[t]);
      const double rx = A.cx[r], ry = A.cy[r];
      const int rm = A.mv[r];
      for (int a = 0; a < g; ++a) kv[a * ld + k] = cov_entry(cp, rx, ry, rm, mx[a], my[a], mmv[a]);
      ws[k] = A.w[r];
    }
    __syncthreads();
    // one wave per chain row: V[k, a] = Linv[k, 0:k] K(S, x_a), u_k = Linv[k, 0:k] w_S
    {
      int t = 0;
      for (int k = wid; k < Ptot; k += PP_NT / 64) {
        while (k >= s_off[t + 1]) ++t;
        const int Kb = s_off[t + 1];
        const double *row = A.panels + s_pan[t] + (size_t)(k - s_off[t]) * Kb;
        double b = 0.0;
        for (int c = lane; c <= k; c += 64) b += row[c] * ws[c];
        b = wave_sum(b);
        if (lane == 0) us[k] = b;
        for (int a = 0; a < g; ++a) {
          const double *ka = kv + a * ld;
          double s = 0.0;
          for (int c = lane; c <= k; c += 64) { const double l = row[c]; s += l * ka[c]; }
          s = wave_sum(s);
          if (lane == 0) vv[a * ld + k] = s;
        }
      }
    }
    __syncthreads();
    // the Gram, one thread per pair a >= b in chain-row order; the means in k_points_generic's order (a partial sum per wave)
    for (int pr = tid; pr < g * (g + 1) / 2; pr += PP_NT) {
      int a = 0;
      while ((a + 1) * (a + 2) / 2 <= pr) ++a;
      const int b = pr - a * (a + 1) / 2;
      const double *va = vv + a * ld, *vb = vv + b * ld;
      double s = 0.0;
      for (int k = 0; k < Ptot; ++k) s += va[k] * vb[k];
      S[a * PJ_LD + b] = s;
    }
    if (tid >= 192 && tid - 192 < g) {
      const int a = tid - 192;
      const double *va = vv + a * ld;
      double tu = 0.0;
      for (int wv = 0; wv < PP_NT / 64; ++wv) {
        double p = 0.0;
        for (int k = wv; k < Ptot; k += PP_NT / 64) p += va[k] * us[k];
        tu += p;
      }
      mean[a] = tu;
    }
    __syncthreads();
    if (tid == 0) joint_finish(J, cp, G, Ptot, S, mx, my, mmv, mean, wd, wk);
    __syncthreads();
    if (tid < g) pj_write(A, s_ci[tid], mean[tid], wk[32 + tid], wd[tid]);
  }
}

template __global__ void k_points_joint_mfma<128>(JointArgs, CovPar);
template __global__ void k_points_joint_mfma<256>(JointArgs, CovPar);

static const char *const k_points_joint_route_names[PP_ROUTE_JOINT_END - PP_ROUTE_JOINT_MFMA128] = {
  "k_points_joint_mfma<128>", "k_points_joint_mfma<256>", "k_points_joint_generic",
};

const char *points_joint_route_name(int code) {
  return (code >= PP_ROUTE_JOINT_MFMA128 && code < PP_ROUTE_JOINT_END) ? k_points_joint_route_names[code - PP_ROUTE_JOINT_MFMA128] : nullptr;
}

// Launches every kernel the joint set needs on `st` (no synchronisation); *route_mask gets bit code - 1 of each one launched.
int points_joint_launch(const JointLaunch &L, const JointArgs &J, const CovPar &cp, hipStream_t st, int *route_mask) {
  int mask = 0;
  if (L.ntile128 > 0) {
    JointArgs a = J;
    a.P.ntiles = L.ntile128;
    const size_t lds = PP_LDS_BYTES(128);
    (void)hipFuncSetAttribute((const void *)k_points_joint_mfma<128>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((k_points_joint_mfma<128>), dim3(L.ntile128), dim3(PP_NT), lds, st, a, cp);
    mask |= 1 << (PP_ROUTE_JOINT_MFMA128 - 1);
  }
  if (L.ntile256 > 0) {
    JointArgs a = J;
    a.P.tiles = J.P.tiles + L.ntile128;
    a.cols = J.cols + (size_t)L.ntile128 * PP_NCOL;
    a.P.ntiles = L.ntile256;
    const size_t lds = PP_LDS_BYTES(256);
    (void)hipFuncSetAttribute((const void *)k_points_joint_mfma<256>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((k_points_joint_mfma<256>), dim3(L.ntile256), dim3(PP_NT), lds, st, a, cp);
    mask |= 1 << (PP_ROUTE_JOINT_MFMA256 - 1);
  }
  if (L.grid_generic > 0 && J.ngen_groups > 0) {
    hipLaunchKernelGGL(k_points_joint_generic, dim3(L.grid_generic), dim3(PP_NT), 0, st, J, cp);
    mask |= 1 << (PP_ROUTE_JOINT_GENERIC - 1);
  }
  *route_mask |= mask;
  return launch_rc();
}

// ---- the pair summaries of st_points_accumulate on a joint set (PointsPairArgs).  They live here, not beside k_points_acc: that
// translation unit launches the per-point update alone.
// One thread per point (member a of its group) updates the pairs (a, b <= a) of that group: the running sum of Sigma_ab and the
// Welford co-moment C_ab += (x_a - m_a) (x_b - m_b'), m the mean before and m' the mean after this iteration (on the diagonal
// exactly PA_M2's update).  Reads the means k_points_acc has not yet moved: launched before it.
__global__ __launch_bounds__(NT) void k_points_pair_acc(PointsPairArgs A) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  const PtJoint G = A.groups[A.pt_grp[i]];
  const int a = A.pt_a[i], g = G.g;
  const double da = A.mean[i] - A.acc[PA_MEAN * A.n + i];
  for (int b = 0; b <= a; ++b) {
    const long long cb = A.members[G.first + b];
    const double xb = A.mean[cb], m0 = A.acc[PA_MEAN * A.n + cb];
    const double db = xb - m0;
    const double m1 = m0 + db / A.count;
    const long long e = G.cov_off + a + (long long)b * g;
    A.pacc[e] += A.cov[e];
    A.pacc[A.cov_total + e] += da * (xb - m1);
  }
}

int points_pair_acc_launch(const PointsPairArgs &A, hipStream_t st) {
  if (A.n <= 0) return 0;
  hipLaunchKernelGGL(k_points_pair_acc, dim3((unsigned)((A.n + NT - 1) / NT)), dim3(NT), 0, st, A);
  return launch_rc();
}
