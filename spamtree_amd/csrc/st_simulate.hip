// st_simulate.hip -- the C-ABI of prior simulation from slot 0 (st_simulate*); the kernels and their launcher live in k_simulate.hip
#include "st_handle.hpp"
#include "simulate_kernels.hpp"

// The state the handle points to (st_handle.hpp): the sweep's levels, their routes and row ranges (a function of the tree only: filled
// once), the draws [row][cap] on the device (allocated on first use, grown with nd) and the device block of every row (built once)
struct SimState {
  std::vector<SimLevel> levels;
  DevBuf<double> d_z, d_e, d_w, d_y;
  DevBuf<int> d_rowblk;
  int cap = 0;
};

void sim_free(st_handle_s *h) { delete h->sim; h->sim = nullptr; }   // the device buffers free themselves

static int sim_pad(int nd) { int p = 1; while (p < nd) p <<= 1; return p; }

// the handle's state with its level plan; no device call
static SimState &sim_plan(st_handle h) {
  if (h->sim) return *h->sim;
  h->sim = new SimState();
  for (int g = 0; g < h->n_actual_groups; ++g) {
    const LevelInfo &L = h->levels[g];
    SimLevel S;
    S.first = L.first; S.count = L.count; S.maxM = 0;
    S.row_lo = LLONG_MAX; S.row_hi = 0;
    for (int k = 0; k < L.count; ++k) {
      const Blk &B = h->blks[h->lvl_list[L.first + k]];
      S.maxM = std::max(S.maxM, B.m);
      S.row_lo = std::min(S.row_lo, B.row0); S.row_hi = std::max(S.row_hi, B.row0 + B.m);
    }
    if (L.count == 0) S.row_lo = 0;
    S.route = simulate_route(L.isref != 0, S.maxM, h->force_generic != 0);
    h->sim->levels.push_back(S);
  }
  return *h->sim;
}

static int sim_refuse(st_handle h, int nd) {
  if (h->world > 1) { h->err = "st_simulate: multi-GPU handles are not supported"; return ST_ERR_UNSUPPORTED; }
  if (h->n_obs != h->n_all) { h->err = "st_simulate: the tree has NA rows; build it with every row observed"; return ST_ERR_UNSUPPORTED; }
  if (nd < 1 || nd > SIM_MAX_ND) { h->err = "st_simulate: nd must be in 1..16"; return ST_ERR_USAGE; }
  if (h->theta[0].empty()) { h->err = "st_simulate before st_factor(slot 0)"; return ST_ERR_USAGE; }
  return ST_OK;
}

// caller's n_all x nd column-major (model order) -> [device row][ndp], unused columns zero
static int sim_upload(st_handle h, const double *src, int nd, int ndp, double *dst) {
  const long long n = h->n_all;
  std::vector<double> tmp((size_t)n * ndp, 0.0);
  for (long long i = 0; i < n; ++i) {
    const long long r = h->dev2model[i];
    for (int d = 0; d < nd; ++d) tmp[(size_t)i * ndp + d] = src[(size_t)d * n + r];
  }
  HCHK(h, hipMemcpyAsync(dst, tmp.data(), tmp.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HCHK(h, hipStreamSynchronize(h->stream));
  return ST_OK;
}
static int sim_download(st_handle h, const double *src, int nd, int ndp, double *dst) {
  const long long n = h->n_all;
  std::vector<double> tmp((size_t)n * ndp);
  HCHK(h, hipMemcpyAsync(tmp.data(), src, tmp.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HCHK(h, hipStreamSynchronize(h->stream));
  for (long long i = 0; i < n; ++i) {
    const long long r = h->dev2model[i];
    for (int d = 0; d < nd; ++d) dst[(size_t)d * n + r] = tmp[(size_t)i * ndp + d];
  }
  return ST_OK;
}

extern "C" int st_simulate(st_handle h, int nd, const double *z, const double *eps, uint64_t seed, uint32_t iter0, double *w_out,
                           double *y_out) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = sim_refuse(h, nd)) return rc;
  HCHK(h, hipSetDevice(h->device));
  if (const int rc = settle_top(h)) return rc;
  if (const int rc = complete_leaf(h, 0)) return rc;
  SimState &S = sim_plan(h);
  const long long n = h->n_all;
  const int ndp = sim_pad(nd);
  for (const SimLevel &V : S.levels)
    if (V.route == SIM_ROUTE_GENERIC && SIM_GEN_LDS(V.maxM, ndp) > h->lds_limit) {
      h->err = "st_simulate: a block too wide for the generic kernel's LDS";
      return ST_ERR_UNSUPPORTED;
    }
  if (ndp > S.cap) {
    S.d_z.free(); S.d_e.free(); S.d_w.free(); S.d_y.free(); S.cap = 0;   // (0: a failing allocation below leaves no buffer of the old width)
    HCHK(h, S.d_z.alloc((size_t)n * ndp)); HCHK(h, S.d_e.alloc((size_t)n * ndp));
    HCHK(h, S.d_w.alloc((size_t)n * ndp)); HCHK(h, S.d_y.alloc((size_t)n * ndp));
    S.cap = ndp;
  }
  if (!S.d_rowblk.p) {
    std::vector<int> rb(n);
    for (size_t b = 0; b < h->blks.size(); ++b)
      for (int i = 0; i < h->blks[b].m; ++i) rb[h->blks[b].row0 + i] = (int)b;
    HCHK(h, S.d_rowblk.upload(rb));
  }
  if (z) { if (const int rc = sim_upload(h, z, nd, ndp, S.d_z.p)) return rc; }
  else HCHK(h, (hipError_t)simulate_normals(S.d_z.p, h->d_dev2model.p, n, nd, ndp, iter0, SIM_NOISE_Z, seed, h->stream));
  if (y_out) {
    if (eps) { if (const int rc = sim_upload(h, eps, nd, ndp, S.d_e.p)) return rc; }
    else HCHK(h, (hipError_t)simulate_normals(S.d_e.p, h->d_dev2model.p, n, nd, ndp, iter0, SIM_NOISE_EPS, seed, h->stream));
  }
  SimArgs A;
  std::memset(&A, 0, sizeof(A));
  A.blks = h->d_blks.p; A.anc_idx = h->d_anc.p; A.list = h->d_lvl.p;
  A.panels = h->d_panels[h->slot_map[0]].p;
  A.z = S.d_z.p; A.eps = S.d_e.p; A.xb = h->d_xb.p; A.mv = h->d_mv.p; A.tsq_inv = h->d_tsq.p;
  A.w = S.d_w.p; A.y = y_out ? S.d_y.p : nullptr; A.rowblk = S.d_rowblk.p;
  int mask = 0;
  HCHK(h, (hipError_t)simulate_launch(S.levels.data(), (int)S.levels.size(), A, ndp, h->stream, &mask));
  if (w_out) { if (const int rc = sim_download(h, S.d_w.p, nd, ndp, w_out)) return rc; }
  if (y_out) { if (const int rc = sim_download(h, S.d_y.p, nd, ndp, y_out)) return rc; }
  return ST_OK;
}

extern "C" int st_simulate_info(st_handle h, int nd, int32_t *route_mask, double *alg_bytes, double *flops) {
  if (!h) return ST_ERR_USAGE;
  if (nd < 1 || nd > SIM_MAX_ND) { h->err = "st_simulate_info: nd must be in 1..16"; return ST_ERR_USAGE; }
  int mask = 0;
  double bytes = 0.0, fl = 0.0;
  for (const SimLevel &S : sim_plan(h).levels) {
    if (S.count == 0) continue;
    mask |= 1 << (S.route - 1);
    for (int k = 0; k < S.count; ++k) {
      const Blk &B = h->blks[h->lvl_list[S.first + k]];
      const double m = B.m, P = B.P, ri = B.isref ? m * (m + 1) / 2 : m;
      bytes += 8.0 * (m * P + ri);                   // the block's panel, once
      fl += 2.0 * nd * (m * P + ri);
    }
  }
  // per row: z, eps, w, y and the ancestor gathers (8 nd B each), XB (8 B)
  bytes += (double)h->n_all * (5.0 * 8.0 * nd + 8.0);
  if (route_mask) *route_mask = mask;
  if (alg_bytes) *alg_bytes = bytes;
  if (flops) *flops = fl;
  return ST_OK;
}

extern "C" const char *st_simulate_route_name(int32_t code) { return simulate_route_name(code); }
