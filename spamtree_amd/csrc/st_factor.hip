// st_factor.hip -- phase A (the factorisation of a slot's panels, level by level) and phase P (st_predict) with their launch
// sites and route codes, and the proposal protocol around phase A: the top levels ahead of time on the second stream
// (st_factor_begin, settle_top, fix_top_comps; state: the handle's AheadTop), the leaf levels' deferred half (complete_leaf),
// enqueue / finish, st_swap.  With a communicator attached the entry points hand over to st_shard.hip.
#include "st_handle.hpp"
#include "st_routes.hpp"
#include "misc_kernels.hpp"

// The instantiations of k_factor_quad, in the order of their route codes: chain rows nkx = 32 / 38 / 44 / 50 (`size` 0 .. 3), each as
// <.., true, true> (reference level, wave Cholesky), <.., true, false> (reference level) and <.., false, true> (leaf) (`kind` 0 .. 2).
typedef void (*QuadKernel)(QuadArgs, CovPar);
static QuadKernel quad_kernel(int size, int kind) {
  static const QuadKernel tab[QUAD_SIZES][QUAD_KINDS] = {
      {k_factor_quad<4, 32, 8, true, true>, k_factor_quad<4, 32, 8, true, false>, k_factor_quad<4, 32, 8, false, true>},
      {k_factor_quad<4, 38, 10, true, true>, k_factor_quad<4, 38, 10, true, false>, k_factor_quad<4, 38, 10, false, true>},
      {k_factor_quad<4, 44, 11, true, true>, k_factor_quad<4, 44, 11, true, false>, k_factor_quad<4, 44, 11, false, true>},
      {k_factor_quad<4, 50, 13, true, true>, k_factor_quad<4, 50, 13, true, false>, k_factor_quad<4, 50, 13, false, true>}};
  return tab[size][kind];
}
const void *quad_kernel_address(int size, int kind) { return (const void *)quad_kernel(size, kind); }
// One launch of k_factor_quad: `nquad` workgroups of four units; returns the route code of the instantiation it took.
static int launch_quad(int nkx, bool isref, bool wave_chol, int nquad, size_t lds, hipStream_t st, const QuadArgs &F, const CovPar &cp) {
  const int size = nkx == 32 ? 0 : nkx == 38 ? 1 : nkx == 44 ? 2 : 3, kind = isref ? (wave_chol ? 0 : 1) : 2;
  hipLaunchKernelGGL(quad_kernel(size, kind), dim3(nquad), dim3(128 * 4), lds, st, F, cp);
  return R_QUAD32_REF_WCH + QUAD_KINDS * size + kind;
}
// What every launch of k_factor_quad is given alike: `nquad` quads of the groups from grp_first, their records (qr_off < 0: none)
// of qr_words words, the arena `phys`.  The sites add their own: the component arrays, wave_chol, mode / vscr / vtiles, predict / z / w_out.
static QuadArgs quad_args(st_handle h, int grp_first, long long qr_off, int qr_words, int nquad, int ldS, int phys, int *errflag) {
  QuadArgs F;
  std::memset(&F, 0, sizeof(F));
  F.blks = h->d_blks.p; F.anc_idx = h->d_anc.p; F.grps = h->d_grps.p + grp_first;
  F.qrec = qr_off >= 0 ? h->d_qrec.p + qr_off : nullptr; F.qrec_stride = qr_words; F.nquad = nquad;
  F.cx = h->d_cx.p; F.cy = h->d_cy.p; F.mv = h->d_mv.p; F.w = h->d_w.p; F.panels = h->d_panels[phys].p;
  F.errflag = errflag; F.ldS = ldS;
  F.g_in = h->d_resid.p;   // leaf bodies (not phase P, not QM_TFROMV): the g of the chain rows, gathered like w
  return F;
}
template <bool BIG, int MODE>
static void launch_factor(st_handle h, const LevelInfo &L, FactorArgs &A, const CovPar &cp, hipStream_t st = nullptr) {
  int grid = A.nlist;
  if (BIG) {
    grid = std::min(grid, h->scratch_wgs);
    A.scratch = h->d_scratch.p; A.scratch_stride = h->scratch_stride;
  }
  hipLaunchKernelGGL((k_factor<BIG, MODE>), dim3(grid), dim3(NT), L.lds_factor, st ? st : h->stream, A, cp);
}

// CovarianceParams::transform (covariance_functions.cpp:34-75) + vec_to_symmat (:77-92)
int make_covpar(st_handle h, const double *theta, int ntheta, CovPar *cp) {
  const int q = h->q, ncb = q > 2 ? 3 : 1, npars = 3 * q + ncb, k = q * (q - 1) / 2;
  if (ntheta != npars + k) { h->err = "theta has the wrong length"; return ST_ERR_USAGE; }
  std::memset(cp, 0, sizeof(*cp));
  cp->q = q; cp->ncb = ncb;
  for (int j = 0; j < q; ++j) { cp->ai1[j] = theta[j]; cp->ai2[j] = theta[q + j]; cp->phi[j] = theta[2 * q + j]; }
  for (int j = 0; j < ncb; ++j) cp->tmv[j] = theta[3 * q + j];
  int ix = 0;
  for (int j = 0; j < q; ++j)
    for (int i = j + 1; i < q; ++i) { cp->D[i * q + j] = theta[npars + ix]; cp->D[j * q + i] = theta[npars + ix]; ++ix; }
  finish_covpar(cp);
  return ST_OK;
}

// readers of a slot's arena while st_factor_begin's launches may still be writing it on the second stream: order the
// main stream behind them (top_pending stays set: the next st_factor still picks the result up)
int settle_top(st_handle h) {
  if (h->ahead.top_pending) { HCHK(h, hipSetDevice(h->device)); HCHK(h, hipStreamWaitEvent(h->stream, h->ahead.ev_top, 0)); }
  return ST_OK;
}
// A slot whose leaf levels ran QM_VONLY gets its leaf panels here (QM_TFROMV, on the launch stream), before anything reads
// them.  The time counts as phase A: the levels' launch slots (mean per phase-A launch) and the phase bracket, no launch added.
int complete_leaf(st_handle h, int slot) {
  const int phys = h->slot_map[slot];
  if (!h->leaf_pending[phys]) return ST_OK;
  HCHK(h, hipSetDevice(h->device));
  const CovPar &cp = h->leaf_cp[phys];
  ProfScope phase(h, 0, -2, 0);
  for (int g = 0; g < h->n_actual_groups; ++g) {
    const LevelInfo &L = h->levels[g];
    if (L.vl_off < 0) continue;
    QuadArgs F = quad_args(h, L.grp_first, L.qr_off, L.qr_words, L.qown_n, L.q_ldS, phys, h->d_err.p);
    F.wave_chol = L.maxM <= 27 ? 1 : 0;
    F.mode = QM_TFROMV; F.vscr = h->d_vleaf.p + L.vl_off; F.vtiles = quad_vtiles(L.q_nkx);
    ProfScope ps(h, 0, g, 0);
    (void)launch_quad(L.q_nkx, false, true, L.qown_n, L.lds_quad, h->stream, F, cp);   // (the route stays that of the level's launch)
    HCHK(h, hipGetLastError());
  }
  h->leaf_pending[phys] = false;   // (only once every launch is in: after an error the slot still counts as unfinished)
  return ST_OK;
}
extern "C" int st_swap(st_handle h) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = refuse_factor_open(h, "st_swap")) return rc;
  if (const int rc = refuse_sweep_pending(h, "st_swap")) return rc;
  if (h->ahead.top_pending) {   // the proposal's top levels are being written into the arena that would become the accepted slot
    h->err = "st_swap between st_factor_begin and the st_factor / st_factor_local that picks its result up";
    return ST_ERR_USAGE;
  }
  { const int rc = complete_leaf(h, 1); if (rc) return rc; }   // the only way a slot becomes the sweep's
  std::swap(h->slot_map[0], h->slot_map[1]);
  std::swap(h->theta[0], h->theta[1]);
  h->gram_valid = false;
  std::fill(h->s0_valid.begin(), h->s0_valid.end(), 0);
  return ST_OK;
}

// levels [g_lo, g_hi); `st` / `errflag`: the launch stream and failure word (st_factor_begin: the second stream, d_err2)
// vonly: the deferrable leaf levels take QM_VONLY (*deferred = true when one did)
static int factor_launch(st_handle h, int phys, const CovPar &cp, int g_lo = 0, int g_hi = INT_MAX, hipStream_t st = nullptr, int *errflag = nullptr,
                         bool vonly = false, bool *deferred = nullptr) {
  g_hi = std::min(g_hi, h->n_actual_groups);
  if (!st) st = h->stream;
  if (!errflag) errflag = h->d_err.p;
  int n_launch = 0;
  for (int g = g_lo; g < g_hi; ++g) n_launch += ((h->levels[g].fast ? h->levels[g].gown_n : h->levels[g].own_n) != 0);
  ProfScope phase(h, 0, -2, n_launch, st);   // profile mode 2: the phase's launches between ONE pair of events (mean launch = total / launches)
  for (int g = g_lo; g < g_hi; ++g) std::fill_n(h->route_a.begin() + (size_t)g * ST_ROUTE_A_SLOTS, ST_ROUTE_A_SLOTS, (int)R_NONE);
  auto route = [&](int g, int code) {   // the next free phase-A slot of level g
    int *r = h->route_a.data() + (size_t)g * ST_ROUTE_A_SLOTS;
    for (int i = 0; i < ST_ROUTE_A_SLOTS; ++i) if (r[i] == R_NONE) { r[i] = code; return; }
  };
  // what the five argument structures of the level kernels name alike; `comps`: the chain and the component arrays of the
  // structures that take a level's blocks to their components in one kernel.  Each branch below sets only what is its own.
  auto common = [&](auto &S) {
    S.blks = h->d_blks.p; S.cx = h->d_cx.p; S.cy = h->d_cy.p; S.mv = h->d_mv.p; S.panels = h->d_panels[phys].p; S.errflag = errflag;
  };
  if (g_lo == 0 && h->limited && !h->twin_list.empty()) {
    MarginalArgs M;
    common(M);
    M.list = h->d_twin.p; M.nlist = (int)h->twin_list.size(); M.maxM = h->twin_maxM;
    M.w = h->d_w.p; M.resid = h->d_resid.p;   // the g of the marginal chains (the conditional residuals below are not stored)
    const size_t lds = (size_t)2 * h->twin_maxM * h->twin_maxM * sizeof(double);
    if (h->twin_maxM <= 27 && !h->force_generic) {   // one block per wave, blocked DPP / MFMA elimination
      route(0, R_MARGINAL_INVCHOL_WAVE);
      hipLaunchKernelGGL(k_marginal_invchol_wave, dim3(std::min((M.nlist + NT / 64 - 1) / (NT / 64), 8 * h->sm_count)), dim3(NT),
                         (size_t)(NT / 64) * 64 * CH_LD * sizeof(double), st, M, cp);
    } else {
      route(0, R_MARGINAL_INVCHOL);
      hipLaunchKernelGGL(k_marginal_invchol, dim3(std::min(M.nlist, 8 * h->sm_count)), dim3(NT), lds, st, M, cp);
    }
  }
  // the reference blocks' residuals, for the leaf quads below them (limited trees: their chains are marginal factors, see above)
  double *resid = h->limited ? nullptr : h->d_resid.p;
  auto comps = [&](auto &S) {
    common(S);
    S.anc_idx = h->d_anc.p; S.logdet_c = h->d_logdet[phys].p; S.loglik_c = h->d_loglik[phys].p; S.resid = resid;
  };
  for (int g = g_lo; g < g_hi; ++g) {
    const LevelInfo &L = h->levels[g];
    if ((L.fast ? L.gown_n : L.own_n) == 0) continue;
    FactorArgs A;
    std::memset(&A, 0, sizeof(A));
    comps(A);
    A.list = h->d_lvl.p + L.first + L.own_lo; A.nlist = L.own_n; A.w_in = h->d_w.p; A.w_out = nullptr; A.z = nullptr;
    A.maxP = L.maxP; A.maxM = L.maxM; A.maxMa = L.maxMa; A.SR = L.big_factor ? 4 : 8;
    {
      ProfScope ps(h, 0, g, 1, st);
      if (L.fast && h->sw.factor_gen == 3 && L.q_nkx > 0) {
        QuadArgs F = quad_args(h, L.grp_first, L.qr_off, L.qr_words, L.qown_n, L.q_ldS, phys, errflag);
        F.logdet_c = h->d_logdet[phys].p; F.loglik_c = h->d_loglik[phys].p; F.resid = resid;
        F.wave_chol = L.maxM <= 27 ? 1 : 0;
        if (!L.isref && vonly && L.vl_off >= 0) { F.mode = QM_VONLY; F.vscr = h->d_vleaf.p + L.vl_off; F.vtiles = quad_vtiles(L.q_nkx); *deferred = true; }
        route(g, launch_quad(L.q_nkx, L.isref != 0, F.wave_chol != 0, L.qown_n, L.lds_quad, st, F, cp));
      } else if (L.fast) {
        FastArgs F;
        std::memset(&F, 0, sizeof(F));
        comps(F);
        F.grps = h->d_grps.p + L.grp_first + L.gown_lo; F.ngrp = L.gown_n; F.w = h->d_w.p;
        F.Pm4 = L.Pm4; F.ldKV = L.ldKV; F.ldS = L.ldS; F.SRm = L.SRm; F.stage_dbl = L.stage_dbl;
        F.gdesc = h->d_gdesc.p + (size_t)(L.grp_first + L.gown_lo) * h->gd_stride; F.gd_stride = h->gd_stride;
        route(g, R_FACTOR_MFMA);
        hipLaunchKernelGGL(k_factor_mfma, dim3(L.gown_n), dim3(NT), L.lds_fast, st, F, cp);
      } else if (L.bigmfma && h->sw.factor_gen == 3 && L.lchain) {
        LcArgs C;
        std::memset(&C, 0, sizeof(C));
        common(C);
        C.anc_idx = h->d_anc.p; C.slabs = h->d_lcslabs.p + L.lc_first; C.nslab = L.lc_count; C.w_in = h->d_w.p;
        C.rowtmp = h->d_lcrow.p; C.n_rows = h->n_all;
        C.errcode = L.lchain_ref ? 2 : 3;
        C.vscr = L.lchain_ref ? h->d_vscr.p : nullptr;
        if (L.lchain == 96) { route(g, R_LCHAIN96); hipLaunchKernelGGL((k_factor_lchain<96>), dim3(L.lc_count), dim3(LC_NT), lc_dyn_doubles(96) * 8, st, C, cp); }
        else { route(g, R_LCHAIN136); hipLaunchKernelGGL((k_factor_lchain<136>), dim3(L.lc_count), dim3(LC_NT), lc_dyn_doubles(136) * 8, st, C, cp); }
        if (L.lchain_ref) {   // the panels hold [ -r_j T_j | r_j ] per column: finish the blocks (Schur complement, factorisation, -Ri T in place)
          A.vscr = h->d_vscr.p; A.voff = h->d_rfvoff.p + L.rf_first; A.hvrow = h->d_lcrow.p;
          route(g, R_REF_FINISH);
          hipLaunchKernelGGL(k_factor_ref_finish, dim3(std::min(A.nlist, 2 * h->sm_count)), dim3(BM_NT), L.lds_ref_finish, st, A, cp);
        } else {
          route(g, R_LCHAIN_SCALARS);
          hipLaunchKernelGGL(k_lchain_scalars, dim3((A.nlist + 255) / 256), dim3(256), 0, st, h->d_blks.p, A.list, A.nlist, h->d_lcrow.p, h->n_all,
                             h->d_logdet[phys].p, h->d_loglik[phys].p);
        }
      } else if (L.bigmfma && h->sw.factor_gen == 3 && L.wide_count > 0) {
        WideArgs W;
        std::memset(&W, 0, sizeof(W));
        comps(W);
        W.list = h->d_lvl.p + L.first + L.own_lo; W.groups = h->d_wgrps.p + L.wide_first; W.ngroups = L.wide_count; W.w_in = h->d_w.p;
        W.scratch = h->d_scratch.p; W.scratch_stride = h->scratch_stride;
        W.maxP = L.maxP; W.maxN = L.wide_maxN; W.maxM = L.maxM; W.maxMa = L.maxMa; W.ldS = L.bm_ldS;
        route(g, R_FACTOR_WIDE);
        hipLaunchKernelGGL((k_factor_wide<WG_JT>), dim3(std::min(L.wide_count, h->sm_count)), dim3(WG_NT), L.lds_wide, st, W, cp);
      } else if (L.bigmfma && h->sw.factor_gen == 3) {
        A.scratch = h->d_scratch.p; A.scratch_stride = h->scratch_stride; A.SR = L.bm_ldS;
        if (L.maxM <= 48) { route(g, R_BIGMFMA3); hipLaunchKernelGGL((k_factor_bigmfma<3, 5, 34>), dim3(std::min(A.nlist, h->sm_count)), dim3(BM_NT), L.lds_bigmfma, st, A, cp); }
        else if (L.maxM <= 64) { route(g, R_BIGMFMA4); hipLaunchKernelGGL((k_factor_bigmfma<4, 5, 34>), dim3(std::min(A.nlist, h->sm_count)), dim3(BM_NT), L.lds_bigmfma, st, A, cp); }
        else { route(g, R_BIGMFMA5); hipLaunchKernelGGL((k_factor_bigmfma<5, 3, 24>), dim3(std::min(A.nlist, h->sm_count)), dim3(BM_NT), L.lds_bigmfma, st, A, cp); }
      } else if (L.big_factor) { route(g, R_FACTOR_SCRATCH); launch_factor<true, MODE_FACTOR>(h, L, A, cp, st); }
      else { route(g, R_FACTOR_LDS); launch_factor<false, MODE_FACTOR>(h, L, A, cp, st); }
    }
    HCHK(h, hipGetLastError());
  }
  return ST_OK;
}

// Phase A of the top levels ahead of time, on the second stream: call before the sweep with the theta st_factor /
// st_factor_local will be given next for the same slot.  A no-op when the tree does not qualify (or SPAMTREE_ASYNC_TOP=0).
extern "C" int st_factor_ahead_levels(st_handle h) { return (h && h->ahead.async_top && !h->ahead.async_top_off) ? h->g_top : 0; }
// measurement: switch the ahead-of-time path off / on at run time (bench.py's per-level pass runs every level of phase A back
// to back on ONE stream; on the second stream, under the sweep, the top levels' launch times are not their own)
extern "C" int st_factor_ahead_enable(st_handle h, int enable) {
  if (!h) return ST_ERR_USAGE;
  h->ahead.async_top_off = !enable;
  return ST_OK;
}
extern "C" int st_factor_begin(st_handle h, int slot, const double *theta, int ntheta) {
  if (!h || !theta || slot < 0 || slot > 1) return ST_ERR_USAGE;
  if (const int rc = refuse_factor_open(h, "st_factor_begin")) return rc;
  if (!h->ahead.async_top || h->ahead.async_top_off) return ST_OK;
  HCHK(h, hipSetDevice(h->device));
  CovPar cp;
  int rc = make_covpar(h, theta, ntheta, &cp);
  if (rc) return rc;
  if (h->ahead.top_pending) HCHK(h, hipStreamWaitEvent(h->stream2, h->ahead.ev_top, 0));
  HCHK(h, hipEventRecord(h->ev_main, h->stream));          // everything issued so far (the previous iteration) comes first
  HCHK(h, hipStreamWaitEvent(h->stream2, h->ev_main, 0));
  const int init[2] = {INT_MAX, 0};
  HCHK(h, hipMemcpyAsync(h->ahead.d_err2.p, init, 2 * sizeof(int), hipMemcpyHostToDevice, h->stream2));
  const int phys = h->slot_map[slot];
  h->leaf_pending[phys] = false;   // the slot is being re-factorised: its deferred half is void
  h->prof_suspend = true;   // not timed: the launches overlap the sweep on another stream
  rc = factor_launch(h, phys, cp, 0, h->g_top, h->stream2, h->ahead.d_err2.p);
  h->prof_suspend = false;
  if (rc) return rc;
  HCHK(h, hipEventRecord(h->ahead.ev_top, h->stream2));
  h->ahead.top_pending = true; h->ahead.top_phys = phys; h->ahead.top_theta.assign(theta, theta + ntheta);
  return ST_OK;
}
// the quadratic forms and the residuals of the top blocks with the CURRENT w (st_factor_begin ran them with the w of the sweep's start)
static int fix_top_comps(st_handle h, int phys) {
  if (h->n_toplist == 0) return ST_OK;
  LoglikArgs A;
  loglik_args(h, phys, h->g_top, h->ahead.d_toplist.p, h->n_toplist, h->d_resid.p, &A);
  {
    ProfScope ps(h, 0, h->g_top > 0 ? h->g_top - 1 : 0);
    hipLaunchKernelGGL(k_loglik, dim3(A.nlist), dim3(NT), lds_loglik_bytes(A.maxP, A.maxM), h->stream, A);
  }
  HCHK(h, hipGetLastError());
  return ST_OK;
}
static int factor_local(st_handle h, int slot, const double *theta, int ntheta, bool vonly) {
  if (!h || !theta || slot < 0 || slot > 1) return ST_ERR_USAGE;
  HCHK(h, hipSetDevice(h->device));
  CovPar cp;
  int rc = make_covpar(h, theta, ntheta, &cp);
  if (rc) return rc;
  h->theta[slot].assign(theta, theta + ntheta);
  if (slot == 0) { h->gram_valid = false; std::fill(h->s0_valid.begin(), h->s0_valid.end(), 0); }
  rc = reset_err(h);
  if (rc) return rc;
  const int phys = h->slot_map[slot];
  h->leaf_pending[phys] = false;
  if (slot == 1) { rc = stats_begin(h); if (rc) return rc; }
  bool reuse = false;
  if (h->ahead.top_pending) {
    HCHK(h, hipStreamWaitEvent(h->stream, h->ahead.ev_top, 0));   // the top levels are done (or at least out of the way) before anything below
    reuse = h->ahead.top_phys == phys && (int)h->ahead.top_theta.size() == ntheta && std::equal(theta, theta + ntheta, h->ahead.top_theta.begin());
    h->ahead.top_pending = false;
  }
  // the top levels ran ahead of time with the w of the sweep's start: their quadratic forms AND the residuals the leaf quads
  // below gather are redone with the current w before those levels are launched (outside factor_launch's phase bracket)
  if (reuse) { rc = fix_top_comps(h, phys); if (rc) return rc; }
  bool deferred = false;
  rc = factor_launch(h, phys, cp, reuse ? h->g_top : 0, INT_MAX, nullptr, nullptr, vonly, &deferred);
  if (deferred) { h->leaf_pending[phys] = true; h->leaf_cp[phys] = cp; }
  if (rc || !reuse) return rc;
  hipLaunchKernelGGL(k_merge_err, dim3(1), dim3(64), 0, h->stream, h->d_err.p, h->ahead.d_err2.p);
  HCHK(h, hipGetLastError());
  return ST_OK;
}
extern "C" int st_factor_local(st_handle h, int slot, const double *theta, int ntheta) {
  if (h) { if (const int rc = refuse_factor_open(h, "st_factor_local")) return rc; }
  return factor_local(h, slot, theta, ntheta, false);
}

// st_factor in two halves (one GPU): everything is ENQUEUED by the first -- the levels, the two sums, the copies of the sums and of
// the failure word to pinned memory, an event behind them -- and the second waits for that event and reads them.  In between the
// host may enqueue work that does not touch the proposal's slot: the C++ driver draws tausq and beta from the sweep's statistics
// (ready early in phase A: they run on the second stream) and uploads them, so that XB is current when phase A ends instead of
// two host round trips later.  With a communicator attached the first half enqueues nothing and the second does all of st_factor.
extern "C" int st_factor_is_async(st_handle h) { return (h && !uses_exchange(h)) ? 1 : 0; }
static int factor_enqueue(st_handle h, int slot, const double *theta, int ntheta, bool vonly) {
  if (!h || !theta || slot < 0 || slot > 1) return ST_ERR_USAGE;
  if (h->factor_open) { h->err = "st_factor_enqueue: the previous one has not been finished"; return ST_ERR_USAGE; }
  if (uses_exchange(h)) return shard_factor_enqueue(h, slot, theta, ntheta);
  int rc = factor_local(h, slot, theta, ntheta, vonly);
  if (rc) return rc;
  // the failure word and the two sums come back in ONE synchronisation (the sums are meaningless after a failure)
  if ((rc = enqueue_slot_result(h, slot, &h->pin->factor)) || (rc = enqueue_fail_word(h, &h->pin->factor))) return rc;
  HCHK(h, hipEventRecord(h->ev_factor, h->stream));
  h->factor_open = true; h->factor_open_slot = slot; h->top_theta_open.clear();
  return ST_OK;
}
// the proposal's slot (1) defers its leaf levels' T (unless st_options.reserved bit 2); synchronous st_factor never does
extern "C" int st_factor_enqueue(st_handle h, int slot, const double *theta, int ntheta) {
  return factor_enqueue(h, slot, theta, ntheta, h && h->defer_leaf && slot == 1);
}
extern "C" int st_factor_finish(st_handle h, double *loglik) {
  if (!h) return ST_ERR_USAGE;
  if (!h->factor_open) { h->err = "st_factor_finish without st_factor_enqueue"; return ST_ERR_USAGE; }
  h->factor_open = false;
  if (uses_exchange(h)) return shard_factor_finish(h, loglik);
  HCHK(h, hipSetDevice(h->device));
  HCHK(h, hipEventSynchronize(h->ev_factor));
  return landing_code(h->pin->factor, loglik);   // a code: the reference's `return false` (:971-982)
}
extern "C" int st_factor(st_handle h, int slot, const double *theta, int ntheta, double *loglik) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = refuse_factor_open(h, "st_factor")) return rc;
  if (uses_exchange(h)) return shard_factor(h, slot, theta, ntheta, loglik);
  int rc = factor_enqueue(h, slot, theta, ntheta, false);
  if (rc) return rc;
  return st_factor_finish(h, loglik);
}

extern "C" int st_predict(st_handle h, int theta_changed) {
  (void)theta_changed;  // H of a prediction block is rebuilt from the ancestor chain every call: same values as the cache
  if (!h) return ST_ERR_USAGE;
  if (const int rc = refuse_factor_open(h, "st_predict")) return rc;
  if (const int rc = refuse_sweep_pending(h, "st_predict")) return rc;
  if (h->pred_list.empty()) return ST_OK;
  invalidate_stats(h);
  if (!h->z_valid) { h->err = "st_predict needs the normals of a preceding st_sample_w (spamtree_model.cpp:1325)"; return ST_ERR_USAGE; }
  if (h->theta[0].empty()) { h->err = "st_predict before st_factor(slot 0)"; return ST_ERR_USAGE; }
  HCHK(h, hipSetDevice(h->device));
  CovPar cp;
  int rc = make_covpar(h, h->theta[0].data(), (int)h->theta[0].size(), &cp);
  if (rc) return rc;
  const LevelInfo &L = h->pred_info;
  if (h->pred_nkx > 0 && h->pred_quad_count > 0) {
    // (the records exist: layout_levels appends them under this very condition)
    QuadArgs F = quad_args(h, h->pred_grp_first, h->pred_qr_off, h->pred_qr_words, h->pred_quad_count, quad_lds_stride(h->pred_nkx), h->slot_map[0], h->d_err.p);
    F.wave_chol = 1; F.predict = 1; F.z = h->d_z.p; F.w_out = h->d_w.p;
    {
      ProfScope ps(h, 6);
      h->route_p = launch_quad(h->pred_nkx, false, true, h->pred_quad_count, h->pred_lds, h->stream, F, cp);
    }
    HCHK(h, hipGetLastError());
    HCHK(h, hipStreamSynchronize(h->stream));
    return ST_OK;
  }
  FactorArgs A;
  std::memset(&A, 0, sizeof(A));
  A.blks = h->d_blks.p; A.anc_idx = h->d_anc.p; A.list = h->d_pred.p; A.nlist = (int)h->pred_list.size();
  A.cx = h->d_cx.p; A.cy = h->d_cy.p; A.mv = h->d_mv.p; A.w_in = h->d_w.p; A.w_out = h->d_w.p; A.z = h->d_z.p;
  A.panels = h->d_panels[h->slot_map[0]].p; A.logdet_c = nullptr; A.loglik_c = nullptr; A.errflag = h->d_err.p;
  A.maxP = L.maxP; A.maxM = L.maxM; A.maxMa = L.maxMa; A.SR = L.big_factor ? 4 : 8;
  {
    ProfScope ps(h, 6);
    if (L.big_factor) { h->route_p = R_PREDICT_SCRATCH; launch_factor<true, MODE_PREDICT>(h, L, A, cp); }
    else { h->route_p = R_PREDICT_LDS; launch_factor<false, MODE_PREDICT>(h, L, A, cp); }
  }
  HCHK(h, hipGetLastError());
  HCHK(h, hipStreamSynchronize(h->stream));
  return ST_OK;
}
