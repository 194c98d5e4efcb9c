// st_sweep.hip -- phase B (the Gibbs sweep of w, level by level from the leaves up) and phase C (the log-density of w) with their
// launch sites and route codes, and the one-GPU forms of the sweep's entry points: st_sample_w, st_loglik_w, the fused
// st_sample_w_loglik and its _begin / _end.  With a communicator attached the entry points hand over to st_shard.hip.
#include "st_handle.hpp"
#include "st_routes.hpp"
#include "misc_kernels.hpp"

int gen_or_upload_z(st_handle h, const double *z, uint64_t seed, uint32_t iter, unsigned stream_id, double *dst) {
  if (z) return upload_rows(h, z, dst);
  {
    ProfScope ps(h, 5);
    const int grid = (int)((h->n_all + NT - 1) / NT);
    hipLaunchKernelGGL(k_normals, dim3(grid), dim3(NT), 0, h->stream, dst, h->d_dev2model.p, h->n_all, iter, stream_id,
                       (unsigned long long)seed);
  }
  HCHK(h, hipGetLastError());
  return ST_OK;
}

static int sample_launch(st_handle h, int g_hi, int g_lo) {   // levels g_hi-1 ... g_lo
  const int phys = h->slot_map[0];
  const int do_gram = (h->gram_valid && h->cache_gram) ? 0 : 1;
  // what the three argument structures of the level kernels name alike; `sweep`: what the two of the sweep kernels add to it
  auto common = [&](auto &S) {
    S.blks = h->d_blks.p; S.anc_idx = h->d_anc.p; S.dch_idx = h->d_dch.p; S.panels = h->d_panels[phys].p; S.acc = h->d_acc.p;
    S.no_fwd = h->limited ? 1 : 0;
  };
  auto sweep = [&](auto &S) {
    common(S);
    S.w = h->d_w.p; S.y = h->d_y.p; S.xb = h->d_xb.p; S.z = h->d_z.p; S.mv = h->d_mv.p; S.errflag = h->d_err.p; S.do_gram = do_gram;
    for (int j = 0; j < QMAX; ++j) S.tausq_inv[j] = h->tausq_inv[j];
  };
  for (int g = g_hi - 1; g >= g_lo; --g) {
    const LevelInfo &L = h->levels[g];
    int *route = h->route_b.data() + 2 * (size_t)g;   // [0]: the Gram kernel, [1]: the sweep kernel
    route[0] = route[1] = R_NONE;
    if ((L.fast ? L.gown_n : L.own_n) == 0) continue;
    SampleArgs A;
    std::memset(&A, 0, sizeof(A));
    sweep(A);
    A.list = h->d_lvl.p + L.first + L.own_lo; A.nlist = L.own_n; A.obs = h->d_obs.p; A.maxP = L.maxP; A.maxM = L.maxM; A.maxLd = L.maxLd;
    A.lds_sq = (L.big_sample && L.sample_sq) ? 2 : 0;
    A.s0 = h->d_s0.p; A.s0off = h->d_s0off.p;
    {
      ProfScope ps(h, 1, h->n_actual_groups + g);   // per-level slots of phase B follow those of phase A
      if (L.fast) {
        SampleFastArgs F;
        std::memset(&F, 0, sizeof(F));
        sweep(F);
        F.grps = h->d_grps.p + L.grp_first + L.gown_lo; F.ngrp = L.gown_n;
        F.ldN = L.ldN; F.Mr4 = L.Mr4; F.Mrows = L.Mrows; F.maxP = L.maxP; F.av_dbl = L.av_dbl;
        F.gdesc = h->d_gdesc.p + (size_t)(L.grp_first + L.gown_lo) * h->gd_stride; F.gd_stride = h->gd_stride;
        const bool lean_ok = h->sw.sample_lean && !(!L.isref && L.maxP > 255);
        F.gdesc_all = h->d_gdesc.p;
        // does level `gq` take k_gram + the lean kernels on a rebuild sweep?  (the same test for the level itself, below)
        auto splits = [&](int gq) {
          const LevelInfo &Lq = h->levels[gq];
          const bool lean_q = h->sw.sample_lean && !(!Lq.isref && Lq.maxP > 255);
          return Lq.fast && lean_q && h->sw.split_gram && (h->sw.split_gram == 2 || (Lq.isref && Lq.gown_n >= 32 * h->sm_count));
        };
        // the leaf level of a rebuild sweep writes NO Gram parts when its parents form them from the leaf panels (k_gram_direct)
        const bool direct_parent = F.do_gram && h->gram_direct_level == g && splits(g) && h->levels[g + 1].gown_n > 0;
        if (F.do_gram && lean_ok && g == h->gram_direct_level + 1 && h->gram_direct_level >= 0 && splits(g - 1) && h->levels[g - 1].gown_n > 0) F.do_gram = 0;
        // the theta-only Gram parts on their own (k_gram), then the lean sweep kernels: pays on big reference levels (n = 1e6,
        // level 7: 0.84 -> 0.72 ms averaged over a run's sweeps), loses on leaf levels and on smaller reference levels, where
        // the staged Gram of k_sample_mfma is cheaper (SPAMTREE_SPLIT_GRAM=2: every level; records identical either way)
        if (F.do_gram && lean_ok && h->sw.split_gram && (h->sw.split_gram == 2 || (L.isref && L.gown_n >= 32 * h->sm_count))) {
          if (direct_parent) { route[0] = R_GRAM_DIRECT; hipLaunchKernelGGL(k_gram_direct, dim3(L.gown_n), dim3(NT), 0, h->stream, F); }
          else { route[0] = R_GRAM; hipLaunchKernelGGL(k_gram, dim3(L.gown_n), dim3(NT), 0, h->stream, F); }
          F.do_gram = 0;
        }
        // reference levels on the lean kernels: the theta-only part of the posterior precision (Ri' Ri + the children's Gram parts)
        // is stored by the first such sweep after the records were rebuilt and loaded by the following ones (same bits either way)
        if (!(F.do_gram || !lean_ok) && L.isref) {
          F.s0 = h->d_s0.p; F.s0off = h->d_s0off.p;
          F.s0_mode = !h->cache_gram ? 0 : (h->s0_valid[g] ? 2 : 1);
          if (h->cache_gram) h->s0_valid[g] = 1;
        }
        if (F.do_gram || !lean_ok) { route[1] = R_SAMPLE_MFMA; hipLaunchKernelGGL(k_sample_mfma, dim3(L.gown_n), dim3(NT), L.lds_sfast, h->stream, F); }
        else if (!L.isref) {
          // segment-aligned lanes where the level's chains have at most 12 ancestors of at most 32 rows (SPAMTREE_LEAF_SEG=0: the
          // column-aligned kernel)
          const int need = (L.maxJ + 1) / 2;
          if (h->sw.leaf_seg && need <= 4 && L.maxMa <= 32) { route[1] = R_LEAF_SEG4; hipLaunchKernelGGL((k_sample_leaf_seg<4>), dim3(L.gown_n), dim3(NT), ((size_t)4 * 64 * 4 + 3 * 32) * 8, h->stream, F); }
          else if (h->sw.leaf_seg && need <= 6 && L.maxMa <= 32) { route[1] = R_LEAF_SEG6; hipLaunchKernelGGL((k_sample_leaf_seg<6>), dim3(L.gown_n), dim3(NT), ((size_t)4 * 64 * 6 + 3 * 32) * 8, h->stream, F); }
          else { route[1] = R_SAMPLE_LEAF; hipLaunchKernelGGL(k_sample_leaf, dim3(L.gown_n), dim3(NT), ((size_t)L.maxP + 32 + 4 * 256 + 3 * 32) * 8, h->stream, F); }
        }
        else if (h->sw.sample_wave && L.maxM <= 27 && (h->sw.sample_wave == 2 || L.gown_n >= 8 * h->sm_count)) {   // one block per wave: faster on a level
          // that keeps every CU busy for several rounds (n = 1e6 after the row-wise panel pass: level 7 0.44 -> 0.35 ms, level 6 -- 4096 blocks --
          // 0.151 -> 0.117), a wash at 1024 blocks (0.050 -> 0.046 there, 0.034 -> 0.039 at config #5), slower on latency-bound small levels (256 blocks: 0.029 -> 0.040): gd | wv | seg | tv, ev | Ri, per wave
          const size_t per = (((size_t)h->gd_stride + L.maxP + 32 + L.av_dbl + 64 + (size_t)std::max(L.maxM, 1) * CH_LD + 1) & ~(size_t)1);
          F.ldN = (int)per; F.Mrows = L.maxM;
          route[1] = R_SAMPLE_WAVE;
          hipLaunchKernelGGL(k_sample_wave, dim3((L.gown_n + NT / 64 - 1) / (NT / 64)), dim3(NT), per * 8 * (NT / 64), h->stream, F);
        } else {
          // levels that do not fill the chip (fewer groups than 2 x CUs x the five workgroups the occupancy variant fits): the
          // latency variant -- every descriptor-only load of a block in one round trip (SPAMTREE_SAMPLE_LAT=0: never; identical draws)
          F.av_dbl = L.av_dbl + 224;
          if (h->sw.sample_lat && L.gown_n <= 2 * h->sm_count) { route[1] = R_SAMPLE_LEAN_LAT; hipLaunchKernelGGL((k_sample_lean<true>), dim3(L.gown_n), dim3(NT), L.lds_slean, h->stream, F); }
          else { route[1] = R_SAMPLE_LEAN; hipLaunchKernelGGL((k_sample_lean<false>), dim3(L.gown_n), dim3(NT), L.lds_slean, h->stream, F); }
        }
      } else {
        if (A.do_gram && L.big_sample && h->sw.gram_big) {
          // the theta-only parts first, on the matrix cores (k_gram_big); the sweep kernel then takes its cached branch
          GramBigArgs Gb;
          std::memset(&Gb, 0, sizeof(Gb));
          common(Gb);
          Gb.list = A.list; Gb.nlist = A.nlist; Gb.s0 = A.s0; Gb.s0off = A.s0off;
          // both triangles unless every level of the tree is read by k_gram_big / the generic sweep's cached branch (tiles it >= jt /
          // the lower triangle only)
          bool all_big = true;
          for (const auto &L2 : h->levels) all_big = all_big && (L2.count == 0 || L2.big_sample);
          Gb.mirror = all_big ? 0 : 1;
          route[0] = R_GRAM_BIG;
          hipLaunchKernelGGL(k_gram_big, dim3(A.nlist), dim3(NT), 0, h->stream, Gb);
          A.do_gram = 0;
        }
        if (L.big_sample) {
          A.scratch = h->d_scratch.p; A.scratch_stride = h->scratch_stride;
          if (L.isref) { route[1] = R_SAMPLE_BIG_REF; hipLaunchKernelGGL((k_sample<true, false>), dim3(std::min(L.own_n, h->scratch_wgs)), dim3(NT), L.lds_sample, h->stream, A); }
          else if (h->sw.leaf_wide && !A.do_gram && L.maxM <= 64 && L.maxMa <= 96 && L.maxJ <= 8) {   // one coalesced pass, segment-aligned lanes
            route[1] = R_SAMPLE_LEAF_WIDE;
            hipLaunchKernelGGL(k_sample_leaf_wide, dim3(std::min(L.own_n, 16 * h->sm_count)), dim3(NT), ((size_t)4 * 64 * 12 + 3 * 64) * 8, h->stream, A);
          } else { route[1] = R_SAMPLE_BIG_LEAF; hipLaunchKernelGGL((k_sample<true, true>), dim3(std::min(L.own_n, h->scratch_wgs)), dim3(NT), L.lds_sample, h->stream, A); }
        } else {
          route[1] = R_SAMPLE_SMALL;
          hipLaunchKernelGGL((k_sample<false>), dim3(L.own_n), dim3(NT), L.lds_sample, h->stream, A);
        }
      }
    }
    HCHK(h, hipGetLastError());
  }
  return ST_OK;
}

// levels below the cut (this rank's subtrees); then the cut level's message records of the other ranks are zeroed so
// that an all-reduce(sum) over st_mg_top_region() completes them
extern "C" int st_sample_w_local(st_handle h, const double *z, uint64_t seed, uint32_t iter) {
  if (!h) return ST_ERR_USAGE;
  invalidate_stats(h);
  HCHK(h, hipSetDevice(h->device));
  int rc = gen_or_upload_z(h, z, seed, iter, 0u, h->d_z.p);
  if (rc) return rc;
  h->z_valid = true;
  rc = reset_err(h);
  if (rc) return rc;
  rc = sample_launch(h, h->n_actual_groups, std::min(h->cut, h->n_actual_groups));
  if (rc) return rc;
  for (auto &zr : h->top_zero) HCHK(h, hipMemsetAsync(h->d_acc.p + zr.first, 0, (size_t)zr.second * sizeof(double), h->stream));
  return ST_OK;
}
extern "C" int st_sample_w_top(st_handle h) {   // the replicated levels above the cut
  if (!h) return ST_ERR_USAGE;
  invalidate_stats(h);
  HCHK(h, hipSetDevice(h->device));
  const int rc = sample_launch(h, std::min(h->cut, h->n_actual_groups), 0);
  if (rc == ST_OK) h->gram_valid = true;   // every record now carries the Gram sums of the accepted theta
  return rc;
}
extern "C" int st_sample_w(st_handle h, const double *z, uint64_t seed, uint32_t iter) {
  if (!h) return ST_ERR_USAGE;
  if (const int rc = refuse_factor_open(h, "st_sample_w")) return rc;
  if (const int rc = refuse_sweep_pending(h, "st_sample_w")) return rc;
  if (uses_exchange(h)) return shard_sample_w(h, z, seed, iter);
  int rc = st_sample_w_local(h, z, seed, iter);
  if (rc) return rc;
  rc = st_sample_w_top(h);
  if (rc) return rc;
  Landing res;
  rc = enqueue_fail_word(h, &res);
  if (rc) return rc;
  HCHK(h, hipStreamSynchronize(h->stream));
  return landing_code(res, nullptr);  // 10 / 11: the reference stops with "Error at gibbs_sample_w" (:1215-1217)
}

// k_loglik's arguments for the blocks of `list` in the arena `phys`, sized by the levels [0, n_levels): phase C below, and the top
// blocks' components redone with the current w (st_factor.hip, fix_top_comps: with `resid`)
void loglik_args(st_handle h, int phys, int n_levels, const int *list, int nlist, double *resid, LoglikArgs *A) {
  int maxP = 0, maxM = 0;
  for (int g = 0; g < n_levels; ++g) { maxP = std::max(maxP, h->levels[g].maxP); maxM = std::max(maxM, h->levels[g].maxM); }
  A->blks = h->d_blks.p; A->anc_idx = h->d_anc.p; A->list = list; A->nlist = nlist;
  A->panels = h->d_panels[phys].p; A->w = h->d_w.p; A->loglik_c = h->d_loglik[phys].p; A->resid = resid; A->maxP = maxP; A->maxM = maxM;
}
extern "C" int st_loglik_local(st_handle h, int slot) {
  if (!h || slot < 0 || slot > 1) return ST_ERR_USAGE;
  HCHK(h, hipSetDevice(h->device));
  if (slot == 1) { const int rc0 = settle_top(h); if (rc0) return rc0; }
  { const int rc0 = complete_leaf(h, slot); if (rc0) return rc0; }
  const int phys = h->slot_map[slot];
  LoglikArgs A;
  loglik_args(h, phys, (int)h->levels.size(), h->d_ownslow.p, (int)h->own_obs_slow.size(), nullptr, &A);
  const int maxP = A.maxP;
  const size_t lds = lds_loglik_bytes(A.maxP, A.maxM);
  {
    ProfScope ps(h, 2);
    if (A.nlist > 0) hipLaunchKernelGGL(k_loglik, dim3(A.nlist), dim3(NT), lds, h->stream, A);
    if (!h->own_grp_list.empty()) {
      LoglikGrpArgs Gr;
      Gr.blks = h->d_blks.p; Gr.anc_idx = h->d_anc.p; Gr.grps = h->d_grps.p; Gr.list = h->d_owngrp.p; Gr.nlist = (int)h->own_grp_list.size();
      Gr.panels = h->d_panels[phys].p; Gr.w = h->d_w.p; Gr.loglik_c = h->d_loglik[phys].p; Gr.maxP = maxP;
      Gr.gdesc = h->d_gdesc.p; Gr.gd_stride = h->gd_stride;
      hipLaunchKernelGGL(k_loglik_grp, dim3(Gr.nlist), dim3(NT), (size_t)(maxP + 32) * sizeof(double), h->stream, Gr);
    }
  }
  HCHK(h, hipGetLastError());
  HCHK(h, reset_err(h) == ST_OK ? hipSuccess : hipErrorUnknown);
  return ST_OK;
}
extern "C" int st_loglik_w(st_handle h, int slot, double *loglik) {
  if (!h) return ST_ERR_USAGE;
  if (slot >= 0 && slot <= 1) { if (const int rc = refuse_factor_open(h, "st_loglik_w", slot)) return rc; }
  if (const int rc = refuse_sweep_pending(h, "st_loglik_w")) return rc;
  if (slot >= 0 && slot <= 1) { const int rc0 = complete_leaf(h, slot); if (rc0) return rc0; }
  if (uses_exchange(h)) return shard_loglik_w(h, slot, loglik);
  int rc = st_loglik_local(h, slot);
  if (rc) return rc;
  Landing res;
  rc = enqueue_slot_result(h, slot, &res);
  if (rc) return rc;
  HCHK(h, hipStreamSynchronize(h->stream));
  return landing_code(res, loglik);
}

// The sweep and the log-density of its w (one GPU), ENQUEUED with their read-back into dst: the sweep's failure word travels with
// the sums, so that ONE synchronisation brings both.  10 / 11: the reference stops with "Error at gibbs_sample_w" (:1215-1217).
static int enqueue_sweep_loglik(st_handle h, const double *z, uint64_t seed, uint32_t iter, int slot, Landing *dst) {
  int rc = st_sample_w_local(h, z, seed, iter);
  if (rc) return rc;
  rc = st_sample_w_top(h);
  if (rc) return rc;
  rc = enqueue_fail_word(h, dst);
  if (rc) return rc;
  rc = st_loglik_local(h, slot);   // resets the failure word after the copy above (stream order)
  if (rc) return rc;
  return enqueue_slot_result(h, slot, dst);
}

// st_sample_w followed by st_loglik_w(slot) with ONE synchronisation.
extern "C" int st_sample_w_loglik(st_handle h, const double *z, uint64_t seed, uint32_t iter, int slot, double *loglik) {
  if (!h || slot < 0 || slot > 1) return ST_ERR_USAGE;
  if (const int rc = refuse_factor_open(h, "st_sample_w_loglik")) return rc;
  if (const int rc = refuse_sweep_pending(h, "st_sample_w_loglik")) return rc;
  { const int rc0 = complete_leaf(h, slot); if (rc0) return rc0; }
  if (uses_exchange(h)) return shard_sample_w_loglik(h, z, seed, iter, slot, loglik);
  const int rc = enqueue_sweep_loglik(h, z, seed, iter, slot, &h->pin->sweep);
  if (rc) return rc;
  HCHK(h, hipStreamSynchronize(h->stream));
  return landing_code(h->pin->sweep, loglik);
}

// The same pair WITHOUT the host synchronisation: the log-density of the sweep's w is not needed on the host before the
// Metropolis step, i.e. after the proposal's factorisation -- whose own synchronisation then brings it along.  One round trip
// and one idle gap of the GPU less per iteration (the driver enqueues phase A right behind phase C).  _end returns what the
// synchronous call would have returned (failure code of the sweep / the log-density); it synchronises only if nobody has yet.
// With a communicator attached (multi-GPU) _begin simply runs the synchronous protocol and _end hands its result over.
extern "C" int st_sample_w_loglik_begin(st_handle h, const double *z, uint64_t seed, uint32_t iter, int slot) {
  if (!h || slot < 0 || slot > 1) return ST_ERR_USAGE;
  if (const int rc = refuse_factor_open(h, "st_sample_w_loglik_begin")) return rc;
  if (const int rc = refuse_sweep_pending(h, "st_sample_w_loglik_begin")) return rc;
  { const int rc0 = complete_leaf(h, slot); if (rc0) return rc0; }
  if (uses_exchange(h)) return shard_sample_w_loglik_begin(h, z, seed, iter, slot);
  const int rc = enqueue_sweep_loglik(h, z, seed, iter, slot, &h->pin->deferred);
  if (rc) return rc;
  h->c_rc = INT_MIN;   // not known yet
  h->c_pending = true;
  return ST_OK;
}
extern "C" int st_sample_w_loglik_end(st_handle h, double *loglik) {
  if (!h) return ST_ERR_USAGE;
  if (!h->c_pending) { h->err = "st_sample_w_loglik_end without st_sample_w_loglik_begin"; return ST_ERR_USAGE; }
  h->c_pending = false;
  if (h->c_rc != INT_MIN) {   // the synchronous protocol ran in _begin
    if (h->c_rc == ST_OK && loglik) *loglik = h->c_ll;
    return h->c_rc;
  }
  HCHK(h, hipStreamSynchronize(h->stream));   // returns at once when a later call (st_factor) has synchronised already
  return landing_code(h->pin->deferred, loglik);
}
