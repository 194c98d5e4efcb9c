// tree_layout.cpp -- see tree_layout.hpp.  Pure host arithmetic: no HIP or RCCL call, no handle.  The ORDER of the steps in
// layout_order and layout_levels is part of the behaviour (which check reports first, which flag a later step sees):
// DESIGN.md, "st_create in three steps", has the rule.
#include "tree_layout.hpp"
#include "st_protocol.hpp"

Switches read_switches() {
  auto level = [](const char *name) {   // 0 / 2 when the value starts with '0' / '2', else (unset too) 1
    const char *e = getenv(name);
    return (e && e[0] == '0') ? 0 : ((e && e[0] == '2') ? 2 : 1);
  };
  Switches s;
  s.wide = level("SPAMTREE_WIDE"); s.split_gram = level("SPAMTREE_SPLIT_GRAM"); s.sample_wave = level("SPAMTREE_SAMPLE_WAVE");
  s.lchain = level("SPAMTREE_LCHAIN"); s.lchain_ref = level("SPAMTREE_LCHAIN_REF"); s.gram_big = level("SPAMTREE_GRAM_BIG");
  s.gram_direct = level("SPAMTREE_GRAM_DIRECT"); s.sample_lean = level("SPAMTREE_SAMPLE_LEAN"); s.sample_lat = level("SPAMTREE_SAMPLE_LAT");
  s.leaf_seg = level("SPAMTREE_LEAF_SEG"); s.leaf_wide = level("SPAMTREE_LEAF_WIDE"); s.async_top = level("SPAMTREE_ASYNC_TOP");
  const char *e;
  if ((e = getenv("SPAMTREE_LCHAIN_REF_MIN"))) s.lchain_ref_min = atoi(e);
  if ((e = getenv("SPAMTREE_FACTOR_KERNEL")) && e[0] == '1') s.factor_gen = 1;
  if ((e = getenv("SPAMTREE_QUAD_UNITS"))) s.quad_units = atoi(e);
  if ((e = getenv("SPAMTREE_QUAD_MIN"))) s.quad_min = std::max(atoi(e), 0);   // (any value <= 0 lets every level through)
  return s;
}

static int refuse(std::string &msg, int code, const std::string &text) { msg = text; return code; }

static size_t lds_factor_bytes(int maxP, int maxM, int maxMa, int SR, bool big) {
  size_t dbl = (size_t)3 * (maxP + maxM) + 3 * (size_t)maxM + (size_t)SR * maxP;
  size_t bytes = dbl * 8 + (size_t)((maxP + maxM + 1) & ~1) * 4;
  if (!big) bytes += ((size_t)2 * maxP * maxM + (size_t)maxMa * maxM + (size_t)2 * maxM * maxM) * 8;
  return bytes + 64;
}
static size_t scratch_factor_doubles(int maxP, int maxM, int maxMa) {
  return (size_t)2 * maxP * maxM + (size_t)maxMa * maxM + (size_t)2 * maxM * maxM;
}
static size_t lds_sample_sq_bytes(int maxM) { return ((size_t)maxM * ((maxM + 7) | 1) + maxM + 16) * 8; }   // S (odd row stride) + the pivot column
static size_t lds_sample_bytes(int maxP, int maxM, int maxLd, bool big) {
  size_t dbl = (size_t)(maxP + maxM) + 4 * (size_t)maxM + (size_t)MAXJ * maxM;   // ... + segment sums seg[t][r]
  if (!big) dbl += (size_t)maxM * maxLd + (size_t)maxM * maxM;
  return dbl * 8 + 64;
}
// device id of a block's last ancestor (its direct parent), or `none`
static int last_parent(const TreeLayout &t, const Blk &B, int none) { return B.nanc ? t.anc_idx[B.anc_ptr + B.nanc - 1] : none; }
// row stride of a staged chain row: 2 * odd, so that the A-operand reads are conflict-free
static int stage_stride(int ldS) {
  while ((ldS & 1) || ((ldS >> 1) & 1) == 0) ++ldS;
  return ldS;
}
// k_factor_quad's instantiation for chains of up to maxP rows
static int quad_nkx(int maxP) {
  const int need = (maxP + 3) / 4;
  return need <= 32 ? 32 : (need <= 38 ? 38 : (need <= 44 ? 44 : 50));
}

// ---- layout_order
struct Census {
  std::vector<int> m_of, obs_of, grp_of, order;   // per model block: rows, observed rows, level; device position -> model block
  int G = 0, n_actual = 0;                        // levels named by block_groups / levels with observations
};

static int check_arguments(const st_problem *pb, const st_options *opt, std::string &msg) {
  if (!pb) return refuse(msg, ST_ERR_USAGE, "st_create: null argument");
  if (pb->d != 2) return refuse(msg, ST_ERR_UNSUPPORTED, "only d=2 is reachable from spamtree() (R/spamtree_fit.R:58-60)");
  if (pb->q < 1 || pb->q > QMAX) return refuse(msg, ST_ERR_UNSUPPORTED, "q out of range");
  if (pb->p < 1 || pb->p > ST_MAX_P) return refuse(msg, ST_ERR_UNSUPPORTED, "p must be in 1.." + std::to_string(ST_MAX_P) + " (ST_MAX_P)");
  if (opt && (opt->world < 1 || opt->rank < 0 || opt->rank >= opt->world || opt->world > ST_MAX_RANKS)) return refuse(msg, ST_ERR_USAGE, "bad rank/world");
  // the covariance helpers map a NaN distance to a covariance of 0 (cov_exp clamps with fmax), so a non-finite coordinate
  // would factorise silently instead of failing
  if (pb->n_all > 0 && !pb->coords) return refuse(msg, ST_ERR_USAGE, "st_create: coords is NULL");
  for (int64_t i = 0; i < 2 * pb->n_all; ++i)
    if (!std::isfinite(pb->coords[i]))
      return refuse(msg, ST_ERR_USAGE, "st_create: coordinates must be finite (row " + std::to_string(i % pb->n_all) + ")");
  return ST_OK;
}
// block census (na_study :303-313), levels (make_gibbs_groups :194-301)
static int take_census(const st_problem *pb, TreeLayout &t, Census &c, std::string &msg) {
  const long long n = t.n_all, nb = t.n_blocks;
  c.m_of.assign(nb, 0); c.obs_of.assign(nb, 0); c.grp_of.assign(nb, 0);
  std::vector<long long> labels(pb->block_groups, pb->block_groups + nb);
  std::sort(labels.begin(), labels.end());
  labels.erase(std::unique(labels.begin(), labels.end()), labels.end());
  if ((int)labels.size() > pb->n_groups) return refuse(msg, ST_ERR_TOPOLOGY, "more levels in block_groups than entries in res_is_ref");
  std::vector<char> row_seen(n, 0);
  for (long long u = 0; u < nb; ++u) {
    c.m_of[u] = (int)(pb->indexing_ptr[u + 1] - pb->indexing_ptr[u]);
    c.grp_of[u] = (int)(std::lower_bound(labels.begin(), labels.end(), pb->block_groups[u]) - labels.begin());
    for (long long k = pb->indexing_ptr[u]; k < pb->indexing_ptr[u + 1]; ++k) {
      const long long r = pb->indexing_idx[k];
      if (r < 0 || r >= n || row_seen[r]) return refuse(msg, ST_ERR_TOPOLOGY, "indexing is not a partition of the rows");
      row_seen[r] = 1;
      if (std::isfinite(pb->y[r])) c.obs_of[u]++;
    }
  }
  for (long long r = 0; r < n; ++r)
    if (!row_seen[r]) return refuse(msg, ST_ERR_TOPOLOGY, "row without a block");
  c.G = (int)labels.size();
  std::vector<int> grp_has_obs(c.G, 0);
  for (long long u = 0; u < nb; ++u)
    if (c.obs_of[u] > 0) grp_has_obs[c.grp_of[u]] = 1;
  for (int g = 0; g < c.G; ++g) c.n_actual += grp_has_obs[g];
  for (int g = 0; g < c.n_actual; ++g)
    if (!grp_has_obs[g]) return refuse(msg, ST_ERR_TOPOLOGY, "an empty level precedes an observed one");
  t.n_actual_groups = c.n_actual;
  return ST_OK;
}
// device block order: by (level, id); rows contiguous per block
static int order_blocks(const st_problem *pb, TreeLayout &t, Census &c, std::string &msg) {
  const long long n = t.n_all;
  const int nb = (int)t.n_blocks;
  c.order.resize(nb);
  std::iota(c.order.begin(), c.order.end(), 0);
  std::stable_sort(c.order.begin(), c.order.end(), [&](int a, int b) { return c.grp_of[a] < c.grp_of[b]; });
  t.blk_model2dev.assign(nb, -1);
  // inside a level, blocks with the same last parent (identical ancestor chain) are made contiguous, so a
  // workgroup can take several sibling leaf blocks as one column group
  int i0 = 0;
  while (i0 < nb) {
    int i1 = i0;
    while (i1 < nb && c.grp_of[c.order[i1]] == c.grp_of[c.order[i0]]) ++i1;
    auto key = [&](int u) -> long long {
      const long long p0 = pb->parents_ptr[u], p1 = pb->parents_ptr[u + 1];
      if (p1 == p0) return -1;
      const long long a = pb->parents_idx[p1 - 1];
      return (a >= 0 && a < nb) ? (long long)t.blk_model2dev[a] : -1;
    };
    std::stable_sort(c.order.begin() + i0, c.order.begin() + i1, [&](int a, int b) { return key(a) < key(b); });
    for (int i = i0; i < i1; ++i) t.blk_model2dev[c.order[i]] = i;
    i0 = i1;
  }
  t.dev2model.resize(n); t.model2dev.resize(n);
  t.blks.resize(nb);
  long long row = 0;
  for (int i = 0; i < nb; ++i) {
    const int u = c.order[i];
    Blk &B = t.blks[i];
    B.row0 = row; B.m = c.m_of[u]; B.level = c.grp_of[u]; B.model_id = u; B.nobs = c.obs_of[u];
    for (long long k = pb->indexing_ptr[u]; k < pb->indexing_ptr[u + 1]; ++k) {
      if (k > pb->indexing_ptr[u] && pb->indexing_idx[k] <= pb->indexing_idx[k - 1])
        return refuse(msg, ST_ERR_TOPOLOGY, "indexing(u) must be ascending");
      t.dev2model[row] = pb->indexing_idx[k];
      t.model2dev[pb->indexing_idx[k]] = row;
      ++row;
    }
  }
  return ST_OK;
}
// ancestors: chain property anc(u) = anc(last parent) + [last parent]; the panels of the observed blocks
static int link_ancestors(const st_problem *pb, TreeLayout &t, const Census &c, std::string &msg) {
  const int nb = (int)t.n_blocks;
  long long panel_total = 0;
  for (int i = 0; i < nb; ++i) {
    const int u = c.order[i];
    Blk &B = t.blks[i];
    const long long p0 = pb->parents_ptr[u], p1 = pb->parents_ptr[u + 1];
    B.nanc = (int)(p1 - p0);
    if (B.nanc > MAXJ) return refuse(msg, ST_ERR_UNSUPPORTED, "more than ST_MAX_ANCESTORS ancestors");
    B.anc_ptr = (int)t.anc_idx.size();
    int P = 0;
    for (long long k = p0; k < p1; ++k) {
      const long long a = pb->parents_idx[k];
      if (a < 0 || a >= nb) return refuse(msg, ST_ERR_TOPOLOGY, "parent id out of range");
      if (k > p0 && a <= pb->parents_idx[k - 1]) return refuse(msg, ST_ERR_TOPOLOGY, "parents(u) must be ascending");
      if (c.grp_of[a] >= c.grp_of[u]) return refuse(msg, ST_ERR_TOPOLOGY, "parent on the same or a deeper level");
      if (pb->res_is_ref[c.grp_of[a]] != 1) return refuse(msg, ST_ERR_TOPOLOGY, "parent on a non-reference level");
      if (c.obs_of[a] == 0) return refuse(msg, ST_ERR_TOPOLOGY, "ancestor block without observations");
      t.anc_idx.push_back(t.blk_model2dev[a]);
      P += c.m_of[a];
    }
    B.P = P;
    if (t.limited) {
      if (B.nanc > 1) return refuse(msg, ST_ERR_TOPOLOGY, "limited_tree: a block has more than one parent (make_edges_limited gives one)");
    } else if (B.nanc > 0) {
      const long long last = pb->parents_idx[p1 - 1];
      const long long q0 = pb->parents_ptr[last], q1 = pb->parents_ptr[last + 1];
      bool ok = (q1 - q0) == (p1 - p0 - 1);
      for (long long k = 0; ok && k < q1 - q0; ++k) ok = pb->parents_idx[q0 + k] == pb->parents_idx[p0 + k];
      if (!ok) return refuse(msg, ST_ERR_UNSUPPORTED, "parents(u) is not parents(last parent)+[last parent]: for make_edges_limited's single-parent lists set the limited_tree bit of st_options");
    }
    const bool observed = B.nobs > 0;
    B.isref = (observed && B.level < pb->n_groups && pb->res_is_ref[B.level] == 1) ? 1 : 0;
    B.ld = B.P + (B.isref ? B.m : 1);
    B.panel_off = -1; B.acc_off = 0; B.acc_len = 0;
    B.chain_off = -1;
    if (observed) {
      B.panel_off = panel_total;
      panel_total += (long long)B.m * B.ld;
      B.chain_off = B.panel_off;
      if (t.limited) {
        B.chain_off = -1;
        if (B.isref) {   // every observed reference block may be somebody's parent (observed or prediction children)
          B.chain_off = panel_total;
          panel_total += (long long)B.m * B.m;
          t.twin_list.push_back(i);
          t.twin_maxM = std::max(t.twin_maxM, B.m);
        }
      }
    }
  }
  t.panel_total = (size_t)panel_total;
  return ST_OK;
}
// the message records of the observed blocks, one (m_a x m_a, m_a) pair per ancestor
static int place_records(TreeLayout &t, std::string &msg) {
  long long acc_total = 0;
  for (Blk &B : t.blks) {
    if (B.nobs == 0) continue;
    long long len = 0;
    for (int a = 0; a < B.nanc; ++a) {
      const int ma = t.blks[t.anc_idx[B.anc_ptr + a]].m;
      len += (long long)ma * ma + ma;
    }
    if (len > INT_MAX) return refuse(msg, ST_ERR_UNSUPPORTED, "message record too large");
    B.acc_len = (int)len;
    B.acc_off = acc_total;
    acc_total += len;
  }
  t.acc_total = (size_t)acc_total;
  return ST_OK;
}
// multi-GPU ownership: whole subtrees below a cut level go to one rank, the levels
// above the cut are replicated.  cut = first reference level (not the last observed one) with >= 2*world
// observed blocks; its blocks, contiguous in device order, are split into `world` runs of equal weight
// (weight = sum over the subtree of m*P^2, the factorisation cost).
static int assign_owners(const st_problem *pb, TreeLayout &t, const Census &c, std::string &msg) {
  const int nb = (int)t.n_blocks;
  t.blk_owner.assign(nb, -1);
  t.cut = c.n_actual;            // nothing sharded unless a cut is found
  if (t.world <= 1) return ST_OK;
  std::vector<int> cnt(c.G, 0);
  for (int i = 0; i < nb; ++i) if (t.blks[i].nobs > 0) cnt[t.blks[i].level]++;
  for (int g = 0; g + 1 < c.n_actual; ++g)
    if (pb->res_is_ref[g] == 1 && cnt[g] >= 2 * t.world) { t.cut = g; break; }
  if (t.cut >= c.n_actual) return ST_OK;
  const int cut = t.cut;
  std::vector<int> root_of(nb, -1);   // device index of the cut-level ancestor (or self)
  std::vector<double> wsub(nb, 0.0);
  for (int i = 0; i < nb; ++i) {
    const Blk &B = t.blks[i];
    if (B.level < cut) continue;
    int r = -1;
    if (B.level == cut) r = i;
    else if (B.nanc > 0) {
      // through the DIRECT parent (the last ancestor), whose own root is known already: device order sorts blocks by level.
      // Works for make_edges' full ancestor lists and for make_edges_limited's single parents (tree_dep.cpp:133-186) alike
      const int par = t.anc_idx[B.anc_ptr + B.nanc - 1];
      r = t.blks[par].level == cut ? par : root_of[par];
    }
    if (r < 0) return refuse(msg, ST_ERR_TOPOLOGY, "block below the cut level without an ancestor on it");
    root_of[i] = r;
    wsub[r] += (double)B.m * ((double)B.P * B.P + 1.0);
  }
  std::vector<int> roots;
  double tot = 0;
  for (int i = 0; i < nb; ++i) if (t.blks[i].level == cut && t.blks[i].nobs > 0) { roots.push_back(i); tot += wsub[i]; }
  double acc_w = 0;
  std::vector<int> root_owner(nb, 0);
  for (size_t k = 0; k < roots.size(); ++k) {
    int r = (int)std::floor((acc_w + 0.5 * wsub[roots[k]]) / tot * t.world);
    r = std::min(std::max(r, 0), t.world - 1);
    if (k > 0) r = std::max(r, root_owner[roots[k - 1]]);   // keep runs contiguous
    root_owner[roots[k]] = r;
    acc_w += wsub[roots[k]];
  }
  for (int i = 0; i < nb; ++i) if (root_of[i] >= 0) t.blk_owner[i] = root_owner[root_of[i]];
  return ST_OK;
}

int layout_order(const st_problem *pb, const st_options *opt, TreeLayout &t, std::string &msg) {
  if (int rc = check_arguments(pb, opt, msg)) return rc;
  t.rank = opt ? opt->rank : 0;
  t.world = opt ? opt->world : 1;
  t.force_generic = opt ? opt->force_generic : 0;
  t.limited = opt && (opt->reserved & 2);
  t.defer_leaf = !(opt && (opt->reserved & 4));
  t.n_all = pb->n_all; t.n_blocks = pb->n_blocks; t.q = pb->q; t.p = pb->p; t.d = pb->d; t.n_groups = pb->n_groups;
  Census c;
  if (int rc = take_census(pb, t, c, msg)) return rc;
  if (int rc = order_blocks(pb, t, c, msg)) return rc;
  if (int rc = link_ancestors(pb, t, c, msg)) return rc;
  if (int rc = place_records(t, msg)) return rc;
  return assign_owners(pb, t, c, msg);
}

// ---- layout_levels
// extents, algorithmic bytes / flops and the generic kernels' LDS of a block list
static void level_geometry(const TreeLayout &t, LevelInfo &L, const std::vector<int> &list, bool is_pred) {
  for (int b : list) {
    const Blk &B = t.blks[b];
    L.maxP = std::max(L.maxP, B.P); L.maxM = std::max(L.maxM, B.m); L.maxLd = std::max(L.maxLd, B.ld); L.maxJ = std::max(L.maxJ, B.nanc);
    for (int a = 0; a < B.nanc; ++a) L.maxMa = std::max(L.maxMa, t.blks[t.anc_idx[B.anc_ptr + a]].m);
    const double m = B.m, P = B.P, tri = P * (P + 1) / 2, rim = B.isref ? m * (m + 1) / 2 : m;
    double trisum = 0;
    for (int a = 0; a < B.nanc; ++a) { const double ma = t.blks[t.anc_idx[B.anc_ptr + a]].m; trisum += ma * (ma + 1) / 2; }
    if (!is_pred) {
      L.alg_bytes_A += (8.0 * 2 + 8) * (m + P) + (t.q > 1 ? 4 * (m + P) : 0) + 8 * tri + 8 * m * P + 8 * rim + 16;
      L.alg_bytes_B += 8 * m * P + 8 * rim + 8 * P + 40 * m;
      L.alg_bytes_C += 8 * m * P + 8 * rim + 8 * (m + P) + 8;
      L.alg_bytes_msg += 2 * 8 * (P + trisum);
      L.flops_A += 2 * m * P * P + (B.isref ? 2 * m * m * P + m * m * m : 0);
      L.flops_B += (B.isref ? 2.0 / 3 * m * m * m : 0) + 4 * m * P;
      for (int a = 0; a < B.nanc; ++a) { const double ma = t.blks[t.anc_idx[B.anc_ptr + a]].m; L.flops_B += 2 * ma * ma * m; }
      L.flops_C += 2 * m * P + (B.isref ? m * m : 0);
    }
  }
  L.maxMa = std::max(L.maxMa, 1);
  const int SR = 8;
  L.lds_factor = lds_factor_bytes(L.maxP, L.maxM, L.maxMa, SR, false);
  L.big_factor = t.force_generic || L.lds_factor > t.lds_limit;
  if (L.big_factor) L.lds_factor = lds_factor_bytes(L.maxP, L.maxM, L.maxMa, 4, true);
  L.lds_sample = lds_sample_bytes(L.maxP, L.maxM, L.maxLd, false);
  L.big_sample = t.force_generic || L.lds_sample > t.lds_limit || (L.isref && L.maxM > 32 && L.maxM <= 80);   // wide reference blocks: the
  // scratch-arena kernel has the blocked matrix-core solve (the LDS-panel kernel factorises with three barriers per pivot)
  if (L.big_sample) {
    L.lds_sample = lds_sample_bytes(L.maxP, L.maxM, L.maxLd, true);
    // the posterior precision in LDS, factorised and solved by ONE wave without workgroup barriers (wave_chol_solve_lds):
    // every reference level where it fits (config #4: 74 KB, two workgroups per CU).  [The earlier LDS variant -- S and
    // chol(S)^-1, 100 KB, one barrier per pivot -- only paid on levels of at most 2 x CUs blocks.]
    if (L.isref && L.maxM <= 80 && L.lds_sample + lds_sample_sq_bytes(L.maxM) <= t.lds_limit) {
      L.lds_sample += lds_sample_sq_bytes(L.maxM); L.sample_sq = true;
    }
  }
  L.lds_loglik = lds_loglik_bytes(L.maxP, L.maxM);
}
// One column group from list[i] on: the block alone, or (non-reference) the block and its consecutive siblings, at most 32
// blocks and 32 columns.  same_shape adds the prediction groups' two conditions: rows contiguous, one chain length.
// Returns the position behind the group.
static size_t take_group(const TreeLayout &t, const std::vector<int> &list, size_t i, bool same_shape, Grp &G) {
  const Blk &B = t.blks[list[i]];
  G.row0 = B.row0; G.blk0 = list[i]; G.nblk = 1; G.M = B.m; G.P = B.P;
  size_t j = i + 1;
  if (B.isref) return j;
  const int lastp = last_parent(t, B, -1);
  while (j < list.size() && G.nblk < 32) {
    const Blk &C = t.blks[list[j]];
    if (C.isref || last_parent(t, C, -1) != lastp || list[j] != list[j - 1] + 1 || G.M + C.m > 32) break;
    if (same_shape && (C.row0 != G.row0 + G.M || C.P != B.P)) break;
    G.M += C.m; G.nblk += 1; ++j;
  }
  return j;
}
// column groups for the MFMA path: a reference block alone, or consecutive sibling non-reference blocks; L.fast and the
// LDS layout of k_factor_mfma / k_sample_mfma where every block of the level fits
static void level_column_groups(TreeLayout &t, LevelInfo &L, const std::vector<int> &list) {
  L.grp_first = (int)t.grps.size();
  bool ok = !t.force_generic && L.maxP <= 256 && L.maxMa <= 32;
  int maxM = 0, maxKb = 0, maxSub = 1;
  size_t i = 0;
  while (ok && i < list.size()) {
    const Blk &B = t.blks[list[i]];
    if (B.m > 32) { ok = false; break; }
    Grp G;
    i = take_group(t, list, i, false, G);
    maxM = std::max(maxM, G.M);
    for (int a = 0; a < B.nanc; ++a) {
      const int ma = t.blks[t.anc_idx[B.anc_ptr + a]].m;
      maxSub = std::max(maxSub, ma > 16 ? (ma + 1) / 2 : ma);
    }
    maxKb = std::max(maxKb, B.P);
    t.grps.push_back(G);
  }
  L.grp_count = (int)t.grps.size() - L.grp_first;
  if (ok) {
    L.Pm4 = (L.maxP + 3) & ~3;
    L.ldKV = std::max(2, (maxM + 1) & ~1);
    L.ldS = stage_stride(std::max(2, maxKb + 4));          // 4 zero-filled pad columns per staged row
    L.SRm = maxSub;
    size_t st = (size_t)L.SRm * L.ldS + 16;
    st = std::max(st, (size_t)2 * L.Pm4 + L.Pm4 / 2 + 2);   // prologue alias: ancestor x, y, outcome ids
    st = std::max(st, (size_t)2 * 32 * CH_LD + 216 + 36);     // epilogue alias: R, Ri (stride CH_LD), elimination scratch
    st = ((st + 1) & ~(size_t)1) + (size_t)L.ldS + 16;       // + the zero row at the end
    L.stage_dbl = (int)((st + 1) & ~(size_t)1);
    L.lds_fast = ((size_t)L.Pm4 * L.ldKV + 16 + L.stage_dbl + FM_VPART + 5 * 32) * 8 + 64 * 4 + 64;
    ok = L.lds_fast <= t.lds_limit;
  }
  if (ok) {
    L.Mr4 = std::max(4, (maxM + 3) & ~3);
    L.Mrows = std::max(1, maxM);
    L.ldN = L.maxLd | 1;              // odd stride >= the longest panel row
    L.av_dbl = std::max(32 * L.maxJ, 224);
    const size_t dbl = (size_t)maxM * L.ldN + 32 + (size_t)L.maxP + 32 + 6 * 32 + (size_t)L.av_dbl + 16 + (L.isref ? (size_t)maxM * CH_LD : 0) + 16;
    L.lds_sfast = dbl * 8 + 64 * 4 + 64;
    L.lds_slean = ((size_t)L.maxP + 32 + (size_t)L.av_dbl + 224 + 16 + 7 * 32 + (L.isref ? 2 * 32 * CH_LD : 0) + 16) * 8;
    ok = L.lds_sfast <= t.lds_limit;
  }
  L.fast = ok;
  if (!ok) { t.grps.resize(L.grp_first); L.grp_count = 0; }
}
// a level off the column-group path: k_factor_bigmfma where its LDS fits, and on top of that the lchain flags
static void level_big_routes(const TreeLayout &t, LevelInfo &L, const std::vector<int> &list) {
  if (L.fast || t.force_generic || L.maxM > 80 || L.maxP > BM_MAXP) return;   // (a root level, P = 0, included: its 75 x 75 factorisation is the blocked one of the epilogue)
  const int ldS = stage_stride(L.maxP + 24);
  L.bm_ldS = ldS;
  const size_t work = std::max((size_t)17 * ldS + 16 * 80 + BM_KS * 5 * 256, (size_t)2 * L.maxM * L.maxM + 64);   // stage + zero row + V tile + partial V tiles | R, Ri of the epilogue
  L.lds_bigmfma = ((size_t)3 * (L.maxP + L.maxM) + 3 * (size_t)L.maxM + work) * 8 + (size_t)((L.maxP + L.maxM + 1) & ~1) * 4 + 64;
  L.bigmfma = L.lds_bigmfma <= t.lds_limit;
  if (!L.bigmfma || !t.sw.lchain || t.limited || L.maxP > 544) return;
  // non-reference blocks, <= 64 columns, every block behind at least one ancestor: k_factor_lchain (K in registers, the
  // chain factor streamed through LDS twice); a property of the level, the same on every rank
  if (!L.isref && L.maxM <= 64) {
    bool all_anc = true;
    for (int b : list) all_anc = all_anc && t.blks[b].nanc >= 1 && !t.blks[b].isref;
    if (all_anc) L.lchain = L.maxP <= 384 ? 96 : 136;
  }
  // REFERENCE levels behind a chain (round 3): k_factor_lchain for the chain pass (it runs it at more than twice
  // k_factor_bigmfma's rate, and a block's columns are two slabs on two CUs: the single-block top levels gain too), then
  // k_factor_ref_finish per block.  L.count, not the rank's share: a property of the level
  if (t.sw.lchain_ref && L.isref && L.maxM <= 80 && L.count >= t.sw.lchain_ref_min) {
    bool all_anc = true;
    for (int b : list) all_anc = all_anc && t.blks[b].nanc >= 1 && t.blks[b].isref;
    if (all_anc) { L.lchain = L.maxP <= 384 ? 96 : 136; L.lchain_ref = true; }
  }
}
// level lists (u_by_block_groups), per-level geometry and the route flags that depend on the level alone
static int build_levels(const st_problem *pb, TreeLayout &t, std::string &msg) {
  const long long nb = t.n_blocks;
  t.levels.resize(t.n_actual_groups);
  for (int g = 0; g < t.n_actual_groups; ++g) {
    LevelInfo &L = t.levels[g];
    L.first = (int)t.lvl_list.size();
    L.isref = (int)pb->res_is_ref[g];
    // reference order inside a level: block_names order (make_gibbs_groups :238-246); order is irrelevant on device
    for (long long i = 0; i < nb; ++i) {
      const long long u = pb->block_names[i] - 1;
      if (u < 0 || u >= nb) return refuse(msg, ST_ERR_TOPOLOGY, "block_names out of range");
      const Blk &B = t.blks[t.blk_model2dev[u]];
      if (B.level == g && B.nobs > 0) t.lvl_list.push_back(t.blk_model2dev[u]);
    }
    L.count = (int)t.lvl_list.size() - L.first;
    std::sort(t.lvl_list.begin() + L.first, t.lvl_list.end());
    const std::vector<int> list(t.lvl_list.begin() + L.first, t.lvl_list.end());
    level_geometry(t, L, list, false);
    level_column_groups(t, L, list);
    level_big_routes(t, L, list);
    if (L.lds_factor > t.lds_limit || L.lds_sample > t.lds_limit || L.lds_loglik > t.lds_limit)
      return refuse(msg, ST_ERR_UNSUPPORTED, "block too large for the LDS-resident vectors");
  }
  return ST_OK;
}
// direct children that hold a message record: every observed block of a generic level, the first block of each
// column group of a fast level (the group's record is the sum over its sibling blocks)
static int link_children(TreeLayout &t, std::string &msg) {
  const int nb = (int)t.n_blocks;
  std::vector<std::vector<int>> dch(nb);
  for (int i = 0; i < nb; ++i)
    if (t.blks[i].nobs > 0 && t.blks[i].nanc > 0) dch[last_parent(t, t.blks[i], -1)].push_back(i);
  std::vector<char> holder(nb, 0);
  for (const LevelInfo &L : t.levels) {
    if (L.fast) for (int k = 0; k < L.grp_count; ++k) holder[t.grps[L.grp_first + k].blk0] = 1;
    else for (int k = 0; k < L.count; ++k) holder[t.lvl_list[L.first + k]] = 1;
  }
  for (int i = 0; i < nb; ++i) {
    Blk &B = t.blks[i];
    B.dch_ptr = (int)t.dch_idx.size();
    B.ndch = 0;
    if (!dch[i].empty() && !B.isref) return refuse(msg, ST_ERR_TOPOLOGY, "a non-reference block has observed children");
    for (int c : dch[i]) if (holder[c]) { t.dch_idx.push_back(c); B.ndch++; }
    if (B.ndch > 64 && B.nobs > 0 && t.levels[B.level].fast)
      return refuse(msg, ST_ERR_UNSUPPORTED, "more than 64 direct child groups under one block");
  }
  return ST_OK;
}
// [lo, lo + n): from the first to the last k of 0 .. count-1 with mine(k); (0, 0) when there is none
template <typename F>
static void own_run(int count, F mine, int &lo_out, int &n_out) {
  int lo = count, hi = 0;
  for (int k = 0; k < count; ++k) if (mine(k)) { lo = std::min(lo, k); hi = std::max(hi, k + 1); }
  lo_out = lo < hi ? lo : 0; n_out = lo < hi ? hi - lo : 0;
}
// this rank's run of a level's block list and group list
static int level_own_runs(const TreeLayout &t, LevelInfo &L, int g, std::string &msg) {
  L.own_lo = 0; L.own_n = L.count; L.gown_lo = 0; L.gown_n = L.grp_count;
  if (g < t.cut) return ST_OK;
  own_run(L.count, [&](int k) { return t.blk_owner[t.lvl_list[L.first + k]] == t.rank; }, L.own_lo, L.own_n);
  for (int k = L.own_lo; k < L.own_lo + L.own_n; ++k)
    if (t.blk_owner[t.lvl_list[L.first + k]] != t.rank) return refuse(msg, ST_ERR_TOPOLOGY, "a rank's blocks are not contiguous in a level");
  if (!L.fast) return ST_OK;
  for (int k = 0; k < L.grp_count; ++k) {
    const Grp &Gr = t.grps[L.grp_first + k];
    for (int b2 = 1; b2 < Gr.nblk; ++b2)
      if ((t.blk_owner[Gr.blk0 + b2] == t.rank) != (t.blk_owner[Gr.blk0] == t.rank)) return refuse(msg, ST_ERR_TOPOLOGY, "a column group straddles two ranks");
  }
  own_run(L.grp_count, [&](int k) { return t.blk_owner[t.grps[L.grp_first + k].blk0] == t.rank; }, L.gown_lo, L.gown_n);
  return ST_OK;
}
// sibling groups for k_factor_wide (levels on the wide-block path): consecutive blocks of this rank's run with the same
// last parent (= the same chain; device order keeps siblings and their rows contiguous), at most WG_MAXB blocks and
// WG_MAXN columns per group.  Reads L.lchain as build_levels left it: a level that demote_lchain takes off the lchain
// route later has no wide groups and goes to k_factor_bigmfma.
static void level_wide_groups(TreeLayout &t, LevelInfo &L) {
  L.wide_first = (int)t.wgrps.size(); L.wide_count = 0; L.wide_maxN = 0;
  // measured at config #4 (577^2 x 3 outcomes): the leaf level 32.7 -> 28.2 ms, the 75-column reference level 13.9 -> 15.1 ms
  // (two blocks per group: more passes than staging saved), levels with fewer groups than CUs lose parallelism -- so only
  // big non-reference levels take it (SPAMTREE_WIDE=2 forces it on every eligible level: tests).  L.count, not the rank's
  // share: the two kernels round differently, and a level must take the same one on every rank of every world size
  // (bit-identical sharded runs)
  if (!(L.bigmfma && !L.lchain && t.sw.wide && !t.limited && (t.sw.wide == 2 || (!L.isref && L.count >= 2 * t.sm_count)))) return;
  int k = L.own_lo;
  const int kend = L.own_lo + L.own_n;
  while (k < kend) {
    const int b0 = t.lvl_list[L.first + k];
    const Blk &B0 = t.blks[b0];
    const int lastp = last_parent(t, B0, -1);
    WideGrp Gw; Gw.first = k - L.own_lo; Gw.count = 1;
    int Ncols = B0.m;
    while (k + Gw.count < kend && Gw.count < WG_MAXB) {
      const int b1 = t.lvl_list[L.first + k + Gw.count];
      const Blk &B1 = t.blks[b1];
      if (last_parent(t, B1, -2) != lastp || B1.nanc != B0.nanc || B1.isref != B0.isref || b1 != b0 + Gw.count || Ncols + B1.m > WG_MAXN ||
          B1.row0 != B0.row0 + Ncols) break;
      Ncols += B1.m; ++Gw.count;
    }
    L.wide_maxN = std::max(L.wide_maxN, Ncols);
    t.wgrps.push_back(Gw);
    ++L.wide_count;
    k += Gw.count;
  }
  const size_t work = std::max((size_t)17 * L.bm_ldS + 16 * 16 * WG_JT, (size_t)2 * L.maxM * L.maxM + 64);   // (bm_ldS: level_big_routes)
  L.lds_wide = ((size_t)3 * (L.maxP + L.wide_maxN) + 2 * (size_t)L.wide_maxN + work) * 8 + (size_t)((L.maxP + L.wide_maxN + 1) & ~1) * 4 + 64;
  if (L.lds_wide > t.lds_limit) { t.wgrps.resize(L.wide_first); L.wide_count = 0; }
}
// slabs for k_factor_lchain: sibling groups (consecutive blocks of this rank's run with the same last parent, contiguous
// rows AND panels, one row stride) cut into runs of <= 4 column tiles, as equal as possible (9 tiles -> 3 + 3 + 3).
// vscr_need counts every level flagged here, also one that demote_lchain takes off the route afterwards.
static void level_lchain_slabs(TreeLayout &t, LevelInfo &L) {
  L.lc_first = (int)t.lcslabs.size(); L.lc_count = 0;
  L.rf_first = (int)t.rfvoff.size();
  if (!L.lchain) return;
  int k = L.own_lo;
  const int kend = L.own_lo + L.own_n;
  long long vrun = 0;   // reference levels: the groups' V matrices (P x the group's columns, row-major) follow each other
  while (k < kend) {
    const int b0 = t.lvl_list[L.first + k];
    const Blk &B0 = t.blks[b0];
    const int lastp = t.anc_idx[B0.anc_ptr + B0.nanc - 1];
    int cnt = 1, Ncols = B0.m;
    while (k + cnt < kend && cnt < 16) {
      const int b1 = t.lvl_list[L.first + k + cnt];
      const Blk &B1 = t.blks[b1];
      if (b1 != b0 + cnt || B1.nanc != B0.nanc || t.anc_idx[B1.anc_ptr + B1.nanc - 1] != lastp || B1.P != B0.P || B1.ld != B0.ld ||
          B1.row0 != B0.row0 + Ncols || B1.panel_off != B0.panel_off + (long long)Ncols * B0.ld) break;
      Ncols += B1.m; ++cnt;
    }
    const int JT = (Ncols + 15) / 16, nsl = (JT + 3) / 4, tps = (JT + nsl - 1) / nsl;
    for (int s0 = 0; s0 < Ncols; s0 += 16 * tps) {
      LcSlab S;
      S.row0 = B0.row0 + s0; S.pan0 = B0.panel_off + (long long)s0 * B0.ld; S.blk0 = b0;
      S.ncol = std::min(16 * tps, Ncols - s0); S.ld = B0.ld; S.vcol0 = s0; S.vs0 = vrun;
      t.lcslabs.push_back(S);
      ++L.lc_count;
    }
    if (L.lchain_ref) {   // the group's blocks are equally wide (same P and ld): block i of the group owns columns [i m, (i + 1) m)
      for (int i = 0; i < cnt; ++i) { t.rfvoff.push_back(vrun); vrun += rf_vsize(B0.P); }
    }
    k += cnt;
  }
  if (L.lchain_ref) t.vscr_need = std::max(t.vscr_need, (size_t)vrun);
}
// One quad from group k of the grp_count groups at grp_first: up to nu_max consecutive column groups that share their
// ancestor chain (reference blocks) or the chain without its last ancestor (non-reference blocks: cousins).  same_owner:
// a quad does not cross from one rank's groups into another's.  (Prediction blocks are never reference blocks, so the
// isref comparison is vacuous for them.)
static Quad take_quad(const TreeLayout &t, int grp_first, int grp_count, int k, int nu_max, bool same_owner) {
  const Grp &G0 = t.grps[grp_first + k];
  const Blk &B0 = t.blks[G0.blk0];
  const int J = B0.nanc;
  Quad Qd;
  Qd.g0 = k; Qd.nu = 1; Qd.Jc = B0.isref ? J : std::max(J - 1, 0); Qd.Pc = 0;
  for (int a = 0; a < Qd.Jc; ++a) Qd.Pc += t.blks[t.anc_idx[B0.anc_ptr + a]].m;
  while (Qd.nu < nu_max && k + Qd.nu < grp_count) {
    const Grp &G1 = t.grps[grp_first + k + Qd.nu];
    const Blk &B1 = t.blks[G1.blk0];
    if (B1.nanc != J || B1.isref != B0.isref) break;
    if (same_owner && t.blk_owner[G1.blk0] != t.blk_owner[G0.blk0]) break;
    bool same = true;
    for (int a = 0; a < Qd.Jc && same; ++a) same = t.anc_idx[B1.anc_ptr + a] == t.anc_idx[B0.anc_ptr + a];
    if (!same) break;
    ++Qd.nu;
  }
  return Qd;
}
static size_t quad_lds_bytes(int quad_nu, int nkx, bool isref) {   // arena, zero row, V exchange / covariance scratch
  const int ldS = quad_lds_stride(nkx);   // the kernel's compile-time row stride (>= maxP + 24)
  return ((size_t)quad_nu * 16 * ldS + ldS + (isref ? (size_t)quad_nu * 512 : (size_t)2 * quad_nu * QUAD_LEAF_KH * 64)) * 8;
}
// quads for k_factor_quad: runs of up to quad_nu column groups of one rank
static void level_quads(TreeLayout &t, LevelInfo &L, int g) {
  L.quad_first = (int)t.quads.size(); L.quad_count = 0; L.q_nkx = 0; L.qown_lo = 0; L.qown_n = 0;
  if (!(L.fast && L.maxP > 0 && L.maxP <= 200 && L.maxMa <= 32)) return;
  // units per workgroup on THIS rank: a sharded level with few owned groups takes smaller quads, so that its
  // workgroups still cover the CUs (a workgroup of 2 / 1 units lives about 0.72 / 0.5 as long as one of 4; results do
  // not depend on the grouping: every unit's arithmetic is its own)
  int nu_max = t.quad_nu, owned = 0;
  for (int k = 0; k < L.grp_count; ++k)
    if (g < t.cut || t.blk_owner[t.grps[L.grp_first + k].blk0] == t.rank) ++owned;
  double best = 1e300;
  const int cand[3] = {4, 2, 1};
  const double tl[3] = {1.0, 0.72, 0.5};
  for (int c = 0; c < 3; ++c) {
    if (cand[c] > t.quad_nu) continue;
    const double rounds = std::ceil((double)std::max(owned, 1) / (double)(cand[c] * t.sm_count));
    if (rounds * tl[c] < best - 1e-9) { best = rounds * tl[c]; nu_max = cand[c]; }
  }
  if (t.sw.quad_units >= 1 && t.sw.quad_units <= t.quad_nu) nu_max = t.sw.quad_units;   // tests: force the units per workgroup
  // pass 0 ignores ownership: its quad count decides eligibility, so that every rank of every world size takes
  // the same kernel for a level (results are then bit-identical across world sizes); pass 1 builds this rank's quads
  bool mixed = false;
  int nq_any = 0;
  for (int pass = 0; pass < 2; ++pass) {
    for (int k = 0; k < L.grp_count;) {
      const int blk0 = t.grps[L.grp_first + k].blk0;
      if ((t.blks[blk0].isref != 0) != (L.isref != 0)) mixed = true;
      const Quad Qd = take_quad(t, L.grp_first, L.grp_count, k, pass == 0 ? t.quad_nu : nu_max, pass == 1);
      if (pass == 0) ++nq_any;
      else { t.quads.push_back(Qd); L.quad_count++; }
      k += Qd.nu;
    }
  }
  own_run(L.quad_count, [&](int k) { return g < t.cut || t.blk_owner[t.grps[L.grp_first + t.quads[L.quad_first + k].g0].blk0] == t.rank; },
          L.qown_lo, L.qown_n);
  L.q_nkx = quad_nkx(L.maxP);
  L.q_ldS = quad_lds_stride(L.q_nkx);
  L.lds_quad = quad_lds_bytes(t.quad_nu, L.q_nkx, L.isref);
  const int min_groups = t.sw.quad_min >= 0 ? t.sw.quad_min : 2 * t.sm_count;   // smaller levels do not fill the chip with quads: k_factor_mfma's 4x more workgroups win
  if (L.grp_count < 2 * nq_any || mixed || L.grp_count < min_groups) L.q_nkx = 0;   // mostly singletons: nothing to share
  if (L.isref && L.q_nkx == 50) L.q_nkx = 0;                   // that instantiation spills registers: k_factor_mfma is faster
}
// exchange masks, this rank's observed blocks, the cut level's record region
static void mark_owned(TreeLayout &t) {
  const int nb = (int)t.n_blocks;
  t.rowmask.assign(t.n_all, 0); t.blkmask.assign(nb, 0);
  for (int i = 0; i < nb; ++i) {
    const Blk &B = t.blks[i];
    const bool mine = (t.blk_owner[i] == t.rank) || (t.blk_owner[i] < 0 && t.rank == 0);
    t.blkmask[i] = mine ? 1 : 0;
    if (mine) for (int r2 = 0; r2 < B.m; ++r2) t.rowmask[B.row0 + r2] = 1;
    if (B.nobs > 0 && (t.blk_owner[i] < 0 || t.blk_owner[i] == t.rank)) t.own_obs_list.push_back(i);
  }
  if (t.cut >= t.n_actual_groups) return;
  const LevelInfo &L = t.levels[t.cut];
  long long lo = -1, hi = -1;
  for (int k = 0; k < L.count; ++k) {
    const Blk &B = t.blks[t.lvl_list[L.first + k]];
    if (lo < 0) lo = B.acc_off;
    hi = B.acc_off + B.acc_len;
    if (t.blk_owner[t.lvl_list[L.first + k]] != t.rank && B.acc_len > 0) t.top_zero.push_back({B.acc_off, (long long)B.acc_len});
  }
  t.top_off = std::max(0LL, lo); t.top_len = hi > lo ? hi - lo : 0;
}
// phase P on the leaf path of k_factor_quad (prediction blocks are non-reference blocks behind a chain of reference
// blocks, exactly what a leaf level is: spamtree_model.cpp:1296-1326 is A7 + a draw): column groups of consecutive sibling
// prediction blocks (<= 32 columns) and quads of up to four groups that share all but the last ancestor.  Every rank predicts
// every block (as the generic kernel does: w is replicated).  Not eligible (long chains, wide blocks): the generic kernel.
static int build_prediction(TreeLayout &t, std::string &msg) {
  for (int i = 0; i < (int)t.n_blocks; ++i) {
    if (t.blks[i].nobs > 0) t.all_obs_list.push_back(i);
    else {
      if (t.blks[i].nanc == 0) return refuse(msg, ST_ERR_TOPOLOGY, "prediction block without parents");
      t.pred_list.push_back(i);
    }
  }
  level_geometry(t, t.pred_info, t.pred_list, true);
  t.pred_grp_first = (int)t.grps.size(); t.pred_grp_count = 0; t.pred_quad_first = (int)t.quads.size(); t.pred_quad_count = 0; t.pred_nkx = 0;
  const LevelInfo &Lp = t.pred_info;
  const std::vector<int> &list = t.pred_list;
  bool ok = !t.force_generic && !list.empty() && Lp.maxP > 0 && Lp.maxP <= 200 && Lp.maxMa <= 32 && Lp.maxM <= 32;
  size_t i = 0;
  while (ok && i < list.size()) {
    const Blk &B = t.blks[list[i]];
    if (B.isref || B.nanc < 1) { ok = false; break; }
    Grp G;
    i = take_group(t, list, i, true, G);
    t.grps.push_back(G);
  }
  if (!ok) t.grps.resize(t.pred_grp_first);
  t.pred_grp_count = (int)t.grps.size() - t.pred_grp_first;
  if (!ok || t.pred_grp_count == 0) return ST_OK;
  for (int k = 0; k < t.pred_grp_count; k += t.quads.back().nu)
    t.quads.push_back(take_quad(t, t.pred_grp_first, t.pred_grp_count, k, t.quad_nu, false));
  t.pred_quad_count = (int)t.quads.size() - t.pred_quad_first;
  t.pred_nkx = quad_nkx(Lp.maxP);
  t.pred_lds = quad_lds_bytes(t.quad_nu, t.pred_nkx, false);
  return ST_OK;
}
// group descriptors: the flattened metadata of every column group (layout: GdHead / gd_unpack)
static int pack_group_descriptors(TreeLayout &t, const std::vector<long long> &blk2grp, std::string &msg) {
  int stride = 8;
  for (const Grp &G : t.grps) {
    const Blk &B0 = t.blks[G.blk0];
    stride = std::max(stride, 8 + 4 * B0.nanc + 3 * G.nblk + 2 * std::min(B0.ndch, 64));   // children: record offset + group id
  }
  stride = (stride + 1) & ~1;
  if (stride > GD_MAXW) return refuse(msg, ST_ERR_UNSUPPORTED, "group descriptor too long");
  t.gd_stride = stride;
  t.gdesc.assign(std::max<size_t>(1, t.grps.size()) * (size_t)stride, 0);
  auto pack = [](long long lo, long long hi) { return (lo & 0xffffffffLL) | (hi << 32); };
  for (size_t g = 0; g < t.grps.size(); ++g) {
    const Grp &G = t.grps[g];
    const Blk &B0 = t.blks[G.blk0];
    long long *w = t.gdesc.data() + g * (size_t)stride;
    const int nch = std::min(B0.ndch, 64);
    w[0] = G.row0; w[1] = B0.acc_off; w[2] = pack(G.M, G.P); w[3] = pack(B0.nanc, G.nblk); w[4] = pack(B0.isref, B0.level);
    w[5] = pack(nch, t.limited ? 0 : B0.acc_len); w[6] = pack(G.blk0, 0);
    long long ao = 0, aoff = 0;
    for (int j = 0; j < B0.nanc; ++j) {
      const Blk &Ba = t.blks[t.anc_idx[B0.anc_ptr + j]];
      long long *a = w + 8 + 4 * j;
      a[0] = pack(Ba.m, ao); a[1] = Ba.row0; a[2] = Ba.chain_off; a[3] = aoff;
      ao += Ba.m; aoff += (long long)Ba.m * Ba.m + Ba.m;
    }
    w[7] = aoff;
    for (int b = 0; b < G.nblk; ++b) {
      const Blk &Bb = t.blks[G.blk0 + b];
      long long *q = w + 8 + 4 * B0.nanc + 3 * b;
      q[0] = Bb.panel_off; q[1] = Bb.row0; q[2] = Bb.ld;
    }
    for (int c = 0; c < nch; ++c) w[8 + 4 * B0.nanc + 3 * G.nblk + c] = t.blks[t.dch_idx[B0.dch_ptr + c]].acc_off;
    for (int c = 0; c < nch; ++c) w[8 + 4 * B0.nanc + 3 * G.nblk + nch + c] = blk2grp[t.dch_idx[B0.dch_ptr + c]];   // k_gram_direct
  }
  return ST_OK;
}
// Gram parts of the last reference level straight from the leaf groups' panels (k_gram_direct): every block of that level
// has at most GRAM_DIRECT_MAXCH children, all of them column groups of the (non-reference) last level
static void choose_gram_direct(TreeLayout &t, const std::vector<long long> &blk2grp) {
  t.gram_direct_level = -1;
  const int gl = t.n_actual_groups - 1, gp = t.n_actual_groups - 2;
  if (!(t.sw.gram_direct && gp >= 0 && !t.limited && t.levels[gl].fast && !t.levels[gl].isref && t.levels[gp].fast && t.levels[gp].isref &&
        t.levels[gl].maxM <= 32 && t.levels[gl].maxP <= 255)) return;
  bool ok = true;
  const LevelInfo &Lp = t.levels[gp], &Ll = t.levels[gl];
  for (int k = 0; k < Lp.grp_count && ok; ++k) {
    const Grp &G = t.grps[Lp.grp_first + k];
    const Blk &B0 = t.blks[G.blk0];
    if (G.nblk != 1 || B0.ndch > GRAM_DIRECT_MAXCH) ok = false;
    for (int c = 0; c < B0.ndch && ok; ++c) {
      const long long cg = blk2grp[t.dch_idx[B0.dch_ptr + c]];
      if (cg < Ll.grp_first || cg >= Ll.grp_first + Ll.grp_count || t.grps[cg].M > 32) ok = false;
    }
  }
  // ... and every leaf group's record is read by a block of that level only (its direct parent): a leaf block hanging
  // from a shallower reference level would leave that parent's Gram part unwritten on rebuild sweeps
  for (int k = 0; k < Ll.grp_count && ok; ++k) {
    const Grp &G = t.grps[Ll.grp_first + k];
    for (int b = 0; b < G.nblk && ok; ++b) {
      const Blk &Bl = t.blks[G.blk0 + b];
      if (Bl.nanc == 0 || t.blks[last_parent(t, Bl, 0)].level != gp) ok = false;
    }
  }
  if (ok) t.gram_direct_level = gp;
}
// what the device step allocates by the layout's count: the reference blocks' Ri' Ri, this rank's group / block lists of
// phase C, the all-gather index of w, the generic kernels' scratch
static void size_buffers(TreeLayout &t) {
  const int nb = (int)t.n_blocks;
  t.s0off.assign((size_t)(nb > 0 ? nb : 1), -1);
  for (const LevelInfo &L : t.levels) {
    if (!L.isref || !(L.big_sample || L.fast)) continue;   // generic wide-block levels (round 2) and the column-group levels (round 3)
    for (int k = 0; k < L.count; ++k) {
      const int b = t.lvl_list[L.first + k];
      t.s0off[b] = (long long)t.s0_total;
      t.s0_total += (size_t)t.blks[b].m * t.blks[b].m;
    }
  }
  for (const LevelInfo &L : t.levels)
    if (L.fast) for (int k = 0; k < L.gown_n; ++k) t.own_grp_list.push_back(L.grp_first + L.gown_lo + k);
  for (int b : t.own_obs_list) if (!t.levels[t.blks[b].level].fast) t.own_obs_slow.push_back(b);
  // all-gather of w: every rank's owned rows (blocks below the cut, prediction blocks included), in device order; the
  // replicated top is sampled identically everywhere and does not travel
  std::vector<std::vector<int>> rows_of(t.world);
  for (int i = 0; i < nb; ++i) {
    const int o = t.blk_owner[i];
    if (o < 0) continue;
    const Blk &B = t.blks[i];
    for (int r2 = 0; r2 < B.m; ++r2) rows_of[o].push_back((int)(B.row0 + r2));
  }
  size_t mx = 0;
  for (auto &v : rows_of) mx = std::max(mx, v.size());
  t.gather_cnt = (int)mx + 1;   // last slot: the rank's failure word
  t.gidx.assign((size_t)t.world * t.gather_cnt, -1);
  for (int r = 0; r < t.world; ++r) std::copy(rows_of[r].begin(), rows_of[r].end(), t.gidx.begin() + (size_t)r * t.gather_cnt);
  // scratch for the generic kernels: a bounded number of resident workgroups, each with its own slice
  size_t need = 0;
  auto upd = [&](const LevelInfo &L) {
    if (L.big_factor || L.bigmfma) need = std::max(need, scratch_factor_doubles(L.maxP, L.maxM, L.maxMa));
    if (L.wide_count > 0) need = std::max(need, (size_t)2 * L.maxP * L.wide_maxN + (size_t)L.maxMa * L.wide_maxN);
    if (L.big_sample) need = std::max(need, (size_t)L.maxM * L.maxM);
  };
  for (auto &L : t.levels) upd(L);
  if (!t.pred_list.empty()) upd(t.pred_info);
  if (need > 0) {
    t.scratch_wgs = t.sm_count * 4;
    t.scratch_stride = (long long)((need + 15) & ~(size_t)15);
  }
}
// The kernels' static LDS decides last: k_factor_lchain and k_factor_quad need static + dynamic LDS within one CU's 160 KB,
// else the level stays on the older kernels (k_factor_bigmfma / k_factor_mfma).  Then, with the quads settled, the V tiles
// of the deferred leaf levels (one GPU only: the sharded protocol has no st_factor_enqueue of its own).
static void demote_by_static_lds(TreeLayout &t, const DeviceLimits &dl) {
  for (auto &L : t.levels) {
    if (!L.lchain) continue;
    const int i = L.lchain == 96 ? 0 : 1;
    if (lc_dyn_doubles(L.lchain) * 8 + dl.lchain_static[i] > DeviceLimits::CU_LDS || !dl.lchain_no_scratch[i]) { L.lchain = 0; L.lchain_ref = false; }
    if (L.lchain_ref) {
      L.lds_ref_finish = rf_lds_bytes(L.maxM);
      if (L.lds_ref_finish > t.lds_limit) { L.lchain = 0; L.lchain_ref = false; }
    }
  }
  for (auto &L : t.levels)
    if (L.q_nkx && L.lds_quad + dl.quad_static > DeviceLimits::CU_LDS) L.q_nkx = 0;
  if (t.pred_nkx && t.pred_lds + dl.quad_static > DeviceLimits::CU_LDS) t.pred_nkx = 0;
  for (auto &L : t.levels) {
    L.vl_off = -1;
    if (!t.defer_leaf || t.world > 1 || t.limited || t.sw.factor_gen != 3 || !L.fast || L.isref || L.q_nkx == 0 || L.qown_n == 0) continue;
    L.vl_off = (long long)t.vleaf_total;
    t.vleaf_total += (size_t)L.qown_n * quad_vtiles(L.q_nkx) * (2 * t.quad_nu) * 256;
  }
}
// One quad's record (QuadRec, factor_quad.hpp) from the blocks and groups: the values k_factor_quad's prologue used to
// gather -- the units' extents, the shared chain's and the private ancestors' rows with their coordinates, the units'
// columns, the rows' places in the panel arena.  Coordinates and outcome ids are the device arrays' (create_rows): row r is
// model row dev2model[r].  The slots wpa / colw / pw take the entry's global row (the kernel puts w there).
template <int PMAX, bool ISREF>
static void fill_quad_record(const st_problem *pb, const TreeLayout &t, int grp_first, const Quad &Qd, long long *out) {
  typedef QuadRec<4, PMAX, ISREF> Rec;
  Rec R;
  std::memset(&R, 0, sizeof(R));
  const long long n = t.n_all;
  auto put = [&](long long r, double &x, double &y, int &mv, double &wslot) {
    const long long m = t.dev2model[r];
    x = pb->coords[m]; y = pb->coords[n + m]; mv = (int)(pb->mv_id[m] - 1);
    std::memcpy(&wslot, &r, sizeof(double));
  };
  const long long none = -1;
  for (int i = 0; i < 4 * 32; ++i) std::memcpy(&R.colw[0][0] + i, &none, sizeof(double));
  for (int i = 0; i < Rec::NUL * Rec::NLD; ++i) std::memcpy(&R.pw[0][0] + i, &none, sizeof(double));
  for (int k = 0; k < PMAX; ++k) std::memcpy(&R.wpa[k], &none, sizeof(double));
  R.g0 = Qd.g0; R.nu = Qd.nu; R.Jc = Qd.Jc; R.Pc = Qd.Pc;
  R.nit = (Qd.Pc + 31) >> 5;
  const Blk &U0 = t.blks[t.grps[grp_first + Qd.g0].blk0];
  R.level = U0.level;
  int k = 0;   // the shared chain: the first Jc ancestors of unit 0, row after row
  for (int a = 0; a < Qd.Jc; ++a) {
    const Blk &Ba = t.blks[t.anc_idx[U0.anc_ptr + a]];
    const int len = k + Ba.m;   // a row runs to the end of its own ancestor's rows
    for (int i = 0; i < Ba.m && k < PMAX; ++i, ++k) {
      put(Ba.row0 + i, R.sx[k], R.sy[k], R.smv[k], R.wpa[k]);
      R.rlen[k] = len; R.rsrc[k] = Ba.chain_off + (long long)i * len;
    }
  }
  for (int u = 0; u < Qd.nu; ++u) {
    const Grp &G = t.grps[grp_first + Qd.g0 + u];
    const Blk &B0 = t.blks[G.blk0];
    R.uM[u] = G.M; R.uP[u] = G.P; R.ublk0[u] = G.blk0; R.unblk[u] = G.nblk; R.uref[u] = B0.isref; R.uJ[u] = B0.nanc; R.urow0[u] = G.row0;
    if (B0.nanc > Qd.Jc) {   // the private (last) ancestor
      const Blk &Bp = t.blks[t.anc_idx[B0.anc_ptr + Qd.Jc]];
      R.pm[u] = Bp.m; R.prow[u] = Bp.row0; R.ppan[u] = Bp.chain_off;
      if constexpr (!ISREF) for (int i = 0; i < Bp.m && i < 32; ++i) put(Bp.row0 + i, R.px[u][i], R.py[u][i], R.pmv[u][i], R.pw[u][i]);
    }
    for (int b = 0; b < G.nblk && b < Rec::NB; ++b) {
      const Blk &Bb = t.blks[G.blk0 + b];
      R.bpan[u][b] = Bb.panel_off; R.brow[u][b] = Bb.row0; R.bld[u][b] = Bb.ld;
    }
    int bi = 0;
    for (int i = 0; i < G.M && i < 32; ++i) {
      put(G.row0 + i, R.colx[u][i], R.coly[u][i], R.colmv[u][i], R.colw[u][i]);
      if constexpr (!ISREF) {
        while (bi + 1 < G.nblk && G.row0 + i >= t.blks[G.blk0 + bi + 1].row0) ++bi;
        R.colblk[u][i] = bi;
      }
    }
  }
  std::memcpy(out, &R, sizeof(R));
}
// the records of `count` quads from quads[qfirst] on (their groups from grp_first on), appended to qrec; returns their offset
static long long append_quad_records(const st_problem *pb, TreeLayout &t, int grp_first, int qfirst, int count, int nkx, bool isref, int &words) {
  words = quad_rec_words(nkx, isref);
  const long long off = (long long)t.qrec.size();
  t.qrec.resize(t.qrec.size() + (size_t)count * words);
  for (int k = 0; k < count; ++k) {
    long long *out = t.qrec.data() + off + (size_t)k * words;
    const Quad &Qd = t.quads[qfirst + k];
#define QR(P_) (isref ? fill_quad_record<P_, true>(pb, t, grp_first, Qd, out) : fill_quad_record<P_, false>(pb, t, grp_first, Qd, out))
    if (nkx == 32) QR(128); else if (nkx == 38) QR(152); else if (nkx == 44) QR(176); else QR(200);
#undef QR
  }
  return off;
}
// Quad records of every level that takes k_factor_quad (this rank's run of its quads: a launch's workgroup i starts from
// record i) and of the prediction quads.  After demote_by_static_lds: q_nkx / pred_nkx are final.
static void build_quad_records(const st_problem *pb, TreeLayout &t) {
  t.qrec.clear(); t.pred_qr_off = -1; t.pred_qr_words = 0;
  for (auto &L : t.levels) {
    L.qr_off = -1; L.qr_words = 0;
    if (t.sw.factor_gen != 3 || !L.fast || L.q_nkx == 0 || L.qown_n == 0) continue;
    L.qr_off = append_quad_records(pb, t, L.grp_first, L.quad_first + L.qown_lo, L.qown_n, L.q_nkx, L.isref != 0, L.qr_words);
  }
  if (t.pred_nkx && t.pred_quad_count > 0)
    t.pred_qr_off = append_quad_records(pb, t, t.pred_grp_first, t.pred_quad_first, t.pred_quad_count, t.pred_nkx, false, t.pred_qr_words);
  t.qrec_bytes = t.qrec.size() * sizeof(long long);
}
// top levels that st_factor_begin may run ahead: the leading levels on k_factor_mfma (no global scratch), when every
// level of the tree is on the column-group path (the generic kernels share one scratch arena between phases)
static void choose_top_levels(TreeLayout &t) {
  const int n_actual = t.n_actual_groups;
  t.g_top = 0;
  bool all_fast = !t.limited && !t.force_generic;
  for (int g = 0; g < n_actual; ++g) all_fast = all_fast && t.levels[g].fast;
  if (all_fast) {
    while (t.g_top < n_actual && !(t.sw.factor_gen == 3 && t.levels[t.g_top].q_nkx > 0)) ++t.g_top;
    if (t.g_top >= n_actual) t.g_top = 0;   // nothing would be left for the main stream to hide it under
  }
  for (int b : t.own_obs_list) if (t.blks[b].level < t.g_top) t.top_list.push_back(b);
  t.n_toplist = (int)t.top_list.size();
}

int layout_levels(const st_problem *pb, const Switches &sw, const DeviceLimits &dl, TreeLayout &t, std::string &msg) {
  t.sw = sw;
  t.sm_count = dl.sm_count;
  t.lds_limit = std::min(dl.lds_limit, DeviceLimits::CU_LDS);
  // limited_tree: k_marginal_invchol keeps K_uu and its inverse factor of a reference block in LDS (2 m^2 doubles: 101 rows
  // at 160 KB).  Refused here: at launch the runtime would only answer "invalid argument" from inside st_factor
  if (t.limited && (size_t)2 * t.twin_maxM * t.twin_maxM * sizeof(double) > t.lds_limit) {
    const int lim = (int)std::floor(std::sqrt((double)t.lds_limit / (2.0 * sizeof(double))));
    return refuse(msg, ST_ERR_UNSUPPORTED, "limited_tree: a reference block of " + std::to_string(t.twin_maxM) + " rows is wider than the " +
                  std::to_string(lim) + " rows whose marginal factor fits the LDS (k_marginal_invchol keeps 2 m^2 doubles)");
  }
  if (int rc = build_levels(pb, t, msg)) return rc;
  if (int rc = link_children(t, msg)) return rc;
  for (int g = 0; g < t.n_actual_groups; ++g) {
    LevelInfo &L = t.levels[g];
    if (int rc = level_own_runs(t, L, g, msg)) return rc;
    level_wide_groups(t, L);     // before demote_by_static_lds, on purpose: see there
    level_lchain_slabs(t, L);
    level_quads(t, L, g);
  }
  mark_owned(t);
  if (int rc = build_prediction(t, msg)) return rc;
  for (long long r = 0; r < t.n_all; ++r)
    if (pb->mv_id[r] < 1 || pb->mv_id[r] > pb->q) return refuse(msg, ST_ERR_USAGE, "mv_id out of range");
  std::vector<long long> blk2grp((size_t)t.n_blocks, -1);   // the group that holds a block (its first block holds the group's record)
  for (size_t g = 0; g < t.grps.size(); ++g)
    for (int b = 0; b < t.grps[g].nblk; ++b) blk2grp[t.grps[g].blk0 + b] = (long long)g;
  if (int rc = pack_group_descriptors(t, blk2grp, msg)) return rc;
  choose_gram_direct(t, blk2grp);
  size_buffers(t);
  demote_by_static_lds(t, dl);
  build_quad_records(pb, t);
  choose_top_levels(t);
  return ST_OK;
}
