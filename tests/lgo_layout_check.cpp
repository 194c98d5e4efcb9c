// lgo_layout_check -- a stand-alone CPU program: builds the group structures of st_rows_loo_groups_* (spamtree_amd/csrc/lgo_layout.cpp)
// on the tree layout of a problem and a file of labels and checks, with plain loops, what the pair part of k_loo_block and
// k_lgo_groups assume of them.  It rebuilds nothing with the code under test: every check reads the finished LgoLayout, the
// LooLayout and the TreeLayout.  Prints "OK key=value ..." or the first violated invariant (exit status 1); a refusal of either
// layout prints "REFUSED <code> <message>" (exit status 2).
//
//   lgo_layout_check PROBLEM LABELS [force-generic] [limited] [world2] [swap-pair] [drop-finish] [double-finish]
//
// PROBLEM: the problem as tests/test_tree_layout_cpu.py writes it.  LABELS: n_all int64 values, model row order.  swap-pair,
// drop-finish, double-finish: the negative cases -- after the layout is built, the first two pairs of the first child block with
// two inherited pairs are swapped / the first finishing slot is taken away / given to a second pair; the checks must name it.
#include <cstdarg>
#include <set>

#include "lgo_layout.hpp"

[[noreturn]] static void violated(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  printf("VIOLATED ");
  vprintf(fmt, ap);
  printf("\n");
  va_end(ap);
  exit(1);
}
#define REQUIRE(cond, ...) do { if (!(cond)) violated(__VA_ARGS__); } while (0)

struct Problem {
  int64_t head[6];
  std::vector<int64_t> arr[13];   // y, X, coords as raw 8-byte words
  st_problem pb;
};

static bool read_problem(const char *path, Problem &P) {
  FILE *f = fopen(path, "rb");
  if (!f) return false;
  bool ok = fread(P.head, 8, 6, f) == 6;
  for (int a = 0; ok && a < 13; ++a) {
    int64_t cnt = 0;
    ok = fread(&cnt, 8, 1, f) == 1 && cnt >= 0 && cnt < (1LL << 32);
    if (ok) { P.arr[a].resize((size_t)cnt); ok = fread(P.arr[a].data(), 8, (size_t)cnt, f) == (size_t)cnt; }
  }
  fclose(f);
  if (!ok) return false;
  auto dp = [&](int a) { return P.arr[a].empty() ? nullptr : (const double *)P.arr[a].data(); };
  auto ip = [&](int a) { return P.arr[a].empty() ? nullptr : P.arr[a].data(); };
  P.pb = st_problem{P.head[0], (int32_t)P.head[1], (int32_t)P.head[2], (int32_t)P.head[3], (int32_t)P.head[4], P.head[5],
                    dp(0), dp(1), dp(2), ip(3), ip(4), ip(5), ip(6), ip(7), ip(8), ip(9), ip(10), ip(11), ip(12)};
  return true;
}

int main(int argc, char **argv) {
  if (argc < 3) { fprintf(stderr, "usage: lgo_layout_check PROBLEM LABELS [force-generic] [limited] [world2] [swap-pair] [drop-finish] [double-finish]\n"); return 3; }
  Problem P;
  if (!read_problem(argv[1], P)) { fprintf(stderr, "lgo_layout_check: cannot read %s\n", argv[1]); return 3; }
  bool force_generic = false, limited = false, world2 = false, swap_pair = false, drop_finish = false, double_finish = false;
  for (int a = 3; a < argc; ++a) {
    force_generic |= !strcmp(argv[a], "force-generic"); limited |= !strcmp(argv[a], "limited"); world2 |= !strcmp(argv[a], "world2");
    swap_pair |= !strcmp(argv[a], "swap-pair"); drop_finish |= !strcmp(argv[a], "drop-finish"); double_finish |= !strcmp(argv[a], "double-finish");
  }
  DeviceLimits dl;
  dl.lds_limit = 160 * 1024; dl.sm_count = 256;
  dl.lchain_no_scratch[0] = dl.lchain_no_scratch[1] = true;
  st_options opt = {0, 1, 0, world2 ? 2 : 1, force_generic ? 1 : 0, limited ? 2 : 0};
  TreeLayout t;
  std::string msg;
  int rc = layout_order(&P.pb, &opt, t, msg);
  if (rc == ST_OK) rc = layout_levels(&P.pb, read_switches(), dl, t, msg);
  if (rc != ST_OK) { fprintf(stderr, "lgo_layout_check: the tree layout is refused: %s\n", msg.c_str()); return 3; }
  const long long n = t.n_all;
  std::vector<long long> labels((size_t)n);
  {
    FILE *f = fopen(argv[2], "rb");
    const bool ok = f && fread(labels.data(), 8, (size_t)n, f) == (size_t)n;
    if (f) fclose(f);
    if (!ok) { fprintf(stderr, "lgo_layout_check: cannot read %lld labels from %s\n", n, argv[2]); return 3; }
  }
  std::vector<unsigned char> obs((size_t)n);
  for (long long r = 0; r < n; ++r) obs[(size_t)t.model2dev[r]] = !std::isnan(P.pb.y[r]);
  LooLayout L;
  rc = loo_layout(t, L, msg);
  if (rc != ST_OK) { printf("REFUSED %d %s\n", rc, msg.c_str()); return 2; }
  LgoLayout G;
  rc = lgo_layout(t, L, labels.data(), obs.data(), G, msg);
  if (rc != ST_OK) { printf("REFUSED %d %s\n", rc, msg.c_str()); return 2; }
  const int nb = (int)t.n_blocks;
  if (swap_pair) {
    int c = -1;
    for (int u = 0; u < nb && c < 0; ++u)
      for (int j = L.ch_ptr[u]; j < L.ch_ptr[u + 1] && c < 0; ++j)
        if (G.pr_ptr[u + 1] - G.pr_ptr[u] >= 2) c = L.ch_idx[j];
    REQUIRE(c >= 0, "swap-pair: no child inherits two pairs");
    std::swap(G.pr_a[G.pr_ptr[c]], G.pr_a[G.pr_ptr[c] + 1]); std::swap(G.pr_b[G.pr_ptr[c]], G.pr_b[G.pr_ptr[c] + 1]);
  }
  if (drop_finish || double_finish) {
    size_t k = 0;
    while (k < G.pr_fin.size() && G.pr_fin[k] < 0) ++k;
    REQUIRE(k < G.pr_fin.size(), "drop-finish: no pair finishes");
    if (drop_finish) G.pr_fin[k] = -1;
    else {
      size_t k2 = 0;
      while (k2 < G.pr_fin.size() && (k2 == k || G.pr_fin[k2] >= 0)) ++k2;
      REQUIRE(k2 < G.pr_fin.size(), "double-finish: every pair slot finishes");
      G.pr_fin[k2] = G.pr_fin[k];
    }
  }

  // 1. the groups: labels ascending, members ascending model rows of the density, every labelled row of the density once
  const long long ng = G.n_groups;
  REQUIRE((long long)G.label.size() == ng && (long long)G.grp_ptr.size() == ng + 1 && (long long)G.gp_ptr.size() == ng + 1, "groups: sizes");
  REQUIRE(G.grp_ptr[0] == 0 && G.grp_ptr[ng] == G.n_members && (long long)G.mem_row.size() == G.n_members && (long long)G.mem_model.size() == G.n_members, "groups: members");
  std::vector<int> gid((size_t)n, -1), mi((size_t)n, -1), blk_of((size_t)n, -1);   // per device row
  for (int b = 0; b < nb; ++b)
    for (int i = 0; i < t.blks[b].m; ++i) blk_of[(size_t)(t.blks[b].row0 + i)] = b;
  long long max_members = 0, spans_max = 0;
  for (long long g = 0; g < ng; ++g) {
    REQUIRE(g == 0 || G.label[g] > G.label[g - 1], "groups: labels not ascending at group %lld", g);
    const int a = G.grp_ptr[g], b = G.grp_ptr[g + 1], gm = b - a;
    REQUIRE(gm >= 1 && gm <= LGO_MAX_MEMBERS, "groups: group %lld has %d members", g, gm);
    REQUIRE(G.gp_ptr[g + 1] - G.gp_ptr[g] == gm * (gm - 1) / 2, "groups: group %lld's pair table has the wrong size", g);
    max_members = std::max<long long>(max_members, gm);
    bool any = false;
    std::set<int> blocks;
    for (int k = a; k < b; ++k) {
      const long long r = G.mem_model[k], dr = G.mem_row[k];
      REQUIRE(r >= 0 && r < n && t.model2dev[r] == dr, "groups: member %d of group %lld: rows do not match", k - a, g);
      REQUIRE(k == a || r > G.mem_model[k - 1], "groups: group %lld's members are not ascending", g);
      REQUIRE(labels[r] == G.label[g], "groups: row %lld has label %lld, its group %lld", r, labels[r], G.label[g]);
      REQUIRE(L.voff[blk_of[(size_t)dr]] >= 0, "groups: row %lld lies in a prediction block", r);
      REQUIRE(gid[(size_t)dr] < 0, "groups: row %lld is a member twice", r);
      gid[(size_t)dr] = (int)g; mi[(size_t)dr] = k - a;
      any |= obs[(size_t)dr] != 0;
      blocks.insert(blk_of[(size_t)dr]);
    }
    REQUIRE(any, "groups: group %lld has no observed member", g);
    spans_max = std::max<long long>(spans_max, (long long)blocks.size());
  }
  for (long long r = 0; r < n; ++r) {
    const long long dr = t.model2dev[r];
    const bool want = labels[r] >= 0 && L.voff[blk_of[(size_t)dr]] >= 0;
    REQUIRE((gid[(size_t)dr] >= 0) == want, "groups: row %lld (label %lld) is %s", r, labels[r], want ? "in no group" : "in a group");
  }
  // 2. the pair lists: in range, sorted by (b, a), same group, no structural zero, and complete
  REQUIRE((int)G.pr_ptr.size() == nb + 1 && G.pr_ptr[0] == 0 && (size_t)G.pr_ptr[nb] == G.pr_a.size() && G.pr_a.size() == G.pr_b.size() &&
          G.pr_a.size() == G.pr_fin.size(), "pairs: pr_ptr does not span the lists");
  std::vector<std::vector<long long>> cols(nb);
  long long blocks_with = 0, blocks_without = 0;
  for (int b = 0; b < nb; ++b) {
    const Blk &B = t.blks[b];
    const int p0 = G.pr_ptr[b], np = G.pr_ptr[b + 1] - p0;
    REQUIRE(np >= 0, "pairs: pr_ptr decreases at block %d", b);
    if (L.voff[b] < 0) { REQUIRE(np == 0, "pairs: prediction block %d has pairs", b); continue; }
    (np ? blocks_with : blocks_without) += 1;
    for (int a = 0; a < B.nanc; ++a) {
      const Blk &U = t.blks[t.anc_idx[B.anc_ptr + a]];
      for (int i = 0; i < U.m; ++i) cols[b].push_back(U.row0 + i);
    }
    for (int i = 0; i < B.m; ++i) cols[b].push_back(B.row0 + i);
    const int len = B.P + B.m;
    REQUIRE((int)cols[b].size() == len, "pairs: block %d's columns", b);
    long long want = 0;
    for (int cb = 0; cb < len; ++cb)
      for (int ca = 0; ca < cb; ++ca)
        want += gid[(size_t)cols[b][ca]] >= 0 && gid[(size_t)cols[b][ca]] == gid[(size_t)cols[b][cb]] && (B.isref || ca < B.P);
    REQUIRE(want == np, "pairs: block %d lists %d pairs, its columns hold %lld", b, np, want);
    for (int k = 0; k < np; ++k) {
      const int ca = G.pr_a[p0 + k], cb = G.pr_b[p0 + k];
      REQUIRE(0 <= ca && ca < cb && cb < len, "pairs: block %d pair %d = (%d, %d) out of range", b, k, ca, cb);
      REQUIRE(gid[(size_t)cols[b][ca]] >= 0 && gid[(size_t)cols[b][ca]] == gid[(size_t)cols[b][cb]], "pairs: block %d pair %d joins two groups", b, k);
      REQUIRE(B.isref || ca < B.P, "pairs: block %d pair %d is a structural zero", b, k);
      REQUIRE(k == 0 || cb > G.pr_b[p0 + k - 1] || (cb == G.pr_b[p0 + k - 1] && ca > G.pr_a[p0 + k - 1]), "pairs: block %d is not sorted by (b, a) at pair %d", b, k);
      REQUIRE((G.pr_fin[p0 + k] >= 0) == (cb >= B.P), "pairs: block %d pair %d (%d, %d), P = %d: finishing slot %d", b, k, ca, cb, B.P, G.pr_fin[p0 + k]);
    }
  }
  // 3. the prefix property on every parent / child edge
  long long edges = 0;
  for (int u = 0; u < nb; ++u)
    for (int j = L.ch_ptr[u]; j < L.ch_ptr[u + 1]; ++j) {
      const int c = L.ch_idx[j];
      const int pu = G.pr_ptr[u], npu = G.pr_ptr[u + 1] - pu, pc = G.pr_ptr[c], npc = G.pr_ptr[c + 1] - pc;
      REQUIRE(npc >= npu, "prefix: child %d has %d pairs, its parent %d has %d", c, npc, u, npu);
      for (int k = 0; k < npu; ++k)
        REQUIRE(G.pr_a[pc + k] == G.pr_a[pu + k] && G.pr_b[pc + k] == G.pr_b[pu + k], "prefix: pair %d of child %d is (%d, %d), of its parent %d (%d, %d)",
                k, c, G.pr_a[pc + k], G.pr_b[pc + k], u, G.pr_a[pu + k], G.pr_b[pu + k]);
      REQUIRE(npc == npu || G.pr_b[pc + npu] >= t.blks[c].P, "prefix: child %d's pair %d lies in its chain and is not its parent's", c, npu);
      ++edges;
    }
  // 4. every non-structural member pair has exactly one finishing block, and the group's table names its slot
  std::vector<int> fin_count((size_t)std::max<long long>(G.n_pairs, 1), 0);
  std::vector<int> table(G.gp_idx.size(), -1);
  for (int b = 0; b < nb; ++b)
    for (int k = G.pr_ptr[b]; k < G.pr_ptr[b + 1]; ++k) {
      const int f = G.pr_fin[k];
      if (f < 0) continue;
      REQUIRE(f < G.n_pairs, "finish: slot %d of block %d outside the %lld slots", f, b, G.n_pairs);
      REQUIRE(fin_count[f] == 0, "finish: slot %d is written twice", f);
      fin_count[f] += 1;
      const long long ra = cols[b][G.pr_a[k]], rb = cols[b][G.pr_b[k]];
      const int g = gid[(size_t)ra], i = std::min(mi[(size_t)ra], mi[(size_t)rb]), j2 = std::max(mi[(size_t)ra], mi[(size_t)rb]);
      int &slot = table[(size_t)G.gp_ptr[g] + (size_t)j2 * (j2 - 1) / 2 + i];
      REQUIRE(slot < 0, "finish: members %d and %d of group %d finish in two blocks", i, j2, g);
      slot = f;
    }
  long long structural = 0, finished = 0;
  auto on_path = [&](int ba, int bb) {   // ba == bb or ba an ancestor of bb
    if (ba == bb) return true;
    const Blk &B = t.blks[bb];
    for (int a = 0; a < B.nanc; ++a) if (t.anc_idx[B.anc_ptr + a] == ba) return true;
    return false;
  };
  for (long long g = 0; g < ng; ++g) {
    const int a = G.grp_ptr[g], gm = G.grp_ptr[g + 1] - a;
    for (int j = 1; j < gm; ++j)
      for (int i = 0; i < j; ++i) {
        const int bi = blk_of[(size_t)G.mem_row[a + i]], bj = blk_of[(size_t)G.mem_row[a + j]];
        const bool zero = !(on_path(bi, bj) || on_path(bj, bi)) || (bi == bj && !t.blks[bi].isref);
        const size_t at = (size_t)G.gp_ptr[g] + (size_t)j * (j - 1) / 2 + i;
        REQUIRE(G.gp_idx[at] == table[at], "finish: group %lld members (%d, %d): the table says slot %d, the blocks write %d", g, i, j, G.gp_idx[at], table[at]);
        REQUIRE((table[at] >= 0) == !zero, "finish: group %lld members (%d, %d) are %s and have %s finishing block", g, i, j,
                zero ? "a structural zero" : "no structural zero", table[at] >= 0 ? "a" : "no");
        structural += zero; finished += !zero;
      }
  }
  REQUIRE(finished == G.n_pairs, "finish: %lld member pairs finish, the layout counts %lld", finished, G.n_pairs);
  // 5. the vectors with their pair part do not overlap and lie inside the arena
  std::vector<std::pair<long long, long long>> iv;
  for (int b = 0; b < nb; ++b) {
    REQUIRE((G.voff[b] >= 0) == (L.voff[b] >= 0), "vectors: block %d", b);
    if (G.voff[b] >= 0) iv.push_back({G.voff[b], G.voff[b] + 2ll * (t.blks[b].P + t.blks[b].m) + (G.pr_ptr[b + 1] - G.pr_ptr[b])});
  }
  std::sort(iv.begin(), iv.end());
  for (size_t k = 0; k < iv.size(); ++k) {
    REQUIRE(iv[k].first >= 0 && iv[k].second <= G.arena, "vectors: [%lld, %lld) leaves the arena of %lld", iv[k].first, iv[k].second, G.arena);
    REQUIRE(k == 0 || iv[k].first >= iv[k - 1].second, "vectors: [%lld, %lld) overlaps [%lld, %lld)", iv[k].first, iv[k].second, iv[k - 1].first, iv[k - 1].second);
  }
  REQUIRE(G.arena == L.arena + G.n_pair_slots && G.n_pair_slots == (long long)G.pr_a.size(), "vectors: the arena grows by %lld, the pair slots are %lld",
          G.arena - L.arena, G.n_pair_slots);
  printf("OK groups=%lld members=%lld max_members=%lld max_blocks_spanned=%lld pairs=%lld structural_zeros=%lld pair_slots=%lld blocks_with_pairs=%lld "
         "blocks_without_pairs=%lld edges=%lld\n", ng, G.n_members, max_members, spans_max, G.n_pairs, structural, G.n_pair_slots, blocks_with,
         blocks_without, edges);
  return 0;
}
