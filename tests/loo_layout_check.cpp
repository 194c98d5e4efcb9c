// loo_layout_check -- a stand-alone CPU program: builds the launch structures of st_rows_loo_* (spamtree_amd/csrc/loo_layout.cpp)
// on the tree layout of a problem and checks, with plain loops, what k_loo_block assumes of them.  It rebuilds nothing with the
// code under test: every check reads the finished LooLayout and the TreeLayout.  Prints "OK key=value ..." or the first violated
// invariant (exit status 1); a refusal of the layout prints "REFUSED <code> <message>" (exit status 2).
//
//   loo_layout_check PROBLEM [force-generic] [limited] [world2] [overlap] [drop-child]
//
// PROBLEM: the problem as tests/test_tree_layout_cpu.py writes it.  overlap, drop-child: the negative cases -- after the layout is
// built, the second block's vector is moved onto the first one's / the last child of the first parent is taken off its list; the
// checks must name it.
#include <cstdarg>

#include "loo_layout.hpp"

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
  if (argc < 2) { fprintf(stderr, "usage: loo_layout_check PROBLEM [force-generic] [limited] [world2] [overlap] [drop-child]\n"); return 3; }
  Problem P;
  if (!read_problem(argv[1], P)) { fprintf(stderr, "loo_layout_check: cannot read %s\n", argv[1]); return 3; }
  bool force_generic = false, limited = false, world2 = false, overlap = false, drop_child = false;
  for (int a = 2; a < argc; ++a) {
    force_generic |= !strcmp(argv[a], "force-generic"); limited |= !strcmp(argv[a], "limited"); world2 |= !strcmp(argv[a], "world2");
    overlap |= !strcmp(argv[a], "overlap"); drop_child |= !strcmp(argv[a], "drop-child");
  }
  DeviceLimits dl;
  dl.lds_limit = 160 * 1024; dl.sm_count = 256;
  dl.lchain_no_scratch[0] = dl.lchain_no_scratch[1] = true;
  st_options opt = {0, 1, 0, world2 ? 2 : 1, force_generic ? 1 : 0, limited ? 2 : 0};
  TreeLayout t;
  std::string msg;
  int rc = layout_order(&P.pb, &opt, t, msg);
  if (rc == ST_OK) rc = layout_levels(&P.pb, read_switches(), dl, t, msg);
  if (rc != ST_OK) { fprintf(stderr, "loo_layout_check: the tree layout is refused: %s\n", msg.c_str()); return 3; }
  LooLayout L;
  rc = loo_layout(t, L, msg);
  if (rc != ST_OK) { printf("REFUSED %d %s\n", rc, msg.c_str()); return 2; }
  const int nb = (int)t.n_blocks;
  if (overlap) {
    REQUIRE(L.list.size() >= 2, "overlap: fewer than two blocks");
    L.voff[L.list[1]] = L.voff[L.list[0]];
  }
  if (drop_child) {
    int u = 0;
    while (u < nb && L.ch_ptr[u + 1] == L.ch_ptr[u]) ++u;
    REQUIRE(u < nb, "drop-child: no block has a child");
    L.ch_idx.erase(L.ch_idx.begin() + L.ch_ptr[u + 1] - 1);
    for (int b = u + 1; b <= nb; ++b) L.ch_ptr[b] -= 1;
  }

  // 1. every block of the density appears once, on its own level; the levels go from the deepest to the root
  REQUIRE((int)L.voff.size() == nb && (int)L.ch_ptr.size() == nb + 1, "sizes: voff / ch_ptr do not cover the %d blocks", nb);
  std::vector<int> seen(nb, 0);
  long long n_density = 0, rows = 0, max_len = 0, max_children = 0, n_prediction = 0;
  int at = 0, prev_level = INT_MAX;
  for (const LooLevel &V : L.levels) {
    REQUIRE(V.first == at && V.count > 0 && (size_t)at + V.count <= L.list.size(), "levels: level %d does not start where the one before ends", V.level);
    REQUIRE(V.level < prev_level, "levels: level %d does not lie above level %d", V.level, prev_level);
    prev_level = V.level;
    for (int k = 0; k < V.count; ++k) {
      const int b = L.list[at + k];
      REQUIRE(b >= 0 && b < nb, "levels: block id %d out of range", b);
      const Blk &B = t.blks[b];
      REQUIRE(k == 0 || b > L.list[at + k - 1], "levels: level %d is not ascending at entry %d", V.level, k);
      REQUIRE(B.level == V.level, "levels: block %d of level %d stands in level %d's list", b, B.level, V.level);
      REQUIRE(B.nobs > 0 && B.panel_off >= 0, "levels: block %d has no observed row", b);
      REQUIRE((B.isref != 0) == (V.isref != 0), "levels: block %d's kind differs from its level's", b);
      REQUIRE(B.P + B.m <= V.maxLen && B.m <= V.maxM, "levels: block %d exceeds its level's maxLen / maxM", b);
      seen[b] += 1;
      rows += B.m;
      max_len = std::max<long long>(max_len, B.P + B.m);
    }
    at += V.count;
  }
  REQUIRE((size_t)at == L.list.size(), "levels: the levels hold %d blocks, the list %zu", at, L.list.size());
  for (int b = 0; b < nb; ++b) {
    const bool in = t.blks[b].nobs > 0;
    REQUIRE(seen[b] == (in ? 1 : 0), "levels: block %d (%s) appears %d times", b, in ? "observed" : "prediction", seen[b]);
    REQUIRE((L.voff[b] >= 0) == in, "vectors: block %d (%s) has offset %lld", b, in ? "observed" : "prediction", L.voff[b]);
    n_density += in; n_prediction += !in;
  }
  // 2. the children lists partition the non-root blocks of the density; a child's prefix length equals its parent's vector length
  std::vector<int> child_of(nb, -1);
  REQUIRE(L.ch_ptr[0] == 0 && (size_t)L.ch_ptr[nb] == L.ch_idx.size(), "children: ch_ptr does not span ch_idx");
  for (int u = 0; u < nb; ++u) {
    REQUIRE(L.ch_ptr[u + 1] >= L.ch_ptr[u], "children: ch_ptr decreases at block %d", u);
    max_children = std::max<long long>(max_children, L.ch_ptr[u + 1] - L.ch_ptr[u]);
    for (int j = L.ch_ptr[u]; j < L.ch_ptr[u + 1]; ++j) {
      const int c = L.ch_idx[j];
      REQUIRE(c >= 0 && c < nb && seen[c] == 1, "children: child %d of block %d is no block of the density", c, u);
      REQUIRE(seen[u] == 1, "children: block %d has children and is outside the density", u);
      REQUIRE(j == L.ch_ptr[u] || c > L.ch_idx[j - 1], "children: the list of block %d is not ascending", u);
      REQUIRE(child_of[c] < 0, "children: block %d is a child of blocks %d and %d", c, child_of[c], u);
      child_of[c] = u;
      const Blk &C = t.blks[c], &U = t.blks[u];
      REQUIRE(C.nanc >= 1 && t.anc_idx[C.anc_ptr + C.nanc - 1] == u, "children: block %d's last parent is not block %d", c, u);
      REQUIRE(C.P == U.P + U.m, "children: child %d's prefix has %d entries, its parent %d's vector %d", c, C.P, u, U.P + U.m);
      REQUIRE(C.level > U.level, "children: child %d does not lie below its parent %d", c, u);
    }
  }
  for (int b = 0; b < nb; ++b)
    if (seen[b]) REQUIRE((child_of[b] >= 0) == (t.blks[b].nanc > 0), "children: block %d with %d ancestors is %s", b, t.blks[b].nanc,
                         child_of[b] >= 0 ? "on a list" : "on no list");
  // 3. the vectors do not overlap and lie inside the arena
  std::vector<std::pair<long long, long long>> iv;
  for (int b = 0; b < nb; ++b)
    if (seen[b]) iv.push_back({L.voff[b], L.voff[b] + 2ll * (t.blks[b].P + t.blks[b].m)});
  std::sort(iv.begin(), iv.end());
  for (size_t k = 0; k < iv.size(); ++k) {
    REQUIRE(iv[k].first >= 0 && iv[k].second <= L.arena, "vectors: [%lld, %lld) leaves the arena of %lld", iv[k].first, iv[k].second, L.arena);
    REQUIRE(k == 0 || iv[k].first >= iv[k - 1].second, "vectors: [%lld, %lld) overlaps [%lld, %lld)", iv[k].first, iv[k].second, iv[k - 1].first, iv[k - 1].second);
  }
  printf("OK blocks=%lld prediction_blocks=%lld levels=%zu rows=%lld max_len=%lld max_children=%lld arena=%lld ref_levels=%d leaf_levels=%d\n",
         n_density, n_prediction, L.levels.size(), rows, max_len, max_children, L.arena,
         (int)std::count_if(L.levels.begin(), L.levels.end(), [](const LooLevel &V) { return V.isref != 0; }),
         (int)std::count_if(L.levels.begin(), L.levels.end(), [](const LooLevel &V) { return V.isref == 0; }));
  return 0;
}
