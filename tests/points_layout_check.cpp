// points_layout_check -- a stand-alone CPU program: builds the launch structures of a set of new points
// (spamtree_amd/csrc/points_layout.cpp) on the tree layout of a problem and checks, with plain loops, what k_points_* and
// k_points_joint_* assume of them.  It rebuilds nothing with the code under test: every check reads the finished PointsLayout,
// the TreeLayout and the caller's arrays.  Prints "OK key=value ..." or the first violated invariant (exit status 1); a refusal
// of the layout prints "REFUSED <code> <message>" (exit status 2).
//
//   points_layout_check PROBLEM POINTS LDS_LIMIT [force-generic] [limited] [world2] [move-col]
//
// PROBLEM: the problem as tests/test_tree_layout_cpu.py writes it.  POINTS: 2 int64 (n_new, joint: 0 / 1), then coords (2 n_new
// doubles, column-major), mv, anchor and joint_id, each an int64 count followed by that many 8-byte values (count 0: a null
// pointer).  LDS_LIMIT: the device's dynamic LDS per workgroup in bytes.  move-col: the negative case, the first member column of
// a joint tile moved into the neighbouring slot after the layout is built -- the checks must name it.
#include <cstdarg>
#include <unordered_map>

#include "points_layout.hpp"

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
struct Points {
  int64_t n_new = 0, joint = 0;
  std::vector<int64_t> arr[4];    // coords (raw words), mv, anchor, joint_id
  const double *coords() const { return arr[0].empty() ? nullptr : (const double *)arr[0].data(); }
  const int64_t *ip(int a) const { return arr[a].empty() ? nullptr : arr[a].data(); }
};

static bool read_arrays(FILE *f, std::vector<int64_t> *arr, int count) {
  bool ok = true;
  for (int a = 0; ok && a < count; ++a) {
    int64_t cnt = 0;
    ok = fread(&cnt, 8, 1, f) == 1 && cnt >= 0 && cnt < (1LL << 32);
    if (ok) { arr[a].resize((size_t)cnt); ok = fread(arr[a].data(), 8, (size_t)cnt, f) == (size_t)cnt; }
  }
  return ok;
}

static bool read_problem(const char *path, Problem &P) {
  FILE *f = fopen(path, "rb");
  if (!f) return false;
  const bool ok = fread(P.head, 8, 6, f) == 6 && read_arrays(f, P.arr, 13);
  fclose(f);
  if (!ok) return false;
  auto dp = [&](int a) { return P.arr[a].empty() ? nullptr : (const double *)P.arr[a].data(); };
  auto ip = [&](int a) { return P.arr[a].empty() ? nullptr : P.arr[a].data(); };
  P.pb = st_problem{P.head[0], (int32_t)P.head[1], (int32_t)P.head[2], (int32_t)P.head[3], (int32_t)P.head[4], P.head[5],
                    dp(0), dp(1), dp(2), ip(3), ip(4), ip(5), ip(6), ip(7), ip(8), ip(9), ip(10), ip(11), ip(12)};
  return true;
}

static bool read_points(const char *path, Points &Q) {
  FILE *f = fopen(path, "rb");
  if (!f) return false;
  int64_t head[2];
  const bool ok = fread(head, 8, 2, f) == 2 && read_arrays(f, Q.arr, 4);
  fclose(f);
  Q.n_new = head[0]; Q.joint = head[1];
  return ok;
}

// the rule of the kernel classes: 0 k_points_mfma<128>, 1 <256>, 2 generic
static int class_rule(const TreeLayout &t, const PtChain &C) {
  const bool generic = t.force_generic || C.rows > 256 || (C.rows > 128 && PP_LDS_BYTES(256) > t.lds_limit) || C.nblk > PP_MAXB;
  return generic ? 2 : (C.rows <= 128 ? 0 : 1);
}
static int chain_end(const PointsLayout &L, int c) { const PtChain &C = L.chains[c]; return C.nblk ? L.chain_blk[C.first + C.nblk - 1] : -1; }

struct Report {
  long long ref_anchors = 0, nonref_anchors = 0, mixed_chains = 0, multi_tile_chains = 0, max_chain_rows = 0, min_chain_rows = 1 << 30;
  long long padded_slots = 0, full_slots = 0, tiles4 = 0, max_g = 0;
};

static void check_chains(const TreeLayout &t, const Points &Q, const PointsLayout &L, Report &R) {
  const int nc = (int)L.chains.size();
  REQUIRE(L.n_chains == nc && nc >= 1, "chains: n_chains is %d, the list has %d", L.n_chains, nc);
  int at = 0;
  for (int c = 0; c < nc; ++c) {
    const PtChain &C = L.chains[c];
    REQUIRE(C.first == at && C.nblk >= 0 && (size_t)at + C.nblk <= L.chain_blk.size(), "chains: chain %d does not start where chain %d ends", c, c - 1);
    at += C.nblk;
    REQUIRE(c == 0 || chain_end(L, c) > chain_end(L, c - 1), "chains: chain %d does not end in a later block than chain %d", c, c - 1);
    if (C.nblk == 0) { REQUIRE(C.rows == 0, "chains: empty chain %d has %d rows", c, C.rows); continue; }
    const int r = chain_end(L, c);
    REQUIRE(r >= 0 && r < (int)t.n_blocks, "chains: chain %d ends in block %d", c, r);
    const Blk &B = t.blks[r];
    REQUIRE(B.isref && B.nobs > 0, "chains: chain %d ends in block %d, which is no observed reference block", c, r);
    REQUIRE(C.nblk == B.nanc + 1, "chains: chain %d has %d blocks, its end block has %d ancestors", c, C.nblk, B.nanc);
    for (int a = 0; a < B.nanc; ++a)
      REQUIRE(L.chain_blk[C.first + a] == t.anc_idx[B.anc_ptr + a], "chains: block %d of chain %d is not ancestor %d of its end block", a, c, a);
    REQUIRE(C.rows == B.P + B.m, "chains: chain %d has %d rows, P + m of its end block is %d", c, C.rows, B.P + B.m);
    R.max_chain_rows = std::max<long long>(R.max_chain_rows, C.rows);
    R.min_chain_rows = std::min<long long>(R.min_chain_rows, C.rows);
  }
  REQUIRE((size_t)at == L.chain_blk.size(), "chains: the chains hold %d blocks, chain_blk %zu", at, L.chain_blk.size());
  // every point's chain ends at its anchor (a reference block) or at the anchor's last parent
  std::vector<char> kinds(nc, 0);
  REQUIRE((int64_t)L.order.size() == Q.n_new && (int64_t)L.pt_chain.size() == Q.n_new, "order: order and pt_chain do not have n_new entries");
  for (int64_t s = 0; s < Q.n_new; ++s) {
    const int64_t i = L.order[s];
    const int c = L.pt_chain[s];
    REQUIRE(i >= 0 && i < Q.n_new, "order: entry %lld (%lld) is out of range", (long long)s, (long long)i);
    REQUIRE(c >= 0 && c < nc, "chains: sorted point %lld has chain %d", (long long)s, c);
    const int b = t.blk_model2dev[Q.ip(2)[i]];
    const Blk &B = t.blks[b];
    const int want = B.isref ? b : (B.nanc ? t.anc_idx[B.anc_ptr + B.nanc - 1] : -1);
    REQUIRE(chain_end(L, c) == want, "chains: point %lld is on a chain that ends in block %d, its anchor rule gives %d", (long long)i, chain_end(L, c), want);
    kinds[c] |= B.isref ? 1 : 2;
    if (B.isref) ++R.ref_anchors; else ++R.nonref_anchors;
  }
  for (int c = 0; c < nc; ++c) { REQUIRE(kinds[c] != 0, "chains: chain %d has no point", c); R.mixed_chains += kinds[c] == 3; }
}

static void check_order_and_tiles(const TreeLayout &t, const Points &Q, const PointsLayout &L, Report &R) {
  const int64_t n = Q.n_new;
  std::vector<char> seen(n, 0);
  for (int64_t s = 0; s < n; ++s) {
    const long long i = L.order[s];
    REQUIRE(!seen[i], "order: entry %lld (%lld) is repeated", (long long)s, i);
    seen[i] = 1;
    if (s == 0) continue;
    const int c0 = L.pt_chain[s - 1], c1 = L.pt_chain[s], k0 = class_rule(t, L.chains[c0]), k1 = class_rule(t, L.chains[c1]);
    REQUIRE(k0 < k1 || (k0 == k1 && (c0 < c1 || (c0 == c1 && L.order[s - 1] < i))), "order: sorted points %lld and %lld are not in (class, chain, caller index) order", (long long)s - 1, (long long)s);
  }
  REQUIRE((int)L.tiles.size() == L.ntile128 + L.ntile256, "tiles: %zu tiles, ntile128 + ntile256 = %d", L.tiles.size(), L.ntile128 + L.ntile256);
  int64_t at = 0;
  std::vector<int> tiles_of(L.chains.size(), 0);
  for (int k = 0; k < (int)L.tiles.size(); ++k) {
    const PtTile &T = L.tiles[k];
    REQUIRE(T.p0 == at, "tiles: tile %d starts at sorted point %d, the tiles before it end at %lld", k, T.p0, (long long)at);
    REQUIRE(T.np >= 1 && T.np <= PP_NCOL && at + T.np <= n, "tiles: tile %d has %d points", k, T.np);
    REQUIRE(T.chain >= 0 && T.chain < (int)L.chains.size(), "tiles: tile %d has chain %d", k, T.chain);
    for (int j = 0; j < T.np; ++j) REQUIRE(L.pt_chain[at + j] == T.chain, "tiles: tile %d straddles chains %d and %d", k, T.chain, L.pt_chain[at + j]);
    REQUIRE(class_rule(t, L.chains[T.chain]) == (k < L.ntile128 ? 0 : 1), "tiles: tile %d is launched with the wrong chain length (class %d)", k, class_rule(t, L.chains[T.chain]));
    if (++tiles_of[T.chain] == 2) ++R.multi_tile_chains;
    at += T.np;
  }
  REQUIRE((int64_t)L.gen.size() == n - at, "generic list: %zu entries, %lld sorted points follow the tiles", L.gen.size(), (long long)(n - at));
  long long maxrows = 1;
  for (size_t k = 0; k < L.gen.size(); ++k) {
    REQUIRE(L.gen[k] == at + (int64_t)k, "generic list: entry %zu is %d", k, L.gen[k]);
    const PtChain &C = L.chains[L.pt_chain[L.gen[k]]];
    REQUIRE(class_rule(t, C) == 2, "generic list: sorted point %d is on a chain of an MFMA class", L.gen[k]);
    maxrows = std::max<long long>(maxrows, C.rows);
  }
  REQUIRE(L.scratch_stride % 32 == 0 && L.scratch_stride >= maxrows, "scratch: stride %lld for generic chains of up to %lld rows", L.scratch_stride, maxrows);
  REQUIRE(L.grid_generic == (int)std::min<size_t>(L.gen.size(), (size_t)4 * t.sm_count), "generic list: grid of %d for %zu points", L.grid_generic, L.gen.size());
}

static void check_groups(const Points &Q, const PointsLayout &L, Report &R) {
  const int64_t n = Q.n_new, nj = L.n_joint;
  REQUIRE((int64_t)L.j_off.size() == nj + 1 && (int64_t)L.j_mptr.size() == nj + 1 && (int64_t)L.j_mem.size() == n, "joint groups: j_off, j_mptr or j_mem has the wrong length");
  REQUIRE(L.j_off[0] == 0 && L.j_mptr[0] == 0 && L.j_mptr[nj] == n && L.cov_total == L.j_off[nj], "joint groups: the offsets do not start at 0 or end at n_new / cov_total");
  if (n == 0) return;
  REQUIRE((int64_t)L.pt_grp.size() == n && (int64_t)L.pt_a.size() == n && (int64_t)L.groups.size() == nj, "joint groups: pt_grp, pt_a or groups has the wrong length");
  std::unordered_map<int64_t, int> label;
  std::vector<int64_t> pos(n);      // caller index -> sorted position
  for (int64_t s = 0; s < n; ++s) pos[L.order[s]] = s;
  for (int64_t i = 0; i < n; ++i) {
    auto it = label.find(Q.ip(3)[i]);
    if (it == label.end()) it = label.emplace(Q.ip(3)[i], (int)label.size()).first;
    REQUIRE(L.pt_grp[i] == it->second, "joint groups: point %lld is in group %d, its label is the %d-th to appear", (long long)i, L.pt_grp[i], it->second);
  }
  REQUIRE((int64_t)label.size() == nj, "joint groups: %zu labels, %lld groups", label.size(), (long long)nj);
  for (int64_t k = 0; k < nj; ++k) {
    const int64_t g = L.j_mptr[k + 1] - L.j_mptr[k];
    REQUIRE(g >= 1 && g <= PJ_MAXG, "joint groups: group %lld has %lld members", (long long)k, (long long)g);
    REQUIRE(L.j_off[k + 1] - L.j_off[k] == g * g, "joint groups: group %lld of %lld members takes %lld packed entries", (long long)k, (long long)g, (long long)(L.j_off[k + 1] - L.j_off[k]));
    const PtJoint &G = L.groups[k];
    REQUIRE(G.cov_off == L.j_off[k] && G.first == L.j_mptr[k] && G.g == g, "joint groups: record %lld does not repeat j_off / j_mptr", (long long)k);
    for (int64_t a = 0; a < g; ++a) {
      const int64_t i = L.j_mem[L.j_mptr[k] + a];
      REQUIRE(i >= 0 && i < n && (a == 0 || i > L.j_mem[L.j_mptr[k] + a - 1]), "joint groups: the members of group %lld are not in the caller's order", (long long)k);
      REQUIRE(L.pt_grp[i] == k && L.pt_a[i] == a, "joint groups: pt_grp / pt_a of point %lld do not invert the member list (group %lld, member %lld)", (long long)i, (long long)k, (long long)a);
      REQUIRE(L.pt_chain[pos[i]] == G.chain, "joint groups: member %lld of group %lld is on chain %d, the group on %d", (long long)a, (long long)k, L.pt_chain[pos[i]], G.chain);
    }
    R.max_g = std::max<long long>(R.max_g, g);
  }
}

static void check_packing(const TreeLayout &t, const PointsLayout &L, Report &R) {
  const int nj = (int)L.n_joint, nt = (int)L.jtiles.size();
  REQUIRE(nt == L.jtile128 + L.jtile256, "joint packing: %d tiles, jtile128 + jtile256 = %d", nt, L.jtile128 + L.jtile256);
  REQUIRE(L.jcols.size() == (nt ? (size_t)nt * PP_NCOL : 1), "joint packing: %zu columns for %d tiles", L.jcols.size(), nt);
  if (nt == 0) REQUIRE(L.jcols[0].a < 0, "joint packing: the dummy column is a member");
  std::vector<int> placed(nj, 0);
  for (int k = 0; k < nt; ++k) {
    const PtTile &T = L.jtiles[k];
    REQUIRE(T.chain >= 0 && T.chain < (int)L.chains.size() && class_rule(t, L.chains[T.chain]) == (k < L.jtile128 ? 0 : 1), "joint packing: tile %d is launched with the wrong chain length", k);
    REQUIRE(T.np >= 1 && T.np <= 4, "joint packing: tile %d has %d slots in use", k, T.np);
    R.tiles4 += T.np == 4;
    for (int sl = 0; sl < 4; ++sl) {
      const PtCol *col = L.jcols.data() + (size_t)k * PP_NCOL + sl * 16;
      int used = 0;
      for (int j = 0; j < 16;) {
        REQUIRE(col[j].grp >= 0 && col[j].grp < nj, "joint packing: tile %d slot %d column %d names group %d", k, sl, j, col[j].grp);
        if (col[j].a < 0) { ++j; continue; }
        const PtJoint &G = L.groups[col[j].grp];
        REQUIRE(col[j].a == 0, "joint packing: tile %d slot %d column %d is member %d of group %d, which does not start in the column before it", k, sl, j, col[j].a, col[j].grp);
        REQUIRE(j + G.g <= 16, "joint packing: group %d at tile %d slot %d column %d runs past the slot's 16 columns", col[j].grp, k, sl, j);
        for (int a = 0; a < G.g; ++a)
          REQUIRE(col[j + a].grp == col[j].grp && col[j + a].a == a, "joint packing: tile %d slot %d column %d is not member %d of group %d", k, sl, j + a, a, col[j].grp);
        REQUIRE(G.chain == T.chain, "joint packing: group %d of chain %d sits in tile %d of chain %d", col[j].grp, G.chain, k, T.chain);
        ++placed[col[j].grp];
        used += G.g; j += G.g;
      }
      REQUIRE((used > 0) == (sl < T.np), "joint packing: tile %d says %d slots are in use, slot %d holds %d members", k, T.np, sl, used);
      if (used == 16) ++R.full_slots; else if (used > 0) ++R.padded_slots;
    }
  }
  std::vector<int> listed(nj, 0);
  for (int k : L.jgen) { REQUIRE(k >= 0 && k < nj, "joint packing: the generic list names group %d", k); ++listed[k]; }
  for (int k = 0; k < nj; ++k) {
    const bool generic = class_rule(t, L.chains[L.groups[k].chain]) == 2;
    REQUIRE(placed[k] == (generic ? 0 : 1), "joint packing: group %d (%s chain) sits in %d slots", k, generic ? "generic" : "MFMA", placed[k]);
    REQUIRE(listed[k] == (generic ? 1 : 0), "joint packing: group %d (%s chain) is %d times in the generic list", k, generic ? "generic" : "MFMA", listed[k]);
  }
  REQUIRE(L.jgrid_generic == (int)std::min<size_t>(L.jgen.size(), (size_t)4 * t.sm_count), "joint packing: grid of %d for %zu generic groups", L.jgrid_generic, L.jgen.size());
}

// FNV-1a over every list and count of the layout (doubles by their bits): equal hashes before and after a restructuring
struct Hash {
  unsigned long long h = 1469598103934665603ULL;
  void bytes(const void *p, size_t n) { for (size_t i = 0; i < n; ++i) { h ^= ((const unsigned char *)p)[i]; h *= 1099511628211ULL; } }
  template <typename T> void val(T v) { bytes(&v, sizeof(v)); }
  template <typename T> void vec(const std::vector<T> &v) { val((long long)v.size()); if (!v.empty()) bytes(v.data(), v.size() * sizeof(T)); }
};
static unsigned long long layout_hash(const PointsLayout &L) {
  Hash H;
  H.vec(L.chains); H.vec(L.chain_blk); H.vec(L.order); H.vec(L.pt_chain); H.vec(L.tiles); H.vec(L.gen);
  H.val(L.ntile128); H.val(L.ntile256); H.val(L.grid_generic); H.val(L.n_chains); H.val(L.scratch_stride); H.val(L.alg_bytes); H.val(L.flops);
  H.vec(L.j_off); H.vec(L.j_mptr); H.vec(L.j_mem); H.vec(L.pt_grp); H.vec(L.pt_a); H.vec(L.groups); H.vec(L.jtiles); H.vec(L.jcols); H.vec(L.jgen);
  H.val(L.jtile128); H.val(L.jtile256); H.val(L.jgrid_generic); H.val(L.n_joint); H.val(L.cov_total); H.val(L.j_alg_bytes); H.val(L.j_flops);
  return H.h;
}

int main(int argc, char **argv) {
  if (argc < 4) { fprintf(stderr, "usage: points_layout_check PROBLEM POINTS LDS_LIMIT [force-generic] [limited] [world2] [move-col]\n"); return 3; }
  Problem P;
  Points Q;
  if (!read_problem(argv[1], P) || !read_points(argv[2], Q)) { fprintf(stderr, "points_layout_check: cannot read %s or %s\n", argv[1], argv[2]); return 3; }
  bool force_generic = false, limited = false, world2 = false, move_col = false;
  for (int a = 4; a < argc; ++a) {
    force_generic |= !strcmp(argv[a], "force-generic"); limited |= !strcmp(argv[a], "limited");
    world2 |= !strcmp(argv[a], "world2"); move_col |= !strcmp(argv[a], "move-col");
  }
  DeviceLimits dl;   // quad_static / lchain_static: the named fallbacks
  dl.lds_limit = (size_t)atoll(argv[3]); dl.sm_count = 256;
  dl.lchain_no_scratch[0] = dl.lchain_no_scratch[1] = true;
  st_options opt = {0, 1, 0, world2 ? 2 : 1, force_generic ? 1 : 0, limited ? 2 : 0};
  TreeLayout t;
  std::string msg;
  int rc = layout_order(&P.pb, &opt, t, msg);
  if (rc == ST_OK) rc = layout_levels(&P.pb, read_switches(), dl, t, msg);
  if (rc != ST_OK) { fprintf(stderr, "points_layout_check: the tree layout is refused: %s\n", msg.c_str()); return 3; }
  PointsLayout L;
  static const int64_t no_label = 0;   // a joint set without a point still passes a label array
  rc = points_layout(t, Q.n_new, Q.coords(), Q.ip(1), Q.ip(2), Q.joint ? (Q.ip(3) ? Q.ip(3) : &no_label) : nullptr, L, msg);
  if (rc != ST_OK) { printf("REFUSED %d %s\n", rc, msg.c_str()); return 2; }
  if (move_col) {
    size_t at = 0;      // the first column of a slot that a group of two or more members opens, and of a slot that has a right neighbour
    while (at + 16 < L.jcols.size() && !(at % PP_NCOL < 48 && L.jcols[at].a == 0 && L.groups[L.jcols[at].grp].g >= 2)) at += 16;
    REQUIRE(at + 16 < L.jcols.size(), "move-col: no slot of the set starts with a group of two or more members");
    std::swap(L.jcols[at], L.jcols[at + 16]);
  }
  Report R;
  if (Q.n_new > 0) {
    check_chains(t, Q, L, R);
    check_order_and_tiles(t, Q, L, R);
  } else {
    REQUIRE(L.chains.empty() && L.chain_blk.empty() && L.order.empty() && L.pt_chain.empty() && L.tiles.empty() && L.gen.empty() && L.groups.empty() &&
            L.jtiles.empty() && L.jcols.empty() && L.jgen.empty() && L.n_chains == 0 && L.ntile128 + L.ntile256 + L.grid_generic == 0 &&
            L.jtile128 + L.jtile256 + L.jgrid_generic == 0 && L.n_joint == 0, "empty set: the layout is not empty");
    REQUIRE(Q.joint ? (L.j_off == std::vector<int64_t>{0} && L.j_mptr == std::vector<int64_t>{0}) : (L.j_off.empty() && L.j_mptr.empty()), "empty set: j_off / j_mptr are not {0} (joint) or empty");
  }
  if (Q.joint) {
    check_groups(Q, L, R);
    if (Q.n_new > 0) check_packing(t, L, R);
  } else {
    REQUIRE(L.j_off.empty() && L.j_mptr.empty() && L.j_mem.empty() && L.pt_grp.empty() && L.groups.empty() && L.jtiles.empty() && L.jcols.empty() && L.jgen.empty(),
            "plain set: it carries joint lists");
  }
  printf("OK n=%lld chains=%d min_chain_rows=%lld max_chain_rows=%lld ntile128=%d ntile256=%d gen=%zu grid_generic=%d multi_tile_chains=%lld "
         "ref_anchors=%lld nonref_anchors=%lld mixed_chains=%lld groups=%lld max_g=%lld jtile128=%d jtile256=%d jgen=%zu padded_slots=%lld "
         "full_slots=%lld tiles4=%lld cov_total=%lld hash=%llu\n",
         (long long)Q.n_new, L.n_chains, Q.n_new ? R.min_chain_rows : 0, R.max_chain_rows, L.ntile128, L.ntile256, L.gen.size(), L.grid_generic, R.multi_tile_chains,
         R.ref_anchors, R.nonref_anchors, R.mixed_chains, L.n_joint, R.max_g, L.jtile128, L.jtile256, L.jgen.size(), R.padded_slots,
         R.full_slots, R.tiles4, L.cov_total, layout_hash(L));
  return 0;
}
