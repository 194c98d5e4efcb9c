// layout_check -- a stand-alone CPU program: builds the launch structures of a problem (spamtree_amd/csrc/tree_layout.cpp) with
// the MI355X's limits and checks, with plain loops, what the kernels assume of them.  It rebuilds nothing: every check
// reads the finished TreeLayout.  Prints "OK key=value ..." or the first violated invariant (exit status 1); a refusal
// of the layout itself prints "REFUSED <code> <message>" (exit status 2).
//
//   layout_check FILE WORLD RANK [limited] [raise-group-m]
//
// FILE: the problem as tests/test_tree_layout_cpu.py writes it: 6 int64 (n_all, d, q, p, n_groups, n_blocks), then 13
// arrays in st_problem's order, each an int64 count followed by that many 8-byte values (count 0: a null pointer).
// The library's SPAMTREE_* switches are read from the environment.  raise-group-m: the negative case, one group's M
// raised by one after the layout is built -- the checks must name it.
#include <cstdarg>

#include "tree_layout.hpp"

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

static DeviceLimits mi355x() {
  DeviceLimits dl;   // quad_static / lchain_static: the named fallbacks
  dl.lds_limit = 160 * 1024; dl.sm_count = 256;
  dl.lchain_no_scratch[0] = dl.lchain_no_scratch[1] = true;
  return dl;
}

static int last_parent(const TreeLayout &t, const Blk &B) { return B.nanc ? t.anc_idx[B.anc_ptr + B.nanc - 1] : -1; }
static bool owns(const TreeLayout &t, int g, int blk) { return g < t.cut || t.blk_owner[blk] == t.rank; }

// [off, off + len) pieces must tile [0, total)
static void check_tiling(std::vector<std::pair<long long, long long>> pieces, size_t total, const char *what) {
  std::sort(pieces.begin(), pieces.end());
  long long at = 0;
  for (auto &pc : pieces) {
    REQUIRE(pc.first == at, "blocks: %s overlap or leave a gap at offset %lld (next piece starts at %lld)", what, at, pc.first);
    at += pc.second;
  }
  REQUIRE((size_t)at == total, "blocks: %s sum to %lld, not to the total %zu", what, at, total);
}

static void check_blocks(const TreeLayout &t) {
  const int nb = (int)t.n_blocks;
  long long row = 0;
  std::vector<char> seen(t.n_all, 0);
  std::vector<std::pair<long long, long long>> panels, records;
  for (int i = 0; i < nb; ++i) {
    const Blk &B = t.blks[i];
    REQUIRE(B.row0 == row && B.m >= 0, "blocks: block %d starts at row %lld, the blocks before it end at %lld", i, B.row0, row);
    for (int r = 0; r < B.m; ++r) {
      const long long mr = t.dev2model[row + r];
      REQUIRE(mr >= 0 && mr < t.n_all && !seen[mr] && t.model2dev[mr] == row + r, "blocks: device row %lld does not map to one model row", row + r);
      seen[mr] = 1;
    }
    row += B.m;
    REQUIRE(i == 0 || B.level >= t.blks[i - 1].level, "blocks: levels decrease at block %d", i);
    REQUIRE(t.blk_model2dev[B.model_id] == i, "blocks: blk_model2dev does not invert model_id at block %d", i);
    int P = 0;
    for (int a = 0; a < B.nanc; ++a) {
      const int anc = t.anc_idx[B.anc_ptr + a];
      REQUIRE(anc >= 0 && anc < i && t.blks[anc].level < B.level, "blocks: ancestor %d of block %d does not precede it", a, i);
      P += t.blks[anc].m;
    }
    REQUIRE(P == B.P, "blocks: P of block %d is %d, its ancestors have %d rows", i, B.P, P);
    REQUIRE(B.ld == B.P + (B.isref ? B.m : 1), "blocks: ld of block %d", i);
    if (B.nobs > 0) {
      panels.push_back({B.panel_off, (long long)B.m * B.ld});
      if (t.limited && B.isref) panels.push_back({B.chain_off, (long long)B.m * B.m});
      if (!t.limited) REQUIRE(B.chain_off == B.panel_off, "blocks: chain_off of block %d", i);
      records.push_back({B.acc_off, B.acc_len});
    } else REQUIRE(B.panel_off == -1 && B.acc_len == 0 && !B.isref, "blocks: unobserved block %d owns a panel, a record or is a reference block", i);
  }
  REQUIRE(row == t.n_all, "blocks: rows sum to %lld of %lld", row, t.n_all);
  check_tiling(panels, t.panel_total, "panels");
  check_tiling(records, t.acc_total, "records");
}

// the groups [first, first + count) partition `list` in order; returns nothing, stops at the first violation
static void check_groups(const TreeLayout &t, const int *list, int nlist, int first, int count, bool level_isref, const char *what, int g) {
  int pos = 0;
  for (int k = 0; k < count; ++k) {
    const Grp &G = t.grps[first + k];
    REQUIRE(pos < nlist && G.blk0 == list[pos], "column groups: %s %d group %d does not start where the previous one ends", what, g, k);
    REQUIRE(G.nblk >= 1 && G.nblk <= 32 && pos + G.nblk <= nlist, "column groups: %s %d group %d has %d blocks", what, g, k, G.nblk);
    const Blk &B0 = t.blks[G.blk0];
    REQUIRE(G.row0 == B0.row0 && G.P == B0.P, "column groups: %s %d group %d: row0 / P are not its first block's", what, g, k);
    REQUIRE(G.nblk == 1 || !level_isref, "column groups: %s %d group %d joins blocks of a reference level", what, g, k);
    int M = 0;
    for (int b = 0; b < G.nblk; ++b) {
      const Blk &B = t.blks[G.blk0 + b];
      REQUIRE(list[pos + b] == G.blk0 + b, "column groups: %s %d group %d: device ids are not consecutive", what, g, k);
      REQUIRE(B.row0 == G.row0 + M, "column groups: %s %d group %d: rows are not consecutive", what, g, k);
      REQUIRE(last_parent(t, B) == last_parent(t, B0), "column groups: %s %d group %d: blocks with different last parents", what, g, k);
      REQUIRE(G.nblk == 1 || !B.isref, "column groups: %s %d group %d joins a reference block", what, g, k);
      M += B.m;
    }
    REQUIRE(G.M == M, "column groups: %s %d group %d: M is %d, its blocks have %d rows", what, g, k, G.M, M);
    REQUIRE(G.M <= 32, "column groups: %s %d group %d has %d columns", what, g, k, G.M);
    pos += G.nblk;
  }
  REQUIRE(pos == nlist, "column groups: %s %d: the groups cover %d of %d blocks", what, g, pos, nlist);
}

// the quads [qfirst, qfirst + qcount) partition the groups [gfirst, gfirst + gcount) in order
static void check_quads(const TreeLayout &t, int gfirst, int gcount, int qfirst, int qcount, int g, const LevelInfo *L) {
  int pos = 0, lo = INT_MAX, hi = 0;
  for (int k = 0; k < qcount; ++k) {
    const Quad &Q = t.quads[qfirst + k];
    REQUIRE(Q.g0 == pos, "quads: level %d quad %d does not start where the previous one ends", g, k);
    REQUIRE(Q.nu >= 1 && Q.nu <= 4 && pos + Q.nu <= gcount, "quads: level %d quad %d has %d units", g, k, Q.nu);
    const Blk &B0 = t.blks[t.grps[gfirst + pos].blk0];
    REQUIRE(Q.Jc >= 0 && Q.Jc <= B0.nanc && Q.Jc >= B0.nanc - 1, "quads: level %d quad %d: Jc = %d of %d ancestors", g, k, Q.Jc, B0.nanc);
    int Pc = 0;
    for (int a = 0; a < Q.Jc; ++a) Pc += t.blks[t.anc_idx[B0.anc_ptr + a]].m;
    REQUIRE(Pc == Q.Pc, "quads: level %d quad %d: Pc is %d, the shared chain has %d rows", g, k, Q.Pc, Pc);
    for (int u = 0; u < Q.nu; ++u) {
      const int blk = t.grps[gfirst + pos + u].blk0;
      const Blk &B = t.blks[blk];
      REQUIRE(B.nanc >= Q.Jc && B.nanc <= Q.Jc + 1, "quads: level %d quad %d unit %d has %d ancestors, Jc = %d", g, k, u, B.nanc, Q.Jc);
      for (int a = 0; a < Q.Jc; ++a)
        REQUIRE(t.anc_idx[B.anc_ptr + a] == t.anc_idx[B0.anc_ptr + a], "quads: level %d quad %d unit %d does not share ancestor %d", g, k, u, a);
      if (L && g >= t.cut) REQUIRE(t.blk_owner[blk] == t.blk_owner[t.grps[gfirst + pos].blk0], "quads: level %d quad %d mixes owners", g, k);
    }
    if (L && owns(t, g, t.grps[gfirst + pos].blk0)) { lo = std::min(lo, k); hi = std::max(hi, k + 1); }
    pos += Q.nu;
  }
  REQUIRE(pos == gcount, "quads: level %d: the quads cover %d of %d groups", g, pos, gcount);
  if (!L) return;
  REQUIRE(L->qown_n == (lo < hi ? hi - lo : 0) && (lo >= hi || L->qown_lo == lo), "quads: level %d: [qown_lo, qown_lo + qown_n) is not this rank's run", g);
  for (int k = L->qown_lo; k < L->qown_lo + L->qown_n; ++k)
    REQUIRE(owns(t, g, t.grps[gfirst + t.quads[qfirst + k].g0].blk0), "quads: level %d: quad %d inside the own run belongs to another rank", g, k);
}

static void check_wide(const TreeLayout &t, const LevelInfo &L, int g) {
  int pos = 0;
  for (int k = 0; k < L.wide_count; ++k) {
    const WideGrp &W = t.wgrps[L.wide_first + k];
    REQUIRE(W.first == pos && W.count >= 1 && W.count <= WG_MAXB && pos + W.count <= L.own_n, "wide groups: level %d group %d: first %d count %d", g, k, W.first, W.count);
    const Blk &B0 = t.blks[t.lvl_list[L.first + L.own_lo + pos]];
    int N = 0;
    for (int b = 0; b < W.count; ++b) {
      const Blk &B = t.blks[t.lvl_list[L.first + L.own_lo + pos + b]];
      REQUIRE(B.row0 == B0.row0 + N, "wide groups: level %d group %d: rows are not contiguous", g, k);
      N += B.m;
    }
    REQUIRE(N <= WG_MAXN && N <= L.wide_maxN, "wide groups: level %d group %d has %d columns", g, k, N);
    pos += W.count;
  }
  REQUIRE(pos == L.own_n, "wide groups: level %d: the groups cover %d of the rank's %d blocks", g, pos, L.own_n);
}

static void check_lchain(const TreeLayout &t, const LevelInfo &L, int g) {
  int k = 0, pos = 0;   // slab, block of the own run
  long long vrun = 0;
  while (k < L.lc_count) {
    const LcSlab &S0 = t.lcslabs[L.lc_first + k];
    REQUIRE(pos < L.own_n && S0.blk0 == t.lvl_list[L.first + L.own_lo + pos], "lchain slabs: level %d slab %d does not start at the next block of the run", g, k);
    const Blk &B0 = t.blks[S0.blk0];
    int cols = 0;
    bool last = false;
    for (; k < L.lc_count && t.lcslabs[L.lc_first + k].blk0 == S0.blk0; ++k) {
      const LcSlab &S = t.lcslabs[L.lc_first + k];
      REQUIRE(!last, "lchain slabs: level %d slab %d follows a slab that is no multiple of 16 wide", g, k);
      REQUIRE(S.vcol0 == cols && S.ncol >= 1 && S.ncol <= 64, "lchain slabs: level %d slab %d: vcol0 %d ncol %d", g, k, S.vcol0, S.ncol);
      REQUIRE(S.row0 == B0.row0 + cols && S.pan0 == B0.panel_off + (long long)cols * B0.ld && S.ld == B0.ld, "lchain slabs: level %d slab %d: row0 / pan0 / ld disagree with block %d", g, k, S.blk0);
      REQUIRE(!L.lchain_ref || S.vs0 == vrun, "lchain slabs: level %d slab %d: vs0 is not its group's place in the V scratch", g, k);
      last = S.ncol % 16 != 0;
      cols += S.ncol;
    }
    int N = 0;   // the sibling group: consecutive blocks of the run, contiguous rows and panels, until its columns are used up
    while (N < cols) {
      REQUIRE(pos < L.own_n, "lchain slabs: level %d: the slabs of block %d reach past the rank's run", g, S0.blk0);
      const int b = t.lvl_list[L.first + L.own_lo + pos];
      const Blk &B = t.blks[b];
      REQUIRE(B.row0 == B0.row0 + N && B.panel_off == B0.panel_off + (long long)N * B0.ld && B.ld == B0.ld && B.P == B0.P,
              "lchain slabs: level %d: block %d does not continue the sibling group of block %d", g, b, S0.blk0);
      if (L.lchain_ref) {
        REQUIRE(t.rfvoff[L.rf_first + pos] == vrun, "lchain slabs: level %d: rfvoff of block %d is %lld, expected %lld", g, b, t.rfvoff[L.rf_first + pos], vrun);
        vrun += rf_vsize(B.P);
      }
      N += B.m; ++pos;
    }
    REQUIRE(N == cols, "lchain slabs: level %d: the slabs of block %d tile %d of its group's %d columns", g, S0.blk0, cols, N);
  }
  REQUIRE(pos == L.own_n, "lchain slabs: level %d: the slabs cover %d of the rank's %d blocks", g, pos, L.own_n);
  REQUIRE(!L.lchain_ref || (size_t)vrun <= t.vscr_need, "lchain slabs: level %d needs %lld doubles of V scratch, vscr_need is %zu", g, vrun, t.vscr_need);
}

static void check_descriptors(const TreeLayout &t) {
  REQUIRE(t.gd_stride % 2 == 0 && t.gd_stride >= 8 && t.gd_stride <= GD_MAXW, "group descriptors: stride %d", t.gd_stride);
  REQUIRE(t.gdesc.size() == std::max<size_t>(1, t.grps.size()) * t.gd_stride, "group descriptors: %zu words for %zu groups", t.gdesc.size(), t.grps.size());
  std::vector<long long> blk2grp(t.n_blocks, -1);
  for (size_t g = 0; g < t.grps.size(); ++g)
    for (int b = 0; b < t.grps[g].nblk; ++b) blk2grp[t.grps[g].blk0 + b] = (long long)g;
  auto lo = [](long long v) { return (int)(v & 0xffffffffLL); };
  auto hi = [](long long v) { return (int)(v >> 32); };
  for (size_t g = 0; g < t.grps.size(); ++g) {
    const Grp &G = t.grps[g];
    const Blk &B0 = t.blks[G.blk0];
    const long long *w = t.gdesc.data() + g * (size_t)t.gd_stride;
    const int nch = std::min(B0.ndch, 64);
    REQUIRE(8 + 4 * B0.nanc + 3 * G.nblk + 2 * nch <= t.gd_stride, "group descriptors: group %zu does not fit the stride", g);
    REQUIRE(w[0] == G.row0 && w[1] == B0.acc_off && lo(w[2]) == G.M && hi(w[2]) == G.P && lo(w[3]) == B0.nanc && hi(w[3]) == G.nblk &&
            lo(w[4]) == B0.isref && hi(w[4]) == B0.level && lo(w[5]) == nch && hi(w[5]) == (t.limited ? 0 : B0.acc_len) && lo(w[6]) == G.blk0,
            "group descriptors: head of group %zu differs from its Grp / Blk", g);
    long long ao = 0, aoff = 0;
    for (int a = 0; a < B0.nanc; ++a) {
      const Blk &Ba = t.blks[t.anc_idx[B0.anc_ptr + a]];
      const long long *q = w + 8 + 4 * a;
      REQUIRE(lo(q[0]) == Ba.m && hi(q[0]) == ao && q[1] == Ba.row0 && q[2] == Ba.chain_off && q[3] == aoff, "group descriptors: ancestor %d of group %zu", a, g);
      ao += Ba.m; aoff += (long long)Ba.m * Ba.m + Ba.m;
    }
    REQUIRE(w[7] == aoff, "group descriptors: record length of group %zu", g);
    for (int b = 0; b < G.nblk; ++b) {
      const Blk &Bb = t.blks[G.blk0 + b];
      const long long *q = w + 8 + 4 * B0.nanc + 3 * b;
      REQUIRE(q[0] == Bb.panel_off && q[1] == Bb.row0 && q[2] == Bb.ld, "group descriptors: block %d of group %zu", b, g);
    }
    for (int c = 0; c < nch; ++c) {
      const int ch = t.dch_idx[B0.dch_ptr + c];
      const long long *q = w + 8 + 4 * B0.nanc + 3 * G.nblk;
      REQUIRE(q[c] == t.blks[ch].acc_off && q[nch + c] == blk2grp[ch], "group descriptors: child %d of group %zu", c, g);
    }
  }
}

static void check_lds(const TreeLayout &t, const DeviceLimits &dl) {
  auto one = [&](const LevelInfo &L, int g) {
    REQUIRE(L.lds_factor <= t.lds_limit && L.lds_sample <= t.lds_limit && L.lds_loglik <= t.lds_limit, "LDS: level %d: the generic kernels' vectors", g);
    REQUIRE(!L.fast || (L.lds_fast <= t.lds_limit && L.lds_sfast <= t.lds_limit), "LDS: level %d: fast is set, lds_fast %zu lds_sfast %zu", g, L.lds_fast, L.lds_sfast);
    REQUIRE(!L.bigmfma || L.lds_bigmfma <= t.lds_limit, "LDS: level %d: bigmfma is set, lds_bigmfma %zu", g, L.lds_bigmfma);
    REQUIRE(L.wide_count == 0 || L.lds_wide <= t.lds_limit, "LDS: level %d: wide groups, lds_wide %zu", g, L.lds_wide);
    REQUIRE(L.q_nkx == 0 || L.lds_quad + dl.quad_static <= DeviceLimits::CU_LDS, "LDS: level %d: q_nkx %d, lds_quad %zu", g, L.q_nkx, L.lds_quad);
    REQUIRE(L.lchain == 0 || lc_dyn_doubles(L.lchain) * 8 + dl.lchain_static[L.lchain == 96 ? 0 : 1] <= DeviceLimits::CU_LDS, "LDS: level %d: lchain %d", g, L.lchain);
    REQUIRE(!L.lchain_ref || (L.lchain && L.lds_ref_finish <= t.lds_limit), "LDS: level %d: lchain_ref is set, lds_ref_finish %zu", g, L.lds_ref_finish);
  };
  for (int g = 0; g < t.n_actual_groups; ++g) one(t.levels[g], g);
  if (!t.pred_list.empty()) REQUIRE(t.pred_info.lds_factor <= t.lds_limit, "LDS: the prediction blocks' generic kernel");
  REQUIRE(t.pred_nkx == 0 || t.pred_lds + dl.quad_static <= DeviceLimits::CU_LDS, "LDS: pred_nkx %d, pred_lds %zu", t.pred_nkx, t.pred_lds);
}

// over the ranks of the world: own runs, row mask, gather index
static void check_sharding(const std::vector<TreeLayout> &T) {
  const TreeLayout &t0 = T[0];
  const int world = (int)T.size();
  for (int g = 0; g < t0.n_actual_groups; ++g) {
    int at = 0;
    for (int r = 0; r < world; ++r) {
      const LevelInfo &L = T[r].levels[g];
      REQUIRE(T[r].cut == t0.cut && L.count == t0.levels[g].count, "sharding: rank %d sees another cut or level %d", r, g);
      if (g < t0.cut) { REQUIRE(L.own_lo == 0 && L.own_n == L.count, "sharding: level %d above the cut is not whole on rank %d", g, r); continue; }
      REQUIRE(L.own_n == 0 || L.own_lo == at, "sharding: level %d: the run of rank %d starts at %d, the ranks before it end at %d", g, r, L.own_lo, at);
      for (int k = L.own_lo; k < L.own_lo + L.own_n; ++k)
        REQUIRE(T[r].blk_owner[T[r].lvl_list[L.first + k]] == r, "sharding: level %d: block %d of rank %d's run belongs to another rank", g, k, r);
      at += L.own_n;
    }
    REQUIRE(g < t0.cut || at == t0.levels[g].count, "sharding: level %d: the ranks' runs cover %d of %d blocks", g, at, t0.levels[g].count);
  }
  for (long long row = 0; row < t0.n_all; ++row) {
    int sum = 0;
    for (int r = 0; r < world; ++r) sum += T[r].rowmask[row];
    REQUIRE(sum == 1, "sharding: rowmask sums to %d at row %lld", sum, row);
  }
  for (int r = 0; r < world; ++r) {
    const TreeLayout &t = T[r];
    std::vector<int> cnt(t.n_all, 0);
    REQUIRE((int)t.gidx.size() == world * t.gather_cnt, "sharding: gather index of rank %d has %zu slots", r, t.gidx.size());
    for (int s = 0; s < t.gather_cnt; ++s) {
      const int row = t.gidx[(size_t)r * t.gather_cnt + s];
      REQUIRE(row >= -1 && row < t.n_all && (s + 1 < t.gather_cnt || row == -1), "sharding: gather slot %d of rank %d holds %d", s, r, row);
      if (row >= 0) cnt[row]++;
    }
    for (int i = 0; i < (int)t.n_blocks; ++i)
      for (int k = 0; k < t.blks[i].m; ++k)
        REQUIRE(cnt[t.blks[i].row0 + k] == (t.blk_owner[i] == r ? 1 : 0), "sharding: row %lld is %d times in the gather index of rank %d", t.blks[i].row0 + k, cnt[t.blks[i].row0 + k], r);
  }
}

static void check_rank(const TreeLayout &t, const DeviceLimits &dl) {
  check_blocks(t);
  for (int g = 0; g < t.n_actual_groups; ++g) {
    const LevelInfo &L = t.levels[g];
    if (L.fast) check_groups(t, t.lvl_list.data() + L.first, L.count, L.grp_first, L.grp_count, L.isref != 0, "level", g);
    else REQUIRE(L.grp_count == 0, "column groups: level %d is not fast and has groups", g);
    if (L.quad_count > 0) check_quads(t, L.grp_first, L.grp_count, L.quad_first, L.quad_count, g, &L);
    else REQUIRE(L.q_nkx == 0 || L.grp_count == 0, "quads: level %d has q_nkx %d and no quads", g, L.q_nkx);
    if (L.wide_count > 0) check_wide(t, L, g);
    if (L.lchain || L.lc_count > 0) check_lchain(t, L, g);
  }
  check_groups(t, t.pred_list.data(), t.pred_grp_count ? (int)t.pred_list.size() : 0, t.pred_grp_first, t.pred_grp_count, false, "prediction list", -1);
  if (t.pred_grp_count > 0) check_quads(t, t.pred_grp_first, t.pred_grp_count, t.pred_quad_first, t.pred_quad_count, -1, nullptr);
  check_descriptors(t);
  check_lds(t, dl);
}

int main(int argc, char **argv) {
  if (argc < 4) { fprintf(stderr, "usage: layout_check FILE WORLD RANK [limited] [raise-group-m]\n"); return 3; }
  Problem P;
  if (!read_problem(argv[1], P)) { fprintf(stderr, "layout_check: cannot read %s\n", argv[1]); return 3; }
  const int world = atoi(argv[2]), rank = atoi(argv[3]);
  bool limited = false, raise_m = false;
  for (int a = 4; a < argc; ++a) { limited |= !strcmp(argv[a], "limited"); raise_m |= !strcmp(argv[a], "raise-group-m"); }
  const DeviceLimits dl = mi355x();
  const Switches sw = read_switches();
  std::vector<TreeLayout> T(std::max(world, 1));
  for (int r = 0; r < (int)T.size(); ++r) {
    st_options opt = {0, 1, world == (int)T.size() ? r : rank, world, 0, limited ? 2 : 0};
    std::string msg;
    int rc = layout_order(&P.pb, &opt, T[r], msg);
    if (rc == ST_OK) rc = layout_levels(&P.pb, sw, dl, T[r], msg);
    if (rc != ST_OK) { printf("REFUSED %d %s\n", rc, msg.c_str()); return 2; }
  }
  REQUIRE(rank >= 0 && rank < (int)T.size(), "usage: rank %d of world %d", rank, world);
  TreeLayout &t = T[rank];
  if (raise_m) { REQUIRE(!t.grps.empty(), "raise-group-m: the problem has no column group"); t.grps[t.grps.size() / 2].M += 1; }
  check_rank(t, dl);
  check_sharding(T);
  int last_ref = -1, n_fast = 0, n_lchain = 0, n_quad = 0;
  for (int g = 0; g < t.n_actual_groups; ++g) {
    if (t.levels[g].isref) last_ref = g;
    n_fast += t.levels[g].fast; n_lchain += t.levels[g].lchain != 0; n_quad += t.levels[g].q_nkx != 0;
  }
  int max_chain = 0;
  for (const Grp &G : t.grps) max_chain = std::max(max_chain, G.P);
  printf("OK levels=%d cut=%d fast_levels=%d quad_levels=%d lchain_levels=%d groups=%zu quads=%zu pred_groups=%d pred_quads=%d pred_nkx=%d "
         "wide_groups=%zu slabs=%zu rfvoff=%zu gram_direct_level=%d last_ref_level=%d max_group_chain=%d twins=%zu\n",
         t.n_actual_groups, t.cut, n_fast, n_quad, n_lchain, t.grps.size(), t.quads.size(), t.pred_grp_count, t.pred_quad_count, t.pred_nkx,
         t.wgrps.size(), t.lcslabs.size(), t.rfvoff.size(), t.gram_direct_level, last_ref, max_chain, t.twin_list.size());
  return 0;
}
