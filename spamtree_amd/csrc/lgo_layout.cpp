// lgo_layout.cpp -- see lgo_layout.hpp.  Host code only.
#include <map>

#include "lgo_layout.hpp"

int lgo_layout(const TreeLayout &t, const LooLayout &lo, const long long *labels, const unsigned char *obs, LgoLayout &o, std::string &msg) {
  o = LgoLayout();
  if (!labels || !obs) { msg = "no labels"; return ST_ERR_USAGE; }
  const long long n = t.n_all;
  const int nb = (int)t.n_blocks;
  // the rows of the density, per device row
  std::vector<unsigned char> in_density((size_t)n, 0);
  for (int b = 0; b < nb; ++b)
    if (lo.voff[b] >= 0)
      for (int i = 0; i < t.blks[b].m; ++i) in_density[(size_t)(t.blks[b].row0 + i)] = 1;
  // groups by ascending label, members by ascending model row
  std::map<long long, std::vector<long long>> by_label;
  for (long long r = 0; r < n; ++r)
    if (labels[r] >= 0 && in_density[(size_t)t.model2dev[r]]) by_label[labels[r]].push_back(r);
  std::vector<int> gid((size_t)n, -1), mi((size_t)n, -1);   // per device row: its group and its place among the members
  o.grp_ptr.push_back(0);
  o.gp_ptr.push_back(0);
  // the device indexes members, pair tables, pair slots and the groups' g x g matrices with 32-bit integers
  const long long lim = INT_MAX;
  long long n_tab = 0, n_sq = 0;
  const auto too_many = [&](const char *what, long long cnt) {
    msg = std::string("the labelling needs ") + std::to_string(cnt) + " " + what + ", at most " + std::to_string(lim) + " are supported";
    return ST_ERR_UNSUPPORTED;
  };
  for (const auto &kv : by_label) {
    const std::vector<long long> &mem = kv.second;
    if ((long long)mem.size() > LGO_MAX_MEMBERS) {
      msg = "the group of label " + std::to_string(kv.first) + " has " + std::to_string(mem.size()) + " members, at most " +
            std::to_string(LGO_MAX_MEMBERS) + " are supported";
      return ST_ERR_UNSUPPORTED;
    }
    bool any = false;
    for (long long r : mem) any |= obs[(size_t)t.model2dev[r]] != 0;
    if (!any) { msg = "the group of label " + std::to_string(kv.first) + " has no member with an observed y"; return ST_ERR_USAGE; }
    n_tab += (long long)(mem.size() * (mem.size() - 1) / 2); n_sq += (long long)(mem.size() * mem.size());
    if (n_tab > lim) return too_many("member pairs", n_tab);
    if (n_sq > lim) return too_many("entries of the groups' matrices", n_sq);
    const int g = (int)o.label.size();
    for (size_t k = 0; k < mem.size(); ++k) {
      const long long dr = t.model2dev[mem[k]];
      gid[(size_t)dr] = g; mi[(size_t)dr] = (int)k;
      o.mem_row.push_back(dr); o.mem_model.push_back(mem[k]);
    }
    o.label.push_back(kv.first);
    o.grp_ptr.push_back((int)o.mem_row.size());
    o.gp_ptr.push_back(o.gp_ptr.back() + (int)(mem.size() * (mem.size() - 1) / 2));
  }
  o.n_groups = (long long)o.label.size();
  o.n_members = (long long)o.mem_row.size();
  o.gp_idx.assign((size_t)o.gp_ptr.back(), -1);
  // the pair lists, in device block order
  o.voff.assign(nb, -1);
  o.pr_ptr.assign(nb + 1, 0);
  std::vector<long long> col_row;
  std::vector<std::vector<int>> seen((size_t)std::max<long long>(o.n_groups, 1));   // per group: the columns met so far, ascending
  std::vector<int> touched;
  for (int b = 0; b < nb; ++b) {
    o.pr_ptr[b + 1] = o.pr_ptr[b];
    if (lo.voff[b] < 0) continue;
    const Blk &B = t.blks[b];
    col_row.clear();
    for (int a = 0; a < B.nanc; ++a) {
      const Blk &U = t.blks[t.anc_idx[B.anc_ptr + a]];
      for (int i = 0; i < U.m; ++i) col_row.push_back(U.row0 + i);
    }
    if ((int)col_row.size() != B.P) { msg = "a block's chain does not have P rows"; return ST_ERR_TOPOLOGY; }
    for (int i = 0; i < B.m; ++i) col_row.push_back(B.row0 + i);
    touched.clear();
    for (int c = 0; c < (int)col_row.size(); ++c) {
      const int g = gid[(size_t)col_row[c]];
      if (g < 0) continue;
      std::vector<int> &prev = seen[g];
      if (prev.empty()) touched.push_back(g);
      for (int a : prev) {
        if (!B.isref && a >= B.P) continue;   // two own rows of a non-reference block: a structural zero
        if ((long long)o.pr_a.size() >= lim) return too_many("pair slots in the upward vectors", (long long)o.pr_a.size() + 1);
        int fin = -1;
        if (c >= B.P) {
          fin = (int)o.n_pairs++;
          const int i = mi[(size_t)col_row[a]], j = mi[(size_t)col_row[c]], lo_m = std::min(i, j), hi_m = std::max(i, j);
          o.gp_idx[(size_t)o.gp_ptr[g] + (size_t)hi_m * (hi_m - 1) / 2 + lo_m] = fin;
        }
        o.pr_a.push_back(a); o.pr_b.push_back(c); o.pr_fin.push_back(fin);
        // its products: every row of a reference block from b's first on, one product of a non-reference own column
        const double rows = c < B.P ? B.m : (B.isref ? B.m - (c - B.P) : 1);
        o.flops += 2.0 * rows;
      }
      prev.push_back(c);
    }
    for (int g : touched) seen[g].clear();
    o.pr_ptr[b + 1] = (int)o.pr_a.size();
    const int np = o.pr_ptr[b + 1] - o.pr_ptr[b];
    o.max_block_pairs = std::max(o.max_block_pairs, np);
    // the pair's two indices and its slot read, the p part written and read once by the parent (the panel comes from cache)
    o.alg_bytes += np * (12.0 + 16.0);
  }
  o.n_pair_slots = (long long)o.pr_a.size();
  // the vectors, in the order of LooLayout's list
  for (int b : lo.list) {
    const Blk &B = t.blks[b];
    o.voff[b] = o.arena;
    o.arena += 2ll * (B.P + B.m) + (o.pr_ptr[b + 1] - o.pr_ptr[b]);
  }
  // k_lgo_groups: per group its g^2 + 2 g gathered values, the four values of _last per entry written, the state
  for (long long g = 0; g < o.n_groups; ++g) {
    const double gm = o.grp_ptr[g + 1] - o.grp_ptr[g];
    o.alg_bytes += 8.0 * (gm * gm + 6.0 * gm) + 8.0 * (2.0 * gm * gm + 2.0 * gm) + 2.0 * 8.0 * (4.0 + 2.0 * gm);
    o.flops += 2.0 * gm * gm * gm;
  }
  o.alg_bytes += 8.0 * (double)o.n_pairs;   // the finished values written
  return ST_OK;
}
