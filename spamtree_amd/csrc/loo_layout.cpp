// loo_layout.cpp -- see loo_layout.hpp.  Host code only.
#include "loo_layout.hpp"

int loo_layout(const TreeLayout &t, LooLayout &o, std::string &msg) {
  o = LooLayout();
  if (t.limited) { msg = "limited_tree handles are not supported"; return ST_ERR_UNSUPPORTED; }
  if (t.world > 1) { msg = "multi-GPU handles are not supported"; return ST_ERR_UNSUPPORTED; }
  const int nb = (int)t.n_blocks;
  o.voff.assign(nb, -1);
  std::vector<std::vector<int>> ch(nb);
  for (int g = t.n_actual_groups - 1; g >= 0; --g) {
    const LevelInfo &L = t.levels[g];
    if (L.count == 0) continue;
    LooLevel V;
    V.first = (int)o.list.size(); V.count = L.count; V.level = g; V.isref = L.isref;
    for (int k = 0; k < L.count; ++k) {
      const int b = t.lvl_list[L.first + k];   // ascending inside a level (build_levels sorts)
      const Blk &B = t.blks[b];
      if (B.nobs <= 0 || B.panel_off < 0) { msg = "a block of a level list has no panel"; return ST_ERR_TOPOLOGY; }
      if ((B.isref != 0) != (L.isref != 0)) { msg = "a block's kind differs from its level's"; return ST_ERR_TOPOLOGY; }
      const int len = B.P + B.m;
      o.list.push_back(b);
      o.voff[b] = o.arena;
      o.arena += 2ll * len;
      V.maxLen = std::max(V.maxLen, len); V.maxM = std::max(V.maxM, B.m);
      if (B.nanc > 0) {
        const int u = t.anc_idx[B.anc_ptr + B.nanc - 1];
        const Blk &U = t.blks[u];
        bool ok = U.nobs > 0 && U.isref && U.nanc == B.nanc - 1 && U.P + U.m == B.P;
        for (int a = 0; ok && a < U.nanc; ++a) ok = t.anc_idx[U.anc_ptr + a] == t.anc_idx[B.anc_ptr + a];
        if (!ok) { msg = "a block's chain is not its last parent's chain plus that parent"; return ST_ERR_TOPOLOGY; }
        ch[u].push_back(b);
      }
      const double m = B.m, P = B.P, own = B.isref ? m * (m + 1) / 2 : m;
      // the panel once (its second use comes from cache), the gathered w, the vector written and read once by the parent,
      // per row: y, xb, mv and the four values of _last written, six doubles of state read and written
      o.alg_bytes += 8.0 * (m * P + own) + 8.0 * (P + m) + 2.0 * 16.0 * (P + m) + m * (20.0 + 32.0 + 96.0);
      o.flops += 6.0 * (m * P + own) + 2.0 * (P + m);
    }
    o.levels.push_back(V);
  }
  o.ch_ptr.assign(nb + 1, 0);
  for (int b = 0; b < nb; ++b) {
    std::sort(ch[b].begin(), ch[b].end());
    o.ch_ptr[b + 1] = o.ch_ptr[b] + (int)ch[b].size();
    o.ch_idx.insert(o.ch_idx.end(), ch[b].begin(), ch[b].end());
  }
  return ST_OK;
}
