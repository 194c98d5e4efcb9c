// points_layout.cpp -- the launch structures of a set of new points, without a HIP call (points_layout.hpp).  One function per
// job; points_layout at the end runs them in order.  tests/points_layout_check.cpp checks the result on the CPU.
#include <unordered_map>

#include "points_layout.hpp"

namespace {

// per chain its class (0: k_points_mfma<128>, 1: <256>, 2: the generic route) and per point, caller order, its chain
struct ChainMap {
  std::vector<int> cls, chain_of;
};

const double PER_POINT_BYTES = 2 * 8.0 + 4.0 + 8.0 + 8.0 + 4 * 8.0;   // coordinates, margin, order, z in; mean, var, w, yhat out

int refuse(std::string &msg, int code, const std::string &text) {
  msg = text;
  return code;
}

int check_args(const TreeLayout &t, int64_t n_new, const double *coords, const int64_t *mv, const int64_t *anchor, std::string &msg) {
  if (t.limited) return refuse(msg, ST_ERR_UNSUPPORTED, "st_points_set: limited_tree handles are not supported (new-point prediction is out of scope for them)");
  if (t.world > 1) return refuse(msg, ST_ERR_UNSUPPORTED, "st_points_set: multi-GPU handles (world > 1) are not supported (new-point prediction is out of scope for them)");
  if (n_new < 0 || n_new > (int64_t)INT32_MAX || (n_new > 0 && (!coords || !mv || !anchor))) return refuse(msg, ST_ERR_USAGE, "st_points_set: bad sizes or NULL inputs");
  for (int64_t i = 0; i < n_new; ++i) {
    if (anchor[i] < 0 || anchor[i] >= t.n_blocks) return refuse(msg, ST_ERR_USAGE, "st_points_set: anchor " + std::to_string(i) + " is not a block id");
    if (t.blks[t.blk_model2dev[anchor[i]]].nobs == 0) return refuse(msg, ST_ERR_USAGE, "st_points_set: anchor " + std::to_string(i) + " is a prediction block (no observed rows)");
    if (mv[i] < 1 || mv[i] > t.q) return refuse(msg, ST_ERR_USAGE, "st_points_set: margin of point " + std::to_string(i) + " is not in 1..q");
    if (!std::isfinite(coords[i]) || !std::isfinite(coords[n_new + i])) return refuse(msg, ST_ERR_USAGE, "st_points_set: coordinates must be finite");
  }
  return ST_OK;
}

// conditioning chain of every point: ends at r = the anchor (reference) or its last parent (non-reference); -1: no chain
std::vector<int> chain_ends(const TreeLayout &t, int64_t n_new, const int64_t *anchor) {
  std::vector<int> rdev(n_new);
  for (int64_t i = 0; i < n_new; ++i) {
    const int b = t.blk_model2dev[anchor[i]];
    const Blk &B = t.blks[b];
    rdev[i] = B.isref ? b : (B.nanc > 0 ? t.anc_idx[B.anc_ptr + B.nanc - 1] : -1);
  }
  return rdev;
}

// joint groups: by first appearance, members in the caller's order; one chain and at most ST_POINTS_MAX_JOINT members each
int group_joint(int64_t n_new, const int64_t *joint_id, const std::vector<int> &rdev, PointsLayout &out, std::string &msg) {
  std::unordered_map<int64_t, int> index;
  std::vector<int> gsz;
  std::vector<int64_t> first;   // per group: its first member
  out.pt_grp.resize(n_new); out.pt_a.resize(n_new);
  for (int64_t i = 0; i < n_new; ++i) {
    auto it = index.find(joint_id[i]);
    if (it == index.end()) { it = index.emplace(joint_id[i], (int)gsz.size()).first; gsz.push_back(0); first.push_back(i); }
    const int k = it->second;
    if (rdev[i] != rdev[first[k]])
      return refuse(msg, ST_ERR_USAGE, "st_points_set_joint: the members of joint group " + std::to_string(joint_id[i]) +
                                           " do not end in the same conditioning chain (point " + std::to_string(i) + " and point " +
                                           std::to_string(first[k]) + ")");
    out.pt_grp[i] = k; out.pt_a[i] = gsz[k]++;
    if (gsz[k] > ST_POINTS_MAX_JOINT)
      return refuse(msg, ST_ERR_UNSUPPORTED, "st_points_set_joint: joint group " + std::to_string(joint_id[i]) + " has more than " +
                                                 std::to_string(ST_POINTS_MAX_JOINT) + " members (ST_POINTS_MAX_JOINT)");
  }
  const size_t nj = gsz.size();
  out.n_joint = (long long)nj;
  out.j_mptr.assign(nj + 1, 0); out.j_off.assign(nj + 1, 0);
  for (size_t k = 0; k < nj; ++k) {
    out.j_mptr[k + 1] = out.j_mptr[k] + gsz[k];
    out.j_off[k + 1] = out.j_off[k] + (int64_t)gsz[k] * gsz[k];
  }
  out.cov_total = out.j_off[nj];
  out.j_mem.assign(n_new, 0);
  for (int64_t i = 0; i < n_new; ++i) out.j_mem[out.j_mptr[out.pt_grp[i]] + out.pt_a[i]] = i;
  return ST_OK;
}

// the distinct chains in the order of their last block, root first each, and the kernel class of each
ChainMap build_chains(const TreeLayout &t, const std::vector<int> &rdev, PointsLayout &out) {
  std::vector<int> keys(rdev);
  std::sort(keys.begin(), keys.end());
  keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  ChainMap cm;
  cm.cls.resize(keys.size()); cm.chain_of.resize(rdev.size());
  out.chains.resize(keys.size());
  out.n_chains = (int)keys.size();
  const bool lds256 = PP_LDS_BYTES(256) <= t.lds_limit;
  long long maxrows = 1;
  for (size_t c = 0; c < keys.size(); ++c) {
    PtChain &C = out.chains[c];
    C.first = (int)out.chain_blk.size(); C.nblk = 0; C.rows = 0; C.pad = 0;
    if (keys[c] >= 0) {
      const Blk &R = t.blks[keys[c]];
      for (int a = 0; a < R.nanc; ++a) out.chain_blk.push_back(t.anc_idx[R.anc_ptr + a]);
      out.chain_blk.push_back(keys[c]);
      C.nblk = R.nanc + 1;
      C.rows = R.P + R.m;
    }
    const bool generic = t.force_generic || C.rows > 256 || (C.rows > 128 && !lds256) || C.nblk > PP_MAXB;
    cm.cls[c] = generic ? 2 : (C.rows <= 128 ? 0 : 1);
    if (generic) maxrows = std::max<long long>(maxrows, C.rows);
  }
  out.scratch_stride = (maxrows + 31) & ~31LL;
  for (size_t i = 0; i < rdev.size(); ++i) cm.chain_of[i] = (int)(std::lower_bound(keys.begin(), keys.end(), rdev[i]) - keys.begin());
  return cm;
}

// the byte and flop model of one chain: its stored panels (+ coordinates, margin, w of the chain rows) and one
// lower-triangular product, 2 x rows (rows + 1) / 2
void chain_cost(const TreeLayout &t, const PointsLayout &out, const PtChain &C, double *panel_bytes, double *tri_flops) {
  double pb = 0.0;
  long long o = 0;
  for (int a = 0; a < C.nblk; ++a) { const Blk &A = t.blks[out.chain_blk[C.first + a]]; o += A.m; pb += (double)A.m * (double)o * 8.0; }
  *panel_bytes = pb + (double)C.rows * 28.0;
  *tri_flops = (double)C.rows * (double)(C.rows + 1);
}

// sorted order: 128-row chains, then 256-row chains, then the generic route; by chain, then by the caller's index.  A run of
// one chain becomes tiles of at most PP_NCOL points, or entries of the generic list
void order_and_tiles(const TreeLayout &t, const ChainMap &cm, PointsLayout &out) {
  const int64_t n_new = (int64_t)cm.chain_of.size();
  out.order.resize(n_new); out.pt_chain.resize(n_new);
  std::iota(out.order.begin(), out.order.end(), 0LL);
  std::stable_sort(out.order.begin(), out.order.end(), [&](long long a, long long b) {
    const int ca = cm.chain_of[a], cb = cm.chain_of[b];
    return cm.cls[ca] != cm.cls[cb] ? cm.cls[ca] < cm.cls[cb] : ca < cb;
  });
  double bytes = 0.0, flops = 0.0;
  for (int64_t s = 0; s < n_new;) {
    const int c = cm.chain_of[out.order[s]];
    int64_t e = s;
    while (e < n_new && cm.chain_of[out.order[e]] == c) { out.pt_chain[e] = c; ++e; }
    const double rows = out.chains[c].rows;
    double pb, tf;
    chain_cost(t, out, out.chains[c], &pb, &tf);
    if (cm.cls[c] == 2) {
      for (int64_t i = s; i < e; ++i) out.gen.push_back((int)i);
      bytes += (double)(e - s) * (pb + PER_POINT_BYTES);
      flops += (double)(e - s) * (2.0 * tf + 4.0 * rows);              // v and u per point, then v'v and v'u
    } else {
      for (int64_t p0 = s; p0 < e; p0 += PP_NCOL) {
        PtTile T; T.chain = c; T.p0 = (int)p0; T.np = (int)std::min<int64_t>(PP_NCOL, e - p0); T.pad = 0;
        out.tiles.push_back(T);
        if (cm.cls[c] == 0) ++out.ntile128; else ++out.ntile256;
        bytes += pb;
        flops += tf + (double)T.np * (tf + 4.0 * rows);                // u once per tile, v per point
      }
      bytes += (double)(e - s) * PER_POINT_BYTES;
    }
    s = e;
  }
  out.alg_bytes = bytes; out.flops = flops;
  out.grid_generic = (int)std::min<size_t>(out.gen.size(), (size_t)4 * t.sm_count);
}

// the groups `ks` of MFMA-class chain c into 16-column slots of whole groups, four slots to a tile (workgroup); a padding column
// names the group that opened its tile.  Adds the tiles' share of the model
void pack_chain_slots(int c, const std::vector<int> &ks, double pb, double tf, PointsLayout &out, int *ntile, double *jb, double *jf) {
  const double rows = out.chains[c].rows;
  int slot = 4, used = 16;                                             // no open tile
  for (int k : ks) {
    const int g = out.groups[k].g;
    if (used + g > 16) {
      if (++slot >= 4) {
        PtTile T; T.chain = c; T.p0 = 0; T.np = 0; T.pad = 0;
        out.jtiles.push_back(T);
        out.jcols.resize(out.jcols.size() + PP_NCOL, PtCol{k, -1});
        ++*ntile;
        *jb += pb; *jf += tf;
        slot = 0;
      }
      used = 0;
      out.jtiles.back().np = slot + 1;
    }
    PtCol *col = out.jcols.data() + (out.jtiles.size() - 1) * PP_NCOL + slot * 16 + used;
    for (int a = 0; a < g; ++a) { col[a].grp = k; col[a].a = a; }
    used += g;
    *jf += g * (tf + 4.0 * rows);
  }
}

// the joint packing: the groups of MFMA-class chains into slots, one chain per workgroup, 128-row chains first; the groups of
// the other chains one workgroup each
void pack_joint(const TreeLayout &t, const ChainMap &cm, PointsLayout &out) {
  const int64_t nj = out.n_joint;
  out.groups.resize(nj);
  std::vector<std::vector<int>> by_chain(out.chains.size());
  for (int64_t k = 0; k < nj; ++k) {
    PtJoint &G = out.groups[k];
    G.cov_off = out.j_off[k]; G.first = (int)out.j_mptr[k]; G.g = (int)(out.j_mptr[k + 1] - out.j_mptr[k]);
    G.chain = cm.chain_of[out.j_mem[out.j_mptr[k]]]; G.pad = 0;
    by_chain[G.chain].push_back((int)k);
  }
  double jb = 0.0, jf = 0.0;
  for (int pass = 0; pass < 3; ++pass)
    for (size_t c = 0; c < out.chains.size(); ++c) {
      if (cm.cls[c] != pass || by_chain[c].empty()) continue;
      double pb, tf;
      chain_cost(t, out, out.chains[c], &pb, &tf);
      const double rows = out.chains[c].rows;
      for (int k : by_chain[c]) {
        const double g = out.groups[k].g;
        jb += g * (PER_POINT_BYTES + 8.0) + 2.0 * g * g * 8.0;         // + the member index; cov and chol out
        jf += g * (g + 1.0) * rows + g * g * g / 3.0 + g * (g + 1.0);  // the Gram, the factorisation, L z
      }
      if (pass < 2) { pack_chain_slots((int)c, by_chain[c], pb, tf, out, pass == 0 ? &out.jtile128 : &out.jtile256, &jb, &jf); continue; }
      for (int k : by_chain[c]) {
        out.jgen.push_back(k);
        jb += pb + out.groups[k].g * 2.0 * rows * 8.0;                 // the chain once per group; V written and read
        jf += (out.groups[k].g + 1.0) * (tf + 2.0 * rows);
      }
    }
  out.j_alg_bytes = jb; out.j_flops = jf;
  out.jgrid_generic = (int)std::min<size_t>(out.jgen.size(), (size_t)4 * t.sm_count);
  if (out.jcols.empty()) out.jcols.push_back(PtCol{0, -1});
}

}   // namespace

int points_layout(const TreeLayout &t, int64_t n_new, const double *coords, const int64_t *mv, const int64_t *anchor,
                  const int64_t *joint_id, PointsLayout &out, std::string &msg) {
  out = PointsLayout();
  if (int rc = check_args(t, n_new, coords, mv, anchor, msg)) return rc;
  const std::vector<int> rdev = chain_ends(t, n_new, anchor);
  if (joint_id)
    if (int rc = group_joint(n_new, joint_id, rdev, out, msg)) return rc;
  if (n_new == 0) return ST_OK;
  const ChainMap cm = build_chains(t, rdev, out);
  order_and_tiles(t, cm, out);
  if (joint_id) pack_joint(t, cm, out);
  return ST_OK;
}

// ---- linear functionals (points_fun.hpp): argument checks, the linear and the variance term list, their chunks ----
namespace {

int check_functionals(const FunFacts &p, int64_t n_fun, const int64_t *ptr, const int64_t *idx, const double *wt, std::string &msg) {
  const char *who = "st_points_functionals_set: ";
  if (n_fun < 0 || n_fun > (int64_t)INT32_MAX || (n_fun > 0 && !ptr)) return refuse(msg, ST_ERR_USAGE, std::string(who) + "bad sizes or NULL inputs");
  if (n_fun == 0) return ST_OK;
  if (ptr[0] != 0) return refuse(msg, ST_ERR_USAGE, std::string(who) + "ptr[0] is not 0");
  for (int64_t f = 0; f < n_fun; ++f)
    if (ptr[f + 1] < ptr[f]) return refuse(msg, ST_ERR_USAGE, std::string(who) + "ptr decreases at functional " + std::to_string(f));
  if (ptr[n_fun] > 0 && (!idx || !wt)) return refuse(msg, ST_ERR_USAGE, std::string(who) + "bad sizes or NULL inputs");
  std::vector<int64_t> seen((size_t)p.n, -1);   // the last functional that named the point
  for (int64_t f = 0; f < n_fun; ++f)
    for (int64_t k = ptr[f]; k < ptr[f + 1]; ++k) {
      const std::string at = "functional " + std::to_string(f) + ", entry " + std::to_string(k - ptr[f]);
      if (idx[k] < 0 || idx[k] >= p.n) return refuse(msg, ST_ERR_USAGE, who + at + ": index " + std::to_string(idx[k]) + " is not a point of the set (0.." + std::to_string(p.n - 1) + ")");
      if (!std::isfinite(wt[k])) return refuse(msg, ST_ERR_USAGE, who + at + ": the weight is not finite");
      if (seen[idx[k]] == f) return refuse(msg, ST_ERR_USAGE, who + at + ": point " + std::to_string(idx[k]) + " occurs twice in the functional");
      seen[idx[k]] = f;
    }
  return ST_OK;
}

// the variance terms of functional [k0, k1): (a_i^2, i), or per touched group (layout order) the pairs a >= b of its members in
// column-major order with (a_a a_b, doubled off the diagonal; j_off[g] + a + b g)
void variance_terms(const FunFacts &p, const int64_t *idx, const double *wt, int64_t k0, int64_t k1, std::vector<FunTerm> &var) {
  if (!p.joint) {
    for (int64_t k = k0; k < k1; ++k) var.push_back(FunTerm{wt[k] * wt[k], (long long)idx[k]});
    return;
  }
  struct Mem { int grp, a; double w; };
  std::vector<Mem> mem;
  mem.reserve((size_t)(k1 - k0));
  for (int64_t k = k0; k < k1; ++k) mem.push_back(Mem{p.pt_grp[idx[k]], p.pt_a[idx[k]], wt[k]});
  std::sort(mem.begin(), mem.end(), [](const Mem &x, const Mem &y) { return x.grp != y.grp ? x.grp < y.grp : x.a < y.a; });
  for (size_t s = 0; s < mem.size();) {
    size_t e = s;
    while (e < mem.size() && mem[e].grp == mem[s].grp) ++e;
    const long long o = p.j_off[mem[s].grp], g = p.j_mptr[mem[s].grp + 1] - p.j_mptr[mem[s].grp];
    for (size_t b = s; b < e; ++b)
      for (size_t a = b; a < e; ++a) {
        const double c = mem[a].w * mem[b].w;
        var.push_back(FunTerm{a == b ? c : 2.0 * c, o + mem[a].a + (long long)mem[b].a * g});
      }
    s = e;
  }
}

// terms [t0, t1) of a list, all of functional f, into chunks of FUN_CHUNK
void cut_chunks(long long t0, long long t1, int f, std::vector<FunChunk> &chunks) {
  for (long long t = t0; t < t1; t += FUN_CHUNK) chunks.push_back(FunChunk{t, (int)std::min<long long>(FUN_CHUNK, t1 - t), f});
}

}   // namespace

int functionals_layout(const FunFacts &p, int64_t n_fun, const int64_t *ptr, const int64_t *idx, const double *wt, FunLayout &out,
                       std::string &msg) {
  out = FunLayout();
  if (int rc = check_functionals(p, n_fun, ptr, idx, wt, msg)) return rc;
  out.n_fun = n_fun;
  out.lin_cptr.assign((size_t)n_fun + 1, 0); out.var_cptr.assign((size_t)n_fun + 1, 0);
  if (n_fun == 0) return ST_OK;
  out.nnz = ptr[n_fun];
  out.lin.reserve((size_t)out.nnz);
  for (int64_t f = 0; f < n_fun; ++f) {
    const long long l0 = (long long)out.lin.size(), v0 = (long long)out.var.size();
    for (int64_t k = ptr[f]; k < ptr[f + 1]; ++k) out.lin.push_back(FunTerm{wt[k], (long long)idx[k]});
    variance_terms(p, idx, wt, ptr[f], ptr[f + 1], out.var);
    cut_chunks(l0, (long long)out.lin.size(), (int)f, out.lin_chunks);
    cut_chunks(v0, (long long)out.var.size(), (int)f, out.var_chunks);
    out.lin_cptr[f + 1] = (long long)out.lin_chunks.size(); out.var_cptr[f + 1] = (long long)out.var_chunks.size();
  }
  out.n_var_terms = (long long)out.var.size();
  if (out.lin_chunks.size() + out.var_chunks.size() > (size_t)INT32_MAX) return refuse(msg, ST_ERR_UNSUPPORTED, "st_points_functionals_set: more than 2^31 - 1 chunks");
  return ST_OK;
}
