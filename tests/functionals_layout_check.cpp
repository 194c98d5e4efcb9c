// functionals_layout_check -- a stand-alone CPU program: builds the term lists of a set of linear functionals
// (functionals_layout in spamtree_amd/csrc/points_layout.cpp) and checks, with plain loops, what k_fun_chunks and k_fun_finish
// trust of them.  It rebuilds nothing with the code under test: the joint groups come from the labels by a loop of its own, and
// every check reads the finished FunLayout and the caller's arrays.  Prints "OK key=value ..." or the first violated invariant
// (exit status 1); a refusal of the layout prints "REFUSED <code> <message>" (exit status 2).
//
//   functionals_layout_check INPUT [shift-chunk] [swap-pair]
//
// INPUT: 3 int64 (n_new, joint: 0 / 1, n_fun), then the joint labels, ptr, idx and wt (raw 8-byte words), each an int64 count
// followed by that many 8-byte values (count 0: a null pointer).  The negative cases, applied after the layout is built --
// the checks must name them: shift-chunk moves the start of the last linear chunk by one term; swap-pair exchanges the first two
// variance terms of the first functional that has two.
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

struct Input {
  int64_t n_new = 0, joint = 0, n_fun = 0;
  std::vector<int64_t> arr[4];   // labels, ptr, idx, wt (raw words)
  const int64_t *ip(int a) const { return arr[a].empty() ? nullptr : arr[a].data(); }
  const double *wt() const { return arr[3].empty() ? nullptr : (const double *)arr[3].data(); }
};

static bool read_input(const char *path, Input &Q) {
  FILE *f = fopen(path, "rb");
  if (!f) return false;
  int64_t head[3];
  bool ok = fread(head, 8, 3, f) == 3;
  for (int a = 0; ok && a < 4; ++a) {
    int64_t cnt = 0;
    ok = fread(&cnt, 8, 1, f) == 1 && cnt >= 0 && cnt < (1LL << 32);
    if (ok) { Q.arr[a].resize((size_t)cnt); ok = fread(Q.arr[a].data(), 8, (size_t)cnt, f) == (size_t)cnt; }
  }
  fclose(f);
  Q.n_new = head[0]; Q.joint = head[1]; Q.n_fun = head[2];
  return ok;
}

// the joint groups of the labels: by first appearance, members in the caller's order, g x g packed blocks
struct Groups {
  std::vector<int64_t> j_off{0}, j_mptr{0}, j_mem;
  std::vector<int> pt_grp, pt_a;
};
static Groups groups_of(const Input &Q) {
  Groups G;
  std::unordered_map<int64_t, int> index;
  std::vector<std::vector<int64_t>> mem;
  G.pt_grp.resize(Q.n_new); G.pt_a.resize(Q.n_new);
  for (int64_t i = 0; i < Q.n_new; ++i) {
    auto it = index.find(Q.arr[0][i]);
    if (it == index.end()) { it = index.emplace(Q.arr[0][i], (int)mem.size()).first; mem.emplace_back(); }
    G.pt_grp[i] = it->second; G.pt_a[i] = (int)mem[it->second].size();
    mem[it->second].push_back(i);
  }
  for (const auto &m : mem) {
    G.j_mptr.push_back(G.j_mptr.back() + (int64_t)m.size());
    G.j_off.push_back(G.j_off.back() + (int64_t)(m.size() * m.size()));
    G.j_mem.insert(G.j_mem.end(), m.begin(), m.end());
  }
  return G;
}

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

struct Report {
  long long max_lin_chunks = 0, max_var_chunks = 0, empty = 0, full_chunks = 0, cross_group = 0, offdiag = 0;
};

// one list's chunks: per functional consecutive, in order, without a gap or an overlap, full but for the last
static void check_chunks(const char *what, int64_t n_fun, const std::vector<long long> &want_terms, const std::vector<FunChunk> &chunks,
                         const std::vector<long long> &cptr, size_t list_len, long long *max_chunks, Report &R) {
  REQUIRE((int64_t)cptr.size() == n_fun + 1 && cptr[0] == 0 && cptr[n_fun] == (long long)chunks.size(), "%s chunks: cptr does not run from 0 to the %zu chunks", what, chunks.size());
  long long at = 0;
  for (int64_t f = 0; f < n_fun; ++f) {
    REQUIRE(cptr[f + 1] >= cptr[f], "%s chunks: cptr decreases at functional %lld", what, (long long)f);
    const long long nc = cptr[f + 1] - cptr[f];
    REQUIRE(nc == (want_terms[f] + FUN_CHUNK - 1) / FUN_CHUNK, "%s chunks: functional %lld of %lld terms has %lld chunks", what, (long long)f, want_terms[f], nc);
    const long long end = at + want_terms[f];
    for (long long c = cptr[f]; c < cptr[f + 1]; ++c) {
      const FunChunk &C = chunks[c];
      REQUIRE(C.fun == f, "%s chunks: chunk %lld of functional %lld names functional %d", what, c, (long long)f, C.fun);
      REQUIRE(C.t0 == at, "%s chunks: chunk %lld starts at term %lld, the chunks before it end at %lld", what, c, C.t0, at);
      REQUIRE(C.nt >= 1 && C.nt <= FUN_CHUNK && at + C.nt <= end, "%s chunks: chunk %lld holds %d terms (functional %lld ends at term %lld)", what, c, C.nt, (long long)f, end);
      REQUIRE(C.nt == FUN_CHUNK || c + 1 == cptr[f + 1], "%s chunks: chunk %lld holds %d terms and is not the last of functional %lld", what, c, C.nt, (long long)f);
      R.full_chunks += C.nt == FUN_CHUNK;
      at += C.nt;
    }
    REQUIRE(at == end, "%s chunks: the chunks of functional %lld end at term %lld, its terms at %lld", what, (long long)f, at, end);
    *max_chunks = std::max(*max_chunks, nc);
  }
  REQUIRE((size_t)at == list_len, "%s chunks: the chunks cover %lld terms, the list has %zu", what, at, list_len);
}

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: functionals_layout_check INPUT [shift-chunk] [swap-pair]\n"); return 3; }
  Input Q;
  if (!read_input(argv[1], Q)) { fprintf(stderr, "functionals_layout_check: cannot read %s\n", argv[1]); return 3; }
  bool shift_chunk = false, swap_pair = false;
  for (int a = 2; a < argc; ++a) { shift_chunk |= !strcmp(argv[a], "shift-chunk"); swap_pair |= !strcmp(argv[a], "swap-pair"); }
  REQUIRE(!Q.joint || (int64_t)Q.arr[0].size() == Q.n_new, "input: %zu labels for %lld points", Q.arr[0].size(), (long long)Q.n_new);
  const Groups G = Q.joint ? groups_of(Q) : Groups();
  FunFacts F;
  F.n = Q.n_new; F.joint = Q.joint != 0;
  F.j_off = G.j_off.data(); F.j_mptr = G.j_mptr.data(); F.pt_grp = G.pt_grp.data(); F.pt_a = G.pt_a.data();
  FunLayout L;
  std::string msg;
  const int rc = functionals_layout(F, Q.n_fun, Q.ip(1), Q.ip(2), Q.wt(), L, msg);
  if (rc != ST_OK) { printf("REFUSED %d %s\n", rc, msg.c_str()); return 2; }
  const int64_t nf = Q.n_fun;
  const int64_t *ptr = Q.ip(1), *idx = Q.ip(2);
  const double *wt = Q.wt();
  if (shift_chunk) {
    REQUIRE(!L.lin_chunks.empty(), "shift-chunk: the set has no linear chunk");
    L.lin_chunks.back().t0 += 1;
  }
  if (swap_pair) {
    int64_t f = 0;
    while (f < nf && L.var_chunks.size() && !(L.var_cptr[f + 1] > L.var_cptr[f] && L.var_chunks[L.var_cptr[f]].nt >= 2)) ++f;
    REQUIRE(f < nf && !L.var_chunks.empty(), "swap-pair: no functional has two variance terms");
    const long long t = L.var_chunks[L.var_cptr[f]].t0;
    std::swap(L.var[t], L.var[t + 1]);
  }
  Report R;
  REQUIRE(L.n_fun == nf && L.nnz == (nf ? ptr[nf] : 0) && (long long)L.lin.size() == L.nnz && (long long)L.var.size() == L.n_var_terms,
          "counts: n_fun %lld, nnz %lld, n_var_terms %lld against %lld functionals, %zu linear and %zu variance terms", L.n_fun, L.nnz, L.n_var_terms, (long long)nf, L.lin.size(), L.var.size());

  // the linear list: the caller's terms in the caller's order, every source index a point
  for (long long k = 0; k < L.nnz; ++k) {
    REQUIRE(L.lin[k].src == idx[k] && same_bits(L.lin[k].c, wt[k]), "linear list: term %lld is not the caller's entry %lld", k, k);
    REQUIRE(L.lin[k].src >= 0 && L.lin[k].src < Q.n_new, "linear list: term %lld reads point %lld of %lld", k, L.lin[k].src, (long long)Q.n_new);
  }
  std::vector<long long> lin_terms(nf), var_terms(nf);
  const long long vlen = Q.joint ? G.j_off.back() : Q.n_new;   // the length of the variance list's source vector

  // the variance list, functional after functional
  long long vt = 0;
  std::vector<double> w_of(Q.n_new, 0.0);
  std::vector<int64_t> in_f(Q.n_new, -1);
  for (int64_t f = 0; f < nf; ++f) {
    lin_terms[f] = ptr[f + 1] - ptr[f];
    R.empty += lin_terms[f] == 0;
    if (!Q.joint) {
      var_terms[f] = lin_terms[f];
      for (int64_t k = ptr[f]; k < ptr[f + 1]; ++k, ++vt) {
        REQUIRE(vt < (long long)L.var.size(), "variance list: it ends inside functional %lld", (long long)f);
        REQUIRE(L.var[vt].src == idx[k] && same_bits(L.var[vt].c, wt[k] * wt[k]), "variance list: term %lld is not (a^2, i) of entry %lld of functional %lld", vt, (long long)(k - ptr[f]), (long long)f);
        REQUIRE(L.var[vt].src >= 0 && L.var[vt].src < vlen, "variance list: term %lld reads element %lld of %lld", vt, L.var[vt].src, vlen);
      }
      continue;
    }
    std::unordered_map<int, long long> members;   // group -> members of it in f
    for (int64_t k = ptr[f]; k < ptr[f + 1]; ++k) { in_f[idx[k]] = f; w_of[idx[k]] = wt[k]; ++members[G.pt_grp[idx[k]]]; }
    long long want = 0;
    for (const auto &kv : members) want += kv.second * (kv.second + 1) / 2;
    R.cross_group += members.size() > 1;
    var_terms[f] = want;
    long long pk = -1, pa = -1, pb = -1;   // the previous term's (group, column, row)
    for (long long j = 0; j < want; ++j, ++vt) {
      REQUIRE(vt < (long long)L.var.size(), "variance list: it ends inside functional %lld", (long long)f);
      const FunTerm &T = L.var[vt];
      REQUIRE(T.src >= 0 && T.src < vlen, "variance list: term %lld reads element %lld of %lld", vt, T.src, vlen);
      const long long k = (long long)(std::upper_bound(G.j_off.begin(), G.j_off.end(), (int64_t)T.src) - G.j_off.begin()) - 1;
      const long long g = G.j_mptr[k + 1] - G.j_mptr[k], r = T.src - G.j_off[k], a = r % g, b = r / g;
      REQUIRE(r < g * g, "variance list: term %lld lies outside the block of group %lld", vt, k);
      REQUIRE(a >= b, "variance list: term %lld of functional %lld reads the upper triangle of group %lld (row %lld, column %lld)", vt, (long long)f, k, a, b);
      const int64_t ia = G.j_mem[G.j_mptr[k] + a], ib = G.j_mem[G.j_mptr[k] + b];
      REQUIRE(in_f[ia] == f && in_f[ib] == f, "variance list: term %lld of functional %lld pairs points %lld and %lld, which are not both in it", vt, (long long)f, (long long)ia, (long long)ib);
      const double c = w_of[ia] * w_of[ib];
      REQUIRE(same_bits(T.c, a == b ? c : 2.0 * c), "variance list: term %lld of functional %lld does not carry a_a a_b (doubled off the diagonal)", vt, (long long)f);
      REQUIRE(k > pk || (k == pk && (b > pb || (b == pb && a > pa))), "variance list: term %lld of functional %lld is not in (group, column, row) order", vt, (long long)f);
      pk = k; pa = a; pb = b;
      R.offdiag += a != b;
    }
  }
  REQUIRE(vt == (long long)L.var.size(), "variance list: %zu terms, the functionals account for %lld", L.var.size(), vt);

  check_chunks("linear", nf, lin_terms, L.lin_chunks, L.lin_cptr, L.lin.size(), &R.max_lin_chunks, R);
  check_chunks("variance", nf, var_terms, L.var_chunks, L.var_cptr, L.var.size(), &R.max_var_chunks, R);
  for (int64_t f = 0; f < nf; ++f)
    if (lin_terms[f] == 0) REQUIRE(L.lin_cptr[f + 1] == L.lin_cptr[f] && L.var_cptr[f + 1] == L.var_cptr[f], "empty functional %lld has chunks", (long long)f);

  printf("OK n_fun=%lld nnz=%lld n_var_terms=%lld n_chunks=%zu max_lin_chunks=%lld max_var_chunks=%lld full_chunks=%lld empty=%lld cross_group=%lld offdiag=%lld\n",
         L.n_fun, L.nnz, L.n_var_terms, L.lin_chunks.size() + L.var_chunks.size(), R.max_lin_chunks, R.max_var_chunks, R.full_chunks, R.empty,
         R.cross_group, R.offdiag);
  return 0;
}
