// quad_record_check -- a stand-alone CPU program: builds the launch structures of a problem (spamtree_amd/csrc/tree_layout.cpp)
// with the MI355X's limits and rebuilds every quad record (QuadRec, factor_quad.hpp) by the rules k_factor_quad's prologue
// used before the records existed: the quad from `quads`, its units from their group descriptors (`gdesc`), the rows'
// coordinates and outcome ids from the problem in device order.  Every field of every record must equal the rebuilt one
// bit for bit.  Prints "OK key=value ..." or the first difference (exit status 1); a refusal of the layout prints
// "REFUSED <code> <message>" (exit status 2).
//
//   quad_record_check FILE WORLD RANK [limited] [corrupt]
//
// FILE: the problem as tests/test_tree_layout_cpu.py writes it.  The library's SPAMTREE_* switches are read from the
// environment.  corrupt: the negative case, one chain row's length in the middle record raised by one after the layout is
// built -- the comparison must name it.
#include <cstdarg>
#include <cstddef>

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

// the row data in device order, as the device step uploads it
struct Rows {
  std::vector<double> cx, cy;
  std::vector<int> mv;
};
static Rows device_rows(const st_problem &pb, const TreeLayout &t) {
  Rows R;
  const long long n = t.n_all;
  R.cx.resize(n); R.cy.resize(n); R.mv.resize(n);
  for (long long i = 0; i < n; ++i) {
    const long long r = t.dev2model[i];
    R.cx[i] = pb.coords[r]; R.cy[i] = pb.coords[n + r]; R.mv[i] = (int)(pb.mv_id[r] - 1);
  }
  return R;
}

struct Counts {
  long long quads = 0, pred_quads = 0, ref_quads = 0, priv_gt16 = 0, priv_le16 = 0, nu_lt4 = 0, units = 0, units_m_le16 = 0, levels = 0;
};

static double row_bits(long long r) { double d; std::memcpy(&d, &r, sizeof(d)); return d; }

// The record of quad Qd (its groups counted from grp_first) as the prologue derived it: from gdesc and the device rows.
template <int PMAX, bool ISREF>
static void expect_record(const TreeLayout &t, const Rows &D, int grp_first, const Quad &Qd, QuadRec<4, PMAX, ISREF> &E, Counts &c) {
  typedef QuadRec<4, PMAX, ISREF> Rec;
  std::memset(&E, 0, sizeof(E));
  for (int i = 0; i < 4 * 32; ++i) (&E.colw[0][0])[i] = row_bits(-1);
  for (int i = 0; i < Rec::NUL * Rec::NLD; ++i) (&E.pw[0][0])[i] = row_bits(-1);
  for (int k = 0; k < PMAX; ++k) E.wpa[k] = row_bits(-1);
  auto lo = [](long long v) { return (int)(v & 0xffffffffLL); };
  auto hi = [](long long v) { return (int)(v >> 32); };
  const int gds = t.gd_stride, Jc = Qd.Jc, Pc = Qd.Pc, nu = Qd.nu;
  REQUIRE(nu >= 1 && nu <= 4 && Pc >= 0 && Pc <= PMAX && Jc >= 0 && Jc <= MAXJ, "quad: nu %d, Jc %d, Pc %d do not fit the record (PMAX %d)", nu, Jc, Pc, PMAX);
  E.g0 = Qd.g0; E.nu = nu; E.Jc = Jc; E.Pc = Pc;
  E.nit = (Pc + 31) >> 5;
  const long long *g0 = t.gdesc.data() + (size_t)(grp_first + Qd.g0) * gds;
  E.level = hi(g0[4]);
  // the shared chain: the first Jc ancestors of unit 0
  int am[MAXJ + 1], ao[MAXJ + 1];
  long long arow[MAXJ + 1], apan[MAXJ + 1];
  for (int tt = 0; tt < Jc; ++tt) {
    const long long *a = g0 + 8 + 4 * tt;
    am[tt] = lo(a[0]); ao[tt] = hi(a[0]); arow[tt] = a[1]; apan[tt] = a[2];
  }
  ao[Jc] = Pc;
  (void)am;
  for (int k = 0; k < Pc; ++k) {
    int tt = 0;
    for (int j = 1; j < Jc; ++j) tt += (k >= ao[j]) ? 1 : 0;
    const long long r = arow[tt] + (k - ao[tt]);
    REQUIRE(r >= 0 && r < t.n_all, "quad: chain row %d maps to row %lld", k, r);
    E.sx[k] = D.cx[r]; E.sy[k] = D.cy[r]; E.smv[k] = D.mv[r]; E.wpa[k] = row_bits(r);
    const int len = ao[tt + 1];
    E.rlen[k] = len; E.rsrc[k] = apan[tt] + (long long)(k - ao[tt]) * len;
  }
  bool gt16 = false, any_priv = false;
  for (int u = 0; u < nu; ++u) {
    const long long *g = t.gdesc.data() + (size_t)(grp_first + Qd.g0 + u) * gds;
    const int M = lo(g[2]), P = hi(g[2]), J = lo(g[3]), nblk = hi(g[3]);
    REQUIRE(M >= 0 && M <= 32 && nblk >= 1 && nblk <= Rec::NB, "quad: unit %d has %d columns in %d blocks", u, M, nblk);
    E.urow0[u] = g[0]; E.uM[u] = M; E.uP[u] = P; E.uJ[u] = J; E.unblk[u] = nblk; E.uref[u] = lo(g[4]); E.ublk0[u] = lo(g[6]);
    ++c.units; c.units_m_le16 += M <= 16;
    if (J > Jc) {
      const long long *a = g + 8 + 4 * Jc;
      E.pm[u] = lo(a[0]); E.prow[u] = a[1]; E.ppan[u] = a[2];
      REQUIRE(E.pm[u] >= 0 && E.pm[u] <= 32, "quad: unit %d: private ancestor of %d rows", u, E.pm[u]);
      any_priv = true; gt16 = gt16 || E.pm[u] > 16;
      if constexpr (!ISREF)
        for (int i = 0; i < E.pm[u]; ++i) {
          const long long r = E.prow[u] + i;
          E.px[u][i] = D.cx[r]; E.py[u][i] = D.cy[r]; E.pmv[u][i] = D.mv[r]; E.pw[u][i] = row_bits(r);
        }
    }
    for (int b = 0; b < nblk; ++b) {
      const long long *q = g + 8 + 4 * J + 3 * b;
      E.bpan[u][b] = q[0]; E.brow[u][b] = q[1]; E.bld[u][b] = (int)q[2];
    }
    for (int i = 0; i < M; ++i) {
      const long long r = E.urow0[u] + i;
      REQUIRE(r >= 0 && r < t.n_all, "quad: unit %d column %d maps to row %lld", u, i, r);
      E.colx[u][i] = D.cx[r]; E.coly[u][i] = D.cy[r]; E.colmv[u][i] = D.mv[r]; E.colw[u][i] = row_bits(r);
      if constexpr (!ISREF) {
        int bi = 0;
        while (bi + 1 < nblk && r >= E.brow[u][bi + 1]) ++bi;
        E.colblk[u][i] = bi;
      }
    }
  }
  c.nu_lt4 += nu < 4;
  c.priv_gt16 += gt16; c.priv_le16 += any_priv && !gt16;
}

template <int PMAX, bool ISREF>
static void compare_record(const TreeLayout &t, const Rows &D, int grp_first, const Quad &Qd, const long long *rec, const char *what, int g, int k, Counts &c) {
  typedef QuadRec<4, PMAX, ISREF> Rec;
  static Rec E, R;
  expect_record<PMAX, ISREF>(t, D, grp_first, Qd, E, c);
  std::memcpy(&R, rec, sizeof(R));
  if (!std::memcmp(&E, &R, sizeof(R))) return;
  struct Field { const char *name; size_t off; };
#define F(n_) {#n_, offsetof(Rec, n_)}
  const Field fields[] = {F(g0), F(nu), F(Jc), F(Pc), F(level), F(nit), F(pad), F(uM), F(uP), F(ublk0), F(unblk), F(uref), F(uJ), F(pm), F(fail),
                          F(urow0), F(prow), F(ppan), F(bpan), F(brow), F(bld), F(colx), F(coly), F(colw), F(colmv), F(colblk), F(px), F(py),
                          F(pw), F(pmv), F(sx), F(sy), F(wpa), F(smv), F(rlen), F(rsrc), {"end", sizeof(Rec)}};
#undef F
  size_t at = 0;
  while (((const char *)&E)[at] == ((const char *)&R)[at]) ++at;
  int f = 0;
  while (fields[f + 1].off <= at) ++f;
  violated("quad records: %s %d quad %d: field %s differs at byte %zu of the field (record byte %zu)", what, g, k, fields[f].name, at - fields[f].off, at);
}

static void check_run(const TreeLayout &t, const Rows &D, int grp_first, int qfirst, int count, int nkx, bool isref, long long off, int words,
                      const char *what, int g, Counts &c) {
  REQUIRE(words == quad_rec_words(nkx, isref), "quad records: %s %d: %d words per record, the kernel's record has %d", what, g, words, quad_rec_words(nkx, isref));
  REQUIRE(off >= 0 && (size_t)off + (size_t)count * words <= t.qrec.size(), "quad records: %s %d: [%lld, + %d x %d) leaves the buffer of %zu words", what, g, off, count, words, t.qrec.size());
  REQUIRE(off % 2 == 0 && words % 2 == 0, "quad records: %s %d: records are not 16-byte aligned", what, g);
  for (int k = 0; k < count; ++k) {
    const Quad &Qd = t.quads[qfirst + k];
    const long long *rec = t.qrec.data() + off + (size_t)k * words;
#define CR(P_) (isref ? compare_record<P_, true>(t, D, grp_first, Qd, rec, what, g, k, c) : compare_record<P_, false>(t, D, grp_first, Qd, rec, what, g, k, c))
    if (nkx == 32) CR(128); else if (nkx == 38) CR(152); else if (nkx == 44) CR(176); else CR(200);
#undef CR
  }
}

template <int PMAX>
static size_t rlen_offset(bool isref) {
  typedef QuadRec<4, PMAX, true> RecR;
  typedef QuadRec<4, PMAX, false> RecL;
  return isref ? offsetof(RecR, rlen) : offsetof(RecL, rlen);
}

int main(int argc, char **argv) {
  if (argc < 4) { fprintf(stderr, "usage: quad_record_check FILE WORLD RANK [limited] [corrupt]\n"); return 3; }
  Problem P;
  if (!read_problem(argv[1], P)) { fprintf(stderr, "quad_record_check: cannot read %s\n", argv[1]); return 3; }
  const int world = atoi(argv[2]), rank = atoi(argv[3]);
  bool limited = false, corrupt = false;
  for (int a = 4; a < argc; ++a) { limited |= !strcmp(argv[a], "limited"); corrupt |= !strcmp(argv[a], "corrupt"); }
  const DeviceLimits dl = mi355x();
  const Switches sw = read_switches();
  TreeLayout t;
  {
    st_options opt = {0, 1, rank, world, 0, limited ? 2 : 0};
    std::string msg;
    int rc = layout_order(&P.pb, &opt, t, msg);
    if (rc == ST_OK) rc = layout_levels(&P.pb, sw, dl, t, msg);
    if (rc != ST_OK) { printf("REFUSED %d %s\n", rc, msg.c_str()); return 2; }
  }
  REQUIRE(t.qrec_bytes == t.qrec.size() * sizeof(long long), "quad records: qrec_bytes is %zu, the buffer has %zu words", t.qrec_bytes, t.qrec.size());
  if (corrupt) {   // a chain row's length in the middle record of the first run
    REQUIRE(!t.qrec.empty(), "corrupt: the problem has no quad record");
    long long off = t.pred_qr_off; int words = t.pred_qr_words, count = t.pred_quad_count, nkx = t.pred_nkx; bool isref = false;
    for (const LevelInfo &L : t.levels) if (L.qr_off >= 0) { off = L.qr_off; words = L.qr_words; count = L.qown_n; nkx = L.q_nkx; isref = L.isref != 0; break; }
    const size_t rl = nkx == 32 ? rlen_offset<128>(isref) : nkx == 38 ? rlen_offset<152>(isref) : nkx == 44 ? rlen_offset<176>(isref) : rlen_offset<200>(isref);
    int *p = (int *)((char *)(t.qrec.data() + off + (size_t)(count / 2) * words) + rl);
    p[0] += 1;
  }
  const Rows D = device_rows(P.pb, t);
  Counts c;
  // the runs tile the buffer in order: levels, then the prediction quads
  long long at = 0;
  for (int g = 0; g < t.n_actual_groups; ++g) {
    const LevelInfo &L = t.levels[g];
    const bool takes = t.sw.factor_gen == 3 && L.fast && L.q_nkx > 0 && L.qown_n > 0;
    REQUIRE((L.qr_off >= 0) == takes, "quad records: level %d %s k_factor_quad and has %s", g, takes ? "takes" : "does not take", L.qr_off >= 0 ? "records" : "none");
    if (!takes) continue;
    REQUIRE(L.qr_off == at, "quad records: level %d starts at word %lld, the runs before it end at %lld", g, L.qr_off, at);
    check_run(t, D, L.grp_first, L.quad_first + L.qown_lo, L.qown_n, L.q_nkx, L.isref != 0, L.qr_off, L.qr_words, "level", g, c);
    c.quads += L.qown_n; c.ref_quads += L.isref ? L.qown_n : 0; ++c.levels;
    at += (long long)L.qown_n * L.qr_words;
  }
  const bool pred = t.pred_nkx > 0 && t.pred_quad_count > 0;
  REQUIRE((t.pred_qr_off >= 0) == pred, "quad records: phase P %s k_factor_quad and has %s", pred ? "takes" : "does not take", t.pred_qr_off >= 0 ? "records" : "none");
  if (pred) {
    REQUIRE(t.pred_qr_off == at, "quad records: the prediction quads start at word %lld, the runs before them end at %lld", t.pred_qr_off, at);
    check_run(t, D, t.pred_grp_first, t.pred_quad_first, t.pred_quad_count, t.pred_nkx, false, t.pred_qr_off, t.pred_qr_words, "prediction", -1, c);
    c.pred_quads += t.pred_quad_count;
    at += (long long)t.pred_quad_count * t.pred_qr_words;
  }
  REQUIRE((size_t)at == t.qrec.size(), "quad records: the runs cover %lld of %zu words", at, t.qrec.size());
  printf("OK levels=%d cut=%d quad_levels=%lld quads=%lld ref_quads=%lld pred_quads=%lld priv_gt16=%lld priv_le16=%lld nu_lt4=%lld units=%lld units_m_le16=%lld "
         "record_bytes=%zu\n", t.n_actual_groups, t.cut, c.levels, c.quads, c.ref_quads, c.pred_quads, c.priv_gt16, c.priv_le16, c.nu_lt4, c.units,
         c.units_m_le16, t.qrec_bytes);
  return 0;
}
