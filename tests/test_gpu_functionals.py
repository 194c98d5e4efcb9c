"""GPU: linear functionals of the new-point predictions (st_points_functionals_*, k_fun_chunks / k_fun_finish, stm_mcmc_functionals,
predict.fit_predict(functionals=)).

The rounding bound is the one spamtree_amd/csrc/points_fun.hpp states with the summation order: a list of T terms is cut into
ceil(T / FUN_CHUNK) chunks; a lane adds at most ceil(min(T, FUN_CHUNK) / 64) terms, one fused multiply-add (one rounding) each; six
butterfly levels; the chunk sums in order.  With c(T) = ceil(min(T, FUN_CHUNK) / 64) + 6 + ceil(T / FUN_CHUNK),
    |F - exact| <= c(T) 2^-53 sum |coefficient value|,
checked in exact rational arithmetic against the per-point outputs the same call returned.  The coefficients are those of the term
lists: the caller's weights, fl(a_i a_i) into cond_var, fl(a_a a_b) (doubled off the diagonal) into the packed Sigma."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from tests.util import make_problem

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUN_CHUNK = int(re.search(r"#define FUN_CHUNK (\d+)", open(os.path.join(ROOT, "spamtree_amd", "csrc", "points_fun.hpp")).read()).group(1))
SIZES = (0, 1, 63, 64, 65, FUN_CHUNK - 1, FUN_CHUNK, FUN_CHUNK + 1, 2 * FUN_CHUNK + 3)
ST_ERR_USAGE, ST_ERR_UNSUPPORTED = -1, -4
U = Fraction(1, 2 ** 53)
ITERS = 6
QS = (0.0, 0.3, 0.5, 0.975, 1.0)
dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))    # noqa: E731


def chain(T):
    """The longest addition chain of a list of T terms."""
    return -(-min(T, FUN_CHUNK) // 64) + 6 + -(-T // FUN_CHUNK)


_PB = {}


def problem(q):
    if q not in _PB:
        _PB[q] = make_problem(side=20, q=q, seed=40 + q, missing=0.1, p=2)
    return _PB[q]


def model(pb, fg=False, limited=False):
    from spamtree_amd.model import SpamTreeMV
    rng = np.random.default_rng(6)
    hm = SpamTreeMV(pb["y"], pb["X"], pb["Z"], pb["coords"], pb["mv_id"], pb["blocking"], pb["gix_block"], pb["res_is_ref"],
                    pb["parents"], pb["children"], limited, pb["block_names"], pb["block_groups"], pb["indexing"],
                    rng.standard_normal(pb["n"]), np.zeros(pb["p"]), pb["theta"], 5.0, force_generic=fg)
    assert hm.get_loglik_comps_w(0)
    return hm


def plain_points(pb, n, seed, with_X=True):
    from spamtree_amd.predict import locate
    rng = np.random.default_rng(seed)
    lo, hi = pb["coords"].min(axis=0), pb["coords"].max(axis=0)
    pts = lo + (hi - lo) * rng.uniform(size=(n, 2))
    mv = rng.integers(1, pb["q"] + 1, size=n)
    return pts, mv, locate(pb["topo"], pts, mv, device=0), (rng.standard_normal((n, pb["p"])) if with_X else None)


def site_points(pb, n_sites, seed):
    """The q outcomes at n_sites sites, one joint group a site (predict.group_sites)."""
    from spamtree_amd.predict import group_sites, locate
    rng = np.random.default_rng(seed)
    lo, hi = pb["coords"].min(axis=0), pb["coords"].max(axis=0)
    q = pb["q"]
    pts = np.repeat(lo + (hi - lo) * rng.uniform(size=(n_sites, 2)), q, axis=0)
    mv = np.tile(np.arange(1, q + 1), n_sites)
    labels = group_sites(pts)
    return pts, mv, locate(pb["topo"], pts, mv, device=0, joint=labels), rng.standard_normal((pts.shape[0], pb["p"])), labels


def sized_rows(n, rng, sizes=SIZES):
    """Functionals of the given term counts: points without repetition, mixed-sign weights over 1e-3 .. 1e3."""
    return [(rng.choice(n, k, replace=False), rng.choice([-1.0, 1.0], k) * 10.0 ** rng.uniform(-3, 3, k)) for k in sizes]


def accumulate(hm, pb, iters=ITERS, seed=9, state_seed=77):
    """iters saved iterations with another w, beta, tausq and theta each: (per-point outputs, functionals_last) per iteration."""
    rng = np.random.default_rng(state_seed)
    outs, lasts = [], []
    for s in range(iters):
        hm.set_w(rng.standard_normal(pb["n"]))
        hm.beta_update(np.asfortranarray(rng.standard_normal((pb["p"], pb["q"]))))
        hm.tausq_inv = 1.0 / rng.uniform(0.05, 0.5, pb["q"])
        hm._check(hm.lib.st_set_tausq_inv(hm.h, dp(hm.tausq_inv)))
        hm.theta_update(0, pb["theta"] * (1.0 + 0.03 * s))
        assert hm.get_loglik_comps_w(0)
        outs.append(hm.accumulate_points(seed=seed, it=s))
        lasts.append(hm.functionals_last() if hm.n_functionals else None)
    return outs, lasts


def start(hm, A, keep=ITERS):
    hm.set_functionals(A)
    hm._check(hm.lib.st_points_summary_reserve(hm.h, keep))
    hm._check(hm.lib.st_points_summary_reset(hm.h))


def exact_sum(coef, values):
    """(sum coef value, sum |coef value|), exactly."""
    t = [Fraction(float(c)) * Fraction(float(v)) for c, v in zip(coef, values)]
    return sum(t, Fraction(0)), sum((abs(x) for x in t), Fraction(0))


def assert_within(got, coef, values, T, tag):
    want, mag = exact_sum(coef, values)
    err = abs(Fraction(float(got)) - want)
    tol = chain(T) * U * mag
    print(f"{tag}: T={T} c={chain(T)} err={float(err):.3e} tol={float(tol):.3e}")
    assert err <= tol, (tag, float(err), float(tol))


def fma(a, b, c):
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))     # one rounding


def host_summaries(lasts, has_y=True):
    """The recursion of k_fun_finish over the device's own per-iteration values, and st_points_functionals_get's expressions."""
    nf = lasts[0]["w"].size
    m, M2, V, W, Y = (np.zeros(nf) for _ in range(5))
    for s, la in enumerate(lasts):
        x = la["cond_mean"]
        d = x - m
        m1 = m + d / float(s + 1)
        M2 = np.array([fma(d[i], x[i] - m1[i], M2[i]) for i in range(nf)])
        m = m1
        V = V + la["cond_var"]
        W = W + la["w"]
        if has_y:
            Y = Y + la["yhat"]
    cnt = float(len(lasts))
    return dict(mean=m, var=V / cnt + M2 / cnt, w_mean=W / cnt, yhat_mean=Y / cnt if has_y else None)


def assert_summaries(hm, lasts, has_y=True):
    from oracle.list_summaries import list_qtile
    from tests.test_outputs_reference import qtile_bound
    got, want = hm.functionals(), host_summaries(lasts, has_y)
    assert got["n"] == len(lasts)
    for k in ("mean", "var", "w_mean") + (("yhat_mean",) if has_y else ()):
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
    for key, which in (("w", 0), ("yhat", 1)) if has_y else (("w", 0),):
        draws = np.stack([la[key] for la in lasts])
        for q in QS:
            gq = hm.functionals_quantile(q)[which]
            assert np.all(np.abs(gq - list_qtile(list(draws), q)) <= qtile_bound(draws, q)), (key, q)


# ---- 1. identity functionals are the per-point summaries, bit for bit -------------------------------------------------------
@pytest.mark.parametrize("q", [1, 2])
def test_identity_functionals_are_the_point_summaries(q):
    pb = problem(q)
    hm = model(pb)
    if q == 1:
        pts, mv, anchor, X = plain_points(pb, 3001, 11)
        hm.set_points(pts, mv, anchor, X)
    else:
        pts, mv, anchor, X, labels = site_points(pb, 1500, 12)
        hm.set_points(pts, mv, anchor, X, joint=labels)
    n = pts.shape[0]
    sub = np.random.default_rng(1).choice(n, 257, replace=False)
    start(hm, [([i], [1.0]) for i in sub])
    outs, lasts = accumulate(hm, pb)
    for o, la in zip(outs, lasts):
        for kf, kp in (("w", "w"), ("cond_mean", "mean"), ("cond_var", "var"), ("yhat", "yhat")):
            assert np.array_equal(la[kf], o[kp][sub]), kf
    mean, var, wm, ym = (np.zeros(n) for _ in range(4))
    hm._check(hm.lib.st_points_summary_get(hm.h, dp(mean), dp(var), dp(wm), dp(ym), None))
    f = hm.functionals()
    for got, want in ((f["mean"], mean), (f["var"], var), (f["w_mean"], wm), (f["yhat_mean"], ym)):
        assert np.array_equal(got, want[sub])
    wq, yq = np.zeros(n), np.zeros(n)
    for qq in QS:
        hm._check(hm.lib.st_points_summary_quantile(hm.h, qq, dp(wq), dp(yq)))
        fw, fy = hm.functionals_quantile(qq)
        assert np.array_equal(fw, wq[sub]) and np.array_equal(fy, yq[sub]), qq
    hm.close()


# ---- 2. against an exact reference, within the derived bound; 7. the same on a force_generic handle ----------------------------
@pytest.mark.parametrize("fg", [False, True])
def test_values_against_the_exact_reference(fg):
    pb = problem(1)
    hm = model(pb, fg=fg)
    n = 3001
    pts, mv, anchor, X = plain_points(pb, n, 13)
    hm.set_points(pts, mv, anchor, X)
    rows = sized_rows(n, np.random.default_rng(2))
    start(hm, rows)
    info = hm.functionals_info()
    nch = sum(-(-k // FUN_CHUNK) for k in SIZES)
    assert info["n_fun"] == len(SIZES) and info["nnz"] == info["n_var_terms"] == sum(SIZES) and info["n_chunks"] == 2 * nch
    assert info["alg_bytes"] >= 16.0 * 2 * sum(SIZES) + 32.0 * sum(SIZES)
    outs, lasts = accumulate(hm, pb)
    assert ("k_points_generic" in hm.points_info()["routes"]) == fg
    for s, (o, la) in enumerate(zip(outs, lasts)):
        for f, (idx, wt) in enumerate(rows):
            T = len(idx)
            assert_within(la["w"][f], wt, o["w"][idx], T, f"iter {s} fun {f} F_w")
            assert_within(la["cond_mean"][f], wt, o["mean"][idx], T, f"iter {s} fun {f} F_m")
            assert_within(la["yhat"][f], wt, o["yhat"][idx], T, f"iter {s} fun {f} F_y")
            assert_within(la["cond_var"][f], wt * wt, o["var"][idx], T, f"iter {s} fun {f} F_v")
        assert la["w"][0] == 0.0 and la["cond_var"][0] == 0.0       # the empty functional
        assert np.all(la["cond_var"] >= 0.0)
    assert_summaries(hm, lasts)
    hm.close()


# ---- 3. joint sets ---------------------------------------------------------------------------------------------------------
def variance_terms(idx, wt, hm):
    """The variance list of one functional on a joint set, rebuilt here: groups in layout order, pairs a >= b column-major."""
    grp_of, a_of = {}, {}
    for k, g in enumerate(hm.joint_groups):
        for a, i in enumerate(g):
            grp_of[int(i)], a_of[int(i)] = k, a
    mem = sorted((grp_of[int(i)], a_of[int(i)], float(w)) for i, w in zip(idx, wt))
    coef, src = [], []
    s = 0
    while s < len(mem):
        e = s
        while e < len(mem) and mem[e][0] == mem[s][0]:
            e += 1
        k = mem[s][0]
        g = hm.joint_groups[k].size
        for b in range(s, e):
            for a in range(b, e):
                c = mem[a][2] * mem[b][2]
                coef.append(c if a == b else 2.0 * c)
                src.append(int(hm.joint_offsets[k]) + mem[a][1] + mem[b][1] * g)
        s = e
    return np.array(coef), np.array(src, dtype=np.int64)


def test_joint_sets():
    pb = problem(2)
    hm = model(pb)
    pts, mv, anchor, X, labels = site_points(pb, 1500, 14)
    n = pts.shape[0]
    hm.set_points(pts, mv, anchor, X, joint=labels)
    rng = np.random.default_rng(3)
    G = hm.joint_groups
    assert len(G) == 1500 and all(g.size == 2 for g in G)
    contrast_sites = rng.choice(1500, 40, replace=False)
    rows = [((G[k][0], G[k][1]), (1.0, -1.0)) for k in contrast_sites]
    n_contrast = len(rows)
    rows.append(((G[5][0], G[9][1]), (0.75, -1.25)))                                                    # one member each of two groups
    others = np.setdiff1d(np.arange(n), G[7])
    rows.append((np.concatenate([G[7], rng.choice(others, 30, replace=False)]), rng.standard_normal(32)))   # a whole group plus others
    rows.append((rng.permutation(n), rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-3, 3, n)))          # 4500 variance terms
    start(hm, rows)
    vt = [variance_terms(i, w, hm) for i, w in rows]
    info = hm.functionals_info()
    assert info["n_var_terms"] == sum(c.size for c, _ in vt) and info["nnz"] == sum(len(r[0]) for r in rows)
    assert vt[-1][0].size == 4500 > FUN_CHUNK and vt[n_contrast][0].size == 2 and vt[n_contrast + 1][0].size == 3 + 30
    assert info["n_chunks"] == sum(-(-len(r[0]) // FUN_CHUNK) for r in rows) + sum(-(-c.size // FUN_CHUNK) for c, _ in vt)
    outs, lasts = accumulate(hm, pb)
    for s, (o, la) in enumerate(zip(outs, lasts)):
        cov = o["cov_packed"]
        for f, (idx, wt) in enumerate(rows):
            idx, wt = np.asarray(idx), np.asarray(wt, dtype=np.float64)
            assert_within(la["w"][f], wt, o["w"][idx], idx.size, f"iter {s} fun {f} F_w")
            assert_within(la["cond_mean"][f], wt, o["mean"][idx], idx.size, f"iter {s} fun {f} F_m")
            assert_within(la["yhat"][f], wt, o["yhat"][idx], idx.size, f"iter {s} fun {f} F_y")
            coef, src = vt[f]
            want, _ = exact_sum(coef, cov[src])
            if want >= 0:
                assert_within(la["cond_var"][f], coef, cov[src], coef.size, f"iter {s} fun {f} F_v")
            else:
                assert la["cond_var"][f] == 0.0
        for j, k in enumerate(contrast_sites):     # F_v = Sigma_11 + Sigma_22 - 2 Sigma_12 of the returned cond_cov
            S = o["cov"][k]
            assert_within(la["cond_var"][j], [1.0, -2.0, 1.0], [S[0, 0], S[1, 0], S[1, 1]], 3, f"iter {s} contrast {j} F_v")
    assert_summaries(hm, lasts)
    # var of a contrast against st_points_summary_get_cov by the same formula
    packed = np.zeros(int(hm.joint_offsets[-1]))
    hm._check(hm.lib.st_points_summary_get_cov(hm.h, dp(packed)))
    Cv = hm.unpack_joint(packed)
    var = hm.functionals()["var"]
    for j, k in enumerate(contrast_sites):
        assert_within(var[j], [1.0, -2.0, 1.0], [Cv[k][0, 0], Cv[k][1, 0], Cv[k][1, 1]], 3, f"contrast {j} var against get_cov")
    hm.close()


# ---- 4. independence, bit for bit -------------------------------------------------------------------------------------------
def test_a_functional_does_not_depend_on_the_others_or_on_the_point_order():
    """F_w and F_y of a reordered point set are another realisation (Philox streams 6 / 7 count the caller's positions, as the
    point tests note); its F_m, F_v, mean and var follow the functional bit for bit."""
    pb = problem(1)
    n = 3001
    pts, mv, anchor, X = plain_points(pb, n, 15)
    rows = sized_rows(n, np.random.default_rng(4))
    keys = ("w", "cond_mean", "cond_var", "yhat")

    def run(rows_, order=None):
        hm = model(pb)
        if order is None:
            hm.set_points(pts, mv, anchor, X)
        else:
            hm.set_points(pts[order], mv[order], anchor[order], X[order])
        start(hm, rows_)
        _, lasts = accumulate(hm, pb)
        out = dict(lasts=lasts, summ=hm.functionals(), q=[hm.functionals_quantile(q) for q in QS])
        hm.close()
        return out

    base = run(rows)
    pick = [len(rows) - 1, 5, 1]                    # alone: the others removed
    for f in pick:
        alone = run([rows[f]])
        for la, lb in zip(alone["lasts"], base["lasts"]):
            assert all(la[k][0] == lb[k][f] for k in keys), f
        assert all(alone["summ"][k][0] == base["summ"][k][f] for k in ("mean", "var", "w_mean", "yhat_mean")), f
        assert all(a[0][0] == b[0][f] and a[1][0] == b[1][f] for a, b in zip(alone["q"], base["q"])), f
    perm = np.random.default_rng(5).permutation(len(rows))
    shuffled = run([rows[f] for f in perm])
    for la, lb in zip(shuffled["lasts"], base["lasts"]):
        assert all(np.array_equal(la[k], lb[k][perm]) for k in keys)
    assert all(np.array_equal(shuffled["summ"][k], base["summ"][k][perm]) for k in ("mean", "var", "w_mean", "yhat_mean"))
    assert all(np.array_equal(a[0], b[0][perm]) and np.array_equal(a[1], b[1][perm]) for a, b in zip(shuffled["q"], base["q"]))
    order = np.random.default_rng(6).permutation(n)          # new position j holds old point order[j]
    pos = np.empty(n, dtype=np.int64)
    pos[order] = np.arange(n)
    moved = run([(pos[np.asarray(i)], w) for i, w in rows], order=order)
    for la, lb in zip(moved["lasts"], base["lasts"]):
        assert np.array_equal(la["cond_mean"], lb["cond_mean"]) and np.array_equal(la["cond_var"], lb["cond_var"])
    assert np.array_equal(moved["summ"]["mean"], base["summ"]["mean"]) and np.array_equal(moved["summ"]["var"], base["summ"]["var"])


# ---- 5. lifecycle and refusals ----------------------------------------------------------------------------------------------
def test_lifecycle_and_refusals():
    pb = problem(1)
    hm = model(pb)
    lib, h = hm.lib, hm.h
    from spamtree_amd.model import functionals_csr
    gp, gi, gw = functionals_csr([([0, 1, 2], [1.0, 2.0, 3.0]), ([], []), ([5, 7], [0.5, -0.5])], 40)
    assert lib.st_points_functionals_set(h, 3, ip(gp), ip(gi), dp(gw)) == ST_ERR_USAGE                  # before any point set
    assert b"before st_points_set" in lib.st_last_error(h)
    v = [C.c_int64(7) for _ in range(4)]
    assert lib.st_points_functionals_info(h, *[C.byref(x) for x in v], None) == 0 and [x.value for x in v] == [0, 0, 0, 0]
    n = 40
    pts, mv, anchor, _ = plain_points(pb, n, 16, with_X=False)
    hm.set_points(pts, mv, anchor)                                                                      # no X
    out = np.zeros(3)
    assert lib.st_points_functionals_get(h, dp(out), None, None, None, None) == ST_ERR_USAGE            # no functionals yet
    assert lib.st_points_functionals_set(h, 3, ip(gp), ip(gi), dp(gw)) == 0
    hm.n_functionals = 3
    cnt = C.c_int64(-1)
    assert lib.st_points_functionals_get(h, dp(out), None, None, None, C.byref(cnt)) == ST_ERR_USAGE and cnt.value == 0
    assert b"no iteration accumulated" in lib.st_last_error(h)
    assert lib.st_points_functionals_last(h, dp(out), None, None, None) == ST_ERR_USAGE
    o1 = hm.accumulate_points(seed=3, it=0)
    assert lib.st_points_functionals_quantile(h, 0.5, dp(out), None) == ST_ERR_USAGE                    # no reservation
    assert b"no draw stored" in lib.st_last_error(h)
    assert lib.st_points_functionals_quantile(h, 1.5, dp(out), None) == ST_ERR_USAGE
    assert lib.st_points_functionals_get(h, None, None, None, dp(out), None) == ST_ERR_USAGE            # yhat without X
    assert lib.st_points_functionals_last(h, None, None, None, dp(out)) == ST_ERR_USAGE
    assert lib.st_points_functionals_quantile(h, 0.5, None, dp(out)) == ST_ERR_USAGE
    la = hm.functionals_last()
    assert la["yhat"] is None and la["w"][1] == 0.0
    assert la["cond_mean"][2] == 0.5 * o1["mean"][5] - 0.5 * o1["mean"][7]

    # every bad input names its functional and entry and leaves the previous functionals usable
    def bad(edit, text):
        p_, i_, w_ = gp.copy(), gi.copy(), gw.copy()
        edit(p_, i_, w_)
        assert lib.st_points_functionals_set(h, 3, ip(p_), ip(i_), dp(w_)) == ST_ERR_USAGE
        assert text in lib.st_last_error(h).decode(), lib.st_last_error(h)
        assert hm.functionals()["n"] == 1 and np.array_equal(hm.functionals_last()["w"], la["w"])

    bad(lambda p_, i_, w_: p_.__setitem__(0, 1), "ptr[0] is not 0")
    bad(lambda p_, i_, w_: p_.__setitem__(2, 2), "ptr decreases at functional 1")
    bad(lambda p_, i_, w_: i_.__setitem__(4, n), "functional 2, entry 1: index 40")
    bad(lambda p_, i_, w_: i_.__setitem__(0, -1), "functional 0, entry 0: index -1")
    bad(lambda p_, i_, w_: w_.__setitem__(1, np.nan), "functional 0, entry 1: the weight is not finite")
    bad(lambda p_, i_, w_: i_.__setitem__(2, 0), "functional 0, entry 2: point 0 occurs twice")

    # reserve and reset size and clear the functional stores and accumulators; the point summaries of a new set of functionals stay
    assert lib.st_points_summary_reserve(h, 2) == 0
    for s in range(3):
        hm.accumulate_points(seed=3, it=1 + s)
    assert hm.functionals()["n"] == 4
    wq = hm.functionals_quantile(0.0)[0]                  # over the two stored draws
    assert lib.st_points_functionals_set(h, 3, ip(gp), ip(gi), dp(gw)) == 0                             # replaces: zeroed
    assert lib.st_points_functionals_get(h, dp(out), None, None, None, C.byref(cnt)) == ST_ERR_USAGE and cnt.value == 0
    assert lib.st_points_functionals_quantile(h, 0.5, dp(out), None) == ST_ERR_USAGE
    pm = np.zeros(n)
    assert lib.st_points_summary_get(h, dp(pm), None, None, None, C.byref(cnt)) == 0 and cnt.value == 4   # left alone
    o = hm.accumulate_points(seed=3, it=9)
    assert hm.functionals()["n"] == 1 and np.isfinite(wq).all()
    assert lib.st_points_summary_reset(h) == 0
    assert lib.st_points_functionals_get(h, dp(out), None, None, None, C.byref(cnt)) == ST_ERR_USAGE and cnt.value == 0
    o = hm.accumulate_points(seed=3, it=10)
    f = hm.functionals()
    assert f["n"] == 1 and f["mean"][2] == 0.5 * o["mean"][5] - 0.5 * o["mean"][7] and f["w_mean"][1] == 0.0
    assert hm.functionals_quantile(1.0)[0][0] == hm.functionals_last()["w"][0]

    # n_fun = 0 removes them; a new point set drops them
    assert lib.st_points_functionals_set(h, 0, None, None, None) == 0
    assert lib.st_points_functionals_get(h, dp(out), None, None, None, None) == ST_ERR_USAGE
    assert b"before st_points_functionals_set" in lib.st_last_error(h)
    hm.accumulate_points(seed=3, it=11)                   # as without functionals
    assert lib.st_points_functionals_set(h, 3, ip(gp), ip(gi), dp(gw)) == 0
    hm.set_points(pts, mv, anchor)
    assert lib.st_points_functionals_info(h, *[C.byref(x) for x in v], None) == 0 and v[0].value == 0
    assert lib.st_points_functionals_last(h, dp(out), None, None, None) == ST_ERR_USAGE

    # a point set of size 0: only empty functionals fit; they are 0
    hm.set_points(np.zeros((0, 2)), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))
    assert lib.st_points_functionals_set(h, 3, ip(gp), ip(gi), dp(gw)) == ST_ERR_USAGE
    ep = np.zeros(3, dtype=np.int64)
    assert lib.st_points_functionals_set(h, 2, ip(ep), None, None) == 0
    hm.n_functionals = 2
    hm.accumulate_points(seed=3, it=0)
    f = hm.functionals()
    assert f["n"] == 1 and np.array_equal(f["mean"], [0.0, 0.0]) and np.array_equal(f["var"], [0.0, 0.0])
    hm.close()

    # a limited_tree handle is refused as its siblings are
    pl = make_problem(side=20, q=1, seed=41, missing=0.1, p=2, limited_tree=True)
    hl = model(pl, limited=True)
    assert hl.lib.st_points_functionals_set(hl.h, 3, ip(gp), ip(gi), dp(gw)) == ST_ERR_UNSUPPORTED
    assert b"limited_tree" in hl.lib.st_last_error(hl.h)
    assert hl.lib.st_points_functionals_get(hl.h, dp(out), None, None, None, None) == ST_ERR_UNSUPPORTED
    hl.close()


# ---- 6. the driver ---------------------------------------------------------------------------------------------------------
MCMC = dict(mcmc_keep=6, mcmc_burn=4, mcmc_thin=2, adapting=True, sample_theta=True, seed=1234, device=0)


def same_tree(a, b, path="new"):
    """Every array of two result trees, bit for bit."""
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), path
        for k in a:
            same_tree(a[k], b[k], f"{path}.{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            same_tree(x, y, f"{path}[{i}]")
    elif a is None:
        assert b is None, path
    else:
        assert np.array_equal(np.asarray(a), np.asarray(b)), path


@pytest.mark.parametrize("joint", [False, True])
def test_the_driver(joint):
    from spamtree_amd.predict import areal_means, contrasts, fit_predict, predict_new
    pb = problem(2 if joint else 1)
    if joint:
        pts, mv, _, X, labels = site_points(pb, 300, 17)
        rows = contrasts(np.arange(600).reshape(300, 2)[:50])
    else:
        pts, mv, _, X = plain_points(pb, 1500, 18)
        labels = None
        rows = areal_means(np.random.default_rng(7).integers(-1, 12, size=1500))
    n = pts.shape[0]
    big = (np.arange(n), np.linspace(-1.0, 2.0, n))
    A = [(rows[1][rows[0][f]:rows[0][f + 1]], rows[2][rows[0][f]:rows[0][f + 1]]) for f in range(rows[0].size - 1)] + [big]
    base = fit_predict(pb, pts, mv, X, quantiles=QS, joint=labels, **MCMC)
    out = fit_predict(pb, pts, mv, X, quantiles=QS, joint=labels, functionals=A, **MCMC)
    fun = out["new"].pop("functionals")
    for key in ("beta_mcmc", "tausq_mcmc", "theta_mcmc", "paramsd", "w_mcmc", "yhat_mcmc"):
        same_tree(out[key], base[key], key)
    same_tree(out["new"], base["new"])                     # every output of stm_mcmc_points(_joint), bit for bit
    keep = MCMC["mcmc_keep"]
    assert fun["w"].shape == (len(A), keep)
    # the functional outputs are those of the step-by-step st_points_accumulate route over the saved draws.  On the plain set
    # the replay gives the per-point draws and moments bit for bit (tests/test_gpu_fit_predict.py), with a theta accepted inside
    # the saved window, and so the functionals; a joint set's replayed covariances agree to rounding only
    # (tests/test_gpu_predict_joint.py), so there the functionals are held against the fit's own per-point outputs alone
    rep = predict_new(pb, out, pts, mv, X, seed=MCMC["seed"], device=0, joint=labels, functionals=A, return_moments=True)
    rep0 = predict_new(pb, out, pts, mv, X, seed=MCMC["seed"], device=0, joint=labels, return_moments=True)
    rf = rep.pop("functionals")
    same_tree(rep, rep0, "replay")                         # st_points_accumulate in place of st_points_predict: the same bits
    if not joint:
        assert len({tuple(c) for c in np.asarray(out["theta_mcmc"]).T}) >= 2
        for key in ("w", "cond_mean", "cond_var", "mean", "var", "w_mean"):
            assert np.array_equal(rf[key], fun[key]), key
    else:                                                  # the joint replay's functionals against its own per-point outputs
        assert rf["w"].shape == fun["w"].shape and np.all(np.isfinite(rf["var"])) and np.all(rf["var"] >= 0)
        for s in range(keep):
            for f, (idx, wt) in enumerate(A):
                idx, wt = np.asarray(idx), np.asarray(wt, dtype=np.float64)
                for kf, kp in (("w", "w"), ("cond_mean", "cond_mean"), ("yhat", "yhat")):
                    assert_within(rf[kf][f, s], wt, rep[kp][idx, s], idx.size, f"replay draw {s} fun {f} {kf}")
                if f < len(A) - 1:
                    S = rep["cond_cov"][s][f]
                    assert_within(rf["cond_var"][f, s], [1.0, -2.0, 1.0], [S[0, 0], S[1, 0], S[1, 1]], 3, f"replay draw {s} contrast {f} cond_var")
        want_rep = host_summaries([dict(w=rf["w"][:, s], cond_mean=rf["cond_mean"][:, s], cond_var=rf["cond_var"][:, s], yhat=rf["yhat"][:, s])
                                   for s in range(keep)])
        for key in ("mean", "var", "w_mean", "yhat_mean"):
            assert np.array_equal(rf[key], want_rep[key]), key
    for s in range(keep):                                  # sums of the fit's own per-point outputs of that draw, yhat included
        for f, (idx, wt) in enumerate(A):
            idx, wt = np.asarray(idx), np.asarray(wt, dtype=np.float64)
            for kf, kp in (("w", "w"), ("cond_mean", "cond_mean"), ("yhat", "yhat")):
                assert_within(fun[kf][f, s], wt, out["new"][kp][idx, s], idx.size, f"draw {s} fun {f} {kf}")
            if not joint:
                assert_within(fun["cond_var"][f, s], wt * wt, out["new"]["cond_var"][idx, s], idx.size, f"draw {s} fun {f} cond_var")
            elif f < len(A) - 1:                           # the contrast at site f: Sigma_11 + Sigma_22 - 2 Sigma_12
                S = out["new"]["cond_cov"][s][f]
                assert_within(fun["cond_var"][f, s], [1.0, -2.0, 1.0], [S[0, 0], S[1, 0], S[1, 1]], 3, f"draw {s} contrast {f} cond_var")
    lasts = [dict(w=fun["w"][:, s], cond_mean=fun["cond_mean"][:, s], cond_var=fun["cond_var"][:, s], yhat=fun["yhat"][:, s]) for s in range(keep)]
    want = host_summaries(lasts)
    for key in ("mean", "var", "w_mean", "yhat_mean"):
        assert np.array_equal(fun[key], want[key]), key
    assert sorted(fun["quantiles"]) == sorted(QS)
    assert np.array_equal(fun["quantiles"][0.0][0], fun["w"].min(axis=1)) and np.array_equal(fun["quantiles"][1.0][1], fun["yhat"].max(axis=1))
    # summaries only: the same functional summaries, nothing per draw
    lean = fit_predict(pb, pts, mv, X, quantiles=QS, joint=labels, functionals=A, return_draws=False, save_w=False, save_yhat=False, **MCMC)
    lf = lean["new"]["functionals"]
    assert all(k not in lf for k in ("w", "cond_mean", "cond_var", "yhat"))
    for key in ("mean", "var", "w_mean", "yhat_mean"):
        assert np.array_equal(lf[key], fun[key]), key
    for q in QS:
        assert np.array_equal(lf["quantiles"][q][0], fun["quantiles"][q][0]) and np.array_equal(lf["quantiles"][q][1], fun["quantiles"][q][1]), q
