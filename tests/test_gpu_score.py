"""GPU: scores of held-out observations at new points (st_points_score_*, k_score_acc / k_score_joint_acc / k_score_crps,
stm_mcmc_scored, predict.fit_predict(y_new=) and predict.predict_new(y_new=)).

The reference of every value is tests/score_reference.py, evaluated at 50 digits (CRPS: exactly) on the per-draw cond_mean, cond_var,
packed cond_cov, yhat, beta and tausq_inv that the same calls returned or were given; the allowed error is the bound DESIGN.md
section 19 derives from the kernels' operation chains, which score_reference states next to each value."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from tests import score_reference as sr
from tests.util import make_problem

pytestmark = pytest.mark.gpu

ST_ERR_USAGE, ST_ERR_UNSUPPORTED = -1, -4
dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731

_PB = {}


def problem(q):
    if q not in _PB:
        _PB[q] = make_problem(side=20, q=q, seed=50 + q, missing=0.1, p=2)
    return _PB[q]


def model(pb, fg=False, limited=False):
    from spamtree_amd.model import SpamTreeMV
    rng = np.random.default_rng(6)
    hm = SpamTreeMV(pb["y"], pb["X"], pb["Z"], pb["coords"], pb["mv_id"], pb["blocking"], pb["gix_block"], pb["res_is_ref"],
                    pb["parents"], pb["children"], limited, pb["block_names"], pb["block_groups"], pb["indexing"],
                    rng.standard_normal(pb["n"]), np.zeros(pb["p"]), pb["theta"], 5.0, force_generic=fg)
    assert hm.get_loglik_comps_w(0)
    return hm


def plain_points(pb, n, seed):
    from spamtree_amd.predict import locate
    rng = np.random.default_rng(seed)
    lo, hi = pb["coords"].min(axis=0), pb["coords"].max(axis=0)
    pts = lo + (hi - lo) * rng.uniform(size=(n, 2))
    mv = rng.integers(1, pb["q"] + 1, size=n)
    return pts, mv, locate(pb["topo"], pts, mv, device=0), rng.standard_normal((n, pb["p"]))


def set_state(hm, pb, s, rng, tausq=None, theta=True):
    """Another w, beta, tausq and theta; returns (beta p x q, tausq_inv q) as the device got them."""
    hm.set_w(rng.standard_normal(pb["n"]))
    beta = np.asfortranarray(rng.standard_normal((pb["p"], pb["q"])))
    hm.beta_update(beta)
    hm.tausq_inv = 1.0 / (rng.uniform(0.05, 0.5, pb["q"]) if tausq is None else np.full(pb["q"], tausq))
    hm._check(hm.lib.st_set_tausq_inv(hm.h, dp(hm.tausq_inv)))
    if theta:
        hm.theta_update(0, pb["theta"] * (1.0 + 0.03 * s))
        assert hm.get_loglik_comps_w(0)
    return beta.copy(), hm.tausq_inv.copy()


def accumulate(hm, pb, S, state_seed=77, seed=9, after=None, **kw):
    """S saved iterations with a new state each: (outs, betas, tausq_invs); after(s) runs behind iteration s."""
    rng = np.random.default_rng(state_seed)
    outs, betas, tis = [], [], []
    for s in range(S):
        b, t = set_state(hm, pb, s, rng, **kw)
        outs.append(hm.accumulate_points(seed=seed, it=s))
        betas.append(b)
        tis.append(t)
        if after:
            after(s)
    return outs, betas, tis


def check_points(sc, y, X, mv, outs, betas, tis, tag, idx=None):
    """lpd and pit of every (listed) point within the bound of section 19; NaN exactly where y is."""
    S = len(outs)
    worst = [0.0, 0.0]
    for i in (range(y.size) if idx is None else idx):
        if np.isnan(y[i]):
            assert np.isnan(sc["lpd"][i]) and np.isnan(sc["pit"][i]), (tag, i)
            continue
        j = mv[i] - 1
        lpd, lb, pit, pb_ = sr.point_scores(y[i], X[i], [betas[s][:, j] for s in range(S)], [outs[s]["mean"][i] for s in range(S)],
                                            [outs[s]["var"][i] for s in range(S)], [tis[s][j] for s in range(S)])
        el, ep = abs(float(sr.mp.mpf(float(sc["lpd"][i])) - lpd)), abs(float(sr.mp.mpf(float(sc["pit"][i])) - pit))
        worst = [max(worst[0], el / lb), max(worst[1], ep / pb_)]
        assert np.isfinite(sc["lpd"][i]) and el <= lb, (tag, i, el, lb)
        assert 0.0 <= sc["pit"][i] <= 1.0 and ep <= pb_, (tag, i, ep, pb_)
    print(f"{tag}: S={S} worst error / bound: lpd {worst[0]:.3f} pit {worst[1]:.3f}")


def summaries(hm, n, qs=(0.0, 0.4, 1.0)):
    """Everything the summaries return, for bit comparisons."""
    m, v, wm, ym = (np.zeros(n) for _ in range(4))
    cnt = C.c_int64()
    hm._check(hm.lib.st_points_summary_get(hm.h, dp(m), dp(v), dp(wm), dp(ym), C.byref(cnt)))
    out = [m, v, wm, ym, np.array([cnt.value])]
    for q in qs:
        a, b = np.zeros(n), np.zeros(n)
        hm._check(hm.lib.st_points_summary_quantile(hm.h, q, dp(a), dp(b)))
        out += [a, b]
    return out


# ---- 1. plain sets ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fg", [False, True], ids=["mfma", "generic"])
@pytest.mark.parametrize("q", [1, 2])
def test_plain_sets(q, fg):
    pb = problem(q)
    n, S = 301, 7
    pts, mv, anchor, X = plain_points(pb, n, 30 + q)
    rng = np.random.default_rng(5)
    y = 1.5 * rng.standard_normal(n)
    y[rng.uniform(size=n) < 0.15] = np.nan
    y[0], y[n - 1] = np.nan, 0.25
    hm = model(pb, fg)
    hm.set_points(pts, mv, anchor, X)
    hm.set_scores(y)
    hm._check(hm.lib.st_points_summary_reserve(hm.h, S))
    hm._check(hm.lib.st_points_summary_reset(hm.h))
    got = {}
    outs, betas, tis = accumulate(hm, pb, S, after=lambda s: got.__setitem__(s + 1, hm.scores(crps=False)))
    assert ("k_points_generic" in hm.points_info()["routes"]) == fg
    for k in (1, 2, 7):
        assert got[k]["n_scored"] == int(np.sum(~np.isnan(y))) and got[k]["n_degenerate"] == 0
        check_points(got[k], y, X, mv, outs[:k], betas[:k], tis[:k], f"q={q} fg={fg}")
    base = summaries(hm, n)
    tot = got[7]["totals"]
    assert tot["lpd"] == np.mean(got[7]["lpd"][~np.isnan(y)]) and tot["by_outcome"]["pit"].shape == (q,)
    hm.close()

    # the same saved iterations without scores: every output of st_points_accumulate and of the summaries, bit for bit
    h0 = model(pb, fg)
    h0.set_points(pts, mv, anchor, X)
    h0._check(h0.lib.st_points_summary_reserve(h0.h, S))
    h0._check(h0.lib.st_points_summary_reset(h0.h))
    outs0, _, _ = accumulate(h0, pb, S)
    for a, b in zip(outs, outs0):
        for key in ("w", "mean", "var", "yhat"):
            assert np.array_equal(a[key], b[key]), key
    for a, b in zip(base, summaries(h0, n)):
        assert np.array_equal(a, b)
    h0.close()

    # a permutation of the points: the same bits per point
    perm = np.random.default_rng(8).permutation(n)
    hp = model(pb, fg)
    hp.set_points(pts[perm], mv[perm], anchor[perm], X[perm])
    hp.set_scores(y[perm])
    accumulate(hp, pb, S)
    sp = hp.scores(crps=False)
    for key in ("lpd", "pit"):
        assert np.array_equal(sp[key], got[7][key][perm], equal_nan=True), key
    hp.close()


# ---- 2. the edges of the streaming log-sum-exp --------------------------------------------------------------------------------
def test_log_sum_exp_edges():
    pb = problem(1)
    n = 64
    pts, mv, anchor, X = plain_points(pb, n, 41)
    X[:, 0] = 1.0                                      # beta[0] shifts every predictive mean
    hm = model(pb)
    hm.set_points(pts, mv, anchor, X)
    rng = np.random.default_rng(3)
    set_state(hm, pb, 0, rng, tausq=0.2)
    b1 = 0.7
    cm = hm.predict_points(mode=1)["mean"]
    centre = cm + b1 * X[:, 1]                         # y - mu = -beta[0] up to rounding when y = centre

    def run(y, b0s):
        hm.set_scores(y)
        outs, betas, tis = [], [], []
        for s, b0 in enumerate(b0s):
            beta = np.asfortranarray(np.array([[b0], [b1]]))
            hm.beta_update(beta)
            outs.append(hm.accumulate_points(seed=4, it=s))
            betas.append(beta)
            tis.append(hm.tausq_inv.copy())
        return hm.scores(crps=False), outs, betas, tis

    def ells(y, outs, betas, tis, i):
        return [float(sr.point_draw(y[i], X[i], betas[s][:, 0], outs[s]["mean"][i], outs[s]["var"][i], tis[s][0])[0]) for s in range(len(outs))]

    for tag, b0s in (("rising", [6.0, 4.0, 2.0, 0.5]), ("falling", [0.5, 2.0, 4.0, 6.0]), ("ties", [1.0, 1.0, 1.0]),
                     ("mixed", [3.0, 1.0, 1.0, 5.0, 0.0, 0.0, 2.0]), ("single", [1.5])):
        sc, outs, betas, tis = run(centre, b0s)
        for i in (0, n // 2, n - 1):                   # the sequences do what their names say: each branch of the update runs
            e = ells(centre, outs, betas, tis, i)
            d = np.diff(e)
            assert {"rising": np.all(d > 0), "falling": np.all(d < 0), "ties": np.all(d == 0)}.get(tag, True), (tag, e)
        check_points(sc, centre, X, mv, outs, betas, tis, tag)
    # 40 sigma and more out: every exp l underflows, lpd stays finite and within the bound
    far = centre + 64.0                                # sigma <= sqrt(2.3 + 0.2) = 1.6: at least 40 sigma
    sc, outs, betas, tis = run(far, [0.0, 0.5, -0.5, 0.25])
    for i in range(n):
        assert max(ells(far, outs, betas, tis, i)) < -745.2 and np.isfinite(sc["lpd"][i])
        assert sc["pit"][i] >= 1.0 - 1e-15
    check_points(sc, far, X, mv, outs, betas, tis, "40 sigma")
    hm.close()


# ---- 3. CRPS -----------------------------------------------------------------------------------------------------------------
CRPS_K = (1, 2, 3, 4, 5, 64, 65, 2049, 4097, 8193)     # R = 8 up to 2048 draws, then 4, 2 (and 1 beyond 8192) rows a workgroup


def test_crps():
    pb = problem(1)
    n = 37                                             # no multiple of any R
    pts, mv, anchor, X = plain_points(pb, n, 43)
    hm = model(pb)
    hm.set_points(pts, mv, anchor, X)
    set_state(hm, pb, 0, np.random.default_rng(2), tausq=0.3)
    its = lambda k: k - (k // 3)                       # noqa: E731   every third draw repeats the one before it: duplicates
    first = np.stack([hm.accumulate_points(seed=11, it=its(k))["yhat"] for k in range(5)])
    y = np.empty(n)
    y[0::4], y[1::4] = -1e3, 1e3                       # below all draws, above all
    y[2::4] = first[0, 2::4]                           # equal to one of them
    y[3::4] = first.mean(axis=0)[3::4]
    y[n - 1] = np.nan
    hm.set_scores(y)
    hm.accumulate_points(seed=11, it=0)
    assert hm.lib.st_points_score_get(hm.h, None, None, dp(np.zeros(n)), None, None, None) == ST_ERR_USAGE   # no stored draw
    assert b"crps needs a stored draw" in hm.lib.st_last_error(hm.h)
    hm._check(hm.lib.st_points_summary_reserve(hm.h, max(CRPS_K)))
    hm._check(hm.lib.st_points_summary_reset(hm.h))
    draws = np.zeros((max(CRPS_K), n))
    got = {}
    for k in range(max(CRPS_K)):
        draws[k] = hm.accumulate_points(seed=11, it=its(k))["yhat"]
        if k + 1 in CRPS_K:
            got[k + 1] = hm.scores()["crps"]
    assert np.array_equal(draws[:5], first) and np.array_equal(draws[2], draws[3])
    for K in CRPS_K:
        worst = 0.0
        for i in range(n):
            if np.isnan(y[i]):
                assert np.isnan(got[K][i])
                continue
            want, mad = sr.crps_sorted(draws[:K, i], y[i])
            err, tol = abs(Fraction(float(got[K][i])) - want), sr.crps_bound(K, mad)
            worst = max(worst, float(err) / tol if tol else 0.0)
            assert err <= tol, (K, i, float(err), tol)
        assert np.all(got[K][~np.isnan(y)] >= 0)
        print(f"crps K={K}: worst error / bound {worst:.3f}")
    hm.close()


def test_crps_of_fewer_points_than_a_workgroup_takes():
    """n = 5 points where a workgroup takes R = 8: the tile's last three rows are padding only.  K = 1, 3 and 4 stored draws (a
    padding column, one, none), y below, above and among the draws and one NaN; the reference and the bound of test_crps."""
    pb = problem(1)
    n = 5
    pts, mv, anchor, X = plain_points(pb, n, 47)
    hm = model(pb)
    hm.set_points(pts, mv, anchor, X)
    set_state(hm, pb, 0, np.random.default_rng(2), tausq=0.3)
    y = np.array([-1e3, 1e3, 0.0, 0.5, np.nan])
    hm.set_scores(y)
    hm._check(hm.lib.st_points_summary_reserve(hm.h, 4))
    draws = np.zeros((4, n))
    for k in range(4):
        draws[k] = hm.accumulate_points(seed=11, it=k)["yhat"]
        if k + 1 in (1, 3, 4):
            got = hm.scores()["crps"]
            assert np.isnan(got[4])
            for i in range(4):
                want, mad = sr.crps_sorted(draws[:k + 1, i], y[i])
                assert abs(Fraction(float(got[i])) - want) <= sr.crps_bound(k + 1, mad), (k + 1, i)
    hm.close()


def test_crps_of_a_point_does_not_depend_on_the_other_points():
    """The same stored draws in sets of different size and order: k_score_crps gives the same bits.  The draws of a point follow its
    index in the caller's order (the Philox counter), so the sets are built to keep each compared point at the same index."""
    pb = problem(1)
    pts, mv, anchor, X = plain_points(pb, 20, 44)
    y = np.linspace(-2.0, 2.0, 20)
    res = []
    for n in (20, 11):                                  # 11: other workgroup boundaries (R = 8), fewer neighbours
        hm = model(pb)
        hm.set_points(pts[:n], mv[:n], anchor[:n], X[:n])
        set_state(hm, pb, 0, np.random.default_rng(2), tausq=0.3)
        yy = y[:n].copy()
        if n == 11:
            yy[1::2] = np.nan                           # ... some of them not scored
        hm.set_scores(yy)
        hm._check(hm.lib.st_points_summary_reserve(hm.h, 9))
        for k in range(9):
            hm.accumulate_points(seed=11, it=k)
        res.append(hm.scores())
        hm.close()
    for key in ("crps", "lpd", "pit"):
        assert np.array_equal(res[0][key][0:11:2], res[1][key][0:11:2]), key
        assert np.all(np.isnan(res[1][key][1::2]))


# ---- 4. joint sets -----------------------------------------------------------------------------------------------------------
def joint_set(pb, seed, n_sites=40, extra=True):
    """Site groups of q = 3 outcomes, plus (extra) groups of 1, 2 and 16 points and a group of 3 whose last member repeats its
    first.  Returns pts, mv, X, labels."""
    rng = np.random.default_rng(seed)
    lo, hi = pb["coords"].min(axis=0), pb["coords"].max(axis=0)
    q = pb["q"]
    sites = lo + (hi - lo) * rng.uniform(size=(n_sites, 2))
    pts, mv, labels = [np.repeat(sites, q, axis=0)], [np.tile(np.arange(1, q + 1), n_sites)], [np.repeat(np.arange(n_sites), q)]
    if extra:
        for lab, g in ((1000, 1), (1001, 2), (1002, 16), (1004, 16), (1005, 2), (1006, 16)):
            c = lo + (hi - lo) * (0.3 + 0.02 * rng.uniform(size=(g, 2)))
            pts.append(c); mv.append(rng.integers(1, q + 1, size=g)); labels.append(np.full(g, lab))
        c = lo + (hi - lo) * rng.uniform(size=(2, 2))
        pts.append(c[[0, 1, 0]]); mv.append(np.array([2, 1, 2])); labels.append(np.full(3, 1003))
    pts, mv, labels = np.concatenate(pts), np.concatenate(mv), np.concatenate(labels)
    return pts, mv, rng.standard_normal((pts.shape[0], pb["p"])), labels


def joint_reference(groups, y, X, mv, outs, betas, tis, k, extra=0):
    """(lpd_joint, bound, n_degenerate) of group k (groups: the member indices of every group) from the per-draw outputs."""
    m = groups[k]
    o = m[~np.isnan(y[m])]
    if o.size == 0:
        return None
    pos = np.nonzero(~np.isnan(y[m]))[0]
    draws = []
    for s in range(len(outs)):
        Sig = np.asarray(outs[s]["cov"][k])[np.ix_(pos, pos)]
        draws.append(sr.joint_draw(y[o], X[o], [betas[s][:, mv[i] - 1] for i in o], outs[s]["mean"][o], Sig,
                                   [tis[s][mv[i] - 1] for i in o], extra=extra))
    return sr.joint_scores(draws)


def test_joint_sets():
    from spamtree_amd.predict import locate
    pb = problem(3)
    pts, mv, X, labels = joint_set(pb, 61)
    n = pts.shape[0]
    anchor = locate(pb["topo"], pts, mv, device=0, joint=labels)
    rng = np.random.default_rng(12)
    y = 1.2 * rng.standard_normal(n)
    site = labels < 1000
    y[(labels % 4 == 1) & site & (mv == 2)] = np.nan                  # a strict subset
    y[(labels % 4 == 2) & site & (mv != 3)] = np.nan                  # one member
    y[(labels % 4 == 3) & site] = np.nan                              # none
    sixteen = np.nonzero(labels == 1002)[0]
    y[sixteen[[1, 5, 6, 15]]] = np.nan                                # 12 of 16, the first and last gaps apart; 1004: all 16
    y[np.nonzero(labels == 1005)[0][0]] = np.nan                      # the second of two
    y[labels == 1006] = np.nan                                        # none of 16
    hm = model(pb)
    hm.set_points(pts, mv, anchor, X, joint=labels)
    assert sorted({g.size for g in hm.joint_groups}) == [1, 2, 3, 16]
    hm.set_scores(y)
    S = 3
    outs, betas, tis = accumulate(hm, pb, S)
    sc = hm.scores(crps=False)
    assert sc["n_degenerate"] == 0 and sc["lpd_joint"].shape == (len(hm.joint_groups),)
    check_points(sc, y, X, mv, outs, betas, tis, "joint set, per point")
    kinds, worst = set(), 0.0
    for k, m in enumerate(hm.joint_groups):
        ref = joint_reference(hm.joint_groups, y, X, mv, outs, betas, tis, k)
        n_obs = int(np.sum(~np.isnan(y[m])))
        kinds.add((m.size, n_obs))
        if ref is None:
            assert np.isnan(sc["lpd_joint"][k]), k
            continue
        err = abs(float(sr.mp.mpf(float(sc["lpd_joint"][k])) - ref[0]))
        worst = max(worst, err / ref[1])
        assert np.isfinite(sc["lpd_joint"][k]) and err <= ref[1], (k, m.size, n_obs, err, ref[1])
        if m.size == 1:                                               # g = 1 is the plain l of that point
            i = m[0]
            _, lb, _, _ = sr.point_scores(y[i], X[i], [b[:, mv[i] - 1] for b in betas], [o["mean"][i] for o in outs],
                                          [o["var"][i] for o in outs], [t[mv[i] - 1] for t in tis])
            assert abs(sc["lpd_joint"][k] - sc["lpd"][i]) <= lb + ref[1]
    print(f"joint groups: worst error / bound {worst:.3f}; (g, g_o) kinds {sorted(kinds)}")
    assert {(3, 3), (3, 2), (3, 1), (3, 0), (1, 1), (2, 2), (2, 1), (16, 16), (16, 12), (16, 0)} <= kinds
    dupk = [k for k, m in enumerate(hm.joint_groups) if labels[m[0]] == 1003][0]
    assert np.isfinite(sc["lpd_joint"][dupk])                         # Sigma singular: finite through tau2
    by_site = {tuple(pts[m[0]]): sc["lpd_joint"][k] for k, m in enumerate(hm.joint_groups) if m.size == 3 and labels[m[0]] < 1000}
    hm.close()

    # a group's value does not depend on the other groups, their order or the labels: the site groups alone (the narrow
    # instantiation of the kernel), in reverse, under other labels
    keep = np.nonzero(site)[0][::-1]
    keep = keep.reshape(-1, 3)[:, ::-1].reshape(-1)                   # sites reversed, members in their order
    h2 = model(pb)
    lab2 = 7 * (labels[keep].max() - labels[keep]) + 3
    h2.set_points(pts[keep], mv[keep], locate(pb["topo"], pts[keep], mv[keep], device=0, joint=lab2), X[keep], joint=lab2)
    h2.set_scores(y[keep])
    accumulate(h2, pb, S)
    s2 = h2.scores(crps=False)
    for k, m in enumerate(h2.joint_groups):
        assert np.array_equal(s2["lpd_joint"][k], by_site[tuple(pts[keep][m[0]])], equal_nan=True), k
    h2.close()


def test_degenerate_pivots_are_counted_and_nothing_is_nan():
    """Pairs of identical points with tau2 = 1e-30: Sigma + tau2 I rounds to the singular Sigma and the second pivot is rounding.
    The test repeats the kernel's two-column elimination in double to know which draws the device must count."""
    from spamtree_amd.predict import locate
    pb = problem(3)
    rng = np.random.default_rng(13)
    lo, hi = pb["coords"].min(axis=0), pb["coords"].max(axis=0)
    G = 24
    c = lo + (hi - lo) * rng.uniform(size=(G, 2))
    pts, mv, labels = np.repeat(c, 2, axis=0), np.repeat(rng.integers(1, 4, size=G), 2), np.repeat(np.arange(G), 2)
    X = rng.standard_normal((2 * G, pb["p"]))
    anchor = locate(pb["topo"], pts, mv, device=0, joint=labels)
    hm = model(pb)
    hm.set_points(pts, mv, anchor, X, joint=labels)
    y = rng.standard_normal(2 * G)
    hm.set_scores(y)
    S = 3
    outs, betas, tis = accumulate(hm, pb, S, tausq=1e-30)
    sc = hm.scores(crps=False)
    want = 0
    alive = np.zeros(len(hm.joint_groups), dtype=bool)
    for s in range(S):
        for k, m in enumerate(hm.joint_groups):
            Sg = np.asarray(outs[s]["cov"][k])
            tau2 = 1.0 / tis[s][mv[m[0]] - 1]
            a00, a11 = Sg[0, 0] + tau2, Sg[1, 1] + tau2
            bad = not a00 > 0
            if not bad:
                l10 = Sg[1, 0] / np.sqrt(a00)
                piv = float(Fraction(float(a11)) - Fraction(float(l10)) * Fraction(float(l10)))      # one rounding: the fma
                bad = not piv > 0
            want += bad
            alive[k] |= not bad
    print(f"degenerate draws: {want} of {S * G}")
    assert want >= 1 and sc["n_degenerate"] == want
    assert not np.any(np.isnan(sc["lpd_joint"])) and not np.any(np.isnan(sc["lpd"])) and not np.any(np.isnan(sc["pit"]))
    assert np.array_equal(np.isfinite(sc["lpd_joint"]), alive)        # no draw of positive density: log 0
    hm.close()


# ---- 5. the driver -----------------------------------------------------------------------------------------------------------
MCMC = dict(mcmc_keep=6, mcmc_burn=4, mcmc_thin=2, adapting=True, sample_theta=True, seed=1234, device=0)
QS = (0.1, 0.5, 0.9)


def same_tree(a, b, path="new"):
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
        a, b = np.asarray(a), np.asarray(b)
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), path


def manual_scores(pb, pts, mv, X, labels, y):
    """The saved iterations of fit_predict(**MCMC) (its default start values) stepped by hand: stm_step for the chain,
    st_points_accumulate on every saved one, st_points_score_get at the end."""
    from spamtree_amd import _lib, fit
    from spamtree_amd.model import _f64, _i64
    from spamtree_amd.predict import locate
    lib = _lib.load()
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))   # noqa: E731
    st, hold, n_all, p, q = fit._problem(pb["y"], pb["X"], pb["coords"], pb["mv_id"], pb["res_is_ref"], pb["parents"], pb["children"],
                                         pb["block_names"], pb["block_groups"], pb["indexing"])
    theta = _f64(pb["theta"])
    bounds = np.asfortranarray(np.asarray(pb["bounds"], dtype=np.float64))
    sd = np.asfortranarray(0.01 * np.eye(theta.size))
    opt = _lib.StOptions(0, 1, 0, 1, 0, 0)
    fl = _lib.StmFlags(int(MCMC["adapting"]), 1, 1, int(MCMC["sample_theta"]), 1, 0)
    c = C.c_void_p()
    assert lib.stm_create(C.byref(st), C.byref(opt), dp(bounds), dp(sd), dp(theta), theta.size, dp(np.zeros(p)), 0.1, MCMC["seed"],
                          C.byref(fl), C.byref(c)) == 0
    try:
        n = pts.shape[0]
        keep, burn, thin = MCMC["mcmc_keep"], MCMC["mcmc_burn"], MCMC["mcmc_thin"]
        pc, pmv, Xf, yy = np.asfortranarray(pts), _i64(mv), np.asfortranarray(X), _f64(y)
        lab = None if labels is None else _i64(labels)
        anchor = _i64(locate(pb["topo"], pts, mv, device=0, joint=labels))
        assert lib.stm_points_set_joint(c, n, dp(pc), ip(pmv), ip(anchor), dp(Xf), ip(lab) if lab is not None else None, keep) == 0
        assert lib.stm_points_score_set(c, dp(yy)) == 0
        assert lib.stm_init(c) == 0
        h = lib.stm_handle(c)
        saved = 0
        for m in range(thin * keep + burn):
            assert lib.stm_step(c, 1) == 0
            if m >= burn and (m - burn) % thin == 0 and saved < keep:
                assert lib.st_points_accumulate(h, MCMC["seed"], saved, None, None, None, None) == 0
                saved += 1
        out = dict(lpd=np.zeros(n), pit=np.zeros(n), crps=np.zeros(n))
        nj = C.c_int64(0)
        if lab is not None:
            assert lib.st_points_joint_layout(h, C.byref(nj), None, None, None) == 0
            out["lpd_joint"] = np.zeros(nj.value)
        ns, nd = C.c_int64(), C.c_int64()
        assert lib.st_points_score_get(h, dp(out["lpd"]), dp(out["pit"]), dp(out["crps"]), dp(out["lpd_joint"]) if lab is not None else None,
                                       C.byref(ns), C.byref(nd)) == 0
        out.update(n_scored=ns.value, n_degenerate=nd.value)
        return out
    finally:
        lib.stm_destroy(c)
        del hold


@pytest.mark.parametrize("joint", [False, True], ids=["plain", "joint"])
def test_the_driver(joint):
    from spamtree_amd.predict import fit_predict, group_sites, predict_new
    pb = problem(3 if joint else 1)
    rng = np.random.default_rng(21)
    if joint:
        pts, mv, X, _ = joint_set(pb, 62, n_sites=60, extra=False)
        labels = group_sites(pts)
    else:
        pts, mv, _, X = plain_points(pb, 200, 19)
        labels = None
    n = pts.shape[0]
    y = 1.5 * rng.standard_normal(n)
    y[rng.uniform(size=n) < 0.2] = np.nan
    if joint:                                                         # sites with no observed member, with one, the others mixed
        y[(labels % 5 == 0)] = np.nan
        y[(labels % 5 == 1) & (mv != 2)] = np.nan
    keep = MCMC["mcmc_keep"]
    fun = [(np.arange(5), np.ones(5) / 5)]
    base = fit_predict(pb, pts, mv, X, quantiles=QS, joint=labels, functionals=fun, **MCMC)      # stm_mcmc_functionals
    out = fit_predict(pb, pts, mv, X, quantiles=QS, joint=labels, functionals=fun, y_new=y, **MCMC)
    sc = out["new"].pop("scores")
    for key in ("beta_mcmc", "tausq_mcmc", "theta_mcmc", "paramsd", "w_mcmc", "yhat_mcmc"):
        same_tree(out[key], base[key], key)
    same_tree(out["new"], base["new"])                                # every older output, bit for bit
    assert sc["n_scored"] == int(np.sum(~np.isnan(y))) and sc["n_degenerate"] == 0
    # the scores against the restatement on the fit's own per-draw outputs
    new = out["new"]
    outs = [dict(mean=new["cond_mean"][:, s], var=new["cond_var"][:, s]) for s in range(keep)]
    betas = [np.asarray(out["beta_mcmc"])[:, s, :] for s in range(keep)]
    tis = [1.0 / np.asarray(out["tausq_mcmc"])[:, s] for s in range(keep)]
    # summaries only: the same scores with nothing per draw on the host
    lean = fit_predict(pb, pts, mv, X, quantiles=QS, joint=labels, functionals=fun, y_new=y, return_draws=False, save_w=False,
                       save_yhat=False, **MCMC)
    same_tree(lean["new"]["scores"], sc, "lean scores")
    # the replay scores the same draws through the manual st_points_accumulate loop.  It hands the device tis = 1 / tausq_mcmc
    # itself, the fit had the tausq_inv whose reciprocal was saved: within 2 u of tis, 2 u (r^2 + 1) in l and 2 u (|r| + 1) in
    # Phi to first order.  Both are held against the restatement on their own per-draw outputs (a joint set's replayed moments
    # agree with the fit's to rounding only, tests/test_gpu_predict_joint.py).
    rep = predict_new(pb, out, pts, mv, X, seed=MCMC["seed"], device=0, joint=labels, y_new=y, quantiles=QS, return_moments=True)
    rs = rep["scores"]
    assert rs["n_scored"] == sc["n_scored"] and rs["n_degenerate"] == 0
    routs = [dict(mean=rep["cond_mean"][:, s], var=rep["cond_var"][:, s]) for s in range(keep)]
    for i in range(0, n, 3):
        if np.isnan(y[i]):
            assert np.isnan(sc["lpd"][i]) and np.isnan(sc["crps"][i]) and np.isnan(rs["lpd"][i])
            continue
        j = mv[i] - 1
        for got, oo, yh, slack in ((sc, outs, new["yhat"], 1.0), (rs, routs, rep["yhat"], 0.0)):
            lpd, lb, pit, pbd = sr.point_scores(y[i], X[i], [b[:, j] for b in betas], [o["mean"][i] for o in oo], [o["var"][i] for o in oo],
                                                [t[j] for t in tis])
            r2 = max(float(sr.point_draw(y[i], X[i], betas[s][:, j], oo[s]["mean"][i], oo[s]["var"][i], tis[s][j])[1]) ** 2 for s in range(keep))
            assert abs(float(sr.mp.mpf(float(got["lpd"][i])) - lpd)) <= lb + slack * 2 * sr.U * (r2 + 1), i
            assert abs(float(sr.mp.mpf(float(got["pit"][i])) - pit)) <= pbd + slack * 2 * sr.U * (np.sqrt(r2) + 1), i
            want, mad = sr.crps_sorted(yh[i, :], y[i])
            assert abs(Fraction(float(got["crps"][i])) - want) <= sr.crps_bound(keep, mad), i
    cover = (y >= new["quantiles"][0.1][1]) & (y <= new["quantiles"][0.9][1])
    assert sc["totals"]["coverage"] == np.mean(cover[~np.isnan(y)])
    assert sc["totals"]["crps"] == np.mean(sc["crps"][~np.isnan(y)])
    if joint:
        # lpd_joint of the fit and of the replay against the restatement on their own per-draw cond_cov and cond_mean, group by
        # group in the order of `groups` (the fit's tausq_inv: within 2 u of tis, two more u tr A in the bound)
        groups = new["groups"]
        assert sc["lpd_joint"].shape == (len(groups),) and rs["lpd_joint"].shape == (len(groups),)
        assert all(np.array_equal(a, b) for a, b in zip(groups, rep["groups"]))
        kinds, worst = set(), 0.0
        for got, oo, cc, extra in ((sc, outs, new["cond_cov"], 2), (rs, routs, rep["cond_cov"], 0)):
            jo = [dict(mean=oo[s]["mean"], cov=cc[s]) for s in range(keep)]
            for k, m in enumerate(groups):
                ref = joint_reference(groups, y, X, mv, jo, betas, tis, k, extra=extra)
                kinds.add(int(np.sum(~np.isnan(y[m]))))
                if ref is None:
                    assert np.isnan(got["lpd_joint"][k]), k
                    continue
                err = abs(float(sr.mp.mpf(float(got["lpd_joint"][k])) - ref[0]))
                worst = max(worst, err / ref[1])
                assert np.isfinite(got["lpd_joint"][k]) and err <= ref[1], (k, err, ref[1])
        print(f"driver lpd_joint: worst error / bound {worst:.3f}")
        assert kinds == {0, 1, 2, 3}
    # a manual loop over the C-ABI -- stm_create, the point set, the scores, then stm_step and st_points_accumulate on every saved
    # iteration -- gives the scores of stm_mcmc_scored bit for bit (sample_predicts off in both: the loop has no st_predict)
    nop = dict(sample_predicts=False, save_w=False, save_yhat=False)
    fm = fit_predict(pb, pts, mv, X, joint=labels, y_new=y, return_draws=False, **nop, **MCMC)["new"]["scores"]
    ml = manual_scores(pb, pts, mv, X, labels, y)
    for key in ("lpd", "pit", "crps") + (("lpd_joint",) if joint else ()):
        assert np.array_equal(ml[key], fm[key], equal_nan=True), key
    assert ml["n_scored"] == fm["n_scored"] and ml["n_degenerate"] == fm["n_degenerate"]
    # crps=False: the same lpd and pit with no draw kept on the device
    nc = fit_predict(pb, pts, mv, X, joint=labels, y_new=y, crps=False, return_draws=False, **nop, **MCMC)["new"]["scores"]
    assert nc["crps"] is None and "crps" not in nc["totals"]
    assert np.array_equal(nc["lpd"], fm["lpd"], equal_nan=True) and np.array_equal(nc["pit"], fm["pit"], equal_nan=True)
    # with tausq fixed (1 / 0.1 = 10 and back, exactly) a plain set's replay is the manual st_points_accumulate loop over the same
    # states bit for bit, and so are the scores
    if not joint:
        fx = fit_predict(pb, pts, mv, X, y_new=y, sample_tausq=False, **MCMC)
        rx = predict_new(pb, fx, pts, mv, X, seed=MCMC["seed"], device=0, y_new=y)
        assert len({tuple(c) for c in np.asarray(fx["theta_mcmc"]).T}) >= 2
        assert np.array_equal(rx["yhat"], fx["new"]["yhat"])
        for key in ("lpd", "pit", "crps"):
            assert np.array_equal(rx["scores"][key], fx["new"]["scores"][key], equal_nan=True), key


# ---- 6. lifecycle and refusals -----------------------------------------------------------------------------------------------
def test_lifecycle_and_refusals():
    pb = problem(1)
    hm = model(pb)
    lib, h = hm.lib, hm.h
    n = 40
    y = np.linspace(-1.0, 1.0, n)
    out = np.zeros(n)
    assert lib.st_points_score_set(h, dp(y)) == ST_ERR_USAGE and b"before st_points_set" in lib.st_last_error(h)   # no point set
    assert lib.st_points_score_get(h, dp(out), None, None, None, None, None) == ST_ERR_USAGE
    pts, mv, anchor, X = plain_points(pb, n, 16)
    hm.set_points(pts, mv, anchor)                                                                      # no X
    assert lib.st_points_score_set(h, dp(y)) == ST_ERR_USAGE and b"need the regressors X" in lib.st_last_error(h)
    assert lib.st_points_score_set(h, None) == 0                                                        # nothing to remove
    hm.set_points(pts, mv, anchor, X)
    assert lib.st_points_score_get(h, dp(out), None, None, None, None, None) == ST_ERR_USAGE
    assert b"before st_points_score_set" in lib.st_last_error(h)
    bad = y.copy(); bad[17] = -np.inf
    assert lib.st_points_score_set(h, dp(bad)) == ST_ERR_USAGE and b"y_new[17] is infinite" in lib.st_last_error(h)
    hm.set_scores(y)
    rng = np.random.default_rng(1)
    w_a, w_b = rng.standard_normal(pb["n"]), rng.standard_normal(pb["n"])
    hm.set_w(w_a)
    ns = C.c_int64(-1)
    assert lib.st_points_score_get(h, dp(out), None, None, None, C.byref(ns), None) == ST_ERR_USAGE and ns.value == n   # before any draw
    assert b"no iteration accumulated" in lib.st_last_error(h)
    hm.accumulate_points(seed=3, it=0)
    assert lib.st_points_score_set(h, dp(bad)) == ST_ERR_USAGE                                          # the previous scores stay
    one = hm.scores(crps=False)
    assert np.all(np.isfinite(one["lpd"])) and one["lpd_joint"] is None
    assert lib.st_points_score_get(h, None, None, None, dp(out), None, None) == ST_ERR_USAGE            # lpd_joint on a plain set
    assert b"st_points_set_joint" in lib.st_last_error(h)
    assert lib.st_points_score_get(h, None, None, None, None, None, None) == 0                          # every output may be NULL
    hm.set_w(w_b)
    hm.accumulate_points(seed=3, it=1)
    two = hm.scores(crps=False)
    assert not np.array_equal(two["lpd"], one["lpd"])
    # replace: zeroed; the point summaries are left alone
    hm.set_scores(y)
    cnt = C.c_int64()
    assert lib.st_points_summary_get(h, dp(out), None, None, None, C.byref(cnt)) == 0 and cnt.value == 2
    assert lib.st_points_score_get(h, dp(out), None, None, None, None, None) == ST_ERR_USAGE
    hm.set_w(w_a)
    hm.accumulate_points(seed=3, it=0)
    assert np.array_equal(hm.scores(crps=False)["lpd"], one["lpd"])                                     # the same draw alone again
    # st_points_summary_reset clears them
    hm.set_w(w_b)
    hm.accumulate_points(seed=3, it=1)
    assert np.array_equal(hm.scores(crps=False)["lpd"], two["lpd"])
    hm.set_w(w_a)
    assert lib.st_points_summary_reset(h) == 0
    assert lib.st_points_score_get(h, dp(out), None, None, None, None, None) == ST_ERR_USAGE
    hm.accumulate_points(seed=3, it=0)
    assert np.array_equal(hm.scores(crps=False)["lpd"], one["lpd"])
    # every y NaN: predicted as before, nothing to score
    hm.set_scores(np.full(n, np.nan))
    hm.accumulate_points(seed=3, it=0)
    assert lib.st_points_score_get(h, dp(out), None, None, None, C.byref(ns), None) == ST_ERR_USAGE and ns.value == 0
    assert b"no point is scored" in lib.st_last_error(h)
    # remove; a new point set drops them
    hm.set_scores(None)
    hm.accumulate_points(seed=3, it=0)
    assert lib.st_points_score_get(h, dp(out), None, None, None, None, None) == ST_ERR_USAGE
    hm.set_scores(y)
    hm.set_points(pts, mv, anchor, X)
    assert lib.st_points_score_get(h, dp(out), None, None, None, None, None) == ST_ERR_USAGE
    assert b"before st_points_score_set" in lib.st_last_error(h)
    hm.close()
    # a limited_tree handle is refused as its siblings are, with their text
    pl = make_problem(side=20, q=1, seed=41, missing=0.1, p=2, limited_tree=True)
    hl = model(pl, limited=True)
    assert hl.lib.st_points_score_set(hl.h, dp(y)) == ST_ERR_UNSUPPORTED
    assert b"limited_tree and multi-GPU handles are not supported (out of scope)" in hl.lib.st_last_error(hl.h)
    assert hl.lib.st_points_score_get(hl.h, dp(out), None, None, None, None, None) == ST_ERR_UNSUPPORTED
    hl.close()
