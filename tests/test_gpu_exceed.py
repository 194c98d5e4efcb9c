"""GPU: Rao-Blackwellised exceedance probabilities at new points (st_points_exceed_*, k_exceed_acc / k_exceed_fun_acc, the rb member
of stm_excursions, fit.spamtree_mv_mcmc(new_points=dict(exceed=)), predict.fit_predict(exceed=) and predict.predict_new(exceed=)).

The reference of every value is tests/exceed_reference.py, evaluated at 50 digits on the per-draw cond_mean, cond_var, F_m, F_v,
beta and tausq_inv that the same calls returned or were given; the allowed error is the bound DESIGN.md section 30 derives from
the kernels' operation chain, which exceed_reference states next to each value."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import exceed_reference as er
from tests import score_reference as sr
from tests.test_gpu_score import MCMC, accumulate, joint_set, model, plain_points, problem, same_tree, set_state, summaries

pytestmark = pytest.mark.gpu

ST_ERR_USAGE, ST_ERR_UNSUPPORTED = -1, -4
dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731

# thresholds from deep in one tail to deep in the other, the outermost 1e3 away; mixed sides.  Outcome j takes base + 0.1 j.
THR = {1: ([0.1], [-1]),
       3: ([-1e3, 0.2, 6.0], [-1, 1, 1]),
       8: ([-1e3, -6.0, -2.0, -0.3, 0.4, 2.5, 7.0, 1e3], [1, -1, 1, 1, -1, 1, -1, -1])}


def thresholds(T, q):
    base, side = THR[T]
    return [[b + 0.1 * j for j in range(q)] for b in base], side


def references(outs, betas, tis, X, mv, thr, side, ks, idx=None):
    """{k: (w refs, yhat refs)} over the first k draws for every k of ``ks``; refs[t][i] is exceed_reference.finish's tuple.  Each
    draw's 50-digit values are formed once and shared by the prefixes."""
    n = mv.size
    idx = range(n) if idx is None else idx
    S = max(ks)
    T = range(len(side))
    mw = [[er.moments_w(outs[s]["mean"][i], outs[s]["var"][i]) for s in range(S)] for i in idx]
    dw = [[[er.draw(m, thr[t][mv[i] - 1], side[t]) for m in mw[a]] for a, i in enumerate(idx)] for t in T]
    dy = None
    if X is not None:
        my = [[er.moments_yhat(X[i], betas[s][:, mv[i] - 1], outs[s]["mean"][i], outs[s]["var"][i], tis[s][mv[i] - 1]) for s in range(S)] for i in idx]
        dy = [[[er.draw(m, thr[t][mv[i] - 1], side[t]) for m in my[a]] for a, i in enumerate(idx)] for t in T]
    fin = lambda d, k: [[er.finish(pt[:k]) for pt in row] for row in d]   # noqa: E731
    return {k: (fin(dw, k), None if dy is None else fin(dy, k)) for k in ks}


def pick(ex, idx):
    return {key: np.asarray(v)[:, idx] for key, v in ex.items()}


# ---- 1. plain sets -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 3, 8])
@pytest.mark.parametrize("fg", [False, True], ids=["mfma", "generic"])
@pytest.mark.parametrize("q", [1, 2])
def test_plain_sets(q, fg, T):
    pb = problem(q)
    n, S = 301, 7
    pts, mv, anchor, X = plain_points(pb, n, 30 + q)
    thr, side = thresholds(T, q)
    hm = model(pb, fg)
    hm.set_points(pts, mv, anchor, X)
    hm.set_exceed(thr, side)
    got = {}
    outs, betas, tis = accumulate(hm, pb, S, after=lambda s: got.__setitem__(s + 1, hm.exceed()))
    assert ("k_points_generic" in hm.points_info()["routes"]) == fg
    hm.close()
    refs = references(outs, betas, tis, X, mv, thr, side, (1, 2, 7))
    for k in (1, 2, 7):
        assert got[k]["n_accumulated"] == k and got[k]["w"]["prob"].shape == (T, n)
        ww = er.check_target(got[k]["w"], refs[k][0], f"w k={k}")
        wy = er.check_target(got[k]["yhat"], refs[k][1], f"yhat k={k}")
        print(f"q={q} fg={fg} T={T} S={k}: worst error / bound: w prob {ww[0]:.3f} prob_var {ww[1]:.3f}; yhat prob {wy[0]:.3f} prob_var {wy[1]:.3f}")
    for t, (b, s) in enumerate(zip(*THR[T])):            # the far tails are exact
        if abs(b) == 1e3:
            want = 1.0 if (b < 0) == (s > 0) else 0.0
            for tg in ("w", "yhat"):
                assert np.all(got[7][tg]["prob"][t] == want) and np.all(got[7][tg]["prob_var"][t] == 0.0), (t, tg)


# ---- 2. bit identity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fg", [False, True], ids=["mfma", "generic"])
def test_every_other_output_is_the_same_bit_for_bit(fg):
    pb = problem(2)
    n, S = 301, 7
    pts, mv, anchor, X = plain_points(pb, n, 32)
    thr, side = thresholds(3, 2)

    def run(perm=None, exceed=True):
        hm = model(pb, fg)
        o = slice(None) if perm is None else perm
        hm.set_points(pts[o], mv[o], anchor[o], X[o])
        if exceed:
            hm.set_exceed(thr, side)
        hm._check(hm.lib.st_points_summary_reserve(hm.h, S))
        hm._check(hm.lib.st_points_summary_reset(hm.h))
        outs, _, _ = accumulate(hm, pb, S)
        res = (outs, summaries(hm, n), hm.exceed() if exceed else None)
        hm.close()
        return res

    outs, base, ex = run()
    outs0, base0, _ = run(exceed=False)                  # the same saved iterations without thresholds
    for a, b in zip(outs, outs0):
        for key in ("w", "mean", "var", "yhat"):
            assert np.array_equal(a[key], b[key]), key
    for a, b in zip(base, base0):
        assert np.array_equal(a, b)
    perm = np.random.default_rng(8).permutation(n)       # a permutation of the points: the same bits per point
    _, _, exp = run(perm)
    for tg in ("w", "yhat"):
        for key in ("prob", "prob_var"):
            assert np.array_equal(exp[tg][key], ex[tg][key][:, perm]), (tg, key)


# ---- 3. v = 0, the strict side -----------------------------------------------------------------------------------------------
def test_a_point_mass_at_the_threshold_is_on_neither_side():
    """Points on rows of their own conditioning set: nothing is left to draw, cond_var = max(rounding, 0).  Where it is exactly 0 the
    draw equals cond_mean; with c set to exactly that value neither w* > c nor w* < c holds."""
    from spamtree_amd.predict import conditioning_set, locate
    pb = problem(1)
    topo = pb["topo"]
    p0, mv0, a0, _ = plain_points(pb, 60, 45)
    rows = np.array([int(np.concatenate([topo.indexing(int(u)) for u in conditioning_set(topo, int(b))])[-1]) for b in a0])
    pts, mv = topo.coords[rows], topo.mv_id[rows]
    anchor = locate(topo, pts, mv, device=0)
    keep = np.array([r in np.concatenate([topo.indexing(int(u)) for u in conditioning_set(topo, int(b))]) for r, b in zip(rows, anchor)])
    pts, mv, anchor = pts[keep], mv[keep], anchor[keep]
    free, fmv, fa, _ = plain_points(pb, 5, 46)           # ... and a few ordinary points
    pts, mv, anchor = np.concatenate([pts, free]), np.concatenate([mv, fmv]), np.concatenate([anchor, fa])
    hm = model(pb)
    hm.set_points(pts, mv, anchor)
    one = hm.predict_points(mode=1)
    zero = np.nonzero(one["var"] == 0.0)[0]
    print(f"points on a conditioning row: {int(keep.sum())}, cond_var exactly 0 at {zero.size}")
    assert zero.size >= 1
    i0 = int(zero[0])
    c = float(one["mean"][i0])
    hm.set_exceed([c, c], [1, -1])
    out = hm.accumulate_points(seed=3, it=0)
    assert out["mean"][i0] == c and out["var"][i0] == 0.0 and out["w"][i0] == c
    ex = hm.exceed()
    assert ex["yhat"] is None and ex["n_accumulated"] == 1
    assert np.all(ex["w"]["prob"][:, i0] == 0.0) and np.all(ex["w"]["prob_var"] == 0.0)      # S = 1: no variance anywhere
    for i in zero:                                       # every point mass is an exact indicator, one side at most
        d = out["mean"][i] - c
        assert ex["w"]["prob"][0, i] == float(d > 0) and ex["w"]["prob"][1, i] == float(d < 0), i
    refs = references([out], None, None, None, mv, [[c], [c]], [1, -1], (1,))
    er.check_target(ex["w"], refs[1][0], "point masses and free points")
    assert not np.isnan(ex["w"]["prob"]).any()
    hm.close()


# ---- 4. against the existing kernels -----------------------------------------------------------------------------------------
def test_prob_yhat_is_one_minus_the_pit_of_the_scores():
    pb = problem(2)
    n, S = 101, 7
    pts, mv, anchor, X = plain_points(pb, n, 33)
    thr = [[0.3, -0.4]]
    hm = model(pb)
    hm.set_points(pts, mv, anchor, X)
    y = np.array([thr[0][j - 1] for j in mv])
    hm.set_scores(y)
    hm.set_exceed(thr, 1)
    outs, betas, tis = accumulate(hm, pb, S)
    ex, sc = hm.exceed(), hm.scores(crps=False)
    hm.close()
    worst = 0.0
    for i in range(n):
        j = mv[i] - 1
        args = ([betas[s][:, j] for s in range(S)], [outs[s]["mean"][i] for s in range(S)], [outs[s]["var"][i] for s in range(S)],
                [tis[s][j] for s in range(S)])
        _, _, _, pit_bound = sr.point_scores(y[i], X[i], *args)
        _, prob_bound, _, _ = er.point_yhat(X[i], *args, y[i], 1)
        gap = abs(ex["yhat"]["prob"][0, i] + sc["pit"][i] - 1.0)
        worst = max(worst, gap / (prob_bound + pit_bound))
        assert gap <= prob_bound + pit_bound, (i, gap, prob_bound, pit_bound)
    print(f"prob_yhat(+1) + pit - 1: worst / (sum of the two bounds) {worst:.3f}")


def test_the_stored_draw_count_is_a_sum_of_bernoullis_with_these_probabilities():
    """An independent check of sign and side: given the chain, draw s exceeds with probability p_s, independently, so by Bernstein's
    inequality |count - sum p_s| <= L / 3 + sqrt(L^2 / 9 + 2 V L), V = sum p_s (1 - p_s), fails for a given point and threshold with
    probability at most 2 exp(-L); with L = ln(4 n T / 1e-6) the whole test fails by chance with probability below 1e-6."""
    pb = problem(2)
    n, S = 40, 200
    pts, mv, anchor, X = plain_points(pb, n, 34)
    thr, side = [[0.4, -0.3], [0.6, 0.1]], [1, -1]
    T = len(side)
    hm = model(pb)
    hm.set_points(pts, mv, anchor, X)
    hm._check(hm.lib.st_points_summary_reserve(hm.h, S))
    hm._check(hm.lib.st_points_summary_reset(hm.h))
    hm.set_exceed(thr, side)
    outs, _, _ = accumulate(hm, pb, S, theta=False)
    count = hm.points_excursions(S, thr, side=side)["w"]["count"]
    ex = hm.exceed()
    hm.close()
    L = math.log(4 * n * T / 1e-6)
    worst = 0.0
    for t in range(T):
        for i in range(n):
            mean, V = er.bernoulli_variance([o["mean"][i] for o in outs], [o["var"][i] for o in outs], thr[t][mv[i] - 1], side[t])
            width = L / 3 + math.sqrt(L * L / 9 + 2 * V * L)
            worst = max(worst, abs(count[t, i] - mean) / width)
            assert abs(count[t, i] - mean) <= width, (t, i, int(count[t, i]), mean, V)
            assert abs(S * ex["w"]["prob"][t, i] - mean) <= 1e-9
    print(f"|count - sum p_s| / Bernstein width: worst {worst:.3f} (S = {S}, L = {L:.2f})")


# ---- 5. joint set and functionals --------------------------------------------------------------------------------------------
def test_joint_set_and_functionals():
    from spamtree_amd.predict import locate
    pb = problem(3)
    pts, mv, X, labels = joint_set(pb, 63, n_sites=18, extra=False)
    sel = (labels % 3 == 0) | ((labels % 3 == 1) & (mv != 2)) | ((labels % 3 == 2) & (mv == 3))      # groups of 3, 2 and 1
    pts, mv, X, labels = pts[sel], mv[sel], X[sel], labels[sel]
    n = pts.shape[0]
    anchor = locate(pb["topo"], pts, mv, device=0, joint=labels)
    rng = np.random.default_rng(14)
    fun = [(np.zeros(0, dtype=np.int64), np.zeros(0)),                                                # an empty one
           (np.arange(n), np.full(n, 1.0 / n)),                                                     # over all points
           (np.array([0, n - 1]), np.array([1.0, -1.0])),                                           # a contrast
           (np.arange(0, n, 2), rng.standard_normal((n + 1) // 2)),
           (np.array([3]), np.array([2.0]))]
    thr, side = thresholds(3, 3)
    thr_fun = [[-1e3] * 5, [0.0, 0.05, -0.1, 0.3, 0.2], [0.0, 1.0, 2.0, 3.0, 4.0]]
    hm = model(pb)
    hm.set_points(pts, mv, anchor, X, joint=labels)
    assert sorted({g.size for g in hm.joint_groups}) == [1, 2, 3]
    hm.set_functionals(fun)
    hm.set_exceed(thr, side, thr_fun)
    S = 3
    lasts = []
    outs, betas, tis = accumulate(hm, pb, S, after=lambda s: lasts.append(hm.functionals_last()))
    ex = hm.exceed()
    hm.close()
    for o in outs:                                       # the points use max(Sigma_aa, 0)
        for k, m in enumerate(hm.joint_groups):
            assert np.array_equal(o["var"][m], np.maximum(np.diag(np.asarray(o["cov"][k])), 0.0))
    refs = references(outs, betas, tis, X, mv, thr, side, (S,))
    ww = er.check_target(ex["w"], refs[S][0], "joint w")
    wy = er.check_target(ex["yhat"], refs[S][1], "joint yhat")
    frefs = [[er.finish([er.draw_w(l["cond_mean"][f], l["cond_var"][f], thr_fun[t][f], side[t]) for l in lasts]) for f in range(5)]
             for t in range(3)]
    wf = er.check_target(ex["functionals"]["w"], frefs, "functionals")
    print(f"joint set: worst error / bound: w {ww[0]:.3f} {ww[1]:.3f}; yhat {wy[0]:.3f} {wy[1]:.3f}; functionals {wf[0]:.3f} {wf[1]:.3f}")
    fp = ex["functionals"]["w"]["prob"]
    assert all(l["cond_mean"][0] == 0.0 and l["cond_var"][0] == 0.0 for l in lasts)                   # the empty functional: m = v = 0
    assert fp[0, 0] == 0.0 and fp[1, 0] == 0.0 and fp[2, 0] == 0.0                                    # 0 < -1e3, 0 > 0, 0 > 0: none holds
    assert np.all(fp[0] == 0.0)


# ---- 6. the driver -----------------------------------------------------------------------------------------------------------
def manual_exceed(pb, pts, mv, X, fun, thr, side, thr_fun):
    """The saved iterations of fit_predict(**MCMC) (its default start values) stepped by hand: stm_step for the chain,
    st_points_accumulate on every saved one, st_points_exceed_get at the end."""
    from spamtree_amd import _lib, fit
    from spamtree_amd.model import _f64, _i64, functionals_csr
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
        pc, pmv, Xf = np.asfortranarray(pts), _i64(mv), np.asfortranarray(X)
        anchor = _i64(locate(pb["topo"], pts, mv, device=0))
        assert lib.stm_points_set_joint(c, n, dp(pc), ip(pmv), ip(anchor), dp(Xf), None, 0) == 0
        ptr, idx, wt = functionals_csr(fun, n)
        assert lib.stm_points_functionals_set(c, ptr.size - 1, ip(ptr), ip(idx), dp(wt)) == 0
        h = lib.stm_handle(c)
        t_, s_, f_ = np.ascontiguousarray(thr, dtype=np.float64), np.ascontiguousarray(side, dtype=np.int32), np.ascontiguousarray(thr_fun, dtype=np.float64)
        assert lib.st_points_exceed_set(h, t_.shape[0], dp(t_), s_.ctypes.data_as(C.POINTER(C.c_int32)), dp(f_)) == 0
        assert lib.stm_init(c) == 0
        saved = 0
        for m in range(thin * keep + burn):
            assert lib.stm_step(c, 1) == 0
            if m >= burn and (m - burn) % thin == 0 and saved < keep:
                assert lib.st_points_accumulate(h, MCMC["seed"], saved, None, None, None, None) == 0
                saved += 1
        T, nf = t_.shape[0], ptr.size - 1
        out = {k: dict(prob=np.zeros((T, m)), prob_var=np.zeros((T, m))) for k, m in (("w", n), ("yhat", n), ("fun", nf))}
        rb = {k: _lib.StRbOut(dp(v["prob"]), dp(v["prob_var"])) for k, v in out.items()}
        cnt = C.c_int64()
        assert lib.st_points_exceed_get(h, C.byref(rb["w"]), C.byref(rb["yhat"]), C.byref(rb["fun"]), C.byref(cnt)) == 0
        out["n_accumulated"] = cnt.value
        return out
    finally:
        lib.stm_destroy(c)
        del hold


def test_the_driver():
    from spamtree_amd.predict import fit_predict, predict_new
    pb = problem(2)
    pts, mv, _, X = plain_points(pb, 200, 19)
    n, keep = pts.shape[0], MCMC["mcmc_keep"]
    fun = [(np.arange(5), np.ones(5) / 5), (np.array([7, 9]), np.array([1.0, -1.0]))]
    thr, side = thresholds(3, 2)
    thr_fun = [[-1e3, 0.0], [0.1, 0.2], [0.5, -0.5]]
    spec = dict(thresholds=thr, side=side, thresholds_fun=thr_fun)
    base = fit_predict(pb, pts, mv, X, functionals=fun, **MCMC)
    out = fit_predict(pb, pts, mv, X, functionals=fun, exceed=spec, **MCMC)
    ex, fex = out["new"].pop("exceed"), out["new"]["functionals"].pop("exceed")
    for key in ("beta_mcmc", "tausq_mcmc", "theta_mcmc", "paramsd", "w_mcmc", "yhat_mcmc"):   # the chain is the same draw for draw
        same_tree(out[key], base[key], key)
    same_tree(out["new"], base["new"])                   # every other output, bit for bit
    assert ex["n_accumulated"] == keep and fex["n_accumulated"] == keep and ex["side"].tolist() == side
    # a manual loop over the C-ABI -- stm_create, the point set, the functionals, the thresholds, then stm_step and
    # st_points_accumulate on every saved iteration -- gives the driver's values bit for bit (sample_predicts off in both: the loop
    # has no st_predict)
    nop = dict(sample_predicts=False, save_w=False, save_yhat=False)
    fm = fit_predict(pb, pts, mv, X, functionals=fun, exceed=spec, return_draws=False, **nop, **MCMC)["new"]
    man = manual_exceed(pb, pts, mv, X, fun, thr, side, thr_fun)
    assert man["n_accumulated"] == keep
    same_tree(fm["exceed"]["w"], man["w"], "w")
    same_tree(fm["exceed"]["yhat"], man["yhat"], "yhat")
    same_tree(fm["functionals"]["exceed"]["w"], man["fun"], "fun")
    # ... and what it should be, from the fit's own per-draw outputs
    new = out["new"]
    idx = list(range(0, n, 5))
    outs = [dict(mean=new["cond_mean"][:, s], var=new["cond_var"][:, s]) for s in range(keep)]
    betas = [np.asarray(out["beta_mcmc"])[:, s, :] for s in range(keep)]
    tis = [1.0 / np.asarray(out["tausq_mcmc"])[:, s] for s in range(keep)]
    refs = references(outs, betas, tis, X, mv, thr, side, (keep,), idx)
    er.check_target(pick(ex["w"], idx), refs[keep][0], "driver w")
    # summaries only: the same values with nothing per draw on the host
    lean = fit_predict(pb, pts, mv, X, functionals=fun, exceed=spec, return_draws=False, save_w=False, save_yhat=False, **MCMC)
    same_tree(lean["new"]["exceed"], ex, "lean")
    same_tree(lean["new"]["functionals"]["exceed"], fex, "lean fun")
    # an exc whose only content is rb goes with the excursions of the stored draws in one request
    both = fit_predict(pb, pts, mv, X, functionals=fun, exceed=spec, excursions=dict(thresholds=0.2), **MCMC)
    same_tree(both["new"]["exceed"], ex, "with excursions")
    # the replay of the saved chain: the moments of w* are the fit's bit for bit, so are its probabilities.  The yhat target reads
    # 1 / tausq_inv, and the replay hands the device tausq_inv = 1 / tausq_mcmc, within 2 u of the fit's: held against the
    # restatement on the replay's own per-draw inputs.
    rep = predict_new(pb, out, pts, mv, X, seed=MCMC["seed"], device=0, functionals=fun, exceed=spec, return_moments=True)
    same_tree(rep["exceed"]["w"], ex["w"], "replay w")
    same_tree(rep["functionals"]["exceed"]["w"], fex["w"], "replay fun")
    assert rep["exceed"]["n_accumulated"] == keep
    routs = [dict(mean=rep["cond_mean"][:, s], var=rep["cond_var"][:, s]) for s in range(keep)]
    rrefs = references(routs, betas, tis, X, mv, thr, side, (keep,), idx)
    er.check_target(pick(rep["exceed"]["yhat"], idx), rrefs[keep][1], "replay yhat")
    same = all(np.array_equal(1.0 / tis[s], np.asarray(out["tausq_mcmc"])[:, s]) for s in range(keep))
    if same:                                             # the round trip of tausq was exact: then the yhat target's bits are the fit's too
        same_tree(rep["exceed"]["yhat"], ex["yhat"], "replay yhat")
    print(f"replay: tausq_inv round trip exact on every draw: {bool(same)}")


def test_two_chains_pool():
    from spamtree_amd.predict import fit_predict
    pb = problem(1)
    pts, mv, _, X = plain_points(pb, 60, 20)
    keep = MCMC["mcmc_keep"]
    thr, side = thresholds(3, 1)
    out = fit_predict(pb, pts, mv, X, exceed=dict(thresholds=thr, side=side), chains=2, chain_seeds=[11, 12], **MCMC)
    ex, new = out["new"]["exceed"], out["new"]
    assert ex["n_accumulated"] == 2 * keep and new["cond_mean"].shape == (60, 2 * keep)
    outs = [dict(mean=new["cond_mean"][:, s], var=new["cond_var"][:, s]) for s in range(2 * keep)]
    betas = [np.asarray(out["beta_mcmc"])[:, s, :] for s in range(2 * keep)]
    tis = [1.0 / np.asarray(out["tausq_mcmc"])[:, s] for s in range(2 * keep)]
    refs = references(outs, betas, tis, None, mv, thr, side, (2 * keep,))
    worst = er.check_target(ex["w"], refs[2 * keep][0], "two chains")
    print(f"two chains pooled: worst error / bound {worst[0]:.3f} {worst[1]:.3f}")
    one = fit_predict(pb, pts, mv, X, exceed=dict(thresholds=thr, side=side), **dict(MCMC, seed=11))
    assert not np.array_equal(one["new"]["exceed"]["w"]["prob"], ex["w"]["prob"])    # the second chain's draws are in


# ---- 7. lifecycle and refusals -----------------------------------------------------------------------------------------------
def test_lifecycle_and_refusals():
    from spamtree_amd import _lib
    pb = problem(2)
    n = 50
    pts, mv, anchor, X = plain_points(pb, n, 35)
    hm = model(pb)
    lib, h = hm.lib, hm.h
    err = lambda: lib.st_last_error(h).decode()          # noqa: E731
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))   # noqa: E731
    buf = dict(prob=np.full((3, n), -1.0), prob_var=np.full((3, n), -1.0))
    rb = _lib.StRbOut(dp(buf["prob"]), dp(buf["prob_var"]))
    cnt = C.c_int64(-5)
    one = np.zeros((1, 2))
    assert lib.st_points_exceed_set(h, 1, dp(one), None, None) == ST_ERR_USAGE and "before st_points_set" in err()
    hm.set_points(pts, mv, anchor, X)
    assert lib.st_points_exceed_get(h, C.byref(rb), None, None, C.byref(cnt)) == ST_ERR_USAGE and "before st_points_exceed_set" in err()
    hm.set_exceed([0.1, 0.3], [1, -1])
    assert lib.st_points_exceed_get(h, C.byref(rb), None, None, C.byref(cnt)) == ST_ERR_USAGE and "no iteration accumulated" in err()
    assert cnt.value == 0
    rng = np.random.default_rng(1)
    set_state(hm, pb, 0, rng)
    hm.accumulate_points(seed=5, it=0)
    hm.accumulate_points(seed=5, it=1)
    two = hm.exceed()
    assert two["n_accumulated"] == 2 and two["w"]["prob"].shape == (2, n)
    # what _set refuses, with the index in the text; the previous thresholds stay
    bad = np.array([[0.0, 0.0], [0.0, np.inf]])
    for args, text in (((9, dp(np.zeros((9, 2))), None, None), "n_thr = 9"), ((-1, dp(one), None, None), "n_thr = -1"),
                       ((2, dp(bad), None, None), "thr[3]"), ((2, dp(np.zeros((2, 2))), i32(np.array([1, 0], dtype=np.int32)), None), "side[1]"),
                       ((1, dp(one), None, dp(np.zeros(4))), "thr_fun before st_points_functionals_set")):
        assert lib.st_points_exceed_set(h, *args) == ST_ERR_USAGE and text in err(), (text, err())
    same_tree(hm.exceed(), two, "after the refusals")
    # replace: new thresholds, state zeroed; every other summary left alone
    base = hm.lib.st_points_summary_get(h, None, None, None, None, C.byref(cnt))
    assert base == 0 and cnt.value == 2
    hm.set_exceed([0.1, 0.3, 0.5], 1)
    assert lib.st_points_exceed_get(h, C.byref(rb), None, None, C.byref(cnt)) == ST_ERR_USAGE and cnt.value == 0
    assert hm.lib.st_points_summary_get(h, None, None, None, None, C.byref(cnt)) == 0 and cnt.value == 2
    o3 = hm.accumulate_points(seed=5, it=2)
    three = hm.exceed()
    assert three["n_accumulated"] == 1 and three["w"]["prob"].shape == (3, n) and np.all(three["w"]["prob_var"] == 0.0)
    # reset clears the state and keeps the thresholds
    hm._check(lib.st_points_summary_reset(h))
    assert lib.st_points_exceed_get(h, C.byref(rb), None, None, C.byref(cnt)) == ST_ERR_USAGE and "no iteration accumulated" in err()
    assert np.all(buf["prob"] == -1.0) and np.all(buf["prob_var"] == -1.0)               # a refusal writes nothing
    o4 = hm.accumulate_points(seed=5, it=2)
    assert np.array_equal(o3["mean"], o4["mean"])
    same_tree(hm.exceed(), three, "after reset")
    # functionals: their thresholds leave with them, the points' stay and keep accumulating
    hm.set_functionals([(np.arange(4), np.ones(4) / 4), (np.array([5]), np.array([1.0]))])
    hm.set_exceed([0.1, 0.3, 0.5], 1, thresholds_fun=[[0.0, 0.1]] * 3)
    hm.accumulate_points(seed=5, it=2)
    withf = hm.exceed()
    assert withf["functionals"]["w"]["prob"].shape == (3, 2)
    same_tree(withf["w"], three["w"], "with functionals")
    hm.set_functionals([(np.arange(3), np.ones(3) / 3)])
    fb = _lib.StRbOut(dp(np.zeros((3, 2))), None)
    assert lib.st_points_exceed_get(h, None, None, C.byref(fb), C.byref(cnt)) == ST_ERR_USAGE and "fun_w without functional thresholds" in err()
    assert "functionals" not in hm.exceed() and hm.exceed()["n_accumulated"] == 1
    hm.accumulate_points(seed=5, it=3)
    assert hm.exceed()["n_accumulated"] == 2
    # NULL outputs, NULL structs: nothing is written, the count still is
    assert lib.st_points_exceed_get(h, None, None, None, C.byref(cnt)) == 0 and cnt.value == 2
    only = _lib.StRbOut(None, dp(buf["prob_var"]))
    assert lib.st_points_exceed_get(h, C.byref(only), None, None, None) == 0
    assert np.all(buf["prob"] == -1.0) and np.all((buf["prob_var"] >= 0.0) & (buf["prob_var"] <= 0.25))
    # removal, and a new point set drops the thresholds
    hm.set_exceed(None)
    assert lib.st_points_exceed_get(h, C.byref(rb), None, None, None) == ST_ERR_USAGE and "before st_points_exceed_set" in err()
    hm.set_exceed(0.0)
    hm.set_points(pts, mv, anchor)                       # ... without X
    assert lib.st_points_exceed_get(h, C.byref(rb), None, None, None) == ST_ERR_USAGE and "before st_points_exceed_set" in err()
    hm.set_exceed(0.0)
    hm.accumulate_points(seed=5, it=0)
    assert lib.st_points_exceed_get(h, C.byref(rb), C.byref(rb), None, None) == ST_ERR_USAGE and "needs the regressors X" in err()
    assert hm.exceed()["yhat"] is None
    # an empty point set: ST_OK, nothing written
    hm.set_points(np.zeros((0, 2)), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))
    hm.set_exceed(0.0)
    hm.accumulate_points(seed=5, it=0)
    buf["prob"][:] = -1.0
    cnt.value = -5
    assert lib.st_points_exceed_get(h, C.byref(rb), None, None, C.byref(cnt)) == 0 and cnt.value == 1 and np.all(buf["prob"] == -1.0)
    hm.close()
    # limited_tree handles are refused like all new-point prediction
    from tests.util import make_problem
    hl = model(make_problem(side=20, q=1, seed=41, missing=0.1, p=2, limited_tree=True), limited=True)
    assert hl.lib.st_points_exceed_set(hl.h, 1, dp(one), None, None) == ST_ERR_UNSUPPORTED
    assert b"limited_tree and multi-GPU handles are not supported (out of scope)" in hl.lib.st_last_error(hl.h)
    assert hl.lib.st_points_exceed_get(hl.h, C.byref(rb), None, None, None) == ST_ERR_UNSUPPORTED
    hl.close()
