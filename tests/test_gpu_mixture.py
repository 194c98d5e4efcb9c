"""GPU: quantiles and the exact CRPS of the mixture predictive at new points (st_points_mixture_*, k_mix_store / k_mix_quantile /
k_mix_crps, stm_fit_run's mix, fit.spamtree_mv_mcmc(new_points=dict(mixture=)), predict.fit_predict(mixture=) and
predict.predict_new(mixture=)).

The reference of every value is tests/mixture_reference.py, evaluated at 50 digits on the per-draw moments the device itself stored
(st_points_mixture_draws; the functionals' F_m and F_v from st_points_functionals_last).  A quantile is held to the definition --
F(x + delta) >= p - eps_F and F(x - delta) <= p + eps_F -- with the width and the rounding bound spamtree_amd/csrc/points_mixture.hpp
states; the CRPS and the spread to that header's bound.  The shapes are sized by the reference's cost (a 50-digit erfc per
component, series and probability; an erf and an exp per pair of components): every series of a launch is checked, so the long
stores meet the short point sets and the other way round."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import mixture_reference as mr
from tests import score_reference as sr
from tests.test_gpu_score import MCMC, accumulate, joint_set, model, plain_points, problem, same_tree, summaries

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spamtree_amd", "csrc")

ST_ERR_USAGE, ST_ERR_UNSUPPORTED = -1, -4
dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731

PROBS = {1: [0.5],
         3: [0.975, 0.025, 0.5],                                        # in no order: the results come back in the caller's
         8: [1e-6, 0.025, 0.1, 0.5, 0.9, 0.975, 1 - 1e-6, 0.3]}
WORST = {}   # worst error / bound of the run, by quantity: printed by each test as it goes (profiles/r04/mixture has one run's)


def note(key, ratio):
    WORST[key] = max(WORST.get(key, -math.inf), ratio)


@pytest.fixture(scope="module", autouse=True)
def worst_ratios():
    """After the module's tests: the worst error-over-bound ratios of the run in one place (each is asserted where it arises)."""
    yield
    for key in sorted(WORST):
        print(f"worst {key}: {WORST[key]:.3f}")


_TILE_ROWS = {}


def tile_rows(K, tmp_path_factory):
    """The series a workgroup of k_mix_quantile takes at K components under the device's 160 KB of LDS, asked of mix_quantile_plan
    itself (spamtree_amd/csrc/mixture_plan.cpp, compiled into a host program once per run)."""
    if not _TILE_ROWS:
        d = tmp_path_factory.mktemp("mixture_plan")
        src = d / "rows.cpp"
        src.write_text('#include <cstdio>\n#include "mixture_plan.hpp"\nint main() { for (long long K = 1; K <= ST_MIX_MAX_DRAWS; ++K) { MixPlan P; '
                       'if (!mix_quantile_plan(K, 1000, 163840, &P)) return 1; std::printf("%lld %d\\n", K, P.R); } return 0; }\n')
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        if not os.path.exists(hipcc):
            hipcc = shutil.which("hipcc")
        subprocess.run([hipcc, "--offload-host-only", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", CSRC, str(src),
                        os.path.join(CSRC, "mixture_plan.cpp"), "-o", str(d / "rows")], check=True, timeout=600)
        out = subprocess.run([str(d / "rows")], capture_output=True, text=True, timeout=60, check=True).stdout
        _TILE_ROWS.update({int(a): int(b) for a, b in (line.split() for line in out.splitlines())})
    return _TILE_ROWS[K]


def target_comps(dr, mv, K, i, target):
    if target == "w":
        return mr.components(dr["m"][:K, i], dr["v"][:K, i])
    return mr.components(dr["mu"][:K, i], dr["v"][:K, i], dr["tau2"][:K, mv[i] - 1])


def check_quantiles(got, probs, comps_of, n, tag):
    """Every series and probability of one target against the definition; the quantiles never decrease in p.  ``got``: T x n."""
    order = np.argsort(probs)
    worst = -math.inf
    for i in range(n):
        comps = comps_of(i)
        for t, p in enumerate(probs):
            r = mr.check_quantile(got[t, i], p, comps)
            worst = max(worst, r)
            assert r <= 1.0, (tag, i, p, got[t, i], r)
        assert np.all(np.diff(got[order, i]) >= 0.0), (tag, i)
    return worst


# ---- 1. the store ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fg", [False, True], ids=["mfma", "generic"])
def test_the_store_holds_what_accumulate_returned(fg):
    from spamtree_amd.exceed import xb_chain
    pb = problem(2)
    n, keep, S = 37, 5, 7
    pts, mv, anchor, X = plain_points(pb, n, 61)
    hm = model(pb, fg)
    lib, h = hm.lib, hm.h
    cnt = C.c_int64(-1)
    assert lib.st_points_mixture_reserve(h, 4) == ST_ERR_USAGE and b"before st_points_set" in lib.st_last_error(h)
    hm.set_points(pts, mv, anchor, X)
    assert lib.st_points_mixture_draws(h, None, None, None, None, C.byref(cnt)) == ST_ERR_USAGE
    assert b"before st_points_mixture_reserve" in lib.st_last_error(h)
    assert lib.st_points_mixture_reserve(h, 8193) == ST_ERR_UNSUPPORTED
    assert b"8193" in lib.st_last_error(h) and b"8192" in lib.st_last_error(h)
    hm.reserve_mixture(keep)
    assert lib.st_points_mixture_quantiles(h, 1, dp(np.array([0.5])), None, None, None) == ST_ERR_USAGE and b"no stored draw" in lib.st_last_error(h)
    outs, betas, tis = accumulate(hm, pb, S)
    assert ("k_points_generic" in hm.points_info()["routes"]) == fg
    dr = hm.mixture_draws()
    assert dr["n_stored"] == keep and dr["m"].shape == (keep, n) and dr["tau2"].shape == (keep, 2)     # draws beyond keep are not stored
    for s in range(keep):
        assert np.array_equal(dr["m"][s], outs[s]["mean"]) and np.array_equal(dr["v"][s], outs[s]["var"]), s
        assert np.array_equal(dr["tau2"][s], 1.0 / tis[s]), s
        for j in range(2):
            sel = mv == j + 1
            assert np.array_equal(dr["mu"][s][sel], xb_chain(X[sel], betas[s][:, j]) + outs[s]["mean"][sel]), (s, j)
    # the refusals of the probabilities name the index
    q8 = np.zeros((9, n))
    for bad, idx in (([0.5, 0.0], 1), ([1.0], 0), ([0.2, 0.3, np.nan], 2), ([-0.5], 0)):
        pr = np.array(bad)
        out = hm_out(q8)
        assert lib.st_points_mixture_quantiles(h, pr.size, dp(pr), C.byref(out[0]), None, None) == ST_ERR_USAGE
        assert f"probs[{idx}]".encode() in lib.st_last_error(h), bad
    pr = np.full(9, 0.5)
    assert lib.st_points_mixture_quantiles(h, 9, dp(pr), C.byref(hm_out(q8)[0]), None, None) == ST_ERR_USAGE and b"n_probs = 9" in lib.st_last_error(h)
    assert lib.st_points_mixture_quantiles(h, 1, dp(pr), None, None, C.byref(hm_out(q8)[0])) == ST_ERR_USAGE            # fun_w without functionals
    assert b"st_points_functionals_set" in lib.st_last_error(h)
    assert lib.st_points_mixture_crps(h, dp(np.zeros(n)), None, None) == ST_ERR_USAGE and b"before st_points_score_set" in lib.st_last_error(h)
    hm.set_scores(np.full(n, np.nan))
    assert lib.st_points_mixture_crps(h, dp(np.zeros(n)), None, C.byref(cnt)) == ST_ERR_USAGE and cnt.value == 0
    assert b"no point is scored" in lib.st_last_error(h)
    assert not q8.any()
    # st_points_summary_reset clears the count, the room stays
    hm._check(lib.st_points_summary_reset(h))
    assert hm.mixture_draws()["n_stored"] == 0
    two = [hm.accumulate_points(seed=9, it=s) for s in range(2)]
    dr = hm.mixture_draws()
    assert dr["n_stored"] == 2 and np.array_equal(dr["m"][1], two[1]["mean"])
    # st_points_functionals_set drops the functional part only: the functionals' store starts empty, the points' stays
    hm.set_functionals([(np.arange(3), np.ones(3) / 3)])
    assert hm.mixture_draws()["n_stored"] == 2
    out = hm_out(np.zeros((1, 1)))
    assert lib.st_points_mixture_quantiles(h, 1, dp(pr), None, None, C.byref(out[0])) == ST_ERR_USAGE and b"no stored draw" in lib.st_last_error(h)
    hm.accumulate_points(seed=9, it=2)
    fq = hm.mixture_quantiles([0.5])
    last = hm.functionals_last()
    r = mr.check_quantile(fq["functionals"]["w"][0, 0], 0.5, mr.components(last["cond_mean"][:1], last["cond_var"][:1]))
    assert r <= 1.0 and fq["functionals"]["n_unconverged"] == 0
    # keep = 0 releases the store; a new point set drops it
    hm.reserve_mixture(0)
    assert lib.st_points_mixture_draws(h, None, None, None, None, C.byref(cnt)) == ST_ERR_USAGE
    hm.reserve_mixture(3)
    hm.set_points(pts, mv, anchor)                       # no X
    assert lib.st_points_mixture_draws(h, None, None, None, None, C.byref(cnt)) == ST_ERR_USAGE
    hm.reserve_mixture(3)
    hm.accumulate_points(seed=9, it=0)
    assert lib.st_points_mixture_draws(h, None, None, dp(np.zeros(n)), None, C.byref(cnt)) == ST_ERR_USAGE and cnt.value == 1      # mu without X
    assert lib.st_points_mixture_quantiles(h, 1, dp(pr), None, C.byref(hm_out(q8)[0]), None) == ST_ERR_USAGE                      # yhat without X
    assert b"needs the regressors X" in lib.st_last_error(h)
    assert hm.mixture_quantiles([0.5])["yhat"] is None
    # an empty point set: ST_OK, nothing written
    hm.set_points(np.zeros((0, 2)), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))
    hm.reserve_mixture(2)
    hm.accumulate_points(seed=9, it=0)
    assert lib.st_points_mixture_quantiles(h, 1, dp(pr), C.byref(hm_out(q8)[0]), None, None) == 0 and not q8.any()
    hm.close()
    from tests.util import make_problem
    hl = model(make_problem(side=12, q=1, seed=41, missing=0.1, p=2, limited_tree=True), limited=True)   # limited_tree handles are refused
    assert hl.lib.st_points_mixture_reserve(hl.h, 4) == ST_ERR_UNSUPPORTED
    assert hl.lib.st_points_mixture_crps(hl.h, None, None, None) == ST_ERR_UNSUPPORTED
    hl.close()


def hm_out(q):
    """(st_mix_out over ``q``, its counter): the counter must outlive the call."""
    from spamtree_amd import _lib
    unc = C.c_int64()
    return _lib.StMixOut(dp(q), C.pointer(unc)), unc


@pytest.mark.parametrize("fg", [False, True], ids=["mfma", "generic"])
def test_every_other_output_is_the_same_bit_for_bit(fg):
    pb = problem(2)
    n, S = 301, 7
    pts, mv, anchor, X = plain_points(pb, n, 62)
    y = np.random.default_rng(5).standard_normal(n)
    y[::3] = np.nan
    probs = PROBS[3]

    def run(perm=None, mix=True):
        hm = model(pb, fg)
        o = slice(None) if perm is None else perm
        hm.set_points(pts[o], mv[o], anchor[o], X[o])
        hm.set_scores(y[o])
        hm.set_exceed([[0.2, -0.1]], 1)
        if mix:
            hm.reserve_mixture(S)
        hm._check(hm.lib.st_points_summary_reserve(hm.h, S))
        hm._check(hm.lib.st_points_summary_reset(hm.h))
        outs, _, _ = accumulate(hm, pb, S)
        sc, ex = hm.scores(), hm.exceed()
        res = (outs, summaries(hm, n), sc, ex, (hm.mixture_quantiles(probs), hm.mixture_crps()) if mix else None)
        hm.close()
        return res

    outs, base, sc, ex, mx = run()
    outs0, base0, sc0, ex0, _ = run(mix=False)           # the same saved iterations without the store
    for a, b in zip(outs, outs0):
        for key in ("w", "mean", "var", "yhat"):
            assert np.array_equal(a[key], b[key]), key
    for a, b in zip(base, base0):
        assert np.array_equal(a, b)
    same_tree(sc, sc0, "scores")
    same_tree(ex, ex0, "exceed")
    perm = np.random.default_rng(8).permutation(n)       # a permutation of the points: the same bits per point
    _, _, _, _, mxp = run(perm)
    for tg in ("w", "yhat"):
        assert np.array_equal(mxp[0][tg], mx[0][tg][:, perm]), tg
    for key in ("crps", "spread"):
        assert np.array_equal(mxp[1][key], mx[1][key][perm], equal_nan=True), key
    assert mx[0]["n_unconverged"] == 0 and mx[1]["n_scored"] == int(np.sum(~np.isnan(y)))
    assert np.array_equal(np.isnan(mx[1]["crps"]), np.isnan(y)) and np.array_equal(np.isnan(mx[1]["spread"]), np.isnan(y))


# ---- 2. quantiles ------------------------------------------------------------------------------------------------------------
# (q, generic route, the point sets' sizes, {stored draws K: probabilities T}).  n = 7 and 9 straddle the tile of 8 series a
# workgroup takes up to K = 256, n = 1, 6 and 8 the tile of 7 at K = 257: the test asks the plan for both.
QUANTILE_CASES = {
    "q2-mfma-n301": (2, False, (301,), {1: 8, 2: 8, 63: 1}),
    "q1-generic-n41": (1, True, (41,), {64: 3, 65: 3}),
    "q2-generic-tiles": (2, True, (7, 9), {63: 3, 65: 3}),
    "q1-mfma-K257-n1": (1, False, (1,), {257: 8}),
    "q1-mfma-K257-n6": (1, False, (6,), {257: 3}),
    "q1-mfma-K257-n8": (1, False, (8,), {257: 1}),
}


@pytest.mark.parametrize("case", sorted(QUANTILE_CASES))
def test_quantiles(case, tmp_path_factory):
    q, fg, sizes, shapes = QUANTILE_CASES[case]
    pb = problem(q)
    S = max(shapes)
    if len(sizes) == 2:                                  # the two sizes straddle the tile at every K they are checked at
        assert all(sizes == (tile_rows(K, tmp_path_factory) - 1, tile_rows(K, tmp_path_factory) + 1) for K in shapes)
    for n in sizes:
        if S > 100:
            R = tile_rows(S, tmp_path_factory)
            assert n in (1, R - 1, R + 1)
        pts, mv, anchor, X = plain_points(pb, n, 63 + n)
        hm = model(pb, fg)
        hm.set_points(pts, mv, anchor, X)
        hm.reserve_mixture(S)
        got = {}
        accumulate(hm, pb, S, theta=S <= 65,
                   after=lambda s: got.__setitem__(s + 1, dict(hm.mixture_quantiles(PROBS[shapes[s + 1]]), info=hm.mixture_info()))
                   if s + 1 in shapes else None)
        assert ("k_points_generic" in hm.points_info()["routes"]) == fg
        dr = hm.mixture_draws()
        hm.close()
        assert dr["n_stored"] == S
        for K, T in shapes.items():
            g = got[K]
            assert g["n_unconverged"] == 0 and g["w"].shape == (T, n) and g["yhat"].shape == (T, n)
            assert g["info"]["n_solved"] == 2 * T * n and g["info"]["n_stored"] == K and g["info"]["keep"] == S
            assert g["info"]["n_passes"] <= 25 * g["info"]["n_solved"]      # Newton, a probe and a bisection over 256 widths: far below the cap
            assert g["info"]["store_bytes"] == S * (24 * n + 8 * q)
            print(f"{case} n={n} K={K} T={T}: {g['info']['n_passes'] / g['info']['n_solved']:.2f} passes per quantile")
            for tg in ("w", "yhat"):
                worst = check_quantiles(g[tg], PROBS[T], lambda i: target_comps(dr, mv, K, i, tg), n, f"{case} n={n} K={K} {tg}")
                note(f"quantile {tg}", worst)
                print(f"{case} n={n} K={K} T={T} {tg}: worst violation / eps_F {worst:.3f}")
            if K == 1:                                   # one component: the quantile is m + z_p sd itself, to the width
                for t, p in enumerate(PROBS[T]):
                    z = float(mr.norm_quantile(p))
                    want = dr["m"][0] + z * np.sqrt(dr["v"][0])
                    assert np.all(np.abs(g["w"][t] - want) <= 2.0 ** -49 * (np.abs(dr["m"][0]) + abs(z) * np.sqrt(dr["v"][0])))


def test_point_masses():
    """Points on rows of their own conditioning set: cond_var = max(rounding, 0), exactly 0 at some (section 30 used the same).  Their
    components are steps; with every component a step the quantile is the order statistic of the means itself."""
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
    n, S = pts.shape[0], 3
    hm = model(pb)
    hm.set_points(pts, mv, anchor)
    hm.reserve_mixture(S)
    rng = np.random.default_rng(12)
    for s in range(S):
        hm.set_w(rng.standard_normal(pb["n"]))
        hm.accumulate_points(seed=3, it=s)
    dr = hm.mixture_draws()
    probs = [0.2, 0.5, 0.9]
    got = hm.mixture_quantiles(probs)
    hm.close()
    zero = np.nonzero(np.all(dr["v"] == 0.0, axis=0))[0]
    some = np.nonzero(np.any(dr["v"] == 0.0, axis=0))[0]
    print(f"points on a conditioning row: {int(keep.sum())}; every cond_var exactly 0 at {zero.size}, some at {some.size}")
    assert zero.size >= 1 and got["n_unconverged"] == 0 and got["yhat"] is None
    worst = check_quantiles(got["w"], probs, lambda i: mr.components(dr["m"][:, i], dr["v"][:, i]), n, "point masses")
    note("quantile w", worst)
    for i in zero:                                       # inf{x : F(x) >= p} of three steps: the ceil(3 p)-th smallest mean, to the width
        srt = np.sort(dr["m"][:, i])
        for t, p in enumerate(probs):
            want = srt[math.ceil(S * p) - 1]
            assert want <= got["w"][t, i] <= want + 2.0 ** -50 * np.abs(dr["m"][:, i]).max(), (i, p)


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
    S, probs = 5, PROBS[3]
    hm = model(pb)
    hm.set_points(pts, mv, anchor, X, joint=labels)
    assert sorted({len(g) for g in hm.joint_groups}) == [1, 2, 3]
    hm.set_functionals(fun)
    hm.reserve_mixture(S)
    lasts = []
    outs, _, _ = accumulate(hm, pb, S, after=lambda s: lasts.append(hm.functionals_last()))
    dr = hm.mixture_draws()
    got = hm.mixture_quantiles(probs)
    hm.close()
    for s in range(S):                                   # on a joint set v is max(Sigma_aa, 0), as accumulate returns it
        assert np.array_equal(dr["m"][s], outs[s]["mean"]) and np.array_equal(dr["v"][s], outs[s]["var"]), s
    assert got["n_unconverged"] == 0 and got["functionals"]["n_unconverged"] == 0
    for tg in ("w", "yhat"):
        worst = check_quantiles(got[tg], probs, lambda i: target_comps(dr, mv, S, i, tg), n, f"joint {tg}")
        note(f"quantile {tg}", worst)
        print(f"joint set {tg}: worst violation / eps_F {worst:.3f}")
    fm = np.array([la["cond_mean"] for la in lasts])
    fv = np.array([la["cond_var"] for la in lasts])
    fw = got["functionals"]["w"]
    assert fw.shape == (3, len(fun))
    worst = check_quantiles(fw, probs, lambda f: mr.components(fm[:, f], fv[:, f]), len(fun), "functionals")
    note("quantile fun_w", worst)
    print(f"functionals: worst violation / eps_F {worst:.3f}")
    assert np.all(fm[:, 0] == 0.0) and np.all(fv[:, 0] == 0.0) and np.all(fw[:, 0] == 0.0)           # the empty one: a point mass at 0


# ---- 3. the CRPS -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ks", [(1, 2, 63), (64, 65), (257,)], ids=["K1-2-63", "K64-65", "K257"])
def test_crps(Ks):
    """NaNs interleaved in y_new; at the longest store one scored point, at the others also every point scored; y below, above and
    among the components.  K = 257 is one above the workgroup's 256 threads: the first thread owns two components."""
    pb = problem(1)
    S = max(Ks)
    n = 3 if S > 100 else 5
    pts, mv, anchor, X = plain_points(pb, n, 71)
    hm = model(pb)
    hm.set_points(pts, mv, anchor, X)
    hm.reserve_mixture(S)
    y1 = np.full(n, np.nan)
    y1[1::2] = [0.3, -25.0][:len(y1[1::2])]              # scored: points 1 (and 3)
    if S > 100:
        y1 = np.array([np.nan, 0.3, np.nan])             # one scored point
    y2 = np.array([40.0, -0.2, 0.0, 1.5, -3.0][:n])      # every point scored
    hm.set_scores(y1)
    got = {}

    def read(s):
        if s + 1 in Ks:
            a = hm.mixture_crps()
            hm.set_scores(y2 if S <= 100 else np.array([np.nan, -4.0, np.nan]))      # the store stays; only y changes
            b = hm.mixture_crps()
            hm.set_scores(y1)
            got[s + 1] = (a, b)
    accumulate(hm, pb, S, theta=S <= 65, after=read)
    dr = hm.mixture_draws()
    assert crps_refused_without_scores(hm)
    hm.close()
    for K in Ks:
        a, b = got[K]
        ya, yb = y1, (y2 if S <= 100 else np.array([np.nan, -4.0, np.nan]))
        assert a["n_scored"] == int(np.sum(~np.isnan(ya))) and b["n_scored"] == int(np.sum(~np.isnan(yb)))
        worst = [0.0, 0.0]
        for i in range(n):
            if np.isnan(ya[i]) and np.isnan(yb[i]):
                assert np.isnan(a["crps"][i]) and np.isnan(b["spread"][i])
                continue
            comps = target_comps(dr, mv, K, i, "yhat")
            spr = mr.spread(comps)
            for res, y in ((a, ya), (b, yb)):
                if np.isnan(y[i]):
                    assert np.isnan(res["crps"][i]) and np.isnan(res["spread"][i]), (K, i)
                    continue
                t1 = mr.t1_mean(y[i], comps)
                bc, bs = mr.crps_bounds(K, t1, spr)
                ec, es = mr.err(res["crps"][i], t1 - spr), mr.err(res["spread"][i], spr)
                worst = [max(worst[0], ec / bc), max(worst[1], es / bs)]
                assert ec <= bc and es <= bs, (K, i, ec, bc, es, bs)
                assert res["crps"][i] >= 0.0 and res["spread"][i] > 0.0
                if K == 1:                               # the closed form of one normal
                    want = mr.crps_normal(y[i], comps[0][0], mr.mp.sqrt(comps[0][1]))
                    assert mr.err(res["crps"][i], want) <= bc, (i, float(want))
            if not np.isnan(ya[i]) and not np.isnan(yb[i]):
                assert a["spread"][i] == b["spread"][i]  # spread does not depend on y_new: the same bits
        note("crps", worst[0]); note("spread", worst[1])
        print(f"crps K={K}: worst error / bound: crps {worst[0]:.3f} spread {worst[1]:.3f}")


def crps_refused_without_scores(hm):
    hm.set_scores(None)
    ok = hm.lib.st_points_mixture_crps(hm.h, None, None, None) == ST_ERR_USAGE
    return ok and b"before st_points_score_set" in hm.lib.st_last_error(hm.h)


# ---- 4. against the existing families ------------------------------------------------------------------------------------------
def test_cross_checks_through_predict_new():
    """One saved chain replayed twice.  The first replay gives the mixture quantiles; the second scores y_new = the yhat quantile of
    p = 0.9, so that (a) the PIT of section 19 at it is p within eps_F plus the PIT's own bound, (b) the number of stored yhat*
    draws at or below the quantile is a sum of Bernoullis with probabilities Phi_s: within Bernstein's width
    L / 3 + sqrt(L^2 / 9 + 2 V L) of K p, V = sum Phi_s (1 - Phi_s), L = ln(4 n T / 1e-6) (an independent check of sign and side), and
    (c), a sanity check only, the exact CRPS of the mixture does not exceed the CRPS of the stored draws (one noisy draw per
    component) by more than the Monte-Carlo allowance of that estimator, 10 spread / sqrt(K) with the reference's spread."""
    from spamtree_amd.predict import fit_predict, predict_new
    pb = problem(2)
    n, keep = 40, 120
    pts, mv, _, X = plain_points(pb, n, 81)
    mc = dict(MCMC, mcmc_keep=keep, mcmc_thin=1)
    out = fit_predict(pb, pts, mv, X, return_draws=False, **mc)
    probs = [0.1, 0.5, 0.9]
    one = predict_new(pb, out, pts, mv, X, seed=mc["seed"], device=0, mixture=dict(probs=probs), return_moments=True)
    mq = one["mixture"]
    assert mq["n_stored"] == keep and mq["n_unconverged"] == 0 and mq["w"].shape == (3, n)
    y = mq["yhat"][2].copy()
    two = predict_new(pb, out, pts, mv, X, seed=mc["seed"], device=0, y_new=y, mixture=dict(probs=probs, crps=True), return_moments=True)
    assert np.array_equal(two["mixture"]["yhat"], mq["yhat"]) and np.array_equal(two["mixture"]["w"], mq["w"])      # the replay repeats
    sc = two["scores"]
    betas = [np.asarray(out["beta_mcmc"])[:, s, :] for s in range(keep)]
    tis = [1.0 / np.asarray(out["tausq_mcmc"])[:, s] for s in range(keep)]
    L = math.log(4 * n * len(probs) / 1e-6)
    worst = dict(pit=0.0, bernstein=0.0, crps=-math.inf)
    for i in range(n):
        j = mv[i] - 1
        cm, cv = two["cond_mean"][i], two["cond_var"][i]
        comps = [(mr.mp.fsum(mr.mp.mpf(float(a)) * mr.mp.mpf(float(b)) for a, b in zip(X[i], betas[s][:, j])) + mr.mp.mpf(float(cm[s])),
                  mr.mp.mpf(float(cv[s])) + 1 / mr.mp.mpf(float(tis[s][j]))) for s in range(keep)]
        # (a) the PIT of the scores at the quantile of p
        _, _, pit, pit_bound = sr.point_scores(y[i], X[i], [b[:, j] for b in betas], list(cm), list(cv), [t[j] for t in tis])
        eps = mr.eps_F(y[i], comps)
        gap = abs(sc["pit"][i] - 0.9)
        worst["pit"] = max(worst["pit"], gap / (eps + pit_bound))
        assert gap <= eps + pit_bound, (i, gap, eps, pit_bound)
        # (the exact F at the device's quantile is within eps_F and the CDF's change over the width delta of p)
        assert abs(float(pit) - 0.9) <= eps + mr.delta(0.9, comps) / math.sqrt(2 * math.pi * float(min(v for _, v in comps)))
        # (b) Bernstein, for every probability
        for t, p in enumerate(probs):
            x = mr.mp.mpf(float(mq["yhat"][t, i]))
            ph = [mr.mp.erfc(-(x - m) / mr.mp.sqrt(v) * mr.RSQRT2) / 2 for m, v in comps]
            V = float(mr.mp.fsum(a * (1 - a) for a in ph))
            count = int(np.sum(two["yhat"][i] <= mq["yhat"][t, i]))
            width = L / 3 + math.sqrt(L * L / 9 + 2 * V * L)
            worst["bernstein"] = max(worst["bernstein"], abs(count - keep * p) / width)
            assert abs(count - keep * p) <= width, (i, p, count, V)
        # (c) the exact CRPS beside the CRPS of the stored draws
        if i % 8 == 0:
            spr = float(mr.spread(comps))
            allow = 10 * spr / math.sqrt(keep)
            worst["crps"] = max(worst["crps"], (sc["crps_mixture"][i] - sc["crps"][i]) / allow)
            assert sc["crps_mixture"][i] <= sc["crps"][i] + allow, (i, sc["crps_mixture"][i], sc["crps"][i], allow)
    assert sc["totals"]["crps_mixture"] == np.mean(sc["crps_mixture"]) and sc["totals"]["spread"] == np.mean(sc["spread"])
    for key, v in worst.items():
        note(f"cross {key}", v)
    print(f"|pit - p| / (eps_F + PIT bound): worst {worst['pit']:.3f}; |count - K p| / Bernstein width: worst {worst['bernstein']:.3f}; "
          f"(crps_mixture - crps) / allowance: largest {worst['crps']:.3f}")


# ---- 5. the whole fit ----------------------------------------------------------------------------------------------------------
def test_the_whole_fit():
    from spamtree_amd.predict import fit_predict, predict_new
    pb = problem(1)
    n = 60
    pts, mv, _, X = plain_points(pb, n, 91)
    rng = np.random.default_rng(22)
    y = 1.5 * rng.standard_normal(n)
    y[rng.uniform(size=n) < 0.3] = np.nan
    keep = MCMC["mcmc_keep"]
    fun = [(np.arange(5), np.ones(5) / 5), (np.array([0, n - 1]), np.array([1.0, -1.0]))]
    probs = [0.05, 0.5, 0.95]
    mc = dict(MCMC, sample_tausq=False)                  # 1 / 0.1 = 10 and back, exactly: the replay below gets the fit's tausq_inv
    base = fit_predict(pb, pts, mv, X, functionals=fun, y_new=y, **mc)
    out = fit_predict(pb, pts, mv, X, functionals=fun, y_new=y, mixture=dict(probs=probs, crps=True), **mc)
    new = out["new"]
    mq, fmq = new.pop("mixture"), new["functionals"].pop("mixture")
    sc = new["scores"]
    cm, spr = sc.pop("crps_mixture"), sc.pop("spread")
    for key in ("crps_mixture", "spread"):
        assert sc["totals"].pop(key) == np.mean((cm if key == "crps_mixture" else spr)[~np.isnan(y)])
        sc["totals"]["by_outcome"].pop(key)
    for key in ("beta_mcmc", "tausq_mcmc", "theta_mcmc", "paramsd", "w_mcmc", "yhat_mcmc"):
        same_tree(out[key], base[key], key)
    same_tree(new, base["new"])                          # every other output, bit for bit
    assert len({tuple(c) for c in np.asarray(out["theta_mcmc"]).T}) >= 2
    assert mq["n_stored"] == keep == fmq["n_stored"] and mq["n_unconverged"] == 0 and fmq["n_unconverged"] == 0
    assert mq["w"].shape == (3, n) and fmq["w"].shape == (3, 2) and np.array_equal(np.isnan(cm), np.isnan(y))
    # the handle-level calls on the same chain: the replay goes through st_points_accumulate and st_points_mixture_*
    rep = predict_new(pb, out, pts, mv, X, seed=mc["seed"], device=0, functionals=fun, y_new=y, mixture=dict(probs=probs, crps=True))
    assert np.array_equal(rep["yhat"], new["yhat"])
    for tg in ("w", "yhat"):
        assert np.array_equal(rep["mixture"][tg], mq[tg]), tg
    assert np.array_equal(rep["functionals"]["mixture"]["w"], fmq["w"])
    assert np.array_equal(rep["scores"]["crps_mixture"], cm, equal_nan=True) and np.array_equal(rep["scores"]["spread"], spr, equal_nan=True)
    # ... and against the reference on the fit's own per-draw outputs
    tau2 = np.asarray(out["tausq_mcmc"])
    worst = -math.inf
    for i in range(0, n, 7):
        comps = mr.components(new["cond_mean"][i], new["cond_var"][i])
        for t, p in enumerate(probs):
            worst = max(worst, mr.check_quantile(mq["w"][t, i], p, comps))
    assert worst <= 1.0
    note("quantile w", worst)
    # lean: nothing per draw on the host, the same mixture outputs
    lean = fit_predict(pb, pts, mv, X, functionals=fun, y_new=y, mixture=dict(probs=probs, crps=True), return_draws=False, save_w=False,
                       save_yhat=False, **mc)
    same_tree(lean["new"]["mixture"], mq, "lean mixture")
    assert np.array_equal(lean["new"]["scores"]["crps_mixture"], cm, equal_nan=True)
    # two chains: the store runs across them
    two = fit_predict(pb, pts, mv, X, mixture=dict(probs=probs), chains=2, chain_seeds=[11, 12], return_draws=False, **mc)
    assert two["new"]["mixture"]["n_stored"] == 2 * keep and two["new"]["mixture"]["n_unconverged"] == 0
    assert tau2.shape == (1, keep)
