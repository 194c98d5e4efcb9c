"""GPU: exceedance probabilities, excursion functions and simultaneous bands of the stored draws (st_summary_excursions,
st_points_summary_excursions, st_points_functionals_excursions, k_store_colstats, k_store_drawreduce, stm_mcmc_excursions,
fit.spamtree_mv_mcmc(excursions=)).

The stores are filled through the real calls, exactly as tests/test_gpu_diagnostics.py fills them -- rows: st_set_w with the
series' value then st_summary_accumulate, the yhat series read back per call through st_yhat; points and functionals:
st_points_accumulate and st_points_functionals_last -- and the reference (tests/excursion_reference.py) is always evaluated on the
very draws the device stored.

count, prob, excur, joint_all, n_flat and n_draws are compared bit for bit on every series.  mean, sd and maxdev are compared
within the bound excursion_reference.band_bounds derives from the kernel's own chain (K sequential fma steps, first order,
doubled; its docstring has the derivation, and asserts the neglected second-order terms small).

Shapes: n = 81 and 64 rows (one workgroup of pass 1, one tile of pass 2), 75 rows of three interleaved outcomes, point sets of 1,
9, 300 (past one workgroup of pass 1 and one stride of a pass-2 tile) and 1100 points (past one pass-2 tile of 512 or 1024 series:
the tiles of a draw meet in the atomic maximum); K = 1, 2, 63, 64, 65, 257 (below, at and above the batch of 16 draws and the
chunks pass 2 splits them into) and 16384 once (the K + 1 bin histogram at its largest, the whole count range)."""
import ctypes as C

import numpy as np
import pytest

from tests import excursion_reference as ref
from tests.test_gpu_diagnostics import feed_points, feed_rows, fit_args, hip_model, points_setup, series_rows
from tests.util import make_problem

pytestmark = pytest.mark.gpu

ST_ERR_USAGE, ST_ERR_UNSUPPORTED = -1, -4
EXACT = ("count", "prob", "excur", "joint_all")
_PB = {}
OBSERVED = dict(mean=0.0, sd=0.0, maxdev=0.0, mean_abs=0.0, sd_rel=0.0, maxdev_abs=0.0)


def problem(name):
    if name not in _PB:
        _PB[name] = dict(n64=lambda: make_problem(side=8, q=1, seed=71, p=2), n81=lambda: make_problem(side=9, q=1, seed=72, p=2),
                         q3=lambda: make_problem(side=5, q=3, seed=74, p=2),
                         lim=lambda: make_problem(side=8, q=1, seed=73, p=2, limited_tree=True))[name]()
    return _PB[name]


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_store(got, X, thr, side, dom, G, mask, band, tag):
    """One store's outputs against the reference on the draws X[K][n] the device stored.  thr: (T, G) per outcome (or (T, n) per
    series when ``dom`` is None: functionals), or None; dom: the n outcomes."""
    K, n = X.shape
    outcome = np.zeros(n, dtype=np.int64) if dom is None else np.asarray(dom, dtype=np.int64)
    g = outcome.copy()
    if mask is not None:
        g[np.asarray(mask) == 0] = -1
    assert got["n_draws"] == K, (tag, got["n_draws"])
    if thr is not None:
        thr = np.asarray(thr, dtype=np.float64)
        per_series = thr if dom is None else thr[:, outcome]
        want = ref.exceedance(X, per_series, np.asarray(side).reshape(-1), g, G)
        for key in EXACT:
            assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, (tag, key)
            assert np.array_equal(got[key], want[key], equal_nan=True), (tag, key, np.argwhere(~np.isclose(got[key], want[key], equal_nan=True))[:5])
        inn = g >= 0
        assert np.all(got["excur"][:, inn] <= got["prob"][:, inn]) and np.isnan(got["excur"][:, ~inn]).all()
    if band:
        r = ref.band(X, g, G)
        b = ref.band_bounds(X, g, G, r)
        ok = r["ok"]
        assert np.array_equal(got["n_flat"], r["n_flat"]), (tag, got["n_flat"], r["n_flat"])
        flat = ~ok & ~np.isnan(r["sd"].astype(np.float64))
        assert np.all(got["sd"][flat] == 0.0)
        e_mean = np.abs(got["mean"] - r["mean"].astype(np.float64))
        assert np.all(e_mean[ok] <= b["mean"][ok]), (tag, "mean", float((e_mean[ok] / b["mean"][ok]).max()))
        e_sd = np.abs(got["sd"][ok] / r["sd"][ok].astype(np.float64) - 1.0)
        assert np.all(e_sd <= b["sd"][ok]), (tag, "sd", float((e_sd / b["sd"][ok]).max()))
        e_dev = np.abs(got["maxdev"] - r["maxdev"].astype(np.float64))
        assert np.all(e_dev <= b["maxdev"]), (tag, "maxdev", float(e_dev.max()))
        assert np.all(got["maxdev"] >= 0.0)
        if ok.any():
            OBSERVED["mean"] = max(OBSERVED["mean"], float((e_mean[ok] / b["mean"][ok]).max()))
            OBSERVED["sd"] = max(OBSERVED["sd"], float((e_sd / b["sd"][ok]).max()))
            OBSERVED["mean_abs"] = max(OBSERVED["mean_abs"], float((e_mean[ok] / np.maximum(r["max_abs_x"][ok], 1e-300)).max()))
            OBSERVED["sd_rel"] = max(OBSERVED["sd_rel"], float(e_sd.max()))
            pos = b["maxdev"] > 0
            if pos.any():
                OBSERVED["maxdev"] = max(OBSERVED["maxdev"], float((e_dev[pos] / b["maxdev"][pos]).max()))
                OBSERVED["maxdev_abs"] = max(OBSERVED["maxdev_abs"], float(e_dev.max()))
    print(f"{tag}: K = {K}, n = {n}, T = {0 if thr is None else thr.shape[0]}, G = {G}, band = {band}: equal / within bounds")


def threshold_sets(ws, ys, m):
    """T = 8 with mixed sides -- below every draw, above every draw, equal to a stored value of w and of yhat from both sides, at
    the median -- per outcome the same value, and T = 1 at the median."""
    lo, hi = min(ws.min(), ys.min()) - 1.0, max(ws.max(), ys.max()) + 1.0
    K = ws.shape[0]
    eq_w, eq_y, med = float(ws[K // 2, 3 % ws.shape[1]]), float(ys[K // 2, 3 % ys.shape[1]]), float(np.median(ws))
    t8 = np.repeat(np.array([lo, hi, eq_w, med, eq_w, med, eq_y, eq_y])[:, None], m, axis=1)
    return (t8, np.array([1, 1, 1, 1, -1, -1, 1, -1])), (np.full((1, m), med), np.array([1]))


# ---- 1. values ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 63, 64, 65, 257])
def test_row_stores_against_the_reference(K):
    pb = problem("n81")
    hm = hip_model(pb)
    n = pb["n"]
    draws = series_rows(K, n, seed=K)
    assert hm.lib.st_summary_reserve(hm.h, K) == 0
    ys = feed_rows(hm, draws)
    dom = np.asarray(pb["mv_id"]).reshape(-1) - 1
    band = K >= 2
    mask = (np.arange(n) % 4 != 1).astype(np.uint8)
    for (thr, side), mk in zip(threshold_sets(draws, ys, 1), (None, mask)):
        got = hm.summary_excursions(K, list(thr), side, mask=mk, band=band)
        check_store(got["w"], draws, thr, side, dom, 1, mk, band, f"w T={len(side)}")
        check_store(got["yhat"], ys, thr, side, dom, 1, mk, band, f"yhat T={len(side)}")
    hm.close()


def test_row_store_with_16384_draws():
    K = 16384
    pb = problem("n64")
    hm = hip_model(pb)
    draws = series_rows(K, pb["n"], seed=7, once=(8, 9))
    assert hm.lib.st_summary_reserve(hm.h, K) == 0
    ys = feed_rows(hm, draws)
    thr = np.array([[float(np.median(draws))], [float(draws[K // 2, 3])]])
    side = np.array([1, -1])
    got = hm.summary_excursions(K, list(thr), side, band=True)
    dom = np.zeros(pb["n"], dtype=np.int64)
    check_store(got["w"], draws, thr, side, dom, 1, None, True, "w K=16384")
    check_store(got["yhat"], ys, thr, side, dom, 1, None, True, "yhat K=16384")
    assert got["w"]["count"].max() == K or got["w"]["count"].min() == 0   # the trend and constant rows reach an end of the count range
    hm.close()


def test_three_interleaved_domains_and_an_emptied_one():
    K = 65
    pb = problem("q3")
    hm = hip_model(pb)
    n = pb["n"]
    draws = series_rows(K, n, seed=5)
    assert hm.lib.st_summary_reserve(hm.h, K) == 0
    ys = feed_rows(hm, draws)
    dom = np.asarray(pb["mv_id"]).reshape(-1) - 1
    assert set(dom.tolist()) == {0, 1, 2}
    (t8, s8), (t1, s1) = threshold_sets(draws, ys, 3)
    t8 = t8 + np.array([0.0, 0.25, -0.25])[None, :] * (np.arange(8)[:, None] == 3)   # the median threshold differs by outcome
    mask = (dom != 1).astype(np.uint8)
    for thr, side, mk in ((t8, s8, None), (t8, s8, mask), (t1, s1, mask)):
        got = hm.summary_excursions(K, list(thr), side, mask=mk, band=True)
        check_store(got["w"], draws, thr, side, dom, 3, mk, True, "q3 w")
        check_store(got["yhat"], ys, thr, side, dom, 3, mk, True, "q3 yhat")
        if mk is not None:
            assert np.all(got["w"]["joint_all"][:, 1] == 1.0) and np.all(got["w"]["maxdev"][1] == 0.0) and got["w"]["n_flat"][1] == 0
    hm.close()


@pytest.mark.parametrize("n_new", [1, 9, 300, 1100])
def test_point_and_functional_stores_against_the_reference(n_new):
    K = 5
    pb = problem("n64")
    hm = hip_model(pb)
    assert hm.get_loglik_comps_w(0)
    points_setup(hm, pb, n_new, seed=5)
    if n_new >= 3:
        hm.set_functionals([([0, 1, 2], [1.0, 2.0, -3.0]), ([n_new - 1], [1.0]), (list(range(n_new)), [1.0 / n_new] * n_new)])
    else:
        hm.set_functionals([([0], [1.0]), ([0], [2.0]), ([0], [-1.0])])
    assert hm.lib.st_points_summary_reserve(hm.h, K) == 0
    ws, ys, fw, fy = feed_points(hm, pb, K, seed=n_new)
    dom = np.zeros(n_new, dtype=np.int64)
    mask = (np.arange(n_new) % 3 != 2).astype(np.uint8) if n_new > 1 else None
    for (thr, side), mk in zip(threshold_sets(ws, ys, 1), (mask, None)):
        got = hm.points_excursions(K, list(thr), side, mask=mk, band=True)
        check_store(got["w"], ws, thr, side, dom, 1, mk, True, "w*")
        check_store(got["yhat"], ys, thr, side, dom, 1, mk, True, "yhat*")
    (t8, s8), (t1, s1) = threshold_sets(fw, fy, 3)
    t8[3] = np.median(fw, axis=0)   # a threshold value per functional
    fmask = np.array([1, 0, 1], dtype=np.uint8)
    for thr, side, mk in ((t8, s8, None), (t1, s1, fmask)):
        gf = hm.functionals_excursions(K, list(thr), side, mask=mk, band=True)
        check_store(gf["w"], fw, thr, side, None, 1, mk, True, "F_w")
        check_store(gf["yhat"], fy, thr, side, None, 1, mk, True, "F_y")
    hm.close()


# ---- 2. the outputs one at a time, and twice ---------------------------------------------------------------------------------------
def test_outputs_one_at_a_time_and_twice_give_the_same_bits():
    from spamtree_amd import _lib
    from spamtree_amd.model import excursion_buffers, excursion_spec
    K = 65
    pb = problem("q3")
    hm = hip_model(pb)
    n = pb["n"]
    draws = series_rows(K, n, seed=9)
    assert hm.lib.st_summary_reserve(hm.h, K) == 0
    ys = feed_rows(hm, draws)
    (t8, s8), _ = threshold_sets(draws, ys, 3)
    mask = (np.arange(n) % 5 != 0).astype(np.uint8)
    kw = dict(thresholds=list(t8), side=s8, mask=mask, band=True)
    a, b = hm.summary_excursions(K, **kw), hm.summary_excursions(K, **kw)
    names = ("count", "prob", "excur", "joint_all", "mean", "sd", "maxdev", "n_flat")
    for part in ("w", "yhat"):
        for key in names:
            assert same_bits(a[part][key], b[part][key]), (part, key)
    spec, keep = excursion_spec(np.ascontiguousarray(t8), s8.astype(np.int32), mask, False)   # want_band 0: a band pointer alone asks for it
    for key in names:
        d, full = excursion_buffers(n, 8, 3, K, True)
        one = _lib.StExcursionOut()
        setattr(one, key, getattr(full, key))
        assert hm.lib.st_summary_excursions(hm.h, C.byref(spec), C.byref(one), None) == 0, hm.lib.st_last_error(hm.h)
        assert same_bits(d[key], a["w"][key]), key
        for other in names:
            assert other == key or not d[other].any(), (key, other)   # nothing else was written
        assert hm.lib.st_summary_excursions(hm.h, C.byref(spec), None, C.byref(one)) == 0
        assert same_bits(d[key], a["yhat"][key]), key
    del keep
    hm.close()


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    from spamtree_amd import _lib
    from spamtree_amd.model import SpamTreeError, excursion_buffers, excursion_spec
    pb = problem("n64")
    hm = hip_model(pb)
    lib, h, n = hm.lib, hm.h, pb["n"]
    thr1, side1 = np.zeros((1, 1)), np.array([1], dtype=np.int32)

    def call(f, thr=thr1, side=side1, n_thr=None, band=False, band_out=False, thr_out=True, y=False, size=n, G=1):
        spec, keep = excursion_spec(thr, side, None, band)
        if n_thr is not None:
            spec.n_thr = n_thr
        T = 0 if (thr is None or not thr_out) else thr.shape[0]
        d, o = excursion_buffers(size, T, G, 16, band or band_out)
        rc = f(h, C.byref(spec), C.byref(o), C.byref(o) if y else None)
        return rc, lib.st_last_error(h)

    rc, msg = call(lib.st_summary_excursions)
    assert rc == ST_ERR_USAGE and b"no draw stored" in msg                                     # no reservation, no draw
    assert lib.st_summary_reserve(h, 8) == 0
    draws = series_rows(8, n, seed=1)
    feed_rows(hm, draws[:1])
    rc, msg = call(lib.st_summary_excursions, band=True)
    assert rc == ST_ERR_USAGE and b"at least 2" in msg                                          # want_band with K = 1
    rc, msg = call(lib.st_summary_excursions, band_out=True)
    assert rc == ST_ERR_USAGE and b"at least 2" in msg                                          # a band output with K = 1
    assert call(lib.st_summary_excursions)[0] == 0                                              # K = 1 without the band answers
    feed_rows(hm, draws[1:3])
    for n_thr in (0, 9, -1):
        rc, msg = call(lib.st_summary_excursions, thr=np.zeros((9, 1)), side=np.ones(9, dtype=np.int32), n_thr=n_thr)
        assert rc == ST_ERR_USAGE and b"1 .. 8" in msg
    for bad in (np.nan, np.inf, -np.inf):
        rc, msg = call(lib.st_summary_excursions, thr=np.array([[0.0], [bad]]), side=np.array([1, 1], dtype=np.int32))
        assert rc == ST_ERR_USAGE and b"not finite" in msg
    for bad in (0, 2, -2):
        rc, msg = call(lib.st_summary_excursions, side=np.array([bad], dtype=np.int32))
        assert rc == ST_ERR_USAGE and b"+1 or -1" in msg
    rc, msg = call(lib.st_summary_excursions, thr=None, side=None)
    assert rc == ST_ERR_USAGE and b"neither thresholds nor a band" in msg
    spec, keep = excursion_spec(None, None, None, True)
    d, o = excursion_buffers(n, 1, 1, 16, True)   # threshold outputs without thresholds
    assert lib.st_summary_excursions(h, C.byref(spec), C.byref(o), None) == ST_ERR_USAGE and b"need thresholds" in lib.st_last_error(h)
    assert lib.st_summary_excursions(h, None, C.byref(o), None) == ST_ERR_USAGE
    got = hm.summary_excursions(3, 0.0, band=True)                                              # still answers
    check_store(got["w"], draws[:3], np.zeros((1, 1)), [1], np.zeros(n, dtype=np.int64), 1, None, True, "after the refusals")
    # points and functionals: before their sets, without a stored draw, yhat without X
    assert call(lib.st_points_summary_excursions)[0] == ST_ERR_USAGE and b"before st_points_set" in lib.st_last_error(h)
    assert call(lib.st_points_functionals_excursions)[0] == ST_ERR_USAGE
    assert hm.get_loglik_comps_w(0)
    points_setup(hm, pb, 9, seed=2, X=False)
    rc, msg = call(lib.st_points_functionals_excursions, size=9)
    assert rc == ST_ERR_USAGE and b"before st_points_functionals_set" in msg
    hm.set_functionals([([0, 1], [1.0, 1.0])])
    rc, msg = call(lib.st_points_summary_excursions, size=9)
    assert rc == ST_ERR_USAGE and b"no draw stored" in msg
    rc, msg = call(lib.st_points_functionals_excursions, size=1)
    assert rc == ST_ERR_USAGE and b"no draw stored" in msg
    assert lib.st_points_summary_reserve(h, 6) == 0
    hm.accumulate_points(seed=1, it=0)
    rc, msg = call(lib.st_points_summary_excursions, size=9, band=True)
    assert rc == ST_ERR_USAGE and b"at least 2" in msg
    hm.accumulate_points(seed=1, it=1)
    rc, msg = call(lib.st_points_summary_excursions, size=9, y=True)
    assert rc == ST_ERR_USAGE and b"needs the regressors X" in msg
    rc, msg = call(lib.st_points_functionals_excursions, size=1, y=True)
    assert rc == ST_ERR_USAGE and b"needs the regressors X" in msg
    got = hm.points_excursions(2, 0.0, band=True)
    assert got["yhat"] is None and got["w"]["n_draws"] == 2 and np.all(got["w"]["sd"] > 0)
    gf = hm.functionals_excursions(2, 0.0, band=True)
    assert gf["yhat"] is None and gf["w"]["count"].shape == (1, 1)
    # a point set of size 0: ST_OK, nothing written
    hm.set_points(np.zeros((0, 2)), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))
    spec, keep = excursion_spec(thr1, side1, None, False)
    d, o = excursion_buffers(4, 1, 1, 16, False)
    d["prob"][:] = -7.0
    assert lib.st_points_summary_excursions(h, C.byref(spec), C.byref(o), None) == 0 and np.all(d["prob"] == -7.0)
    hm.close()
    # a limited_tree handle: the rows are supported, the point calls refused as their quantile siblings are
    pl = problem("lim")
    hl = hip_model(pl)
    assert hl.lib.st_summary_reserve(hl.h, 5) == 0
    dl = series_rows(5, pl["n"], seed=4)
    yl = feed_rows(hl, dl)
    (t8, s8), _ = threshold_sets(dl, yl, 1)
    got = hl.summary_excursions(5, list(t8), s8, band=True)
    check_store(got["w"], dl, t8, s8, np.zeros(pl["n"], dtype=np.int64), 1, None, True, "limited_tree w")
    check_store(got["yhat"], yl, t8, s8, np.zeros(pl["n"], dtype=np.int64), 1, None, True, "limited_tree yhat")
    d, o = excursion_buffers(1, 1, 1, 5, False)
    assert hl.lib.st_points_summary_excursions(hl.h, C.byref(spec), C.byref(o), None) == ST_ERR_UNSUPPORTED
    hl.n_points, hl.points_have_X = 1, False
    with pytest.raises(SpamTreeError):
        hl.points_excursions(5, 0.0)
    hl.close()
    del keep


# ---- 4. the driver ----------------------------------------------------------------------------------------------------------------
KW = dict(mcmc_keep=40, mcmc_burn=5, mcmc_thin=1, seed=23, adapting=True, main_verbose=False)
stack = lambda lst: np.stack([np.asarray(a).reshape(-1) for a in lst])   # noqa: E731
NAMES = ("count", "prob", "excur", "joint_all", "mean", "sd", "maxdev", "n_flat", "n_draws")


def same_parts(a, b):
    for part in ("w", "yhat"):
        for key in NAMES:
            assert same_bits(a[part][key], b[part][key]), (part, key)


def test_driver_plain_chain_the_lean_call_and_diagnostics_together():
    from spamtree_amd import fit
    pb = problem("n64")
    n = pb["n"]
    mask = (np.arange(n) % 7 != 3).astype(np.uint8)
    x = dict(thresholds=[0.0, 0.5, -0.5], side=[1, 1, -1], mask=mask, band=True)
    thr, side = np.array([[0.0], [0.5], [-0.5]]), [1, 1, -1]
    res = fit.spamtree_mv_mcmc(*fit_args(pb), excursions=x, **KW)
    base = fit.spamtree_mv_mcmc(*fit_args(pb), **KW)
    for key in ("beta_mcmc", "tausq_mcmc", "theta_mcmc", "paramsd"):
        assert np.array_equal(res[key], base[key]), key
    for key in ("w_mcmc", "yhat_mcmc"):
        assert all(np.array_equal(a, b) for a, b in zip(res[key], base[key])), key
    assert "excursions" not in base
    dom = np.zeros(n, dtype=np.int64)
    check_store(res["excursions"]["w"], stack(res["w_mcmc"]), thr, side, dom, 1, mask, True, "driver w")
    check_store(res["excursions"]["yhat"], stack(res["yhat_mcmc"]), thr, side, dom, 1, mask, True, "driver yhat")
    lean = fit.spamtree_mv_mcmc(*fit_args(pb), excursions=x, save_w=False, save_yhat=False, **KW)
    assert "w_mcmc" not in lean and "yhat_mcmc" not in lean
    same_parts(lean["excursions"], res["excursions"])
    both = fit.spamtree_mv_mcmc(*fit_args(pb), excursions=x, diagnostics=True, **KW)
    diag = fit.spamtree_mv_mcmc(*fit_args(pb), diagnostics=True, **KW)
    same_parts(both["excursions"], res["excursions"])
    for part in ("w", "yhat"):
        for key in ("ess", "mcse", "sd", "rhat", "lags"):
            assert np.array_equal(both["diagnostics"][part][key], diag["diagnostics"][part][key], equal_nan=True), (part, key)
    assert np.array_equal(both["theta_mcmc"], base["theta_mcmc"])
    band_only = fit.spamtree_mv_mcmc(*fit_args(pb), excursions=dict(band=True), save_w=False, save_yhat=False, **KW)
    assert "count" not in band_only["excursions"]["w"]
    assert same_bits(band_only["excursions"]["w"]["mean"], fit.spamtree_mv_mcmc(*fit_args(pb), excursions=dict(band=True, thresholds=1.0),
                                                                                  save_w=False, save_yhat=False, **KW)["excursions"]["w"]["mean"])


def test_driver_with_new_points_and_functionals():
    from spamtree_amd import fit
    from spamtree_amd.predict import locate
    pb = problem("n64")
    rng = np.random.default_rng(8)
    n_new = 9
    lo, hi = pb["coords"].min(axis=0), pb["coords"].max(axis=0)
    pts = lo + (hi - lo) * rng.uniform(size=(n_new, 2))
    mv = np.ones(n_new, dtype=np.int64)
    new_points = dict(coords=pts, mv=mv, anchor=locate(pb["topo"], pts, mv, device=0), X=rng.standard_normal((n_new, pb["p"])),
                      functionals=[([0, 1, 2], [1.0, 2.0, -3.0]), (list(range(n_new)), [1.0 / n_new] * n_new)])
    mnew = np.array([1, 1, 0, 1, 1, 1, 0, 1, 1], dtype=np.uint8)
    x = dict(thresholds=[0.0, 0.3], side=[1, -1], band=True, mask_new=mnew, thresholds_fun=[[0.0, 0.1], [0.3, 0.2]])
    thr, side = np.array([[0.0], [0.3]]), [1, -1]
    res = fit.spamtree_mv_mcmc(*fit_args(pb), excursions=x, diagnostics=True, new_points=new_points, **KW)
    base = fit.spamtree_mv_mcmc(*fit_args(pb), new_points=new_points, **KW)
    for key in ("beta_mcmc", "tausq_mcmc", "theta_mcmc", "paramsd"):
        assert np.array_equal(res[key], base[key]), key
    assert all(np.array_equal(a, b) for a, b in zip(res["w_mcmc"], base["w_mcmc"]))
    for key in ("w", "yhat", "cond_mean", "cond_var", "mean", "var", "w_mean", "yhat_mean"):
        assert np.array_equal(res["new"][key], base["new"][key]), key
        assert np.array_equal(res["new"]["functionals"][key], base["new"]["functionals"][key]), key
    assert "excursions" not in base["new"] and "diagnostics" in res and "diagnostics" in res["new"]
    n = pb["n"]
    check_store(res["excursions"]["w"], stack(res["w_mcmc"]), thr, side, np.zeros(n, dtype=np.int64), 1, None, True, "rows w")
    check_store(res["excursions"]["yhat"], stack(res["yhat_mcmc"]), thr, side, np.zeros(n, dtype=np.int64), 1, None, True, "rows yhat")
    dn = np.zeros(n_new, dtype=np.int64)
    check_store(res["new"]["excursions"]["w"], res["new"]["w"].T, thr, side, dn, 1, mnew, True, "points w")
    check_store(res["new"]["excursions"]["yhat"], res["new"]["yhat"].T, thr, side, dn, 1, mnew, True, "points yhat")
    tf = np.array([[0.0, 0.1], [0.3, 0.2]])
    check_store(res["new"]["functionals"]["excursions"]["w"], res["new"]["functionals"]["w"].T, tf, side, None, 1, None, True, "functionals w")
    check_store(res["new"]["functionals"]["excursions"]["yhat"], res["new"]["functionals"]["yhat"].T, tf, side, None, 1, None, True, "functionals yhat")
    lean = fit.spamtree_mv_mcmc(*fit_args(pb), excursions=x, new_points=new_points, new_draws=False, save_w=False, save_yhat=False, **KW)
    assert "w" not in lean["new"]
    same_parts(lean["excursions"], res["excursions"])
    same_parts(lean["new"]["excursions"], res["new"]["excursions"])
    same_parts(lean["new"]["functionals"]["excursions"], res["new"]["functionals"]["excursions"])


def test_driver_on_a_limited_tree():
    from spamtree_amd import _lib, fit
    pl = problem("lim")
    x = dict(thresholds=0.0, band=True)
    res = fit.spamtree_mv_mcmc(*fit_args(pl), excursions=x, **KW)
    base = fit.spamtree_mv_mcmc(*fit_args(pl), **KW)
    assert np.array_equal(res["theta_mcmc"], base["theta_mcmc"]) and all(np.array_equal(a, b) for a, b in zip(res["w_mcmc"], base["w_mcmc"]))
    dom = np.zeros(pl["n"], dtype=np.int64)
    check_store(res["excursions"]["w"], stack(res["w_mcmc"]), np.zeros((1, 1)), [1], dom, 1, None, True, "limited_tree driver w")
    check_store(res["excursions"]["yhat"], stack(res["yhat_mcmc"]), np.zeros((1, 1)), [1], dom, 1, None, True, "limited_tree driver yhat")
    assert _lib.SIGNATURES["stm_mcmc_excursions"][1][-1]._type_ is _lib.StmExcursions


def test_fit_predict_and_the_replay_pass_excursions_on():
    """predict.fit_predict(excursions=) and predict.predict_new(excursions=) on a q = 2 problem with points of both outcomes and two
    functionals: each against the reference on the draws it returned; the w* draws of the fit and of the replay are the same
    bits, so are their excursion outputs."""
    from spamtree_amd.predict import fit_predict, predict_new
    pb = make_problem(side=12, q=2, seed=2, p=2)
    rng = np.random.default_rng(31)
    n_new = 40
    lo, hi = pb["coords"].min(axis=0), pb["coords"].max(axis=0)
    pts = lo + (hi - lo) * rng.uniform(size=(n_new, 2))
    mv = rng.integers(1, 3, size=n_new)
    Xn = rng.standard_normal((n_new, pb["p"]))
    A = [([0, 1, 2], [1.0, 2.0, -3.0]), (list(range(n_new)), [1.0 / n_new] * n_new)]
    mask = (np.arange(n_new) % 5 != 0).astype(np.uint8)
    thr = np.array([[0.0, 0.2], [0.5, 0.5]])
    side = [1, -1]
    tf = np.array([[0.0, 0.1], [0.3, 0.3]])
    kw = dict(mcmc_keep=12, mcmc_burn=4, mcmc_thin=1, adapting=True, seed=77, device=0)
    out = fit_predict(pb, pts, mv, Xn, functionals=A, excursions=dict(thresholds=[[0.0, 0.2], 0.5], side=side, band=True, mask_new=mask,
                                                                       thresholds_fun=[[0.0, 0.1], 0.3]), **kw)
    rep = predict_new(pb, out, pts, mv, Xn, seed=77, device=0, functionals=A,
                      excursions=dict(thresholds=[[0.0, 0.2], 0.5], side=side, band=True, mask=mask, thresholds_fun=[[0.0, 0.1], 0.3]))
    dom = mv - 1
    for res, fun, tag in ((out["new"]["excursions"], out["new"]["functionals"], "fit_predict"), (rep["excursions"], rep["functionals"], "replay")):
        src = out["new"] if tag == "fit_predict" else rep
        check_store(res["w"], src["w"].T, thr, side, dom, 2, mask, True, f"{tag} w*")
        check_store(res["yhat"], src["yhat"].T, thr, side, dom, 2, mask, True, f"{tag} yhat*")
        check_store(fun["excursions"]["w"], fun["w"].T, tf, side, None, 1, None, True, f"{tag} F_w")
        check_store(fun["excursions"]["yhat"], fun["yhat"].T, tf, side, None, 1, None, True, f"{tag} F_y")
    assert np.array_equal(out["new"]["w"], rep["w"])
    for key in NAMES:
        assert same_bits(out["new"]["excursions"]["w"][key], rep["excursions"]["w"][key]), key
    rows_dom = np.asarray(pb["mv_id"]).reshape(-1) - 1
    check_store(out["excursions"]["w"], stack(out["w_mcmc"]), thr, side, rows_dom, 2, None, True, "fit_predict rows w")


def test_zz_report_the_largest_observed_error():
    """Prints the largest errors of mean, sd and maxdev the cases above met, as fractions of their bounds and as such (DESIGN.md
    section 22 records them)."""
    print("largest observed error / bound: mean {mean:.3g}, sd {sd:.3g}, maxdev {maxdev:.3g}; largest |mean error| / max|x| {mean_abs:.3g}, "
          "relative sd error {sd_rel:.3g}, absolute maxdev error {maxdev_abs:.3g}".format(**OBSERVED))
    assert max(OBSERVED["mean"], OBSERVED["sd"], OBSERVED["maxdev"]) <= 1.0
