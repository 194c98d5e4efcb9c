"""GPU: rank-normalised R-hat, bulk, tail, quantile and exceedance ESS of the stored draws (st_summary_rank_diagnostics,
st_points_summary_rank_diagnostics, st_points_functionals_rank_diagnostics, k_series_rank).

The stores are filled through the real calls as tests/test_gpu_diagnostics.py fills them, and the reference
(tests/rank_reference.py: integer ranks and A_t, rational rho and tau, 50-digit Phi^-1, long-double moments) is always evaluated on
the very draws the device stored.

Integer-defined outputs.  prob is compared bitwise with the reference's c / K and with st_*_excursions on the same store; ess_q,
ess_tail, ess_exc and mcse_prob within 1e-14 relative: the A_t are exact integers and the pairs are walked on their integer
numerators, so the device walks exactly the reference's pairs, and only 1 / log10 K, tau's one quotient, the final division and
the square root can differ.  (A first version rounded every rho_t to double and summed the pairs in double, as the plain
diagnostics do: the Cauchy column at K = 8192 then came out 1.25e-14 from the rational reference.)  The C-ABI returns no lag
count of an indicator series; the host function's are compared exactly on the CPU.  The driver cases compare the device outputs
with the reference on the returned w_mcmc, yhat_mcmc and per-draw point arrays, and every chain output with the run without
rank_diagnostics bit for bit, also combined with diagnostics=True and excursions=, and in the lean call.

Score-defined outputs (rhat_bulk, rhat_fold, rhat_rank, ess_bulk): within rank_reference.score_bounds -- the sibling's bound with
D = ceil(K / 64) + 6 additions behind any one sum, and every z_s off by at most 2 PHI_ERR_MEASURED |z_s| (the error of Phi^-1
measured on the CPU, doubled because the device compiler may contract multiply-adds the host's does not).  lags_bulk and the
truncated state are compared wherever the reference's smallest |Gamma_k| exceeds 1e-8; at most 2 % of the series may be left out
(the seeds below leave none out: checked on the CPU with the reference alone).
"""
import ctypes as C
import math

import numpy as np
import pytest

from tests import rank_reference as rr
from tests.test_gpu_diagnostics import feed_points, feed_rows, hip_model, points_setup, problem, series_rows

pytestmark = pytest.mark.gpu

ST_ERR_USAGE, ST_ERR_UNSUPPORTED = -1, -4
INT_RTOL = 1e-14
EPS_PHI = 2 * rr.PHI_ERR_MEASURED
PROBS = (0.025, 0.5, 0.9)
OBSERVED = dict(max_err_over_bound=0.0, max_rel_err=0.0, max_int_rel_err=0.0, stores=0, series=0)


def rank_rows(K, n, seed, once=()):
    """series_rows (AR(1) with six phis, white noise, a constant, the alternating series, a trend, noise on an offset of 1e3) with
    columns 11, 12, 13 replaced by the tie blocks (shuffled), a two-valued series and the split-scale Cauchy."""
    out = series_rows(K, n, seed, once)
    rng = np.random.default_rng(seed + 77)
    out[:, 11] = rr.tie_blocks(K)[rng.permutation(K)]
    out[:, 12] = np.where(rng.uniform(size=K) < 0.3, 1.5, -1.0)
    out[:, 13] = rr.split_scale_cauchy(K, seed + 5)
    return out


def close(a, b, rtol):
    return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= rtol * abs(b)


def check_store(got, draws, thr, sides, max_lag, tag, probs=PROBS, cols=None):
    """Every series (or those of ``cols``) of draws[K][n] against the reference.  ``thr``: (T, n) values per series."""
    K, n = draws.shape
    depth = -(-K // 64) + 6
    left_out, worst, worst_rel, worst_int, seen = 0, 0.0, 0.0, 0.0, 0
    for i in (range(n) if cols is None else cols):
        r = rr.reference(draws[:, i], probs, [t[i] for t in thr], sides, max_lag)
        seen += 1
        for key, want in (("ess_q", r["ess_q"]), ("ess_exc", r["ess_exc"]), ("mcse_prob", r["mcse_prob"])):
            for k, w in enumerate(want):
                g = float(got[key][k][i])
                assert close(g, w, INT_RTOL), (tag, i, key, k, g, w)
                if not math.isnan(w) and w != 0.0:
                    worst_int = max(worst_int, abs(g - w) / abs(w))
        assert close(float(got["ess_tail"][i]), r["ess_tail"], INT_RTOL), (tag, i, got["ess_tail"][i], r["ess_tail"])
        for t, w in enumerate(r["prob"]):
            assert np.array([got["prob"][t][i]]).tobytes() == np.array([w], dtype=np.float64).tobytes(), (tag, i, t, got["prob"][t][i], w)
        g = {k: float(got[k][i]) for k in ("rhat_rank", "rhat_bulk", "rhat_fold", "ess_bulk")}
        lags = int(got["lags_bulk"][i])
        for part, keys in (("bulk", (("rhat_bulk", "rhat"), ("ess_bulk", "ess"))), ("fold", (("rhat_fold", "rhat"),))):
            rec = r[part]
            if rec["gamma0"] == 0.0:
                assert all(math.isnan(g[a]) for a, _ in keys) and (part != "bulk" or lags == 0), (tag, i, part, g, lags)
                continue
            b = rr.score_bounds(rec, K, lags // 2, depth, EPS_PHI)
            for a, key in keys:
                if math.isnan(rec[key]):
                    assert math.isnan(g[a]), (tag, i, a, g[a])
                    continue
                err = abs(g[a] - rec[key]) / abs(rec[key])
                worst, worst_rel = max(worst, err / b[key]), max(worst_rel, err)
                assert err <= b[key], (tag, i, a, g[a], rec[key], err, b[key])
        assert np.array([g["rhat_rank"]]).tobytes() == np.array([rr.fmax(g["rhat_bulk"], g["rhat_fold"])]).tobytes(), (tag, i, g)
        if r["bulk"]["gamma0"] != 0.0:
            _, k_max = rr.lag_cap(K, max_lag)
            if r["bulk"]["min_abs_gamma"] > 1e-8:
                assert lags == r["lags_bulk"] and (lags == 2 * (k_max + 1)) == r["truncated"], (tag, i, lags, r["lags_bulk"])
            else:
                left_out += 1
            assert lags % 2 == 0 and 0 <= lags <= 2 * (k_max + 1)
    assert left_out <= 0.02 * seen, (tag, left_out)
    for k, v in (("max_err_over_bound", worst), ("max_rel_err", worst_rel), ("max_int_rel_err", worst_int)):
        OBSERVED[k] = max(OBSERVED[k], v)
    assert seen > 0, tag
    OBSERVED["stores"] += 1
    OBSERVED["series"] += seen
    print(f"{tag}: K = {K}, n = {seen}, max_lag = {max_lag}: score outputs max err / bound {worst:.3g}, max relative err {worst_rel:.3g}; "
          f"integer-defined outputs max relative err {worst_int:.3g}; left out of the lags comparison {left_out}")


def thresholds_for(draws):
    """Two thresholds for a q = 1 store: the median of all its values (side +1) and their lower quartile (side -1); as (T, n)."""
    t = [float(np.median(draws)), float(np.quantile(draws, 0.25))]
    return t, [np.full(draws.shape[1], v) for v in t], (1, -1)


def rows_case(K, pb_name, max_lags, once=(), cols=None, seed=None):
    """``cols``: {(name, max_lag): columns to compare}; None: all of them."""
    pb = problem(pb_name)
    hm = hip_model(pb)
    draws = rank_rows(K, pb["n"], seed=K if seed is None else seed, once=once)
    assert hm.lib.st_summary_reserve(hm.h, K) == 0
    ys = feed_rows(hm, draws)
    for max_lag in max_lags:
        for name, d in (("w", draws), ("yhat", ys)):
            t, per, sides = thresholds_for(d)
            got = hm.summary_rank_diagnostics(PROBS, t, sides, max_lag, n_kept=K)[name]
            check_store(got, d, per, sides, max_lag, name, cols=None if cols is None else cols[name, max_lag])
            exc = hm.summary_excursions(K, thresholds=t, side=list(sides))[name]
            assert got["prob"].tobytes() == exc["prob"].tobytes()     # bit for bit st_summary_excursions' prob on the same store
    hm.close()


# ---- 1. values ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [4, 5, 63, 64, 65, 129, 257])
def test_row_stores_against_the_reference(K):
    """n = 81 rows in tiles of 8 (the last tile holds one), every kind of series, K below, at and above one, two and four words
    of the bit masks, max_lag 0, 1, 7 and K; w and yhat."""
    rows_case(K, "n81", (0, 1, 7, K))


@pytest.mark.parametrize("K", [2500, 8192, 8193, 16384])
def test_row_stores_with_long_series(K):
    """One series per tile.  K = 8192 is the last length whose scores live in LDS beside the sorted copy (64 KB + 64 KB); from
    8193 on the padded sorted copy alone takes 128 KB and the scores go to the workgroup's global slice.  n = 64 rows.  The
    reference costs up to seconds per series at these lengths, so it is evaluated on a choice of columns.  K = 2500: for w with
    the default cap the first fourteen (every kind of series once) and two AR(1) columns from later tiles, the last row among
    them; with max_lag = K an AR(1), the alternating series (its scores alternate too: every pair is walked) and the two-valued
    one; for yhat five and one of them.  From K = 8192 on: one column of each kind that behaves differently (AR(1) with phi -0.9
    and 0.99, the constant, the alternating series, the trend, the tie blocks, the two-valued series, the Cauchy, the last row);
    with max_lag = K the alternating series (an AR(1) at 16384, where walking 8191 pairs takes the reference 10 s); two yhat
    columns with the default cap and one (white noise) with max_lag = K.  Only max_lag 0 and K are run at these lengths.  prob
    is compared with st_summary_excursions on every column."""
    if K < 8192:
        every = list(range(14)) + [40, 63]
        cols = {("w", 0): every, ("w", K): [3, 8, 12], ("yhat", 0): [0, 6, 10, 13, 63], ("yhat", K): [3]}
    else:
        cols = {("w", 0): [0, 5, 7, 8, 9, 11, 12, 13, 63], ("w", K): [8 if K < 16384 else 3], ("yhat", 0): [6, 63], ("yhat", K): [6]}
    rows_case(K, "n64", (0, K), once=(8, 9), seed=7, cols=cols)


@pytest.mark.parametrize("K", [5, 65])
def test_point_and_functional_stores_against_the_reference(K):
    pb = problem("n64")
    hm = hip_model(pb)
    assert hm.get_loglik_comps_w(0)
    n_new = 9
    points_setup(hm, pb, n_new, seed=5)
    hm.set_functionals([([0, 1, 2], [1.0, 2.0, -3.0]), ([4], [1.0]), (list(range(n_new)), [1.0 / n_new] * n_new)])
    assert hm.lib.st_points_summary_reserve(hm.h, K) == 0
    ws, ys, fw, fy = feed_points(hm, pb, K, seed=K)
    for max_lag in (0, 2):
        for name, d in (("w", ws), ("yhat", ys)):
            t, per, sides = thresholds_for(d)
            got = hm.points_rank_diagnostics(PROBS, t, sides, max_lag, n_kept=K)[name]
            check_store(got, d, per, sides, max_lag, name + "*")
            assert got["prob"].tobytes() == hm.points_excursions(K, thresholds=t, side=list(sides))[name]["prob"].tobytes()
        for name, d in (("w", fw), ("yhat", fy)):   # a threshold value per functional
            per = [np.median(d, axis=0), np.quantile(d, 0.25, axis=0)]
            got = hm.functionals_rank_diagnostics(PROBS, per, (1, -1), max_lag, n_kept=K)[name]
            check_store(got, d, per, (1, -1), max_lag, "F_" + name)
            assert got["prob"].tobytes() == hm.functionals_excursions(K, thresholds=per, side=[1, -1])[name]["prob"].tobytes()
            assert got["truncated"].dtype == bool and got["ess_q"].shape == (3, 3)
    hm.close()


def test_only_what_is_asked_for_is_computed():
    """Each output asked for alone gives the bits of the full call; a spec without probs or thresholds gives the five series outputs."""
    from spamtree_amd import _lib
    K = 65
    pb = problem("n64")
    hm = hip_model(pb)
    draws = rank_rows(K, pb["n"], seed=3)
    assert hm.lib.st_summary_reserve(hm.h, K) == 0
    feed_rows(hm, draws)
    t, _, sides = thresholds_for(draws)
    full = hm.summary_rank_diagnostics(PROBS, t, sides)["w"]
    bare = hm.summary_rank_diagnostics()["w"]
    for k in ("rhat_rank", "rhat_bulk", "rhat_fold", "ess_bulk", "ess_tail", "lags_bulk"):
        assert bare[k].tobytes() == full[k].tobytes(), k
    assert bare["ess_q"].shape == (0, pb["n"]) and bare["prob"].shape == (0, pb["n"])
    dp = C.POINTER(C.c_double)
    prob = np.array(PROBS)
    thr = np.array(t).reshape(2, 1)
    side = np.array(sides, dtype=np.int32)
    spec = _lib.StRankSpec(0, 3, prob.ctypes.data_as(dp), 2, thr.ctypes.data_as(dp), side.ctypes.data_as(C.POINTER(C.c_int32)))
    for k in ("rhat_rank", "rhat_bulk", "rhat_fold", "ess_bulk", "ess_tail", "ess_q", "ess_exc", "mcse_prob", "prob"):
        buf = np.full(full[k].shape, -7.0)
        out = _lib.StRankOut()
        setattr(out, k, buf.ctypes.data_as(dp))
        assert hm.lib.st_summary_rank_diagnostics(hm.h, C.byref(spec), C.byref(out), None) == 0
        assert buf.tobytes() == full[k].tobytes(), k
    hm.close()


# ---- 2. the outputs of a series do not depend on where it is stored -------------------------------------------------------------
FLOAT_KEYS = ("rhat_rank", "rhat_bulk", "rhat_fold", "ess_bulk", "ess_tail", "lags_bulk", "ess_q", "ess_exc", "mcse_prob", "prob")


def test_a_series_gives_the_same_bits_wherever_it_is_stored():
    """One series -- the w* draws of point 3 of a point set -- as that point, as a functional of weight 1 on it, as row 0 of the
    n = 64 handle and as row 50 of the n = 81 handle: every output agrees bit for bit, for two lag caps.  A functional of weight
    2.0 on the same point is an exact monotone map: its rhat_bulk, ess_bulk, ess_q and ess_tail are the point's bits, and with
    doubled thresholds so are its ess_exc, mcse_prob and prob."""
    K = 129
    pb = problem("n64")
    hm = hip_model(pb)
    assert hm.get_loglik_comps_w(0)
    points_setup(hm, pb, 9, seed=5)
    hm.set_functionals([([3], [1.0]), ([0, 1], [0.5, 0.5]), ([3], [2.0])])
    assert hm.lib.st_points_summary_reserve(hm.h, K) == 0
    ws, ys, fw, _ = feed_points(hm, pb, K, seed=3)
    x = ws[:, 3].copy()
    assert np.array_equal(fw[:, 0], x) and np.array_equal(fw[:, 2], 2.0 * x)
    t = [float(np.median(x)), float(np.quantile(x, 0.2))]
    sides = (1, -1)
    pick = lambda d, i: {k: np.asarray(d[k])[..., i].copy() for k in FLOAT_KEYS}   # noqa: E731
    outs, doubled = {}, {}
    for max_lag in (0, 7):
        fthr = [np.array([v, v, 2.0 * v]) for v in t]
        fun = hm.functionals_rank_diagnostics(PROBS, fthr, sides, max_lag)["w"]
        outs[max_lag] = [pick(hm.points_rank_diagnostics(PROBS, t, sides, max_lag)["w"], 3), pick(fun, 0)]
        doubled[max_lag] = pick(fun, 2)
    for name, row in (("n64", 0), ("n81", 50)):
        pr = problem(name)
        hr = hip_model(pr) if name != "n64" else hm
        draws = rank_rows(K, pr["n"], seed=11 + row)
        draws[:, row] = x
        assert hr.lib.st_summary_reserve(hr.h, K) == 0
        feed_rows(hr, draws)
        for max_lag in (0, 7):
            outs[max_lag].append(pick(hr.summary_rank_diagnostics(PROBS, t, sides, max_lag)["w"], row))
        if hr is not hm:
            hr.close()
    hm.close()
    for max_lag, o in outs.items():
        for other in o[1:]:
            for k in FLOAT_KEYS:
                assert o[0][k].tobytes() == other[k].tobytes(), (max_lag, k, o[0][k], other[k])
        for k in ("rhat_bulk", "ess_bulk", "ess_tail", "lags_bulk", "ess_q", "ess_exc", "mcse_prob", "prob"):
            assert o[0][k].tobytes() == doubled[max_lag][k].tobytes(), (max_lag, k, o[0][k], doubled[max_lag][k])
        assert o[0]["ess_bulk"] > 0 and o[0]["lags_bulk"] > 0 and 0 < o[0]["prob"][0] < 1


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    from spamtree_amd import _lib
    from spamtree_amd.model import rank_buffers
    pb = problem("n64")
    hm = hip_model(pb)
    lib, h = hm.lib, hm.h
    n = pb["n"]
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    d, o = rank_buffers(n, 2, 2)
    keep = []

    def spec(max_lag=0, probs=(0.1, 0.9), thr=(0.0, 1.0), sides=(1, -1), n_prob=None, n_thr=None):
        p, t = np.array(probs, dtype=np.float64), np.array(thr, dtype=np.float64)
        s = None if sides is None else np.array(sides, dtype=np.int32)
        keep.extend((p, t, s))
        return _lib.StRankSpec(max_lag, len(probs) if n_prob is None else n_prob, p.ctypes.data_as(dp) if p.size else None,
                               len(thr) if n_thr is None else n_thr, t.ctypes.data_as(dp) if t.size else None,
                               None if s is None else s.ctypes.data_as(ip))

    def refused(f, s, text, w=True, y=False, code=ST_ERR_USAGE):
        rc = f(h, C.byref(s) if s is not None else None, C.byref(o) if w else None, C.byref(o) if y else None)
        assert rc == code and text in lib.st_last_error(h), (rc, text, lib.st_last_error(h))

    rows = lib.st_summary_rank_diagnostics
    refused(rows, spec(), b"0 draws stored, the diagnostics need at least 4")           # no reservation
    assert lib.st_summary_reserve(h, 8) == 0
    draws = rank_rows(8, n, seed=1)
    feed_rows(hm, draws[:3])
    refused(rows, spec(), b"3 draws stored")
    feed_rows(hm, draws[3:4])
    refused(rows, spec(max_lag=-1), b"max_lag")
    refused(rows, spec(probs=(0.5,) * 9), b"n_prob = 9 must lie in 0 .. 8")
    refused(rows, spec(n_prob=-1), b"n_prob = -1")
    refused(rows, spec(thr=(0.0,) * 9, sides=(1,) * 9), b"n_thr = 9 must lie in 0 .. 8")
    refused(rows, spec(n_thr=-1), b"n_thr = -1")
    for bad in (0.0, 1.0, -0.5, math.nan):
        refused(rows, spec(probs=(0.5, bad)), b"prob 1 must lie strictly inside (0, 1)")
    refused(rows, spec(thr=(0.0, math.nan)), b"threshold 1 is not finite")
    refused(rows, spec(thr=(math.inf, 0.0)), b"threshold 0 is not finite")
    refused(rows, spec(sides=(1, 0)), b"side 1 must be +1 or -1")
    refused(rows, spec(probs=()), b"ess_q needs prob")
    refused(rows, spec(thr=(), sides=None), b"need thresholds")
    refused(rows, None, b"no spec")
    got = hm.summary_rank_diagnostics(PROBS, [0.0], (1,), n_kept=4)["w"]                # still answers
    check_store(got, np.vstack([draws[:3], draws[3:4]]), [np.zeros(n)], (1,), 0, "after the refusals")
    assert lib.st_summary_rank_diagnostics(h, C.byref(spec()), None, None) == 0
    # points and functionals: before a set, without stored draws, yhat without X
    pts, fun = lib.st_points_summary_rank_diagnostics, lib.st_points_functionals_rank_diagnostics
    refused(pts, spec(), b"before st_points_set")
    refused(fun, spec(), b"")
    assert hm.get_loglik_comps_w(0)
    points_setup(hm, pb, 9, seed=2, X=False)
    refused(fun, spec(), b"before st_points_functionals_set")
    hm.set_functionals([([0, 1], [1.0, 1.0])])
    refused(pts, spec(), b"at least 4")
    refused(fun, spec(thr=(0.0, 1.0)), b"at least 4")
    assert lib.st_points_summary_reserve(h, 6) == 0
    for it in range(3):
        hm.accumulate_points(seed=1, it=it)
    refused(pts, spec(), b"3 draws stored")
    refused(fun, spec(), b"3 draws stored")
    hm.accumulate_points(seed=1, it=3)
    refused(pts, spec(), b"needs the regressors X", y=True)
    refused(fun, spec(), b"needs the regressors X", y=True)
    refused(pts, spec(max_lag=-1), b"max_lag")
    refused(fun, spec(probs=(0.5, 1.5)), b"prob 1")
    got = hm.points_rank_diagnostics(PROBS, [0.0], (1,))
    assert got["yhat"] is None and np.all(got["w"]["ess_bulk"] > 0) and np.all(hm.functionals_rank_diagnostics()["w"]["ess_tail"] > 0)
    # a point set of size 0: ST_OK, nothing written
    hm.set_points(np.zeros((0, 2)), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))
    d["ess_bulk"][:] = -7.0
    assert pts(h, C.byref(spec()), C.byref(o), None) == 0 and np.all(d["ess_bulk"] == -7.0)
    hm.close()
    # a limited_tree handle: the rows are supported, the point calls refused as their siblings are
    pl = problem("lim")
    hl = hip_model(pl)
    assert hl.lib.st_summary_reserve(hl.h, 5) == 0
    dl = rank_rows(5, pl["n"], seed=4)
    feed_rows(hl, dl)
    t, per, sides = thresholds_for(dl)
    check_store(hl.summary_rank_diagnostics(PROBS, t, sides)["w"], dl, per, sides, 0, "limited_tree")
    dd, oo = rank_buffers(pl["n"], 2, 2)
    assert hl.lib.st_points_summary_rank_diagnostics(hl.h, C.byref(spec()), C.byref(oo), None) == ST_ERR_UNSUPPORTED
    hl.close()


# ---- 4. the driver ----------------------------------------------------------------------------------------------------------------
RK = dict(probs=(0.1, 0.5), thresholds=(0.0, 0.4), sides=(1, -1))
RANK_OUT = ("rhat_rank", "rhat_bulk", "rhat_fold", "ess_bulk", "ess_tail", "lags_bulk", "ess_q", "ess_exc", "mcse_prob", "prob", "truncated")


def check_parts(d, draws_by_key, tag, max_lag=0):
    for key, draws in draws_by_key.items():
        per = [np.full(draws.shape[1], t) for t in RK["thresholds"]]
        check_store(d[key], draws, per, RK["sides"], max_lag, f"{tag} {key}", probs=RK["probs"])
        assert d[key]["truncated"].dtype == bool


def same_rank(a, b):
    for part in ("w", "yhat"):
        for key in RANK_OUT:
            assert np.array_equal(a[part][key], b[part][key], equal_nan=True), (part, key)


def stack(lst):
    return np.stack([np.asarray(a).reshape(-1) for a in lst])


def test_driver_plain_chain_combined_and_lean():
    from spamtree_amd import diagnostics as dg
    from spamtree_amd import fit
    from tests.test_gpu_diagnostics import KW, fit_args
    pb = problem("n64")
    res = fit.spamtree_mv_mcmc(*fit_args(pb), rank_diagnostics=RK, **KW)
    base = fit.spamtree_mv_mcmc(*fit_args(pb), **KW)
    both = fit.spamtree_mv_mcmc(*fit_args(pb), rank_diagnostics=RK, diagnostics=True, excursions=dict(thresholds=[0.0, 0.4], side=[1, -1]), **KW)
    only = fit.spamtree_mv_mcmc(*fit_args(pb), diagnostics=True, excursions=dict(thresholds=[0.0, 0.4], side=[1, -1]), **KW)
    for other in (res, both):
        for key in ("beta_mcmc", "tausq_mcmc", "theta_mcmc", "paramsd"):
            assert np.array_equal(other[key], base[key]), key
        for key in ("w_mcmc", "yhat_mcmc"):
            assert all(np.array_equal(a, b) for a, b in zip(other[key], base[key])), key
    assert "rank_diagnostics" not in base and "rank_diagnostics" not in only
    r = res["rank_diagnostics"]
    check_parts(r, dict(w=stack(res["w_mcmc"]), yhat=stack(res["yhat_mcmc"])), "driver")
    same_rank(both["rank_diagnostics"], r)
    for part in ("w", "yhat"):   # the siblings' outputs are the same with and without, and prob is the excursions' prob
        for key in ("ess", "mcse", "sd", "rhat", "lags"):
            assert np.array_equal(both["diagnostics"][part][key], only["diagnostics"][part][key], equal_nan=True), (part, key)
        for key in ("count", "prob", "excur", "joint_all"):
            assert np.array_equal(both["excursions"][part][key], only["excursions"][part][key]), (part, key)
        assert both["excursions"][part]["prob"].tobytes() == r[part]["prob"].tobytes()
    k = res["theta_mcmc"].shape[0]
    for j in range(k):   # the scalar chains on the host
        want = dg.rank_series_diagnostics(res["theta_mcmc"][j], probs=RK["probs"])
        assert want["ess_bulk"] == r["theta"]["ess_bulk"][j] and np.array_equal(want["ess_q"], r["theta"]["ess_q"][:, j])
    p, _, q = res["beta_mcmc"].shape
    assert r["beta"]["rhat_rank"].shape == (p, q) and r["tausq"]["ess_tail"].shape == (q,) and r["beta"]["ess_q"].shape == (2, p, q)
    assert set(r["summary"]) == {"theta", "beta", "tausq", "w", "yhat"} and r["summary"]["w"]["n"] == pb["n"]
    assert set(r["summary"]["w"]["by_outcome"]) == {1}
    lean = fit.spamtree_mv_mcmc(*fit_args(pb), rank_diagnostics=RK, save_w=False, save_yhat=False, **KW)
    assert "w_mcmc" not in lean and "yhat_mcmc" not in lean
    same_rank(lean["rank_diagnostics"], r)
    bare = fit.spamtree_mv_mcmc(*fit_args(pb), rank_diagnostics=True, **KW)["rank_diagnostics"]
    assert bare["w"]["ess_q"].shape == (0, pb["n"]) and np.array_equal(bare["w"]["rhat_rank"], r["w"]["rhat_rank"], equal_nan=True)


def test_driver_with_new_points_and_functionals():
    from spamtree_amd import fit
    from spamtree_amd.predict import locate
    from tests.test_gpu_diagnostics import KW, fit_args
    pb = problem("n64")
    rng = np.random.default_rng(8)
    n_new = 9
    lo, hi = pb["coords"].min(axis=0), pb["coords"].max(axis=0)
    pts = lo + (hi - lo) * rng.uniform(size=(n_new, 2))
    mv = np.ones(n_new, dtype=np.int64)
    new_points = dict(coords=pts, mv=mv, anchor=locate(pb["topo"], pts, mv, device=0), X=rng.standard_normal((n_new, pb["p"])),
                      functionals=[([0, 1, 2], [1.0, 2.0, -3.0]), (list(range(n_new)), [1.0 / n_new] * n_new)])
    res = fit.spamtree_mv_mcmc(*fit_args(pb), rank_diagnostics=RK, new_points=new_points, **KW)
    base = fit.spamtree_mv_mcmc(*fit_args(pb), new_points=new_points, **KW)
    for key in ("beta_mcmc", "tausq_mcmc", "theta_mcmc", "paramsd"):
        assert np.array_equal(res[key], base[key]), key
    assert all(np.array_equal(a, b) for a, b in zip(res["w_mcmc"], base["w_mcmc"]))
    for key in ("w", "yhat", "cond_mean", "cond_var", "mean", "var", "w_mean", "yhat_mean"):
        assert np.array_equal(res["new"][key], base["new"][key]), key
        assert np.array_equal(res["new"]["functionals"][key], base["new"]["functionals"][key]), key
    assert "rank_diagnostics" not in base and "rank_diagnostics" not in base["new"]
    check_parts(res["rank_diagnostics"], dict(w=stack(res["w_mcmc"]), yhat=stack(res["yhat_mcmc"])), "rows")
    check_parts(res["new"]["rank_diagnostics"], dict(w=res["new"]["w"].T, yhat=res["new"]["yhat"].T), "points")
    check_parts(res["new"]["functionals"]["rank_diagnostics"],
                dict(w=res["new"]["functionals"]["w"].T, yhat=res["new"]["functionals"]["yhat"].T), "functionals")
    lean = fit.spamtree_mv_mcmc(*fit_args(pb), rank_diagnostics=RK, new_points=new_points, new_draws=False, save_w=False, save_yhat=False, **KW)
    assert "w" not in lean["new"]
    same_rank(lean["rank_diagnostics"], res["rank_diagnostics"])
    same_rank(lean["new"]["rank_diagnostics"], res["new"]["rank_diagnostics"])
    same_rank(lean["new"]["functionals"]["rank_diagnostics"], res["new"]["functionals"]["rank_diagnostics"])


def test_fit_predict_and_the_replay_pass_rank_diagnostics_on():
    """predict.fit_predict(rank_diagnostics=) and predict.predict_new(rank_diagnostics=) on a q = 2 problem with points of both
    outcomes and two functionals: each against the reference on the draws it returned; the w* draws of the fit and of the replay
    are the same bits, so are their rank outputs."""
    from spamtree_amd.predict import fit_predict, predict_new
    from tests.util import make_problem
    pb = make_problem(side=12, q=2, seed=2, p=2)
    rng = np.random.default_rng(31)
    n_new = 40
    lo, hi = pb["coords"].min(axis=0), pb["coords"].max(axis=0)
    pts = lo + (hi - lo) * rng.uniform(size=(n_new, 2))
    mv = rng.integers(1, 3, size=n_new)
    Xn = rng.standard_normal((n_new, pb["p"]))
    A = [([0, 1, 2], [1.0, 2.0, -3.0]), (list(range(n_new)), [1.0 / n_new] * n_new)]
    thr = np.array([[0.0, 0.2], [0.5, 0.5]])      # per threshold and outcome
    tf = np.array([[0.0, 0.1], [0.3, 0.3]])       # per threshold and functional
    sides = (1, -1)
    rk = dict(probs=(0.25, 0.5), thresholds=[[0.0, 0.2], 0.5], sides=sides, thresholds_fun=[[0.0, 0.1], 0.3])
    kw = dict(mcmc_keep=12, mcmc_burn=4, mcmc_thin=1, adapting=True, seed=77, device=0)
    out = fit_predict(pb, pts, mv, Xn, functionals=A, rank_diagnostics=rk, **kw)
    rep = predict_new(pb, out, pts, mv, Xn, seed=77, device=0, functionals=A, rank_diagnostics=rk)
    per = [t[mv - 1] for t in thr]
    for res, fun, src, tag in ((out["new"]["rank_diagnostics"], out["new"]["functionals"], out["new"], "fit_predict"),
                               (rep["rank_diagnostics"], rep["functionals"], rep, "replay")):
        check_store(res["w"], src["w"].T, per, sides, 0, f"{tag} w*", probs=rk["probs"])
        check_store(res["yhat"], src["yhat"].T, per, sides, 0, f"{tag} yhat*", probs=rk["probs"])
        check_store(fun["rank_diagnostics"]["w"], fun["w"].T, list(tf), sides, 0, f"{tag} F_w", probs=rk["probs"])
        check_store(fun["rank_diagnostics"]["yhat"], fun["yhat"].T, list(tf), sides, 0, f"{tag} F_y", probs=rk["probs"])
    assert np.array_equal(out["new"]["w"], rep["w"])
    for key in RANK_OUT:
        assert np.array_equal(out["new"]["rank_diagnostics"]["w"][key], rep["rank_diagnostics"]["w"][key], equal_nan=True), key
    rows_per = [t[np.asarray(pb["mv_id"]).reshape(-1) - 1] for t in thr]
    check_store(out["rank_diagnostics"]["w"], stack(out["w_mcmc"]), rows_per, sides, 0, "fit_predict rows w", probs=rk["probs"])


def test_zz_report_the_largest_observed_error():
    """Prints the largest error the cases above met (DESIGN.md section 23 records it); fails unless they compared stores (run
    with the file: alone, or without the library's calls, there is nothing to report)."""
    assert OBSERVED["stores"] > 0 and OBSERVED["series"] > 0, "no store was compared"
    print(f"largest observed: score outputs err / bound {OBSERVED['max_err_over_bound']:.3g}, relative err {OBSERVED['max_rel_err']:.3g}; "
          f"integer-defined outputs relative err {OBSERVED['max_int_rel_err']:.3g}")
    assert OBSERVED["max_err_over_bound"] <= 1.0 and OBSERVED["max_int_rel_err"] <= INT_RTOL
