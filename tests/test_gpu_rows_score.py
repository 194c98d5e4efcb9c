"""GPU: criteria over the fit's own rows (st_rows_score_*, k_rows_score_acc / k_rows_score_totals, stm_mcmc_criteria,
fit.spamtree_mv_mcmc(criteria=True)).

The C-ABI is driven directly: w, beta and tausq_inv of every draw are set by the test (st_set_w, st_set_beta, st_set_tausq_inv), XB
is read back (st_get_xb) and taken as exact input.  The reference of every value is tests/rows_score_reference.py at 50 digits (CRPS:
exact rationals); the allowed error is the bound DESIGN.md section 20 derives from the kernels' operation chains.

Not verified here: the refusal of world > 1 handles (ST_ERR_UNSUPPORTED, the first test of every entry point) -- the suite builds
such handles only in spawned rank processes with a communicator."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import rows_score_reference as rr
from tests.util import make_problem

pytestmark = pytest.mark.gpu

ST_ERR_USAGE, ST_ERR_UNSUPPORTED = -1, -4
dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
ROW_KEYS = ("lppd", "p_waic", "mean_ll", "mu_mean", "pit")
mpf = lambda x: rr.mp.mpf(float(x))   # noqa: E731

_PB = {}


def problem(key):
    if key not in _PB:
        _PB[key] = {"q1": lambda: make_problem(side=8, q=1, seed=61, missing=0.2, p=2),
                    "q3": lambda: make_problem(side=14, q=3, seed=63, missing=(0.1, 0.3, 0.5), p=2),
                    "single": lambda: make_problem(side=8, q=2, seed=62, missing=0.2, p=2, single_obs=2)}[key]()
    return _PB[key]


def model(pb, limited=False):
    from spamtree_amd.model import SpamTreeMV
    return SpamTreeMV(pb["y"], pb["X"], pb["Z"], pb["coords"], pb["mv_id"], pb["blocking"], pb["gix_block"], pb["res_is_ref"],
                      pb["parents"], pb["children"], limited, pb["block_names"], pb["block_groups"], pb["indexing"],
                      np.zeros(pb["n"]), np.zeros(pb["p"]), pb["theta"], 5.0)


def holdout(pb, frac=0.5, seed=5, scale=1.5):
    """Held-out values at about `frac` of the NA rows (at least one where there is any), NaN elsewhere."""
    rng = np.random.default_rng(seed)
    na = np.nonzero(np.isnan(pb["y"]))[0]
    pick = na[rng.uniform(size=na.size) < frac] if frac < 1.0 else na
    if na.size and not pick.size:
        pick = na[:1]
    h = np.full(pb["n"], np.nan)
    h[pick] = scale * rng.standard_normal(pick.size)
    return h


def set_tausq_inv(hm, ti):
    hm.tausq_inv = np.ascontiguousarray(ti, dtype=np.float64)
    hm._check(hm.lib.st_set_tausq_inv(hm.h, dp(hm.tausq_inv)))


def draws(hm, pb, S, seed=77, tausq_inv=None, w=None):
    """S accumulated draws with a state of the test's own each: (xbs, ws, tis), what the device had at every draw."""
    rng = np.random.default_rng(seed)
    xbs, ws, tis = [], [], []
    for s in range(S):
        wv = rng.standard_normal(pb["n"]) if w is None else np.asarray(w[s], dtype=np.float64)
        hm.set_w(wv)
        hm.beta_update(np.asfortranarray(rng.standard_normal((pb["p"], pb["q"]))))
        set_tausq_inv(hm, rng.uniform(2.0, 20.0, pb["q"]) if tausq_inv is None else tausq_inv[s])
        xbs.append(hm.get_XB())
        ws.append(wv.copy())
        tis.append(hm.tausq_inv.copy())
        hm.rows_score_accumulate()
    return xbs, ws, tis


def targets(pb, hold):
    t = pb["y"].copy()
    if hold is not None:
        t[np.isnan(t)] = hold[np.isnan(t)]
    return t


def check_rows(got, pb, hold, xbs, ws, tis, tag, rows=None):
    """Every per-row output of the (listed) rows within its bound; NaN exactly where the definitions say."""
    S = len(xbs)
    t = targets(pb, hold)
    obs = np.isfinite(pb["y"])
    worst = {k: 0.0 for k in ROW_KEYS}
    for i in (range(pb["n"]) if rows is None else rows):
        if np.isnan(t[i]):
            assert all(np.isnan(got[k][i]) for k in ROW_KEYS), (tag, i)
            continue
        j = pb["mv_id"][i] - 1
        ref = rr.row_values(t[i], [x[i] for x in xbs], [w[i] for w in ws], [ti[j] for ti in tis], held=not obs[i])
        if obs[i]:
            assert np.isnan(got["pit"][i]), (tag, i)
        for k, (val, bound) in ref.items():
            err = abs(float(mpf(got[k][i]) - val))
            assert np.isfinite(got[k][i]) and err <= bound, (tag, k, i, err, bound, got[k][i], float(val))
            if bound > 0:
                worst[k] = max(worst[k], err / bound)
    print(f"{tag}: S={S} worst error / bound: " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def check_totals(hm, got, pb, hold, tis, tag, dhat=True, crps=None):
    """The tables against math.fsum over the device's own per-row outputs within gamma_c sum |term|; Dhat (dhat=True) against the
    50-digit log N(t; mu_mean, tau2bar) at the device's own mu_mean; the derived rows exactly."""
    from spamtree_amd import _lib
    tobs, theld, n_obs, n_held = hm.rows_score_totals(raw=True)
    t = targets(pb, hold)
    obs = np.isfinite(pb["y"])
    n = pb["n"]
    O = {k: i for i, k in enumerate(_lib.ST_ROWS_OBS)}
    H = {k: i for i, k in enumerate(_lib.ST_ROWS_HELD)}
    for j in range(pb["q"]):
        mj = pb["mv_id"] == j + 1
        so, sh = obs & mj, ~obs & mj & np.isfinite(t)
        assert n_obs[j] == so.sum() and n_held[j] == sh.sum(), (tag, j)
        col = tobs[:, j]
        if not so.any():
            assert not col.any(), (tag, j)
        for key, rk, mult in (("lppd", "lppd", 1.0), ("p_waic", "p_waic", 1.0), ("Dbar", "mean_ll", -2.0)):
            terms = got[rk][so]
            want = mult * math.fsum(terms)
            assert abs(col[O[key]] - want) <= abs(mult) * rr.totals_bound(n, terms), (tag, j, key, col[O[key]], want)
        assert col[O["waic"]] == -2.0 * (col[O["lppd"]] - col[O["p_waic"]]), (tag, j)
        assert col[O["p_D"]] == col[O["Dbar"]] - col[O["Dhat"]] and col[O["dic"]] == col[O["Dbar"]] + col[O["p_D"]], (tag, j)
        if dhat and so.any():
            t2, t2rel = rr.tau2bar([ti[j] for ti in tis])
            ln = [rr.log_normal_at_mean(t[i], got["mu_mean"][i], t2, t2rel) for i in np.nonzero(so)[0]]
            want = -2 * rr.mp.fsum(x[0] for x in ln)
            bound = 2 * (math.fsum(x[1] for x in ln) + rr.totals_bound(n, [x[0] for x in ln]))
            assert abs(float(mpf(col[O["Dhat"]]) - want)) <= bound, (tag, j, col[O["Dhat"]], float(want), bound)
        hcol = theld[:, j]
        for key, rk in (("lppd", "lppd"), ("pit", "pit")):
            terms = got[rk][sh]
            assert abs(hcol[H[key]] - math.fsum(terms)) <= rr.totals_bound(n, terms), (tag, j, key)
        e2 = [(mpf(t[i]) - mpf(got["mu_mean"][i])) ** 2 for i in np.nonzero(sh)[0]]
        # e = fl(t - mu_mean) squared inside the fused multiply-add: 2 u e^2 per term on top of the chain
        assert abs(float(mpf(hcol[H["sqerr"]]) - rr.mp.fsum(e2))) <= rr.totals_bound(n, e2) + 2 * rr.U * float(rr.mp.fsum(e2)), (tag, j)
        if crps is None:
            assert hcol[H["crps"]] == 0.0, (tag, j)
        else:
            assert abs(hcol[H["crps"]] - math.fsum(crps[sh])) <= rr.totals_bound(n, crps[sh]), (tag, j)
    return tobs, theld, n_obs, n_held


# ---- 1. per-row values against the 50-digit restatement ---------------------------------------------------------------------
@pytest.mark.parametrize("key,S", [("q1", 5), ("q3", 5)])
def test_rows_against_extended_precision(key, S):
    pb = problem(key)
    assert pb["n"] == {"q1": 64, "q3": 588}[key]
    hold = holdout(pb)
    hm = model(pb)
    hm.rows_score_set(hold, y=pb["y"])
    xbs, ws, tis = draws(hm, pb, S)
    got = hm.rows_score_get()
    assert got["n_accumulated"] == S
    check_rows(got, pb, hold, xbs, ws, tis, key)
    check_totals(hm, got, pb, hold, tis, key)
    by = hm.rows_score_info()["alg_bytes"]
    nt, nh = int(np.isfinite(targets(pb, hold)).sum()), int(np.isfinite(hold).sum())
    assert by == 8.0 * pb["n"] + 101.0 * nt + 16.0 * nh
    hm.close()


# ---- 2. edges on the 64-row problem ---------------------------------------------------------------------------------------------
def test_edges():
    pb = problem("q1")
    n = pb["n"]
    hold = holdout(pb, frac=1.0)
    hm = model(pb)
    # S = 1: lppd = mean_ll = l, no penalty
    hm.rows_score_set(hold, y=pb["y"])
    xbs, ws, tis = draws(hm, pb, 1)
    one = hm.rows_score_get()
    tg = np.isfinite(targets(pb, hold))
    assert np.array_equal(one["lppd"][tg], one["mean_ll"][tg]) and not one["p_waic"][tg].any()
    check_rows(one, pb, hold, xbs, ws, tis, "S=1")
    check_totals(hm, one, pb, hold, tis, "S=1")
    # the same state accumulated twice: A = 2 and lppd = M + log(2 / 2) = l bit for bit, p_waic = 0 exactly, the means unchanged
    hm.rows_score_accumulate()
    two = hm.rows_score_get()
    assert two["n_accumulated"] == 2
    for k in ROW_KEYS:
        assert np.array_equal(two[k], one[k], equal_nan=True), k
    # targets 1e4 sigma away: every exp l underflows, lppd stays finite and within the bound
    far = np.where(np.isnan(pb["y"]), 1e4, np.nan)
    hm.rows_score_set(far, y=pb["y"])
    xbs, ws, tis = draws(hm, pb, 4, seed=3, tausq_inv=[[1.0]] * 4, w=[np.zeros(n)] * 4)
    g = hm.rows_score_get()
    na = np.isnan(pb["y"])
    assert np.all(g["lppd"][na] < -4e7) and np.all(np.isfinite(g["lppd"][na])) and np.all(g["pit"][na] == 1.0)
    check_rows(g, pb, far, xbs, ws, tis, "far", rows=np.nonzero(na)[0])
    # tausq_inv of 1e30 and 1e-30: nothing NaN
    hm.rows_score_set(hold, y=pb["y"])
    xbs, ws, tis = draws(hm, pb, 4, seed=4, tausq_inv=[[1e30], [1e-30], [1e30], [1e-30]])
    g = hm.rows_score_get()
    for k in ROW_KEYS[:4]:
        assert np.all(np.isfinite(g[k][tg])), k
    assert np.all(np.isfinite(g["pit"][na]))
    check_rows(g, pb, hold, xbs, ws, tis, "tausq_inv 1e+-30")
    tobs, theld, _, _ = check_totals(hm, g, pb, hold, tis, "tausq_inv 1e+-30")
    assert np.all(np.isfinite(tobs)) and np.all(np.isfinite(theld))
    # a target equal to mu: beta = 0 gives XB = 0 exactly, w = the target
    hm.rows_score_set(hold, y=pb["y"])
    t = targets(pb, hold)
    hm.beta_update(np.zeros((pb["p"], 1)))
    assert not hm.get_XB().any()
    hm.set_w(np.where(np.isfinite(t), t, 0.0))
    set_tausq_inv(hm, [4.0])
    hm.rows_score_accumulate()
    g = hm.rows_score_get()
    assert np.all(g["lppd"][tg] == g["lppd"][tg][0]) and np.array_equal(g["mu_mean"][tg], t[tg]) and np.all(g["pit"][na] == 0.5)
    # l = -log(1 / 2) - log(2 pi) / 2 = -0.226: the log within 2 u log 2, the rounded constant within u 0.92, the add within u 0.23
    assert abs(g["lppd"][tg][0] - float(-rr.mp.log(rr.mp.mpf(0.5)) - rr.HL2PI)) <= 3 * rr.U
    hm.close()


def test_no_held_out_value_equals_the_null_call_and_an_outcome_with_one_row():
    pb = problem("q1")
    res = []
    for hold in (None, np.full(pb["n"], np.nan)):
        hm = model(pb)
        hm.rows_score_set(hold)
        draws(hm, pb, 3)
        res.append((hm.rows_score_get(), hm.rows_score_totals(raw=True)))
        hm.close()
    for k in ROW_KEYS:
        assert np.array_equal(res[0][0][k], res[1][0][k], equal_nan=True), k
    for a, b in zip(res[0][1], res[1][1]):
        assert np.array_equal(a, b)
    assert res[1][1][3].tolist() == [0] and not res[1][1][1].any() and np.isnan(res[1][0]["pit"]).all()
    # q = 2 with a single observed row of outcome 2 and none of it held out
    ps = problem("single")
    assert np.isfinite(ps["y"][ps["mv_id"] == 2]).sum() == 1
    hold = holdout(ps, frac=1.0)
    hold[ps["mv_id"] == 2] = np.nan
    hm = model(ps)
    hm.rows_score_set(hold, y=ps["y"])
    xbs, ws, tis = draws(hm, ps, 3)
    g = hm.rows_score_get()
    check_rows(g, ps, hold, xbs, ws, tis, "single_obs")
    tobs, theld, n_obs, n_held = check_totals(hm, g, ps, hold, tis, "single_obs")
    i = int(np.nonzero((ps["mv_id"] == 2) & np.isfinite(ps["y"]))[0][0])
    assert n_obs[1] == 1 and n_held[1] == 0 and not theld[:, 1].any()
    assert tobs[0, 1] == g["lppd"][i] and tobs[1, 1] == g["p_waic"][i] and tobs[3, 1] == -2.0 * g["mean_ll"][i]
    tot = hm.rows_score_totals()
    assert np.isnan(tot["held_out"]["by_outcome"]["rmse"][1]) and tot["observed"]["n"] == int(n_obs.sum())
    hm.close()


@pytest.mark.parametrize("ti_mid", [0.0, np.inf])
def test_a_draw_of_density_zero(ti_mid):
    """tausq_inv of 0 (sigma infinite: r = 0, l = -inf) or infinity (sigma 0: r infinite, l = inf - inf) in the middle draw of three:
    the draw leaves the log-sum-exp alone and enters the moments of l at their running mean, S counts it, nothing is NaN."""
    pb = problem("q1")
    hold = holdout(pb, frac=1.0)
    hm = model(pb)
    hm.rows_score_set(hold, y=pb["y"])
    xbs, ws, tis = draws(hm, pb, 3, seed=8, tausq_inv=[[4.0], [ti_mid], [9.0]])
    g = hm.rows_score_get()
    t = targets(pb, hold)
    tg, na = np.isfinite(t), np.isnan(pb["y"])
    for k in ROW_KEYS[:4]:
        assert np.all(np.isfinite(g[k][tg])), k
    assert np.all(np.isfinite(g["pit"][na]))
    mp = rr.mp
    for i in np.nonzero(tg)[0]:
        d = [rr.row_draw(t[i], xbs[s][i], ws[s][i], tis[s][0]) for s in (0, 2)]
        (l1, r1, _, dl1, dp1), (l3, r3, _, dl3, dp3) = d
        dl = max(dl1, dl3)
        seq = [l1, l1, l3]                                            # the skipped draw at the running mean
        mean = mp.fsum(seq) / 3
        m2 = mp.fsum((x - mean) ** 2 for x in seq)
        sq = float(mp.fsum(x * x for x in seq))
        lppd = mp.log((mp.exp(l1) + mp.exp(l3)) / 3)
        assert abs(float(mpf(g["lppd"][i]) - lppd)) <= dl + rr.lme_bound(3, lppd), i
        assert abs(float(mpf(g["mean_ll"][i]) - mean)) <= dl + rr.welford_mean_bound(3, sq), i
        assert abs(float(mpf(g["p_waic"][i]) - m2 / 2)) <= rr.welford_m2_bound(3, sq, m2, dl) / 2 + rr.U * float(m2 / 2), i
        mus = [mpf(xbs[s][i]) + mpf(ws[s][i]) for s in range(3)]
        sm = float(mp.fsum(m * m for m in mus))
        assert abs(float(mpf(g["mu_mean"][i]) - mp.fsum(mus) / 3)) <= rr.U * math.sqrt(sm) + rr.welford_mean_bound(3, sm), i
        if na[i]:
            mid = mp.mpf(0.5) if ti_mid == 0.0 else mp.mpf(1.0 if t[i] > float(mus[1]) else 0.0)
            pit = (mp.erfc(-r1 / mp.sqrt(2)) / 2 + mid + mp.erfc(-r3 / mp.sqrt(2)) / 2) / 3
            assert abs(float(mpf(g["pit"][i]) - pit)) <= max(dp1, dp3) + rr.U * (2 * rr.E_ERFC + 3 + 1), i
    tobs, theld, _, _ = hm.rows_score_totals(raw=True)
    assert not np.isnan(tobs).any() and not np.isnan(theld).any()
    assert hm.rows_score_totals()["held_out"]["crps"] is None          # no draw is stored
    hm.close()


# ---- 3. launch shapes ------------------------------------------------------------------------------------------------------------
_PROBE = {}


def probe():
    """A 25-row handle whose rows stand in for rows of another problem: X = 0 makes XB = 0 exactly, so with w = fl(XB + w) of the
    other row, its target as the held-out value and its tausq_inv, a probe row sees that row's inputs bit for bit -- alone."""
    if not _PROBE:
        pb = make_problem(side=5, q=1, seed=64, missing=0.6, p=2)
        pb = dict(pb, X=np.zeros_like(pb["X"]))
        _PROBE.update(pb=pb, hm=model(pb), slots=np.nonzero(np.isnan(pb["y"]))[0])
    return _PROBE["pb"], _PROBE["hm"], _PROBE["slots"]


def rows_alone(t, mus, tis):
    """lppd, p_waic, mean_ll, mu_mean and pit of rows with targets t (k), per-draw means mus (S x k) and tausq_inv tis (S), each
    computed on the probe handle."""
    pb, hm, slots = probe()
    k = len(t)
    assert k <= slots.size
    hold = np.full(pb["n"], np.nan)
    hold[slots[:k]] = t
    hm.rows_score_set(hold, y=pb["y"])
    for mu, ti in zip(mus, tis):
        w = np.zeros(pb["n"])
        w[slots[:k]] = mu
        hm.set_w(w)
        set_tausq_inv(hm, [ti])
        hm.rows_score_accumulate()
    g = hm.rows_score_get()
    return {key: g[key][slots[:k]] for key in ROW_KEYS}


@pytest.mark.parametrize("side", [5, 16, 17, 513])
def test_launch_shapes(side):
    NT, STATS_WG = rr.NT, rr.STATS_WG
    pb = make_problem(side=side, q=1, seed=70 + side % 7, missing=0.25, p=2)
    n, S = pb["n"], 3
    assert n == side * side and (side != 513 or n >= STATS_WG * NT + 1) and (side != 16 or n == NT)
    hold = holdout(pb, frac=0.7, seed=side)
    hm = model(pb)
    hm.rows_score_set(hold, y=pb["y"])
    xbs, ws, tis = draws(hm, pb, S, seed=side)
    got = hm.rows_score_get()
    t = targets(pb, hold)
    assert np.array_equal(np.isnan(got["lppd"]), np.isnan(t))
    check_totals(hm, got, pb, hold, tis, f"side={side}", dhat=side <= 17)
    # sampled rows alone, a probe's worth at a time: the first and last targeted rows and random ones; observed rows too (the probe
    # scores them as held-out rows, the same operations plus the pit)
    rng = np.random.default_rng(side)
    tg = np.nonzero(np.isfinite(t))[0]
    rows = np.unique(np.concatenate([tg[:6], tg[-6:], rng.choice(tg, min(36, tg.size), replace=False)]))
    k = probe()[2].size
    for lo in range(0, rows.size, k):
        rb = rows[lo:lo + k]
        alone = rows_alone(t[rb], [x[rb] + w[rb] for x, w in zip(xbs, ws)], [ti[0] for ti in tis])
        for key in ROW_KEYS[:4]:
            assert np.array_equal(alone[key], got[key][rb]), (side, key, lo)
        held = np.isnan(pb["y"][rb])
        assert np.array_equal(alone["pit"][held], got["pit"][rb][held]), (side, lo)
    hm.close()


# ---- 4. CRPS of the stored yhat draws -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3, 33])
def test_crps(K):
    from fractions import Fraction
    pb = problem("q1")
    hold = holdout(pb, frac=0.8, seed=9)
    hm = model(pb)
    hm.rows_score_set(hold, y=pb["y"])
    hm._check(hm.lib.st_summary_reset(hm.h))
    hm._check(hm.lib.st_summary_reserve(hm.h, K))
    rng = np.random.default_rng(K)
    yh = []
    for s in range(K):
        hm.set_w(rng.standard_normal(pb["n"]))
        hm.beta_update(np.asfortranarray(rng.standard_normal((pb["p"], 1))))
        set_tausq_inv(hm, rng.uniform(2.0, 20.0, 1))
        hm.rows_score_accumulate()
        hm._check(hm.lib.st_summary_accumulate(hm.h, 11, s))
        yh.append(hm.yhat(seed=11, it=s))                   # stream 5 with the same counter: the stored draw
    g = hm.rows_score_get(crps=True)
    hd = np.isfinite(hold)
    assert np.isnan(g["crps"][~hd]).all() and hd.sum() >= 5
    for i in np.nonzero(hd)[0]:
        want, mad = rr.crps_sorted([y[i] for y in yh], hold[i])
        assert abs(Fraction(float(g["crps"][i])) - want) <= rr.crps_bound(K, mad), (K, i)
    check_totals(hm, g, pb, hold, None, f"crps K={K}", dhat=False, crps=g["crps"])
    tot = hm.rows_score_totals()["held_out"]
    assert tot["crps"] is not None and abs(tot["crps"] - math.fsum(g["crps"][hd]) / hd.sum()) <= rr.totals_bound(pb["n"], g["crps"][hd]) / hd.sum() + 2 * rr.U * tot["crps"]
    hm.close()


# ---- 5. failures and refusals -----------------------------------------------------------------------------------------------------
def test_refusals():
    pb = problem("q1")
    hm = model(pb)
    lib, h, n = hm.lib, hm.h, pb["n"]
    out = np.zeros(n)
    tab = np.zeros(7)
    cnt = np.zeros(1, dtype=np.int64)
    ip = cnt.ctypes.data_as(C.POINTER(C.c_int64))
    for call in (lambda: lib.st_rows_score_accumulate(h), lambda: lib.st_rows_score_get(h, dp(out), None, None, None, None, None, None),
                 lambda: lib.st_rows_score_totals(h, dp(tab), None, ip, None)):
        assert call() == ST_ERR_USAGE and b"before st_rows_score_set" in lib.st_last_error(h)
    by = C.c_double(-1.0)
    assert lib.st_rows_score_info(h, C.byref(by)) == 0 and by.value == 0.0
    assert lib.st_rows_score_clear(h) == 0                                     # nothing to free is no error
    na, ob = np.nonzero(np.isnan(pb["y"]))[0], np.nonzero(np.isfinite(pb["y"]))[0]
    good = np.full(n, np.nan)
    good[na[0]] = 0.5
    assert lib.st_rows_score_set(h, dp(good)) == 0
    assert lib.st_rows_score_get(h, dp(out), None, None, None, None, None, ip) == ST_ERR_USAGE and cnt[0] == 0
    assert b"no iteration accumulated" in lib.st_last_error(h)
    assert lib.st_rows_score_totals(h, dp(tab), None, None, None) == ST_ERR_USAGE and b"no iteration accumulated" in lib.st_last_error(h)
    hm.rows_score_accumulate()
    before = hm.rows_score_get()
    # a bad y_holdout names the row and leaves the previous state in place
    bad = good.copy()
    bad[ob[3]] = 1.0
    assert lib.st_rows_score_set(h, dp(bad)) == ST_ERR_USAGE
    assert f"y_holdout[{ob[3]}] is finite at an observed row".encode() in lib.st_last_error(h)
    bad = good.copy()
    bad[na[1]] = np.inf
    assert lib.st_rows_score_set(h, dp(bad)) == ST_ERR_USAGE and f"y_holdout[{na[1]}] is infinite".encode() in lib.st_last_error(h)
    after = hm.rows_score_get()
    assert after["n_accumulated"] == 1
    for k in ROW_KEYS:
        assert np.array_equal(before[k], after[k], equal_nan=True), k
    # crps without a stored draw
    assert lib.st_rows_score_get(h, None, None, None, None, None, dp(out), None) == ST_ERR_USAGE
    assert b"crps needs a stored draw" in lib.st_last_error(h)
    # every output may be NULL
    assert lib.st_rows_score_get(h, None, None, None, None, None, None, None) == 0
    assert lib.st_rows_score_totals(h, None, None, None, None) == 0
    assert lib.st_rows_score_clear(h) == 0
    assert lib.st_rows_score_accumulate(h) == ST_ERR_USAGE and b"before st_rows_score_set" in lib.st_last_error(h)
    hm.close()


def test_a_limited_tree_handle_is_supported():
    pl = make_problem(side=8, q=1, seed=61, missing=0.2, p=2, limited_tree=True)
    hold = holdout(pl)
    hl = model(pl, limited=True)
    hl.rows_score_set(hold, y=pl["y"])
    xbs, ws, tis = draws(hl, pl, 3)
    g = hl.rows_score_get()
    check_rows(g, pl, hold, xbs, ws, tis, "limited_tree")
    check_totals(hl, g, pl, hold, tis, "limited_tree")
    hl.close()


# ---- 6. the driver ----------------------------------------------------------------------------------------------------------------
def fit_args(pb):
    k = pb["theta"].size
    return (pb["y"], pb["X"], pb["Z"], pb["coords"], pb["mv_id"], pb["blocking"], pb["gix_block"], pb["res_is_ref"], pb["parents"],
            pb["children"], False, pb["block_names"], pb["block_groups"], pb["indexing"], pb["bounds"], np.zeros(pb["n"]), pb["theta"],
            np.zeros(pb["p"]), 0.1, 0.02 * np.eye(k))


def test_driver_equals_the_hand_stepped_calls_and_leaves_the_chain_alone():
    from spamtree_amd import _lib, fit
    pb = problem("q3")
    keep = 12
    kw = dict(mcmc_keep=keep, mcmc_burn=0, mcmc_thin=1, seed=17, adapting=True, main_verbose=False)
    # observed rows only, without prediction: what stm_step runs per iteration
    res = fit.spamtree_mv_mcmc(*fit_args(pb), criteria=True, sample_predicts=False, **kw)
    base = fit.spamtree_mv_mcmc(*fit_args(pb), sample_predicts=False, **kw)
    for key in ("beta_mcmc", "tausq_mcmc", "theta_mcmc", "paramsd"):
        assert np.array_equal(res[key], base[key]), key
    for key in ("w_mcmc", "yhat_mcmc"):
        assert all(np.array_equal(a, b) for a, b in zip(res[key], base[key])), key
    ch = fit.Chain(pb["y"], pb["X"], pb["Z"], pb["coords"], pb["mv_id"], pb["blocking"], pb["gix_block"], pb["res_is_ref"], pb["parents"],
                   pb["children"], False, pb["block_names"], pb["block_groups"], pb["indexing"], pb["bounds"], pb["theta"], np.zeros(pb["p"]),
                   0.1, 0.02 * np.eye(pb["theta"].size), seed=17, adapting=True)
    lib = ch.lib
    assert lib.stm_rows_score_set(ch.c, None) == 0
    for _ in range(keep):
        ch.step(1)
        assert lib.st_rows_score_accumulate(ch.h) == 0
    n, q = pb["n"], pb["q"]
    rows = {k: np.zeros(n) for k in ROW_KEYS}
    cnt = C.c_int64()
    assert lib.st_rows_score_get(ch.h, dp(rows["lppd"]), dp(rows["p_waic"]), dp(rows["mean_ll"]), dp(rows["mu_mean"]), dp(rows["pit"]),
                                 None, C.byref(cnt)) == 0 and cnt.value == keep
    tobs, theld = np.zeros((7, q), order="F"), np.zeros((4, q), order="F")
    assert lib.st_rows_score_totals(ch.h, dp(tobs), dp(theld), None, None) == 0
    ch.close()
    cr = res["criteria"]
    assert cr["n_accumulated"] == keep and cr["crps"] is None
    for k in ROW_KEYS:
        assert np.array_equal(cr[k], rows[k], equal_nan=True), k
    o = cr["totals"]["observed"]
    for i, k in enumerate(_lib.ST_ROWS_OBS):
        assert np.array_equal(o["by_outcome"][k], tobs[i]), k
    assert cr["totals"]["held_out"]["n"] == 0 and o["n"] == int(np.isfinite(pb["y"]).sum())


def test_the_driver_passes_on_the_refusal_of_a_bad_y_holdout():
    from spamtree_amd import _lib, fit
    pb = problem("q1")
    lib = _lib.load()
    spb, keep, n, p, q = fit._problem(pb["y"], pb["X"], pb["coords"], pb["mv_id"], pb["res_is_ref"], pb["parents"], pb["children"],
                                      pb["block_names"], pb["block_groups"], pb["indexing"])
    k = pb["theta"].size
    bounds, sd = np.asfortranarray(pb["bounds"]), np.asfortranarray(0.02 * np.eye(k))
    theta, beta = np.ascontiguousarray(pb["theta"]), np.zeros(p)
    opt = _lib.StOptions(0, 1, 0, 1, 0, 0)
    fl = _lib.StmFlags(1, 1, 1, 1, 1, 1)
    bad = np.full(n, np.nan)
    bad[np.nonzero(np.isfinite(pb["y"]))[0][2]] = 0.5                 # finite at an observed row: st_rows_score_set refuses
    cs = _lib.StmCriteria(dp(bad), 0, *([None] * 11))
    rc = lib.stm_mcmc_criteria(C.byref(spb), C.byref(opt), dp(bounds), dp(theta), k, dp(beta), 0.1, dp(sd), 2, 0, 1, 17, C.byref(fl),
                               None, None, None, None, None, None, None, C.byref(cs))
    assert rc == ST_ERR_USAGE


def test_fit_returns_the_documented_criteria_with_held_out_rows():
    from spamtree_amd import _lib, fit
    pb = problem("q3")
    keep = 12
    hold = holdout(pb, frac=0.6, seed=2)
    kw = dict(mcmc_keep=keep, mcmc_burn=2, mcmc_thin=1, seed=23, adapting=True, main_verbose=False)
    res = fit.spamtree_mv_mcmc(*fit_args(pb), y_holdout=hold, save_w=False, save_yhat=False, **kw)
    base = fit.spamtree_mv_mcmc(*fit_args(pb), **kw)
    for key in ("beta_mcmc", "tausq_mcmc", "theta_mcmc", "paramsd"):
        assert np.array_equal(res[key], base[key]), key
    assert "w_mcmc" not in res and "yhat_mcmc" not in res
    cr = res["criteria"]
    assert set(cr) == {"lppd", "p_waic", "mean_ll", "mu_mean", "pit", "crps", "n_accumulated", "totals"} and cr["n_accumulated"] == keep
    t = targets(pb, hold)
    hd = np.isfinite(hold)
    for k in ROW_KEYS[:4]:
        assert np.array_equal(np.isnan(cr[k]), np.isnan(t)), k
    assert np.array_equal(np.isfinite(cr["pit"]), hd) and np.array_equal(np.isfinite(cr["crps"]), hd)
    # the stored yhat draws are st_yhat's: the CRPS of base's yhat_mcmc at the held-out rows, exactly restated
    for i in np.nonzero(hd)[0][:20]:
        want, mad = rr.crps_sorted([y[i, 0] for y in base["yhat_mcmc"]], hold[i])
        assert abs(float(cr["crps"][i]) - float(want)) <= rr.crps_bound(keep, mad) + rr.U * float(want), i
    tot = cr["totals"]
    o, h = tot["observed"], tot["held_out"]
    assert set(o) == {"n", "by_outcome", *_lib.ST_ROWS_OBS} and set(h) == {"n", "by_outcome", "lppd", "pit", "crps", "mse", "rmse"}
    assert o["waic"] == -2.0 * (o["lppd"] - o["p_waic"]) and o["dic"] == o["Dbar"] + o["p_D"] and o["p_D"] == o["Dbar"] - o["Dhat"]
    b = o["by_outcome"]
    assert np.array_equal(b["waic"], -2.0 * (b["lppd"] - b["p_waic"])) and np.array_equal(b["dic"], b["Dbar"] + b["p_D"])
    assert o["n"] == int(np.isfinite(pb["y"]).sum()) and h["n"] == int(hd.sum()) and h["by_outcome"]["n"].sum() == h["n"]
    assert h["rmse"] == math.sqrt(h["mse"]) and 0.0 < h["pit"] < 1.0 and h["crps"] > 0.0 and np.isfinite(h["lppd"])
    # the reduction's chain, the rounded difference squared inside the fused multiply-add (2 u), the host's sum over the outcomes
    # and its division, and this line's own squares: 8 u on top of gamma_c
    e2 = (t[hd] - cr["mu_mean"][hd]) ** 2
    assert abs(h["mse"] - math.fsum(e2) / h["n"]) <= (rr.totals_bound(pb["n"], e2) + 8 * rr.U * math.fsum(e2)) / h["n"]
    assert o["p_waic"] > 0.0 and o["p_D"] != 0.0
