"""GPU: Pareto smoothing of the leave-one-out weights (k_loo_psis / k_psis_finish through st_psis, st_rows_loo_reserve / _draws /
_psis / _psis_totals, stm_mcmc_fit with loo's psis part, fit.spamtree_mv_mcmc(loo=True, psis=True)).

The reference is tests/psis_reference.py, the 50-digit restatement; integers, the inf / NaN pattern and which series smooth must be
exact, the doubles lie within DEVICE_FACTOR = 256 times the float64 definition's measured distance from the restatement
(F64_DISTANCE = 1.9e-13, tests/test_psis_cpu.py: 4.9e-11 in psis_reference.distance's measure), taken over the whole list.

MEASURED on an MI355X (the first test prints it): the largest distance of the device from the restatement over the 733 series is
5.33e-14 (khat of a K = 25 series), 0.0011 of the bound; the series that do not smooth lie within 0.018 of get_bounds' bound of the
long-double raw estimator.
"""
import ctypes as C
import math

import numpy as np
import pytest

from tests import loo_reference as lr
from tests import psis_reference as pr
from tests.test_gpu_rows_loo import fit_args, get_bounds, tausq_rows
from tests.test_gpu_simulate import CASES, hip_model
from tests.util import make_problem

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
ST_ERR_USAGE, ST_ERR_UNSUPPORTED = -1, -4
DBL = ("khat", "elpd_psis", "pit_psis", "mu_psis", "weight_ess_psis")
INT = ("tail_len", "n_draws")
ALL = DBL + INT


def dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


def same(a, b, keys=ALL):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


@pytest.fixture(scope="module")
def hm():
    m = hip_model(CASES["q1_grid"]())
    yield m
    m.close()


def test_case_list_against_the_restatement(hm):
    bound = pr.DEVICE_FACTOR * pr.F64_DISTANCE
    worst, where, raw_worst, n_series, n_smooth = 0.0, None, 0.0, 0, 0
    for name, t, phi, mu in pr.case_list():
        ref = pr.reference(name)
        got = hm.psis(t, phi, mu)
        K, n = t.shape
        info = hm.psis_info(n, K)
        assert info["Kpad"] >= K and info["Kpad"] < max(2 * K, 3) and 1 <= info["R"] <= 8
        for i in range(n):
            g = {k: got[k][i] for k in ALL}
            assert g["tail_len"] == ref[i]["tail_len"] and g["n_draws"] == ref[i]["n_draws"], (name, i, g)
            assert (g["tail_len"] > 0) == ref[i]["smoothed"]
            d = pr.distance(ref[i], g)        # asserts the inf / NaN pattern
            if d > worst:
                worst, where = d, (name, i)
            n_series += 1
            n_smooth += ref[i]["smoothed"]
            if not ref[i]["smoothed"] and ref[i]["n_draws"] > 0:
                # no smoothing: the long-double raw estimator under the existing test's bounds (the ratios are given: z = 0, sigma = 1)
                ok = np.isfinite(t[:, i])
                ls, ph, ms = -t[ok, i][:, None], phi[ok, i][:, None], mu[ok, i][:, None]
                raw, skipped, _ = lr.estimator_ld(ls, ph, ms)
                assert skipped == 0 and g["khat"] == math.inf
                b = get_bounds(ls, np.zeros_like(ls), np.ones_like(ls), ms, int(ok.sum()))
                for a, r in (("elpd_psis", "elpd_loo"), ("pit_psis", "pit_loo"), ("mu_psis", "mu_loo"), ("weight_ess_psis", "weight_ess")):
                    e = abs(g[a] - raw[r][0])
                    raw_worst = max(raw_worst, e / b[r][0])
                    assert e <= b[r][0], (name, i, a, g[a], raw[r][0], b[r][0])
    print(f"device against the restatement: {worst:.3e} at {where} = {worst / bound:.4f} of the bound {bound:.2e}; "
          f"{n_smooth} of {n_series} series smooth; raw cases: worst error / bound {raw_worst:.3f}")
    assert n_series == 733 and n_smooth == 420
    assert worst <= bound, (worst, where)


def test_the_shortest_stores_against_the_restatement(hm):
    """K = 1 (the fewest draws st_psis takes: one value beside one padding column), 2, 3 and 5, n = 5 series where a tile takes
    eight: no tail is long enough to smooth, so these are the stage, the sort and the raw estimator alone.  The restatement and the
    bound of the case list."""
    bound = pr.DEVICE_FACTOR * pr.F64_DISTANCE
    kinds = ("gauss", "sprinkled", "skipped", "ties", "gpd0.5")
    for K in (1, 2, 3, 5):
        cols = [pr.make_series(kind, K, 40 + i) for i, kind in enumerate(kinds)]
        t, phi, mu = (np.ascontiguousarray(np.stack([c[k] for c in cols], axis=1)) for k in range(3))
        got = hm.psis(t, phi, mu)
        for i in range(len(kinds)):
            ref = pr.series(t[:, i], phi[:, i], mu[:, i])
            g = {k: got[k][i] for k in ALL}
            assert g["tail_len"] == 0 and g["n_draws"] == ref["n_draws"], (K, i, g)
            assert pr.distance(ref, g) <= bound, (K, i, g)


def test_companions_are_optional(hm):
    name, t, phi, mu = next(c for c in pr.case_list() if c[0] == "K100_n9")
    full = hm.psis(t, phi, mu)
    for kw, gone in ((dict(phi=None, mu=mu), "pit_psis"), (dict(phi=phi, mu=None), "mu_psis")):
        part = hm.psis(t, **kw)
        assert gone not in part and same(part, full, [k for k in ALL if k != gone])
    from spamtree_amd import psis
    one = psis.psis(t[:, 1], phi[:, 1], mu[:, 1], handle=hm)
    assert all(np.array_equal(one[k], full[k][1], equal_nan=True) for k in ALL)


def test_geometry_independence_and_repeatability(hm):
    rng = np.random.default_rng(3)
    outs = []
    for K, kind in ((100, "ties"), (1000, "gpd0.5"), (1025, "sprinkled")):
        s = pr.make_series(kind, K, 77)
        ref = None
        for n in (5, 37):
            for pos in (0, 3, n - 1):
                for others in (False, True):
                    if others:
                        t, phi, mu = (np.ascontiguousarray(np.stack([pr.make_series(pr.KINDS[j % len(pr.KINDS)], K, 500 + j)[k] for j in range(n)], axis=1))
                                      for k in range(3))
                    else:
                        t, phi, mu = np.full((K, n), np.nan), rng.random((K, n)), rng.random((K, n))
                    t[:, pos], phi[:, pos], mu[:, pos] = s
                    a, b = hm.psis(t, phi, mu), hm.psis(t, phi, mu)
                    assert same(a, b)                         # two calls on the same store
                    one = {k: a[k][pos] for k in ALL}
                    if ref is None:
                        ref = one
                        assert one["n_draws"] > 0 and (kind != "gpd0.5" or one["tail_len"] > 0)
                    assert all(np.array_equal(one[k], ref[k], equal_nan=True) for k in ALL), (K, kind, n, pos, others)
                    if not others:                            # the empty neighbours: S = 0
                        rest = np.arange(n) != pos
                        assert np.all(np.isnan(a["khat"][rest])) and np.all(a["n_draws"][rest] == 0) and np.all(a["tail_len"][rest] == 0)
        outs.append(ref)
    assert outs[1]["tail_len"] == 95


def draw_bounds(y, last, xb, tq):
    """The bounds of tests/test_gpu_rows_loo.get_bounds for one draw's terms: dl <= u (4 z^2 + 3 |log sigma| + 2 |l| + 4),
    dPhi <= 0.4 dz + 4 u with dz <= 4 u |z|; mu is one addition."""
    from spamtree_amd import loo
    l, phi, mu = loo.draw_terms(y, xb, last["cond_mean"], last["cond_var"], tq)
    with np.errstate(all="ignore"):
        sig = np.sqrt(last["cond_var"] + tq)
        z = (y - mu) / sig
        bl = U * (4 * z ** 2 + 3 * np.abs(np.log(sig)) + 2 * np.abs(l) + 4)
        bp = 0.4 * 4 * U * np.abs(z) + 4 * U
    return (l, phi, mu), (bl, bp, 2 * U * np.abs(mu))


@pytest.mark.parametrize("name", ["q1_grid", "q3_wide"])
def test_the_store(name):
    pb = CASES[name]()
    n, q, y = pb["n"], pb["q"], pb["y"]
    obs = np.isfinite(y)
    keep, skip_at = 30, 11
    rng = np.random.default_rng(5)
    ws = [rng.standard_normal(n) * (1.0 + 0.05 * s) for s in range(keep)]
    plain = hip_model(pb)              # no store reserved
    hm = hip_model(pb)
    plain.rows_loo_set()
    hm.rows_loo_set()
    hm.rows_loo_reserve(keep)
    xb, tq = hm.get_XB(), tausq_rows(pb)
    tinv = np.array(hm.tausq_inv, dtype=np.float64).reshape(-1) * np.ones(q)
    zero = np.zeros(q)
    terms = []
    for s in range(keep):
        for m in (plain, hm):
            if s == skip_at:
                assert m.lib.st_set_tausq_inv(m.h, dp(zero)) == 0
            m.set_w(ws[s])
            m.rows_loo_accumulate()
            if s == skip_at:
                assert m.lib.st_set_tausq_inv(m.h, dp(tinv)) == 0
        terms.append(draw_bounds(y, hm.rows_loo_last(), xb, tq))
    # the streaming outputs: bitwise those of the handle without a store
    a, b = plain.rows_loo_get(), hm.rows_loo_get()
    assert a["n_accumulated"] == b["n_accumulated"] == keep and a["n_skipped"] == b["n_skipped"] == int(obs.sum())
    assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in ("elpd_loo", "pit_loo", "mu_loo", "weight_ess"))
    ta, tb = plain.rows_loo_totals(raw=True), hm.rows_loo_totals(raw=True)
    assert np.array_equal(ta[0], tb[0], equal_nan=True) and np.array_equal(ta[1], tb[1])
    plain.close()
    # the stored columns against each draw's own terms
    dr = hm.rows_loo_draws(keep)
    for s in range(keep):
        (l, phi, mu), (bl, bp, bm) = terms[s]
        for k in ("t", "phi", "mu"):
            assert np.all(np.isnan(dr[k][s][~obs])), (s, k)
            assert np.all(np.isnan(dr[k][s][obs]) == (s == skip_at)), (s, k)
        if s != skip_at:
            assert np.all(np.abs(dr["t"][s][obs] + l[obs]) <= bl[obs]) and np.all(np.abs(dr["phi"][s][obs] - phi[obs]) <= bp[obs])
            assert np.all(np.abs(dr["mu"][s][obs] - mu[obs]) <= bm[obs])
    # the rows' outputs are st_psis of the read-out, bitwise; repeatable; the streaming state, the store and w are untouched
    got = hm.rows_loo_psis()
    assert same(got, hm.psis(dr["t"], dr["phi"], dr["mu"])) and same(got, hm.rows_loo_psis())
    assert np.array_equal(np.isfinite(got["elpd_psis"]), obs) and np.all(got["n_draws"][obs] == keep - 1) and np.all(got["n_draws"][~obs] == 0)
    # S = 29: a tail of 5 wherever the fit is finite
    assert np.all(np.isin(got["tail_len"][obs], (0, 5))) and (got["tail_len"][obs] == 5).mean() > 0.9
    assert np.array_equal(got["tail_len"] > 0, np.isfinite(got["khat"])) and np.all(got["khat"][obs & (got["tail_len"] == 0)] == math.inf)
    b2, dr2 = hm.rows_loo_get(), hm.rows_loo_draws(keep)
    assert all(np.array_equal(b[k], b2[k], equal_nan=True) for k in ("elpd_loo", "pit_loo", "mu_loo", "weight_ess"))
    assert all(np.array_equal(dr[k], dr2[k], equal_nan=True) for k in dr) and np.array_equal(hm.get_w(), ws[-1])
    # the totals: a fixed tree over the device's own row values
    tot, n_obs = hm.rows_loo_psis_totals(raw=True)
    tot2, n_obs2 = hm.rows_loo_psis_totals(raw=True)
    assert np.array_equal(tot, tot2, equal_nan=True) and np.array_equal(n_obs, n_obs2)
    crit = hm.rows_loo_psis_totals()
    mv = pb["mv_id"] - 1
    thr = min(1.0 - 1.0 / math.log10(keep), 0.7)
    LD = np.longdouble
    for j in range(q):
        k = (mv == j) & obs
        cnt = int(k.sum())
        e, kh = got["elpd_psis"][k], got["khat"][k]
        assert n_obs[j] == cnt and tot[0, j] == cnt
        assert abs(tot[1, j] - e.astype(LD).sum()) <= cnt * U * np.abs(e).sum()
        assert abs(tot[2, j] - (e.astype(LD) ** 2).sum()) <= (cnt + 3) * U * (e ** 2).sum()
        sq = (y[k] - got["mu_psis"][k]).astype(LD) ** 2
        assert abs(tot[3, j] - sq.sum()) <= (cnt + 3) * U * float(sq.sum())
        assert abs(tot[4, j] - got["pit_psis"][k].astype(LD).sum()) <= cnt * U * got["pit_psis"][k].sum()
        assert tot[5, j] == got["weight_ess_psis"][k].min() and tot[6, j] == kh.max()
        assert tot[7, j] == (kh > 0.7).sum() and tot[8, j] == (kh > thr).sum()
    assert crit["n"] == int(obs.sum()) and crit["max_khat"] == got["khat"][obs].max() and crit["n_khat_bad"] == int((got["khat"][obs] > 0.7).sum())
    # one more draw is refused before any launch, and nothing moved
    assert hm.lib.st_rows_loo_accumulate(hm.h) == ST_ERR_USAGE
    msg = hm.lib.st_last_error(hm.h)
    assert b"30" in msg and b"st_rows_loo_reserve" in msg
    assert same(got, hm.rows_loo_psis()) and hm.rows_loo_get()["n_accumulated"] == keep
    hm.close()


def test_refusals_leave_a_text_and_a_usable_handle():
    from spamtree_amd import _lib
    from spamtree_amd.model import SpamTreeMV
    pb = CASES["q1_grid"]()
    hm = SpamTreeMV(pb["y"], pb["X"], pb["Z"], pb["coords"], pb["mv_id"], pb["blocking"], pb["gix_block"], pb["res_is_ref"],
                    pb["parents"], pb["children"], False, pb["block_names"], pb["block_groups"], pb["indexing"], np.zeros(pb["n"]),
                    pb["beta_true"], pb["theta"], 5.0)
    lib, h, n = hm.lib, hm.h, pb["n"]
    err = lambda: lib.st_last_error(h)      # noqa: E731
    out = _lib.StPsisOut()
    assert lib.st_rows_loo_reserve(h, 30) == ST_ERR_USAGE and b"before st_rows_loo_set" in err()
    assert lib.st_rows_loo_set(h) == 0
    assert lib.st_rows_loo_reserve(h, 16385) == ST_ERR_UNSUPPORTED and b"16385" in err() and b"16384" in err()
    assert lib.st_rows_loo_reserve(h, -1) == ST_ERR_UNSUPPORTED and b"-1" in err()
    assert hm.get_loglik_comps_w(0)
    # no store reserved
    assert lib.st_rows_loo_accumulate(h) == 0
    for call in (lambda: lib.st_rows_loo_psis(h, C.byref(out)), lambda: lib.st_rows_loo_psis_totals(h, None, None),
                 lambda: lib.st_rows_loo_draws(h, None, None, None)):
        assert call() == ST_ERR_USAGE and b"no store reserved" in err()
    assert lib.st_rows_loo_reserve(h, 30) == ST_ERR_USAGE and b"after 1 accumulated" in err()     # reserve after an accumulate
    # reserved, nothing accumulated yet
    assert lib.st_rows_loo_set(h) == 0 and lib.st_rows_loo_reserve(h, 30) == 0
    assert lib.st_rows_loo_psis(h, C.byref(out)) == ST_ERR_USAGE and b"no iteration accumulated" in err()
    assert lib.st_rows_loo_psis_totals(h, None, None) == ST_ERR_USAGE and b"no iteration accumulated" in err()
    for s in range(30):
        assert lib.st_rows_loo_accumulate(h) == 0
    assert lib.st_rows_loo_accumulate(h) == ST_ERR_USAGE and b"30" in err()                        # the 31st
    assert lib.st_rows_loo_psis(h, C.byref(out)) == 0 and hm.rows_loo_get()["n_accumulated"] == 30
    assert lib.st_rows_loo_reserve(h, 0) == ST_ERR_USAGE                                          # (draws are accumulated)
    # st_psis: K outside 1 .. 16384; n = 0 writes nothing
    t = np.zeros(4)
    for K in (0, 16385):
        assert lib.st_psis(h, 1, K, dp(t), None, None, C.byref(out)) == ST_ERR_UNSUPPORTED and str(K).encode() in err()
    kh = np.full(3, 7.0)
    o2 = _lib.StPsisOut(khat=dp(kh))
    assert lib.st_psis(h, 0, 5, None, None, None, C.byref(o2)) == 0 and np.all(kh == 7.0)
    assert hm.get_loglik_w(0) == hm.get_loglik_w(0)      # still usable
    hm.close()
    # a limited tree: the rows' store is refused, st_psis works
    lim = hip_model(CASES["limited"]())
    assert lim.lib.st_rows_loo_reserve(lim.h, 30) == ST_ERR_UNSUPPORTED and b"limited_tree" in lim.lib.st_last_error(lim.h)
    assert lim.lib.st_rows_loo_psis(lim.h, C.byref(out)) == ST_ERR_UNSUPPORTED
    s = pr.make_series("gpd0.5", 100, 1)
    a = lim.psis(*[v[:, None] for v in s])
    assert a["tail_len"][0] == 20 and lim.get_loglik_w(0) == lim.get_loglik_w(0)
    lim.close()


def test_driver_equals_the_hand_stepped_calls_and_leaves_everything_else_alone():
    from spamtree_amd import fit
    pb = make_problem(side=12, q=3, seed=5, missing=0.1)
    keep = 40
    kw = dict(mcmc_keep=keep, mcmc_burn=0, mcmc_thin=1, seed=17, adapting=True, main_verbose=False, sample_predicts=False)
    res = fit.spamtree_mv_mcmc(*fit_args(pb), loo=True, psis=True, psis_draws=True, criteria=True, **kw)
    base = fit.spamtree_mv_mcmc(*fit_args(pb), loo=True, criteria=True, **kw)
    nodraws = fit.spamtree_mv_mcmc(*fit_args(pb), loo=True, psis=True, save_w=False, save_yhat=False, **kw)
    for key in ("beta_mcmc", "tausq_mcmc", "theta_mcmc", "paramsd"):
        assert np.array_equal(res[key], base[key]) and np.array_equal(nodraws[key], base[key]), key
    for key in ("w_mcmc", "yhat_mcmc"):
        assert all(np.array_equal(a, b) for a, b in zip(res[key], base[key])), key
    for key in ("lppd", "p_waic", "mean_ll", "mu_mean", "pit"):
        assert np.array_equal(res["criteria"][key], base["criteria"][key], equal_nan=True), key
    for key in ("elpd_loo", "pit_loo", "mu_loo", "weight_ess"):
        assert np.array_equal(res["criteria"]["loo"][key], base["criteria"]["loo"][key], equal_nan=True), key
    assert "psis" not in base["criteria"]["loo"]
    assert np.array_equal(res["criteria"]["loo"]["totals"]["by_outcome"]["elpd_loo"], base["criteria"]["loo"]["totals"]["by_outcome"]["elpd_loo"])
    # the hand-stepped calls
    ch = fit.Chain(pb["y"], pb["X"], pb["Z"], pb["coords"], pb["mv_id"], pb["blocking"], pb["gix_block"], pb["res_is_ref"], pb["parents"],
                   pb["children"], False, pb["block_names"], pb["block_groups"], pb["indexing"], pb["bounds"], pb["theta"], np.zeros(pb["p"]),
                   0.1, 0.02 * np.eye(pb["theta"].size), seed=17, adapting=True)
    lib = ch.lib
    assert lib.st_rows_loo_set(ch.h) == 0 and lib.st_rows_loo_reserve(ch.h, keep) == 0
    for _ in range(keep):
        ch.step(1)
        assert lib.st_rows_loo_accumulate(ch.h) == 0
    from spamtree_amd import _lib
    n, q = pb["n"], pb["q"]
    rows = {k: np.zeros(n) for k in DBL}
    rows.update({k: np.zeros(n, dtype=np.int32) for k in INT})
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))      # noqa: E731
    out = _lib.StPsisOut(*[dp(rows[k]) for k in DBL], i32(rows["tail_len"]), i32(rows["n_draws"]))
    assert lib.st_rows_loo_psis(ch.h, C.byref(out)) == 0
    tot = np.zeros((len(_lib.ST_ROWS_PSIS), q), order="F")
    assert lib.st_rows_loo_psis_totals(ch.h, dp(tot), None) == 0
    draws = {k: np.zeros((keep, n)) for k in ("t", "phi", "mu")}
    assert lib.st_rows_loo_draws(ch.h, dp(draws["t"]), dp(draws["phi"]), dp(draws["mu"])) == 0
    ch.close()
    obs = np.isfinite(pb["y"])
    for r in (res, nodraws):
        ps = r["criteria"]["loo"]["psis"]
        assert set(ps) == set(ALL) | {"totals"} | ({"t", "phi", "mu"} if r is res else set())
        assert same(ps, rows) and np.array_equal(np.isfinite(ps["elpd_psis"]), obs)
        assert np.all(np.isin(ps["tail_len"][obs], (0, 8))) and (ps["tail_len"][obs] == 8).mean() > 0.9 and np.all(ps["n_draws"][obs] == keep)
        assert np.array_equal(ps["totals"]["by_outcome"]["elpd_psis"], tot[1]) and np.array_equal(ps["totals"]["by_outcome"]["max_khat"], tot[6])
        assert ps["totals"]["n"] == int(obs.sum()) and math.isfinite(ps["totals"]["se"]) and ps["totals"]["se"] > 0
    for k in draws:
        assert np.array_equal(res["criteria"]["loo"]["psis"][k], draws[k], equal_nan=True), k
