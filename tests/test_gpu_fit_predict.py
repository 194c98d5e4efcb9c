"""GPU: prediction at new locations during the fit (stm_mcmc_points, st_points_accumulate, predict.fit_predict).

  * what the fit predicts on each saved iteration is what predict_new gives when it replays that saved draw: conditional
    mean, conditional variance and draw bit for bit, yhat to 1e-14, the Rao-Blackwellised moments to 1e-12 -- on
    k_points_mfma<128>, k_points_mfma<256> and k_points_generic, with at least one accepted theta inside the saved window;
  * the chain is the same bit for bit with and without points;
  * the device summaries equal list_mean / list_qtile of the returned draws; a summaries-only run gives them bit for bit;
  * the moments do not depend on the order of the points; the refusals come before any iteration; one run at config #3's size.
"""
import ctypes as C

import numpy as np
import pytest

from tests.util import make_problem

pytestmark = pytest.mark.gpu

ST_ERR_USAGE, ST_ERR_UNSUPPORTED = -1, -4
QS = (0.0, 0.025, 0.3, 0.5, 0.975, 1.0)
MCMC = dict(mcmc_keep=8, mcmc_burn=6, mcmc_thin=2, adapting=True, sample_theta=True)


def relerr(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(1e-300, np.abs(b).max()))


def points_for(pb, n, seed, beyond=0.0):
    rng = np.random.default_rng(seed)
    lo, hi = pb["coords"].min(axis=0), pb["coords"].max(axis=0)
    span = hi - lo
    pts = (lo - beyond * span) + (1 + 2 * beyond) * span * rng.uniform(size=(n, 2))
    mv = rng.integers(1, pb["q"] + 1, size=n)
    Xn = rng.standard_normal((n, pb["p"]))
    return pts, mv, Xn


CASES = {
    # q = 1 grid, 10 % NA: chains of <= 128 rows
    "q1_grid": dict(pb=lambda: make_problem(side=30, q=1, seed=1, missing=0.1), n=400, seed=21, beyond=0.0, fg=False,
                    routes={"k_points_mfma<128>"}),
    # README-shaped: random-uniform coordinates, n = 625, 10 % NA, points among and beyond the data
    "readme": dict(pb=lambda: make_problem(side=25, q=1, seed=3, missing=0.1, random_coords=True), n=300, seed=22, beyond=0.25,
                   fg=False, routes=None),
    # q = 2 with missing outcomes: chains on both sides of 128 rows
    "q2": dict(pb=lambda: make_problem(side=24, q=2, seed=2, missing=0.2), n=500, seed=23, beyond=0.0, fg=False,
               routes={"k_points_mfma<128>", "k_points_mfma<256>"}),
    # q = 4 (a 21-entry theta), 24-row blocks with missing outcomes
    # (sd: the initial proposal scales.  ai1[1:] range over (-1e3, 1e3), where the default 0.01 moves them by about 5 and no
    # proposal is accepted; with these the chain accepts at iterations 0, 5, 7 and 16, two of them inside the saved window)
    "q4": dict(pb=lambda: make_problem(side=12, q=4, seed=4, missing=0.2, cell_size=6), n=300, seed=25, beyond=0.0, fg=False,
               routes=None, sd=np.diag(np.where(np.isin(np.arange(21), (1, 2, 3)), 2e-5, 1e-3))),
    "generic": dict(pb=lambda: make_problem(side=30, q=1, seed=1, missing=0.1), n=200, seed=24, beyond=0.1, fg=True,
                    routes={"k_points_generic"}),
}


def run_case(name, **extra):
    from spamtree_amd.predict import fit_predict
    c = CASES[name]
    pb = c["pb"]()
    pts, mv, Xn = points_for(pb, c["n"], c["seed"], c["beyond"])
    seed = 1000 + c["seed"]
    kw = dict(MCMC, seed=seed, force_generic=c["fg"], device=0)
    if "sd" in c:
        kw["mcmcsd"] = c["sd"]
    kw.update(extra)
    out = fit_predict(pb, pts, mv, Xn, quantiles=QS, **kw)
    return pb, pts, mv, Xn, seed, out


def distinct_columns(theta):
    return len({tuple(col) for col in np.asarray(theta).T})


@pytest.mark.parametrize("case", list(CASES))
def test_fit_time_prediction_equals_the_replay(case):
    from spamtree_amd import fit
    from spamtree_amd.predict import predict_new
    pb, pts, mv, Xn, seed, out = run_case(case)
    assert distinct_columns(out["theta_mcmc"]) >= 2, out["theta_mcmc"]    # a swapped slot 0 inside the saved window
    new = out["new"]
    if CASES[case]["routes"] is not None:
        assert set(new["route"]) == CASES[case]["routes"], new["route"]
    rep = predict_new(pb, out, pts, mv, Xn, seed=seed, device=0, force_generic=CASES[case]["fg"], return_moments=True)
    assert set(rep["route"]) == set(new["route"])
    assert np.array_equal(rep["anchor"], new["anchor"])
    keep = MCMC["mcmc_keep"]
    assert new["w"].shape == (pts.shape[0], keep)
    for s in range(keep):
        assert np.array_equal(new["cond_mean"][:, s], rep["cond_mean"][:, s]), s
        assert np.array_equal(new["cond_var"][:, s], rep["cond_var"][:, s]), s
        assert np.array_equal(new["w"][:, s], rep["w"][:, s]), s
        assert relerr(new["yhat"][:, s], rep["yhat"][:, s]) <= 1e-14, s
    assert relerr(new["mean"], rep["mean"]) <= 1e-12
    assert relerr(new["var"], rep["var"]) <= 1e-12
    assert np.all(new["var"] >= 0) and np.all(np.isfinite(new["mean"]))

    # the chain does not see the points
    plain = fit.spamtree_mv_mcmc(pb["y"], pb["X"], pb["Z"], pb["coords"], pb["mv_id"], pb["blocking"], pb["gix_block"],
                                 pb["res_is_ref"], pb["parents"], pb["children"], False, pb["block_names"], pb["block_groups"],
                                 pb["indexing"], pb["bounds"], np.zeros((pb["n"], 1)), pb["theta"], np.zeros(pb["p"]), 0.1,
                                 CASES[case].get("sd", 0.01 * np.eye(pb["theta"].size)), seed=seed, force_generic=CASES[case]["fg"], device=0, **MCMC)
    for key in ("beta_mcmc", "tausq_mcmc", "theta_mcmc", "paramsd"):
        assert np.array_equal(plain[key], out[key]), key
    for key in ("w_mcmc", "yhat_mcmc"):
        assert all(np.array_equal(a, b) for a, b in zip(plain[key], out[key])), key


@pytest.mark.parametrize("case", ["q2", "generic"])
def test_device_summaries_match_the_draws_and_a_summaries_only_run(case):
    from oracle.list_summaries import list_mean, list_qtile
    pb, pts, mv, Xn, seed, out = run_case(case)
    new = out["new"]
    keep = MCMC["mcmc_keep"]
    ws = [new["w"][:, s] for s in range(keep)]
    ys = [new["yhat"][:, s] for s in range(keep)]
    assert relerr(new["w_mean"], list_mean(ws)) <= 1e-12
    assert relerr(new["yhat_mean"], list_mean(ys)) <= 1e-12
    assert sorted(new["quantiles"]) == sorted(QS)
    for q in QS:
        wq, yq = new["quantiles"][q]
        assert relerr(wq, list_qtile(ws, q)) <= 1e-12, q
        assert relerr(yq, list_qtile(ys, q)) <= 1e-12, q
    assert np.array_equal(new["quantiles"][0.0][0], np.min(ws, axis=0))
    assert np.array_equal(new["quantiles"][1.0][0], np.max(ws, axis=0))

    _, _, _, _, _, lean = run_case(case, return_draws=False, save_w=False, save_yhat=False)
    assert "w_mcmc" not in lean and "yhat_mcmc" not in lean
    for key in ("w", "yhat", "cond_mean", "cond_var"):
        assert key not in lean["new"], key
    for key in ("mean", "var", "w_mean", "yhat_mean"):
        assert np.array_equal(lean["new"][key], new[key]), key
    for q in QS:
        assert np.array_equal(lean["new"]["quantiles"][q][0], new["quantiles"][q][0]), q
        assert np.array_equal(lean["new"]["quantiles"][q][1], new["quantiles"][q][1]), q
    assert np.array_equal(lean["theta_mcmc"], out["theta_mcmc"])


def test_moments_do_not_depend_on_the_order_of_the_points():
    """The conditional moments follow the points bitwise.  The draws index Philox streams 6 / 7 by the position in the caller's
    order (as predict_new does), so a permuted set draws a different realisation of the same predictive."""
    from spamtree_amd.predict import fit_predict
    pb, pts, mv, Xn, seed, out = run_case("q2")
    perm = np.random.default_rng(31).permutation(pts.shape[0])
    o2 = fit_predict(pb, pts[perm], mv[perm], Xn[perm], quantiles=(0.5,), **dict(MCMC, seed=seed, device=0))
    for key in ("cond_mean", "cond_var"):
        assert np.array_equal(o2["new"][key], out["new"][key][perm]), key
    for key in ("mean", "var"):
        assert np.array_equal(o2["new"][key], out["new"][key][perm]), key
    assert np.array_equal(o2["new"]["anchor"], out["new"]["anchor"][perm])
    assert np.array_equal(o2["theta_mcmc"], out["theta_mcmc"])


def _chain(pb, **kw):
    from spamtree_amd.fit import Chain
    k = pb["theta"].size
    return Chain(pb["y"], pb["X"], pb["Z"], pb["coords"], pb["mv_id"], pb["blocking"], pb["gix_block"], pb["res_is_ref"],
                 pb["parents"], pb["children"], pb.get("limited_tree", False), pb["block_names"], pb["block_groups"],
                 pb["indexing"], pb["bounds"], pb["theta"], np.zeros(pb["p"]), 0.1, 0.01 * np.eye(k), defer_comm=True, **kw)


def test_refusals_come_before_any_iteration():
    from spamtree_amd.model import SpamTreeError
    from spamtree_amd.predict import fit_predict, locate
    dp, ip = (lambda a: a.ctypes.data_as(C.POINTER(C.c_double))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_int64)))
    pb = make_problem(side=20, q=1, seed=18, missing=0.1)
    pts, mv, _ = points_for(pb, 30, 19)
    anchor = np.ascontiguousarray(locate(pb["topo"], pts, mv, device=0))
    c = np.asfortranarray(pts)
    mv = np.ascontiguousarray(mv, dtype=np.int64)
    empty = np.nonzero(np.bincount(pb["blocking"] - 1, weights=np.isfinite(pb["y"]).astype(float)) == 0)[0]
    assert empty.size
    ch = _chain(pb)
    lib = ch.lib
    for bad in (pb["block_names"].size, -1, int(empty[0])):
        a = anchor.copy(); a[3] = bad
        assert lib.stm_points_set(ch.c, 30, dp(c), ip(mv), ip(a), None, 0) == ST_ERR_USAGE, bad
    assert lib.stm_points_set(ch.c, 30, dp(c), ip(mv), ip(anchor), None, 16385) == ST_ERR_UNSUPPORTED
    assert ch.state()["iteration"] == 0
    assert lib.stm_points_set(ch.c, 30, dp(c), ip(mv), ip(anchor), None, 0) == 0
    ch.start()
    ch.step(2)
    h = ch.h
    out = np.zeros(30)
    assert lib.st_points_summary_quantile(h, 0.5, dp(out), None) == ST_ERR_USAGE            # no reservation
    assert lib.st_points_accumulate(h, 5, 0, None, None, None, None) == 0
    assert lib.st_points_summary_quantile(h, 0.5, dp(out), None) == ST_ERR_USAGE            # accumulated, still none stored
    assert lib.st_points_summary_reserve(h, 2) == 0
    assert lib.st_points_accumulate(h, 5, 1, None, None, None, None) == 0
    assert lib.st_points_summary_quantile(h, 1.5, dp(out), None) == ST_ERR_USAGE
    assert lib.st_points_summary_quantile(h, 0.5, dp(out), None) == 0 and np.all(np.isfinite(out))
    n_acc = C.c_int64()
    mean = np.zeros(30)
    assert lib.st_points_summary_get(h, dp(mean), None, None, None, C.byref(n_acc)) == 0 and n_acc.value == 2
    assert lib.st_points_summary_get(h, None, None, None, dp(out), None) == ST_ERR_USAGE     # yhat_mean without X
    # the accumulated draw is st_points_predict's draw with the same seed and counter
    got = {k: np.zeros(30) for k in ("w", "m", "v")}
    assert lib.st_points_accumulate(h, 77, 4, dp(got["w"]), dp(got["m"]), dp(got["v"]), None) == 0
    ref = {k: np.zeros(30) for k in ("w", "m", "v")}
    assert lib.st_points_predict(h, 0, None, 77, 4, dp(ref["w"]), dp(ref["m"]), dp(ref["v"]), None) == 0
    for k in got:
        assert np.array_equal(got[k], ref[k]), k
    ch.close()

    fit_kw = dict(mcmc_keep=2, mcmc_burn=0, mcmc_thin=1, device=0)
    with pytest.raises(SpamTreeError) as e:
        fit_predict(pb, pts, mv, None, quantiles=(0.5,), **dict(fit_kw, mcmc_keep=16385, save_w=False, save_yhat=False))
    assert e.value.code == ST_ERR_UNSUPPORTED
    pl = make_problem(side=20, q=1, seed=18, missing=0.1, limited_tree=True)
    cl = _chain(pl)
    al = np.ascontiguousarray(locate(pl["topo"], pts, mv, device=0))
    assert cl.lib.stm_points_set(cl.c, 30, dp(c), ip(mv), ip(al), None, 0) == ST_ERR_UNSUPPORTED
    assert b"limited_tree" in cl.lib.stm_last_error(cl.c)
    assert cl.state()["iteration"] == 0
    cl.close()
    with pytest.raises(SpamTreeError) as e:
        fit_predict(pl, pts, mv, None, **fit_kw)
    assert e.value.code == ST_ERR_UNSUPPORTED


def test_config3_size():
    """n = 1e6 (config #3's tree), 1e5 new points, keep 2: finite outputs on k_points_mfma<256>, summaries only."""
    from spamtree_amd.predict import fit_predict
    from spamtree_amd.synthetic import make_workload
    wl = make_workload(1000, device=0)
    rng = np.random.default_rng(5)
    pts = rng.uniform(size=(100_000, 2))
    mv = np.ones(100_000, dtype=np.int64)
    Xn = rng.standard_normal((100_000, wl["p"]))
    out = fit_predict(wl, pts, mv, Xn, quantiles=(0.5,), return_draws=False, mcmc_keep=2, mcmc_burn=1, mcmc_thin=1, seed=7,
                      save_w=False, save_yhat=False, device=0)
    new = out["new"]
    assert "k_points_mfma<256>" in new["route"], new["route"]
    for key in ("mean", "var", "w_mean", "yhat_mean"):
        assert new[key].shape == (100_000,) and np.all(np.isfinite(new[key])), key
    assert np.all(new["var"] >= 0)
    assert all(np.all(np.isfinite(a)) for a in new["quantiles"][0.5])
