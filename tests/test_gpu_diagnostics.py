"""GPU: the convergence diagnostics of the stored draws (st_summary_diagnostics, st_points_summary_diagnostics,
st_points_functionals_diagnostics, k_series_diag, stm_mcmc_diagnosed, fit.spamtree_mv_mcmc(diagnostics=True)).

The stores are filled through the real calls -- rows: st_set_w with the series' value then st_summary_accumulate, the yhat series
read back per call through st_yhat; points and functionals: st_points_accumulate and st_points_functionals_last -- and the
reference (tests/diag_reference.py, long double) is always evaluated on the very draws the device stored.

The error bound (series_bounds) is the rounding of the kernel's own addition chains (spamtree_amd/csrc/diag_kernels.hpp), to
first order and then doubled; the neglected terms are products of two of these errors, each asserted below 1e-6.  With u = 2^-53,
c = ceil(K / 64) terms per lane, D = c + 6 additions behind any one sum (a lane's chain and the six butterfly levels), A = max|x|,
Dm = max|d|, s0 = sqrt(gamma_0):
  mean        delta = |m_dev - m| <= u A + (D + 2) u Dm            (m0's own error cancels in m0 + sum(x - m0) / K)
  d_s         within delta + u |d_s|
  a_t / g0    e_a = (D + 2) u + 2 delta / s0                       (sum |d_s d_{s+t}| <= K gamma_0, sum |d_s| <= K s0)
  Gamma_k     e_G = 4 e_a + 4 u                                    (two quotients, one addition; min() is 1-Lipschitz)
  tau         e_tau = 4 P e_G + 2 P u tsum + 4 u (2 tsum + 1) + 4 u tau, P = the larger pair count of device and reference: where
              the two stop at different pairs the deciding one is within e_G of zero and so, by the monotone rule, is every
              pair one of them adds behind it (at most 2 e_G each); log10 and the floor's quotient within 4 u
  ess         e_tau / tau + u;   sd: e_a / 2 + 2 u;   mcse: e_sd + e_ess / 2 + 2 u
  rhat        the half means of d within e_m = 2 (D + 3) u Dm of each other's difference (the common shift delta cancels); an
              element d_s - mu_j within e_e = 2 (D + 4) u Dm; W within e_W = (D + 4) u + 3 e_e / sqrt(W) relative;
              Q = (m1 - m2)^2 / 2 within dQ = |m1 - m2| e_m + e_m^2 / 2 + 4 u Q;  rhat within ((dQ + Q e_W) / W) / (2 rhat^2) + 4 u.
"""
import ctypes as C
import math

import numpy as np
import pytest

from tests import diag_reference as ref
from tests.util import make_problem

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
ST_ERR_USAGE, ST_ERR_UNSUPPORTED = -1, -4
KEYS = ("ess", "mcse", "sd", "rhat")
PHIS = (-0.9, -0.5, 0.3, 0.7, 0.9, 0.99)
_PB = {}
OBSERVED = dict(max_err_over_bound=0.0, max_rel_err=0.0)


def problem(name):
    if name not in _PB:
        _PB[name] = dict(n64=lambda: make_problem(side=8, q=1, seed=71, p=2), n81=lambda: make_problem(side=9, q=1, seed=72, p=2),
                         lim=lambda: make_problem(side=8, q=1, seed=73, p=2, limited_tree=True))[name]()
    return _PB[name]


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def hip_model(pb, tausq=0.25, beta=None):
    from spamtree_amd.model import SpamTreeMV
    return SpamTreeMV(pb["y"], pb["X"], pb["Z"], pb["coords"], pb["mv_id"], pb["blocking"], pb["gix_block"], pb["res_is_ref"],
                      pb["parents"], pb["children"], bool(pb["limited_tree"]), pb["block_names"], pb["block_groups"], pb["indexing"],
                      np.zeros(pb["n"]), np.array([0.7, -1.3]) if beta is None else beta, pb["theta"], 1.0 / tausq)


def series_rows(K, n, seed, once=()):
    """[K][n]: column i carries a series of kind i mod 11 -- AR(1) with the six phis, white noise, a constant, the alternating
    series, a linear trend, noise on an offset of 1e3.  Kinds in ``once`` appear in the first eleven columns only (the long
    series: their reference walks thousands of lags), AR(1) and white noise take their later places."""
    out = np.empty((K, n))
    for i in range(n):
        kind = i % 11
        if kind in once and i >= 11:
            kind = i % 7
        if kind < 6:
            out[:, i] = ref.ar1(K, PHIS[kind], seed=seed * 1000 + i, scale=1.0 + 0.1 * i)
        elif kind == 6:
            out[:, i] = ref.ar1(K, 0.0, seed=seed * 1000 + i)
        elif kind == 7:
            out[:, i] = 0.1 * (i + 1)
        elif kind == 8:
            out[:, i] = np.where(np.arange(K) % 2 == 0, 1.0, -1.0)
        elif kind == 9:
            out[:, i] = np.arange(K, dtype=np.float64)
        else:
            out[:, i] = ref.ar1(K, 0.0, seed=seed * 1000 + i, offset=1e3)
    return out


def feed_rows(hm, draws, seed=9):
    """st_set_w(draw) + st_summary_accumulate per draw; returns the yhat series st_yhat gives for the same seed and counter (the
    yhat the store holds)."""
    ys = np.empty_like(draws)
    for d in range(draws.shape[0]):
        assert hm.lib.st_set_w(hm.h, _dp(np.ascontiguousarray(draws[d]))) == 0
        assert hm.lib.st_summary_accumulate(hm.h, seed, d) == 0
        ys[d] = hm.yhat(seed=seed, it=d)
    return ys


def series_bounds(r, K, pairs_dev):
    """Relative bounds on ess, mcse, sd, rhat of one series from its reference record (the module docstring derives them)."""
    D = -(-K // 64) + 6
    A, Dm, s0 = r["max_abs_x"], r["max_abs_d"], math.sqrt(r["gamma0"])
    delta = U * A + (D + 2) * U * Dm
    e_a = (D + 2) * U + 2 * delta / s0
    assert e_a < 1e-6
    e_G = 4 * e_a + 4 * U
    P = max(r["pairs"], pairs_dev)
    e_tau = 4 * P * e_G + 2 * P * U * r["tsum"] + 4 * U * (2 * r["tsum"] + 1) + 4 * U * r["tau"]
    e_ess = e_tau / r["tau"] + U
    e_sd = e_a / 2 + 2 * U
    b = dict(ess=2 * e_ess, sd=2 * e_sd, mcse=2 * (e_sd + e_ess / 2 + 2 * U), e_G=e_G)
    if r["W"] > 0:
        e_m, e_e = 2 * (D + 3) * U * Dm, 2 * (D + 4) * U * Dm
        e_W = (D + 4) * U + 3 * e_e / math.sqrt(r["W"])
        assert e_W < 1e-6
        Q = r["dmu"] ** 2 / 2
        dQ = r["dmu"] * e_m + e_m * e_m / 2 + 4 * U * Q
        b["rhat"] = 2 * (((dQ + Q * e_W) / r["W"]) / (2 * r["rhat"] ** 2) + 4 * U)
    return b


def check_store(got, draws, max_lag, tag):
    """Every series of draws[K][n] against the long-double reference: ess, mcse, sd, rhat on every series within series_bounds;
    lags and the truncated state wherever the reference's smallest |Gamma_k| exceeds 1e-8 (at most 1 % of the series left out)."""
    from spamtree_amd import diagnostics as dg
    K, n = draws.shape
    left_out, worst, worst_rel = 0, 0.0, 0.0
    _, k_max = ref.lag_cap(K, max_lag)
    for i in range(n):
        r = ref.reference(draws[:, i], max_lag)
        g = {k: float(got[k][i]) for k in KEYS}
        lags = int(got["lags"][i])
        if r["gamma0"] == 0.0:
            assert math.isnan(g["ess"]) and math.isnan(g["rhat"]) and g["mcse"] == 0.0 and g["sd"] == 0.0 and lags == 0, (tag, i, g)
            continue
        b = series_bounds(r, K, lags // 2)
        for k in KEYS:
            if math.isnan(r[k]):
                assert math.isnan(g[k]), (tag, i, k, g[k])
                continue
            err = abs(g[k] - r[k]) / abs(r[k])
            worst, worst_rel = max(worst, err / b[k]), max(worst_rel, err)
            assert err <= b[k], (tag, i, k, g[k], r[k], err, b[k])
        if r["min_abs_gamma"] > 1e-8:
            assert lags == r["lags"] and (lags == 2 * (k_max + 1)) == r["truncated"], (tag, i, lags, r["lags"])
        else:
            left_out += 1
        assert lags % 2 == 0 and 0 <= lags <= 2 * (k_max + 1)
    assert left_out <= 0.01 * n, (tag, left_out)
    assert np.array_equal(dg.truncated(got["lags"], K, max_lag), np.asarray(got["lags"]) == 2 * (k_max + 1))
    OBSERVED["max_err_over_bound"] = max(OBSERVED["max_err_over_bound"], worst)
    OBSERVED["max_rel_err"] = max(OBSERVED["max_rel_err"], worst_rel)
    print(f"{tag}: K = {K}, n = {n}, max_lag = {max_lag}: max err / bound {worst:.3g}, max relative err {worst_rel:.3g}, "
          f"left out of the lags comparison {left_out}")


# ---- 1. values ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [4, 5, 63, 64, 65, 129, 257])
def test_row_stores_against_the_long_double_reference(K):
    """n = 81 rows, 8 series per workgroup (81 = 1 mod 8: the last workgroup holds one), every kind of series, K below, at and
    above one and two and four terms per lane, max_lag 0, 1, 2, 7 and K; w and yhat from one staging each."""
    pb = problem("n81")
    hm = hip_model(pb)
    draws = series_rows(K, pb["n"], seed=K)
    assert hm.lib.st_summary_reserve(hm.h, K) == 0
    ys = feed_rows(hm, draws)
    for max_lag in (0, 1, 2, 7, K):
        got = hm.summary_diagnostics(max_lag)
        check_store(got["w"], draws, max_lag, "w")
        check_store(got["yhat"], ys, max_lag, "yhat")
    hm.close()


@pytest.mark.parametrize("K", [2500, 16384])
def test_row_stores_with_long_series(K):
    """K = 16384: one series per workgroup, the 128 KB tile, one wave; K = 2500: the first K at which fewer than four series (three)
    fit a workgroup.  n = 64 rows, not a multiple of three.  max_lag = K lets the alternating rows run through all of their
    (K - 2) / 2 pairs; the alternating series and the trend are carried by one row each."""
    pb = problem("n64")
    hm = hip_model(pb)
    draws = series_rows(K, pb["n"], seed=7, once=(8, 9))
    assert hm.lib.st_summary_reserve(hm.h, K) == 0
    ys = feed_rows(hm, draws)
    for max_lag in (0, K):
        got = hm.summary_diagnostics(max_lag)
        check_store(got["w"], draws, max_lag, "w")
        check_store(got["yhat"], ys, max_lag, "yhat")
    hm.close()


def points_setup(hm, pb, n_new, seed, X=True):
    from spamtree_amd.predict import locate
    rng = np.random.default_rng(seed)
    lo, hi = pb["coords"].min(axis=0), pb["coords"].max(axis=0)
    pts = lo + (hi - lo) * rng.uniform(size=(n_new, 2))
    mv = np.ones(n_new, dtype=np.int64)
    hm.set_points(pts, mv, locate(pb["topo"], pts, mv, device=0), X=rng.standard_normal((n_new, pb["p"])) if X else None)


def feed_points(hm, pb, K, seed, phi=0.9):
    """K saved iterations whose w follows an AR(1) over the iterations, row by row: (w* draws, yhat* draws, F_w draws, F_y draws),
    [K][.] each, as st_points_accumulate and st_points_functionals_last returned them."""
    rng = np.random.default_rng(seed)
    w = rng.standard_normal(pb["n"])
    ws, ys, fw, fy = [], [], [], []
    for d in range(K):
        w = phi * w + math.sqrt(1 - phi * phi) * rng.standard_normal(pb["n"])
        hm.set_w(w)
        out = hm.accumulate_points(seed=13, it=d)
        ws.append(out["w"])
        ys.append(out["yhat"])
        if hm.n_functionals:
            la = hm.functionals_last()
            fw.append(la["w"])
            fy.append(la["yhat"])
    return np.array(ws), np.array(ys), np.array(fw), np.array(fy)


@pytest.mark.parametrize("K", [5, 65])
def test_point_and_functional_stores_against_the_long_double_reference(K):
    pb = problem("n64")
    hm = hip_model(pb)
    assert hm.get_loglik_comps_w(0)
    n_new = 9
    points_setup(hm, pb, n_new, seed=5)
    hm.set_functionals([([0, 1, 2], [1.0, 2.0, -3.0]), ([4], [1.0]), (list(range(n_new)), [1.0 / n_new] * n_new)])
    assert hm.lib.st_points_summary_reserve(hm.h, K) == 0
    ws, ys, fw, fy = feed_points(hm, pb, K, seed=K)
    for max_lag in (0, 2):
        got = hm.points_diagnostics(max_lag, n_kept=K)
        check_store(got["w"], ws, max_lag, "w*")
        check_store(got["yhat"], ys, max_lag, "yhat*")
        gf = hm.functionals_diagnostics(max_lag, n_kept=K)
        check_store(gf["w"], fw, max_lag, "F_w")
        check_store(gf["yhat"], fy, max_lag, "F_y")
        assert got["w"]["truncated"].dtype == bool and gf["w"]["truncated"].shape == (3,)
    hm.close()


# ---- 2. the outputs of a series do not depend on where it is stored -------------------------------------------------------------
def test_a_series_gives_the_same_bits_wherever_it_is_stored():
    """One series -- the w* draws of point 3 of a point set -- as that point, as a functional of weight 1 on it, as row 0 of the
    n = 64 handle among other neighbours and as row 50 of the n = 81 handle: the five outputs agree bit for bit, for two lag caps."""
    K = 129
    pb = problem("n64")
    hm = hip_model(pb)
    assert hm.get_loglik_comps_w(0)
    points_setup(hm, pb, 9, seed=5)
    hm.set_functionals([([3], [1.0]), ([0, 1], [0.5, 0.5])])
    assert hm.lib.st_points_summary_reserve(hm.h, K) == 0
    ws, ys, fw, _ = feed_points(hm, pb, K, seed=3)
    x = ws[:, 3].copy()
    assert np.array_equal(fw[:, 0], x)
    outs = {}
    for max_lag in (0, 7):
        outs[max_lag] = [{k: v[3] for k, v in hm.points_diagnostics(max_lag)["w"].items()},
                         {k: v[0] for k, v in hm.functionals_diagnostics(max_lag)["w"].items()}]
    for name, row in (("n64", 0), ("n81", 50)):
        pr = problem(name)
        hr = hip_model(pr) if name != "n64" else hm
        draws = series_rows(K, pr["n"], seed=11 + row)
        draws[:, row] = x
        assert hr.lib.st_summary_reserve(hr.h, K) == 0
        feed_rows(hr, draws)
        for max_lag in (0, 7):
            outs[max_lag].append({k: v[row] for k, v in hr.summary_diagnostics(max_lag)["w"].items()})
        if hr is not hm:
            hr.close()
    hm.close()
    for max_lag, o in outs.items():
        for other in o[1:]:
            for k in KEYS + ("lags",):
                assert np.array([o[0][k]]).tobytes() == np.array([other[k]]).tobytes(), (max_lag, k, o[0][k], other[k])
        assert o[0]["ess"] > 0 and o[0]["lags"] > 0


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    from spamtree_amd.model import SpamTreeError, series_diag_buffers
    pb = problem("n64")
    hm = hip_model(pb)
    lib, h = hm.lib, hm.h
    d, s = series_diag_buffers(pb["n"])
    call = lambda f, lag, w=True, y=False: f(h, lag, C.byref(s) if w else None, C.byref(s) if y else None)   # noqa: E731
    assert call(lib.st_summary_diagnostics, 0) == ST_ERR_USAGE and b"at least 4" in lib.st_last_error(h)      # no reservation
    assert lib.st_summary_reserve(h, 8) == 0
    draws = series_rows(8, pb["n"], seed=1)
    feed_rows(hm, draws[:3])
    assert call(lib.st_summary_diagnostics, 0) == ST_ERR_USAGE and b"3 draws stored" in lib.st_last_error(h)  # three stored draws
    feed_rows(hm, draws[3:4])
    assert call(lib.st_summary_diagnostics, -1) == ST_ERR_USAGE and b"max_lag" in lib.st_last_error(h)
    assert call(lib.st_summary_diagnostics, 0) == 0                                                            # still answers
    assert call(lib.st_summary_diagnostics, 0, w=False) == 0 and lib.st_summary_diagnostics(h, 0, None, C.byref(s)) == 0
    check_store(hm.summary_diagnostics()["w"], np.vstack([draws[:3], draws[3:4]]), 0, "after the refusals")
    # points: before a point set, without a reservation, three draws, yhat without X, max_lag < 0
    assert call(lib.st_points_summary_diagnostics, 0) == ST_ERR_USAGE and b"before st_points_set" in lib.st_last_error(h)
    assert call(lib.st_points_functionals_diagnostics, 0) == ST_ERR_USAGE
    assert hm.get_loglik_comps_w(0)
    points_setup(hm, pb, 9, seed=2, X=False)
    assert call(lib.st_points_functionals_diagnostics, 0) == ST_ERR_USAGE and b"before st_points_functionals_set" in lib.st_last_error(h)
    hm.set_functionals([([0, 1], [1.0, 1.0])])
    assert call(lib.st_points_summary_diagnostics, 0) == ST_ERR_USAGE and b"at least 4" in lib.st_last_error(h)
    assert call(lib.st_points_functionals_diagnostics, 0) == ST_ERR_USAGE and b"at least 4" in lib.st_last_error(h)
    assert lib.st_points_summary_reserve(h, 6) == 0
    for it in range(3):
        hm.accumulate_points(seed=1, it=it)
    assert call(lib.st_points_summary_diagnostics, 0) == ST_ERR_USAGE and b"3 draws stored" in lib.st_last_error(h)
    assert call(lib.st_points_functionals_diagnostics, 0) == ST_ERR_USAGE and b"3 draws stored" in lib.st_last_error(h)
    hm.accumulate_points(seed=1, it=3)
    assert call(lib.st_points_summary_diagnostics, 0, y=True) == ST_ERR_USAGE and b"needs the regressors X" in lib.st_last_error(h)
    assert call(lib.st_points_functionals_diagnostics, 0, y=True) == ST_ERR_USAGE and b"needs the regressors X" in lib.st_last_error(h)
    assert call(lib.st_points_summary_diagnostics, -1) == ST_ERR_USAGE and call(lib.st_points_functionals_diagnostics, -1) == ST_ERR_USAGE
    got = hm.points_diagnostics()
    assert got["yhat"] is None and np.all(got["w"]["ess"] > 0) and np.all(hm.functionals_diagnostics()["w"]["sd"] > 0)
    # a point set of size 0: ST_OK, nothing written
    hm.set_points(np.zeros((0, 2)), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))
    d["ess"][:] = -7.0
    assert call(lib.st_points_summary_diagnostics, 0) == 0 and np.all(d["ess"] == -7.0)
    hm.close()
    # a limited_tree handle: the rows are supported, the point calls refused as their quantile siblings are
    pl = problem("lim")
    hl = hip_model(pl)
    assert hl.lib.st_summary_reserve(hl.h, 5) == 0
    dl = series_rows(5, pl["n"], seed=4)
    feed_rows(hl, dl)
    check_store(hl.summary_diagnostics()["w"], dl, 0, "limited_tree")
    with pytest.raises(SpamTreeError):
        hl._diagnostics(hl.lib.st_points_summary_diagnostics, 1, 0, False, None)
    assert hl.lib.st_points_summary_diagnostics(hl.h, 0, C.byref(s), None) == ST_ERR_UNSUPPORTED
    hl.close()


# ---- 4. the driver ----------------------------------------------------------------------------------------------------------------
def fit_args(pb):
    k = pb["theta"].size
    return (pb["y"], pb["X"], pb["Z"], pb["coords"], pb["mv_id"], pb["blocking"], pb["gix_block"], pb["res_is_ref"], pb["parents"],
            pb["children"], bool(pb["limited_tree"]), pb["block_names"], pb["block_groups"], pb["indexing"], pb["bounds"],
            np.zeros(pb["n"]), pb["theta"], np.zeros(pb["p"]), 0.1, 0.02 * np.eye(k))


KW = dict(mcmc_keep=40, mcmc_burn=5, mcmc_thin=1, seed=23, adapting=True, main_verbose=False)


def check_parts(d, draws_by_key, max_lag, tag):
    for key, draws in draws_by_key.items():
        check_store(d[key], draws, max_lag, f"{tag} {key}")
        assert d[key]["truncated"].dtype == bool


def host_chain_checks(res, max_lag):
    from spamtree_amd import diagnostics as dg
    d = res["diagnostics"]
    k, keep = res["theta_mcmc"].shape
    for j in range(k):
        want = dg.series_diagnostics(res["theta_mcmc"][j], max_lag)
        assert all(np.array([want[key]]).tobytes() == np.array([d["theta"][key][j]], dtype=np.float64).tobytes() for key in KEYS)
    p, _, q = res["beta_mcmc"].shape
    assert d["beta"]["ess"].shape == (p, q) and d["tausq"]["ess"].shape == (q,)
    assert d["beta"]["sd"][1, 0] == dg.series_diagnostics(res["beta_mcmc"][1, :, 0], max_lag)["sd"]
    assert set(d["summary"]) == {"theta", "beta", "tausq", "w", "yhat"} and d["summary"]["w"]["n"] == d["w"]["ess"].size
    assert set(d["summary"]["w"]["by_outcome"]) == {1}


def test_driver_plain_chain_and_the_lean_call():
    from spamtree_amd import fit
    pb = problem("n64")
    res = fit.spamtree_mv_mcmc(*fit_args(pb), diagnostics=True, **KW)
    base = fit.spamtree_mv_mcmc(*fit_args(pb), **KW)
    for key in ("beta_mcmc", "tausq_mcmc", "theta_mcmc", "paramsd"):
        assert np.array_equal(res[key], base[key]), key
    for key in ("w_mcmc", "yhat_mcmc"):
        assert all(np.array_equal(a, b) for a, b in zip(res[key], base[key])), key
    stack = lambda lst: np.stack([np.asarray(a).reshape(-1) for a in lst])   # noqa: E731
    check_parts(res["diagnostics"], dict(w=stack(res["w_mcmc"]), yhat=stack(res["yhat_mcmc"])), 0, "driver")
    host_chain_checks(res, 0)
    lean = fit.spamtree_mv_mcmc(*fit_args(pb), diagnostics=True, save_w=False, save_yhat=False, **KW)
    assert "w_mcmc" not in lean and "yhat_mcmc" not in lean
    for part in ("w", "yhat"):
        for key in KEYS + ("lags", "truncated"):
            assert np.array_equal(lean["diagnostics"][part][key], res["diagnostics"][part][key], equal_nan=True), (part, key)
    capped = fit.spamtree_mv_mcmc(*fit_args(pb), diagnostics=True, diagnostics_max_lag=2, **KW)
    check_parts(capped["diagnostics"], dict(w=stack(capped["w_mcmc"])), 2, "driver max_lag 2")
    host_chain_checks(capped, 2)


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
    res = fit.spamtree_mv_mcmc(*fit_args(pb), diagnostics=True, new_points=new_points, **KW)
    base = fit.spamtree_mv_mcmc(*fit_args(pb), new_points=new_points, **KW)
    for key in ("beta_mcmc", "tausq_mcmc", "theta_mcmc", "paramsd"):
        assert np.array_equal(res[key], base[key]), key
    assert all(np.array_equal(a, b) for a, b in zip(res["w_mcmc"], base["w_mcmc"]))
    for key in ("w", "yhat", "cond_mean", "cond_var", "mean", "var", "w_mean", "yhat_mean"):
        assert np.array_equal(res["new"][key], base["new"][key]), key
        assert np.array_equal(res["new"]["functionals"][key], base["new"]["functionals"][key]), key
    assert "diagnostics" not in base and "diagnostics" not in base["new"]
    stack = lambda lst: np.stack([np.asarray(a).reshape(-1) for a in lst])   # noqa: E731
    check_parts(res["diagnostics"], dict(w=stack(res["w_mcmc"]), yhat=stack(res["yhat_mcmc"])), 0, "rows")
    check_parts(res["new"]["diagnostics"], dict(w=res["new"]["w"].T, yhat=res["new"]["yhat"].T), 0, "points")
    check_parts(res["new"]["functionals"]["diagnostics"], dict(w=res["new"]["functionals"]["w"].T, yhat=res["new"]["functionals"]["yhat"].T),
                0, "functionals")
    lean = fit.spamtree_mv_mcmc(*fit_args(pb), diagnostics=True, new_points=new_points, new_draws=False, save_w=False, save_yhat=False, **KW)
    assert "w" not in lean["new"]
    for a, b in ((lean["diagnostics"], res["diagnostics"]), (lean["new"]["diagnostics"], res["new"]["diagnostics"]),
                 (lean["new"]["functionals"]["diagnostics"], res["new"]["functionals"]["diagnostics"])):
        for part in ("w", "yhat"):
            for key in KEYS + ("lags", "truncated"):
                assert np.array_equal(a[part][key], b[part][key], equal_nan=True), (part, key)


def test_driver_on_a_limited_tree():
    from spamtree_amd import fit
    pl = problem("lim")
    res = fit.spamtree_mv_mcmc(*fit_args(pl), diagnostics=True, **KW)
    base = fit.spamtree_mv_mcmc(*fit_args(pl), **KW)
    assert np.array_equal(res["theta_mcmc"], base["theta_mcmc"]) and all(np.array_equal(a, b) for a, b in zip(res["w_mcmc"], base["w_mcmc"]))
    stack = lambda lst: np.stack([np.asarray(a).reshape(-1) for a in lst])   # noqa: E731
    check_parts(res["diagnostics"], dict(w=stack(res["w_mcmc"]), yhat=stack(res["yhat_mcmc"])), 0, "limited_tree driver")


def test_zz_report_the_largest_observed_error():
    """Prints the largest error the cases above met, relative and as a fraction of its bound (DESIGN.md section 21 records it)."""
    print(f"largest observed: err / bound {OBSERVED['max_err_over_bound']:.3g}, relative err {OBSERVED['max_rel_err']:.3g}")
    assert OBSERVED["max_err_over_bound"] <= 1.0
