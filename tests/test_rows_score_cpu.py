"""CPU-only: the declarations and exports of the criteria over the fit's own rows (st_rows_score_*, stm_mcmc_criteria), the Python
argument checks of y_holdout, the table-to-dict helper, and the restatement tests/rows_score_reference.py against closed forms."""
import ctypes as C
import math
import os
import re

import mpmath as mp
import numpy as np
import pytest

from tests import rows_score_reference as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ST_NEW = ("st_rows_score_set", "st_rows_score_clear", "st_rows_score_accumulate", "st_rows_score_get", "st_rows_score_totals",
          "st_rows_score_info")
STM_NEW = ("stm_rows_score_set", "stm_mcmc_criteria")


def test_the_built_library_exports_every_new_symbol_and_the_binding_lists_it():
    from spamtree_amd import _lib
    from spamtree_amd.build import LIB
    assert os.path.exists(LIB), "the library is built by __graft_entry__.build()"
    lib = C.CDLL(LIB)
    for name in ST_NEW + STM_NEW:
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None, name          # AttributeError: not exported


def test_header_and_binding_declare_the_same_symbols_and_table_rows():
    from spamtree_amd import _lib
    strip = lambda t: re.sub(r"/\*.*?\*/", "", t, flags=re.S)   # noqa: E731
    hip = strip(open(os.path.join(ROOT, "include", "spamtree_hip.h")).read())
    fit_h = strip(open(os.path.join(ROOT, "include", "spamtree_fit.h")).read())
    for name in ST_NEW + STM_NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hip if name.startswith("st_") else fit_h)
        assert m, name
        assert len(_lib.SIGNATURES[name][1]) == len(m.group(1).split(",")), name       # one ctypes argument per parameter
    assert _lib.SIGNATURES["stm_mcmc_criteria"][1][:-1] == _lib.SIGNATURES["spamtree_mv_mcmc_c"][1]
    fields = re.search(r"typedef struct stm_criteria \{(.*?)\} stm_criteria;", fit_h, flags=re.S).group(1)
    names = re.findall(r"[\*\s](\w+)\s*[,;]", fields)
    assert names == [f[0] for f in _lib.StmCriteria._fields_]
    # the rows of the two tables, in the header's order
    for prefix, keys in (("ST_ROWS_OBS_", _lib.ST_ROWS_OBS), ("ST_ROWS_HELD_", _lib.ST_ROWS_HELD)):
        macros = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define " + prefix + r"(\w+) (\d+)", hip)}
        assert macros.pop("N") == len(keys)
        assert sorted(macros, key=macros.get) == [k.upper() for k in keys] and sorted(macros.values()) == list(range(len(keys)))


def test_y_holdout_is_checked_before_any_device_call():
    from spamtree_amd import fit
    from spamtree_amd.model import rows_holdout
    y = np.array([1.0, np.nan, 2.0, np.nan])
    assert rows_holdout(None, y) is None
    ok = rows_holdout([np.nan, 0.5, np.nan, np.nan], y)
    assert ok.dtype == np.float64 and ok[1] == 0.5 and np.isnan(ok[[0, 2, 3]]).all()
    assert rows_holdout(np.full((4, 1), np.nan), y).shape == (4,)
    with pytest.raises(ValueError, match=r"y_holdout\[2\] is finite at an observed row"):
        rows_holdout([np.nan, 0.5, 0.0, np.nan], y)
    with pytest.raises(ValueError, match=r"y_holdout\[3\] is infinite"):
        rows_holdout([np.nan, 0.5, np.nan, np.inf], y)
    with pytest.raises(ValueError, match=r"y_holdout\[0\] is infinite"):      # at an observed row too: infinite comes first
        rows_holdout([-np.inf, 0.5, np.nan, np.nan], y)
    with pytest.raises(ValueError, match="one value per row of y"):
        rows_holdout([0.5, 0.5, 0.5], y)
    with pytest.raises(ValueError, match="one value per row of y"):
        rows_holdout(np.zeros((2, 2)), y)
    # the fit refuses before it loads the library: none of these reaches a device
    from tests.util import make_problem
    pb = make_problem(side=8, q=1, seed=1, missing=0.2)
    args = (pb["y"], pb["X"], pb["Z"], pb["coords"], pb["mv_id"], pb["blocking"], pb["gix_block"], pb["res_is_ref"], pb["parents"],
            pb["children"], False, pb["block_names"], pb["block_groups"], pb["indexing"], pb["bounds"], np.zeros(pb["n"]), pb["theta"],
            np.zeros(pb["p"]), 0.1, 0.05 * np.eye(pb["theta"].size))
    hold = np.where(np.isnan(pb["y"]), 0.25, np.nan)
    with pytest.raises(ValueError, match="at most 16384"):
        fit.spamtree_mv_mcmc(*args, mcmc_keep=16385, mcmc_burn=0, y_holdout=hold)
    with pytest.raises(ValueError, match="needs sample_predicts"):
        fit.spamtree_mv_mcmc(*args, mcmc_keep=2, mcmc_burn=0, y_holdout=hold, sample_predicts=False)
    with pytest.raises(ValueError, match="finite at an observed row"):
        fit.spamtree_mv_mcmc(*args, mcmc_keep=2, mcmc_burn=0, y_holdout=np.zeros(pb["n"]))
    with pytest.raises(ValueError, match="one per call"):
        fit.spamtree_mv_mcmc(*args, mcmc_keep=2, mcmc_burn=0, criteria=True, new_points=dict())


def test_the_driver_refuses_before_it_creates_a_chain():
    """stm_mcmc_criteria's own refusals come before stm_create, so they need no device: called through the C-ABI directly."""
    from spamtree_amd import _lib, fit
    from tests.util import make_problem
    lib = _lib.load()
    pb = make_problem(side=8, q=1, seed=1, missing=0.2)
    spb, keep, n, p, q = fit._problem(pb["y"], pb["X"], pb["coords"], pb["mv_id"], pb["res_is_ref"], pb["parents"], pb["children"],
                                      pb["block_names"], pb["block_groups"], pb["indexing"])
    k = pb["theta"].size
    dp = lambda a: a.ctypes.data_as(_lib.c_dp)   # noqa: E731
    bounds, sd = np.asfortranarray(pb["bounds"]), np.asfortranarray(0.05 * np.eye(k))
    theta, beta = np.ascontiguousarray(pb["theta"]), np.zeros(p)
    opt = _lib.StOptions(0, 1, 0, 1, 0, 0)
    hold = np.where(np.isnan(pb["y"]), 0.25, np.nan)
    out = np.zeros(n)

    def call(mcmc_keep, flags, cs):
        fl = _lib.StmFlags(*flags)
        return lib.stm_mcmc_criteria(C.byref(spb), C.byref(opt), dp(bounds), dp(theta), k, dp(beta), 0.1, dp(sd), mcmc_keep, 0, 1, 17,
                                     C.byref(fl), None, None, None, None, None, None, None, C.byref(cs))
    on = (1, 1, 1, 1, 1, 1)
    none = [None] * 11
    assert call(16385, on, _lib.StmCriteria(dp(hold), 1, *none)) == -4                    # ST_ERR_UNSUPPORTED: the CRPS's draws
    assert call(2, (1, 1, 1, 1, 1, 0), _lib.StmCriteria(dp(hold), 0, *none)) == -1        # y_holdout without sample_predicts
    assert call(2, (1, 1, 1, 1, 0, 1), _lib.StmCriteria(dp(hold), 0, *none)) == -1        # ... without sample_w
    crps_only = [None] * 5 + [dp(out)] + [None] * 5
    assert call(2, on, _lib.StmCriteria(dp(hold), 0, *crps_only)) == -1                   # crps without want_crps
    assert call(2, on, _lib.StmCriteria(None, 1, *crps_only)) == -1                       # crps without y_holdout


def test_rows_criteria_turns_the_tables_into_the_documented_dict():
    from spamtree_amd import _lib
    from spamtree_amd.model import rows_criteria
    q = 3
    obs = np.zeros((len(_lib.ST_ROWS_OBS), q), order="F")
    held = np.zeros((len(_lib.ST_ROWS_HELD), q), order="F")
    prim = dict(lppd=[-10.1, -20.3, 0.0], p_waic=[1.7, 2.9, 0.0], Dbar=[25.3, 48.1, 0.0], Dhat=[22.2, 41.7, 0.0])
    for k, v in prim.items():
        obs[_lib.ST_ROWS_OBS.index(k)] = v
    obs[2] = -2.0 * (obs[0] - obs[1]); obs[5] = obs[3] - obs[4]; obs[6] = obs[3] + obs[5]
    held[:, 1] = [-6.0, 1.5, 0.9, 12.0]
    t = rows_criteria(obs, held, [5, 9, 0], [0, 3, 0])
    o, h = t["observed"], t["held_out"]
    assert o["n"] == 14 and o["lppd"] == (-10.1 + -20.3) + 0.0 and o["Dbar"] == (25.3 + 48.1) + 0.0
    assert o["waic"] == -2.0 * (o["lppd"] - o["p_waic"]) and o["p_D"] == o["Dbar"] - o["Dhat"] and o["dic"] == o["Dbar"] + o["p_D"]
    assert set(o["by_outcome"]) == {"n", *_lib.ST_ROWS_OBS} and o["by_outcome"]["waic"].tolist() == obs[2].tolist()
    assert h["n"] == 3 and h["lppd"] == -2.0 and h["pit"] == 0.5 and h["crps"] == pytest.approx(0.3) and h["mse"] == 4.0 and h["rmse"] == 2.0
    assert set(h["by_outcome"]) == {"n", "lppd", "pit", "crps", "mse", "rmse"}
    assert np.isnan(h["by_outcome"]["lppd"][[0, 2]]).all() and h["by_outcome"]["rmse"][1] == 2.0
    none = rows_criteria(obs, np.zeros_like(held), [5, 9, 0], [0, 0, 0], have_crps=False)["held_out"]
    assert none["n"] == 0 and math.isnan(none["lppd"]) and none["crps"] is None


# ---- the reference against closed forms ----------------------------------------------------------------------------------------
def _ell(t, mu, tausq_inv):
    var = 1 / mp.mpf(tausq_inv)
    return -(mp.mpf(t) - mp.mpf(mu)) ** 2 / (2 * var) - mp.log(2 * mp.pi * var) / 2


def test_one_draw_gives_lppd_equal_to_l_and_no_penalty():
    v = rr.row_values(0.7, [0.25], [-0.5], [4.0], held=True)
    want = _ell(0.7, -0.25, 4.0)
    assert abs(v["lppd"][0] - want) <= mp.mpf(10) ** -45 and abs(v["mean_ll"][0] - want) <= mp.mpf(10) ** -45
    assert v["p_waic"] == (0, 0.0)
    assert abs(v["mu_mean"][0] - mp.mpf(-0.25)) <= mp.mpf(10) ** -45
    assert abs(v["pit"][0] - mp.ncdf((mp.mpf(0.7) + mp.mpf(0.25)) * 2)) <= mp.mpf(10) ** -45
    assert all(0 <= b < 1e-12 for _, b in v.values())                 # rounding-sized bounds


def test_identical_draws_give_no_penalty_and_lppd_equal_to_l():
    v = rr.row_values(1.5, [0.5] * 4, [0.25] * 4, [2.0] * 4, held=False)
    want = _ell(1.5, 0.75, 2.0)
    assert v["p_waic"][0] == 0 and abs(v["lppd"][0] - want) <= mp.mpf(10) ** -45 and "pit" not in v


def test_two_draws_symmetric_about_the_target():
    # mu = t -/+ a: the same l twice (p_waic 0, lppd = l), Phi(r) + Phi(-r) = 1 (pit 1/2), mu_mean = t
    t, a, ti = 0.5, 0.75, 4.0
    v = rr.row_values(t, [t - a, t + a], [0.0, 0.0], [ti, ti], held=True)
    want = _ell(t, t - a, ti)
    assert abs(v["lppd"][0] - want) <= mp.mpf(10) ** -45 and v["p_waic"][0] == 0
    assert abs(v["pit"][0] - mp.mpf(1) / 2) <= mp.mpf(10) ** -45 and abs(v["mu_mean"][0] - mp.mpf(t)) <= mp.mpf(10) ** -45
    # and two different variances: p_waic = (l1 - l2)^2 / 2, the sample variance of two values
    v = rr.row_values(t, [t, t], [0.0, 0.0], [1.0, 100.0], held=False)
    l1, l2 = _ell(t, t, 1.0), _ell(t, t, 100.0)
    assert abs(v["p_waic"][0] - (l1 - l2) ** 2 / 2) <= mp.mpf(10) ** -40
    assert abs(v["lppd"][0] - mp.log((mp.exp(l1) + mp.exp(l2)) / 2)) <= mp.mpf(10) ** -40


@pytest.mark.parametrize("ells", [[-1.25], [-3.0, -2.0, -1.0], [-0.5, -2.0, -2.0, -9.0], [-5e7, -5.0000001e7, -4.99e7]])
def test_the_streaming_log_sum_exp_equals_the_direct_one(ells):
    e = [mp.mpf(x) for x in ells]
    assert abs(rr.log_mean_exp_stream(e) - rr.log_mean_exp_direct(e)) <= mp.mpf(10) ** -40 * (1 + abs(e[0]))


def test_welford_bounds_cover_a_double_precision_run_of_the_recursion():
    # the recursion of the kernel, step for step in doubles, against the exact mean and M2 of the same values
    rng = np.random.default_rng(11)
    for S, scale, shift in ((2, 1.0, 0.0), (5, 3.0, -40.0), (33, 0.01, -5e7), (200, 50.0, 1e3)):
        x = shift + scale * rng.standard_normal(S)
        m, m2 = 0.0, 0.0
        for k, v in enumerate(x, 1):
            d = v - m
            m += d / k
            m2 = float(mp.mpf(d) * mp.mpf(v - m) + mp.mpf(m2))       # one rounding: the fused multiply-add
        em = mp.fsum(mp.mpf(float(v)) for v in x) / S
        e2 = mp.fsum((mp.mpf(float(v)) - em) ** 2 for v in x)
        sq = float(mp.fsum(mp.mpf(float(v)) ** 2 for v in x))
        assert abs(mp.mpf(m) - em) <= rr.welford_mean_bound(S, sq), (S, shift)
        assert abs(mp.mpf(m2) - e2) <= rr.welford_m2_bound(S, sq, e2, 0.0), (S, shift)


def test_the_totals_chain_counts_the_reduction_shape():
    assert rr.totals_chain(25) == 1 + 22 and rr.totals_chain(256 * 1024) == 1 + 22 and rr.totals_chain(256 * 1024 + 1) == 2 + 22
    assert rr.totals_chain(10 ** 6) == 4 + 22
    assert rr.totals_bound(64, [1.0, -2.0]) == rr.gamma(23) * 3.0
