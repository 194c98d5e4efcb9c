"""CPU: the definition of the exceedance, excursion and band outputs (include/spamtree_hip.h, st_*_excursions) on hand cases, the
host restatement spamtree_amd.excursions.store_excursions against the tests' reference (tests/excursion_reference.py: the excursion
function from the definition of the nested family, the band in long double), band_factor as an order statistic, and every
ValueError of the Python front doors."""
import math

import numpy as np
import pytest

from spamtree_amd import excursions as ex
from tests import excursion_reference as ref

HAND = np.array([[2.0, 2.0, 0.0], [2.0, 0.0, 2.0], [2.0, 2.0, 2.0], [2.0, 2.0, 2.0]])


def both(X, thr, side, dom=None, G=1, mask=None):
    """(host restatement, reference) of one store; the integer outputs of the two must agree exactly."""
    K, n = X.shape
    thr = np.asarray(thr, dtype=np.float64).reshape(-1, n)
    side = np.asarray(side).reshape(-1)
    got = ex.store_excursions(X, thr, side, domain=dom, G=G, mask=mask)
    d = np.zeros(n, dtype=np.int64) if dom is None else np.asarray(dom).copy()
    if mask is not None:
        d[np.asarray(mask) == 0] = -1
    want = ref.exceedance(X, thr, side, d, G)
    for key in ("count", "prob", "excur", "joint_all"):
        assert np.array_equal(got[key], want[key], equal_nan=True), key
    return got, want


def test_the_hand_case():
    got, _ = both(HAND, np.full((1, 3), 1.0), [1])
    assert got["count"].tolist() == [[4, 3, 3]] and got["count"].dtype == np.int32
    assert got["prob"].tolist() == [[1.0, 0.75, 0.75]]
    assert got["excur"].tolist() == [[1.0, 0.5, 0.5]]
    assert got["joint_all"].tolist() == [[0.5]] and got["n_draws"] == 4
    assert ex.excursion_set(got["excur"][0], 0.5).tolist() == [True, True, True]
    assert ex.excursion_set(got["excur"][0], 0.05).tolist() == [True, False, False]


def test_all_true_and_none_true_thresholds():
    X = np.random.default_rng(1).standard_normal((7, 5))
    got, _ = both(X, [np.full(5, -100.0), np.full(5, 100.0)], [1, 1])
    assert np.all(got["count"][0] == 7) and np.all(got["excur"][0] == 1.0) and got["joint_all"][0, 0] == 1.0
    # count = 0 everywhere: D(0) is the whole domain, every draw fails on it with m(d) = 0, and #{d : m(d) < 0} = 0
    assert np.all(got["count"][1] == 0) and got["joint_all"][1, 0] == 0.0
    assert np.all(got["excur"][1] == 0.0) and np.all(got["prob"][1] == 0.0)
    low, _ = both(X, [np.full(5, -100.0), np.full(5, 100.0)], [-1, -1])   # the same from below
    assert np.all(low["count"][0] == 0) and np.all(low["count"][1] == 7) and np.all(low["excur"][1] == 1.0)


def test_strictness_on_both_sides():
    X = np.array([[1.0, 3.0], [2.0, 2.0], [3.0, 1.0]])
    got, _ = both(X, [np.full(2, 2.0), np.full(2, 2.0)], [1, -1])
    assert got["count"].tolist() == [[1, 1], [1, 1]]   # the draw equal to the threshold counts on neither side


def test_mask_and_domains():
    rng = np.random.default_rng(3)
    X = rng.standard_normal((9, 8))
    dom = np.array([0, 1, 0, 1, 2, 2, 0, 1])
    mask = np.array([1, 1, 0, 1, 0, 0, 1, 1])   # empties domain 2
    got, _ = both(X, [np.zeros(8)], [1], dom=dom, G=3, mask=mask)
    assert np.isnan(got["excur"][0, [2, 4, 5]]).all() and not np.isnan(got["excur"][0, [0, 1, 3, 6, 7]]).any()
    assert got["joint_all"][0, 2] == 1.0   # an empty domain
    free, _ = both(X, [np.zeros(8)], [1], dom=dom, G=3)
    assert np.array_equal(free["count"], got["count"]) and np.array_equal(free["prob"], got["prob"])   # marginals stay


def test_nan_draws_make_the_event_false():
    X = np.array([[1.0, np.nan], [1.0, 1.0], [np.nan, 1.0]])
    for side in (1, -1):
        got, _ = both(X, [np.full(2, 0.0 if side > 0 else 2.0)], [side])
        assert got["count"].tolist() == [[2, 2]] and got["joint_all"][0, 0] == 1.0 / 3.0


@pytest.mark.parametrize("seed", range(6))
def test_excur_below_prob_and_monotone_in_count(seed):
    rng = np.random.default_rng(seed)
    K, n, G = int(rng.integers(1, 40)), int(rng.integers(1, 30)), int(rng.integers(1, 4))
    X = np.round(rng.standard_normal((K, n)) * 2) / 2   # ties with the thresholds
    dom = rng.integers(0, G, n)
    mask = rng.integers(0, 4, n) > 0
    thr = rng.choice([-0.5, 0.0, 0.5], size=(3, n))
    got, _ = both(X, thr, [1, -1, 1], dom=dom, G=G, mask=mask)
    inn = mask != 0
    assert np.all(got["excur"][:, inn] <= got["prob"][:, inn])
    for t in range(3):
        for g in range(G):
            sel = inn & (dom == g)
            order = np.argsort(got["count"][t, sel], kind="stable")
            assert np.all(np.diff(got["excur"][t, sel][order]) >= 0)
            full = got["count"][t, sel] == K
            assert np.all(got["excur"][t, sel][full] >= got["joint_all"][t, g])


@pytest.mark.parametrize("K", [2, 3, 100])
def test_band_factor_is_an_order_statistic(K):
    v = np.random.default_rng(K).permutation(np.arange(1.0, K + 1))
    assert ex.band_factor(v, 0.0) == K              # the last rank
    assert ex.band_factor(v, 1.0) == 1.0            # the first (rank 0 is lifted to 1)
    assert ex.band_factor(v, (K - 1) / K) == 1.0
    assert ex.band_factor(v, 0.5) == math.ceil(0.5 * K)
    for alpha in (0.05, 0.1, 0.32):
        r = math.ceil((1 - alpha) * K)
        assert ex.band_factor(v, alpha) == float(r) and ex.band_factor(v, alpha) in v   # never interpolated


def test_band_against_the_long_double_reference():
    rng = np.random.default_rng(5)
    K, n = 50, 12
    X = rng.standard_normal((K, n)) * (1 + np.arange(n))
    X[:, 3] = 0.7            # flat
    X[:, 4] += 1e3           # an offset
    dom = np.arange(n) % 2
    got = ex.store_excursions(X, domain=dom, G=2, want_band=True)
    r = ref.band(X, dom, 2)
    b = ref.band_bounds(X, dom, 2, r)
    ok = r["ok"]
    assert got["n_flat"].tolist() == r["n_flat"].tolist() == [0, 1] and got["sd"][3] == 0.0
    assert np.all(np.abs(got["mean"] - r["mean"].astype(np.float64)) <= b["mean"])
    assert np.all(np.abs(got["sd"][ok] / r["sd"][ok].astype(np.float64) - 1) <= b["sd"][ok])
    assert np.all(np.abs(got["maxdev"] - r["maxdev"].astype(np.float64)) <= b["maxdev"])
    lo, hi = ex.band(got["mean"], got["sd"], got["maxdev"], 0.1, dom)
    f0 = ex.band_factor(got["maxdev"][0], 0.1)
    assert np.array_equal(hi[dom == 0], got["mean"][dom == 0] + f0 * got["sd"][dom == 0]) and np.all(lo <= hi)
    inside = ((X >= lo) & (X <= hi))[:, ok & (dom == 0)].all(axis=1)
    assert np.count_nonzero(inside) >= math.ceil(0.9 * K)   # the band holds whole draws of the domain at the stated share


def test_expand_thresholds():
    thr, side = ex.expand_thresholds(0.5, 3)
    assert thr.tolist() == [[0.5, 0.5, 0.5]] and side.tolist() == [1] and side.dtype == np.int32
    thr, side = ex.expand_thresholds([0.0, [1.0, 2.0, 3.0]], 3, side=[1, -1])
    assert thr.tolist() == [[0.0, 0.0, 0.0], [1.0, 2.0, 3.0]] and side.tolist() == [1, -1]
    for bad in (dict(thresholds=[0.0] * 9, m=2), dict(thresholds=[], m=2), dict(thresholds=[[1.0, 2.0]], m=3),
                dict(thresholds=[np.nan], m=1), dict(thresholds=[np.inf], m=1), dict(thresholds=0.0, m=1, side=0),
                dict(thresholds=[0.0, 1.0], m=1, side=[1, 1, 1]), dict(thresholds=[np.zeros((2, 2))], m=4)):
        with pytest.raises(ValueError):
            ex.expand_thresholds(**bad)


def test_the_other_value_errors():
    with pytest.raises(ValueError):
        ex.check_mask(np.ones(3), 4)
    for K, band in ((0, False), (16385, False), (1, True)):
        with pytest.raises(ValueError):
            ex.check_keep(K, band)
    ex.check_keep(1, False)
    ex.check_keep(16384, True)
    with pytest.raises(ValueError):
        ex.excursion_set(np.zeros(2), 1.5)
    with pytest.raises(ValueError):
        ex.band_factor(np.zeros(0), 0.1)
    with pytest.raises(ValueError):
        ex.band(np.zeros(2), np.zeros(3), np.zeros((1, 4)), 0.1)
    with pytest.raises(ValueError):
        ex.store_excursions(np.zeros((1, 2)), want_band=True)


def test_fit_refuses_before_any_device_call():
    from spamtree_amd import fit
    from tests.util import make_problem
    args = [None] * 20
    for kw in (dict(excursions=dict(thresholds=0.0), criteria=True), dict(excursions=dict(thresholds=0.0), y_holdout=np.zeros(3)),
               dict(excursions=dict(thresholds=0.0), mcmc_keep=0), dict(excursions=dict(thresholds=0.0), mcmc_keep=16385),
               dict(excursions=dict(thresholds=0.0, band=True), mcmc_keep=1), dict(excursions=dict(thresholds=[0.0] * 9), mcmc_keep=5),
               dict(excursions=dict(thresholds=[np.nan]), mcmc_keep=5), dict(excursions=dict(thresholds=0.0, side=2), mcmc_keep=5),
               dict(excursions=dict(), mcmc_keep=5), dict(excursions=dict(thresholds=0.0, level=0.1), mcmc_keep=5)):
        with pytest.raises(ValueError):
            fit.spamtree_mv_mcmc(*args, **kw)
    # the shapes need the problem, still no device: two values for one outcome, a mask of the wrong length, point keys without points
    pb = make_problem(side=8, q=1, seed=1)
    k = pb["theta"].size
    real = (pb["y"], pb["X"], pb["Z"], pb["coords"], pb["mv_id"], pb["blocking"], pb["gix_block"], pb["res_is_ref"], pb["parents"],
            pb["children"], bool(pb["limited_tree"]), pb["block_names"], pb["block_groups"], pb["indexing"], pb["bounds"],
            np.zeros(pb["n"]), pb["theta"], np.zeros(pb["p"]), 0.1, 0.02 * np.eye(k))
    for x in (dict(thresholds=[[0.0, 1.0]]), dict(thresholds=0.0, mask=np.ones(pb["n"] + 1)), dict(thresholds=0.0, mask_new=np.ones(3))):
        with pytest.raises(ValueError):
            fit.spamtree_mv_mcmc(*real, excursions=x, mcmc_keep=5, mcmc_burn=1, main_verbose=False)


def test_driver_refuses_before_the_first_factorisation():
    """stm_mcmc_excursions returns its refusals before it creates the chain: no device is touched, so they are checked here.  Only
    the problem's q is read; every other argument may be NULL."""
    import ctypes as C
    from spamtree_amd import _lib
    from spamtree_amd.model import excursion_buffers, excursion_spec
    from tests.util import make_problem, problem_arrays, st_problem_struct
    lib = _lib.load()
    a = problem_arrays(make_problem(side=8, q=1, seed=1))
    pb = st_problem_struct(a)
    n = int(a["n_all"])

    def run(keep, thr=np.zeros((1, 1)), side=np.array([1], dtype=np.int32), band=False, want_rows=1, rows=True, new=False, n_thr=None):
        spec, alive = excursion_spec(thr, side, None, band)
        if n_thr is not None:
            spec.n_thr = n_thr
        xs = _lib.StmExcursions()
        xs.want_rows = want_rows
        xs.rows_spec = xs.new_spec = spec
        d, o = excursion_buffers(n, 0 if thr is None else 1, 1, max(keep, 1), band)
        if rows:
            xs.rows_w = o
        if new:
            xs.new_w = o
        common = (C.byref(pb), None, None, None, 4, None, 0.1, None, keep, 1, 1, 1, None, None, None, None, None, None, None, None)
        return lib.stm_mcmc_excursions(*common, 0, None, None, None, None, None, 0, None, 0, *([None] * 15), None, C.byref(xs))

    assert run(16385) == -4                                             # ST_ERR_UNSUPPORTED: the stores' limit
    for kw in (dict(keep=0), dict(keep=1, band=True), dict(keep=5, n_thr=9), dict(keep=5, n_thr=0), dict(keep=5, thr=np.array([[np.nan]])),
               dict(keep=5, thr=np.array([[np.inf]])), dict(keep=5, side=np.array([0], dtype=np.int32)), dict(keep=5, want_rows=0),
               dict(keep=5, new=True), dict(keep=5, thr=None, side=None)):
        assert run(**kw) == -1, kw                                      # ST_ERR_USAGE
