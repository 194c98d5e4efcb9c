"""GPU: each feature family's state is its own.  The criteria over the rows (st_rows_score_*), leave-one-out with its Pareto store
(st_rows_loo_*), prior simulation (st_simulate) and the running summaries (st_summary_*) keep their state in structures of their
own that the handle points to; one handle running all four interleaved must return, bit for bit, what four handles running one
feature each return, and setting, clearing and destroying one feature's state must leave the others' alone.  No new kernel.

The problem: make_problem's 25 x 25 grid with q = 2 and every row observed (st_simulate refuses NA rows): 625 locations per
outcome, n_all = 1250 rows.
"""
import ctypes as C

import numpy as np
import pytest

from spamtree_amd.model import SpamTreeError
from tests.test_gpu_simulate import hip_model
from tests.util import make_problem

pytestmark = pytest.mark.gpu

ST_ERR_USAGE = -1
SEED, ITERS, QUANTILE = 77, 3, 0.3
FEATURES = ("rows", "loo", "sim", "summary")


def dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def start(hm, feats):
    """Everything before the sweeps, in the interleaved order; returns the simulation's outputs."""
    out = {}
    if "rows" in feats:
        hm.rows_score_set(None)
    if "loo" in feats:
        hm.rows_loo_set()
        hm.rows_loo_reserve(ITERS)
    if "summary" in feats:
        assert hm.lib.st_summary_reserve(hm.h, ITERS) == 0
    if "sim" in feats:
        out["sim2_w"], out["sim2_y"] = hm.simulate(nd=2, seed=SEED, it=5)
        out["sim3_w"], out["sim3_y"] = hm.simulate(nd=3, seed=SEED, it=5)      # the buffers grow
    return out


def sweeps(hm, feats):
    for it in range(ITERS):
        hm.deal_with_w(seed=SEED, it=it)
        if "summary" in feats:
            assert hm.lib.st_summary_accumulate(hm.h, SEED, it) == 0
        if "rows" in feats:
            hm.rows_score_accumulate()
        if "loo" in feats:
            hm.rows_loo_accumulate()


def read(hm, feats):
    out = {}
    n = hm.n_all
    if "rows" in feats:
        out.update({"rows_" + k: v for k, v in hm.rows_score_get().items() if v is not None})      # (no crps: None)
        for k, v in zip(("obs", "held", "n_obs", "n_held"), hm.rows_score_totals(raw=True)):
            out["rows_tot_" + k] = v
    if "loo" in feats:
        out.update({"loo_" + k: v for k, v in hm.rows_loo_get().items()})
        for k, v in zip(("tot", "n_obs"), hm.rows_loo_totals(raw=True)):
            out["loo_tot_" + k] = v
        out.update({"psis_" + k: v for k, v in hm.rows_loo_psis().items()})
        for k, v in zip(("tot", "n_obs"), hm.rows_loo_psis_totals(raw=True)):
            out["psis_tot_" + k] = v
    if "summary" in feats:
        wm, ym, wq, yq = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
        cnt = C.c_int64()
        assert hm.lib.st_summary_get(hm.h, dp(wm), dp(ym), C.byref(cnt)) == 0
        assert hm.lib.st_summary_quantile(hm.h, QUANTILE, dp(wq), dp(yq)) == 0
        out.update(summary_w_mean=wm, summary_yhat_mean=ym, summary_n=int(cnt.value), summary_w_q=wq, summary_yhat_q=yq)
    return out


def run(pb, feats):
    hm = hip_model(pb)
    out = start(hm, feats)
    sweeps(hm, feats)
    out.update(read(hm, feats))
    return hm, out


def same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k


@pytest.fixture(scope="module")
def runs():
    pb = make_problem(side=25, q=2, seed=5)
    assert pb["q"] == 2 and pb["n"] == 1250 and np.all(np.isfinite(pb["y"]))
    r = {"pb": pb}
    r["A"], r["all"] = run(pb, FEATURES)            # the interleaved handle stays open for the lifetime test
    for f in FEATURES:
        hm, r[f] = run(pb, (f,))
        hm.close()
    yield r
    r["A"].close()


@pytest.mark.parametrize("feature", FEATURES)
def test_interleaved_handle_equals_the_handle_with_one_feature(runs, feature):
    prefix = {"rows": "rows_", "loo": ("loo_", "psis_"), "sim": "sim", "summary": "summary_"}[feature]
    mine = {k: v for k, v in runs["all"].items() if k.startswith(prefix)}
    assert mine and len(mine) == len(runs[feature])
    same(mine, runs[feature])
    if feature == "rows":
        assert mine["rows_n_accumulated"] == ITERS
    if feature == "loo":
        assert mine["loo_n_accumulated"] == ITERS and mine["psis_n_draws"].max() <= ITERS
    if feature == "summary":
        assert mine["summary_n"] == ITERS


def test_one_features_lifetime_leaves_the_others_alone(runs):
    A, pb = runs["A"], runs["pb"]
    # a second rows_loo_set drops the draws and the Pareto store with everything else
    A.rows_loo_set()
    cnt = C.c_int64(-1)
    assert A.lib.st_rows_loo_get(A.h, None, None, None, None, C.byref(cnt), None) == ST_ERR_USAGE and cnt.value == 0
    with pytest.raises(SpamTreeError, match="no store reserved"):
        A.rows_loo_psis()
    A.rows_score_clear()
    with pytest.raises(SpamTreeError, match=" before st_rows_score_set"):
        A.rows_score_accumulate()
    # the simulation's and the summaries' state saw none of that
    w, y = A.simulate(nd=2, seed=SEED, it=5)
    assert np.array_equal(w, runs["sim"]["sim2_w"]) and np.array_equal(y, runs["sim"]["sim2_y"])
    same(read(A, ("summary",)), runs["summary"])
    A.close()                                       # the leave-one-out and simulation state still live
    F, out = run(pb, ("rows",))
    F.close()
    same(out, runs["rows"])
