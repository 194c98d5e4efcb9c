"""GPU: the order in which the twelve summaries of the stored draws refuse -- st_summary_*, st_points_summary_* and
st_points_functionals_* x quantile, diagnostics, excursions, rank_diagnostics.  Every entry point follows one order:

  1. a null handle
  2. the store exists (a point set; functionals)
  3. the arguments that do not depend on the store: q in [0, 1], max_lag >= 0
  4. an empty store is ST_OK with nothing written (points and functionals; not the quantiles, which refuse "no draw stored")
  5. the spec and the number of stored draws
  6. yhat on a point set without X

The walk below puts two faults into one call wherever two steps can meet and asserts the code and the text of the earlier one, in
four states: no reservation, K = 3 stored draws, K = 4, and an empty point set with functionals.  After every refusal a valid call
on the same handle succeeds.  The tree is small (q = 2, 128 rows), the point set has 5 points without X and two functionals."""
import ctypes as C
import math

import numpy as np
import pytest

from tests.test_gpu_diagnostics import feed_rows, hip_model
from tests.util import make_problem

pytestmark = pytest.mark.gpu

ST_ERR_USAGE = -1
KINDS = ("quantile", "diagnostics", "excursions", "rank_diagnostics")
DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int32)


class Store:
    """One of the three places draws are kept: its four entry points, its series n, threshold values per t and domains."""

    def __init__(self, lib, prefix, n, m, G, has_yhat):
        self.name, self.n, self.m, self.G, self.has_yhat = prefix, n, m, G, has_yhat
        self.fn = {k: getattr(lib, prefix + k) for k in KINDS}


def call(h, st, kind, fault=None, w=True, y=False, K=4, fill=None):
    """The entry point ``kind`` of ``st`` with valid arguments, or with one ``fault``: "arg" (q = 1.5, max_lag = -1), "spec" (a NaN
    threshold), "nospec", "nothr" (threshold outputs without thresholds).  Returns (code, the w output buffers)."""
    from spamtree_amd import _lib
    from spamtree_amd.model import excursion_buffers, excursion_spec, rank_buffers, series_diag_buffers
    n, m = st.n, st.m
    f = st.fn[kind]
    thr = np.zeros((1, m))
    if fault == "spec":
        thr[0, 0] = math.nan
    side = np.ones(1, dtype=np.int32)
    if kind == "quantile":
        bw, by = np.full(n, -7.0), np.full(n, -7.0)
        rc = f(h, 1.5 if fault == "arg" else 0.5, bw.ctypes.data_as(DP) if w else None, by.ctypes.data_as(DP) if y else None)
        return rc, dict(q=bw)
    if kind == "diagnostics":
        (dw, sw), (dy, sy) = series_diag_buffers(n), series_diag_buffers(n)
        out = (dw, sw)
        args = (-1 if fault == "arg" else 0,)
    elif kind == "excursions":
        band = fault == "nothr"
        (dw, sw), (dy, sy) = excursion_buffers(n, 1, st.G, K, band), excursion_buffers(n, 1, st.G, K, band)
        spec, keep = excursion_spec(None if band else thr, side, None, band)
        out = (dw, sw)
        args = (None if fault == "nospec" else C.byref(spec),)
    else:
        (dw, sw), (dy, sy) = rank_buffers(n, 1, 1), rank_buffers(n, 1, 1)
        prob = np.array([0.5])
        none = fault == "nothr"
        spec = _lib.StRankSpec(-1 if fault == "arg" else 0, 1, prob.ctypes.data_as(DP), 0 if none else 1, None if none else thr.ctypes.data_as(DP),
                               None if none else side.ctypes.data_as(IP))
        out = (dw, sw)
        args = (None if fault == "nospec" else C.byref(spec),)
    if fill is not None:
        for v in dw.values():
            v[...] = fill
    rc = f(h, *args, C.byref(sw) if w else None, C.byref(sy) if y else None)
    return rc, out[0]


def test_the_twelve_entry_points_refuse_in_one_order():
    pb = make_problem(side=8, q=2, seed=75, p=2)
    hm = hip_model(pb)
    lib, h, n = hm.lib, hm.h, pb["n"]
    rows = Store(lib, "st_summary_", n, 2, 2, True)
    seen = dict(refusals=0, valid=0)

    def refused(st, kind, text, valid, **kw):
        rc, _ = call(h, st, kind, **kw)
        msg = lib.st_last_error(h)
        assert rc == ST_ERR_USAGE and text in msg, (st.name, kind, kw, rc, text, msg)
        seen["refusals"] += 1
        valid()
        seen["valid"] += 1

    def accepted(st, kind, **kw):
        rc, out = call(h, st, kind, **kw)
        assert rc == 0, (st.name, kind, kw, rc, lib.st_last_error(h))
        return out

    def get_w():
        assert hm.get_w().size == n

    # ---- state A: no reservation, no point set
    pts, fun = Store(lib, "st_points_summary_", 5, 2, 2, False), Store(lib, "st_points_functionals_", 2, 2, 1, False)
    for st in (rows, pts, fun):
        for kind in KINDS:
            assert call(None, st, kind)[0] == ST_ERR_USAGE                                   # 1. a null handle
    for st in (pts, fun):
        for kind in KINDS:
            refused(st, kind, b"before st_points_set", get_w)                               # 2. before 3: no point set, a bad argument
            refused(st, kind, b"before st_points_set", get_w, fault="arg")
    refused(rows, "quantile", b"", get_w, fault="arg")                                       # 3. before 5: a bad argument, no draw
    refused(rows, "diagnostics", b"max_lag", get_w, fault="arg")
    refused(rows, "quantile", b"no draw stored", get_w)                                     # 5. K = 0
    refused(rows, "diagnostics", b"0 draws stored, the diagnostics need at least 4", get_w)
    refused(rows, "excursions", b"no draw stored", get_w)
    refused(rows, "rank_diagnostics", b"0 draws stored, the diagnostics need at least 4", get_w)
    refused(rows, "rank_diagnostics", b"max_lag", get_w, fault="arg")                        # (the rank spec's max_lag belongs to step 5)

    # ---- state B: 5 points of both outcomes without X; functionals missing, then two of them; still no reservation
    from spamtree_amd.predict import locate
    assert hm.get_loglik_comps_w(0)
    rng = np.random.default_rng(4)
    lo, hi = pb["coords"].min(axis=0), pb["coords"].max(axis=0)
    xy = lo + (hi - lo) * rng.uniform(size=(5, 2))
    mv = np.array([1, 2, 1, 2, 1], dtype=np.int64)
    hm.set_points(xy, mv, locate(pb["topo"], xy, mv, device=0))
    for kind in KINDS:
        refused(fun, kind, b"before st_points_functionals_set", get_w)                       # 2. before 3
        refused(fun, kind, b"before st_points_functionals_set", get_w, fault="arg")
    hm.set_functionals([([0, 1], [1.0, -1.0]), ([2, 3, 4], [0.5, 0.25, 0.25])])
    for st in (pts, fun):
        refused(st, "quantile", b"q must lie in [0, 1]", get_w, fault="arg")                # 3. before 5
        refused(st, "diagnostics", b"max_lag", get_w, fault="arg")
        refused(st, "quantile", b"no draw stored", get_w)                                   # 5. K = 0
        refused(st, "quantile", b"no draw stored", get_w, y=True)                           # 5. before 6
        refused(st, "diagnostics", b"0 draws stored, the diagnostics need at least 4", get_w, y=True)
        refused(st, "excursions", b"no draw stored", get_w, y=True)
        refused(st, "rank_diagnostics", b"at least 4", get_w, y=True)

    # ---- state C: K = 3 stored draws in every store
    assert lib.st_summary_reserve(h, 8) == 0 and lib.st_points_summary_reserve(h, 8) == 0
    draws = rng.standard_normal((4, n))
    feed_rows(hm, draws[:3])
    for it in range(3):
        hm.set_w(draws[it])
        hm.accumulate_points(seed=5, it=it)
    for st in (rows, pts, fun):
        valid = lambda st=st: accepted(st, "quantile", K=3)   # noqa: E731
        valid()
        accepted(st, "excursions", K=3)                                                      # one draw is enough for them
        refused(st, "quantile", b"" if st is rows else b"q must lie in [0, 1]", valid, fault="arg")
        refused(st, "diagnostics", b"max_lag", valid, fault="arg")                          # 3. before 5
        refused(st, "diagnostics", b"3 draws stored", valid)
        refused(st, "rank_diagnostics", b"3 draws stored", valid)
        refused(st, "rank_diagnostics", b"threshold 0 is not finite", valid, fault="spec")   # (the spec before the count)
        refused(st, "excursions", b"threshold 0 is not finite", valid, fault="spec", K=3)
        if not st.has_yhat:
            refused(st, "diagnostics", b"3 draws stored", valid, y=True)                    # 5. before 6
            refused(st, "rank_diagnostics", b"3 draws stored", valid, y=True)
            refused(st, "excursions", b"threshold 0 is not finite", valid, fault="spec", y=True, K=3)
            refused(st, "quantile", b"needs the regressors X", valid, y=True)                # 6.
            refused(st, "excursions", b"needs the regressors X", valid, y=True, K=3)

    # ---- state D: K = 4
    feed_rows(hm, draws[3:4])
    hm.set_w(draws[3])
    hm.accumulate_points(seed=5, it=3)
    for st in (rows, pts, fun):
        for kind in KINDS:
            valid = lambda st=st, kind=kind: accepted(st, kind)   # noqa: E731
            valid()
            if kind in ("quantile", "diagnostics"):
                refused(st, kind, b"" if (st is rows and kind == "quantile") else b"q must lie" if kind == "quantile" else b"max_lag", valid, fault="arg")
                refused(st, kind, b"" if (st is rows and kind == "quantile") else b"q must lie" if kind == "quantile" else b"max_lag", valid,
                        fault="arg", y=True)                                                 # 3. before 6
            else:
                refused(st, kind, b"no spec", valid, fault="nospec")                        # 5.
                refused(st, kind, b"threshold 0 is not finite", valid, fault="spec")
                refused(st, kind, b"need thresholds", valid, fault="nothr")
                refused(st, kind, b"threshold 0 is not finite", valid, fault="spec", y=True)   # 5. before 6
            if kind == "rank_diagnostics":
                refused(st, kind, b"max_lag", valid, fault="arg")
            if st.has_yhat:
                accepted(st, kind, y=True)
            else:
                refused(st, kind, b"needs the regressors X", valid, y=True)                  # 6.
    sums = {k: v.copy() for k, v in accepted(rows, "rank_diagnostics").items()}              # the answers did not move either
    assert np.all(sums["ess_bulk"] > 0) and np.all((sums["prob"] >= 0) & (sums["prob"] <= 1))

    # ---- state E: an empty point set with two (empty) functionals; the rows keep their four draws
    hm.set_points(np.zeros((0, 2)), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))
    hm.set_functionals([([], []), ([], [])])
    assert lib.st_points_summary_reserve(h, 8) == 0
    hm.accumulate_points(seed=5, it=4)
    pts0, fun0 = Store(lib, "st_points_summary_", 0, 2, 2, False), Store(lib, "st_points_functionals_", 2, 2, 1, False)
    for st in (pts0, fun0):
        refused(st, "quantile", b"q must lie in [0, 1]", get_w, fault="arg")                # 3.
        refused(st, "quantile", b"no draw stored", get_w)                                   # (the quantiles have no step 4)
        refused(st, "diagnostics", b"max_lag", get_w, fault="arg")                          # 3. before 4
        for kind in KINDS[1:]:
            for kw in (dict(), dict(y=True)) + ((dict(fault="spec"), dict(fault="nospec"), dict(fault="nothr")) if kind != "diagnostics" else ()):
                out = accepted(st, kind, fill=-7, **kw)                                      # 4. before 5 and 6: ST_OK, nothing written
                assert all(np.all(v == -7) for k, v in out.items()), (st.name, kind, kw)
                seen["valid"] += 1
    for kind in KINDS:
        accepted(rows, kind, y=True)
    hm.close()
    print("refusals walked: %(refusals)d, valid calls after them: %(valid)d" % seen)
    assert seen["refusals"] > 100
