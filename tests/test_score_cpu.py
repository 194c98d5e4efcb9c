"""CPU-only: the restatement of the held-out scores (tests/score_reference.py) against direct evaluations, the Python argument
checks of y_new, and the declarations of the new symbols."""
import ctypes as C
import os
import re
from fractions import Fraction

import mpmath as mp
import numpy as np
import pytest

from tests import score_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("ells", [
    [-1.25],                                         # S = 1
    [-3.0, -2.0, -1.0, -0.5],                        # rising: the rescaling branch every time
    [-0.5, -1.0, -2.0, -3.0],                        # falling: the adding branch every time
    [-2.0, -2.0, -2.0],                              # exact ties
    [-1.0, -5.0, -1.0, 0.25, 0.25, -7.0],            # mixed
    [-800.0, -803.5, -799.25, -1200.0],              # every exp l underflows in double
    [-1e4, -5.0],                                    # a term that vanishes against the maximum
])
def test_streaming_log_mean_exp_equals_the_direct_evaluation(ells):
    e = [mp.mpf(x) for x in ells]
    got, want = sr.log_mean_exp_stream(e), sr.log_mean_exp_direct(e)
    assert mp.isfinite(got)
    assert abs(got - want) <= mp.mpf(10) ** -45 * (1 + abs(want))


def test_streaming_log_mean_exp_skips_draws_of_density_zero():
    e = [mp.mpf(-1), -mp.inf, mp.mpf(-2)]
    want = mp.log((mp.exp(-1) + mp.exp(-2)) / 3)
    assert abs(sr.log_mean_exp_stream(e) - want) <= mp.mpf(10) ** -45
    assert sr.log_mean_exp_stream([-mp.inf, -mp.inf]) == -mp.inf


def test_mixture_lpd_of_a_point_against_a_direct_50_digit_evaluation():
    rng = np.random.default_rng(3)
    S, p = 7, 3
    x = rng.standard_normal(p)
    betas = rng.standard_normal((S, p))
    cm, cv, ti = rng.standard_normal(S), rng.uniform(0.0, 2.0, S), rng.uniform(2.0, 20.0, S)
    for y in (0.3, 55.0):                            # the second: about 40 sigma out
        lpd, lb, pit, pb = sr.point_scores(y, x, betas, cm, cv, ti)
        dens, cdf = mp.mpf(0), mp.mpf(0)
        for s in range(S):
            mu = mp.fsum(mp.mpf(float(a)) * mp.mpf(float(b)) for a, b in zip(x, betas[s])) + mp.mpf(float(cm[s]))
            var = mp.mpf(float(cv[s])) + 1 / mp.mpf(float(ti[s]))
            dens += mp.exp(-(mp.mpf(y) - mu) ** 2 / (2 * var)) / mp.sqrt(2 * mp.pi * var)
            cdf += mp.ncdf((mp.mpf(y) - mu) / mp.sqrt(var))
        assert abs(lpd - mp.log(dens / S)) <= mp.mpf(10) ** -40 * (1 + abs(lpd))
        assert abs(pit - cdf / S) <= mp.mpf(10) ** -40
        assert 0 < lb < 1e-9 and 0 < pb < 1e-12      # the bounds are rounding-sized


def test_joint_draw_equals_the_density_and_a_single_member_equals_the_point():
    rng = np.random.default_rng(4)
    g, p = 4, 2
    B = rng.standard_normal((g, g))
    Sig = B @ B.T
    X, betas = rng.standard_normal((g, p)), rng.standard_normal((g, p))
    mean, y, ti = rng.standard_normal(g), rng.standard_normal(g), rng.uniform(2.0, 20.0, g)
    l, b = sr.joint_draw(y, X, betas, mean, Sig, ti)
    A = mp.matrix(Sig.tolist()) + mp.diag([1 / mp.mpf(float(t)) for t in ti])
    e = mp.matrix([mp.mpf(float(y[a])) - mp.mpf(float(mean[a])) - mp.fsum(mp.mpf(float(u)) * mp.mpf(float(v)) for u, v in zip(X[a], betas[a]))
                   for a in range(g)])
    want = -(e.T * mp.inverse(A) * e)[0] / 2 - mp.log(mp.det(A)) / 2 - g * mp.log(2 * mp.pi) / 2
    assert abs(l - want) <= mp.mpf(10) ** -40 * (1 + abs(want))
    assert 0 < b < 1e-10
    l1, _ = sr.joint_draw(y[:1], X[:1], betas[:1], mean[:1], Sig[:1, :1], ti[:1])
    lp, _, _, _ = sr.point_draw(y[0], X[0], betas[0], mean[0], Sig[0, 0], ti[0])
    assert abs(l1 - lp) <= mp.mpf(10) ** -45
    # a duplicated member: Sigma singular, finite through tau2; without tau2 the pivot is not > 0 and the density is 0
    dup = np.full((2, 2), 4.0)                       # (4.0: the extended-precision pivot 4 - 2 * 2 is exactly 0)
    ld, bd = sr.joint_draw(y[:2], X[[0, 0]], betas[[0, 0]], mean[[0, 0]], dup, ti[[0, 0]])
    assert mp.isfinite(ld) and np.isfinite(bd)
    assert sr.joint_draw(y[:2], X[[0, 0]], betas[[0, 0]], mean[[0, 0]], dup, [np.inf, np.inf])[0] == -mp.inf


@pytest.mark.parametrize("K", [1, 2, 3, 8])
def test_sorted_crps_equals_the_brute_force_form_exactly(K):
    rng = np.random.default_rng(K)
    for trial in range(6):
        x = rng.standard_normal(K) * 3 + 100.0
        if K >= 2 and trial % 2:
            x[rng.integers(K)] = x[0]               # ties among the draws
        if K == 8 and trial == 3:
            x[:] = x[0]                             # all equal
        for y in (x.min() - 1.0, x.max() + 2.0, x[K // 2], float(np.mean(x))):
            got, mean_abs = sr.crps_sorted(x, y)
            assert isinstance(got, Fraction) and got == sr.crps_brute(x, y)
            assert got >= 0 and mean_abs >= got


def test_y_new_is_checked_before_any_device_call(monkeypatch):
    from spamtree_amd import _lib, fit, model, predict
    from tests.util import make_problem

    def no_device(*a, **k):
        raise AssertionError("the library was loaded before the inputs were checked")
    monkeypatch.setattr(_lib, "load", no_device)
    y = model.score_values([1.0, np.nan, -2.0], 3)
    assert y.dtype == np.float64 and np.isnan(y[1])
    with pytest.raises(ValueError, match="one value per new point"):
        model.score_values([1.0, 2.0], 3)
    with pytest.raises(ValueError, match=r"y_new\[2\] is infinite"):
        model.score_values([1.0, np.nan, np.inf], 3)
    with pytest.raises(ValueError, match=r"y_new\[0\] is infinite"):
        model.score_values([-np.inf, np.nan, 0.0], 3)
    with pytest.raises(ValueError, match="needs X_new"):
        model.score_values([1.0, 2.0, 3.0], 3, have_X=False)
    pts = dict(coords=np.zeros((4, 2)), mv=np.ones(4, dtype=np.int64), anchor=np.zeros(4, dtype=np.int64))
    assert fit._points_inputs(dict(pts, X=np.ones((4, 2)), y=[0.0, 1.0, np.nan, 2.0]), 2, 1, ())[7].size == 4
    assert fit._points_inputs(pts, 2, 1, ())[7] is None
    with pytest.raises(ValueError, match="new_points: y_new must hold one value per new point"):
        fit._points_inputs(dict(pts, X=np.ones((4, 2)), y=np.zeros(3)), 2, 1, ())
    with pytest.raises(ValueError, match="new_points: y_new needs X_new"):
        fit._points_inputs(dict(pts, y=np.zeros(4)), 2, 1, ())
    with pytest.raises(ValueError, match="new_points: .*infinite"):
        fit._points_inputs(dict(pts, X=np.ones((4, 2)), y=[0.0, np.inf, 0.0, 0.0]), 2, 1, ())
    pb = make_problem(side=8, q=1, seed=1)
    new, mv, Xn = np.array([[0.2, 0.3], [0.6, 0.1]]), np.ones(2, dtype=np.int64), np.ones((2, pb["p"]))
    for call in (lambda **k: predict.fit_predict(pb, new, mv, mcmc_keep=1, mcmc_burn=0, **k),
                 lambda **k: predict.predict_new(pb, dict(w_mcmc=[]), new, mv, **k)):
        with pytest.raises(ValueError, match="one value per new point"):
            call(X_new=Xn, y_new=np.zeros(3))
        with pytest.raises(ValueError, match="needs X_new"):
            call(y_new=np.zeros(2))
        with pytest.raises(ValueError, match="infinite"):
            call(X_new=Xn, y_new=[0.0, -np.inf])
    # the CRPS keeps every saved draw on the device, at most 16384: refused up front, and crps=False scores without it
    assert fit._points_inputs(dict(pts, X=np.ones((4, 2)), y=np.zeros(4)), 2, 1, ())[8] is True
    assert fit._points_inputs(dict(pts, X=np.ones((4, 2)), y=np.zeros(4), crps=False), 2, 1, ())[8] is False
    assert fit._points_inputs(pts, 2, 1, ())[8] is False
    with pytest.raises(ValueError, match="new_points: crps needs y"):
        fit._points_inputs(dict(pts, crps=True), 2, 1, ())
    with pytest.raises(ValueError, match="at most 16384"):
        predict.fit_predict(pb, new, mv, X_new=Xn, y_new=np.zeros(2), mcmc_keep=16385, mcmc_burn=0)
    with pytest.raises(ValueError, match="at most 16384"):
        predict.predict_new(pb, dict(w_mcmc=[None] * 16385), new, mv, X_new=Xn, y_new=np.zeros(2))
    with pytest.raises(ValueError, match="crps=True"):
        predict.predict_new(pb, dict(w_mcmc=[]), new, mv, X_new=Xn, y_new=np.zeros(2), quantiles=(0.1, 0.9), crps=False)
    with pytest.raises(ValueError, match="z=None and mode=0"):
        predict.predict_new(pb, dict(w_mcmc=[]), new, mv, X_new=Xn, y_new=np.zeros(2), mode=1)
    with pytest.raises(ValueError, match="z=None and mode=0"):
        predict.predict_new(pb, dict(w_mcmc=[]), new, mv, X_new=Xn, y_new=np.zeros(2), z=np.zeros((2, 1)))


def test_score_totals():
    from spamtree_amd.model import score_totals
    y = np.array([1.0, np.nan, 3.0, 0.0])
    sc = dict(lpd=np.array([-1.0, np.nan, -3.0, -5.0]), pit=np.array([0.5, np.nan, 0.25, 0.75]), crps=None)
    t = score_totals(sc, y, [1, 1, 2, 2], 3, yhat_lo=np.array([0.0, 0.0, 4.0, 0.0]), yhat_hi=np.array([2.0, 1.0, 5.0, 0.0]))
    assert t["lpd"] == -3.0 and t["pit"] == 0.5 and "crps" not in t
    assert t["coverage"] == pytest.approx(2.0 / 3.0)
    assert t["by_outcome"]["lpd"][:2].tolist() == [-1.0, -4.0] and np.isnan(t["by_outcome"]["lpd"][2])
    assert t["by_outcome"]["coverage"][:2].tolist() == [1.0, 0.5]


def test_header_and_binding_declare_the_same_new_symbols():
    from spamtree_amd import _lib
    hip = open(os.path.join(ROOT, "include", "spamtree_hip.h")).read()
    fit_h = open(os.path.join(ROOT, "include", "spamtree_fit.h")).read()
    strip = lambda t: re.sub(r"/\*.*?\*/", "", t, flags=re.S)   # noqa: E731
    decl = {"st_points_score_set": strip(hip), "st_points_score_get": strip(hip), "stm_points_score_set": strip(fit_h),
            "stm_mcmc_scored": strip(fit_h)}
    for name, txt in decl.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", txt)
        assert m, name
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == len(m.group(1).split(",")), name       # one ctypes argument per parameter
    assert _lib.SIGNATURES["stm_mcmc_scored"][1][:-1] == _lib.SIGNATURES["stm_mcmc_functionals"][1]
    fields = re.search(r"typedef struct stm_scores \{(.*?)\} stm_scores;", strip(fit_h), flags=re.S).group(1)
    names = re.findall(r"\*\s*(\w+)", fields)
    assert names == [f[0] for f in _lib.StmScores._fields_]
    assert all(f[1] in (_lib.c_dp, _lib.c_ip) for f in _lib.StmScores._fields_)
    assert C.sizeof(_lib.StmScores) == 8 * len(names)
