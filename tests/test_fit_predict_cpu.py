"""CPU-only checks of prediction during the fit (stm_mcmc_points, st_points_accumulate / st_points_summary_*,
fit.spamtree_mv_mcmc(new_points=...), predict.fit_predict): the new symbols are declared, exported and bound, the
accumulation kernel is proven to run by a GPU test, and inconsistent input is refused in Python before any device call."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests.util import make_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_HIP = ["st_points_accumulate", "st_points_summary_reset", "st_points_summary_reserve", "st_points_summary_get",
           "st_points_summary_quantile"]
NEW_FIT = ["stm_points_set", "stm_mcmc_points"]


def header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_new_symbols_are_declared_bound_and_exported():
    from spamtree_amd import _lib, build
    lib = ctypes.CDLL(build.build())
    for hdr, syms in (("spamtree_hip.h", NEW_HIP), ("spamtree_fit.h", NEW_FIT)):
        txt = header(hdr)
        for s in syms:
            assert re.search(r"\b" + s + r"\s*\(", txt), (hdr, s)
            assert s in _lib.SIGNATURES, s
            assert hasattr(lib, s), s
    # the ctypes binding has one argument per parameter of the declaration
    decl = re.search(r"int stm_mcmc_points\((.*?)\);", header("spamtree_fit.h"), re.S).group(1)
    assert len(_lib.SIGNATURES["stm_mcmc_points"][1]) == decl.count(",") + 1
    decl = re.search(r"int spamtree_mv_mcmc_c\((.*?)\);", header("spamtree_fit.h"), re.S).group(1)
    assert len(_lib.SIGNATURES["spamtree_mv_mcmc_c"][1]) == decl.count(",") + 1 == 20


def test_accumulation_kernel_is_proven_to_run_by_a_gpu_test():
    src = open(os.path.join(ROOT, "spamtree_amd", "csrc", "k_points_acc.hip")).read()
    launched = set(re.findall(r"hipLaunchKernelGGL\(\s*\(?\s*([A-Za-z_]\w*)", src))
    assert launched == {"k_points_acc"}
    gsrc = open(os.path.join(ROOT, "tests", "test_gpu_fit_predict.py")).read()
    assert "pytestmark = pytest.mark.gpu" in gsrc and "st_points_accumulate" in gsrc and "fit_predict" in gsrc


def _args(pb):
    k = pb["theta"].size
    return (pb["y"], pb["X"], pb["Z"], pb["coords"], pb["mv_id"], pb["blocking"], pb["gix_block"], pb["res_is_ref"],
            pb["parents"], pb["children"], False, pb["block_names"], pb["block_groups"], pb["indexing"], pb["bounds"],
            np.zeros((pb["n"], 1)), pb["theta"], np.zeros(pb["p"]), 0.1, 0.01 * np.eye(k))


def _points(pb, n=10):
    rng = np.random.default_rng(0)
    return dict(coords=rng.uniform(size=(n, 2)), mv=np.ones(n, dtype=np.int64), anchor=np.zeros(n, dtype=np.int64),
                X=rng.standard_normal((n, pb["p"])))


@pytest.mark.parametrize("bad", ["mv_len", "anchor_len", "X_rows", "X_cols", "mv_range", "coords_cols", "coords_nan",
                                 "anchor_float", "unknown_key", "quantile_hi", "quantile_lo"])
def test_inconsistent_points_raise_before_any_device_call(bad, monkeypatch):
    """ValueError in Python; the library's entry points are replaced by traps, so any device call would fail the test."""
    from spamtree_amd import _lib, fit
    pb = make_problem(side=8, q=1, seed=1)
    pts = _points(pb)
    qs = ()
    if bad == "mv_len":
        pts["mv"] = pts["mv"][:-1]
    elif bad == "anchor_len":
        pts["anchor"] = np.zeros(11, dtype=np.int64)
    elif bad == "X_rows":
        pts["X"] = pts["X"][:-1]
    elif bad == "X_cols":
        pts["X"] = pts["X"][:, :-1]
    elif bad == "mv_range":
        pts["mv"] = pts["mv"] + 1
    elif bad == "coords_cols":
        pts["coords"] = np.zeros((10, 3))
    elif bad == "coords_nan":
        pts["coords"][2, 0] = np.nan
    elif bad == "anchor_float":
        pts["anchor"] = pts["anchor"].astype(np.float64)
    elif bad == "unknown_key":
        pts["Z"] = 1
    elif bad == "quantile_hi":
        qs = (0.5, 1.01)
    elif bad == "quantile_lo":
        qs = (-0.1,)

    class Trap:
        def __getattr__(self, name):
            raise AssertionError(f"device call {name} before the input check")
    monkeypatch.setattr(_lib, "load", lambda: Trap())
    with pytest.raises(ValueError):
        fit.spamtree_mv_mcmc(*_args(pb), mcmc_keep=2, mcmc_burn=0, new_points=pts, new_quantiles=qs)


@pytest.mark.parametrize("bad", ["mv_len", "X_shape", "quantile"])
def test_fit_predict_checks_its_inputs_first(bad, monkeypatch):
    from spamtree_amd import _lib, predict
    pb = make_problem(side=8, q=1, seed=1)
    pts = np.random.default_rng(1).uniform(size=(10, 2))
    mv = np.ones(10 if bad != "mv_len" else 9, dtype=np.int64)
    Xn = np.zeros((10, pb["p"] + (bad == "X_shape")))
    qs = (1.5,) if bad == "quantile" else ()
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("device call before the input check")))
    monkeypatch.setattr(predict, "locate", lambda *a, **k: (_ for _ in ()).throw(AssertionError("locate before the input check")))
    with pytest.raises(ValueError):
        predict.fit_predict(pb, pts, mv, Xn, quantiles=qs, mcmc_keep=2)


def test_quantiles_need_points(monkeypatch):
    from spamtree_amd import _lib, fit
    pb = make_problem(side=8, q=1, seed=1)
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("device call before the input check")))
    with pytest.raises(ValueError):
        fit.spamtree_mv_mcmc(*_args(pb), mcmc_keep=2, mcmc_burn=0, new_quantiles=(0.5,))
