"""GPU: the HIP kernels against outputs of the reference's OWN compiled source, with no oracle in between.

tests/golden/ref_*.npz were recorded by tests/golden/make_reference_golden.py from the reference's covariance_functions.cpp,
mh_adapt.h and list_mean.cpp (compiled unchanged, oracle/Makefile).  This file reads those fixtures only: never the reference
tree, never the library built from it (tests/test_reference_binary.py proves on the CPU that the fixtures are that library's
outputs).  Tolerances are those of the existing tests of the same quantities:
  * st_cross_covariance_ag10: 1e-14 max|ref|, as tests/test_gpu_parity.py::test_cross_covariance_ag10_export;
  * the dense-DAG density and the one-level exact GP (tests/test_gpu_reference_math.py) with the full covariance matrix K
    taken from the fixture: 1e-8 and 1e-9 relative at q >= 2; at q = 1 the reference's K carries its cancellation-form
    distance |x|^2 + |y|^2 - 2 x.y while the kernels compute sqrt(dx^2 + dy^2), so the bound is BASELINE.md's stated parity
    tolerance stated_tol(phi) = 1e-6 max(1, phi / 30), as in test_factors_and_draws_vs_reference_distance_formula;
  * device quantiles and running means: tests/test_outputs_reference.py's qtile_bound and mean_bound, as tests/test_gpu_outputs.py.
"""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

from tests import test_outputs_reference as outref
from tests.golden.make_reference_golden import from_upper
from tests.test_gpu_outputs import _dp, feed
from tests.test_gpu_outputs import hip_model as outputs_model
from tests.test_gpu_parity import hip_model
from tests.test_gpu_reference_math import stated_tol
from tests.test_oracle_identities import dense_precision
from tests.util import make_problem

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_LOADED = {}


def fixture(name):
    if name not in _LOADED:
        with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
            _LOADED[name] = {k: z[k] for k in z.files}
    return _LOADED[name]


# ---------------------------------------------------------------------------------------------------------------------
# CrossCovarianceAG10
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["q2", "q3", "q4", "q5", "q6", "q3_zeroD"])
def test_cross_covariance_ag10_against_recorded_reference(case):
    """60 x 50 points, every per-outcome parameter and Dmat entry different, five coincident points (h = 0); q3_zeroD: a zero
    Dmat entry between different outcomes, where the reference takes the same-variable branch with the row's ai1^2, ai2^2."""
    from spamtree_amd.covariance import CrossCovarianceAG10
    f = fixture("ref_crosscov")
    assert case in list(f["cases"])
    g = {k: f[f"{case}_{k}"] for k in ("coords1", "mv1", "coords2", "mv2", "ai1", "ai2", "phi_i", "thetamv", "Dmat", "out")}
    ref = g["out"]
    h0 = np.all(g["coords1"][:, None, :] == g["coords2"][None, :, :], axis=2)
    assert ref.shape == (60, 50) and h0.sum() == 5
    if case == "q3_zeroD":
        assert g["Dmat"][2, 0] == 0.0 and np.any((g["mv1"][:, None] == 1) & (g["mv2"][None, :] == 3))
    got = CrossCovarianceAG10(g["coords1"], g["mv1"], g["coords2"], g["mv2"], g["ai1"], g["ai2"], g["phi_i"], g["thetamv"], g["Dmat"])
    err = np.abs(got - ref)
    print(f"{case}: max |got - ref| / max|ref| = {err.max() / np.abs(ref).max():.3g}, at h = 0: {err[h0].max() / np.abs(ref).max():.3g}")
    assert err.max() <= 1e-14 * np.abs(ref).max()


def test_cross_covariance_ag10_rd_example_against_recorded_reference():
    """The man-page inputs of tests/test_gpu_parity.py::test_cross_covariance_ag10_export (q = 2, 200 x 200, symmetric)."""
    from spamtree_amd.covariance import CrossCovarianceAG10
    f = fixture("ref_crosscov_rd")
    ref = from_upper(f["out_upper"], 200)
    got = CrossCovarianceAG10(f["cx"], f["mv"], f["cx"], f["mv"], f["ai1"], f["ai2"], f["phi_i"], f["thetamv"], f["Dmat"])
    assert got.shape == (200, 200) and np.abs(got - ref).max() <= 1e-14 * np.abs(ref).max()


# ---------------------------------------------------------------------------------------------------------------------
# the kernels' covariance inside phases A and C, through dense identities on the reference's K
# ---------------------------------------------------------------------------------------------------------------------
def recorded_problem(name, theta_name):
    """The problem a ref_dense_* fixture was recorded for, rebuilt from its recorded arguments (the recorded coordinates and
    outcomes must be the rebuilt ones), its theta and the reference's full Covariancef(., same = true) matrix."""
    f = fixture("ref_dense_" + name)
    pb = make_problem(**json.loads(str(f["kw"])))
    assert np.array_equal(pb["coords"], f["coords"]) and np.array_equal(pb["mv_id"], f["mv_id"])
    assert theta_name in list(f["theta_names"])
    K = from_upper(f["K_upper_" + theta_name], pb["n"])
    return pb, f["theta_" + theta_name].copy(), K


DENSE_CASES = [("q1_grid", "nice"), ("q1_grid", "mh_start"), ("q1_random", "nice"), ("q1_random", "mh_start"), ("q2", "nice"),
               ("q3", "distinct"), ("q5", "distinct")]


@pytest.mark.parametrize("name,theta_name", DENSE_CASES)
@pytest.mark.parametrize("generic", [False, True])
def test_hip_loglik_equals_dense_dag_density_of_reference_covariance(name, theta_name, generic):
    """tests/test_gpu_reference_math.py::test_hip_loglik_equals_dense_dag_density with K from the compiled reference: three-level
    trees with blocks of at most 32 rows, on the column-group kernels and (generic) on the generic family."""
    pb, theta, K = recorded_problem(name, theta_name)
    assert np.unique(pb["block_groups"]).size == 3 and max(len(ix) for ix in pb["indexing"]) <= 32
    w = np.random.default_rng(1).standard_normal(pb["n"])
    hm = hip_model(pb, theta=theta, w=w, force_generic=generic)
    assert hm.get_loglik_comps_w(0)
    Q, logdet = dense_precision(pb, theta, K=K)
    exact = -0.5 * pb["n"] * math.log(2 * math.pi) + 0.5 * logdet - 0.5 * w @ Q @ w
    tol = stated_tol(theta[3]) if pb["q"] == 1 else 1e-8
    a, c = hm.loglik_w[0], hm.get_loglik_w(0)
    print(f"{name} {theta_name} generic={generic}: relative difference {abs(a - exact) / abs(exact):.3g} (A), "
          f"{abs(c - exact) / abs(exact):.3g} (C), bound {tol:.3g}")
    assert abs(a - exact) < tol * abs(exact)
    assert abs(c - exact) < tol * abs(exact)
    hm.close()


@pytest.mark.parametrize("name,theta_name", [("onelevel", "nice"), ("onelevel_q3", "distinct")])
def test_hip_one_level_tree_is_exact_gp_of_reference_covariance(name, theta_name):
    """tests/test_gpu_reference_math.py::test_hip_one_level_tree_is_exact_gp with the reference's K, q = 1 and q = 3."""
    pb, theta, K = recorded_problem(name, theta_name)
    assert len(pb["indexing"]) == 1
    w = np.random.default_rng(0).standard_normal(pb["n"])
    hm = hip_model(pb, theta=theta, w=w)
    assert hm.get_loglik_comps_w(0)
    exact = -0.5 * pb["n"] * math.log(2 * math.pi) - 0.5 * np.linalg.slogdet(K)[1] - 0.5 * w @ np.linalg.solve(K, w)
    tol = stated_tol(theta[3]) if pb["q"] == 1 else 1e-9
    print(f"{name}: relative difference {abs(hm.loglik_w[0] - exact) / abs(exact):.3g}, bound {tol:.3g}")
    assert abs(hm.loglik_w[0] - exact) < tol * abs(exact)
    hm.close()


# ---------------------------------------------------------------------------------------------------------------------
# posterior summaries
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep", [1, 2, 7, 40])
def test_device_quantiles_and_means_against_recorded_reference(keep):
    """st_summary_quantile and st_summary_get on the recorded draws of a 64-row column against the recorded list_qtile /
    list_mean, for every quantile in the fixture: 0, 0.025, 0.25, 0.5, 0.975, 1, one q whose r = q keep lands on an integer and
    one on a half-integer."""
    f = fixture("ref_summaries")
    assert keep in list(f["keeps"])
    draws, qs, want_q, want_m = f[f"draws_{keep}"], f[f"qs_{keep}"], f[f"qtile_{keep}"], f[f"mean_{keep}"]
    n = draws.shape[1]
    assert n == 64 and want_q.shape == (qs.size, n) and set([0.0, 0.025, 0.25, 0.5, 0.975, 1.0] + list(f[f"landing_{keep}"])) == set(qs)
    pb = make_problem(side=8, q=1, p=2, seed=51)
    assert pb["n"] == n
    hm = outputs_model(pb)
    assert hm.lib.st_summary_reserve(hm.h, keep) == 0
    feed(hm, draws)
    wq, wm = np.zeros(n), np.zeros(n)
    for i, q in enumerate(qs):
        assert hm.lib.st_summary_quantile(hm.h, float(q), _dp(wq), None) == 0
        tol = outref.qtile_bound(draws, float(q))
        bad = np.nonzero(~(np.abs(wq - want_q[i]) <= tol))[0]
        assert bad.size == 0, (q, bad[:8], wq[bad[:8]], want_q[i][bad[:8]])
    cnt = C.c_int64()
    assert hm.lib.st_summary_get(hm.h, _dp(wm), None, C.byref(cnt)) == 0 and cnt.value == keep
    assert np.all(np.abs(wm - want_m) <= outref.mean_bound(draws))
    hm.close()
