"""The leave-one-out criteria with the latent field integrated out, on the CPU: that the estimator of spamtree_amd/loo.py IS the
leave-one-out density (against the exact Gaussian value at fixed theta, beta, tausq, from draws of the exact posterior), the
float64 definition against the long-double reference (tests/loo_reference.py), its edge cases, the launch structures
(tests/loo_layout_check.cpp over spamtree_amd/csrc/loo_layout.cpp) and every ValueError of fit."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from spamtree_amd import loo
from tests import loo_reference as lr
from tests.test_tree_layout_cpu import write_problem
from tests.util import make_problem, problem_arrays, strip_coords

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spamtree_amd", "csrc")
TAUSQ = 0.2


def exact_case(side, q, S=4000):
    """The problem, its exact leave-one-out densities and S draws' worth of (l, Phi, mu) from the exact posterior of w."""
    pb = make_problem(side=side, q=q, seed=5)
    n = pb["n"]
    Q, rows = lr.density_precision(pb, pb["theta"])
    assert rows.size == n
    xb, tq = np.zeros(n), np.full(n, TAUSQ)
    exact = lr.exact_loo(pb, Q, rows, xb, tq)
    mean, chol = lr.posterior_w(pb, Q, rows, xb, tq)
    W = mean[None, :] + np.random.default_rng(1).standard_normal((S, n)) @ chol.T
    d = np.diag(Q)
    CM = W - (W @ Q) / d          # Q symmetric
    terms = [loo.draw_terms(pb["y"], xb, CM[s], 1.0 / d, tq) for s in range(S)]
    return pb, exact, terms, W


@pytest.fixture(scope="module")
def case_q1():
    return exact_case(12, 1)


@pytest.mark.parametrize("side,q", [(12, 1), (10, 2)])
def test_estimator_is_the_leave_one_out_density(side, q, case_q1):
    """Every row within 5 standard errors of the exact value (measured: largest ratio 3.16 at side 12, q = 1 and 3.37 at side 10,
    q = 2, smallest weight_ess 0.41 S and 0.22 S; the conditional lppd of the same rows is 76 % away from the exact total)."""
    pb, exact, terms, W = case_q1 if (side, q) == (12, 1) else exact_case(side, q)
    S = len(terms)
    state = loo.new_state(pb["n"])
    for l, phi, mu in terms:
        loo.update(state, l, phi, mu)
    rows = loo.finish(state, S)
    _, skipped, se = lr.estimator_ld(*[np.array([t[k] for t in terms]) for k in range(3)])
    assert skipped == 0
    ratio = np.abs(rows["elpd_loo"] - exact) / se
    print(f"side {side} q {q}: largest ratio {ratio.max():.2f}, total {rows['elpd_loo'].sum():.2f} exact {exact.sum():.2f}, "
          f"min weight_ess / S {rows['weight_ess'].min() / S:.3f}")
    assert np.all(ratio <= 5.0), ratio.max()
    assert rows["weight_ess"].min() > 0.17 * S
    if q == 1:
        # the criteria conditional on w are a different quantity: far from the exact total
        lc = np.array([-0.5 * (pb["y"] - w) ** 2 / TAUSQ - 0.5 * np.log(TAUSQ) + loo.HL2PI for w in W])
        lppd = (np.log(np.mean(np.exp(lc - lc.max(axis=0)), axis=0)) + lc.max(axis=0)).sum()
        assert abs(exact.sum() - (-317.3)) < 0.1 and abs(lppd - (-75.4)) < 1.5
        assert abs(rows["elpd_loo"].sum() - exact.sum()) < 0.01 * abs(exact.sum())


def test_float64_definition_matches_the_long_double_reference(case_q1):
    pb, _, terms, _ = case_q1
    terms = terms[:300]
    ls, phis, mus = (np.array([t[k] for t in terms]) for k in range(3))
    ref, _, _ = lr.estimator_ld(ls, phis, mus)
    state = loo.new_state(pb["n"])
    for l, phi, mu in terms:
        loo.update(state, l, phi, mu)
    got = loo.finish(state, len(terms))
    # 300 updates, each a handful of roundings on sums of positive terms (mu_loo: against the sum of |terms|)
    for k in ref:
        scale = np.abs(mus).max() if k == "mu_loo" else np.maximum(np.abs(ref[k]), 1.0)
        assert np.all(np.abs(got[k] - ref[k]) <= 300 * 8 * 2.0 ** -53 * scale), k
    # conditional_moments against the long-double product
    Q, rows = lr.density_precision(pb, pb["theta"])
    w = np.random.default_rng(3).standard_normal(pb["n"])
    m = lr.moments(Q, w, rows)
    d, c, cm, cv = loo.conditional_moments(Q, w)
    n = pb["n"]
    bound = (n + 2) * 2.0 ** -53 * (np.abs(Q) @ np.abs(w))
    assert np.array_equal(d, m["q_diag"]) and np.all(np.abs(c - m["qw"]) <= bound)
    assert np.all(np.abs(cm - m["cond_mean"]) <= bound / d + 4 * 2.0 ** -53 * np.abs(w)) and np.allclose(cv, m["cond_var"], rtol=1e-15)
    # the totals
    mv = pb["mv_id"] - 1
    t = loo.totals(got, pb["y"], mv, 1)
    assert t["n"][0] == n and abs(t["elpd_loo"][0] - ref["elpd_loo"].sum()) <= 1e-10 and t["looic"][0] == -2.0 * t["elpd_loo"][0]
    assert t["min_weight_ess"][0] == got["weight_ess"].min()


@pytest.mark.parametrize("S", [1, 2])
def test_one_and_two_draws(S):
    l = np.array([[-1.0, -700.0, 3.0], [-2.5, -1.0, 3.0]])[:S]
    phi = np.array([[0.2, 0.5, 0.9], [0.4, 0.1, 0.9]])[:S]
    mu = np.array([[1.0, -2.0, 0.0], [3.0, 5.0, 0.0]])[:S]
    st = loo.new_state(3)
    for s in range(S):
        loo.update(st, l[s], phi[s], mu[s])
    got = loo.finish(st, S)
    ref, _, _ = lr.estimator_ld(l, phi, mu)
    for k in ref:
        assert np.allclose(got[k], ref[k], rtol=1e-14, atol=0), k
    if S == 1:
        assert np.array_equal(got["elpd_loo"], l[0]) and np.array_equal(got["weight_ess"], np.ones(3))
        assert np.array_equal(got["pit_loo"], phi[0]) and np.array_equal(got["mu_loo"], mu[0])


def test_maximum_renewed_at_every_draw_and_never_and_a_skipped_draw():
    S = 40
    rng = np.random.default_rng(0)
    up = -np.arange(S, dtype=np.float64) * 3.0          # l falls: t = -l grows, the maximum is renewed at every draw
    down = np.arange(S, dtype=np.float64) * 3.0 - 200   # l grows: the first draw stays the maximum
    l = np.stack([up, down, rng.normal(size=S)], axis=1)
    l[7, 2] = -np.inf
    l[9, 2] = np.nan
    phi, mu = rng.uniform(size=(S, 3)), rng.normal(size=(S, 3))
    st = loo.new_state(3)
    for s in range(S):
        before = {k: v.copy() for k, v in st.items()}
        loo.update(st, l[s], phi[s], mu[s])
        if s in (7, 9):   # a skipped draw leaves the row's five values bit for bit
            assert all(st[k][2] == before[k][2] for k in ("M", "A1", "A2", "AP", "AM")) and st["NS"][2] == before["NS"][2] + 1
    assert st["M"][0] == -up[-1] and st["M"][1] == -down[0] and st["NS"].tolist() == [0, 0, 2]
    got = loo.finish(st, S)
    ref, skipped, _ = lr.estimator_ld(l, phi, mu)
    assert skipped == 2
    for k in ref:
        assert np.allclose(got[k], ref[k], rtol=1e-13, atol=0), k
    # every draw skipped: NaN, not a number made of nothing
    st = loo.new_state(1)
    loo.update(st, np.array([np.inf]), np.array([0.5]), np.array([0.0]))
    assert all(np.isnan(v[0]) for v in loo.finish(st, 1).values())


# ---- the launch structures ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def layout_check(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    exe = str(tmp_path_factory.mktemp("loo_layout_check") / "loo_layout_check")
    subprocess.run([hipcc, "--offload-host-only", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "loo_layout_check.cpp"), os.path.join(CSRC, "tree_layout.cpp"),
                    os.path.join(CSRC, "loo_layout.cpp"), "-o", exe], check=True, timeout=600)
    return exe


LAYOUT_CASES = {
    "q1_grid": (lambda: make_problem(side=20, q=1, seed=5), dict(leaf_levels=1, prediction_blocks=0)),
    "leaf_reference": (lambda: make_problem(side=20, q=1, seed=5, last_not_reference=False), dict(leaf_levels=0, prediction_blocks=0)),
    "q3_wide": (lambda: make_problem(side=12, q=3, seed=5), dict(leaf_levels=1)),
    "missing": (lambda: make_problem(side=20, q=1, seed=5, missing=0.2), dict(leaf_levels=1)),
    "strip_deep": (lambda: make_problem(coords=strip_coords(640, 4, 1)[0], mv_id=strip_coords(640, 4, 1)[1], q=1, seed=5, K=(2, 1),
                                        cell_size=16, tree_depth=7), dict(levels=8, rows=2560)),
}


def run_check(exe, tmp_path, pb, *flags):
    path = str(tmp_path / "problem.bin")
    write_problem(path, problem_arrays(pb))
    r = subprocess.run([exe, path, *flags], capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout.strip()


def report(out):
    assert out.startswith("OK "), out
    return {k: int(v) for k, v in (kv.split("=") for kv in out.split()[1:])}


@pytest.mark.parametrize("name", sorted(LAYOUT_CASES))
def test_layout_invariants(layout_check, tmp_path, name):
    make, want = LAYOUT_CASES[name]
    pb = make()
    for flags in ((), ("force-generic",)):
        rc, out = run_check(layout_check, tmp_path, pb, *flags)
        assert rc == 0, out
        rep = report(out)
        n_density = len(lr.density_blocks(pb))
        assert rep["blocks"] == n_density and rep["blocks"] + rep["prediction_blocks"] == len(pb["indexing"])
        assert rep["rows"] == sum(pb["indexing"][u].size for u in lr.density_blocks(pb)) and rep["max_children"] >= 2
        for k, v in want.items():
            assert rep[k] == v, (k, rep)
    if name == "missing":
        assert rep["prediction_blocks"] > 0      # the case is here for them


def test_layout_checks_can_fail_and_refusals(layout_check, tmp_path):
    pb = LAYOUT_CASES["q1_grid"][0]()
    rc, out = run_check(layout_check, tmp_path, pb, "overlap")
    assert rc == 1 and out.startswith("VIOLATED vectors:") and "overlaps" in out, out
    rc, out = run_check(layout_check, tmp_path, pb, "drop-child")
    assert rc == 1 and out.startswith("VIOLATED children:") and "on no list" in out, out
    rc, out = run_check(layout_check, tmp_path, pb, "world2")
    assert rc == 2 and out.startswith("REFUSED -4 ") and "multi-GPU" in out, out
    lim = make_problem(side=20, q=2, seed=5, limited_tree=True)
    rc, out = run_check(layout_check, tmp_path, lim, "limited")
    assert rc == 2 and out.startswith("REFUSED -4 ") and "limited_tree" in out, out


# ---- fit's refusals, all before any device call -----------------------------------------------------------------------------
def fit_args(pb):
    return (pb["y"], pb["X"], pb["Z"], pb["coords"], pb["mv_id"], pb["blocking"], pb["gix_block"], pb["res_is_ref"], pb["parents"],
            pb["children"], pb.get("limited_tree", False), pb["block_names"], pb["block_groups"], pb["indexing"],
            pb["bounds"], np.zeros(pb["n"]), pb["theta"], np.zeros(pb["p"]), 0.2, 0.02 * np.eye(pb["theta"].size))


def test_fit_value_errors(monkeypatch):
    from spamtree_amd import _lib, fit

    def no_device():
        raise AssertionError("the library was loaded before the refusal")
    monkeypatch.setattr(_lib, "load", no_device)
    pb = make_problem(side=8, q=1, seed=5)
    lim = make_problem(side=8, q=1, seed=5, limited_tree=True)
    kw = dict(mcmc_keep=8, mcmc_burn=0, mcmc_thin=1, loo=True)
    with pytest.raises(ValueError, match="limited_tree"):
        fit.spamtree_mv_mcmc(*fit_args(lim), **kw)
    for extra, text in ((dict(chains=2), "chains and criteria"), (dict(diagnostics=True), "diagnostics and criteria"),
                        (dict(rank_diagnostics=True), "rank_diagnostics and criteria"),
                        (dict(excursions=dict(thresholds=0.0)), "excursions and criteria"),
                        (dict(new_points=dict(coords=np.zeros((1, 2)))), "criteria and new_points")):
        with pytest.raises(ValueError, match=text):
            fit.spamtree_mv_mcmc(*fit_args(pb), **kw, **extra)
    # combined with y_holdout it keeps that argument's checks
    with pytest.raises(ValueError, match="y_holdout"):
        fit.spamtree_mv_mcmc(*fit_args(pb), **kw, y_holdout=np.zeros(3))
    # and with nothing refused the next thing it does is load the library
    with pytest.raises(AssertionError, match="before the refusal"):
        fit.spamtree_mv_mcmc(*fit_args(pb), **kw)
