"""The leave-group-out criteria on the CPU: that the estimator of spamtree_amd/loo.py IS the leave-group-out density (against the
exact Gaussian log p(y_G | y_-G) at fixed theta, beta, tausq, from draws of the exact posterior), the float64 definition against
the long-double reference (tests/lgo_reference.py), its edge cases, the group structures (tests/lgo_layout_check.cpp over
spamtree_amd/csrc/lgo_layout.cpp) and every ValueError of the labelling helpers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from spamtree_amd import loo
from tests import lgo_reference as gr
from tests import loo_reference as lr
from tests.test_rows_loo_cpu import CSRC, LAYOUT_CASES, ROOT, TAUSQ
from tests.test_tree_layout_cpu import write_problem
from tests.util import make_problem, problem_arrays

S_EXACT = 4000


def exact_case(side, q, labels_of, S=S_EXACT, na=None):
    """The problem, its groups, their exact leave-group-out densities and the estimator's result over S draws of the exact posterior
    of w (the procedure of tests/test_rows_loo_cpu.exact_case).  na: rows whose y is set to NaN after the problem is built."""
    pb = make_problem(side=side, q=q, seed=5)
    if na is not None:
        pb["y"] = pb["y"].copy()
        pb["y"][na] = np.nan
    n = pb["n"]
    Q, rows = lr.density_precision(pb, pb["theta"])
    assert rows.size == n
    xb, tq = np.zeros(n), np.full(n, TAUSQ)
    label, members = loo.group_index(labels_of(pb), rows, np.isfinite(pb["y"]))
    exact = gr.exact_lgo(pb, Q, rows, xb, tq, members)
    mean, chol = lr.posterior_w(pb, Q, rows, xb, tq)
    W = mean[None, :] + np.random.default_rng(1).standard_normal((S, n)) @ chol.T
    batches = [loo.group_terms_batch(Q, W, m, pb["y"], xb, tq) for m in members]
    for s in (0, S - 1):                                  # the batch over the draws is the per-draw definition
        for b, m in list(zip(batches, members))[::7]:
            t = loo.group_terms(Q, W[s], m, pb["y"], xb, tq)
            assert abs(t["l"] - b["l"][s]) <= 1e-11 * max(abs(t["l"]), 1.0) and np.allclose(t["mu"], b["mu"][s], rtol=0, atol=1e-11)
            assert np.allclose(t["phi"], b["phi"][s], rtol=0, atol=1e-11) and np.array_equal(t["obs"], b["obs"])
    ls = np.stack([b["l"] for b in batches], axis=1)
    state = loo.new_group_state(members)
    for s in range(S):
        loo.update_groups(state, [dict(l=b["l"][s], phi=b["phi"][s], mu=b["mu"][s], obs=b["obs"]) for b in batches])
    res = loo.finish_groups(state, S, members, n, np.isfinite(pb["y"]))
    _, skipped, se = lr.estimator_ld(ls, np.zeros_like(ls), np.zeros_like(ls))
    assert skipped == 0
    return pb, members, exact, res, se, (Q, W, ls)


def sites(pb):
    return loo.site_groups(pb["coords"])


CASES = {"sites_q2": (10, 2, sites, True), "cells2": (12, 1, lambda pb: gr.cell_labels(pb, 2), True),
         "cells3": (12, 1, lambda pb: gr.cell_labels(pb, 3), True), "cells4": (12, 1, lambda pb: gr.cell_labels(pb, 4), True),
         "sites_q3": (10, 3, sites, False)}


@pytest.mark.parametrize("name", sorted(CASES))
def test_estimator_is_the_leave_group_out_density(name):
    """Every group within 5 standard errors of the exact log p(y_G | y_-G) (measured, largest ratio / smallest weight_ess / S:
    sites q 2: 2.65 / 0.169; 2 x 2: 2.36 / 0.580; 3 x 3: 2.02 / 0.645; 4 x 4: 1.67 / 0.414; sites q 3: 2.24 / 0.011, its heavy-tailed
    ratios are what the group k-hat is for, so its weight_ess is printed and not asserted)."""
    side, q, labels_of, ess_asserted = CASES[name]
    pb, members, exact, res, se, _ = exact_case(side, q, labels_of)
    ratio = np.abs(res["elpd_lgo"] - exact) / se
    print(f"{name}: {len(members)} groups, largest ratio {ratio.max():.2f}, total {res['elpd_lgo'].sum():.2f} exact {exact.sum():.2f}, "
          f"min weight_ess / S {res['weight_ess'].min() / S_EXACT:.3f}")
    assert np.all(ratio <= 5.0), ratio.max()
    if ess_asserted:
        assert res["weight_ess"].min() > 0.1 * S_EXACT
    if name == "cells3":
        assert len(members) == 16 and abs(exact.sum() - (-301.40)) < 0.01
        tot = loo.group_totals(res, pb["y"], pb["mv_id"] - 1, 1)
        assert tot["n_groups"] == 16 and tot["lgoic"] == -2.0 * tot["elpd_lgo"] and tot["by_outcome"]["count"][0] == pb["n"]
        assert abs(tot["elpd_lgo"] - exact.sum()) < 0.01 * abs(exact.sum())
        assert abs(tot["elpd_lgo"] - (-317.33)) > 0.02 * 317.33          # not the leave-one-out total
    if name == "cells4":
        assert max(m.size for m in members) == 16


def test_singleton_groups_reproduce_the_rows():
    S = 300
    pb, members, _, res, _, (Q, W, _) = exact_case(12, 1, lambda pb: np.arange(pb["n"]), S=S)
    n = pb["n"]
    d = np.diag(Q)
    state = loo.new_state(n)
    for s in range(S):
        cm = W[s] - (Q @ W[s]) / d
        loo.update(state, *loo.draw_terms(pb["y"], np.zeros(n), cm, 1.0 / d, np.full(n, TAUSQ)))
    rows = loo.finish(state, S)
    assert all(m.size == 1 and m[0] == i for i, m in enumerate(members))
    # the same quantity row by row; the two routes differ by a handful of roundings per update (the bound of the long-double comparison)
    for a, b in (("elpd_lgo", "elpd_loo"), ("weight_ess", "weight_ess"), ("mu_lgo", "mu_loo"), ("pit_lgo", "pit_loo")):
        scale = np.maximum(np.abs(rows[b]), 1.0) if b != "mu_loo" else np.abs(W).max()
        assert np.all(np.abs(res[a] - rows[b]) <= S * 8 * 2.0 ** -53 * scale * (S if b == "weight_ess" else 1.0)), a


def test_na_members_are_integrated_out_with_their_group():
    """Two rows of two different 3 x 3 cells lose their y after the problem is built: they stay in their blocks and groups, are not
    scored, and the estimator follows the exact density of the remaining members."""
    pb0 = make_problem(side=12, q=1, seed=5)
    lab = gr.cell_labels(pb0, 3)
    na = np.array([np.nonzero(lab == lab.min())[0][4], np.nonzero(lab == lab.max())[0][0]])
    pb, members, exact, res, se, _ = exact_case(12, 1, lambda pb: gr.cell_labels(pb, 3), S=2000, na=na)
    assert sum(m.size for m in members) == pb["n"] and all(m.size == 9 for m in members)      # the NA rows are members
    assert np.all(np.isnan(res["mu_lgo"][na])) and np.all(np.isnan(res["pit_lgo"][na]))
    assert np.isfinite(res["mu_lgo"]).sum() == pb["n"] - 2
    ratio = np.abs(res["elpd_lgo"] - exact) / se
    print("NA members: largest ratio", ratio.max())
    assert np.all(ratio <= 5.0)
    full = gr.exact_lgo(make_problem(side=12, q=1, seed=5), *lr.density_precision(pb0, pb0["theta"]), np.zeros(pb["n"]), np.full(pb["n"], TAUSQ), members)
    hit = [g for g, m in enumerate(members) if np.intersect1d(m, na).size]
    assert len(hit) == 2 and np.all(np.abs(exact[hit] - full[hit]) > 0.1)          # eight members are not nine


def test_float64_definition_matches_the_long_double_reference():
    pb = make_problem(side=12, q=2, seed=5)
    n = pb["n"]
    Q, rows = lr.density_precision(pb, pb["theta"])
    _, members = loo.group_index(loo.site_groups(pb["coords"]), rows)
    rng = np.random.default_rng(3)
    S = 40
    xb, tq = 0.1 * rng.standard_normal(n), np.where(pb["mv_id"] == 1, 0.2, 0.05)
    state = loo.new_group_state(members)
    ls = np.zeros((S, len(members)), dtype=np.longdouble)
    for s in range(S):
        w = rng.standard_normal(n) * (1 + 0.1 * s)
        terms = [loo.group_terms(Q, w, m, pb["y"], xb, tq) for m in members]
        for g, (m, t) in enumerate(zip(members, terms)):
            ref = gr.group_terms_ld(Q[np.ix_(m, m)], Q[m] @ w, w[m], pb["y"][m], xb[m], tq[m])
            k = max(ref["kappa_A"], ref["kappa_S"])
            assert abs(t["l"] - float(ref["l"])) <= 64 * 2.0 ** -53 * k * (abs(float(ref["l"])) + ref["quad"] + 2)
            assert np.allclose(t["cond_cov"], ref["cond_cov"].astype(np.float64), rtol=64 * 2.0 ** -53 * k, atol=0)
            assert np.all(np.abs(t["cond_mean"] - ref["cond_mean"].astype(np.float64)) <= 64 * 2.0 ** -53 * k * (np.abs(t["cond_cov"]) @ np.abs(t["qw"]) + np.abs(w[m])))
            assert np.allclose(t["phi"], ref["phi"], rtol=0, atol=1e-12) and np.allclose(t["mu"], ref["mu"].astype(np.float64), rtol=0, atol=1e-12)
            ls[s, g] = ref["l"]
        loo.update_groups(state, terms)
    got = loo.finish_groups(state, S, members, n, np.isfinite(pb["y"]))
    ref, _, _ = lr.estimator_ld(ls, np.zeros(ls.shape), np.zeros(ls.shape))
    assert np.all(np.abs(got["elpd_lgo"] - ref["elpd_loo"]) <= 1e-10 * np.maximum(np.abs(ref["elpd_loo"]), 1.0))
    assert np.allclose(got["weight_ess"], ref["weight_ess"], rtol=1e-10)


@pytest.mark.parametrize("S", [1, 2])
def test_one_and_two_draws(S):
    members = [np.array([0, 2]), np.array([1])]
    mk = lambda l, phi, mu, ob: dict(l=l, phi=np.array(phi), mu=np.array(mu), obs=np.array(ob, dtype=np.int64))   # noqa: E731
    draws = [[mk(-1.0, [0.2, 0.4], [1.0, -1.0], [0, 1]), mk(-700.0, [0.5], [2.0], [0])],
             [mk(-2.5, [0.6, 0.1], [3.0, 0.5], [0, 1]), mk(-1.0, [0.9], [5.0], [0])]][:S]
    st = loo.new_group_state(members)
    for terms in draws:
        loo.update_groups(st, terms)
    got = loo.finish_groups(st, S, members, 3, np.ones(3, dtype=bool))
    ls = np.array([[t["l"] for t in terms] for terms in draws])
    ref, _, _ = lr.estimator_ld(ls, np.zeros_like(ls), np.zeros_like(ls))
    assert np.allclose(got["elpd_lgo"], ref["elpd_loo"], rtol=1e-14, atol=0) and np.allclose(got["weight_ess"], ref["weight_ess"], rtol=1e-14)
    r = np.exp(-(ls - ls.min(axis=0)))
    r /= r.sum(axis=0)
    assert np.allclose(got["mu_lgo"][[0, 2]], sum(r[s, 0] * draws[s][0]["mu"] for s in range(S)), rtol=1e-13)
    assert np.allclose(got["pit_lgo"][1], sum(r[s, 1] * draws[s][1]["phi"][0] for s in range(S)), rtol=1e-13)
    if S == 1:
        assert np.array_equal(got["elpd_lgo"], ls[0]) and np.array_equal(got["weight_ess"], np.ones(2))
        assert np.array_equal(got["mu_lgo"], [1.0, 2.0, -1.0]) and np.array_equal(got["pit_lgo"], [0.2, 0.5, 0.4])


def test_a_skipped_draw():
    members = [np.array([0, 1])]
    mk = lambda l: dict(l=l, phi=np.array([0.3, 0.6]), mu=np.array([1.0, 2.0]), obs=np.array([0, 1]))   # noqa: E731
    st = loo.new_group_state(members)
    loo.update_groups(st, [mk(-1.0)])
    before = {k: (np.copy(v) if k in ("M", "A1", "A2", "NS") else [a.copy() for a in v]) for k, v in st.items()}
    for bad in (np.nan, -np.inf, np.inf):
        loo.update_groups(st, [mk(bad)])
    assert st["NS"][0] == 3 and all(st[k][0] == before[k][0] for k in ("M", "A1", "A2"))
    assert np.array_equal(st["AP"][0], before["AP"][0]) and np.array_equal(st["AM"][0], before["AM"][0])
    got = loo.finish_groups(st, 4, members, 2, np.ones(2, dtype=bool))
    assert got["elpd_lgo"][0] == -1.0 and got["n_skipped"][0] == 3
    # a pivot that is not > 0: A indefinite, the draw is skipped
    t = loo.group_terms_from(np.array([[1.0, 2.0], [2.0, 1.0]]), np.zeros(2), np.zeros(2), np.zeros(2), np.zeros(2), np.ones(2))
    assert np.isnan(t["l"])
    st = loo.new_group_state(members)
    loo.update_groups(st, [t])
    out = loo.finish_groups(st, 1, members, 2, np.ones(2, dtype=bool))
    assert np.isnan(out["elpd_lgo"][0]) and np.all(np.isnan(out["mu_lgo"])) and out["n_skipped"][0] == 1


# ---- the group structures ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def layout_check(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    exe = str(tmp_path_factory.mktemp("lgo_layout_check") / "lgo_layout_check")
    subprocess.run([hipcc, "--offload-host-only", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "lgo_layout_check.cpp"), os.path.join(CSRC, "tree_layout.cpp"),
                    os.path.join(CSRC, "loo_layout.cpp"), os.path.join(CSRC, "lgo_layout.cpp"), "-o", exe], check=True, timeout=600)
    return exe


def run_check(exe, tmp_path, pb, labels, *flags):
    path, lpath = str(tmp_path / "problem.bin"), str(tmp_path / "labels.bin")
    write_problem(path, problem_arrays(pb))
    np.ascontiguousarray(labels, dtype=np.int64).tofile(lpath)
    r = subprocess.run([exe, path, lpath, *flags], capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout.strip()


def report(out):
    assert out.startswith("OK "), out
    return {k: int(v) for k, v in (kv.split("=") for kv in out.split()[1:])}


def cells_or_columns(pb):
    x = pb["coords"][:, 0]
    if np.unique(pb["coords"][:, 1]).size == 4:          # the strip: 4 consecutive columns of its 4 rows
        return (np.searchsorted(np.unique(x), x) // 4).astype(np.int64)
    return gr.cell_labels(pb, 2)


@pytest.mark.parametrize("name", sorted(LAYOUT_CASES))
@pytest.mark.parametrize("kind", ["sites", "cells", "random"])
def test_layout_invariants(layout_check, tmp_path, name, kind):
    pb = LAYOUT_CASES[name][0]()
    labels = {"sites": sites, "cells": cells_or_columns, "random": lambda pb: gr.random_labels(pb["n"], 3, 7)}[kind](pb)
    obs = np.isfinite(pb["y"])
    for v in np.unique(labels[labels >= 0]):             # the `missing` case: a group left without an observed member leaves
        if not obs[labels == v].any():
            labels[labels == v] = -1
    rows = np.sort(np.concatenate([pb["indexing"][u] for u in lr.density_blocks(pb)]))
    _, members = loo.group_index(labels, rows, obs)
    for flags in ((), ("force-generic",)):
        rc, out = run_check(layout_check, tmp_path, pb, labels, *flags)
        assert rc == 0, out
        rep = report(out)
        assert rep["groups"] == len(members) and rep["members"] == sum(m.size for m in members)
        assert rep["max_members"] == max(m.size for m in members) and rep["pair_slots"] >= rep["pairs"]
        assert rep["pairs"] + rep["structural_zeros"] == sum(m.size * (m.size - 1) // 2 for m in members)
        assert rep["edges"] > 0
    if kind == "random":
        assert rep["structural_zeros"] > 0               # members on different branches
    if kind == "sites" and pb["q"] == 1:
        assert rep["pairs"] == 0 and rep["blocks_with_pairs"] == 0
    if name == "strip_deep" and kind == "cells":
        assert rep["max_members"] == 16 and rep["max_blocks_spanned"] >= 3


def test_a_block_without_pairs_among_blocks_that_have_them(layout_check, tmp_path):
    pb = LAYOUT_CASES["q1_grid"][0]()
    labels = gr.cell_labels(pb, 2)
    labels[np.isin(labels, np.unique(labels)[10:])] = -1     # ten cells only: most blocks see no group
    rc, out = run_check(layout_check, tmp_path, pb, labels)
    assert rc == 0, out
    rep = report(out)
    assert rep["groups"] == 10 and rep["blocks_with_pairs"] > 0 and rep["blocks_without_pairs"] > 0


def test_layout_checks_can_fail_and_refusals(layout_check, tmp_path):
    pb = LAYOUT_CASES["q1_grid"][0]()
    cells = gr.cell_labels(pb, 2)
    rc, out = run_check(layout_check, tmp_path, pb, cells, "swap-pair")
    assert rc == 1 and out.startswith("VIOLATED pairs:") and "not sorted" in out, out
    rc, out = run_check(layout_check, tmp_path, pb, cells, "drop-finish")
    assert rc == 1 and out.startswith("VIOLATED pairs:") and "finishing slot -1" in out, out
    rc, out = run_check(layout_check, tmp_path, pb, cells, "double-finish")
    assert rc == 1 and out.startswith("VIOLATED "), out
    big = gr.cell_labels(pb, 4)
    big[np.nonzero(big == 3)[0][0]] = 0
    rc, out = run_check(layout_check, tmp_path, pb, big)
    assert rc == 2 and out.startswith("REFUSED -4 ") and "17 members" in out and "16" in out, out
    na = LAYOUT_CASES["q1_grid"][0]()                    # two rows lose their y after the problem is built: NA rows in density blocks
    na["y"] = na["y"].copy()
    na["y"][[3, 200]] = np.nan
    lab = -np.ones(na["n"], dtype=np.int64)
    lab[[3, 200]] = 5
    rc, out = run_check(layout_check, tmp_path, na, lab)
    assert rc == 2 and out.startswith("REFUSED -1 ") and "no member with an observed y" in out, out
    rc, out = run_check(layout_check, tmp_path, pb, cells, "world2")
    assert rc == 2 and out.startswith("REFUSED -4 ") and "multi-GPU" in out, out
    lim = make_problem(side=20, q=2, seed=5, limited_tree=True)
    rc, out = run_check(layout_check, tmp_path, lim, np.zeros(lim["n"], dtype=np.int64) - 1, "limited")
    assert rc == 2 and out.startswith("REFUSED -4 ") and "limited_tree" in out, out


# ---- the labelling helpers and their refusals ---------------------------------------------------------------------------------
def test_labelling_helpers_and_value_errors():
    pb = make_problem(side=6, q=2, seed=5)
    s = loo.site_groups(pb["coords"])
    assert s.dtype == np.int64 and np.unique(s).size == 36 and all((s == v).sum() == 2 for v in np.unique(s))
    assert all(np.unique(pb["mv_id"][s == v]).size == 2 for v in np.unique(s))
    b = loo.block_groups(pb["coords"], 0.5)
    assert b.dtype == np.int64 and np.unique(b).size <= 9 and np.array_equal(b[pb["mv_id"] == 1], b[pb["mv_id"] == 2])
    label, members = loo.group_index(np.array([3, -1, 0, 3, 0, 7]), rows=np.array([0, 1, 2, 3, 4]))
    assert label.tolist() == [0, 3] and [m.tolist() for m in members] == [[2, 4], [0, 3]]
    # one sort each, no loop over groups or rows: the same as the plain definition on random labels, and a million rows at once
    rng = np.random.default_rng(2)
    lab = rng.integers(-3, 400, size=3000)
    rows, obs = np.sort(rng.choice(3000, 2500, replace=False)), rng.uniform(size=3000) < 0.9
    label, members = loo.group_index(lab, rows, None)
    inrows = np.zeros(3000, dtype=bool)
    inrows[rows] = True
    want = [v for v in range(400) if (inrows & (lab == v)).any()]
    assert label.tolist() == want and all(np.array_equal(m, np.nonzero(inrows & (lab == v))[0]) for v, m in zip(want, members))
    xy = rng.integers(0, 30, size=(2000, 2)).astype(np.float64)
    s2 = loo.site_groups(xy)
    keys = {tuple(c) for c in xy}
    assert np.unique(s2).size == len(keys) and all(len({tuple(c) for c in xy[s2 == v]}) == 1 for v in np.unique(s2)[::17])
    big = loo.block_groups(np.stack(np.meshgrid(np.arange(1000.0), np.arange(1000.0), indexing="ij"), -1).reshape(-1, 2), 2.0)
    label, members = loo.group_index(big, None, np.ones(big.size, dtype=bool))
    assert label.size == 250000 and all(m.size == 4 for m in members[::5003]) and members[0].tolist() == [0, 1, 1000, 1001]
    with pytest.raises(ValueError, match="n x d"):
        loo.site_groups(np.zeros(4))
    with pytest.raises(ValueError, match="d >= 2"):
        loo.block_groups(np.zeros((4, 1)), 0.1)
    for cell in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="positive"):
            loo.block_groups(pb["coords"], cell)
    with pytest.raises(ValueError, match="one integer label per row"):
        loo.group_index(np.zeros(4))
    with pytest.raises(ValueError, match="one integer label per row"):
        loo.group_index(np.zeros((4, 2), dtype=np.int64))
    with pytest.raises(ValueError, match="17 members, at most 16"):
        loo.group_index(np.zeros(17, dtype=np.int64))
    with pytest.raises(ValueError, match="no member with an observed y"):
        loo.group_index(np.array([0, 0, 1]), observed=np.array([True, False, False]))


# ---- fit's refusals, all before any device call -----------------------------------------------------------------------------
def test_fit_value_errors(monkeypatch):
    from spamtree_amd import _lib, fit
    from tests.test_rows_loo_cpu import fit_args

    def no_device():
        raise AssertionError("the library was loaded before the refusal")
    monkeypatch.setattr(_lib, "load", no_device)
    pb = make_problem(side=8, q=2, seed=5)
    n = pb["n"]
    site = loo.site_groups(pb["coords"])
    kw = dict(mcmc_keep=8, mcmc_burn=0, mcmc_thin=1)
    with pytest.raises(ValueError, match="needs loo=True"):
        fit.spamtree_mv_mcmc(*fit_args(pb), **kw, loo_groups=site)
    with pytest.raises(ValueError, match="one integer label per row"):
        fit.spamtree_mv_mcmc(*fit_args(pb), **kw, loo=True, loo_groups=site[:-1])
    with pytest.raises(ValueError, match="one integer label per row"):
        fit.spamtree_mv_mcmc(*fit_args(pb), **kw, loo=True, loo_groups=site.astype(np.float64))
    with pytest.raises(ValueError, match="17 members, at most 16"):
        fit.spamtree_mv_mcmc(*fit_args(pb), **kw, loo=True, loo_groups=np.where(np.arange(n) < 17, 0, -1))
    na = dict(pb, y=pb["y"].copy())
    na["y"][site == 3] = np.nan                          # a site that lost both outcomes after the problem was built
    with pytest.raises(ValueError, match="label 3 has no member with an observed y"):
        fit.spamtree_mv_mcmc(*fit_args(na), **kw, loo=True, loo_groups=site)
    with pytest.raises(ValueError, match="limited_tree"):  # loo's own refusals come first
        fit.spamtree_mv_mcmc(*fit_args(make_problem(side=8, q=1, seed=5, limited_tree=True)), **kw, loo=True, loo_groups=np.zeros(64, dtype=np.int64))
    # and with nothing refused the next thing it does is load the library
    with pytest.raises(AssertionError, match="before the refusal"):
        fit.spamtree_mv_mcmc(*fit_args(pb), **kw, loo=True, loo_groups=site)
