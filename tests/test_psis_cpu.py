"""CPU-only: Pareto smoothing of the leave-one-out weights.  The float64 definition (spamtree_amd/psis.py) against the 50-digit
restatement (tests/psis_reference.py) on the whole case list, the integers of the definition, the recovery of a known shape, the
cases that do not smooth against the raw estimator, the end-to-end total on the exact Gaussian, the host-only plan
(tests/psis_plan_check.cpp over spamtree_amd/csrc/psis_plan.cpp) and every ValueError of fit.

MEASURED (psis_reference.distance: |x - ref| / max(|ref|, 1), the largest over khat, elpd_psis, pit_psis, mu_psis, weight_ess_psis and
sigma, over all 733 series of the case list, 420 of which smooth): 1.886e-13, at weight_ess_psis of a K = 16384 series -- the
definition's sums are plain chains of up to 16384 additions; khat 2.8e-14, sigma 2.0e-15, elpd_psis 7.9e-14.  Recorded as
psis_reference.F64_DISTANCE = 1.9e-13; the bound here is 4 times that.

RECOVERY BANDS (psis_reference.KHAT_BAND): the largest |khat - k| of the restatement over the seeds 1000 .. 1199 of
scipy.stats.genpareto.rvs(k, size=4000), times 1.5: k = -0.3: 0.2072 -> 0.311;  0.1: 0.2400 -> 0.360;  0.5: 0.3175 -> 0.477;
0.9: 0.3927 -> 0.590;  1.5: 0.4785 -> 0.718.  The estimator is that wide at S = 4000 (a tail of 190 draws).
"""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from spamtree_amd import loo, psis
from tests import psis_reference as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spamtree_amd", "csrc")
U = 2.0 ** -53


def test_definition_against_the_restatement_on_the_case_list():
    worst, where, smoothed, total = 0.0, None, 0, 0
    for name, t, phi, mu in pr.case_list():
        ref = pr.reference(name)
        for i in range(t.shape[1]):
            got = psis.estimates(t[:, i], phi[:, i], mu[:, i])
            assert got["tail_len"] == ref[i]["tail_len"] and got["n_draws"] == ref[i]["n_draws"], (name, i)
            d = pr.distance(ref[i], got, pr.DOUBLES + (("sigma",) if ref[i]["smoothed"] else ()))   # asserts the inf / NaN pattern
            if d > worst:
                worst, where = d, (name, i)
            smoothed += ref[i]["smoothed"]
            total += 1
    print(f"float64 definition against the restatement: {worst:.3e} at {where}; {smoothed} of {total} series smooth")
    assert total == 733 and 300 < smoothed < total
    assert worst <= 4 * pr.F64_DISTANCE, (worst, where)


def test_every_kind_of_the_case_list_does_what_it_is_there_for():
    """The kinds that must not smooth do not, the others do once S allows a tail; ties straddle the cut with different companions."""
    seen = {k: [0, 0] for k in pr.KINDS}
    for a, K in enumerate(pr.KS):
        for name, t, phi, mu in pr.case_list():
            if not name.startswith(f"K{K}_"):
                continue
            ref = pr.reference(name)
            for i in range(t.shape[1]):
                kind = pr.KINDS[(i + a) % len(pr.KINDS)]
                seen[kind][ref[i]["smoothed"]] += 1
                if kind == "skipped":
                    assert ref[i]["n_draws"] == 0 and math.isnan(ref[i]["khat"])
                if kind in ("const_tail", "quarter") or ref[i]["n_draws"] < 25:
                    assert not ref[i]["smoothed"], (name, i, kind)
                if kind in ("gpd0.5", "gauss", "range") and K >= 25:
                    assert ref[i]["smoothed"] and ref[i]["tail_len"] == pr.tail_length_rational(K), (name, i, kind)
                if kind == "ties" and ref[i]["smoothed"]:
                    col = t[:, i]
                    order = sorted(range(K), key=lambda s: (col[s], s))
                    M = ref[i]["tail_len"]
                    below, first = order[K - M - 1], order[K - M]
                    assert col[below] == col[first] and below < first and phi[below, i] != phi[first, i]   # a tie across the cut
    assert seen["ties"][1] > 0 and seen["sprinkled"][0] > 0 and seen["sprinkled"][1] > 0 and seen["gpd1.5"][1] > 0 and seen["gpd-0.3"][1] > 0


def test_integers():
    for S in range(1, 16385):
        assert psis.tail_length(S) == pr.tail_length_rational(S), S
    assert psis.tail_length(16384) == psis.MAX_TAIL == 384 and psis.tail_length(24) == 4 and psis.tail_length(25) == 5
    for N in range(5, 385):
        assert psis.quarter_index(N) == (N + 2) // 4 and 1 <= psis.quarter_index(N) <= N
        assert psis.grid_size(N) == 30 + math.isqrt(N) <= 49
    assert psis.khat_threshold(1000) == 1.0 - 1.0 / 3.0 and psis.khat_threshold(10 ** 6) == 0.7


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_recovery_of_a_known_shape(seed):
    from scipy.stats import genpareto
    got = []
    for k in pr.KHAT_BAND:
        r = genpareto.rvs(k, size=4000, random_state=seed)
        e = psis.estimates(np.log(r))
        assert e["tail_len"] == 190 and e["n_draws"] == 4000
        print(f"seed {seed} k {k}: khat {e['khat']:.4f} (band {pr.KHAT_BAND[k]})")
        assert abs(e["khat"] - k) <= pr.KHAT_BAND[k], (k, e["khat"])
        got.append(e["khat"])
    assert all(a < b for a, b in zip(got, got[1:])), got


def raw_rows(t, phi, mu):
    st = loo.new_state(t.shape[1])
    for s in range(t.shape[0]):
        loo.update(st, -t[s], phi[s], mu[s])
    return loo.finish(st, t.shape[0])


def no_smoothing_series():
    rng = np.random.default_rng(7)
    out = {}
    for K in (1, 2, 7, 24):
        out[f"S{K}"] = rng.standard_normal(K)
    t = rng.standard_normal(200) - 4.0
    t[rng.choice(200, size=45, replace=False)] = 2.25          # M = 40: a constant tail
    out["const_tail"] = t
    t = rng.standard_normal(200)
    order = np.argsort(t, kind="stable")
    t[order[160:160 + 10]] = t[order[159]]                      # x_1 .. x_10 = 0: the quarter index 10 is tied with the cut
    out["quarter"] = t
    t = rng.standard_normal(30)
    t[[3, 17]] = [np.nan, -np.inf]                              # S = 28: M = 5; and a skipped pair
    t[rng.choice(np.setdiff1d(np.arange(30), [3, 17]), size=8, replace=False)] = 3.0
    out["skips_const"] = t
    return out


@pytest.mark.parametrize("name", sorted(no_smoothing_series()))
def test_no_smoothing_means_raw(name):
    t = no_smoothing_series()[name]
    K = t.size
    rng = np.random.default_rng(K)
    phi, mu = rng.random(K), rng.standard_normal(K)
    e = psis.estimates(t, phi, mu)
    assert e["khat"] == math.inf and e["tail_len"] == 0 and e["n_draws"] == int(np.isfinite(t).sum())
    raw = raw_rows(t[:, None], phi[:, None], mu[:, None])
    # loo's streaming sums and the definition's direct ones: a few roundings per draw on sums of positive terms (mu: against |mu|)
    for a, b, scale in (("elpd_psis", "elpd_loo", None), ("pit_psis", "pit_loo", None), ("mu_psis", "mu_loo", np.abs(mu).max()),
                        ("weight_ess_psis", "weight_ess", None)):
        s = max(abs(raw[b][0]), 1.0) if scale is None else scale
        assert abs(e[a] - raw[b][0]) <= K * 8 * U * s, (a, e[a], raw[b][0])


def test_end_to_end_on_the_exact_gaussian():
    """side 12, q = 1, 4000 draws of the exact posterior (tests/test_rows_loo_cpu.py's set-up).  The total's Monte-Carlo standard error
    by the delta method on the self-normalised ratio: elpd_i = log(mean_s e^u_is / mean_s e^lw'_is), so draw s moves the total by
    G_s = sum_i (e^u_is / mean e^u_i - e^lw'_is / mean e^lw'_i) / S and se = sd(G_s) / sqrt(S) (the rows share the draws: no
    independence across rows is assumed)."""
    from tests.test_rows_loo_cpu import exact_case
    pb, exact, terms, _ = exact_case(12, 1)
    S, n = len(terms), pb["n"]
    t, phi, mu = (np.array([x[k] for x in terms]) for k in range(3))
    t = -t
    rows = psis.estimates_store(t, phi, mu)
    G = np.zeros(S)
    for i in range(n):
        sm = psis.smooth(t[:, i])
        eu, ew = np.exp(sm["lw_s"] - sm["lw"]), np.exp(sm["lw_s"])
        G += eu / eu.mean() - ew / ew.mean()
    se = G.std(ddof=1) / math.sqrt(S)
    total, ex = rows["elpd_psis"].sum(), exact.sum()
    raw = raw_rows(t, phi, mu)
    print(f"sum elpd_psis {total:.3f}, raw {raw['elpd_loo'].sum():.3f}, exact {ex:.3f}, se {se:.3f}, ratio {abs(total - ex) / se:.2f}; "
          f"max khat {rows['khat'].max():.3f}, min {rows['khat'].min():.3f}, rows above 0.7: {(rows['khat'] > 0.7).sum()}")
    assert abs(ex - (-317.33)) < 0.01
    assert np.all(rows["tail_len"] == 190) and np.all(rows["n_draws"] == S)
    assert abs(total - ex) <= 5.0 * se, (total, ex, se)
    assert np.all((rows["pit_psis"] > 0) & (rows["pit_psis"] < 1)) and np.all(rows["weight_ess_psis"] > 1)


# ---- host-only: the plan and the store's bookkeeping ---------------------------------------------------------------------------
def test_plan_check_program(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    exe = str(tmp_path / "psis_plan_check")
    # the stand-alone host program with the sanitizers, on the CPU: nothing is preloaded
    subprocess.run([hipcc, "--offload-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "psis_plan_check.cpp"),
                    os.path.join(CSRC, "psis_plan.cpp"), "-o", exe], check=True, timeout=600)
    for lim in ("163840", "65536", "4096"):
        r = subprocess.run([exe, lim], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.startswith("OK "), (lim, r.stdout, r.stderr)


def test_criteria_dict_from_a_totals_table():
    from spamtree_amd import _lib
    from spamtree_amd.model import rows_psis_criteria
    assert len(_lib.ST_ROWS_PSIS) == 9
    rng = np.random.default_rng(0)
    e = [rng.standard_normal(5) - 2, rng.standard_normal(3) - 1]
    tot = np.zeros((9, 3), order="F")
    for j, v in enumerate(e):
        tot[:, j] = [v.size, v.sum(), (v * v).sum(), 2.0 * v.size, 0.5 * v.size, 30.0 + j, 0.4 + 0.5 * j, j, 2 * j]
    tot[5, 2] = tot[6, 2] = np.nan                                   # an outcome without rows
    c = rows_psis_criteria(tot, np.array([5, 3, 0]))
    allv = np.concatenate(e)
    assert c["n"] == 8 and abs(c["elpd_psis"] - allv.sum()) < 1e-12 and c["looic"] == -2.0 * c["elpd_psis"]
    assert abs(c["se"] - math.sqrt(8 * allv.var(ddof=1))) < 1e-12
    assert abs(c["by_outcome"]["se"][0] - math.sqrt(5 * e[0].var(ddof=1))) < 1e-12 and math.isnan(c["by_outcome"]["se"][2])
    assert c["max_khat"] == 0.9 and c["min_weight_ess"] == 30.0 and c["n_khat_bad"] == 1 and c["n_khat_above"] == 2
    assert c["mse"] == 2.0 and c["pit"] == 0.5 and abs(c["rmse"] - math.sqrt(2.0)) < 1e-15


# ---- fit: every ValueError comes before any device call -------------------------------------------------------------------------
def test_fit_value_errors_come_before_the_device(monkeypatch):
    from spamtree_amd import _lib, fit
    from tests.util import make_problem

    def fit_args(pb):
        k = pb["theta"].size
        return (pb["y"], pb["X"], pb["Z"], pb["coords"], pb["mv_id"], pb["blocking"], pb["gix_block"], pb["res_is_ref"], pb["parents"],
                pb["children"], False, pb["block_names"], pb["block_groups"], pb["indexing"], pb["bounds"], np.zeros(pb["n"]), pb["theta"],
                np.zeros(pb["p"]), 0.1, 0.02 * np.eye(k))

    def no_device():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_device)
    pb = make_problem(side=8, q=1, seed=5)
    with pytest.raises(ValueError, match="needs loo=True"):
        fit.spamtree_mv_mcmc(*fit_args(pb), psis=True, mcmc_keep=4, mcmc_burn=0)
    with pytest.raises(ValueError, match="needs loo=True"):
        fit.spamtree_mv_mcmc(*fit_args(pb), psis_draws=True, mcmc_keep=4, mcmc_burn=0)
    for keep in (0, 16385):
        with pytest.raises(ValueError, match=f"mcmc_keep = {keep} must lie in 1 .. 16384"):
            fit.spamtree_mv_mcmc(*fit_args(pb), loo=True, psis=True, mcmc_keep=keep, mcmc_burn=0)
    with pytest.raises(AssertionError, match="the library was loaded"):      # a good request gets as far as the device
        fit.spamtree_mv_mcmc(*fit_args(pb), loo=True, psis=True, mcmc_keep=4, mcmc_burn=0)


def test_device_entry_needs_a_handle():
    with pytest.raises(ValueError, match="handle"):
        psis.psis(np.zeros((4, 2)))
