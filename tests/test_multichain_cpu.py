"""CPU: the multi-chain diagnostics on the host (spamtree_amd.diagnostics.multichain_diagnostics, multichain_indicator_ess,
multichain_rank_diagnostics) against tests/multichain_reference.py (long double; the indicator ESS in Python integers and exact
rationals), and the pure check of n_chains (store_spec.cpp, check_chains) as a stand-alone program.

The host functions work in float64 with NumPy's own sums, so their distance from the long-double reference is bounded here by the
reference's device bound (multichain_reference.chain_bounds: the lane-strided chains are no shorter than NumPy's pairwise ones)
with every series' condition in it; integer-defined outputs (the indicator ESS, prob, lags away from a pair near zero) are held
to 4 ulp of the one quotient and the one division."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from spamtree_amd import diagnostics as dg
from tests import diag_reference as dref
from tests import multichain_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spamtree_amd", "csrc")
MS, NS = (1, 2, 3, 4, 16), (4, 5, 63, 64, 65, 129)
U = 2.0 ** -53


def series(M, N, seed, kind):
    """M chains of N draws end to end: AR(1) chains of differing levels and scales, or chains that agree in distribution."""
    rng = np.random.default_rng(seed)
    if kind == "shifted":
        return np.concatenate([dref.ar1(N, 0.7, seed=seed * 100 + c, scale=1.0 + 0.2 * c) + 0.5 * c for c in range(M)])
    if kind == "offset":
        return np.concatenate([dref.ar1(N, -0.5, seed=seed * 100 + c, offset=1e3) for c in range(M)])
    return rng.standard_normal(M * N)


def close(got, want, bound, what):
    if math.isnan(want):
        assert math.isnan(got), what
    else:
        assert abs(got - want) <= bound * abs(want), (what, got, want, abs(got - want) / abs(want), bound)


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N", NS)
def test_moments_against_the_long_double_reference(M, N):
    for kind in ("shifted", "offset", "white"):
        x = series(M, N, seed=M * 1000 + N, kind=kind)
        for max_lag in (0, 3, 2 * N):
            got, r = dg.multichain_diagnostics(x, M, max_lag), ref.reference(x, M, max_lag)
            b = ref.chain_bounds(r, M * N, got["lags"] // 2)
            for k in ("ess", "mcse", "sd", "rhat"):
                close(got[k], r[k], b[k] if not math.isnan(r[k]) else 0.0, (kind, max_lag, k))
            if r["min_abs_gamma"] > 1e-8:
                assert got["lags"] == r["lags"] and got["truncated"] == r["truncated"], (kind, max_lag)


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N", NS)
def test_rank_family_against_the_reference(M, N):
    x = series(M, N, seed=M * 77 + N, kind="shifted")
    kw = dict(probs=(0.1, 0.5), thresholds=(0.3, 1.0), sides=(1, -1), max_lag=0)
    got = dg.multichain_rank_diagnostics(x, M, **kw)
    eps = ref.rr.PHI_ERR_MEASURED   # the host's own Phi^-1
    if M == 1:   # the single-chain reference and its bound
        r = ref.rr.reference(x, **kw)
        depth = -(-N // 64) + 6
        bb, bf = ref.rr.score_bounds(r["bulk"], N, got["lags_bulk"] // 2, depth, eps), ref.rr.score_bounds(r["fold"], N, 0, depth, eps)
    else:
        r = ref.rank_reference(x, M, **kw)
        bb, bf = ref.chain_bounds(r["bulk"], M * N, got["lags_bulk"] // 2, eps), ref.chain_bounds(r["fold"], M * N, 0, eps)
    close(got["ess_bulk"], r["ess_bulk"], bb["ess"], "ess_bulk")
    close(got["rhat_bulk"], r["rhat_bulk"], bb.get("rhat", 0.0), "rhat_bulk")
    close(got["rhat_fold"], r["rhat_fold"], bf.get("rhat", 0.0), "rhat_fold")
    close(got["rhat_rank"], r["rhat_rank"], max(bb.get("rhat", 0.0), bf.get("rhat", 0.0)), "rhat_rank")
    for k, lk in (("ess_q", "lags_q"), ("ess_exc", "lags_exc")):
        for j, want in enumerate(r[k]):
            close(float(got[k][j]), want, 4 * U, (k, j))
            assert int(got[lk][j]) == r[lk][j]   # integers decide the pairs: no tolerance
    close(got["ess_tail"], r["ess_tail"], 4 * U, "ess_tail")
    assert [float(p) for p in got["prob"]] == r["prob"]
    for j, want in enumerate(r["mcse_prob"]):
        close(float(got["mcse_prob"][j]), want, 8 * U, ("mcse_prob", j))


def same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


@pytest.mark.parametrize("N", NS + (1000,))
def test_one_chain_is_the_single_chain_function(N):
    x = series(1, N, seed=N, kind="shifted")
    for max_lag in (0, 3):
        same_bits(dg.multichain_diagnostics(x, 1, max_lag), dg.series_diagnostics(x, max_lag))
        kw = dict(probs=(0.25,), thresholds=(0.1,), sides=(1,), max_lag=max_lag)
        same_bits(dg.multichain_rank_diagnostics(x, 1, **kw), dg.rank_series_diagnostics(x, **kw))
        I = x > 0.2
        assert dg.multichain_indicator_ess(I, 1, max_lag) == dg.indicator_ess(I, max_lag)


@pytest.mark.parametrize("M", (2, 4, 16))
def test_the_integer_bound_on_its_worst_cases(M):
    """K = 16384: half the chains all ones and the rest all zeros (N D = K^3 / 4, every S_t = 0), and every chain half ones, as one
    block (the largest A_{c,t}) -- multichain_reference.indicator_ess asserts N D <= K^3 / 4, |M (M - 1) S_t| < K^3 / 4,
    |Num_t| < 2^41 and |2 sum N_k - Num_0| < 2^57 in Python integers on every lag it visits; the host function agrees with it."""
    K = 16384
    N = K // M
    split = np.concatenate([np.ones(N, dtype=int) if c < M // 2 else np.zeros(N, dtype=int) for c in range(M)])
    assert 4 * N * sum((M * int(split[c * N:(c + 1) * N].sum()) - int(split.sum())) ** 2 for c in range(M)) == K ** 3
    half = np.tile(np.concatenate([np.ones(N // 2, dtype=int), np.zeros(N - N // 2, dtype=int)]), M)
    for I, lag in ((split, 0), (half, 0)):   # (the default cap: 512 pairs, or all N / 2 - 1 of them at M = 16)
        ess, lags, _, worst = ref.indicator_ess(I, M, lag)
        assert worst[0] < 2 ** 41 and worst[1] < 2 ** 57
        got = dg.multichain_indicator_ess(I, M, lag)
        assert got[1] == lags and abs(got[0] - ess) <= 4 * U * ess
    assert ref.indicator_ess(split, M, 0)[3][0] == K ** 3 // 4   # rho_t = 1 at every lag: the bound on N D is attained


def test_chains_in_different_modes_are_seen_only_across_chains():
    """What the feature is for: four chains at levels A, B, A, B.  The pooled split-R-hat of the concatenation compares (A, B) with
    (A, B) and sits near 1; the multi-chain R-hat compares the eight half chains and is far above it, and the combined ESS is far
    below the pooled one.  Levels 0 and 3 (delta = 3) with unit-innovation AR(1) noise (phi = 0.5, variance 1.33), N = 250:
      R-hat  the between-chain variance B' is about delta^2 / 3 = 3 against 1.33 within, so rhat^2 is about 1 + 3 / 1.33: 1.8;
      ESS    the multi-chain rho_t tends to r' = B' / (B' + gbar_0) = 0.69 and never to 0: the pairs stay positive up to the lag cap
             N - 2 and tau is about 2 r' N (truncated).  The pooled series is autocorrelated too (a level lasts N draws): of its
             lag-t pairs (N - t) / N lie inside a chain and t / N straddle an A-B boundary, so the levels' share of its rho_t is
             r (1 - 2 t / N) with r = (delta^2 / 4) / (1.33 + delta^2 / 4) = 0.63, positive up to N / 2: tau is about r N / 2.
             The ratio of the two is about 4 r' / r = 4.4, less what the noise's own terms add to both: the reference gives 3.5.
    Asserted on the reference's own values with room for it: a factor 1.5 in R-hat and 3 in ESS."""
    N = 250
    x = ref.abab(N)
    pooled, multi = dref.reference(x), ref.reference(x, 4)
    print(f"pooled rhat {pooled['rhat']:.4f} ess {pooled['ess']:.2f}; four chains rhat {multi['rhat']:.4f} ess {multi['ess']:.2f}")
    # "near 1" and "far above 1" against each other: the pooled R-hat's distance from 1 is below a tenth of the multi-chain one's
    assert 10 * abs(pooled["rhat"] - 1) < multi["rhat"] - 1 and 1.5 * pooled["rhat"] < multi["rhat"]
    assert 3 * multi["ess"] < pooled["ess"] and multi["truncated"] and not pooled["truncated"]
    got_p, got_m = dg.series_diagnostics(x), dg.multichain_diagnostics(x, 4)
    assert 10 * abs(got_p["rhat"] - 1) < got_m["rhat"] - 1 and got_m["rhat"] > 1.5 * got_p["rhat"] and 3 * got_m["ess"] < got_p["ess"]
    assert abs(got_m["rhat"] - multi["rhat"]) <= 1e-12 * multi["rhat"] and got_m["sd"] == got_p["sd"]
    # the rank-normalised family sees it too
    rk, rk_one = dg.multichain_rank_diagnostics(x, 4, probs=(0.5,)), dg.rank_series_diagnostics(x)
    rk_ref = ref.rank_reference(x, 4, probs=(0.5,))
    assert rk["rhat_rank"] > 1.5 * rk_one["rhat_rank"] and 3 * rk["ess_bulk"] < rk_one["ess_bulk"]
    assert rk_ref["rhat_rank"] > 1.5 * rk_one["rhat_rank"] and abs(rk["rhat_rank"] - rk_ref["rhat_rank"]) <= 1e-12 * rk_ref["rhat_rank"]


def test_edge_cases():
    N, M = 21, 3
    base = dref.ar1(N, 0.6, seed=3)
    # identical copies: B' = 0, and rho_t is one chain's
    x = np.tile(base, M)
    got, r = dg.multichain_diagnostics(x, M), ref.reference(x, M)
    assert r["Bp"] == 0.0 and abs(got["ess"] - r["ess"]) <= 1e-12 * r["ess"]
    one = dg.series_diagnostics(base)   # (tau is about (1 + phi) / (1 - phi) = 4, far above either floor)
    assert got["lags"] == one["lags"] and abs(got["ess"] - M * one["ess"]) <= 1e-12 * got["ess"]
    # one constant chain among varying ones
    x = np.concatenate([base, np.full(N, 0.25), base[::-1]])
    got, r = dg.multichain_diagnostics(x, M), ref.reference(x, M)
    for k in ("ess", "mcse", "sd", "rhat"):
        assert abs(got[k] - r[k]) <= 1e-12 * abs(r[k]), k
    assert got["lags"] == r["lags"]
    # all constant
    got = dg.multichain_diagnostics(np.full(M * N, 1.7), M)
    assert math.isnan(got["ess"]) and math.isnan(got["rhat"]) and got["mcse"] == 0.0 and got["sd"] == 0.0 and got["lags"] == 0
    assert ref.reference(np.full(M * N, 1.7), M)["den"] == 0.0
    # every chain constant at its own value: W = 0 (rhat NaN only), gbar_t = 0, rho_t = 1 at every lag: truncated
    x = np.repeat([1.0, 2.0, 4.0], N)
    got, r = dg.multichain_diagnostics(x, M), ref.reference(x, M)
    assert math.isnan(got["rhat"]) and math.isnan(r["rhat"]) and got["truncated"] and r["truncated"] and got["sd"] > 0
    assert got["lags"] == r["lags"] == 2 * (dg.lag_cap(N)[1] + 1) and abs(got["ess"] - r["ess"]) <= 1e-12 * r["ess"]
    # a NaN draw: through the formulas as the single-chain functions take it; the rank family marks the series
    x = np.tile(base, M)
    x[N + 2] = math.nan
    got = dg.multichain_diagnostics(x, M)
    assert math.isnan(got["sd"]) and math.isnan(got["rhat"]) and math.isnan(got["mcse"]) and got["lags"] == 0
    rk = dg.multichain_rank_diagnostics(x, M, probs=(0.5,), thresholds=(0.0,))
    assert math.isnan(rk["rhat_rank"]) and math.isnan(rk["ess_q"][0]) and math.isnan(rk["prob"][0]) and rk["lags_bulk"] == 0
    assert ref.rank_reference(x, M, probs=(0.5,), thresholds=(0.0,))["lags_bulk"] == 0


def test_indicator_edge_cases():
    N, M = 21, 3
    rng = np.random.default_rng(5)
    # c_c = 0 in one chain, 0 < C < K
    I = np.concatenate([rng.integers(0, 2, N), np.zeros(N, dtype=int), rng.integers(0, 2, N)])
    got, want = dg.multichain_indicator_ess(I, M), ref.indicator_ess(I, M)
    assert got[1] == want[1] and abs(got[0] - want[0]) <= 4 * U * want[0]
    # every chain constant at different values: S_t = 0, D > 0, Num_t = Num_0 at every lag: truncated
    I = np.concatenate([np.ones(N, dtype=int), np.zeros(N, dtype=int), np.ones(N, dtype=int)])
    got, want = dg.multichain_indicator_ess(I, M), ref.indicator_ess(I, M)
    assert got[1] == want[1] == 2 * (dg.lag_cap(N)[1] + 1) and abs(got[0] - want[0]) <= 4 * U * want[0]
    assert all(ref.indicator_num(I, M, t) == ref.indicator_num(I, M, 0) for t in range(N - 1))
    # C = 0 and C = K
    for I in (np.zeros(M * N, dtype=int), np.ones(M * N, dtype=int)):
        got = dg.multichain_indicator_ess(I, M)
        assert math.isnan(got[0]) and got[1] == 0


def test_refusals_on_the_host():
    x = np.arange(24.0)
    for M, text in ((0, "must lie in 1 .. 16"), (17, "must lie in 1 .. 16"), (5, "not a multiple"), (8, "3 per chain")):
        with pytest.raises(ValueError, match=text):
            dg.multichain_diagnostics(x, M)
        with pytest.raises(ValueError, match=text):
            dg.multichain_rank_diagnostics(x, M)
        with pytest.raises(ValueError, match=text):
            dg.multichain_indicator_ess(x > 3, M)


def test_scalar_chain_helpers_take_n_chains():
    """chains_diagnostics / chains_rank_diagnostics (theta, beta, tausq) along the last axis with n_chains: the per-series functions'
    values; the default is what it was."""
    a = np.stack([series(3, 21, seed=s, kind="shifted") for s in (1, 2)]).reshape(2, 1, 63)
    got, one = dg.chains_diagnostics(a, 0, n_chains=3), dg.chains_diagnostics(a)
    assert got["ess"].shape == (2, 1) and got["ess"][1, 0] == dg.multichain_diagnostics(a[1, 0], 3)["ess"]
    assert one["ess"][1, 0] == dg.series_diagnostics(a[1, 0])["ess"] and got["sd"][0, 0] == one["sd"][0, 0]
    rk = dg.chains_rank_diagnostics(a, probs=(0.5,), n_chains=3)
    assert rk["ess_q"].shape == (1, 2, 1) and rk["rhat_rank"][0, 0] == dg.multichain_rank_diagnostics(a[0, 0], 3, probs=(0.5,))["rhat_rank"]


def test_disperse_theta():
    from spamtree_amd import mcmc
    from tests.util import default_bounds
    b = default_bounds(2)
    t = mcmc.disperse_theta(b, 4, seed=3)
    assert t.shape == (4, b.shape[0]) and np.all(t > b[:, 0]) and np.all(t < b[:, 1])
    assert np.array_equal(t, mcmc.disperse_theta(b, 4, seed=3)) and not np.array_equal(t[0], t[1])
    with pytest.raises(ValueError):
        mcmc.disperse_theta(b[:, ::-1], 2)


def test_front_door_refuses_before_any_device_call():
    from spamtree_amd import fit
    from tests.util import make_problem
    pb = make_problem(side=8, q=1, seed=71, p=2)
    k = pb["theta"].size
    args = (pb["y"], pb["X"], pb["Z"], pb["coords"], pb["mv_id"], pb["blocking"], pb["gix_block"], pb["res_is_ref"], pb["parents"],
            pb["children"], False, pb["block_names"], pb["block_groups"], pb["indexing"], pb["bounds"], np.zeros(pb["n"]), pb["theta"],
            np.zeros(pb["p"]), 0.1, 0.02 * np.eye(k))
    for bad, text in ((dict(chains=2, mcmc_keep=8193), "16384"), (dict(chains=17), "1 .. 16"), (dict(chains=0), "1 .. 16"),
                      (dict(chains=2, criteria=True), "separate drivers"), (dict(chains=2, chain_seeds=(1, 2, 3)), "one seed per chain"),
                      (dict(chain_seeds=(1,)), "need chains > 1"), (dict(chains=2, chain_theta=np.ones((3, k))), "one start per chain")):
        with pytest.raises(ValueError, match=text):
            fit.spamtree_mv_mcmc(*args, **dict(dict(mcmc_keep=8, mcmc_burn=1, main_verbose=False), **bad))


def test_driver_refuses_before_the_first_factorisation():
    """stm_mcmc_chains returns its own refusals before it creates the chain: no device is touched."""
    import ctypes as C
    from spamtree_amd import _lib
    from spamtree_amd.model import series_diag_buffers
    from tests.util import make_problem, problem_arrays, st_problem_struct
    lib = _lib.load()
    a = problem_arrays(make_problem(side=8, q=1, seed=1))
    pb = st_problem_struct(a)
    _, s = series_diag_buffers(int(a["n_all"]))
    theta = np.ones(4)
    seeds = np.arange(1, 17, dtype=np.uint64)

    def run(M, keep, want_rows=1, with_seeds=True, world=1):
        ds = _lib.StmDiagnostics(0, want_rows, s, s) if want_rows else None
        ch = _lib.StmChains(M, seeds.ctypes.data_as(C.POINTER(C.c_uint64)) if with_seeds else None, None, None, None)
        opt = _lib.StOptions(0, 1, 0, world, 0, 0)
        common = (C.byref(pb), C.byref(opt), None, theta.ctypes.data_as(C.POINTER(C.c_double)), 4, None, 0.1, None, keep, 1, 1, 1, None,
                  None, None, None, None, None, None, None)
        return lib.stm_mcmc_chains(*common, 0, None, None, None, None, None, 0, None, 0, *([None] * 15),
                                   C.byref(ds) if ds is not None else None, None, None, C.byref(ch))

    said = lambda: lib.stm_mcmc_chains_last_error().decode()   # noqa: E731  (the text of a refusal made before a chain exists)
    assert run(0, 8) == -1 and "n_chains = 0 must lie in 1 .. 16" in said()                  # ST_ERR_USAGE
    assert run(17, 8) == -1 and "n_chains = 17 must lie in 1 .. 16" in said()
    assert run(2, 8, with_seeds=False) == -1 and "seeds is NULL" in said()
    assert run(2, 8193) == -4 and "2 chains x mcmc_keep = 8193 are 16386 stored draws, at most 16384" in said()   # ST_ERR_UNSUPPORTED
    assert run(16, 1025) == -4 and "16400 stored draws" in said()
    assert run(4, 3) == -1 and said() == ""                                                   # fewer than ST_DIAG_MIN_DRAWS per chain: the tier's own refusal
    assert run(2, 0, want_rows=0) == -1 and "mcmc_keep = 0" in said()                         # chains of no saved draw
    assert run(2, 8, world=2) == -4 and "world = 2" in said()                                 # one problem on several GPUs: refused


# ---- the pure check of n_chains (store_spec.cpp), as a stand-alone program ---------------------------------------------------------
def build_check(tmp, name, extra):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    exe = str(tmp / name)
    subprocess.run([hipcc, "--offload-host-only", "-std=c++17", "-O1"] + extra + ["-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "store_spec_chain_check.cpp"), os.path.join(CSRC, "store_spec.cpp"), "-o", exe],
                   check=True, timeout=600)
    return exe


def run_check(exe, *args):
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=120)
    return r.returncode, (r.stdout + r.stderr).strip()


# 22 values of n_chains (-2 .. 19) x 306 values of K (0 .. 300, 16380 .. 16384); 6 x 306 of them outside 1 .. 16
CHAIN_WANT = dict(total=22 * 306, ranges=6 * 306)


def test_the_chain_check_against_its_rule(tmp_path_factory):
    exe = build_check(tmp_path_factory.mktemp("chain_check"), "chain_check", [])
    rc, out = run_check(exe)
    assert rc == 0 and out.startswith("OK "), out
    r = {k: int(v) for k, v in (kv.split("=") for kv in out.split()[1:])}
    assert r["accepted"] + r["refused"] == CHAIN_WANT["total"] and r["ranges"] == CHAIN_WANT["ranges"], out
    assert r["refused"] == r["ranges"] + r["multiples"] + r["short"] and r["multiples"] > 0 and r["short"] > 0 and r["accepted"] > 0, out
    rc, out = run_check(exe, "late")
    assert rc == 1 and out.startswith("VIOLATED code: n_chains 1 K 3 "), out


def test_the_chain_check_runs_clean_under_the_sanitizers(tmp_path_factory):
    """The stand-alone program with -fsanitize=address,undefined, on the CPU: nothing is preloaded."""
    exe = build_check(tmp_path_factory.mktemp("chain_check_san"), "chain_check_san",
                      ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"])
    rc, out = run_check(exe)
    assert rc == 0 and out.startswith("OK "), out
