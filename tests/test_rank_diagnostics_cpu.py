"""CPU: the rank-normalised diagnostics (include/spamtree_hip.h, st_*_rank_diagnostics) without a device.

1. The normal quantile function of spamtree_amd/csrc/norm_quantile.hpp -- the text the device runs -- built into
   tests/rank_norm_check.cpp by the host compiler alone, against 50-digit arithmetic (tests/rank_reference.norm_ppf) at every
   argument the rank scores use for K = 4, 5, 64, 1000 and 16384.  The bound is reasoned (PHI_BOUND below); the largest error met is
   printed, and must not exceed the recorded figure the GPU tests double (rank_reference.PHI_ERR_MEASURED).
2. The host function spamtree_amd.diagnostics.rank_series_diagnostics against tests/rank_reference.py on the hand series.
   Integer-defined outputs (ess_q, ess_tail, ess_exc, prob, mcse_prob, their lags) within 1e-14 relative and exactly; the
   score-defined ones (rhat_*, ess_bulk) within rank_reference.score_bounds with depth K (any summation order of K terms) and
   the Phi^-1 term.
"""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from spamtree_amd import diagnostics as dg
from tests import rank_reference as rr
from tests.diag_reference import ar1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spamtree_amd", "csrc")
U = 2.0 ** -53
# Wichura states about 1e-16 for the approximations themselves.  Rounding: num and den are Horner chains of degree 7 with positive
# coefficients and a positive argument, 14 operations each, so each is within 14 u and their quotient within 28 u + u; q * num one
# more; the argument r = sqrt(-log t) - 1.6 (or 0.180625 - q^2) carries the rounding of log, sqrt and one subtraction, at most 4 u
# of r's scale before the subtraction, which moves z by no more than about that relative amount (dz/dr is of order z / r): 36 u.
PHI_BOUND = 1e-16 + 36 * U
INT_RTOL = 1e-14
KS = (4, 5, 64, 1000, 16384)


def close(a, b, rtol=INT_RTOL):
    return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= rtol * abs(b)


@pytest.fixture(scope="module")
def norm_check(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    exe = str(tmp_path_factory.mktemp("rank_norm") / "rank_norm_check")
    subprocess.run([hipcc, "--offload-host-only", "-std=c++17", "-O1", "-I", CSRC, os.path.join(ROOT, "tests", "rank_norm_check.cpp"),
                    "-o", exe], check=True, timeout=600)
    return exe


def test_norm_quantile_against_50_digits(norm_check):
    out = subprocess.run([norm_check] + [str(K) for K in KS], capture_output=True, text=True, check=True, timeout=600).stdout.splitlines()
    assert out[-1].startswith("edge")
    edge = out[-1].split()[1:]
    assert edge[0] == "-inf" and edge[1] == "inf" and float.fromhex(edge[2]) == 0.0 and edge[8].endswith("nan") and edge[9].endswith("nan")
    points = (0.075, 0.925, 1e-20, 1e-12, 1.0 - 1e-12, None, None, 1e-11, 1e-15, 1e-30, 1e-60, 1e-120, 1e-300)
    for tok, p in zip(edge[3:], points):   # both region boundaries and the far tails (r > 5: beyond what the rank scores reach)
        if p is None:
            continue
        z, want = float.fromhex(tok), rr.norm_ppf(p)
        assert abs((rr.mp.mpf(z) - want) / want) <= PHI_BOUND, (p, z)
    worst = {K: 0.0 for K in KS}
    lines = out[:-1]
    assert len(lines) == sum(2 * K - 1 for K in KS)
    for ln in lines:
        K, r2, p, z = ln.split()
        K, r2, p, z = int(K), int(r2), float.fromhex(p), float.fromhex(z)
        assert p == float(4 * r2 - 3) / float(8 * K + 2)
        if 4 * r2 - 3 == 4 * K + 1:   # p = 1/2 exactly
            assert z == 0.0
            continue
        want = rr.norm_ppf(p)
        worst[K] = max(worst[K], float(abs((rr.mp.mpf(z) - want) / want)))
    print("largest relative error of Phi^-1 by K:", {K: f"{v:.3g}" for K, v in worst.items()})
    assert max(worst.values()) <= PHI_BOUND
    assert max(worst.values()) <= rr.PHI_ERR_MEASURED   # the recorded figure still holds
    # the library's host function is the same text: same bits
    ps = np.array([float.fromhex(ln.split()[2]) for ln in lines[:200]])
    zs = np.array([float.fromhex(ln.split()[3]) for ln in lines[:200]])
    assert dg.norm_quantile(ps).tobytes() == zs.tobytes()


def check_series(x, probs=(), thresholds=(), sides=None, max_lag=0):
    """The host function against the reference on one series; returns (host, reference)."""
    got = dg.rank_series_diagnostics(x, probs, thresholds, sides, max_lag)
    want = rr.reference(x, probs, thresholds, sides, max_lag)
    K = len(x)
    for k in range(len(probs)):
        assert close(got["ess_q"][k], want["ess_q"][k]) and got["lags_q"][k] == want["lags_q"][k], (k, got["ess_q"], want["ess_q"])
    for t in range(len(thresholds)):
        assert close(got["ess_exc"][t], want["ess_exc"][t]) and got["lags_exc"][t] == want["lags_exc"][t], (t, got["ess_exc"], want["ess_exc"])
        assert close(got["prob"][t], want["prob"][t], 0.0) and close(got["mcse_prob"][t], want["mcse_prob"][t]), (t, got["prob"], got["mcse_prob"])
    assert close(got["ess_tail"], want["ess_tail"])
    if want["bulk"] is None:   # a NaN draw
        assert all(math.isnan(got[k]) for k in ("rhat_rank", "rhat_bulk", "rhat_fold", "ess_bulk")) and got["lags_bulk"] == 0
        return got, want
    for part, keys in (("bulk", (("rhat_bulk", "rhat"), ("ess_bulk", "ess"))), ("fold", (("rhat_fold", "rhat"),))):
        rec = want[part]
        if rec["gamma0"] == 0.0:
            assert all(math.isnan(got[a]) for a, _ in keys)
            continue
        b = rr.score_bounds(rec, K, got["lags_bulk"] // 2, K, rr.PHI_ERR_MEASURED)
        for a, key in keys:
            if math.isnan(rec[key]):
                assert math.isnan(got[a]), (a, got[a])
            else:
                assert abs(got[a] - rec[key]) <= b[key] * abs(rec[key]), (a, got[a], rec[key], b[key])
    if want["bulk"]["min_abs_gamma"] > 1e-8:
        assert got["lags_bulk"] == want["lags_bulk"] and got["truncated"] == want["truncated"]
    assert close(got["rhat_rank"], rr.fmax(got["rhat_bulk"], got["rhat_fold"]), 0.0)
    return got, want


def test_zero_to_fifteen_ranks_are_the_identity():
    x = np.arange(16, dtype=np.float64)
    assert rr.twice_ranks(x) == [2 * s + 2 for s in range(16)]
    r2, z = dg.rank_scores(x)
    assert list(r2) == [2 * s + 2 for s in range(16)]
    for s in range(16):   # z is known: Phi^-1((8 s + 5) / 130)
        want = rr.norm_ppf(float(8 * s + 5) / 130.0)
        assert abs((rr.mp.mpf(float(z[s])) - want) / want) <= PHI_BOUND
    assert np.array_equal(z, -z[::-1])   # symmetric scores, bit for bit (1 - p is exact)
    got, _ = check_series(x, probs=(0.25, 0.5), thresholds=(7.5,))
    plain = dg.series_diagnostics(z)     # the outputs are the diagnostics applied to z
    assert got["rhat_bulk"] == plain["rhat"] and got["ess_bulk"] == plain["ess"] and got["lags_bulk"] == plain["lags"]
    assert got["rhat_bulk"] > 2.0        # a trend: the halves disagree


def test_tie_blocks_share_their_rank():
    x = rr.tie_blocks(10)
    assert list(x) == [1, 1, 2, 2, 2, 3, 3, 4, 4, 4]
    by_hand = [3, 3, 8, 8, 8, 13, 13, 18, 18, 18]   # lo + hi + 1: (0, 2), (2, 5), (5, 7), (7, 10)
    assert rr.twice_ranks(x) == by_hand and list(dg.rank_scores(x)[0]) == by_hand
    check_series(x, probs=(0.3, 0.5), thresholds=(2.0, 2.0), sides=(1, -1))
    check_series(rr.tie_blocks(257)[np.random.default_rng(3).permutation(257)], probs=(0.05, 0.5, 0.95), thresholds=(40.0,))


def test_two_valued_series():
    rng = np.random.default_rng(11)
    x = (rng.uniform(size=129) < 0.3).astype(np.float64) * 2.5 - 1.0
    c0 = int(np.count_nonzero(x < 0))
    assert set(rr.twice_ranks(x)) == {c0 + 1, c0 + 129 + 1}
    got, want = check_series(x, probs=(0.1, 0.5, 0.9), thresholds=(0.0, 0.0, 5.0), sides=(1, -1, 1))
    assert want["count"] == [129 - c0, c0, 0] and math.isnan(got["ess_exc"][2]) and got["mcse_prob"][2] == 0.0 and got["prob"][2] == 0.0
    # the quantile indicators of a two-valued series are that series or all ones
    assert math.isnan(got["ess_q"][2]) and got["lags_q"][2] == 0     # xs[j] is the upper value: c == K


def test_period_four_indicator_by_hand():
    I = [1, 1, 0, 0] * 4
    assert [rr.indicator_A(I, t) for t in range(4)] == [1024, 64, -896, -64]
    ess, lags, _ = rr.indicator_ess(I)
    assert lags == 2 and ess == 16 / 1.125       # pair 0 = 1.0625, pair 1 = -0.9375: tau = 1.125 above the floor 1 / log10 16
    assert dg.indicator_ess(I) == (16 / 1.125, 2)
    x = np.array(I, dtype=np.float64)
    got, _ = check_series(x, thresholds=(0.5,))
    assert got["ess_exc"][0] == 16 / 1.125 and got["prob"][0] == 0.5 and got["mcse_prob"][0] == math.sqrt(0.25 / (16 / 1.125))


def test_constants_and_a_nan_draw():
    got, _ = check_series(np.full(9, 3.25), probs=(0.5,), thresholds=(3.25, 0.0))
    assert all(math.isnan(got[k]) for k in ("rhat_rank", "rhat_bulk", "rhat_fold", "ess_bulk", "ess_tail")) and got["lags_bulk"] == 0
    assert math.isnan(got["ess_q"][0]) and list(got["prob"]) == [0.0, 1.0] and list(got["mcse_prob"]) == [0.0, 0.0]
    x = ar1(20, 0.5, seed=1)
    x[7] = math.nan
    got, _ = check_series(x, probs=(0.5,), thresholds=(0.0,))
    assert math.isnan(got["ess_q"][0]) and math.isnan(got["prob"][0]) and math.isnan(got["mcse_prob"][0]) and got["lags_exc"][0] == 0


@pytest.mark.parametrize("K", [4, 5])
def test_shortest_series(K):
    for seed in range(4):
        check_series(ar1(K, 0.3, seed=seed), probs=(0.05, 0.5, 0.95), thresholds=(0.0,), max_lag=seed % 3)


def test_prob_at_both_clamps():
    K = 64
    x = ar1(K, 0.6, seed=5)
    xs = np.sort(x)
    assert rr.quantile_order(1e-9, K) == 0 and dg.quantile_order(1e-9, K) == 0                  # ceil(prob K) = 1
    assert rr.quantile_order(1 - 1e-9, K) == K - 2 and dg.quantile_order(1 - 1e-9, K) == K - 2  # ceil = K, clamped to K - 1
    assert dg.quantile_order(0.5, K) == 31 and dg.quantile_order(1.0 / K, K) == 0 and dg.quantile_order(1.5 / K, K) == 1
    got, want = check_series(x, probs=(1e-9, 1 - 1e-9, 0.5))
    assert dg.indicator_ess(x <= xs[0])[0] == got["ess_q"][0] and dg.indicator_ess(x <= xs[K - 2])[0] == got["ess_q"][1]
    assert not math.isnan(got["ess_q"][0]) and not math.isnan(got["ess_q"][1])   # c = 1 and c = K - 1: neither degenerate


def test_monotone_invariance():
    x = ar1(400, 0.7, seed=9)
    maps = (x, np.exp(x), 1e3 + 1e-6 * x)
    assert all(rr.twice_ranks(m) == rr.twice_ranks(x) for m in maps)   # strictly monotone in floating point: no new ties
    outs = [dg.rank_series_diagnostics(m, probs=(0.1, 0.5, 0.9)) for m in maps]
    for o in outs[1:]:
        for k in ("rhat_bulk", "ess_bulk", "ess_tail", "lags_bulk"):
            assert np.array([o[k]]).tobytes() == np.array([outs[0][k]]).tobytes(), k
        assert o["ess_q"].tobytes() == outs[0]["ess_q"].tobytes()
    assert outs[0]["ess_bulk"] < 400 and outs[0]["lags_bulk"] > 2


def test_split_scale_series_is_seen_by_the_folded_rhat_only():
    x = rr.split_scale_cauchy(1000, seed=2)
    got, want = check_series(x, probs=(0.05, 0.95))
    plain = dg.series_diagnostics(x)
    from tests.diag_reference import reference as plain_reference
    pr = plain_reference(x)
    assert abs(plain["rhat"] - pr["rhat"]) <= 1e-10 * pr["rhat"]
    assert want["rhat_fold"] > 1.05 and want["rhat_fold"] > want["rhat_bulk"] and want["rhat_fold"] > pr["rhat"]
    assert got["rhat_fold"] > got["rhat_bulk"] and got["rhat_fold"] > plain["rhat"] and got["rhat_rank"] == got["rhat_fold"]
    assert want["rhat_bulk"] < 1.01


def test_ar1_and_lag_caps_against_the_reference():
    for phi, K, max_lag in ((-0.9, 63, 0), (0.9, 129, 7), (0.99, 257, 0), (0.0, 65, 1), (0.5, 64, 64)):
        check_series(ar1(K, phi, seed=K), probs=(0.025, 0.5, 0.975), thresholds=(0.0, 1.0), sides=(1, -1), max_lag=max_lag)
    alt = np.where(np.arange(64) % 2 == 0, 1.0, -1.0)
    got, want = check_series(alt, thresholds=(0.0,), max_lag=64)
    assert want["lags_exc"][0] == 62 and got["lags_exc"][0] == 62   # every pair is 1/64 > 0: the lag cap is reached


def test_value_errors():
    x = ar1(16, 0.2, seed=1)
    for kw in (dict(max_lag=-1), dict(probs=[0.1] * 9), dict(probs=(0.0,)), dict(probs=(1.0,)), dict(probs=(math.nan,)),
               dict(thresholds=[0.0] * 9), dict(thresholds=(math.nan,)), dict(thresholds=(math.inf,)), dict(thresholds=(0.0,), sides=(0,)),
               dict(thresholds=(0.0, 1.0), sides=(1, 1, 1))):
        with pytest.raises(ValueError):
            dg.rank_series_diagnostics(x, **kw)
    with pytest.raises(ValueError):
        dg.rank_series_diagnostics(x[:3])
    with pytest.raises(ValueError):
        dg.rank_series_diagnostics(np.zeros(dg.MAX_DRAWS + 1))
    with pytest.raises(ValueError):
        dg.summarise_rank(dict(rhat_rank=np.ones(3), ess_bulk=np.ones(3), ess_tail=np.ones(3)), mv=[1, 2])


def test_summarise_rank():
    a = np.stack([ar1(200, phi, seed=i) for i, phi in enumerate((0.0, 0.9, 0.5, 0.95))] + [np.full(200, 2.0)])
    d = dg.chains_rank_diagnostics(a, probs=(0.5,), thresholds=(0.0,))
    assert d["ess_q"].shape == (1, 5) and d["prob"].shape == (1, 5) and d["truncated"].dtype == bool and d["lags_bulk"].dtype == np.int32
    s = dg.summarise_rank(d, mv=[1, 1, 2, 2, 2])
    ok = ~np.isnan(d["ess_bulk"])
    assert s["n"] == 5 and s["max_rhat_rank"] == np.nanmax(d["rhat_rank"]) and s["min_ess_bulk"] == d["ess_bulk"][ok].min()
    assert s["median_ess_tail"] == float(np.median(d["ess_tail"][ok])) and s["min_ess_tail"] == d["ess_tail"][ok].min()
    assert s["n_low_ess_bulk"] == int(np.count_nonzero(d["ess_bulk"][ok] < dg.ESS_LOW))
    assert s["n_low_ess_tail"] == int(np.count_nonzero(d["ess_tail"][ok] < dg.ESS_LOW))
    assert set(s["by_outcome"]) == {1, 2} and s["by_outcome"][2]["n"] == 3 and s["by_outcome"][1]["median_ess_bulk"] == float(np.median(d["ess_bulk"][:2]))
    empty = dg.summarise_rank(dict(rhat_rank=np.array([math.nan]), ess_bulk=np.array([math.nan]), ess_tail=np.array([math.nan])))
    assert empty["n"] == 1 and math.isnan(empty["max_rhat_rank"]) and empty["n_low_ess_bulk"] == 0


def test_fit_refuses_before_any_device_call():
    from spamtree_amd import fit
    from tests.util import make_problem
    args = [None] * 20
    for kw in (dict(rank_diagnostics=True, criteria=True), dict(rank_diagnostics=True, y_holdout=np.zeros(3)),
               dict(rank_diagnostics=True, mcmc_keep=3), dict(rank_diagnostics=True, mcmc_keep=16385),
               dict(rank_diagnostics=dict(probs=[0.5] * 9), mcmc_keep=5), dict(rank_diagnostics=dict(probs=[1.0]), mcmc_keep=5),
               dict(rank_diagnostics=dict(thresholds=[0.0] * 9), mcmc_keep=5), dict(rank_diagnostics=dict(thresholds=[np.nan]), mcmc_keep=5),
               dict(rank_diagnostics=dict(thresholds=[0.0], sides=[2]), mcmc_keep=5), dict(rank_diagnostics=dict(max_lag=-1), mcmc_keep=5),
               dict(rank_diagnostics=dict(level=0.1), mcmc_keep=5)):
        with pytest.raises(ValueError):
            fit.spamtree_mv_mcmc(*args, **kw)
    # the shapes need the problem, still no device: two values for one outcome, thresholds_fun without points
    pb = make_problem(side=8, q=1, seed=1)
    k = pb["theta"].size
    real = (pb["y"], pb["X"], pb["Z"], pb["coords"], pb["mv_id"], pb["blocking"], pb["gix_block"], pb["res_is_ref"], pb["parents"],
            pb["children"], bool(pb["limited_tree"]), pb["block_names"], pb["block_groups"], pb["indexing"], pb["bounds"],
            np.zeros(pb["n"]), pb["theta"], np.zeros(pb["p"]), 0.1, 0.02 * np.eye(k))
    for x in (dict(thresholds=[[0.0, 1.0]]), dict(thresholds=[0.0], thresholds_fun=[1.0])):
        with pytest.raises(ValueError):
            fit.spamtree_mv_mcmc(*real, rank_diagnostics=x, mcmc_keep=5, mcmc_burn=1, main_verbose=False)


def test_driver_refuses_before_the_first_factorisation():
    """stm_mcmc_ranked returns its refusals before it creates the chain: no device is touched, so they are checked here.  Only the
    problem's q is read; every other argument may be NULL."""
    import ctypes as C
    from spamtree_amd import _lib
    from spamtree_amd.model import rank_buffers, rank_spec
    from tests.util import make_problem, problem_arrays, st_problem_struct
    lib = _lib.load()
    a = problem_arrays(make_problem(side=8, q=1, seed=1))
    pb = st_problem_struct(a)
    n = int(a["n_all"])

    def run(keep, probs=(0.5,), thr=(0.0,), sides=(1,), want_rows=1, new=False, fun=False, tweak=None):
        spec, hold, n_prob, n_thr = rank_spec(probs, thr, sides, 0, 1)
        if tweak:
            tweak(spec)
        d, o = rank_buffers(n, max(n_prob, 1), max(n_thr, 1))
        rs = _lib.StmRankDiagnostics()
        rs.want_rows = want_rows
        rs.rows_spec = spec
        rs.rows_w = o
        if new:
            rs.new_w = o
        if fun:
            rs.fun_w = o
        common = (C.byref(pb), None, None, None, 4, None, 0.1, None, keep, 1, 1, 1, None, None, None, None, None, None, None, None)
        return lib.stm_mcmc_ranked(*common, 0, None, None, None, None, None, 0, None, 0, *([None] * 15), None, None, C.byref(rs))

    assert run(16385) == -4                                             # ST_ERR_UNSUPPORTED: the stores' limit
    assert run(3) == -1                                                 # fewer than ST_DIAG_MIN_DRAWS
    assert run(5, want_rows=0) == -1 and run(5, new=True) == -1 and run(5, fun=True) == -1   # outputs without their set
    assert run(5, probs=()) == -1 and run(5, thr=(), sides=None) == -1  # ess_q without prob, exceedance outputs without thr
    for tweak in (lambda s: setattr(s, "max_lag", -1), lambda s: setattr(s, "n_prob", 9), lambda s: setattr(s, "n_thr", 9),
                  lambda s: setattr(s, "n_prob", -1), lambda s: setattr(s, "n_thr", -1)):
        assert run(5, tweak=tweak) == -1
    bad_p, bad_t, bad_s = np.array([1.0]), np.array([np.inf]), np.array([0], dtype=np.int32)
    dp = C.POINTER(C.c_double)
    assert run(5, tweak=lambda s: setattr(s, "prob", bad_p.ctypes.data_as(dp))) == -1
    assert run(5, tweak=lambda s: setattr(s, "thr", bad_t.ctypes.data_as(dp))) == -1
    assert run(5, tweak=lambda s: setattr(s, "side", bad_s.ctypes.data_as(C.POINTER(C.c_int32)))) == -1
