"""CPU: spamtree_amd.diagnostics (the float64 restatement used for the scalar chains) against the exact rationals of
tests/diag_reference.py on hand series, against an FFT autocovariance on random AR(1) series, the continuity of ess in the data,
the ValueErrors of fit.spamtree_mv_mcmc(diagnostics=True) and summarise on a worked example."""
import math
from fractions import Fraction

import numpy as np
import pytest

from spamtree_amd import diagnostics as dg
from tests import diag_reference as ref

U = 2.0 ** -53


def close(got, want, rel):
    if isinstance(want, float) and math.isnan(want):
        return isinstance(got, float) and math.isnan(got)
    return abs(got - want) <= rel * abs(want)


def assert_matches_exact(x, max_lag=0, rel=None):
    """series_diagnostics == the exact rationals' outputs.  Bound: float64 dot products over K terms of a series whose values
    are O(max|d|): each gamma_t within (K + 4) U sum |d_s d_{s+t}| <= (K + 4) U K gamma_0, so each rho within 2 (K + 4) U, tau
    within 4 pairs (K + 4) U, relative to tau >= 1 / log10 K; a factor 4 covers the centring and the final operations."""
    x = np.asarray(x, dtype=np.float64)
    K = x.size
    got, want = dg.series_diagnostics(x, max_lag), ref.exact_outputs(x, max_lag)
    if rel is None:
        rel = 16 * (want["lags"] // 2 + 2) * (K + 4) * U * math.log10(K) * max(1.0, float(np.abs(x).max()) / max(want["sd"], 1e-300))
    assert got["lags"] == want["lags"] and got["truncated"] == want["truncated"], (got, want)
    for k in ("ess", "mcse", "sd", "rhat"):
        assert close(got[k], want[k], rel), (k, got[k], want[k], rel)
    return got, want


def test_alternating_series_reaches_the_floor_and_is_truncated():
    x = np.array([1.0, -1.0] * 32)
    e = ref.exact(x)
    assert e["gammas"] == [Fraction(1, 64)] * 31 and e["pairs"] == 31 and e["truncated"]
    assert e["tau_raw"] == Fraction(62, 64) - 1
    got, _ = assert_matches_exact(x)
    assert got["lags"] == 62 and got["truncated"]
    assert close(got["ess"], 64 * math.log10(64), 4 * U)


def test_linear_trend_0_to_15():
    x = np.arange(16.0)
    got, want = assert_matches_exact(x)
    assert got["lags"] == 6 and not got["truncated"]
    assert abs(want["ess"] - 2.8669) < 1e-4 and abs(want["rhat"] - 2.4917) < 1e-4
    # rhat^2 by hand: h = 8, W = 6, B = 8 * 2 * 16 = 256: (7/8 * 6 + 32) / 6
    assert ref.exact(x)["rhat2"] == (Fraction(7, 8) * 6 + 32) / 6


@pytest.mark.parametrize("c", [0.0, 0.1, -1e3, 1e-300])
@pytest.mark.parametrize("K", [4, 63, 1000])
def test_constant_series(c, K):
    got = dg.series_diagnostics(np.full(K, c))
    assert math.isnan(got["ess"]) and math.isnan(got["rhat"]) and got["mcse"] == 0.0 and got["sd"] == 0.0 and got["lags"] == 0
    assert not got["truncated"]
    assert ref.exact_outputs(np.full(K, c))["lags"] == 0 and ref.reference(np.full(K, c))["sd"] == 0.0


def test_constant_halves_have_no_rhat_only():
    x = np.array([1.0] * 5 + [3.0] * 5)
    got, want = assert_matches_exact(x)
    assert math.isnan(got["rhat"]) and got["sd"] > 0 and got["ess"] > 0


@pytest.mark.parametrize("K", [4, 5])
def test_shortest_series_and_the_odd_split(K):
    rng = np.random.default_rng(K)
    for _ in range(20):
        x = rng.standard_normal(K)
        assert_matches_exact(x)
    x = np.array([0.3, -1.2, 2.5, 0.1, 0.9][:K])
    e = ref.exact(x)
    h = K // 2
    a, b = [Fraction(float(v)) for v in x[:h]], [Fraction(float(v)) for v in x[K - h:]]   # K = 5: the middle draw is in neither
    m1, m2 = sum(a) / h, sum(b) / h
    W = (sum((v - m1) ** 2 for v in a) + sum((v - m2) ** 2 for v in b)) / (h - 1) / 2
    assert e["rhat2"] == (Fraction(h - 1, h) * W + (m1 - m2) ** 2 / 2) / W
    assert ref.lag_cap(K) == (K - 2, (K - 3) // 2)


@pytest.mark.parametrize("max_lag", [1, 2, 7, 0, 10 ** 6])
def test_lag_cap(max_lag):
    x = ref.ar1(300, 0.95, seed=3)
    got, want = assert_matches_exact(x, max_lag)
    L, k_max = ref.lag_cap(300, max_lag)
    assert L == min(max_lag if max_lag else 1024, 298) and got["lags"] <= 2 * (k_max + 1)
    if max_lag in (1, 2):
        assert got["lags"] == 2 and got["truncated"]        # one pair, rho_0 + rho_1 > 0: the cap is all that stops it
    with pytest.raises(ValueError):
        dg.series_diagnostics(x, -1)
    with pytest.raises(ValueError):
        dg.series_diagnostics(x[:3])


def _fft_diag(x, max_lag=0):
    K = x.size
    d = x - x.mean()
    f = np.fft.rfft(d, 2 * K)
    g = np.fft.irfft(f * np.conj(f))[:K] / K
    rho = g / g[0]
    _, k_max = ref.lag_cap(K, max_lag)
    tsum, prev, pairs, mag = 0.0, math.inf, 0, math.inf
    for k in range(k_max + 1):
        G = rho[2 * k] + rho[2 * k + 1]
        mag = min(mag, abs(G))
        if not G > 0:
            break
        G = min(G, prev)
        prev = G
        tsum += G
        pairs += 1
    tau = max(2 * tsum - 1, 1 / math.log10(K))
    return K / tau, 2 * pairs, mag


@pytest.mark.parametrize("phi", [-0.9, -0.5, 0.0, 0.3, 0.7, 0.9, 0.99])
def test_against_an_fft_autocovariance(phi):
    """The FFT gives every gamma_t within a few 2^-53 log2(2K) K gamma_0 of the direct sums: 1e-10 on ess is far above that and
    far below any error of the definition (a wrong lag, a missed term, a wrong divisor).  Where the deciding pair is within 1e-8
    of zero the two may stop at different pairs; ess is continuous, lags is compared elsewhere only."""
    for K in (4, 5, 17, 64, 129, 1000):
        for seed in range(4):
            x = ref.ar1(K, phi, seed=1000 * seed + K)
            got = dg.series_diagnostics(x)
            ess, lags, mag = _fft_diag(x)
            assert abs(got["ess"] - ess) <= 1e-10 * ess * (got["lags"] + 2), (K, seed, got, ess)
            if mag > 1e-8:
                assert got["lags"] == lags
            want = ref.reference(x)
            assert abs(got["ess"] - want["ess"]) <= 1e-11 * want["ess"] * (got["lags"] + 2)
            assert abs(got["rhat"] - want["rhat"]) <= 1e-11 * want["rhat"] and abs(got["sd"] - want["sd"]) <= 1e-13 * want["sd"]


def test_ess_is_continuous_where_the_deciding_pair_crosses_zero():
    """Two series that differ by a perturbation of 1e-13 and whose deciding pair has opposite signs: without the monotone rule tau
    would jump by the pairs behind it; with it every later pair is capped by the deciding one, so tau moves by at most
    2 (pairs left) x that pair, plus what 1e-13 moves the sums themselves."""
    x = ref.ar1(200, 0.5, seed=13)
    v = np.random.default_rng(12).standard_normal(200)
    k0 = dg.series_diagnostics(x)["lags"] // 2

    def pairs(eps):   # of the function under test: the two sides of ITS decision
        return dg.series_diagnostics(x + eps * v)["lags"] // 2

    lo, hi = 0.0, None
    for eps in np.linspace(0.05, 5.0, 100):
        if pairs(eps) != k0:
            hi = eps
            break
        lo = eps
    assert hi is not None
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if pairs(mid) != k0:
            hi = mid
        else:
            lo = mid
    assert hi - lo < 1e-13
    a, b = dg.series_diagnostics(x + lo * v), dg.series_diagnostics(x + hi * v)
    assert a["lags"] == 2 * k0 and b["lags"] != a["lags"]
    k_c = min(a["lags"], b["lags"]) // 2             # the pair that crosses: positive in one series, not in the other
    g = max(abs(float(ref.exact(x + e * v)["gammas"][k_c])) for e in (lo, hi))
    assert g < 1e-10
    _, k_max = ref.lag_cap(200)
    tau_a, tau_b = 200 / a["ess"], 200 / b["ess"]
    assert abs(tau_b - tau_a) <= 2 * (k_max + 1) * g + 1e-10
    assert abs(a["ess"] - b["ess"]) <= 1e-8 * a["ess"]


def test_fit_refuses_before_any_device_call():
    from spamtree_amd import fit
    args = [None] * 20
    for kw in (dict(criteria=True), dict(y_holdout=np.zeros(3)), dict(mcmc_keep=3), dict(mcmc_keep=16385), dict(mcmc_keep=0),
               dict(diagnostics_max_lag=-1)):
        with pytest.raises(ValueError):
            fit.spamtree_mv_mcmc(*args, diagnostics=True, **kw)


def test_summarise_worked_example():
    d = dict(ess=np.array([50.0, 400.0, np.nan, 150.0]), mcse=np.array([0.2, 0.05, 0.0, 0.1]), sd=np.array([1.0, 1.0, 0.0, 2.0]),
             rhat=np.array([1.2, 1.0, np.nan, 1.05]), truncated=np.array([True, False, False, False]))
    s = dg.summarise(d, mv=np.array([1, 1, 2, 2]))
    assert s["n"] == 4 and s["min_ess"] == 50.0 and s["median_ess"] == 150.0 and s["max_rhat"] == 1.2
    assert s["max_mcse_over_sd"] == 0.2 and s["n_truncated"] == 1 and s["n_constant"] == 1 and s["n_low_ess"] == 1
    assert s["by_outcome"][1] == dict(n=2, min_ess=50.0, median_ess=225.0, max_rhat=1.2, max_mcse_over_sd=0.2, n_truncated=1,
                                      n_constant=0, n_low_ess=1)
    assert s["by_outcome"][2]["n_constant"] == 1 and s["by_outcome"][2]["min_ess"] == 150.0 and s["by_outcome"][2]["max_rhat"] == 1.05
    c = dg.chains_diagnostics(np.stack([ref.ar1(100, 0.5, 1), np.full(100, 2.0)]))
    assert c["ess"].shape == (2,) and math.isnan(c["ess"][1]) and c["lags"].dtype == np.int32
    assert dg.summarise(c)["n_constant"] == 1
    assert np.array_equal(dg.truncated(np.array([62, 6]), 64), [True, False])
