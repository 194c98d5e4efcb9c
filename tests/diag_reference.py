"""The definition of the convergence diagnostics (include/spamtree_hip.h, st_*_diagnostics) restated twice, sharing no code with
the library: in np.longdouble for every output, and in exact rationals (fractions.Fraction) for everything up to tau and rhat^2.

For a series x_0 .. x_{K-1}, K >= 4:
  m = (1/K) sum x_s;  d_s = x_s - m;  gamma_t = (1/K) sum_{s=0}^{K-1-t} d_s d_{s+t};  sd = sqrt(K/(K-1) gamma_0);  rho_t = gamma_t / gamma_0
  L = min(max_lag, K - 2), max_lag = 0 meaning 1024;  k_max = (L - 1) // 2
  Gamma_k = rho_2k + rho_2k+1, k = 0 .. k_max;  stop at the first k with not (Gamma_k > 0);  otherwise Gamma_k <- min(Gamma_k, Gamma_k-1)
  tau = -1 + 2 sum Gamma_k, floored at 1 / log10 K;  ess = K / tau;  mcse = sd / sqrt(ess);  lags = 2 x pairs added
  truncated: the loop ended at k_max without a non-positive pair
  h = K // 2; halves x[:h], x[K-h:]; W = (s1^2 + s2^2) / 2 (divisor h - 1); B = h ((m1 - mb)^2 + (m2 - mb)^2); rhat^2 = ((h-1)/h W + B/h) / W
  gamma_0 == 0: ess = NaN, mcse = 0, sd = 0, rhat = NaN, lags = 0;  W == 0: rhat = NaN.
"""
import math
from fractions import Fraction

import numpy as np

DEFAULT_MAX_LAG = 1024
LD = np.longdouble


def lag_cap(K, max_lag=0):
    L = min(max_lag if max_lag else DEFAULT_MAX_LAG, K - 2)
    return L, (L - 1) // 2


def exact(x, max_lag=0):
    """Exact rationals: dict(gamma0, tau_raw (before the floor; None for a constant series), rhat2 (None where W == 0), pairs,
    truncated, gammas = the Gamma_k visited, the stopping one included, before the monotone rule)."""
    x = [Fraction(float(v)) for v in x]
    K = len(x)
    L, k_max = lag_cap(K, max_lag)
    m = sum(x) / K
    d = [v - m for v in x]
    g0 = sum(v * v for v in d) / K
    if g0 == 0:
        return dict(gamma0=g0, tau_raw=None, rhat2=None, pairs=0, truncated=False, gammas=[])

    def rho(t):
        return sum(d[s] * d[s + t] for s in range(K - t)) / K / g0
    tsum, prev, pairs, gammas = Fraction(0), None, 0, []
    for k in range(k_max + 1):
        G = rho(2 * k) + rho(2 * k + 1)
        gammas.append(G)
        if not G > 0:
            break
        if prev is not None:
            G = min(G, prev)
        prev = G
        tsum += G
        pairs += 1
    h = K // 2
    a, b = x[:h], x[K - h:]
    m1, m2 = sum(a) / h, sum(b) / h
    s1 = sum((v - m1) ** 2 for v in a) / (h - 1)
    s2 = sum((v - m2) ** 2 for v in b) / (h - 1)
    W = (s1 + s2) / 2
    mb = (m1 + m2) / 2
    B = h * ((m1 - mb) ** 2 + (m2 - mb) ** 2)
    rhat2 = (Fraction(h - 1, h) * W + B / h) / W if W != 0 else None
    return dict(gamma0=g0, tau_raw=2 * tsum - 1, rhat2=rhat2, pairs=pairs, truncated=pairs == k_max + 1, gammas=gammas)


def exact_outputs(x, max_lag=0):
    """The five outputs from the exact rationals, rounded to float once each (the floor and the square roots in long double)."""
    e = exact(x, max_lag)
    K = len(x)
    if e["gamma0"] == 0:
        return dict(ess=math.nan, mcse=0.0, sd=0.0, rhat=math.nan, lags=0, truncated=False)
    floor = 1 / np.log10(LD(K))
    tau = max(LD(e["tau_raw"].numerator) / LD(e["tau_raw"].denominator), floor)
    ess = LD(K) / tau
    g = e["gamma0"] * K / (K - 1)
    sd = np.sqrt(LD(g.numerator) / LD(g.denominator))
    r2 = e["rhat2"]
    rhat = float(np.sqrt(LD(r2.numerator) / LD(r2.denominator))) if r2 is not None else math.nan
    return dict(ess=float(ess), mcse=float(sd / np.sqrt(ess)), sd=float(sd), rhat=rhat, lags=2 * e["pairs"], truncated=e["truncated"])


def _mean(x):
    """The mean in long double, to the rounding of the spread (not of the offset): math.fsum's correctly rounded sum first."""
    m0 = LD(math.fsum(float(v) for v in x)) / LD(x.size)
    return m0 + (x - m0).sum() / LD(x.size)


def reference(x, max_lag=0):
    """Long double: dict(ess, mcse, sd, rhat, lags, truncated) as floats plus what a test's error bound needs: tau (floored), tsum
    (the sum of the pairs added), pairs, min_abs_gamma (the smallest |Gamma_k| over the pairs visited, the stopping one
    included, before the monotone rule; inf for a constant series), gamma0, max_abs_x, max_abs_d, W, dmu = |m1 - m2|."""
    x = np.asarray(x, dtype=np.float64).astype(LD)
    K = x.size
    L, k_max = lag_cap(K, max_lag)
    d = x - _mean(x)
    g0 = (d @ d) / LD(K)
    extra = dict(gamma0=float(g0), max_abs_x=float(np.abs(x).max()), max_abs_d=float(np.abs(d).max()))
    if g0 == 0:
        return dict(ess=math.nan, mcse=0.0, sd=0.0, rhat=math.nan, lags=0, truncated=False, tau=math.nan, tsum=0.0, pairs=0,
                    min_abs_gamma=math.inf, W=0.0, dmu=0.0, **extra)
    sd = np.sqrt(LD(K) / LD(K - 1) * g0)
    tsum, prev, pairs, mag = LD(0), LD(np.inf), 0, math.inf
    for k in range(k_max + 1):
        t = 2 * k
        G = (d[:K - t] @ d[t:]) / LD(K) / g0 + (d[:K - t - 1] @ d[t + 1:]) / LD(K) / g0
        mag = min(mag, abs(float(G)))
        if not G > 0:
            break
        G = min(G, prev)
        prev = G
        tsum += G
        pairs += 1
    tau = max(2 * tsum - 1, 1 / np.log10(LD(K)))
    ess = LD(K) / tau
    h = K // 2
    a, b = x[:h], x[K - h:]
    m1, m2 = _mean(a), _mean(b)
    s1 = ((a - m1) @ (a - m1)) / LD(h - 1)
    s2 = ((b - m2) @ (b - m2)) / LD(h - 1)
    W = (s1 + s2) / 2
    mb = (m1 + m2) / 2
    B = h * ((m1 - mb) ** 2 + (m2 - mb) ** 2)
    rhat = float(np.sqrt((LD(h - 1) / LD(h) * W + B / h) / W)) if W != 0 else math.nan
    return dict(ess=float(ess), mcse=float(sd / np.sqrt(ess)), sd=float(sd), rhat=rhat, lags=2 * pairs, truncated=pairs == k_max + 1,
                tau=float(tau), tsum=float(tsum), pairs=pairs, min_abs_gamma=mag, W=float(W), dmu=float(abs(m1 - m2)), **extra)


def ar1(K, phi, seed, scale=1.0, offset=0.0):
    """A stationary AR(1) series of K values (phi = 0: white noise)."""
    rng = np.random.default_rng(seed)
    e = rng.standard_normal(K)
    x = np.empty(K)
    x[0] = e[0] / math.sqrt(1.0 - phi * phi)
    for s in range(1, K):
        x[s] = phi * x[s - 1] + e[s]
    return offset + scale * x
