"""Convergence diagnostics of one chain's saved draws, on the host, for the scalar chains (theta, beta, tausq): the definition of
include/spamtree_hip.h (st_*_diagnostics) restated in float64 -- the latent field's rows, the new points and the functionals get
theirs on the device from the same definition (spamtree_amd/csrc/diag_kernels.hpp).  NumPy only.

For a series x_0 .. x_{K-1}, K >= 4:
  m = mean(x);  d = x - m;  gamma_t = (1/K) sum_{s <= K-1-t} d_s d_{s+t};  sd = sqrt(K/(K-1) gamma_0);  rho_t = gamma_t / gamma_0
  L = min(max_lag, K - 2) (max_lag = 0: DEFAULT_MAX_LAG);  k_max = (L - 1) // 2
  Gamma_k = rho_2k + rho_2k+1 for k = 0 .. k_max;  stop at the first k with not (Gamma_k > 0);  else Gamma_k = min(Gamma_k, Gamma_k-1)
  tau = max(-1 + 2 sum Gamma_k, 1 / log10 K);  ess = K / tau;  mcse = sd / sqrt(ess);  lags = 2 x pairs added
  truncated: lags == 2 (k_max + 1) -- the loop ran into the lag cap, ess is an overestimate
  split-R-hat: h = K // 2, halves x[:h] and x[K-h:], W = mean of the half sample variances (divisor h - 1),
               B = h sum (m_j - mb)^2, rhat = sqrt(((h-1)/h W + B/h) / W)
  gamma_0 == 0: ess = NaN, mcse = 0, sd = 0, rhat = NaN, lags = 0;  W == 0: rhat = NaN."""
from __future__ import annotations

import math

import numpy as np

MIN_DRAWS = 4            # include/spamtree_hip.h: ST_DIAG_MIN_DRAWS
DEFAULT_MAX_LAG = 1024   # ST_DIAG_DEFAULT_MAX_LAG: a design constant bounding the cost per series
MAX_DRAWS = 16384        # the stores' limit (st_summary_reserve)
ESS_LOW = 100.0          # summarise() counts the series below it

KEYS = ("ess", "mcse", "sd", "rhat", "lags")


def lag_cap(K, max_lag=0):
    """(L, k_max) of a series of K draws."""
    if max_lag < 0:
        raise ValueError("max_lag must not be negative (0: the default cap)")
    L = min(int(max_lag) if max_lag else DEFAULT_MAX_LAG, K - 2)
    return L, (L - 1) // 2


def _mean(x):
    m0 = x.sum() / x.size
    return m0 + (x - m0).sum() / x.size   # to the rounding of the spread: a constant series centres to 0 exactly


def series_diagnostics(x, max_lag=0):
    """dict(ess, mcse, sd, rhat, lags, truncated) of one series of at least MIN_DRAWS draws, in float64."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    K = x.size
    if K < MIN_DRAWS:
        raise ValueError(f"the diagnostics need at least {MIN_DRAWS} draws, got {K}")
    L, k_max = lag_cap(K, max_lag)
    d = x - _mean(x)
    g0 = float(d @ d)
    if g0 == 0.0:
        return dict(ess=math.nan, mcse=0.0, sd=0.0, rhat=math.nan, lags=0, truncated=False)
    sd = math.sqrt(g0 / (K - 1))
    h = K // 2
    d1, d2 = d[:h], d[K - h:]
    mu1, mu2 = d1.sum() / h, d2.sum() / h
    W = (float((d1 - mu1) @ (d1 - mu1)) / (h - 1) + float((d2 - mu2) @ (d2 - mu2)) / (h - 1)) / 2.0
    mb = (mu1 + mu2) / 2.0
    B = h * ((mu1 - mb) ** 2 + (mu2 - mb) ** 2)
    rhat = math.sqrt(((h - 1) / h * W + B / h) / W) if W != 0.0 else math.nan
    tsum, prev, pairs = 0.0, math.inf, 0
    for k in range(k_max + 1):
        t = 2 * k
        G = float(d[:K - t] @ d[t:]) / g0 + float(d[:K - t - 1] @ d[t + 1:]) / g0
        if not G > 0.0:
            break
        G = min(G, prev)
        prev = G
        tsum += G
        pairs += 1
    tau = max(2.0 * tsum - 1.0, 1.0 / math.log10(K))
    ess = K / tau
    return dict(ess=ess, mcse=sd / math.sqrt(ess), sd=sd, rhat=rhat, lags=2 * pairs, truncated=pairs == k_max + 1)


def chains_diagnostics(a, max_lag=0):
    """series_diagnostics along the last axis of ``a`` (... x K): a dict of arrays of the leading shape."""
    a = np.asarray(a, dtype=np.float64)
    lead = a.shape[:-1]
    rows = [series_diagnostics(r, max_lag) for r in a.reshape(-1, a.shape[-1])]
    out = {k: np.array([r[k] for r in rows], dtype=np.int32 if k == "lags" else np.float64).reshape(lead) for k in KEYS}
    out["truncated"] = np.array([r["truncated"] for r in rows], dtype=bool).reshape(lead)
    return out


def truncated(lags, K, max_lag=0):
    """Which series ran into the lag cap: lags == 2 (k_max + 1)."""
    return np.asarray(lags) == 2 * (lag_cap(int(K), max_lag)[1] + 1)


def _summary(ess, mcse, sd, rhat, trunc):
    ok = ~np.isnan(ess)   # the constant series have no ess
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = mcse[ok] / sd[ok]
    rh = rhat[~np.isnan(rhat)]
    return dict(n=int(ess.size), min_ess=float(ess[ok].min()) if ok.any() else math.nan,
                median_ess=float(np.median(ess[ok])) if ok.any() else math.nan,
                max_rhat=float(rh.max()) if rh.size else math.nan,
                max_mcse_over_sd=float(rel.max()) if rel.size else math.nan,
                n_truncated=int(np.count_nonzero(trunc)), n_constant=int(np.count_nonzero(~ok)),
                n_low_ess=int(np.count_nonzero(ess[ok] < ESS_LOW)))


def summarise(d, mv=None):
    """The figures to look at first, of a dict of per-series arrays (ess, mcse, sd, rhat and ``truncated``): dict(n, min_ess,
    median_ess, max_rhat, max_mcse_over_sd, n_truncated, n_constant, n_low_ess) over all series and, with ``mv`` (one margin per
    series), ``by_outcome``: the same per margin, keyed by it.  Constant series (ess NaN) count in n_constant only."""
    ess, mcse, sd, rhat = (np.asarray(d[k], dtype=np.float64).reshape(-1) for k in ("ess", "mcse", "sd", "rhat"))
    trunc = np.asarray(d["truncated"], dtype=bool).reshape(-1)
    out = _summary(ess, mcse, sd, rhat, trunc)
    if mv is not None:
        mv = np.asarray(mv).reshape(-1)
        if mv.size != ess.size:
            raise ValueError("mv must hold one margin per series")
        out["by_outcome"] = {int(j): _summary(ess[mv == j], mcse[mv == j], sd[mv == j], rhat[mv == j], trunc[mv == j])
                             for j in np.unique(mv)}
    return out
