"""Quantiles and the exact CRPS of the mixture predictive at new points: the definition of st_points_mixture_*
(include/spamtree_hip.h, spamtree_amd/csrc/points_mixture.hpp) restated in float64 for small inputs.  NumPy and the standard
library only.

Saved draw s gives a target its exact conditional law N(m_s, v_s) (w: cond_mean and the clamped cond_var; yhat: x'beta + cond_mean
and cond_var + 1 / tausq_inv; a functional: F_m, F_v).  The predictive is the equal-weight mixture of the K stored components:
  CDF       F(x) = (1 / K) sum_s Phi((x - m_s) / sd_s),  Phi(z) = erfc(-z / sqrt 2) / 2;  a component with v_s == 0 is the
            right-continuous step 1(x >= m_s).
  quantile  inf{x : F(x) >= p} for p strictly inside (0, 1): here by plain bisection on the definition.
  CRPS at y A(d, s2) = d erf(d / (s sqrt 2)) + s sqrt(2 / pi) exp(-d^2 / (2 s2)),  A(d, 0) = |d|   (= E|N(d, s2)|)
            crps = (1 / K) sum_s A(y - m_s, v_s) - spread,   spread = (1 / (2 K^2)) sum_s sum_t A(m_s - m_t, v_s + v_t)
            (Grimit et al. 2006), the double sum as its diagonal plus twice the pairs s < t.  spread does not depend on y.
Unlike the quantiles and the CRPS of the stored draws (one draw per component, steps of 1 / K) these are exact in the mixture."""
from __future__ import annotations

import math
from statistics import NormalDist

import numpy as np

MAX_PROBS = 8        # ST_MIX_MAX_PROBS
MAX_DRAWS = 8192     # ST_MIX_MAX_DRAWS
_RSQRT2 = 0.70710678118654752440
_SQRT_2_OVER_PI = 0.79788456080286535588


def check_probs(probs):
    """The probabilities as a float64 vector: 1 .. MAX_PROBS of them, each finite and strictly inside (0, 1); ValueError naming
    the index otherwise."""
    p = np.atleast_1d(np.asarray(probs, dtype=np.float64)).reshape(-1)
    if not 1 <= p.size <= MAX_PROBS:
        raise ValueError(f"mixture: {p.size} probabilities, must be 1 .. {MAX_PROBS}")
    for t, v in enumerate(p):
        if not (0.0 < v < 1.0):
            raise ValueError(f"mixture: probs[{t}] = {v} is not strictly inside (0, 1)")
    return np.ascontiguousarray(p)


def check_spec(spec, has_X=True, has_y=True, keep=None, y=None):
    """The option ``mixture=dict(probs=, crps=)`` of fit and predict: returns (probs float64 vector or None, crps bool).
    ValueError for unknown keys, nothing asked for, what ``check_probs`` refuses, ``crps`` without regressors, without held-out
    observations or (``y``: them, when at hand) with none that is not NaN, and more than MAX_DRAWS components (``keep``: the saved
    draws over all chains)."""
    spec = dict(spec)
    unknown = set(spec) - {"probs", "crps"}
    if unknown:
        raise ValueError(f"mixture: unknown keys {sorted(unknown)} (probs, crps)")
    probs = check_probs(spec["probs"]) if spec.get("probs") is not None else None
    crps = bool(spec.get("crps", False))
    if probs is None and not crps:
        raise ValueError("mixture: probs or crps=True are needed")
    if crps and not has_X:
        raise ValueError("mixture: crps needs the regressors X_new")
    if crps and not has_y:
        raise ValueError("mixture: crps needs held-out observations y_new")
    if crps and y is not None and np.size(y) > 0 and np.all(np.isnan(np.asarray(y, dtype=np.float64))):
        raise ValueError("mixture: crps with no scored point (every y_new is NaN)")
    if keep is not None and keep > MAX_DRAWS:
        raise ValueError(f"mixture: {keep} saved draws beyond the store's {MAX_DRAWS}")
    return probs, crps


def _components(m, v):
    m = np.asarray(m, dtype=np.float64).reshape(-1)
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    if m.size == 0 or m.size != v.size:
        raise ValueError("mixture: m and v must hold the same K >= 1 components")
    if not (np.all(np.isfinite(m)) and np.all(v >= 0.0) and np.all(np.isfinite(v))):
        raise ValueError("mixture: the means must be finite and the variances finite and >= 0")
    return m, v


def cdf(x, m, v):
    """F(x) of the mixture with means ``m`` and variances ``v`` (K each) at the scalar ``x``."""
    m, v = _components(m, v)
    x = float(x)
    tot = 0.0
    for ms, vs in zip(m, v):
        if vs > 0.0:
            tot += 0.5 * math.erfc(-((x - float(ms)) / math.sqrt(float(vs))) * _RSQRT2)
        else:
            tot += 1.0 if x >= ms else 0.0
    return tot / m.size


def quantile(p, m, v):
    """inf{x : F(x) >= p} by bisection inside [min_s, max_s] of m_s + z_p sd_s (at the upper end every component's CDF is >= p),
    widened by one part in 2^40 for the rounding of the ends; stops when no double lies between the ends."""
    m, v = _components(m, v)
    p = float(check_probs([p])[0])
    z = NormalDist().inv_cdf(p)
    e = m + z * np.sqrt(v)
    lo, hi = float(e.min()), float(e.max())
    pad = max(abs(lo), abs(hi)) * 2.0 ** -40
    lo, hi = lo - pad, hi + pad
    if cdf(lo, m, v) >= p:
        return lo
    while True:
        mid = lo + 0.5 * (hi - lo)
        if not lo < mid < hi:
            return hi
        if cdf(mid, m, v) >= p:
            hi = mid
        else:
            lo = mid


def _A(d, s2):
    if s2 > 0.0:
        s = math.sqrt(s2)
        r = d / s
        return d * math.erf(r * _RSQRT2) + s * _SQRT_2_OVER_PI * math.exp(-0.5 * r * r)
    return abs(d)


def spread(m, v):
    """(1 / (2 K^2)) sum_s sum_t A(m_s - m_t, v_s + v_t): the diagonal plus twice the pairs s < t, each sum by math.fsum."""
    m, v = _components(m, v)
    K = m.size
    diag = math.fsum(_A(0.0, float(2.0 * vs)) for vs in v)
    pairs = math.fsum(_A(float(m[s]) - float(m[t]), float(v[s]) + float(v[t])) for s in range(K) for t in range(s + 1, K))
    return (diag + 2.0 * pairs) / (2.0 * K * K)


def point_means(values, y, mv, q):
    """(mean over the scored points, per-outcome means) of one per-point array of the scores -- crps_mixture, spread -- where
    ``y`` is not NaN; ``mv`` the 1-based margins; NaN for an outcome (or a set) without a scored point."""
    values, obs, mv = np.asarray(values, dtype=np.float64), ~np.isnan(np.asarray(y, dtype=np.float64)), np.asarray(mv).reshape(-1)
    mean = lambda sel: float(np.mean(values[sel])) if np.any(sel) else float("nan")   # noqa: E731
    return mean(obs), np.array([mean(obs & (mv == j + 1)) for j in range(int(q))])


def crps(y, m, v):
    """The CRPS of the mixture at the observation ``y``: (1 / K) sum_s A(y - m_s, v_s) - spread."""
    m, v = _components(m, v)
    y = float(y)
    return math.fsum(_A(y - float(ms), float(vs)) for ms, vs in zip(m, v)) / m.size - spread(m, v)
