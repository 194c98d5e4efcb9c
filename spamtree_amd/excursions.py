"""Exceedance probabilities, excursion sets and simultaneous credible bands of the stored draws: what is done with the device's
outputs (st_*_excursions, include/spamtree_hip.h has the definition), and the definition restated in float64 for small inputs.
NumPy only.

One store X[d][i] has draws d < K and series i < n.  Every series has a domain g(i) in {-1, 0 .. G-1} (rows and new points: the
outcome; functionals: one domain; a mask entry 0 puts the series in no domain, g = -1).  T thresholds, each with a side +1 / -1
and values c_t(i); the event E_t(d,i) is X[d][i] > c_t(i) (side +1) or X[d][i] < c_t(i) (side -1), strict, false for a NaN draw.
  count_t(i) = #{d : E_t(d,i)};  prob_t(i) = count_t(i) / K
  m_{t,g}(d) = max{count_t(i) : g(i) = g, not E_t(d,i)}, -1 if no series of the domain fails
  excur_t(i) = #{d : m_{t,g(i)}(d) < count_t(i)} / K (NaN for g(i) = -1);  joint_all[t][g] = #{d : m_{t,g}(d) < 0} / K
  the level-alpha excursion set of a domain: {i : excur_t(i) >= 1 - alpha}; excur <= prob, and excur does not decrease with count
  band: mean_i, sd_i (divisor K - 1) by Welford over ascending d;  maxdev[g][d] = max{|X[d][i] - mean_i| / sd_i : g(i) = g,
  sd_i > 0 and finite}, 0 without such a series; the others of the domain are counted in n_flat[g];  the band factor of a domain is
  the ceil((1 - alpha) K)-th smallest maxdev[g][.] (an order statistic, not interpolated), the band mean +- factor sd.
These are probabilities of the stored draws (no Rao-Blackwellisation at new points); one outcome at a time."""
from __future__ import annotations

import math

import numpy as np

MAX_THRESHOLDS = 8    # include/spamtree_hip.h: ST_EXC_MAX_THRESHOLDS
MAX_DRAWS = 16384     # the stores' limit (st_summary_reserve)


def threshold_entries(thresholds):
    """The list of a caller's thresholds: a scalar is one entry (the entries of a sequence may differ in kind: scalars, vectors)."""
    if np.isscalar(thresholds) or (isinstance(thresholds, np.ndarray) and thresholds.ndim == 0):
        return [thresholds]
    return list(thresholds)


def expand_thresholds(thresholds, m, side=1):
    """The ABI's arrays from what a caller writes.  ``thresholds``: a scalar (one threshold, the same for all m outcomes or
    functionals) or a sequence of T entries, each a scalar or m values.  ``side``: +1 / -1, a scalar or one per threshold.
    Returns (thr (T, m) float64, side (T,) int32).  ValueError: no or more than MAX_THRESHOLDS thresholds, a wrong length, a
    non-finite value, a side other than +-1."""
    m = int(m)
    entries = threshold_entries(thresholds)
    if not 1 <= len(entries) <= MAX_THRESHOLDS:
        raise ValueError(f"excursions: {len(entries)} thresholds, must be 1 .. {MAX_THRESHOLDS}")
    thr = np.empty((len(entries), m))
    for t, e in enumerate(entries):
        e = np.asarray(e, dtype=np.float64)
        if e.ndim > 1 or (e.ndim == 1 and e.size != m):
            raise ValueError(f"excursions: threshold {t} must be a scalar or hold {m} values, got shape {e.shape}")
        thr[t] = e
    if not np.all(np.isfinite(thr)):
        raise ValueError("excursions: thresholds must be finite")
    sd = np.asarray(side)
    if sd.ndim > 1 or (sd.ndim == 1 and sd.size != len(entries)):
        raise ValueError(f"excursions: side must be a scalar or hold one entry per threshold ({len(entries)})")
    if not np.all((sd == 1) | (sd == -1)):
        raise ValueError("excursions: a side must be +1 or -1")
    return np.ascontiguousarray(thr), np.ascontiguousarray(np.broadcast_to(sd, (len(entries),)).astype(np.int32))


def check_mask(mask, n):
    """``mask`` as n bytes (0 = out), or None."""
    if mask is None:
        return None
    mk = np.asarray(mask)
    if mk.shape != (int(n),):
        raise ValueError(f"excursions: mask must hold {int(n)} entries, got shape {mk.shape}")
    return np.ascontiguousarray(mk != 0).astype(np.uint8)


def check_keep(K, band):
    """ValueError unless 1 <= K <= MAX_DRAWS (2 with a band)."""
    K = int(K)
    if not 1 <= K <= MAX_DRAWS:
        raise ValueError(f"excursions: {K} stored draws, must be 1 .. {MAX_DRAWS}")
    if band and K < 2:
        raise ValueError("excursions: the band needs at least 2 stored draws")


def excursion_set(excur, alpha):
    """The level-alpha excursion set: the boolean array excur >= 1 - alpha (False where excur is NaN: masked-out series)."""
    if not 0.0 <= alpha <= 1.0:
        raise ValueError("alpha must lie in [0, 1]")
    e = np.asarray(excur, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return e >= 1.0 - alpha


def band_factor(maxdev, alpha):
    """The ceil((1 - alpha) K)-th smallest (1-based, at least the first) of the K values ``maxdev`` of one domain."""
    v = np.sort(np.asarray(maxdev, dtype=np.float64).reshape(-1))
    if v.size < 1 or not 0.0 <= alpha <= 1.0:
        raise ValueError("band_factor needs at least one value and alpha in [0, 1]")
    r = min(max(v.size - math.floor(alpha * v.size), 1), v.size)   # = ceil((1 - alpha) K) for integer K, with one rounding, not two
    return float(v[r - 1])


def band(mean, sd, maxdev, alpha, domain=None):
    """(lower, upper) = mean -+ factor sd with each domain's own factor.  ``maxdev``: (G, K); ``domain``: one of -1, 0 .. G-1 per
    series (None: all 0).  Series of domain -1 get NaN."""
    mean, sd = np.asarray(mean, dtype=np.float64), np.asarray(sd, dtype=np.float64)
    md = np.atleast_2d(np.asarray(maxdev, dtype=np.float64))
    dom = np.zeros(mean.shape, dtype=np.int64) if domain is None else np.asarray(domain, dtype=np.int64)
    if dom.shape != mean.shape or sd.shape != mean.shape or (dom >= md.shape[0]).any():
        raise ValueError("band: mean, sd and domain must have one shape and the domains a row of maxdev each")
    f = np.full(mean.shape, np.nan)
    for g in range(md.shape[0]):
        f[dom == g] = band_factor(md[g], alpha)
    return mean - f * sd, mean + f * sd


def store_excursions(X, thr=None, side=None, domain=None, G=1, mask=None, want_band=False):
    """The definition on the host, float64, for small inputs.  ``X``: (K, n).  ``thr``: (T, n) values c_t(i), or None.  ``side``:
    (T,) of +-1.  ``domain``: n outcomes in 0 .. G-1 (None: all 0).  ``mask``: n, 0 = out.  Returns the dict the device calls
    return: count, prob, excur (T, n), joint_all (T, G), and with ``want_band`` mean, sd (n), maxdev (G, K), n_flat (G); n_draws."""
    X = np.asarray(X, dtype=np.float64)
    K, n = X.shape
    dom = np.zeros(n, dtype=np.int64) if domain is None else np.asarray(domain, dtype=np.int64).copy()
    if mask is not None:
        dom[np.asarray(mask) == 0] = -1
    out = dict(n_draws=K)
    if thr is not None:
        thr = np.asarray(thr, dtype=np.float64).reshape(-1, n)
        T = thr.shape[0]
        side = np.ones(T, dtype=np.int64) if side is None else np.asarray(side).reshape(T)
        count = np.zeros((T, n), dtype=np.int32)
        excur = np.full((T, n), np.nan)
        joint = np.ones((T, G))
        for t in range(T):
            E = (X > thr[t]) if side[t] > 0 else (X < thr[t])
            count[t] = E.sum(axis=0)
            for g in range(G):
                sel = dom == g
                m = np.where(~E[:, sel], count[t, sel], -1).max(axis=1, initial=-1)   # (K,)
                H = np.searchsorted(np.sort(m), np.arange(K + 1), side="left")       # H[c] = #{d : m(d) < c}
                excur[t, sel] = H[count[t, sel]] / K
                joint[t, g] = H[0] / K
        out.update(count=count, prob=count / K, excur=excur, joint_all=joint)
    if want_band:
        if K < 2:
            raise ValueError("the band needs at least 2 draws")
        mean, M2 = np.zeros(n), np.zeros(n)
        with np.errstate(invalid="ignore", over="ignore"):
            for d in range(K):
                delta = X[d] - mean
                mean = mean + delta * (1.0 / (d + 1))
                M2 = M2 + delta * (X[d] - mean)
            sd = np.sqrt(M2 / (K - 1))
            ok = (sd > 0) & np.isfinite(sd)
            maxdev, n_flat = np.zeros((G, K)), np.zeros(G, dtype=np.int64)
            for g in range(G):
                sel = (dom == g) & ok
                n_flat[g] = np.count_nonzero((dom == g) & ~ok)
                if sel.any():
                    maxdev[g] = (np.abs(X[:, sel] - mean[sel]) / sd[sel]).max(axis=1)
        out.update(mean=mean, sd=sd, maxdev=maxdev, n_flat=n_flat)
    return out
