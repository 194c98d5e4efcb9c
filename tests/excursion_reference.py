"""The tests' reference for the exceedance, excursion and band outputs of a store (include/spamtree_hip.h, st_*_excursions).

Items 1 and 2 (count, prob, excur, joint_all, n_flat) are plain NumPy integer arithmetic and one double division: exact, compared
without a tolerance.  The excursion function is evaluated from the DEFINITION of the nested family, not through the per-draw
maximum the kernels use: D_{t,g}(c) = {i : g(i) = g, count_t(i) >= c}, and excur_t(i) is the share of draws whose event holds on
all of D_{t,g(i)}(count_t(i)).  Item 3 (mean, sd, maxdev) is np.longdouble, two-pass.

X[d][i], d < K, i < n; dom[i] in -1 .. G-1 (the mask already applied); thr[t][i]; side[t] in +-1."""
import numpy as np

U = 2.0 ** -53


def events(X, thr_t, side_t):
    with np.errstate(invalid="ignore"):
        return (X > thr_t[None, :]) if side_t > 0 else (X < thr_t[None, :])   # strict; NaN: False


def exceedance(X, thr, side, dom, G):
    """dict(count (T, n) int32, prob, excur (T, n), joint_all (T, G))."""
    K, n = X.shape
    T = thr.shape[0]
    count = np.zeros((T, n), dtype=np.int32)
    excur = np.full((T, n), np.nan)
    joint = np.empty((T, G))
    for t in range(T):
        E = events(X, thr[t], side[t])
        count[t] = np.count_nonzero(E, axis=0)
        for g in range(G):
            sel = dom == g
            joint[t, g] = np.float64(np.count_nonzero(E[:, sel].all(axis=1))) / np.float64(K)
            for c in np.unique(count[t, sel]):
                inD = sel & (count[t] >= c)
                share = np.float64(np.count_nonzero(E[:, inD].all(axis=1))) / np.float64(K)
                excur[t, sel & (count[t] == c)] = share
    return dict(count=count, prob=count.astype(np.float64) / np.float64(K), excur=excur, joint_all=joint)


def band(X, dom, G):
    """Long double, two-pass: dict(mean, sd (n), maxdev (G, K), n_flat (G), and what the error bounds need: max_abs_x, range (n))."""
    K, n = X.shape
    L = X.astype(np.longdouble)
    with np.errstate(invalid="ignore", over="ignore"):
        mean = L.sum(axis=0) / K
        dvs = L - mean
        M2 = (dvs * dvs).sum(axis=0)
        sd = np.sqrt(M2 / (K - 1))
        # a series is flat exactly when all its draws are equal (the Welford chain then gives M2 = 0 exactly) or not finite
        const = (X == X[0]).all(axis=0)
        ok = ~const & np.isfinite(sd) & (sd > 0)
        maxdev = np.zeros((G, K), dtype=np.longdouble)
        n_flat = np.zeros(G, dtype=np.int64)
        for g in range(G):
            n_flat[g] = np.count_nonzero((dom == g) & ~ok)
            sel = (dom == g) & ok
            if sel.any():
                maxdev[g] = (np.abs(dvs[:, sel]) / sd[sel]).max(axis=1)
        return dict(mean=mean, sd=sd, M2=M2, maxdev=maxdev, n_flat=n_flat, ok=ok, max_abs_x=np.abs(X).max(axis=0),
                    range=X.max(axis=0) - X.min(axis=0))


def band_bounds(X, dom, G, r):
    """Bounds on |mean - ref| (absolute, n), |sd - ref| / ref (relative, n) and |maxdev - ref| (absolute, (G, K)) of the kernel's
    chain -- K sequential steps delta = x - m; m = fma(delta, r_d, m); M2 = fma(delta, x - m, M2) -- to first order, doubled.
      mean    step j rounds m (at most u A, A = max|x|) and delta r_d (two roundings, at most 2 u R / (j + 1), R the range); the
              recursion m_d = m_{d-1} j / (j + 1) + x / (j + 1) shrinks an error made at step j to (j + 1) / K of itself at the
              end:  e_mean = u A (K + 1) / 2 + 2 u R.  Every running mean is within e_mean too.
      M2      the terms delta (x - m_d) are non-negative and sum to M2; a step rounds the sum (at most u M2), the two factors
              (2 u of the term) and inherits the running means' errors (at most R (e_{d-1} + e_d)):
              e_M2 = (K + 2) u + 2 K R e_mean / M2 relative;  sd: e_sd = e_M2 / 2 + 2 u (one division, one square root)
      maxdev  |x - mean| within e_mean + u |x - mean|, 1 / sd within e_sd + u, one product; the maximum is 1-Lipschitz:
              e_dev(g, d) = max over the domain's series of e_mean / sd + dev (e_sd + 3 u)
    The second-order terms are products of these; e_M2 < 1e-6 is asserted."""
    K, n = X.shape
    A, R = r["max_abs_x"].astype(np.float64), r["range"].astype(np.float64)
    ok = r["ok"]
    e_mean = U * A * (K + 1) / 2 + 2 * U * R
    M2 = np.where(ok, r["M2"].astype(np.float64), 1.0)
    e_M2 = (K + 2) * U + 2 * K * R * e_mean / M2
    assert np.all(e_M2[ok] < 1e-6), float(e_M2[ok].max())
    e_sd = e_M2 / 2 + 2 * U
    e_dev = np.zeros((G, K))
    sd = np.where(ok, r["sd"].astype(np.float64), 1.0)
    dev = np.abs(X - r["mean"].astype(np.float64)) / sd
    for g in range(G):
        sel = (dom == g) & ok
        if sel.any():
            e_dev[g] = (e_mean[sel] / sd[sel] + dev[:, sel] * (e_sd[sel] + 3 * U)).max(axis=1)
    return dict(mean=2 * e_mean, sd=2 * e_sd, maxdev=2 * e_dev)
