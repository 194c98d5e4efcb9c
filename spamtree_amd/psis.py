"""Pareto-smoothed importance sampling of one series of log ratios: the definition in float64 NumPy (no device, no library).

Vehtari, Simpson, Gelman, Yao, Gabry, "Pareto smoothed importance sampling", with the generalised Pareto fit of Zhang and Stephens
(2009) under the weakly informative prior of ``loo::gpdfit``, r_eff = 1.  spamtree_amd/csrc/psis_kernels.hpp restates it in the
order the device evaluates it; ``psis`` below runs that kernel.

A series is K values t_0 .. t_{K-1}, the log importance ratios (for the rows' own leave-one-out weights t_s = -l_s of
``spamtree_amd.loo``), optionally with companions Phi_s, mu_s.  A draw whose t_s is not finite is skipped; S = the number of finite
ones.  S = 0: every double output NaN, tail_len = 0, n_draws = 0.

    shift       c = max t_s,  lw_s = t_s - c
    tail        M = min(floor(S / 5), m*), m* the smallest integer with m*^2 >= 9 S;  M < 5: no smoothing
    order       ascending by (t_s, s);  the tail is the last M draws, cut = lw of the draw just below it,
                x_j = exp(lw_(S-M+j)) - exp(cut), j = 1 .. M.  The tail's largest and smallest t equal, or x_floor((M+2)/4) == 0:
                no smoothing
    fit         N = M, G = 30 + isqrt(N), x* = x_floor((N+2)/4),  theta_j = 1 / x_N + (1 - sqrt(G / (j - 0.5))) / (3 x*), j = 1 .. G,
                k_j = mean_i log1p(-theta_j x_i),  l_j = N (log(-theta_j / k_j) - k_j - 1),  omega_j = 1 / sum_i exp(l_i - l_j),
                theta^ = sum theta_j omega_j,  k = mean_i log1p(-theta^ x_i),  sigma = -k / theta^,  khat = (k N + 5) / (N + 10);
                khat or sigma not finite: no smoothing
    smoothing   p_j = (j - 0.5) / M,  q_j = sigma expm1(-khat log1p(-p_j)) / khat  (khat == 0: -sigma log1p(-p_j)),
                lw'_(S-M+j) = min(log(q_j + exp(cut)), 0);  every other draw keeps lw' = lw
    estimates   u_s = lw'_s - lw_s,  W1 = sum exp(lw'_s),  W2 = sum exp(2 lw'_s),  U = sum exp(u_s),
                elpd_psis = -c + log U - log W1,  pit_psis = sum e^lw' Phi_s / W1,  mu_psis = sum e^lw' mu_s / W1,
                weight_ess_psis = W1^2 / W2,  tail_len = M (0 when not smoothed),  n_draws = S

"No smoothing" gives khat = +inf, tail_len = 0 and the raw estimates (lw' = lw: elpd_psis = -log mean exp(t_s)).  Every sum here
is one chain of additions in ascending index (draw index; j over the tail and over the grid).
"""
import math

import numpy as np

MAX_DRAWS = 16384      # ST_PSIS_MAX_DRAWS
MAX_TAIL = 384         # tail_length(MAX_DRAWS)
KHAT_BAD = 0.7


def _asum(a, axis=-1):
    """One chain of additions in ascending index."""
    a = np.asarray(a, dtype=np.float64)
    if a.shape[axis] == 0:
        return np.zeros(np.delete(a.shape, axis))
    return np.take(np.cumsum(a, axis=axis), -1, axis=axis)


def tail_length(S):
    """M = min(floor(S / 5), m*), m* the smallest integer with m*^2 >= 9 S (integers only)."""
    S = int(S)
    m = math.isqrt(9 * S)
    if m * m < 9 * S:
        m += 1
    return min(S // 5, m)


def grid_size(N):
    """G = 30 + isqrt(N)."""
    return 30 + math.isqrt(int(N))


def quarter_index(N):
    """The 1-based index floor((N + 2) / 4) of x*."""
    return (int(N) + 2) // 4


def khat_threshold(S):
    """min(1 - 1 / log10 S, 0.7): the sample-size dependent threshold of the paper's second edition."""
    return min(1.0 - 1.0 / math.log10(S), KHAT_BAD) if S > 1 else -math.inf


def gpdfit(x):
    """(khat, sigma) of the ascending positive exceedances x_1 .. x_N; (+inf, nan) where the fit is not defined (x* == 0 or a
    value that is not finite on the way)."""
    x = np.asarray(x, dtype=np.float64)
    N = x.size
    if N < 1:
        return math.inf, math.nan
    G = grid_size(N)
    xs = x[max(quarter_index(N), 1) - 1]
    if not xs > 0.0:
        return math.inf, math.nan
    with np.errstate(all="ignore"):
        j = np.arange(1, G + 1, dtype=np.float64)
        theta = 1.0 / x[N - 1] + (1.0 - np.sqrt(G / (j - 0.5))) / (3.0 * xs)
        kj = _asum(np.log1p(-theta[:, None] * x[None, :]), axis=1) / N
        lj = N * (np.log(-theta / kj) - kj - 1.0)
        omega = 1.0 / _asum(np.exp(lj[None, :] - lj[:, None]), axis=1)
        th = float(_asum(theta * omega))
        k = float(_asum(np.log1p(-th * x))) / N
        sigma = -k / th
        khat = (k * N + 5.0) / (N + 10.0)
    if not (math.isfinite(khat) and math.isfinite(sigma)):
        return math.inf, math.nan
    return khat, sigma


def _split(t):
    t = np.asarray(t, dtype=np.float64).ravel()
    ok = np.isfinite(t)
    idx = np.nonzero(ok)[0]
    return t, idx


def smooth(t):
    """dict(lw, lw_s, khat, sigma, tail_len, n_draws, c, idx): lw = t - c and the smoothed lw_s of the finite draws (``idx``, draw
    order).  khat = +inf, tail_len = 0 and lw_s = lw where there is no smoothing."""
    t, idx = _split(t)
    S = idx.size
    if S == 0:
        return dict(lw=np.zeros(0), lw_s=np.zeros(0), khat=math.nan, sigma=math.nan, tail_len=0, n_draws=0, c=math.nan, idx=idx)
    tf = t[idx]
    c = tf.max()
    lw = tf - c
    out = dict(lw=lw, lw_s=lw.copy(), khat=math.inf, sigma=math.nan, tail_len=0, n_draws=S, c=c, idx=idx)
    M = tail_length(S)
    if M < 5:
        return out
    order = np.lexsort((np.arange(S), tf))          # ascending by (t, s)
    tail = order[S - M:]
    if tf[tail[-1]] == tf[tail[0]]:
        return out
    cut = lw[order[S - M - 1]]
    with np.errstate(all="ignore"):
        ecut = math.exp(cut)
        x = np.exp(lw[tail]) - ecut
        if x[quarter_index(M) - 1] == 0.0:
            return out
        khat, sigma = gpdfit(x)
        if not math.isfinite(khat):
            return out
        p = (np.arange(1, M + 1, dtype=np.float64) - 0.5) / M
        q = -sigma * np.log1p(-p) if khat == 0.0 else sigma * np.expm1(-khat * np.log1p(-p)) / khat
        out["lw_s"][tail] = np.minimum(np.log(q + ecut), 0.0)
    out.update(khat=khat, sigma=sigma, tail_len=M)
    return out


def estimates(t, phi=None, mu=None):
    """dict(khat, sigma, elpd_psis, pit_psis, mu_psis, weight_ess_psis, tail_len, n_draws) of one series (pit / mu NaN without
    their companions)."""
    sm = smooth(t)
    nan = math.nan
    out = dict(khat=sm["khat"], sigma=sm["sigma"], elpd_psis=nan, pit_psis=nan, mu_psis=nan, weight_ess_psis=nan,
               tail_len=sm["tail_len"], n_draws=sm["n_draws"])
    if sm["n_draws"] == 0:
        return out
    lw, lws, idx = sm["lw"], sm["lw_s"], sm["idx"]
    with np.errstate(all="ignore"):
        e = np.exp(lws)
        W1, W2, U = float(_asum(e)), float(_asum(np.exp(2.0 * lws))), float(_asum(np.exp(lws - lw)))
        out["elpd_psis"] = -sm["c"] + math.log(U) - math.log(W1)
        out["weight_ess_psis"] = W1 * W1 / W2
        if phi is not None:
            out["pit_psis"] = float(_asum(e * np.asarray(phi, dtype=np.float64).ravel()[idx])) / W1
        if mu is not None:
            out["mu_psis"] = float(_asum(e * np.asarray(mu, dtype=np.float64).ravel()[idx])) / W1
    return out


OUT_DOUBLE = ("khat", "elpd_psis", "pit_psis", "mu_psis", "weight_ess_psis")
OUT_INT = ("tail_len", "n_draws")


def estimates_store(t, phi=None, mu=None):
    """``estimates`` of every column of a [K][n] store: dict of n-vectors (without sigma)."""
    t = np.asarray(t, dtype=np.float64)
    K, n = t.shape
    out = {k: np.full(n, np.nan) for k in OUT_DOUBLE}
    out.update({k: np.zeros(n, dtype=np.int32) for k in OUT_INT})
    for i in range(n):
        e = estimates(t[:, i], None if phi is None else np.asarray(phi)[:, i], None if mu is None else np.asarray(mu)[:, i])
        for k in OUT_DOUBLE + OUT_INT:
            out[k][i] = e[k]
    return out


def psis(log_ratios, phi=None, mu=None, handle=None):
    """The device's k_loo_psis (st_psis) on a [K][n] array of log ratios (a vector is one series), 1 <= K <= 16384, with optional
    companions of the same shape: dict(khat, elpd_psis, weight_ess_psis, tail_len, n_draws[, pit_psis][, mu_psis]) of n values.
    ``handle``: a ``SpamTreeMV`` (any, limited_tree included); it lends its stream and device only."""
    if handle is None:
        raise ValueError("psis: a SpamTreeMV handle is needed (the kernel runs on its device and stream)")
    t = np.asarray(log_ratios, dtype=np.float64)
    one = t.ndim == 1
    if one:
        t = t[:, None]
    if t.ndim != 2:
        raise ValueError("psis: log_ratios must be [K] or [K][n]")
    comp = []
    for name, a in (("phi", phi), ("mu", mu)):
        if a is not None:
            a = np.asarray(a, dtype=np.float64)
            a = a[:, None] if one and a.ndim == 1 else a
            if a.shape != t.shape:
                raise ValueError(f"psis: {name} has shape {a.shape}, log_ratios {t.shape}")
        comp.append(a)
    out = handle.psis(t, comp[0], comp[1])
    return {k: v[0] for k, v in out.items()} if one else out
