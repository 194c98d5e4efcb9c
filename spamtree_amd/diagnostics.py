"""Convergence diagnostics of one chain's saved draws, on the host, for the scalar chains (theta, beta, tausq): the definition of
include/spamtree_hip.h (st_*_diagnostics) restated in float64 -- the latent field's rows, the new points and the functionals get
theirs on the device from the same definition (spamtree_amd/csrc/diag_kernels.hpp).  NumPy only; the rank-normalised functions at
the end of the file also call the library's host function st_norm_quantile (no device).

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


# ---- rank-normalised R-hat, bulk, tail, quantile and exceedance ESS (include/spamtree_hip.h, st_*_rank_diagnostics) ------------------
# One series x_0 .. x_{K-1}, MIN_DRAWS <= K <= MAX_DRAWS; xs its ascending sort.  "the diagnostics" are series_diagnostics above.
#   ranks      lo_s = #{u : x_u < x_s}, hi_s = #{u : x_u <= x_s};  r2_s = lo_s + hi_s + 1 (twice the average 1-based rank; ties share it)
#   scores     p_s = (4 r2_s - 3) / (8 K + 2), one double division of exact integers;  z_s = Phi^-1(p_s) by the library's own text
#              (st_norm_quantile: spamtree_amd/csrc/norm_quantile.hpp, the function the device runs)
#   bulk       rhat_bulk, ess_bulk, lags_bulk = the diagnostics' rhat, ess, lags on z (ess_bulk is not split into half chains)
#   folded     med = xs[(K-1)/2] (K odd), 0.5 (xs[K/2-1] + xs[K/2]) (K even);  f_s = |x_s - med|;  zf = the scores of f;
#              rhat_fold = the diagnostics' rhat on zf;  rhat_rank = fmax(rhat_bulk, rhat_fold) (NaN only if both are)
#   indicator  a 0/1 series I with c = sum I: c in {0, K} gives ess = NaN, lags = 0; otherwise, in integers,
#              A_t = K^2 n11_t - K c (head_t + tail_t) + (K - t) c^2,  n11_t = sum_{s<K-t} I_s I_{s+t}, head_t = sum_{s<K-t} I_s,
#              tail_t = sum_{s>=t} I_s;  rho_t = A_t / A_0, so Gamma_k = N_k / A_0 with N_k = A_2k + A_2k+1: the diagnostics' stop
#              rule (N_k > 0), monotone rule (N_k <- min(N_k, N_k-1)) and sum on these integers;
#              tau = max(float(2 sum N_k - A_0) / float(A_0), 1 / log10 K);  ess = K / tau
#   quantile   j = min(max(ceil(prob K), 1), K - 1) - 1;  I_s = [x_s <= xs[j]];  ess_q = its indicator ESS;
#              ess_tail = fmin(indicator ESS at 0.05, at 0.95)
#   exceedance I_s = [x_s > thr] (side +1) or [x_s < thr] (side -1);  ess_exc = its indicator ESS;  prob = c / K;
#              mcse_prob = sqrt(prob (1 - prob) / ess_exc), 0 where c is 0 or K
#   a NaN draw: NaN in every float output, 0 in the lags.  A constant series: z = 0, the diagnostics' degenerate outputs.
MAX_PROBS = 8            # ST_RANK_MAX_PROBS
MAX_THRESHOLDS = 8       # ST_EXC_MAX_THRESHOLDS
RANK_KEYS = ("rhat_rank", "rhat_bulk", "rhat_fold", "ess_bulk", "ess_tail", "lags_bulk")


def norm_quantile(p):
    """Phi^-1 of an array of probabilities by the text the device runs (the library's st_norm_quantile; no device needed)."""
    from . import _lib
    p = np.ascontiguousarray(p, dtype=np.float64)
    z = np.empty_like(p)
    dp = _lib.c_dp
    rc = _lib.load().st_norm_quantile(p.ctypes.data_as(dp), z.ctypes.data_as(dp), p.size)
    if rc != 0:
        raise RuntimeError(f"st_norm_quantile returned {rc}")
    return z


def rank_scores(v):
    """(r2, z) of a series without NaN: twice the average ranks (int64) and their normal scores."""
    v = np.asarray(v, dtype=np.float64)
    K = v.size
    s = np.sort(v)
    r2 = (np.searchsorted(s, v, side="left") + np.searchsorted(s, v, side="right") + 1).astype(np.int64)
    return r2, norm_quantile((4 * r2 - 3).astype(np.float64) / np.float64(8 * K + 2))


def quantile_order(prob, K):
    """j of a probability strictly inside (0, 1): min(max(ceil(prob K), 1), K - 1) - 1."""
    return min(max(int(math.ceil(float(prob) * K)), 1), K - 1) - 1


def indicator_ess(I, max_lag=0):
    """(ess, lags) of a 0/1 series: integer A_t, one float division per lag, then the diagnostics' pairs."""
    I = np.asarray(I).astype(np.int64).reshape(-1)
    K = I.size
    c = int(I.sum())
    if c == 0 or c == K:
        return math.nan, 0
    _, k_max = lag_cap(K, max_lag)
    csum = np.concatenate(([0], np.cumsum(I)))   # csum[t] = sum_{s<t} I_s
    A0 = K * c * (K - c)

    def A(t):
        n11 = int(I[:K - t] @ I[t:])
        head, tail = int(csum[K - t]), c - int(csum[t])
        return K * K * n11 - K * c * (head + tail) + (K - t) * c * c
    nsum, prev, pairs = 0, None, 0
    for k in range(k_max + 1):
        N = A(2 * k) + A(2 * k + 1)    # Gamma_k = N / A_0, kept as its integer numerator
        if not N > 0:
            break
        N = N if prev is None else min(N, prev)
        prev = N
        nsum += N
        pairs += 1
    tau = max(float(2 * nsum - A0) / float(A0), 1.0 / math.log10(K))
    return K / tau, 2 * pairs


def _fmax(a, b):
    return b if math.isnan(a) else a if math.isnan(b) else max(a, b)


def _fmin(a, b):
    return b if math.isnan(a) else a if math.isnan(b) else min(a, b)


def check_rank_spec(probs=(), thresholds=(), sides=None, max_lag=0):
    """(probs, thresholds, sides) as lists, checked: what st_*_rank_diagnostics refuses of a spec is a ValueError here."""
    if max_lag < 0:
        raise ValueError("max_lag must not be negative (0: the default cap)")
    probs = [float(p) for p in np.asarray(probs, dtype=np.float64).reshape(-1)]
    if len(probs) > MAX_PROBS:
        raise ValueError(f"rank diagnostics: {len(probs)} probabilities, at most {MAX_PROBS}")
    if any(not 0.0 < p < 1.0 for p in probs):
        raise ValueError("rank diagnostics: a probability must lie strictly inside (0, 1)")
    thresholds = list(thresholds)
    if len(thresholds) > MAX_THRESHOLDS:
        raise ValueError(f"rank diagnostics: {len(thresholds)} thresholds, at most {MAX_THRESHOLDS}")
    if any(not np.all(np.isfinite(np.asarray(t, dtype=np.float64))) for t in thresholds):
        raise ValueError("rank diagnostics: thresholds must be finite")
    if sides is None:
        sides = 1
    if np.ndim(sides) != 0 and len(sides) != len(thresholds):
        raise ValueError(f"rank diagnostics: sides must be a scalar or hold one entry per threshold ({len(thresholds)})")
    sides = [int(s) for s in np.broadcast_to(np.asarray(sides), (len(thresholds),))]
    if any(s not in (1, -1) for s in sides):
        raise ValueError("rank diagnostics: a side must be +1 or -1")
    return probs, thresholds, sides


def rank_series_diagnostics(x, probs=(), thresholds=(), sides=None, max_lag=0):
    """dict(rhat_rank, rhat_bulk, rhat_fold, ess_bulk, ess_tail, lags_bulk, truncated, ess_q (n_prob), lags_q, ess_exc, mcse_prob,
    prob (n_thr), lags_exc) of one series of at least MIN_DRAWS draws: the definition in float64 with integer ranks and integer A_t.
    ``thresholds``: one scalar each; ``sides``: +1 / -1 per threshold (None: all +1)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    K = x.size
    if K < MIN_DRAWS:
        raise ValueError(f"the diagnostics need at least {MIN_DRAWS} draws, got {K}")
    if K > MAX_DRAWS:
        raise ValueError(f"the rank diagnostics take at most {MAX_DRAWS} draws, got {K}")
    probs, thresholds, sides = check_rank_spec(probs, thresholds, sides, max_lag)
    thresholds = [float(t) for t in thresholds]
    nq, nt = len(probs), len(thresholds)
    if np.isnan(x).any():
        nan_q, nan_t = np.full(nq, math.nan), np.full(nt, math.nan)
        return dict(rhat_rank=math.nan, rhat_bulk=math.nan, rhat_fold=math.nan, ess_bulk=math.nan, ess_tail=math.nan, lags_bulk=0,
                    truncated=False, ess_q=nan_q, lags_q=np.zeros(nq, dtype=np.int32), ess_exc=nan_t, mcse_prob=nan_t.copy(),
                    prob=nan_t.copy(), lags_exc=np.zeros(nt, dtype=np.int32))
    xs = np.sort(x)
    bulk = series_diagnostics(rank_scores(x)[1], max_lag)
    med = xs[(K - 1) // 2] if K % 2 else 0.5 * (xs[K // 2 - 1] + xs[K // 2])
    fold = series_diagnostics(rank_scores(np.abs(x - med))[1], max_lag)
    qs = [indicator_ess(x <= xs[quantile_order(p, K)], max_lag) for p in probs]
    tails = [indicator_ess(x <= xs[quantile_order(p, K)], max_lag)[0] for p in (0.05, 0.95)]
    ex = [indicator_ess(x > t if s > 0 else x < t, max_lag) for t, s in zip(thresholds, sides)]
    cnt = [int(np.count_nonzero(x > t if s > 0 else x < t)) for t, s in zip(thresholds, sides)]
    prob = np.array([c / K for c in cnt], dtype=np.float64)
    mcse = np.array([0.0 if c in (0, K) else math.sqrt(p * (1.0 - p) / e[0]) for c, p, e in zip(cnt, prob, ex)], dtype=np.float64)
    return dict(rhat_rank=_fmax(bulk["rhat"], fold["rhat"]), rhat_bulk=bulk["rhat"], rhat_fold=fold["rhat"], ess_bulk=bulk["ess"],
                ess_tail=_fmin(tails[0], tails[1]), lags_bulk=bulk["lags"], truncated=bulk["truncated"],
                ess_q=np.array([e for e, _ in qs], dtype=np.float64), lags_q=np.array([l for _, l in qs], dtype=np.int32),
                ess_exc=np.array([e for e, _ in ex], dtype=np.float64), mcse_prob=mcse, prob=prob,
                lags_exc=np.array([l for _, l in ex], dtype=np.int32))


def chains_rank_diagnostics(a, probs=(), thresholds=(), sides=None, max_lag=0):
    """rank_series_diagnostics along the last axis of ``a`` (... x K): per-series outputs of the leading shape, ess_q
    (n_prob, ...) and ess_exc, mcse_prob, prob (n_thr, ...)."""
    a = np.asarray(a, dtype=np.float64)
    lead = a.shape[:-1]
    rows = [rank_series_diagnostics(r, probs, thresholds, sides, max_lag) for r in a.reshape(-1, a.shape[-1])]
    out = {k: np.array([r[k] for r in rows], dtype=np.int32 if k == "lags_bulk" else np.float64).reshape(lead) for k in RANK_KEYS}
    out["truncated"] = np.array([r["truncated"] for r in rows], dtype=bool).reshape(lead)
    for k in ("ess_q", "ess_exc", "mcse_prob", "prob"):
        m = np.array([r[k] for r in rows], dtype=np.float64).reshape(len(rows), -1)
        out[k] = m.T.reshape((m.shape[1],) + lead)
    return out


def _rank_summary(rhat, bulk, tail):
    fin = lambda v: v[~np.isnan(v)]   # noqa: E731
    rh, b, t = fin(rhat), fin(bulk), fin(tail)
    return dict(n=int(rhat.size), max_rhat_rank=float(rh.max()) if rh.size else math.nan,
                min_ess_bulk=float(b.min()) if b.size else math.nan, median_ess_bulk=float(np.median(b)) if b.size else math.nan,
                min_ess_tail=float(t.min()) if t.size else math.nan, median_ess_tail=float(np.median(t)) if t.size else math.nan,
                n_low_ess_bulk=int(np.count_nonzero(b < ESS_LOW)), n_low_ess_tail=int(np.count_nonzero(t < ESS_LOW)))


def summarise_rank(d, mv=None):
    """The figures to look at first, of a dict of per-series arrays (rhat_rank, ess_bulk, ess_tail): dict(n, max_rhat_rank,
    min_ess_bulk, median_ess_bulk, min_ess_tail, median_ess_tail, n_low_ess_bulk, n_low_ess_tail (below ESS_LOW)) over all series
    and, with ``mv`` (one margin per series), ``by_outcome``: the same per margin.  NaN entries (constant series) are left out."""
    rhat, bulk, tail = (np.asarray(d[k], dtype=np.float64).reshape(-1) for k in ("rhat_rank", "ess_bulk", "ess_tail"))
    out = _rank_summary(rhat, bulk, tail)
    if mv is not None:
        mv = np.asarray(mv).reshape(-1)
        if mv.size != rhat.size:
            raise ValueError("mv must hold one margin per series")
        out["by_outcome"] = {int(j): _rank_summary(rhat[mv == j], bulk[mv == j], tail[mv == j]) for j in np.unique(mv)}
    return out
