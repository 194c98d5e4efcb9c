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


def chains_diagnostics(a, max_lag=0, n_chains=1):
    """series_diagnostics along the last axis of ``a`` (... x K): a dict of arrays of the leading shape.  With ``n_chains`` > 1
    every series is that many chains laid end to end (multichain_diagnostics)."""
    a = np.asarray(a, dtype=np.float64)
    lead = a.shape[:-1]
    rows = [multichain_diagnostics(r, n_chains, max_lag) for r in a.reshape(-1, a.shape[-1])]
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


def chains_rank_diagnostics(a, probs=(), thresholds=(), sides=None, max_lag=0, n_chains=1):
    """rank_series_diagnostics along the last axis of ``a`` (... x K): per-series outputs of the leading shape, ess_q
    (n_prob, ...) and ess_exc, mcse_prob, prob (n_thr, ...).  With ``n_chains`` > 1 every series is that many chains laid end to
    end (multichain_rank_diagnostics)."""
    a = np.asarray(a, dtype=np.float64)
    lead = a.shape[:-1]
    rows = [multichain_rank_diagnostics(r, n_chains, probs, thresholds, sides, max_lag) for r in a.reshape(-1, a.shape[-1])]
    out = {k: np.array([r[k] for r in rows], dtype=np.int32 if k == "lags_bulk" else np.float64).reshape(lead) for k in RANK_KEYS}
    out["truncated"] = np.array([r["truncated"] for r in rows], dtype=bool).reshape(lead)
    for k in ("ess_q", "ess_exc", "mcse_prob", "prob"):
        m = np.array([r[k] for r in rows], dtype=np.float64).reshape(len(rows), -1)
        out[k] = m.T.reshape((m.shape[1],) + lead)
    return out


# ---- several chains in one series (include/spamtree_hip.h, st_*_chain_diagnostics and st_*_chain_rank_diagnostics) ------------------
# A series of K = M N draws is M = n_chains chains of N draws laid end to end: x_{c,s} = x[c N + s].  1 <= M <= MAX_CHAINS, N >= MIN_DRAWS.
#   M = 1      series_diagnostics / rank_series_diagnostics, bit for bit
#   lag cap    L = min(max_lag, N - 2) (max_lag = 0: DEFAULT_MAX_LAG);  k_max = (L - 1) // 2
#   within     mu_c = mean of chain c;  d_{c,s} = x_{c,s} - mu_c;  gamma_{c,t} = (1/N) sum_{s<N-t} d_{c,s} d_{c,s+t};  gbar_t = mean_c gamma_{c,t}
#   between    mubar = mean_c mu_c;  B' = sum_c (mu_c - mubar)^2 / (M - 1)
#   rho, ess   rho_t = (B' + gbar_t) / (B' + gbar_0), then the pairs, the stop and monotone rules, tau floored at 1 / log10 K, ess = K / tau
#   sd, mcse   sd = the pooled sd of the K draws (divisor K - 1);  mcse = sd / sqrt(ess)
#   rhat       h = N // 2; the S = 2M half chains x_c[:h], x_c[N-h:]; W = mean of their sample variances (divisor h - 1);
#              B = h / (S - 1) sum (m_j - mbar)^2;  rhat = sqrt(((h-1)/h W + B/h) / W)
#   degenerate B' + gbar_0 == 0: ess NaN, mcse 0, sd 0, rhat NaN, lags 0;  W == 0: rhat NaN
#   indicator  integers: c_c = sum_s I_{c,s}, A_{c,t} = indicator_ess's A_t of chain c alone (K -> N), C = sum c_c, D = sum (M c_c - C)^2,
#              Num_t = N D + M (M - 1) sum_c A_{c,t};  rho_t = Num_t / Num_0;  the pairs on N_k = Num_2k + Num_2k+1;
#              tau = max(float(2 sum N_k - Num_0) / float(Num_0), 1 / log10 K);  C in {0, K}: ess NaN, lags 0
#   rank       ranks, scores, median, folded series and xs[j] of the pooled K draws; bulk / fold = the multi-chain diagnostics on z / zf;
#              quantile, tail and exceedance ESS = the multi-chain indicator ESS;  prob = C / K, mcse_prob as before
MAX_CHAINS = 16          # ST_DIAG_MAX_CHAINS


def check_chains(K, n_chains):
    """N = K // n_chains, checked as st_*_chain_diagnostics checks it (ValueError)."""
    M = int(n_chains)
    if not 1 <= M <= MAX_CHAINS:
        raise ValueError(f"n_chains = {M} must lie in 1 .. {MAX_CHAINS}")
    if K % M:
        raise ValueError(f"{K} draws are not a multiple of n_chains = {M}")
    if K // M < MIN_DRAWS:
        raise ValueError(f"{K} draws in {M} chains are {K // M} per chain, the diagnostics need at least {MIN_DRAWS}")
    return K // M


def multichain_diagnostics(x, n_chains=1, max_lag=0):
    """dict(ess, mcse, sd, rhat, lags, truncated) of one series of n_chains chains laid end to end, in float64."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    K, M = x.size, int(n_chains)
    if M == 1:
        return series_diagnostics(x, max_lag)
    N = check_chains(K, M)
    L, k_max = lag_cap(N, max_lag)
    y = x - _mean(x)
    g0 = float(y @ y)
    yc = y.reshape(M, N)
    nu = np.array([_mean(r) for r in yc])
    d = yc - nu[:, None]
    Q = K * float(((nu - nu.sum() / M) ** 2).sum()) / (M - 1)
    den = Q + float((d * d).sum())
    if den == 0.0:
        return dict(ess=math.nan, mcse=0.0, sd=0.0, rhat=math.nan, lags=0, truncated=False)
    sd = math.sqrt(g0 / (K - 1))
    h = N // 2
    seg = np.concatenate([np.stack([r[:h], r[N - h:]]) for r in d])   # 2M x h, about the chain's mean
    mu = seg.sum(axis=1) / h
    W = float((((seg - mu[:, None]) ** 2).sum(axis=1) / (h - 1)).sum()) / (2 * M)
    mj = np.repeat(nu, 2) + mu
    B = h / (2 * M - 1) * float(((mj - mj.sum() / (2 * M)) ** 2).sum())
    rhat = math.sqrt(((h - 1) / h * W + B / h) / W) if W != 0.0 else math.nan
    tsum, prev, pairs = 0.0, math.inf, 0
    for k in range(k_max + 1):
        t = 2 * k
        a0, a1 = float((d[:, :N - t] * d[:, t:]).sum()), float((d[:, :N - t - 1] * d[:, t + 1:]).sum())
        G = (Q + a0) / den + (Q + a1) / den
        if not G > 0.0:
            break
        G = min(G, prev)
        prev = G
        tsum += G
        pairs += 1
    tau = max(2.0 * tsum - 1.0, 1.0 / math.log10(K))
    ess = K / tau
    return dict(ess=ess, mcse=sd / math.sqrt(ess), sd=sd, rhat=rhat, lags=2 * pairs, truncated=pairs == k_max + 1)


def multichain_indicator_ess(I, n_chains=1, max_lag=0):
    """(ess, lags) of a 0/1 series of n_chains chains laid end to end: integer Num_t, one float division, the diagnostics' pairs."""
    I = np.asarray(I).astype(np.int64).reshape(-1)
    K, M = I.size, int(n_chains)
    if M == 1:
        return indicator_ess(I, max_lag)
    N = check_chains(K, M)
    Ic = I.reshape(M, N)
    cc = [int(v) for v in Ic.sum(axis=1)]
    C = sum(cc)
    if C == 0 or C == K:
        return math.nan, 0
    _, k_max = lag_cap(N, max_lag)
    D = sum((M * c - C) ** 2 for c in cc)

    def Num(t):
        S = 0
        for r, c in zip(Ic, cc):
            n11 = int(r[:N - t] @ r[t:])
            head, tail = int(r[:N - t].sum()), int(r[t:].sum())
            S += N * N * n11 - N * c * (head + tail) + (N - t) * c * c
        return N * D + M * (M - 1) * S
    Num0 = Num(0)
    nsum, prev, pairs = 0, None, 0
    for k in range(k_max + 1):
        Nk = Num(2 * k) + Num(2 * k + 1)
        if not Nk > 0:
            break
        Nk = Nk if prev is None else min(Nk, prev)
        prev = Nk
        nsum += Nk
        pairs += 1
    tau = max(float(2 * nsum - Num0) / float(Num0), 1.0 / math.log10(K))
    return K / tau, 2 * pairs


def multichain_rank_diagnostics(x, n_chains=1, probs=(), thresholds=(), sides=None, max_lag=0):
    """rank_series_diagnostics' dict of one series of n_chains chains laid end to end: ranks, scores, median and order statistics of
    the pooled draws, the moments and the indicator ESS by the multi-chain definition."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    K, M = x.size, int(n_chains)
    if M == 1:
        return rank_series_diagnostics(x, probs, thresholds, sides, max_lag)
    N = check_chains(K, M)
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
    bulk = multichain_diagnostics(rank_scores(x)[1], M, max_lag)
    med = xs[(K - 1) // 2] if K % 2 else 0.5 * (xs[K // 2 - 1] + xs[K // 2])
    fold = multichain_diagnostics(rank_scores(np.abs(x - med))[1], M, max_lag)
    qs = [multichain_indicator_ess(x <= xs[quantile_order(p, K)], M, max_lag) for p in probs]
    tails = [multichain_indicator_ess(x <= xs[quantile_order(p, K)], M, max_lag)[0] for p in (0.05, 0.95)]
    ex = [multichain_indicator_ess(x > t if s > 0 else x < t, M, max_lag) for t, s in zip(thresholds, sides)]
    cnt = [int(np.count_nonzero(x > t if s > 0 else x < t)) for t, s in zip(thresholds, sides)]
    prob = np.array([c / K for c in cnt], dtype=np.float64)
    mcse = np.array([0.0 if c in (0, K) else math.sqrt(p * (1.0 - p) / e[0]) for c, p, e in zip(cnt, prob, ex)], dtype=np.float64)
    return dict(rhat_rank=_fmax(bulk["rhat"], fold["rhat"]), rhat_bulk=bulk["rhat"], rhat_fold=fold["rhat"], ess_bulk=bulk["ess"],
                ess_tail=_fmin(tails[0], tails[1]), lags_bulk=bulk["lags"], truncated=bulk["truncated"],
                ess_q=np.array([e for e, _ in qs], dtype=np.float64), lags_q=np.array([l for _, l in qs], dtype=np.int32),
                ess_exc=np.array([e for e, _ in ex], dtype=np.float64), mcse_prob=mcse, prob=prob,
                lags_exc=np.array([l for _, l in ex], dtype=np.int32))


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
