"""Pareto-smoothed importance sampling of one series in 50-digit mpmath: the restatement the float64 definition
(spamtree_amd/psis.py) and the device kernel (k_loo_psis) are measured against.  Written from the text of Vehtari, Simpson, Gelman,
Yao, Gabry, "Pareto smoothed importance sampling" (tail length, the shift by the largest ratio, replacing the M largest ratios by the
quantiles of the fitted generalised Pareto distribution, truncation at the largest raw ratio) and of Zhang and Stephens (2009), "A new
and efficient estimation method for the generalized Pareto distribution" (the profile-likelihood grid and its posterior-mean weights),
with the weakly informative prior of the first paper's appendix (khat shrunk towards 0.5 with the weight of ten observations), r_eff = 1.
Nothing here imports spamtree_amd.

Also the case list of the CPU and GPU tests: ``case_list`` builds every series once, ``reference`` evaluates them once per process.
"""
import functools
import math

import mpmath as mp
import numpy as np

mp.mp.dps = 50
F = mp.mpf

# measured (tests/test_psis_cpu.py has the figures): the float64 definition's largest ``distance`` from this restatement over the case
# list, and per shape k the largest |khat - k| of this restatement over 200 seeds of 4000 generalised Pareto draws, times 1.5
F64_DISTANCE = 1.9e-13
DEVICE_FACTOR = 256
KHAT_BAND = {-0.3: 0.311, 0.1: 0.360, 0.5: 0.477, 0.9: 0.590, 1.5: 0.718}


def tail_length_rational(S):
    """min(floor(S / 5), ceil(3 sqrt S)) with math.isqrt: ceil(3 sqrt S) = ceil(sqrt(9 S))."""
    r = math.isqrt(9 * S)
    return min(S // 5, r if r * r == 9 * S else r + 1)


def gpd_fit(x):
    """(khat, sigma) of Zhang and Stephens' estimator with the prior, of ascending positive exceedances (mpf); None: not defined."""
    N = len(x)
    G = 30 + math.isqrt(N)
    xs = x[(N + 2) // 4 - 1]
    if xs == 0:
        return None
    theta = [1 / x[-1] + (1 - mp.sqrt(F(G) / (F(j) - F(1) / 2))) / (3 * xs) for j in range(1, G + 1)]
    try:
        kj = [mp.fsum(mp.log1p(-th * xi) for xi in x) / N for th in theta]
        lj = [N * (mp.log(-th / k) - k - 1) for th, k in zip(theta, kj)]
    except (ZeroDivisionError, ValueError):
        return None
    om = [1 / mp.fsum(mp.exp(li - l) for li in lj) for l in lj]
    th = mp.fsum(t * o for t, o in zip(theta, om))
    k = mp.fsum(mp.log1p(-th * xi) for xi in x) / N
    sigma = -k / th
    khat = (k * N + 5) / (N + 10)
    if not (mp.isfinite(khat) and mp.isfinite(sigma)):
        return None
    return khat, sigma


def series(t, phi=None, mu=None):
    """dict(khat, sigma, elpd_psis, pit_psis, mu_psis, weight_ess_psis: mpf or float inf / nan; tail_len, n_draws, smoothed)."""
    t = np.asarray(t, dtype=np.float64)
    idx = [s for s in range(t.size) if np.isfinite(t[s])]
    S = len(idx)
    nan = float("nan")
    out = dict(khat=nan, sigma=nan, elpd_psis=nan, pit_psis=nan, mu_psis=nan, weight_ess_psis=nan, tail_len=0, n_draws=S, smoothed=False)
    if S == 0:
        return out
    tv = [F(float(t[s])) for s in idx]
    c = max(tv)
    lw = [v - c for v in tv]
    lws = list(lw)
    out["khat"] = float("inf")
    M = tail_length_rational(S)
    if M >= 5:
        order = sorted(range(S), key=lambda a: (tv[a], a))
        tail = order[S - M:]
        if tv[tail[-1]] != tv[tail[0]]:
            cut = lw[order[S - M - 1]]
            ecut = mp.exp(cut)
            # the exceedances as the float64 definition sees them: exp underflows below about -745, where a double is exactly 0
            x = [mp.exp(lw[a]) - ecut for a in tail]
            xq = x[(M + 2) // 4 - 1]
            if float(mp.exp(lw[tail[(M + 2) // 4 - 1]])) - float(ecut) != 0.0 and xq != 0:
                fit = gpd_fit(x)
                if fit is not None:
                    khat, sigma = fit
                    for j in range(1, M + 1):
                        p = (F(j) - F(1) / 2) / M
                        q = -sigma * mp.log1p(-p) if khat == 0 else sigma * mp.expm1(-khat * mp.log1p(-p)) / khat
                        lws[tail[j - 1]] = min(mp.log(q + ecut), F(0))
                    out.update(khat=khat, sigma=sigma, tail_len=M, smoothed=True)
    e = [mp.exp(v) for v in lws]
    W1, W2 = mp.fsum(e), mp.fsum(v * v for v in e)
    U = mp.fsum(mp.exp(a - b) for a, b in zip(lws, lw))
    out["elpd_psis"] = -c + mp.log(U) - mp.log(W1)
    out["weight_ess_psis"] = W1 * W1 / W2
    if phi is not None:
        out["pit_psis"] = mp.fsum(w * F(float(phi[s])) for w, s in zip(e, idx)) / W1
    if mu is not None:
        out["mu_psis"] = mp.fsum(w * F(float(mu[s])) for w, s in zip(e, idx)) / W1
    return out


# ---- the case list: (name, K, t, phi, mu) ----
KS = (4, 24, 25, 63, 64, 65, 100, 1000, 1025, 8192, 8193, 16384)
DOUBLES = ("khat", "elpd_psis", "pit_psis", "mu_psis", "weight_ess_psis")


def _gpd(rng, k, K):
    """log of generalised Pareto draws of shape k (inverse cdf), shifted so that the ratios are of order one."""
    u = rng.random(K)
    r = -np.log1p(-u) if k == 0 else np.expm1(-k * np.log1p(-u)) / k
    return np.log(r + 1e-3)


def make_series(kind, K, seed):
    """(t, phi, mu) of one series of K draws."""
    rng = np.random.default_rng([seed, K, sum(map(ord, kind))])
    phi, mu = rng.random(K), rng.standard_normal(K)
    if kind.startswith("gpd"):
        t = _gpd(rng, float(kind[3:]), K)
    elif kind == "gauss":
        t = 1.3 * rng.standard_normal(K) + 2.0
    elif kind == "range":           # a range above 1500: exp underflows below the cut
        t = np.sort(rng.standard_normal(K))
        t = t + np.linspace(-1600.0, 0.0, K)
        t = t[rng.permutation(K)]
    elif kind == "sprinkled":       # NaN / +-inf draws: S differs per series
        t = 0.8 * rng.standard_normal(K)
        bad = rng.random(K) < (0.45 if seed % 2 else 0.1)
        t[bad] = rng.choice([np.nan, np.inf, -np.inf], size=int(bad.sum()))
    elif kind == "skipped":
        t = np.full(K, np.nan)
        t[::3] = np.inf
    elif kind == "ties":            # exact ties straddling the cut, different companions on the tied draws
        t = np.round(rng.standard_normal(K), 1 if K >= 60 else 0)
        M = tail_length_rational(K)
        if M >= 5:
            srt = np.sort(t)
            v = srt[K - M]          # the smallest tail value: make sure it also occurs below the cut
            t[rng.choice(K, size=min(3, K), replace=False)] = v
    elif kind == "const_tail":
        t = rng.standard_normal(K) - 5.0
        M = max(tail_length_rational(K), 1)
        t[rng.choice(K, size=min(K, M + 2), replace=False)] = 1.5
    elif kind == "quarter":         # a quarter of the tail equal to the cut
        t = rng.standard_normal(K)
        M = tail_length_rational(K)
        if M >= 5:
            srt = np.sort(t)
            cutv = srt[K - M - 1]
            order = np.argsort(t, kind="stable")
            t[order[K - M:K - M + (M + 2) // 4]] = cutv
    else:
        raise ValueError(kind)
    return t, phi, mu


KINDS = ("gpd-0.3", "gpd0.5", "gpd1.5", "gauss", "range", "sprinkled", "skipped", "ties", "const_tail", "quarter")


@functools.lru_cache(maxsize=None)
def case_list():
    """Every store of the case list: tuple of (name, t [K][n], phi, mu); column i of a store is series kind KINDS[i % len(KINDS)].
    K in KS; n in {1, 7, 9, 300} for the short K, n in {1, 7, 9} spread over the long ones (the large K only need n <= 9)."""
    cases = []
    for a, K in enumerate(KS):
        if K <= 100:
            ns = (1, 7, 9, 300) if K in (25, 64) else (9,) if K in (4, 24) else (7, 9)
        else:
            ns = {1000: (9,), 1025: (7,), 8192: (1,), 8193: (7,), 16384: (9,)}[K]
        for n in ns:
            cols = [make_series(KINDS[(i + a) % len(KINDS)], K, 1000 * n + i) for i in range(n)]
            t, phi, mu = (np.ascontiguousarray(np.stack([c[k] for c in cols], axis=1)) for k in range(3))
            cases.append((f"K{K}_n{n}", t, phi, mu))
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement's outputs of every column of case ``name``: list of ``series`` dicts."""
    for nm, t, phi, mu in case_list():
        if nm == name:
            return [series(t[:, i], phi[:, i], mu[:, i]) for i in range(t.shape[1])]
    raise KeyError(name)


def distance(ref, got, keys=DOUBLES):
    """max over ``keys`` of |got - ref| / max(|ref|, 1) for one series (ref: ``series``' dict; got: a dict of floats); the NaN / inf
    pattern must agree exactly (AssertionError)."""
    worst = 0.0
    for k in keys:
        r, g = ref[k], float(got[k])
        if isinstance(r, float) and (math.isnan(r) or math.isinf(r)):
            assert (math.isnan(r) and math.isnan(g)) or r == g, (k, r, g)
            continue
        assert math.isfinite(g), (k, r, g)
        worst = max(worst, float(abs(F(g) - r) / max(abs(r), 1)))
    return worst
