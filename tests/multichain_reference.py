"""The definition of the multi-chain diagnostics (include/spamtree_hip.h, st_*_chain_diagnostics and st_*_chain_rank_diagnostics)
restated, sharing no code with the library: the moments in np.longdouble, the indicator ESS in Python integers and exact rationals
(fractions.Fraction) up to the final division, the normal scores from tests/rank_reference.py (mpmath).

A series x_0 .. x_{K-1}, K = M N, is M chains x_{c,s} = x_{cN+s}, c < M, s < N;  1 <= M <= 16, N >= 4, K <= 16384.
  L = min(max_lag, N - 2), max_lag = 0 meaning 1024;  k_max = (L - 1) // 2
  mu_c = mean of chain c;  d_{c,s} = x_{c,s} - mu_c;  gamma_{c,t} = (1/N) sum_{s<N-t} d_{c,s} d_{c,s+t};  gbar_t = (1/M) sum_c gamma_{c,t}
  mubar = (1/M) sum_c mu_c;  B' = sum_c (mu_c - mubar)^2 / (M - 1)  (0 at M = 1)
  rho_t = (B' + gbar_t) / (B' + gbar_0);  Gamma_k = rho_2k + rho_2k+1, stop at the first not (Gamma_k > 0), Gamma_k <- min(Gamma_k, Gamma_k-1)
  tau = -1 + 2 sum Gamma_k, floored at 1 / log10 K;  ess = K / tau;  lags = 2 x pairs added;  truncated: the loop ended at k_max
  sd = the pooled sd of the K draws about the pooled mean, divisor K - 1;  mcse = sd / sqrt(ess)
  h = N // 2;  the S = 2M segments x_c[:h], x_c[N-h:], means m_j, sample variances s_j^2 (divisor h - 1);  W = (1/S) sum s_j^2;
  B = h / (S - 1) sum (m_j - mbar)^2;  rhat = sqrt(((h-1)/h W + B/h) / W)
  B' + gbar_0 == 0: ess NaN, mcse 0, sd 0, rhat NaN, lags 0;  W == 0 otherwise: rhat NaN only
  indicator (M >= 2): c_c = sum_s I_{c,s};  A_{c,t} = N^2 n11 - N c_c (head + tail) + (N - t) c_c^2 on chain c alone;  C = sum c_c;
  D = sum_c (M c_c - C)^2;  S_t = sum_c A_{c,t};  Num_t = N D + M (M - 1) S_t;  rho_t = Num_t / Num_0;  C in {0, K}: ess NaN, lags 0
  rank family: ranks, scores, median, folded series and xs[j] of the pooled K draws; the moments and indicator ESS as above.
"""
import math
from fractions import Fraction

import numpy as np

from tests import rank_reference as rr
from tests.diag_reference import LD, lag_cap

MAX_CHAINS = 16


def _mean(x):
    m0 = LD(math.fsum(float(v) for v in x)) / LD(x.size) if x.dtype == np.float64 else x.sum() / LD(x.size)
    x = x.astype(LD)
    return m0 + (x - m0).sum() / LD(x.size)


def moments(x, n_chains, max_lag=0, lags=True):
    """Long double, of a float64 or long-double series: dict(ess, mcse, sd, rhat, lags, truncated) as floats and what a test's bound
    needs: tau (floored), tsum, pairs, min_abs_gamma (the smallest |Gamma_k| visited, the stopping one included; inf if none),
    den (= B' + gbar_0), Bp (= B'), gamma0 (the pooled divisor-K variance), max_abs_x, max_abs_y (about the pooled mean), max_abs_d
    (about the chain means), W, B, N, M.  Without ``lags`` the pairs are not walked (ess, mcse NaN)."""
    x0 = np.asarray(x)
    x = x0.astype(LD)
    K, M = x.size, int(n_chains)
    assert 1 <= M <= MAX_CHAINS and K % M == 0 and K // M >= 4
    N = K // M
    _, k_max = lag_cap(N, max_lag)
    y = x - _mean(x0 if x0.dtype == np.float64 else x)
    g0 = (y @ y) / LD(K)
    xc = x.reshape(M, N)
    mu = np.array([_mean(np.asarray(r, dtype=x0.dtype if x0.dtype == np.float64 else LD)) for r in x0.reshape(M, N)], dtype=LD)
    d = xc - mu[:, None]
    Bp = ((mu - mu.sum() / LD(M)) ** 2).sum() / LD(M - 1) if M > 1 else LD(0)
    gbar0 = (d * d).sum() / LD(K)
    den = Bp + gbar0
    extra = dict(den=float(den), Bp=float(Bp), gamma0=float(g0), max_abs_x=float(np.abs(x).max()), max_abs_y=float(np.abs(y).max()),
                 max_abs_d=float(np.abs(d).max()), N=N, M=M)
    if den == 0:
        return dict(ess=math.nan, mcse=0.0, sd=0.0, rhat=math.nan, lags=0, truncated=False, tau=math.nan, tsum=0.0, pairs=0,
                    min_abs_gamma=math.inf, W=0.0, B=0.0, **extra)
    sd = np.sqrt(LD(K) / LD(K - 1) * g0)
    tsum, prev, pairs, mag = LD(0), LD(np.inf), 0, math.inf
    for k in range(k_max + 1 if lags else 0):
        t = 2 * k
        r0 = (Bp + (d[:, :N - t] * d[:, t:]).sum() / LD(K)) / den
        r1 = (Bp + (d[:, :N - t - 1] * d[:, t + 1:]).sum() / LD(K)) / den
        G = r0 + r1
        mag = min(mag, abs(float(G)))
        if not G > 0:
            break
        G = min(G, prev)
        prev = G
        tsum += G
        pairs += 1
    tau = max(2 * tsum - 1, 1 / np.log10(LD(K)))
    ess = LD(K) / tau
    h = N // 2
    seg = np.concatenate([np.stack([r[:h], r[N - h:]]) for r in xc])
    mj = np.array([s.sum() / LD(h) for s in seg - mu.repeat(2)[:, None]], dtype=LD) + mu.repeat(2)
    sj = np.array([((s - m) @ (s - m)) / LD(h - 1) for s, m in zip(seg, mj)], dtype=LD)
    S = 2 * M
    W = sj.sum() / LD(S)
    B = LD(h) / LD(S - 1) * ((mj - mj.sum() / LD(S)) ** 2).sum()
    rhat = float(np.sqrt((LD(h - 1) / LD(h) * W + B / h) / W)) if W != 0 else math.nan
    return dict(ess=float(ess) if lags else math.nan, mcse=float(sd / np.sqrt(ess)) if lags else math.nan, sd=float(sd), rhat=rhat,
                lags=2 * pairs, truncated=bool(lags) and pairs == k_max + 1, tau=float(tau), tsum=float(tsum), pairs=pairs, min_abs_gamma=mag,
                W=float(W), B=float(B), **extra)


def reference(x, n_chains, max_lag=0):
    return moments(np.asarray(x, dtype=np.float64), n_chains, max_lag)


def chain_A(I, t):
    """A_t of one chain's 0/1 list in Python integers."""
    N, c = len(I), sum(I)
    n11 = sum(I[s] & I[s + t] for s in range(N - t)) if N <= 512 else int(np.asarray(I[:N - t], dtype=np.int64) @ np.asarray(I[t:], dtype=np.int64))
    head, tail = sum(I[:N - t]), sum(I[t:])
    return N * N * n11 - N * c * (head + tail) + (N - t) * c * c


def indicator_num(I, n_chains, t):
    """Num_t in Python integers."""
    I = [int(bool(v)) for v in I]
    M = int(n_chains)
    N = len(I) // M
    ch = [I[c * N:(c + 1) * N] for c in range(M)]
    C = sum(I)
    D = sum((M * sum(r) - C) ** 2 for r in ch)
    return N * D + M * (M - 1) * sum(chain_A(r, t) for r in ch)


def indicator_ess(I, n_chains, max_lag=0):
    """(ess, lags, min_abs_gamma, worst) of a 0/1 series of M >= 2 chains: Num_t in Python integers, rho_t and tau in exact rationals,
    the floor and the final division in long double.  The integer bounds of the definition are asserted on the way: N D <= K^3 / 4,
    |M (M - 1) S_t| < K^3 / 4, |Num_t| < 2^41, |2 sum N_k - Num_0| < 2^57; ``worst`` = (max |Num_t|, |2 sum N_k - Num_0|)."""
    I = [int(bool(v)) for v in I]
    K, M, C = len(I), int(n_chains), sum(I)
    assert 2 <= M <= MAX_CHAINS and K % M == 0 and K // M >= 4 and K <= 16384
    N = K // M
    if C == 0 or C == K:
        return math.nan, 0, math.inf, (0, 0)
    _, k_max = lag_cap(N, max_lag)
    ch = [I[c * N:(c + 1) * N] for c in range(M)]
    cc = [sum(r) for r in ch]
    D = sum((M * c - C) ** 2 for c in cc)
    assert 4 * N * D <= K ** 3
    Num0 = N * D + M * (M - 1) * sum(N * c * (N - c) for c in cc)
    assert Num0 == indicator_num(I, M, 0) and Num0 > 0
    # (M - 1) M^2 N^3 (B' + gbar_0) in rationals, from the chain means and variances themselves
    p = [Fraction(c, N) for c in cc]
    pbar = sum(p) / M
    assert Num0 == (M - 1) * M * M * N ** 3 * (sum((v - pbar) ** 2 for v in p) / (M - 1) + sum(v * (1 - v) for v in p) / M)
    tsum, prev, pairs, mag, big, nsum = Fraction(0), None, 0, math.inf, Num0, 0
    for k in range(k_max + 1):
        nums = []
        for t in (2 * k, 2 * k + 1):
            St = sum(chain_A(r, t) for r in ch)
            assert 4 * abs(M * (M - 1) * St) < K ** 3
            nums.append(N * D + M * (M - 1) * St)
            assert abs(nums[-1]) < 2 ** 41
            big = max(big, abs(nums[-1]))
        G = Fraction(nums[0], Num0) + Fraction(nums[1], Num0)
        mag = min(mag, abs(float(G)))
        if not G > 0:
            break
        if prev is not None:
            G = min(G, prev)
        prev = G
        tsum += G
        nsum += G * Num0   # the integer the device adds: min() keeps one of the N_k
        pairs += 1
    assert nsum.denominator == 1 and abs(2 * int(nsum) - Num0) < 2 ** 57
    raw = 2 * tsum - 1
    tau = max(LD(raw.numerator) / LD(raw.denominator), 1 / np.log10(LD(K)))
    return float(LD(K) / tau), 2 * pairs, mag, (big, abs(2 * int(nsum) - Num0))


def rank_reference(x, n_chains, probs=(), thresholds=(), sides=None, max_lag=0, want_z=True):
    """Every output of one series of M >= 2 chains, as tests/rank_reference.reference lays them out (``bulk`` and ``fold`` are the
    records of ``moments`` above)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    K, M = x.size, int(n_chains)
    sides = [1] * len(thresholds) if sides is None else list(sides)
    nq, nt = len(probs), len(thresholds)
    if np.isnan(x).any():
        return dict(rhat_rank=math.nan, rhat_bulk=math.nan, rhat_fold=math.nan, ess_bulk=math.nan, ess_tail=math.nan, lags_bulk=0,
                    truncated=False, ess_q=[math.nan] * nq, lags_q=[0] * nq, ess_exc=[math.nan] * nt, lags_exc=[0] * nt,
                    prob=[math.nan] * nt, mcse_prob=[math.nan] * nt, bulk=None, fold=None)
    xs = np.sort(x)
    out = {}
    if want_z:
        bulk = moments(rr.scores(x), M, max_lag)
        med = xs[(K - 1) // 2] if K % 2 else 0.5 * (xs[K // 2 - 1] + xs[K // 2])
        fold = moments(rr.scores(np.abs(x - med)), M, max_lag, lags=False)
        out.update(rhat_bulk=bulk["rhat"], ess_bulk=bulk["ess"], lags_bulk=bulk["lags"], truncated=bulk["truncated"],
                   rhat_fold=fold["rhat"], rhat_rank=rr.fmax(bulk["rhat"], fold["rhat"]), bulk=bulk, fold=fold)
    q = [indicator_ess(x <= xs[rr.quantile_order(p, K)], M, max_lag) for p in probs]
    tl = [indicator_ess(x <= xs[rr.quantile_order(p, K)], M, max_lag) for p in (0.05, 0.95)]
    ind = [(x > float(t)) if s > 0 else (x < float(t)) for t, s in zip(thresholds, sides)]
    e = [indicator_ess(I, M, max_lag) for I in ind]
    cnt = [int(np.count_nonzero(I)) for I in ind]
    prob = [c / K for c in cnt]
    mcse = [0.0 if c in (0, K) else float(np.sqrt(LD(p) * (1 - LD(p)) / LD(v[0]))) for c, p, v in zip(cnt, prob, e)]
    out.update(ess_q=[v[0] for v in q], lags_q=[v[1] for v in q], mag_q=[v[2] for v in q], ess_tail=rr.fmin(tl[0][0], tl[1][0]),
               lags_tail=[v[1] for v in tl], mag_tail=[v[2] for v in tl], ess_exc=[v[0] for v in e], lags_exc=[v[1] for v in e],
               mag_exc=[v[2] for v in e], prob=prob, mcse_prob=mcse, count=cnt)
    return out


U = 2.0 ** -53


def chain_bounds(rec, K, pairs_other, eps_phi=0.0):
    """Relative bounds on ess, mcse, sd, rhat of the device's multi-chain diagnostics from a ``moments`` record: the single-chain
    derivation (tests/test_gpu_diagnostics.py, series_bounds; tests/rank_reference.score_bounds for a score series whose every value
    is off by at most eta = eps_phi max|x|) extended for the B' term; first order, then doubled, the neglected products asserted
    below 1e-6.
    With u = 2^-53, N = K / M, D = ceil(K / 64) + 6 additions behind a pooled sum, Dc = ceil(N / 64) + 6 behind a chain's (a lag sum
    over the chains has at most ceil(N / 64) M <= ceil(K / 64) + M terms per lane: Dl = D + M), A = max|x|, Y = max|y| about the
    pooled mean, Dm = max|d| about the chain means, v = B' + gbar_0, s = sqrt(v):
      y_s        x_s - m with m off by a common shift delta <= u A + (D + 2) u Y, to which everything below but the pooled sum of
                 squares is invariant (that one moves by K delta^2: delta^2 / gamma_0 relative); its own rounding u Y; so each y
                 is within e_y = u Y + 2 eta of a shifted x
      nu_c       (chain mean less m) within e_nu = e_y + (Dc + 2) u Dm + u Y   (C1's two passes: the first's error cancels)
      d_s        within e_d = e_nu + e_y + u Dm
      a_t        sum |d d'| <= K gbar_0 <= K v;  relative to K v:  (Dl + 2) u + 2 e_d sqrt(gbar_0) / v <= (Dl + 2) u + 2 e_d / s
      Q = K B'   nu_c - nb within 2 e_nu + (10 + 2) u Y (the butterfly of M lane values: 6 levels, the division, the subtraction);
                 sum_c |nu_c - nb| <= sqrt(M (M - 1) B'), so Q / K within 2 sqrt(M / (M - 1)) sqrt(B') e_b + 9 u B',
                 e_b = 2 e_nu + 12 u Y;  relative to v: <= 2 sqrt(2) e_b / s + 9 u
      rho_t      e_a = (Dl + 4) u + 2 e_d / s + 2 sqrt(2) e_b / s + 9 u for numerator and denominator alike
      Gamma_k    e_G = 4 e_a + 4 u;  tau, ess, sd, mcse as in series_bounds (sd is the pooled P3 chain: e_sd = (D + 2) u / 2 +
                 2 (u Y + 2 eta) / sqrt(gamma_0) + delta^2 / gamma_0 + 2 u)
      rhat       a segment mean less its chain's within e_m = e_d + (Dc + 3) u Dm, a segment mean m_j within e_mj = e_m + e_nu + u Y;
                 an element d_s - mu_j within e_e = e_d + e_m + u Dm;  W within e_W = (Dc + 12) u + 3 e_e / sqrt(W) relative;
                 B = h / (S - 1) sum (m_j - mb)^2 within dB = 2 sqrt(h S / (S - 1)) sqrt(B) (2 e_mj) + h S / (S - 1) (2 e_mj)^2 + 12 u B;
                 rhat^2 = (h - 1) / h + B / (h W), so rhat within ((dB + B e_W) / (h W)) / (2 rhat^2) + 4 u."""
    N, M = rec["N"], rec["M"]
    D, Dc = -(-K // 64) + 6, -(-N // 64) + 6
    Dl = D + M
    Y, Dm, s = rec["max_abs_y"], rec["max_abs_d"], math.sqrt(rec["den"])
    eta = eps_phi * rec["max_abs_x"]
    delta = U * rec["max_abs_x"] + (D + 2) * U * Y
    e_y = U * Y + 2 * eta
    e_nu = e_y + (Dc + 2) * U * Dm + U * Y
    e_d = e_nu + e_y + U * Dm
    e_b = 2 * e_nu + 12 * U * Y
    e_a = (Dl + 4) * U + 2 * e_d / s + 2 * math.sqrt(2) * e_b / s + 9 * U
    assert e_a < 1e-6
    e_G = 4 * e_a + 4 * U
    b = dict(e_G=e_G)
    e_sd = (D + 2) * U / 2 + 2 * e_y / math.sqrt(rec["gamma0"]) + delta * delta / rec["gamma0"] + 2 * U
    b["sd"] = 2 * e_sd
    if not math.isnan(rec["tau"]) and not math.isnan(rec["ess"]):
        P = max(rec["pairs"], pairs_other)
        e_tau = 4 * P * e_G + 2 * P * U * rec["tsum"] + 4 * U * (2 * rec["tsum"] + 1) + 4 * U * rec["tau"]
        e_ess = e_tau / rec["tau"] + U
        b.update(ess=2 * e_ess, mcse=2 * (e_sd + e_ess / 2 + 2 * U))
    if rec["W"] > 0:
        h, S = N // 2, 2 * M
        e_m = e_d + (Dc + 3) * U * Dm
        e_mj = e_m + e_nu + U * Y
        e_e = e_d + e_m + U * Dm
        e_W = (Dc + 12) * U + 3 * e_e / math.sqrt(rec["W"])
        assert e_W < 1e-6
        f = h * S / (S - 1)
        dB = 2 * math.sqrt(f * rec["B"]) * 2 * e_mj + f * (2 * e_mj) ** 2 + 12 * U * rec["B"]
        b["rhat"] = 2 * (((dB + rec["B"] * e_W) / (h * rec["W"])) / (2 * rec["rhat"] ** 2) + 4 * U)
    return b


def abab(N, levels=(0.0, 3.0), phi=0.5, seed=1):
    """Four chains of N draws at levels A, B, A, B with AR(1) noise, laid end to end."""
    from tests.diag_reference import ar1
    return np.concatenate([ar1(N, phi, seed=seed * 10 + c) + levels[c % 2] for c in range(4)])
