"""The definition of the rank-normalised diagnostics (include/spamtree_hip.h, st_*_rank_diagnostics) restated, sharing no code with
the library: ranks and A_t in Python integers, rho_t and tau of the indicator series in exact rationals up to the final division,
Phi^-1 from mpmath at 50 digits, the moments and lag sums of the normal scores in np.longdouble (as tests/diag_reference.py).

One series x_0 .. x_{K-1}, 4 <= K <= 16384; xs its ascending sort.  "the diagnostics" are those of tests/diag_reference.py.
  ranks      lo_s = #{u : x_u < x_s}, hi_s = #{u : x_u <= x_s};  r2_s = lo_s + hi_s + 1
  scores     p_s = (4 r2_s - 3) / (8 K + 2), ONE double division (the library's p is this double);  z_s = Phi^-1(p_s)
  bulk       rhat_bulk, ess_bulk, lags_bulk = the diagnostics' rhat, ess, lags on z
  folded     med = xs[(K-1)/2] (K odd), 0.5 (xs[K/2-1] + xs[K/2]) (K even), in float64 as the library forms it;
             f_s = |x_s - med| (float64);  zf = the scores of f;  rhat_fold = the diagnostics' rhat on zf;
             rhat_rank = fmax(rhat_bulk, rhat_fold)
  indicator  c = sum I: c in {0, K}: ess = NaN, lags = 0; else A_t = K^2 n11_t - K c (head_t + tail_t) + (K - t) c^2,
             rho_t = A_t / A_0, an exact rational, then the diagnostics' pairs, tau, floor, ess = K / tau
  quantile   j = min(max(ceil(prob K), 1), K - 1) - 1 (prob K one double multiplication);  I_s = [x_s <= xs[j]]
  tail       ess_tail = fmin(indicator ESS at 0.05, at 0.95)
  exceedance I_s = [x_s > thr] or [x_s < thr];  prob = c / K;  mcse_prob = sqrt(prob (1 - prob) / ess), 0 where c is 0 or K
  a NaN draw: NaN in every float output, 0 in the lags.
"""
import bisect
import math
import statistics
from fractions import Fraction

import mpmath as mp
import numpy as np

from tests.diag_reference import LD, lag_cap

mp.mp.dps = 50
_PPF, _PPF_LD = {}, {}
_START = statistics.NormalDist()


def norm_ppf(p):
    """Phi^-1 of the double p as an mpmath number, 50 digits: the root of mpmath's ncdf(z) - p by Newton's iteration until the
    step falls below 1e-40 of z.  The start (the standard library's double-precision inverse) only decides how many steps it
    takes -- two from a start good to 1e-16; the root is ncdf's alone.  Cached by p."""
    p = float(p)
    z = _PPF.get(p)
    if z is None:
        tail = min(p, 1.0 - p)
        extra = 0 if tail > 1e-6 else int(-math.log10(tail)) + 10   # 2 p - 1 needs the digits of the tail
        with mp.workdps(50 + extra):
            P = mp.mpf(p)
            if P == mp.mpf(1) / 2:
                z = mp.mpf(0)
            else:
                z = mp.mpf(_START.inv_cdf(p))
                for _ in range(12):
                    step = (mp.ncdf(z) - P) / mp.npdf(z)
                    z = z - step
                    if abs(step) <= mp.mpf(10) ** -40 * abs(z):
                        break
                else:
                    raise ArithmeticError(f"Newton's iteration for Phi^-1({p!r}) did not settle")
        _PPF[p] = +z
    return z


def to_ld(z):
    """An mpmath number as np.longdouble (through 25 significant digits: more than the 64-bit significand holds)."""
    return LD(mp.nstr(z, 25, strip_zeros=False))


def twice_ranks(v):
    """r2_s = lo_s + hi_s + 1 in Python integers."""
    v = [float(t) for t in v]
    s = sorted(v)
    return [bisect.bisect_left(s, t) + bisect.bisect_right(s, t) + 1 for t in v]


def score_p(r2, K):
    return float(4 * r2 - 3) / float(8 * K + 2)


def scores(v):
    """The normal scores of a series in long double."""
    K = len(v)
    out = np.empty(K, dtype=LD)
    for s, r in enumerate(twice_ranks(v)):
        p = score_p(r, K)
        z = _PPF_LD.get(p)
        if z is None:
            z = _PPF_LD[p] = to_ld(norm_ppf(p))
        out[s] = z
    return out


def moments(z, max_lag=0, lags=True):
    """The diagnostics of a long-double series (tests/diag_reference.reference's arithmetic, which takes float64 input only, on z
    itself): dict(ess, rhat, lags, truncated) and what a test's bound needs (tau, tsum, pairs, min_abs_gamma, gamma0, max_abs_x,
    max_abs_d, W, dmu).  Without ``lags`` the pairs are not walked (ess NaN)."""
    z = np.asarray(z, dtype=LD)
    K = z.size
    _, k_max = lag_cap(K, max_lag)
    m0 = z.sum() / LD(K)
    m = m0 + (z - m0).sum() / LD(K)
    d = z - m
    g0 = (d @ d) / LD(K)
    extra = dict(gamma0=float(g0), max_abs_x=float(np.abs(z).max()), max_abs_d=float(np.abs(d).max()))
    if g0 == 0:
        return dict(ess=math.nan, rhat=math.nan, lags=0, truncated=False, tau=math.nan, tsum=0.0, pairs=0, min_abs_gamma=math.inf,
                    W=0.0, dmu=0.0, **extra)
    tsum, prev, pairs, mag = LD(0), LD(np.inf), 0, math.inf
    for k in range(k_max + 1 if lags else 0):
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
    h = K // 2
    a, b = z[:h], z[K - h:]
    m1, m2 = a.sum() / LD(h), b.sum() / LD(h)
    s1 = ((a - m1) @ (a - m1)) / LD(h - 1)
    s2 = ((b - m2) @ (b - m2)) / LD(h - 1)
    W = (s1 + s2) / 2
    mb = (m1 + m2) / 2
    B = h * ((m1 - mb) ** 2 + (m2 - mb) ** 2)
    rhat = float(np.sqrt((LD(h - 1) / LD(h) * W + B / h) / W)) if W != 0 else math.nan
    return dict(ess=float(LD(K) / tau) if lags else math.nan, rhat=rhat, lags=2 * pairs, truncated=lags and pairs == k_max + 1,
                tau=float(tau), tsum=float(tsum), pairs=pairs, min_abs_gamma=mag, W=float(W), dmu=float(abs(m1 - m2)), **extra)


def indicator_A(I, t):
    """A_t of a 0/1 list in Python integers (the sums themselves by exact int64 dot products)."""
    I = np.asarray(I, dtype=np.int64)
    K = int(I.size)
    c = int(I.sum())
    n11 = int(I[:K - t] @ I[t:])
    head, tail = int(I[:K - t].sum()), int(I[t:].sum())
    return K * K * n11 - K * c * (head + tail) + (K - t) * c * c


def indicator_ess(I, max_lag=0):
    """(ess, lags, min_abs_gamma) of a 0/1 series: rho_t and tau in exact rationals, the floor and the final division in long
    double."""
    I = [int(bool(v)) for v in I]
    K, c = len(I), sum(I)
    if c == 0 or c == K:
        return math.nan, 0, math.inf
    _, k_max = lag_cap(K, max_lag)
    A0 = K * c * (K - c)
    assert indicator_A(I, 0) == A0
    tsum, prev, pairs, mag = Fraction(0), None, 0, math.inf
    for k in range(k_max + 1):
        a0, a1 = indicator_A(I, 2 * k), indicator_A(I, 2 * k + 1)
        assert abs(a0) <= 2 ** 42 and abs(a1) <= 2 ** 42
        G = Fraction(a0, A0) + Fraction(a1, A0)
        mag = min(mag, abs(float(G)))
        if not G > 0:
            break
        if prev is not None:
            G = min(G, prev)
        prev = G
        tsum += G
        pairs += 1
    raw = 2 * tsum - 1
    tau = max(LD(raw.numerator) / LD(raw.denominator), 1 / np.log10(LD(K)))
    return float(LD(K) / tau), 2 * pairs, mag


def quantile_order(prob, K):
    return min(max(int(math.ceil(float(prob) * K)), 1), K - 1) - 1


def fmin(a, b):
    return b if math.isnan(a) else a if math.isnan(b) else min(a, b)


def fmax(a, b):
    return b if math.isnan(a) else a if math.isnan(b) else max(a, b)


def reference(x, probs=(), thresholds=(), sides=None, max_lag=0, want_z=True):
    """Every output of one series: dict(rhat_rank, rhat_bulk, rhat_fold, ess_bulk, ess_tail, lags_bulk, truncated; ess_q, lags_q,
    mag_q per probability; ess_exc, lags_exc, mag_exc, prob, mcse_prob, count per threshold; lags_tail, mag_tail (two entries);
    ``bulk`` and ``fold``: the records of ``moments`` for the tests' bounds).  ``want_z`` False leaves the score-defined outputs
    out (the integer-defined ones cost far less)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    K = x.size
    sides = [1] * len(thresholds) if sides is None else list(sides)
    nq, nt = len(probs), len(thresholds)
    if np.isnan(x).any():
        return dict(rhat_rank=math.nan, rhat_bulk=math.nan, rhat_fold=math.nan, ess_bulk=math.nan, ess_tail=math.nan, lags_bulk=0,
                    truncated=False, ess_q=[math.nan] * nq, lags_q=[0] * nq, ess_exc=[math.nan] * nt, lags_exc=[0] * nt,
                    prob=[math.nan] * nt, mcse_prob=[math.nan] * nt, bulk=None, fold=None)
    xs = np.sort(x)
    out = {}
    if want_z:
        bulk = moments(scores(x), max_lag)
        med = xs[(K - 1) // 2] if K % 2 else 0.5 * (xs[K // 2 - 1] + xs[K // 2])
        fold = moments(scores(np.abs(x - med)), max_lag, lags=False)
        out.update(rhat_bulk=bulk["rhat"], ess_bulk=bulk["ess"], lags_bulk=bulk["lags"], truncated=bulk["truncated"],
                   rhat_fold=fold["rhat"], rhat_rank=fmax(bulk["rhat"], fold["rhat"]), bulk=bulk, fold=fold)
    q = [indicator_ess(x <= xs[quantile_order(p, K)], max_lag) for p in probs]
    tl = [indicator_ess(x <= xs[quantile_order(p, K)], max_lag) for p in (0.05, 0.95)]
    ind = [(x > float(t)) if s > 0 else (x < float(t)) for t, s in zip(thresholds, sides)]
    e = [indicator_ess(I, max_lag) for I in ind]
    cnt = [int(np.count_nonzero(I)) for I in ind]
    prob = [c / K for c in cnt]
    # (prob is the double c / K by definition: 1 - prob is taken of that double, exactly, not of the rational)
    mcse = [0.0 if c in (0, K) else float(np.sqrt(LD(p) * (1 - LD(p)) / LD(v[0]))) for c, p, v in zip(cnt, prob, e)]
    out.update(ess_q=[v[0] for v in q], lags_q=[v[1] for v in q], mag_q=[v[2] for v in q], ess_tail=fmin(tl[0][0], tl[1][0]),
               lags_tail=[v[1] for v in tl], mag_tail=[v[2] for v in tl], ess_exc=[v[0] for v in e], lags_exc=[v[1] for v in e],
               mag_exc=[v[2] for v in e], prob=prob, mcse_prob=mcse, count=cnt)
    return out


U = 2.0 ** -53
# The relative error of the library's Phi^-1 on the rank scores' arguments, measured against norm_ppf by
# tests/test_rank_diagnostics_cpu.py over K = 4, 5, 64, 1000, 16384 (the test asserts that the figure still holds); the device
# bound takes twice it, since the device compiler may contract multiply-adds that the host's does not.
PHI_ERR_MEASURED = 7.5e-16   # 7.47e-16 at K = 16384; 4.5e-16 to 5.8e-16 at the shorter ones


def score_bounds(rec, K, pairs_other, depth, eps_phi):
    """Relative bounds on ess and rhat of the diagnostics of a score series, from its ``moments`` record: the sibling's bound
    (tests/test_gpu_diagnostics.py, series_bounds: the first-order rounding of the addition chains, doubled; ``depth`` additions
    behind any one sum) with one more source of error: every z_s is off by at most eta = eps_phi max|z|, so every centred value by
    at most 2 eta more (its own error and the mean's).  With u = 2^-53, A = max|z|, Dm = max|d|, s0 = sqrt(gamma_0):
      delta = u A + (D + 2) u Dm + 2 eta;   e_a = (D + 2) u + 2 delta / s0;   e_G = 4 e_a + 4 u
      e_tau = 4 P e_G + 2 P u tsum + 4 u (2 tsum + 1) + 4 u tau,  P = the larger pair count;   ess: e_tau / tau + u
      rhat: e_m = 2 (D + 3) u Dm + 2 eta;  e_e = 2 (D + 4) u Dm + 2 eta;  e_W = (D + 4) u + 3 e_e / sqrt(W);
            Q = dmu^2 / 2;  dQ = dmu e_m + e_m^2 / 2 + 4 u Q;  ((dQ + Q e_W) / W) / (2 rhat^2) + 4 u
    Second-order terms are asserted below 1e-6."""
    D = depth
    A, Dm, s0 = rec["max_abs_x"], rec["max_abs_d"], math.sqrt(rec["gamma0"])
    eta = eps_phi * A
    delta = U * A + (D + 2) * U * Dm + 2 * eta
    e_a = (D + 2) * U + 2 * delta / s0
    assert e_a < 1e-6
    e_G = 4 * e_a + 4 * U
    b = dict(e_G=e_G)
    if not math.isnan(rec["tau"]):
        P = max(rec["pairs"], pairs_other)
        e_tau = 4 * P * e_G + 2 * P * U * rec["tsum"] + 4 * U * (2 * rec["tsum"] + 1) + 4 * U * rec["tau"]
        b["ess"] = 2 * (e_tau / rec["tau"] + U)
    if rec["W"] > 0:
        e_m, e_e = 2 * (D + 3) * U * Dm + 2 * eta, 2 * (D + 4) * U * Dm + 2 * eta
        e_W = (D + 4) * U + 3 * e_e / math.sqrt(rec["W"])
        assert e_W < 1e-6
        Q = rec["dmu"] ** 2 / 2
        dQ = rec["dmu"] * e_m + e_m * e_m / 2 + 4 * U * Q
        b["rhat"] = 2 * (((dQ + Q * e_W) / rec["W"]) / (2 * rec["rhat"] ** 2) + 4 * U)
    return b


def split_scale_cauchy(K, seed, scale=3.0):
    """Cauchy draws whose second half is scaled: the halves agree in location, not in scale."""
    x = np.random.default_rng(seed).standard_cauchy(K)
    x[K // 2:] *= scale
    return x


def tie_blocks(K):
    """1, 1, 2, 2, 2, 3, 3, 4, 4, 4, ...: blocks of two and three equal values, ascending."""
    out, v = [], 1
    while len(out) < K:
        out += [float(v)] * (2 if v % 2 else 3)
        v += 1
    return np.array(out[:K])
