"""Restatement of the mixture predictive's CDF, quantile and CRPS (spamtree_amd/csrc/points_mixture.hpp) in
extended precision, with the termination width delta and the rounding bounds eps_F and crps_bound as the kernel header states them.
Not a test module: tests/test_mixture_cpu.py holds spamtree_amd.mixture against it, tests/test_gpu_mixture.py the device.

A mixture is a list of components (mean, variance) as 50-digit numbers, built by ``components`` from the doubles the device
itself stored: m and v for target w (and a functional's F_m, F_v), mu and v + tau2 -- the sum exact, not rounded -- for target yhat.
u = 2^-53.

QUANTILES are judged on the definition, not against a root: the device's x must satisfy
    F(x + delta) >= p - eps_F   and   F((x - delta)-) <= p + eps_F,        delta = 2^-50 max(|lo0|, |hi0|),
lo0 / hi0 the least / greatest m_s + z_p sd_s.  The second is the left limit: x - delta is not above inf{x : F(x) >= p} exactly when F
stays below p to the left of it, and a point mass sitting at x - delta itself (an empty functional: every component a step at 0,
delta = 0, the quantile 0) does not count against it.  eps_F is the first-order bound of one evaluation of F in doubles:
    eps_F(x) = (1 / K) sum_s [phi(max(|z_s| - dz_s, 0)) dz_s + 10 u Phi_s] + (ceil(K / 64) + 8) u F + 6 x 2^-1074,   dz_s = 6 u |z_s|
(point masses contribute an exact 0 or 1 and no error), taken as the largest of its values at x - delta, x and x + delta: the
kernel evaluated F at the two ends of its last bracket, which lie in that interval.
CRPS.  One A is off by at most 24 u of itself; the sums add non-negative terms along chains of c1 = ceil(K / G) + 10 (T1 and the
diagonal) and c2 = ceil(K / G) (floor(K / 8) + 2) + 12 (the pairs) additions, G = 64 up to K = 64, 128 up to K = 128, else 256:
    |crps^ - crps| <= (27 + c1) u T1 / K + (27 + c2) u spread,     |spread^ - spread| <= (27 + c2) u spread."""
import math

import mpmath as mp

mp.mp.dps = 50
U = 2.0 ** -53
ETA = 2.0 ** -1074
E_ERFC = 5          # ulp error assumed of the device's erfc and erf (sections 19 and 30); 1 ulp <= 2 u relative
RSQRT2 = 1 / mp.sqrt(2)
SQRT_2_OVER_PI = mp.sqrt(2 / mp.pi)
DELTA_REL = 2.0 ** -50


def components(mean, var, tau2=None):
    """[(mean, variance)] at 50 digits from the stored doubles; ``tau2`` (a scalar or one per component) is added exactly."""
    K = len(mean)
    t = [0.0] * K if tau2 is None else ([float(tau2)] * K if not hasattr(tau2, "__len__") else tau2)
    return [(mp.mpf(float(a)), mp.mpf(float(b)) + mp.mpf(float(c))) for a, b, c in zip(mean, var, t)]


def norm_quantile(p):
    return mp.sqrt(2) * mp.erfinv(2 * mp.mpf(float(p)) - 1)


def cdf(x, comps, left=False):
    """F(x); ``left``: its left limit F(x-), which differs at a point mass only."""
    x = mp.mpf(x)
    tot = mp.mpf(0)
    for m, v in comps:
        tot += mp.erfc(-(x - m) / mp.sqrt(v) * RSQRT2) / 2 if v > 0 else (1 if (x > m if left else x >= m) else 0)
    return tot / len(comps)


def bracket(p, comps):
    z = norm_quantile(p)
    e = [m + z * mp.sqrt(v) for m, v in comps]
    return min(e), max(e)


def delta(p, comps):
    lo, hi = bracket(p, comps)
    return DELTA_REL * float(max(abs(lo), abs(hi)))


def eps_F(x, comps):
    """The rounding bound of one evaluation of F at the double x, in float64 (a bound needs no more)."""
    x = float(x)
    K = len(comps)
    tot, F = 0.0, 0.0
    for m, v in comps:
        m, v = float(m), float(v)
        if v > 0:
            z = (x - m) / math.sqrt(v)
            dz = 6 * U * abs(z)
            a = max(abs(z) - dz, 0.0)
            Phi = 0.5 * math.erfc(-z * 0.7071067811865476)
            tot += math.exp(-min(a * a / 2, 745.0)) / math.sqrt(2 * math.pi) * dz + 2 * E_ERFC * U * Phi
            F += Phi
        else:
            F += 1.0 if x >= m else 0.0
    return tot / K + (math.ceil(K / 64) + 8) * U * (F / K) + 6 * ETA


def check_quantile(x, p, comps):
    """The two conditions on the device's quantile x of probability p; returns the larger of the two violations over eps_F
    (<= 1 passes; negative: both hold without any allowance)."""
    x = float(x)
    d = delta(p, comps)
    eps = max(eps_F(x - d, comps), eps_F(x, comps), eps_F(x + d, comps))
    pm = mp.mpf(float(p))
    up = float(pm - cdf(mp.mpf(x) + d, comps))      # must be <= eps
    dn = float(cdf(mp.mpf(x) - d, comps, left=True) - pm)   # must be <= eps
    return max(up, dn) / eps


def quantile(p, comps, rel=mp.mpf(10) ** -40):
    """inf{x : F(x) >= p} at 50 digits by bisection from a widened bracket: (lo, hi) with F(lo) < p <= F(hi), hi - lo below
    ``rel`` of the bracket's scale."""
    p = mp.mpf(float(p))
    lo, hi = bracket(p, comps)
    scale = max(abs(lo), abs(hi), mp.mpf(10) ** -300)
    lo, hi = lo - scale * mp.mpf(10) ** -30, hi + scale * mp.mpf(10) ** -30
    assert cdf(lo, comps) < p <= cdf(hi, comps)
    while hi - lo > rel * scale:
        mid = (lo + hi) / 2
        if cdf(mid, comps) >= p:
            hi = mid
        else:
            lo = mid
    return lo, hi


def A(d, s2):
    if s2 > 0:
        s = mp.sqrt(s2)
        return d * mp.erf(d / s * RSQRT2) + s * SQRT_2_OVER_PI * mp.exp(-d * d / (2 * s2))
    return abs(d)


def spread(comps):
    K = len(comps)
    diag = mp.fsum(A(mp.mpf(0), 2 * v) for _, v in comps)
    pairs = mp.fsum(A(comps[s][0] - comps[t][0], comps[s][1] + comps[t][1]) for s in range(K) for t in range(s + 1, K))
    return (diag + 2 * pairs) / (2 * K * K)


def t1_mean(y, comps):
    y = mp.mpf(float(y))
    return mp.fsum(A(y - m, v) for m, v in comps) / len(comps)


def crps(y, comps, spr=None):
    return t1_mean(y, comps) - (spread(comps) if spr is None else spr)


def crps_group(K):
    """The threads k_mix_crps gives one point (mixture_plan.hpp)."""
    return 64 if K <= 64 else 128 if K <= 128 else 256


def crps_bounds(K, t1m, spr):
    """(bound of crps, bound of spread) for K components, T1 / K = ``t1m`` and ``spr`` the spread."""
    own = math.ceil(K / crps_group(K))
    c1, c2 = own + 10, own * (K // 8 + 2) + 12
    bs = (27 + c2) * U * float(spr)
    return (27 + c1) * U * float(t1m) + bs, bs


def crps_normal(y, m, sd):
    """The closed form of one normal: sd [z (2 Phi(z) - 1) + 2 phi(z) - 1 / sqrt(pi)], z = (y - m) / sd."""
    y, m, sd = mp.mpf(float(y)), mp.mpf(m), mp.mpf(sd)
    z = (y - m) / sd
    return sd * (z * (2 * mp.ncdf(z) - 1) + 2 * mp.npdf(z) - 1 / mp.sqrt(mp.pi))


def crps_by_quadrature(y, comps):
    """integral (F(x) - 1(x >= y))^2 dx, split at y, the means and the point masses: does not go through A."""
    y = mp.mpf(float(y))
    sd = max([mp.sqrt(v) for _, v in comps] + [mp.mpf(0)])
    ms = sorted({m for m, _ in comps} | {y})
    lo, hi = ms[0] - 40 * sd - 1, ms[-1] + 40 * sd + 1
    pts = [lo] + ms + [hi]
    f = lambda x: (cdf(x, comps) - (1 if x >= y else 0)) ** 2   # noqa: E731
    return mp.fsum(mp.quad(f, [a, b]) for a, b in zip(pts[:-1], pts[1:]) if b > a)


def err(got, want):
    return abs(float(mp.mpf(float(got)) - want))
