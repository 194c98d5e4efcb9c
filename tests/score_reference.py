"""Restatement of the scores of held-out observations (spamtree_amd/csrc/points_score.hpp) in extended
precision, with the rounding bounds of section 19.  Not a test module: tests/test_score_cpu.py checks it against direct
evaluations, tests/test_gpu_score.py checks the device against it.

Every function takes the per-draw quantities the device itself returned (cond_mean, cond_var, the packed cond_cov) and the beta and
tausq_inv it was given, evaluates the definition at 50 digits (CRPS: in exact rationals) and returns the value with the bound that
section 19 derives for the kernels' operation chain.  u = 2^-53."""
import math
from fractions import Fraction

import mpmath as mp
import numpy as np

mp.mp.dps = 50
U = 2.0 ** -53
E_LOG, E_EXP, E_ERFC = 1, 1, 5      # ulp errors of the device's log, exp and erfc that section 19 assumes (1 ulp <= 2 u relative)
HL2PI = mp.log(2 * mp.pi) / 2


def gamma(k):
    return k * U / (1.0 - k * U)


def log_mean_exp_direct(ells):
    """log((1 / S) sum exp l) evaluated directly (mpmath keeps the exponent range: nothing underflows)."""
    return mp.log(mp.fsum(mp.exp(l) for l in ells) / len(ells))


def log_mean_exp_stream(ells):
    """The kernel's recursion on (M, A) -- first draw, l <= M, l > M -- and lpd = M + log(A / S); -inf draws (density 0) skipped."""
    M, A = mp.mpf(0), mp.mpf(0)
    for l in ells:
        if l == -mp.inf:
            continue
        if A == 0:
            M, A = l, mp.mpf(1)
        elif l <= M:
            A += mp.exp(l - M)
        else:
            A = A * mp.exp(M - l) + 1
            M = l
    return (M + mp.log(A / len(ells))) if A > 0 else -mp.inf


def lme_bound(S, lpd):
    """Rounding of the recursion and of lpd = M + log(A / S) (section 19): S updates of relative error (3 + max(1, ln S)) u each
    (one exp of E_EXP ulp on a rounded argument, one rounding of the add or fused multiply-add), the division, the host's log
    and the final add."""
    return U * (S * (1 + 2 * E_EXP + max(1.0, math.log(S))) + 1 + 2 * math.log(S) + abs(float(lpd)))


def point_draw(y, x, beta, cond_mean, cond_var, tausq_inv):
    """One draw of one point: (l, r, bound on l, bound on Phi(r)) at 50 digits."""
    p = len(x)
    xb_abs = sum(abs(float(a) * float(b)) for a, b in zip(x, beta))
    mu = mp.fsum(mp.mpf(float(a)) * mp.mpf(float(b)) for a, b in zip(x, beta)) + mp.mpf(float(cond_mean))
    s2 = mp.mpf(float(cond_var)) + 1 / mp.mpf(float(tausq_inv))
    sig = mp.sqrt(s2)
    r = (mp.mpf(float(y)) - mu) / sig
    l = -r * r / 2 - mp.log(sig) - HL2PI
    # e = y - mu behind p + 2 roundings; sigma behind three (1 / tausq_inv, the add, the square root: relative 2 u); the division
    dr = 3 * U * abs(float(r)) + gamma(p + 2) * (abs(float(y)) + xb_abs + abs(float(cond_mean))) / float(sig)
    ls = abs(float(mp.log(sig)))
    dl = abs(float(r)) * dr + dr * dr / 2 + 2 * U + 2 * E_LOG * U * ls + U * (float(r * r) / 2 + ls) + U * abs(float(l))
    phi = math.exp(-min(float(r * r) / 2, 700.0)) / math.sqrt(2 * math.pi)
    dphi = phi * (dr + 2 * U * abs(float(r)))
    return l, r, dl, dphi


def point_scores(y, x, betas, cond_means, cond_vars, tausq_invs):
    """lpd and pit of one point over S draws with their bounds: (lpd, lpd_bound, pit, pit_bound)."""
    S = len(betas)
    d = [point_draw(y, x, betas[s], cond_means[s], cond_vars[s], tausq_invs[s]) for s in range(S)]
    lpd = log_mean_exp_stream([t[0] for t in d])
    pit = mp.fsum(mp.erfc(-t[1] / mp.sqrt(2)) / 2 for t in d) / S
    lb = max(t[2] for t in d) + lme_bound(S, lpd)
    pb = max(t[3] for t in d) + U * (2 * E_ERFC + S + 1)
    return lpd, lb, pit, pb


def joint_draw(y_o, X_o, betas_o, mean_o, Sigma_oo, tsq_inv_o, extra=0):
    """One draw of one group's observed members: l^G at 50 digits and its bound.  betas_o: the coefficient vector of each member's
    margin; Sigma_oo: the g_o x g_o block as the device returned it (lower triangle read); tsq_inv_o: tausq_inv of each member's margin.
    extra: a further perturbation of A of that many u tr A that the bound is to cover (a tausq_inv known to 2 u only: 2).
    Returns (-inf, 0) when the extended-precision factorisation meets a pivot that is not > 0."""
    g = len(y_o)
    p = len(X_o[0])
    A = mp.matrix(g, g)
    for a in range(g):
        for b in range(a + 1):
            A[a, b] = A[b, a] = mp.mpf(float(Sigma_oo[a][b]))
        A[a, a] += 1 / mp.mpf(float(tsq_inv_o[a]))
    e = mp.matrix(g, 1)
    de2 = 0.0
    for a in range(g):
        mu = mp.fsum(mp.mpf(float(u)) * mp.mpf(float(v)) for u, v in zip(X_o[a], betas_o[a])) + mp.mpf(float(mean_o[a]))
        e[a] = mp.mpf(float(y_o[a])) - mu
        mag = abs(float(y_o[a])) + sum(abs(float(u) * float(v)) for u, v in zip(X_o[a], betas_o[a])) + abs(float(mean_o[a]))
        de2 += (gamma(p + 2) * mag) ** 2
    L = mp.matrix(g, g)
    for j in range(g):
        s = A[j, j] - mp.fsum(L[j, k] ** 2 for k in range(j))
        if not s > 0:
            return -mp.inf, 0.0
        L[j, j] = mp.sqrt(s)
        for i in range(j + 1, g):
            L[i, j] = (A[i, j] - mp.fsum(L[i, k] * L[j, k] for k in range(j))) / L[j, j]
    z = mp.lu_solve(L, e) if g > 1 else mp.matrix([[e[0] / L[0, 0]]])
    q = mp.fsum(z[a] ** 2 for a in range(g))
    ld = mp.fsum(mp.log(L[a, a]) for a in range(g))
    l = -q / 2 - ld - g * HL2PI
    Af = np.array([[float(A[a, b]) for b in range(g)] for a in range(g)])
    lam = float(np.linalg.eigvalsh(Af)[0])
    tr = float(np.trace(Af))
    en = float(mp.sqrt(mp.fsum(e[a] ** 2 for a in range(g))))
    sl = float(mp.fsum(abs(mp.log(L[a, a])) for a in range(g)))
    if lam <= 0:
        return l, float("inf")
    # section 19: ||dA|| <= (g + 3) u tr A for the factorisation (g + 1) with 1 / tausq_inv and its add, (2 g + 4) u tr A with the solve
    dld = 0.5 * math.sqrt(g) / lam * (g + 3 + extra) * U * tr + g * U + (g + 2 * E_LOG) * U * sl
    dq = 0.5 * ((en / lam) ** 2 * (2 * g + 4 + extra) * U * tr + 2 * en / lam * math.sqrt(de2) + g * U * float(q))
    return l, dld + dq + 2 * U * abs(float(l))


def joint_scores(draws):
    """lpd_joint of one group over S draws: draws = [(l, bound)] from joint_draw.  (lpd_joint, bound, n_degenerate)."""
    S = len(draws)
    lpd = log_mean_exp_stream([d[0] for d in draws])
    ndeg = sum(1 for d in draws if d[0] == -mp.inf)
    if lpd == -mp.inf:
        return lpd, 0.0, ndeg
    return lpd, max(d[1] for d in draws) + lme_bound(S, lpd), ndeg


def crps_sorted(x, y):
    """(1 / K) sum |d_(k)| - (1 / K^2) sum (2 k - K - 1) d_(k), d = x - y sorted ascending; exact (doubles are dyadic rationals: the
    sums run over integers on their common denominator).  Returns (crps, mean |d|) as Fractions."""
    fr = [Fraction(float(v)) for v in x] + [Fraction(float(y))]
    den = max(f.denominator for f in fr)
    ints = [f.numerator * (den // f.denominator) for f in fr]
    d = sorted(v - ints[-1] for v in ints[:-1])
    K = len(d)
    s1 = sum(abs(v) for v in d)
    s2 = sum((2 * (k + 1) - K - 1) * v for k, v in enumerate(d))
    return Fraction(s1, K * den) - Fraction(s2, K * K * den), Fraction(s1, K * den)


def crps_brute(x, y):
    """(1 / K) sum |x - y| - (1 / 2 K^2) sum sum |x_s - x_t|; exact."""
    xs = [Fraction(float(v)) for v in x]
    K = len(xs)
    yy = Fraction(float(y))
    return sum((abs(v - yy) for v in xs), Fraction(0)) / K - sum((abs(a - b) for a in xs for b in xs), Fraction(0)) / (2 * K * K)


def crps_bound(K, mean_abs_d):
    """(2 c + 5) u mean|d|, c = ceil(K / 64) + 6: the rounding of d = x - y (its effect on both sums), c additions of |d| and c fused
    multiply-adds of (2 k - K - 1) d on the longest path (a lane's terms, then six butterfly levels), two divisions, the
    subtraction."""
    c = -(-K // 64) + 6
    return (2 * c + 5) * U * float(mean_abs_d)
