"""Restatement of the criteria over the fit's own rows (spamtree_amd/csrc/rows_score.hpp) in extended
precision, with the rounding bounds of section 20.  Not a test module: tests/test_rows_score_cpu.py checks it against closed forms,
tests/test_gpu_rows_score.py checks the device against it.

Inputs are what the device itself was given or returned as exact inputs: the target t, XB (st_get_xb), w (st_set_w), tausq_inv
(st_set_tausq_inv).  Every bound is first order in u = 2^-53 and was derived from the kernels' operation chains (k_rows_score.hip
states them) before any device value was seen; none is fitted.  The per-draw bounds, the log-sum-exp bound and the CRPS come from
tests/score_reference.py unchanged: a row's draw is a scored point with one regressor x = XB, beta = 1, cond_mean = w, cond_var = 0
(the device forms mu = XB + w in one rounding, the bound allows the three of the general chain)."""
import math

from tests.score_reference import (E_ERFC, E_LOG, HL2PI, U, crps_bound, crps_sorted, gamma, lme_bound,  # noqa: F401
                                   log_mean_exp_direct, log_mean_exp_stream, mp, point_draw)

NT, STATS_WG = 256, 1024      # spamtree_amd/csrc/st_device.hpp, misc_kernels.hpp


def row_draw(t, xb, w, tausq_inv):
    """One draw of one row: (l, r, mu, bound on l, bound on Phi(r)) at 50 digits; cond_var = 0."""
    l, r, dl, dphi = point_draw(t, [xb], [1.0], w, 0.0, tausq_inv)
    return l, r, mp.mpf(float(xb)) + mp.mpf(float(w)), dl, dphi


def welford_mean_bound(S, sumsq):
    """|computed - exact| of the recursion m_k = m_(k-1) + (x_k - m_(k-1)) / k over S values with sum of squares `sumsq`.
    Step k commits 2 u |x_k - m_(k-1)| / k (the subtraction and the division) + u |m_k| (the addition); the errors obey
    k e_k = (k - 1) e_(k-1) + k rho_k, so S |e_S| <= sum_k (2 u |x_k - m_(k-1)| + k u |m_k|).  With |m_k| <= sqrt(sumsq / k) and
    |x_k - m_(k-1)| <= 2 sqrt(sumsq):  |e_S| <= u sqrt(sumsq) (4 + sqrt S).  (Step 1 is exact: 0 + x / 1.)"""
    return U * math.sqrt(float(sumsq)) * (4.0 + math.sqrt(S))


def welford_m2_bound(S, sumsq, m2, dx):
    """|computed - exact| of M2_k = fma(x_k - m_(k-1), x_k - m_k, M2_(k-1)) where every x carries an input error of at most dx.
    Each fused multiply-add rounds once (S u M2 in all: M2 never decreases), each factor is a rounded difference (2 u M2) of a
    value and a mean in error by at most E = welford_mean_bound: sum_k (|e_(k-1)| + |e_k|) |d_k| <= 2 E sqrt(2 S M2), as
    d_k^2 <= 2 d_k d'_k for k >= 2 and step 1 adds nothing.  The inputs' own errors move the exact M2 by at most
    2 sqrt(S M2) dx + S dx^2."""
    E = welford_mean_bound(S, sumsq)
    m2 = float(m2)
    return (S + 2) * U * m2 + 2 * E * math.sqrt(2 * S * m2) + 2 * math.sqrt(S * m2) * dx + S * dx * dx


def row_values(t, xbs, ws, tausq_invs, held):
    """The per-row outputs over S draws at 50 digits with their bounds:
    dict(name -> (value, bound)) for lppd, mean_ll, p_waic, mu_mean and, on a held-out row, pit."""
    S = len(xbs)
    d = [row_draw(t, xbs[s], ws[s], tausq_invs[s]) for s in range(S)]
    ls = [x[0] for x in d]
    dl = max(x[3] for x in d)
    lppd = log_mean_exp_stream(ls)
    mean_ll = mp.fsum(ls) / S
    m2 = mp.fsum((l - mean_ll) ** 2 for l in ls)
    sq_l = float(mp.fsum(l * l for l in ls))
    mus = [x[2] for x in d]
    sq_mu = float(mp.fsum(m * m for m in mus))
    out = dict(lppd=(lppd, dl + lme_bound(S, lppd)),
               mean_ll=(mean_ll, dl + welford_mean_bound(S, sq_l)),
               # mu_s = fl(XB + w): u |mu_s| each, at most u sqrt(sum mu^2) in the mean
               mu_mean=(mp.fsum(mus) / S, U * math.sqrt(sq_mu) + welford_mean_bound(S, sq_mu)))
    if S > 1:
        pw = m2 / (S - 1)
        out["p_waic"] = (pw, welford_m2_bound(S, sq_l, m2, dl) / (S - 1) + U * float(pw))
    else:
        out["p_waic"] = (mp.mpf(0), 0.0)
    if held:
        pit = mp.fsum(mp.erfc(-x[1] / mp.sqrt(2)) / 2 for x in d) / S
        out["pit"] = (pit, max(x[4] for x in d) + U * (2 * E_ERFC + S + 1))
    return out


def tau2bar(tausq_invs):
    """mean_s 1 / tausq_inv_s at 50 digits and the relative error of the host's sum (S reciprocals, S - 1 additions, one division)."""
    S = len(tausq_invs)
    return mp.fsum(1 / mp.mpf(float(x)) for x in tausq_invs) / S, gamma(S + 1)


def log_normal_at_mean(t, mu_mean, t2bar, t2rel):
    """log N(t; mu_mean, tau2bar) with mu_mean the device's own double (exact input) and its bound: sigma = sqrt(tau2bar) has the
    relative error t2rel / 2 + u, e = t - mu_mean one rounding, r = e / sigma one more."""
    sig = mp.sqrt(t2bar)
    r = (mp.mpf(float(t)) - mp.mpf(float(mu_mean))) / sig
    l = -r * r / 2 - mp.log(sig) - HL2PI
    ds = t2rel / 2 + U
    dr = abs(float(r)) * (2 * U + ds)
    ls = abs(float(mp.log(sig)))
    return l, abs(float(r)) * dr + dr * dr / 2 + ds + 2 * E_LOG * U * ls + U * (float(r * r) / 2 + ls) + U * abs(float(l)) + 2 * U


def totals_chain(n):
    """c of the totals' bound gamma_c sum |term|: the additions on the longest path of one sum -- a thread's serial walk over every
    NT-th row of its chunk of ceil(n / STATS_WG) rows, six wave levels and four wave sums in block_sum, then k_stats_final's four
    partial sums per thread and its eight tree levels."""
    chunk = -(-n // STATS_WG)
    return -(-chunk // NT) + 6 + 4 + STATS_WG // NT + 8


def totals_bound(n, terms):
    return gamma(totals_chain(n)) * math.fsum(abs(float(x)) for x in terms)
