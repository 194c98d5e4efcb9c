"""Restatement of the Rao-Blackwellised exceedance probabilities (spamtree_amd/csrc/points_exceed.hpp) in
extended precision, with the rounding bounds of section 30.  Not a test module: tests/test_exceed_cpu.py holds spamtree_amd.exceed
against it, tests/test_gpu_exceed.py the device.

Every function takes the per-draw quantities the device itself returned (cond_mean, cond_var, the functionals' F_m and F_v) and the
beta and tausq_inv it was given, evaluates the definition at 50 digits and returns each value with the bound that section 30
derives from the kernels' operation chain.  u = 2^-53.

THE BOUNDS.  One draw, v > 0.  Target w: d = m - c (one rounding, relative u), sd = sqrt(v) (u), d / sd (u), the product with the
rounded constant 1 / sqrt 2 (2 u): the argument of erfc carries a relative error of 5 u, dz = 5 u |z|.  Target yhat: mu behind
p + 1 roundings and the subtraction (gamma(p + 2) (|c| + sum |x b| + |m|) absolute), sigma behind three (1 / tausq_inv, the add, the
root: 2 u relative), the division and the product (3 u): dz = 5 u |z| + gamma(p + 2) (|c| + sum |x b| + |m|) / sigma.  Through Phi
that is at most phi(max(|z| - dz, 0)) dz; erfc itself is taken at E_ERFC = 5 ulp (10 u relative, on p_s <= 1); the halving is exact:
    eps_s = phi(max(|z| - dz, 0)) dz + 2 E_ERFC u p_s + (E_ERFC + 1) 2^-1074
(the last term: where erfc underflows gradually, beyond |z| = 37.5, its ulp is the subnormal spacing and the halving rounds).
v == 0: p_s is an exact comparison of the same doubles, eps_s = 0.
The mean.  Update k forms m_k = fl(m + fl(fl(p - m) / k)): roundings of at most u |p - m|, u |p - m| / k and u |m_k|, all values in
[0, 1]: rho_k <= u (1 + 2 / k) <= 2 u, and rho_1 = 0 (every operation of the first update is exact).  An error e of the previous mean
enters as (1 - 1 / k) e and one of p_k as eps / k, so by induction
    |prob - exact| <= E + 2 u (S - 1),   E = max_s eps_s.                                                         (prob_bound)
M2.  Update k adds fl(fl(p - m_{k-1}) fl(p - m_k)) with both factors in [-1, 1]; each factor is off by at most E + prob_bound + u,
the product rounds once (u), the addition to M2 <= k / 4 once more (u k / 4, in sum u S^2 / 8), and M2 / S rounds once (u / 4):
    |prob_var - exact| <= 2 (E + prob_bound + u) + u + u S / 8 + u = 2 E + 2 prob_bound + u (S / 8 + 4)            (var_bound)
an absolute bound on the variance itself, not on a standard deviation."""
import math

import mpmath as mp
import numpy as np

mp.mp.dps = 50
U = 2.0 ** -53
E_ERFC = 5      # ulp error of the device's erfc that sections 19 and 30 assume (1 ulp <= 2 u relative)
RSQRT2 = 1 / mp.sqrt(2)
ETA = 2.0 ** -1074   # the spacing of the subnormal numbers: an ulp of erfc where it underflows gradually (|z| beyond 37.5)


def gamma(k):
    return k * U / (1.0 - k * U)


def _phi_eps(z, dz, p):
    a = max(abs(float(z)) - dz, 0.0)
    phi = math.exp(-min(a * a / 2, 745.0)) / math.sqrt(2 * math.pi)
    return phi * dz + 2 * E_ERFC * U * float(p) + (E_ERFC + 1) * ETA


def moments_w(m, v):
    """What a draw of target w (or of a functional: m = F_m, v = F_v) is judged on, whatever the threshold: (mean, sd or None for a
    point mass, magnitude behind the mean's rounding, its gamma)."""
    m, v = mp.mpf(float(m)), mp.mpf(float(v))
    return m, (mp.sqrt(v) if v > 0 else None), 0.0, 0.0


def moments_yhat(x, beta, m, v, tausq_inv):
    """The same of target yhat: mu = x'beta + m, sigma = sqrt(v + 1 / tausq_inv)."""
    xb_abs = sum(abs(float(a) * float(b)) for a, b in zip(x, beta))
    mu = mp.fsum(mp.mpf(float(a)) * mp.mpf(float(b)) for a, b in zip(x, beta)) + mp.mpf(float(m))
    return mu, mp.sqrt(mp.mpf(float(v)) + 1 / mp.mpf(float(tausq_inv))), xb_abs + abs(float(m)), gamma(len(x) + 2)


def draw(mom, c, side):
    """One draw at one threshold from its moments: (p_s, eps_s) at 50 digits."""
    mean, sd, mag, g = mom
    c = mp.mpf(float(c))
    d = side * (mean - c)
    if sd is None:
        return (mp.mpf(1) if d > 0 else mp.mpf(0)), 0.0
    z = d / sd
    p = mp.erfc(-z * RSQRT2) / 2
    return p, _phi_eps(z, 5 * U * abs(float(z)) + g * (abs(float(c)) + mag) / float(sd), p)


def draw_w(m, v, c, side):
    return draw(moments_w(m, v), c, side)


def draw_yhat(x, beta, m, v, tausq_inv, c, side):
    return draw(moments_yhat(x, beta, m, v, tausq_inv), c, side)


def finish(draws):
    """The exact mean and population variance of p_s over the draws [(p_s, eps_s)] with their bounds:
    (prob, prob_bound, prob_var, var_bound)."""
    S = len(draws)
    ps = [d[0] for d in draws]
    E = max(d[1] for d in draws)
    prob = mp.fsum(ps) / S
    var = mp.fsum((p - prob) ** 2 for p in ps) / S
    pb = E + 2 * U * (S - 1)
    vb = 2 * E + 2 * pb + U * (S / 8 + 4)
    return prob, pb, var, vb


def point_w(cond_means, cond_vars, c, side):
    return finish([draw_w(m, v, c, side) for m, v in zip(cond_means, cond_vars)])


def point_yhat(x, betas, cond_means, cond_vars, tausq_invs, c, side):
    return finish([draw_yhat(x, b, m, v, t, c, side) for b, m, v, t in zip(betas, cond_means, cond_vars, tausq_invs)])


def bernoulli_variance(cond_means, cond_vars, c, side):
    """(sum_s p_s, V = sum_s p_s (1 - p_s)) of target w as floats: the mean and variance of the stored-draw count."""
    ps = [draw_w(m, v, c, side)[0] for m, v in zip(cond_means, cond_vars)]
    return float(mp.fsum(ps)), float(mp.fsum(p * (1 - p) for p in ps))


def err(got, want):
    """|got - want| of a double against a 50-digit value, as a float."""
    return abs(float(mp.mpf(float(got)) - want))


def check_target(got, refs, tag):
    """``got``: dict(prob, prob_var) of T x n arrays; ``refs[t][i]``: finish()'s tuple.  Asserts every value within its bound and in
    [0, 1]; returns the worst error / bound of prob and prob_var."""
    worst = [0.0, 0.0]
    P, V = np.asarray(got["prob"]), np.asarray(got["prob_var"])
    for t, row in enumerate(refs):
        for i, (prob, pb, var, vb) in enumerate(row):
            ep, ev = err(P[t, i], prob), err(V[t, i], var)
            worst = [max(worst[0], ep / pb if pb else float(ep > 0)), max(worst[1], ev / vb)]
            assert 0.0 <= P[t, i] <= 1.0 and 0.0 <= V[t, i] <= 1.0, (tag, t, i, P[t, i], V[t, i])
            assert ep <= pb, (tag, "prob", t, i, ep, pb)
            assert ev <= vb, (tag, "prob_var", t, i, ev, vb)
    return worst
