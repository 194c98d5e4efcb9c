"""Leave-one-out criteria with the latent field integrated out: the definition in float64 NumPy (no device, no library).

The criteria of ``rows_score`` are conditional on w.  Here saved draw s gives an observed row i of margin j the density of y_i with
its own w_i integrated out against the prior full conditional of the tree's DAG, w_i | w_-i, theta ~ N(m_i, v_i):

    v_i = 1 / Q_ii,   m_i = w_i - (Q w)_i / Q_ii,   Q = the DAG's prior precision over the blocks with observed rows,
    mu_s = XB_i + m_i,   sigma2_s = v_i + tausq_j,   l_s = log N(y_i; mu_s, sigma2_s),   Phi_s = Phi((y_i - mu_s) / sigma_s).

Over the S saved draws, with the weights r_s = exp(-l_s):

    elpd_loo_i = -log((1 / S) sum r_s),   pit_loo_i = sum r_s Phi_s / sum r_s,   mu_loo_i = sum r_s mu_s / sum r_s,
    weight_ess_i = (sum r_s)^2 / sum r_s^2.

E_post[1 / p(y_i | w_-i, theta, beta, tausq)] = 1 / p(y_i | y_-i), so elpd_loo_i estimates the leave-one-out log predictive density
log p(y_i | y_-i).  These are the raw weights, with ``weight_ess`` as their diagnostic (on the checks of tests/test_rows_loo_cpu.py it
stayed above 0.17 S); ``spamtree_amd.psis`` smooths their tail and gives k-hat from the per-draw terms the device keeps when asked
(``draw_terms`` below: t_s = -l_s, Phi_s, mu_s).  NA rows get no leave-one-out value: they are leaves, predict them as new points.

The streaming state is what the device keeps (spamtree_amd/csrc/loo_kernels.hpp gives the order of every operation there): the
running maximum M of t_s = -l_s, A1 = sum e^(t - M), A2 = sum e^(2 (t - M)), AP = sum e^(t - M) Phi, AM = sum e^(t - M) mu, rescaled
when M grows, and NS, the number of draws skipped because l_s was not finite.
"""
import math

import numpy as np

HL2PI = -0.91893853320467274178
STATE = ("M", "A1", "A2", "AP", "AM", "NS")


def conditional_moments(Q, w):
    """(q_diag, qw, cond_mean, cond_var) of every row from a precision matrix Q and a field w: Q_ii, (Q w)_i, w_i - (Q w)_i / Q_ii
    and 1 / Q_ii."""
    Q, w = np.asarray(Q, dtype=np.float64), np.asarray(w, dtype=np.float64)
    d = np.diag(Q).copy()
    c = Q @ w
    return d, c, w - c / d, 1.0 / d


def draw_terms(y, xb, cond_mean, cond_var, tausq):
    """(l, Phi, mu) of one draw: the log density of y under N(xb + cond_mean, cond_var + tausq) per row (``tausq`` per row), its
    distribution function at y and its mean."""
    y = np.asarray(y, dtype=np.float64)
    mu = np.asarray(xb, dtype=np.float64) + np.asarray(cond_mean, dtype=np.float64)
    with np.errstate(all="ignore"):
        sig = np.sqrt(np.asarray(cond_var, dtype=np.float64) + np.asarray(tausq, dtype=np.float64))
        z = (y - mu) / sig
        l = -0.5 * z * z - np.log(sig) + HL2PI
    phi = 0.5 * np.array([math.erfc(-v * 0.70710678118654752440) if np.isfinite(v) else np.nan for v in np.ravel(z)]).reshape(np.shape(z))
    return l, phi, mu


def new_state(n):
    return {k: np.zeros(n) for k in STATE}


def update(state, l, phi, mu):
    """One draw into the streaming state (in place; returns it).  Rows whose l is not finite are skipped and counted in NS."""
    l, phi, mu = (np.asarray(a, dtype=np.float64) for a in (l, phi, mu))
    ok = np.isfinite(l)
    state["NS"][~ok] += 1.0
    t = np.where(ok, -l, 0.0)
    M, A1, A2, AP, AM = (state[k] for k in ("M", "A1", "A2", "AP", "AM"))
    first = ok & (A1 == 0.0)
    low = ok & ~first & (t <= M)
    high = ok & ~first & (t > M)
    with np.errstate(all="ignore"):
        x = np.exp(np.where(low, t - M, 0.0))
        A1[low] += x[low]; A2[low] += (x * x)[low]; AP[low] += (x * phi)[low]; AM[low] += (x * mu)[low]
        x = np.exp(np.where(high, M - t, 0.0))
        A1[high] = (A1 * x + 1.0)[high]; A2[high] = (A2 * x * x + 1.0)[high]
        AP[high] = (AP * x + phi)[high]; AM[high] = (AM * x + mu)[high]
        M[high] = t[high]
    M[first] = t[first]; A1[first] = 1.0; A2[first] = 1.0; AP[first] = phi[first]; AM[first] = mu[first]
    return state


def finish(state, S):
    """dict(elpd_loo, pit_loo, mu_loo, weight_ess) after S draws; NaN where every draw was skipped."""
    with np.errstate(all="ignore"):
        Si = S - state["NS"]
        A1 = np.where(Si > 0, state["A1"], np.nan)
        return dict(elpd_loo=-(state["M"] + np.log(A1 / Si)), pit_loo=state["AP"] / A1, mu_loo=state["AM"] / A1,
                    weight_ess=A1 * A1 / state["A2"])


def totals(rows, y, mv, q):
    """Per outcome (``mv`` 0-based) over the rows with a finite elpd_loo: dict(n, elpd_loo, looic, sqerr, pit, min_weight_ess), q
    values each (sums, not means)."""
    y, mv = np.asarray(y, dtype=np.float64), np.asarray(mv)
    out = dict(n=np.zeros(q, dtype=np.int64), elpd_loo=np.zeros(q), looic=np.zeros(q), sqerr=np.zeros(q), pit=np.zeros(q),
               min_weight_ess=np.full(q, np.nan))
    for j in range(q):
        k = (mv == j) & np.isfinite(rows["elpd_loo"])
        out["n"][j] = int(k.sum())
        if not k.any():
            continue
        out["elpd_loo"][j] = rows["elpd_loo"][k].sum()
        out["looic"][j] = -2.0 * out["elpd_loo"][j]
        out["sqerr"][j] = ((y[k] - rows["mu_loo"][k]) ** 2).sum()
        out["pit"][j] = rows["pit_loo"][k].sum()
        out["min_weight_ess"][j] = rows["weight_ess"][k].min()
    return out


def accumulate(draws, y, xb, tausq):
    """The whole estimator from an iterable of (cond_mean, cond_var) per draw with fixed xb and per-row tausq: (rows, S)."""
    state, S = None, 0
    for cm, cv in draws:
        if state is None:
            state = new_state(np.size(cm))
        update(state, *draw_terms(y, xb, cm, cv, tausq))
        S += 1
    return finish(state, S), S
