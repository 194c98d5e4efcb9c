"""Rao-Blackwellised exceedance probabilities at new points: the definition of st_points_exceed_* (include/spamtree_hip.h,
spamtree_amd/csrc/points_exceed.hpp) restated in float64, operation for operation, for small inputs.  NumPy, math and (for the
fused multiply-add where math has none) fractions only.

T thresholds, each with a side s_t = +1 / -1 and a value c per outcome (points) or per functional.  Saved draw s gives a target
with conditional mean m and variance v (w: cond_mean, clamped cond_var; yhat: x'beta + cond_mean, cond_var + 1 / tausq_inv;
a functional: F_m, F_v)
  v > 0:   z = s_t (m - c) / sqrt(v),  p_s = erfc(-z / sqrt 2) / 2 = Phi(z)
  v == 0:  p_s = 1 if s_t (m - c) > 0 else 0     (strict, like the event of the stored-draw excursions)
and over the S draws, in order, the Welford mean and M2 of p_s (d = p - mean; mean += d / count; M2 += d (p - mean)):
  prob = mean,  prob_var = M2 / S  (population variance of p_s over the draws; MCSE = sqrt(prob_var / ESS)).
Unlike ``excursions`` (counts over stored draws) nothing per draw is kept, the answer is not quantised in steps of 1 / K and
carries no Monte-Carlo noise of the indicator."""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

from . import excursions as _exc

MAX_THRESHOLDS = _exc.MAX_THRESHOLDS
_RSQRT2 = 0.70710678118654752440


def expand(thresholds, m, side=1):
    """``excursions.expand_thresholds`` with this module's name in its errors: (thr (T, m) float64, side (T,) int32)."""
    try:
        return _exc.expand_thresholds(thresholds, m, side)
    except ValueError as e:
        raise ValueError(str(e).replace("excursions:", "exceed:")) from None


def check_spec(spec, q, n_fun=None):
    """The option ``exceed=dict(thresholds=, side=, thresholds_fun=)`` of fit and predict against the problem: returns
    (thr (T, q), side (T,), thr_fun (T, n_fun) or None).  ValueError for unknown keys, no thresholds, what ``expand`` refuses, and
    ``thresholds_fun`` without functionals."""
    spec = dict(spec)
    unknown = set(spec) - {"thresholds", "side", "thresholds_fun"}
    if unknown:
        raise ValueError(f"exceed: unknown keys {sorted(unknown)} (thresholds, side, thresholds_fun)")
    if spec.get("thresholds") is None:
        raise ValueError("exceed: thresholds are needed")
    thr, side = expand(spec["thresholds"], q, spec.get("side", 1))
    thr_fun = None
    if spec.get("thresholds_fun") is not None:
        if not n_fun:
            raise ValueError("exceed: thresholds_fun needs functionals")
        thr_fun, _ = expand(spec["thresholds_fun"], n_fun, side)
        if thr_fun.shape[0] != thr.shape[0]:
            raise ValueError(f"exceed: thresholds_fun must hold one entry per threshold ({thr.shape[0]})")
    return thr, side, thr_fun


def draw_prob(mean, var, thr, side):
    """p_s of one draw: ``mean``, ``var``, ``thr`` broadcast against each other, ``side`` +1 or -1 (a scalar or broadcastable).
    The kernel's operations in its order: d = side (mean - thr), z = d / sqrt(var), erfc(-z / sqrt 2) / 2; var == 0: d > 0."""
    m, v, c, s = np.broadcast_arrays(np.asarray(mean, dtype=np.float64), np.asarray(var, dtype=np.float64),
                                     np.asarray(thr, dtype=np.float64), np.asarray(side, dtype=np.float64))
    out = np.empty(m.shape)
    mf, vf, cf, sf, of = m.reshape(-1), v.reshape(-1), c.reshape(-1), s.reshape(-1), out.reshape(-1)
    for k in range(of.size):
        d = (float(cf[k]) - float(mf[k])) if sf[k] < 0 else (float(mf[k]) - float(cf[k]))
        if vf[k] > 0.0:
            z = d / math.sqrt(float(vf[k]))       # (the root of a subnormal is a normal number: never a division by 0)
            of[k] = 0.5 * math.erfc(-z * _RSQRT2)
        else:
            of[k] = 1.0 if d > 0.0 else 0.0
    return out if out.ndim else float(out)


class Stream:
    """The streaming state of one target: ``update(p)`` folds one draw's probabilities (any shape, the same every time) into the
    Welford mean and M2, ``finish()`` returns dict(prob, prob_var, n_accumulated)."""

    def __init__(self):
        self.count, self.mean, self.m2 = 0, None, None

    def update(self, p):
        p = np.asarray(p, dtype=np.float64)
        if self.mean is None:
            self.mean, self.m2 = np.zeros(p.shape), np.zeros(p.shape)
        self.count += 1
        d = p - self.mean
        self.mean = self.mean + d / float(self.count)
        self.m2 = self.m2 + d * (p - self.mean)
        return self

    def finish(self):
        if self.count == 0:
            raise ValueError("exceed: no draw accumulated")
        return dict(prob=self.mean.copy(), prob_var=self.m2 / float(self.count), n_accumulated=self.count)


def exceed_w(cond_mean, cond_var, mv, thr, side):
    """prob, prob_var of target w from the per-draw moments: ``cond_mean``, ``cond_var`` (n, S), ``mv`` the 1-based margins (n),
    ``thr`` (T, q), ``side`` (T,).  Returns dict(prob (T, n), prob_var (T, n), n_accumulated)."""
    cm, cv = np.asarray(cond_mean, dtype=np.float64), np.asarray(cond_var, dtype=np.float64)
    thr, side = np.asarray(thr, dtype=np.float64), np.asarray(side)
    c = thr[:, np.asarray(mv, dtype=np.int64) - 1]                       # (T, n)
    st = Stream()
    for s in range(cm.shape[1]):
        st.update(draw_prob(cm[None, :, s], cv[None, :, s], c, side[:, None]))
    return st.finish()


def xb_chain(X, b):
    """x_i'b as the kernels form it: one fused multiply-add chain k = 0..p-1 (``math.fma`` where Python has it; otherwise each
    step is formed in exact rationals and rounded once)."""
    X = np.asarray(X, dtype=np.float64)
    out = np.zeros(X.shape[0])
    fma = getattr(math, "fma", None)
    for i in range(X.shape[0]):
        acc = 0.0
        for k in range(X.shape[1]):
            if fma is not None:
                acc = fma(float(X[i, k]), float(b[k]), acc)
            else:
                acc = float(Fraction(float(X[i, k])) * Fraction(float(b[k])) + Fraction(acc))
        out[i] = acc
    return out


def exceed_yhat(cond_mean, cond_var, mv, X, beta, tausq_inv, thr, side):
    """prob, prob_var of target yhat: ``X`` (n, p), ``beta`` (p, S, q) as the fit's ``beta_mcmc``, ``tausq_inv``
    (q, S).  mu = xb_chain + cond_mean, sigma2 = cond_var + 1 / tausq_inv."""
    cm, cv = np.asarray(cond_mean, dtype=np.float64), np.asarray(cond_var, dtype=np.float64)
    thr, side = np.asarray(thr, dtype=np.float64), np.asarray(side)
    j = np.asarray(mv, dtype=np.int64) - 1
    c = thr[:, j]
    beta, tsi = np.asarray(beta, dtype=np.float64), np.asarray(tausq_inv, dtype=np.float64)
    st = Stream()
    for s in range(cm.shape[1]):
        xb = np.zeros(cm.shape[0])
        for jj in np.unique(j):
            sel = j == jj
            xb[sel] = xb_chain(np.asarray(X)[sel], beta[:, s, jj])
        mu = xb + cm[:, s]
        s2 = cv[:, s] + 1.0 / tsi[j, s]
        st.update(draw_prob(mu[None, :], s2[None, :], c, side[:, None]))
    return st.finish()
