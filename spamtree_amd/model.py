"""Host-side mirror of the reference's `SpamTreeMV` (/root/reference/src/spamtree_model.h:22-212) over the C-ABI.

Same constructor arguments, method names and failure behaviour as the reference class, so parity tests read like
calls into the reference; every hot method is one C-ABI call into the HIP library.  Nothing here computes on the
CPU: without the library and a GPU the constructor raises.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from . import diagnostics as _diag
from . import exceed as _rb
from . import excursions as _exc
from . import mixture as _mix


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def _dp(a):
    return a.ctypes.data_as(_lib.c_dp)


def _ip(a):
    return a.ctypes.data_as(_lib.c_ip)


def _lists_to_csr(lists):
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(x) for x in lists])
    idx = np.concatenate([np.asarray(x, dtype=np.int64) for x in lists]) if len(lists) and ptr[-1] > 0 \
        else np.zeros(0, dtype=np.int64)
    return ptr, _i64(idx)


class SpamTreeError(RuntimeError):
    pass


def series_diag_buffers(n, want=True):
    """(dict of n-vectors ess, mcse, sd, rhat, lags; the st_series_diag pointing at them), or (None, None) without ``want``."""
    if not want:
        return None, None
    d = {k: np.zeros(n) for k in ("ess", "mcse", "sd", "rhat")}
    d["lags"] = np.zeros(n, dtype=np.int32)
    s = _lib.StSeriesDiag(_dp(d["ess"]), _dp(d["mcse"]), _dp(d["sd"]), _dp(d["rhat"]), d["lags"].ctypes.data_as(C.POINTER(C.c_int32)))
    return d, s


def series_diag_finish(d, K, max_lag=0):
    """Adds ``truncated`` (the series that ran into the lag cap) to a dict of device diagnostics of K stored draws."""
    if d is not None:
        d["truncated"] = _diag.truncated(d["lags"], K, max_lag)
    return d


def excursion_spec(thr, side, mask, band):
    """The st_excursion_spec of checked inputs (``thr`` (T, m) float64 or None, ``side`` (T,) int32, ``mask`` uint8 or None) and
    the arrays it points at, which must outlive the call."""
    keep = (thr, side, mask)
    s = _lib.StExcursionSpec(0 if thr is None else int(thr.shape[0]), None if thr is None else _dp(thr),
                             None if thr is None else side.ctypes.data_as(C.POINTER(C.c_int32)),
                             None if mask is None else mask.ctypes.data_as(C.POINTER(C.c_uint8)), 1 if band else 0)
    return s, keep


def excursion_buffers(n, T, G, K, band, want=True):
    """(dict of the outputs of one store; the st_excursion_out pointing at them), or (None, None) without ``want``: count, prob,
    excur (T, n) and joint_all (T, G) with T > 0; mean, sd (n), maxdev (G, K), n_flat (G) with ``band``; n_draws."""
    if not want:
        return None, None
    d, o = {}, _lib.StExcursionOut()
    if T:
        d.update(count=np.zeros((T, n), dtype=np.int32), prob=np.zeros((T, n)), excur=np.zeros((T, n)), joint_all=np.zeros((T, G)))
        o.count = d["count"].ctypes.data_as(C.POINTER(C.c_int32))
        o.prob, o.excur, o.joint_all = _dp(d["prob"]), _dp(d["excur"]), _dp(d["joint_all"])
    if band:
        d.update(mean=np.zeros(n), sd=np.zeros(n), maxdev=np.zeros((G, K)), n_flat=np.zeros(G, dtype=np.int64))
        o.mean, o.sd, o.maxdev = _dp(d["mean"]), _dp(d["sd"]), _dp(d["maxdev"])
        o.n_flat = d["n_flat"].ctypes.data_as(C.POINTER(C.c_int64))
    d["n_draws"] = np.zeros(1, dtype=np.int64)
    o.n_draws = d["n_draws"].ctypes.data_as(C.POINTER(C.c_int64))
    return d, o


def excursion_finish(d):
    if d is not None:
        d["n_draws"] = int(d["n_draws"][0])
    return d


def rank_spec(probs, thresholds, sides, max_lag, m):
    """The st_rank_spec of ``probs`` (at most 8, strictly inside (0, 1)), ``thresholds`` (at most 8 entries, each a scalar or m
    values: ``excursions.expand_thresholds``) and ``sides``, checked (ValueError), and the arrays it points at, which must
    outlive the call: (spec, keep, n_prob, n_thr)."""
    pr, th, sd = _diag.check_rank_spec(probs, thresholds, 1 if sides is None else sides, max_lag)
    prob = np.ascontiguousarray(pr, dtype=np.float64)
    thr = side = None
    if th:
        thr, side = _exc.expand_thresholds(th, m, sd)
    s = _lib.StRankSpec(int(max_lag), prob.size, _dp(prob) if prob.size else None, 0 if thr is None else int(thr.shape[0]),
                        None if thr is None else _dp(thr), None if thr is None else side.ctypes.data_as(C.POINTER(C.c_int32)))
    return s, (prob, thr, side), prob.size, 0 if thr is None else int(thr.shape[0])


def rank_buffers(n, n_prob, n_thr, want=True):
    """(dict of the outputs of one store; the st_rank_out pointing at them), or (None, None) without ``want``: rhat_rank,
    rhat_bulk, rhat_fold, ess_bulk, ess_tail, lags_bulk (n); ess_q (n_prob, n); ess_exc, mcse_prob, prob (n_thr, n)."""
    if not want:
        return None, None
    d = {k: np.zeros(n) for k in ("rhat_rank", "rhat_bulk", "rhat_fold", "ess_bulk", "ess_tail")}
    d["lags_bulk"] = np.zeros(n, dtype=np.int32)
    d["ess_q"] = np.zeros((n_prob, n))
    d.update({k: np.zeros((n_thr, n)) for k in ("ess_exc", "mcse_prob", "prob")})
    o = _lib.StRankOut(_dp(d["rhat_rank"]), _dp(d["rhat_bulk"]), _dp(d["rhat_fold"]), _dp(d["ess_bulk"]), _dp(d["ess_tail"]),
                       d["lags_bulk"].ctypes.data_as(C.POINTER(C.c_int32)), _dp(d["ess_q"]) if n_prob else None,
                       _dp(d["ess_exc"]) if n_thr else None, _dp(d["mcse_prob"]) if n_thr else None, _dp(d["prob"]) if n_thr else None)
    return d, o


def rank_finish(d, K, max_lag=0):
    """Adds ``truncated`` (the series whose bulk pairs ran into the lag cap) to a dict of device rank diagnostics of K draws."""
    if d is not None:
        d["truncated"] = _diag.truncated(d["lags_bulk"], K, max_lag)
    return d


POINTS_MAX_JOINT = 16   # include/spamtree_hip.h: ST_POINTS_MAX_JOINT


def joint_labels(joint, n):
    """The joint-group labels of a point set as int64, checked: one integer per point, at most POINTS_MAX_JOINT per label."""
    labels = np.asarray(joint)
    if labels.ndim != 1 or labels.shape[0] != n:
        raise ValueError("joint must hold one label per point")
    if not np.issubdtype(labels.dtype, np.integer):
        raise ValueError("joint labels must be integers")
    if n and np.unique(labels, return_counts=True)[1].max() > POINTS_MAX_JOINT:
        raise ValueError(f"a joint group holds at most {POINTS_MAX_JOINT} points")
    return _i64(labels)


def score_values(y_new, n_points, have_X=True):
    """Held-out observations at ``n_points`` points as one float64 vector, checked before any device call: one value per point,
    NaN for a point that is not scored, nothing infinite; the scores need the regressors of the points."""
    y = np.asarray(y_new, dtype=np.float64)
    if y.ndim == 2 and 1 in y.shape:
        y = y.reshape(-1)
    if y.ndim != 1 or y.size != n_points:
        raise ValueError(f"y_new must hold one value per new point ({n_points}), NaN where a point is not scored")
    if not have_X:
        raise ValueError("y_new needs X_new: the scored predictive is that of the outcome, x'beta + w + noise")
    bad = np.nonzero(np.isinf(y))[0]
    if bad.size:
        raise ValueError(f"y_new[{int(bad[0])}] is infinite (NaN marks a point that is not scored)")
    return _f64(y)


def score_totals(scores, y, mv, q, yhat_lo=None, yhat_hi=None):
    """Host-side totals of st_points_score_get's per-point arrays: the mean lpd, pit and crps over the scored points, overall and
    per outcome (``by_outcome``: q entries, NaN for an outcome without a scored point) and, with the lowest and highest requested
    quantile of yhat, the coverage of [yhat_lo, yhat_hi]."""
    obs = ~np.isnan(y)
    mv = np.asarray(mv).reshape(-1)
    keys = [k for k in ("lpd", "pit", "crps") if scores.get(k) is not None]
    cover = None
    if yhat_lo is not None and yhat_hi is not None:
        cover = ((y >= yhat_lo) & (y <= yhat_hi)).astype(np.float64)
        keys.append("coverage")

    def mean(k, sel):
        v = cover if k == "coverage" else scores[k]
        return float(np.mean(v[sel])) if np.any(sel) else float("nan")
    tot = {k: mean(k, obs) for k in keys}
    tot["by_outcome"] = {k: np.array([mean(k, obs & (mv == j + 1)) for j in range(q)]) for k in keys}
    return tot


def rows_holdout(y_holdout, y):
    """Held-out values at NA rows of the problem as one float64 vector in model row order, checked before any device call: one
    value per row of ``y``, NaN where there is none, finite only where ``y`` is NaN, nothing infinite.  None stays None."""
    if y_holdout is None:
        return None
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    t = np.asarray(y_holdout, dtype=np.float64)
    if t.ndim == 2 and 1 in t.shape:
        t = t.reshape(-1)
    if t.ndim != 1 or t.size != y.size:
        raise ValueError(f"y_holdout must hold one value per row of y ({y.size}), NaN where there is no held-out value")
    bad = np.nonzero(np.isinf(t))[0]
    if bad.size:
        raise ValueError(f"y_holdout[{int(bad[0])}] is infinite (NaN marks a row without a held-out value)")
    bad = np.nonzero(np.isfinite(t) & np.isfinite(y))[0]
    if bad.size:
        raise ValueError(f"y_holdout[{int(bad[0])}] is finite at an observed row (held-out values belong to the NA rows of y)")
    return _f64(t)


def rows_criteria(obs, held, n_obs, n_held, have_crps=True):
    """st_rows_score_totals' two tables (ST_ROWS_OBS_N x q and ST_ROWS_HELD_N x q, one column per outcome) as
    dict(observed, held_out), each overall and ``by_outcome``.  observed: n, lppd, p_waic, waic, Dbar, Dhat, p_D, dic -- the overall
    lppd, p_waic, Dbar and Dhat are the outcomes' sums in outcome order and waic = -2 (lppd - p_waic), p_D = Dbar - Dhat,
    dic = Dbar + p_D are formed from those doubles, as the library forms each outcome's.  held_out: n and the means lppd (the log
    score), pit, crps (None without stored draws), mse, and rmse; NaN where there is no held-out row.  All conditional on w."""
    obs = np.asarray(obs, dtype=np.float64).reshape(len(_lib.ST_ROWS_OBS), -1, order="F")
    held = np.asarray(held, dtype=np.float64).reshape(len(_lib.ST_ROWS_HELD), -1, order="F")
    n_obs, n_held = np.asarray(n_obs, dtype=np.int64), np.asarray(n_held, dtype=np.int64)
    o = {k: obs[i].copy() for i, k in enumerate(_lib.ST_ROWS_OBS)}
    observed = dict(n=int(n_obs.sum()))
    for k in ("lppd", "p_waic", "Dbar", "Dhat"):
        t = 0.0
        for v in o[k]:          # in outcome order
            t = t + float(v)
        observed[k] = t
    observed["waic"] = -2.0 * (observed["lppd"] - observed["p_waic"])
    observed["p_D"] = observed["Dbar"] - observed["Dhat"]
    observed["dic"] = observed["Dbar"] + observed["p_D"]
    observed["by_outcome"] = dict(o, n=n_obs.copy())
    with np.errstate(invalid="ignore", divide="ignore"):
        hm = {k: np.where(n_held > 0, held[i] / n_held, np.nan) for i, k in enumerate(_lib.ST_ROWS_HELD)}
    nh = int(n_held.sum())
    held_out = dict(n=nh)
    for i, k in enumerate(_lib.ST_ROWS_HELD):
        t = 0.0
        for v in held[i]:
            t = t + float(v)
        held_out[k] = t / nh if nh else float("nan")
    for d in (held_out, hm):
        d["mse"] = d.pop("sqerr")
        d["rmse"] = np.sqrt(d["mse"])
        if not have_crps:
            d["crps"] = None
    held_out["rmse"] = float(held_out["rmse"])
    held_out["by_outcome"] = dict(hm, n=n_held.copy())
    return dict(observed=observed, held_out=held_out)


def rows_loo_criteria(tot, n_obs):
    """st_rows_loo_totals' table (ST_ROWS_LOO_N x q, one column per outcome) as a dict, overall and ``by_outcome``: n, elpd_loo,
    looic = -2 elpd_loo, the means mse, rmse and pit of the leave-one-out predictions, and min_weight_ess.  The overall elpd_loo and
    the sums behind the means are the outcomes' in outcome order.  Marginal over each row's own w_i (``spamtree_amd.loo``)."""
    tot = np.asarray(tot, dtype=np.float64).reshape(len(_lib.ST_ROWS_LOO), -1, order="F")
    n_obs = np.asarray(n_obs, dtype=np.int64)
    t = {k: tot[i].copy() for i, k in enumerate(_lib.ST_ROWS_LOO)}
    nn = int(n_obs.sum())
    sums = {}
    for k in ("elpd_loo", "sqerr", "pit"):
        a = 0.0
        for v, c in zip(t[k], n_obs):          # in outcome order
            if c > 0:
                a = a + float(v)
        sums[k] = a
    with np.errstate(invalid="ignore", divide="ignore"):
        by = dict(n=n_obs.copy(), elpd_loo=t["elpd_loo"], looic=t["looic"], mse=np.where(n_obs > 0, t["sqerr"] / n_obs, np.nan),
                  pit=np.where(n_obs > 0, t["pit"] / n_obs, np.nan), min_weight_ess=t["min_weight_ess"])
    by["rmse"] = np.sqrt(by["mse"])
    ess = [float(v) for v, c in zip(t["min_weight_ess"], n_obs) if c > 0]
    out = dict(n=nn, elpd_loo=sums["elpd_loo"], looic=-2.0 * sums["elpd_loo"], mse=sums["sqerr"] / nn if nn else float("nan"),
               pit=sums["pit"] / nn if nn else float("nan"), min_weight_ess=min(ess) if ess else float("nan"))
    out["rmse"] = float(np.sqrt(out["mse"]))
    out["by_outcome"] = by
    return out


def rows_psis_criteria(tot, n_obs):
    """st_rows_loo_psis_totals' table (ST_ROWS_PSIS_N x q, one column per outcome) as a dict, overall and ``by_outcome``: n (rows with
    a value), elpd_psis, looic = -2 elpd_psis, se = sqrt(n var) of the pointwise elpd_psis (var with divisor n - 1; NaN below two
    rows), the means mse, rmse and pit, min_weight_ess, max_khat, n_khat_bad (khat > 0.7) and n_khat_above (khat above the
    sample-size threshold min(1 - 1 / log10 S, 0.7)).  The overall sums are the outcomes' in outcome order."""
    tot = np.asarray(tot, dtype=np.float64).reshape(len(_lib.ST_ROWS_PSIS), -1, order="F")
    n_obs = np.asarray(n_obs, dtype=np.int64)
    t = {k: tot[i].copy() for i, k in enumerate(_lib.ST_ROWS_PSIS)}
    cnt = t["count"].astype(np.int64)

    def se(n, s1, s2):
        if n < 2:
            return float("nan")
        var = max(s2 - s1 * s1 / n, 0.0) / (n - 1)
        return float(np.sqrt(n * var))

    sums = {}
    for k in ("elpd_psis", "elpd_psis_sq", "sqerr", "pit", "n_khat_bad", "n_khat_above"):
        a = 0.0
        for v, c in zip(t[k], cnt):          # in outcome order
            if c > 0:
                a = a + float(v)
        sums[k] = a
    with np.errstate(invalid="ignore", divide="ignore"):
        by = dict(n=cnt, n_obs=n_obs.copy(), elpd_psis=t["elpd_psis"], looic=-2.0 * t["elpd_psis"],
                  se=np.array([se(int(c), float(a), float(b)) for c, a, b in zip(cnt, t["elpd_psis"], t["elpd_psis_sq"])]),
                  mse=np.where(cnt > 0, t["sqerr"] / cnt, np.nan), pit=np.where(cnt > 0, t["pit"] / cnt, np.nan),
                  min_weight_ess=t["min_weight_ess"], max_khat=t["max_khat"], n_khat_bad=t["n_khat_bad"].astype(np.int64),
                  n_khat_above=t["n_khat_above"].astype(np.int64))
    by["rmse"] = np.sqrt(by["mse"])
    nn = int(cnt.sum())
    ess = [float(v) for v, c in zip(t["min_weight_ess"], cnt) if c > 0]
    kh = [float(v) for v, c in zip(t["max_khat"], cnt) if c > 0]
    out = dict(n=nn, elpd_psis=sums["elpd_psis"], looic=-2.0 * sums["elpd_psis"], se=se(nn, sums["elpd_psis"], sums["elpd_psis_sq"]),
               mse=sums["sqerr"] / nn if nn else float("nan"), pit=sums["pit"] / nn if nn else float("nan"),
               min_weight_ess=min(ess) if ess else float("nan"), max_khat=max(kh) if kh else float("nan"),
               n_khat_bad=int(sums["n_khat_bad"]), n_khat_above=int(sums["n_khat_above"]))
    out["rmse"] = float(np.sqrt(out["mse"]))
    out["by_outcome"] = by
    return out


def functionals_csr(A, n_points):
    """Linear functionals of the predictions at ``n_points`` points as CSR ``(ptr, idx, wt)``, checked before any device call.
    ``A``: a ``(ptr, idx, wt)`` triple (a tuple of three whose entries are not themselves (indices, weights) pairs); a dense n_fun x n_points array, whose zeros are dropped; or a list of
    ``(indices, weights)`` pairs.  ValueError on bad shapes, indices outside 0..n_points-1, non-finite weights or a point that
    occurs twice in one functional."""
    n_points = int(n_points)
    if isinstance(A, tuple) and len(A) == 3 and not all(isinstance(x, (list, tuple)) and len(x) == 2 and np.ndim(x[0]) == 1 for x in A):
        ptr, idx, wt = (np.asarray(x) for x in A)
        if ptr.ndim != 1 or idx.ndim != 1 or wt.ndim != 1 or ptr.size < 1:
            raise ValueError("functionals: ptr, idx and wt must be one-dimensional and ptr must hold n_fun + 1 entries")
        if not (np.issubdtype(ptr.dtype, np.integer) and np.issubdtype(idx.dtype, np.integer)):
            raise ValueError("functionals: ptr and idx must be integers")
    elif isinstance(A, (list, tuple)):
        rows = []
        for f, pair in enumerate(A):
            if not (isinstance(pair, (list, tuple)) and len(pair) == 2):
                raise ValueError(f"functionals: entry {f} is not an (indices, weights) pair")
            i, w = np.asarray(pair[0]).reshape(-1), np.asarray(pair[1], dtype=np.float64).reshape(-1)
            if i.size and not np.issubdtype(i.dtype, np.integer):
                raise ValueError(f"functionals: the indices of functional {f} must be integers")
            if i.size != w.size:
                raise ValueError(f"functionals: functional {f} has {i.size} indices and {w.size} weights")
            rows.append((i.astype(np.int64), w))
        ptr = np.concatenate([[0], np.cumsum([r[0].size for r in rows])]).astype(np.int64)
        idx = np.concatenate([r[0] for r in rows]) if rows else np.zeros(0, dtype=np.int64)
        wt = np.concatenate([r[1] for r in rows]) if rows else np.zeros(0)
    else:
        D = np.asarray(A, dtype=np.float64)
        if D.ndim != 2 or D.shape[1] != n_points:
            raise ValueError(f"functionals: a dense array must be n_fun x n_new = n_fun x {n_points}")
        if not np.all(np.isfinite(D)):
            raise ValueError("functionals: weights must be finite")
        r, c = np.nonzero(D)
        ptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=D.shape[0]))]).astype(np.int64)
        idx, wt = c.astype(np.int64), D[r, c]
    ptr, idx, wt = _i64(ptr), _i64(idx), _f64(wt)
    if ptr[0] != 0 or np.any(np.diff(ptr) < 0) or ptr[-1] != idx.size or idx.size != wt.size:
        raise ValueError("functionals: ptr must start at 0, not decrease and end at the number of entries of idx and wt")
    if idx.size and (idx.min() < 0 or idx.max() >= n_points):
        raise ValueError(f"functionals: indices must lie in 0..{n_points - 1}")
    if not np.all(np.isfinite(wt)):
        raise ValueError("functionals: weights must be finite")
    row = np.repeat(np.arange(ptr.size - 1, dtype=np.int64), np.diff(ptr))
    if idx.size and np.unique(row * max(n_points, 1) + idx).size != idx.size:
        raise ValueError("functionals: a point occurs twice in one functional")
    return ptr, idx, wt


class SpamTreeMV:
    """spamtree_model.cpp:8-192.  `param_data` / `alter_data` are slots 0 / 1 of the device handle."""

    PARAM, ALTER = 0, 1

    def __init__(self, y, X, Z, coords, mv_id, blocking, gix_block, res_is_ref, parents, children, limited_tree,
                 block_names, block_groups, indexing, w, beta, theta, tausq_inv,
                 device=0, reference_quirks=True, force_generic=False, rank=0, world=1, cache_gram=True,
                 defer_leaf=True):
        self.lib = _lib.load()
        y = _f64(np.asarray(y).reshape(-1))
        X = np.asfortranarray(np.asarray(X, dtype=np.float64))
        coords = np.asfortranarray(np.asarray(coords, dtype=np.float64))
        mv_id = _i64(mv_id)
        self.n_all, self.p = X.shape
        self.q = int(np.unique(mv_id).size)
        self.dd = coords.shape[1]
        ip, ii = indexing if isinstance(indexing, tuple) else _lists_to_csr(indexing)
        pp, pi = parents if isinstance(parents, tuple) else _lists_to_csr(parents)
        cp, ci = children if isinstance(children, tuple) else _lists_to_csr(children)
        keep = [y, X, coords, mv_id, _i64(res_is_ref), _i64(block_names), _i64(block_groups), _i64(ip), _i64(ii),
                _i64(pp), _i64(pi), _i64(cp), _i64(ci)]
        pb = _lib.StProblem(self.n_all, self.dd, self.q, self.p, int(keep[4].size), int(keep[5].size),
                            _dp(y), _dp(X), _dp(coords), _ip(mv_id), _ip(keep[4]), _ip(keep[5]), _ip(keep[6]),
                            _ip(keep[7]), _ip(keep[8]), _ip(keep[9]), _ip(keep[10]), _ip(keep[11]), _ip(keep[12]))
        opt = _lib.StOptions(int(device), int(bool(reference_quirks)), int(rank), int(world), int(bool(force_generic)),
                              (0 if cache_gram else 1) | (2 if limited_tree else 0) | (0 if defer_leaf else 4))
        self.rank, self.world = int(rank), int(world)
        h = C.c_void_p()
        rc = self.lib.st_create(C.byref(pb), C.byref(opt), C.byref(h))
        if rc != 0:
            raise SpamTreeError(f"st_create failed ({rc}): {self.lib.st_last_error(None).decode()}")
        self.h = h
        self.n_blocks = int(keep[5].size)
        self.theta = [np.asarray(theta, dtype=np.float64).copy(), np.asarray(theta, dtype=np.float64).copy()]
        self.loglik_w = [float("nan"), float("nan")]
        self.last_errtype = self.last_sample_errtype = -1      # errtype of the last phase A / sweep (-1: none)
        self.Bcoeff = np.zeros((self.p, self.q), order="F")
        beta = np.asarray(beta, dtype=np.float64).reshape(-1)
        for j in range(self.q):
            self.Bcoeff[:, j] = beta
        self.beta_update(self.Bcoeff)
        self.tausq_inv = np.ones(self.q) * float(tausq_inv)
        self._check(self.lib.st_set_tausq_inv(self.h, _dp(self.tausq_inv)))
        self.w = np.asarray(w, dtype=np.float64).reshape(-1).copy()
        self._check(self.lib.st_set_w(self.h, _dp(_f64(self.w))))
        xtx = np.zeros(self.p * self.p * self.q)
        self._check(self.lib.st_xtx(self.h, _dp(xtx)))
        self.XtX = [xtx[j * self.p * self.p:(j + 1) * self.p * self.p].reshape(self.p, self.p).T.copy()
                    for j in range(self.q)]
        self.Vi = 0.01 * np.eye(self.p)
        self.Vim = np.zeros(self.p)
        nq = np.zeros(self.q, dtype=np.int64)
        ssq = np.zeros(self.q)
        self._check(self.lib.st_tausq_stats(self.h, _dp(ssq), _ip(nq)))
        self.n_obs_by_q = nq

    def close(self):
        if getattr(self, "h", None):
            self.lib.st_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc < 0:
            raise SpamTreeError(f"spamtree_hip error {rc}: {self.lib.st_last_error(self.h).decode()}")
        return rc

    # ---- spamtree_model.cpp:1420-1422
    def theta_update(self, slot, new_param):
        self.theta[slot] = np.asarray(new_param, dtype=np.float64).copy()

    # ---- spamtree_model.cpp:829-998 ; returns the reference's bool
    def get_loglik_comps_w(self, slot) -> bool:
        th = _f64(self.theta[slot])
        ll = C.c_double(0.0)
        rc = self._check(self.lib.st_factor(self.h, slot, _dp(th), th.size, C.byref(ll)))
        self.last_errtype = rc if rc > 0 else -1
        if rc > 0:
            return False
        self.loglik_w[slot] = ll.value
        return True

    # ---- spamtree_model.cpp:1000-1226
    def deal_with_w(self, z=None, seed=0, it=0):
        if z is not None:
            z = _f64(z)
            rc = self._check(self.lib.st_sample_w(self.h, _dp(z), 0, 0))
        else:
            rc = self._check(self.lib.st_sample_w(self.h, None, int(seed), int(it)))
        self.last_sample_errtype = rc if rc > 0 else -1
        if rc > 0:
            raise SpamTreeError("Error at gibbs_sample_w")           # Rcpp::stop (:1215-1217)

    gibbs_sample_w = deal_with_w

    # ---- spamtree_model.cpp:776-826
    def get_loglik_w(self, slot):
        ll = C.c_double(0.0)
        self._check(self.lib.st_loglik_w(self.h, slot, C.byref(ll)))
        self.loglik_w[slot] = ll.value
        return ll.value

    # ---- spamtree_model.cpp:1229-1358
    def predict(self, theta_update=True):
        self._check(self.lib.st_predict(self.h, int(bool(theta_update))))

    # ---- spamtree_model.cpp:1364-1391 (normals_by_q[j] = arma::randn(p) of :1378)
    def gibbs_sample_beta(self, normals_by_q):
        xty = np.zeros(self.p * self.q)
        self._check(self.lib.st_beta_stats(self.h, _dp(xty)))
        xty = xty.reshape(self.q, self.p).T
        for j in range(self.q):
            Si_chol = np.linalg.cholesky(self.tausq_inv[j] * self.XtX[j] + self.Vi)
            Sc = np.linalg.solve(Si_chol, np.eye(self.p))
            Xprecy_j = self.Vim + self.tausq_inv[j] * xty[:, j]
            self.Bcoeff[:, j] = Sc.T @ (Sc @ Xprecy_j) + Sc.T @ np.asarray(normals_by_q[j], dtype=np.float64)
        self.beta_update(self.Bcoeff)

    deal_with_beta = gibbs_sample_beta

    # ---- spamtree_model.cpp:1393-1417 (gamma_draw(j, shape, scale) = R::rgamma)
    def gibbs_sample_tausq(self, gamma_draw):
        ssq = np.zeros(self.q)
        self._check(self.lib.st_tausq_stats(self.h, _dp(ssq), None))
        for j in range(self.q):
            aparam = 2.01 + self.n_obs_by_q[j] / 2.0
            bparam = 1.0 / (1.0 + 0.5 * ssq[j])
            self.tausq_inv[j] = gamma_draw(j, aparam, bparam)
        self._check(self.lib.st_set_tausq_inv(self.h, _dp(_f64(self.tausq_inv))))

    def tausq_update(self, new_tausq):                                  # :1424-1426
        self.tausq_inv = np.ones(self.q) / float(new_tausq)
        self._check(self.lib.st_set_tausq_inv(self.h, _dp(_f64(self.tausq_inv))))

    def beta_update(self, new_beta):                                    # :1428-1430 (+ XB refresh)
        self.Bcoeff = np.asfortranarray(np.asarray(new_beta, dtype=np.float64).reshape(self.p, self.q))
        self._check(self.lib.st_set_beta(self.h, _dp(self.Bcoeff)))

    def accept_make_change(self):                                       # :1432-1435
        self._check(self.lib.st_swap(self.h))
        self.theta[0], self.theta[1] = self.theta[1], self.theta[0]
        self.loglik_w[0], self.loglik_w[1] = self.loglik_w[1], self.loglik_w[0]

    # ---- public fields of the reference object
    def get_w(self):
        out = np.zeros(self.n_all)
        self._check(self.lib.st_get_w(self.h, _dp(out)))
        self.w = out
        return out

    def set_w(self, w):
        self.w = np.asarray(w, dtype=np.float64).copy()
        self._check(self.lib.st_set_w(self.h, _dp(_f64(self.w))))

    def get_XB(self):
        out = np.zeros(self.n_all)
        self._check(self.lib.st_get_xb(self.h, _dp(out)))
        return out

    def stats(self):
        xty = np.zeros(self.p * self.q)
        ssq = np.zeros(self.q)
        self._check(self.lib.st_beta_stats(self.h, _dp(xty)))
        self._check(self.lib.st_tausq_stats(self.h, _dp(ssq), None))
        return xty.reshape(self.q, self.p).T.copy(), ssq

    def yhat(self, noise=None, seed=0, it=0):
        out = np.zeros(self.n_all)
        if noise is not None:
            noise = _f64(noise)
            self._check(self.lib.st_yhat(self.h, _dp(noise), 0, 0, _dp(out)))
        else:
            self._check(self.lib.st_yhat(self.h, None, int(seed), int(it), _dp(out)))
        return out

    # ---- inspection for parity tests
    def block(self, slot, u, raw=False):
        """(H, Ri) of block u: H = K_{u,pa} K_{pa,pa}^{-1} (m x P) recovered from the stored panel, Ri = chol(R)^{-1}
        (m x m) for a reference block or the m per-row values 1/sqrt(r_ii) for a non-reference block.  raw=True: (N, Ri)
        with N = -Ri H (m x P) the stored panel itself, without the solve that recovers H."""
        m, P = C.c_int64(), C.c_int64()
        isref, nobs = C.c_int32(), C.c_int32()
        self._check(self.lib.st_block_dims(self.h, u, C.byref(m), C.byref(P), C.byref(isref), C.byref(nobs)))
        m, P = m.value, P.value
        N = np.zeros(m * max(P, 1))
        Ri = np.zeros(m * m if isref.value else m)
        self._check(self.lib.st_get_block(self.h, slot, u, _dp(N), _dp(Ri)))
        N = N[: m * P].reshape(P, m).T if P else np.zeros((m, 0))
        if isref.value:
            Ri = Ri.reshape(m, m).T
        if raw:
            return N, Ri
        if isref.value:
            H = -np.linalg.solve(Ri, N) if P else N
        else:
            H = -N / Ri[:, None] if P else N
        return H, Ri

    def simulate(self, nd=1, z=None, eps=None, seed=2021, it=0, outcomes=True):
        """Draws from the model slot 0 was last factorised for (st_simulate): w ~ N(0, C_DAG) and y = XB + w + tau eps with
        the handle's beta and tausq.  Returns (w, y), n x nd in model order (y None without ``outcomes``).  Draw d uses Philox
        iteration it + d (streams 8 / 9), or column d of the caller's ``z`` / ``eps`` (n x nd).  Changes no state."""
        nd = int(nd)
        zz = None if z is None else np.asfortranarray(np.asarray(z, dtype=np.float64).reshape(self.n_all, nd))
        ee = None if eps is None else np.asfortranarray(np.asarray(eps, dtype=np.float64).reshape(self.n_all, nd))
        w = np.zeros((self.n_all, max(nd, 0)), order="F")
        y = np.zeros((self.n_all, max(nd, 0)), order="F") if outcomes else None
        self._check(self.lib.st_simulate(self.h, nd, _dp(zz) if zz is not None else None, _dp(ee) if ee is not None else None,
                                         int(seed), int(it), _dp(w), _dp(y) if y is not None else None))
        return w, y

    def simulate_info(self, nd=1):
        mask, b, f = C.c_int32(0), C.c_double(0.0), C.c_double(0.0)
        self._check(self.lib.st_simulate_info(self.h, int(nd), C.byref(mask), C.byref(b), C.byref(f)))
        names = [self.lib.st_simulate_route_name(c).decode() for c in range(1, 32) if mask.value >> (c - 1) & 1]
        return dict(route_mask=mask.value, routes=names, alg_bytes=b.value, flops=f.value)

    def comps(self, slot):
        a = np.zeros(self.n_blocks)
        b = np.zeros(self.n_blocks)
        self._check(self.lib.st_get_comps(self.h, slot, _dp(a), _dp(b)))
        return a, b

    def algorithmic_bytes(self):
        out = np.zeros(5)
        fl = np.zeros(3)
        self._check(self.lib.st_algorithmic_bytes(self.h, _dp(out), _dp(fl)))
        return dict(A=out[0], B=out[1], C=out[2], msg=out[3], S=out[4], total=float(out.sum()),
                    flops_A=fl[0], flops_B=fl[1], flops_C=fl[2])

    def profile(self, enable):
        self._check(self.lib.st_profile_enable(self.h, 2 if enable == 2 else int(bool(enable))))

    def profile_get(self):
        ms = np.zeros(8)
        n = np.zeros(8, dtype=np.int64)
        self._check(self.lib.st_profile_get(self.h, _dp(ms), _ip(n)))
        names = ["factor", "sample", "loglik", "reduce", "stats", "rng", "predict", "comm"]
        return {k: (float(ms[i]), int(n[i])) for i, k in enumerate(names)}

    def profile_levels(self):
        nl = C.c_int32()
        ms = np.zeros(64)
        by = np.zeros(64)
        self._check(self.lib.st_profile_levels(self.h, C.byref(nl), _dp(ms), _dp(by), 64))
        return ms[: nl.value].copy(), by[: nl.value].copy()

    def profile_levels_sample(self):
        """Mean k_sample* launch time per level (ms) since the last call."""
        nl = C.c_int32()
        ms = np.zeros(128)
        by = np.zeros(128)
        self._check(self.lib.st_profile_levels(self.h, C.byref(nl), _dp(ms), _dp(by), 128))
        return ms[nl.value: 2 * nl.value].copy(), by[nl.value: 2 * nl.value].copy()

    KERNEL_NAMES = ["generic_lds", "generic_scratch", "k_factor_mfma", "k_factor_quad", "k_factor_bigmfma", "k_factor_wide", "k_factor_lchain", "k_factor_lchain+ref_finish"]

    def level_info(self):
        """Per observed level: dict(kernel=name of the phase-A kernel, max_m, max_P, n_blocks)."""
        nl = C.c_int32()
        arr = [np.zeros(64, dtype=np.int32) for _ in range(4)]
        ptr = [a.ctypes.data_as(C.POINTER(C.c_int32)) for a in arr]
        self._check(self.lib.st_level_info(self.h, C.byref(nl), ptr[0], ptr[1], ptr[2], ptr[3], 64))
        return [dict(kernel=self.KERNEL_NAMES[arr[0][g]], max_m=int(arr[1][g]), max_P=int(arr[2][g]), n_blocks=int(arr[3][g]))
                for g in range(nl.value)]

    def route_info(self):
        """What the launch sites actually ran the last time: dict(levels=[dict(A=[kernels of phase A in launch order],
        gram=Gram kernel of the level's last sweep or None, sweep=its sweep kernel or None) per observed level],
        predict=kernel of the last predict or None).  Names are the template instantiations as the source spells them."""
        nl = C.c_int32()
        cap = 64
        a = np.zeros(3 * cap, dtype=np.int32)
        b = np.zeros(2 * cap, dtype=np.int32)
        p = C.c_int32()
        ip = C.POINTER(C.c_int32)
        self._check(self.lib.st_route_info(self.h, C.byref(nl), a.ctypes.data_as(ip), b.ctypes.data_as(ip), C.byref(p), cap))

        def name(code):
            return self.lib.st_route_name(int(code)).decode() if code else None
        levels = [dict(A=[name(c) for c in a[3 * g:3 * g + 3] if c], gram=name(b[2 * g]), sweep=name(b[2 * g + 1]))
                  for g in range(min(nl.value, cap))]
        return dict(levels=levels, predict=name(p.value))

    def synchronize(self):
        self._check(self.lib.st_synchronize(self.h))

    # ---- new-point prediction (include/spamtree_hip.h, st_points_*): not a method of the reference object
    def set_points(self, coords, mv, anchor, X=None, joint=None):
        """New locations to predict at: coords n_new x 2, mv 1-based margins, anchor 0-based block ids
        (spamtree_amd.predict.locate), X n_new x p regressors or None (then no yhat).  ``joint``: one integer label per
        point; points with the same label (at most 16, one conditioning chain: give them one anchor, predict.locate(joint=))
        form a joint group and predict_points draws them together (st_points_set_joint)."""
        coords = np.asfortranarray(np.asarray(coords, dtype=np.float64).reshape(-1, 2))
        n = coords.shape[0]
        mv = _i64(np.asarray(mv).reshape(-1))
        anchor = _i64(np.asarray(anchor).reshape(-1))
        if mv.size != n or anchor.size != n:
            raise ValueError("coords, mv and anchor must describe the same points")
        Xf = None
        if X is not None:
            Xf = np.asfortranarray(np.asarray(X, dtype=np.float64).reshape(n, self.p))
        Xp = _dp(Xf) if Xf is not None else None
        self.joint_groups = None
        if joint is None:
            self._check(self.lib.st_points_set(self.h, n, _dp(coords), _ip(mv), _ip(anchor), Xp))
        else:
            labels = joint_labels(joint, n)
            self._check(self.lib.st_points_set_joint(self.h, n, _dp(coords), _ip(mv), _ip(anchor), Xp, _ip(labels)))
            nj = C.c_int64()
            self._check(self.lib.st_points_joint_layout(self.h, C.byref(nj), None, None, None))
            off, ptr, mem = (np.zeros(nj.value + 1, dtype=np.int64), np.zeros(nj.value + 1, dtype=np.int64),
                             np.zeros(n, dtype=np.int64))
            self._check(self.lib.st_points_joint_layout(self.h, C.byref(nj), _ip(off), _ip(ptr), _ip(mem)))
            self.joint_offsets = off
            self.joint_groups = [mem[ptr[k]:ptr[k + 1]].copy() for k in range(nj.value)]
        self.n_points = n
        self.points_have_X = Xf is not None
        self.n_functionals = 0       # a new point set has none
        self.score_y = None          # ... and no scores
        self.exceed_spec = None      # ... and no exceedance thresholds
        self.mixture_keep = 0        # ... and no mixture store
        self.points_mv = mv

    def unpack_joint(self, packed):
        """The g x g blocks of a packed cond_cov / cond_chol / summary covariance, in group order: one [n_groups, g, g] array
        when every group has the same size, else a list."""
        off = self.joint_offsets
        blocks = [np.asarray(packed[off[k]:off[k + 1]]).reshape(m.size, m.size, order="F").copy()
                  for k, m in enumerate(self.joint_groups)]
        if blocks and len({b.shape for b in blocks}) == 1:
            return np.stack(blocks)
        return blocks

    def predict_points(self, mode=0, z=None, seed=0, it=0):
        """Predictive at the point set on slot 0 and the current w / beta / tausq: dict(w, mean, var, yhat) in the caller's
        order (yhat None without X).  mode 0 draws (z given, or Philox stream 6), mode 1 gives the conditional mean.
        On a joint set (set_points(joint=)) the groups are drawn jointly and the dict also holds ``cov`` and ``chol``, the
        conditional covariance of every group and its lower Cholesky factor (unpack_joint; groups and members as
        ``joint_groups``), and ``var`` is the diagonal of ``cov`` clamped at 0."""
        n = self.n_points
        if getattr(self, "joint_groups", None) is not None:
            return self._predict_points_joint(mode, z, seed, it)
        out = {k: np.zeros(n) for k in ("w", "mean", "var")}
        out["yhat"] = np.zeros(n) if self.points_have_X else None
        zz = _f64(np.asarray(z).reshape(-1)) if z is not None else None
        if zz is not None and zz.size != n:
            raise ValueError("z must hold one normal per point")
        self._check(self.lib.st_points_predict(self.h, int(mode), _dp(zz) if zz is not None else None, int(seed), int(it),
                                               _dp(out["w"]), _dp(out["mean"]), _dp(out["var"]),
                                               _dp(out["yhat"]) if out["yhat"] is not None else None))
        return out

    def _predict_points_joint(self, mode, z, seed, it):
        n = self.n_points
        out = {k: np.zeros(n) for k in ("w", "mean", "var")}
        out["yhat"] = np.zeros(n) if self.points_have_X else None
        zz = _f64(np.asarray(z).reshape(-1)) if z is not None else None
        if zz is not None and zz.size != n:
            raise ValueError("z must hold one normal per point")
        cov, chol = np.zeros(int(self.joint_offsets[-1])), np.zeros(int(self.joint_offsets[-1]))
        self._check(self.lib.st_points_predict_joint(self.h, int(mode), _dp(zz) if zz is not None else None, int(seed), int(it),
                                                     _dp(out["w"]), _dp(out["mean"]), _dp(cov), _dp(chol),
                                                     _dp(out["yhat"]) if out["yhat"] is not None else None))
        out["cov"], out["chol"] = self.unpack_joint(cov), self.unpack_joint(chol)
        out["cov_packed"], out["chol_packed"] = cov, chol
        for k, m in enumerate(self.joint_groups):
            out["var"][m] = np.maximum(cov[self.joint_offsets[k]:self.joint_offsets[k + 1]][::m.size + 1], 0.0)
        return out

    def accumulate_points(self, seed=0, it=0):
        """One saved iteration (st_points_accumulate): predict_points' draw with Philox streams 6 / 7 and counter ``it``, folded
        into the device summaries and, when set, the functionals.  Returns predict_points' dict."""
        n = self.n_points
        out = {k: np.zeros(n) for k in ("w", "mean", "var")}
        out["yhat"] = np.zeros(n) if self.points_have_X else None
        yp = _dp(out["yhat"]) if out["yhat"] is not None else None
        if getattr(self, "joint_groups", None) is None:
            self._check(self.lib.st_points_accumulate(self.h, int(seed), int(it), _dp(out["w"]), _dp(out["mean"]), _dp(out["var"]), yp))
            return out
        cov, chol = np.zeros(int(self.joint_offsets[-1])), np.zeros(int(self.joint_offsets[-1]))
        self._check(self.lib.st_points_accumulate_joint(self.h, int(seed), int(it), _dp(out["w"]), _dp(out["mean"]), _dp(cov), _dp(chol), yp))
        out["cov"], out["chol"] = self.unpack_joint(cov), self.unpack_joint(chol)
        out["cov_packed"], out["chol_packed"] = cov, chol
        for k, m in enumerate(self.joint_groups):
            out["var"][m] = np.maximum(cov[self.joint_offsets[k]:self.joint_offsets[k + 1]][::m.size + 1], 0.0)
        return out

    # ---- linear functionals of the predictions at the point set (st_points_functionals_*)
    def set_functionals(self, A):
        """Functionals F = sum a_i value_i of the point set's predictions (``functionals_csr`` has the accepted forms of ``A``;
        None or no row removes them).  Every accumulate_points then also forms them on the device."""
        ptr, idx, wt = functionals_csr(A, self.n_points) if A is not None else (np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0))
        self._check(self.lib.st_points_functionals_set(self.h, ptr.size - 1, _ip(ptr), _ip(idx), _dp(wt)))
        self.n_functionals = ptr.size - 1
        if getattr(self, "exceed_spec", None) is not None:   # the library drops the functional part of the thresholds
            self.exceed_spec = self.exceed_spec[:2] + (None,)

    def functionals_last(self):
        """F_w, F_m, F_v, F_y of the last accumulated iteration: dict(w, cond_mean, cond_var, yhat), yhat None without X."""
        nf = self.n_functionals
        out = {k: np.zeros(nf) for k in ("w", "cond_mean", "cond_var")}
        out["yhat"] = np.zeros(nf) if self.points_have_X else None
        self._check(self.lib.st_points_functionals_last(self.h, _dp(out["w"]), _dp(out["cond_mean"]), _dp(out["cond_var"]),
                                                        _dp(out["yhat"]) if out["yhat"] is not None else None))
        return out

    def functionals(self):
        """Summaries over the accumulated iterations: dict(mean, var, w_mean, yhat_mean, n) -- mean of F_m, mean of F_v +
        population variance of F_m, means of the draws."""
        nf = self.n_functionals
        out = {k: np.zeros(nf) for k in ("mean", "var", "w_mean")}
        out["yhat_mean"] = np.zeros(nf) if self.points_have_X else None
        cnt = C.c_int64()
        self._check(self.lib.st_points_functionals_get(self.h, _dp(out["mean"]), _dp(out["var"]), _dp(out["w_mean"]),
                                                       _dp(out["yhat_mean"]) if out["yhat_mean"] is not None else None, C.byref(cnt)))
        out["n"] = int(cnt.value)
        return out

    def functionals_quantile(self, q):
        """(w_q, yhat_q) of the stored functional draws (st_points_summary_reserve before the iterations); yhat_q None without X."""
        nf = self.n_functionals
        wq = np.zeros(nf)
        yq = np.zeros(nf) if self.points_have_X else None
        self._check(self.lib.st_points_functionals_quantile(self.h, float(q), _dp(wq), _dp(yq) if yq is not None else None))
        return wq, yq

    def functionals_info(self):
        """dict(n_fun, nnz, n_chunks, n_var_terms, alg_bytes) of the functionals' term lists."""
        v = [C.c_int64() for _ in range(4)]
        by = C.c_double()
        self._check(self.lib.st_points_functionals_info(self.h, *[C.byref(x) for x in v], C.byref(by)))
        return dict(n_fun=v[0].value, nnz=v[1].value, n_chunks=v[2].value, n_var_terms=v[3].value, alg_bytes=by.value)

    # ---- scores of held-out observations at the point set (st_points_score_*)
    def set_scores(self, y_new):
        """Held-out observations at the point set, one per point in the caller's order, NaN where a point is not scored
        (``score_values`` checks them); None removes the scores.  Every accumulate_points then also scores them on the device."""
        if y_new is None:
            self._check(self.lib.st_points_score_set(self.h, None))
            self.score_y = None
            return
        y = score_values(y_new, self.n_points, self.points_have_X)
        self._check(self.lib.st_points_score_set(self.h, _dp(y)))
        self.score_y = y

    def scores(self, crps=True, yhat_lo=None, yhat_hi=None):
        """The scores over the iterations accumulated since set_scores: dict(lpd, pit, crps, n_scored, n_degenerate), the arrays
        in the caller's order with NaN where a point is not scored; on a joint set also ``lpd_joint``, one per group of
        ``joint_groups``; ``crps`` (None with ``crps=False``) needs a stored draw (st_points_summary_reserve).  ``totals`` has
        ``score_totals``' means, with the coverage of [yhat_lo, yhat_hi] when both are given."""
        if self.score_y is None:
            raise ValueError("scores before set_scores")
        n = self.n_points
        out = dict(lpd=np.zeros(n), pit=np.zeros(n), crps=np.zeros(n) if crps else None)
        joint = getattr(self, "joint_groups", None) is not None
        out["lpd_joint"] = np.zeros(len(self.joint_groups)) if joint else None
        ns, nd = C.c_int64(), C.c_int64()
        self._check(self.lib.st_points_score_get(self.h, _dp(out["lpd"]), _dp(out["pit"]), _dp(out["crps"]) if crps else None,
                                                 _dp(out["lpd_joint"]) if joint else None, C.byref(ns), C.byref(nd)))
        out.update(n_scored=int(ns.value), n_degenerate=int(nd.value))
        out["totals"] = score_totals(out, self.score_y, self.points_mv, self.q, yhat_lo, yhat_hi)
        return out

    # ---- Rao-Blackwellised exceedance probabilities at the point set (st_points_exceed_*; spamtree_amd.exceed has the definition)
    def set_exceed(self, thresholds, side=1, thresholds_fun=None):
        """Thresholds of the exceedance probabilities P(w* > c) (side +1) or P(w* < c) (side -1) and, with X, of yhat*:
        ``thresholds`` a scalar or up to 8 entries, each a scalar or one value per outcome; ``side`` a scalar or one per threshold;
        ``thresholds_fun`` likewise with one value per functional (needs set_functionals).  None removes them.  Every
        accumulate_points then also folds each draw's exact conditional probability into a running mean and variance on the
        device: nothing per draw is stored."""
        if thresholds is None:
            self._check(self.lib.st_points_exceed_set(self.h, 0, None, None, None))
            self.exceed_spec = None
            return
        thr, sd, thr_fun = _rb.check_spec(dict(thresholds=thresholds, side=side, thresholds_fun=thresholds_fun), self.q,
                                          getattr(self, "n_functionals", 0))
        self._check(self.lib.st_points_exceed_set(self.h, thr.shape[0], _dp(thr), sd.ctypes.data_as(C.POINTER(C.c_int32)),
                                                  _dp(thr_fun) if thr_fun is not None else None))
        self.exceed_spec = (thr, sd, thr_fun)

    def exceed(self):
        """The exceedance probabilities over the iterations accumulated since set_exceed: dict(thr, side, w=dict(prob, prob_var),
        yhat=the same or None without X, n_accumulated), the arrays T x n_points in the caller's order; with ``thresholds_fun``
        also ``functionals=dict(thr, w=dict(prob, prob_var))``, T x n_functionals.  ``prob_var`` is the population variance of the
        per-draw probabilities: the MCSE of ``prob`` is sqrt(prob_var / ESS)."""
        if getattr(self, "exceed_spec", None) is None:
            raise ValueError("exceed before set_exceed")
        thr, sd, thr_fun = self.exceed_spec
        T, n = thr.shape[0], self.n_points

        def bufs(m):
            d = dict(prob=np.zeros((T, m)), prob_var=np.zeros((T, m)))
            return d, _lib.StRbOut(_dp(d["prob"]), _dp(d["prob_var"]))
        w, sw = bufs(n)
        y, sy = bufs(n) if self.points_have_X else (None, None)
        f, sf = bufs(self.n_functionals) if thr_fun is not None else (None, None)
        cnt = C.c_int64()
        self._check(self.lib.st_points_exceed_get(self.h, C.byref(sw), C.byref(sy) if sy is not None else None,
                                                  C.byref(sf) if sf is not None else None, C.byref(cnt)))
        out = dict(thr=thr.copy(), side=sd.copy(), w=w, yhat=y, n_accumulated=int(cnt.value))
        if f is not None:
            out["functionals"] = dict(thr=thr_fun.copy(), w=f)
        return out

    # ---- quantiles and the exact CRPS of the mixture predictive at the point set (st_points_mixture_*; spamtree_amd.mixture)
    def reserve_mixture(self, keep):
        """Room for the per-draw moments of the first ``keep`` saved draws (at most 8192; 0 releases it): every accumulate_points then
        also stores cond_mean, cond_var and, with X, x'beta + cond_mean and 1 / tausq_inv -- the components of the mixture predictive."""
        keep = int(keep)
        if keep < 0 or keep > _lib.ST_MIX_MAX_DRAWS:
            raise ValueError(f"reserve_mixture: keep = {keep} must lie in 0 .. {_lib.ST_MIX_MAX_DRAWS}")
        self._check(self.lib.st_points_mixture_reserve(self.h, keep))
        self.mixture_keep = keep

    def mixture_draws(self):
        """The stored components in the caller's order: dict(m, v, mu (None without X), tau2, n_stored), the arrays n_stored x n_points
        and tau2 n_stored x q."""
        cnt = C.c_int64()
        self._check(self.lib.st_points_mixture_draws(self.h, None, None, None, None, C.byref(cnt)))
        K, n = int(cnt.value), self.n_points
        out = dict(m=np.zeros((K, n)), v=np.zeros((K, n)), mu=np.zeros((K, n)) if self.points_have_X else None, tau2=np.zeros((K, self.q)))
        self._check(self.lib.st_points_mixture_draws(self.h, _dp(out["m"]), _dp(out["v"]), _dp(out["mu"]) if out["mu"] is not None else None,
                                                     _dp(out["tau2"]), C.byref(cnt)))
        out["n_stored"] = K
        return out

    def mixture_quantiles(self, probs, functionals=None):
        """Quantiles of the mixture predictive at up to 8 probabilities strictly inside (0, 1): dict(probs, w (T x n_points), yhat (the
        same, None without X), n_unconverged); with functionals set (``functionals`` None: when there are any) also
        ``functionals=dict(w (T x n_functionals), n_unconverged)``."""
        p = _mix.check_probs(probs)
        T, n = p.size, self.n_points
        nf = getattr(self, "n_functionals", 0)
        want_f = bool(nf) if functionals is None else bool(functionals)
        if want_f and not nf:
            raise ValueError("mixture_quantiles: functionals before set_functionals")

        def bufs(m):
            q, unc = np.zeros((T, m)), C.c_int64()
            return q, unc, _lib.StMixOut(_dp(q), C.pointer(unc))
        w, uw, sw = bufs(n)
        y, uy, sy = bufs(n) if self.points_have_X else (None, None, None)
        f, uf, sf = bufs(nf) if want_f else (None, None, None)
        self._check(self.lib.st_points_mixture_quantiles(self.h, T, _dp(p), C.byref(sw), C.byref(sy) if sy is not None else None,
                                                         C.byref(sf) if sf is not None else None))
        out = dict(probs=p.copy(), w=w, yhat=y, n_unconverged=int(uw.value) + (int(uy.value) if uy is not None else 0))
        if f is not None:
            out["functionals"] = dict(w=f, n_unconverged=int(uf.value))
        return out

    def mixture_info(self):
        """dict(keep, n_stored, store_bytes, n_solved, n_passes): the store's room, components and bytes on the device, and the
        quantiles solved by the last mixture_quantiles with the evaluations of the CDF they took together."""
        v = [C.c_int64() for _ in range(4)]
        by = C.c_double()
        self._check(self.lib.st_points_mixture_info(self.h, C.byref(v[0]), C.byref(v[1]), C.byref(by), C.byref(v[2]), C.byref(v[3])))
        return dict(keep=v[0].value, n_stored=v[1].value, store_bytes=by.value, n_solved=v[2].value, n_passes=v[3].value)

    def mixture_crps(self):
        """The exact CRPS of the mixture predictive of yhat at every scored point (set_scores) and its sharpness term:
        dict(crps, spread, n_scored), NaN where a point is not scored.  O(K^2) per scored point."""
        if getattr(self, "score_y", None) is None:
            raise ValueError("mixture_crps before set_scores")
        n = self.n_points
        out = dict(crps=np.zeros(n), spread=np.zeros(n))
        ns = C.c_int64()
        self._check(self.lib.st_points_mixture_crps(self.h, _dp(out["crps"]), _dp(out["spread"]), C.byref(ns)))
        out["n_scored"] = int(ns.value)
        return out

    # ---- convergence diagnostics of the stored draws (st_*_diagnostics; spamtree_amd.diagnostics has the definition)
    def _diagnostics(self, call, n, max_lag, yhat, n_kept, n_chains=1, chain_call=None):
        dw, sw = series_diag_buffers(n)
        dy, sy = series_diag_buffers(n, yhat)
        outs = (C.byref(sw), C.byref(sy) if sy is not None else None)
        if n_chains == 1:
            self._check(call(self.h, int(max_lag), *outs))
        else:   # the stored draws are n_chains chains laid end to end (st_*_chain_diagnostics)
            self._check(chain_call(self.h, int(n_chains), int(max_lag), *outs))
        if n_kept is not None:   # the number of stored draws per chain tells which series ran into the lag cap
            series_diag_finish(dw, n_kept // n_chains, max_lag)
            series_diag_finish(dy, n_kept // n_chains, max_lag)
        return dict(w=dw, yhat=dy)

    def summary_diagnostics(self, max_lag=0, n_kept=None, n_chains=1):
        """ESS, MCSE, sd, split-R-hat and lags of every row's stored w and yhat draws (st_summary_reserve before the saved
        iterations): dict(w=dict(ess, mcse, sd, rhat, lags), yhat=the same), n_all values each in model row order.  With
        ``n_kept``, the number of stored draws, each also holds ``truncated``: the series that ran into the lag cap.  With
        ``n_chains`` > 1 the stored draws are that many chains laid end to end: the ESS of the combined chains and the R-hat over
        all half chains (st_summary_chain_diagnostics)."""
        return self._diagnostics(self.lib.st_summary_diagnostics, self.n_all, max_lag, True, n_kept, n_chains,
                                 self.lib.st_summary_chain_diagnostics)

    def points_diagnostics(self, max_lag=0, n_kept=None, n_chains=1):
        """The same of the point set's stored w* and yhat* draws (st_points_summary_reserve), in the caller's order; ``yhat``
        None without X."""
        return self._diagnostics(self.lib.st_points_summary_diagnostics, self.n_points, max_lag, self.points_have_X, n_kept, n_chains,
                                 self.lib.st_points_summary_chain_diagnostics)

    def functionals_diagnostics(self, max_lag=0, n_kept=None, n_chains=1):
        """The same of the functionals' stored F_w and F_y draws; ``yhat`` None without X."""
        return self._diagnostics(self.lib.st_points_functionals_diagnostics, self.n_functionals, max_lag, self.points_have_X, n_kept,
                                 n_chains, self.lib.st_points_functionals_chain_diagnostics)

    # ---- rank-normalised R-hat, bulk / tail / quantile / exceedance ESS of the stored draws (st_*_rank_diagnostics)
    def _rank_diagnostics(self, call, n, m, probs, thresholds, sides, max_lag, yhat, n_kept, n_chains=1, chain_call=None):
        spec, keep, n_prob, n_thr = rank_spec(probs, thresholds, sides, max_lag, m)
        dw, ow = rank_buffers(n, n_prob, n_thr)
        dy, oy = rank_buffers(n, n_prob, n_thr, yhat)
        outs = (C.byref(spec), C.byref(ow), C.byref(oy) if oy is not None else None)
        if n_chains == 1:
            self._check(call(self.h, *outs))
        else:   # the stored draws are n_chains chains laid end to end (st_*_chain_rank_diagnostics)
            self._check(chain_call(self.h, int(n_chains), *outs))
        del keep
        if n_kept is not None:
            rank_finish(dw, n_kept // n_chains, max_lag)
            rank_finish(dy, n_kept // n_chains, max_lag)
        return dict(w=dw, yhat=dy)

    def summary_rank_diagnostics(self, probs=(), thresholds=(), sides=None, max_lag=0, n_kept=None, n_chains=1):
        """Rank-normalised R-hat (bulk, folded, their maximum), bulk and tail ESS, the ESS of the quantiles ``probs`` and of the
        exceedances of ``thresholds`` (a scalar or q values each, ``sides`` +1 / -1) with their probability and its MCSE, of every
        row's stored w and yhat draws (st_summary_reserve before the saved iterations): dict(w=dict(rhat_rank, rhat_bulk,
        rhat_fold, ess_bulk, ess_tail, lags_bulk (n_all), ess_q (n_prob, n_all), ess_exc, mcse_prob, prob (n_thr, n_all)),
        yhat=the same), model row order.  With ``n_kept`` each also holds ``truncated``.  With ``n_chains`` > 1 the stored draws
        are that many chains laid end to end (st_summary_chain_rank_diagnostics)."""
        return self._rank_diagnostics(self.lib.st_summary_rank_diagnostics, self.n_all, self.q, probs, thresholds, sides, max_lag,
                                      True, n_kept, n_chains, self.lib.st_summary_chain_rank_diagnostics)

    def points_rank_diagnostics(self, probs=(), thresholds=(), sides=None, max_lag=0, n_kept=None, n_chains=1):
        """The same of the point set's stored w* and yhat* draws, in the caller's order; ``yhat`` None without X."""
        return self._rank_diagnostics(self.lib.st_points_summary_rank_diagnostics, self.n_points, self.q, probs, thresholds, sides,
                                      max_lag, self.points_have_X, n_kept, n_chains, self.lib.st_points_summary_chain_rank_diagnostics)

    def functionals_rank_diagnostics(self, probs=(), thresholds=(), sides=None, max_lag=0, n_kept=None, n_chains=1):
        """The same of the functionals' stored F_w and F_y draws: a threshold value per functional (a scalar entry serves all);
        ``yhat`` None without X."""
        return self._rank_diagnostics(self.lib.st_points_functionals_rank_diagnostics, self.n_functionals, self.n_functionals,
                                      probs, thresholds, sides, max_lag, self.points_have_X, n_kept, n_chains,
                                      self.lib.st_points_functionals_chain_rank_diagnostics)

    # ---- exceedance, excursion functions and simultaneous bands of the stored draws (st_*_excursions; spamtree_amd.excursions)
    def _excursions(self, call, n, m, G, n_kept, thresholds, side, mask, band, yhat):
        thr = sd = None
        if thresholds is not None:
            thr, sd = _exc.expand_thresholds(thresholds, m, side)
        elif not band:
            raise ValueError("excursions: neither thresholds nor band")
        mk = _exc.check_mask(mask, n)
        _exc.check_keep(n_kept, band)
        spec, keep = excursion_spec(thr, sd, mk, band)
        T = 0 if thr is None else thr.shape[0]
        dw, ow = excursion_buffers(n, T, G, int(n_kept), band)
        dy, oy = excursion_buffers(n, T, G, int(n_kept), band, yhat)
        self._check(call(self.h, C.byref(spec), C.byref(ow), C.byref(oy) if oy is not None else None))
        del keep
        return dict(w=excursion_finish(dw), yhat=excursion_finish(dy))

    def summary_excursions(self, n_kept, thresholds=None, side=1, mask=None, band=False):
        """Exceedance counts and probabilities, the excursion function and, with ``band``, the mean, sd and per-draw largest
        standardised deviation of every row's stored w and yhat draws (st_summary_reserve before the saved iterations; ``n_kept``
        of them are stored).  ``thresholds``: ``excursions.expand_thresholds`` over the q outcomes; ``mask``: n_all entries in
        model row order, 0 = in no domain.  dict(w=dict(count, prob, excur (T, n_all), joint_all (T, q), mean, sd (n_all),
        maxdev (q, K), n_flat (q), n_draws), yhat=the same), model row order."""
        return self._excursions(self.lib.st_summary_excursions, self.n_all, self.q, self.q, n_kept, thresholds, side, mask, band, True)

    def points_excursions(self, n_kept, thresholds=None, side=1, mask=None, band=False):
        """The same of the point set's stored w* and yhat* draws (st_points_summary_reserve), caller order; ``yhat`` None without X."""
        return self._excursions(self.lib.st_points_summary_excursions, self.n_points, self.q, self.q, n_kept, thresholds, side, mask,
                                band, self.points_have_X)

    def functionals_excursions(self, n_kept, thresholds=None, side=1, mask=None, band=False):
        """The same of the functionals' stored F_w and F_y draws: one domain, a threshold value per functional (a scalar entry
        serves all); ``yhat`` None without X."""
        return self._excursions(self.lib.st_points_functionals_excursions, self.n_functionals, self.n_functionals, 1, n_kept, thresholds,
                                side, mask, band, self.points_have_X)

    # ---- criteria over the fit's own rows (st_rows_score_*): conditional on w
    def rows_score_set(self, y_holdout=None, y=None):
        """Starts the criteria over the model's rows: WAIC / DIC over the observed rows and, with ``y_holdout`` (one value per
        row in model row order, NaN = none, finite only at NA rows), the scores of those held-out values.  ``y``: the model's y,
        to check ``y_holdout`` against before the device call (``rows_holdout``); without it the library checks."""
        t = rows_holdout(y_holdout, y) if (y is not None and y_holdout is not None) else (None if y_holdout is None else _f64(y_holdout))
        if t is not None and t.shape != (self.n_all,):
            raise ValueError(f"y_holdout must hold one value per row ({self.n_all})")
        self._check(self.lib.st_rows_score_set(self.h, _dp(t) if t is not None else None))

    def rows_score_clear(self):
        self._check(self.lib.st_rows_score_clear(self.h))

    def rows_score_accumulate(self):
        """One draw from the current w, XB and tausq_inv into the criteria's state; nothing comes to the host."""
        self._check(self.lib.st_rows_score_accumulate(self.h))

    def rows_score_get(self, crps=False):
        """dict(lppd, p_waic, mean_ll, mu_mean, pit, crps, n_accumulated): n_all values each in model row order, NaN where a row
        has no target (pit, crps: off the held-out rows); ``crps`` needs draws stored by st_summary_reserve / st_summary_accumulate."""
        out = {k: np.zeros(self.n_all) for k in ("lppd", "p_waic", "mean_ll", "mu_mean", "pit")}
        out["crps"] = np.zeros(self.n_all) if crps else None
        cnt = C.c_int64()
        self._check(self.lib.st_rows_score_get(self.h, _dp(out["lppd"]), _dp(out["p_waic"]), _dp(out["mean_ll"]), _dp(out["mu_mean"]),
                                               _dp(out["pit"]), _dp(out["crps"]) if crps else None, C.byref(cnt)))
        out["n_accumulated"] = int(cnt.value)
        return out

    def rows_score_totals(self, raw=False, have_crps=None):
        """``rows_criteria`` of st_rows_score_totals' tables; ``raw``: (obs, held, n_obs, n_held) as the library returned them.
        ``have_crps``: whether yhat draws are stored (st_summary_reserve / st_summary_accumulate), so that the held-out ``crps``
        is a figure and not None; by default asked of the library (st_rows_score_get refuses ``crps`` without a stored draw)."""
        obs = np.zeros((len(_lib.ST_ROWS_OBS), self.q), order="F")
        held = np.zeros((len(_lib.ST_ROWS_HELD), self.q), order="F")
        n_obs, n_held = np.zeros(self.q, dtype=np.int64), np.zeros(self.q, dtype=np.int64)
        self._check(self.lib.st_rows_score_totals(self.h, _dp(obs), _dp(held), _ip(n_obs), _ip(n_held)))
        if raw:
            return obs, held, n_obs, n_held
        if have_crps is None:
            have_crps = self.lib.st_rows_score_get(self.h, None, None, None, None, None, _dp(np.zeros(self.n_all)), None) == 0
        return rows_criteria(obs, held, n_obs, n_held, have_crps=bool(have_crps))

    def rows_score_info(self):
        by = C.c_double()
        self._check(self.lib.st_rows_score_info(self.h, C.byref(by)))
        return dict(alg_bytes=float(by.value))

    # ---- leave-one-out criteria with each row's own w_i integrated out (st_rows_loo_*)
    def rows_loo_set(self):
        self._check(self.lib.st_rows_loo_set(self.h))

    def rows_loo_clear(self):
        self._check(self.lib.st_rows_loo_clear(self.h))

    def rows_loo_accumulate(self):
        """One draw from the current w, XB, tausq_inv and slot 0 into the state; nothing comes to the host."""
        self._check(self.lib.st_rows_loo_accumulate(self.h))

    def rows_loo_last(self):
        """dict(q_diag, qw, cond_mean, cond_var) of the last accumulate: n_all values each, NaN at the rows of prediction blocks."""
        out = {k: np.zeros(self.n_all) for k in ("q_diag", "qw", "cond_mean", "cond_var")}
        self._check(self.lib.st_rows_loo_last(self.h, _dp(out["q_diag"]), _dp(out["qw"]), _dp(out["cond_mean"]), _dp(out["cond_var"])))
        return out

    def rows_loo_get(self):
        """dict(elpd_loo, pit_loo, mu_loo, weight_ess, n_accumulated, n_skipped): n_all values each, NaN off the observed rows."""
        out = {k: np.zeros(self.n_all) for k in ("elpd_loo", "pit_loo", "mu_loo", "weight_ess")}
        cnt, skip = C.c_int64(), C.c_int64()
        self._check(self.lib.st_rows_loo_get(self.h, _dp(out["elpd_loo"]), _dp(out["pit_loo"]), _dp(out["mu_loo"]), _dp(out["weight_ess"]),
                                             C.byref(cnt), C.byref(skip)))
        out["n_accumulated"], out["n_skipped"] = int(cnt.value), int(skip.value)
        return out

    def rows_loo_totals(self, raw=False):
        """``rows_loo_criteria`` of st_rows_loo_totals' table; ``raw``: (tot, n_obs) as the library returned them."""
        tot = np.zeros((len(_lib.ST_ROWS_LOO), self.q), order="F")
        n_obs = np.zeros(self.q, dtype=np.int64)
        self._check(self.lib.st_rows_loo_totals(self.h, _dp(tot), _ip(n_obs)))
        return (tot, n_obs) if raw else rows_loo_criteria(tot, n_obs)

    def rows_loo_info(self):
        """dict(routes=[kernel names of one accumulate], alg_bytes, flops), from shapes."""
        r = C.c_int32()
        by, fl = C.c_double(), C.c_double()
        self._check(self.lib.st_rows_loo_info(self.h, C.byref(r), C.byref(by), C.byref(fl)))
        routes = []
        code = 1
        while self.lib.st_rows_loo_route_name(code) is not None:
            if r.value & (1 << (code - 1)):
                routes.append(self.lib.st_rows_loo_route_name(code).decode())
            code += 1
        return dict(routes=routes, alg_bytes=float(by.value), flops=float(fl.value))

    # ---- leave-group-out criteria: a group's rows integrated out jointly (st_rows_loo_groups_*; ``spamtree_amd.loo``)
    def rows_loo_groups_set(self, labels):
        """One int64 label per model row, negative = in no group (``loo.site_groups``, ``loo.block_groups``); after rows_loo_set,
        before the first accumulate."""
        labels = np.ascontiguousarray(labels, dtype=np.int64)
        if labels.shape != (self.n_all,):
            raise ValueError(f"labels must hold one value per row ({self.n_all}), got shape {labels.shape}")
        self._check(self.lib.st_rows_loo_groups_set(self.h, _ip(labels)))

    def rows_loo_groups_clear(self):
        self._check(self.lib.st_rows_loo_groups_clear(self.h))

    def rows_loo_groups_index(self):
        """dict(label, ptr, rows, n_groups, n_members, n_pairs, n_matrix): group g has the model rows rows[ptr[g]:ptr[g + 1]]."""
        c = [C.c_int64() for _ in range(4)]
        self._check(self.lib.st_rows_loo_groups_count(self.h, *[C.byref(v) for v in c]))
        ng, nm, npair, nsq = (int(v.value) for v in c)
        label, ptr, rows = np.zeros(ng, dtype=np.int64), np.zeros(ng + 1, dtype=np.int64), np.zeros(nm, dtype=np.int64)
        self._check(self.lib.st_rows_loo_groups_index(self.h, _ip(label), _ip(ptr), _ip(rows)))
        return dict(label=label, ptr=ptr, rows=rows, n_groups=ng, n_members=nm, n_pairs=npair, n_matrix=nsq)

    def rows_loo_groups_last(self):
        """Per group of the last accumulate, lists of arrays: q_gg and cond_cov (g x g), qw and cond_mean (g)."""
        ix = self.rows_loo_groups_index()
        qg, cv = np.zeros(ix["n_matrix"]), np.zeros(ix["n_matrix"])
        c, m = np.zeros(ix["n_members"]), np.zeros(ix["n_members"])
        self._check(self.lib.st_rows_loo_groups_last(self.h, _dp(qg), _dp(c), _dp(m), _dp(cv)))
        out = dict(q_gg=[], qw=[], cond_mean=[], cond_cov=[])
        at = 0
        for g in range(ix["n_groups"]):
            a, b = int(ix["ptr"][g]), int(ix["ptr"][g + 1])
            k = b - a
            out["q_gg"].append(qg[at:at + k * k].reshape(k, k)); out["cond_cov"].append(cv[at:at + k * k].reshape(k, k))
            out["qw"].append(c[a:b]); out["cond_mean"].append(m[a:b])
            at += k * k
        return out

    def rows_loo_groups_get(self):
        """dict(elpd_lgo, weight_ess, n_skipped per group; mu_lgo, pit_lgo per row, NaN off the observed members; n_accumulated)."""
        ng = self.rows_loo_groups_index()["n_groups"]
        out = dict(elpd_lgo=np.zeros(ng), weight_ess=np.zeros(ng), n_skipped=np.zeros(ng, dtype=np.int64), mu_lgo=np.zeros(self.n_all),
                   pit_lgo=np.zeros(self.n_all))
        cnt = C.c_int64()
        self._check(self.lib.st_rows_loo_groups_get(self.h, _dp(out["elpd_lgo"]), _dp(out["weight_ess"]), _ip(out["n_skipped"]),
                                                    _dp(out["mu_lgo"]), _dp(out["pit_lgo"]), C.byref(cnt)))
        out["n_accumulated"] = int(cnt.value)
        return out

    def rows_loo_groups_totals(self):
        """dict(elpd_lgo, lgoic, se, min_weight_ess, n_groups, by_outcome=dict(sqerr, pit, count: q values each))."""
        tot = np.zeros(len(_lib.ST_ROWS_LGO))
        by = np.zeros((len(_lib.ST_ROWS_LGO_OUT), self.q), order="F")
        self._check(self.lib.st_rows_loo_groups_totals(self.h, _dp(tot), _dp(by)))
        out = {k: float(tot[i]) for i, k in enumerate(_lib.ST_ROWS_LGO)}
        out["n_groups"] = int(out["n_groups"])
        out["by_outcome"] = {k: by[i].copy() for i, k in enumerate(_lib.ST_ROWS_LGO_OUT)}
        return out

    def rows_loo_groups_draws(self):
        """The stored group log ratios t = -l, [n_accumulated][n_groups] (needs rows_loo_reserve)."""
        ng = self.rows_loo_groups_index()["n_groups"]
        cnt = C.c_int64()
        self._check(self.lib.st_rows_loo_groups_get(self.h, None, None, None, None, None, C.byref(cnt)))
        out = np.zeros((int(cnt.value), ng))
        self._check(self.lib.st_rows_loo_groups_draws(self.h, _dp(out)))
        return out

    def rows_loo_groups_psis(self):
        """dict(khat, elpd_psis, weight_ess_psis, tail_len, n_draws) per group: the Pareto smoothing of the stored group ratios."""
        ng = self.rows_loo_groups_index()["n_groups"]
        out = dict(khat=np.zeros(ng), elpd_psis=np.zeros(ng), weight_ess_psis=np.zeros(ng), tail_len=np.zeros(ng, dtype=np.int32),
                   n_draws=np.zeros(ng, dtype=np.int32))
        i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))   # noqa: E731
        self._check(self.lib.st_rows_loo_groups_psis(self.h, _dp(out["khat"]), _dp(out["elpd_psis"]), _dp(out["weight_ess_psis"]),
                                                     i32(out["tail_len"]), i32(out["n_draws"])))
        return out

    # ---- Pareto smoothing of the leave-one-out weights (st_rows_loo_reserve / _draws / _psis*, st_psis; ``spamtree_amd.psis``)
    def rows_loo_reserve(self, keep):
        """Room for ``keep`` accumulated draws' (t, Phi, mu) on the device; after rows_loo_set, before the first accumulate.  0 frees."""
        self._check(self.lib.st_rows_loo_reserve(self.h, int(keep)))

    def rows_loo_draws(self, n_accumulated):
        """dict(t, phi, mu): the stored columns, [n_accumulated][n_all] each in model row order (NaN: skipped, or no observed y)."""
        out = {k: np.zeros((int(n_accumulated), self.n_all)) for k in ("t", "phi", "mu")}
        self._check(self.lib.st_rows_loo_draws(self.h, _dp(out["t"]), _dp(out["phi"]), _dp(out["mu"])))
        return out

    @staticmethod
    def _psis_out(n, pit=True, mu=True):
        out = {k: np.zeros(n) for k in ("khat", "elpd_psis", "weight_ess_psis")}
        if pit:
            out["pit_psis"] = np.zeros(n)
        if mu:
            out["mu_psis"] = np.zeros(n)
        out["tail_len"], out["n_draws"] = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        st = _lib.StPsisOut(_dp(out["khat"]), _dp(out["elpd_psis"]), _dp(out["pit_psis"]) if pit else None,
                            _dp(out["mu_psis"]) if mu else None, _dp(out["weight_ess_psis"]), i32(out["tail_len"]), i32(out["n_draws"]))
        return out, st

    def rows_loo_psis(self):
        """dict(khat, elpd_psis, pit_psis, mu_psis, weight_ess_psis, tail_len, n_draws): n_all values each, NaN / 0 off the observed rows."""
        out, st = self._psis_out(self.n_all)
        self._check(self.lib.st_rows_loo_psis(self.h, C.byref(st)))
        return out

    def rows_loo_psis_totals(self, raw=False):
        """``rows_psis_criteria`` of st_rows_loo_psis_totals' table; ``raw``: (tot, n_obs) as the library returned them."""
        tot = np.zeros((len(_lib.ST_ROWS_PSIS), self.q), order="F")
        n_obs = np.zeros(self.q, dtype=np.int64)
        self._check(self.lib.st_rows_loo_psis_totals(self.h, _dp(tot), _ip(n_obs)))
        return (tot, n_obs) if raw else rows_psis_criteria(tot, n_obs)

    def psis(self, t, phi=None, mu=None):
        """st_psis on host arrays [K][n] (float64): the kernel of rows_loo_psis on the caller's log ratios and companions."""
        t = np.ascontiguousarray(t, dtype=np.float64)
        K, n = t.shape
        phi = None if phi is None else np.ascontiguousarray(phi, dtype=np.float64)
        mu = None if mu is None else np.ascontiguousarray(mu, dtype=np.float64)
        out, st = self._psis_out(n, phi is not None, mu is not None)
        self._check(self.lib.st_psis(self.h, n, K, _dp(t), None if phi is None else _dp(phi), None if mu is None else _dp(mu), C.byref(st)))
        return out

    def psis_info(self, n, K, n_comp=2):
        """dict(R, Kpad, lds_bytes, alg_bytes) of a pass of k_loo_psis over an n x K store, from shapes."""
        r, kp, lb, by = C.c_int32(), C.c_int32(), C.c_int64(), C.c_double()
        self._check(self.lib.st_psis_info(self.h, int(n), int(K), int(n_comp), C.byref(r), C.byref(kp), C.byref(lb), C.byref(by)))
        return dict(R=int(r.value), Kpad=int(kp.value), lds_bytes=int(lb.value), alg_bytes=float(by.value))

    def points_info(self):
        """Of the last predict_points: dict(routes=[kernel names that ran], n_groups, alg_bytes, flops)."""
        r = C.c_int32()
        ng = C.c_int64()
        by, fl = C.c_double(), C.c_double()
        self._check(self.lib.st_points_info(self.h, C.byref(r), C.byref(ng), C.byref(by), C.byref(fl)))
        routes = []
        code = 1
        while self.lib.st_points_route_name(code) is not None:
            if r.value & (1 << (code - 1)):
                routes.append(self.lib.st_points_route_name(code).decode())
            code += 1
        return dict(routes=routes, n_groups=int(ng.value), alg_bytes=float(by.value), flops=float(fl.value))
