"""Prediction at new locations from a saved chain, without refitting.

The model defines the predictive of a location that is not a row of the problem through the way it treats NA rows:
``make_tree`` sends an NA row to the block of its nearest row on the deepest knot level (same margin when
``cherrypick_same_margin`` is set, ties to the lowest row), and ``predict_std`` draws it from its conditional given the
reference ancestors on that path.  :func:`locate` is that first step for arbitrary points; :func:`predict_new` replays a
saved chain draw by draw through ``st_points_predict`` (include/spamtree_hip.h); :func:`fit_predict` predicts during the
fit instead, on every saved iteration, with the summaries kept on the device (``st_points_accumulate``).

Points can be predicted jointly: ``joint`` labels put up to 16 points that share a conditioning chain into one joint group
(:func:`group_sites` labels the outcomes of a site), which is drawn from its g-variate conditional and reported with its
g x g predictive covariance (``st_points_set_joint``).
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import exceed as _rb
from . import mixture as _mix
from . import excursions as _exc
from . import fit
from .model import SpamTreeMV, _dp, _f64, functionals_csr, joint_labels, score_values
from .topology import Topology, _nearest_rows

__all__ = ["locate", "conditioning_set", "group_sites", "predict_new", "fit_predict", "areal_means", "contrasts"]


def areal_means(labels, weights=None):
    """One averaging functional per region: ``labels`` holds one integer per point, a negative label means no region; the
    functionals come in ascending label order.  ``weights`` (one positive number per point, e.g. cell areas) are normalised to
    sum to 1 inside each region; None: equal weights.  Returns CSR ``(ptr, idx, wt)`` for ``functionals=``."""
    labels = np.asarray(labels)
    if labels.ndim != 1 or (labels.size and not np.issubdtype(labels.dtype, np.integer)):
        raise ValueError("areal_means: labels must hold one integer per point")
    w = np.ones(labels.size) if weights is None else np.asarray(weights, dtype=np.float64)
    if w.shape != labels.shape or not np.all(np.isfinite(w)) or np.any(w <= 0):
        raise ValueError("areal_means: weights must hold one positive finite number per point")
    idx = np.nonzero(labels >= 0)[0]
    idx = idx[np.argsort(labels[idx], kind="stable")].astype(np.int64)         # by region, the caller's order inside it
    regions, counts = np.unique(labels[idx], return_counts=True)
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    wt = w[idx].copy()
    for k in range(regions.size):
        wt[ptr[k]:ptr[k + 1]] /= wt[ptr[k]:ptr[k + 1]].sum()
    return ptr, idx, wt


def contrasts(pairs):
    """The functionals value_i - value_j for every ``(i, j)`` of ``pairs`` (k x 2 point indices, i != j): CSR ``(ptr, idx, wt)``."""
    pairs = np.asarray(pairs)
    if pairs.size == 0:
        return np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0)
    if pairs.ndim != 2 or pairs.shape[1] != 2 or not np.issubdtype(pairs.dtype, np.integer):
        raise ValueError("contrasts: pairs must be k x 2 integer point indices")
    if np.any(pairs[:, 0] == pairs[:, 1]) or pairs.min() < 0:
        raise ValueError("contrasts: a pair needs two different points, indices from 0")
    k = pairs.shape[0]
    return 2 * np.arange(k + 1, dtype=np.int64), pairs.astype(np.int64).reshape(-1), np.tile([1.0, -1.0], k)


def group_sites(coords) -> np.ndarray:
    """Joint-group labels that put the points with identical coordinates (the outcomes at one site) into one group:
    0, 1, ... by first appearance in the caller's order."""
    coords = np.asarray(coords, dtype=np.float64).reshape(-1, 2)
    if coords.shape[0] == 0:
        return np.zeros(0, dtype=np.int64)
    _, first, inv = np.unique(coords, axis=0, return_index=True, return_inverse=True)
    rank = np.empty(first.size, dtype=np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(first.size)
    return rank[np.asarray(inv).reshape(-1)]


def locate(topo: Topology, coords_new, mv_new, device: Optional[int] = None, joint=None) -> np.ndarray:
    """0-based anchor block of every new point, in the caller's order: the block of the nearest row on the deepest knot
    level -- the rule ``make_tree`` applies to missing rows, through the same nearest-row search (``device``: on the GPU).
    ``joint``: one label per point; every member of a joint group gets the anchor of the group's first member, so that
    the group shares one conditioning chain (as ``cherrypick_group_locations`` keeps same-location rows in one block)."""
    if topo.knot_level is None:
        raise ValueError("this topology does not record its deepest knot level (build it with topology.prepare)")
    coords_new = np.asarray(coords_new, dtype=np.float64).reshape(-1, 2)
    mv_new = np.asarray(mv_new, dtype=np.int64).reshape(-1)
    if mv_new.size != coords_new.shape[0]:
        raise ValueError("coords_new and mv_new must describe the same points")
    labels = None if joint is None else joint_labels(joint, coords_new.shape[0])
    if coords_new.shape[0] == 0:
        return np.zeros(0, dtype=np.int64)
    res_row = topo.block_groups[topo.blocking - 1]
    targets = np.nonzero(res_row == topo.knot_level)[0]           # ascending row ids, as make_tree orders its knots
    n_marg = int(topo.mv_id.max())
    nn = _nearest_rows(topo.coords[targets], topo.mv_id[targets] - 1, coords_new, mv_new - 1, n_marg,
                       topo.cherrypick_same_margin, device)
    anchor = (topo.blocking[targets[nn]] - 1).astype(np.int64)
    if labels is not None:
        _, first, inv = np.unique(labels, return_index=True, return_inverse=True)
        anchor = anchor[first[np.asarray(inv).reshape(-1)]]
    return anchor


def conditioning_set(topo: Topology, anchor: int) -> np.ndarray:
    """Blocks a point anchored at ``anchor`` conditions on: parents(anchor), plus the anchor itself when it is a reference
    block -- the ancestors of the missing block ``make_tree`` would hang under it."""
    levels = np.unique(topo.block_groups)
    rank = int(np.searchsorted(levels, topo.block_groups[anchor]))
    par = topo.parents(int(anchor))
    return np.concatenate([par, [int(anchor)]]).astype(np.int64) if topo.res_is_ref[rank] else par.astype(np.int64)


def predict_new(model_inputs, draws, coords_new, mv_new, X_new=None, seed=2021, return_draws=True, device=0, z=None,
                mode=0, force_generic=False, return_moments=False, joint=None, functionals=None, y_new=None, quantiles=(),
                crps=True, diagnostics=False, diagnostics_max_lag=0, excursions=None, rank_diagnostics=None, exceed=None, mixture=None):
    """Predictive at new locations for every saved draw of a chain.

    ``model_inputs``: the problem as ``spamtree_mv_mcmc`` took it (the dict of ``synthetic.make_workload``; its ``topo``
    locates the points).  ``draws``: the dict ``fit.spamtree_mv_mcmc`` returns (``w_mcmc``, ``beta_mcmc``, ``tausq_mcmc``,
    ``theta_mcmc``).  For saved draw s: st_set_w, st_set_beta, st_set_tausq_inv, st_factor(0, theta_s), st_points_predict
    with iteration counter s (``z``: n_new x keep caller normals instead of Philox stream 6).

    Returns dict(mean, var) -- the Rao-Blackwellised predictive mean (mean of the conditional means) and variance (mean of
    the conditional variances + variance of the conditional means) of w -- and, with ``return_draws``, ``w`` and ``yhat``
    (n_new x keep; yhat only with ``X_new``); with ``return_moments`` also the per-draw ``cond_mean`` and ``cond_var``
    (n_new x keep).  Everything in the caller's order of the points.

    ``joint``: one label per point (see :func:`group_sites`); the groups are located together and drawn jointly.  Then the
    result also holds ``groups`` (the member indices of every group), ``cov`` -- per group the Rao-Blackwellised predictive
    covariance, mean of the conditional covariances + covariance of the conditional means -- and, with ``return_draws``,
    ``cond_cov``: per saved draw the conditional covariances (``SpamTreeMV.unpack_joint``'s list or array).

    ``functionals``: linear functionals of the predictions (``model.functionals_csr``'s forms, :func:`areal_means`,
    :func:`contrasts`).  The replay then goes through ``st_points_accumulate`` -- the same draw as ``st_points_predict`` with
    that seed and counter, so every other output is unchanged bit for bit -- which needs the device's normals (``z`` None) and
    ``mode`` 0.  The result also holds ``functionals``: dict(mean, var, w_mean, yhat_mean) and, with ``return_draws``, the
    n_fun x keep arrays ``w``, ``cond_mean``, ``cond_var``, ``yhat``.

    ``y_new``: held-out observations at the points (one per point, NaN = not scored; needs ``X_new``), scored on the device.
    As with ``functionals`` the replay goes through ``st_points_accumulate`` (``z`` None, ``mode`` 0), with every saved draw's
    yhat kept on the device for the CRPS.  The result also holds ``scores`` (``SpamTreeMV.scores``); ``quantiles=(lo, ..., hi)``
    adds the coverage of [yhat_lo, yhat_hi] to its totals.  ``crps=False`` leaves the CRPS out and keeps no draw on the device
    (neither then has ``quantiles``); with it the chain may hold at most 16384 saved draws.

    ``diagnostics``: ESS, MCSE, sd and split-R-hat of every point's w* and yhat* draws (``spamtree_amd.diagnostics``), formed on
    the device after the last draw from the draws it keeps (``z`` None, ``mode`` 0; 4 .. 16384 saved draws).  The result then
    holds ``diagnostics``: dict(w, yhat) and, with ``functionals``, ``functionals["diagnostics"]``.

    ``excursions=dict(thresholds=, side=, mask=, band=)``: exceedance probabilities, excursion function and band ingredients of
    the points' w* and yhat* draws (``spamtree_amd.excursions``; ``mask`` has one entry per point), formed on the device after the
    last draw from the draws it keeps (``z`` None, ``mode`` 0; 1 .. 16384 saved draws).  The result then holds ``excursions``:
    dict(w, yhat) and, with ``functionals``, ``functionals["excursions"]`` (``thresholds_fun``, ``mask_fun`` as in
    ``fit.spamtree_mv_mcmc``).

    ``rank_diagnostics=True | dict(probs=, thresholds=, sides=, max_lag=, thresholds_fun=)``: rank-normalised R-hat, bulk, tail,
    quantile and exceedance ESS of the points' w* and yhat* draws (``spamtree_amd.diagnostics``), formed on the device after the
    last draw from the draws it keeps (``z`` None, ``mode`` 0; 4 .. 16384 saved draws).  The result then holds
    ``rank_diagnostics``: dict(w, yhat) and, with ``functionals``, ``functionals["rank_diagnostics"]``.

    ``exceed=dict(thresholds=, side=, thresholds_fun=)``: Rao-Blackwellised exceedance probabilities (``spamtree_amd.exceed``), the
    mean over the saved draws of each draw's exact conditional probability, formed on the device as the replay goes through
    ``st_points_accumulate`` (``z`` None, ``mode`` 0); no draw is kept for it.  The result then holds ``exceed``: dict(thr, side,
    w=dict(prob, prob_var), yhat=the same or None, n_accumulated) and, with ``thresholds_fun``, ``functionals["exceed"]``.
    ``mixture=dict(probs=, crps=True)``: quantiles and the exact CRPS of the mixture predictive (``spamtree_amd.mixture``) from the
    per-draw moments the replay stores on the device as it goes through ``st_points_accumulate`` (``z`` None, ``mode`` 0; at most
    8192 saved draws).  The result then holds ``mixture``: dict(probs, w, yhat or None, n_stored, n_unconverged), with functionals
    ``functionals["mixture"]``, and with ``y_new`` and ``crps=True`` ``scores["crps_mixture"]`` and ``scores["spread"]``.
    """
    mi = model_inputs
    topo = mi["topo"]
    coords_new = np.asarray(coords_new, dtype=np.float64).reshape(-1, 2)
    mv_new = np.asarray(mv_new, dtype=np.int64).reshape(-1)
    n_new = coords_new.shape[0]
    fun = None
    if functionals is not None:
        fun = functionals_csr(functionals, n_new)
        if z is not None or mode != 0:
            raise ValueError("functionals need the device draw: z=None and mode=0")
    ys = None
    if y_new is not None:
        ys = score_values(y_new, n_new, X_new is not None)
        if z is not None or mode != 0:
            raise ValueError("y_new needs the device draw: z=None and mode=0")
    if diagnostics:
        if z is not None or mode != 0:
            raise ValueError("diagnostics need the device draw: z=None and mode=0")
        if not 4 <= len(draws["w_mcmc"]) <= fit.MAX_STORED_DRAWS:
            raise ValueError(f"diagnostics need 4 .. {fit.MAX_STORED_DRAWS} saved draws (the device keeps them)")
        if int(diagnostics_max_lag) < 0:
            raise ValueError("diagnostics_max_lag must not be negative (0: the default cap)")
    exc = None
    if excursions is not None:
        exc = dict(excursions)
        if set(exc) - {"thresholds", "side", "mask", "band", "thresholds_fun", "mask_fun"}:
            raise ValueError("excursions: unknown keys")
        if z is not None or mode != 0:
            raise ValueError("excursions need the device draw: z=None and mode=0")
        if exc.get("thresholds") is None and not exc.get("band"):
            raise ValueError("excursions: neither thresholds nor band")
        _exc.check_keep(len(draws["w_mcmc"]), bool(exc.get("band")))
        _exc.check_mask(exc.get("mask"), n_new)
        if exc.get("thresholds") is not None:
            _exc.expand_thresholds(exc["thresholds"], int(np.unique(np.asarray(mi["mv_id"])).size), exc.get("side", 1))
    rb = None
    if exceed is not None:
        if z is not None or mode != 0:
            raise ValueError("exceed needs the device draw: z=None and mode=0")
        try:
            rb = _rb.check_spec(exceed, int(np.unique(np.asarray(mi["mv_id"])).size), None if fun is None else fun[0].size - 1)
        except TypeError as e:
            raise ValueError(f"exceed: {e}") from None
    mix = None
    if mixture is not None:
        if z is not None or mode != 0:
            raise ValueError("mixture needs the device draw: z=None and mode=0")
        try:
            mix = _mix.check_spec(mixture, X_new is not None, ys is not None, len(draws["w_mcmc"]), ys)
        except TypeError as e:
            raise ValueError(f"mixture: {e}") from None
    rank = None
    if rank_diagnostics is not None and rank_diagnostics is not False:   # fit.spamtree_mv_mcmc's argument, for the points
        from . import diagnostics as _diag
        rank = {} if rank_diagnostics is True else dict(rank_diagnostics)
        if set(rank) - {"probs", "thresholds", "sides", "max_lag", "thresholds_fun"}:
            raise ValueError("rank_diagnostics: unknown keys")
        if z is not None or mode != 0:
            raise ValueError("rank_diagnostics need the device draw: z=None and mode=0")
        if not 4 <= len(draws["w_mcmc"]) <= fit.MAX_STORED_DRAWS:
            raise ValueError(f"rank_diagnostics need 4 .. {fit.MAX_STORED_DRAWS} saved draws (the device keeps them)")
        rank["max_lag"] = int(rank.get("max_lag", 0))
        rank["probs"], rank["thresholds"], rank["sides"] = _diag.check_rank_spec(rank.get("probs", ()), rank.get("thresholds", ()),
                                                                                  rank.get("sides"), rank["max_lag"])
    qs = tuple(float(x) for x in quantiles)
    if not all(0.0 <= x <= 1.0 for x in qs):
        raise ValueError("quantiles must lie in [0, 1]")
    if qs and ys is None:
        raise ValueError("quantiles need y_new (they bound the interval whose coverage is scored)")
    if qs and not crps:
        raise ValueError("quantiles need the stored draws: crps=True")
    if ys is not None and crps and len(draws["w_mcmc"]) > fit.MAX_STORED_DRAWS:
        raise ValueError(f"the CRPS keeps every saved draw of yhat on the device, at most {fit.MAX_STORED_DRAWS} (crps=False scores without)")
    anchor = locate(topo, coords_new, mv_new, device=device, joint=joint)
    w_list = draws["w_mcmc"]
    keep = len(w_list)
    p, q = int(mi["p"]), int(mi["q"])
    beta = np.asarray(draws["beta_mcmc"]).reshape(p, keep, q)
    tausq = np.asarray(draws["tausq_mcmc"]).reshape(q, keep)
    theta = np.asarray(draws["theta_mcmc"])
    theta = theta.reshape(theta.shape[0], keep)
    if z is not None:
        z = np.asarray(z, dtype=np.float64).reshape(n_new, keep)
    m = SpamTreeMV(mi["y"], mi["X"], mi["Z"], mi["coords"], mi["mv_id"], mi["blocking"], mi["gix_block"], mi["res_is_ref"],
                   mi["parents"], mi["children"], False, mi["block_names"], mi["block_groups"], mi["indexing"],
                   np.asarray(w_list[0]).reshape(-1), np.zeros(p), theta[:, 0], 1.0 / tausq[0, 0], device=device,
                   force_generic=force_generic)
    try:
        m.set_points(coords_new, mv_new, anchor, X_new, joint=joint)
        fdraws = None
        if fun is not None:
            m.set_functionals(fun)
            fdraws = {k: np.zeros((fun[0].size - 1, keep)) for k in ("w", "cond_mean", "cond_var", "yhat")}
        if ys is not None:
            m.set_scores(ys)
            if crps:
                m._check(m.lib.st_points_summary_reserve(m.h, keep))
        if diagnostics or exc is not None or rank is not None:
            m._check(m.lib.st_points_summary_reserve(m.h, keep))
        if rb is not None:
            m.set_exceed(list(rb[0]), rb[1], None if rb[2] is None else list(rb[2]))
        if mix is not None:
            m.reserve_mixture(keep)
        cc = []
        w_out = np.zeros((n_new, keep)) if return_draws else None
        y_out = np.zeros((n_new, keep)) if (return_draws and X_new is not None) else None
        cm = np.zeros((n_new, keep))
        cv = np.zeros((n_new, keep))
        for s in range(keep):
            m.set_w(np.asarray(w_list[s]).reshape(-1))
            m.beta_update(beta[:, s, :])
            m.tausq_inv = _f64(1.0 / tausq[:, s])
            m._check(m.lib.st_set_tausq_inv(m.h, _dp(m.tausq_inv)))
            m.theta_update(0, theta[:, s])
            if not m.get_loglik_comps_w(0):
                raise FloatingPointError(f"st_factor failed on saved draw {s} (errtype {m.last_errtype})")
            if fun is None and ys is None and not diagnostics and exc is None and rank is None and rb is None and mix is None:
                out = m.predict_points(mode=mode, z=None if z is None else z[:, s], seed=seed, it=s)
            else:
                out = m.accumulate_points(seed=seed, it=s)
                for k, v in (m.functionals_last().items() if fun is not None else ()):
                    if v is not None:
                        fdraws[k][:, s] = v
            cm[:, s] = out["mean"]
            cv[:, s] = out["var"]
            if joint is not None:
                cc.append(out["cov_packed"])
            if w_out is not None:
                w_out[:, s] = out["w"]
            if y_out is not None:
                y_out[:, s] = out["yhat"]
        res = dict(mean=cm.mean(axis=1), var=cv.mean(axis=1) + cm.var(axis=1), anchor=anchor, route=m.points_info()["routes"])
        if return_draws:
            res["w"] = w_out
            res["yhat"] = y_out
        if return_moments:
            res["cond_mean"] = cm
            res["cond_var"] = cv
        if fun is not None:
            res["functionals"] = {k: v for k, v in m.functionals().items() if k != "n"} if keep else {}
            if return_draws:
                res["functionals"].update(fdraws, yhat=fdraws["yhat"] if X_new is not None else None)
        if ys is not None and keep:
            lo_hi = (None, None)
            if len(qs) >= 2:
                yq = np.zeros(n_new)
                lo_hi = []
                for x in (min(qs), max(qs)):
                    m._check(m.lib.st_points_summary_quantile(m.h, x, None, _dp(yq)))
                    lo_hi.append(yq.copy())
            res["scores"] = m.scores(crps=crps, yhat_lo=lo_hi[0], yhat_hi=lo_hi[1])
        if rb is not None and keep:
            ex = m.exceed()
            fex = ex.pop("functionals", None)
            res["exceed"] = ex
            if fex is not None:
                res["functionals"]["exceed"] = dict(fex, side=ex["side"], n_accumulated=ex["n_accumulated"])
        if mix is not None and keep:
            if mix[0] is not None:
                mq = m.mixture_quantiles(mix[0])
                fmq = mq.pop("functionals", None)
                res["mixture"] = dict(mq, n_stored=keep)
                if fmq is not None:
                    res["functionals"]["mixture"] = dict(fmq, probs=mq["probs"], n_stored=keep)
            if mix[1]:
                mc = m.mixture_crps()
                res["scores"].update(crps_mixture=mc["crps"], spread=mc["spread"])
                tot = res["scores"]["totals"]
                for key, v in (("crps_mixture", mc["crps"]), ("spread", mc["spread"])):
                    tot[key], tot["by_outcome"][key] = _mix.point_means(v, ys, mv_new, q)
        if diagnostics and n_new:
            res["diagnostics"] = m.points_diagnostics(int(diagnostics_max_lag), n_kept=keep)
            if fun is not None:
                res["functionals"]["diagnostics"] = m.functionals_diagnostics(int(diagnostics_max_lag), n_kept=keep)
        if exc is not None and n_new:
            kw = dict(side=exc.get("side", 1), band=bool(exc.get("band")))
            res["excursions"] = m.points_excursions(keep, exc.get("thresholds"), mask=exc.get("mask"), **kw)
            if fun is not None:
                res["functionals"]["excursions"] = m.functionals_excursions(keep, exc.get("thresholds_fun", exc.get("thresholds")),
                                                                            mask=exc.get("mask_fun"), **kw)
        if rank is not None and n_new:
            kw = dict(probs=rank["probs"], sides=rank["sides"], max_lag=rank["max_lag"], n_kept=keep)
            res["rank_diagnostics"] = m.points_rank_diagnostics(thresholds=rank["thresholds"], **kw)
            if fun is not None:
                tf = rank.get("thresholds_fun")
                res["functionals"]["rank_diagnostics"] = m.functionals_rank_diagnostics(thresholds=rank["thresholds"] if tf is None else tf, **kw)
        if joint is not None:
            packed = np.mean(cc, axis=0) if keep else np.zeros(0)
            for k, g in enumerate(m.joint_groups):
                d = cm[g] - cm[g].mean(axis=1, keepdims=True)
                packed[m.joint_offsets[k]:m.joint_offsets[k + 1]] += (d @ d.T / keep).reshape(-1, order="F")
            res["groups"] = m.joint_groups
            res["cov"] = m.unpack_joint(packed)
            if return_draws:
                res["cond_cov"] = [m.unpack_joint(c) for c in cc]
        return res
    finally:
        m.close()


def fit_predict(model_inputs, coords_new, mv_new, X_new=None, quantiles=(), return_draws=True, joint=None, functionals=None,
                y_new=None, crps=True, diagnostics=False, diagnostics_max_lag=0, excursions=None, rank_diagnostics=None, chains=1,
                chain_seeds=None, chain_theta=None, exceed=None, mixture=None, **mcmc):
    """Fit the chain and predict at new locations on every saved iteration, without replaying it.

    ``model_inputs``: the problem as for :func:`predict_new`.  The points are located with :func:`locate` and handed to
    ``fit.spamtree_mv_mcmc(new_points=...)``; ``mcmc`` takes its keyword arguments (start values default to the workload's
    ``theta``, beta 0, tausq 0.1 and mcmcsd 0.01 I).  Each saved draw s is the one :func:`predict_new` gives for that draw
    with ``seed`` = the chain's seed, and the chain is the same as without points.

    Returns the fit's dict plus ``new``: ``mean``, ``var`` (Rao-Blackwellised, as :func:`predict_new`), ``anchor``, ``route``,
    ``w_mean``, ``yhat_mean`` and ``quantiles[q] = (w_q, yhat_q)`` from the device summaries, and with ``return_draws`` the
    n_new x keep draws ``w``, ``yhat`` and the per-draw ``cond_mean``, ``cond_var``.  yhat entries are None without ``X_new``.
    With ``joint`` labels also ``groups``, ``cov`` and (``return_draws``) ``cond_cov``, as :func:`predict_new`.
    With ``functionals`` (as :func:`predict_new`) also ``functionals``: dict(mean, var, w_mean, yhat_mean, quantiles) from the
    device and, with ``return_draws``, the n_fun x keep arrays ``w``, ``cond_mean``, ``cond_var``, ``yhat``.
    With ``y_new`` (held-out observations, one per point, NaN = not scored; needs ``X_new``) also ``scores``: the per-point ``lpd``,
    ``pit`` and ``crps``, per joint group ``lpd_joint``, ``n_scored``, ``n_degenerate`` and ``totals`` (means over the scored
    points, overall and per outcome; with two or more ``quantiles`` the coverage of [yhat_lo, yhat_hi]), all formed on the device
    during the fit, whatever ``return_draws`` is.  For the CRPS the device keeps ``mcmc_keep`` draws of w and yhat per point (16 B
    each per point and draw, at most 16384 draws); ``crps=False`` scores without it and stores nothing.
    With ``diagnostics`` the fit's ``diagnostics`` (``fit.spamtree_mv_mcmc``) and ``new["diagnostics"]``, ``new["functionals"]["diagnostics"]``.
    With ``excursions`` (the dict of ``fit.spamtree_mv_mcmc``) the fit's ``excursions``, ``new["excursions"]`` and
    ``new["functionals"]["excursions"]``.
    With ``rank_diagnostics`` (True or the dict of ``fit.spamtree_mv_mcmc``) the fit's ``rank_diagnostics``,
    ``new["rank_diagnostics"]`` and ``new["functionals"]["rank_diagnostics"]``.
    With ``exceed=dict(thresholds=, side=, thresholds_fun=)`` also ``new["exceed"]`` and ``new["functionals"]["exceed"]``: the
    Rao-Blackwellised exceedance probabilities of ``fit.spamtree_mv_mcmc(new_points=dict(exceed=))`` -- with ``return_draws=False``
    an exceedance map of any number of points with nothing of size n_new x mcmc_keep anywhere.
    With ``mixture=dict(probs=, crps=True)`` also ``new["mixture"]``, ``new["functionals"]["mixture"]`` and, with ``y_new``,
    ``new["scores"]["crps_mixture"]`` and ``["spread"]``: the quantiles and the exact CRPS of the mixture predictive of
    ``fit.spamtree_mv_mcmc(new_points=dict(mixture=))`` (at most 8192 saved draws over all chains).
    With ``chains`` > 1 (``chain_seeds``, ``chain_theta``: as ``fit.spamtree_mv_mcmc``) that many chains run one after another: every
    per-draw array holds ``chains * mcmc_keep`` columns, chain after chain (``chain_id``), the summaries are those of the pooled
    draws and the diagnostics the multi-chain ones.  :func:`predict_new` takes the concatenated result as it takes one chain's.
    """
    mi = model_inputs
    coords_new = np.asarray(coords_new, dtype=np.float64).reshape(-1, 2)
    mv_new = np.asarray(mv_new, dtype=np.int64).reshape(-1)
    if mv_new.size != coords_new.shape[0]:
        raise ValueError("coords_new and mv_new must describe the same points")
    if X_new is not None and np.asarray(X_new).shape != (coords_new.shape[0], int(mi["p"])):
        raise ValueError("X_new must be n_new x p")
    qs = tuple(float(x) for x in quantiles)
    if not all(0.0 <= x <= 1.0 for x in qs):
        raise ValueError("quantiles must lie in [0, 1]")
    fun = None if functionals is None else functionals_csr(functionals, coords_new.shape[0])
    ys = None if y_new is None else score_values(y_new, coords_new.shape[0], X_new is not None)
    if ys is not None and crps and int(chains) == 1 and int(mcmc.get("mcmc_keep", 100)) > fit.MAX_STORED_DRAWS:
        raise ValueError(f"the CRPS keeps mcmc_keep draws per point on the device, at most {fit.MAX_STORED_DRAWS} (crps=False scores without it)")
    if exceed is not None:   # before the points are located: that may use the device
        try:
            _rb.check_spec(exceed, int(np.unique(np.asarray(mi["mv_id"])).size), None if fun is None else fun[0].size - 1)
        except TypeError as e:
            raise ValueError(f"exceed: {e}") from None
    if mixture is not None:   # likewise
        try:
            _mix.check_spec(mixture, X_new is not None, ys is not None, int(chains) * int(mcmc.get("mcmc_keep", 100)), ys)
        except TypeError as e:
            raise ValueError(f"mixture: {e}") from None
    anchor = locate(mi["topo"], coords_new, mv_new, device=mcmc.get("device", 0), joint=joint)
    points = dict(coords=coords_new, mv=mv_new, anchor=anchor, X=X_new)
    if joint is not None:
        points["joint"] = joint
    if fun is not None:
        points["functionals"] = fun
    if ys is not None:
        points["y"] = ys
        points["crps"] = bool(crps)
    if exceed is not None:
        points["exceed"] = exceed
    if mixture is not None:
        points["mixture"] = mixture
    theta = np.asarray(mcmc.pop("theta", mi["theta"]), dtype=np.float64)
    kw = dict(set_unif_bounds_in=mi["bounds"], start_w=np.zeros((int(mi["n"]), 1)), theta=theta, beta=np.zeros(int(mi["p"])),
              tausq=0.1, mcmcsd=0.01 * np.eye(theta.size))
    kw.update(mcmc)
    out = fit.spamtree_mv_mcmc(mi["y"], mi["X"], mi["Z"], mi["coords"], mi["mv_id"], mi["blocking"], mi["gix_block"],
                               mi["res_is_ref"], mi["parents"], mi["children"], bool(mi.get("limited_tree", False)),
                               mi["block_names"], mi["block_groups"], mi["indexing"],
                               new_points=points, new_draws=return_draws,
                               new_quantiles=qs, diagnostics=diagnostics, diagnostics_max_lag=diagnostics_max_lag, excursions=excursions,
                               rank_diagnostics=rank_diagnostics, chains=chains, chain_seeds=chain_seeds, chain_theta=chain_theta, **kw)
    out["new"]["anchor"] = anchor
    return out
