"""Python face of the C++ host driver (spamtree_amd/csrc/spamtree_fit.cpp, include/spamtree_fit.h): the same
`spamtree_mv_mcmc(...)` argument list and returned names as the reference's Rcpp export
(/root/reference/src/spamtree_fit.cpp:5-54, 403-414), and a steppable `Chain` for benchmarking."""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace
from typing import NamedTuple, Optional

import numpy as np

from . import _lib
from . import diagnostics as _diag
from . import exceed as _rb
from . import mixture as _mix
from . import excursions as _exc
from . import loo as _loo
from .model import (SpamTreeError, _dp, _f64, _i64, _ip, _lists_to_csr, functionals_csr, joint_labels, rows_criteria, rows_holdout,
                    rows_loo_criteria, rows_psis_criteria, score_totals,
                    score_values, series_diag_buffers, series_diag_finish, excursion_spec, excursion_buffers, excursion_finish,
                    rank_spec, rank_buffers, rank_finish)


def _problem(y, X, coords, mv_id, res_is_ref, parents, children, block_names, block_groups, indexing):
    y = _f64(np.asarray(y).reshape(-1))
    X = np.asfortranarray(np.asarray(X, dtype=np.float64))
    coords = np.asfortranarray(np.asarray(coords, dtype=np.float64))
    mv_id = _i64(mv_id)
    ip, ii = indexing if isinstance(indexing, tuple) else _lists_to_csr(indexing)
    pp, pi = parents if isinstance(parents, tuple) else _lists_to_csr(parents)
    cp, ci = children if isinstance(children, tuple) else _lists_to_csr(children)
    keep = [y, X, coords, mv_id, _i64(res_is_ref), _i64(block_names), _i64(block_groups), _i64(ip), _i64(ii), _i64(pp),
            _i64(pi), _i64(cp), _i64(ci)]
    n, p = X.shape
    q = int(np.unique(mv_id).size)
    pb = _lib.StProblem(n, coords.shape[1], q, p, int(keep[4].size), int(keep[5].size), _dp(y), _dp(X), _dp(coords),
                        _ip(mv_id), *[_ip(a) for a in keep[4:]])
    return pb, keep, n, p, q


def make_unique_id():
    """128-byte RCCL unique id (rank 0 creates it; broadcast it to the other ranks, e.g. with torch.distributed)."""
    lib = _lib.load()
    buf = C.create_string_buffer(128)
    n = lib.st_comm_unique_id(C.cast(buf, C.c_void_p), 128)
    if n <= 0:
        raise SpamTreeError("st_comm_unique_id failed")
    return bytes(buf.raw[:128])


class Chain:
    """stm_chain: SpamTreeMV + RAMAdapt + loop state, stepped from C++ (one ctypes call per `step(n)`)."""

    def __init__(self, y, X, Z, coords, mv_id, blocking, gix_block, res_is_ref, parents, children, limited_tree,
                 block_names, block_groups, indexing, set_unif_bounds, theta, beta, tausq, mcmcsd, seed=2021,
                 adapting=True, sample_beta=True, sample_tausq=True, sample_theta=True, sample_w=True, device=0,
                 reference_quirks=True, rank=0, world=1, unique_id=None, defer_comm=False, defer_leaf=True):
        self.lib = _lib.load()
        pb, self._keep, self.n, self.p, self.q = _problem(y, X, coords, mv_id, res_is_ref, parents, children,
                                                          block_names, block_groups, indexing)
        theta = _f64(theta)
        self.k = theta.size
        bounds = np.asfortranarray(np.asarray(set_unif_bounds, dtype=np.float64))
        sd = np.asfortranarray(np.asarray(mcmcsd, dtype=np.float64))
        opt = _lib.StOptions(int(device), int(bool(reference_quirks)), int(rank), int(world), 0,
                             (2 if limited_tree else 0) | (0 if defer_leaf else 4))
        fl = _lib.StmFlags(int(adapting), int(sample_beta), int(sample_tausq), int(sample_theta), int(sample_w), 1)
        c = C.c_void_p()
        self.c = None
        if world > 1 and unique_id is None and not defer_comm:
            raise SpamTreeError("world > 1 needs the RCCL unique id of rank 0 (spamtree_amd.fit.make_unique_id)")
        rc = self.lib.stm_create(C.byref(pb), C.byref(opt), _dp(bounds), _dp(sd), _dp(theta), self.k, _dp(_f64(beta)),
                                 float(tausq), int(seed), C.byref(fl), C.byref(c))
        self.c = c
        if rc != 0:
            msg = self.lib.stm_last_error(c).decode() if c else self.lib.st_last_error(None).decode()
            if c:
                self.lib.stm_destroy(c)
                self.c = None
            raise SpamTreeError(f"stm_create failed ({rc}): {msg or self.lib.st_last_error(None).decode()}")
        self.h = C.c_void_p(self.lib.stm_handle(self.c))
        self.rank, self.world = int(rank), int(world)
        # defer_comm: stop after the local part (st_create), so that the ranks can first agree that it succeeded everywhere:
        # ncclCommInitRank is collective and a rank that failed before it would leave the others blocked in the bootstrap.
        # The caller then runs comm_init(unique_id) -- a failure INSIDE that collective cannot be recovered from -- and start().
        if defer_comm:
            return
        if world > 1 or unique_id is not None:   # a unique id with world == 1: the RCCL protocol path on a single rank (tests)
            self.comm_init(unique_id)
        self.start()

    def comm_init(self, unique_id):
        buf = C.create_string_buffer(bytes(unique_id), 128)
        rc = self.lib.st_comm_init(self.h, C.cast(buf, C.c_void_p))
        if rc != 0:
            raise SpamTreeError(f"st_comm_init failed ({rc}): {self.lib.st_last_error(self.h).decode()}")

    def start(self):
        rc = self.lib.stm_init(self.c)
        if rc != 0:
            raise SpamTreeError(f"stm_init failed ({rc}): {self.lib.stm_last_error(self.c).decode()}")

    def step(self, n=1):
        rc = self.lib.stm_step(self.c, int(n))
        if rc != 0:
            raise SpamTreeError(f"stm_step failed ({rc}): {self.lib.stm_last_error(self.c).decode()}")

    def state(self):
        theta = np.zeros(self.k); B = np.zeros(self.p * self.q); tsq = np.zeros(self.q); sd = np.zeros(self.k * self.k)
        ll, ar, it = C.c_double(), C.c_double(), C.c_int64()
        self.lib.stm_state(self.c, _dp(theta), _dp(B), _dp(tsq), C.byref(ll), C.byref(ar), C.byref(it), _dp(sd))
        return dict(theta=theta, Bcoeff=B.reshape(self.q, self.p).T.copy(), tausq_inv=tsq, loglik=ll.value,
                    accept_ratio=ar.value, iteration=it.value, paramsd=sd.reshape(self.k, self.k).T.copy())

    def get_w(self):
        out = np.zeros(self.n)
        self.lib.st_get_w(self.h, _dp(out))
        return out

    # measurement helpers (same as SpamTreeMV's)
    def algorithmic_bytes(self):
        out, fl = np.zeros(5), np.zeros(3)
        self.lib.st_algorithmic_bytes(self.h, _dp(out), _dp(fl))
        return dict(A=out[0], B=out[1], C=out[2], msg=out[3], S=out[4], total=float(out.sum()), flops_A=fl[0],
                    flops_B=fl[1], flops_C=fl[2])

    def profile(self, enable):
        self.lib.st_profile_enable(self.h, 2 if enable == 2 else int(bool(enable)))

    def profile_get(self):
        ms, n = np.zeros(8), np.zeros(8, dtype=np.int64)
        self.lib.st_profile_get(self.h, _dp(ms), _ip(n))
        names = ["factor", "sample", "loglik", "reduce", "stats", "rng", "predict", "comm"]
        return {k: (float(ms[i]), int(n[i])) for i, k in enumerate(names)}

    def profile_levels(self):
        nl = C.c_int32(); ms = np.zeros(64); by = np.zeros(64)
        self.lib.st_profile_levels(self.h, C.byref(nl), _dp(ms), _dp(by), 64)
        return ms[: nl.value].copy(), by[: nl.value].copy()

    def profile_levels_all(self):
        """(phase A ms, phase A algorithmic bytes, phase B ms, phase B + message bytes) per level since the last call."""
        nl = C.c_int32(); ms = np.zeros(128); by = np.zeros(128)
        self.lib.st_profile_levels(self.h, C.byref(nl), _dp(ms), _dp(by), 128)
        k = nl.value
        return ms[:k].copy(), by[:k].copy(), ms[k: 2 * k].copy(), by[k: 2 * k].copy()

    def factor_ahead_levels(self):
        """Leading levels whose phase A the driver starts before the sweep (st_factor_begin); 0 = none."""
        return int(self.lib.st_factor_ahead_levels(self.h))

    def synchronize(self):
        self.lib.st_synchronize(self.h)

    def shard_info(self):
        r, w, c = C.c_int32(), C.c_int32(), C.c_int32()
        ob, orow = C.c_int64(), C.c_int64()
        self.lib.st_shard_info(self.h, C.byref(r), C.byref(w), C.byref(c), C.byref(ob), C.byref(orow))
        return dict(rank=r.value, world=w.value, cut_level=c.value, owned_blocks=ob.value, owned_rows=orow.value)

    def close(self):
        if self.c:
            self.lib.stm_destroy(self.c)
            self.c = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


MAX_STORED_DRAWS = 16384   # st_points_summary_reserve: one point's draws are sorted in one workgroup's LDS


class PointsInputs(NamedTuple):
    """The checked point set of spamtree_mv_mcmc(new_points=...)."""
    coords: np.ndarray
    mv: np.ndarray
    anchor: np.ndarray
    X: Optional[np.ndarray]
    quantiles: np.ndarray
    labels: Optional[np.ndarray]
    functionals: Optional[tuple]   # model.functionals_csr's (ptr, idx, wt); None: no functional
    y: Optional[np.ndarray]
    crps: bool


def _points_inputs(new_points, p, q, new_quantiles):
    """Checks the point set of spamtree_mv_mcmc(new_points=...) against itself and the problem, before any device call."""
    pts = dict(new_points)
    unknown = set(pts) - {"coords", "mv", "anchor", "X", "joint", "functionals", "y", "crps", "exceed", "mixture"}
    if unknown:
        raise ValueError(f"new_points: unknown keys {sorted(unknown)} (coords, mv, anchor, X, joint, functionals, y, crps, exceed, mixture)")
    coords = np.asarray(pts["coords"], dtype=np.float64)
    if coords.ndim != 2 or coords.shape[1] != 2:
        raise ValueError("new_points: coords must be n_new x 2")
    n_new = coords.shape[0]
    mv = np.asarray(pts["mv"])
    anchor = np.asarray(pts["anchor"])
    if mv.shape != (n_new,) or anchor.shape != (n_new,):
        raise ValueError("new_points: mv and anchor must hold one entry per row of coords")
    if not (np.issubdtype(mv.dtype, np.integer) and np.issubdtype(anchor.dtype, np.integer)):
        raise ValueError("new_points: mv and anchor must be integers")
    if n_new and (mv.min() < 1 or mv.max() > q):
        raise ValueError(f"new_points: mv must lie in 1..{q}")
    if not np.all(np.isfinite(coords)):
        raise ValueError("new_points: coords must be finite")
    X = pts.get("X")
    if X is not None:
        X = np.asfortranarray(np.asarray(X, dtype=np.float64))
        if X.shape != (n_new, p):
            raise ValueError(f"new_points: X must be n_new x p = {n_new} x {p}")
    qs = np.asarray(new_quantiles, dtype=np.float64).reshape(-1)
    if not np.all((qs >= 0.0) & (qs <= 1.0)):
        raise ValueError("new_quantiles must lie in [0, 1]")
    labels = pts.get("joint")
    if labels is not None:
        try:
            labels = joint_labels(labels, n_new)
        except ValueError as e:
            raise ValueError(f"new_points: {e}") from None
    fun = pts.get("functionals")
    if fun is not None:
        try:
            fun = functionals_csr(fun, n_new)
        except ValueError as e:
            raise ValueError(f"new_points: {e}") from None
        if fun[0].size == 1:
            fun = None
    y = pts.get("y")
    if y is not None:
        try:
            y = score_values(y, n_new, X is not None)
        except ValueError as e:
            raise ValueError(f"new_points: {e}") from None
    crps = bool(pts.get("crps", True)) and y is not None
    if "crps" in pts and y is None:
        raise ValueError("new_points: crps needs y")
    return PointsInputs(np.asfortranarray(coords), _i64(mv), _i64(anchor), X, qs, labels, fun, y, crps)


def _exceed_inputs(new_points, pts, q):
    """``new_points["exceed"]`` checked against the point set ``pts`` (_points_inputs') before any device call: exceed.check_spec's
    (thr, side, thr_fun), or None without the key."""
    spec = dict(new_points).get("exceed")
    if spec is None:
        return None
    try:
        return _rb.check_spec(spec, q, None if pts.functionals is None else pts.functionals[0].size - 1)
    except (ValueError, TypeError) as e:
        raise ValueError(f"new_points: {e}") from None


def _mixture_inputs(new_points, pts, keep_all):
    """``new_points["mixture"]`` checked against the point set ``pts`` (_points_inputs') and the saved draws of all chains before any
    device call: mixture.check_spec's (probs or None, crps), or None without the key."""
    spec = dict(new_points).get("mixture")
    if spec is None:
        return None
    try:
        return _mix.check_spec(spec, pts.X is not None, pts.y is not None, keep_all, pts.y)
    except (ValueError, TypeError) as e:
        raise ValueError(f"new_points: {e}") from None


def _joint_layout(labels):
    """Host mirror of st_points_joint_layout: groups by first appearance, members in the caller's order, g x g blocks."""
    _, first, inv = np.unique(labels, return_index=True, return_inverse=True)
    rank = np.empty(first.size, dtype=np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(first.size)
    grp = rank[np.asarray(inv).reshape(-1)]
    groups = [np.nonzero(grp == k)[0] for k in range(first.size)]
    off = np.concatenate([[0], np.cumsum([g.size ** 2 for g in groups])]).astype(np.int64)
    return groups, off


def _unpack_joint(packed, groups, off):
    blocks = [np.asarray(packed[off[k]:off[k + 1]]).reshape(g.size, g.size, order="F").copy() for k, g in enumerate(groups)]
    return np.stack(blocks) if blocks and len({b.shape for b in blocks}) == 1 else blocks


def spamtree_mv_mcmc(y, X, Z, coords, mv_id, blocking, gix_block, res_is_ref, parents, children, limited_tree,
                     layer_names, layer_gibbs_group, indexing, set_unif_bounds_in, start_w, theta, beta, tausq, mcmcsd,
                     mcmc_keep=100, mcmc_burn=100, mcmc_thin=1, num_threads=1, use_alg="S", adapting=False,
                     main_verbose=True, verbose=False, debug=False, printall=False, sample_beta=True, sample_tausq=True,
                     sample_theta=True, sample_w=True, sample_predicts=True, seed=2021, device=0, reference_quirks=True,
                     new_points=None, new_draws=True, new_quantiles=(), save_w=True, save_yhat=True, force_generic=False,
                     criteria=False, y_holdout=None, holdout_crps=True, diagnostics=False, diagnostics_max_lag=0, excursions=None,
                     rank_diagnostics=None, chains=1, chain_seeds=None, chain_theta=None, loo=False, psis=False, psis_draws=False,
                     loo_groups=None):
    """spamtree_fit.cpp:5-430 through the C++ driver.  `num_threads`, `use_alg`, the verbosity flags and `start_w` are
    accepted and ignored exactly where the reference ignores them (start_w, :95) or where they do not apply to a GPU.

    Not in the reference: ``save_w`` / ``save_yhat`` False leave ``w_mcmc`` / ``yhat_mcmc`` out (nothing is copied or
    allocated for them); ``force_generic`` runs the generic kernels.  ``new_points=dict(coords, mv, anchor, X=None)``
    (n_new x 2, 1-based margins, 0-based anchor blocks of ``predict.locate``, n_new x p regressors) predicts at those
    locations on every saved iteration, on the device (stm_mcmc_points); the chain is the same bit for bit.  Then the
    result also holds ``new``: dict(mean, var, w_mean, yhat_mean, quantiles={q: (w_q, yhat_q)}, route) and, with
    ``new_draws``, the per-draw n_new x keep arrays ``w``, ``cond_mean``, ``cond_var``, ``yhat`` (yhat entries None
    without X).  ``new_quantiles`` keeps the draws on the device.  With points, a failure raises SpamTreeError.
    ``new_points["joint"]``: one integer label per point; each label's points (at most 16, one anchor) are drawn jointly
    (stm_mcmc_points_joint) and ``new`` also holds ``groups`` (member indices per group), ``cov`` (per group the predictive
    covariance, mean conditional covariance + covariance of the conditional means) and, with ``new_draws``, ``cond_cov``
    (per saved draw, per group).
    ``new_points["functionals"]``: linear functionals of the predictions (``model.functionals_csr`` has the accepted forms;
    ``predict.areal_means`` / ``predict.contrasts`` build common ones), summarised on the device (stm_mcmc_functionals); ``new``
    then also holds ``functionals``: dict(mean, var, w_mean, yhat_mean, quantiles={q: (w_q, yhat_q)}) and, with ``new_draws``,
    the per-draw n_fun x keep arrays ``w``, ``cond_mean``, ``cond_var``, ``yhat``.
    ``new_points["y"]``: held-out observations at the points (one per point, NaN = not scored; needs ``X``), scored on the device
    on every saved iteration (stm_mcmc_scored); ``new`` then also holds ``scores``: dict(lpd, pit, crps, lpd_joint, n_scored,
    n_degenerate, totals) -- the per-point log predictive density of the mixture over the saved draws, its PIT, the CRPS of the
    stored yhat draws (which stay on the device: nothing per draw comes to the host for it), per joint group the joint log
    predictive density, and ``model.score_totals``' means, with the coverage of [yhat_lo, yhat_hi] for the lowest and highest of
    two or more ``new_quantiles``.  The CRPS makes the device keep ``mcmc_keep`` draws of w and yhat per point (16 B each per
    point and draw; at most 16384 draws, more is a ValueError); ``new_points["crps"] = False`` scores without it and stores nothing.
    ``new_points["exceed"] = dict(thresholds=, side=, thresholds_fun=)``: Rao-Blackwellised exceedance probabilities
    (``spamtree_amd.exceed``; thresholds as for ``excursions``: up to 8, each a scalar or one value per outcome, sides +-1) -- on
    every saved iteration the exact conditional probability of w* (and, with ``X``, yhat*) lying beyond each threshold is folded
    into a running mean and variance on the device, so nothing per draw is stored and ``new_draws=False`` stays lean.  ``new``
    then also holds ``exceed``: dict(thr, side, w=dict(prob, prob_var), yhat=the same or None, n_accumulated), T x n_new arrays
    (``prob_var``: the population variance of the per-draw probabilities, MCSE = sqrt(prob_var / ESS)), and with
    ``thresholds_fun`` (one value per functional) ``new["functionals"]["exceed"]`` for the functionals' w.
    ``new_points["mixture"] = dict(probs=, crps=True)``: quantiles and the exact CRPS of the mixture predictive
    (``spamtree_amd.mixture``): every saved draw's exact conditional law is one component, stored on the device (24 B per point and
    draw; at most 8192 draws over all chains).  ``new`` then holds ``mixture``: dict(probs, w, yhat (None without X), n_stored,
    n_unconverged), T x n_new arrays, and with functionals ``new["functionals"]["mixture"]``; with ``y`` and ``crps=True``
    ``new["scores"]`` also holds ``crps_mixture`` and ``spread`` (O(K^2) per scored point) with their means in ``totals``.
    ``criteria=True``: WAIC and DIC over the observed rows, on the device (stm_mcmc_criteria; the chain is the same bit for bit, and
    nothing per draw comes to the host, so it works with ``save_w=False, save_yhat=False``).  ``y_holdout``: the truth at NA rows
    of ``y`` (one value per row, NaN = none; ``model.rows_holdout`` checks it), scored there on every saved iteration; it implies
    ``criteria`` and needs ``sample_predicts``.  The result then holds ``criteria``: the per-row arrays ``lppd``, ``p_waic``,
    ``mean_ll``, ``mu_mean``, ``pit``, ``crps`` (NaN where a row has no target; pit and crps at held-out rows only) and ``totals`` =
    ``model.rows_criteria``'s dict(observed, held_out), each overall and by outcome.  Every criterion is CONDITIONAL ON w: the
    likelihood is N(y; XB + w, tausq), so the WAIC and DIC penalties count the effective dimension of the latent field too.  The
    CRPS makes the device keep ``mcmc_keep`` draws of w and yhat per row (at most 16384, more is a ValueError);
    ``holdout_crps=False`` scores without it.  Not together with ``new_points``.  As with ``new_points``, a failure of the
    chain (a refusal of the library, a Cholesky failure code) raises SpamTreeError with ``code`` set, where the plain call prints
    "MCMC has been interrupted." and returns ``{"None": ...}``; a NaN log-density is a FloatingPointError in both.
    ``loo=True``: leave-one-out criteria with each row's own w_i integrated out, on the device (stm_mcmc_loo: stm_mcmc_criteria plus
    st_rows_loo_accumulate on every saved iteration; the chain and the conditional criteria are the same bit for bit).  It may be
    combined with ``criteria`` / ``y_holdout`` and not with what ``criteria`` excludes.  The result's ``criteria["loo"]`` holds the
    per-row arrays ``elpd_loo``, ``pit_loo``, ``mu_loo``, ``weight_ess`` (NaN where a row has no observed y), ``n_accumulated``,
    ``n_skipped`` and ``totals`` = ``model.rows_loo_criteria``'s dict, overall and by outcome (``spamtree_amd.loo`` has the
    definition).  These are the raw weights, with ``weight_ess`` as their diagnostic.  ValueError before any device call for
    ``limited_tree``.
    ``loo=True, psis=True``: the weights are also Pareto smoothed on the device (``spamtree_amd.psis`` has the definition): every
    saved draw's log ratio, Phi and mu are kept there (24 B per row and draw), and ``criteria["loo"]["psis"]`` holds the per-row
    arrays ``khat``, ``elpd_psis``, ``pit_psis``, ``mu_psis``, ``weight_ess_psis``, ``tail_len``, ``n_draws`` and ``totals`` =
    ``model.rows_psis_criteria``'s dict (``se``, ``max_khat``, the counts of rows with a large khat), and with ``psis_draws=True`` the
    pointwise matrices ``t``, ``phi``, ``mu`` (mcmc_keep x n).  The chain and every other output are the same bit for bit.
    ValueError before any device call: ``psis`` without ``loo``, ``mcmc_keep`` outside 1 .. 16384.
    ``loo=True, loo_groups=labels``: leave-group-out criteria on top (``spamtree_amd.loo`` has the definition): one int64 label per
    row, negative = in no group; the rows of one label (1 .. 16 of them, in blocks with an observed row) are left out together and
    their rows of w integrated out jointly -- ``loo.site_groups(coords)`` labels all outcomes at a location, ``loo.block_groups(coords,
    cell)`` square cells.  The same sweep serves rows and groups; ``criteria["loo"]`` is bit for bit that of the call without groups
    and also holds ``groups``: dict(label, members (a list of row arrays), elpd_lgo, weight_ess, n_skipped per group; mu_lgo, pit_lgo
    per row, NaN off the observed members; totals = dict(elpd_lgo, lgoic, se, min_weight_ess, n_groups, by_outcome)) and, with
    ``psis=True``, the groups' ``khat``, ``elpd_psis`` and ``weight_ess_psis``.  ValueError before any device call: labels that are
    not one integer per row, a group of more than 16 members or without an observed member, ``loo_groups`` without ``loo``.
    ``diagnostics=True``: the effective sample size ``ess``, the Monte-Carlo standard error of the posterior mean ``mcse``, the
    posterior sd of the draws ``sd``, the split-R-hat of the one chain ``rhat``, the lags used ``lags`` and whether the lag cap was
    hit ``truncated`` (``spamtree_amd.diagnostics`` has the definition; ``diagnostics_max_lag`` = 0 is its default cap of 1024
    lags).  The result then holds ``diagnostics``: ``theta`` (k), ``beta`` (p x q) and ``tausq`` (q) from the saved scalar chains
    on the host; ``w`` and ``yhat`` per row of the problem from the device, which keeps ``mcmc_keep`` draws of both per row for it
    (stm_mcmc_diagnosed: the chain is the same bit for bit; nothing per draw comes to the host, so it works with ``save_w=False,
    save_yhat=False, new_draws=False``); and ``summary``: ``diagnostics.summarise`` of each part, w and yhat also by outcome.  With
    ``new_points`` also ``new["diagnostics"]`` (w, yhat per point) and ``new["functionals"]["diagnostics"]``.  ``mcmc_keep`` must lie
    in 4 .. 16384 (ValueError); not together with ``criteria`` / ``y_holdout`` (one driver per call).  A failure of the chain raises
    SpamTreeError, as with ``new_points``.
    ``excursions=dict(thresholds=, side=, mask=, band=)``: exceedance probabilities, the excursion function and, with ``band``,
    the simultaneous band's ingredients (``spamtree_amd.excursions`` has the definition and what to do with them), formed on the
    device after the last iteration from ``mcmc_keep`` draws of w and yhat it keeps per row (stm_mcmc_excursions: the chain is the
    same bit for bit; it works with ``save_w=False, save_yhat=False, new_draws=False``).  ``thresholds``: a scalar or up to 8
    entries, each a scalar or one value per outcome; ``side``: +1 (above) / -1 (below), a scalar or one per threshold; ``mask``:
    one entry per row, 0 = in no domain.  The result holds ``excursions``: dict(w, yhat) of dict(count, prob, excur (T x n),
    joint_all (T x q), mean, sd (n), maxdev (q x K), n_flat (q), n_draws).  With ``new_points`` also ``new["excursions"]``
    (``mask_new`` masks the points) and ``new["functionals"]["excursions"]`` (``thresholds_fun``: entries scalar or one value per
    functional, default ``thresholds`` when all its entries are scalars; ``mask_fun``).  May be combined with ``diagnostics``, not
    with ``criteria`` / ``y_holdout``.  ValueError before any device call: bad shapes, more than 8 thresholds, non-finite
    thresholds, ``mcmc_keep`` outside 1 .. 16384 (2 with ``band``).

    ``rank_diagnostics=True`` or ``dict(probs=, thresholds=, sides=, max_lag=, thresholds_fun=)``: rank-normalised R-hat, bulk and
    tail ESS, the ESS of the quantiles ``probs`` and of the exceedances of ``thresholds`` with their probability and its MCSE
    (``spamtree_amd.diagnostics`` has the definition), formed on the device after the last iteration from ``mcmc_keep`` draws of w
    and yhat it keeps per row (stm_mcmc_ranked: the chain is the same bit for bit).  The result holds ``rank_diagnostics``:
    ``theta``, ``beta``, ``tausq`` from ``diagnostics.chains_rank_diagnostics`` on the saved scalar chains (host; ``probs`` only: the
    thresholds are the field's), ``w`` and ``yhat`` per row from the device, and ``summary`` (``diagnostics.summarise_rank``, by
    outcome for the rows); with ``new_points`` also ``new["rank_diagnostics"]`` and ``new["functionals"]["rank_diagnostics"]``
    (``thresholds_fun``: entries scalar or one value per functional, default ``thresholds``).  May be combined with
    ``diagnostics`` and ``excursions``, not with ``criteria`` / ``y_holdout``.  ValueError before any device call: what the calls
    refuse of a spec, bad shapes, ``mcmc_keep`` outside 4 .. 16384.

    ``chains=M`` > 1 (at most 16): M chains one after another on one handle (stm_mcmc_chains), each the fit from scratch with
    ``chain_seeds[c]`` (default ``seed + c``) from ``chain_theta[c]`` (M x k; default ``theta``; ``mcmc.disperse_theta`` draws
    dispersed starts) -- chain c's draws are, bit for bit, those of the single-chain call with that seed and start.  Every per-draw
    array then has ``M * mcmc_keep`` columns, chain after chain, with ``chain_id`` naming each column's chain; ``paramsd`` is
    k x k x M, ``chain_time`` the seconds per chain.  Means, variances, quantiles, excursions and scores are those of the pooled
    draws.  ``diagnostics`` and ``rank_diagnostics`` are the multi-chain ones (``diagnostics.multichain_diagnostics``: the R-hat
    over all 2M half chains, the ESS of the combined chains) under the same keys, on the device for rows, points and functionals
    and on the host for theta, beta and tausq, with ``n_chains`` recorded in them; ``mcmc_keep`` is then the length of one chain.
    ValueError: ``M * mcmc_keep`` > 16384, M outside 1 .. 16, together with ``criteria`` / ``y_holdout`` (a separate driver)."""
    rq = _check_request(y, X, mv_id, theta, limited_tree, mcmc_keep, sample_predicts, sample_w, seed, new_points, new_quantiles, criteria,
                        y_holdout, holdout_crps, diagnostics, diagnostics_max_lag, excursions, rank_diagnostics, chains, chain_seeds,
                        chain_theta, loo, psis, psis_draws)
    rq.groups = _check_groups(loo_groups, rq.loo, y, indexing)
    M, keep_all, max_lag = rq.M, rq.keep_all, rq.max_lag
    lib = _lib.load()
    pb, keep, n, p, q = _problem(y, X, coords, mv_id, res_is_ref, parents, children, layer_names, layer_gibbs_group, indexing)
    theta, beta = _f64(theta), _f64(beta)
    k = theta.size
    bounds = np.asfortranarray(np.asarray(set_unif_bounds_in, dtype=np.float64))
    sd = np.asfortranarray(np.asarray(mcmcsd, dtype=np.float64))
    opt = _lib.StOptions(int(device), int(bool(reference_quirks)), 0, 1, int(bool(force_generic)), 2 if limited_tree else 0)
    fl = _lib.StmFlags(int(adapting), int(sample_beta), int(sample_tausq), int(sample_theta), int(sample_w), int(sample_predicts))
    w_all = np.zeros((n, keep_all), order="F") if save_w else None
    yh_all = np.zeros((n, keep_all), order="F") if save_yhat else None
    beta_mcmc = np.zeros((p, keep_all, q), order="F"); tausq_mcmc = np.zeros((q, keep_all), order="F")
    theta_mcmc = np.zeros((k, keep_all), order="F"); paramsd = np.zeros((k, k), order="F")
    t = C.c_double()
    # the request (include/spamtree_fit.h, stm_fit): the run, then one pointer per part that is asked for
    req = _lib.StmFit()
    req.run = _lib.StmRun(C.pointer(pb), C.pointer(opt), _dp(bounds), _dp(theta), k, _dp(beta), float(tausq), _dp(sd), int(mcmc_keep),
                          int(mcmc_burn), int(mcmc_thin), int(seed), C.pointer(fl), _opt(w_all), _opt(yh_all), _dp(beta_mcmc),
                          _dp(tausq_mcmc), _dp(theta_mcmc), _dp(paramsd), C.pointer(t))
    if M > 1:
        paramsd_all, chain_time = np.zeros((k, k, M), order="F"), np.zeros(M)
        chs = _lib.StmChains(M, rq.seeds.ctypes.data_as(C.POINTER(C.c_uint64)), _opt(rq.theta0), _dp(paramsd_all), _dp(chain_time))
        req.ch = C.pointer(chs)
    rows = _row_parts(req, rq, n, q, mcmc_keep)
    new_result = _point_parts(lib, req, rq, rows, q, mcmc_keep, new_draws) if rq.pts is not None else None

    rc = lib.stm_mcmc_fit(C.byref(req)) if rq.more is None else lib.stm_fit_run(C.byref(req), C.byref(rq.more))
    if rc == -10:
        raise FloatingPointError("At nan loglik: error.")
    if rc != 0:
        driver = _reported_driver(rq)
        if driver is None:
            if main_verbose:
                print("MCMC has been interrupted.")
            return {"None": np.zeros(0)}
        text = f"{driver} failed ({rc})"
        if driver == "stm_mcmc_chains":   # what the library refused of the chains before a chain existed to carry the text
            text = f"{text} {lib.stm_mcmc_chains_last_error().decode()}".rstrip()
        err = SpamTreeError(text)
        err.code = rc
        raise err

    out = {}
    if save_w:
        out["w_mcmc"] = [w_all[:, i].reshape(-1, 1).copy() for i in range(keep_all)]
    if save_yhat:
        out["yhat_mcmc"] = [yh_all[:, i].reshape(-1, 1).copy() for i in range(keep_all)]
    out.update(beta_mcmc=beta_mcmc, tausq_mcmc=tausq_mcmc, theta_mcmc=theta_mcmc, paramsd=paramsd, mcmc_time=t.value)
    if M > 1:   # per-draw arrays hold chain after chain; the multi-chain diagnostics name their n_chains
        out.update(paramsd=paramsd_all, chain_time=chain_time, chain_id=np.repeat(np.arange(M), int(mcmc_keep)), n_chains=M)
    if new_result is not None:
        out["new"] = new = new_result()
        if M > 1:
            for part in (new, new.get("functionals", {})):
                for key in ("diagnostics", "rank_diagnostics"):
                    if key in part:
                        part[key]["n_chains"] = M
    if rows.criteria is not None and mcmc_keep > 0:
        out["criteria"] = rows.criteria()
    mv_rows = _i64(mv_id).reshape(-1)
    scalars = dict(theta=theta_mcmc, beta=np.transpose(beta_mcmc, (0, 2, 1)), tausq=tausq_mcmc)   # the saved scalar chains: on the host

    def rows_summary(host, finish, bufs, summarise):
        d = {key: host(a) for key, a in scalars.items()}
        d.update({key: finish(v) for key, v in bufs.items()})
        d["summary"] = {key: summarise(d[key], mv_rows if key in ("w", "yhat") else None) for key in ("theta", "beta", "tausq", "w", "yhat")}
        if M > 1:
            d["n_chains"] = M
        return d
    if rows.diag is not None:
        out["diagnostics"] = rows_summary(lambda a: _diag.chains_diagnostics(a, max_lag, M),
                                          lambda v: series_diag_finish(v, mcmc_keep, max_lag), rows.diag, _diag.summarise)
    if rows.exc is not None:
        out["excursions"] = {key: excursion_finish(v) for key, v in rows.exc.items()}
    if rows.rank is not None:
        rank = rq.rank
        out["rank_diagnostics"] = rows_summary(
            lambda a: _diag.chains_rank_diagnostics(a, probs=rank["probs"], max_lag=rank["max_lag"], n_chains=M),
            lambda v: rank_finish(v, mcmc_keep, rank["max_lag"]), rows.rank, _diag.summarise_rank)
    return out


def _opt(a, ptr=_dp):
    return ptr(a) if a is not None else None


def _reported_driver(rq):
    """The entry point a failure of the chain is reported under in "<driver> failed (rc)": the positional one (include/spamtree_fit.h)
    of the request's family.  None: the plain fit, which prints "MCMC has been interrupted." where the others raise."""
    if rq.crit:
        return "stm_mcmc_loo" if rq.loo else "stm_mcmc_criteria"
    if rq.pts is not None:
        return "stm_mcmc_points"
    if rq.M > 1:
        return "stm_mcmc_chains"
    if rq.rank is not None:
        return "stm_mcmc_ranked"
    if rq.exc is not None:
        return "stm_mcmc_excursions"
    return "stm_mcmc_diagnosed" if rq.diagnostics else None


def _check_groups(loo_groups, loo, y, indexing):
    """The labels of ``loo_groups`` as an int64 array after every check that needs no device (ValueError), or None."""
    if loo_groups is None:
        return None
    if not loo:
        raise ValueError("loo_groups labels the groups of the leave-group-out criteria: it needs loo=True")
    labels = np.asarray(loo_groups)
    y = np.asarray(y, dtype=np.float64).ravel()
    if labels.shape != y.shape:
        raise ValueError(f"loo_groups must be one integer label per row ({y.size}), got shape {labels.shape}")
    obs = np.isfinite(y)
    blocks = [np.asarray(ix, dtype=np.int64).ravel() for ix in indexing]
    rows = np.concatenate([ix for ix in blocks if obs[ix].any()] + [np.zeros(0, dtype=np.int64)])   # the blocks of the density
    _loo.group_index(labels, rows, obs)
    return np.ascontiguousarray(labels, dtype=np.int64)


def _check_request(y, X, mv_id, theta, limited_tree, mcmc_keep, sample_predicts, sample_w, seed, new_points, new_quantiles, criteria,
                   y_holdout, holdout_crps, diagnostics, diagnostics_max_lag, excursions, rank_diagnostics, chains, chain_seeds, chain_theta,
                   loo, psis=False, psis_draws=False):
    """Every check of spamtree_mv_mcmc's optional parts that needs no device (ValueError), and what they normalise: the chains'
    seeds and starts, the rank and excursion specs, the held-out values of the rows, the point set."""
    crit_cond = bool(criteria) or y_holdout is not None
    loo = bool(loo)
    if loo and limited_tree:
        raise ValueError("loo: limited_tree workloads are not supported (the leave-one-out criteria need the full chain factors)")
    psis = bool(psis) or bool(psis_draws)
    if psis and not loo:
        raise ValueError("psis smooths the leave-one-out weights: it needs loo=True")
    if psis and not 1 <= int(mcmc_keep) <= _lib.ST_PSIS_MAX_DRAWS:
        raise ValueError(f"psis: mcmc_keep = {int(mcmc_keep)} must lie in 1 .. {_lib.ST_PSIS_MAX_DRAWS} (the device keeps every saved draw's ratios)")
    crit = crit_cond or loo   # one driver: what excludes criteria excludes loo
    M = int(chains)
    if not 1 <= M <= _diag.MAX_CHAINS:
        raise ValueError(f"chains = {M} must lie in 1 .. {_diag.MAX_CHAINS}")
    keep_all = M * int(mcmc_keep)   # the columns of every per-draw array
    seeds = theta0 = None
    if M > 1:
        if crit:
            raise ValueError("chains and criteria / y_holdout are separate drivers (stm_mcmc_chains, stm_mcmc_criteria): one per call")
        if int(mcmc_keep) < 1 or keep_all > _diag.MAX_DRAWS:
            raise ValueError(f"chains: {M} x mcmc_keep = {keep_all} draws must lie in {M} .. {_diag.MAX_DRAWS} (what the device stores)")
        seeds = np.array([int(seed) + c for c in range(M)] if chain_seeds is None else [int(s) for s in chain_seeds], dtype=np.uint64)
        if seeds.shape != (M,):
            raise ValueError(f"chain_seeds must hold one seed per chain ({M})")
        if chain_theta is not None:
            theta0 = np.ascontiguousarray(chain_theta, dtype=np.float64)   # M x k in C order: k x M column-major
            if theta0.shape != (M, np.size(theta)):
                raise ValueError(f"chain_theta must be {M} x {np.size(theta)}: one start per chain")
    elif chain_seeds is not None or chain_theta is not None:
        raise ValueError("chain_seeds and chain_theta need chains > 1")
    rank = None
    if rank_diagnostics is not None and rank_diagnostics is not False:
        rank = {} if rank_diagnostics is True else dict(rank_diagnostics)
        unknown = set(rank) - {"probs", "thresholds", "sides", "max_lag", "thresholds_fun"}
        if unknown:
            raise ValueError(f"rank_diagnostics: unknown keys {sorted(unknown)}")
        if crit:
            raise ValueError("rank_diagnostics and criteria / y_holdout are separate drivers (stm_mcmc_ranked, stm_mcmc_criteria): one per call")
        if not _diag.MIN_DRAWS <= int(mcmc_keep) <= _diag.MAX_DRAWS:
            raise ValueError(f"rank_diagnostics: mcmc_keep = {int(mcmc_keep)} must lie in {_diag.MIN_DRAWS} .. {_diag.MAX_DRAWS} "
                             "(the series' length, and the draws the device keeps per row)")
        rank["max_lag"] = int(rank.get("max_lag", 0))
        rank["probs"], rank["thresholds"], rank["sides"] = _diag.check_rank_spec(rank.get("probs", ()), rank.get("thresholds", ()),
                                                                                  rank.get("sides"), rank["max_lag"])
    exc = None
    if excursions is not None:
        exc = dict(excursions)
        unknown = set(exc) - {"thresholds", "side", "mask", "band", "mask_new", "thresholds_fun", "mask_fun"}
        if unknown:
            raise ValueError(f"excursions: unknown keys {sorted(unknown)}")
        if crit:
            raise ValueError("excursions and criteria / y_holdout are separate drivers (stm_mcmc_excursions, stm_mcmc_criteria): one per call")
        exc["band"] = bool(exc.get("band", False))
        if exc.get("thresholds") is None and not exc["band"]:
            raise ValueError("excursions: neither thresholds nor band")
        _exc.check_keep(mcmc_keep, exc["band"])
        if exc.get("thresholds") is not None:   # the count, the values and the sides; the shapes once q is known
            entries = _exc.threshold_entries(exc["thresholds"])
            _exc.expand_thresholds([0.0] * len(entries), 1, exc.get("side", 1))
            for e in entries:
                _exc.expand_thresholds([e], np.size(e), 1)
    diagnostics = bool(diagnostics)
    if diagnostics:
        if crit:
            raise ValueError("diagnostics and criteria / y_holdout are separate drivers (stm_mcmc_diagnosed, stm_mcmc_criteria): one per call")
        if not _diag.MIN_DRAWS <= int(mcmc_keep) <= _diag.MAX_DRAWS:
            raise ValueError(f"diagnostics: mcmc_keep = {int(mcmc_keep)} must lie in {_diag.MIN_DRAWS} .. {_diag.MAX_DRAWS} "
                             "(the series' length, and the draws the device keeps per row)")
        if int(diagnostics_max_lag) < 0:
            raise ValueError("diagnostics_max_lag must not be negative (0: the default cap)")
    y_hold, want_crps = None, False
    if crit:
        if new_points is not None:
            raise ValueError("criteria and new_points are separate drivers (stm_mcmc_criteria, stm_mcmc_scored): one per call")
        y_hold = rows_holdout(y_holdout, y) if crit_cond else None
        if y_hold is not None and not (sample_predicts and sample_w):
            raise ValueError("y_holdout needs sample_predicts and sample_w: the NA rows' w would be stale")
        want_crps = bool(holdout_crps) and y_hold is not None
        if want_crps and int(mcmc_keep) > MAX_STORED_DRAWS:
            raise ValueError(f"y_holdout: the CRPS keeps mcmc_keep = {int(mcmc_keep)} draws per row on the device, at most "
                             f"{MAX_STORED_DRAWS} (holdout_crps=False scores without it)")
    pts = rb_spec = mix_spec = None
    q_out = int(np.unique(_i64(mv_id)).size)
    if new_points is not None:
        pts = _points_inputs(new_points, np.asarray(X).shape[1], q_out, new_quantiles)
        rb_spec = _exceed_inputs(new_points, pts, q_out)
        mix_spec = _mixture_inputs(new_points, pts, keep_all)
        if pts.crps and int(mcmc_keep) > MAX_STORED_DRAWS:
            raise ValueError(f"new_points: the CRPS keeps mcmc_keep = {int(mcmc_keep)} draws per point on the device, at most "
                             f"{MAX_STORED_DRAWS} (crps=False scores without it)")
    elif len(tuple(new_quantiles)):
        raise ValueError("new_quantiles needs new_points")
    n_fun = None if pts is None or pts.functionals is None else pts.functionals[0].size - 1
    if exc is not None:   # the shapes, still before any device call
        thr = sides = None
        if exc.get("thresholds") is not None:
            thr, sides = _exc.expand_thresholds(exc["thresholds"], q_out, exc.get("side", 1))
        exc["spec_rows"] = excursion_spec(thr, sides, _exc.check_mask(exc.get("mask"), int(np.asarray(y).size)), exc["band"])
        exc["T"] = 0 if thr is None else thr.shape[0]
        if pts is not None:
            exc["spec_new"] = excursion_spec(thr, sides, _exc.check_mask(exc.get("mask_new"), pts.coords.shape[0]), exc["band"])
            if n_fun is not None:
                tf = exc.get("thresholds_fun", exc.get("thresholds"))
                thr_f = sides_f = None
                if tf is not None:
                    thr_f, sides_f = _exc.expand_thresholds(tf, n_fun, exc.get("side", 1))
                exc["spec_fun"] = excursion_spec(thr_f, sides_f, _exc.check_mask(exc.get("mask_fun"), n_fun), exc["band"])
        elif any(exc.get(key) is not None for key in ("mask_new", "thresholds_fun", "mask_fun")):
            raise ValueError("excursions: mask_new, thresholds_fun and mask_fun need new_points")
    if rank is not None:   # the shapes, still before any device call
        rank["spec_rows"] = rank_spec(rank["probs"], rank["thresholds"], rank["sides"], rank["max_lag"], q_out)
        if pts is not None:
            rank["spec_new"] = rank_spec(rank["probs"], rank["thresholds"], rank["sides"], rank["max_lag"], q_out)
            if n_fun is not None:
                tf = rank.get("thresholds_fun")
                tf, sf = (rank["thresholds"], rank["sides"]) if tf is None else _diag.check_rank_spec((), tf, rank["sides"], 0)[1:]
                rank["spec_fun"] = rank_spec(rank["probs"], tf, sf, rank["max_lag"], n_fun)
        elif rank.get("thresholds_fun") is not None:
            raise ValueError("rank_diagnostics: thresholds_fun needs new_points")
    return SimpleNamespace(crit_cond=crit_cond, loo=loo, psis=psis, psis_draws=bool(psis_draws), crit=crit, M=M, keep_all=keep_all, seeds=seeds, theta0=theta0, rank=rank, exc=exc,
                           diagnostics=diagnostics, max_lag=int(diagnostics_max_lag), y_hold=y_hold, want_crps=want_crps, pts=pts, exceed=rb_spec, mixture=mix_spec, more=None)


def _row_parts(req, rq, n, q, mcmc_keep):
    """The parts of the request over the fit's own rows, set in ``req``, and their buffers: the row members of diagnostics, excursions
    and rank diagnostics (``ds``, ``xs``, ``rs``: _point_parts sets the points' and functionals' members), the criteria and the
    leave-one-out criteria (``criteria()``: their part of the result)."""
    out = SimpleNamespace(diag=None, exc=None, rank=None, ds=None, xs=None, rs=None, criteria=None)
    if rq.diagnostics:
        dw, sw = series_diag_buffers(n)
        dy, sy = series_diag_buffers(n)
        out.diag, out.ds = dict(w=dw, yhat=dy), _lib.StmDiagnostics(rq.max_lag, 1, sw, sy)
        req.diag = C.pointer(out.ds)
    if rq.exc is not None:
        exc = rq.exc
        out.xs = xs = _lib.StmExcursions()
        xs.want_rows = 1
        xs.rows_spec = exc["spec_rows"][0]
        xw, xs.rows_w = excursion_buffers(n, exc["T"], q, rq.keep_all, exc["band"])
        xy, xs.rows_yhat = excursion_buffers(n, exc["T"], q, rq.keep_all, exc["band"])
        out.exc = dict(w=xw, yhat=xy)
        req.exc = C.pointer(xs)
    if rq.rank is not None:
        out.rs = rs = _lib.StmRankDiagnostics()
        rs.want_rows = 1
        rs.rows_spec, _, n_prob, n_thr = rq.rank["spec_rows"]
        rw, rs.rows_w = rank_buffers(n, n_prob, n_thr)
        ry, rs.rows_yhat = rank_buffers(n, n_prob, n_thr)
        out.rank = dict(w=rw, yhat=ry)
        req.rk = C.pointer(rs)
    if rq.crit_cond:
        rows = {key: np.zeros(n) for key in ("lppd", "p_waic", "mean_ll", "mu_mean", "pit")}
        rows["crps"] = np.zeros(n) if (rq.want_crps and mcmc_keep > 0) else None
        tobs = np.zeros((len(_lib.ST_ROWS_OBS), q), order="F"); theld = np.zeros((len(_lib.ST_ROWS_HELD), q), order="F")
        n_obs, n_held = np.zeros(q, dtype=np.int64), np.zeros(q, dtype=np.int64)
        nacc = C.c_int64()
        cs = _lib.StmCriteria(_opt(rq.y_hold), int(rq.want_crps), *[_opt(rows[key]) for key in ("lppd", "p_waic", "mean_ll", "mu_mean", "pit", "crps")],
                              _dp(tobs), _dp(theld), _ip(n_obs), _ip(n_held), C.pointer(nacc))
        req.criteria = C.pointer(cs)
    if rq.loo:
        lrows = {key: np.zeros(n) for key in ("elpd_loo", "pit_loo", "mu_loo", "weight_ess")}
        ltot, ln_obs = np.zeros((len(_lib.ST_ROWS_LOO), q), order="F"), np.zeros(q, dtype=np.int64)
        lacc, lskip = C.c_int64(), C.c_int64()
        ls = _lib.StmLoo(*[_dp(lrows[key]) for key in ("elpd_loo", "pit_loo", "mu_loo", "weight_ess")], _dp(ltot), _ip(ln_obs),
                         C.pointer(lacc), C.pointer(lskip))
        if rq.psis:
            prow = {key: np.zeros(n) for key in ("khat", "elpd_psis", "pit_psis", "mu_psis", "weight_ess_psis")}
            prow.update(tail_len=np.zeros(n, dtype=np.int32), n_draws=np.zeros(n, dtype=np.int32))
            ptot, pn_obs = np.zeros((len(_lib.ST_ROWS_PSIS), q), order="F"), np.zeros(q, dtype=np.int64)
            pdraws = {key: np.zeros((mcmc_keep, n)) for key in ("t", "phi", "mu")} if rq.psis_draws else {}
            i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
            ps = _lib.StmLooPsis(_lib.StPsisOut(*[_dp(prow[key]) for key in ("khat", "elpd_psis", "pit_psis", "mu_psis", "weight_ess_psis")],
                                                i32(prow["tail_len"]), i32(prow["n_draws"])), _dp(ptot), _ip(pn_obs),
                                 *[_opt(pdraws.get(key)) for key in ("t", "phi", "mu")])
            ls.psis = C.pointer(ps)
        if rq.groups is not None:
            gcnt = [C.c_int64() for _ in range(3)]
            gidx = dict(label=np.zeros(n, dtype=np.int64), ptr=np.zeros(n + 1, dtype=np.int64), rows=np.zeros(n, dtype=np.int64))
            gout = {key: np.zeros(n) for key in ("elpd_lgo", "weight_ess", "mu_lgo", "pit_lgo", "khat", "elpd_psis", "weight_ess_psis")}
            gskip = np.zeros(n, dtype=np.int64)
            gtot, gby = np.zeros(len(_lib.ST_ROWS_LGO)), np.zeros((len(_lib.ST_ROWS_LGO_OUT), q), order="F")
            gs = _lib.StmLooGroups(_ip(rq.groups), *[C.pointer(v) for v in gcnt], _ip(gidx["label"]), _ip(gidx["ptr"]), _ip(gidx["rows"]),
                                   _dp(gout["elpd_lgo"]), _dp(gout["weight_ess"]), _ip(gskip), _dp(gout["mu_lgo"]), _dp(gout["pit_lgo"]),
                                   _dp(gtot), _dp(gby), _dp(gout["khat"]), _dp(gout["elpd_psis"]), _dp(gout["weight_ess_psis"]))
            ls.groups = C.pointer(gs)
        req.loo = C.pointer(ls)

    def groups():
        ng, nm = int(gcnt[0].value), int(gcnt[1].value)
        res = dict(label=gidx["label"][:ng].copy(), members=[gidx["rows"][gidx["ptr"][g]:gidx["ptr"][g + 1]].copy() for g in range(ng)],
                   n_pairs=int(gcnt[2].value), elpd_lgo=gout["elpd_lgo"][:ng].copy(), weight_ess=gout["weight_ess"][:ng].copy(),
                   n_skipped=gskip[:ng].copy(), mu_lgo=gout["mu_lgo"], pit_lgo=gout["pit_lgo"])
        tot = {key: float(gtot[i]) for i, key in enumerate(_lib.ST_ROWS_LGO)}
        tot["n_groups"] = int(tot["n_groups"])
        tot["by_outcome"] = {key: gby[i].copy() for i, key in enumerate(_lib.ST_ROWS_LGO_OUT)}
        res["totals"] = tot
        if rq.psis:
            res.update({key: gout[key][:ng].copy() for key in ("khat", "elpd_psis", "weight_ess_psis")})
        assert nm == sum(m.size for m in res["members"])
        return res

    def criteria():
        res = {}
        if rq.crit_cond:
            res = dict(rows, n_accumulated=int(nacc.value), totals=rows_criteria(tobs, theld, n_obs, n_held, have_crps=rows["crps"] is not None))
        if rq.loo:
            res["loo"] = dict(lrows, n_accumulated=int(lacc.value), n_skipped=int(lskip.value), totals=rows_loo_criteria(ltot, ln_obs))
            if rq.psis:
                res["loo"]["psis"] = dict(prow, totals=rows_psis_criteria(ptot, pn_obs), **pdraws)
            if rq.groups is not None:
                res["loo"]["groups"] = groups()
        return res
    if rq.crit:
        out.criteria = criteria
    return out


def _point_parts(lib, req, rq, rows, q, mcmc_keep, new_draws):
    """The parts of the request at the new points, set in ``req``, and their buffers: the point set, its functionals and scores, and
    the points' and functionals' members of ``rows.ds``, ``rows.xs`` and ``rows.rs``.  Returns the function that forms ``new`` of the
    result after the call."""
    pc, pmv, pan, pX, qs, labels, fun, ynew, want_crps = rq.pts
    rb = rq.exceed
    keep_all, has_X = rq.keep_all, pX is not None
    n_new = pc.shape[0]

    def outputs(m):
        """Of a set of m series: the per-draw arrays, the summaries, the quantiles of w and yhat, and the ten pointers to them in
        the order of stm_new_points and stm_functionals (yhat only with X, per-draw only with new_draws, quantiles only when asked)."""
        draws = {key: np.zeros((m, keep_all), order="F") if new_draws else None for key in ("w", "cond_mean", "cond_var")}
        draws["yhat"] = np.zeros((m, keep_all), order="F") if (new_draws and has_X) else None
        summ = {key: np.zeros(m) for key in ("mean", "var", "w_mean")}
        summ["yhat_mean"] = np.zeros(m) if has_X else None
        wq = np.zeros((m, qs.size), order="F")
        yq = np.zeros((m, qs.size), order="F") if has_X else None
        return draws, summ, wq, yq, [_opt(a) for a in (*draws.values(), *summ.values(), wq if qs.size else None, yq if qs.size else None)]
    draws, summ, wq, yq, ptrs = outputs(n_new)
    route = C.c_int32()
    groups = off = ccov = cov = None
    if labels is not None:
        groups, off = _joint_layout(labels)
        ccov = np.zeros((int(off[-1]), keep_all), order="F") if new_draws else None
        cov = np.zeros(int(off[-1]))
    ps = _lib.StmNewPoints(n_new, _dp(pc), _ip(pmv), _ip(pan), _opt(pX), _opt(labels, _ip), int(mcmc_keep) if (qs.size or want_crps) else 0,
                           _dp(qs), int(qs.size), *ptrs, C.pointer(route), _opt(ccov), _opt(cov))
    req.pts = C.pointer(ps)
    sets = dict(new=n_new)   # the sets of series a stored-draw summary can be asked of, and their sizes
    if fun is not None:
        sets["fun"] = nf = fun[0].size - 1
        fdraws, fsumm, fwq, fyq, fptrs = outputs(nf)
        fs = _lib.StmFunctionals(nf, _ip(fun[0]), _ip(fun[1]), _dp(fun[2]), *fptrs)
        req.fun = C.pointer(fs)
    if ynew is not None:      # crps from the draws the device keeps
        sc = dict(lpd=np.zeros(n_new), pit=np.zeros(n_new), crps=np.zeros(n_new) if (want_crps and mcmc_keep > 0) else None,
                  lpd_joint=np.zeros(len(groups)) if labels is not None else None)
        nsc, ndg = C.c_int64(), C.c_int64()
        ss = _lib.StmScores(_dp(ynew), _opt(sc["lpd"]), _opt(sc["pit"]), _opt(sc["crps"]), _opt(sc["lpd_joint"]), C.pointer(nsc), C.pointer(ndg))
        req.scores = C.pointer(ss)

    def stored(part, buffers):
        """The buffers of one stored-draw summary for every set, its <set>_w and <set>_yhat members of ``part`` pointing at them; yhat
        only with X.  ``buffers(set, m, want)`` is the summary's (dict, struct) of m series."""
        out = {}
        for name, m in sets.items():
            bw, sw = buffers(name, m, True)
            by, sy = buffers(name, m, has_X)
            setattr(part, name + "_w", sw)
            if sy is not None:
                setattr(part, name + "_yhat", sy)
            out[name] = dict(w=bw, yhat=by)
        return out
    summaries = []   # (result key, how a buffer dict is finished, the buffers by set)
    if rq.diagnostics:
        summaries.append(("diagnostics", lambda v: series_diag_finish(v, mcmc_keep, rq.max_lag),
                          stored(rows.ds, lambda name, m, want: series_diag_buffers(m, want))))
    if rq.exc is not None:
        exc, xs = rq.exc, rows.xs
        xs.new_spec = exc["spec_new"][0]
        shape = dict(new=(exc["T"], q))
        if fun is not None:
            xs.fun_spec = exc["spec_fun"][0]
            shape["fun"] = (int(xs.fun_spec.n_thr), 1)
        summaries.append(("excursions", excursion_finish,
                          stored(xs, lambda name, m, want: excursion_buffers(m, *shape[name], keep_all, exc["band"], want))))
    if rq.rank is not None:
        rank, rs, counts = rq.rank, rows.rs, {}
        rs.new_spec, _, *counts["new"] = rank["spec_new"]
        if fun is not None:
            rs.fun_spec, _, *counts["fun"] = rank["spec_fun"]
        summaries.append(("rank_diagnostics", lambda v: rank_finish(v, mcmc_keep, rank["max_lag"]),
                          stored(rs, lambda name, m, want: rank_buffers(m, *counts[name], want))))

    if rb is not None:        # the Rao-Blackwellised exceedance probabilities: a member of the excursions' part that reads no store
        rthr, rside, rthr_fun = rb

        def rb_bufs(m, want=True):
            d = dict(prob=np.zeros((rthr.shape[0], m)), prob_var=np.zeros((rthr.shape[0], m))) if want else None
            return d, (_lib.StRbOut(_dp(d["prob"]), _dp(d["prob_var"])) if want else _lib.StRbOut())
        rb_w, rb_sw = rb_bufs(n_new)
        rb_y, rb_sy = rb_bufs(n_new, has_X)
        rb_f, rb_sf = rb_bufs(sets.get("fun", 0), rthr_fun is not None)
        rb_acc = C.c_int64()
        rbs = _lib.StmRbExceed(rthr.shape[0], _dp(rthr), rside.ctypes.data_as(C.POINTER(C.c_int32)), _opt(rthr_fun), rb_sw, rb_sy, rb_sf,
                               C.pointer(rb_acc))
        if rows.xs is None:   # an exc whose only content is rb
            rows.xs = _lib.StmExcursions()
            req.exc = C.pointer(rows.xs)
        rows.xs.rb = C.pointer(rbs)

    mix = rq.mixture
    if mix is not None:       # the mixture predictive: travels beside the request (stm_fit_more)
        mprobs, mcrps = mix
        T = 0 if mprobs is None else mprobs.size

        def mix_bufs(m, want=True):
            want = want and T > 0
            qv, unc = (np.zeros((T, m)), C.c_int64()) if want else (None, None)
            return qv, unc, (_lib.StMixOut(_dp(qv), C.pointer(unc)) if want else _lib.StMixOut())
        mx_w, mx_uw, mx_sw = mix_bufs(n_new)
        mx_y, mx_uy, mx_sy = mix_bufs(n_new, has_X)
        mx_f, mx_uf, mx_sf = mix_bufs(sets.get("fun", 0), fun is not None)
        mx_crps, mx_spread = (np.zeros(n_new), np.zeros(n_new)) if mcrps else (None, None)
        mx_n = C.c_int64()
        mxs = _lib.StmMixture(_opt(mprobs), T, mx_sw, mx_sy, mx_sf, _opt(mx_crps), _opt(mx_spread), C.pointer(mx_n))
        rq.more = _lib.StmFitMore(C.pointer(mxs))
        rq.more_held = mxs

    def result():
        names, code = [], 1
        while lib.st_points_route_name(code) is not None:
            if route.value & (1 << (code - 1)):
                names.append(lib.st_points_route_name(code).decode())
            code += 1
        quantiles = lambda w_q, y_q: {float(x): (w_q[:, i].copy(), None if y_q is None else y_q[:, i].copy()) for i, x in enumerate(qs)}   # noqa: E731
        new = dict(summ, route=names, quantiles=quantiles(wq, yq))
        if new_draws:
            new.update(draws)
        if labels is not None:
            new.update(groups=groups, cov=_unpack_joint(cov, groups, off))
            if new_draws:
                new["cond_cov"] = [_unpack_joint(ccov[:, s], groups, off) for s in range(keep_all)]
        if fun is not None:
            new["functionals"] = dict(fsumm, quantiles=quantiles(fwq, fyq))
            if new_draws:
                new["functionals"].update(fdraws)
        if ynew is not None and mcmc_keep > 0:
            sc.update(n_scored=int(nsc.value), n_degenerate=int(ndg.value))
            lo_hi = (yq[:, int(np.argmin(qs))], yq[:, int(np.argmax(qs))]) if qs.size >= 2 else (None, None)
            sc["totals"] = score_totals(sc, ynew, pmv, q, *lo_hi)
            new["scores"] = sc
        if rb is not None and mcmc_keep > 0:
            new["exceed"] = dict(thr=rthr, side=rside, w=rb_w, yhat=rb_y, n_accumulated=int(rb_acc.value))
            if rb_f is not None:
                new["functionals"]["exceed"] = dict(thr=rthr_fun, side=rside, w=rb_f, n_accumulated=int(rb_acc.value))
        if mix is not None and mcmc_keep > 0:
            unc = lambda *u: sum(int(x.value) for x in u if x is not None)   # noqa: E731
            if T > 0:
                new["mixture"] = dict(probs=mprobs, w=mx_w, yhat=mx_y, n_stored=int(mx_n.value), n_unconverged=unc(mx_uw, mx_uy))
                if mx_f is not None:
                    new["functionals"]["mixture"] = dict(probs=mprobs, w=mx_f, n_stored=int(mx_n.value), n_unconverged=unc(mx_uf))
            if mcrps:
                new["scores"].update(crps_mixture=mx_crps, spread=mx_spread)
                tot = new["scores"]["totals"]
                for key, v in (("crps_mixture", mx_crps), ("spread", mx_spread)):
                    tot[key], tot["by_outcome"][key] = _mix.point_means(v, ynew, pmv, q)
        for key, finish, by_set in summaries:
            for name, bufs in by_set.items() if n_new > 0 else ():
                (new if name == "new" else new["functionals"])[key] = {k: finish(v) for k, v in bufs.items()}
        return new
    return result
