"""Simulation from the tree prior on the device: exact draws of the latent field and the outcomes of the model the package
fits, at any size the fit runs at (st_simulate: one factorisation, then one root-to-leaf sweep per batch of up to 16 draws).

    w ~ N(0, C_DAG(theta)),   y = X beta_j + w + sqrt(tausq_j) eps        (j = the row's outcome)

C_DAG is the covariance of the tree's DAG factorisation (the model the sampler targets), not the dense GP's.
"""
import math

import numpy as np

from ._lib import ST_MAX_P
from .synthetic import theta_layout
from .topology import prepare

_BATCH = 16


def _check_inputs(coords, theta, mv_id, X, beta, tausq, n_draws):
    coords = np.asarray(coords, dtype=np.float64)
    if coords.ndim != 2 or coords.shape[1] != 2 or coords.shape[0] < 1:
        raise ValueError("coords must be an n x 2 array")
    if not np.isfinite(coords).all():
        raise ValueError("coords must be finite")
    n = coords.shape[0]
    mv_id = np.ones(n, dtype=np.int64) if mv_id is None else np.asarray(mv_id).reshape(-1)
    if mv_id.size != n:
        raise ValueError("mv_id must have one entry per row")
    if not np.all(np.equal(np.mod(mv_id, 1), 0)):
        raise ValueError("mv_id must hold integer margins")
    mv_id = mv_id.astype(np.int64)
    q = int(mv_id.max()) if n else 0
    if mv_id.min() < 1 or not np.array_equal(np.unique(mv_id), np.arange(1, q + 1)):
        raise ValueError("mv_id must use every margin 1..q")
    npars, _, k = theta_layout(q)
    theta = np.asarray(theta, dtype=np.float64).reshape(-1)
    if theta.size != npars + k:
        raise ValueError(f"theta must have {npars + k} entries for q = {q} (synthetic.theta_layout)")
    if not np.isfinite(theta).all():
        raise ValueError("theta must be finite")
    if X is None:
        X = np.zeros((n, 1))
        beta = np.zeros((1, q)) if beta is None else beta
        if np.any(np.asarray(beta, dtype=np.float64) != 0):
            raise ValueError("beta without X")
        beta = np.zeros((1, q))
    X = np.asarray(X, dtype=np.float64)
    if X.ndim == 1:
        X = X[:, None]
    if X.ndim != 2 or X.shape[0] != n or not 1 <= X.shape[1] <= ST_MAX_P:
        raise ValueError(f"X must be n x p with 1 <= p <= {ST_MAX_P}")
    if not np.isfinite(X).all():
        raise ValueError("X must be finite")
    p = X.shape[1]
    beta = np.zeros(p) if beta is None else np.asarray(beta, dtype=np.float64)
    if beta.ndim == 1:
        if beta.size != p:
            raise ValueError("beta must have p entries (or be p x q)")
        beta = np.repeat(beta[:, None], q, axis=1)
    if beta.shape != (p, q) or not np.isfinite(beta).all():
        raise ValueError("beta must be finite, p or p x q")
    tausq = np.full(q, 0.1) if tausq is None else np.asarray(tausq, dtype=np.float64).reshape(-1)
    if tausq.size == 1:
        tausq = np.full(q, float(tausq[0]))
    if tausq.size != q or not np.isfinite(tausq).all() or (tausq <= 0).any():
        raise ValueError("tausq must be positive and finite, a scalar or one per margin")
    if int(n_draws) != n_draws or n_draws < 1:
        raise ValueError("n_draws must be a positive integer")
    return coords, mv_id, q, theta, X, beta, tausq


def simulate(coords, theta, mv_id=None, X=None, beta=None, tausq=None, n_draws=1, seed=2021, device=0, cell_size=25, K=None,
             start_level=0, tree_depth=math.inf, last_not_reference=True, cherrypick_same_margin=True,
             cherrypick_group_locations=True, limited_tree=False, mvbias=0.0, force_generic=False):
    """Draw ``n_draws`` latent fields and outcome vectors from the tree prior at ``coords`` (n x 2; ``mv_id``: 1-based
    margins, default all 1).  ``theta`` in the reference's layout (synthetic.theta_layout(q)); ``X`` n x p (None: no
    regressors, y = w + noise), ``beta`` p or p x q, ``tausq`` scalar or q.  The tree is built with every row observed and
    the tree arguments of ``topology.prepare``.  Draw d uses Philox iteration d (streams 8 / 9) under ``seed``.

    Returns dict(w, y, theta, beta, tausq, topo, route) with w and y n x n_draws in the caller's row order; ``route`` names
    the kernels of the sweep.  A covariance whose factorisation fails raises SpamTreeError with st_factor's code."""
    no_x = X is None
    coords, mv_id, q, theta, X, beta, tausq = _check_inputs(coords, theta, mv_id, X, beta, tausq, n_draws)
    from .model import SpamTreeError, SpamTreeMV, _dp
    n = coords.shape[0]
    topo = prepare(np.zeros(n), coords, mv_id, cell_size=cell_size, K=K, start_level=start_level, tree_depth=tree_depth,
                   last_not_reference=last_not_reference, cherrypick_same_margin=cherrypick_same_margin,
                   cherrypick_group_locations=cherrypick_group_locations, limited_tree=limited_tree, mvbias=mvbias)
    s = topo.sort_ix
    Z = np.zeros((n, q))
    Z[np.arange(n), topo.mv_id - 1] = 1.0
    hm = SpamTreeMV(np.zeros(n), X[s], Z, topo.coords, topo.mv_id, topo.blocking, topo.gix_block, topo.res_is_ref,
                    (topo.parents_ptr, topo.parents_idx), (topo.children_ptr, topo.children_idx), limited_tree,
                    topo.block_names, topo.block_groups, (topo.indexing_ptr, topo.indexing_idx), np.zeros(n),
                    np.zeros(X.shape[1]), theta, 1.0, device=device, force_generic=force_generic)
    try:
        hm.beta_update(np.asfortranarray(beta))
        hm.tausq_inv = 1.0 / tausq
        hm._check(hm.lib.st_set_tausq_inv(hm.h, _dp(hm.tausq_inv)))
        hm.theta_update(0, theta)
        if not hm.get_loglik_comps_w(0):
            raise SpamTreeError(f"st_factor failed with code {hm.last_errtype}: the covariance is not positive definite "
                                "on some block")
        nd = int(n_draws)
        w = np.empty((n, nd))
        y = np.empty((n, nd))
        for d0 in range(0, nd, _BATCH):
            b = min(_BATCH, nd - d0)
            wb, yb = hm.simulate(b, seed=seed, it=d0)
            w[s, d0:d0 + b] = wb
            y[s, d0:d0 + b] = yb
        route = hm.simulate_info(1)["routes"]
    finally:
        hm.close()
    return dict(w=w, y=y, theta=theta, beta=beta, tausq=tausq, topo=topo, route=route, coords=coords, mv_id=mv_id,
                X=None if no_x else X)


def as_workload(sim, draw=0, missing=None, seed=2021, cell_size=25, limited_tree=False, device=None):
    """One draw of :func:`simulate` as the dict ``synthetic.make_workload`` returns (rows sorted, tree rebuilt on the mask),
    ready for ``fit.spamtree_mv_mcmc`` / ``predict.fit_predict``.  ``missing``: None or per-margin NA rates in [0, 1)."""
    if not isinstance(sim, dict) or "y" not in sim or "coords" not in sim:
        raise ValueError("sim must be the dict simulate returns")
    y_all = np.asarray(sim["y"], dtype=np.float64)
    if y_all.ndim != 2 or int(draw) != draw or not 0 <= draw < y_all.shape[1]:
        raise ValueError("draw out of range")
    coords, mv_id = np.asarray(sim["coords"]), np.asarray(sim["mv_id"], dtype=np.int64)
    n = coords.shape[0]
    q = int(mv_id.max())
    y = y_all[:, int(draw)].copy()
    if missing is not None:
        pr = np.asarray(missing, dtype=np.float64).reshape(-1)
        if pr.size == 1:
            pr = np.full(q, float(pr[0]))
        if pr.size != q or not np.isfinite(pr).all() or (pr < 0).any() or (pr >= 1).any():
            raise ValueError("missing must hold one rate in [0, 1) per margin")
        rng = np.random.default_rng(seed)
        y[rng.uniform(size=n) < pr[mv_id - 1]] = np.nan
    X = sim.get("X")
    X = np.zeros((n, 1)) if X is None else np.asarray(X)
    beta = np.asarray(sim["beta"])
    topo = prepare(y, coords, mv_id, cell_size=cell_size, limited_tree=limited_tree, device=device)
    s = topo.sort_ix
    Z = np.zeros((n, q))
    Z[np.arange(n), topo.mv_id - 1] = 1.0
    from .synthetic import default_bounds
    return dict(topo=topo, y=y[s], X=X[s], Z=Z, coords=topo.coords, mv_id=topo.mv_id, blocking=topo.blocking,
                gix_block=topo.gix_block, res_is_ref=topo.res_is_ref,
                parents=(topo.parents_ptr, topo.parents_idx), children=(topo.children_ptr, topo.children_idx),
                block_names=topo.block_names, block_groups=topo.block_groups,
                indexing=(topo.indexing_ptr, topo.indexing_idx), n=n, q=q, p=X.shape[1],
                bounds=default_bounds(q), theta=np.asarray(sim["theta"]).copy(), beta_true=beta[:, 0].copy(),
                w_true=np.asarray(sim["w"])[s, int(draw)])
