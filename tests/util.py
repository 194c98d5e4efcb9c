"""Shared synthetic-problem builders for the tests (inputs only; no product logic here), and what reads the oracle's state for them."""
import numpy as np

from spamtree_amd.topology import grid_coords, prepare


def csr_to_lists(ptr, idx):
    return [idx[ptr[i]:ptr[i + 1]].copy() for i in range(ptr.size - 1)]


def theta_layout(q):
    n_cbase = 3 if q > 2 else 1
    npars = 3 * q + n_cbase
    k = q * (q - 1) // 2
    return npars, n_cbase, k


def default_bounds(q, btmlim=1e-3, toplim=1e3):
    """set_unif_bounds of R/spamtree_fit.R:105-133."""
    npars, n_cbase, k = theta_layout(q)
    b = np.zeros((npars, 2))
    b[:, 0] = btmlim
    b[:, 1] = toplim
    if q > 1:
        b[1:q, 0] = -toplim
    if n_cbase == 3:
        b[npars - 2, :] = (btmlim, 1 - btmlim)
    if q > 1:
        vb = np.zeros((k, 2))
        vb[:, 0] = btmlim
        vb[:, 1] = toplim - btmlim
        b = np.vstack([b, vb])
    return b


def nice_theta(q):
    """A well-conditioned covariance parameter vector for tests (q=1: sigma^2=2.3, phi=6 as README.md:39-42)."""
    if q == 1:
        return np.array([2.3, 1.0, 1.0, 6.0])
    if q == 2:
        return np.array([1.0, 1.5, 0.3, 0.51, 3.0, 4.0, 5.0, 1.0])
    ai1 = np.array([1.0, -0.8, 1.3][:q] + [1.0] * max(0, q - 3))
    ai2 = np.linspace(0.3, 0.6, q)
    phi = np.linspace(3.0, 5.0, q)
    thetamv = np.array([1.2, 0.7, 4.0])
    k = q * (q - 1) // 2
    dvec = np.linspace(0.5, 1.5, k)
    return np.concatenate([ai1, ai2, phi, thetamv, dvec])


def distinct_theta(q):
    """nice_theta with every per-outcome and per-pair entry different (q >= 3): ai1 of mixed sign and distinct for outcomes
    4 to 6 (nice_theta gives them all 1.0), so an index mix-up among the later outcomes changes the covariance.  The dense K
    of the many-outcome shapes (n = 864 to 1280) has eigenvalues between 0.044 and 226."""
    assert 3 <= q <= 6
    ai1 = np.array([1.0, -0.8, 1.3, 0.9, -1.1, 0.7][:q])
    ai2 = np.linspace(0.3, 0.6, q)
    phi = np.linspace(3.0, 5.0, q)
    thetamv = np.array([1.2, 0.7, 4.0])
    dvec = np.linspace(0.5, 1.5, q * (q - 1) // 2)
    return np.concatenate([ai1, ai2, phi, thetamv, dvec])


def make_problem(side=25, q=1, seed=0, missing=0.0, coords=None, mv_id=None, p=3, random_coords=False, single_obs=None,
                 **tree_kw):
    """Synthetic inputs in the layout spamtree_mv_mcmc receives (R/spamtree_fit.R:327-362)."""
    rng = np.random.default_rng(seed)
    if coords is None:
        if random_coords:
            n0 = side * side
            base = rng.uniform(size=(n0, 2))
            coords = np.tile(base, (q, 1))
            mv_id = np.repeat(np.arange(1, q + 1), n0)
        else:
            coords, mv_id = grid_coords(side, q)
    n = coords.shape[0]
    X = rng.standard_normal((n, p))
    beta = np.array([-1.0, 0.5, 1.0, 0.25, -0.3, 0.7, -0.6, 0.4][:p])      # p = 1..8 (the library's limit)
    f = np.zeros(n)
    for _ in range(6):
        kx, ky, ph = rng.uniform(1, 6), rng.uniform(1, 6), rng.uniform(0, 6.28)
        f += rng.normal() * np.sin(kx * coords[:, 0] + ky * coords[:, 1] + ph + 0.7 * mv_id)
    y = X @ beta + f + np.sqrt(0.1) * rng.standard_normal(n)
    if np.ndim(missing) > 0:      # per-outcome drop probabilities (config #5: 0.1, 0.3, 0.5 -- imbalanced)
        y = y.copy()
        y[rng.uniform(size=n) < np.asarray(missing, dtype=np.float64)[np.asarray(mv_id) - 1]] = np.nan
    elif missing > 0:
        y = y.copy()
        y[rng.uniform(size=n) < missing] = np.nan
    if single_obs is not None:    # outcome `single_obs` (1-based) keeps exactly one observed row, its first finite one
        y = y.copy()
        rows = np.nonzero((np.asarray(mv_id) == single_obs) & np.isfinite(y))[0]
        y[rows[1:]] = np.nan
    limited_tree = bool(tree_kw.get("limited_tree", False))
    topo = prepare(y, coords, mv_id, **tree_kw)
    s = topo.sort_ix
    Z = np.zeros((n, q))
    Z[np.arange(n), topo.mv_id - 1] = 1.0
    return dict(
        topo=topo, y=y[s], X=X[s], Z=Z, coords=topo.coords, mv_id=topo.mv_id, blocking=topo.blocking,
        gix_block=topo.gix_block, res_is_ref=topo.res_is_ref,
        parents=csr_to_lists(topo.parents_ptr, topo.parents_idx),
        children=csr_to_lists(topo.children_ptr, topo.children_idx),
        block_names=topo.block_names, block_groups=topo.block_groups,
        indexing=csr_to_lists(topo.indexing_ptr, topo.indexing_idx),
        q=q, p=p, n=n, beta_true=beta, bounds=default_bounds(q), theta=nice_theta(q), limited_tree=limited_tree)


def oracle_model(pb, theta=None, beta=None, tausq=0.1, w=None, **kw):
    from oracle.spamtree_oracle import SpamTreeMV
    theta = pb["theta"] if theta is None else theta
    beta = np.zeros(pb["p"]) if beta is None else beta
    w = np.zeros(pb["n"]) if w is None else w
    beta, tausq = np.asarray(beta, dtype=np.float64), np.asarray(tausq, dtype=np.float64)
    om = SpamTreeMV(pb["y"], pb["X"], pb["Z"], pb["coords"], pb["mv_id"], pb["blocking"], pb["gix_block"],
                    pb["res_is_ref"], pb["parents"], pb["children"], pb.get("limited_tree", False), pb["block_names"],
                    pb["block_groups"], pb["indexing"], w, beta[:, 0] if beta.ndim == 2 else beta, theta,
                    1.0 / float(tausq.ravel()[0]), **kw)
    if beta.ndim == 2 or tausq.ndim > 0:
        per_outcome(om, beta if beta.ndim == 2 else None, tausq if tausq.ndim > 0 else None)
    return om


def per_outcome(om, Bcoeff=None, tausq=None):
    """Gives an oracle model one coefficient column (Bcoeff p x q) and one noise variance (tausq, q values) per outcome, as
    its beta and tausq updates leave them (the constructor takes one of each for all outcomes)."""
    if Bcoeff is not None:
        om.Bcoeff = np.array(Bcoeff, dtype=np.float64)
        for j in range(om.q):
            om.XB[om.ix_by_q[j]] = om.X[om.ix_by_q[j]] @ om.Bcoeff[:, j]
    if tausq is not None:
        om.tausq_inv = 1.0 / np.asarray(tausq, dtype=np.float64)
        for j in range(om.q):
            om.tausq_inv_long[om.ix_by_q[j]] = om.tausq_inv[j]


def level_failure_problem(pb, level, n_relabel=12, seed=0, blocks=None):
    """A copy of `pb` (q <= 5 outcomes) in which some observed rows of ONE level (index into the sorted level labels, as
    the oracle's groups and st_level_info count them; a sequence: of each of these levels) are relabelled as outcome q + 1,
    with Z, the bounds and theta extended.  Nothing else changes: the tree, the block widths and the chain lengths are those
    of `pb`.  `blocks`: take the rows from these blocks of the level only (a multi-rank test keeps them inside one rank's
    subtrees).  Returns
    (problem, fail), the problem with theta = nice_theta(q + 1), and fail =
      theta_bad     the same theta with the Dmat entries towards the new outcome negative (finite, outside the bounds): the
                    cross-covariance between the new outcome and the others is inflated about tenfold, so exactly the
                    conditional variances of that level's relabelled rows go negative, while shallower levels hold no row of
                    the new outcome and see the same covariances as before;
      tausq_inv_ok / tausq_inv_bad   per-outcome tausq^-1; the bad one is negative for the new outcome only, so only that
                    level's posterior precisions are indefinite;
      levels, rows  the levels and the relabelled rows."""
    from oracle.spamtree_oracle import vec_to_symmat
    q = int(pb["q"])
    assert q <= 5
    labels = np.unique(pb["block_groups"])
    levels = [int(level)] if np.ndim(level) == 0 else [int(g) for g in level]
    rng = np.random.default_rng(seed)
    pick = []
    for g in levels:
        in_level = [u for u in range(len(pb["indexing"])) if pb["block_groups"][u] == labels[g]]
        if blocks is not None:
            assert set(blocks) <= set(in_level)
            in_level = list(blocks)
        rows = np.concatenate([pb["indexing"][u] for u in in_level])
        rows = rows[np.isfinite(pb["y"][rows])]
        pick.append(rng.choice(rows, min(n_relabel, rows.size), replace=False))
    pick = np.sort(np.concatenate(pick))
    mv = np.asarray(pb["mv_id"]).copy()
    mv[pick] = q + 1
    Z = np.zeros((pb["n"], q + 1))
    Z[np.arange(pb["n"]), mv - 1] = 1.0
    good = nice_theta(q + 1)
    npars, n_cbase, k = theta_layout(q + 1)
    to_new = vec_to_symmat(np.arange(1.0, k + 1))[q, :q].astype(np.int64) - 1     # positions of Dmat[q, 0..q-1] in the vector
    bad = good.copy()
    # q + 1 = 2: psi = v + 1; q + 1 > 2: psi = (1 + a v)^beta with a = thetamv[0].  1 + a v = 0.1 in both
    bad[npars + to_new] = -0.9 if q + 1 == 2 else -0.9 / good[3 * (q + 1)]
    ok_t = np.full(q + 1, 5.0)
    bad_t = ok_t.copy()
    bad_t[q] = -1e6
    out = dict(pb, mv_id=mv, Z=Z, q=q + 1, bounds=default_bounds(q + 1), theta=good)
    return out, dict(theta_bad=bad, tausq_inv_ok=ok_t, tausq_inv_bad=bad_t, levels=levels, rows=pick)


def oracle_phase_a_failure(om, data):
    """Runs the oracle's phase A on `data` and returns (errtype, level): the oracle returns after the first level with an
    error, so the failing level is the deepest one whose blocks it visited -- read from its per-block log-density
    components, cleared beforehand.  (-1, None) where it succeeds."""
    data.loglik_w_comps[:] = 0.0
    with np.errstate(all="ignore"):
        if om.get_loglik_comps_w(data):
            return -1, None
    seen = [g for g, us in enumerate(om.u_by_block_groups) if any(data.loglik_w_comps[u] != 0.0 for u in us)]
    return om.last_errtype, max(seen)


def oracle_sweep_failing_levels(om):
    """The levels holding a block whose posterior precision, rebuilt from the oracle's per-block caches and its current
    tausq^-1, is not positive definite: where a sweep fails."""
    groups = om.u_by_block_groups
    pd = om.param_data
    bad = []
    for g, us in enumerate(groups):
        for u in us:
            iu = om.indexing[u]
            if om.res_is_ref[g] == 1:
                S = pd.w_cond_prec[u].copy()
                if om.children[u].size:
                    S += np.sum(pd.Sigi_children[u], axis=2)
                S[np.diag_indices_from(S)] += om.tausq_inv_long[iu]
                ok = np.all(np.isfinite(S)) and np.linalg.eigvalsh(np.triu(S) + np.triu(S, 1).T).min() > 0
            else:
                ok = all(pd.w_cond_prec_noref[u][ix][0, 0] + om.tausq_inv_long[iu[ix]] > 0 for ix in range(iu.size))
            if not ok:
                bad.append(g)
                break
    return bad


def strip_coords(nx, ny, q, width=0.02):
    """An nx x ny grid on the thin strip [0,1] x [0,width], replicated per outcome: with K = (2, 1) the tree splits one axis
    only, so it gets DEEP (long ancestor chains) with few rows -- chains of config #4 / #5 length at oracle-friendly sizes."""
    xs = np.linspace(0.0, 1.0, nx)
    ys = np.linspace(0.0, width, ny)
    g = np.stack(np.meshgrid(xs, ys, indexing="ij"), axis=-1).reshape(-1, 2)
    return np.tile(g, (q, 1)), np.repeat(np.arange(1, q + 1), nx * ny)


def visible_gpus():
    """GPUs torch sees, asked in a child process.  torch bundles its own HIP / HSA runtimes: once the library has loaded the
    system ones, importing torch loads a second set next to them, and after torch's set has initialised the library's finds
    no device.  So a test process that uses the library never initialises torch's runtime itself."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.device_count())"], capture_output=True,
                       text=True, timeout=300, check=True)
    return int(r.stdout.split()[-1])


def problem_arrays(pb):
    """The arrays of a make_problem result in the layout st_problem points at (int64 ids, column-major X and coords).  The
    caller may corrupt an entry before handing them to st_problem_struct."""
    from spamtree_amd.model import _f64, _i64, _lists_to_csr
    a = dict(n_all=int(pb["n"]), d=2, q=int(pb["q"]), p=int(pb["p"]), y=_f64(pb["y"]).copy(),
             X=np.asfortranarray(pb["X"], dtype=np.float64).copy(order="F"),
             coords=np.asfortranarray(pb["coords"], dtype=np.float64).copy(order="F"), mv_id=_i64(pb["mv_id"]).copy(),
             res_is_ref=_i64(pb["res_is_ref"]).copy(), block_names=_i64(pb["block_names"]).copy(),
             block_groups=_i64(pb["block_groups"]).copy())
    for name in ("indexing", "parents", "children"):
        a[name + "_ptr"], a[name + "_idx"] = _lists_to_csr(pb[name])
    return a


def st_problem_struct(a):
    """st_problem over the arrays of problem_arrays (which must outlive it); a None array becomes a null pointer."""
    from spamtree_amd import _lib

    def ptr(x, ty):
        return x.ctypes.data_as(ty) if x is not None else ty()
    return _lib.StProblem(a["n_all"], a["d"], a["q"], a["p"], int(a["res_is_ref"].size), int(a["block_names"].size),
                          ptr(a["y"], _lib.c_dp), ptr(a["X"], _lib.c_dp), ptr(a["coords"], _lib.c_dp), ptr(a["mv_id"], _lib.c_ip),
                          *[ptr(a[k], _lib.c_ip) for k in ("res_is_ref", "block_names", "block_groups", "indexing_ptr",
                                                           "indexing_idx", "parents_ptr", "parents_idx", "children_ptr",
                                                           "children_idx")])
