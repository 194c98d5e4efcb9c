"""GPU: joint prediction of groups of new points (st_points_set_joint, st_points_predict_joint, the pair summaries).

A joint group is 1..16 new points on one conditioning chain S; its conditional mean, covariance Sigma = K_GG - K_GS K_SS^-1 K_SG,
Cholesky factor and draw are checked against the dense identities, on every route (k_points_joint_mfma<128> / <256>,
k_points_joint_generic), together with the independence from the layout, the zero-pivot rule, the refusals, the summaries
over saved iterations and the whole path through the fit.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests.test_gpu_predict_points import _deep4, _deep5, args_of, fitted, hip_model, new_points, relerr
from tests.util import distinct_theta, make_problem

pytestmark = pytest.mark.gpu

ST_ERR_USAGE, ST_ERR_UNSUPPORTED = -1, -4
MFMA = {"k_points_joint_mfma<128>", "k_points_joint_mfma<256>"}
SIZES = (1, 2, 5, 6, 6, 6, 16)
U = 2.0 ** -53

dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))    # noqa: E731


def is_reference(topo, b):
    from spamtree_amd.predict import conditioning_set
    return int(b) in conditioning_set(topo, int(b))


def some_reference_anchors(topo, anchor, labels, both=True):
    """Every third group moves to the reference block its chain ends in (the last parent of a non-reference anchor): the same
    chain, reached through the other branch of the anchor rule.  both: the set must then hold anchors of either kind (the deep
    strips locate every point on a reference block already)."""
    from spamtree_amd.predict import conditioning_set
    anchor = anchor.copy()
    for lab in np.unique(labels)[::3]:
        m = labels == lab
        anchor[m] = conditioning_set(topo, int(anchor[m][0]))[-1]
    kinds = {is_reference(topo, b) for b in np.unique(anchor)}
    assert kinds == {True, False} if both else True in kinds, kinds
    return anchor


def site_set(pb, n_sites, seed, both=True):
    """The q outcomes at n_sites random sites: coords, mv, labels (one joint group per site), anchors."""
    from spamtree_amd.predict import group_sites, locate
    pts, _ = new_points(pb, n_sites, seed)
    q = pb["q"]
    coords, mv = np.repeat(pts, q, axis=0), np.tile(np.arange(1, q + 1), n_sites)
    labels = group_sites(coords)
    anchor = some_reference_anchors(pb["topo"], locate(pb["topo"], coords, mv, device=0, joint=labels), labels, both)
    return coords, mv, labels, anchor


def run_set(pb, n, seed):
    """n random points in the caller's random order, cut into joint groups of SIZES over the points of one anchor (each anchor's
    run starts at another place of the cycle, so that a 16 fits): slots with padding, and groups that fill a whole wave tile."""
    from spamtree_amd.predict import locate
    pts, mv = new_points(pb, n, seed)
    anchor = locate(pb["topo"], pts, mv, device=0)
    labels = np.zeros(n, dtype=np.int64)
    lab = 0
    for r, b in enumerate(np.unique(anchor)):
        idx = np.nonzero(anchor == b)[0]
        k, at = r, 0
        while at < idx.size:
            g = SIZES[k % len(SIZES)]
            labels[idx[at:at + g]] = lab
            lab, k, at = lab + 1, k + 1, at + g
    sizes = set(np.bincount(labels).tolist())
    assert {1, 2, 5, 6, 16} <= sizes, sizes
    return pts, mv, labels, some_reference_anchors(pb["topo"], anchor, labels)


def dense_moments(pb, w, pts, mv, anchor, groups):
    """Per group: K_GS K_SS^-1 w_S, K_GG - K_GS K_SS^-1 K_SG, the rows of S and diag K_GG."""
    from oracle.spamtree_oracle import CovarianceParams, Covariancef
    from spamtree_amd.predict import conditioning_set
    topo = pb["topo"]
    cp = CovarianceParams(2, pb["q"])
    cp.transform(pb["theta"])
    allc = np.vstack([topo.coords, pts])
    allv = np.concatenate([topo.mv_id - 1, mv - 1])
    n = pb["n"]
    res = []
    for g in groups:
        S = np.concatenate([topo.indexing(int(b)) for b in conditioning_set(topo, int(anchor[g[0]]))])
        Kss = Covariancef(allc, allv, S, S, cp, same=True)
        Ksg = Covariancef(allc, allv, S, n + g, cp)
        Kgg = Covariancef(allc, allv, n + g, n + g, cp)
        sol = np.linalg.solve(Kss, np.column_stack([w[S], Ksg]))
        res.append((Ksg.T @ sol[:, 0], Kgg - Ksg.T @ sol[:, 1:], S.size, np.diag(Kgg).copy()))
    return res


def blocks(x):
    """The g x g blocks of a cov / chol output, which is a list or, when all groups have one size, a stacked array."""
    return list(x)


def check_dense(pb, hm, pts, mv, labels, anchor, routes):
    hm.set_points(pts, mv, anchor, joint=labels)
    out = hm.predict_points(mode=1)
    assert set(hm.points_info()["routes"]) <= routes and hm.points_info()["routes"], hm.points_info()
    assert np.array_equal(out["w"], out["mean"])
    ref = dense_moments(pb, hm.get_w(), pts, mv, anchor, hm.joint_groups)
    mean = np.zeros(pts.shape[0])
    for g, (m, _, _, _) in zip(hm.joint_groups, ref):
        mean[g] = m
    print("mean relerr", relerr(out["mean"], mean))
    assert relerr(out["mean"], mean) <= 1e-9
    worst = max(np.abs(c - r[1]).max() / max(1.0, np.abs(r[1]).max()) for c, r in zip(blocks(out["cov"]), ref))
    print("cov err", worst)
    assert worst <= 1e-9
    for c in blocks(out["cov"]):
        assert np.array_equal(c, c.T)
    return out


@functools.lru_cache(maxsize=None)
def small(q):
    if q == 6:      # 54-row blocks of six outcomes, chains of <= 128 rows, every per-outcome and per-pair parameter different
        pb = make_problem(side=12, q=q, seed=5, missing=0.1, cell_size=9)
        pb["theta"] = distinct_theta(q)
        return pb
    return make_problem(side=20, q=q, seed=5, missing=0.1)


@pytest.mark.parametrize("q", [1, 3, 6])
def test_conditional_moments_equal_the_dense_identity(q):
    """25-row blocks (sub-panels of 16 + 9 rows: the stale rows of a short sub-panel must not reach the Gram); q = 3: 100 sites
    of 3 outcomes, q = 6: 60 sites of all six outcomes (g = 6, a 6 x 6 predictive covariance per site), q = 1: groups of 1, 2,
    5, 6 and 16 same-anchor points.  This is also the check of the MFMA operand layout."""
    pb = small(q)
    hm = fitted(pb, 6)
    points = site_set(pb, 60 if q == 6 else 100, 7) if q >= 3 else run_set(pb, 300, 7)
    if q == 6:
        assert np.all(np.bincount(points[2]) == 6)
    check_dense(pb, hm, *points, MFMA)
    hm.close()


@pytest.mark.parametrize("case", ["deep5", "deep4", "force_generic"])
def test_every_route_equals_the_dense_identity(case):
    """k_points_joint_mfma<256> (chains of 129-256 rows), k_points_joint_generic (444-475 rows, and a force_generic handle)."""
    pb = {"deep5": _deep5, "deep4": _deep4, "force_generic": lambda: small(3)}[case]()
    rng = np.random.default_rng(6)
    hm = hip_model(pb, w=rng.standard_normal(pb["n"]), beta=rng.standard_normal(pb["p"]), force_generic=case == "force_generic")
    assert hm.get_loglik_comps_w(0)
    want = {"deep5": {"k_points_joint_mfma<256>"}, "deep4": {"k_points_joint_generic"}, "force_generic": {"k_points_joint_generic"}}[case]
    check_dense(pb, hm, *site_set(pb, 40, 8, both=case == "force_generic"), want)
    hm.close()


@pytest.mark.parametrize("q", [1, 3])
def test_mfma_and_generic_routes_agree(q):
    pb = small(q)
    pts, mv, labels, anchor = site_set(pb, 100, 7) if q == 3 else run_set(pb, 300, 7)
    z = np.random.default_rng(12).standard_normal(pts.shape[0])
    res = {}
    for fg in (False, True):
        rng = np.random.default_rng(6)
        hm = hip_model(pb, w=rng.standard_normal(pb["n"]), beta=rng.standard_normal(pb["p"]), force_generic=fg)
        assert hm.get_loglik_comps_w(0)
        hm.set_points(pts, mv, anchor, joint=labels)
        res[fg] = hm.predict_points(mode=0, z=z)
        assert set(hm.points_info()["routes"]) <= (MFMA if not fg else {"k_points_joint_generic"})
        hm.close()
    for key in ("mean", "w", "cov_packed", "chol_packed"):
        print(key, relerr(res[False][key], res[True][key]))
        assert relerr(res[False][key], res[True][key]) <= 1e-12, key


def test_factor_and_draw():
    """|L L' - Sigma|_ab <= (g + 1) 2^-52 sqrt(Sigma_aa Sigma_bb) (the backward error of a Cholesky factorisation; L L' formed in
    extended precision), w = mean + L z for the caller's z and for the default stream 6, yhat as test_default_streams_6_and_7."""
    from spamtree_amd.rng import HostRng
    pb = small(1)
    hm = fitted(pb, 6)
    pts, mv, labels, anchor = run_set(pb, 300, 7)
    n = pts.shape[0]
    hm.set_points(pts, mv, anchor, joint=labels)
    z = np.random.default_rng(12).standard_normal(n)
    out = hm.predict_points(mode=0, z=z)
    for g, S, L in zip(hm.joint_groups, blocks(out["cov"]), blocks(out["chol"])):
        assert np.all(np.diag(L) > 0) and np.array_equal(L, np.tril(L))
        Lx = L.astype(np.longdouble)
        d = np.sqrt(np.diag(S))
        assert np.all(np.abs((Lx @ Lx.T).astype(np.float64) - S) <= (g.size + 1) * 2.0 ** -52 * np.outer(d, d)), g
        assert np.abs(out["w"][g] - out["mean"][g] - L @ z[g]).max() <= 1e-12 * np.abs(out["w"]).max()
    seed, it = 123456789, 5
    o2 = hm.predict_points(mode=0, seed=seed, it=it)
    zz = HostRng(seed).point_normals(it, n)
    assert np.array_equal(o2["chol_packed"], out["chol_packed"]) and np.array_equal(o2["mean"], out["mean"])
    for g, L in zip(hm.joint_groups, blocks(o2["chol"])):
        assert np.abs(o2["w"][g] - o2["mean"][g] - L @ zz[g]).max() <= 1e-12 * np.abs(o2["w"]).max()
    hm.close()
    pb = make_problem(side=20, q=3, seed=14, missing=0.1)
    hm = fitted(pb, 15)
    hm.tausq_update(0.37)
    pts, mv, labels, anchor = site_set(pb, 130, 16)
    n = pts.shape[0]
    Xn = np.random.default_rng(17).standard_normal((n, pb["p"]))
    hm.set_points(pts, mv, anchor, Xn, joint=labels)
    out = hm.predict_points(mode=0, seed=seed, it=it)
    rng = HostRng(seed)
    zz = rng.point_normals(it, n)
    for g, L in zip(hm.joint_groups, blocks(out["chol"])):
        assert np.abs(out["w"][g] - out["mean"][g] - L @ zz[g]).max() <= 1e-12 * np.abs(out["w"]).max()
    xb = np.einsum("ik,ki->i", Xn, hm.Bcoeff[:, mv - 1])
    assert np.abs(out["yhat"] - out["w"] - xb - np.sqrt(0.37) * rng.point_noise(it, n)).max() <= 1e-12 * np.abs(out["yhat"]).max()
    assert set(hm.points_info()["routes"]) <= MFMA
    hm.close()


def test_singletons_and_null_labels():
    """Groups of one: cond_mean bitwise st_points_predict's; cond_cov within 2 (P + 4) 2^-53 K(x, x) of cond_var (the same P
    non-negative products summed in two orders).  joint_id NULL is st_points_set."""
    pb = small(3)
    hm = fitted(pb, 6)
    pts, mv = new_points(pb, 300, 7)
    from spamtree_amd.predict import locate
    anchor = locate(pb["topo"], pts, mv, device=0)
    n = pts.shape[0]
    Xn = np.random.default_rng(17).standard_normal((n, pb["p"]))
    z = np.random.default_rng(12).standard_normal(n)
    hm.set_points(pts, mv, anchor, Xn)
    base = hm.predict_points(mode=0, z=z, seed=3, it=2)
    hm.set_points(pts, mv, anchor, Xn, joint=np.arange(n)[::-1].copy())
    out = hm.predict_points(mode=0, z=z, seed=3, it=2)
    assert set(hm.points_info()["routes"]) <= MFMA
    assert np.array_equal(out["mean"], base["mean"])
    ref = dense_moments(pb, hm.get_w(), pts, mv, anchor, hm.joint_groups)
    for g, c, r in zip(hm.joint_groups, blocks(out["cov"]), ref):
        assert abs(c[0, 0] - base["var"][g[0]]) <= 2 * (r[2] + 4) * U * r[3][0], g
    c = np.asfortranarray(pts)
    lib, h = hm.lib, hm.h
    assert lib.st_points_set_joint(h, n, dp(c), ip(np.ascontiguousarray(mv)), ip(np.ascontiguousarray(anchor)), dp(np.asfortranarray(Xn)), None) == 0
    o = {k: np.zeros(n) for k in ("w", "mean", "var", "yhat")}
    assert lib.st_points_predict(h, 0, dp(z), 3, 2, dp(o["w"]), dp(o["mean"]), dp(o["var"]), dp(o["yhat"])) == 0
    for k in o:
        assert np.array_equal(o[k], base[k]), k
    assert lib.st_points_predict_joint(h, 0, None, 3, 2, dp(o["w"]), None, None, None, None) == ST_ERR_USAGE   # not a joint set
    hm.close()


def by_label(hm, labels, out):
    """label -> (mean, w, cov, chol) of its group."""
    return {int(labels[g[0]]): (out["mean"][g], out["w"][g], c, L)
            for g, c, L in zip(hm.joint_groups, blocks(out["cov"]), blocks(out["chol"]))}


def test_results_do_not_depend_on_the_layout():
    pb = small(1)
    hm = fitted(pb, 6)
    pts, mv, labels, anchor = run_set(pb, 300, 7)
    n = pts.shape[0]
    z = np.random.default_rng(12).standard_normal(n)
    hm.set_points(pts, mv, anchor, joint=labels)
    base = by_label(hm, labels, hm.predict_points(mode=0, z=z))

    def same(sel, relabel=lambda x: x):
        hm.set_points(pts[sel], mv[sel], anchor[sel], joint=relabel(labels[sel]))
        got = by_label(hm, labels[sel], hm.predict_points(mode=0, z=z[sel]))
        for lab, vals in got.items():
            for a, b in zip(vals, base[lab]):
                assert np.array_equal(a, b), lab
        return len(got)
    rng = np.random.default_rng(13)
    order = rng.permutation(np.unique(labels))                                  # whole groups, members in their order
    assert same(np.concatenate([np.nonzero(labels == lab)[0] for lab in order])) == order.size
    first = np.isin(labels, order[: order.size // 3])                           # two point sets
    assert same(np.nonzero(first)[0]) + same(np.nonzero(~first)[0]) == order.size
    assert same(np.arange(n), lambda x: 7 - 3 * x) == order.size                # other labels
    hm.close()


def test_degenerate_pivots():
    from oracle.spamtree_oracle import CovarianceParams, Covariancef
    from spamtree_amd.predict import conditioning_set, locate
    pb = make_problem(side=24, q=2, seed=8, missing=0.2)
    topo = pb["topo"]
    hm = fitted(pb, 9)
    w = hm.get_w()
    pts, mv = new_points(pb, 50, 10)
    anchor = locate(topo, pts, mv, device=0)
    rows = np.array([int(np.concatenate([topo.indexing(int(u)) for u in conditioning_set(topo, int(b))])[-1]) for b in anchor])
    pts2, mv2 = topo.coords[rows], topo.mv_id[rows]
    a2 = locate(topo, pts2, mv2, device=0)
    keep = np.array([r in np.concatenate([topo.indexing(int(u)) for u in conditioning_set(topo, int(b))]) for r, b in zip(rows, a2)])
    m = int(keep.sum())
    assert m >= 10
    # group k: {the conditioning row with its margin, a free point}; then groups of one free point listed twice
    coords = np.vstack([np.column_stack([pts2[keep], pts[keep]]).reshape(-1, 2), np.repeat(pts[keep], 2, axis=0)])
    mvs = np.concatenate([np.column_stack([mv2[keep], mv[keep]]).reshape(-1), np.repeat(mv[keep], 2)])
    anc = np.concatenate([np.repeat(a2[keep], 2), np.repeat(a2[keep], 2)])
    labels = np.repeat(np.arange(2 * m), 2)
    hm.set_points(coords, mvs, anc, joint=labels)
    out = hm.predict_points(mode=0, z=np.ones(4 * m))
    for key in ("w", "mean", "cov_packed", "chol_packed"):
        assert np.all(np.isfinite(out[key])), key
    on_row = np.arange(0, 2 * m, 2)
    assert relerr(out["w"][on_row], w[rows[keep]]) <= 1e-8
    cp = CovarianceParams(2, pb["q"])
    cp.transform(pb["theta"])
    d1, d2 = np.arange(2 * m, 4 * m, 2), np.arange(2 * m + 1, 4 * m, 2)
    for a, b in zip(d1, d2):
        sd = np.sqrt(Covariancef(coords, mvs - 1, [a], [a], cp)[0, 0])
        assert abs(out["w"][a] - out["w"][b]) <= 1e-8 * sd, (a, out["w"][a], out["w"][b])
    assert np.abs(out["w"][d1] - out["mean"][d1]).max() > 1e-3                  # and they are draws, not means
    hm.close()


def test_refusals_leave_the_handle_usable():
    from spamtree_amd.predict import conditioning_set, locate
    pb = small(1)
    hm = hip_model(pb, w=np.random.default_rng(19).standard_normal(pb["n"]))
    lib, h = hm.lib, hm.h
    pts, mv = new_points(pb, 40, 20)
    anchor = locate(pb["topo"], pts, mv, device=0)
    order = np.argsort(anchor, kind="stable")
    pts, mv, anchor = np.asfortranarray(pts[order]), np.ascontiguousarray(mv[order]), np.ascontiguousarray(anchor[order])
    assert np.unique(anchor).size > 1
    anchor1 = np.full(40, anchor[0])
    call = lambda a, lab: lib.st_points_set_joint(h, 40, dp(pts), ip(mv), ip(a), None, ip(np.ascontiguousarray(lab, dtype=np.int64)))   # noqa: E731
    good = lambda: call(anchor1, np.arange(40) // 16)   # noqa: E731
    out = np.zeros(40)
    assert good() == 0
    assert lib.st_points_predict_joint(h, 0, None, 1, 0, dp(out), None, None, None, None) == ST_ERR_USAGE      # before st_factor(0)
    assert b"st_factor" in lib.st_last_error(h)
    assert hm.get_loglik_comps_w(0)
    assert call(anchor1, np.arange(40) // 17) == ST_ERR_UNSUPPORTED and b"16" in lib.st_last_error(h)
    assert lib.st_points_predict_joint(h, 0, None, 1, 0, dp(out), None, None, None, None) == 0 and np.all(np.isfinite(out))
    ends = np.array([conditioning_set(pb["topo"], int(b))[-1] for b in anchor])     # the block each point's chain ends in
    other = int(np.nonzero(ends != ends[0])[0][0])
    lab = np.arange(40) + 200
    lab[0] = lab[other] = 100
    assert call(anchor, lab) == ST_ERR_USAGE and b"group 100" in lib.st_last_error(h)
    assert good() == 0
    assert lib.st_points_predict_joint(h, 0, None, 1, 0, dp(out), None, None, None, None) == 0
    nj = C.c_int64(-1)
    assert lib.st_points_set_joint(h, 0, None, None, None, None, ip(np.zeros(1, dtype=np.int64))) == 0
    assert lib.st_points_joint_layout(h, C.byref(nj), None, None, None) == 0 and nj.value == 0
    assert lib.st_points_predict_joint(h, 0, None, 1, 0, None, None, None, None, None) == 0
    assert good() == 0
    hm.close()
    pl = make_problem(side=20, q=1, seed=5, missing=0.1, limited_tree=True)
    hl = hip_model(pl)
    assert hl.get_loglik_comps_w(0)
    al = np.full(40, locate(pl["topo"], pts, mv)[0])
    rc = hl.lib.st_points_set_joint(hl.h, 40, dp(pts), ip(mv), ip(al), None, ip(np.arange(40) // 16))
    assert rc == ST_ERR_UNSUPPORTED and b"limited_tree" in hl.lib.st_last_error(hl.h)
    assert hl.get_loglik_comps_w(0)
    hl.close()


def test_summaries_over_saved_iterations():
    """Five st_points_accumulate_joint calls with another w and theta each.  st_points_summary_get_cov against the extended-
    precision mean_s(Sigma_s) + cov_s(mean_s) of the per-call outputs.  The bound follows the kernel's own chain for n calls,
    u = 2^-53, X_a = max_s |mean_s,a|:
      * the running sum of Sigma_ab: n - 1 rounded additions of partial sums below sum_s |Sigma_s,ab|: (n - 1) u mean_s |Sigma_ab|
        after the division;
      * a Welford mean m + (x - m) / s: three roundings of at most u 2 X, and the recurrence contracts, so it is off by <= 6 s u X;
        each factor of a co-moment term (x_a - m_a)(x_b - m_b') by <= (6 n + 2) u X, the term (factors <= 2 X, one product
        rounding) by <= (24 n + 12) u X_a X_b; n terms and n - 1 additions of partial sums <= 4 n X_a X_b: (28 n + 8) u X_a X_b
        after the division;
      * two divisions and the final addition: 3 u (mean |Sigma_ab| + 4 X_a X_b).
    Together u [(n + 2) mean_s |Sigma_s,ab| + (28 n + 20) X_a X_b], first order; the test allows 2 u [..] for the second-order
    terms and the rounding of the reference to double."""
    pb = small(3)
    rng = np.random.default_rng(21)
    hm = fitted(pb, 6)
    pts, mv, labels, anchor = site_set(pb, 60, 22)
    n, ncalls = pts.shape[0], 5
    hm.set_points(pts, mv, anchor, joint=labels)
    lib, h = hm.lib, hm.h
    tot = int(hm.joint_offsets[-1])
    means, covs = np.zeros((ncalls, n)), np.zeros((ncalls, tot))
    for s in range(ncalls):
        hm.set_w(rng.standard_normal(pb["n"]))
        hm.theta_update(0, pb["theta"] * (1.0 + 0.05 * s))
        assert hm.get_loglik_comps_w(0)
        wn = np.zeros(n)
        hm._check(lib.st_points_accumulate_joint(h, 5, s, dp(wn), dp(means[s]), dp(covs[s]), None, None))
        assert np.all(np.isfinite(wn))
    got = np.zeros(tot)
    hm._check(lib.st_points_summary_get_cov(h, dp(got)))
    mean, var = np.zeros(n), np.zeros(n)
    cnt = C.c_int64()
    hm._check(lib.st_points_summary_get(h, dp(mean), dp(var), None, None, C.byref(cnt)))
    assert cnt.value == ncalls
    mx, cx = means.astype(np.longdouble), covs.astype(np.longdouble)
    X = np.abs(means).max(axis=0)
    for k, g in enumerate(hm.joint_groups):
        sl = slice(int(hm.joint_offsets[k]), int(hm.joint_offsets[k + 1]))
        d = mx[:, g] - mx[:, g].mean(axis=0)
        want = (cx[:, sl].mean(axis=0).reshape(g.size, g.size, order="F") + d.T @ d / ncalls).astype(np.float64)
        tol = 2 * U * ((ncalls + 2) * np.abs(covs[:, sl]).mean(axis=0).reshape(g.size, g.size, order="F") + (28 * ncalls + 20) * np.outer(X[g], X[g]))
        G = got[sl].reshape(g.size, g.size, order="F")
        assert np.all(np.abs(G - want) <= tol), (k, np.abs(G - want).max(), tol.min())
        assert np.array_equal(G, G.T)
        assert np.all(np.abs(np.diag(G) - var[g]) <= np.diag(tol)), k
    assert lib.st_points_summary_reset(h) == 0
    assert lib.st_points_summary_get_cov(h, dp(got)) == ST_ERR_USAGE                # nothing accumulated
    hm._check(lib.st_points_accumulate(h, 5, 0, None, None, None, None))
    hm._check(lib.st_points_summary_get_cov(h, dp(got)))
    assert relerr(got, covs[-1]) <= 4 * U                                           # one call: Sigma itself, no spread of the means
    hm.close()


def test_whole_path_through_the_fit():
    from spamtree_amd import fit
    from spamtree_amd.predict import group_sites, locate, predict_new
    pb = make_problem(side=24, q=2, seed=2, missing=0.2)
    k = pb["theta"].size
    burn, thin, keep, seed = 2, 2, 3, 77
    pts, _ = new_points(pb, 60, 23)
    coords, mv = np.repeat(pts, 2, axis=0), np.tile([1, 2], 60)
    sites = group_sites(coords)
    assert np.array_equal(sites, np.repeat(np.arange(60), 2))
    anchor = locate(pb["topo"], coords, mv, device=0, joint=sites)
    kw = dict(mcmc_keep=keep, mcmc_burn=burn, mcmc_thin=thin, seed=seed)
    plain = fit.spamtree_mv_mcmc(*args_of(pb, k), **kw)
    out = fit.spamtree_mv_mcmc(*args_of(pb, k), new_points=dict(coords=coords, mv=mv, anchor=anchor, joint=sites), **kw)
    for key in ("beta_mcmc", "tausq_mcmc", "theta_mcmc", "paramsd"):
        assert np.array_equal(out[key], plain[key]), key
    for key in ("w_mcmc", "yhat_mcmc"):
        assert all(np.array_equal(a, b) for a, b in zip(out[key], plain[key])), key
    new = out["new"]
    assert set(new["route"]) <= MFMA and new["route"]
    rep = predict_new(pb, plain, coords, mv, seed=seed, joint=sites)
    assert np.array_equal(rep["anchor"], anchor)
    for s in range(keep):
        assert np.abs(new["cond_cov"][s] - rep["cond_cov"][s]).max() <= 1e-9 * max(1.0, np.abs(rep["cond_cov"][s]).max()), s
        assert np.array_equal(new["cond_var"][:, s], np.maximum(new["cond_cov"][s][:, [0, 1], [0, 1]].reshape(-1), 0.0))
    assert np.abs(new["cov"] - rep["cov"]).max() <= 1e-9 * max(1.0, np.abs(rep["cov"]).max())
    assert new["cov"].shape == (60, 2, 2) and all(np.array_equal(g, [2 * i, 2 * i + 1]) for i, g in enumerate(new["groups"]))
    for c in new["cov"]:
        assert np.array_equal(c, c.T) and np.linalg.eigvalsh(c).min() >= -1e-12 * np.trace(c)
    assert np.abs(new["cov"][:, 1, 0]).max() > 1e-6                             # what no per-point predictive can give
    assert np.abs(np.diagonal(new["cov"], axis1=1, axis2=2).reshape(-1) - new["var"]).max() <= 1e-12 * new["var"].max()
