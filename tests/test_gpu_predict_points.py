"""GPU: prediction at new locations (st_points_*, spamtree_amd/predict.py).

  * replaying a saved chain at the NA rows' coordinates, with the sweep normals of each saved iteration, reproduces the
    chain's own draws of those rows (phase P): the whole path pinned against the existing predict_std kernels;
  * the conditional mean and variance equal the dense kriging identities on the conditioning set;
  * k_points_mfma<128>, k_points_mfma<256> and k_points_generic each run (st_points_info), agree, and give results that do
    not depend on the order or grouping of the points; the Philox streams 6 / 7; the refusals.
"""
import numpy as np
import pytest

from tests.util import distinct_theta, make_problem, strip_coords

pytestmark = pytest.mark.gpu

ST_ERR_USAGE, ST_ERR_UNSUPPORTED = -1, -4


def relerr(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(1e-300, np.abs(b).max()))


def hip_model(pb, w=None, beta=None, tausq=0.2, **kw):
    from spamtree_amd.model import SpamTreeMV
    w = np.zeros(pb["n"]) if w is None else w
    beta = np.zeros(pb["p"]) if beta is None else beta
    return SpamTreeMV(pb["y"], pb["X"], pb["Z"], pb["coords"], pb["mv_id"], pb["blocking"], pb["gix_block"], pb["res_is_ref"],
                      pb["parents"], pb["children"], pb.get("limited_tree", False), pb["block_names"], pb["block_groups"],
                      pb["indexing"], w, beta, pb["theta"], 1.0 / tausq, device=0, **kw)


def fitted(pb, seed):
    """A model on a random state of pb with slot 0 factorised."""
    rng = np.random.default_rng(seed)
    hm = hip_model(pb, w=rng.standard_normal(pb["n"]), beta=rng.standard_normal(pb["p"]))
    assert hm.get_loglik_comps_w(0)
    return hm


def new_points(pb, n, seed):
    rng = np.random.default_rng(seed)
    lo, hi = pb["coords"].min(axis=0), pb["coords"].max(axis=0)
    pts = lo + (hi - lo) * rng.uniform(size=(n, 2))
    mv = rng.integers(1, pb["q"] + 1, size=n)
    return pts, mv


def args_of(pb, k):
    return (pb["y"], pb["X"], pb["Z"], pb["coords"], pb["mv_id"], pb["blocking"], pb["gix_block"], pb["res_is_ref"],
            pb["parents"], pb["children"], False, pb["block_names"], pb["block_groups"], pb["indexing"], pb["bounds"],
            np.zeros((pb["n"], 1)), pb["theta"], np.zeros(pb["p"]), 0.1, 0.01 * np.eye(k))


def _deep4():
    coords, mv = strip_coords(370, 10, 3)
    return make_problem(coords=coords, mv_id=mv, q=3, seed=3, K=(2, 1), tree_depth=7, missing=0.1)


def _deep5():
    coords, mv = strip_coords(900, 6, 3)
    return make_problem(coords=coords, mv_id=mv, q=3, seed=4, K=(2, 1), cell_size=9, tree_depth=9, missing=0.1)


@pytest.mark.parametrize("case", ["q1", "q2", "deep4", "deep5"])
def test_replay_at_the_na_rows_reproduces_the_chain(case):
    """k_points_mfma<128> / <256> (q1, q2, deep5: chains of 71-228 rows) and k_points_generic (deep4: 444-475 rows, config #4's
    75-row blocks) against phase P of the chain itself: w_mcmc[:, s] at the NA rows, to 1e-9."""
    from spamtree_amd import fit
    from spamtree_amd.predict import predict_new
    from spamtree_amd.rng import HostRng
    pb = {"q1": lambda: make_problem(side=30, q=1, seed=1, missing=0.1),
          "q2": lambda: make_problem(side=24, q=2, seed=2, missing=0.2),
          "deep4": _deep4, "deep5": _deep5}[case]()
    k = pb["theta"].size
    burn, thin, keep, seed = 2, 2, 3, 77
    draws = fit.spamtree_mv_mcmc(*args_of(pb, k), mcmc_keep=keep, mcmc_burn=burn, mcmc_thin=thin, seed=seed)
    assert "None" not in draws
    na = np.nonzero(~np.isfinite(pb["y"]))[0]
    rng = HostRng(seed)
    z = np.column_stack([rng._normal(na, 0, burn + s * thin, 0) for s in range(keep)])
    out = predict_new(pb, draws, pb["coords"][na], pb["mv_id"][na], seed=seed, z=z, device=0)
    want = {"q1": {"k_points_mfma<128>"}, "q2": {"k_points_mfma<128>", "k_points_mfma<256>"},
            "deep4": {"k_points_generic"}, "deep5": {"k_points_mfma<256>"}}[case]
    assert set(out["route"]) == want, out["route"]
    for s in range(keep):
        assert relerr(out["w"][:, s], np.asarray(draws["w_mcmc"][s]).reshape(-1)[na]) <= 1e-9, s
    cm = np.mean([out["w"][:, s] for s in range(keep)], axis=0)
    assert np.all(np.isfinite(out["mean"])) and np.all(out["var"] >= 0) and cm.shape == out["mean"].shape


@pytest.mark.parametrize("q", [1, 3, 5])
def test_conditional_moments_equal_the_dense_identity(q):
    from oracle.spamtree_oracle import CovarianceParams, Covariancef
    from spamtree_amd.predict import conditioning_set, locate
    if q == 5:      # 45-row blocks, chains of <= 135 rows (the default 125-row blocks would leave the column-group kernels);
        pb = make_problem(side=14, q=q, seed=5, missing=0.1, cell_size=9)      # every per-outcome parameter different
        pb["theta"] = distinct_theta(q)
    else:
        pb = make_problem(side=20, q=q, seed=5, missing=0.1)
    topo = pb["topo"]
    hm = fitted(pb, 6)
    w = hm.get_w()
    pts, mv = new_points(pb, 300, 7)
    anchor = locate(topo, pts, mv, device=0)
    hm.set_points(pts, mv, anchor)
    out = hm.predict_points(mode=1)
    assert out["yhat"] is None and np.array_equal(out["w"], out["mean"])
    cp = CovarianceParams(2, q)
    cp.transform(pb["theta"])
    allc = np.vstack([topo.coords, pts])
    allv = np.concatenate([topo.mv_id - 1, mv - 1])
    n = pb["n"]
    mean, var = np.zeros(pts.shape[0]), np.zeros(pts.shape[0])
    for i in range(pts.shape[0]):
        S = np.concatenate([topo.indexing(int(b)) for b in conditioning_set(topo, int(anchor[i]))])
        Kss = Covariancef(allc, allv, S, S, cp, same=True)
        ks = Covariancef(allc, allv, S, [n + i], cp)[:, 0]
        kxx = Covariancef(allc, allv, [n + i], [n + i], cp)[0, 0]
        sol = np.linalg.solve(Kss, np.column_stack([w[S], ks]))
        mean[i] = ks @ sol[:, 0]
        var[i] = kxx - ks @ sol[:, 1]
    assert relerr(out["mean"], mean) <= 1e-9
    assert np.abs(out["var"] - np.maximum(var, 0)).max() <= 1e-9 * max(1.0, np.abs(var).max())
    assert set(hm.points_info()["routes"]) <= {"k_points_mfma<128>", "k_points_mfma<256>"}
    hm.close()


def test_point_on_a_conditioning_row_returns_its_w():
    from spamtree_amd.predict import conditioning_set, locate
    pb = make_problem(side=24, q=2, seed=8, missing=0.2)
    topo = pb["topo"]
    hm = fitted(pb, 9)
    w = hm.get_w()
    pts, mv = new_points(pb, 50, 10)
    anchor = locate(topo, pts, mv, device=0)
    # the last row of each point's own conditioning set (the anchor's block for a reference anchor, else its last parent)
    rows = np.array([int(np.concatenate([topo.indexing(int(u)) for u in conditioning_set(topo, int(b))])[-1]) for b in anchor])
    pts2, mv2 = topo.coords[rows], topo.mv_id[rows]
    a2 = locate(topo, pts2, mv2, device=0)
    keep = np.array([r in np.concatenate([topo.indexing(int(u)) for u in conditioning_set(topo, int(b))]) for r, b in zip(rows, a2)])
    assert keep.sum() >= 10
    hm.set_points(pts2[keep], mv2[keep], a2[keep])
    out = hm.predict_points(mode=0, z=np.ones(int(keep.sum())))
    assert np.all(np.isfinite(out["w"])) and np.all(np.isfinite(out["var"])) and np.all(out["var"] >= 0)
    assert relerr(out["mean"], w[rows[keep]]) <= 1e-8
    assert out["var"].max() <= 1e-8 * pb["theta"][0] ** 2                       # nothing left to draw at a conditioning row
    assert np.array_equal(out["w"], out["mean"] + np.sqrt(out["var"]))          # z = 1
    hm.close()


def test_routes_agree_and_results_do_not_depend_on_order_or_grouping():
    """k_points_mfma<128> and k_points_mfma<256> (chains of 108-129 rows) against k_points_generic (force_generic) on the same
    points, to 1e-12; bitwise invariance under a permutation and under a split into two point sets."""
    from spamtree_amd.predict import locate
    pb = make_problem(side=24, q=2, seed=2, missing=0.2)
    pts, mv = new_points(pb, 700, 11)
    anchor = locate(pb["topo"], pts, mv, device=0)
    z = np.random.default_rng(12).standard_normal(pts.shape[0])
    res = {}
    for fg in (False, True):
        rng = np.random.default_rng(6)
        hm = hip_model(pb, w=rng.standard_normal(pb["n"]), beta=rng.standard_normal(pb["p"]), force_generic=fg)
        assert hm.get_loglik_comps_w(0)
        hm.set_points(pts, mv, anchor)
        out = hm.predict_points(mode=0, z=z)
        info = hm.points_info()
        res[fg] = out
        if not fg:
            assert set(info["routes"]) == {"k_points_mfma<128>", "k_points_mfma<256>"}, info
            perm = np.random.default_rng(13).permutation(pts.shape[0])
            hm.set_points(pts[perm], mv[perm], anchor[perm])
            o2 = hm.predict_points(mode=0, z=z[perm])
            for key in ("mean", "var", "w"):
                assert np.array_equal(o2[key], out[key][perm]), key
            half = pts.shape[0] // 3
            parts = []
            for sl in (slice(0, half), slice(half, None)):
                hm.set_points(pts[sl], mv[sl], anchor[sl])
                parts.append(hm.predict_points(mode=0, z=z[sl]))
            for key in ("mean", "var", "w"):
                assert np.array_equal(np.concatenate([parts[0][key], parts[1][key]]), out[key]), key
        else:
            assert info["routes"] == ["k_points_generic"], info
        assert info["n_groups"] > 1 and info["alg_bytes"] > 0 and info["flops"] > 0
        hm.close()
    for key in ("mean", "var", "w"):
        assert relerr(res[False][key], res[True][key]) <= 1e-12, key


def test_default_streams_6_and_7():
    from spamtree_amd.predict import locate
    from spamtree_amd.rng import HostRng
    pb = make_problem(side=20, q=3, seed=14, missing=0.1)
    hm = fitted(pb, 15)
    hm.tausq_update(0.37)
    pts, mv = new_points(pb, 400, 16)
    Xn = np.random.default_rng(17).standard_normal((400, pb["p"]))
    hm.set_points(pts, mv, locate(pb["topo"], pts, mv, device=0), Xn)
    seed, it = 123456789, 5
    out = hm.predict_points(mode=0, seed=seed, it=it)
    rng = HostRng(seed)
    assert relerr(out["w"], out["mean"] + np.sqrt(out["var"]) * rng.point_normals(it, 400)) <= 1e-12
    xb = np.einsum("ik,ki->i", Xn, hm.Bcoeff[:, mv - 1])
    assert np.abs(out["yhat"] - out["w"] - xb - np.sqrt(0.37) * rng.point_noise(it, 400)).max() <= 1e-12 * np.abs(out["yhat"]).max()
    assert "k_points_mfma<128>" in hm.points_info()["routes"] or "k_points_mfma<256>" in hm.points_info()["routes"]
    hm.close()


def test_refusals_leave_the_handle_usable():
    from spamtree_amd.model import SpamTreeError
    from spamtree_amd.predict import locate
    import ctypes as C
    pb = make_problem(side=20, q=1, seed=18, missing=0.1)
    hm = hip_model(pb, w=np.random.default_rng(19).standard_normal(pb["n"]))
    lib, h = hm.lib, hm.h
    pts, mv = new_points(pb, 30, 20)
    anchor = locate(pb["topo"], pts, mv, device=0)
    c = np.asfortranarray(pts)
    dp, ip = (lambda a: a.ctypes.data_as(C.POINTER(C.c_double))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_int64)))
    good = lambda: lib.st_points_set(h, 30, dp(c), ip(np.ascontiguousarray(mv)), ip(np.ascontiguousarray(anchor)), None)
    assert good() == 0
    out = np.zeros(30)
    assert lib.st_points_predict(h, 0, None, 1, 0, dp(out), None, None, None) == ST_ERR_USAGE      # before st_factor(0)
    assert b"st_factor" in lib.st_last_error(h)
    empty = np.nonzero(np.bincount(pb["blocking"] - 1, weights=np.isfinite(pb["y"]).astype(float)) == 0)[0]
    assert empty.size
    for bad_anchor, bad_mv in [(pb["block_names"].size, 1), (-1, 1), (int(empty[0]), 1), (int(anchor[0]), 0), (int(anchor[0]), 2)]:
        a = np.ascontiguousarray(anchor.copy()); m = np.ascontiguousarray(mv.copy())
        a[3], m[3] = bad_anchor, bad_mv
        assert lib.st_points_set(h, 30, dp(c), ip(m), ip(a), None) == ST_ERR_USAGE, (bad_anchor, bad_mv)
    assert hm.get_loglik_comps_w(0)
    assert good() == 0
    assert lib.st_points_predict(h, 0, None, 1, 0, dp(out), None, None, None) == 0 and np.all(np.isfinite(out))
    with pytest.raises(SpamTreeError):      # yhat without the regressors of st_points_set
        hm._check(lib.st_points_predict(h, 0, None, 1, 0, None, None, None, dp(out)))
    hm.close()
    pl = make_problem(side=20, q=1, seed=18, missing=0.1, limited_tree=True)
    hl = hip_model(pl)
    assert hl.get_loglik_comps_w(0)
    rc = hl.lib.st_points_set(hl.h, 30, dp(c), ip(np.ascontiguousarray(mv)), ip(np.ascontiguousarray(locate(pl["topo"], pts, mv))), None)
    assert rc == ST_ERR_UNSUPPORTED and b"limited_tree" in hl.lib.st_last_error(hl.h)
    assert hl.get_loglik_comps_w(0)
    hl.close()


def test_a_refused_set_leaves_the_previous_point_set_in_place():
    """st_points_set and st_points_set_joint refuse before they release the old set: after a bad margin and after a 17-member
    joint group the next st_points_predict, without setting the points anew, gives the first one's outputs bit for bit."""
    from spamtree_amd.predict import locate
    import ctypes as C
    pb = make_problem(side=20, q=1, seed=18, missing=0.1)
    hm = fitted(pb, 19)
    lib, h = hm.lib, hm.h
    pts, mv = new_points(pb, 30, 20)
    anchor = np.ascontiguousarray(locate(pb["topo"], pts, mv, device=0))
    c, mv = np.asfortranarray(pts), np.ascontiguousarray(mv)
    dp, ip = (lambda a: a.ctypes.data_as(C.POINTER(C.c_double))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_int64)))
    z = np.random.default_rng(21).standard_normal(30)

    def predict():
        out = np.full((4, 30), np.nan)
        assert lib.st_points_predict(h, 0, dp(z), 1, 0, dp(out[0]), dp(out[1]), dp(out[2]), None) == 0
        assert np.all(np.isfinite(out[:3]))
        return out[:3].copy()

    assert lib.st_points_set(h, 30, dp(c), ip(mv), ip(anchor), None) == 0
    first = predict()
    bad_mv = mv.copy()
    bad_mv[3] = 2
    assert lib.st_points_set(h, 30, dp(c), ip(bad_mv), ip(anchor), None) == ST_ERR_USAGE
    assert b"margin of point 3" in lib.st_last_error(h)
    labels = np.ascontiguousarray(np.concatenate([np.zeros(17), np.arange(1, 14)]).astype(np.int64))
    same = np.ascontiguousarray(np.full(30, anchor[0]))
    assert lib.st_points_set_joint(h, 30, dp(c), ip(mv), ip(same), None, ip(labels)) == ST_ERR_UNSUPPORTED
    assert b"more than 16 members" in lib.st_last_error(h)
    assert np.array_equal(predict(), first)
    hm.close()
