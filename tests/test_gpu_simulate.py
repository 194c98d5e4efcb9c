"""st_simulate (prior draws from slot 0) on the GPU: against the NumPy restatement of the sweep, the per-block identity
||Ri w_u + N w_pa||^2 = ||z_u||^2 at any size, batch invariance, an untouched chain, the draws' statistics, the refusals and
the front door (spamtree_amd.simulate)."""
import ctypes as C

import numpy as np
import pytest

from tests.prior_sweep import prior_sweep
from tests.test_oracle_identities import dense_precision
from tests.util import distinct_theta, make_problem, oracle_model, strip_coords

pytestmark = pytest.mark.gpu

HL2PI = -0.91893853320467274178032973640562


def hip_model(pb, force_generic=False, tausq=0.2):
    from spamtree_amd.model import SpamTreeMV
    hm = SpamTreeMV(pb["y"], pb["X"], pb["Z"], pb["coords"], pb["mv_id"], pb["blocking"], pb["gix_block"], pb["res_is_ref"],
                    pb["parents"], pb["children"], pb.get("limited_tree", False), pb["block_names"], pb["block_groups"],
                    pb["indexing"], np.zeros(pb["n"]), pb["beta_true"], pb["theta"], 1.0 / tausq, force_generic=force_generic)
    if "tausq" in pb:       # one noise variance per outcome
        hm.tausq_inv = 1.0 / np.asarray(pb["tausq"], dtype=np.float64)
        assert hm.lib.st_set_tausq_inv(hm.h, hm.tausq_inv.ctypes.data_as(C.POINTER(C.c_double))) == 0
    assert hm.get_loglik_comps_w(0)
    return hm


def q5_problem():
    """Five outcomes (20-row blocks), every per-outcome and per-pair covariance parameter and every tausq different."""
    pb = make_problem(side=12, q=5, seed=5, cell_size=6)
    pb.update(theta=distinct_theta(5), tausq=np.array([0.2, 0.05, 0.4, 0.1, 0.3]))
    return pb


CASES = {
    "q1_grid": lambda: make_problem(side=20, q=1, seed=5),
    "q1_random": lambda: make_problem(side=20, q=1, seed=5, random_coords=True),
    "q2": lambda: make_problem(side=14, q=2, seed=5),
    "q3_wide": lambda: make_problem(side=12, q=3, seed=5),
    "limited": lambda: make_problem(side=20, q=2, seed=5, limited_tree=True),
    "q5": q5_problem,
    "strip_deep": lambda: make_problem(coords=strip_coords(640, 4, 1)[0], mv_id=strip_coords(640, 4, 1)[1], q=1, seed=5,
                                       K=(2, 1), cell_size=16, tree_depth=7),
}
RUNS = [(k, False) for k in CASES] + [("q1_grid", True), ("q3_wide", True)]


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def test_caller_normals_match_the_restated_sweep_and_reach_every_route():
    reached = 0
    for name, generic in RUNS:
        pb = CASES[name]()
        om = oracle_model(pb)
        assert om.get_loglik_comps_w(om.param_data)
        hm = hip_model(pb, force_generic=generic)
        rng = np.random.default_rng(1)
        n = pb["n"]
        z, eps = rng.standard_normal((n, 3)), rng.standard_normal((n, 3))
        w, y = hm.simulate(3, z=z, eps=eps)
        wr = prior_sweep(om, z)
        assert rel(w, wr) <= 1e-10, (name, generic, rel(w, wr))
        tau = np.sqrt(np.broadcast_to(pb.get("tausq", 0.2), (pb["q"],)))[pb["mv_id"] - 1][:, None]
        yr = (pb["X"] @ pb["beta_true"])[:, None] + wr + tau * eps
        assert rel(y, yr) <= 1e-10, (name, generic)
        reached |= hm.simulate_info(3)["route_mask"]
        hm.close()
    from spamtree_amd import _lib
    lib = _lib.load()
    codes = [c for c in range(1, 32) if lib.st_simulate_route_name(c)]
    assert reached == sum(1 << (c - 1) for c in codes), (bin(reached), codes)




def check_identity(hm, indexing, nd=2, seed=3):
    n = hm.n_all
    z = np.random.default_rng(seed).standard_normal((n, nd))
    w, _ = hm.simulate(nd, z=z, outcomes=False)
    m = np.array([ix.size for ix in indexing])
    for d in range(nd):
        hm.set_w(w[:, d])
        hm.get_loglik_w(0)
        _, comps = hm.comps(0)
        zz = np.array([np.dot(z[ix, d], z[ix, d]) for ix in indexing])
        want = m * HL2PI - 0.5 * zz
        assert np.abs(comps - want).max() <= 1e-10 * np.abs(want).max()


def test_per_block_identity_at_test_size():
    for name in ("q1_grid", "q3_wide", "limited"):
        pb = CASES[name]()
        hm = hip_model(pb)
        check_identity(hm, pb["indexing"])
        hm.close()


def test_per_block_identity_on_config3_full_tree():
    from spamtree_amd import synthetic
    wl = synthetic.make_workload(1000, q=1, p=3)
    pb = dict(wl, parents=wl["parents"], beta_true=wl["beta_true"])
    hm = hip_model(pb)
    ip, ii = wl["indexing"]
    check_identity(hm, [ii[ip[u]:ip[u + 1]] for u in range(ip.size - 1)], nd=1)
    hm.close()


def test_batch_invariance_and_device_streams():
    from oracle.spamtree_oracle import StRng
    pb = CASES["q2"]()
    hm = hip_model(pb)
    w16, y16 = hm.simulate(16, seed=77, it=5)
    for d in range(16):
        w1, y1 = hm.simulate(1, seed=77, it=5 + d)
        assert np.array_equal(w1[:, 0], w16[:, d]) and np.array_equal(y1[:, 0], y16[:, d]), d
    w3, _ = hm.simulate(3, seed=77, it=5)
    assert np.array_equal(w3, w16[:, :3])
    n = pb["n"]
    rng = StRng(77)
    z = np.stack([rng.normal(np.arange(n), 0, 5 + d, 8) for d in range(2)], axis=1)
    eps = np.stack([rng.normal(np.arange(n), 0, 5 + d, 9) for d in range(2)], axis=1)
    wz, yz = hm.simulate(2, z=z, eps=eps)      # the host stream's log / cos may differ from the device's in the last bit
    assert rel(wz, w16[:, :2]) <= 1e-12 and rel(yz, y16[:, :2]) <= 1e-12
    hm.close()


def test_chain_state_is_untouched():
    pb = CASES["q1_grid"]()
    runs = []
    for interleave in (False, True):
        hm = hip_model(pb)
        hm.deal_with_w(None, seed=3, it=0)
        out = []
        for it in range(1, 4):
            if interleave:
                hm.simulate(4, seed=9, it=it)
            hm.deal_with_w(None, seed=3, it=it)
            if interleave:
                hm.simulate(2, seed=9, it=it)
            th = pb["theta"] * (1.0 + 0.01 * it)
            hm.theta_update(1, th)
            hm.get_loglik_comps_w(1)
            hm.accept_make_change()
            out.append((hm.get_w().copy(), hm.get_loglik_w(0), hm.get_XB().copy()))
        runs.append(out)
        hm.close()
    for a, b in zip(*runs):
        assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])


def test_draw_statistics():
    pb = make_problem(side=20, q=1, seed=8)
    hm = hip_model(pb, tausq=0.3)
    n, R = pb["n"], 4096
    W = np.empty((n, R))
    E = np.empty((n, R))
    xb = pb["X"] @ pb["beta_true"]
    for d0 in range(0, R, 16):
        w, y = hm.simulate(16, seed=2024, it=d0)
        W[:, d0:d0 + 16] = w
        E[:, d0:d0 + 16] = y - xb[:, None] - w
    hm.close()
    Q, _ = dense_precision(pb, pb["theta"])
    L = np.linalg.cholesky(Q)              # Q = L L', so L' w ~ N(0, I)
    U = L.T @ W
    S = U @ U.T / R
    # entries of a Wishart(I, R) / R: diagonal sd sqrt(2 / R), off-diagonal sd sqrt(1 / R); 6 sd over n^2 entries
    assert np.abs(np.diag(S) - 1).max() <= 6 * np.sqrt(2.0 / R)
    off = S - np.diag(np.diag(S))
    assert np.abs(off).max() <= 6.5 * np.sqrt(1.0 / R)
    v = (E ** 2).mean()
    assert abs(v / 0.3 - 1) <= 6 * np.sqrt(2.0 / (n * R))


def test_refusals():
    from spamtree_amd import _lib
    lib = _lib.load()
    pb = make_problem(side=12, q=1, seed=2, missing=0.2)
    hm = hip_model(pb)
    w = np.zeros(pb["n"])
    dp = w.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.st_simulate(hm.h, 1, None, None, 1, 0, dp, None) == -4
    hm.close()
    pb = make_problem(side=12, q=1, seed=2)
    from spamtree_amd.model import SpamTreeMV
    hm = SpamTreeMV(pb["y"], pb["X"], pb["Z"], pb["coords"], pb["mv_id"], pb["blocking"], pb["gix_block"], pb["res_is_ref"],
                    pb["parents"], pb["children"], False, pb["block_names"], pb["block_groups"], pb["indexing"],
                    np.zeros(pb["n"]), pb["beta_true"], pb["theta"], 5.0)
    w = np.zeros((pb["n"], 17))
    dp = w.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.st_simulate(hm.h, 1, None, None, 1, 0, dp, None) == -1          # slot 0 never factorised
    assert hm.get_loglik_comps_w(0)
    assert lib.st_simulate(hm.h, 0, None, None, 1, 0, dp, None) == -1
    assert lib.st_simulate(hm.h, 17, None, None, 1, 0, dp, None) == -1
    assert lib.st_simulate(hm.h, 16, None, None, 1, 0, dp, None) == 0
    hm.close()


def test_front_door_permutation_and_fit():
    from spamtree_amd import fit, simulate
    rng = np.random.default_rng(4)
    n = 600
    coords = rng.uniform(size=(n, 2))
    X = np.c_[np.ones(n), rng.standard_normal(n)]
    beta = np.array([1.0, -0.5])
    theta = np.array([1.5, 1.0, 1.0, 5.0])
    a = simulate.simulate(coords, theta, X=X, beta=beta, tausq=0.1, n_draws=3, seed=5)
    perm = rng.permutation(n)
    b = simulate.simulate(coords[perm], theta, X=X[perm], beta=beta, tausq=0.1, n_draws=3, seed=5)
    assert np.array_equal(a["w"][perm], b["w"]) and np.array_equal(a["y"][perm], b["y"])
    wl = simulate.as_workload(a, draw=1, missing=0.1)
    keep = 100
    r = fit.spamtree_mv_mcmc(wl["y"], wl["X"], wl["Z"], wl["coords"], wl["mv_id"], wl["blocking"], wl["gix_block"],
                             wl["res_is_ref"], wl["parents"], wl["children"], False, wl["block_names"], wl["block_groups"],
                             wl["indexing"], wl["bounds"], np.zeros(n), theta, np.zeros(2), 0.1, 0.05 * np.eye(theta.size),
                             mcmc_keep=keep, mcmc_burn=100, seed=6, save_w=False, save_yhat=False)
    bm = r["beta_mcmc"][:, :, 0]
    mu, sd = bm.mean(axis=1), bm.std(axis=1)
    assert (np.abs(mu - beta) <= 4 * sd).all(), (mu, sd)
