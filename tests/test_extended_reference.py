"""CPU: the extended-precision per-block reference (oracle/extended.py) that judges the kernels at ill-conditioned theta.

It is checked against mpmath at 50 digits on small blocks, against the float64 oracle where that oracle is accurate
(nice_theta), and it shows that the oracle itself loses digits as phi falls, which is why the GPU conditioning tests
(tests/test_gpu_conditioning.py) need it.
"""
import types

import numpy as np
import pytest

from oracle.extended import LD, ExtendedBlocks, covariance
from tests.util import distinct_theta, make_problem, nice_theta, oracle_model


def relerr(a, b):
    a = np.asarray(a, dtype=LD)
    b = np.asarray(b, dtype=LD)
    return float(np.abs(a - b).max() / np.abs(b).max())


def tiny_tree(q, nloc=(8, 4, 2), seed=3):
    """Three blocks in a chain: a root of nloc[0] locations, a reference child of nloc[1] and a non-reference grandchild of
    nloc[2] (every location carries all q outcomes).  Only the fields ExtendedBlocks reads."""
    rng = np.random.default_rng(seed)
    ix, rows, mv, coords = [], 0, [], []
    for k in nloc:
        pts = rng.uniform(size=(k, 2))
        ix.append(np.arange(rows, rows + k * q))
        rows += k * q
        coords.append(np.tile(pts, (q, 1)))
        mv.append(np.repeat(np.arange(1, q + 1), k))
    parents = [np.zeros(0, dtype=np.int64), np.array([0]), np.array([0, 1])]
    om = types.SimpleNamespace(
        q=q, coords=np.vstack(coords), mv_id=np.concatenate(mv), indexing=ix,
        parents=parents, children=[np.array([1]), np.array([2]), np.zeros(0, dtype=np.int64)],
        parents_indexing=[np.zeros(0, dtype=np.int64), ix[0], np.concatenate([ix[0], ix[1]])],
        block_groups=np.array([1.0, 2.0, 3.0]), res_is_ref=np.array([1, 1, 0]), limited_tree=False)
    return om


def mp_covariance(om, theta, i1, i2):
    import mpmath as mp
    q = om.q
    K = mp.matrix(len(i1), len(i2))
    if q > 1:
        from oracle.extended import unpack_theta
        ai1, ai2, phi, tmv, D = unpack_theta(theta, q)
    for a, r in enumerate(i1):
        for b, s in enumerate(i2):
            h = mp.sqrt((mp.mpf(om.coords[r, 0]) - mp.mpf(om.coords[s, 0])) ** 2 +
                        (mp.mpf(om.coords[r, 1]) - mp.mpf(om.coords[s, 1])) ** 2)
            if q == 1:
                K[a, b] = mp.mpf(theta[0]) * mp.exp(-mp.mpf(theta[3]) * h)
                continue
            vi, vj = om.mv_id[r] - 1, om.mv_id[s] - 1
            v = mp.mpf(D[vi, vj])
            if q > 2:
                psi = (mp.mpf(tmv[0]) * v + 1) ** mp.mpf(tmv[1])          # (a v + 1)^beta
                cb = mp.exp(-mp.mpf(tmv[2]) * h / mp.sqrt(psi)) / psi
            else:
                cb = mp.exp(-mp.mpf(tmv[0]) * h / mp.sqrt(v + 1)) / (v + 1)
            if v == 0:
                K[a, b] = mp.mpf(ai1[vi]) ** 2 * cb + mp.mpf(ai2[vi]) ** 2 * mp.exp(-mp.mpf(phi[vi]) * h)
            else:
                K[a, b] = mp.mpf(ai1[vi]) * mp.mpf(ai1[vj]) * cb
    return K


def mp_block(om, theta, u):
    import mpmath as mp
    iu, pa = om.indexing[u], om.parents_indexing[u]
    Kuu = mp_covariance(om, theta, iu, iu)
    H = mp_covariance(om, theta, iu, pa) * mp.inverse(mp_covariance(om, theta, pa, pa)) if pa.size else None
    R = Kuu - H * mp_covariance(om, theta, pa, iu) if pa.size else Kuu
    if om.res_is_ref[u] or not pa.size:
        Ri = mp.inverse(mp.cholesky(R))
        diag = [Ri[i, i] for i in range(iu.size)]
        N = -Ri * H if pa.size else None
    else:
        diag = [1 / mp.sqrt(R[i, i]) for i in range(iu.size)]
        Ri = None
        N = mp.matrix([[-diag[i] * H[i, j] for j in range(pa.size)] for i in range(iu.size)])
    return dict(Ri=Ri, N=N, diag=diag, logdet=mp.fsum(mp.log(d) for d in diag))


def as_ld(M):
    return np.array([[LD(str(M[i, j])) for j in range(M.cols)] for i in range(M.rows)], dtype=LD)


@pytest.mark.parametrize("q,theta", [(1, np.array([2.3, 1.0, 1.0, 6.0])), (1, np.array([2.3, 1.0, 1.0, 0.3])),
                                     (3, nice_theta(3)), (4, distinct_theta(4))],
                         ids=["q1_phi6", "q1_phi0.3", "q3_nice", "q4_distinct"])
def test_blocks_match_mpmath(q, theta):
    import mpmath as mp
    om = tiny_tree(q, nloc={1: (8, 4, 2), 3: (6, 2, 2), 4: (4, 2, 2)}[q])     # q = 4: 16-, 8- and 8-row blocks, chains of 16 / 24
    ex = ExtendedBlocks(om, theta)
    with mp.workdps(50):
        for u in range(3):
            assert om.indexing[u].size <= 18 and om.parents_indexing[u].size <= 24
            ref = mp_block(om, theta, u)
            b = ex.block(u)
            diag = np.diag(b["Ri"]) if b["isref"] else b["d"]
            assert relerr(diag, np.array([LD(str(d)) for d in ref["diag"]])) <= 1e-17, u
            if ref["Ri"] is not None:
                assert relerr(b["Ri"], as_ld(ref["Ri"])) <= 1e-17, u
            if ref["N"] is not None:
                assert relerr(b["N"], as_ld(ref["N"])) <= 1e-17, u
            lref = LD(str(ref["logdet"]))
            assert abs(b["logdet"] - lref) <= 1e-17 * max(1, abs(lref)), u


def test_ag10_entries_match_mpmath():
    """The long-double Apanasovich-Genton entries against 50-digit values: the inputs of man/CrossCovarianceAG10.Rd (q = 2,
    the set test_oracle_identities.test_cross_covariance_ag10_mpmath uses), nice_theta(3), and distinct_theta(q) for
    q = 4, 5, 6 (every per-outcome and per-pair parameter different)."""
    import mpmath as mp
    xl = np.linspace(0.0, 1.0, 10)
    g = np.array([(a, b) for b in xl for a in xl])
    th2 = np.array([1.0, 1.5, 0.1, 0.51, 1.0, 2.0, 5.0, 1.0])      # ai1, ai2, phi_i, thetamv, Dvec
    rng = np.random.default_rng(1)
    for q, theta, pts in ((2, th2, g), (3, nice_theta(3), rng.uniform(size=(30, 2)))) + \
            tuple((q, distinct_theta(q), rng.uniform(size=(30, 2))) for q in (4, 5, 6)):
        om = types.SimpleNamespace(q=q, coords=np.tile(pts, (q, 1)), mv_id=np.repeat(np.arange(1, q + 1), pts.shape[0]))
        n = om.coords.shape[0]
        i1, i2 = rng.integers(0, n, 40), rng.integers(0, n, 40)
        if q > 3:       # every ordered pair of outcomes at least once
            i1 = np.concatenate([i1, np.repeat(np.arange(q), q) * pts.shape[0] + rng.integers(0, pts.shape[0], q * q)])
            i2 = np.concatenate([i2, np.tile(np.arange(q), q) * pts.shape[0] + rng.integers(0, pts.shape[0], q * q)])
        K = covariance(om.coords, om.mv_id - 1, theta, q, i1, i2)
        with mp.workdps(50):
            Km = as_ld(mp_covariance(om, theta, i1, i2))
        assert relerr(K, Km) <= 1e-17, q


def oracle_vs_extended(pb, theta, w):
    """Max relative errors of the float64 oracle's Ri and panel N over the reference blocks, and its logdet error (nats)."""
    om = oracle_model(pb, theta=theta, w=w)
    assert om.get_loglik_comps_w(om.param_data)
    pd = om.param_data
    ex = ExtendedBlocks(om, theta)
    eRi = eN = 0.0
    ld = LD(0)
    for u in range(om.n_blocks):
        if om.block_ct_obs[u] == 0:
            continue
        b = ex.block(u)
        ld += b["logdet"]
        if not b["isref"]:
            continue
        eRi = max(eRi, relerr(pd.Rcc_invchol[u], b["Ri"]))
        if b["P"]:
            eN = max(eN, relerr(-pd.Rcc_invchol[u] @ pd.w_cond_mean_K[u], b["N"]))
    return eRi, eN, float(abs(ld - LD(pd.logdetCi)))


def test_oracle_agrees_at_nice_theta():
    w = np.random.default_rng(0).standard_normal(625)
    pb = make_problem(side=25, q=1, seed=11, missing=0.1)
    eRi, eN, eld = oracle_vs_extended(pb, pb["theta"], w)
    assert eRi <= 1e-13 and eN <= 1e-13 and eld <= 1e-13 * 625, (eRi, eN, eld)
    pb = make_problem(side=9, q=3, seed=11)
    eRi, eN, eld = oracle_vs_extended(pb, pb["theta"], np.zeros(pb["n"]))
    assert eRi <= 1e-13 and eN <= 1e-13 and eld <= 1e-13 * pb["n"], (eRi, eN, eld)
    for q, side in ((4, 10), (5, 10), (6, 8)):         # n = 400, 500, 384
        pb = make_problem(side=side, q=q, seed=11)
        eRi, eN, eld = oracle_vs_extended(pb, pb["theta"], np.zeros(pb["n"]))
        assert eRi <= 1e-13 and eN <= 1e-13 and eld <= 1e-13 * pb["n"], (q, eRi, eN, eld)


def test_oracle_loses_digits_as_phi_falls():
    """make_problem(side=25, q=1, seed=11), sigma^2 = 2.3: the float64 oracle's error against the extended reference grows as
    phi falls (measured: Ri 7e-15 / 6e-12 / 4e-10 / 1.3e-6 at phi = 6 / 0.5 / 0.05 / 1e-3), so at the bottom of the bounds
    the suite's REL = 1e-9 against the oracle says nothing about a kernel."""
    pb = make_problem(side=25, q=1, seed=11)
    w = np.random.default_rng(0).standard_normal(pb["n"])
    errs = [oracle_vs_extended(pb, np.array([2.3, 1.0, 1.0, phi]), w) for phi in (6.0, 0.5, 0.05, 1e-3)]
    for k in range(2):                       # Ri, N: monotone in phi
        col = [e[k] for e in errs]
        assert all(a < b for a, b in zip(col, col[1:])), (k, col)
    assert errs[0][0] < 1e-13 and errs[-1][0] > 1e-8 and errs[-1][1] > 1e-8, errs
    assert errs[-1][2] > 1e2 * errs[0][2], errs


# ---- the index-only view and the restated draws (what tests/test_gpu_full_size.py checks full-size runs with)
def view_and_oracle(pb, w, beta, tausq=0.2):
    from oracle.extended import WorkloadView
    om = oracle_model(pb, w=w, beta=beta, tausq=tausq)
    assert om.get_loglik_comps_w(om.param_data)
    view = WorkloadView(csr_problem(pb), beta, 1.0 / tausq, limited_tree=pb.get("limited_tree", False))
    return om, view


def csr_problem(pb):
    """pb with indexing / parents / children as the (ptr, idx) CSR pairs of make_workload."""
    t = pb["topo"]
    return dict(pb, indexing=(t.indexing_ptr, t.indexing_idx), parents=(t.parents_ptr, t.parents_idx),
                children=(t.children_ptr, t.children_idx))


@pytest.mark.parametrize("q,missing,limited", [(1, 0.1, False), (3, 0.2, False), (2, 0.0, True)],
                         ids=["q1_na", "q3_na", "q2_limited"])
def test_view_gives_the_oracle_model_blocks_bitwise(q, missing, limited):
    pb = make_problem(side=16 if q == 1 else 8, q=q, seed=4, missing=missing, limited_tree=limited)
    rng = np.random.default_rng(2)
    w, beta = rng.standard_normal(pb["n"]), rng.standard_normal(pb["p"])
    om, view = view_and_oracle(pb, w, beta)
    from oracle.extended import WorkloadView
    assert isinstance(view, WorkloadView)
    a, b = ExtendedBlocks(om, pb["theta"]), ExtendedBlocks(view, pb["theta"])
    assert np.array_equal(view.block_ct_obs, om.block_ct_obs)
    assert np.array_equal(view.y, om.y) and np.array_equal(view.XB, om.XB)
    assert np.array_equal(view.tausq_inv_long, om.tausq_inv_long)
    for u in range(om.n_blocks):
        assert np.array_equal(view.parents_indexing[u], om.parents_indexing[u]), u
        assert np.array_equal(view.children[u], om.children[u]), u
        x, y = a.block(u), b.block(u)
        for k in ("H", "N", "Ri", "d", "rdiag", "logdet"):
            if k in x:
                assert np.array_equal(x[k], y[k]), (u, k)
        assert a.loglik_comp(u, w) == b.loglik_comp(u, w), u
        if om.block_ct_obs[u] and b.block(u)["isref"]:
            assert np.array_equal(a.cond_mean(u, w), b.cond_mean(u, w)), u


@pytest.mark.parametrize("q,missing,limited", [(1, 0.1, False), (3, 0.2, False), (2, 0.1, True), (5, 0.2, False)],
                         ids=["q1_na", "q3_na", "q2_limited", "q5_na"])
def test_draws_match_the_oracle(q, missing, limited):
    """cond_draw against gibbs_sample_w (each block given the values before the sweep, its descendants' own rows after it),
    predict_draw against predict, at nice theta."""
    pb = make_problem(side=16 if q == 1 else 8, q=q, seed=6, missing=missing, limited_tree=limited)
    rng = np.random.default_rng(3)
    w0, beta, z = rng.standard_normal(pb["n"]), rng.standard_normal(pb["p"]), rng.standard_normal(pb["n"])
    om, view = view_and_oracle(pb, w0, beta)
    ex = ExtendedBlocks(view, pb["theta"])
    om.gibbs_sample_w(z)
    w1 = om.w.copy()
    checked = 0
    for u in range(om.n_blocks):
        if om.block_ct_obs[u] == 0:
            continue
        iu = om.indexing[u]
        assert relerr(ex.cond_draw(u, w0, z[iu], w_desc=w1), w1[iu]) <= 1e-12, u
        checked += 1
    assert checked > 3
    om.predict(True)
    w2 = om.w
    pred = [u for u in range(om.n_blocks) if om.block_ct_obs[u] == 0 and om.indexing[u].size]
    assert pred
    for u in pred:
        iu = om.indexing[u]
        assert relerr(ex.predict_draw(u, w2, z[iu]), w2[iu]) <= 1e-12, u


@pytest.mark.parametrize("q,limited", [(1, False), (3, False), (2, True), (6, False)], ids=["q1", "q3", "q2_limited", "q6"])
def test_prior_draw_matches_the_restated_prior_sweep(q, limited):
    from tests.prior_sweep import prior_sweep
    pb = make_problem(side=16 if q == 1 else 8, q=q, seed=8, limited_tree=limited)
    z = np.random.default_rng(4).standard_normal(pb["n"])
    om, view = view_and_oracle(pb, np.zeros(pb["n"]), np.zeros(pb["p"]))
    W = prior_sweep(om, z)[:, 0]
    ex = ExtendedBlocks(view, pb["theta"])
    for u in range(om.n_blocks):
        iu = om.indexing[u]
        if iu.size:
            assert relerr(ex.prior_draw(u, W, z[iu]), W[iu]) <= 1e-12, u


@pytest.mark.parametrize("q", [1, 3, 5])
def test_point_moments_equal_the_dense_identity(q):
    """The new-point mean and variance on the anchor's chain against the dense kriging identity on its conditioning set (the
    one test_gpu_predict_points checks the kernels with)."""
    from oracle.spamtree_oracle import CovarianceParams, Covariancef
    from spamtree_amd.predict import conditioning_set, locate
    pb = make_problem(side=16 if q == 1 else 9, q=q, seed=5, missing=0.1)
    topo = pb["topo"]
    rng = np.random.default_rng(6)
    w = rng.standard_normal(pb["n"])
    _, view = view_and_oracle(pb, w, np.zeros(pb["p"]))
    ex = ExtendedBlocks(view, pb["theta"])
    pts = rng.uniform(size=(60, 2))
    mv = rng.integers(1, q + 1, size=60)
    anchor = locate(topo, pts, mv)
    cp = CovarianceParams(2, q)
    cp.transform(pb["theta"])
    allc = np.vstack([topo.coords, pts])
    allv = np.concatenate([topo.mv_id - 1, mv - 1])
    n = pb["n"]
    for i in range(pts.shape[0]):
        S = np.concatenate([topo.indexing(int(b)) for b in conditioning_set(topo, int(anchor[i]))])
        Kss = Covariancef(allc, allv, S, S, cp, same=True)
        ks = Covariancef(allc, allv, S, [n + i], cp)[:, 0]
        kxx = Covariancef(allc, allv, [n + i], [n + i], cp)[0, 0]
        sol = np.linalg.solve(Kss, np.column_stack([w[S], ks]))
        mean, var = ex.point_moments(int(anchor[i]), pts[i:i + 1], mv[i:i + 1], w)
        assert abs(float(mean[0]) - ks @ sol[:, 0]) <= 1e-10 * max(1.0, abs(ks @ sol[:, 0])), i
        assert abs(float(var[0]) - max(kxx - ks @ sol[:, 1], 0)) <= 1e-10 * max(1.0, kxx), i
