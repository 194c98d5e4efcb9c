"""GPU: the leaf bodies of k_factor_quad gather g = Linv_pa w_pa from the residuals e = Ri (w_u - H_u w_pa) that every
phase-A route stores for the reference blocks (st_get_resid), instead of forming it from the staged chain rows.

(a) The six rows of tests/test_gpu_leaf_g.py (SPAMTREE_QUAD_MIN=1, every level on k_factor_quad): after st_factor on slot 0
    and after a proposal on slot 1 the stored residuals of the reference blocks against Ri_u (w_u - H_u w_pa) from the oracle's
    per-block factors at tests/test_gpu_parity.py's REL, and each reference block's loglik_w component against
    -m log(2 pi)/2 - sum(e^2)/2 of the returned vector (comp_tol below).
(b) One row per other route that writes a reference block's component -- k_factor_mfma, k_factor_wide,
    k_factor_lchain + k_factor_ref_finish, k_factor_bigmfma, the generic k_factor -- asserted from st_route_info, the same
    comparison.
(c) Top levels factorised ahead of time (st_factor_begin) with the w of the sweep's start: after the sweep, st_factor must
    leave components and residuals of the NEW w (fix_top_comps runs before the levels below); the same with
    SPAMTREE_ASYNC_TOP=0.
(d) A limited tree whose leaf level takes k_factor_quad: there the chain is the parent's marginal factor and
    k_marginal_invchol* store chol(K_pa)^{-1} w_pa; components and log-density against the oracle."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_leaf_deferral import QUAD_MIN, enqueue, model
from tests.test_gpu_leaf_g import BETA, ROWS, TAUSQ, build, leaf_routes
from tests.test_gpu_parity import REL, relerr
from tests.test_gpu_routes import WIDE_ROUTES, build_problem, hip_model, inputs, quad
from tests.util import make_problem, oracle_model

pytestmark = pytest.mark.gpu

HL2PI = -0.91893853320467274178032973640562      # -log(2 pi) / 2 (st_device.hpp; spamtree_model.h:20)
U = 2.0 ** -53      # unit roundoff


def comp_tol(m, quad_half):
    """-m log(2 pi)/2 - sum(e_i^2)/2 in double: m squares (one rounding each, or none when the multiply is contracted into the
    add), m - 1 additions in whatever order the route sums them, the scaling and the final subtraction -- to first order at
    most (m + 2) roundings, each relative to a partial result no larger than the two terms' magnitudes together."""
    return (m + 2) * U * (m * abs(HL2PI) + quad_half)


def get_resid(m):
    out = np.full(m.n_all, np.nan)
    assert m.lib.st_get_resid(m.h, out.ctypes.data_as(C.POINTER(C.c_double)), m.n_all) == 0
    bad = np.zeros(1)
    assert m.lib.st_get_resid(m.h, bad.ctypes.data_as(C.POINTER(C.c_double)), 1) < 0      # n must be n_all
    return out


def ref_blocks(om):
    return [u for u in range(om.n_blocks) if om.block_ct_obs[u] > 0 and om.block_is_reference[u]]


def oracle_resid(om, data):
    """Per observed reference block: Ri_u (w_u - H_u w_pa) from the oracle's per-block factors and its current w."""
    out = {}
    for u in ref_blocks(om):
        r = om.w[om.indexing[u]].copy()
        if om.parents[u].size:
            r -= data.w_cond_mean_K[u] @ om.w[om.parents_indexing[u]]
        out[u] = data.Rcc_invchol[u] @ r
    return out


def check_resid(om, data, resid, comps, blocks=None):
    """The stored residuals against the oracle's, and every reference block's loglik_w component against the stored vector."""
    want = oracle_resid(om, data)
    blocks = list(want) if blocks is None else blocks
    assert blocks
    scale = max(np.abs(e).max() for e in want.values())
    worst = 0.0
    for u in blocks:
        e = resid[om.indexing[u]]
        assert np.all(np.isfinite(e)), u
        worst = max(worst, float(np.abs(e - want[u]).max()) / scale)
        m = e.size
        qh = 0.5 * float(np.sum(e.astype(np.longdouble) ** 2))
        exact = float(np.longdouble(m) * np.longdouble(HL2PI) - np.longdouble(qh))
        assert abs(comps[1][u] - exact) <= comp_tol(m, qh), (u, comps[1][u], exact, comp_tol(m, qh))
    print("residuals: worst relative error", worst, "over", len(blocks), "blocks")
    assert worst <= REL


def check_comps(comps, data):
    assert relerr(comps[0], data.logdetCi_comps) <= REL
    assert relerr(comps[1], data.loglik_w_comps) <= REL


# ---- (a) the quad rows
@pytest.mark.parametrize("row", ROWS, ids=[r["id"] for r in ROWS])
def test_quad_rows_store_the_residuals_the_leaf_level_gathers(row, monkeypatch):
    for k, v in QUAD_MIN.items():
        monkeypatch.setenv(k, v)
    pb = build(row)
    th2 = pb["theta"] * 1.07
    om = oracle_model(pb, w=np.random.default_rng(1).standard_normal(pb["n"]), beta=BETA, tausq=TAUSQ)      # model()'s w
    assert om.get_loglik_comps_w(om.param_data)
    om.theta_update(om.alter_data, th2)
    assert om.get_loglik_comps_w(om.alter_data)
    m = model(pb, True)
    assert m.get_loglik_comps_w(0)
    assert row["leaf"] in leaf_routes(m), leaf_routes(m)
    ref_a = {a for g in m.route_info()["levels"] for a in g["A"] if "k_factor_quad" in a and a.endswith(("true, true>", "true, false>"))}
    assert ref_a, m.route_info()      # at least one reference level on k_factor_quad<.., true, WCH>
    if row["id"] == "strip_nkx50":
        assert quad(32, True, False) in ref_a, ref_a      # 30-row blocks: the team elimination's epilogue (128-thread form)
    if row["id"] == "strip_nkx38":
        assert any(a.endswith("true, true>") for a in ref_a), ref_a      # 24-row blocks: the wave elimination's
    comps0 = m.comps(0)
    check_comps(comps0, om.param_data)
    check_resid(om, om.param_data, get_resid(m), comps0)
    ll1 = enqueue(m, 1, th2)      # the proposal: the V-only leaf body gathers what this factorisation stored
    assert abs(ll1 - om.alter_data.loglik_w) <= REL * abs(om.alter_data.loglik_w)
    comps1 = m.comps(1)
    check_comps(comps1, om.alter_data)
    check_resid(om, om.alter_data, get_resid(m), comps1)
    m.close()


# ---- (b) every other writer
def _wide(rid):
    return next(r for r in WIDE_ROUTES if r["id"] == rid)


WRITERS = [
    dict(id="mfma", row=dict(side=25, kw=dict(missing=0.12), env={}), ref_routes=["k_factor_mfma"]),
    dict(id="wide", row=_wide("wide4_sibling_groups"), ref_routes=["k_factor_wide<WG_JT>"]),
    dict(id="lchain_ref_finish", row=_wide("wide4_default_pred"), ref_routes=["k_factor_ref_finish"]),
    dict(id="bigmfma", row=_wide("wide4_bigmfma"), ref_routes=["k_factor_bigmfma<5, 3, 24>"]),
    dict(id="generic", row=_wide("wide4_generic"), ref_routes=["k_factor<true, MODE_FACTOR>"]),
]
_ORACLE = {}      # per problem: the oracle after phase A on its param_data (rows of one problem share it; nothing changes it)


def writer_oracle(row, pb, inp):
    key = repr((row.get("side"), row.get("strip"), sorted(row["kw"].items())))
    if key not in _ORACLE:
        om = oracle_model(pb, w=inp["w"], beta=inp["beta"], tausq=inp["tausq"])
        assert om.get_loglik_comps_w(om.param_data)
        _ORACLE[key] = om
    return _ORACLE[key]


@pytest.mark.parametrize("case", WRITERS, ids=[c["id"] for c in WRITERS])
def test_every_reference_route_stores_its_residuals(case, monkeypatch):
    row = case["row"]
    for k, v in row["env"].items():
        monkeypatch.setenv(k, v)
    pb = build_problem(row)
    inp = inputs(pb)
    om = writer_oracle(row, pb, inp)
    hm = hip_model(pb, force_generic=row.get("force_generic", False), **inp)
    assert hm.get_loglik_comps_w(0)
    levels = hm.route_info()["levels"]
    info = hm.level_info()
    # the levels of reference blocks: all but the last one (the leaf level)
    ran = {a for g in levels[:-1] for a in g["A"]}
    for name in case["ref_routes"]:
        assert name in ran, (name, levels, info)
    comps = hm.comps(0)
    check_comps(comps, om.param_data)
    check_resid(om, om.param_data, get_resid(hm), comps)
    hm.close()


# ---- (c) top levels that ran ahead of time
@pytest.mark.parametrize("async_top", ["1", "0"])
def test_top_levels_ahead_of_time_leave_residuals_of_the_current_w(async_top, monkeypatch):
    monkeypatch.setenv("SPAMTREE_QUAD_MIN", "1")
    monkeypatch.setenv("SPAMTREE_QUAD_UNITS", "4")
    monkeypatch.setenv("SPAMTREE_ASYNC_TOP", async_top)
    pb = make_problem(side=40, q=1, seed=3, missing=0.05)
    th2 = pb["theta"] * 1.07
    z = np.random.default_rng(23).standard_normal(pb["n"])
    om = oracle_model(pb, w=np.random.default_rng(1).standard_normal(pb["n"]), beta=BETA, tausq=TAUSQ)
    assert om.get_loglik_comps_w(om.param_data)
    w_start = om.w.copy()
    om.gibbs_sample_w(z)
    assert np.abs(om.w - w_start).max() > 0.1      # the sweep moved w: residuals of the old w would be far off
    om.theta_update(om.alter_data, th2)
    assert om.get_loglik_comps_w(om.alter_data)      # with the NEW w

    m = model(pb, True)
    ahead = m.lib.st_factor_ahead_levels(m.h)
    assert (ahead > 0) == (async_top == "1"), ahead
    assert m.get_loglik_comps_w(0)
    th = np.ascontiguousarray(th2, dtype=np.float64)
    assert m.lib.st_factor_begin(m.h, 1, th.ctypes.data_as(C.POINTER(C.c_double)), th.size) == 0
    m.deal_with_w(z)
    m.theta_update(1, th2)
    assert m.get_loglik_comps_w(1)
    assert leaf_routes(m), m.route_info()      # the leaf level gathers: k_factor_quad
    assert abs(m.loglik_w[1] - om.alter_data.loglik_w) <= REL * abs(om.alter_data.loglik_w)
    comps = m.comps(1)
    check_comps(comps, om.alter_data)
    resid = get_resid(m)
    check_resid(om, om.alter_data, resid, comps)
    if ahead > 0:      # ... and the blocks of the levels that ran ahead on their own
        labels = np.sort(np.unique(np.asarray(pb["block_groups"])[[u for u in range(om.n_blocks) if om.block_ct_obs[u] > 0]]))
        top = [u for u in ref_blocks(om) if pb["block_groups"][u] in labels[:ahead]]
        check_resid(om, om.alter_data, resid, comps, blocks=top)
    m.close()


# ---- (d) limited tree
def test_limited_tree_leaf_quads_gather_the_marginal_g(monkeypatch):
    for k, v in QUAD_MIN.items():
        monkeypatch.setenv(k, v)
    pb = make_problem(side=25, q=1, seed=11, missing=0.1, limited_tree=True)
    inp = inputs(pb)
    om = oracle_model(pb, w=inp["w"], beta=inp["beta"], tausq=inp["tausq"])
    assert om.get_loglik_comps_w(om.param_data)
    om.theta_update(om.alter_data, inp["theta2"])
    assert om.get_loglik_comps_w(om.alter_data)
    hm = hip_model(pb, **inp)
    assert hm.lib.st_factor_ahead_levels(hm.h) == 0
    for slot, data in ((0, om.param_data), (1, om.alter_data)):
        hm.theta_update(slot, inp["theta2"] if slot else inp["theta"])
        assert hm.get_loglik_comps_w(slot)
        levels = hm.route_info()["levels"]
        assert "k_marginal_invchol_wave" in levels[0]["A"], levels
        assert levels[-1]["A"] == [quad(32, False, True)], levels
        check_comps(hm.comps(slot), data)
        assert abs(hm.loglik_w[slot] - data.loglik_w) <= REL * abs(data.loglik_w)
        # what the marginal kernels stored: chol(K_uu)^{-1} w_u of every observed reference block
        resid = get_resid(hm)
        worst = 0.0
        om.covpars.transform(data.theta)
        for u in ref_blocks(om):
            Kuu = om._cov(om.indexing[u], om.indexing[u], True)
            want = np.linalg.solve(np.linalg.cholesky(Kuu), om.w[om.indexing[u]])
            worst = max(worst, float(np.abs(resid[om.indexing[u]] - want).max()) / max(1e-300, float(np.abs(want).max())))
        print("marginal g: worst relative error", worst)
        assert worst <= REL
    hm.close()
