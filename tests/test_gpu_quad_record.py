"""GPU: k_factor_quad started from the quad records (one LDS-DMA round and one barrier instead of the descriptor and coordinate
gathers), against the oracle, on the four shapes of tests/test_gpu_leaf_deferral.py with SPAMTREE_QUAD_MIN=1: leaf
instantiations NKX 32, 44 and 50, chains that straddle the 32-row steps, private ancestors above and below 16 rows, quads of
one, two and four units.  In order: st_factor on slot 0 (full bodies of the reference and leaf instantiations), a proposal
through st_factor_enqueue / st_factor_finish (the leaf level's V-only body), the swap (its completion body), a sweep (for
st_predict's normals) and st_predict on the rows without an observation (phase P on the leaf body).

Tolerances: those of tests/test_gpu_parity.py for the same quantities -- 1e-9 relative to the largest magnitude of the
compared array for log-densities, their per-block components, the factors Ri and the draws of w, 1e-8 for H recovered
from a stored panel by a solve."""
import numpy as np
import pytest

from tests.test_gpu_leaf_deferral import CASES, enqueue, problem
from tests.test_gpu_parity import REL, hip_model, relerr
from tests.util import oracle_model

pytestmark = pytest.mark.gpu

# the reference instantiations each row's st_factor must reach besides its leaf instantiation, and phase P's kernel
REF = "k_factor_quad<4, {}, {}, true, {}>"
EXPECT = {
    "grid_na10_nkx32": dict(ref=[REF.format(32, 8, "true")]),
    "grid_na30_two_units": dict(ref=[REF.format(32, 8, "true")]),
    # 1280 x 4 points in cells of 31 over seven levels: reference blocks of at most 27 rows, the one-wave elimination
    "strip_nkx44": dict(ref=[REF.format(32, 8, "true"), REF.format(38, 10, "true")]),
    # 640 x 5 points over six levels: 30-row reference blocks, the team elimination (tests/test_gpu_routes.py, ref30_leaf50_pred50)
    "strip_nkx50": dict(ref=[REF.format(32, 8, "false"), REF.format(38, 10, "false")]),
}


def same_as_oracle(hm, om, data, slot):
    ld, ll = hm.comps(slot)
    assert relerr(ld, data.logdetCi_comps) <= REL
    assert relerr(ll, data.loglik_w_comps) <= REL
    for u in range(om.n_blocks):
        if om.block_ct_obs[u] == 0:
            continue
        H, Ri = hm.block(slot, u)
        if om.parents[u].size:
            assert relerr(H, data.w_cond_mean_K[u]) <= 1e-8, u
        if om.block_is_reference[u]:
            assert relerr(Ri, data.Rcc_invchol[u]) <= REL, u
        else:
            assert relerr(Ri, data.ccholprecdiag[u]) <= REL, u


@pytest.mark.parametrize("row", CASES, ids=[r["id"] for r in CASES])
def test_factor_proposal_completion_and_predict_match_the_oracle(row, monkeypatch):
    for k, v in row["env"].items():
        monkeypatch.setenv(k, v)
    pb = problem(row)
    rng = np.random.default_rng(5)
    w0 = rng.standard_normal(pb["n"])
    beta = np.array([0.3, -0.2, 0.1])
    om = oracle_model(pb, w=w0, beta=beta, tausq=0.2)
    hm = hip_model(pb, w=w0, beta=beta, tausq=0.2)
    assert np.any(np.asarray(om.block_ct_obs) == 0)      # there are rows to predict
    # ---- 1. the full factorisation of slot 0
    assert om.get_loglik_comps_w(om.param_data) and hm.get_loglik_comps_w(0)
    ran = [a for g in hm.route_info()["levels"] for a in g["A"]]
    print(row["id"], "phase A:", sorted(set(ran)))
    assert row["leaf"] in ran, ran
    for name in EXPECT[row["id"]]["ref"]:
        assert name in ran, ran
    assert abs(hm.loglik_w[0] - om.param_data.loglik_w) <= REL * abs(om.param_data.loglik_w)
    same_as_oracle(hm, om, om.param_data, 0)
    # ---- 2. a proposal: the leaf level V only
    th2 = pb["theta"] * 1.07
    om.theta_update(om.alter_data, th2)
    assert om.get_loglik_comps_w(om.alter_data)
    ll = enqueue(hm, 1, th2)
    ran = [a for g in hm.route_info()["levels"] for a in g["A"]]
    assert row["leaf"] in ran, ran
    assert abs(ll - om.alter_data.loglik_w) <= REL * abs(om.alter_data.loglik_w)
    ld, llc = hm.comps(1)
    assert relerr(ld, om.alter_data.logdetCi_comps) <= REL and relerr(llc, om.alter_data.loglik_w_comps) <= REL
    # ---- 3. the swap finishes the leaf panels from the stored V
    hm.theta[1] = th2
    om.accept_make_change()
    hm.accept_make_change()
    same_as_oracle(hm, om, om.param_data, 0)
    # ---- 4. a sweep, then the prediction of the rows without an observation
    z = rng.standard_normal(pb["n"])
    om.gibbs_sample_w(z)
    hm.deal_with_w(z)
    assert relerr(hm.get_w()[om.na_ix_all], om.w[om.na_ix_all]) <= REL
    om.predict(True)
    hm.predict(True)
    print(row["id"], "phase P:", hm.route_info()["predict"])
    assert hm.route_info()["predict"] == row["leaf"]
    assert relerr(hm.get_w(), om.w) <= REL
    hm.close()
