"""GPU: g = Linv_pa w_pa of the leaf k_factor_quad (factor_quad.hpp, grow) with a row's operands requested together and the
lane-group sum by DPP moves instead of shuffles; phase P without g.

(a) The sum helper through st_probe_group_sum: group_xor_sum (DPP) against the __shfl_xor butterfly with the same partners
    and order, NS = 8 and 16, bitwise.

(b) Phase A through the C-ABI with SPAMTREE_QUAD_MIN=1 (small levels take k_factor_quad), one row per shape of the g pass.
    The rows are those of tests/test_gpu_leaf_deferral.py, tests/test_gpu_quad_modes.py and tests/test_gpu_routes.py, each
    with the shape it stands for asserted from st_level_info (pm: the widest private ancestor = the last reference level's
    max_m; Pc: the leaf level's shared chain = that level's max_P) and st_route_info:
      grid_leaf32_pred32   NKX 32 (chains <= 128); units of <= 16 columns (an idle jt = 1 wave) and quads of fewer than four
                           units (tests/test_quad_record_cpu.py proves both for this row on the CPU); two private sub-panels
      strip_nkx38          NKX 38 (<= 152); 24-row ancestors: pm in 17..24 (packed second sub-panel), every 32-row step
                           straddles two ancestors (rows of different length), Pc not a multiple of 32
      strip_nkx44          NKX 44 (<= 176)
      strip_nkx50          NKX 50 (<= 200); pm > 24
      cell9_one_subpanel   pm = 9 (one sub-panel), Pc = 27: one step of 27 rows
      cell4x6_packed_shared  pm = 24, Pc = 48: the chain's first step (16 rows) sits behind the packed sub-panel (pf)
    Per row: per-block logdetCi / loglik_w components of the full body (st_factor, slot 0) and of the V-only body (a proposal
    on slot 1) against the oracle at tests/test_gpu_parity.py's REL = 1e-9; the proposal with and without leaf deferral
    (st_options.reserved bit 2: defer_leaf) bitwise equal in its components and, after st_swap, in the leaf panels; st_predict
    (phase P: the full body without g) fills w bitwise as the build before this change did -- tests/golden/leaf_g_predict/,
    recorded on an MI355X from that build by the same `sequence` below."""
import os

import numpy as np
import pytest

from tests.test_gpu_leaf_deferral import LEAF, QUAD_MIN, blocks, enqueue, model, problem, same_blocks
from tests.test_gpu_parity import REL, relerr
from tests.util import make_problem, oracle_model

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "leaf_g_predict")     # one <row id>.npy per row
STRIP = dict(cell_size=31, missing=0.15)
ROWS = [
    dict(id="grid_leaf32_pred32", side=25, seed=11, kw=dict(missing=0.12), leaf=LEAF.format(32, 8), shape=lambda pm, Pc: pm > 16),
    dict(id="strip_nkx38", strip=(640, 4, 1), kw=dict(STRIP, tree_depth=6), leaf=LEAF.format(38, 10),
         shape=lambda pm, Pc: 17 <= pm <= 24 and Pc % 32 != 0 and 32 % pm != 0 and Pc + pm <= 152),
    dict(id="strip_nkx44", strip=(1280, 4, 1), kw=dict(STRIP, tree_depth=7), leaf=LEAF.format(44, 11), shape=lambda pm, Pc: 152 < Pc + pm <= 176),
    dict(id="strip_nkx50", strip=(640, 5, 1), kw=dict(STRIP, tree_depth=6), leaf=LEAF.format(50, 13), shape=lambda pm, Pc: pm > 24 and 176 < Pc + pm <= 200),
    dict(id="cell9_one_subpanel", side=36, seed=3, kw=dict(missing=0.1, cell_size=9), leaf=LEAF.format(32, 8), shape=lambda pm, Pc: (pm, Pc) == (9, 27)),
    dict(id="cell4x6_packed_shared", side=40, seed=3, kw=dict(missing=0.1, cell_size=(4, 6)), leaf=LEAF.format(32, 8),
         shape=lambda pm, Pc: (pm, Pc) == (24, 48)),
]
BETA = np.array([0.3, -0.2, 0.1])      # what tests.test_gpu_leaf_deferral.model gives its handles, for the oracle
TAUSQ = 0.2


def build(row):
    if "side" in row:
        return make_problem(side=row["side"], q=1, seed=row["seed"], **row["kw"])
    return problem(row)


def leaf_routes(m):
    return [a for g in m.route_info()["levels"] for a in g["A"] if a.endswith("false, true>")]


def sequence(pb, row, defer):
    """One handle: full factorisation, a proposal, its acceptance, a sweep, the prediction.  Returns what the test compares."""
    m = model(pb, defer)
    out = {}
    info = m.level_info()
    out["pm"], out["Pc"] = info[-2]["max_m"], info[-2]["max_P"]
    assert info[-1]["kernel"] == "k_factor_quad", info
    assert m.get_loglik_comps_w(0)
    assert row["leaf"] in leaf_routes(m), leaf_routes(m)
    out["comps0"] = m.comps(0)
    out["ll1"] = enqueue(m, 1, pb["theta"] * 1.07)
    assert row["leaf"] in leaf_routes(m), leaf_routes(m)
    out["comps1"] = m.comps(1)
    m.accept_make_change()
    out["b0"] = blocks(m, 0)
    m.deal_with_w(None, seed=5, it=1)
    m.predict(True)
    assert m.route_info()["predict"] == row["leaf"], m.route_info()["predict"]
    out["w_pred"] = m.get_w().copy()
    m.close()
    return out


@pytest.mark.parametrize("ns", [8, 16])
def test_group_sum_by_dpp_is_bitwise_the_shuffle_butterfly(ns):
    from spamtree_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(ns)
    # 32 waves: magnitudes spread over 60 binades and both signs, so that every addition of the tree rounds
    x = np.ascontiguousarray(rng.standard_normal(64 * 32) * np.exp2(rng.integers(-30, 30, 64 * 32)))
    got = {}
    for dpp in (0, 1):
        out = np.full(x.size, np.nan)
        assert lib.st_probe_group_sum(ns, dpp, x.ctypes.data_as(_lib.c_dp), x.size, 0, out.ctypes.data_as(_lib.c_dp)) == 0
        got[dpp] = out
    assert np.array_equal(got[0].view(np.uint64), got[1].view(np.uint64))
    # ... and it is the group's sum, the same in each of its lanes
    grp = got[1].reshape(-1, ns)
    assert np.all(grp == grp[:, :1])
    exact = x.reshape(-1, ns).astype(np.longdouble)
    assert np.all(np.abs(grp[:, 0] - exact.sum(axis=1)) <= 4 * np.finfo(np.float64).eps * np.abs(exact).sum(axis=1))
    bad = np.zeros(64)
    assert lib.st_probe_group_sum(4, 1, bad.ctypes.data_as(_lib.c_dp), 64, 0, bad.ctypes.data_as(_lib.c_dp)) < 0
    assert lib.st_probe_group_sum(8, 1, bad.ctypes.data_as(_lib.c_dp), 63, 0, bad.ctypes.data_as(_lib.c_dp)) < 0


@pytest.mark.parametrize("row", ROWS, ids=[r["id"] for r in ROWS])
def test_leaf_g_full_vonly_and_predict(row, monkeypatch):
    for k, v in QUAD_MIN.items():
        monkeypatch.setenv(k, v)
    pb = build(row)
    th2 = pb["theta"] * 1.07
    a, b = sequence(pb, row, True), sequence(pb, row, False)
    print(row["id"], "pm", a["pm"], "Pc", a["Pc"])
    assert row["shape"](a["pm"], a["Pc"]), (a["pm"], a["Pc"])
    # ---- the oracle: the full body (slot 0) and the V-only body (the proposal)
    om = oracle_model(pb, w=np.random.default_rng(1).standard_normal(pb["n"]), beta=BETA, tausq=TAUSQ)
    assert om.get_loglik_comps_w(om.param_data)
    om.theta_update(om.alter_data, th2)
    assert om.get_loglik_comps_w(om.alter_data)
    for got, data in ((a["comps0"], om.param_data), (a["comps1"], om.alter_data)):
        assert relerr(got[0], data.logdetCi_comps) <= REL
        assert relerr(got[1], data.loglik_w_comps) <= REL
    assert abs(a["ll1"] - om.alter_data.loglik_w) <= REL * abs(om.alter_data.loglik_w)
    # ---- deferral on (V only, completed at the swap) against off (the full body): the same bits
    assert a["ll1"] == b["ll1"]
    for k in ("comps0", "comps1"):
        assert np.array_equal(a[k][0], b[k][0]) and np.array_equal(a[k][1], b[k][1]), k
    same_blocks(a["b0"], b["b0"])
    # ---- phase P: w as the build before the g pass was skipped there filled it
    assert np.any(~np.isfinite(pb["y"]))
    assert np.array_equal(a["w_pred"], b["w_pred"])
    want = np.load(os.path.join(GOLDEN, row["id"] + ".npy"))
    assert np.array_equal(a["w_pred"].view(np.uint64), want.view(np.uint64))
