"""GPU: a proposal's quad leaf levels factorised without T (st_factor_enqueue on slot 1), their panels finished from the
stored V by the first call that reads the slot.  Log-density terms bitwise equal to the full factorisation, panels bitwise
equal to st_factor's through every reader of a pending slot, chains with the deferral on and off identical."""
import ctypes as C

import numpy as np
import pytest

from tests.util import make_problem, strip_coords

pytestmark = pytest.mark.gpu

QUAD_MIN = {"SPAMTREE_QUAD_MIN": "1"}
LEAF = "k_factor_quad<4, {}, {}, false, true>"
# id, problem, environment, the leaf instantiation the row must reach
CASES = [
    dict(id="grid_na10_nkx32", side=40, kw=dict(missing=0.1), env=QUAD_MIN, leaf=LEAF.format(32, 8)),
    dict(id="grid_na30_two_units", side=36, kw=dict(missing=0.3), env=dict(QUAD_MIN, SPAMTREE_QUAD_UNITS="2"), leaf=LEAF.format(32, 8)),
    dict(id="strip_nkx44", strip=(1280, 4, 1), kw=dict(cell_size=31, tree_depth=7, missing=0.15), env=QUAD_MIN, leaf=LEAF.format(44, 11)),
    dict(id="strip_nkx50", strip=(640, 5, 1), kw=dict(cell_size=31, tree_depth=6, missing=0.15), env=QUAD_MIN, leaf=LEAF.format(50, 13)),
]


def problem(row):
    if "side" in row:
        return make_problem(side=row["side"], q=1, seed=3, **row["kw"])
    nx, ny, q = row["strip"]
    coords, mv = strip_coords(nx, ny, q)
    return make_problem(coords=coords, mv_id=mv, q=q, seed=11, K=(2, 1), **row["kw"])


def model(pb, defer):
    from spamtree_amd.model import SpamTreeMV
    m = SpamTreeMV(pb["y"], pb["X"], pb["Z"], pb["coords"], pb["mv_id"], pb["blocking"], pb["gix_block"], pb["res_is_ref"],
                   pb["parents"], pb["children"], False, pb["block_names"], pb["block_groups"], pb["indexing"],
                   np.random.default_rng(1).standard_normal(pb["n"]), np.array([0.3, -0.2, 0.1]), pb["theta"], 5.0,
                   defer_leaf=defer)
    return m


def enqueue(m, slot, theta):
    th = np.ascontiguousarray(theta, dtype=np.float64)
    assert m.lib.st_factor_enqueue(m.h, slot, th.ctypes.data_as(C.POINTER(C.c_double)), th.size) == 0
    ll = C.c_double()
    assert m.lib.st_factor_finish(m.h, C.byref(ll)) == 0
    return ll.value


def blocks(m, slot):
    from spamtree_amd.model import SpamTreeError
    out = []
    for u in range(m.n_blocks):
        try:
            out.append(m.block(slot, u, raw=True))
        except SpamTreeError:      # a block without observations has no cache
            out.append(None)
    return out


def same_blocks(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])


def read(m, reader):
    """The first read of the pending slot 1 (it finishes the deferred leaf panels), then everything the test compares."""
    out = {}
    if reader == "get_block":
        out["b1"] = blocks(m, 1)
    elif reader == "loglik_w":
        out["ll"] = m.get_loglik_w(1)
    elif reader == "sample_w_loglik":
        ll = C.c_double()
        assert m.lib.st_sample_w_loglik(m.h, None, C.c_uint64(17), C.c_uint32(3), 1, C.byref(ll)) == 0
        out["ll"] = ll.value
        out["w"] = m.get_w()
    elif reader == "swap":
        m.accept_make_change()
        out["b0"] = blocks(m, 0)
    if "b1" not in out and reader != "swap":
        out["b1"] = blocks(m, 1)
    return out


@pytest.mark.parametrize("reader", ["get_block", "loglik_w", "sample_w_loglik", "swap"])
@pytest.mark.parametrize("row", CASES, ids=[r["id"] for r in CASES])
def test_pending_slot_is_bitwise_the_full_factorisation(row, reader, monkeypatch):
    for k, v in row["env"].items():
        monkeypatch.setenv(k, v)
    pb = problem(row)
    th_b = pb["theta"] * 1.07
    got = {}
    for defer in (True, False):
        m = model(pb, defer)
        assert m.get_loglik_comps_w(0)
        ll = enqueue(m, 1, th_b)
        if defer:
            leaf = [a for g in m.route_info()["levels"] for a in g["A"] if a.endswith("false, true>")]
            assert row["leaf"] in leaf, leaf
        comps = m.comps(1)
        got[defer] = (ll, comps, read(m, reader))
        m.close()
    a, b = got[True], got[False]
    assert a[0] == b[0]
    assert np.array_equal(a[1][0], b[1][0]) and np.array_equal(a[1][1], b[1][1])
    assert a[2].keys() == b[2].keys()
    for k in a[2]:
        if k in ("b0", "b1"):
            same_blocks(a[2][k], b[2][k])
        elif k == "w":
            assert np.array_equal(a[2][k], b[2][k])
        else:
            assert a[2][k] == b[2][k]


def test_refactorising_a_pending_slot_drops_the_deferred_half(monkeypatch):
    for k, v in QUAD_MIN.items():
        monkeypatch.setenv(k, v)
    pb = make_problem(side=40, q=1, seed=3, missing=0.1)
    m, ref = model(pb, True), model(pb, False)
    for x in (m, ref):
        assert x.get_loglik_comps_w(0)
    enqueue(m, 1, pb["theta"] * 1.07)        # pending, then replaced by a synchronous full factorisation at another theta
    ref.theta[1] = m.theta[1] = pb["theta"] * 0.93
    assert m.get_loglik_comps_w(1) and ref.get_loglik_comps_w(1)
    m.accept_make_change()
    ref.accept_make_change()
    same_blocks(blocks(m, 0), blocks(ref, 0))
    m.close()
    ref.close()


def test_driver_chains_with_and_without_deferral_are_identical(monkeypatch):
    from spamtree_amd import fit
    for k, v in QUAD_MIN.items():
        monkeypatch.setenv(k, v)
    pb = make_problem(side=40, q=1, seed=3, missing=0.1)
    res = []
    for defer in (True, False):
        ch = fit.Chain(pb["y"], pb["X"], pb["Z"], pb["coords"], pb["mv_id"], pb["blocking"], pb["gix_block"], pb["res_is_ref"],
                       pb["parents"], pb["children"], False, pb["block_names"], pb["block_groups"], pb["indexing"],
                       pb["bounds"], pb["theta"], np.zeros(pb["p"]), 0.1, 0.01 * np.eye(pb["theta"].size), seed=5, defer_leaf=defer)
        thetas = []
        for _ in range(60):
            ch.step(1)
            thetas.append(ch.state()["theta"].copy())
        st = ch.state()
        res.append((np.array(thetas), st["tausq_inv"].copy(), float(st["loglik"]), ch.get_w().copy()))
        ch.close()
    a, b = res
    assert len({tuple(t) for t in a[0]}) > 2, "no accepted proposal: the deferred half was never finished"
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and np.array_equal(a[3], b[3])
