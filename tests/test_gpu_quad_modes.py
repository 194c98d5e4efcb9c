"""GPU: the three bodies of the leaf k_factor_quad (V only, completion from the stored V, full) reached through one code
object, bitwise against a handle that never defers (defer_leaf=False: the full body only).

test_mode_sequence walks one handle through V only (a proposal), the completion (its acceptance), full + phase P
(st_predict), full (a synchronous factorisation) and compares everything it reads on the way.

test_step_shapes covers the shapes of the private (last) ancestor's sub-panels and of the shared chain's steps on q = 1
grids of side 36-40 with 10 % missing rows.  Every row asserts the shape it stands for from st_level_info: the last
reference level's max_m is the widest private ancestor (pm) and its max_P the leaf level's shared chain (Pc, the ancestors
above it), whose step with the chain's last rows has (Pc - 1) % 32 + 1 rows.  Two of the shapes need other cells than the
scalar cell_size of their row, and the scalar rows are kept next to them with what they really are:
  * cell_size=25 gives 25-row ancestors (packed second sub-panel of 12 rows), but Pc is then a multiple of 25 and a grid of
    side <= 48 with 10 % missing rows has fewer observed rows than four reference levels need (25 + 100 + 400 + 1600), so
    Pc = 50 and that step has 18 rows: it does not fit behind the packed sub-panel.  cell_size=(4, 6) -- 24-row ancestors,
    Pc = 48, a 16-row step -- is the shape where it shares the buffer.
  * cell_size=31 gives 6 x 6 = 36 knots per cell on a grid, more than the 32 rows the kernel takes: the level runs on
    another kernel and defers nothing.  31 is prime, and 1 x 31 cells leave leaf blocks of more than 32 rows at these
    sides, so the 16 + 15 split comes from cell_size=(4, 8): 32 knots, of which the cells of the last reference level keep
    30 to 32.  st_level_info reports the widest (32: 16 + 16); that a leaf block hangs below a 31-row ancestor is asserted
    from the tree the handle was given.
"""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_leaf_deferral import CASES, LEAF, QUAD_MIN, blocks, enqueue, model, problem, same_blocks
from tests.util import make_problem

pytestmark = pytest.mark.gpu

# the rows of test_gpu_leaf_deferral (NKX 32, 32 with two units per workgroup, 44, 50), the NKX 38 strip of test_gpu_routes
# (24-row ancestors, leaf chains of 144 rows) and one unit per workgroup
SEQ_CASES = CASES + [
    dict(id="strip_nkx38", strip=(640, 4, 1), kw=dict(cell_size=31, tree_depth=6, missing=0.15), env=QUAD_MIN, leaf=LEAF.format(38, 10)),
    dict(id="grid_na10_one_unit", side=40, kw=dict(missing=0.1), env=dict(QUAD_MIN, SPAMTREE_QUAD_UNITS="1"), leaf=LEAF.format(32, 8)),
]


def leaf_routes(m):
    return [a for g in m.route_info()["levels"] for a in g["A"] if a.endswith("false, true>")]


def walk(m, row, th):
    """The sequence on one handle; returns what it read, in order."""
    out = []
    assert m.get_loglik_comps_w(0)
    m.deal_with_w(None, seed=5, it=1)                               # (st_predict draws from the normals of a preceding sweep)
    out.append(("ll1", enqueue(m, 1, th[0])))                        # V only (deferral on)
    assert row["leaf"] in leaf_routes(m), leaf_routes(m)
    out.append(("comps1", m.comps(1)))
    m.accept_make_change()                                          # the completion
    m.predict(True)                                                 # full + phase P
    pr = m.route_info()["predict"]
    assert pr.startswith("k_factor_quad<4, ") and pr.endswith("false, true>"), pr
    out.append(("w_pred", m.get_w().copy()))
    ll = C.c_double()
    assert m.lib.st_sample_w_loglik(m.h, None, C.c_uint64(17), C.c_uint32(3), 0, C.byref(ll)) == 0
    out.append(("ll_sweep", ll.value))
    out.append(("w_sweep", m.get_w().copy()))
    out.append(("ll2", enqueue(m, 1, th[1])))                        # V only again, left pending ...
    m.theta[1] = th[2]
    assert m.get_loglik_comps_w(1)                                  # ... and replaced by a full factorisation
    out.append(("ll3", m.loglik_w[1]))
    out.append(("comps3", m.comps(1)))
    out.append(("b0", blocks(m, 0)))
    out.append(("b1", blocks(m, 1)))
    return out


def same(a, b):
    assert [k for k, _ in a] == [k for k, _ in b]
    for (k, x), (_, y) in zip(a, b):
        if k in ("b0", "b1"):
            same_blocks(x, y)
        elif k.startswith("comps"):
            assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]), k
        elif k.startswith("w_"):
            assert np.array_equal(x, y), k
        else:
            assert x == y, (k, x, y)


@pytest.mark.parametrize("row", SEQ_CASES, ids=[r["id"] for r in SEQ_CASES])
def test_mode_sequence_is_bitwise_the_undeferred_handle(row, monkeypatch):
    for k, v in row["env"].items():
        monkeypatch.setenv(k, v)
    pb = problem(row)
    th = [pb["theta"] * f for f in (1.07, 0.95, 0.93)]
    got = []
    for defer in (True, False):
        m = model(pb, defer)
        got.append(walk(m, row, th))
        m.close()
    same(got[0], got[1])


# id, make_problem keywords, then the shape the row stands for: pm (the last reference level's max_m), Pc (its max_P), whether
# the leaf level runs on k_factor_quad at all, and for the 16 + 15 split the ancestor width the tree must hold
STEP_CASES = [
    dict(id="cell9_one_subpanel", side=36, kw=dict(cell_size=9), pm=9, Pc=27),
    dict(id="cell16_full_subpanel", side=36, kw=dict(cell_size=16), pm=16, Pc=32),
    dict(id="cell25_packed_unshared", side=40, kw=dict(cell_size=25), pm=25, Pc=50),
    dict(id="cell4x6_packed_shared", side=40, kw=dict(cell_size=(4, 6)), pm=24, Pc=48),
    dict(id="cell31_not_a_quad_level", side=40, kw=dict(cell_size=31), pm=36, Pc=72, quad=False),
    dict(id="cell4x8_split_16_15", side=40, kw=dict(cell_size=(4, 8)), pm=32, Pc=64, parent_rows=31),
]


def step_shape(pm, Pc):
    """What the kernel does with a private ancestor of pm rows behind a shared chain of Pc rows (factor_quad.hpp)."""
    sub1 = pm >> 1 if pm > 16 else 0                 # rows of the second sub-panel (the first has the rest)
    last = (Pc - 1) % 32 + 1                         # rows of the step that holds the chain's last rows
    packed = 0 < sub1 <= 12
    return dict(sub0=pm - sub1, sub1=sub1, packed=packed, last=last, shared=packed and last <= 16)


def parent_rows_of_leaf_blocks(pb):
    """Rows of the last ancestor of every observed block of the last observed level, from the tree itself."""
    grp = np.asarray(pb["block_groups"])
    obs = [u for u, ix in enumerate(pb["indexing"]) if len(ix) and np.isfinite(pb["y"][ix]).any()]
    leaf = max(grp[u] for u in obs)
    return {len(pb["indexing"][pb["parents"][u][-1]]) for u in obs if grp[u] == leaf}


EXPECT = {
    "cell9_one_subpanel": dict(sub0=9, sub1=0, packed=False, last=27, shared=False),
    "cell16_full_subpanel": dict(sub0=16, sub1=0, packed=False, last=32, shared=False),
    "cell25_packed_unshared": dict(sub0=13, sub1=12, packed=True, last=18, shared=False),
    "cell4x6_packed_shared": dict(sub0=12, sub1=12, packed=True, last=16, shared=True),
    "cell4x8_split_16_15": dict(sub0=16, sub1=16, packed=False, last=32, shared=False),
}


def test_step_rows_cover_both_lengths_of_the_last_step():
    last = [e["last"] for e in EXPECT.values()]
    assert any(x <= 16 for x in last) and any(x > 16 for x in last)
    assert [e for e in EXPECT.values() if e["shared"]] and [e for e in EXPECT.values() if e["packed"] and not e["shared"]]


@pytest.mark.parametrize("row", STEP_CASES, ids=[r["id"] for r in STEP_CASES])
def test_step_shapes_deferral_on_against_off(row, monkeypatch):
    for k, v in QUAD_MIN.items():
        monkeypatch.setenv(k, v)
    pb = make_problem(side=row["side"], q=1, seed=3, missing=0.1, **row["kw"])
    th_b = pb["theta"] * 1.07
    got = {}
    for defer in (True, False):
        m = model(pb, defer)
        info = m.level_info()
        ref, leaf = info[-2], info[-1]
        assert (ref["max_m"], ref["max_P"]) == (row["pm"], row["Pc"]), info
        assert leaf["max_P"] == row["Pc"] + row["pm"], info
        assert (leaf["kernel"] == "k_factor_quad") == row.get("quad", True), info
        if row.get("quad", True):
            assert step_shape(row["pm"], row["Pc"]) == EXPECT[row["id"]]
        if "parent_rows" in row:      # a leaf block below an ancestor of that many rows: sub-panels of 16 and 15 rows
            rows = parent_rows_of_leaf_blocks(pb)
            assert row["parent_rows"] in rows and max(rows) == row["pm"], rows
            assert step_shape(row["parent_rows"], row["Pc"])["sub0"] == 16 and step_shape(row["parent_rows"], row["Pc"])["sub1"] == 15
        assert m.get_loglik_comps_w(0)
        ll = enqueue(m, 1, th_b)
        if defer and row.get("quad", True):
            assert leaf_routes(m), m.route_info()
        comps = m.comps(1)
        m.accept_make_change()
        got[defer] = (ll, comps, blocks(m, 0))
        m.close()
    a, b = got[True], got[False]
    assert a[0] == b[0]
    assert np.array_equal(a[1][0], b[1][0]) and np.array_equal(a[1][1], b[1][1])
    same_blocks(a[2], b[2])
