"""Hand-built trees (tests/tree_mutations.py) on the CPU: the references hold on them, the layout accepts them, and the
refusals they can run into are the documented ones.

  * the oracle's loglik_w equals the dense DAG density (tests/test_oracle_identities.dense_precision: no per-block code, any
    parents lists) to 1e-12 relative, and the oracle runs the whole protocol of tests/test_gpu_routes.oracle_protocol: the
    oracle was never pinned on such trees, and tests/test_gpu_handbuilt_trees.py takes it as the reference;
  * tests/layout_check.cpp (the program of tests/test_tree_layout_cpu.py) accepts every shape at world 1 under the route
    switches of the GPU rows, and its report shows what each row is there for;
  * at (world, rank) = (2, 0), (2, 1), (3, 1) a shape passes the invariants or is refused: a tree in which a block below the
    cut level has no ancestor on it (a block that skips that level) cannot be split into subtrees;
  * refusals of st_create's first stage that tests/test_create_errors_cpu.py has no case for.

Like tests/test_create_errors_cpu.py, the first-stage refusals go through st_shard_plan_opt of the built library
(libspamtree_hip.so: build() first); everything else here needs hipcc for tests/layout_check.cpp only.
"""
import math

import numpy as np
import pytest

from tests import tree_mutations as tm
from tests.test_create_errors_cpu import TOPOLOGY, UNSUPPORTED, plan
from tests.test_gpu_routes import _ORACLE, inputs, oracle_protocol
from tests.test_oracle_identities import dense_precision
from tests.test_tree_layout_cpu import layout_check, run_check, write_problem      # noqa: F401  (layout_check: the fixture)
from tests.util import make_problem, oracle_model, problem_arrays

QUAD_MIN = {"SPAMTREE_QUAD_MIN": "1"}
# the quad rows of the GPU file: k_factor_quad on small levels, up to four units per workgroup (at this size the default is one)
QUAD4 = dict(QUAD_MIN, SPAMTREE_QUAD_UNITS="4")
QUAD1 = dict(QUAD_MIN, SPAMTREE_QUAD_UNITS="1")
SKIP_TEXT = "block below the cut level without an ancestor on it"
# shape -> the switch rows its layout is checked under (the environments of the GPU rows that change the layout)
COLUMN_GROUP = ("mixed_chain_leaf", "mixed_chain_ref", "uneven_widths", "one_row_and_wide", "empty_and_childless", "empty_all_observed",
                "many_children_5", "many_children_4", "na_blocks_rehung")
LAYOUT_ROWS = [(s, "default", {}) for s in tm.SHAPES] + [(s, "quad_min_units4", QUAD4) for s in COLUMN_GROUP] + \
              [(s, "quad_min_units1", QUAD1) for s in ("mixed_chain_leaf", "mixed_chain_ref")] + \
              [("wide_mixed", "wide2", {"SPAMTREE_WIDE": "2"}),
               ("wide_mixed", "no_lchain", {"SPAMTREE_LCHAIN": "0", "SPAMTREE_LCHAIN_REF": "0"}),
               ("wide_mixed", "no_lchain_wide2", {"SPAMTREE_LCHAIN": "0", "SPAMTREE_LCHAIN_REF": "0", "SPAMTREE_WIDE": "2"})]
# what a row's report must show, by shape; (by row name) below
BY_SHAPE = {
    "mixed_chain_leaf": lambda r: r["gram_direct_level"] == -1 and r["fast_levels"] == r["levels"],
    "mixed_chain_ref": lambda r: r["fast_levels"] == r["levels"],
    "uneven_widths": lambda r: r["fast_levels"] == r["levels"] and r["gram_direct_level"] == r["last_ref_level"],
    "one_row_and_wide": lambda r: r["lchain_levels"] >= 2 and r["slabs"] > 0 and r["rfvoff"] == 16,
    "empty_and_childless": lambda r: r["pred_groups"] > 0 and r["fast_levels"] == r["levels"],
    "empty_all_observed": lambda r: r["pred_groups"] == 1 and r["fast_levels"] == r["levels"],     # the emptied block: a group of no rows
    "many_children_5": lambda r: r["gram_direct_level"] == -1 and r["fast_levels"] == r["levels"],
    "many_children_4": lambda r: r["last_ref_level"] >= 0 and r["gram_direct_level"] == r["last_ref_level"],
    "na_blocks_rehung": lambda r: r["pred_groups"] > 0 and r["pred_quads"] > 0,
    "wide_mixed": lambda r: r["fast_levels"] == 0,
    "two_outcomes_mixed": lambda r: r["fast_levels"] == 0 and r["lchain_levels"] >= 1,
    "limited_skip": lambda r: r["twins"] > 0,
}
BY_ROW = {
    # quads of several units: at most half as many quads as column groups (all of them, the prediction ones included)
    "quad_min_units4": lambda r: r["quad_levels"] > 0 and 0 < 2 * r["quads"] <= r["groups"],
    # one unit per workgroup: a quad per group of every level below the root (the root's group has no chain: no quad)
    "quad_min_units1": lambda r: r["quad_levels"] > 0 and r["quads"] == r["groups"] - 1,
    "wide2": lambda r: r["wide_groups"] > 0 and r["lchain_levels"] >= 2,      # the root (no chain: never an lchain level) in a wide group
    "no_lchain": lambda r: r["wide_groups"] == 0 and r["lchain_levels"] == 0,
    "no_lchain_wide2": lambda r: r["wide_groups"] > 0 and r["lchain_levels"] == 0,
}


def dense_loglik(pb, theta, w):
    """log N(w_obs; 0, Q^-1) over the rows of the observed blocks, Q from dense_precision: prediction blocks are not part of
    the density the sampler targets, so they enter it without rows."""
    obs = [np.isfinite(pb["y"][ix]).any() for ix in pb["indexing"]]
    sub = dict(pb, indexing=[ix if o else ix[:0] for ix, o in zip(pb["indexing"], obs)])
    Q, logdet = dense_precision(sub, theta)
    rows = sum(ix.size for ix in sub["indexing"])
    return -0.5 * rows * math.log(2 * math.pi) + 0.5 * logdet - 0.5 * w @ Q @ w


@pytest.mark.parametrize("name", list(tm.SHAPES))
def test_oracle_holds_on_the_shape(name):
    pb = tm.shape(name)
    inp = inputs(pb)
    om = oracle_model(pb, w=inp["w"], beta=inp["beta"], tausq=inp["tausq"])
    assert om.get_loglik_comps_w(om.param_data)
    exact = dense_loglik(pb, pb["theta"], inp["w"])
    assert abs(om.param_data.loglik_w - exact) <= 1e-12 * abs(exact), (om.param_data.loglik_w, exact)
    ref = oracle_protocol(pb, inp)
    assert len(ref["steps"]) == (7 if np.any(~np.isfinite(pb["y"])) else 5)
    for st in ref["steps"]:
        assert np.all(np.isfinite(st["w"]))
    _ORACLE.setdefault("handbuilt:" + name, ref)


@pytest.fixture(scope="module")
def shape_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("handbuilt_problems")
    out = {}
    for name in tm.SHAPES:
        pb = tm.shape(name)
        path = str(d / (name + ".bin"))
        write_problem(path, problem_arrays(pb))
        out[name] = (path, pb)
    return out


def report_of(out):
    return {k: int(v) for k, v in (kv.split("=") for kv in out.split()[1:])}


@pytest.mark.parametrize("name,row,env", LAYOUT_ROWS, ids=[f"{s}-{r}" for s, r, _ in LAYOUT_ROWS])
def test_layout_accepts_the_shape(layout_check, shape_files, name, row, env):      # noqa: F811
    path, pb = shape_files[name]
    rc, out = run_check(layout_check, path, dict(env=env), pb["limited_tree"], 1, 0)
    assert rc == 0 and out.startswith("OK "), out
    rep = report_of(out)
    assert BY_SHAPE[name](rep), out
    assert BY_ROW.get(row, lambda r: True)(rep), out


# The shapes in which a block skips a level, and the world sizes whose cut level that is (the cut is a level with enough blocks
# to hand every rank two subtrees: level 2 of the four-level trees at world 2, level 3 at world 3; level 2 of the three-level
# q = 2 and q = 3 trees at world 2, none at world 3): a block below the cut has no ancestor on it
MUST_REFUSE = {("mixed_chain_leaf", 3), ("mixed_chain_ref", 2), ("limited_skip", 3), ("na_blocks_rehung", 2), ("na_blocks_rehung", 3),
               ("wide_mixed", 2), ("two_outcomes_mixed", 2)}
# cut at level 2 of 4: the leaves that hang from the cut level itself sort in front of their cousins (device order keeps
# siblings together: by last parent), so a rank's leaves are two runs of the leaf level, not one -- refused by name
NOT_CONTIGUOUS = {("mixed_chain_leaf", 2), ("limited_skip", 2)}


@pytest.mark.parametrize("world,rank", [(2, 0), (2, 1), (3, 1)])
@pytest.mark.parametrize("name", list(tm.SHAPES))
def test_sharded_layout_passes_or_refuses(layout_check, shape_files, name, world, rank):      # noqa: F811
    path, pb = shape_files[name]
    rc, out = run_check(layout_check, path, dict(env={}), pb["limited_tree"], world, rank)
    if (name, world) in MUST_REFUSE:
        assert rc == 2 and out == f"REFUSED {TOPOLOGY} {SKIP_TEXT}", out
    elif (name, world) in NOT_CONTIGUOUS:
        assert rc == 2 and out == f"REFUSED {TOPOLOGY} a rank's blocks are not contiguous in a level", out
    else:
        assert rc == 0 and out.startswith("OK "), out       # (a violated invariant: exit status 1; a crash: a signal)
        rep = report_of(out)
        # really sharded, except the three-level trees at world 3 (no level of theirs has six blocks above the leaves)
        assert (rep["cut"] < rep["levels"]) == (name not in ("wide_mixed", "two_outcomes_mixed")), out


# ---- refusals without a case in tests/test_create_errors_cpu.py
def test_an_inconsistent_rehang_is_refused():
    """A leaf that drops its direct parent is fine (tree_mutations.rehang); one that drops a middle ancestor and keeps the
    last one breaks parents(u) = parents(last parent) + [last parent]."""
    pb = tm.shape("mixed_chain_leaf")
    u = [v for v in tm.blocks_of_level(pb, 3) if len(pb["parents"][v]) == 3][0]
    pb["parents"][u] = pb["parents"][u][[0, 2]]
    rc, msg, _, _ = plan(problem_arrays(pb))
    assert rc == UNSUPPORTED and "parents(u) is not parents(last parent)+[last parent]" in msg and "make_edges_limited" in msg, msg


def test_a_rehang_below_an_unobserved_parent_is_refused():
    pb = tm.shape("mixed_chain_leaf")
    u = [v for v in tm.blocks_of_level(pb, 3) if len(pb["parents"][v]) == 2][0]
    gp = tm.last_parent(pb, u)
    pb["y"] = pb["y"].copy()
    pb["y"][pb["indexing"][gp]] = np.nan
    rc, msg, _, _ = plan(problem_arrays(pb))
    assert rc == TOPOLOGY and "ancestor block without observations" in msg, msg


def test_65_direct_child_groups_are_refused(layout_check, tmp_path):      # noqa: F811
    """A reference block is a column group of its own, so 65 groups under one block fit in n = 900 rows: the 30 x 30 grid in
    9-row blocks has reference levels of 1 / 4 / 16 / 64 blocks; with 60 (61) blocks of the fourth level re-hung from the
    root, the root has 4 + 60 = 64 direct child groups (accepted, and the layout's invariants hold) or 65 (refused)."""
    for n_hung, ok in ((60, True), (61, False)):
        pb = make_problem(side=30, q=1, seed=11, cell_size=9)
        root, l4 = tm.blocks_of_level(pb, 0), tm.blocks_of_level(pb, 3)
        assert len(root) == 1 and len(l4) == 64 and tm.is_reference_level(pb, l4[0]) and tm.leaf_level(pb) == 4
        for u in l4[:n_hung]:
            tm.rehang(pb, u, drop=2)
        assert len(tm.direct_children(pb, root[0], observed_only=True)) == 4 + n_hung
        path = str(tmp_path / f"hung{n_hung}.bin")
        write_problem(path, problem_arrays(pb))
        rc, out = run_check(layout_check, path, dict(env={}), False, 1, 0)
        if ok:
            assert rc == 0 and out.startswith("OK "), out
        else:
            assert rc == 2 and out == f"REFUSED {UNSUPPORTED} more than 64 direct child groups under one block", out
