"""The refusals of the first stage of st_create (argument checks, census, device order, ancestors, record layout), reached
through st_shard_plan_opt, which runs that stage alone and needs no GPU.  Each case corrupts one thing in a valid problem
and asserts the code and a distinctive part of the message, so the text and the ORDER of the checks are pinned: a corrupted
input that two checks would refuse must keep reporting the first one.

The problem is make_problem(side=8, q=1, seed=1): two levels, five blocks, one parent each.  The messages that need a
block with two parents (parents not ascending, the chain property, limited_tree's single-parent rule) take the same grid
with cell_size=4: three levels, 21 blocks, leaf parents [root, level-1 block].

Left out, because no small corruption of a value array reaches them:
  "more than ST_MAX_ANCESTORS ancestors"                  a chain of more than 16 levels (a *_ptr array would have to change)
  "message record too large"                               a record of more than 2^31 doubles: ancestors of ~46000 rows
  "block below the cut level without an ancestor on it"    every block below a cut level has parents, or an earlier check fires
  "st_create: null argument" for `out`                     st_shard_plan_opt passes its own
and everything after the first stage (st_create only: it queries the device first)."""
import ctypes as C

import numpy as np
import pytest

from spamtree_amd import _lib
from tests.util import make_problem, problem_arrays, st_problem_struct

USAGE, TOPOLOGY, UNSUPPORTED = -1, -3, -4
LIMITED = 2      # st_options.reserved bit 1


@pytest.fixture(scope="module")
def problems():
    return {"flat": make_problem(side=8, q=1, seed=1), "flat_limited": make_problem(side=8, q=1, seed=1, limited_tree=True),
            "deep": make_problem(side=8, q=1, seed=1, cell_size=4),
            "deep_limited": make_problem(side=8, q=1, seed=1, cell_size=4, limited_tree=True)}


def plan(a, world=2, reserved=0, null_problem=False):
    lib = _lib.load()
    st = st_problem_struct(a)
    owner = np.full(int(a["block_names"].size), -7, dtype=np.int64)
    cut = C.c_int32(-7)
    opt = _lib.StOptions(0, 1, 0, 1, 0, reserved)
    rc = lib.st_shard_plan_opt(None if null_problem else C.byref(st), C.byref(opt), world, owner.ctypes.data_as(_lib.c_ip),
                               C.byref(cut))
    return rc, lib.st_last_error(None).decode(), owner, cut.value


def rows_of(a, u):
    return a["indexing_idx"][a["indexing_ptr"][u]:a["indexing_ptr"][u + 1]]


def extra_row(a):
    """One more row that no block lists."""
    n = a["n_all"]
    a["n_all"] = n + 1
    a["y"] = np.append(a["y"], 0.5)
    a["mv_id"] = np.append(a["mv_id"], 1)
    a["X"] = np.asfortranarray(np.vstack([a["X"], np.ones((1, a["p"]))]))
    a["coords"] = np.asfortranarray(np.vstack([a["coords"], [[0.5, 0.5]]]))


def swap(v, i, j):
    v[i], v[j] = v[j], v[i]


# name, problem, options bits, corruption, world, code, part of the message
CASES = [
    ("d", "flat", 0, lambda a: a.update(d=3), 2, UNSUPPORTED, "only d=2 is reachable from spamtree()"),
    ("q_low", "flat", 0, lambda a: a.update(q=0), 2, UNSUPPORTED, "q out of range"),
    ("q_high", "flat", 0, lambda a: a.update(q=7), 2, UNSUPPORTED, "q out of range"),
    ("p_low", "flat", 0, lambda a: a.update(p=0), 2, UNSUPPORTED, "p must be in 1..64 (ST_MAX_P)"),
    ("p_high", "flat", 0, lambda a: a.update(p=65), 2, UNSUPPORTED, "p must be in 1..64 (ST_MAX_P)"),
    ("world_zero", "flat", 0, lambda a: None, 0, USAGE, "bad rank/world"),
    ("world_65", "flat", 0, lambda a: None, 65, USAGE, "bad rank/world"),
    ("coords_null", "flat", 0, lambda a: a.update(coords=None), 2, USAGE, "st_create: coords is NULL"),
    ("coords_nan", "flat", 0, lambda a: a["coords"].__setitem__((3, 0), np.nan), 2, USAGE, "coordinates must be finite (row 3)"),
    ("coords_inf", "flat", 0, lambda a: a["coords"].__setitem__((5, 1), np.inf), 2, USAGE, "coordinates must be finite (row 5)"),
    ("extra_level", "flat", 0, lambda a: a["block_groups"].__setitem__(4, 99), 2, TOPOLOGY,
     "more levels in block_groups than entries in res_is_ref"),
    ("row_twice", "flat", 0, lambda a: a["indexing_idx"].__setitem__(0, a["indexing_idx"][1]), 2, TOPOLOGY,
     "indexing is not a partition of the rows"),
    ("row_out_of_range", "flat", 0, lambda a: a["indexing_idx"].__setitem__(0, a["n_all"]), 2, TOPOLOGY,
     "indexing is not a partition of the rows"),
    ("row_negative", "flat", 0, lambda a: a["indexing_idx"].__setitem__(0, -1), 2, TOPOLOGY, "indexing is not a partition of the rows"),
    ("row_without_block", "flat", 0, extra_row, 2, TOPOLOGY, "row without a block"),
    # the root level loses its only observed block: level 0 is empty, level 1 observed
    ("empty_level", "flat", 0, lambda a: a["y"].__setitem__(rows_of(a, 0), np.nan), 2, TOPOLOGY, "an empty level precedes an observed one"),
    ("indexing_order", "flat", 0, lambda a: swap(a["indexing_idx"], a["indexing_ptr"][1], a["indexing_ptr"][1] + 1), 2, TOPOLOGY,
     "indexing(u) must be ascending"),
    ("parent_range", "flat", 0, lambda a: a["parents_idx"].__setitem__(0, a["block_names"].size), 2, TOPOLOGY, "parent id out of range"),
    ("parent_negative", "flat", 0, lambda a: a["parents_idx"].__setitem__(0, -1), 2, TOPOLOGY, "parent id out of range"),
    ("parents_order", "deep", 0, lambda a: swap(a["parents_idx"], a["parents_ptr"][7], a["parents_ptr"][7] + 1), 2, TOPOLOGY,
     "parents(u) must be ascending"),
    ("parent_same_level", "flat", 0, lambda a: a["parents_idx"].__setitem__(a["parents_ptr"][2], 1), 2, TOPOLOGY,
     "parent on the same or a deeper level"),
    ("parent_itself", "flat", 0, lambda a: a["parents_idx"].__setitem__(a["parents_ptr"][2], 2), 2, TOPOLOGY,
     "parent on the same or a deeper level"),
    ("parent_not_reference", "flat", 0, lambda a: a["res_is_ref"].__setitem__(0, 0), 2, TOPOLOGY, "parent on a non-reference level"),
    # block 1 (level 1, a parent of leaf blocks) loses its observations; its level keeps three observed blocks
    ("ancestor_unobserved", "deep", 0, lambda a: a["y"].__setitem__(rows_of(a, 1), np.nan), 2, TOPOLOGY,
     "ancestor block without observations"),
    ("limited_two_parents", "deep", LIMITED, lambda a: None, 2, TOPOLOGY, "limited_tree: a block has more than one parent"),
    ("chain_single_parents", "deep_limited", 0, lambda a: None, 2, UNSUPPORTED, "parents(u) is not parents(last parent)+[last parent]"),
    # block 7: parents [0, 2] -> [1, 2]: ascending, shallower, reference, observed -- but parents(2) is [0]
    ("chain_other_ancestor", "deep", 0, lambda a: a["parents_idx"].__setitem__(a["parents_ptr"][7], 1), 2, UNSUPPORTED,
     "parents(u) is not parents(last parent)+[last parent]"),
]


@pytest.mark.parametrize("name,which,reserved,corrupt,world,code,text", CASES, ids=[c[0] for c in CASES])
def test_first_stage_refusal(problems, name, which, reserved, corrupt, world, code, text):
    a = problem_arrays(problems[which])
    corrupt(a)
    rc, msg, owner, cut = plan(a, world=world, reserved=reserved)
    assert rc == code, (rc, msg)
    assert text in msg, msg
    assert np.all(owner == -7) and cut == -7      # a refused plan writes nothing


def test_null_problem():
    a = problem_arrays(make_problem(side=8, q=1, seed=1))
    rc, msg, _, _ = plan(a, null_problem=True)
    assert rc == USAGE and msg == "st_create: null argument"


@pytest.mark.parametrize("which,reserved", [("flat", 0), ("flat_limited", LIMITED), ("deep", 0), ("deep_limited", LIMITED)])
def test_uncorrupted_problems_plan(problems, which, reserved):
    """The cases above fail for their corruption alone: the problems they start from are accepted."""
    a = problem_arrays(problems[which])
    for world in (1, 2):
        rc, msg, owner, cut = plan(a, world=world, reserved=reserved)
        assert rc == 0, msg
        assert np.all(owner >= -1) and np.all(owner < world) and 0 <= cut <= a["res_is_ref"].size
