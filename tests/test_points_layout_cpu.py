"""The launch structures st_points_set / st_points_set_joint build (spamtree_amd/csrc/points_layout.cpp), checked on the CPU:
tests/points_layout_check.cpp is compiled against tree_layout.cpp and points_layout.cpp alone (host code only), reads a problem and a
point set from flat binary files, builds the layout with the MI355X's 256 CUs and the row's LDS limit and checks what the
k_points_* and k_points_joint_* kernels assume of chains, order, tiles, joint groups and their packing into 16-column slots.
It prints the first violated invariant.

The problems are those of tests/test_gpu_predict_points.py and tests/test_gpu_predict_joint.py; the anchors are chosen here from
the topology (any block with observed rows is a valid anchor for the layout).  The counts the program reports prove that a row
reached what it is here for (a check over an empty list proves nothing); one negative case proves that the checks can fail; the
refusals are the parent's, code and text; and the same program built with the address and undefined-behaviour sanitizers runs
clean over the good and the refused inputs."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.test_gpu_predict_joint import SIZES, small
from tests.test_gpu_predict_points import _deep4, _deep5
from tests.test_tree_layout_cpu import write_problem
from tests.util import make_problem, problem_arrays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spamtree_amd", "csrc")
ST_ERR_USAGE, ST_ERR_UNSUPPORTED = -1, -4
LDS_160K, LDS_64K = 160 * 1024, 64 * 1024      # PP_LDS_BYTES(256) = 76 800 B fits the first only


def build_check(tmp, name, extra, layout_source=None):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    exe = str(tmp / name)
    subprocess.run([hipcc, "--offload-host-only", "-std=c++17", "-O1"] + extra + ["-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "points_layout_check.cpp"), os.path.join(CSRC, "tree_layout.cpp"),
                    layout_source or os.path.join(CSRC, "points_layout.cpp"), "-o", exe], check=True, timeout=600)
    return exe


def write_points(path, n_new, coords, mv, anchor, joint):
    """n_new, joint flag, then coords (column-major), mv, anchor, joint labels; None: a null pointer."""
    with open(path, "wb") as f:
        np.array([n_new, joint is not None], dtype=np.int64).tofile(f)
        for v, ty in ((coords, np.float64), (mv, np.int64), (anchor, np.int64), (joint, np.int64)):
            v = np.zeros(0, dtype=ty) if v is None else np.ascontiguousarray(np.asarray(v, dtype=ty).ravel(order="F"))
            np.array([v.size], dtype=np.int64).tofile(f)
            v.tofile(f)


# ---- the point sets -------------------------------------------------------------------------------------------------------
def observed_blocks(pb):
    """0-based ids of the blocks with observed rows, and which of them are reference blocks."""
    from spamtree_amd.predict import conditioning_set
    obs = np.nonzero(np.bincount(pb["blocking"] - 1, weights=np.isfinite(pb["y"]).astype(float), minlength=pb["block_names"].size) > 0)[0]
    isref = np.array([int(b) in conditioning_set(pb["topo"], int(b)) for b in obs])
    return obs, isref


def random_coords(pb, n, rng):
    lo, hi = pb["coords"].min(axis=0), pb["coords"].max(axis=0)
    return lo + (hi - lo) * rng.uniform(size=(n, 2))


def run_set(pb, seed):
    """As run_set of tests/test_gpu_predict_joint.py: points in random order, cut into joint groups of SIZES over the points of
    one anchor; 150 points on the first anchor (more than one tile of 64, more than one joint tile), 24 on eleven others."""
    rng = np.random.default_rng(seed)
    obs, isref = observed_blocks(pb)
    pick = np.concatenate([rng.choice(obs[isref], 4, replace=False), rng.choice(obs[~isref], 8, replace=False)])
    anchor = rng.permutation(np.concatenate([np.full(150, pick[0])] + [np.full(24, b) for b in pick[1:]]))
    n = anchor.size
    labels = np.zeros(n, dtype=np.int64)
    lab = 0
    for r, b in enumerate(np.unique(anchor)):
        idx = np.nonzero(anchor == b)[0]
        k, at = r, 0
        while at < idx.size:
            g = SIZES[k % len(SIZES)]
            labels[idx[at:at + g]] = lab
            lab, k, at = lab + 1, k + 1, at + g
    assert {1, 2, 5, 6, 16} <= set(np.bincount(labels).tolist())
    return random_coords(pb, n, rng), np.ones(n, dtype=np.int64), anchor, labels


def site_set(pb, seed, n_sites=None):
    """The q outcomes at one site per joint group; the sites' anchors are random observed blocks (n_sites None: every one)."""
    rng = np.random.default_rng(seed)
    obs, _ = observed_blocks(pb)
    blocks = obs if n_sites is None else rng.choice(obs, n_sites, replace=True)
    q = pb["q"]
    coords = np.repeat(random_coords(pb, blocks.size, rng), q, axis=0)
    return coords, np.tile(np.arange(1, q + 1), blocks.size), np.repeat(blocks, q), np.repeat(np.arange(blocks.size), q) + 1000


def both_kinds_set(pb, seed):
    """Groups of four: two points anchored at a non-reference block, two at the reference block its chain ends in."""
    from spamtree_amd.predict import conditioning_set
    rng = np.random.default_rng(seed)
    obs, isref = observed_blocks(pb)
    leaves = rng.choice(obs[~isref], 10, replace=False)
    anchor = np.concatenate([[b, conditioning_set(pb["topo"], int(b))[-1], b, conditioning_set(pb["topo"], int(b))[-1]] for b in leaves])
    return random_coords(pb, anchor.size, rng), np.ones(anchor.size, dtype=np.int64), anchor, np.repeat(np.arange(10), 4)


def empty_set(pb, seed):
    return np.zeros((0, 2)), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)


# row -> (problem, point set, joint, LDS limit, flags, what its report must show)
CASES = {
    "small1_groups_plain": (lambda: small(1), run_set, False, LDS_160K, [],
                            lambda r: r["ntile128"] > r["chains"] and r["multi_tile_chains"] > 0 and r["ref_anchors"] > 0 and r["nonref_anchors"] > 0
                            and r["gen"] == 0 and r["groups"] == 0),
    "small1_groups_joint": (lambda: small(1), run_set, True, LDS_160K, [],
                            lambda r: r["max_g"] == 16 and r["padded_slots"] > 0 and r["full_slots"] > 0 and r["tiles4"] > 0
                            and r["jtile128"] > r["chains"] and r["jgen"] == 0),
    "small3_sites": (lambda: small(3), lambda pb, s: site_set(pb, s, 100), True, LDS_160K, [],
                     lambda r: r["groups"] == 100 and r["max_g"] == 3 and r["jtile128"] + r["jtile256"] > 0 and r["padded_slots"] > 0),
    "small6_sites": (lambda: small(6), lambda pb, s: site_set(pb, s, 60), True, LDS_160K, [],
                     lambda r: r["groups"] == 60 and r["max_g"] == 6 and r["jtile128"] > 0 and r["padded_slots"] > 0),
    "deep5_lds160k": (_deep5, site_set, True, LDS_160K, [],
                      lambda r: 128 < r["max_chain_rows"] <= 256 and r["ntile256"] > 0 and r["jtile256"] > 0 and r["gen"] == 0 and r["jgen"] == 0),
    "deep5_lds64k": (_deep5, site_set, True, LDS_64K, [],
                     lambda r: 128 < r["max_chain_rows"] <= 256 and r["ntile256"] == 0 and r["jtile256"] == 0 and r["gen"] > 0 and r["jgen"] > 0
                     and r["ntile128"] > 0),
    "deep4": (_deep4, site_set, True, LDS_160K, [],
              lambda r: r["max_chain_rows"] > 256 and r["gen"] > 0 and r["jgen"] > 0 and r["grid_generic"] > 0),
    "small3_force_generic": (lambda: small(3), lambda pb, s: site_set(pb, s, 100), True, LDS_160K, ["force-generic"],
                             lambda r: r["gen"] == r["n"] == 300 and r["jgen"] == r["groups"] == 100 and r["ntile128"] + r["jtile128"] == 0),
    "small1_both_kinds": (lambda: small(1), both_kinds_set, True, LDS_160K, [],
                          lambda r: r["mixed_chains"] > 0 and r["ref_anchors"] == r["nonref_anchors"] == 20 and r["max_g"] == 4),
    "empty_plain": (lambda: small(1), empty_set, False, LDS_160K, [], lambda r: r["n"] == 0 and r["chains"] == 0),
    "empty_joint": (lambda: small(1), empty_set, True, LDS_160K, [], lambda r: r["n"] == 0 and r["groups"] == 0 and r["cov_total"] == 0),
}


_FILES = {}


def problem_file(tmp, key, maker):
    """The problem written once per test session: (path, problem)."""
    if (tmp, key) not in _FILES:
        pb = maker()
        write_problem(os.path.join(tmp, key + ".bin"), problem_arrays(pb))
        _FILES[(tmp, key)] = (os.path.join(tmp, key + ".bin"), pb)
    return _FILES[(tmp, key)]


def case_files(tmp, rid):
    """(problem file, points file, LDS limit, flags) of a row of CASES."""
    maker, points, joint, lds, flags, _ = CASES[rid]
    key = {"small1": "small1", "small3": "small3", "small6": "small6", "deep5": "deep5", "deep4": "deep4", "empty": "small1"}[rid.split("_")[0]]
    path, pb = problem_file(tmp, key, maker)
    coords, mv, anchor, labels = points(pb, 7)
    ppath = os.path.join(tmp, rid + ".pts")
    write_points(ppath, anchor.size, coords, mv, anchor, labels if joint else None)
    return path, ppath, lds, flags


def run_check(exe, path, ppath, lds, flags):
    env = {k: v for k, v in os.environ.items() if not k.startswith("SPAMTREE_")}
    r = subprocess.run([exe, path, ppath, str(lds)] + list(flags), env=env, capture_output=True, text=True, timeout=120)
    return r.returncode, (r.stdout + r.stderr).strip()


def report(out):
    return {k: int(v) for k, v in (kv.split("=") for kv in out.split()[1:])}


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp("points_layout"))


@pytest.fixture(scope="module")
def layout_check(tmp_path_factory):
    return build_check(tmp_path_factory.mktemp("points_layout_check"), "points_layout_check", [])


@pytest.mark.parametrize("rid", list(CASES))
def test_layout_invariants(layout_check, tmp, rid):
    rc, out = run_check(layout_check, *case_files(tmp, rid))
    assert rc == 0 and out.startswith("OK "), out
    assert CASES[rid][5](report(out)), out


def test_a_column_moved_to_the_next_slot_is_named(layout_check, tmp):
    path, ppath, lds, flags = case_files(tmp, "small1_groups_joint")
    rc, out = run_check(layout_check, path, ppath, lds, flags + ["move-col"])
    assert rc == 1, out
    assert out.startswith("VIOLATED joint packing: tile ") and " slot " in out and " column " in out, out


# ---- the refusals of st_points_set / st_points_set_joint, in the order of their checks; texts from the parent's points_set_impl
def refusal_inputs(tmp):
    """name -> (problem file, points file, flags, code, text)."""
    path, pb = problem_file(tmp, "refuse", lambda: make_problem(side=20, q=1, seed=18, missing=0.1))
    lpath, _ = problem_file(tmp, "refuse_limited", lambda: make_problem(side=20, q=1, seed=18, missing=0.1, limited_tree=True))
    from spamtree_amd.predict import conditioning_set
    rng = np.random.default_rng(3)
    obs, isref = observed_blocks(pb)
    n = 30
    empty = np.setdiff1d(np.arange(pb["block_names"].size), obs)
    assert empty.size
    coords, mv = random_coords(pb, n, rng), np.ones(n, dtype=np.int64)
    anchor = rng.choice(obs, n)
    ends = np.array([conditioning_set(pb["topo"], int(b))[-1] for b in anchor])
    out = {}

    def add(name, code, text, flags=(), file=path, n_new=n, c=coords, m=mv, a=anchor, joint=None, set_m=None, set_a=None):
        m, a = (None if x is None else np.array(x, copy=True) for x in (m, a))
        for arr, edit in ((m, set_m), (a, set_a)):
            if edit is not None:
                arr[edit[0]] = edit[1]
        ppath = os.path.join(tmp, "refuse_" + name + ".pts")
        write_points(ppath, n_new, c, m, a, joint)
        out[name] = (file, ppath, list(flags), code, text)

    add("limited", ST_ERR_UNSUPPORTED, "st_points_set: limited_tree handles are not supported (new-point prediction is out of scope for them)",
        flags=["limited"], file=lpath, m=0 * mv)     # (the bad margins behind it are not looked at)
    add("world", ST_ERR_UNSUPPORTED, "st_points_set: multi-GPU handles (world > 1) are not supported (new-point prediction is out of scope for them)",
        flags=["world2"], m=0 * mv)
    sizes = "st_points_set: bad sizes or NULL inputs"
    add("negative_n", ST_ERR_USAGE, sizes, n_new=-1)
    add("n_beyond_int32", ST_ERR_USAGE, sizes, n_new=2 ** 31)
    add("null_coords", ST_ERR_USAGE, sizes, c=None)
    add("null_mv", ST_ERR_USAGE, sizes, m=None)
    add("null_anchor", ST_ERR_USAGE, sizes, a=None)
    add("anchor_negative", ST_ERR_USAGE, "st_points_set: anchor 3 is not a block id", set_a=(3, -1))
    add("anchor_past_the_blocks", ST_ERR_USAGE, "st_points_set: anchor 3 is not a block id", set_a=(3, pb["block_names"].size))
    add("anchor_without_rows", ST_ERR_USAGE, "st_points_set: anchor 3 is a prediction block (no observed rows)", set_a=(3, int(empty[0])))
    add("margin_zero", ST_ERR_USAGE, "st_points_set: margin of point 3 is not in 1..q", set_m=(3, 0))
    add("margin_past_q", ST_ERR_USAGE, "st_points_set: margin of point 3 is not in 1..q", set_m=(3, 2))
    bad_x, bad_y = coords.copy(), coords.copy()
    bad_x[5, 0], bad_y[5, 1] = np.nan, np.inf
    add("x_not_finite", ST_ERR_USAGE, "st_points_set: coordinates must be finite", c=bad_x)
    add("y_not_finite", ST_ERR_USAGE, "st_points_set: coordinates must be finite", c=bad_y)
    # the per-point checks in index order: point 3's margin before point 5's anchor; and all of them before the joint groups
    add("index_order", ST_ERR_USAGE, "st_points_set: margin of point 3 is not in 1..q", set_m=(3, 0), set_a=(5, -1))
    seventeen = np.concatenate([np.full(17, 41), np.arange(n - 17)])
    same = np.full(n, anchor[0])
    add("seventeen_members", ST_ERR_UNSUPPORTED, "st_points_set_joint: joint group 41 has more than 16 members (ST_POINTS_MAX_JOINT)", a=same, joint=seventeen)
    add("points_before_groups", ST_ERR_USAGE, "st_points_set: margin of point 29 is not in 1..q", a=same, joint=seventeen, set_m=(29, 0))
    other = int(np.nonzero(ends != ends[0])[0][0])
    labels = np.arange(n) + 100
    labels[other] = labels[0]
    add("two_chains_in_a_group", ST_ERR_USAGE, "st_points_set_joint: the members of joint group 100 do not end in the same conditioning chain (point %d and point 0)" % other,
        joint=labels)
    return out


REFUSALS = ["limited", "world", "negative_n", "n_beyond_int32", "null_coords", "null_mv", "null_anchor", "anchor_negative", "anchor_past_the_blocks",
            "anchor_without_rows", "margin_zero", "margin_past_q", "x_not_finite", "y_not_finite", "index_order", "seventeen_members",
            "points_before_groups", "two_chains_in_a_group"]


@pytest.fixture(scope="module")
def refusals(tmp):
    out = refusal_inputs(tmp)
    assert sorted(out) == sorted(REFUSALS)
    return out


@pytest.mark.parametrize("name", REFUSALS)
def test_refusals_keep_code_and_text(layout_check, refusals, name):
    path, ppath, flags, code, text = refusals[name]
    rc, out = run_check(layout_check, path, ppath, LDS_160K, flags)
    assert rc == 2 and out == "REFUSED %d %s" % (code, text), out


def test_the_check_runs_clean_under_the_sanitizers(tmp_path_factory, tmp, refusals):
    """The stand-alone program (builder and checker) with -fsanitize=address,undefined, on the CPU: nothing is preloaded."""
    exe = build_check(tmp_path_factory.mktemp("points_layout_check_san"), "points_layout_check_san",
                      ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"])
    for rid in CASES:
        rc, out = run_check(exe, *case_files(tmp, rid))
        assert rc == 0 and out.startswith("OK "), out
    for name, (path, ppath, flags, code, text) in refusals.items():
        rc, out = run_check(exe, path, ppath, LDS_160K, flags)
        assert rc == 2 and out == "REFUSED %d %s" % (code, text), (name, out)
