"""The launch structures st_create builds (spamtree_amd/csrc/tree_layout.cpp), checked on the CPU: tests/layout_check.cpp is
compiled against that file alone (host code only, no sanitiser), reads a problem from a flat binary file, builds its layout
with the MI355X's limits (256 CUs, 160 KB of LDS, the named fallback static sizes) and the row's switches in the
environment, and checks what the kernels assume of blocks, column groups, quads, wide groups, lchain slabs, group
descriptors, sharding and LDS sizes.  It prints the first violated invariant.

The problems are the rows of tests/test_gpu_routes.py that reach each builder at oracle size; every row runs as
(world, rank) = (1, 0), (2, 0), (2, 1), (3, 1).  The counts the program reports prove that the row did reach the builder it
is here for (a check over an empty list proves nothing), and one negative case proves that the checks can fail."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.test_gpu_routes import ROUTES, WIDE_ROUTES, build_problem
from tests.util import problem_arrays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spamtree_amd", "csrc")
ARRAYS = ("y", "X", "coords", "mv_id", "res_is_ref", "block_names", "block_groups", "indexing_ptr", "indexing_idx",
          "parents_ptr", "parents_idx", "children_ptr", "children_idx")
# row -> what its report must show
ROWS = {
    "grid_leaf32_pred32": lambda r: r["groups"] > 0 and r["quads"] > 0 and r["pred_groups"] > 0 and r["pred_quads"] > 0 and r["pred_nkx"] == 32,
    "seg6_gram_direct": lambda r: r["last_ref_level"] >= 0 and r["gram_direct_level"] == r["last_ref_level"],
    "wide4_default_pred": lambda r: r["slabs"] > 0 and r["rfvoff"] > 0 and r["lchain_levels"] >= 2,     # reference and leaf levels
    "wide4_sibling_groups": lambda r: r["wide_groups"] > 0 and r["lchain_levels"] == 0,
    "limited_wave": lambda r: r["twins"] > 0,
    # chains beyond the quads' 200 rows on the column-group path; the shorter levels have quads (too few to take the kernel)
    "cfg5_mfma_chains_pred": lambda r: r["max_group_chain"] > 200 and r["fast_levels"] == r["levels"] and r["quads"] > 0,
}
SHARDS = [(1, 0), (2, 0), (2, 1), (3, 1)]


def write_problem(path, a):
    with open(path, "wb") as f:
        np.array([a["n_all"], a["d"], a["q"], a["p"], a["res_is_ref"].size, a["block_names"].size], dtype=np.int64).tofile(f)
        for name in ARRAYS:
            v = a[name]
            v = np.zeros(0) if v is None else np.asarray(v).ravel(order="F")
            assert v.dtype in (np.float64, np.int64)
            np.array([v.size], dtype=np.int64).tofile(f)
            v.tofile(f)


@pytest.fixture(scope="module")
def layout_check(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    exe = str(tmp_path_factory.mktemp("layout_check") / "layout_check")
    subprocess.run([hipcc, "--offload-host-only", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "layout_check.cpp"), os.path.join(CSRC, "tree_layout.cpp"), "-o", exe],
                   check=True, timeout=600)
    return exe


@pytest.fixture(scope="module")
def problem_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("layout_problems")
    rows = {r["id"]: r for r in ROUTES + WIDE_ROUTES}
    out = {}
    for rid in ROWS:
        pb = build_problem(rows[rid])
        path = str(d / (rid + ".bin"))
        write_problem(path, problem_arrays(pb))
        out[rid] = (path, rows[rid], bool(pb.get("limited_tree", False)))
    return out


def run_check(exe, path, row, limited, world, rank, *extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("SPAMTREE_")}
    env.update(row["env"])
    r = subprocess.run([exe, path, str(world), str(rank)] + (["limited"] if limited else []) + list(extra), env=env,
                       capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout.strip()


@pytest.mark.parametrize("world,rank", SHARDS)
@pytest.mark.parametrize("rid", list(ROWS))
def test_layout_invariants(layout_check, problem_files, rid, world, rank):
    path, row, limited = problem_files[rid]
    rc, out = run_check(layout_check, path, row, limited, world, rank)
    assert rc == 0 and out.startswith("OK "), out
    report = {k: int(v) for k, v in (kv.split("=") for kv in out.split()[1:])}
    assert ROWS[rid](report), out
    if world > 1:
        assert report["cut"] < report["levels"], out      # the row is really sharded


def test_a_raised_group_width_is_named(layout_check, problem_files):
    path, row, limited = problem_files["grid_leaf32_pred32"]
    rc, out = run_check(layout_check, path, row, limited, 1, 0, "raise-group-m")
    assert rc == 1, out
    assert out.startswith("VIOLATED column groups:") and "M is" in out and "its blocks have" in out, out
