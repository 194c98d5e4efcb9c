"""The quad records st_create builds (spamtree_amd/csrc/tree_layout.cpp, build_quad_records), checked on the CPU:
tests/quad_record_check.cpp is compiled against that file alone (host code only), reads a problem from a flat binary file,
builds its layout with the MI355X's limits and rebuilds every field of every record from blks / grps / gdesc / quads and the
coordinates by the rules k_factor_quad's prologue used before the records existed.  The comparison is exact.

The problems are the rows of tests/test_gpu_routes.py that reach quads; every row runs as (world, rank) = (1, 0), (2, 0),
(2, 1), (3, 1), with SPAMTREE_QUAD_UNITS unset, 2 and 4.  SPAMTREE_QUAD_MIN=1 is added to every row's own switches: records
exist for the levels that TAKE k_factor_quad, and cfg5_mfma_chains_pred's own switches leave its (small) levels on
k_factor_mfma.  The counts the program reports prove that the rows met the cases they are here for, one negative case proves
that the comparison can fail, and the same program built with the address and undefined-behaviour sanitizers runs clean."""
import os
import shutil
import subprocess

import pytest

from tests.test_gpu_routes import ROUTES, WIDE_ROUTES, build_problem
from tests.test_tree_layout_cpu import write_problem
from tests.util import problem_arrays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spamtree_amd", "csrc")
ROW_IDS = ("grid_leaf32_pred32", "seg6_gram_direct", "cfg5_mfma_chains_pred")
SHARDS = [(1, 0), (2, 0), (2, 1), (3, 1)]
UNITS = [None, "2", "4"]   # (4: full quads, which a level this small does not take by itself)
# what a row's report must show on ONE GPU with the default units per quad: the cases the row is here for
ROW_CASES = {
    # leaf and prediction quads behind private ancestors of 25 rows (two sub-panels), reference quads above them; groups of
    # at most 16 columns; fewer than four units per quad (a level this small takes quads of one unit)
    "grid_leaf32_pred32": lambda r: (r["quads"] > r["ref_quads"] > 0 and r["pred_quads"] > 0 and r["priv_gt16"] > 0 and r["nu_lt4"] > 0
                                     and r["units_m_le16"] > 0),
    # eight reference levels of 9-row blocks
    "seg6_gram_direct": lambda r: r["ref_quads"] > 0 and r["quad_levels"] >= 8 and r["units_m_le16"] > 0,
    # three outcomes: the reference levels with chains of up to 200 rows
    "cfg5_mfma_chains_pred": lambda r: r["ref_quads"] > 0 and r["quad_levels"] >= 2,
}


def build_check(tmp, name, extra):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    exe = str(tmp / name)
    subprocess.run([hipcc, "--offload-host-only", "-std=c++17", "-O1"] + extra + ["-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "quad_record_check.cpp"), os.path.join(CSRC, "tree_layout.cpp"), "-o", exe],
                   check=True, timeout=600)
    return exe


@pytest.fixture(scope="module")
def record_check(tmp_path_factory):
    return build_check(tmp_path_factory.mktemp("quad_record_check"), "quad_record_check", [])


@pytest.fixture(scope="module")
def problem_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("quad_record_problems")
    rows = {r["id"]: r for r in ROUTES + WIDE_ROUTES}
    out = {}
    for rid in ROW_IDS:
        pb = build_problem(rows[rid])
        path = str(d / (rid + ".bin"))
        write_problem(path, problem_arrays(pb))
        out[rid] = (path, rows[rid], bool(pb.get("limited_tree", False)))
    return out


def run_check(exe, path, row, limited, world, rank, units, *extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("SPAMTREE_")}
    env.update(row["env"])
    env["SPAMTREE_QUAD_MIN"] = "1"
    if units is not None:
        env["SPAMTREE_QUAD_UNITS"] = units
    r = subprocess.run([exe, path, str(world), str(rank)] + (["limited"] if limited else []) + list(extra), env=env,
                       capture_output=True, text=True, timeout=120)
    return r.returncode, (r.stdout + r.stderr).strip()


def report(out):
    return {k: int(v) for k, v in (kv.split("=") for kv in out.split()[1:])}


@pytest.mark.parametrize("units", UNITS, ids=["units_default", "units_2", "units_4"])
@pytest.mark.parametrize("world,rank", SHARDS)
@pytest.mark.parametrize("rid", ROW_IDS)
def test_every_record_field_is_what_the_prologue_derived(record_check, problem_files, rid, world, rank, units):
    path, row, limited = problem_files[rid]
    rc, out = run_check(record_check, path, row, limited, world, rank, units)
    assert rc == 0 and out.startswith("OK "), out
    r = report(out)
    assert r["quads"] + r["pred_quads"] > 0 and r["record_bytes"] > 0, out
    if world == 1 and units is None:
        assert ROW_CASES[rid](r), out
    if units == "2":
        assert r["units"] <= 2 * r["quads"] + 4 * r["pred_quads"], out      # the level quads really have at most two units
    if units == "4" and rid == "grid_leaf32_pred32":
        assert r["nu_lt4"] < r["quads"] + r["pred_quads"], out              # ... and here some have four (the strips' reference blocks share their whole chain with one sibling only)
    if world > 1:
        assert r["cut"] < r["levels"], out                                  # the row is really sharded


def test_a_raised_row_length_is_named(record_check, problem_files):
    path, row, limited = problem_files["grid_leaf32_pred32"]
    rc, out = run_check(record_check, path, row, limited, 1, 0, None, "corrupt")
    assert rc == 1, out
    assert out.startswith("VIOLATED quad records:") and "field rlen differs" in out, out


def test_the_check_runs_clean_under_the_sanitizers(tmp_path_factory, problem_files):
    """The stand-alone program (builder and checker) with -fsanitize=address,undefined, on the CPU: nothing is preloaded."""
    exe = build_check(tmp_path_factory.mktemp("quad_record_check_san"), "quad_record_check_san",
                      ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"])
    for rid in ROW_IDS:
        path, row, limited = problem_files[rid]
        for world, rank, units in ((1, 0, None), (3, 1, "2")):
            rc, out = run_check(exe, path, row, limited, world, rank, units)
            assert rc == 0 and out.startswith("OK "), out
