"""The pure host helpers of the summaries of the stored draws (spamtree_amd/csrc/store_spec.cpp), checked on the CPU:
tests/store_spec_check.cpp is compiled against store_spec.cpp alone (host code only, no HIP header) and compares
thresholds_in_store_order, mask_in_store_order, scatter_rows and check_thresholds with plain loops of its own: n in {1, 5, 64, 65},
T in {0, 1, 8} (T = 0: the band-only excursions, where only the mask and the scatter run), G in {1, 3}, no perm, the identity, a
reversal and a random permutation, thresholds per domain and per series (only the latter follow perm), every single negative side
and its bit, every destination of a scatter written exactly once and none with rows = 0, and the refusals of a NaN, an infinity, a
side of 0 and the counts -1 and ST_EXC_MAX_THRESHOLDS + 1 with the texts the C-ABI calls report.  The three spec checkers the
C-ABI calls and the whole fit's plan share (check_excursion_spec, check_rank_spec, check_exceed_spec): every refusal of each with
its whole text, in its order, and a count out of range refused before any value is read.

The counts the program prints prove that the loops ran; one negative case proves that the checks can fail; and the same program
built with the address and undefined-behaviour sanitizers runs clean (every input array has exactly the size a helper may read)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spamtree_amd", "csrc")


def build_check(tmp, name, extra):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    exe = str(tmp / name)
    subprocess.run([hipcc, "--offload-host-only", "-std=c++17", "-O1"] + extra + ["-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "store_spec_check.cpp"), os.path.join(CSRC, "store_spec.cpp"), "-o", exe], check=True, timeout=600)
    return exe


def run_check(exe, *args):
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=120)
    return r.returncode, (r.stdout + r.stderr).strip()


def report(out):
    return {k: int(v) for k, v in (kv.split("=") for kv in out.split()[1:])}


# 4 sizes x 4 perms: thresholds T in {1, 8} x G x per-domain / per-series; a scatter of T and of 1 rows per T and type; a mask
WANT = dict(thresholds=16 * 8, sides=16 * 4 * (3 + 10), masks=16, scatters=16 * 18)


@pytest.fixture(scope="module")
def spec_check(tmp_path_factory):
    return build_check(tmp_path_factory.mktemp("store_spec_check"), "store_spec_check", [])


def test_helpers_against_plain_loops(spec_check):
    rc, out = run_check(spec_check)
    assert rc == 0 and out.startswith("OK "), out
    r = report(out)
    assert {k: r[k] for k in WANT} == WANT and r["refusals"] >= 5, out


def test_two_exchanged_thresholds_are_named(spec_check):
    rc, out = run_check(spec_check, "swap")
    assert rc == 1 and out.startswith("VIOLATED thresholds: n 5 T 8 ") and "per_series 1" in out and "not at store position" in out, out


def test_no_hip_header_is_included():
    """store_spec.cpp and the header it includes stay free of the HIP runtime: the check above needs no device."""
    for f in ("store_spec.cpp", "draw_store.hpp"):
        text = open(os.path.join(CSRC, f)).read()
        assert "#include <hip" not in text and "st_device.hpp" not in text and "st_handle.hpp" not in text, f


def test_the_check_runs_clean_under_the_sanitizers(tmp_path_factory):
    """The stand-alone program (helpers and checker) with -fsanitize=address,undefined, on the CPU: nothing is preloaded."""
    exe = build_check(tmp_path_factory.mktemp("store_spec_check_san"), "store_spec_check_san",
                      ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"])
    rc, out = run_check(exe)
    assert rc == 0 and out.startswith("OK "), out
    assert report(out)["scatters"] == WANT["scatters"], out
