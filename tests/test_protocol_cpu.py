"""The pure parts of the iteration's read-back protocol (spamtree_amd/csrc/st_protocol.hpp), checked on the CPU:
tests/protocol_check.cpp is compiled against that header alone (host code only; the header includes no HIP header) and run.
It checks landing_code on "no failure" and on failure words of every code at several levels (the code is the low four bits),
rank_failure for 1, 3 and 64 ranks with no, one and two different failures (the smaller word wins), and, with static_asserts,
that the members of the pinned area do not overlap and that a Landing's failure word is 4-byte aligned.  The same program
built with the address and undefined-behaviour sanitizers runs clean; nothing is preloaded."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spamtree_amd", "csrc")
SANITIZE = ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]


def build_check(tmp, name, extra):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    exe = str(tmp / name)
    subprocess.run([hipcc, "--offload-host-only", "-std=c++17", "-O1"] + extra + ["-I", CSRC, os.path.join(ROOT, "tests", "protocol_check.cpp"),
                    "-o", exe], check=True, timeout=600)
    return exe


@pytest.mark.parametrize("name,extra", [("protocol_check", []), ("protocol_check_san", SANITIZE)], ids=["plain", "sanitized"])
def test_protocol_known_answers(tmp_path, name, extra):
    r = subprocess.run([build_check(tmp_path, name, extra)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    words = (r.stdout + r.stderr).split()
    assert words[:2] == ["protocol", "ok"] and int(words[2]) == 40, r.stdout + r.stderr


def test_the_header_includes_no_hip_header():
    """... so that the check above really is host code: only the C++ standard library."""
    src = open(os.path.join(CSRC, "st_protocol.hpp")).read()
    includes = [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include")]
    assert includes and all(i.startswith("<c") and "hip" not in i for i in includes), includes
