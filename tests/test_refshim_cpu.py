"""The Armadillo / Rcpp stand-in the reference's files are compiled against (oracle/refshim/RcppArmadillo.h), checked on the CPU
by a stand-alone program with hand-written known answers: tests/refshim_check.cpp is compiled against that header alone (host
code, no sanitiser here) and run.  It covers inclusive subvec bounds, symmatl against symmatu, the column-major (i, j)
mapping, repmat tiling, sum along both dimensions, chol lower on a 3 x 3 matrix with a known factor and its throw on an
indefinite one, and the order of rows(uvec).  It needs neither the reference tree nor the library built from it."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_refshim_known_answers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    exe = str(tmp_path / "refshim_check")
    # the flags of oracle/Makefile's REF_CXXFLAGS (no -march, no -mfma)
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "oracle", "refshim"),
                    os.path.join(ROOT, "tests", "refshim_check.cpp"), "-o", exe], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    words = r.stdout.split()
    assert words[:2] == ["refshim", "ok"] and int(words[2]) >= 45
