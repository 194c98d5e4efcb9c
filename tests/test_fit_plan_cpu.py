"""CPU-only: the plan step of stm_mcmc_fit (spamtree_amd/csrc/fit_plan.cpp) -- what the whole fit refuses before a chain exists and
the request as it is then run.  tests/fit_plan_check.cpp is compiled against fit_plan.cpp and store_spec.cpp alone (host code, no
HIP header) with the address and undefined-behaviour sanitizers; it is a stand-alone program and nothing is preloaded.  It holds

- accepted requests and their plan: the plain fit; a rows summary beside an empty point argument (dropped) and one with coords_new
  (kept); keep_draws raised to the stored draws of two chains, and to the total of three; an exc whose only content is rb; rb without
  thresholds beside an invalid side (no part); fun with n_fun = 0 and scores without y_new (no part); the criteria's CRPS;
- the order of refusals by two faults in one request, read from the plan's second text: both families before the chains, the stores'
  limit before a spec, diag's max_lag before want_rows, exc's spec before the count of draws, rk's prob before its thresholds, rb's
  point set before its n_thr;
- the texts stm_mcmc_chains_last_error() reports, and "" for every other refusal;
- a NULL pb where the plan needs q: ST_ERR_USAGE, with nothing read through the pointer.

Every array has exactly the size the plan may read."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spamtree_amd", "csrc")


def test_plan_check_program_under_the_sanitizers(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    exe = str(tmp_path / "fit_plan_check")
    subprocess.run([hipcc, "--offload-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "fit_plan_check.cpp"),
                    os.path.join(CSRC, "fit_plan.cpp"), os.path.join(CSRC, "store_spec.cpp"), "-o", exe], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK "), (r.stdout, r.stderr)
    got = {k: int(v) for k, v in (kv.split("=") for kv in r.stdout.split()[1:])}
    assert got == dict(accepted=14, refused=25, null_pb=3, texts=5), r.stdout


def test_the_plan_needs_no_device():
    """fit_plan.cpp and its header include no HIP header and make no st_* or stm_* call: the program above links without the library."""
    for f in ("fit_plan.cpp", "fit_plan.hpp"):
        text = open(os.path.join(CSRC, f)).read()
        assert "#include <hip" not in text and "st_device.hpp" not in text and "st_handle.hpp" not in text, f
