"""The term lists st_points_functionals_set builds (functionals_layout in spamtree_amd/csrc/points_layout.cpp), checked on the CPU:
tests/functionals_layout_check.cpp is compiled against the layout sources alone (host code only), reads a point set's size and joint
labels and the functionals in CSR form from a flat binary file and checks what k_fun_chunks and k_fun_finish trust: the chunks
partition every functional's terms in order, without gap or overlap, at most FUN_CHUNK each; every source index lies inside its
vector; every variance pair lies in one group, inside its block, with its coefficient; an empty functional has no chunk.

The counts the program reports prove that a row reached what it is here for; two negative cases prove that the checks can fail; the
refusals are checked by code and text; and the same program built with the address and undefined-behaviour sanitizers runs clean
over the good and the refused inputs."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spamtree_amd", "csrc")
ST_ERR_USAGE = -1
FUN_CHUNK = int(re.search(r"#define FUN_CHUNK (\d+)", open(os.path.join(CSRC, "points_fun.hpp")).read()).group(1))
SIZES = (0, 1, 63, 64, 65, FUN_CHUNK - 1, FUN_CHUNK, FUN_CHUNK + 1, 2 * FUN_CHUNK + 3)


def build_check(tmp, name, extra):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    exe = str(tmp / name)
    subprocess.run([hipcc, "--offload-host-only", "-std=c++17", "-O1"] + extra + ["-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "functionals_layout_check.cpp"), os.path.join(CSRC, "tree_layout.cpp"),
                    os.path.join(CSRC, "points_layout.cpp"), "-o", exe], check=True, timeout=600)
    return exe


def write_input(path, n_new, labels, n_fun, ptr, idx, wt):
    """n_new, joint flag, n_fun, then labels, ptr, idx, wt; None: a null pointer."""
    with open(path, "wb") as f:
        np.array([n_new, labels is not None, n_fun], dtype=np.int64).tofile(f)
        for v, ty in ((labels, np.int64), (ptr, np.int64), (idx, np.int64), (wt, np.float64)):
            v = np.zeros(0, dtype=ty) if v is None else np.ascontiguousarray(np.asarray(v, dtype=ty).ravel())
            np.array([v.size], dtype=np.int64).tofile(f)
            v.tofile(f)


def csr(rows):
    ptr = np.concatenate([[0], np.cumsum([len(r[0]) for r in rows])]).astype(np.int64)
    idx = np.concatenate([np.asarray(r[0], dtype=np.int64) for r in rows]) if rows else np.zeros(0, dtype=np.int64)
    wt = np.concatenate([np.asarray(r[1], dtype=np.float64) for r in rows]) if rows else np.zeros(0)
    return ptr, idx, wt


def sized_rows(n, rng, sizes=SIZES):
    """Functionals of the given term counts: points without repetition, mixed-sign weights over 1e-3 .. 1e3."""
    return [(rng.choice(n, k, replace=False), rng.choice([-1.0, 1.0], k) * 10.0 ** rng.uniform(-3, 3, k)) for k in sizes]


def site_labels(n, g, rng):
    """Groups of g points each (the last one shorter), the points in random order, labels not in order of appearance."""
    lab = np.empty(n, dtype=np.int64)
    lab[rng.permutation(n)] = 7000 - np.arange(n) // g
    return lab


def joint_rows(n, lab, rng):
    """A contrast inside a group, one member each of two groups, a whole group plus points of others, and a functional whose
    variance list exceeds a chunk; then the sized ones."""
    by = {}
    for i, l in enumerate(lab):
        by.setdefault(int(l), []).append(i)
    full = [m for m in by.values() if len(m) >= 2]
    a, b, c = full[0], full[1], full[2]
    rows = [((a[0], a[1]), (1.0, -1.0)), ((a[0], b[1]), (0.5, 0.5)),
            (list(c) + [a[1], b[0]], rng.standard_normal(len(c) + 2))]
    return rows + sized_rows(n, rng)


def case_plain(rng):
    n = 3000
    return n, None, sized_rows(n, rng) + [((5,), (1.0,))]


def case_sites(rng):
    n = 3000
    lab = site_labels(n, 2, rng)
    return n, lab, joint_rows(n, lab, rng)


def case_groups16(rng):
    n = 2203
    lab = site_labels(n, 16, rng)
    return n, lab, joint_rows(n, lab, rng) + [(np.arange(n), np.ones(n) / n)]


def case_no_points(rng):
    return 0, None, [((), ()), ((), ())]


def case_no_points_joint(rng):
    return 0, np.zeros(0, dtype=np.int64), [((), ())]


def case_no_functionals(rng):
    return 50, None, []


nv_pairs = 16 * 17 // 2
CASES = {
    "plain_sizes": (case_plain, lambda r: r["n_fun"] == len(SIZES) + 1 and r["nnz"] == r["n_var_terms"] == sum(SIZES) + 1 and r["empty"] == 1
                    and r["max_lin_chunks"] == 3 and r["max_var_chunks"] == 3 and r["full_chunks"] >= 8
                    and r["n_chunks"] == 2 * (sum(-(-k // FUN_CHUNK) for k in SIZES) + 1)),
    "joint_sites": (case_sites, lambda r: r["cross_group"] > 0 and r["offdiag"] > 0 and r["max_var_chunks"] >= 3 and r["n_var_terms"] > r["nnz"] and r["empty"] == 1),
    "joint_groups16": (case_groups16, lambda r: r["offdiag"] > 2203 * 7 and r["max_var_chunks"] >= 2203 // 16 * nv_pairs // FUN_CHUNK and r["max_lin_chunks"] == 3),
    "no_points": (case_no_points, lambda r: r["n_fun"] == 2 and r["nnz"] == 0 and r["n_chunks"] == 0 and r["empty"] == 2),
    "no_points_joint": (case_no_points_joint, lambda r: r["n_fun"] == 1 and r["n_chunks"] == 0),
    "no_functionals": (case_no_functionals, lambda r: r["n_fun"] == 0 and r["n_chunks"] == 0),
}


def case_file(tmp, rid):
    path = os.path.join(tmp, rid + ".fun")
    if not os.path.exists(path):
        n, lab, rows = CASES[rid][0](np.random.default_rng(11))
        write_input(path, n, lab, len(rows), *csr(rows))
    return path


def run_check(exe, path, flags=()):
    r = subprocess.run([exe, path] + list(flags), capture_output=True, text=True, timeout=120)
    return r.returncode, (r.stdout + r.stderr).strip()


def report(out):
    return {k: int(v) for k, v in (kv.split("=") for kv in out.split()[1:])}


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp("functionals_layout"))


@pytest.fixture(scope="module")
def layout_check(tmp_path_factory):
    return build_check(tmp_path_factory.mktemp("functionals_layout_check"), "functionals_layout_check", [])


@pytest.mark.parametrize("rid", list(CASES))
def test_layout_invariants(layout_check, tmp, rid):
    rc, out = run_check(layout_check, case_file(tmp, rid))
    assert rc == 0 and out.startswith("OK "), out
    assert CASES[rid][1](report(out)), out


def test_a_shifted_chunk_is_named(layout_check, tmp):
    rc, out = run_check(layout_check, case_file(tmp, "plain_sizes"), ["shift-chunk"])
    assert rc == 1 and out.startswith("VIOLATED linear chunks: chunk ") and " starts at term " in out, out


@pytest.mark.parametrize("rid,text", [("plain_sizes", "is not (a^2, i) of entry"), ("joint_sites", "variance list: term ")])
def test_two_exchanged_variance_terms_are_named(layout_check, tmp, rid, text):
    rc, out = run_check(layout_check, case_file(tmp, rid), ["swap-pair"])
    assert rc == 1 and out.startswith("VIOLATED variance list: term ") and text in out, out


# ---- the refusals of st_points_functionals_set, in the order of their checks
def refusal_inputs(tmp):
    """name -> (input file, text)."""
    n = 40
    good = [((0, 1, 2), (1.0, 2.0, 3.0)), ((), ()), ((5, 7), (0.5, -0.5))]
    out = {}

    def add(name, text, n_new=n, labels=None, n_fun=3, edit=None, null=()):
        ptr, idx, wt = csr(good)
        if edit:
            edit(ptr, idx, wt)
        arrs = dict(ptr=ptr, idx=idx, wt=wt)
        for k in null:
            arrs[k] = None
        path = os.path.join(tmp, "refuse_" + name + ".fun")
        write_input(path, n_new, labels, n_fun, arrs["ptr"], arrs["idx"], arrs["wt"])
        out[name] = (path, "st_points_functionals_set: " + text)

    def setter(which, k, v):
        def edit(ptr, idx, wt):
            dict(ptr=ptr, idx=idx, wt=wt)[which][k] = v
        return edit

    add("negative_n_fun", "bad sizes or NULL inputs", n_fun=-1)
    add("null_ptr", "bad sizes or NULL inputs", null=("ptr",))
    add("null_idx", "bad sizes or NULL inputs", null=("idx",))
    add("null_wt", "bad sizes or NULL inputs", null=("wt",))
    add("ptr0", "ptr[0] is not 0", edit=setter("ptr", 0, 1))
    add("ptr_decreases", "ptr decreases at functional 1", edit=setter("ptr", 2, 2))
    add("index_negative", "functional 2, entry 1: index -1 is not a point of the set (0..39)", edit=setter("idx", 4, -1))
    add("index_past_the_set", "functional 0, entry 2: index 40 is not a point of the set (0..39)", edit=setter("idx", 2, 40))
    add("weight_nan", "functional 0, entry 1: the weight is not finite", edit=setter("wt", 1, np.nan))
    add("weight_inf", "functional 2, entry 0: the weight is not finite", edit=setter("wt", 3, -np.inf))
    add("point_twice", "functional 2, entry 1: point 5 occurs twice in the functional", edit=setter("idx", 4, 5))
    add("point_twice_joint", "functional 0, entry 2: point 0 occurs twice in the functional", labels=np.arange(n) // 2, edit=setter("idx", 2, 0))
    add("no_points", "functional 0, entry 0: index 0 is not a point of the set (0..-1)", n_new=0)
    return out


REFUSALS = ["negative_n_fun", "null_ptr", "null_idx", "null_wt", "ptr0", "ptr_decreases", "index_negative", "index_past_the_set",
            "weight_nan", "weight_inf", "point_twice", "point_twice_joint", "no_points"]


@pytest.fixture(scope="module")
def refusals(tmp):
    out = refusal_inputs(tmp)
    assert sorted(out) == sorted(REFUSALS)
    return out


@pytest.mark.parametrize("name", REFUSALS)
def test_refusals_name_the_functional_and_entry(layout_check, refusals, name):
    path, text = refusals[name]
    rc, out = run_check(layout_check, path)
    assert rc == 2 and out == "REFUSED %d %s" % (ST_ERR_USAGE, text), out


def test_the_same_point_in_two_functionals_is_no_duplicate(layout_check, tmp):
    path = os.path.join(tmp, "shared.fun")
    write_input(path, 10, None, 2, *csr([((1, 2), (1.0, 1.0)), ((2, 1), (1.0, -1.0))]))
    rc, out = run_check(layout_check, path)
    assert rc == 0 and report(out)["nnz"] == 4, out


def test_the_check_runs_clean_under_the_sanitizers(tmp_path_factory, tmp, refusals):
    """The stand-alone program (builder and checker) with -fsanitize=address,undefined, on the CPU: nothing is preloaded."""
    exe = build_check(tmp_path_factory.mktemp("functionals_layout_check_san"), "functionals_layout_check_san",
                      ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"])
    for rid in CASES:
        rc, out = run_check(exe, case_file(tmp, rid))
        assert rc == 0 and out.startswith("OK "), out
    for name, (path, text) in refusals.items():
        rc, out = run_check(exe, path)
        assert rc == 2 and out == "REFUSED %d %s" % (ST_ERR_USAGE, text), (name, out)
