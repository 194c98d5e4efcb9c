"""CPU-only: every kernel instantiation the host code launches is covered -- by a row of the route table of
tests/test_gpu_routes.py (which proves through st_route_info that it reached it and compares it with the oracle), by
the table's explicit exclusions, or by an existing test named here.  A kernel added later without a test fails here."""
import glob
import os
import re

from tests import test_gpu_routes as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spamtree_amd", "csrc")
SRC = os.path.join(CSRC, "spamtree_hip.hip")
SRC_UNITS = sorted(glob.glob(os.path.join(CSRC, "st_*.hip")))   # the host units of the feature families (st_points.hip, ...)
SRC_POINTS_ACC = os.path.join(CSRC, "k_points_acc.hip")

# launched kernels without a route code that other tests compare with the oracle (or, for plumbing, check bit for bit);
# every route-coded kernel is reached by a row of the route table instead (test_every_route_coded_kernel_is_in_the_table)
COVERED_ELSEWHERE = {
    "k_xb": "tests/test_gpu_outputs.py::test_statistics_xb_yhat_xtx_match_extended_precision",
    "k_merge_err": "tests/test_gpu_chain.py::test_cpp_driver_with_top_levels_ahead_of_time",
    "k_pack_comps": "tests/test_gpu_sharded.py::test_sharded_equals_single_process_bitwise",
    "k_normals": "tests/test_gpu_parity.py::test_generated_sweep_normals_are_the_documented_stream",
    "k_pack_w": "tests/test_gpu_sharded.py::test_sharded_equals_single_process_bitwise",
    "k_gather_pack": "tests/test_gpu_sharded.py::test_sharded_equals_single_process_bitwise",
    "k_gather_unpack": "tests/test_gpu_sharded.py::test_sharded_equals_single_process_bitwise",
    "k_loglik": "tests/test_gpu_parity.py::test_factor_sample_loglik_predict_match_oracle",
    "k_loglik_grp": "tests/test_gpu_parity.py::test_factor_sample_loglik_predict_match_oracle",
    "k_stats": "tests/test_gpu_outputs.py::test_statistics_xb_yhat_xtx_match_extended_precision",
    "k_stats_final": "tests/test_gpu_outputs.py::test_statistics_xb_yhat_xtx_match_extended_precision",
    "k_yhat": "tests/test_gpu_outputs.py::test_statistics_xb_yhat_xtx_match_extended_precision",
    "k_cross_cov": "tests/test_gpu_outputs.py::test_cross_covariance_outcomes_and_row_counts",
    "k_axpy_sum": "tests/test_gpu_outputs.py::test_running_means_match_exact_sums",
    "k_qtile": "tests/test_gpu_outputs.py::test_summary_quantiles_at_every_pad_and_row_count",
    "k_points_acc": "tests/test_gpu_outputs.py::test_point_summaries_match_exact_moments",
}


def _norm(name):
    return re.sub(r"\s*,\s*", ", ", re.sub(r"\s+", " ", name.strip()))


def launched_kernels():
    """Every instantiation named by a hipLaunchKernelGGL of the host code, the kernel table and template wrappers expanded."""
    # (st_*.hip: the C-ABI of new-point prediction, the running summaries, ...; k_points_acc is launched from its own translation unit)
    assert SRC_UNITS, CSRC
    src = "".join(open(f).read() for f in [SRC] + SRC_UNITS + [SRC_POINTS_ACC])
    names = set()
    for m in re.finditer(r"hipLaunchKernelGGL\(\s*(\(\s*[A-Za-z_]\w*\s*<[^>]*>\s*\)|[A-Za-z_]\w*)", src):
        names.add(_norm(m.group(1).strip("() ")))
    # launch_quad launches quad_kernel(size, kind): every instantiation of k_factor_quad in that function's table
    assert "quad_kernel" in names, "k_factor_quad is no longer launched through quad_kernel: update this parser"
    names.discard("quad_kernel")
    table = re.search(r"static QuadKernel quad_kernel\(.*?\n}\n", src, re.S)
    quads = {_norm(q) for q in re.findall(r"k_factor_quad<[^>]*>", table.group(0))}
    assert len(quads) == 12, quads
    names |= quads
    # launch_factor<BIG, MODE>: k_factor<BIG, MODE> for every instantiation of the wrapper
    wraps = set(re.findall(r"launch_factor<\s*(true|false)\s*,\s*(MODE_\w+)\s*>", src))
    assert wraps, "launch_factor is no longer instantiated: update this parser"
    names.discard("k_factor<BIG, MODE>")
    names |= {f"k_factor<{b}, {m}>" for b, m in wraps}
    assert not [n for n in names if re.search(r"\b[A-Z][A-Z_]*_\b", n)], names   # no macro parameter left
    return names


def table_routes():
    names = set()
    for row in R.ROUTES + R.WIDE_ROUTES:
        for v in row["routes"].values():
            names.update(v)
    for v in R.CONFIG2_ROUTES.values():
        names.update(v)
    return names | {"k_sample_lean<false>"}      # test_lean_sample_without_latency_variant_matches_oracle_and_is_bitwise_lean_true


def test_every_launched_kernel_has_a_test():
    launched = launched_kernels()
    assert "k_factor_quad<4, 44, 11, true, false>" in launched and "k_sample_lean<true>" in launched   # the parser sees both forms
    assert "k_points_acc" in launched
    table = table_routes()
    missing = sorted(n for n in launched if n not in table and n not in R.EXCLUDED and n not in COVERED_ELSEWHERE)
    assert not missing, f"launched without a test: {missing}"
    stale = sorted(n for n in set(COVERED_ELSEWHERE) | set(R.EXCLUDED) | table if n not in launched)
    assert not stale, f"named but no longer launched: {stale}"


def test_covering_tests_exist():
    for name, ref in COVERED_ELSEWHERE.items():
        path, test = ref.split("::")
        assert re.search(rf"^def {re.escape(test)}\(", open(os.path.join(ROOT, path)).read(), re.M), (name, ref)


def test_route_table_reaches_the_quad_instantiations():
    table = table_routes()
    for nkx in (32, 38, 44):
        for wch in (True, False):
            assert R.quad(nkx, True, wch) in table, (nkx, wch)
    for nkx in (32, 38, 44, 50):
        assert R.quad(nkx, False, True) in table
        assert any(R.quad(nkx, False, True) in row["routes"].get("P", []) for row in R.ROUTES), nkx
    assert {R.quad(50, True, True), R.quad(50, True, False)} <= set(R.EXCLUDED)


def route_names():
    """Every name st_route_name spells (host code only, no device needed), in route-code order."""
    from spamtree_amd import build, _lib
    build.build()          # (a fresh checkout: the library may not be built yet)
    lib = _lib.load()
    assert lib.st_route_name(0) == b""
    names, code = [], 1
    while lib.st_route_name(code) is not None:
        names.append(lib.st_route_name(code).decode())
        code += 1
    return names


def test_route_names_spell_launched_instantiations():
    """st_route_name spells every route code as a launched instantiation."""
    launched = launched_kernels()
    names = route_names()
    assert len(names) == len(set(names))
    assert set(names) <= launched, sorted(set(names) - launched)
    # every instantiation of the per-level phases has a route code
    per_level = {n for n in launched if n.startswith(("k_factor", "k_marginal", "k_lchain", "k_gram", "k_sample"))}
    assert per_level <= set(names), sorted(per_level - set(names))


def test_every_route_coded_kernel_is_in_the_table():
    """A kernel with a route code is reached by a row of the route table (which proves it ran, through st_route_info, before
    comparing with the oracle) or excluded there with its reason -- never only mapped to a test that does not look at routes."""
    names = set(route_names())
    table = table_routes()
    assert not names & set(COVERED_ELSEWHERE), sorted(names & set(COVERED_ELSEWHERE))
    missing = sorted(n for n in names if n not in table and n not in R.EXCLUDED)
    assert not missing, f"route-coded but in no row of the route table: {missing}"
    assert not set(R.EXCLUDED) & table, sorted(set(R.EXCLUDED) & table)
