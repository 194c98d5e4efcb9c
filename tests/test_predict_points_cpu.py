"""CPU-only checks of new-point prediction (spamtree_amd/predict.py, st_points_*): the locator reproduces the tree's own
placement of NA rows, every kernel k_predict.hip launches is proven to run by a GPU test, and the new C-ABI symbols are
declared, bound and exported."""
import ast
import os
import re

import numpy as np
import pytest

from tests.util import make_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KSRC = os.path.join(ROOT, "spamtree_amd", "csrc", "k_predict.hip")
GPU_TESTS = os.path.join(ROOT, "tests", "test_gpu_predict_points.py")
NEW_SYMBOLS = ["st_points_set", "st_points_predict", "st_points_info", "st_points_route_name"]


@pytest.mark.parametrize("kw", [
    dict(side=30, q=1, seed=1, missing=0.1),
    dict(side=20, q=3, seed=3, missing=[0.1, 0.3, 0.5], cherrypick_same_margin=True),
    dict(side=30, q=1, seed=5, missing=0.1, last_not_reference=False),
    dict(side=12, q=6, seed=3, missing=[0.05, 0.1, 0.15, 0.2, 0.3, 0.4], cherrypick_same_margin=True),
], ids=["q1", "q3_same_margin", "reference_anchors", "q6_same_margin"])
def test_locate_reproduces_the_missing_rows_parents(kw):
    from spamtree_amd.predict import conditioning_set, locate
    pb = make_problem(**kw)
    topo = pb["topo"]
    na = np.nonzero(~np.isfinite(pb["y"]))[0]
    assert na.size > 20
    anchor = locate(topo, topo.coords[na], topo.mv_id[na])
    levels = np.unique(topo.block_groups)
    ref_anchor = 0
    for i, b in zip(na, anchor):
        u = int(topo.blocking[i]) - 1                       # the missing block the tree put row i in
        assert np.array_equal(conditioning_set(topo, int(b)), topo.parents(u)), (i, b, u)
        ref_anchor += int(topo.res_is_ref[int(np.searchsorted(levels, topo.block_groups[b]))])
    if kw.get("last_not_reference") is False:
        assert ref_anchor == na.size                        # every anchor is a reference block there
    else:
        assert ref_anchor == 0


def test_locate_in_the_callers_order():
    from spamtree_amd.predict import locate
    pb = make_problem(side=20, q=1, seed=2, missing=0.1)
    rng = np.random.default_rng(0)
    pts = rng.uniform(size=(200, 2))
    mv = np.ones(200, dtype=np.int64)
    a = locate(pb["topo"], pts, mv)
    perm = rng.permutation(200)
    assert np.array_equal(locate(pb["topo"], pts[perm], mv[perm]), a[perm])


def launched_kernels():
    src = open(KSRC).read()
    return {re.sub(r"\s+", "", m.group(1).strip("() "))
            for m in re.finditer(r"hipLaunchKernelGGL\(\s*(\(\s*[A-Za-z_]\w*\s*<[^>]*>\s*\)|[A-Za-z_]\w*)", src)}


def test_every_kernel_of_k_predict_is_proven_to_run_by_a_gpu_test():
    launched = launched_kernels()
    assert {"k_points_mfma<128>", "k_points_mfma<256>", "k_points_generic"} <= launched, launched
    # the route table spells exactly the launched instantiations
    src = open(KSRC).read()
    table = re.search(r"k_points_route_names\[PP_ROUTE_COUNT\]\s*=\s*\{(.*?)\};", src, re.S).group(1)
    named = {re.sub(r"\s+", "", s) for s in re.findall(r'"([^"]*)"', table) if s}
    assert named == launched
    # each one is named by a gpu test that reads st_points_info
    tree = ast.parse(open(GPU_TESTS).read())
    gsrc = open(GPU_TESTS).read()
    assert "pytestmark = pytest.mark.gpu" in gsrc
    bodies = [ast.get_source_segment(gsrc, f) for f in tree.body if isinstance(f, ast.FunctionDef) and f.name.startswith("test_")]
    for k in launched:
        spelled = k.replace(",", ", ")
        assert any((k in re.sub(r"\s+", "", b)) and ("points_info" in b or "route" in b) for b in bodies), \
            f"{spelled}: no gpu test proves through st_points_info that it ran"


def test_new_symbols_are_declared_bound_and_exported():
    from spamtree_amd import _lib, build
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spamtree_hip.h")).read(), flags=re.S)
    import ctypes
    lib = ctypes.CDLL(build.build())
    for s in NEW_SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", hdr), s
        assert s in _lib.SIGNATURES, s
        assert hasattr(lib, s), s


def test_product_sources_of_the_feature_stay_clear_of_the_checker():
    for p in ["spamtree_amd/predict.py", "spamtree_amd/csrc/k_predict.hip", "spamtree_amd/csrc/predict_points.hpp"]:
        assert "oracle" not in open(os.path.join(ROOT, p)).read().lower(), p


def test_new_point_streams_are_documented_and_mirrored():
    from spamtree_amd.rng import HostRng
    fit_h = open(os.path.join(ROOT, "include", "spamtree_fit.h")).read()
    assert re.search(r"stream 6 .*st_points_predict", fit_h) and re.search(r"stream 7 .*st_points_predict", fit_h)
    r = HostRng(7)
    z6, z7 = r.point_normals(3, 5), r.point_noise(3, 5)
    assert np.array_equal(z6, r._normal(np.arange(5), 0, 3, 6)) and np.array_equal(z7, r._normal(np.arange(5), 0, 3, 7))
    assert not np.array_equal(z6, z7)
