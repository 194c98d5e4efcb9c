"""CPU-only: the C-ABI library builds, loads, and exports every symbol include/spamtree_hip.h declares."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    syms = set()
    for hdr in ("spamtree_hip.h", "spamtree_fit.h", "spamtree_tree.h"):
        txt = open(os.path.join(ROOT, "include", hdr)).read()
        txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
        syms |= set(re.findall(r"\b((?:st|stm)_[a-z_0-9]+|spamtree_mv_mcmc_c)\s*\(", txt))
    return sorted(syms)


def test_header_declares_the_boundary():
    syms = declared_symbols()
    for needed in ["st_create", "st_destroy", "st_factor", "st_swap", "st_sample_w", "st_loglik_w", "st_predict",
                   "st_beta_stats", "st_tausq_stats", "st_set_beta", "st_set_tausq_inv", "st_get_w"]:
        assert needed in syms


def test_library_builds_and_exports_every_declared_symbol():
    from spamtree_amd import build, _lib
    path = build.build()
    lib = ctypes.CDLL(path)
    for s in declared_symbols():
        assert hasattr(lib, s), f"{s} declared in the header but not exported"
    assert sorted(_lib.SIGNATURES) == declared_symbols()


def test_product_has_no_cpu_fallback():
    """The host mirror must raise (not compute) when there is no GPU."""
    from tests.util import visible_gpus
    if visible_gpus() > 0:
        pytest.skip("GPU present")
    import numpy as np
    from spamtree_amd.model import SpamTreeMV, SpamTreeError
    from tests.util import make_problem
    pb = make_problem(side=8, q=1, seed=1)
    with pytest.raises(SpamTreeError):
        SpamTreeMV(pb["y"], pb["X"], pb["Z"], pb["coords"], pb["mv_id"], pb["blocking"], pb["gix_block"],
                   pb["res_is_ref"], pb["parents"], pb["children"], False, pb["block_names"], pb["block_groups"],
                   pb["indexing"], np.zeros(pb["n"]), np.zeros(pb["p"]), pb["theta"], 10.0)


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "spamtree_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".cpp", ".h", ".hpp")):
                src = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in src.replace("oracle.StRng", "").lower() or f == "build.py", f
