"""CPU-only: every (row, level) that tests/test_gpu_failure_routes.py makes fail on the device fails on the oracle at
exactly that level with the code the case expects -- phase A with the finite out-of-bounds theta (every shallower level
succeeds: the oracle returns after the first failing level), the sweep with the per-outcome tausq^-1 -- and the relabelling
left the tree, the block widths and the chain lengths alone.  Rows of one problem share the construction: one test for them.
Also: every reference-level case of the phase-A table sits right above a non-reference level (what makes a dropped flag
visible on the device), and the two-rank construction of tests/test_gpu_sharded.py."""
import numpy as np
import pytest

from tests import test_gpu_failure_routes as F
from tests.test_gpu_routes import build_problem

EXPECT = {}      # (problem, level) -> the first row on it, the level, the phase-A code, the sweep code (None: not used)


def expect(row, level, a=None, s=None):
    e = EXPECT.setdefault((F.problem_key(F.ROW[row]), level), dict(row=row, level=level, a=None, s=None))
    for k, v in (("a", a), ("s", s)):
        if v is not None:
            assert e[k] in (None, v), (row, level, k, e[k], v)
            e[k] = v


for c in F.A_CASES:
    expect(c[0], c[1], a=c[3])
for c in F.SWEEP_CASES + [F.TWO_LEVELS]:
    expect(c[0], c[1], s=c[4])
for row in (F.SMALL["id"], F.TOPS["id"]):
    nl = F.n_levels(row)
    expect(row, nl - 1, a=3, s=11)
    expect(row, nl - 2, a=2, s=10)
expect(F.TOPS["id"], "root", a=1)
CASES = sorted(EXPECT.values(), key=lambda e: (e["row"], str(e["level"])))


@pytest.mark.parametrize("case", CASES, ids=[f"{e['row']}-L{e['level']}" for e in CASES])
def test_construction_fails_on_the_oracle_at_the_intended_level(case):
    row, level = case["row"], case["level"]
    ref = F.construction(F.ROW[row], level, recover=False)      # (the recovery run is the GPU cases' own)
    if case["a"] is not None:
        F.check_construction_a(row, level, case["a"], ref)
    if case["s"] is not None:
        F.check_construction_sweep(row, level, case["s"], ref)
    pb, fp = build_problem(F.ROW[row]), ref["fp"]
    for k in ("parents", "children", "indexing"):
        assert all(np.array_equal(a, b) for a, b in zip(pb[k], fp[k])), k
    assert np.array_equal(pb["block_groups"], fp["block_groups"]) and np.array_equal(pb["coords"], fp["coords"])
    assert np.all(np.isfinite(ref["f"]["theta_bad"])) and np.all(np.isfinite(ref["f"]["tausq_inv_bad"]))
    rows = ref["f"]["rows"]
    if level == "root":          # sigma^2 < 0 on the row's own problem: nothing is relabelled
        assert rows.size == 0 and np.array_equal(fp["mv_id"], pb["mv_id"])
        return
    assert fp["q"] == pb["q"] + 1 and np.all(fp["mv_id"][rows] == fp["q"])
    assert np.count_nonzero(fp["mv_id"] != pb["mv_id"]) == rows.size


def test_reference_level_cases_sit_on_the_last_reference_level():
    """The device runs the levels below a failing one too, and they flag the indefinite chain themselves: errtype 2 on a
    reference level, 3 on a non-reference one.  A reference-level case whose flag was dropped returns 3 instead of 2 only if
    the next level is a non-reference one."""
    for c in F.A_CASES:
        row, level, code = c[0], c[1], c[3]
        isref = np.asarray(build_problem(F.ROW[row])["res_is_ref"])
        assert isref[level] == (1 if code in (1, 2) else 0), (row, level, code)
        if code == 2:
            assert isref[level + 1] == 0, (row, level)


def test_two_rank_construction_fails_on_the_oracle_in_one_ranks_subtrees(monkeypatch):
    from tests._sharded_worker import FAILURE_CASE, failure_problem_on_oracle
    monkeypatch.setenv("SPAMTREE_QUAD_MIN", "1")
    (pb, fp, f, level, owner), _, _ = failure_problem_on_oracle(FAILURE_CASE)
    assert np.array_equal(pb["block_groups"], fp["block_groups"]) and fp["q"] == pb["q"] + 1
