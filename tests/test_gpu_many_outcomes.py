"""GPU: four to six outcomes through every kernel family that evaluates the multivariate covariance.

The Apanasovich-Genton covariance is not one function on the device: cov_entry / cov_entry_tab (generic, big, wide, mfma and
predict kernels), the LDS pair tables of k_factor_quad, the LC_CPT table of k_factor_lchain / k_factor_ref_finish and the copies
of the new-point kernels each look a pair of outcomes up on their own.  q = 4 and 5 are the only values whose row stride differs
from both 3 and QMAX = 6; q = 6 is the capacity edge (36 pair entries, a 36-entry theta, tausq_inv[QMAX] full, blocks of
cell_size x 6 rows).  Each row of ROWS is one problem with the switches that select its kernels, and each row, in this order,

  (a) runs the whole device protocol of tests/test_gpu_routes.py (both slots, three sweeps, st_predict, an accepted theta, a
      rebuild sweep and a cached one),
  (b) proves through st_route_info that it reached the instantiations it names, at the chain lengths (`at`) and block widths
      (`widths`) it names, inside A_BOUNDS,
  (c) holds to the NumPy oracle at the route table's REL = 1e-9 / REL_H = 1e-8 (test_row_reaches_its_kernels_and_matches_the_oracle),
  (d) holds to oracle/extended.py by the criterion of tests/test_gpu_conditioning.py, taken unchanged (kernels_vs_extended:
      e_dev <= C_BOUND max(e_64, 64 eps) per level for N, Ri or 1 / sqrt(r), the logdet and loglik_w components, the draws of
      the two deepest observed levels against cond_mean, and here also the rows without observations after st_predict against
      predict_draw), at distinct_theta and, on the big path, at the `cross` regime on it (Dmat entries 1e-3, ai2 = 1e-2 ai1:
      nearly singular q x q site blocks, which grow with q)  (test_row_loses_no_more_than_lapack).

Inputs that tell the outcomes apart, on the device and in both references alike: tests/util.distinct_theta (every per-outcome
and per-pair entry different, ai1 of mixed sign; nice_theta gives outcomes 4 to 6 the same ai1), one tausq and one column of
Bcoeff per outcome (many_inputs), and drop probabilities that rise from a third to five thirds of the row's rate over the
outcomes (uneven).

What the rows established on an MI355X (every expectation below was read from the dispatch code first, then confirmed):
  * st_create refuses no width on a full tree.  The default tree (cell_size 25) has 100-row reference blocks at q = 4 and 117-
    to 138-row ones at q = 6; they are factorised and swept by the scratch-arena generic kernels (k_factor<true, MODE_FACTOR>,
    k_sample<true, false>, k_gram_big), their leaf levels by k_factor_lchain<96>, and agree with both references;
  * blocks without observations take k_factor_quad<4, 32, 8, false, true> on the column-group path whatever SPAMTREE_QUAD_MIN
    says, and the LDS generic kernel k_factor<false, MODE_PREDICT> on the big-path rows;
  * one bug: limited_tree with a reference block of more than 101 rows (the default tree at q = 5 and 6: the row `q6_limited`
    of the plan, side 10, a 150-row root) passed st_create and then failed in st_factor with "hipGetLastError(): invalid
    argument": k_marginal_invchol asks for 2 m^2 doubles of LDS.  st_create now refuses such a tree with ST_ERR_UNSUPPORTED and
    both widths in the text (test_limited_tree_refuses_...); q6_limited96 runs the kernel at 89 to 92 rows instead.

Observed (every case succeeded on the device and in the oracle; columns as in tests/test_gpu_conditioning.py: smallest relative
Schur pivot of the checked blocks, worst e_64, worst e_dev, worst ratio e_dev / max(e_64, 64 eps)):
  row                        regime     pivot    e_64     e_dev    ratio
  q5_colgroup_mfma           distinct   8.8e-02  1.0e-14  3.5e-15   0.25
  q5_colgroup_quad           distinct   8.8e-02  1.0e-14  4.0e-15   0.28
  q6_colgroup_pred_mfma      distinct   8.6e-02  6.8e-15  4.3e-15   0.30
  q6_colgroup_pred_quad      distinct   8.6e-02  6.8e-15  4.3e-15   0.30
  q4_colgroup_mfma           distinct   8.8e-02  1.6e-14  1.5e-14   0.89
  q4_colgroup_quad           distinct   8.8e-02  1.6e-14  3.3e-15   0.20
  q4_big64_pred              distinct   5.9e-02  6.6e-14  1.2e-14   0.50
  q4_big64_pred              cross      1.8e-04  3.0e-09  5.6e-12   3.64
  q5_m80                     distinct   7.1e-02  1.8e-14  5.9e-15   0.41
  q5_m80                     cross      2.1e-04  9.3e-10  3.7e-12  10.73   (root loglik_w: RAISED)
  q6_big50_pred              distinct   7.8e-02  2.0e-14  7.9e-15   0.45
  q6_big50_pred              cross      1.3e-04  1.2e-09  4.1e-12   3.39
  q6_big50_bigmfma           distinct   7.8e-02  2.0e-14  1.3e-14   0.65
  q6_big50_bigmfma           cross      1.3e-04  1.2e-09  1.1e-11   3.39
  q5_m80_generic             distinct   7.1e-02  1.8e-14  6.2e-15   0.38
  q5_m80_generic             cross      2.1e-04  9.3e-10  3.6e-12  11.32   (root loglik_w: RAISED)
  q6_big50_sibling_groups    distinct   7.8e-02  2.0e-14  8.6e-15   0.44
  q6_big50_sibling_groups    cross      1.3e-04  1.2e-09  3.8e-12   3.39
  q4_default                 distinct   6.9e-02  3.1e-14  1.1e-14   0.69
  q4_default                 cross      2.1e-04  1.4e-09  3.9e-12  45.79   (root loglik_w: RAISED)
  q6_default_pred            distinct   8.4e-02  1.7e-14  1.1e-14   0.77
  q6_default_pred            cross      1.4e-04  1.4e-09  3.5e-12   5.85
  q6_limited96               distinct   8.6e-02  6.5e-15  5.4e-15   0.38
  q6_limited96               cross      1.4e-04  2.0e-10  2.5e-12   2.88
The whole file takes about 7 s on an MI355X host (40 cases, none above 1 s).

Shown to catch real errors (local, uncommitted builds; this file and the q > 3 cases of the other GPU files each time):
  1. `ij = vi * QMAX + vj` in lc_cov (factor_lchain.hpp) only: both tests of q4_big64_pred, q5_m80 and q4_default fail, the
     q = 6 rows pass (q = QMAX), as they must.  The mutant is not invisible at q <= 3 (3 != QMAX either): the q = 2 and 3 cases
     of test_gpu_reference_math, test_gpu_predict_points / _joint, test_gpu_simulate and test_gpu_chain fail as well, and so do
     the new q = 4 chain and q = 5 new-point cases.
  2. the same in k_factor_quad's table read (factor_quad.hpp): q5_colgroup_quad, q4_colgroup_quad and q4_colgroup_mfma (whose
     blocks without observations take k_factor_quad) fail in both tests; q6_colgroup_pred_* pass, as they must.
  3. `tausq_inv[min(mv, 2)]` in the generic sweep kernel k_sample<BIG, ...>: both tests of every big-path, default and limited
     row fail (27 cases), and the q = 4 and 6 cases of test_gpu_chain; the column-group rows do not run that kernel.
  4. ai1 of outcomes 4 and 5 swapped in finish_covpar: both tests of every q = 5 and q = 6 row fail (29 cases), and the q = 5
     case of test_gpu_predict_points and test_gpu_simulate, the q = 6 case of test_gpu_predict_joint and test_gpu_chain; the
     q = 4 rows pass, as they must.
"""
import numpy as np
import pytest

from tests.test_gpu_conditioning import kernels_vs_extended
from tests.test_gpu_routes import (NO_LCHAIN, QUAD_MIN, build_problem, check_levels, check_routes, compare_with_oracle, hip_model,
                                   inputs, problem_key, quad, run_device)
from tests.util import distinct_theta

pytestmark = pytest.mark.gpu


def uneven(rate, q):
    """Per-outcome drop probabilities around `rate`: the first outcome loses a third of it, the last five thirds."""
    return tuple(np.round(rate * np.linspace(1.0 / 3.0, 5.0 / 3.0, q), 4))


# Route keys as in tests/test_gpu_routes.py; further: `widths` (kernel, lo, hi: a level whose widest block has lo..hi rows took
# that phase-A kernel).  The geometry in the comments is that of make_problem(seed=11, ...), one line per level: m = block rows,
# P = chain rows.
LEAF_SWEEPS = ["k_sample_mfma", "k_sample_lean<true>", "k_sample_leaf_seg<4>"]
COLGROUP = {"A": ["k_factor_mfma"], "sweep": LEAF_SWEEPS}
COLGROUP_QUAD = {"A": [quad(32, True, True), quad(32, False, True)], "sweep": LEAF_SWEEPS}
PRED32 = {"P": [quad(32, False, True)]}
BIG = {"gram": ["k_gram_big"], "sweep": ["k_sample<true, false>", "k_sample<false>"]}
BIG_PRED = dict(BIG, P=["k_factor<false, MODE_PREDICT>"])
# m 20 / 20 / 15-20 / 5-10 (non-reference), P 0 / 20 / 40 / 55-60
Q5C = dict(side=12, q=5, kw=dict(cell_size=6))
# m 21 / 21-23 / 12-24 / 4-17 (non-reference), P 0 / 21 / 42-44 / 60-67; 32 blocks without observations, P <= 67
Q6C = dict(side=12, q=6, kw=dict(cell_size=5, missing=uneven(0.15, 6)))
# m 14 / 13-15 / 10-16 / 3-12 (non-reference), P 0 / 14 / 27-29 / 41-45; 26 blocks without observations.  (cell_size 7 or 8
# gives 36-row blocks, 30-34 with missing rows, and leaves the column-group path)
Q4C = dict(side=12, q=4, kw=dict(cell_size=6, missing=uneven(0.1, 4)))
# m 61 / 57-62 / 16-51 / 2-9 (non-reference), P 0 / 61 / 118-123 / 140-171; 13 blocks without observations, P <= 171
Q4B = dict(side=16, q=4, kw=dict(cell_size=16, missing=uneven(0.1, 4)))
# m 80 / 80 / 55 (non-reference), P 0 / 80 / 160
Q5B = dict(side=16, q=5, kw=dict(cell_size=16))
# m 44 / 43-49 / 17-35 / 3-10 (non-reference), P 0 / 44 / 87-93 / 104-123; 18 blocks without observations, P <= 123
Q6B = dict(side=12, q=6, kw=dict(cell_size=9, missing=uneven(0.2, 6)))
ROWS = [
    # the column-group path (every block of at most 32 rows) at row strides 5, 6 and 4 of the per-pair tables: by default on
    # k_factor_mfma, with SPAMTREE_QUAD_MIN=1 on k_factor_quad (its LDS pair tables); the blocks without observations on
    # k_factor_quad either way
    dict(id="q5_colgroup_mfma", **Q5C, env={}, regimes=["distinct"], routes=COLGROUP, at=[("k_factor_mfma", 55, 60)]),
    dict(id="q5_colgroup_quad", **Q5C, env=QUAD_MIN, regimes=["distinct"], routes=COLGROUP_QUAD),
    dict(id="q6_colgroup_pred_mfma", **Q6C, env={}, regimes=["distinct"], routes=dict(COLGROUP, **PRED32)),
    dict(id="q6_colgroup_pred_quad", **Q6C, env=QUAD_MIN, regimes=["distinct"], routes=dict(COLGROUP_QUAD, **PRED32)),
    dict(id="q4_colgroup_mfma", **Q4C, env={}, regimes=["distinct"], routes=dict(COLGROUP, **PRED32)),
    dict(id="q4_colgroup_quad", **Q4C, env=QUAD_MIN, regimes=["distinct"], routes=dict(COLGROUP_QUAD, **PRED32)),
    # the big path: a 61-row root on <4, 5, 34>, 62- and 51-row reference levels on k_factor_lchain<96> + k_factor_ref_finish,
    # the leaf level on k_factor_lchain<96>; k_gram_big and the scratch-arena sweep on the reference levels, the LDS generic
    # kernels on the leaf level and the blocks without observations
    dict(id="q4_big64_pred", **Q4B, env={}, regimes=["distinct", "cross"], mirror=1,
         at=[("k_factor_lchain<96>", 140, 171), ("k_factor_ref_finish", 61, 61)],
         widths=[("k_factor_bigmfma<4, 5, 34>", 61, 61), ("k_factor_ref_finish", 62, 62), ("k_factor_ref_finish", 51, 51)],
         routes=dict(BIG_PRED, A=["k_factor_bigmfma<4, 5, 34>", "k_factor_lchain<96>", "k_factor_ref_finish", "k_lchain_scalars"])),
    # exactly 80 rows: the last width of k_factor_bigmfma<5, 3, 24> (the root), of k_factor_ref_finish and of the one-wave
    # solve of the scratch-arena sweep (level 1); a 55-column leaf level on k_factor_lchain<96>
    dict(id="q5_m80", **Q5B, env={}, regimes=["distinct", "cross"], mirror=1, at=[("k_factor_lchain<96>", 160, 160)],
         widths=[("k_factor_bigmfma<5, 3, 24>", 80, 80), ("k_factor_ref_finish", 80, 80), ("k_factor_lchain<96>", 55, 55)],
         routes=dict(BIG, A=["k_factor_bigmfma<5, 3, 24>", "k_factor_lchain<96>", "k_factor_ref_finish", "k_lchain_scalars"])),
    # 36 pair entries in the LC_CPT table of k_factor_lchain / k_factor_ref_finish; a 44-row root on <3, 5, 34>
    dict(id="q6_big50_pred", **Q6B, env={}, regimes=["distinct", "cross"], mirror=1,
         widths=[("k_factor_bigmfma<3, 5, 34>", 44, 44), ("k_factor_ref_finish", 49, 49)],
         routes=dict(BIG_PRED, A=["k_factor_bigmfma<3, 5, 34>", "k_factor_lchain<96>", "k_factor_ref_finish", "k_lchain_scalars"])),
    # one block per workgroup: 44 and 35 columns on <3, 5, 34>, 49 on <4, 5, 34> (the boundary at 48)
    dict(id="q6_big50_bigmfma", **Q6B, env=dict(NO_LCHAIN, SPAMTREE_WIDE="0"), regimes=["distinct", "cross"],
         widths=[("k_factor_bigmfma<3, 5, 34>", 44, 44), ("k_factor_bigmfma<4, 5, 34>", 49, 49), ("k_factor_bigmfma<3, 5, 34>", 35, 35)],
         routes=dict(BIG_PRED, A=["k_factor_bigmfma<3, 5, 34>", "k_factor_bigmfma<4, 5, 34>"]),
         not_routes={"A": ["k_factor_lchain<96>", "k_factor_ref_finish"]}),
    # the generic kernels on every level (every level on the big path: mirror = 0), k_sample_leaf_wide on the leaf level
    dict(id="q5_m80_generic", **Q5B, env={}, force_generic=True, regimes=["distinct", "cross"], mirror=0,
         routes={"A": ["k_factor<true, MODE_FACTOR>"], "gram": ["k_gram_big"], "sweep": ["k_sample<true, false>"],
                 "leaf_rebuild": ["k_sample_leaf_wide"], "leaf_cached": ["k_sample_leaf_wide"]},
         not_routes={"A": ["k_factor_bigmfma<5, 3, 24>", "k_factor_lchain<96>"]}),
    # sibling groups forced onto every level
    dict(id="q6_big50_sibling_groups", **Q6B, env=dict(NO_LCHAIN, SPAMTREE_WIDE="2"), regimes=["distinct", "cross"],
         routes=dict(BIG_PRED, A=["k_factor_wide<WG_JT>"]), not_routes={"A": ["k_factor_lchain<96>", "k_factor_bigmfma<3, 5, 34>"]}),
    # the default tree (cell_size 25) of four outcomes: m 100 / 100 / 16-44 (non-reference), P 0 / 100 / 200.  100-row
    # reference blocks on the scratch-arena generic factor and sweep kernels, the leaf level on k_factor_lchain<96>
    dict(id="q4_default", side=15, q=4, kw={}, env={}, regimes=["distinct", "cross"], mirror=1, at=[("k_factor_lchain<96>", 200, 200)],
         widths=[("k_factor<true, MODE_FACTOR>", 100, 100)],
         routes=dict(BIG, A=["k_factor<true, MODE_FACTOR>", "k_factor_lchain<96>"])),
    # the default tree at the cap of six outcomes: m 138 / 117-131 / 5-24 (non-reference), P 0 / 138 / 255-269; 12 blocks
    # without observations, P <= 269
    dict(id="q6_default_pred", side=12, q=6, kw=dict(missing=uneven(0.1, 6)), env={}, regimes=["distinct", "cross"], mirror=1,
         at=[("k_factor_lchain<96>", 255, 269)], widths=[("k_factor<true, MODE_FACTOR>", 138, 138), ("k_factor<true, MODE_FACTOR>", 131, 131)],
         routes=dict(BIG_PRED, A=["k_factor<true, MODE_FACTOR>", "k_factor_lchain<96>"])),
    # limited_tree: m 92 / 89-90 / 5-39 (non-reference), one parent per block, 15 blocks without observations; the marginal
    # factors of 89- to 92-row reference blocks (k_marginal_invchol holds 101 rows at most: test_limited_tree_refuses_...)
    dict(id="q6_limited96", side=12, q=6, kw=dict(cell_size=16, limited_tree=True, missing=uneven(0.1, 6)), env={},
         regimes=["distinct", "cross"], routes={"A": ["k_marginal_invchol"]}),
]


def check_widths(row, out):
    for name, lo, hi in row.get("widths", []):
        hits = [L["max_m"] for L, r in zip(out["levels"], out["trace"]["A"]) if name in r["A"]]
        assert any(lo <= m <= hi for m in hits), (row["id"], name, lo, hi, hits)


def many_inputs(pb):
    """inputs() of the route table with one coefficient column and one noise variance per outcome, all different."""
    q = pb["q"]
    inp = inputs(pb)
    inp["beta"] = np.outer(inp["beta"], 1.0 - 0.4 * np.arange(q))        # p x q: column j is 1, 0.6, 0.2, -0.2, ... times the first
    inp["tausq"] = np.array([0.2, 0.05, 0.4, 0.1, 0.3, 0.15])[:q]
    return inp


def regime_theta(q, regime):
    """distinct: tests/util.distinct_theta; cross: the conditioning file's regime on it (Dmat entries 1e-3, ai2 = 1e-2 ai1:
    co-located outcomes, nearly singular q x q site blocks)."""
    th = distinct_theta(q)
    if regime == "cross":
        th[q:2 * q] = 1e-2 * th[:q]
        th[3 * q + 3:] = 1e-3
    return th


def problem(row, regime="distinct"):
    pb = build_problem(row)
    pb["theta"] = regime_theta(pb["q"], regime)
    return pb


ROW = {r["id"]: r for r in ROWS}
# Raised bounds, keyed (row, regime, level, quantity), after the C_FAMILY precedent of the conditioning file: the loglik_w
# component of the ROOT block at the cross regime, one number per level.  Measured e_dev / max(e_64, 64 eps), both slots alike:
# q5_m80 10.73 (e_dev 1.8e-13, e_64 1.7e-14), q5_m80_generic 11.32, q4_default 45.79 (e_dev 6.5e-13, e_64 3.6e-15 < 64 eps).
# The quadratic form |Ri w|^2 inherits the error of Ri, which holds C_BOUND on the same blocks (e_dev 1.0e-12 / 1.35e-12, e_64
# 3.2e-13 / 4.0e-13, ratios 3.2 / 3.4): the device's component is as accurate as its factor, the oracle's is 20 to 100 times
# more accurate than its own factor on these single blocks.  Every other level, regime and quantity keeps C_BOUND.
RAISED = {("q5_m80", "cross", 0, "loglik"): 22.0, ("q5_m80_generic", "cross", 0, "loglik"): 23.0,
          ("q4_default", "cross", 0, "loglik"): 92.0}


@pytest.mark.parametrize("row", ROWS, ids=[r["id"] for r in ROWS])
def test_row_reaches_its_kernels_and_matches_the_oracle(row, monkeypatch):
    for k, v in row["env"].items():
        monkeypatch.setenv(k, v)
    pb = problem(row)
    inp = many_inputs(pb)
    out = run_device(pb, inp, force_generic=row.get("force_generic", False))
    check_routes(row, out["routes"])
    check_levels(row, out, pb)
    check_widths(row, out)
    compare_with_oracle(pb, inp, out, key=problem_key(row))


PARAMS = [(r["id"], g) for r in ROWS for g in r["regimes"]]


@pytest.mark.parametrize("rid,regime", PARAMS, ids=[f"{r}-{g}" for r, g in PARAMS])
def test_row_loses_no_more_than_lapack(rid, regime, monkeypatch):
    row = ROW[rid]
    for k, v in row["env"].items():
        monkeypatch.setenv(k, v)
    pb = problem(row, regime)
    theta = pb["theta"]
    inp = dict(many_inputs(pb), theta=theta, theta2=theta)
    res = kernels_vs_extended(row, pb, inp, theta, regime, (problem_key(row), regime), raised=RAISED, predict=True)
    if res is not None:
        print("TABLE  %-26s %-9s %8.1e %8.1e %8.1e %6.2f" % ((rid, regime) + res))


def test_limited_tree_refuses_a_reference_block_wider_than_the_marginal_factor_holds():
    """limited_tree with the default cell size at q = 6: a 150-row root.  k_marginal_invchol keeps K_uu and its inverse factor in
    LDS (2 m^2 doubles: 101 rows at 160 KB), so st_create refuses the tree with ST_ERR_UNSUPPORTED and a message that names
    both widths (before this check st_create succeeded and st_factor answered "invalid argument" from the launch), leaves no
    handle behind, and the next handle works."""
    from spamtree_amd.model import SpamTreeError
    pb = problem(dict(side=10, q=6, kw=dict(limited_tree=True)))      # m 150 / 96-126 (non-reference)
    assert max(len(ix) for ix in pb["indexing"]) == 150
    inp = many_inputs(pb)
    with pytest.raises(SpamTreeError, match=r"st_create failed \(-4\): limited_tree: a reference block of 150 rows .* 101 rows"):
        hip_model(pb, **inp)
    row = ROW["q4_colgroup_mfma"]
    pb = problem(row)
    hm = hip_model(pb, **many_inputs(pb))
    assert hm.get_loglik_comps_w(0) and np.isfinite(hm.loglik_w[0])
    hm.close()
