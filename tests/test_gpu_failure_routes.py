"""GPU: the failure protocol (errtype 1 / 2 / 3 of phase A, 10 / 11 of the sweep) on every kernel route and on every path the
failure word travels to the caller.

Each phase-A and sweep kernel family has its own site that detects a non-positive pivot and writes the failure word
(atomicMin(errflag, level * 16 + code)).  Here every instantiation of the route tables of tests/test_gpu_routes.py (ROUTES /
WIDE_ROUTES, rows reused by id with their environments and force_generic; one row of this file's own, ref30_depth5) is
the kernel of the shallowest failing level: every shallower level succeeds.  tests/util.level_failure_problem relabels a few observed rows of ONE level as outcome q + 1 (the
tree, the block widths and the chain lengths stay the row's own) and gives

  (a) a finite theta outside the bounds (negative Dmat entries towards the new outcome): phase A succeeds on every shallower
      level and fails at that level -- errtype 2 on a reference level, 3 on a non-reference one, 1 at the root;
  (b) a per-outcome tausq^-1 that is negative for the new outcome only: the sweep fails at that level only -- 10 / 11.

Every case asserts first ON THE ORACLE that the construction fails at the intended level with the intended code (the level
derived from the oracle's per-block state, tests/util.oracle_phase_a_failure / oracle_sweep_failing_levels; the same
assertions run without a GPU in tests/test_failure_constructions_cpu.py), then through route_info() of the failing call
that this level ran the instantiation under test, and only then looks at the device's return code.

Phase A (A_CASES): the code is the oracle's; logdet, loglik, Ri and H of every observed block of the levels above the
failing one agree with the oracle (REL / REL_H); the accepted slot is untouched -- st_loglik_w(0) and the w of one sweep with
a fixed z are bit-identical to those of a twin handle that never saw the failing proposal; the proposal slot recovers --
factorised at a valid theta it gives the oracle's loglik_w, and after accept_make_change one sweep matches the oracle.
Sweep (SWEEP_CASES, "rebuild": the failing sweep is the first after the factorisation and forms the Gram parts, "cached": it
reads them): the code is the oracle's; after tausq^-1 and w are restored the next sweep agrees with the oracle and is
bit-identical to the same sweep of a twin handle that never failed (a failed rebuild sweep marks the Gram cache valid, so
this is what shows that the parts it wrote are the ones a successful sweep writes).  One case has a failing reference and a
failing non-reference level: the code is that of the shallower one.

What "the failing level" means on the device.  The oracle returns after the first failing level.  The device launches
every level, and the levels below the failing one meet its relabelled rows in their chains: they fail too and flag their own
level * 16 + code.  atomicMin keeps the shallowest level's word and the caller sees its code only.  So the level under test
is the sole failing kernel of the oracle's run and the shallowest of the device's; were its flag dropped, the caller would
see the code of the level below.  Every reference-level case (errtype 2) therefore sits on the LAST reference level of its
row, right above the leaf level, whose code is 3 (tests/test_failure_constructions_cpu.py asserts this for the table): a
dropped flag returns 3 instead of 2.  Leaf-level cases have nothing below them (0 instead of 3), the root cases have
reference levels below (2 instead of 1).  What the code cannot show: which of the two kernels of a reference level on
k_factor_lchain flagged it (k_factor_ref_finish completes the level; both flag its 2), and

k_marginal_invchol[_wave] (limited_tree: the marginal factors of every block with children, launched once ahead of level
0) cannot be the SOLE failing kernel: K_uu of a block is indefinite only if its Schur complement is, so the level's factor
kernel flags the same word.  Their cases fail a reference level whose blocks are on the marginal list; both kernels write
level * 16 + 2.

The paths of the word (small grids): st_factor_enqueue / st_factor_finish with the leaf deferral on and off,
st_factor_begin + st_factor (k_merge_err; a stale second-stream word does not leak into a factorisation at another theta),
st_sample_w_loglik and its _begin / _end pair, a one-rank communicator (k_pack_comps, st_mg_finish, k_gather_pack and the
fused exchange).  Two ranks with the failure in ONE rank's subtrees: tests/test_gpu_sharded.py.

Deliberate local breakages shown to be caught (uncommitted builds, this whole file each time; the failure-code tests of
tests/test_gpu_reference_math.py stayed green, 10 passed, in each):
  - k_factor_quad without the atomicMin of its reference levels (factor_quad.hpp, all NKX / wave variants at once): all six
    reference-level quad cases return 3 instead of 2 (ref30_depth5 L4, ref30_leaf50_pred50 L5, ref32_nkx44 L5,
    leaf38_pred38_wave L5, leaf44_pred44_leafsweep L6, ref25_wch_nkx44 L7), and so do the reference-level cases of
    st_factor_enqueue (both deferral settings) and of the one-rank communicator;
  - k_factor_bigmfma without its `s_fail = 1` for a non-positive conditional variance of a non-reference row
    (factor_big.hpp): wide4_bigmfma L7 <4, 5, 34> and limited_wide L2 <3, 5, 34> report success instead of errtype 3;
  - k_merge_err as a no-op: the root and the last-reference-level case of
    test_failure_of_levels_run_ahead_reaches_the_caller both return the leaf level's 3, instead of 1 and 2;
  - k_sample_leaf without its `s_fail = 1` (sample_kernels.hpp): leaf44_pred44_leafsweep L7 returns 0 instead of 11.

Wall time of this file (60 cases, the oracle's runs included) as pytest reports it on an MI355X host: 27 s; the two-rank
case of tests/test_gpu_sharded.py: 8 s.  Nearly all of it is the oracle, whose cost depends on the host's CPUs: the same
constructions in tests/test_failure_constructions_cpu.py (without the recovery runs) took about three minutes on a slower
CPU-only host, two of them on the three problems of 11 000 rows (wide4 at levels 6 and 7, leaf256), the only rows that
reach k_factor_lchain<136> and the 256-row chains of k_factor_mfma.

Cases as the tests print them on an MI355X (row, level, [kind,] instantiation, code):
  phase A  ref30_depth5               level 4  k_factor_quad<4, 32, 8, true, false>     code 2
  phase A  ref30_leaf50_pred50        level 5  k_factor_quad<4, 38, 10, true, false>    code 2
  phase A  ref30_leaf50_pred50        level 6  k_factor_quad<4, 50, 13, false, true>    code 3
  phase A  ref32_nkx44                level 5  k_factor_quad<4, 44, 11, true, false>    code 2
  phase A  leaf38_pred38_wave         level 5  k_factor_quad<4, 32, 8, true, true>      code 2
  phase A  leaf44_pred44_leafsweep    level 6  k_factor_quad<4, 38, 10, true, true>     code 2
  phase A  ref25_wch_nkx44            level 7  k_factor_quad<4, 44, 11, true, true>     code 2
  phase A  leaf38_pred38_wave         level 6  k_factor_quad<4, 38, 10, false, true>    code 3
  phase A  leaf44_pred44_leafsweep    level 7  k_factor_quad<4, 44, 11, false, true>    code 3
  phase A  grid_leaf32_pred32         level 3  k_factor_quad<4, 32, 8, false, true>     code 3
  phase A  leaf256_cached_mfma        level 8  k_factor_mfma                            code 3
  phase A  generic_lds                level 3  k_factor_lchain<96>                      code 3
  phase A  generic_lds                level 2  k_factor_lchain<96>                      code 2
  phase A  generic_lds                level 2  k_factor_ref_finish                      code 2
  phase A  wide4_default_pred         level 7  k_factor_lchain<136>                     code 3
  phase A  wide4_default_pred         level 6  k_factor_lchain<136>                     code 2
  phase A  wide4_default_pred         level 6  k_factor_ref_finish                      code 2
  phase A  limited_wide               level 1  k_factor_bigmfma<5, 3, 24>               code 2
  phase A  wide4_bigmfma              level 7  k_factor_bigmfma<4, 5, 34>               code 3
  phase A  limited_wide               level 2  k_factor_bigmfma<3, 5, 34>               code 3
  phase A  wide4_sibling_groups       level 7  k_factor_wide<WG_JT>                     code 3
  phase A  leafwide_edge_ma96_p384    level 3  k_factor<true, MODE_FACTOR>              code 2
  phase A  mixed_colgroup_big_leaf    level 3  k_factor<true, MODE_FACTOR>              code 3
  phase A  wide4_generic              level 6  k_factor<true, MODE_FACTOR>              code 2
  phase A  generic_lds                level 0  k_factor<false, MODE_FACTOR>             code 1
  phase A  limited_wave               level 2  k_marginal_invchol_wave                  code 2
  phase A  limited_wide               level 1  k_marginal_invchol                       code 2
  sweep    ref30_leaf50_pred50        level 6  cached  k_sample_leaf_seg<4>             code 11
  sweep    ref30_leaf50_pred50        level 5  cached  k_sample_lean<true>              code 10
  sweep    ref30_leaf50_pred50        level 5  rebuild k_sample_mfma                    code 10
  sweep    ref30_leaf50_pred50        level 6  rebuild k_sample_mfma                    code 11
  sweep    leaf256_cached_mfma        level 8  cached  k_sample_mfma                    code 11
  sweep    ref25_wch_nkx44            level 7  rebuild k_sample_lean<true>              code 10
  sweep    leaf38_pred38_wave         level 5  cached  k_sample_wave                    code 10
  sweep    leaf44_pred44_leafsweep    level 7  cached  k_sample_leaf                    code 11
  sweep    seg6_gram_direct           level 9  rebuild k_sample_leaf_seg<6>             code 11
  sweep    seg6_gram_direct           level 9  cached  k_sample_leaf_seg<6>             code 11
  sweep    wide4_default_pred         level 6  rebuild k_sample<true, false>            code 10
  sweep    wide4_default_pred         level 6  cached  k_sample<true, false>            code 10
  sweep    wide4_default_pred         level 7  rebuild k_sample_leaf_wide               code 11
  sweep    wide4_default_pred         level 7  cached  k_sample_leaf_wide               code 11
  sweep    wide4_no_grambig           level 7  rebuild k_sample<true, true>             code 11
  sweep    wide4_leafwide_off         level 7  cached  k_sample<true, true>             code 11
  sweep    generic_lds                level 3  rebuild k_sample<false>                  code 11
  sweep    generic_lds                level 3  cached  k_sample<false>                  code 11
  sweep    generic_lds                level 0  cached  k_sample<false>                  code 10
  sweep    ref30_leaf50_pred50        level 5  cached  k_sample_lean<true>              code 10
  sweep    ref30_leaf50_pred50        level 6  cached  k_sample_leaf_seg<4>             code 10
  enqueue  small25                    level 3  k_factor_quad<4, 32, 8, false, true>     code 3  defer True
  enqueue  small25                    level 3  k_factor_quad<4, 32, 8, false, true>     code 3  defer False
  enqueue  small25                    level 2  k_factor_quad<4, 32, 8, true, true>      code 2  defer True
  enqueue  small25                    level 2  k_factor_quad<4, 32, 8, true, true>      code 2  defer False
  begin    small40_tops               level 0  k_factor_mfma                            code 1  (g_top 3)
  begin    small40_tops               level 2  k_factor_mfma                            code 2  (g_top 3)
  begin    small40_tops               level 3  k_factor_quad<4, 32, 8, false, true>     code 3  (g_top 3)
  begin    small40_tops               level 2  stale word, valid theta: code 0
  loglik   small25                    level 3  st_sample_w / _loglik / _begin+_end: codes [11, 11, 11]
  loglik   small25                    level 2  st_sample_w / _loglik / _begin+_end: codes [10, 10, 10]
  comm     small25                    level 3  phase A code 3
  comm     small25                    level 3  st_sample_w / st_sample_w_loglik: codes [11, 11]
  comm     small25                    level 2  phase A code 2
  comm     small25                    level 2  st_sample_w / st_sample_w_loglik: codes [10, 10]
"""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_routes import EXCLUDED, REL, REL_H, ROUTES, WIDE_ROUTES, build_problem, problem_key, quad, relerr
from tests.util import level_failure_problem, oracle_model, oracle_phase_a_failure, oracle_sweep_failing_levels

pytestmark = pytest.mark.gpu

ROW = {r["id"]: r for r in ROUTES + WIDE_ROUTES}
DP = C.POINTER(C.c_double)
# ref30_leaf50_pred50 one level shallower: its 30-row reference level with chains of 120 rows (NKX 32, no wave elimination)
# is the LAST reference level, right above the leaf level
REF30_DEPTH5 = dict(id="ref30_depth5", strip=(640, 5, 1), kw=dict(cell_size=31, tree_depth=5, missing=0.15),
                    env={"SPAMTREE_QUAD_MIN": "1"}, routes={})
ROW[REF30_DEPTH5["id"]] = REF30_DEPTH5

# ---- phase A: row, level, instantiation, code.  `at=0`: the kernel is launched once ahead of level 0 and recorded there
# (the marginal factors).
# The device launches every level whatever the levels above did and keeps atomicMin(level * 16 + code), of which the caller
# sees the code only.  Below a failing reference level every level meets the indefinite chain and flags too: a reference
# level 2, a non-reference level 3.  A dropped flag on the level under test would therefore go unseen under another
# reference level (still 2), and shows as 3 under a non-reference one.  So every reference-level case (errtype 2) sits on
# the LAST reference level of its row, right above the leaf level (asserted for the whole table in
# tests/test_failure_constructions_cpu.py); the root case (errtype 1) shows as 2.
A_CASES = [
    ("ref30_depth5", 4, quad(32, True, False), 2),
    ("ref30_leaf50_pred50", 5, quad(38, True, False), 2),
    ("ref30_leaf50_pred50", 6, quad(50, False, True), 3),
    ("ref32_nkx44", 5, quad(44, True, False), 2),
    ("leaf38_pred38_wave", 5, quad(32, True, True), 2),
    ("leaf44_pred44_leafsweep", 6, quad(38, True, True), 2),
    ("ref25_wch_nkx44", 7, quad(44, True, True), 2),
    ("leaf38_pred38_wave", 6, quad(38, False, True), 3),
    ("leaf44_pred44_leafsweep", 7, quad(44, False, True), 3),
    ("grid_leaf32_pred32", 3, quad(32, False, True), 3),
    ("leaf256_cached_mfma", 8, "k_factor_mfma", 3),                 # leaf chains of 256 rows
    ("generic_lds", 3, "k_factor_lchain<96>", 3),
    # a reference level on k_factor_lchain is finished by k_factor_ref_finish; both flag level * 16 + 2 for a non-positive
    # conditional variance, so neither of the two is the sole failing kernel of its level
    ("generic_lds", 2, "k_factor_lchain<96>", 2),
    ("generic_lds", 2, "k_factor_ref_finish", 2),
    ("wide4_default_pred", 7, "k_factor_lchain<136>", 3),
    ("wide4_default_pred", 6, "k_factor_lchain<136>", 2),
    ("wide4_default_pred", 6, "k_factor_ref_finish", 2),
    ("limited_wide", 1, "k_factor_bigmfma<5, 3, 24>", 2),
    ("wide4_bigmfma", 7, "k_factor_bigmfma<4, 5, 34>", 3),
    ("limited_wide", 2, "k_factor_bigmfma<3, 5, 34>", 3),
    ("wide4_sibling_groups", 7, "k_factor_wide<WG_JT>", 3),
    ("leafwide_edge_ma96_p384", 3, "k_factor<true, MODE_FACTOR>", 2),
    ("mixed_colgroup_big_leaf", 3, "k_factor<true, MODE_FACTOR>", 3),
    ("wide4_generic", 6, "k_factor<true, MODE_FACTOR>", 2),         # force_generic
    ("generic_lds", 0, "k_factor<false, MODE_FACTOR>", 1),          # the LDS generic kernel takes root levels only: errtype 1
    ("limited_wave", 2, "k_marginal_invchol_wave", 2, dict(at=0)),
    ("limited_wide", 1, "k_marginal_invchol", 2, dict(at=0)),
]
A_EXCLUDED = dict(EXCLUDED)      # the instantiations the route table itself never dispatches, and those without a failure site
A_EXCLUDED["k_lchain_scalars"] = "no failure site: it sums the per-row terms k_factor_lchain left (factor_lchain.hpp)"

# ---- sweep: row, level, kind, instantiation, code
SWEEP_CASES = [
    ("ref30_leaf50_pred50", 6, "cached", "k_sample_leaf_seg<4>", 11),
    ("ref30_leaf50_pred50", 5, "cached", "k_sample_lean<true>", 10),
    ("ref30_leaf50_pred50", 5, "rebuild", "k_sample_mfma", 10),
    ("ref30_leaf50_pred50", 6, "rebuild", "k_sample_mfma", 11),
    ("leaf256_cached_mfma", 8, "cached", "k_sample_mfma", 11),
    ("ref25_wch_nkx44", 7, "rebuild", "k_sample_lean<true>", 10),   # behind k_gram_direct
    ("leaf38_pred38_wave", 5, "cached", "k_sample_wave", 10),
    ("leaf44_pred44_leafsweep", 7, "cached", "k_sample_leaf", 11),
    ("seg6_gram_direct", 9, "rebuild", "k_sample_leaf_seg<6>", 11),
    ("seg6_gram_direct", 9, "cached", "k_sample_leaf_seg<6>", 11),
    ("wide4_default_pred", 6, "rebuild", "k_sample<true, false>", 10),
    ("wide4_default_pred", 6, "cached", "k_sample<true, false>", 10),
    ("wide4_default_pred", 7, "rebuild", "k_sample_leaf_wide", 11),
    ("wide4_default_pred", 7, "cached", "k_sample_leaf_wide", 11),
    ("wide4_no_grambig", 7, "rebuild", "k_sample<true, true>", 11),
    ("wide4_leafwide_off", 7, "cached", "k_sample<true, true>", 11),
    ("generic_lds", 3, "rebuild", "k_sample<false>", 11),
    ("generic_lds", 3, "cached", "k_sample<false>", 11),
    ("generic_lds", 0, "cached", "k_sample<false>", 10),            # the root
]
SWEEP_EXCLUDED = {}
SWEEP_KEYS = ("sweep", "rebuild", "cached", "leaf_rebuild", "leaf_cached")
# two failing levels of different kinds: the last reference level (10) and the leaf level (11) -> the shallower one's code
TWO_LEVELS = ("ref30_leaf50_pred50", (5, 6), "cached", ("k_sample_lean<true>", "k_sample_leaf_seg<4>"), 10)


def a_case_id(c):
    return f"{c[0]}-L{c[1]}-{c[2]}".replace(" ", "")


def sweep_case_id(c):
    return f"{c[0]}-L{c[1]}-{c[2]}-{c[3]}".replace(" ", "")


def table_names(keys):
    names = set()
    for row in ROUTES + WIDE_ROUTES:
        for k in keys:
            names.update(row["routes"].get(k, []))
    return names


def test_every_instantiation_of_the_route_tables_is_a_failing_kernel_or_excluded():
    a = table_names(("A",))
    covered = {c[2] for c in A_CASES}
    assert covered | (set(A_EXCLUDED) & a) == a, sorted(a - covered - set(A_EXCLUDED))
    assert not covered & set(A_EXCLUDED)
    s = table_names(SWEEP_KEYS)
    covered = {c[3] for c in SWEEP_CASES}
    assert covered | (set(SWEEP_EXCLUDED) & s) == s, sorted(s - covered - set(SWEEP_EXCLUDED))
    # both kinds of sweep where a row names the instantiation under both
    for key, kind in (("leaf_rebuild", "rebuild"), ("leaf_cached", "cached")):
        for name in table_names((key,)):
            assert any(c[2] == kind and c[3] == name for c in SWEEP_CASES), (kind, name)


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's run of one (problem, level), shared by the cases on it
# ---------------------------------------------------------------------------------------------------------------------
_REF = {}
BETA = np.array([0.3, -0.2, 0.1])


def failure_inputs(pb, level):
    if level == "root":
        # the root's knots of a grid lie too far apart for the inflated cross-covariance to matter (relabelled root rows make
        # level 1 fail instead): a univariate root fails with sigma^2 < 0, finite and outside the bounds, on the row's own problem
        assert pb["q"] == 1
        bad = pb["theta"].copy()
        bad[0] = -1.0
        fp, f = pb, dict(theta_bad=bad, tausq_inv_ok=np.full(1, 5.0), tausq_inv_bad=np.full(1, -1e6), levels=[0],
                         rows=np.zeros(0, dtype=np.int64))
    else:
        fp, f = level_failure_problem(pb, level)
    rng = np.random.default_rng(7)
    f.update(w=rng.standard_normal(pb["n"]), zs=[rng.standard_normal(pb["n"]) for _ in range(3)], theta2=fp["theta"] * 1.03)
    return fp, f


def set_oracle_tausq_inv(om, t):
    om.tausq_inv = np.array(t, dtype=np.float64)
    om.tausq_inv_long = om.tausq_inv[om.mv_id - 1].astype(np.float64)


def construction(row, level, recover=True):
    """The oracle on the relabelled problem of (row, level), no GPU involved: phase A at the valid theta; the failing proposal
    (code, level, the blocks of the levels above); a good sweep; the failing sweep (code, levels); the sweep after tausq^-1 and
    w are restored; the recovery of the proposal slot -- phase A at a valid theta (with the w the device has then: that of the
    sweep with zs[0]), accept_make_change, one sweep (recover=False: without it, and not cached).  The oracle model itself is
    not kept."""
    key = (problem_key(row), level)
    if key in _REF:
        return _REF[key]
    pb = build_problem(row)
    fp, f = failure_inputs(pb, level)
    om = oracle_model(fp, theta=fp["theta"], w=f["w"], beta=BETA, tausq=1.0 / f["tausq_inv_ok"])
    assert om.get_loglik_comps_w(om.param_data)
    ref = dict(fp=fp, f=f, na=om.na_ix_all)
    # (a)
    om.theta_update(om.alter_data, f["theta_bad"])
    ref["a_code"], ref["a_level"] = oracle_phase_a_failure(om, om.alter_data)
    ad = om.alter_data
    above = [int(u) for g in range(ref["a_level"] or 0) for u in om.u_by_block_groups[g]]
    ref["above"] = {u: (ad.w_cond_mean_K[u].copy() if om.parents[u].size else None, ad.Rcc_invchol[u].copy()) for u in above}
    ref["logdet"], ref["loglik"] = ad.logdetCi_comps.copy(), ad.loglik_w_comps.copy()
    # (b): one good sweep first (the oracle's per-row caches start as q x q zeros, which a failing first sweep trips over;
    # nothing a sweep computes depends on an earlier sweep but w)
    om.gibbs_sample_w(f["zs"][0])
    ref["w_sweep0"] = om.w.copy()
    set_oracle_tausq_inv(om, f["tausq_inv_bad"])
    with np.errstate(all="ignore"):
        try:
            om.gibbs_sample_w(f["zs"][1])
        except RuntimeError:
            pass
    ref["s_code"], ref["s_levels"] = om.last_sample_errtype, oracle_sweep_failing_levels(om)
    set_oracle_tausq_inv(om, f["tausq_inv_ok"])
    om.w = f["w"].copy()
    om.gibbs_sample_w(f["zs"][2])
    ref["w_sweep2"] = om.w.copy()
    if not recover:
        return ref
    # the recovery
    om.w = ref["w_sweep0"].copy()
    om.theta_update(om.alter_data, f["theta2"])
    assert om.get_loglik_comps_w(om.alter_data)
    ref["ll_recover"] = om.alter_data.loglik_w
    om.accept_make_change()
    om.gibbs_sample_w(f["zs"][1])
    ref["w_recover"] = om.w.copy()
    _REF[key] = ref
    return ref


def check_construction_a(row, level, code, ref=None):
    ref = ref or construction(ROW[row], level)
    assert (ref["a_code"], ref["a_level"]) == (code, 0 if level == "root" else level), (row, level, ref["a_code"], ref["a_level"])
    return ref


def check_construction_sweep(row, level, code, ref=None):
    ref = ref or construction(ROW[row], level)
    levels = [level] if np.ndim(level) == 0 else sorted(level)
    assert ref["s_code"] == code and ref["s_levels"] == levels, (row, level, ref["s_code"], ref["s_levels"])
    return ref


def set_env(row, monkeypatch):
    for k, v in ROW[row]["env"].items():
        monkeypatch.setenv(k, v)


def handle(row, ref, defer_leaf=True):
    """A device handle on the relabelled problem at its valid theta, with the row's force_generic."""
    from spamtree_amd.model import SpamTreeMV
    pb, f = ref["fp"], ref["f"]
    hm = SpamTreeMV(pb["y"], pb["X"], pb["Z"], pb["coords"], pb["mv_id"], pb["blocking"], pb["gix_block"], pb["res_is_ref"],
                    pb["parents"], pb["children"], pb.get("limited_tree", False), pb["block_names"], pb["block_groups"],
                    pb["indexing"], f["w"], BETA, pb["theta"], 1.0, force_generic=ROW[row].get("force_generic", False),
                    defer_leaf=defer_leaf)
    set_tausq_inv(hm, f["tausq_inv_ok"])
    return hm


def set_tausq_inv(hm, t):
    hm.tausq_inv = np.ascontiguousarray(t, dtype=np.float64)
    assert hm.lib.st_set_tausq_inv(hm.h, hm.tausq_inv.ctypes.data_as(DP)) == 0


def sample_rc(hm, z):
    z = np.ascontiguousarray(z, dtype=np.float64)
    return int(hm.lib.st_sample_w(hm.h, z.ctypes.data_as(DP), 0, 0))


def check_levels_above(hm, ref, slot=1):
    """logdet, loglik, Ri and H of every observed block of the levels above the failing one, against the oracle."""
    ld, ll = hm.comps(slot)
    us = sorted(ref["above"])
    if not us:
        return
    assert relerr(ld[us], ref["logdet"][us]) <= REL and relerr(ll[us], ref["loglik"][us]) <= REL
    for u in us:
        H_ref, Ri_ref = ref["above"][u]
        H, Ri = hm.block(slot, u)
        assert relerr(Ri, Ri_ref) <= REL, u
        if H_ref is not None:
            assert relerr(H, H_ref) <= REL_H, u


def check_accepted_slot_untouched(hm, twin, ref):
    """st_loglik_w(0) and one sweep with a fixed z, bit for bit against a twin that never saw the failure (and the oracle)."""
    assert hm.get_loglik_w(0) == twin.get_loglik_w(0)
    z = ref["f"]["zs"][0]
    hm.deal_with_w(z)
    twin.deal_with_w(z)
    w = hm.get_w().copy()
    assert np.array_equal(w, twin.get_w())
    na = ref["na"]
    assert relerr(w[na], ref["w_sweep0"][na]) <= REL


def check_recovery(hm, ref, factor):
    """The proposal slot at a valid theta (`factor`: how the test factorises it; returns loglik_w), swapped in, swept."""
    ll = factor(ref["f"]["theta2"])
    assert abs(ll - ref["ll_recover"]) <= REL * abs(ref["ll_recover"])
    hm.accept_make_change()
    hm.deal_with_w(ref["f"]["zs"][1])
    na = ref["na"]
    assert relerr(hm.get_w()[na], ref["w_recover"][na]) <= REL


def factor_sync(hm):
    def factor(theta):
        hm.theta_update(1, theta)
        assert hm.get_loglik_comps_w(1)
        return hm.loglik_w[1]
    return factor


# ---------------------------------------------------------------------------------------------------------------------
# 1. phase A, one case per instantiation
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", A_CASES, ids=[a_case_id(c) for c in A_CASES])
def test_phase_a_failure_on_every_instantiation(case, monkeypatch):
    row, level, name, code = case[:4]
    at = case[4]["at"] if len(case) > 4 else level
    check_construction_a(row, level, code)
    ref = construction(ROW[row], level)
    set_env(row, monkeypatch)
    hm, twin = handle(row, ref), handle(row, ref)
    try:
        assert hm.get_loglik_comps_w(0) and twin.get_loglik_comps_w(0)
        hm.theta_update(1, ref["f"]["theta_bad"])
        ok = hm.get_loglik_comps_w(1)
        trace = hm.route_info()["levels"]
        assert name in trace[at]["A"], (row, level, name, trace[at]["A"])          # the failing call ran it on that level
        print(f"phase A  {row:26s} level {level}  {name:40s} code {hm.last_errtype}")
        assert ok is False and hm.last_errtype == code
        check_levels_above(hm, ref)
        check_accepted_slot_untouched(hm, twin, ref)
        check_recovery(hm, ref, factor_sync(hm))
    finally:
        hm.close()
        twin.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. sweep, one case per instantiation and kind
# ---------------------------------------------------------------------------------------------------------------------
def run_sweep_case(row, level, kind, names, code, monkeypatch):
    ref = check_construction_sweep(row, level, code)
    f = ref["f"]
    levels = [level] if np.ndim(level) == 0 else list(level)
    names = [names] if isinstance(names, str) else list(names)
    set_env(row, monkeypatch)
    hm, twin = handle(row, ref), handle(row, ref)
    try:
        assert hm.get_loglik_comps_w(0) and twin.get_loglik_comps_w(0)
        if kind == "cached":         # the sweep that forms the Gram parts succeeds on both
            hm.deal_with_w(f["zs"][0])
            twin.deal_with_w(f["zs"][0])
        set_tausq_inv(hm, f["tausq_inv_bad"])
        rc = sample_rc(hm, f["zs"][1])
        trace = hm.route_info()["levels"]
        for g, name in zip(levels, names):
            assert trace[g]["sweep"] == name, (row, g, name, trace[g])
            print(f"sweep    {row:26s} level {g}  {kind:7s} {name:32s} code {rc}")
        if kind == "cached":
            assert not any(L["gram"] for L in trace), trace
        assert rc == code
        twin.deal_with_w(f["zs"][1])          # the same sweep, succeeding: the twin's caches are in the state hm's claim to be in
        set_tausq_inv(hm, f["tausq_inv_ok"])
        for m in (hm, twin):
            m.set_w(f["w"])
            m.deal_with_w(f["zs"][2])
        w = hm.get_w().copy()
        na = ref["na"]
        assert relerr(w[na], ref["w_sweep2"][na]) <= REL
        assert np.array_equal(w, twin.get_w())
        assert hm.get_loglik_w(0) == twin.get_loglik_w(0)
    finally:
        hm.close()
        twin.close()


@pytest.mark.parametrize("case", SWEEP_CASES, ids=[sweep_case_id(c) for c in SWEEP_CASES])
def test_sweep_failure_on_every_instantiation(case, monkeypatch):
    run_sweep_case(*case, monkeypatch)


def test_sweep_failure_on_two_levels_reports_the_shallower(monkeypatch):
    run_sweep_case(*TWO_LEVELS, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the paths the word travels
# ---------------------------------------------------------------------------------------------------------------------
SMALL = dict(id="small25", side=25, kw=dict(missing=0.1), env={"SPAMTREE_QUAD_MIN": "1"}, routes={})
# SPAMTREE_QUAD_MIN=24: the three reference levels (1, 4 and 16 blocks) stay on k_factor_mfma and run ahead of the leaf level,
# the only one on k_factor_quad
TOPS = dict(id="small40_tops", side=40, kw=dict(missing=0.05), env={"SPAMTREE_QUAD_MIN": "24", "SPAMTREE_ASYNC_TOP": "1"}, routes={})
ROW[SMALL["id"]] = SMALL
ROW[TOPS["id"]] = TOPS


def n_levels(row):
    pb = build_problem(ROW[row])
    labels = np.unique(pb["block_groups"])
    return sum(any(np.isfinite(pb["y"][pb["indexing"][u]]).any() for u in range(len(pb["indexing"]))
                   if pb["block_groups"][u] == lab) for lab in labels)


def enqueue_finish(hm, theta):
    th = np.ascontiguousarray(theta, dtype=np.float64)
    assert hm.lib.st_factor_enqueue(hm.h, 1, th.ctypes.data_as(DP), th.size) == 0
    ll = C.c_double()
    rc = hm.lib.st_factor_finish(hm.h, C.byref(ll))
    hm.theta[1] = th.copy()
    hm.loglik_w[1] = ll.value
    return rc, ll.value


@pytest.mark.parametrize("defer", [True, False], ids=["defer_leaf", "no_defer"])
@pytest.mark.parametrize("which,code", [("leaf", 3), ("ref", 2)])
def test_failure_through_factor_enqueue_and_finish(which, code, defer, monkeypatch):
    """A proposal enqueued on slot 1 (its quad leaf level factorised without T when the deferral is on: the flag comes from the
    V-only pass, factor_quad.hpp) fails in _finish with the oracle's code either way; slot 0 is untouched; a valid proposal
    enqueued, finished, swapped in and swept matches the oracle."""
    row = SMALL["id"]
    level = n_levels(row) - (1 if which == "leaf" else 2)
    check_construction_a(row, level, code)
    ref = construction(ROW[row], level)
    set_env(row, monkeypatch)
    hm, twin = handle(row, ref, defer_leaf=defer), handle(row, ref, defer_leaf=defer)
    try:
        assert hm.get_loglik_comps_w(0) and twin.get_loglik_comps_w(0)
        rc, _ = enqueue_finish(hm, ref["f"]["theta_bad"])
        trace = hm.route_info()["levels"]
        assert trace[-1]["A"] == [quad(32, False, True)], trace[-1]       # the leaf level the deferral applies to
        assert trace[level]["A"] == [quad(32, which == "ref", True)], (level, trace[level])
        print(f"enqueue  {row:26s} level {level}  {trace[level]['A'][0]:40s} code {rc}  defer {defer}")
        assert rc == code
        check_accepted_slot_untouched(hm, twin, ref)

        def factor(theta):
            rc2, ll = enqueue_finish(hm, theta)
            assert rc2 == 0
            return ll
        check_recovery(hm, ref, factor)
    finally:
        hm.close()
        twin.close()


def begin_then_factor(hm, theta_begin, theta):
    tb = np.ascontiguousarray(theta_begin, dtype=np.float64)
    th = np.ascontiguousarray(theta, dtype=np.float64)
    assert hm.lib.st_factor_begin(hm.h, 1, tb.ctypes.data_as(DP), tb.size) == 0
    ll = C.c_double()
    rc = hm.lib.st_factor(hm.h, 1, th.ctypes.data_as(DP), th.size, C.byref(ll))
    return rc, ll.value


@pytest.mark.parametrize("which", ["root", "top", "below", "stale"])
def test_failure_of_levels_run_ahead_reaches_the_caller(which, monkeypatch):
    """st_factor_begin runs the top levels (those ahead of the first k_factor_quad level) on a second stream with a failure
    word of its own; k_merge_err folds it into the main one.  root / top: a failure in a level that ran ahead (errtype 1 /
    2: the last reference level, so that a lost second-stream word shows as the leaf level's 3); below: a failure under
    successful top levels keeps its own code; stale: a st_factor_begin at a failing theta followed by st_factor at another,
    valid theta succeeds with the oracle's value."""
    row = TOPS["id"]
    set_env(row, monkeypatch)
    nl = n_levels(row)
    level, code = {"root": (0, 1), "top": (2, 2), "below": (nl - 1, 3), "stale": (2, 2)}[which]
    key = "root" if which == "root" else level
    check_construction_a(row, key, code)
    ref = construction(ROW[row], key)
    hm = handle(row, ref)
    try:
        g_top = hm.lib.st_factor_ahead_levels(hm.h)
        assert g_top == 3 and nl == 4, (g_top, nl)       # the three reference levels run ahead of the leaf level
        assert hm.get_loglik_comps_w(0)
        bad, ok = ref["f"]["theta_bad"], ref["f"]["theta2"]
        if which == "stale":
            hm.deal_with_w(ref["f"]["zs"][0])            # (the w the oracle's recovery run has)
            rc, ll = begin_then_factor(hm, bad, ok)
            print(f"begin    {row:26s} level {level}  stale word, valid theta: code {rc}")
            assert rc == 0 and abs(ll - ref["ll_recover"]) <= REL * abs(ref["ll_recover"])
            return
        rc, _ = begin_then_factor(hm, bad, bad)
        print(f"begin    {row:26s} level {level}  {hm.route_info()['levels'][level]['A'][0]:40s} code {rc}  (g_top {g_top})")
        assert (level < g_top) == (which != "below")
        assert rc == code
        check_levels_above(hm, ref)
        hm.deal_with_w(ref["f"]["zs"][0])
        rc, ll = begin_then_factor(hm, ok, ok)
        assert rc == 0 and abs(ll - ref["ll_recover"]) <= REL * abs(ref["ll_recover"])
    finally:
        hm.close()


@pytest.mark.parametrize("which,code", [("leaf", 11), ("ref", 10)])
def test_sweep_failure_through_sample_w_loglik_and_its_halves(which, code, monkeypatch):
    row = SMALL["id"]
    level = n_levels(row) - (1 if which == "leaf" else 2)
    ref = check_construction_sweep(row, level, code)
    f = ref["f"]
    set_env(row, monkeypatch)
    hm = handle(row, ref)
    try:
        assert hm.get_loglik_comps_w(0)
        hm.deal_with_w(f["zs"][0])
        lib, h = hm.lib, hm.h
        z = np.ascontiguousarray(f["zs"][1])
        zp = z.ctypes.data_as(DP)
        set_tausq_inv(hm, f["tausq_inv_bad"])
        ll = C.c_double()
        rcs = [sample_rc(hm, z)]
        hm.set_w(f["w"])
        rcs.append(lib.st_sample_w_loglik(h, zp, 0, 0, 0, C.byref(ll)))
        hm.set_w(f["w"])
        assert lib.st_sample_w_loglik_begin(h, zp, 0, 0, 0) == 0
        rcs.append(lib.st_sample_w_loglik_end(h, C.byref(ll)))
        print(f"loglik   {row:26s} level {level}  st_sample_w / _loglik / _begin+_end: codes {rcs}")
        assert rcs == [code] * 3
        set_tausq_inv(hm, f["tausq_inv_ok"])
        hm.set_w(f["w"])
        assert lib.st_sample_w_loglik(h, f["zs"][2].ctypes.data_as(DP), 0, 0, 0, C.byref(ll)) == 0
        na = ref["na"]
        assert relerr(hm.get_w()[na], ref["w_sweep2"][na]) <= REL
    finally:
        hm.close()


@pytest.mark.parametrize("which,a_code,s_code", [("leaf", 3, 11), ("ref", 2, 10)])
def test_failures_through_a_one_rank_communicator(which, a_code, s_code, monkeypatch):
    """With a communicator attached st_factor and st_sample_w take the exchange protocol (k_pack_comps + st_mg_finish, the
    all-gather of w with its failure word, the fused st_sample_w_loglik): the same codes as without."""
    from spamtree_amd import fit
    row = SMALL["id"]
    level = n_levels(row) - (1 if which == "leaf" else 2)
    check_construction_a(row, level, a_code)
    ref = check_construction_sweep(row, level, s_code)
    ref = construction(ROW[row], level)
    f = ref["f"]
    set_env(row, monkeypatch)
    hm = handle(row, ref)
    try:
        buf = C.create_string_buffer(bytes(fit.make_unique_id()), 128)
        assert hm.lib.st_comm_init(hm.h, C.cast(buf, C.c_void_p)) == 0
        assert hm.get_loglik_comps_w(0)
        hm.theta_update(1, f["theta_bad"])
        ok = hm.get_loglik_comps_w(1)
        print(f"comm     {row:26s} level {level}  phase A code {hm.last_errtype}")
        assert ok is False and hm.last_errtype == a_code
        check_levels_above(hm, ref)
        hm.deal_with_w(f["zs"][0])
        na = ref["na"]
        assert relerr(hm.get_w()[na], ref["w_sweep0"][na]) <= REL
        set_tausq_inv(hm, f["tausq_inv_bad"])
        z = np.ascontiguousarray(f["zs"][1])
        ll = C.c_double()
        rcs = [sample_rc(hm, z)]
        hm.set_w(f["w"])
        rcs.append(hm.lib.st_sample_w_loglik(hm.h, z.ctypes.data_as(DP), 0, 0, 0, C.byref(ll)))
        print(f"comm     {row:26s} level {level}  st_sample_w / st_sample_w_loglik: codes {rcs}")
        assert rcs == [s_code] * 2
        set_tausq_inv(hm, f["tausq_inv_ok"])
        hm.set_w(f["w"])
        hm.deal_with_w(f["zs"][2])
        assert relerr(hm.get_w()[na], ref["w_sweep2"][na]) <= REL
    finally:
        hm.close()
