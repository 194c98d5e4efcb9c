"""GPU: hand-built trees the tree builder never produces (tests/tree_mutations.py), on every route.

Every other GPU test takes its tree from topology.prepare: regular trees in which the blocks of a level share one chain
length, every last parent sits on the previous reference level, sibling widths differ by a few rows and no block is empty.
st_create accepts far more (include/spamtree_hip.h, st_problem), and the layout and the kernels carry per-block logic for it:
a caller who builds its own DAG reaches that at once.  The shapes here put two different values of J, P and m inside one
level; tests/test_tree_mutations_cpu.py shows that the references hold on them and which layout structures they reach.

  * every shape and route row: tests/test_gpu_routes.run_device and compare_with_oracle, unchanged (REL = 1e-9, H 1e-8) --
    phase A on both slots, H / Ri of every observed block, three sweeps with log-density components and beta / tausq
    statistics, st_predict, an accepted theta, a rebuild sweep and a cached sweep, st_predict again -- after the row has
    shown through st_route_info that it reached the kernel family it is there for;
  * without the oracle, on the same rows: loglik_w of phases A and C against the dense DAG density, and the z = 0 sweep mean
    of every block of the deepest level against the dense posterior precision Q + I / tausq (1e-8, as
    tests/test_gpu_reference_math.py); the deepest level is sampled first, so the exact full conditional holds for it
    whatever the tree;
  * bit for bit, two handles on one problem: k_gram_direct against k_gram, one quad unit per workgroup against four, the
    deferred leaf completion against the full factorisation;
  * st_simulate against the restated prior sweep; the slots of an emptied block.
"""
import ctypes as C

import numpy as np
import pytest

from tests import tree_mutations as tm
from tests.prior_sweep import prior_sweep
from tests.test_gpu_routes import (_ORACLE, NO_LCHAIN, QUAD_MIN, REL, REL_H, check_routes, compare_with_oracle, hip_model, inputs,
                                   oracle_protocol, relerr, run_device)
from tests.test_tree_mutations_cpu import dense_loglik
from tests.test_oracle_identities import dense_precision
from tests.util import oracle_model

pytestmark = pytest.mark.gpu
REL_DENSE = 1e-8
SPLIT = {"SPAMTREE_SPLIT_GRAM": "2"}      # k_gram / k_gram_direct on every column-group level (default: the big ones only)
ANY_QUAD = "k_factor_quad<"               # a prefix: any instantiation
# k_factor_quad on oracle-size levels, and up to four units per workgroup: by default a level of at most 2 x CUs groups takes
# one unit per workgroup, and the breaks of a quad on the chain length and on the shared chain would decide nothing
# (tests/test_tree_mutations_cpu.py shows from the layout that these rows have quads of several units)
QUAD4 = dict(QUAD_MIN, SPAMTREE_QUAD_UNITS="4")
OBSERVED = {}                             # quantity -> the largest error met


def note(name, err):
    OBSERVED[name] = max(OBSERVED.get(name, 0.0), float(err))


def row(shape, tag, env=None, generic=False, routes=None, not_routes=None):
    return dict(id=f"{shape}-{tag}", shape=shape, env=env or {}, force_generic=generic, routes=routes or {}, not_routes=not_routes or {})


COLUMN_GROUP = ("mixed_chain_leaf", "mixed_chain_ref", "uneven_widths", "empty_and_childless", "empty_all_observed", "many_children_5",
                "many_children_4", "na_blocks_rehung")
HAS_PRED = ("empty_and_childless", "na_blocks_rehung")
NO_DIRECT = ("mixed_chain_leaf", "many_children_5")     # the shapes k_gram_direct must not take
ROWS = []
for s in COLUMN_GROUP:
    pred = {"P": [ANY_QUAD]} if s in HAS_PRED else {}
    ROWS.append(row(s, "default", routes={"A": ["k_factor_mfma"]}))
    ROWS.append(row(s, "quad_min_units4", env=QUAD4, routes=dict({"A": [ANY_QUAD]}, **pred)))
    ROWS.append(row(s, "generic", generic=True, routes=dict({"A": ["k_factor<true, MODE_FACTOR>"]},
                                                            **({"P": ["k_factor<true, MODE_PREDICT>"]} if s in HAS_PRED else {}))))
for s in NO_DIRECT:
    ROWS.append(row(s, "split_gram", env=SPLIT, routes={"gram": ["k_gram"]}, not_routes={"gram": ["k_gram_direct"]}))
for s in ("many_children_4", "uneven_widths"):
    ROWS.append(row(s, "split_gram", env=SPLIT, routes={"gram": ["k_gram", "k_gram_direct"]}))
LCHAIN_REF = ["k_factor_lchain<96>", "k_factor_ref_finish"]
ROWS += [
    # reference blocks of 1 and 45 rows: that level and the leaf level behind it on k_factor_lchain, the levels above on the
    # column groups
    row("one_row_and_wide", "default", routes={"A": ["k_factor_mfma"] + LCHAIN_REF}),
    row("one_row_and_wide", "quad_min_units4", env=QUAD4, routes={"A": [ANY_QUAD] + LCHAIN_REF}),
    row("one_row_and_wide", "generic", generic=True, routes={"A": ["k_factor<true, MODE_FACTOR>"]}),
    row("wide_mixed", "default", routes={"A": LCHAIN_REF}),
    row("wide_mixed", "wide2", env={"SPAMTREE_WIDE": "2"}, routes={"A": ["k_factor_wide<WG_JT>"]}),
    row("wide_mixed", "no_lchain", env=NO_LCHAIN, routes={"A": ["k_factor_bigmfma<"]}, not_routes={"A": ["k_factor_lchain<"]}),
    row("wide_mixed", "no_lchain_wide2", env=dict(NO_LCHAIN, SPAMTREE_WIDE="2"), routes={"A": ["k_factor_wide<WG_JT>"]}),
    row("wide_mixed", "generic", generic=True, routes={"A": ["k_factor<true, MODE_FACTOR>"]}),
    row("two_outcomes_mixed", "default", routes={"A": ["k_factor_lchain<96>"]}),
    row("two_outcomes_mixed", "no_lchain", env=NO_LCHAIN, routes={"A": ["k_factor_bigmfma<"]}),
    row("two_outcomes_mixed", "generic", generic=True, routes={"A": ["k_factor<true, MODE_FACTOR>"]}),
    row("limited_skip", "default", routes={"A": ["k_marginal_invchol_wave"]}),
]


def split_prefixes(names):
    """The kernel names of a row, per route key: (full names, prefixes); a name that ends in '<' is a prefix."""
    exact = {k: [n for n in v if not n.endswith("<")] for k, v in names.items()}
    prefix = {k: [n for n in v if n.endswith("<")] for k, v in names.items()}
    return exact, prefix


def check_row_routes(r, routes):
    """check_routes of tests/test_gpu_routes; a prefix stands for any instantiation of that kernel."""
    exact, prefix = split_prefixes(r["routes"])
    nexact, nprefix = split_prefixes(r["not_routes"])
    check_routes(dict(id=r["id"], routes=exact, not_routes=nexact), routes)
    for key, names in prefix.items():
        for n in names:
            assert any(x.startswith(n) for x in routes[key]), (r["id"], key, n, sorted(routes[key]))
    for key, names in nprefix.items():
        for n in names:
            assert not any(x.startswith(n) for x in routes[key]), (r["id"], key, n, sorted(routes[key]))


def oracle_ref(name, pb, inp):
    key = "handbuilt:" + name
    if key not in _ORACLE:
        _ORACLE[key] = oracle_protocol(pb, inp)
    return key, _ORACLE[key]


@pytest.mark.parametrize("r", ROWS, ids=[r["id"] for r in ROWS])
def test_shape_matches_oracle_on_the_route(r, monkeypatch):
    for k, v in r["env"].items():
        monkeypatch.setenv(k, v)
    pb = tm.shape(r["shape"])
    inp = inputs(pb)
    out = run_device(pb, inp, force_generic=r["force_generic"])
    print(r["id"], {k: sorted(v) for k, v in out["routes"].items()}, [L["kernel"] for L in out["levels"]])
    check_row_routes(r, out["routes"])
    if r["shape"] == "one_row_and_wide" and not r["force_generic"]:     # the level of 1- and 45-row blocks, and the leaves behind it
        assert [L["kernel"] for L in out["levels"]][2:] == ["k_factor_lchain+ref_finish", "k_factor_lchain"], out["levels"]
        assert out["levels"][2]["max_m"] == 45
    key, _ = oracle_ref(r["shape"], pb, inp)
    try:
        compare_with_oracle(pb, inp, out, key=key, record=OBSERVED)
    finally:
        print(r["id"], {k2: f"{v:.2e}" for k2, v in OBSERVED.items()})


# ---- without the oracle
@pytest.mark.parametrize("r", ROWS, ids=[r["id"] for r in ROWS])
def test_shape_matches_the_dense_identities(r, monkeypatch):
    """loglik_w of phase A and of phase C against the dense DAG density; the z = 0 draw of every block of the
    deepest observed level, the blocks that hang from a shallower level included, against its exact full conditional mean
    under the dense posterior precision (the method of test_hip_block_draw_is_exact_full_conditional)."""
    for k, v in r["env"].items():
        monkeypatch.setenv(k, v)
    pb = tm.shape(r["shape"])
    inp = inputs(pb)
    n, tausq = pb["n"], inp["tausq"]
    hm = hip_model(pb, force_generic=r["force_generic"], **inp)
    assert hm.get_loglik_comps_w(0)
    exact = dense_loglik(pb, pb["theta"], inp["w"])
    e_a = abs(hm.loglik_w[0] - exact) / abs(exact)
    e_c = abs(hm.get_loglik_w(0) - exact) / abs(exact)
    hm.deal_with_w(np.zeros(n))
    w1 = hm.get_w()
    hm.close()
    obs_blocks = [u for u in range(tm.n_blocks(pb)) if tm.n_observed(pb, u) > 0]
    in_density = np.zeros(n, dtype=bool)
    in_density[np.concatenate([pb["indexing"][u] for u in obs_blocks])] = True
    # prediction blocks are not part of the density the sampler targets: they enter Q without rows
    sub = dict(pb, indexing=[ix if tm.n_observed(pb, u) > 0 else ix[:0] for u, ix in enumerate(pb["indexing"])])
    Q, _ = dense_precision(sub, pb["theta"])
    seen = np.isfinite(pb["y"])
    Qpost = Q + np.diag(seen / tausq)
    b = np.where(seen, (np.nan_to_num(pb["y"]) - pb["X"] @ inp["beta"]) / tausq, 0.0)
    g = tm.leaf_level(pb)
    deepest = [u for u in tm.blocks_of_level(pb, g) if tm.n_observed(pb, u) > 0]
    assert len(set(len(pb["parents"][u]) for u in deepest)) > 1 or "mixed" not in r["shape"]
    e_m = 0.0
    for u in deepest:
        iu = pb["indexing"][u]
        rest = np.setdiff1d(np.arange(n), iu)
        S = Qpost[np.ix_(iu, iu)]
        if not tm.is_reference_level(pb, u):
            assert np.abs(S - np.diag(np.diag(S))).max() == 0.0
        mean = np.linalg.solve(S, b[iu] - Qpost[np.ix_(iu, rest)] @ np.where(in_density, inp["w"], 0.0)[rest])
        e_m = max(e_m, np.abs(w1[iu] - mean).max() / max(1.0, np.abs(mean).max()))
    note("dense: loglik_w phase A", e_a)
    note("dense: loglik_w phase C", e_c)
    note("dense: z = 0 mean of the deepest level", e_m)
    print(r["id"], f"dense: A {e_a:.2e} C {e_c:.2e} mean {e_m:.2e}")
    assert e_a <= REL_DENSE and e_c <= REL_DENSE and e_m <= REL_DENSE, (e_a, e_c, e_m)


# ---- bit for bit, two handles on one problem
BITWISE_KEYS = ("loglik_A", "ws", "lls", "ll_comps", "xty", "ssq")


def same_bits(a, b, blocks=True):
    for k in BITWISE_KEYS:
        assert np.array_equal(np.array(a[k]), np.array(b[k])), k
    for slot in (0, 1):
        assert np.array_equal(a["comps"][slot][0], b["comps"][slot][0]) and np.array_equal(a["comps"][slot][1], b["comps"][slot][1]), slot
        for u in a["blocks"][slot] if blocks else ():
            for x, y in zip(a["blocks"][slot][u], b["blocks"][slot][u]):
                assert np.array_equal(x, y), (slot, u)


@pytest.mark.parametrize("name", ["uneven_widths", "many_children_4"])
def test_direct_gram_is_bit_identical_on_hand_built_trees(name, monkeypatch):
    """SPAMTREE_GRAM_DIRECT=1 against 0 over the whole protocol, as tests/test_gpu_parity.py has it for builder trees: here
    with reference blocks of 1 to 32 rows and leaf groups of exactly 32 columns, and with the most child groups the kernel
    takes."""
    monkeypatch.setenv("SPAMTREE_SPLIT_GRAM", "2")
    pb = tm.shape(name)
    inp = inputs(pb)
    outs = []
    for direct in ("1", "0"):
        monkeypatch.setenv("SPAMTREE_GRAM_DIRECT", direct)
        outs.append(run_device(pb, inp))
    assert "k_gram_direct" in outs[0]["routes"]["gram"] and "k_gram_direct" not in outs[1]["routes"]["gram"]
    assert "k_gram" in outs[1]["routes"]["gram"]
    same_bits(outs[0], outs[1])


def test_quad_units_do_not_change_a_unit_on_mixed_chains(monkeypatch):
    """SPAMTREE_QUAD_UNITS=4 (up to four units per workgroup; the default at this size is one) against 1 on
    mixed_chain_ref: a unit's arithmetic does not depend on which cousins share its workgroup, also where a level's quads
    break on the chain length.  (The layout rows of tests/test_tree_mutations_cpu.py: 36 quads of one unit, 11 of up to four.)"""
    for k, v in QUAD4.items():
        monkeypatch.setenv(k, v)
    pb = tm.shape("mixed_chain_ref")
    inp = inputs(pb)
    four = run_device(pb, inp)
    monkeypatch.setenv("SPAMTREE_QUAD_UNITS", "1")
    one = run_device(pb, inp)
    assert any(x.startswith(ANY_QUAD) for x in four["routes"]["A"]) and any(x.startswith(ANY_QUAD) for x in one["routes"]["A"])
    same_bits(four, one)


def test_deferred_leaf_completion_gives_identical_panels(monkeypatch):
    """st_options.reserved bit 2 set (a proposal's quad leaf level factorised in full) against clear (its panels finished
    from the stored V by the first reader, here st_swap) on mixed_chain_leaf, with quads of up to four units: identical
    panels, components and draws.  Only st_factor_enqueue on slot 1 defers (the synchronous st_factor never does), so the
    proposal goes through st_factor_enqueue + st_factor_finish, as in tests/test_gpu_leaf_deferral.py."""
    from spamtree_amd.model import SpamTreeMV
    from tests.test_gpu_leaf_deferral import enqueue
    for k, v in QUAD4.items():
        monkeypatch.setenv(k, v)
    pb = tm.shape("mixed_chain_leaf")
    inp = inputs(pb)
    g = tm.leaf_level(pb)
    leaves = [u for u in tm.blocks_of_level(pb, g) if tm.n_observed(pb, u) > 0]
    got = []
    for defer in (True, False):
        hm = SpamTreeMV(pb["y"], pb["X"], pb["Z"], pb["coords"], pb["mv_id"], pb["blocking"], pb["gix_block"], pb["res_is_ref"],
                        pb["parents"], pb["children"], False, pb["block_names"], pb["block_groups"], pb["indexing"], inp["w"],
                        inp["beta"], inp["theta"], 1.0 / inp["tausq"], defer_leaf=defer)
        assert hm.get_loglik_comps_w(0)
        assert hm.lib.st_factor_is_async(hm.h) == 1       # one GPU, no communicator: the enqueue is the deferring one
        hm.theta_update(1, inp["theta2"])
        hm.loglik_w[1] = enqueue(hm, 1, inp["theta2"])
        # the leaf level ran the leaf instantiation of k_factor_quad (the deferrable one), on both handles
        leaf_routes = hm.route_info()["levels"][g]["A"]
        assert leaf_routes and all(x.startswith(ANY_QUAD) and x.endswith("false, true>") for x in leaf_routes), leaf_routes
        res = dict(ll=list(hm.loglik_w), comps=hm.comps(1))
        hm.accept_make_change()
        res["panels"] = [hm.block(0, u, raw=True) for u in leaves]
        hm.deal_with_w(inp["zs"][0])
        res["w"] = hm.get_w().copy()
        res["ll_c"] = hm.get_loglik_w(0)
        got.append(res)
        hm.close()
    a, b = got
    assert a["ll"] == b["ll"] and a["ll_c"] == b["ll_c"] and np.array_equal(a["w"], b["w"])
    assert np.array_equal(a["comps"][0], b["comps"][0]) and np.array_equal(a["comps"][1], b["comps"][1])
    for (Na, Ra), (Nb, Rb) in zip(a["panels"], b["panels"]):
        assert np.array_equal(Na, Nb) and np.array_equal(Ra, Rb)
    # and the panels are the oracle's at theta2 (the accepted slot)
    _, ref = oracle_ref("mixed_chain_leaf", pb, inp)
    for u, (N, Ri) in zip(leaves, a["panels"]):
        H_ref, Ri_ref = ref["slots"][1]["blocks"][u]
        assert relerr(-N / Ri[:, None], H_ref) <= REL_H and relerr(Ri, Ri_ref) <= REL, u


# ---- st_simulate
@pytest.mark.parametrize("name", ["mixed_chain_leaf", "empty_and_childless", "wide_mixed"])
def test_simulate_matches_the_restated_sweep(name):
    """Caller normals against tests/prior_sweep.prior_sweep (the reference function and the 1e-10 of
    test_caller_normals_match_the_restated_sweep_and_reach_every_route).  st_simulate takes trees without NA rows only:
    empty_and_childless is refused by name, and its variant with every row observed (the emptied block and two bare
    reference blocks) is what is drawn from."""
    from spamtree_amd.model import SpamTreeError
    from tests.test_gpu_simulate import hip_model as sim_model, rel
    pb = tm.shape(name)
    n = pb["n"]
    rng = np.random.default_rng(1)
    z, eps = rng.standard_normal((n, 3)), rng.standard_normal((n, 3))
    if name == "empty_and_childless":
        hm = sim_model(pb)
        with pytest.raises(SpamTreeError, match="st_simulate: the tree has NA rows"):
            hm.simulate(3, z=z, eps=eps)
        hm.close()
        pb = tm.shape("empty_all_observed")
        assert len(pb["indexing"][pb["emptied"]]) == 0 and np.all(np.isfinite(pb["y"]))
    om = oracle_model(pb)
    assert om.get_loglik_comps_w(om.param_data)
    hm = sim_model(pb)
    w, y = hm.simulate(3, z=z, eps=eps)
    hm.close()
    wr = prior_sweep(om, z)
    yr = (pb["X"] @ pb["beta_true"])[:, None] + wr + np.sqrt(0.2) * eps
    e_w, e_y = rel(w, wr), rel(y, yr)
    note("st_simulate w", e_w)
    note("st_simulate y", e_y)
    print(name, f"simulate: w {e_w:.2e} y {e_y:.2e}")
    assert e_w <= 1e-10 and e_y <= 1e-10, (e_w, e_y)


# ---- the slots of an emptied block
def test_an_emptied_block_has_no_cache_and_zero_components():
    """include/spamtree_hip.h, st_get_block / st_get_comps: a block without an observed row (an empty one included) has no
    cache -- st_get_block refuses it by name -- and its entries of st_get_comps are zero."""
    from spamtree_amd.model import SpamTreeError
    pb = tm.shape("empty_and_childless")
    inp = inputs(pb)
    u = pb["emptied"]
    hm = hip_model(pb, **inp)
    assert hm.get_loglik_comps_w(0)
    m, P = C.c_int64(-1), C.c_int64(-1)
    isref, nobs = C.c_int32(-1), C.c_int32(-1)
    assert hm.lib.st_block_dims(hm.h, u, C.byref(m), C.byref(P), C.byref(isref), C.byref(nobs)) == 0
    assert (m.value, isref.value, nobs.value) == (0, 0, 0) and P.value == sum(len(pb["indexing"][a]) for a in pb["parents"][u])
    with pytest.raises(SpamTreeError, match="block has no observations, hence no cache"):
        hm.block(0, u)
    hm.deal_with_w(inp["zs"][0])
    hm.get_loglik_w(0)
    ld, ll = hm.comps(0)
    unobserved = [v for v in range(tm.n_blocks(pb)) if tm.n_observed(pb, v) == 0]
    assert u in unobserved and np.all(ld[unobserved] == 0.0) and np.all(ll[unobserved] == 0.0)
    assert np.all(ld[[v for v in range(tm.n_blocks(pb)) if v not in unobserved]] != 0.0)
    hm.close()


def test_zz_report_the_largest_observed_error():
    """Prints the largest error the tests above met, per compared quantity (DESIGN.md section 5 records them)."""
    for k in sorted(OBSERVED):
        print(f"largest observed: {k}: {OBSERVED[k]:.3g}")
    oracle = [v for k, v in OBSERVED.items() if not k.startswith(("dense", "st_simulate")) and k != "H"]
    assert all(v <= REL for v in oracle) and OBSERVED.get("H", 0.0) <= REL_H
    assert all(v <= REL_DENSE for k, v in OBSERVED.items() if k.startswith("dense"))
