"""CPU: the protocol model of tests/protocol_model.py -- the generator is a function of its seed, emits only operations the
model classifies, and the committed (tree, seed) list meets the coverage condition; the oracle executor is deterministic and its
phase-A failure codes are the oracle's own.  tests/test_gpu_protocol_sequences.py replays the same sequences on the library."""
import numpy as np
import pytest

from tests import protocol_model as pm
from tests.util import oracle_model, oracle_phase_a_failure


def committed():
    return [(pm.TREES[t]["has_ahead"], pm.sequence(t, s)) for t, s in pm.cases()]


def test_generator_is_a_function_of_the_seed_and_every_operation_is_classified():
    n_ops = n_refused = 0
    for tree, seed in pm.cases():
        has_ahead = pm.TREES[tree]["has_ahead"]
        ops = pm.sequence(tree, seed)
        assert ops == pm.sequence(tree, seed) and ops == pm.generate(seed, has_ahead)
        assert 36 <= len(ops) <= 60, (tree, seed, len(ops))
        assert ops[0] == pm.Op("factor", slot=0, tid=0)
        m = pm.Model(has_ahead)
        for i, op in enumerate(ops):
            cls = m.classify(op)
            assert cls in (pm.LEGAL, pm.FAILS, pm.REFUSED), (tree, seed, i, pm.show(op), cls, m.flags())
            n_ops += 1
            n_refused += cls == pm.REFUSED
            if cls != pm.REFUSED:
                m.apply(op)
        assert m.open is None and m.pending is None      # nothing is left open at the end of a sequence
    assert pm.generate(3, True) != pm.generate(4, True)
    frac = n_refused / n_ops
    print(f"{len(pm.cases())} sequences, {n_ops} operations, {n_refused} refused ({frac:.3f})")
    assert 1 / 12 <= frac <= 1 / 5            # "roughly one in eight"


def test_the_model_keeps_legal_what_the_driver_issues():
    """step_w_theta and draw_tausq_beta of spamtree_fit.cpp: st_factor_begin, st_sample_w_loglik_begin, st_factor_enqueue, the
    statistics and the two setters, st_factor_finish, st_sample_w_loglik_end, st_swap, st_predict -- on an accepted and on a
    failing proposal -- and the SPAMTREE_DEFER_SYNC=0 / SPAMTREE_EARLY_BETA=0 orders."""
    O = pm.Op
    for has_ahead in (True, False):
        for tid in (7, pm.BAD):
            m = pm.Model(has_ahead)
            tail = [O("swap")] if tid != pm.BAD else []
            it = [O("begin", slot=1, tid=tid), O("sweep_begin", slot=0, key=1), O("enqueue", slot=1, tid=tid), O("tausq_stats"),
                  O("set_tausq", key=2), O("beta_stats"), O("set_beta", key=3), O("finish"), O("sweep_end")] + tail + [O("predict")]
            plain = [O("begin", slot=1, tid=tid), O("sweep_begin", slot=0, key=4), O("sweep_end"), O("factor", slot=1, tid=tid)] + tail + \
                    [O("predict"), O("tausq_stats"), O("set_tausq", key=5), O("beta_stats"), O("set_beta", key=6), O("get_w"), O("yhat", key=7)]
            deferred = [O("sweep_begin", slot=0, key=8), O("factor", slot=1, tid=tid), O("sweep_end")]
            for op in [O("factor", slot=0, tid=0)] + it + plain + deferred + it:
                cls = m.classify(op)
                want = pm.FAILS if tid == pm.BAD and op.name in ("finish", "factor") and op.slot != 0 else pm.LEGAL
                assert cls == want, (pm.show(op), cls, m.flags())
                m.apply(op)


def test_the_model_refuses_what_the_header_forbids():
    O = pm.Op
    m = pm.Model(True)
    for op in (O("factor", slot=0, tid=0), O("factor", slot=1, tid=1), O("sample", key=1), O("enqueue", slot=1, tid=2)):
        m.apply(op)
    for op in (O("swap"), O("sample", key=2), O("sample_ll", slot=0, key=2), O("sweep_begin", slot=0, key=2), O("predict"), O("factor", slot=0, tid=3),
               O("factor", slot=1, tid=3), O("begin", slot=1, tid=3), O("enqueue", slot=1, tid=3), O("get_block", slot=1, u="root"),
               O("get_comps", slot=1), O("loglik", slot=1)):
        assert m.classify(op) == pm.REFUSED, pm.show(op)
    for op in (O("get_block", slot=0, u="leaf"), O("get_comps", slot=0), O("loglik", slot=0), O("set_w", key=3), O("get_w"), O("yhat", key=4),
               O("get_resid"), O("finish")):
        assert m.classify(op) == pm.LEGAL, pm.show(op)
    m.apply(O("finish"))
    m.apply(O("sweep_begin", slot=0, key=5))
    for op in (O("sample", key=6), O("sample_ll", slot=0, key=6), O("sweep_begin", slot=1, key=6), O("set_w", key=7), O("get_w"), O("predict"),
               O("yhat", key=8), O("swap"), O("loglik", slot=0), O("loglik", slot=1)):
        assert m.classify(op) == pm.REFUSED, pm.show(op)
    for op in (O("enqueue", slot=1, tid=4), O("factor", slot=1, tid=4), O("begin", slot=1, tid=4), O("beta_stats"), O("set_beta", key=9),
               O("get_comps", slot=1), O("get_block", slot=0, u="root"), O("get_resid"), O("sweep_end")):
        assert m.classify(op) == pm.LEGAL, pm.show(op)
    # levels ahead of time: the swap is refused, the slot is no theta's until it is factorised
    m.apply(O("sweep_end"))
    m.apply(O("begin", slot=1, tid=5))
    assert m.classify(O("swap")) == pm.REFUSED
    assert m.classify(O("get_comps", slot=1)) == pm.UNSPECIFIED and m.classify(O("get_resid")) == pm.UNSPECIFIED
    m.apply(O("factor", slot=0, tid=6))                 # another slot: the result is dropped, slot 1 stays unreadable
    assert m.top is None and m.classify(O("swap")) == pm.UNSPECIFIED
    m.apply(O("factor", slot=1, tid=pm.BAD))
    assert m.classify(O("swap")) == pm.UNSPECIFIED and m.classify(O("loglik", slot=1)) == pm.UNSPECIFIED
    m.apply(O("factor", slot=1, tid=5))
    assert m.classify(O("swap")) == pm.LEGAL
    # a block without an observed row has no cache, whatever the state; a prediction needs a sweep's normals
    assert m.classify(O("get_block", slot=0, u="empty")) == pm.REFUSED
    assert pm.Model(False).classify(O("predict")) == pm.REFUSED


def test_committed_seeds_meet_the_coverage_condition():
    """For every lazy flag of the handle: each pair of an operation that sets or invalidates it and the next operation that
    reads it occurs at least twice over the committed sequences, at least once with a refused call or a failing proposal in
    between.  Computed from the model alone."""
    table = pm.pair_table(committed())
    empty = []
    for flag, cells in sorted(pm.required_cells(True).items()):
        print(flag)
        for w, r in cells:
            n, marked = table.get((flag, w, r), (0, 0))
            print(f"    {w:12s} -> {r:16s} {n:4d}   with a refusal or a failing proposal in between {marked:3d}")
            if n < 2 or marked < 1:
                empty.append((flag, w, r, n, marked))
    assert not empty, empty


@pytest.fixture(scope="module")
def oracle_replays():
    """Tree a, its first seed with a failing proposal: the oracle executor twice."""
    tree = "a"
    seed = next(s for s in pm.TREES[tree]["seeds"] if any(op.tid == pm.BAD and op.name in ("factor", "enqueue") for op in pm.sequence(tree, s)))
    pb = pm.TREES[tree]["problem"]()
    ops = pm.sequence(tree, seed)
    return pb, seed, ops, [pm.replay(ops, pm.OracleExecutor(pm.Inputs(pb, seed)), pm.TREES[tree]["has_ahead"]) for _ in range(2)]


def equal(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(equal(a[k], b[k]) for k in a)
    if a is None or b is None:
        return a is b
    return np.array_equal(np.asarray(a), np.asarray(b))


def test_oracle_executor_is_deterministic(oracle_replays):
    pb, seed, ops, (first, second) = oracle_replays
    assert len(first) == len(second) == len(ops)
    for i, (a, b) in enumerate(zip(first, second)):
        assert equal(a, b), (i, pm.show(ops[i]))
    m = pm.Model(True)
    for op, o in zip(ops, first):          # it skips exactly the refused calls and what only the lazy handle runs
        cls = m.classify(op)
        assert (o is None) == (cls == pm.REFUSED or op.name in ("begin", "ahead")), pm.show(op)
        if cls != pm.REFUSED:
            m.apply(op)


def test_oracle_executor_reports_the_oracle_s_failure_code(oracle_replays):
    pb, seed, ops, (first, _) = oracle_replays
    inp = pm.Inputs(pb, seed)
    om = oracle_model(pb, theta=inp.bad, w=inp.w0)
    code, level = oracle_phase_a_failure(om, om.param_data)
    assert code in (1, 2, 3)
    m = pm.Model(True)
    seen = 0
    for op, o in zip(ops, first):
        cls = m.classify(op)
        if cls == pm.FAILS:
            assert o["rc"] == code, (pm.show(op), o, code)
            seen += 1
        elif o is not None:
            assert o["rc"] == 0, (pm.show(op), o)
        if cls != pm.REFUSED:
            m.apply(op)
    assert seen > 0


@pytest.mark.parametrize("tree", sorted(pm.TREES))
def test_every_tree_has_a_failing_theta_and_the_block_handful(tree):
    pb = pm.TREES[tree]["problem"]()
    inp = pm.Inputs(pb, 0)
    om = oracle_model(pb, theta=inp.bad)
    assert oracle_phase_a_failure(om, om.param_data)[0] in (1, 2, 3)
    b = inp.blocks
    nobs = [int(np.isfinite(pb["y"][ix]).sum()) for ix in pb["indexing"]]
    assert nobs[b["root"]] > 0 and len(pb["parents"][b["root"]]) == 0
    assert nobs[b["lastref"]] > 0 and nobs[b["leaf"]] > 0 and nobs[b["empty"]] == 0
    assert len({b["root"], b["lastref"], b["leaf"], b["empty"]}) == 4
    assert np.all(np.isfinite(inp.theta(5))) and not np.array_equal(inp.theta(5), inp.theta(6))
