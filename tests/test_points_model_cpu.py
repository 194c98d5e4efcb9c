"""CPU: the model of the new-point family's contract (tests/points_model.py) and its committed seeds.

1. Coverage.  The seed list is asserted outright: every operation kind in every point-set family it applies to, every refusal the
   header names, and every interaction between the riders that tests/test_gpu_points_sequences.py is there for -- each with the
   affected rider holding state.  A change to the generator that loses a case fails here.
2. Sensitivity.  Deliberately wrong variants of the contract (a reset that leaves a rider's state, a functional replacement that
   keeps a functional part, a stored row that follows n_accumulated, ...) replayed on the committed sequences with synthetic
   per-draw outputs: every variant must be told from the contract by at least one read.  This is what shows the sequences would
   notice such a bug in the library, without running a wrong kernel anywhere.
3. The executor's definitions against the references the device tests use, on synthetic draws."""
import numpy as np
import pytest

from tests import points_model as pm
from tests.points_model import LEGAL, REFUSED, Op

RIDER_OF_READ = {r: k for k, v in pm.RIDER_READS.items() for r in v}


def nontrivial(m):
    """Per rider: whether it holds at least one accumulated draw."""
    return dict(fun=bool(m.fun and m.fun.seen), score=bool(m.score and m.score.seen), exceed=bool(m.exceed and m.exceed.seen),
                mix=bool(m.mix and m.mix.cols), summary=bool(m.keep > 0 and m.store))


def walk(ops, model=pm.Model):
    """(index, op, model before it, classification) over a sequence."""
    m = model()
    for i, op in enumerate(ops):
        cls = m.classify(op)
        yield i, op, m, cls
        if cls[0] == LEGAL:
            m.apply(op)
        elif cls[0] == REFUSED:
            m.refuse(op)


def events(ops):
    """What a sequence covers: ("op", kind of the set, operation name), ("refusal", name), ("interaction", name)."""
    out = set()
    dirty_by = None
    after_switch = None
    replaced = set()                 # riders replaced while they held state, in the current point set
    ops = list(ops)
    for i, op, m, cls in walk(ops):
        n, a = op.name, op.arg
        hit = lambda name: out.add(("interaction", name))   # noqa: E731
        if after_switch is not None and i == after_switch + 5:
            names = [o.name for o in ops[after_switch + 1:i + 1]]
            if names == ["fun_get", "score_get", "exceed_get", "mix_draws", "squantile"] and cls[0] == REFUSED:
                hit("new_set_with_all_five_then_refused_reads")
        if cls[0] == LEGAL:
            out.add(("op", m.kind if n != "set" else a, n + ("-null" if n in ("acc", "accj") and not a else "")))
        if cls[0] == REFUSED:
            name = m.refusal_name(op)
            if name:
                out.add(("refusal", name))
            if m.kind == "empty" and n == "score":
                hit("score_on_empty")
            if m.kind == "empty" and n == "squantile" and m.seen:
                hit("summary_on_empty")
            continue
        nt = nontrivial(m)
        if n == "set":
            replaced = set()
        if n in ("fun", "score", "exceed", "mix") and nt[n] and a not in (None, 0):
            replaced.add(n)
        if n == "fun":
            if m.exceed and m.exceed.fun and m.exceed.seen and m.fun:
                hit("fun_removed_under_thr_fun" if a is None else "fun_replaced_under_thr_fun")
            if m.mix and m.mix.fcols:
                hit("fun_set_with_mix_columns_below_keep" if len(m.mix.cols) < m.mix.keep else "fun_set_with_mix_columns_at_keep")
        if n in ("get", "squantile") or n in RIDER_OF_READ:                       # a rider that started later than the summaries
            r = RIDER_OF_READ.get(n)
            ids = {"fun": m.fun and m.fun.seen, "score": m.score and m.score.seen, "exceed": m.exceed and m.exceed.seen,
                   "mix": m.mix and m.mix.cols}.get(r)
            if ids and r in replaced:
                hit(f"{r}_replaced_with_state_then_read")
            if ids and len(m.seen) - len([x for x in m.seen if x >= ids[0]]) >= 2:
                hit(f"{r}_set_after_two_draws")
            if m.kind in ("empty", "single") and (ids or (r == "summary" and (m.seen if m.kind == "empty" else m.store))):
                hit(f"{r}_on_{m.kind}")
        if n == "reserve" and m.keep > 0 and m.seen and m.fun and m.fun.store and m.score and m.score.seen:
            hit("reserve_mid_chain_" + ("to_0" if a == 0 else "growing" if a > m.keep else "shrinking" if a < m.keep else "same"))
        if n == "score_get" and a[0] and m.store[0] > m.seen[0] and m.score.seen[0] < m.store[0]:
            hit("crps_reads_the_new_store")
        if n == "reset" and all(nt.values()):
            hit("reset_with_all_five")
        if n == "set" and m.kind and a != m.kind and all(x is not None for x in (m.fun, m.score, m.exceed, m.mix)) and m.keep > 0:
            after_switch = i
        if n in ("acc", "accj"):
            if m.keep > 0 and len(m.store) == m.keep:
                hit("accumulate_beyond_summary_keep")
            if m.fun and m.keep > 0 and len(m.fun.store) == m.keep:
                hit("accumulate_beyond_functional_keep")
            if m.mix and len(m.mix.cols) == m.mix.keep:
                hit("accumulate_beyond_mixture_keep")
            if m.dirty and m.fun and m.exceed and m.mix and m.seen:
                hit(f"{dirty_by}_between_accumulates_with_riders")
        if n in ("predict", "squantile"):
            dirty_by = n
    return out


OPS_EVERYWHERE = ("set", "reset", "reserve", "fun", "exceed", "mix", "acc", "acc-null", "predict", "get", "fun_get", "fun_last", "fun_info",
                  "exceed_get", "mix_draws", "mix_quantiles", "mix_info", "sweep", "beta", "tausq", "theta")
OPS_WITH_DRAWS = ("squantile", "fun_quantile")                        # not on the empty set: it stores no draw
OPS_WITH_X = ("score", "score_get", "mix_crps")
OPS_JOINT = ("accj", "accj-null", "get_cov", "layout")
INTERACTIONS = ("fun_removed_under_thr_fun", "fun_replaced_under_thr_fun", "fun_set_with_mix_columns_below_keep",
                "fun_set_with_mix_columns_at_keep", "fun_set_after_two_draws", "score_set_after_two_draws", "exceed_set_after_two_draws",
                "mix_set_after_two_draws", "reserve_mid_chain_to_0", "reserve_mid_chain_growing", "reserve_mid_chain_shrinking",
                "crps_reads_the_new_store", "reset_with_all_five", "new_set_with_all_five_then_refused_reads",
                "accumulate_beyond_summary_keep", "accumulate_beyond_functional_keep", "accumulate_beyond_mixture_keep",
                "fun_on_empty", "score_on_empty", "exceed_on_empty", "mix_on_empty", "summary_on_empty",
                "fun_on_single", "score_on_single", "exceed_on_single", "mix_on_single", "summary_on_single",
                "predict_between_accumulates_with_riders", "squantile_between_accumulates_with_riders",
                "fun_replaced_with_state_then_read", "score_replaced_with_state_then_read", "exceed_replaced_with_state_then_read",
                "mix_replaced_with_state_then_read")


def required():
    req = set()
    for kind, (n, has_X, joint) in pm.KINDS.items():
        names = OPS_EVERYWHERE + (OPS_WITH_DRAWS if n > 0 else ()) + (OPS_WITH_X if has_X else ()) + (OPS_JOINT if joint else ())
        req |= {("op", kind, x) for x in names}
    req |= {("refusal", r) for r in pm.REFUSALS}
    req |= {("interaction", x) for x in INTERACTIONS}
    return req


_SEQ = {}


def sequences():
    if not _SEQ:
        _SEQ.update({c: pm.sequence(*c) for c in pm.cases()})
    return _SEQ


def test_the_committed_seeds_cover_every_operation_refusal_and_interaction():
    got = set()
    for ops in sequences().values():
        got |= events(ops)
    missing = sorted(required() - got)
    assert not missing, missing


def test_sequences_hold_only_legal_and_refused_calls_and_the_cli_prints_them():
    for (family, seed), ops in sequences().items():
        assert 70 <= len(ops) <= 90 or family == "regression"
        for i, op, m, cls in walk(ops):
            assert cls[0] in (LEGAL, REFUSED), (family, seed, i, op)
        text = pm.describe(ops, upto=5)
        assert len(text.splitlines()) == 6 and "set=" in text
        m = pm.Model()                                   # w or theta changes between any two accumulates: their conditional moments differ
        for op in ops:
            if m.classify(op)[0] == LEGAL and m.apply(op) not in (None, 0):
                assert m.acc_chain[m.next_id - 1] != m.acc_chain[m.next_id - 2], (family, seed, op)
    assert pm.sequence("joint", 0) == pm.sequence("joint", 0) and pm.sequence("joint", 0) != pm.sequence("joint", 1)
    assert any(f == "joint" for f, _ in pm.GENERIC) and any(f == "plainX" for f, _ in pm.GENERIC) and pm.GENERIC <= set(pm.cases())


def test_every_solo_replay_classifies_its_operations_as_the_interleaved_one():
    """The filter of a rider's solo replay keeps the rider's prerequisites: what it keeps is legal or refused exactly as in the whole
    sequence, and its stores hold the same ids."""
    for case, ops in sequences().items():
        for rider in pm.RIDERS:
            solo = pm.Model()
            for i, op, m, cls in walk(ops):
                if not pm.solo_keeps(rider, op):
                    continue
                assert solo.classify(op) == cls, (case, rider, i, op)
                if op.name in pm.READS + ("squantile",) and cls[0] == LEGAL:
                    c = pm.Contract(None, None)
                    assert c.signature(op, solo) == c.signature(op, m), (case, rider, i, op)
                if cls[0] == LEGAL:
                    solo.apply(op)


# ---- 2. the wrong variants --------------------------------------------------------------------------------------------------
class ResetLeavesScores(pm.Model):
    def on_reset(self):
        keep = self.score and list(self.score.seen)
        super().on_reset()
        if self.score:
            self.score.seen = keep


class ResetLeavesThresholds(pm.Model):
    def on_reset(self):
        keep = self.exceed and list(self.exceed.seen)
        super().on_reset()
        if self.exceed:
            self.exceed.seen = keep


class ResetLeavesMixtureCount(pm.Model):
    def on_reset(self):
        keep = self.mix and (list(self.mix.cols), list(self.mix.fcols))
        super().on_reset()
        if self.mix:
            self.mix.cols, self.mix.fcols = keep


class ResetLeavesPairAccumulators(pm.Model):
    def on_reset(self):
        keep = list(self.pair)
        super().on_reset()
        self.pair = keep


class FunctionalsSetKeepsThresholdPart(pm.Model):
    def on_fun_set(self, a):
        had = self.exceed and self.exceed.fun
        super().on_fun_set(a)
        if self.exceed:
            self.exceed.fun = had


class FunctionalsSetKeepsStorePart(pm.Model):
    def on_fun_set(self, a):
        keep = self.mix and (list(self.mix.fcols), self.mix.n_fun)
        super().on_fun_set(a)
        if self.mix and keep[1] and self.mix.n_fun:
            self.mix.fcols = keep[0]


class StoredRowFollowsNAccumulated(pm.Model):
    """The header's old sentence taken literally: a draw goes to row n_accumulated while the count of stored rows starts again."""
    def _new_set(self):
        super()._new_set()
        self.rows = {}

    def on_reset(self):
        super().on_reset()
        self.rows = {}

    def on_reserve(self):
        self.rows = {}

    def on_store(self, i):
        self.store.append(i)
        self.rows[len(self.seen) - 1] = i

    def stored_rows(self):
        return [self.rows.get(r, -1 - r) for r in range(len(self.store))]


class MixtureFunctionalColumnsKeepFilling(pm.Model):
    def on_mix_step(self, i):
        mx = self.mix
        if len(mx.cols) < mx.keep:
            mx.cols.append(i)
        if mx.n_fun > 0 and self.fun and len(mx.fcols) < mx.keep:
            mx.fcols.append(i)


class RefusalMutates(pm.Model):
    """A refused set drops what it was to replace."""
    def refuse(self, op):
        if self.kind and op.name in ("fun", "score", "exceed"):
            self.apply(Op(op.name, None))
        if self.kind and op.name in ("reserve", "mix"):
            self.apply(Op(op.name, 0))


def keeps_accumulator(rider):
    class ReplacedRiderKeepsItsAccumulator(pm.Model):
        def on_replace(self, r, new):
            old = getattr(self, r)
            if r == rider and old is not None and new is not None:
                if r == "mix":
                    new.cols, new.fcols = list(old.cols)[:new.keep], list(old.fcols)[:new.keep]
                else:
                    new.seen = list(old.seen)
            return new
    ReplacedRiderKeepsItsAccumulator.__name__ += "_" + rider
    return ReplacedRiderKeepsItsAccumulator


class QuantileScratchLeaksIntoFunctionals(pm.Model):
    """The functional step of the next accumulate reads what st_points_summary_quantile or st_points_predict left in the buffer."""
    def fun_source(self, i):
        return -1 - i if self.dirty else i


VARIANTS = [ResetLeavesScores, ResetLeavesThresholds, ResetLeavesMixtureCount, ResetLeavesPairAccumulators, FunctionalsSetKeepsThresholdPart,
            FunctionalsSetKeepsStorePart, StoredRowFollowsNAccumulated, MixtureFunctionalColumnsKeepFilling, RefusalMutates,
            QuantileScratchLeaksIntoFunctionals] + [keeps_accumulator(r) for r in ("fun", "score", "exceed", "mix")]

_INP = []


def inputs():
    if not _INP:
        _INP.append(pm.Inputs())
    return _INP[0]


def differ(a, b):
    if isinstance(a, dict):
        return any(differ(a[k], b[k]) for k in a)
    if a is None or b is None:
        return (a is None) != (b is None)
    a, b = np.asarray(a), np.asarray(b)
    return a.shape != b.shape or not np.array_equal(a, b, equal_nan=True)


def first_detection(variant, ops):
    """Index of the first read of ``ops`` that tells ``variant`` from the contract (None: none does)."""
    inp = inputs()
    right, wrong = pm.Model(), variant()
    records = {}
    c = pm.Contract(inp, records)
    for i, op in enumerate(ops):
        cr, cw = right.classify(op), wrong.classify(op)
        if op.name in pm.READS + ("squantile",):
            sr_, sw = c.signature(op, right), c.signature(op, wrong)
            if sr_ != sw:
                if cr != cw or right.counts(op) != wrong.counts(op):
                    return i
                with np.errstate(all="ignore"):
                    if differ(c.read(op, right), c.read(op, wrong)):
                        return i
        for m, cls in ((right, cr), (wrong, cw)):
            if cls[0] == LEGAL:
                acc = m.apply(op)
                if acc is not None and m is right:
                    records[acc] = pm.synthetic_record(inp, m.kind, acc, m.fun.name if m.fun else None, chain=m.acc_chain[acc])
            elif cls[0] == REFUSED:
                m.refuse(op)
        assert right.next_id == wrong.next_id
    return None


@pytest.mark.parametrize("variant", VARIANTS, ids=[v.__name__ for v in VARIANTS])
def test_every_wrong_variant_is_told_from_the_contract_by_a_read(variant):
    found = {}
    for case, ops in sequences().items():
        i = first_detection(variant, ops)
        if i is not None:
            found[case] = i
    print(f"{variant.__name__}: told apart in {len(found)} of {len(sequences())} sequences, first at {sorted(found.items())[:4]}")
    assert found, f"no committed sequence tells {variant.__name__} from the contract"


def test_the_contract_itself_is_not_told_from_the_contract():
    for ops in sequences().values():
        assert first_detection(pm.Model, ops) is None


# ---- 3. the executor's definitions ----------------------------------------------------------------------------------------------
def test_the_executor_agrees_with_the_references_of_the_device_tests():
    """On synthetic draws of the joint kind: lpd, pit and the empirical CRPS against tests/score_reference.py, the exceedance
    probabilities against tests/exceed_reference.py, the mixture quantile against tests/mixture_reference.py's definition check."""
    from tests import exceed_reference as er
    from tests import mixture_reference as mr
    from tests import score_reference as sr
    inp = inputs()
    m = pm.Model()
    records = {}
    for op in (Op("set", "joint"), Op("theta", 0), Op("fun", "A"), Op("reserve", 5), Op("score", "nan"), Op("exceed", (3, True)), Op("mix", 3)):
        m.apply(op)
    for _ in range(4):
        i = m.apply(Op("accj", True))
        records[i] = pm.synthetic_record(inp, "joint", i, "A")
    c = pm.Contract(inp, records)
    P = inp.points("joint")
    y = inp.y_new("joint", "nan")
    with np.errstate(all="ignore"):
        sc = c.read(Op("score_get", (True, True)), m)
        ex = c.read(Op("exceed_get", True), m)
        mq = c.read(Op("mix_quantiles", True), m)
    recs = [records[i] for i in m.seen]
    thr, side = inp.thresholds(3)
    for i in np.nonzero(~np.isnan(y))[0]:
        j = P["mv"][i] - 1
        lpd, lb, pit, pb = sr.point_scores(y[i], P["X"][i], [r["beta"][:, j] for r in recs], [r["mean"][i] for r in recs],
                                           [r["var"][i] for r in recs], [r["tausq_inv"][j] for r in recs])
        assert abs(sc["lpd"][i] - float(lpd)) <= 1e-12 * max(1.0, abs(float(lpd))) and abs(sc["pit"][i] - float(pit)) <= 1e-13
        want, _ = sr.crps_sorted([r["yhat"][i] for r in recs], y[i])
        assert abs(sc["crps"][i] - float(want)) <= 1e-13
        for t in range(3):
            prob, _, var, _ = er.point_w([r["mean"][i] for r in recs], [r["var"][i] for r in recs], thr[t][j], int(side[t]))
            assert abs(ex["w"]["prob"][t, i] - float(prob)) <= 1e-14 and abs(ex["w"]["prob_var"][t, i] - float(var)) <= 1e-14
    assert np.all(np.isnan(sc["lpd"][np.isnan(y)])) and np.isfinite(sc["lpd_joint"][0]) and ex["fun_w"]["prob"].shape == (3, 3)
    K = len(m.mix.cols)
    assert K == 3
    for i in (0, 5, inp.n_big - 1):
        comps = mr.components(np.array([records[s]["mean"][i] for s in m.mix.cols]), np.array([records[s]["var"][i] for s in m.mix.cols]))
        for t, p in enumerate(pm.PROBS):
            assert mr.check_quantile(mq["w"][t, i], p, comps) <= 1.0
    assert mq["fun_w"].shape == (3, 3)
