"""A host-side model of the call contract of the single-GPU C-ABI (include/spamtree_hip.h), a seeded generator of call
sequences that walks it, and three executors that replay a sequence: the library as the driver uses it (every deferral and
cache on), the same library with every short cut off, and the NumPy oracle.  Pure Python and NumPy; the two library
executors import the library when they are constructed, nothing here needs a GPU before that.

The model holds only what a caller can know: whether a factorisation is open (st_factor_enqueue without its
st_factor_finish), whether a sweep is pending (st_sample_w_loglik_begin without its _end), whether top levels run ahead of
time (st_factor_begin) and for which slot and theta, which theta sits in which slot and whether each slot's last
factorisation succeeded.  `Model.classify` puts every operation in every state into one of
  LEGAL        returns 0 and does what the header says;
  FAILS        legal, and the factorisation fails in phase A (the tree's errtype for its failing theta);
  REFUSED      a negative code, a text in st_last_error, the handle unchanged;
  UNSPECIFIED  the header defines no result (a reader of a slot whose factorisation failed or whose top levels were
               replaced by st_factor_begin, st_swap onto such a slot): the generator never emits these.
The table is the one in include/spamtree_hip.h next to st_factor_enqueue.

    python -m tests.protocol_model --tree a --seed 3 --upto 17

prints the first 18 operations (indices 0 .. 17) of that sequence with the model's flags before each: the prefix a failure
message of tests/test_gpu_protocol_sequences.py names.
"""
from __future__ import annotations

import argparse
import collections
import ctypes as C

import numpy as np

LEGAL, FAILS, REFUSED, UNSPECIFIED = "legal", "fails", "refused", "unspecified"
BAD = -1                                  # theta id of the failing theta
BLOCKS = ("root", "lastref", "leaf", "empty")   # the fixed handful of st_get_block: resolved per tree by block_handful

Op = collections.namedtuple("Op", "name slot tid key u arg", defaults=(None, None, None, None, None))


def kind(op):
    """The operation's name with what selects its code path: the slot, the enable flag."""
    if op.name == "ahead":
        return f"ahead{op.arg}"
    if op.slot is not None:
        return f"{op.name}{op.slot}"
    return op.name


def show(op):
    parts = [kind(op)]
    if op.tid is not None:
        parts.append("theta=" + ("BAD" if op.tid == BAD else str(op.tid)))
    if op.u is not None:
        parts.append("block=" + op.u)
    if op.key is not None:
        parts.append(f"key={op.key}")
    return " ".join(parts)


SWEEPS = ("sample", "sample_ll", "sweep_begin")


class Model:
    """The documented contract.  `has_ahead`: st_factor_ahead_levels(h) > 0 for the tree (a caller can ask)."""

    def __init__(self, has_ahead):
        self.has_ahead = bool(has_ahead)
        self.open = None          # slot of the open factorisation
        self.open_bad = False
        self.pending = None       # slot of the pending sweep's log-density
        self.ahead_on = True
        self.top = None           # (slot, tid) of st_factor_begin's levels in flight
        self.tid = [None, None]   # theta id per slot
        self.ok = [False, False]  # the slot's last factorisation succeeded and st_factor_begin has not replaced its top levels
        self.z_valid = False
        self.resid_ok = False     # d_resid is that of one successful factorisation
        self.predict_tid = 0      # theta at the last prediction (the driver's predict_param; the initial theta before any)
        # what decides how close the two library handles and the oracle must be (not part of the contract)
        self.gram_valid = False   # the next sweep of a caching handle takes the cached-Gram kernels
        self.w_rounding = False   # w has been through such a sweep since the last st_set_w
        self.comps_rounding = [False, False]
        self.resid_rounding = False
        self.open_rounding = self.pending_rounding = False      # ... of the result that st_factor_finish / _end will hand over
        self.w_sweeps = 0         # sweeps since the last st_set_w

    # ---- the table
    def classify(self, op):
        n, s = op.name, op.slot
        is_open, pend = self.open is not None, self.pending is not None
        if n in ("factor", "begin"):
            if is_open:
                return REFUSED
            if n == "factor":
                return FAILS if op.tid == BAD else LEGAL
            return LEGAL
        if n == "enqueue":
            return REFUSED if is_open else LEGAL        # a failing theta: the code comes from finish
        if n == "finish":
            if not is_open:
                return REFUSED
            return FAILS if self.open_bad else LEGAL
        if n == "sweep_end":
            return LEGAL if pend else REFUSED
        if n in ("ahead", "set_beta", "set_tausq", "beta_stats", "tausq_stats"):
            return LEGAL
        if n == "swap":
            if is_open or pend or self.top is not None:
                return REFUSED
            return LEGAL if self.ok[1] else UNSPECIFIED
        if n in SWEEPS:
            if is_open or pend:
                return REFUSED
            if not self.ok[0] or (s is not None and not self.ok[s]):
                return UNSPECIFIED
            return LEGAL
        if n == "loglik":
            if (is_open and self.open == s) or pend:
                return REFUSED
            return LEGAL if self.ok[s] else UNSPECIFIED
        if n == "predict":
            if is_open or pend or not self.z_valid:
                return REFUSED
            return LEGAL if self.ok[0] else UNSPECIFIED
        if n in ("set_w", "get_w", "yhat"):
            return REFUSED if pend else LEGAL
        if n in ("get_comps", "get_block"):
            if is_open and self.open == s:
                return REFUSED
            if n == "get_block" and op.u == "empty":
                return REFUSED                           # "block has no observations, hence no cache", in every state
            return LEGAL if self.ok[s] else UNSPECIFIED
        if n == "get_resid":
            return LEGAL if self.resid_ok else UNSPECIFIED
        raise ValueError(n)

    def theta_changed(self, theta_of):
        """The driver's rule (spamtree_fit.cpp: need_update): the entries of the accepted theta that moved since the last
        prediction by more than 1e-5."""
        a, b = theta_of(self.tid[0]), theta_of(self.predict_tid)
        return int(np.sum(np.abs(a - b) > 1e-05))

    # ---- the effect of a LEGAL / FAILS operation
    def _factorised(self, slot, tid):
        self.top = None
        self.tid[slot] = tid
        self.ok[slot] = tid != BAD
        self.resid_ok = tid != BAD
        self.comps_rounding[slot] = self.w_rounding
        self.resid_rounding = self.w_rounding
        if slot == 0:
            self.gram_valid = False

    def apply(self, op):
        n, s = op.name, op.slot
        if n == "factor":
            self._factorised(s, op.tid)
        elif n == "enqueue":
            self._factorised(s, op.tid)
            self.open, self.open_bad, self.open_rounding = s, op.tid == BAD, self.w_rounding
        elif n == "finish":
            self.open = None
        elif n == "begin":
            if self.ahead_on and self.has_ahead:
                self.top = (s, op.tid)
                self.ok[s] = False
                self.resid_ok = False
        elif n == "ahead":
            self.ahead_on = bool(op.arg)
        elif n == "swap":
            self.tid.reverse(); self.ok.reverse(); self.comps_rounding.reverse()
            self.gram_valid = False
        elif n in SWEEPS:
            self.w_rounding = self.w_rounding or self.gram_valid
            self.gram_valid = True
            self.z_valid = True
            self.w_sweeps += 1
            if s is not None:
                self.comps_rounding[s] = self.w_rounding
            if n == "sweep_begin":
                self.pending, self.pending_rounding = s, self.w_rounding
        elif n == "sweep_end":
            self.pending = None
        elif n == "loglik":
            self.comps_rounding[s] = self.w_rounding
        elif n == "predict":
            self.predict_tid = self.tid[0]
        elif n == "set_w":
            self.w_rounding = False
            self.w_sweeps = 0

    def flags(self):
        return (f"open={self.open}{'(failing)' if self.open_bad and self.open is not None else ''} pending={self.pending} "
                f"top={self.top} ahead_on={self.ahead_on} theta={self.tid} ok={self.ok} z_valid={self.z_valid} "
                f"resid_ok={self.resid_ok} gram_valid={self.gram_valid}")

    def repair(self, op):
        """An operation that brings an UNSPECIFIED `op` closer to LEGAL."""
        if op.name == "get_resid" and self.open is not None:
            return Op("finish")
        need = 0 if (not self.ok[0] and (op.name in SWEEPS or op.name == "predict" or op.slot == 0)) else 1
        if op.name in ("swap",):
            need = 1
        if op.name == "get_resid":
            need = 1
        return Op("factor", slot=need, tid="fresh")


# ---- the lazy state of the handle (spamtree_amd/csrc/st_handle.hpp): which operations write each flag, which read it
def _factor_label(m, op):
    k = kind(op)
    if m.top is None or op.name not in ("factor", "enqueue"):
        return k
    return k + ("_same" if m.top == (op.slot, op.tid) else "_other")


def flag_events(m, op, cls):
    """[(flag, 'w' or 'r', label)] of `op`, classified `cls`, in the state `m` (before it is applied).  A refused operation
    reads the flag that refuses it and writes nothing."""
    k, n, s = kind(op), op.name, op.slot
    ev = []
    done = cls in (LEGAL, FAILS)
    # leaf_pending / leaf_cp / d_vleaf: the proposal's leaf panels, finished by the first reader of the slot
    if done and (k in ("enqueue1", "factor1", "swap")):
        ev.append(("leaf_pending", "w", k))
    if done and k in ("swap", "get_block1", "loglik1", "sample_ll1", "sweep_begin1"):
        ev.append(("leaf_pending", "r", k))
    # gram_valid / s0_valid / cache_gram
    if done and n in SWEEPS:
        ev.append(("gram_valid,s0_valid", "r", n))
    if done and (k in ("factor0", "swap") or n in SWEEPS):
        ev.append(("gram_valid,s0_valid", "w", k if k in ("factor0", "swap") else n))
    # top_pending / top_phys / top_theta, and async_top_off
    if m.has_ahead:
        if n in ("factor", "enqueue") and done:
            ev.append(("top_pending", "r", _factor_label(m, op)))
            ev.append(("top_pending", "w", "factorised"))
        if n == "begin" and done:
            ev.append(("top_pending", "r", k))
            ev.append(("async_top_off", "r", k))
            if m.ahead_on:
                ev.append(("top_pending", "w", k))
        if n == "swap" and m.open is None and m.pending is None:
            ev.append(("top_pending", "r", k))
        if n == "ahead":
            ev.append(("async_top_off", "w", k))
    # factor_open / factor_open_slot
    if n in ("finish", "enqueue", "swap", "predict", "factor", "begin") or n in SWEEPS or k in ("get_block1", "get_comps1", "loglik1"):
        ev.append(("factor_open", "r", k if n not in SWEEPS else n))
    if done and n in ("enqueue", "finish"):
        ev.append(("factor_open", "w", k))
    # c_pending
    if n in ("sweep_end", "set_w", "get_w", "predict", "yhat", "swap", "loglik") or n in SWEEPS:
        if not (m.open is not None and (n in SWEEPS or n in ("swap", "predict") or (n == "loglik" and s == m.open))):
            ev.append(("c_pending", "r", n))          # (refused for the open factorisation first: c_pending is not reached)
    if done and n in ("sweep_begin", "sweep_end"):
        ev.append(("c_pending", "w", n))
    # stats_valid / host_stats_valid / stats_on_stream2 / stats_prefetched
    if done:
        if n in ("beta_stats", "tausq_stats"):
            ev.append(("stats_valid", "r", "stats")); ev.append(("stats_valid", "w", "stats"))
        elif k in ("factor1", "enqueue1"):
            ev.append(("stats_valid", "r", "proposal")); ev.append(("stats_valid", "w", "proposal"))
        elif n in SWEEPS:
            ev.append(("stats_valid", "w", "sweep"))
        elif n in ("set_w", "set_beta", "predict"):
            ev.append(("stats_valid", "w", n))
    # z_valid
    if n == "predict" and m.open is None and m.pending is None:
        ev.append(("z_valid", "r", n))
    if done and n in SWEEPS:
        ev.append(("z_valid", "w", "sweep"))
    # slot_map
    if done and n == "swap":
        ev.append(("slot_map", "w", k))
    if done and (s is not None or n in ("sample", "predict")) and n != "swap":
        ev.append(("slot_map", "r", k))
    # d_resid: one buffer for both slots
    if done and n in ("factor", "enqueue"):
        ev.append(("d_resid", "w", k))
    if done and n == "get_resid":
        ev.append(("d_resid", "r", k))
    return ev


def required_cells(has_ahead=True):
    """flag -> the (writer, reader) pairs the committed sequences must contain: every operation that sets or invalidates the flag
    with every operation that can be the next to read it."""
    sl = ("factor0", "factor1", "enqueue1", "begin1", "loglik0", "loglik1", "sample", "sample_ll0", "sample_ll1", "sweep_begin0",
          "sweep_begin1", "get_comps0", "get_comps1", "get_block0", "get_block1", "predict")
    opened = ("finish", "enqueue1", "swap", "sample", "sample_ll", "sweep_begin", "predict", "factor0", "factor1", "begin1", "get_block1",
              "get_comps1", "loglik1")
    pend = ("sweep_end", "sweep_begin", "sample", "sample_ll", "set_w", "get_w", "predict", "yhat", "swap", "loglik")
    cells = {
        "leaf_pending": [(w, r) for w in ("enqueue1", "factor1", "swap") for r in ("swap", "get_block1", "loglik1", "sample_ll1", "sweep_begin1")],
        "gram_valid,s0_valid": [(w, r) for w in ("factor0", "swap") + SWEEPS for r in SWEEPS],
        "factor_open": [("enqueue1", r) for r in opened] + [("finish", "finish"), ("finish", "enqueue1")],
        "c_pending": [("sweep_begin", r) for r in pend] + [("sweep_end", "sweep_end"), ("sweep_end", "sweep_begin")],
        "stats_valid": [(w, r) for w in ("set_w", "set_beta", "sweep", "predict", "stats", "proposal") for r in ("stats", "proposal")],
        "z_valid": [("sweep", "predict")],
        "slot_map": [("swap", r) for r in sl],
        "d_resid": [(w, "get_resid") for w in ("factor0", "factor1", "enqueue1")],
    }
    if has_ahead:
        cells["top_pending"] = [("begin1", r) for r in ("factor1_same", "factor1_other", "enqueue1_same", "enqueue1_other", "factor0_other",
                                                        "swap", "begin1")] + [("factorised", r) for r in ("swap", "begin1", "factor1", "enqueue1", "factor0")]
        cells["async_top_off"] = [("ahead0", "begin1"), ("ahead1", "begin1")]
    return cells


def pair_table(sequences):
    """{(flag, writer, reader): [count, count with a refused call or a failing proposal in between]} over `sequences`, each a
    (has_ahead, ops) pair: for every read, the pair of the last write of the flag before it and the read."""
    table = collections.defaultdict(lambda: [0, 0])
    for has_ahead, ops in sequences:
        m = Model(has_ahead)
        last = {}                        # flag -> (label, index)
        marks = []                       # indices of refused calls and failing proposals
        for i, op in enumerate(ops):
            cls = m.classify(op)
            assert cls != UNSPECIFIED, (i, show(op), m.flags())
            ev = flag_events(m, op, cls)
            for flag, rw, label in ev:
                if rw == "r" and flag in last:
                    w, j = last[flag]
                    cell = table[(flag, w, label)]
                    cell[0] += 1
                    cell[1] += any(j < x < i for x in marks)
            for flag, rw, label in ev:
                if rw == "w":
                    last[flag] = (label, i)
            if cls == REFUSED or cls == FAILS:
                marks.append(i)
            if cls != REFUSED:
                m.apply(op)
    return table


# ---- the generator
IN_OPEN = ["tausq_stats", "set_tausq", "beta_stats", "set_beta", "get_resid", "get_w", "set_w", "yhat", "get_comps0", "get_block0", "loglik0",
           "ahead"]
IN_PENDING = ["tausq_stats", "set_tausq", "beta_stats", "set_beta", "get_resid", "get_comps0", "get_comps1", "get_block0", "get_block1",
              "factor1", "factor0", "begin1", "ahead"]
ANY = ["factor0", "factor1", "enqueue1", "finish", "begin1", "ahead", "swap", "sample", "sample_ll0", "sample_ll1", "sweep_begin0", "sweep_begin1",
       "sweep_end", "loglik0", "loglik1", "predict", "set_w", "set_beta", "set_tausq", "beta_stats", "tausq_stats", "yhat", "get_w", "get_comps0",
       "get_comps1", "get_block0", "get_block1", "get_resid"]


class Generator:
    """numpy.random.default_rng(seed) and nothing else.  It strings together short scenarios -- a (writer, reader) pair of one
    lazy flag with fillers in between, a split factorisation or a split sweep with calls inside, the driver's own iteration --
    and repairs the state where the next operation of a scenario would be UNSPECIFIED."""

    def __init__(self, seed, has_ahead, n_ops=40):
        self.rng = np.random.default_rng(seed)
        self.m = Model(has_ahead)
        self.n_ops = n_ops
        self.ops = []
        self.n_theta = 0
        self.n_key = 0
        # (the pairs of the ahead-of-time path three times: only a tree with such levels can contribute them)
        cells = [(f, c) for f, cs in sorted(required_cells(has_ahead).items()) for c in cs * (3 if f in ("top_pending", "async_top_off") else 1)]
        self.cells = [cells[i] for i in self.rng.permutation(len(cells))]      # this seed's order through the pairs
        self.next_cell = 0

    def fresh(self):
        self.n_theta += 1
        return self.n_theta

    def key(self):
        self.n_key += 1
        return self.n_key

    def make(self, label, tid=None):
        """A concrete operation of the kind `label` ('factor1', 'sample_ll', 'factor1_same', ...)."""
        r, m = self.rng, self.m
        base, want = label, None
        for suffix in ("_same", "_other"):
            if label.endswith(suffix):
                base, want = label[: -len(suffix)], suffix[1:]
        slot = None
        name = base
        if base[-1] in "01" and base[:-1] in ("factor", "enqueue", "begin", "loglik", "sample_ll", "sweep_begin", "get_comps", "get_block", "ahead"):
            name, slot = base[:-1], int(base[-1])
        if name in ("sample_ll", "sweep_begin", "loglik") and slot is None:
            slot = int(r.integers(2)) if m.ok[1] else 0
        if name == "ahead":
            return Op("ahead", arg=int(r.integers(2)) if slot is None else slot)
        if name in ("factor", "enqueue", "begin"):
            if tid is None:
                x = r.random()
                if want == "same" and m.top is not None:
                    tid = m.top[1]
                elif want == "other" or x < 0.6 or m.tid[slot] is None:
                    tid = "fresh"
                elif x < 0.8:
                    tid = m.tid[slot]                      # the theta already in the slot
                else:
                    tid = BAD
                if want == "other" and m.top is not None and r.random() < 0.3:
                    tid = BAD if m.top[1] != BAD else "fresh"
            return Op(name, slot=slot, tid=tid)
        if name in SWEEPS or name in ("set_w", "set_beta", "set_tausq", "yhat"):
            return Op(name, slot=slot, key=self.key())
        if name == "get_block":
            return Op(name, slot=slot, u=BLOCKS[int(r.integers(len(BLOCKS)))])
        return Op(name, slot=slot)

    def emit(self, op):
        if op.tid == "fresh":
            op = op._replace(tid=self.fresh())
        cls = self.m.classify(op)
        assert cls != UNSPECIFIED
        self.ops.append(op)
        if cls != REFUSED:
            self.m.apply(op)
        return cls

    def put(self, label, tid=None, guard=6):
        """Emits `label`, with repairs in front where it would be UNSPECIFIED; a REFUSED outcome is emitted as it is."""
        for _ in range(guard):
            op = self.make(label, tid)
            probe = op._replace(tid=10 ** 6) if op.tid == "fresh" else op
            if self.m.classify(probe) != UNSPECIFIED:
                return self.emit(op)
            self.emit(self.m.repair(op))
        return None

    def refused_one(self):
        """A deliberately refused call: one that the model refuses in the current state."""
        order = self.rng.permutation(len(ANY))
        for i in order:
            op = self.make(ANY[i])
            if op.name == "get_block" and op.u == "empty" and self.rng.random() < 0.7:
                continue
            probe = op._replace(tid=10 ** 6) if op.tid == "fresh" else op
            if self.m.classify(probe) == REFUSED:
                return self.emit(op)
        return None

    def filler(self, pool):
        label = pool[int(self.rng.integers(len(pool)))]
        op = self.make(label)
        probe = op._replace(tid=10 ** 6) if op.tid == "fresh" else op
        if self.m.classify(probe) in (LEGAL, FAILS):
            self.emit(op)

    def close_all(self):
        if self.m.open is not None:
            self.emit(Op("finish"))
        if self.m.pending is not None:
            self.emit(Op("sweep_end"))

    def scenario(self):
        r, m = self.rng, self.m
        x = r.random()
        if x < 0.72:                                   # one (writer, reader) pair of a flag
            flag, (w, rd) = self.cells[self.next_cell % len(self.cells)]
            self.next_cell += 1
            if flag in ("leaf_pending", "slot_map", "d_resid", "gram_valid,s0_valid", "stats_valid", "z_valid", "top_pending", "async_top_off"):
                self.close_all()
            w_label = {"sweep": SWEEPS[int(r.integers(3))], "stats": ("beta_stats", "tausq_stats")[int(r.integers(2))],
                       "proposal": ("factor1", "enqueue1")[int(r.integers(2))],
                       "factorised": ("factor0", "factor1", "enqueue1")[int(r.integers(3))]}.get(w, w)
            if flag == "top_pending" and w == "begin1" and not m.ahead_on:
                self.emit(Op("ahead", arg=1))
            if flag == "c_pending" and w == "sweep_begin" and m.open is not None and r.random() < 0.7:
                self.emit(Op("finish"))
            self.put(w_label)
            if w_label == "enqueue1" and flag != "factor_open" and m.open is not None:
                if r.random() < 0.15:
                    self.refused_one()
                self.emit(Op("finish"))
            if w == "factorised" and m.open is not None:
                self.emit(Op("finish"))
            for _ in range(int(r.integers(0, 3))):
                if r.random() < 0.30:
                    self.refused_one()
                else:
                    pool = IN_OPEN if m.open is not None else IN_PENDING if m.pending is not None else \
                        ["get_w", "get_resid", "get_comps0", "yhat", "set_tausq", "ahead", "get_block0", "loglik0"]
                    if flag in ("stats_valid", "gram_valid,s0_valid", "d_resid", "top_pending", "leaf_pending"):
                        pool = ["get_w", "get_comps0", "yhat", "set_tausq", "get_block0"]
                        if flag == "top_pending":
                            pool = ["get_w", "yhat", "set_tausq", "tausq_stats", "sample"]
                    self.filler(pool)
            r_label = {"stats": ("beta_stats", "tausq_stats")[int(r.integers(2))], "proposal": ("factor1", "enqueue1")[int(r.integers(2))]}.get(rd, rd)
            same = None
            if flag == "top_pending" and rd.endswith("_same") and m.top is not None:
                same = m.top[1]
            self.put(r_label, tid=same)
        elif x < 0.80:                                 # a factorisation in two halves with calls in between
            self.put("enqueue1")
            for _ in range(int(r.integers(0, 4))):
                if r.random() < 0.2:
                    self.refused_one()
                else:
                    self.filler(IN_OPEN)
            if m.open is not None:
                self.emit(Op("finish"))
        elif x < 0.90:                                 # a sweep in two halves with calls in between
            self.put("sweep_begin")
            for _ in range(int(r.integers(0, 4))):
                y = r.random()
                if y < 0.15:
                    self.refused_one()
                elif y < 0.5 and m.open is None:
                    self.put("enqueue1")
                elif y < 0.65 and m.open is not None:
                    self.emit(Op("finish"))
                else:
                    self.filler(IN_OPEN if m.open is not None else IN_PENDING)
            if r.random() < 0.7:
                self.close_all()
        else:                                          # the C++ driver's iteration (step_w_theta, draw_tausq_beta)
            self.close_all()
            if not m.ok[0]:
                self.put("factor0", tid="fresh")
            tid = BAD if r.random() < 0.2 else self.fresh()
            self.emit(Op("begin", slot=1, tid=tid))
            self.emit(Op("sweep_begin", slot=0, key=self.key()))
            self.emit(Op("enqueue", slot=1, tid=tid))
            self.emit(Op("tausq_stats")); self.emit(Op("set_tausq", key=self.key()))
            self.emit(Op("beta_stats")); self.emit(Op("set_beta", key=self.key()))
            self.emit(Op("finish")); self.emit(Op("sweep_end"))
            if tid != BAD and r.random() < 0.6:
                self.emit(Op("swap"))
            if r.random() < 0.6:
                self.emit(Op("predict"))

    def run(self):
        self.emit(Op("factor", slot=0, tid=0))         # every sequence starts from a factorised accepted slot
        while len(self.ops) < self.n_ops:
            self.scenario()
        self.close_all()
        return self.ops


def generate(seed, has_ahead, n_ops=40):
    return Generator(seed, has_ahead, n_ops).run()


# ---- the trees and the committed (tree, seed) list
def _strip(nx, ny, q, **kw):
    from tests.util import make_problem, strip_coords
    coords, mv = strip_coords(nx, ny, q)
    return make_problem(coords=coords, mv_id=mv, q=q, seed=11, K=(2, 1), **kw)


def _grid(**kw):
    from tests.util import make_problem
    return make_problem(**kw)


QUAD_MIN = {"SPAMTREE_QUAD_MIN": "1"}
TREES = {}      # filled below: id -> dict(problem=callable, env, handle=kwargs of SpamTreeMV, has_ahead, seeds)


def block_handful(pb):
    """The fixed blocks of st_get_block: the root, one on the last reference level, one on the leaf level -- each the first
    with an observed row -- and the first block without one (None where the tree has none)."""
    labels = np.unique(pb["block_groups"])
    nobs = np.array([int(np.isfinite(pb["y"][ix]).sum()) for ix in pb["indexing"]])
    lvl = np.searchsorted(labels, pb["block_groups"])
    obs_levels = [g for g in range(labels.size) if np.any(nobs[lvl == g] > 0)]
    ref_levels = [g for g in obs_levels if pb["res_is_ref"][g] == 1]

    def first(g):
        return int(np.nonzero((lvl == g) & (nobs > 0))[0][0])
    empty = np.nonzero(nobs == 0)[0]
    return dict(root=first(obs_levels[0]), lastref=first(ref_levels[-1]), leaf=first(obs_levels[-1]),
                empty=int(empty[0]) if empty.size else None)


def bad_theta(pb):
    """A theta whose phase A fails, finite and out of range: at q = 1 a negative sigma^2 (the first entry, as in
    test_factor_in_two_halves_equals_st_factor); with more outcomes the first entry is a signed factor, so the range parameters
    phi_i go negative instead and the covariance grows with distance.  The oracle's errtype for it: oracle_phase_a_failure."""
    th = np.array(pb["theta"], dtype=np.float64)
    q = int(pb["q"])
    if q == 1:
        th[0] = -1.0
    else:
        th[2 * q: 3 * q] = -th[2 * q: 3 * q]     # phi_i < 0: the covariance grows with distance
    return th


class Inputs:
    """Every array a sequence hands to a call, a function of (tree, seed, key) only: all three executors see the same."""

    def __init__(self, pb, seed):
        self.pb, self.seed = pb, int(seed)
        self.n, self.p, self.q = int(pb["n"]), int(pb["p"]), int(pb["q"])
        self.theta0 = np.array(pb["theta"], dtype=np.float64)
        self.bad = bad_theta(pb)
        r = np.random.default_rng([self.seed, 0])
        self.w0 = r.standard_normal(self.n)
        self.beta0 = np.array([0.3, -0.2, 0.1, 0.25, -0.3, 0.7, -0.6, 0.4][: self.p])
        self.tausq0 = 0.2
        self.blocks = block_handful(pb)

    def theta(self, tid):
        if tid == BAD:
            return self.bad
        if tid == 0:
            return self.theta0
        r = np.random.default_rng([self.seed, 1000 + int(tid)])
        return self.theta0 * (1.0 + 0.05 * r.standard_normal(self.theta0.size))

    def normals(self, key):
        return np.random.default_rng([self.seed, 2000 + int(key)]).standard_normal(self.n)

    def beta(self, key):
        return np.asfortranarray(0.3 * np.random.default_rng([self.seed, 3000 + int(key)]).standard_normal((self.p, self.q)))

    def tausq_inv(self, key):
        return np.random.default_rng([self.seed, 4000 + int(key)]).uniform(2.0, 8.0, self.q)


# ---- executors: step(op, model) -> observation dict(rc=..., plus the values the call hands back)
def replay(ops, executor, has_ahead=True):
    """Runs `ops` on `executor`, the model beside it (an executor asks it for st_predict's theta_changed and skips what it
    does not run); returns the observations, None for an operation the executor skipped."""
    m = Model(has_ahead)
    out = []
    for op in ops:
        cls = m.classify(op)
        out.append(executor.step(op, m, cls))
        if cls != REFUSED:
            m.apply(op)
    return out


_dp = C.POINTER(C.c_double)


def _p(a):
    return a.ctypes.data_as(_dp)


class HipExecutor:
    """The library.  lazy=True: SpamTreeMV with its defaults, every call as the sequence names it.  lazy=False: cache_gram and
    defer_leaf off, the ahead-of-time path off, every factorisation a plain st_factor, every sweep st_sample_w followed by
    st_loglik_w, st_factor_begin and st_factor_ahead_enable skipped, refused calls skipped."""

    def __init__(self, inp, lazy, **handle_kw):
        from spamtree_amd.model import SpamTreeMV
        pb = inp.pb
        kw = dict(handle_kw) if lazy else dict(handle_kw, cache_gram=False, defer_leaf=False)
        self.inp, self.lazy = inp, lazy
        self.hm = SpamTreeMV(pb["y"], pb["X"], pb["Z"], pb["coords"], pb["mv_id"], pb["blocking"], pb["gix_block"], pb["res_is_ref"],
                             pb["parents"], pb["children"], pb.get("limited_tree", False), pb["block_names"], pb["block_groups"],
                             pb["indexing"], inp.w0, inp.beta0, inp.theta0, 1.0 / inp.tausq0, **kw)
        self.lib, self.h = self.hm.lib, self.hm.h
        if not lazy:
            assert self.lib.st_factor_ahead_enable(self.h, 0) == 0
        self.stash_factor = self.stash_sweep = None

    def close(self):
        self.hm.close()

    def _factor(self, slot, tid):
        th = np.ascontiguousarray(self.inp.theta(tid))
        ll = C.c_double()
        rc = self.lib.st_factor(self.h, slot, _p(th), th.size, C.byref(ll))
        return dict(rc=rc, ll=ll.value) if rc == 0 else dict(rc=rc)

    def _loglik(self, slot):
        ll = C.c_double()
        rc = self.lib.st_loglik_w(self.h, slot, C.byref(ll))
        return dict(rc=rc, ll=ll.value) if rc == 0 else dict(rc=rc)

    def _sweep_plain(self, z, slot):
        rc = self.lib.st_sample_w(self.h, _p(z), 0, 0)
        if rc != 0 or slot is None:
            return dict(rc=rc)
        return self._loglik(slot)

    def snapshot(self, m):
        """Observers that change no lazy state of the handle (plain downloads): w unless a sweep is pending, the log-density
        components of the slots that are not being factorised, the stored residuals."""
        out = {}
        if m.pending is None:
            out["w"] = self.step(Op("get_w"), m, LEGAL)["w"]
        for s in (0, 1):
            if m.open != s:
                o = self.step(Op("get_comps", slot=s), m, LEGAL)
                out[f"logdet{s}"], out[f"loglik{s}"] = o["logdet"], o["loglik"]
        out["resid"] = self.step(Op("get_resid"), m, LEGAL)["resid"]
        return out

    def step(self, op, m, cls):
        lib, h, inp, n, s = self.lib, self.h, self.inp, op.name, op.slot
        if not self.lazy and (cls == REFUSED or n in ("begin", "ahead")):
            return None
        if n == "factor":
            o = self._factor(s, op.tid)
        elif n == "enqueue":
            if self.lazy:
                th = np.ascontiguousarray(inp.theta(op.tid))
                o = dict(rc=lib.st_factor_enqueue(h, s, _p(th), th.size))
            else:
                self.stash_factor = self._factor(s, op.tid)
                o = dict(rc=0)
        elif n == "finish":
            if self.lazy:
                ll = C.c_double()
                rc = lib.st_factor_finish(h, C.byref(ll))
                o = dict(rc=rc, ll=ll.value) if rc == 0 else dict(rc=rc)
            else:
                o = self.stash_factor
        elif n == "begin":
            th = np.ascontiguousarray(inp.theta(op.tid))
            o = dict(rc=lib.st_factor_begin(h, s, _p(th), th.size))
        elif n == "ahead":
            o = dict(rc=lib.st_factor_ahead_enable(h, int(op.arg)))
        elif n == "swap":
            o = dict(rc=lib.st_swap(h))
        elif n == "sample":
            o = dict(rc=lib.st_sample_w(h, _p(inp.normals(op.key)), 0, 0))
        elif n == "sample_ll":
            z = inp.normals(op.key)
            if self.lazy:
                ll = C.c_double()
                rc = lib.st_sample_w_loglik(h, _p(z), 0, 0, s, C.byref(ll))
                o = dict(rc=rc, ll=ll.value) if rc == 0 else dict(rc=rc)
            else:
                o = self._sweep_plain(z, s)
        elif n == "sweep_begin":
            z = inp.normals(op.key)
            if self.lazy:
                o = dict(rc=lib.st_sample_w_loglik_begin(h, _p(z), 0, 0, s))
            else:
                self.stash_sweep = self._sweep_plain(z, s)
                o = dict(rc=0)
        elif n == "sweep_end":
            if self.lazy:
                ll = C.c_double()
                rc = lib.st_sample_w_loglik_end(h, C.byref(ll))
                o = dict(rc=rc, ll=ll.value) if rc == 0 else dict(rc=rc)
            else:
                o = self.stash_sweep
        elif n == "loglik":
            o = self._loglik(s)
        elif n == "predict":
            o = dict(rc=lib.st_predict(h, m.theta_changed(inp.theta) if cls != REFUSED else 1))
        elif n == "set_w":
            o = dict(rc=lib.st_set_w(h, _p(inp.normals(op.key))))
        elif n == "set_beta":
            o = dict(rc=lib.st_set_beta(h, _p(inp.beta(op.key))))
        elif n == "set_tausq":
            o = dict(rc=lib.st_set_tausq_inv(h, _p(inp.tausq_inv(op.key))))
        elif n == "beta_stats":
            xty = np.zeros(inp.p * inp.q)
            o = dict(rc=lib.st_beta_stats(h, _p(xty)), xty=xty.reshape(inp.q, inp.p).T.copy())
        elif n == "tausq_stats":
            ssq = np.zeros(inp.q)
            o = dict(rc=lib.st_tausq_stats(h, _p(ssq), None), ssq=ssq)
        elif n == "yhat":
            out = np.zeros(inp.n)
            o = dict(rc=lib.st_yhat(h, _p(inp.normals(op.key)), 0, 0, _p(out)), yhat=out)
        elif n == "get_w":
            out = np.zeros(inp.n)
            o = dict(rc=lib.st_get_w(h, _p(out)), w=out)
        elif n == "get_comps":
            a, b = np.zeros(self.hm.n_blocks), np.zeros(self.hm.n_blocks)
            o = dict(rc=lib.st_get_comps(h, s, _p(a), _p(b)), logdet=a, loglik=b)
        elif n == "get_block":
            u = inp.blocks[op.u]
            mm, P, isref, nobs = C.c_int64(), C.c_int64(), C.c_int32(), C.c_int32()
            assert lib.st_block_dims(h, u, C.byref(mm), C.byref(P), C.byref(isref), C.byref(nobs)) == 0
            mm, P = mm.value, P.value
            N = np.zeros(mm * max(P, 1))
            Ri = np.zeros(mm * mm if isref.value else mm)
            o = dict(rc=lib.st_get_block(h, s, u, _p(N), _p(Ri)), N=N[: mm * P].reshape(P, mm).T.copy(),
                     Ri=Ri.reshape(mm, mm).T.copy() if isref.value else Ri)
        elif n == "get_resid":
            out = np.zeros(inp.n)
            o = dict(rc=lib.st_get_resid(h, _p(out), inp.n), resid=out)
        else:
            raise ValueError(n)
        if o["rc"] < 0:
            o = dict(rc=o["rc"], err=lib.st_last_error(h).decode())
        return o


class OracleExecutor:
    """oracle.spamtree_oracle.SpamTreeMV through tests.util.oracle_model: theta_update + get_loglik_comps_w, gibbs_sample_w,
    get_loglik_w, predict, accept_make_change, beta_tausq_stats, plain assignments for the setters.  Refused calls, st_factor_begin
    and st_factor_ahead_enable are skipped.  Its prediction always refreshes the prediction blocks' caches: the oracle keeps them
    per data object and only its own driver's call order keeps them current, while st_predict rebuilds H on every call."""

    def __init__(self, inp):
        from tests.util import oracle_model, per_outcome
        self.inp = inp
        self.om = oracle_model(inp.pb, theta=inp.theta0, beta=inp.beta0, tausq=inp.tausq0, w=inp.w0)
        self.per_outcome = per_outcome
        self.stash_factor = self.stash_sweep = None
        self.resid = None

    def close(self):
        pass

    def _data(self, slot):
        return self.om.param_data if slot == 0 else self.om.alter_data

    def _factor(self, slot, tid):
        om, d = self.om, self._data(slot)
        om.theta_update(d, self.inp.theta(tid))
        with np.errstate(all="ignore"):
            ok = om.get_loglik_comps_w(d)
        if not ok:
            return dict(rc=int(om.last_errtype))
        self.resid = self._resid(d)
        return dict(rc=0, ll=float(d.loglik_w))

    def _resid(self, d):
        """Ri_u (w_u - H_u w_pa) of the observed reference blocks at the rows of each (tests/test_gpu_gather_g.py); limited trees
        store another quantity, not restated here."""
        om = self.om
        if om.limited_tree:
            return None
        out = {}
        for u in range(om.n_blocks):
            if om.block_ct_obs[u] > 0 and om.block_is_reference[u]:
                r = om.w[om.indexing[u]].copy()
                if om.parents[u].size:
                    r -= d.w_cond_mean_K[u] @ om.w[om.parents_indexing[u]]
                out[u] = d.Rcc_invchol[u] @ r
        return out

    def _loglik(self, slot):
        d = self._data(slot)
        self.om.get_loglik_w(d)
        return dict(rc=0, ll=float(d.loglik_w))

    def _sweep(self, key, slot):
        self.om.gibbs_sample_w(self.inp.normals(key))
        return dict(rc=0) if slot is None else self._loglik(slot)

    def step(self, op, m, cls):
        om, inp, n, s = self.om, self.inp, op.name, op.slot
        if cls == REFUSED or n in ("begin", "ahead"):
            return None
        if n == "factor":
            return self._factor(s, op.tid)
        if n == "enqueue":
            self.stash_factor = self._factor(s, op.tid)
            return dict(rc=0)
        if n == "finish":
            return self.stash_factor
        if n == "swap":
            om.accept_make_change()
            return dict(rc=0)
        if n == "sample":
            return self._sweep(op.key, None)
        if n == "sample_ll":
            return self._sweep(op.key, s)
        if n == "sweep_begin":
            self.stash_sweep = self._sweep(op.key, s)
            return dict(rc=0)
        if n == "sweep_end":
            return self.stash_sweep
        if n == "loglik":
            return self._loglik(s)
        if n == "predict":
            om.predict(True)
            return dict(rc=0)
        if n == "set_w":
            om.w = inp.normals(op.key).copy()
            return dict(rc=0)
        if n == "set_beta":
            self.per_outcome(om, Bcoeff=inp.beta(op.key))
            return dict(rc=0)
        if n == "set_tausq":
            self.per_outcome(om, tausq=1.0 / inp.tausq_inv(op.key))
            return dict(rc=0)
        if n == "beta_stats":
            return dict(rc=0, xty=om.beta_tausq_stats()[0])
        if n == "tausq_stats":
            return dict(rc=0, ssq=om.beta_tausq_stats()[1])
        if n == "yhat":
            return dict(rc=0, yhat=om.XB + om.w + np.sqrt(1.0 / om.tausq_inv_long) * inp.normals(op.key))
        if n == "get_w":
            return dict(rc=0, w=om.w.copy())
        if n == "get_comps":
            d = self._data(s)
            return dict(rc=0, logdet=d.logdetCi_comps.copy(), loglik=d.loglik_w_comps.copy())
        if n == "get_block":
            d, u = self._data(s), inp.blocks[op.u]
            Ri = d.Rcc_invchol[u] if om.block_is_reference[u] else d.ccholprecdiag[u]
            return dict(rc=0, H=np.array(d.w_cond_mean_K[u]) if om.parents[u].size else None, Ri=np.array(Ri))
        if n == "get_resid":
            return dict(rc=0, resid=self.resid)
        raise ValueError(n)


def describe(ops, has_ahead, upto=None):
    """One line per operation with the model's flags before it."""
    m = Model(has_ahead)
    lines = []
    for i, op in enumerate(ops if upto is None else ops[: upto + 1]):
        cls = m.classify(op)
        lines.append(f"{i:3d} {show(op):34s} {cls:8s} | {m.flags()}")
        if cls != REFUSED:
            m.apply(op)
    return "\n".join(lines)


def _register(tid, problem, env, handle, has_ahead, seeds):
    TREES[tid] = dict(problem=problem, env=env, handle=handle, has_ahead=has_ahead, seeds=list(seeds))


# a: the tree of test_four_ways_to_run_the_sweep_are_bitwise_identical (k_factor_quad reference and leaf levels under a root that
#    runs ahead of time: the only tree here with such levels, hence its longer seed list);
# b: its shape with two outcomes and 30 % of the rows missing -- 40-row blocks, so k_factor_bigmfma, k_factor_lchain +
#    k_factor_ref_finish and k_gram_big;
# c: config #4's strip of tests/test_gpu_deep.py (strip_coords(nx, 10, 3), sibling groups forced) cut to nx = 46 and three
#    levels: k_factor_wide on the reference levels, the generic kernel on a 209-row leaf level, k_gram_big;
# d: tree a on the generic kernels (k_factor, k_sample, d_s0 and s0_valid);
# e: tree a as a limited tree (the marginal chain's use of d_resid; no leaf deferral, no levels ahead).
# The seeds: tests/test_protocol_sequences_cpu.py checks that their union meets the coverage condition.
WIDE_GROUPS = {"SPAMTREE_LCHAIN": "0", "SPAMTREE_LCHAIN_REF": "0", "SPAMTREE_WIDE": "2"}
_register("a", lambda: _grid(side=25, q=1, seed=21, missing=0.1), QUAD_MIN, {}, True, [236, 1, 14, 49, 233, 120, 104, 107])
_register("b", lambda: _grid(side=25, q=2, seed=21, missing=0.3), QUAD_MIN, {}, False, [10, 302, 147, 0, 2, 3])
_register("c", lambda: _strip(46, 10, 3, tree_depth=3, missing=0.1), WIDE_GROUPS, {}, False, [187, 386, 99, 4, 5, 6])
_register("d", lambda: _grid(side=25, q=1, seed=21, missing=0.1), QUAD_MIN, dict(force_generic=True), False, [191, 88, 7, 8, 9, 11])
_register("e", lambda: _grid(side=25, q=1, seed=21, missing=0.1, limited_tree=True), QUAD_MIN, {}, False, [160, 40, 12, 13, 15, 16])


def cases():
    return [(t, s) for t in TREES for s in TREES[t]["seeds"]]


def sequence(tree, seed):
    return generate(seed, TREES[tree]["has_ahead"])


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--tree", required=True, choices=sorted(TREES))
    ap.add_argument("--seed", type=int, required=True)
    ap.add_argument("--upto", type=int, default=None, help="index of the last operation to print")
    a = ap.parse_args()
    print(f"tree {a.tree} seed {a.seed} env {TREES[a.tree]['env']} handle {TREES[a.tree]['handle']}")
    print(describe(sequence(a.tree, a.seed), TREES[a.tree]["has_ahead"], a.upto))
