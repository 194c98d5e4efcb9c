"""A host-side model of the call contract of the new-point family (st_points_*, include/spamtree_hip.h), a seeded generator of
call sequences that walks it, and a NumPy executor of the contract.  Pure Python and NumPy: nothing here needs a GPU or the library.

One point set carries five optional riders -- the functionals, the scores, the Rao-Blackwellised exceedance thresholds, the
mixture store and the stored draws of st_points_summary_reserve -- each with its own rules for what a set, a replacement, a
reservation, a reset and a new point set do to it.  The model holds only what a caller can know:
  the kind of the current point set (none; plain with X; plain without X; joint with X; empty, n_new = 0; single, n_new = 1),
  whether slot 0 is factorised,
  per rider whether it is present and its parameters, and
  per store THE LIST OF ACCUMULATE IDS IT HAS SEEN OR HOLDS.  Every successful st_points_accumulate(_joint) takes the next id.
  There are the Welford summaries (seen), the pair accumulators of a joint set (pair), the stored point draws (store), the
  functionals' accumulators and stored draws, the scores' state, the thresholds' state, and the point and functional columns
  of the mixture store.
`Model.classify` puts every operation in every state into one of
  LEGAL        returns 0 and does what the header says;
  REFUSED      the negative code and a fragment of the st_last_error text; the state stays as it was;
  UNSPECIFIED  the header defines no result: the generator never emits these.
The `Contract` executor turns the per-draw outputs of every accumulate (w_new, cond_mean, cond_var or the packed cond_cov,
yhat_new, beta and tausq_inv at that moment, and the functionals' values of that iteration where the header defines a read from
them) into every read, by the header's definitions in float64, over exactly the ids the model lists.

Decisions where the header was silent or said something else than the code (the header now says the same):
  * a reserved draw is stored at the store's own count: the store holds the first `keep` draws since the latest of st_points_set,
    st_points_summary_reset and st_points_summary_reserve -- not "row n_accumulated", which runs on over a reservation;
  * the functionals' stored draws have a count of their own: the first `keep` since the latest of those and st_points_functionals_set;
  * a functional column of the mixture store is written only on an iteration that writes a point column: functionals set after the
    point columns are full never get a column;
  * a point set of size 0 has no X, whatever was passed: scores on it are refused like on any set without X;
  * st_points_summary_get and _get_cov before the first accumulated iteration are ST_ERR_USAGE (n_accumulated is still written).

    python -m tests.points_model --set joint --seed 3 --upto 17

prints the first 18 operations (indices 0 .. 17) of that sequence with the model's state before each: the prefix a failure message
of tests/test_gpu_points_sequences.py names.
"""
from __future__ import annotations

import argparse
import collections
import math
from types import SimpleNamespace as NS

import numpy as np

LEGAL, REFUSED, UNSPECIFIED = "legal", "refused", "unspecified"
ST_ERR_USAGE, ST_ERR_UNSUPPORTED = -1, -4
N_POINTS = 37                                   # a multiple of nothing in the kernels
KINDS = {"plainX": (N_POINTS, True, False), "plain": (N_POINTS, False, False), "joint": (N_POINTS, True, True),
         "empty": (0, False, False), "single": (1, True, False)}      # kind -> (n_new, has X, joint)
FAMILIES = tuple(KINDS)
SUMMARY_KEEPS, MIX_KEEPS = (0, 2, 5), (0, 3, 6)
SUMMARY_MAX, MIX_MAX = 16384, 8192
EXCEED_SPECS = ((1, False), (1, True), (3, False), (3, True))   # (n_thr, with thr_fun)
PROBS = (0.9, 0.1, 0.5)                                         # st_points_mixture_quantiles, in no order
ACC_SEED = 9

Op = collections.namedtuple("Op", "name arg", defaults=(None,))

CHAIN = ("sweep", "beta", "tausq", "theta")
READS = ("get", "get_cov", "layout", "fun_get", "fun_last", "fun_info", "fun_quantile", "score_get", "exceed_get", "mix_draws",
         "mix_quantiles", "mix_crps", "mix_info")
RIDER_READS = {"fun": ("fun_get", "fun_last", "fun_quantile"), "score": ("score_get",), "exceed": ("exceed_get",),
               "mix": ("mix_draws", "mix_quantiles", "mix_crps"), "summary": ("get", "squantile")}
# the refusals the header names, by the name the coverage test knows them under
REFUSALS = ("before_set", "score_without_X", "thr_fun_without_functionals", "fun_w_after_replacement", "crps_without_draw",
            "lpd_joint_on_plain", "accj_on_plain", "infinite_y", "n_thr_9", "summary_keep_beyond", "mix_keep_beyond", "point_twice")


def show(op):
    return op.name if op.arg is None else f"{op.name}({op.arg})"


def solo_keeps(rider, op):
    """Whether the solo replay of ``rider`` keeps ``op``: the chain, the point sets, the accumulates, the resets, the rider's own
    operations and its prerequisites (the functionals for the functional parts of thresholds and store, the scores for the exact
    CRPS, the reservation for quantiles and the empirical CRPS)."""
    n = op.name
    if n in CHAIN or n in ("set", "reset", "acc", "accj"):
        return True
    own = {"summary": ("reserve", "squantile", "get", "get_cov", "layout"),
           "fun": ("fun", "reserve", "fun_get", "fun_last", "fun_info", "fun_quantile"),
           "score": ("score", "reserve", "score_get"),
           "exceed": ("exceed", "fun", "exceed_get"),
           "mix": ("mix", "fun", "score", "mix_draws", "mix_quantiles", "mix_crps", "mix_info")}[rider]
    return n in own


RIDERS = ("summary", "fun", "score", "exceed", "mix")


class Model:
    """The state a caller can know, and what every operation does to it.  The hooks (on_*) are what the wrong variants of
    tests/test_points_model_cpu.py override."""

    def __init__(self):
        self.kind, self.factor, self.next_id = None, False, 0
        self.chain_id, self.acc_chain = 0, {}       # how often w or theta changed; and that count at every accumulate: two accumulates
        self._new_set()                             # without a change between them have the same conditional moments

    def _new_set(self):
        self.seen, self.pair, self.keep, self.store = [], [], 0, []
        self.fun = self.score = self.exceed = self.mix = None
        self.dirty = False              # st_points_predict or st_points_summary_quantile wrote the outputs' buffer since the last accumulate

    n = property(lambda self: KINDS[self.kind][0] if self.kind else 0)
    has_X = property(lambda self: bool(self.kind) and KINDS[self.kind][1])
    joint = property(lambda self: bool(self.kind) and KINDS[self.kind][2])

    # ---- classification -------------------------------------------------------------------------------------------------
    def classify(self, op):
        """(LEGAL, 0, None), (REFUSED, code, text fragment) or (UNSPECIFIED, None, None)."""
        n, a = op.name, op.arg
        ok, unspec = (LEGAL, 0, None), (UNSPECIFIED, None, None)

        def no(frag, code=ST_ERR_USAGE):
            return (REFUSED, code, frag)
        if n in CHAIN:
            return unspec if (n == "sweep" and not self.factor) else ok
        if n in ("set", "fun_info", "mix_info"):
            return ok
        if n == "accj" and self.kind and not self.joint:
            return no("st_points_accumulate_joint before st_points_set_joint")
        if n == "layout":
            return ok if self.joint else no("st_points_joint_layout before st_points_set_joint")
        if not self.kind:
            return no("before st_points_set")
        if n in ("acc", "accj", "predict"):
            return ok if self.factor else no("before st_factor(slot 0)")
        if n == "reset":
            return ok
        if n == "reserve":
            return no("at most 16384", ST_ERR_UNSUPPORTED) if a > SUMMARY_MAX else ok
        if n == "mix":
            return no("beyond ST_MIX_MAX_DRAWS", ST_ERR_UNSUPPORTED) if a > MIX_MAX else ok
        if n == "fun":
            if a == "dup":
                return no("occurs twice in the functional") if self.n > 0 else unspec
            return ok
        if n == "score":
            if a is None:
                return ok
            if not self.has_X:
                return no("the scores need the regressors X")
            return no("is infinite") if a == "inf" else ok
        if n == "exceed":
            if a is None:
                return ok
            if a[0] == 9:
                return no("n_thr = 9 must lie in 1 .. 8")
            return no("thr_fun before st_points_functionals_set") if (a[1] and not self.fun) else ok
        if n == "squantile":
            return ok if self.store else no("no draw stored")
        if n == "get":
            return ok if self.seen else no("no iteration accumulated")
        if n == "get_cov":
            if not self.joint:
                return no("st_points_summary_get_cov before st_points_set_joint")
            return ok if self.seen else no("no iteration accumulated")
        if n in ("fun_get", "fun_last", "fun_quantile"):
            if not self.fun:
                return no("before st_points_functionals_set")
            if n == "fun_quantile":
                return ok if self.fun.store else no("no draw stored")
            return ok if self.fun.seen else no("no iteration accumulated")
        if n == "score_get":
            crps, lpdj = a
            if not self.score:
                return no("st_points_score_get before st_points_score_set")
            if self.score.n_scored == 0:
                return no("no point is scored")
            if not self.score.seen:
                return no("no iteration accumulated")
            if crps and not self.store:
                return no("crps needs a stored draw")
            return no("lpd_joint before st_points_set_joint") if (lpdj and not self.joint) else ok
        if n == "exceed_get":
            if not self.exceed:
                return no("st_points_exceed_get before st_points_exceed_set")
            if not self.exceed.seen:
                return no("no iteration accumulated")
            return no("fun_w without functional thresholds") if (a and not (self.exceed.fun and self.fun)) else ok
        if n in ("mix_draws", "mix_quantiles", "mix_crps"):
            if not self.mix:
                return no("before st_points_mixture_reserve")
            if n == "mix_draws":
                return ok
            if n == "mix_quantiles":
                if a and not self.fun:
                    return no("fun_w before st_points_functionals_set")
                return no("no stored draw") if (not self.mix.cols or (a and self.n > 0 and not self.mix.fcols)) else ok
            if not self.score:
                return no("st_points_mixture_crps before st_points_score_set")
            if self.score.n_scored == 0:
                return no("no point is scored")
            return ok if self.mix.cols else no("no stored draw")
        raise ValueError(op)

    def refusal_name(self, op):
        """Which of REFUSALS a refused ``op`` is in this state (None: one the list does not name)."""
        n = op.name
        frag = self.classify(op)[2] or ""
        if not self.kind and "before st_points_set" in frag and n not in ("layout",):
            return "before_set"
        return {("score", "the scores need"): "score_without_X", ("exceed", "thr_fun before"): "thr_fun_without_functionals",
                ("exceed_get", "fun_w without"): "fun_w_after_replacement", ("score_get", "crps needs"): "crps_without_draw",
                ("score_get", "lpd_joint before"): "lpd_joint_on_plain", ("accj", "st_points_accumulate_joint before"): "accj_on_plain",
                ("score", "is infinite"): "infinite_y", ("exceed", "n_thr = 9"): "n_thr_9", ("reserve", "at most"): "summary_keep_beyond",
                ("mix", "beyond ST_MIX"): "mix_keep_beyond", ("fun", "occurs twice"): "point_twice"}.get((n, _head(frag)))

    # ---- the counts a call writes ------------------------------------------------------------------------------------------
    def counts(self, op):
        """What the call writes into its count arguments, from the state BEFORE it (reads change nothing); a refused read writes
        the counts that come before its refusal."""
        n = op.name
        if not self.kind and n not in ("fun_info", "mix_info"):
            return {}
        if n == "get":
            return dict(n_accumulated=len(self.seen))
        if n == "fun_get" and self.fun:
            return dict(n_accumulated=len(self.fun.seen))
        if n == "fun_info":
            return dict(n_fun=self.fun.n_fun if self.fun else 0)
        if n == "score_get" and self.score:
            return dict(n_scored=self.score.n_scored)
        if n == "exceed_get" and self.exceed:
            return dict(n_accumulated=len(self.exceed.seen))
        if n == "mix_draws" and self.mix:
            return dict(n_stored=len(self.mix.cols))
        if n == "mix_info":
            return dict(keep=self.mix.keep if self.mix else 0, n_stored=len(self.mix.cols) if self.mix else 0)
        if n == "mix_crps" and self.mix and self.score:
            return dict(n_scored=self.score.n_scored)
        return {}

    # ---- transitions -------------------------------------------------------------------------------------------------------
    def apply(self, op):
        """The state after a LEGAL ``op``; an accumulate returns its id."""
        n, a = op.name, op.arg
        if n in ("theta", "sweep"):
            self.factor = self.factor or n == "theta"
            self.chain_id += 1
        elif n == "set":
            self.kind = a
            self._new_set()
        elif n == "reset":
            self.seen, self.store = [], []
            self.on_reset()
        elif n == "reserve":
            self.store, self.keep = [], (a if self.n > 0 else 0)
            self.on_reserve()
            if self.fun:
                self.fun.store = []
        elif n == "fun":
            self.on_fun_set(a)
        elif n == "score":
            self.score = self.on_replace("score", None if a is None else NS(y=a, n_scored=0 if a == "allnan" else Inputs.n_scored(self.kind), seen=[]))
        elif n == "exceed":
            self.exceed = self.on_replace("exceed", None if a is None else NS(n_thr=a[0], fun=a[1], seen=[]))
        elif n == "mix":
            self.mix = self.on_replace("mix", None if a == 0 else NS(keep=a, cols=[], fcols=[], n_fun=self.fun.n_fun if (self.fun and self.n > 0) else 0))
        elif n in ("acc", "accj"):
            return self.on_accumulate()
        elif n in ("predict", "squantile"):
            self.dirty = True
        return None

    def refuse(self, op):
        """A refused call changes nothing (the variant that breaks this overrides it)."""

    def on_reset(self):
        self.pair = []
        if self.score:
            self.score.seen = []
        if self.exceed:
            self.exceed.seen = []
        if self.mix:
            self.mix.cols, self.mix.fcols = [], []
        if self.fun:
            self.fun.seen, self.fun.store = [], []

    def on_reserve(self):
        pass

    def on_replace(self, rider, new):
        return new

    def on_fun_set(self, a):
        if self.exceed:
            self.exceed.fun = False
        new = None if a is None else NS(name=a, n_fun=Inputs.n_fun(a), seen=[], store=[])
        self.fun = self.on_replace("fun", new)
        if self.mix:
            self.mix.fcols, self.mix.n_fun = [], (new.n_fun if (new and self.n > 0) else 0)

    def stored_rows(self):
        """The ids of the rows the stored-draw reads see."""
        return list(self.store)

    def on_accumulate(self):
        i = self.next_id
        self.next_id += 1
        self.acc_chain[i] = self.chain_id
        self.seen.append(i)
        if self.joint:
            self.pair.append(i)
        if len(self.store) < self.keep:
            self.on_store(i)
        if self.score:
            self.score.seen.append(i)
        if self.fun:
            self.fun.seen.append(self.fun_source(i))
            if len(self.fun.store) < self.keep:
                self.fun.store.append(self.fun_source(i))
        if self.exceed:
            self.exceed.seen.append(i)
        if self.mix:
            self.on_mix_step(i)
        self.dirty = False
        return i

    def on_store(self, i):
        self.store.append(i)

    def fun_source(self, i):
        return i

    def on_mix_step(self, i):
        mx = self.mix
        if len(mx.cols) >= mx.keep:
            return
        mx.cols.append(i)
        if mx.n_fun > 0 and self.fun and len(mx.fcols) < mx.keep:
            mx.fcols.append(i)

    # ---- for people ----------------------------------------------------------------------------------------------------------
    def flags(self):
        p = [f"set={self.kind}", f"factor={int(self.factor)}", f"seen={self.seen}", f"keep={self.keep} store={self.store}"]
        if self.joint:
            p.append(f"pair={self.pair}")
        if self.fun:
            p.append(f"fun={self.fun.name} seen={self.fun.seen} store={self.fun.store}")
        if self.score:
            p.append(f"score={self.score.y} seen={self.score.seen}")
        if self.exceed:
            p.append(f"exceed=T{self.exceed.n_thr}{'+fun' if self.exceed.fun else ''} seen={self.exceed.seen}")
        if self.mix:
            p.append(f"mix={self.mix.keep} cols={self.mix.cols} fcols={self.mix.fcols}")
        if self.dirty:
            p.append("scratch-dirty")
        return " ".join(p)


def _head(frag):
    for key in ("the scores need", "thr_fun before", "fun_w without", "crps needs", "lpd_joint before", "st_points_accumulate_joint before",
                "is infinite", "n_thr = 9", "at most", "beyond ST_MIX", "occurs twice"):
        if key in frag:
            return key
    return frag


# ---- the inputs of the operations: pure data, the same for every executor ------------------------------------------------------
class Inputs:
    """What the operations' arguments stand for.  ``n``: the size of the three big kinds (the CPU tests use a smaller one than the
    device's 37); ``pb``: the problem (tests.util.make_problem) -- with it the points get coordinates and anchors."""

    FUN_SIZES = {"A": 3, "B": 5}
    SCORED_EVERY = 4            # y 'nan': every fourth point is scored, from point 0

    def __init__(self, n=N_POINTS, q=2, p=2, pb=None, seed=0):
        self.n_big, self.q, self.p, self.pb = n, q, p, pb
        rng = np.random.default_rng([17, seed])
        sizes = []
        while sum(sizes) < n:
            sizes.append((3, 2, 1)[len(sizes) % 3])
        sizes[-1] -= sum(sizes) - n
        lab = np.concatenate([np.full(g, 100 + 7 * k) for k, g in enumerate(sizes)])
        # the members of a group need not be adjacent: the first members come first, then the second, then the third
        order = np.argsort(np.concatenate([np.arange(g) for g in sizes]), kind="stable")
        self.rank_in_group = np.concatenate([np.arange(g) for g in sizes])[order]
        self.labels = lab[order].astype(np.int64)
        self.mv = ((self.rank_in_group + (self.labels // 7)) % q + 1).astype(np.int64)
        self.X = rng.standard_normal((n, p))
        self.coords = self.anchor = self.anchor_joint = None
        if pb is not None:
            self._place(rng)
        self.y = {}
        y = np.full(n, np.nan)
        y[::self.SCORED_EVERY] = 1.5 * rng.standard_normal(y[::self.SCORED_EVERY].size)
        self.y["nan"] = y
        self.y["allnan"] = np.full(n, np.nan)
        yi = y.copy()
        yi[0] = np.inf
        self.y["inf"] = yi
        self._chain = np.random.default_rng([18, seed])
        self.betas = [np.asfortranarray(self._chain.standard_normal((p, q))) for _ in range(8)]
        self.tausq_invs = [1.0 / self._chain.uniform(0.05, 0.5, q) for _ in range(8)]
        self.fw = np.random.default_rng([19, seed]).standard_normal(n)

    def _place(self, rng):
        """Coordinates: the members of a group sit within a cell of each other; the third member of the first group of three repeats
        its first (the zero-pivot rule); three single points sit on rows of their own conditioning set."""
        from spamtree_amd.predict import conditioning_set, locate
        pb, n = self.pb, self.n_big
        topo = pb["topo"]
        lo, hi = pb["coords"].min(axis=0), pb["coords"].max(axis=0)
        sites = {}
        pts = np.zeros((n, 2))
        for i in range(n):
            c = sites.setdefault(int(self.labels[i]), lo + (hi - lo) * rng.uniform(0.05, 0.95, size=2))
            pts[i] = c + 0.01 * (hi - lo) * self.rank_in_group[i]
        g0 = np.nonzero(self.labels == self.labels[0])[0]
        pts[g0[2]], self.mv[g0[2]] = pts[g0[0]], self.mv[g0[0]]
        singles = [k for k in np.unique(self.labels) if np.sum(self.labels == k) == 1][:3]
        self.on_rows = []
        for k in singles:
            i = int(np.nonzero(self.labels == k)[0][0])
            b = int(locate(topo, pts[i:i + 1], self.mv[i:i + 1])[0])
            rows = np.concatenate([topo.indexing(int(u)) for u in conditioning_set(topo, b)])
            r = int(rows[-1])
            pts[i], self.mv[i] = topo.coords[r], topo.mv_id[r]
            b2 = int(locate(topo, pts[i:i + 1], self.mv[i:i + 1])[0])
            if r in np.concatenate([topo.indexing(int(u)) for u in conditioning_set(topo, b2)]):
                self.on_rows.append((i, r))
        self.coords = pts
        self.anchor = locate(topo, pts, self.mv)
        self.anchor_joint = locate(topo, pts, self.mv, joint=self.labels)

    # -- the point sets
    def size(self, kind):
        return {"empty": 0, "single": 1}.get(kind, self.n_big)

    def points(self, kind):
        """dict(n, mv, X or None, labels or None, coords, anchor) of a kind."""
        n = self.size(kind)
        _, has_X, joint = KINDS[kind]
        d = dict(n=n, mv=self.mv[:n].copy(), X=self.X[:n].copy() if has_X else None, labels=self.labels[:n].copy() if joint else None,
                 coords=None, anchor=None)
        if self.coords is not None:
            d["coords"] = self.coords[:n].copy()
            d["anchor"] = (self.anchor_joint if joint else self.anchor)[:n].copy()
        return d

    def groups(self, kind):
        """The joint groups of a kind in layout order (first appearance), members in the caller's order, and the packed offsets."""
        if not KINDS[kind][2]:
            return [], np.zeros(1, dtype=np.int64)
        lab = self.labels[:self.size(kind)]
        first = {}
        for i, k in enumerate(lab):
            first.setdefault(int(k), []).append(i)
        groups = [np.array(v, dtype=np.int64) for v in first.values()]
        return groups, np.concatenate([[0], np.cumsum([g.size ** 2 for g in groups])]).astype(np.int64)

    # -- the riders' arguments
    @staticmethod
    def n_fun(name):
        return Inputs.FUN_SIZES[name]

    @staticmethod
    def n_scored(kind, n=None):
        n = KINDS[kind][0] if n is None else n
        return len(range(0, n, Inputs.SCORED_EVERY))

    def functionals(self, kind, name):
        """The rows [(idx, wt)] of set A (3 functionals) or B (5): neither is a prefix of the other.  On the big kinds one row of each
        spans a whole joint group plus other points; one row is empty.  'dup' names point 0 twice."""
        n = self.size(kind)
        e = (np.zeros(0, dtype=np.int64), np.zeros(0))
        if name == "dup":
            return [(np.array([0, 0]), np.array([1.0, 1.0]))]
        if n == 0:
            return [e] * self.n_fun(name)
        if n == 1:
            one = lambda w: (np.array([0]), np.array([w]))   # noqa: E731
            return [one(1.0), one(-2.0), e] if name == "A" else [one(0.5), e, one(3.0), one(1.0), e]
        lab = self.labels[:n]
        g0 = np.nonzero(lab == lab[0])[0]
        g1 = np.nonzero(lab == lab[1])[0]
        rest0 = np.setdiff1d(np.arange(n), g0)[::3]
        rest1 = np.setdiff1d(np.arange(n), g1)[1::4]
        w = self.fw
        if name == "A":
            i0 = np.concatenate([g0, rest0])
            return [(i0, w[:i0.size] + 2.0), (np.array([0, n - 1]), np.array([1.0, -1.0])), e]
        i1 = np.concatenate([g1, rest1])
        return [(np.arange(n), np.full(n, 1.0 / n)), (np.arange(0, n, 2), w[:(n + 1) // 2]), (np.array([min(3, n - 1)]), np.array([2.0])),
                e, (i1, 0.5 * w[:i1.size] - 1.0)]

    def y_new(self, kind, name):
        return self.y[name][:self.size(kind)].copy()

    def thresholds(self, n_thr):
        """(thr n_thr x q, side n_thr): mixed sides."""
        base, side = {1: ([0.1], [-1]), 3: ([-0.5, 0.2, 1.0], [-1, 1, 1]), 9: ([0.1 * t for t in range(9)], [1] * 9)}[n_thr]
        return np.array([[b + 0.1 * j for j in range(self.q)] for b in base]), np.array(side, dtype=np.int32)

    def thresholds_fun(self, n_thr, n_fun):
        return np.array([[0.1 * (t + 1) - 0.05 * f for f in range(n_fun)] for t in range(n_thr)])


# ---- the generator ------------------------------------------------------------------------------------------------------------
class Generator:
    """Walks the model from a seed: legal operations, and with a small probability a refused one followed by reads of the rider it
    was about (they must show the state unchanged)."""

    def __init__(self, family, seed, n_ops=80):
        self.rng = np.random.default_rng([FAMILIES.index(family), seed])
        self.family, self.n_ops = family, n_ops
        self.m, self.ops, self.queue = Model(), [], []

    def pick(self, items, weights=None):
        w = np.ones(len(items)) if weights is None else np.asarray(weights, dtype=np.float64)
        return items[int(self.rng.choice(len(items), p=w / w.sum()))]

    def emit(self, op):
        cls = self.m.classify(op)[0]
        assert cls != UNSPECIFIED, (op, self.m.flags())
        self.ops.append(op)
        if cls == LEGAL:
            self.m.apply(op)
        return cls

    def legal_read(self, name):
        """The read ``name`` with the arguments that are legal now, or None."""
        m = self.m
        if name == "score_get":
            op = Op(name, (bool(m.store), m.joint))
        elif name == "exceed_get":
            op = Op(name, bool(m.exceed and m.exceed.fun and m.fun))
        elif name == "mix_quantiles":
            op = Op(name, True)
            if m.classify(op)[0] != LEGAL:
                op = Op(name, False)
        elif name in ("squantile", "fun_quantile"):
            op = Op(name, self.pick([0.0, 0.3, 0.5, 1.0]))
        else:
            op = Op(name)
        return op if m.classify(op)[0] == LEGAL else None

    def refusals_now(self):
        """The header's refusals that the current state offers."""
        m, out = self.m, []
        out += [Op("reserve", SUMMARY_MAX + 1), Op("mix", MIX_MAX + 1), Op("exceed", (9, False))]
        if m.n > 0:
            out.append(Op("fun", "dup"))
        if m.has_X:
            out.append(Op("score", "inf"))
        else:
            out.append(Op("score", "nan"))
        if not m.fun:
            out.append(Op("exceed", (3, True)))
        if m.exceed and not (m.exceed.fun and m.fun) and m.exceed.seen:
            out.append(Op("exceed_get", True))
        if m.score and m.score.n_scored and m.score.seen:
            if not m.store:
                out.append(Op("score_get", (True, m.joint)))
            if not m.joint:
                out.append(Op("score_get", (bool(m.store), True)))
        if not m.joint:
            out += [Op("accj", True), Op("layout"), Op("get_cov")]
        for name, arg in (("fun_get", None), ("score_get", (False, False)), ("exceed_get", False), ("mix_draws", None), ("mix_crps", None),
                          ("get", None), ("squantile", 0.5), ("fun_quantile", 0.5)):
            if m.classify(Op(name, arg))[0] == REFUSED:
                out.append(Op(name, arg))
        return [op for op in out if m.classify(op)[0] == REFUSED]

    def reads_of(self, op):
        """After a refusal: the reads that show the rider it was about."""
        rider = {"reserve": "summary", "squantile": "summary", "get": "summary", "accj": "summary"}.get(op.name) or \
            next((r for r in ("fun", "score", "exceed", "mix") if op.name.startswith(r)), "summary")
        return [r for r in (self.legal_read(nm) for nm in RIDER_READS[rider]) if r is not None]

    def state_op(self):
        m = self.m
        missing = [r for r in ("fun", "score", "exceed", "mix") if getattr(m, r) is None and (r != "score" or m.has_X)]
        cands, w = [], []

        def add(op, weight):
            if m.classify(op)[0] == LEGAL:
                cands.append(op); w.append(weight)
        add(Op("reset"), 0.5)
        for k in SUMMARY_KEEPS:
            add(Op("reserve", k), 0.4 if k == 0 else (2.0 if m.keep == 0 else 0.8))
        for a in (None, "A", "B"):
            add(Op("fun", a), 0.4 if a is None else (2.5 if "fun" in missing else 1.0))
        if m.has_X:
            for a in (None, "nan", "allnan"):
                add(Op("score", a), {None: 0.3, "allnan": 0.3}.get(a, 2.5 if "score" in missing else 0.8))
        add(Op("exceed", None), 0.3)
        for spec in EXCEED_SPECS:
            add(Op("exceed", spec), (2.0 if "exceed" in missing else 0.6) * (1.5 if spec[1] else 1.0))
        for k in MIX_KEEPS:
            add(Op("mix", k), 0.3 if k == 0 else (2.5 if "mix" in missing else 0.7))
        add(Op("predict"), 1.0)
        return self.pick(cands, w)

    def run(self):
        rng, m = self.rng, self.m
        if rng.random() < 0.6:
            self.emit(self.pick([Op("reset"), Op("reserve", 2), Op("fun", "A"), Op("score", "nan"), Op("exceed", (1, False)), Op("mix", 3),
                                 Op("acc", True), Op("get"), Op("fun_get"), Op("score_get", (False, False)), Op("exceed_get", False), Op("mix_draws")]))
        self.emit(Op("set", self.family))
        if rng.random() < 0.3:
            self.emit(Op("acc", True))                       # before st_factor(slot 0)
        self.emit(Op("theta", 0))
        while len(self.ops) < self.n_ops:
            if self.queue:
                self.emit(self.queue.pop(0))
                continue
            r = rng.random()
            if r < 0.24:
                name = "accj" if (m.joint and rng.random() < 0.5) else "acc"
                if m.next_id and m.acc_chain[m.next_id - 1] == m.chain_id:      # w moves by O(1) between any two saved iterations
                    self.emit(Op("sweep", int(rng.integers(1, 1000))))
                self.emit(Op(name, bool(rng.random() < 0.7)))
            elif r < 0.34:
                self.emit(self.pick([Op("sweep", int(rng.integers(1, 1000))), Op("beta", int(rng.integers(8))), Op("tausq", int(rng.integers(8))),
                                     Op("theta", int(rng.integers(5)))], [3, 1, 1, 1]))
            elif r < 0.60:
                self.emit(self.state_op())
            elif r < 0.90:
                reads = [x for x in (self.legal_read(nm) for nm in READS + ("squantile",)) if x is not None]
                self.emit(self.pick(reads))
            elif r < 0.975:
                op = self.pick(self.refusals_now())
                self.emit(op)
                self.queue += self.reads_of(op)
            elif sum(getattr(m, x) is not None for x in ("fun", "score", "exceed", "mix")) + (m.keep > 0) >= (5 if m.has_X else 4) or rng.random() < 0.08:
                other = self.pick([k for k in FAMILIES if k != m.kind])
                self.emit(Op("set", other))
                self.queue += [Op("fun_get"), Op("score_get", (False, False)), Op("exceed_get", False), Op("mix_draws"), Op("squantile", 0.5)]
        return self.ops


def generate(family, seed, n_ops=80):
    return Generator(family, seed, n_ops).run()


# the committed seeds: tests/test_points_model_cpu.py asserts that their union meets the coverage conditions.  (family, seed,
# force_generic): one plain and one joint sequence run on the generic kernels.
SEEDS = {"plainX": [35, 61, 70, 0, 1], "plain": [65, 235, 0, 1], "joint": [4, 246, 0, 1, 2], "empty": [0, 1, 2, 3], "single": [145, 173, 0, 1]}
GENERIC = {("plainX", 61), ("joint", 246)}

# Named regression cases beside the seeded ones: the shortest failing prefix of anything the sequences exposed (none so far).
REGRESSIONS = {}


def cases():
    return [(f, s) for f in FAMILIES for s in SEEDS[f]] + [("regression", k) for k in REGRESSIONS]


def sequence(family, seed):
    return list(REGRESSIONS[seed]) if family == "regression" else generate(family, seed)


def describe(ops, upto=None, model=Model):
    """One line per operation with the model's state before it."""
    m = model()
    lines = []
    for i, op in enumerate(ops if upto is None else ops[: upto + 1]):
        cls, rc, frag = m.classify(op)
        lines.append(f"{i:3d} {show(op):28s} {cls + ('' if cls != REFUSED else f' {rc} <{frag}>'):60s} | {m.flags()}")
        if cls == LEGAL:
            m.apply(op)
    return "\n".join(lines)


# ---- the contract executor ------------------------------------------------------------------------------------------------------
def fun_values(rows, rec, groups, offsets):
    """F_w, F_m, F_v, F_y of one draw by the header's definition: a'w, a'cond_mean, sum_groups a_g' Sigma_g a_g (a plain set:
    sum a_i^2 cond_var_i; the sum clamped at 0), a'yhat."""
    nf = len(rows)
    out = dict(w=np.zeros(nf), cond_mean=np.zeros(nf), cond_var=np.zeros(nf), yhat=np.zeros(nf) if rec["yhat"] is not None else None)
    where = {}
    for k, g in enumerate(groups):
        for a, i in enumerate(g):
            where[int(i)] = (k, a)
    for f, (idx, wt) in enumerate(rows):
        idx, wt = np.asarray(idx, dtype=np.int64), np.asarray(wt, dtype=np.float64)
        out["w"][f] = math.fsum(wt * rec["w"][idx])
        out["cond_mean"][f] = math.fsum(wt * rec["mean"][idx])
        if out["yhat"] is not None:
            out["yhat"][f] = math.fsum(wt * rec["yhat"][idx])
        if rec.get("cov") is None:
            out["cond_var"][f] = math.fsum(wt * wt * rec["var"][idx])
        else:
            terms = []
            for x, (i, a) in enumerate(zip(idx, wt)):
                for j, b in zip(idx[:x + 1], wt[:x + 1]):
                    (ki, ai), (kj, aj) = where[int(i)], where[int(j)]
                    if ki == kj:
                        g = groups[ki].size
                        s = rec["cov"][int(offsets[ki]) + max(ai, aj) + min(ai, aj) * g]
                        terms.append(a * b * s * (1.0 if i == j else 2.0))
            out["cond_var"][f] = max(math.fsum(terms), 0.0)
    return out


class Contract:
    """Every read from the per-draw records, over the ids the model lists.  ``records[id]`` = dict(kind, w, mean, var, cov (packed, a
    joint set) or None, yhat or None, beta p x q, tausq_inv q, F = the functionals' values of that iteration or None).  A negative id is
    a row or a value nobody wrote (only the wrong variants of the CPU test produce them): a record of its own."""

    def __init__(self, inputs, records):
        self.inp, self.records = inputs, records

    def rec(self, i, kind):
        if i >= 0:
            return self.records[i]
        n = self.inp.size(kind)
        junk = np.full(n, 100.0 + abs(i))
        _, off = self.inp.groups(kind)
        nf = max(Inputs.FUN_SIZES.values())
        F = {k: np.full(nf, 100.0 + abs(i)) for k in ("w", "cond_mean", "cond_var", "yhat")}
        return dict(kind=kind, w=junk, mean=junk + 1, var=junk + 2, cov=np.full(int(off[-1]), 7.0) if KINDS[kind][2] else None,
                    yhat=junk + 3 if KINDS[kind][1] else None, beta=np.ones((self.inp.p, self.inp.q)), tausq_inv=np.ones(self.inp.q), F=F, F_name=None)

    def F(self, i, kind, m):
        """The functionals' values the device reported for iteration ``i``, for the functionals set now (junk where it has none)."""
        r = self.rec(i, kind)
        F = r.get("F")
        if F is None or r.get("F_name") != m.fun.name:
            F = self.rec(-1 - abs(i), kind)["F"]
        return {k: (v[:m.fun.n_fun] if v is not None else None) for k, v in F.items()}

    def stack(self, ids, kind, key):
        n = self.inp.size(kind)
        return np.stack([self.rec(i, kind)[key] for i in ids]) if ids else np.zeros((0, n))

    def fun_draws(self, m, ids):
        """The functionals' values by the definition, per id: dict of [len(ids), n_fun] arrays."""
        rows = self.inp.functionals(m.kind, m.fun.name)
        groups, off = self.inp.groups(m.kind)
        vals = [fun_values(rows, self.rec(i, m.kind), groups, off) if i >= 0 else
                {k: v[:len(rows)] for k, v in self.rec(i, m.kind)["F"].items()} for i in ids]
        return {k: (np.stack([v[k] for v in vals]) if vals[0][k] is not None else None) for k in vals[0]}

    @staticmethod
    def moments(cm, cv, w, y):
        out = dict(mean=cm.mean(axis=0), var=cv.mean(axis=0) + cm.var(axis=0), w_mean=w.mean(axis=0))
        out["yhat_mean"] = y.mean(axis=0) if y is not None else None
        return out

    def signature(self, op, m):
        """Everything the value of a read depends on: equal signatures give equal values."""
        cls = m.classify(op)
        n = op.name
        dep = {"get": lambda: (m.seen,), "get_cov": lambda: (m.seen, m.pair), "squantile": lambda: (m.stored_rows(),),
               "fun_get": lambda: (m.fun.name, m.fun.seen), "fun_last": lambda: (m.fun.name, m.fun.seen[-1:]),
               "fun_quantile": lambda: (m.fun.name, m.fun.store), "fun_info": lambda: (m.fun and m.fun.name,),
               "score_get": lambda: (m.score.y, m.score.seen, m.stored_rows()), "exceed_get": lambda: (m.exceed.n_thr, m.exceed.fun, m.exceed.seen, m.fun and m.fun.name),
               "mix_draws": lambda: (m.mix.cols,), "mix_quantiles": lambda: (m.mix.cols, m.mix.fcols, m.fun and m.fun.name),
               "mix_crps": lambda: (m.score.y, m.mix.cols), "mix_info": lambda: (), "layout": lambda: ()}
        return (n, op.arg, m.kind, cls, tuple(sorted(m.counts(op).items())), repr(dep[n]()) if cls[0] == LEGAL else None)

    def read(self, op, m):
        """The arrays a LEGAL read returns (None where the call writes nothing), by the header's definitions in float64."""
        from oracle.list_summaries import list_qtile
        from spamtree_amd import exceed as rb
        from spamtree_amd import mixture as mixdef
        inp, kind, n, name = self.inp, m.kind, m.n, op.name
        P = inp.points(kind)
        mv0 = P["mv"] - 1
        groups, off = inp.groups(kind)
        S = lambda ids, key: self.stack(ids, kind, key)   # noqa: E731
        if name == "get":
            return self.moments(S(m.seen, "mean"), S(m.seen, "var"), S(m.seen, "w"), S(m.seen, "yhat") if m.has_X else None)
        if name == "get_cov":
            cm, out = S(m.pair, "mean"), np.zeros(int(off[-1]))       # (the pair accumulators hold the ids of the summaries)
            cc = np.stack([self.rec(i, kind)["cov"] for i in m.pair])
            cnt = float(len(m.seen))
            for k, g in enumerate(groups):
                sl = slice(int(off[k]), int(off[k + 1]))
                d = cm[:, g] - cm[:, g].mean(axis=0)
                out[sl] = cc[:, sl].sum(axis=0) / cnt + (d.T @ d / cnt).reshape(-1, order="F")
            return dict(cov=out)
        if name == "layout":
            return dict(n_joint=len(groups), offsets=off, members=np.concatenate(groups) if groups else np.zeros(0, dtype=np.int64),
                        member_ptr=np.concatenate([[0], np.cumsum([g.size for g in groups])]).astype(np.int64))
        if name == "squantile":
            rows = m.stored_rows()
            return dict(w=list_qtile(list(S(rows, "w")), op.arg), yhat=list_qtile(list(S(rows, "yhat")), op.arg) if m.has_X else None)
        if name == "fun_info":
            return {}
        if name in ("fun_get", "fun_last", "fun_quantile"):
            ids = {"fun_get": m.fun.seen, "fun_last": m.fun.seen[-1:], "fun_quantile": m.fun.store}[name]
            F = self.fun_draws(m, ids)
            if name == "fun_last":
                return {k: (v[0] if v is not None else None) for k, v in F.items()}
            if name == "fun_get":
                return self.moments(F["cond_mean"], F["cond_var"], F["w"], F["yhat"])
            return dict(w=list_qtile(list(F["w"]), op.arg), yhat=list_qtile(list(F["yhat"]), op.arg) if m.has_X else None)
        if name == "score_get":
            y = inp.y_new(kind, m.score.y)
            obs = ~np.isnan(y)
            recs = [self.rec(i, kind) for i in m.score.seen]
            ell, phi = np.full((len(recs), n), np.nan), np.full((len(recs), n), np.nan)
            for s, r in enumerate(recs):
                mu = np.einsum("ik,ki->i", P["X"], r["beta"][:, mv0]) + r["mean"]
                sig = np.sqrt(r["var"] + 1.0 / r["tausq_inv"][mv0])
                z = (y - mu) / sig
                ell[s] = -0.5 * z * z - np.log(sig) - 0.5 * math.log(2 * math.pi)
                phi[s] = [0.5 * math.erfc(-t / math.sqrt(2.0)) if np.isfinite(t) else np.nan for t in z]
            mx = ell.max(axis=0)
            out = dict(lpd=np.where(obs, mx + np.log(np.exp(ell - mx).mean(axis=0)), np.nan), pit=np.where(obs, phi.mean(axis=0), np.nan),
                       crps=None, lpd_joint=None)
            if op.arg[0]:
                d = np.sort(S(m.stored_rows(), "yhat") - y, axis=0)
                K = d.shape[0]
                k = np.arange(1, K + 1)[:, None]
                out["crps"] = np.where(obs, np.abs(d).mean(axis=0) - ((2 * k - K - 1) * d).sum(axis=0) / K ** 2, np.nan)
            if op.arg[1]:
                lj = np.full(len(groups), np.nan)
                for k, g in enumerate(groups):
                    o = np.nonzero(obs[g])[0]
                    if o.size == 0:
                        continue
                    dens = []
                    for r in recs:
                        Sg = r["cov"][int(off[k]):int(off[k + 1])].reshape(g.size, g.size, order="F")
                        Sg = np.tril(Sg) + np.tril(Sg, -1).T
                        A = Sg[np.ix_(o, o)] + np.diag(1.0 / r["tausq_inv"][mv0[g[o]]])
                        e = y[g[o]] - (np.einsum("ik,ki->i", P["X"][g[o]], r["beta"][:, mv0[g[o]]]) + r["mean"][g[o]])
                        try:
                            L = np.linalg.cholesky(A)
                            zz = np.linalg.solve(L, e)
                            dens.append(-0.5 * zz @ zz - np.log(np.diag(L)).sum() - 0.5 * o.size * math.log(2 * math.pi))
                        except np.linalg.LinAlgError:
                            dens.append(-np.inf)
                    dens = np.array(dens)
                    lj[k] = -np.inf if not np.isfinite(dens.max()) else dens.max() + math.log(np.exp(dens - dens.max()).mean())
                out["lpd_joint"] = lj
            return out
        if name == "exceed_get":
            thr, side = inp.thresholds(m.exceed.n_thr)
            ids = m.exceed.seen
            if n == 0:
                return dict(w=None, yhat=None, fun_w=None)
            cm, cv = S(ids, "mean").T, S(ids, "var").T
            strip = lambda d: dict(prob=d["prob"], prob_var=d["prob_var"])   # noqa: E731
            out = dict(w=strip(rb.exceed_w(cm, cv, P["mv"], thr, side)), yhat=None, fun_w=None)
            if m.has_X:
                beta = np.stack([self.rec(i, kind)["beta"] for i in ids], axis=1)
                tsi = np.stack([self.rec(i, kind)["tausq_inv"] for i in ids], axis=1)
                out["yhat"] = strip(rb.exceed_yhat(cm, cv, P["mv"], P["X"], beta, tsi, thr, side))
            if op.arg:
                nf = m.fun.n_fun
                tf = inp.thresholds_fun(m.exceed.n_thr, nf)
                st = rb.Stream()
                for i in ids:
                    F = self.F(i, kind, m)
                    st.update(rb.draw_prob(F["cond_mean"][None, :], F["cond_var"][None, :], tf, side[:, None]))
                out["fun_w"] = strip(st.finish())
            return out
        if name == "mix_draws":
            ids = m.mix.cols
            if n == 0 or not ids:
                return dict(m=None, v=None, mu=None, tau2=None)
            out = dict(m=S(ids, "mean"), v=S(ids, "var"), mu=None, tau2=np.stack([1.0 / self.rec(i, kind)["tausq_inv"] for i in ids]))
            if m.has_X:
                out["mu"] = np.stack([self.mu(P, self.rec(i, kind)) for i in ids])
            return out
        if name == "mix_quantiles":
            if n == 0:
                return dict(w=None, yhat=None, fun_w=None)
            ids = m.mix.cols
            mm, vv = S(ids, "mean"), S(ids, "var")
            qs = lambda M, V: np.array([[mixdef.quantile(p, M[:, i], V[:, i]) for i in range(M.shape[1])] for p in PROBS])   # noqa: E731
            out = dict(w=qs(mm, vv), yhat=None, fun_w=None)
            if m.has_X:
                mu = np.stack([self.mu(P, self.rec(i, kind)) for i in ids])
                t2 = np.stack([1.0 / self.rec(i, kind)["tausq_inv"] for i in ids])[:, mv0]
                out["yhat"] = qs(mu, vv + t2)
            if op.arg:
                fm = np.stack([self.F(i, kind, m)["cond_mean"] for i in m.mix.fcols])
                fv = np.stack([self.F(i, kind, m)["cond_var"] for i in m.mix.fcols])
                out["fun_w"] = qs(fm, fv)
            return out
        if name == "mix_crps":
            y = inp.y_new(kind, m.score.y)
            ids = m.mix.cols
            mu = np.stack([self.mu(P, self.rec(i, kind)) for i in ids])
            s2 = S(ids, "var") + np.stack([1.0 / self.rec(i, kind)["tausq_inv"] for i in ids])[:, mv0]
            crps, spread = np.full(n, np.nan), np.full(n, np.nan)
            for i in np.nonzero(~np.isnan(y))[0]:
                crps[i], spread[i] = mixdef.crps(y[i], mu[:, i], s2[:, i]), mixdef.spread(mu[:, i], s2[:, i])
            return dict(crps=crps, spread=spread)
        if name == "mix_info":
            return {}
        raise ValueError(op)

    @staticmethod
    def mu(P, rec):
        """x_i'beta_j + cond_mean_i as the store forms it: spamtree_amd.exceed.xb_chain per outcome, then the add."""
        from spamtree_amd.exceed import xb_chain
        mv0 = P["mv"] - 1
        xb = np.zeros(P["n"])
        for j in np.unique(mv0):
            xb[mv0 == j] = xb_chain(P["X"][mv0 == j], rec["beta"][:, j])
        return xb + rec["mean"]


def synthetic_record(inp, kind, i, fun_name=None, chain=None):
    """Per-draw outputs nobody computed: what the CPU tests feed the executor.  As on the device the conditional moments are a
    function of the chain's state (``chain``: Model.acc_chain of the id), the draws of the id as well: distinct states give
    distinct, O(1)-apart values."""
    rng = np.random.default_rng([23, i if chain is None else chain])
    n = inp.size(kind)
    _, has_X, joint = KINDS[kind]
    groups, off = inp.groups(kind)
    rec = dict(kind=kind, w=None, mean=rng.standard_normal(n), var=rng.uniform(0.1, 1.0, n), cov=None, yhat=None,
               beta=rng.standard_normal((inp.p, inp.q)), tausq_inv=1.0 / rng.uniform(0.05, 0.5, inp.q), F=None)
    if n > 2:
        rec["var"][2] = 0.0
    if joint:
        cov = np.zeros(int(off[-1]))
        for k, g in enumerate(groups):
            B = rng.standard_normal((g.size, g.size + 1))
            Sg = B @ B.T
            cov[int(off[k]):int(off[k + 1])] = Sg.reshape(-1, order="F")
            rec["var"][g] = np.diag(Sg)
        rec["cov"] = cov
    rng = np.random.default_rng([29, i])
    rec["w"] = rec["mean"] + np.sqrt(rec["var"]) * rng.standard_normal(n)
    if has_X:
        rec["yhat"] = rec["w"] + rng.standard_normal(n)
    if fun_name:
        rows = inp.functionals(kind, fun_name)
        rec["F"], rec["F_name"] = fun_values(rows, rec, groups, off), fun_name
    return rec


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--set", required=True, choices=FAMILIES + ("regression",), help="the kind of the first point set")
    ap.add_argument("--seed", required=True)
    ap.add_argument("--upto", type=int, default=None, help="index of the last operation to print")
    a = ap.parse_args()
    seed = a.seed if a.set == "regression" else int(a.seed)
    print(f"set {a.set} seed {seed}" + (" (runs on the generic kernels too)" if (a.set, seed) in GENERIC else ""))
    print(describe(sequence(a.set, seed), a.upto))
