"""GPU: random call sequences over the new-point family (st_points_*; tests/points_model.py has the model of the contract, the seeded
generator and the NumPy executor), on make_problem(side=12, q=2) -- 288 rows, two theta, every row observed -- and sets of 37 new
points: some on conditioning rows, a duplicate inside a joint group, joint groups of 1, 2 and 3 members, the empty and the
single-point set.  Three replays of every sequence:

  1. interleaved   one handle runs everything.  After every operation: the return code and the fragment of st_last_error against
                   Model.classify, every count the call writes (n_accumulated, n_stored, n_scored, n_fun, keep) against the model.
  2. solo          per rider (stored draws, functionals, scores, thresholds, mixture store) a fresh handle replays the sequence
                   filtered to the chain, the point sets, the accumulates, the resets and that rider's own operations with their
                   prerequisites.  Every accumulate's outputs and every read of the rider equal the interleaved handle's bit for
                   bit: the header's "writes nothing another step reads, so every other output is the same bit for bit".
  3. contract      the NumPy executor is fed the interleaved run's per-draw outputs and every read is compared with it: bit for bit
                   where the project claims it (the mixture store's columns), elsewhere within the bound that output has in its
                   own test, imported or restated here and named where it is used.  The sweeps between accumulates move w by O(1),
                   so a read over a wrong set of draws is off by many orders of magnitude more than any of these bounds: this
                   checks WHICH draws a read covers, not rounding.

A failure names the set, the seed, the operation, and `python -m tests.points_model --set S --seed N --upto I`, which prints that
prefix with the model's state before each operation."""
import ctypes as C
import math
import time
from fractions import Fraction
from types import SimpleNamespace as NS

import numpy as np
import pytest

from tests import exceed_reference as er
from tests import mixture_reference as mr
from tests import points_model as pm
from tests import score_reference as sr
from tests import test_outputs_reference as ref
from tests.points_model import LEGAL, REFUSED, Op
from tests.util import make_problem

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None   # noqa: E731
ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64)) if a is not None else None    # noqa: E731
SLOWEST = {}
CHECKED = {}            # (kind of the point set, read) -> how often check 3 compared it with the contract
_SHARED = {}


def shared():
    """The problem and the operations' inputs: built once."""
    if not _SHARED:
        pb = make_problem(side=12, q=2, seed=5, p=2)
        _SHARED.update(pb=pb, inp=pm.Inputs(pb=pb))
    return _SHARED["pb"], _SHARED["inp"]


def some_points(n):
    """The points the 50-digit references are evaluated at: every third one, the first group of three (with its duplicate) and the last."""
    return sorted(set(range(0, n, 3)) | set(range(min(n, 3))) | ({n - 1} if n else set()))


class Handle:
    """One library handle and the calls behind the model's operations, through the C-ABI: a refusal comes back as a code."""

    def __init__(self, pb, inp, fg):
        from spamtree_amd.model import SpamTreeMV
        self.pb, self.inp = pb, inp
        self.hm = SpamTreeMV(pb["y"], pb["X"], pb["Z"], pb["coords"], pb["mv_id"], pb["blocking"], pb["gix_block"], pb["res_is_ref"],
                             pb["parents"], pb["children"], False, pb["block_names"], pb["block_groups"], pb["indexing"],
                             np.random.default_rng(6).standard_normal(pb["n"]), np.zeros(pb["p"]), pb["theta"], 5.0, force_generic=fg)
        self.lib, self.h = self.hm.lib, self.hm.h

    def close(self):
        self.hm.close()

    def err(self):
        return self.lib.st_last_error(self.h).decode()

    def draw(self, m, it, accumulate, outputs, joint_call=False):
        """st_points_predict(_joint) mode 0 or st_points_accumulate(_joint) with that counter: (rc, dict(w, mean, var, yhat, cov))."""
        n, lib, h = m.n, self.lib, self.h
        _, off = self.inp.groups(m.kind) if m.kind else ([], [0])
        o = dict(w=np.zeros(n), mean=np.zeros(n), var=np.zeros(n), yhat=np.zeros(n) if m.has_X else None,
                 cov=np.zeros(int(off[-1])) if m.joint else None)
        chol = np.zeros(int(off[-1])) if m.joint else None
        if not outputs:
            assert accumulate
            call = lib.st_points_accumulate_joint if joint_call else lib.st_points_accumulate
            return (call(h, pm.ACC_SEED, it, None, None, None, None, None) if joint_call else call(h, pm.ACC_SEED, it, None, None, None, None)), None
        if joint_call or (not accumulate and m.joint):
            call = lib.st_points_accumulate_joint if accumulate else lib.st_points_predict_joint
            args = (h, pm.ACC_SEED, it) if accumulate else (h, 0, None, pm.ACC_SEED, it)
            rc = call(*args, dp(o["w"]), dp(o["mean"]), dp(o["cov"]), dp(chol), dp(o["yhat"]))
            if rc == 0 and m.joint:
                groups, off = self.inp.groups(m.kind)
                for k, g in enumerate(groups):
                    o["var"][g] = np.maximum(o["cov"][int(off[k]):int(off[k + 1])][::g.size + 1], 0.0)
        else:
            call = lib.st_points_accumulate if accumulate else lib.st_points_predict
            args = (h, pm.ACC_SEED, it) if accumulate else (h, 0, None, pm.ACC_SEED, it)
            rc = call(*args, dp(o["w"]), dp(o["mean"]), dp(o["var"]), dp(o["yhat"]))
            if m.joint:
                o["cov"] = None                      # st_points_accumulate on a joint set returns cond_var, not the blocks
        return rc, o

    def step(self, op, m, record=False):
        """Runs ``op`` in the model state ``m`` (before it): dict(rc, err, counts, val, out, rec)."""
        n, a, hm, lib, h, inp = op.name, op.arg, self.hm, self.lib, self.h, self.inp
        res = dict(rc=0, err="", counts={}, val=None, out=None, rec=None)
        cnt = C.c_int64(-1)
        N, q = m.n, self.pb["q"]
        nf = m.fun.n_fun if m.fun else 1
        if n == "sweep":
            hm.deal_with_w(seed=pm.ACC_SEED + 1, it=a)
        elif n == "beta":
            hm.beta_update(inp.betas[a])
        elif n == "tausq":
            hm.tausq_inv = inp.tausq_invs[a].copy()
            hm._check(lib.st_set_tausq_inv(h, dp(hm.tausq_inv)))
        elif n == "theta":
            hm.theta_update(0, self.pb["theta"] * (1.0 + 0.03 * a))
            assert hm.get_loglik_comps_w(0)
        elif n == "set":
            P = inp.points(a)
            hm.set_points(P["coords"], P["mv"], P["anchor"], P["X"], joint=P["labels"])
        elif n == "reset":
            res["rc"] = lib.st_points_summary_reset(h)
        elif n == "reserve":
            res["rc"] = lib.st_points_summary_reserve(h, a)
        elif n == "mix":
            res["rc"] = lib.st_points_mixture_reserve(h, a)
        elif n == "fun":
            rows = [] if a is None else inp.functionals(m.kind or "plainX", a)
            ptr = np.concatenate([[0], np.cumsum([len(r[0]) for r in rows])]).astype(np.int64)
            idx = np.concatenate([np.asarray(r[0], dtype=np.int64) for r in rows] + [np.zeros(0, dtype=np.int64)])
            wt = np.concatenate([np.asarray(r[1], dtype=np.float64) for r in rows] + [np.zeros(0)])
            res["rc"] = lib.st_points_functionals_set(h, len(rows), ip(ptr), ip(idx), dp(wt))
        elif n == "score":
            y = None if a is None else inp.y_new(m.kind or "plainX", a)
            res["rc"] = lib.st_points_score_set(h, dp(y))
        elif n == "exceed":
            if a is None:
                res["rc"] = lib.st_points_exceed_set(h, 0, None, None, None)
            else:
                thr, side = inp.thresholds(a[0])
                tf = inp.thresholds_fun(a[0], m.fun.n_fun if m.fun else 3) if a[1] else None
                res["rc"] = lib.st_points_exceed_set(h, a[0], dp(thr), side.ctypes.data_as(C.POINTER(C.c_int32)), dp(tf))
        elif n in ("acc", "accj"):
            legal = m.classify(op)[0] == LEGAL
            pre = None
            if record and legal and (not a or (m.joint and n == "acc")):
                rc0, pre = self.draw(m, m.next_id, False, True)      # the same draw: st_points_predict with that seed and counter
                assert rc0 == 0, self.err()
            res["rc"], res["out"] = self.draw(m, m.next_id, True, a, joint_call=n == "accj")
            if record and legal and res["rc"] == 0:
                rec = dict(pre or res["out"], kind=m.kind, beta=hm.Bcoeff.copy(), tausq_inv=np.asarray(hm.tausq_inv, dtype=np.float64).copy(),
                           F=None, F_name=None)
                if pre is not None and res["out"] is not None:        # st_points_accumulate on a joint set: the draw st_points_predict_joint gave
                    for k in ("w", "mean", "var", "yhat"):
                        assert np.array_equal(pre[k], res["out"][k]), f"st_points_accumulate's {k} is not st_points_predict_joint's"
                if m.fun:
                    F = {k: np.zeros(nf) for k in ("w", "cond_mean", "cond_var")}
                    F["yhat"] = np.zeros(nf) if m.has_X else None
                    hm._check(lib.st_points_functionals_last(h, dp(F["w"]), dp(F["cond_mean"]), dp(F["cond_var"]), dp(F["yhat"])))
                    rec["F"], rec["F_name"] = F, m.fun.name
                res["rec"] = rec
        elif n == "predict":
            _, off = inp.groups(m.kind) if m.kind else ([], [0])
            o = [np.zeros(N) for _ in range(3)] + [np.zeros(N) if m.has_X else None]
            if m.joint:
                res["rc"] = lib.st_points_predict_joint(h, 1, None, 0, 0, dp(o[0]), dp(o[1]), dp(np.zeros(int(off[-1]))), dp(np.zeros(int(off[-1]))), dp(o[3]))
            else:
                res["rc"] = lib.st_points_predict(h, 1, None, 0, 0, dp(o[0]), dp(o[1]), dp(o[2]), dp(o[3]))
            if res["rc"] == 0 and N:
                assert np.array_equal(o[0], o[1]), "mode 1: w_new is the conditional mean"
        elif n in ("squantile", "fun_quantile"):
            k = N if n == "squantile" else nf
            v = dict(w=np.zeros(k), yhat=np.zeros(k) if m.has_X else None)
            call = lib.st_points_summary_quantile if n == "squantile" else lib.st_points_functionals_quantile
            res["rc"], res["val"] = call(h, float(a), dp(v["w"]), dp(v["yhat"])), v
        elif n in ("get", "fun_get"):
            k = N if n == "get" else nf
            v = dict(mean=np.zeros(k), var=np.zeros(k), w_mean=np.zeros(k), yhat_mean=np.zeros(k) if m.has_X else None)
            call = lib.st_points_summary_get if n == "get" else lib.st_points_functionals_get
            res["rc"] = call(h, dp(v["mean"]), dp(v["var"]), dp(v["w_mean"]), dp(v["yhat_mean"]), C.byref(cnt))
            res["val"], res["counts"] = v, dict(n_accumulated=cnt.value)
        elif n == "get_cov":
            _, off = inp.groups(m.kind) if m.kind else ([], [0])
            v = dict(cov=np.zeros(max(int(off[-1]), 1)))
            res["rc"], res["val"] = lib.st_points_summary_get_cov(h, dp(v["cov"])), dict(cov=v["cov"][:int(off[-1])])
        elif n == "layout":
            res["rc"] = lib.st_points_joint_layout(h, C.byref(cnt), None, None, None)
            if res["rc"] == 0:
                off, ptr, mem = np.zeros(cnt.value + 1, dtype=np.int64), np.zeros(cnt.value + 1, dtype=np.int64), np.zeros(N, dtype=np.int64)
                res["rc"] = lib.st_points_joint_layout(h, C.byref(cnt), ip(off), ip(ptr), ip(mem))
                res["val"] = dict(n_joint=cnt.value, offsets=off, members=mem, member_ptr=ptr)
        elif n == "fun_last":
            v = {k: np.zeros(nf) for k in ("w", "cond_mean", "cond_var")}
            v["yhat"] = np.zeros(nf) if m.has_X else None
            res["rc"], res["val"] = lib.st_points_functionals_last(h, dp(v["w"]), dp(v["cond_mean"]), dp(v["cond_var"]), dp(v["yhat"])), v
        elif n == "fun_info":
            c = [C.c_int64(-1) for _ in range(4)]
            res["rc"] = lib.st_points_functionals_info(h, *[C.byref(x) for x in c], None)
            res["counts"], res["val"] = dict(n_fun=c[0].value), {}
        elif n == "score_get":
            groups, _ = inp.groups(m.kind) if m.kind else ([], None)
            v = dict(lpd=np.zeros(N), pit=np.zeros(N), crps=np.zeros(N) if a[0] else None, lpd_joint=np.zeros(max(len(groups), 1)) if a[1] else None)
            nd = C.c_int64(-1)
            res["rc"] = lib.st_points_score_get(h, dp(v["lpd"]), dp(v["pit"]), dp(v["crps"]), dp(v["lpd_joint"]), C.byref(cnt), C.byref(nd))
            v["n_degenerate"] = np.array([nd.value])
            res["val"], res["counts"] = v, dict(n_scored=cnt.value)
        elif n == "exceed_get":
            from spamtree_amd import _lib
            T = m.exceed.n_thr if m.exceed else 1
            keepalive = []

            def bufs(k, want=True):
                if not want:
                    return None, None
                d = dict(prob=np.zeros((T, k)), prob_var=np.zeros((T, k)))
                s = _lib.StRbOut(dp(d["prob"]), dp(d["prob_var"]))
                keepalive.append(s)
                return d, C.byref(s)
            (w, sw), (y, sy), (f, sf) = bufs(N), bufs(N, m.has_X), bufs(nf, bool(a))
            res["rc"] = lib.st_points_exceed_get(h, sw, sy, sf, C.byref(cnt))
            res["val"], res["counts"] = dict(w=w, yhat=y, fun_w=f), dict(n_accumulated=cnt.value)
            if N == 0:
                res["val"] = dict(w=None, yhat=None, fun_w=None)
        elif n == "mix_draws":
            res["rc"] = lib.st_points_mixture_draws(h, None, None, None, None, C.byref(cnt))
            res["counts"] = dict(n_stored=cnt.value)
            res["val"] = dict(m=None, v=None, mu=None, tau2=None)
            if res["rc"] == 0 and cnt.value > 0 and N > 0:
                K = cnt.value
                v = dict(m=np.zeros((K, N)), v=np.zeros((K, N)), mu=np.zeros((K, N)) if m.has_X else None, tau2=np.zeros((K, q)))
                res["rc"] = lib.st_points_mixture_draws(h, dp(v["m"]), dp(v["v"]), dp(v["mu"]), dp(v["tau2"]), C.byref(cnt))
                res["val"] = v
        elif n == "mix_quantiles":
            from spamtree_amd import _lib
            T = len(pm.PROBS)
            keepalive, unc = [], []

            def bufs(k, want=True):
                if not want:
                    return None, None
                qv, u = np.zeros((T, k)), C.c_int64(0)
                s = _lib.StMixOut(dp(qv), C.pointer(u))
                keepalive.append(s); unc.append(u)
                return qv, C.byref(s)
            (w, sw), (y, sy), (f, sf) = bufs(N), bufs(N, m.has_X), bufs(nf, bool(a))
            res["rc"] = lib.st_points_mixture_quantiles(h, T, dp(np.array(pm.PROBS)), sw, sy, sf)
            res["val"] = dict(w=w, yhat=y, fun_w=f) if N else dict(w=None, yhat=None, fun_w=None)
            if res["rc"] == 0:
                assert all(u.value == 0 for u in unc), "n_unconverged"
        elif n == "mix_crps":
            v = dict(crps=np.zeros(N), spread=np.zeros(N))
            res["rc"] = lib.st_points_mixture_crps(h, dp(v["crps"]), dp(v["spread"]), C.byref(cnt))
            res["val"], res["counts"] = v, dict(n_scored=cnt.value)
        elif n == "mix_info":
            c = [C.c_int64(-1) for _ in range(4)]
            res["rc"] = lib.st_points_mixture_info(h, C.byref(c[0]), C.byref(c[1]), None, C.byref(c[2]), C.byref(c[3]))
            res["counts"], res["val"] = dict(keep=c[0].value, n_stored=c[1].value), {}
        else:
            raise ValueError(op)
        if res["rc"] < 0:
            res["err"] = self.err()
        return res


def same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and sorted(a) == sorted(b) and all(same(a[k], b[k]) for k in a)
    if a is None or b is None:
        return a is None and b is None
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


# ---- check 3: a read against the contract executor, each within the bound of the output's own test --------------------------------
def fun_bounds(rows, rec, groups, off):
    """Per functional the bound of tests/test_gpu_functionals.py on each of F_w, F_m, F_v, F_y of one draw: c(T) 2^-53 sum |coefficient
    value| with c = test_gpu_functionals.chain over the T terms of the list (the variance list of a joint set: variance_terms).  That
    test compares with exact rationals; the executor's values are float64 sums of float64 products, so c grows by the roundings of
    one of its terms: 2 (a linear term and the sum), 3 (a a v) and 4 (2 a b Sigma)."""
    from tests.test_gpu_functionals import chain, variance_terms
    ns = NS(joint_groups=groups, joint_offsets=off)
    out = {k: np.zeros(len(rows)) for k in ("w", "cond_mean", "cond_var", "yhat")}
    for f, (idx, wt) in enumerate(rows):
        idx, wt = np.asarray(idx, dtype=np.int64), np.asarray(wt, dtype=np.float64)
        T = idx.size
        for key, src in (("w", "w"), ("cond_mean", "mean"), ("yhat", "yhat")):
            if rec[src] is not None:
                out[key][f] = (chain(T) + 2) * U * np.abs(wt * rec[src][idx]).sum()
        if rec.get("cov") is None:
            out["cond_var"][f] = (chain(T) + 3) * U * np.abs(wt * wt * rec["var"][idx]).sum()
        elif T:
            coef, src = variance_terms(idx, wt, ns)
            out["cond_var"][f] = (chain(coef.size) + 4) * U * np.abs(coef * rec["cov"][src]).sum()
    return out


class Checker:
    def __init__(self, inp, records, where):
        self.inp, self.records, self.where = inp, records, where
        self.c = pm.Contract(inp, records)

    def close(self, name, got, want, tol):
        got, want, tol = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), np.asarray(tol, dtype=np.float64)
        bad = ~(np.abs(got - want) <= tol)
        assert not bad.any(), self.where(f"{name}: off the contract by {np.abs(got - want)[bad].max():.3g} (bound {np.broadcast_to(tol, got.shape)[bad].min():.3g}) "
                                         f"at {np.argwhere(bad)[:4].tolist()}")

    def bits(self, name, got, want):
        assert same(got, want), self.where(f"{name}: not the contract's bits")

    def welford(self, name, got, X, B, has_y):
        """The Welford summaries of st_points_summary_get / _functionals_get over the per-draw values X = dict(mean, var, w, yhat)
        [N, k], each known to the per-draw bound B (0 for the points): the bounds of test_point_summaries_match_exact_moments
        (tests/test_gpu_outputs.py) plus what a perturbation of the inputs by B moves the exact value."""
        N = X["mean"].shape[0]
        e_mean, e_M2, b_M2 = ref.exact_moments(X["mean"])
        bm, bv = np.max(B["mean"], axis=0), np.mean(B["var"], axis=0)
        self.close(name + ".mean", got["mean"], e_mean, N * U * np.abs(X["mean"]).max(axis=0) + bm)
        sum_var = X["var"].sum(axis=0)
        e_var = sum_var / N + e_M2 / N
        spread = np.abs(X["mean"] - e_mean).max(axis=0)
        b_var = b_M2 / N + (N + 1) * U * sum_var / N + 3 * U * e_var + bv + 4 * bm * spread + bm * bm
        self.close(name + ".var", got["var"], e_var, b_var)
        for key, src in (("w_mean", "w"), ("yhat_mean", "yhat")) if has_y else (("w_mean", "w"),):
            want = np.array([math.fsum(X[src][:, i]) / N for i in range(X[src].shape[1])])
            self.close(f"{name}.{key}", got[key], want, ref.mean_bound(X[src]) + np.max(B[src], axis=0))

    def per_draw(self, m, ids):
        return [dict(mean=self.records[i]["mean"], var=self.records[i]["var"]) for i in ids], [self.records[i]["beta"] for i in ids], \
            [self.records[i]["tausq_inv"] for i in ids]

    def check(self, op, m, got):
        from oracle.list_summaries import list_qtile
        inp, c, kind, n, name = self.inp, self.c, m.kind, m.n, op.name
        P = inp.points(kind)
        groups, off = inp.groups(kind)
        zero = lambda k: dict(mean=np.zeros((1, k)), var=np.zeros((1, k)), w=np.zeros((1, k)), yhat=np.zeros((1, k)))   # noqa: E731
        if name in ("fun_info", "mix_info"):
            return
        CHECKED[(kind, name)] = CHECKED.get((kind, name), 0) + 1
        if name in ("layout", "get_cov", "mix_draws"):
            want = c.read(op, m)
        if name == "layout":
            return self.bits(name, got, want)
        if name == "get":
            if n:
                X = {k: c.stack(m.seen, kind, k) for k in ("mean", "var", "w")}
                X["yhat"] = c.stack(m.seen, kind, "yhat") if m.has_X else None
                self.welford(name, got, X, zero(n), m.has_X)
            return
        if name == "get_cov":
            # test_summaries_over_saved_iterations (tests/test_gpu_predict_joint.py): 2 u ((N + 2) mean |Sigma| + (28 N + 20) X_a X_b)
            N = len(m.seen)
            cm = c.stack(m.seen, kind, "mean")
            cc = np.stack([self.records[i]["cov"] for i in m.seen])
            Xa = np.abs(cm).max(axis=0)
            tol = np.zeros(int(off[-1]))
            for k, g in enumerate(groups):
                sl = slice(int(off[k]), int(off[k + 1]))
                tol[sl] = 2 * U * ((N + 2) * np.abs(cc[:, sl]).mean(axis=0) + (28 * N + 20) * np.outer(Xa[g], Xa[g]).reshape(-1, order="F"))
            return self.close(name, got["cov"], want["cov"], tol)
        if name == "squantile":
            rows = m.stored_rows()
            for key in ("w", "yhat") if m.has_X else ("w",):
                d = c.stack(rows, kind, key)
                self.close(f"{name}.{key}", got[key], list_qtile(list(d), op.arg), ref.qtile_bound(d, op.arg))      # tests/test_gpu_outputs.py
            return
        if name in ("fun_last", "fun_get", "fun_quantile"):
            if n == 0:                                  # the functionals of an empty set have no term: zeros
                assert all(v is None or not np.any(v) for v in got.values()), self.where(f"{name} on the empty set is not 0")
                return
            rows = inp.functionals(kind, m.fun.name)
            ids = {"fun_get": m.fun.seen, "fun_last": m.fun.seen[-1:], "fun_quantile": m.fun.store}[name]
            F = c.fun_draws(m, ids)
            Bs = [fun_bounds(rows, self.records[i], groups, off) for i in ids]
            B = {k: np.stack([b[k] for b in Bs]) for k in Bs[0]}
            if name == "fun_last":
                for k in ("w", "cond_mean", "cond_var") + (("yhat",) if m.has_X else ()):
                    self.close(f"{name}.{k}", got[k], F[k][0], B[k][0])
                # ... and what the interleaved handle recorded behind that accumulate is what it returns now
                return self.bits(name + " (recorded)", {k: got[k] for k in ("cond_mean", "cond_var")},
                                 {k: self.records[ids[0]]["F"][k] for k in ("cond_mean", "cond_var")})
            if name == "fun_get":
                X = dict(mean=F["cond_mean"], var=F["cond_var"], w=F["w"], yhat=F["yhat"])
                return self.welford(name, got, X, dict(mean=B["cond_mean"], var=B["cond_var"], w=B["w"], yhat=B["yhat"]), m.has_X)
            for key in ("w", "yhat") if m.has_X else ("w",):
                self.close(f"{name}.{key}", got[key], list_qtile(list(F[key]), op.arg), ref.qtile_bound(F[key], op.arg) + B[key].max(axis=0))
            return
        if name == "score_get":
            from tests.test_gpu_score import check_points, joint_reference
            y = inp.y_new(kind, m.score.y)
            outs, betas, tis = self.per_draw(m, m.score.seen)
            try:
                check_points(got, y, P["X"], P["mv"], outs, betas, tis, "score_get")
            except AssertionError as e:
                raise AssertionError(self.where(f"score_get: lpd or pit off the contract: {e}")) from None
            if op.arg[0]:
                d = c.stack(m.stored_rows(), kind, "yhat")
                for i in np.nonzero(~np.isnan(y))[0]:
                    w_, mad = sr.crps_sorted(d[:, i], y[i])
                    e = abs(Fraction(float(got["crps"][i])) - w_)
                    assert e <= sr.crps_bound(d.shape[0], mad), self.where(f"score_get.crps[{i}] off the contract by {float(e):.3g}")
                assert np.all(np.isnan(got["crps"][np.isnan(y)]))
            if op.arg[1]:
                for s, o in enumerate(outs):
                    cov = self.records[m.score.seen[s]]["cov"]
                    o["cov"] = [cov[int(off[k]):int(off[k + 1])].reshape(g.size, g.size, order="F") for k, g in enumerate(groups)]
                ndeg = 0
                for k in range(len(groups)):
                    r = joint_reference(groups, y, P["X"], P["mv"], outs, betas, tis, k)
                    if r is None:
                        assert np.isnan(got["lpd_joint"][k]), self.where(f"lpd_joint[{k}] of a group without an observed member")
                        continue
                    lpd, bound, nd = r
                    ndeg += nd
                    if lpd == -sr.mp.inf:
                        assert got["lpd_joint"][k] == -np.inf, self.where(f"lpd_joint[{k}]")
                    else:
                        e = abs(float(sr.mp.mpf(float(got["lpd_joint"][k])) - lpd))
                        assert e <= bound, self.where(f"score_get.lpd_joint[{k}] off the contract by {e:.3g} (bound {bound:.3g})")
            return
        if name == "exceed_get":
            if n == 0:
                return
            from tests.test_gpu_exceed import references
            thr, side = inp.thresholds(m.exceed.n_thr)
            outs, betas, tis = self.per_draw(m, m.exceed.seen)
            idx = some_points(n)
            S = len(outs)
            refs = references(outs, betas, tis, P["X"], P["mv"], thr.tolist(), [int(s) for s in side], (S,), idx=idx)[S]
            pick = lambda d: {k: np.asarray(v)[:, idx] for k, v in d.items()}   # noqa: E731
            try:
                er.check_target(pick(got["w"]), refs[0], "w")
                if m.has_X:
                    er.check_target(pick(got["yhat"]), refs[1], "yhat")
                if op.arg:
                    tf = inp.thresholds_fun(m.exceed.n_thr, m.fun.n_fun)
                    Fs = [self.records[i]["F"] for i in m.exceed.seen]
                    frefs = [[er.finish([er.draw_w(F["cond_mean"][f], F["cond_var"][f], tf[t][f], int(side[t])) for F in Fs])
                              for f in range(m.fun.n_fun)] for t in range(m.exceed.n_thr)]
                    er.check_target(got["fun_w"], frefs, "fun_w")
            except AssertionError as e:
                raise AssertionError(self.where(f"exceed_get off the contract: {e}")) from None
            return
        if name == "mix_draws":
            return self.bits(name, got, want)                                                                        # tests/test_gpu_mixture.py: bit for bit
        if name == "mix_quantiles":
            if n == 0:
                return
            dr = c.read(Op("mix_draws"), m)
            K = len(m.mix.cols)
            targets = [("w", lambda i: mr.components(dr["m"][:K, i], dr["v"][:K, i]), some_points(n))]
            if m.has_X:
                targets.append(("yhat", lambda i: mr.components(dr["mu"][:K, i], dr["v"][:K, i], dr["tau2"][:K, P["mv"][i] - 1]), some_points(n)))
            if op.arg:
                Fs = [self.records[i]["F"] for i in m.mix.fcols]
                targets.append(("fun_w", lambda f: mr.components(np.array([F["cond_mean"][f] for F in Fs]), np.array([F["cond_var"][f] for F in Fs])),
                                range(m.fun.n_fun)))
            order = np.argsort(pm.PROBS)
            for tg, comps_of, idx in targets:
                for i in idx:
                    comps = comps_of(i)
                    for t, p in enumerate(pm.PROBS):
                        r = mr.check_quantile(got[tg][t, i], p, comps)
                        assert r <= 1.0, self.where(f"mix_quantiles.{tg}[{t}, {i}] violates the definition: {r:.3g} eps_F")
                assert np.all(np.diff(got[tg][order], axis=0) >= 0.0), self.where(f"mix_quantiles.{tg} decreases in p")
            return
        if name == "mix_crps":
            y = inp.y_new(kind, m.score.y)
            dr = c.read(Op("mix_draws"), m)
            K = len(m.mix.cols)
            for i in range(n):
                if np.isnan(y[i]):
                    assert np.isnan(got["crps"][i]) and np.isnan(got["spread"][i]), self.where(f"mix_crps[{i}] of an unscored point")
                    continue
                comps = mr.components(dr["mu"][:K, i], dr["v"][:K, i], dr["tau2"][:K, P["mv"][i] - 1])
                spr, t1 = mr.spread(comps), mr.t1_mean(y[i], comps)
                bc, bs = mr.crps_bounds(K, t1, spr)
                ec, es = mr.err(got["crps"][i], t1 - spr), mr.err(got["spread"][i], spr)
                assert ec <= bc and es <= bs, self.where(f"mix_crps[{i}] off the contract: crps {ec:.3g} ({bc:.3g}), spread {es:.3g} ({bs:.3g})")
            return
        raise ValueError(op)


class Case:
    def __init__(self, family, seed, model=pm.Model):
        self.family, self.seed, self.model = family, seed, model
        self.pb, self.inp = shared()
        self.ops = pm.sequence(family, seed)
        self.fg = (family, seed) in pm.GENERIC
        self.i, self.who = 0, "interleaved"

    def where(self, what):
        return (f"{what}\nset {self.family} seed {self.seed} ({self.who} handle{', generic kernels' if self.fg else ''}) operation {self.i} "
                f"{pm.show(self.ops[self.i])}\npython -m tests.points_model --set {self.family} --seed {self.seed} --upto {self.i}\n"
                + pm.describe(self.ops, self.i))

    def expect(self, op, m, res):
        cls, code, frag = m.classify(op)
        assert cls != pm.UNSPECIFIED, self.where("the sequence holds an operation the header does not define")
        if cls == LEGAL:
            assert res["rc"] == 0, self.where(f"the model says legal, the code is {res['rc']}: {res['err']}")
        else:
            assert res["rc"] == code and frag in res["err"], self.where(f"the model says refused {code} <{frag}>, got {res['rc']}: {res['err']}")
        for k, v in m.counts(op).items():
            assert res["counts"].get(k) == v, self.where(f"{k} is {res['counts'].get(k)}, the model says {v}")
        return cls

    def run(self, solo=True):
        records, log = {}, []
        check = Checker(self.inp, records, self.where)
        m = self.model()
        H = Handle(self.pb, self.inp, self.fg)
        routes = set()
        try:
            for self.i, op in enumerate(self.ops):
                res = H.step(op, m, record=True)
                cls = self.expect(op, m, res)
                if cls == LEGAL and res["val"] is not None:
                    check.check(op, m, res["val"])
                if cls == REFUSED:
                    m.refuse(op)
                if cls == LEGAL:
                    acc = m.apply(op)
                    if acc is not None:
                        records[acc] = res["rec"]
                        if m.n:
                            routes |= set(H.hm.points_info()["routes"])
                log.append(res)
        finally:
            H.close()
        if self.fg:
            assert any("generic" in r for r in routes), routes
        for self.who in pm.RIDERS if solo else ():
            solo, S = pm.Model(), Handle(self.pb, self.inp, self.fg)
            try:
                for self.i, op in enumerate(self.ops):
                    if not pm.solo_keeps(self.who, op):
                        continue
                    res = S.step(op, solo)
                    cls = self.expect(op, solo, res)
                    assert res["rc"] == log[self.i]["rc"], self.where("the solo handle's return code is not the interleaved one's")
                    if cls == LEGAL:
                        if res["out"] is not None:
                            assert same(res["out"], log[self.i]["out"]), self.where("an accumulate's outputs differ from the interleaved handle's")
                        if res["val"] is not None:
                            assert same(res["val"], log[self.i]["val"]), self.where("a read differs from the interleaved handle's")
                        solo.apply(op)
            finally:
                S.close()
        return routes


def test_the_point_sets_are_what_the_sequences_are_about():
    """37 points, joint groups of 1, 2 and 3 members that are not adjacent, a duplicate inside a group whose conditional variance is 0
    to rounding, points on conditioning rows, and both kernel families on the route lists."""
    pb, inp = shared()
    assert pb["n"] == 288 and pb["q"] == 2 and np.isfinite(pb["y"]).all()
    groups, _ = inp.groups("joint")
    assert inp.size("joint") == 37 and sorted({g.size for g in groups}) == [1, 2, 3] and any(np.any(np.diff(g) > 1) for g in groups)
    assert len(inp.on_rows) >= 1, "no point sits on a row of its conditioning set"
    g0 = groups[0]
    assert np.array_equal(inp.coords[g0[0]], inp.coords[g0[2]]) and inp.mv[g0[0]] == inp.mv[g0[2]]
    from oracle.spamtree_oracle import CovarianceParams, Covariancef
    from tests.test_gpu_parity import relerr
    cp = CovarianceParams(2, pb["q"])
    cp.transform(pb["theta"])
    for fg in (False, True):
        H, m = Handle(pb, inp, fg), pm.Model()
        try:
            seen = set()
            for op in (Op("set", "joint"), Op("theta", 0), Op("accj", True), Op("predict")):
                res = H.step(op, m, record=True)
                assert res["rc"] == 0, res
                if op.name == "accj":
                    rec = res["rec"]
                    seen |= set(H.hm.points_info()["routes"])
                m.apply(op)
            # tests/test_gpu_predict_joint.py, test_degenerate_pivots: a duplicate repeats its draw within 1e-8 prior standard deviations,
            # a point on a conditioning row gets that row's w within 1e-8
            sd = np.sqrt(Covariancef(inp.coords, inp.mv - 1, [int(g0[0])], [int(g0[0])], cp)[0, 0])
            assert abs(rec["w"][g0[2]] - rec["w"][g0[0]]) <= 1e-8 * sd and rec["w"][g0[0]] != rec["mean"][g0[0]]
            pts_on, rows_on = [i for i, _ in inp.on_rows], [r for _, r in inp.on_rows]
            assert relerr(rec["w"][pts_on], H.hm.get_w()[rows_on]) <= 1e-8
            for kind in ("plainX", "single"):
                for op in (Op("set", kind), Op("acc", True)):
                    assert H.step(op, m, record=True)["rc"] == 0
                    m.apply(op)
                seen |= set(H.hm.points_info()["routes"])
            print(f"force_generic={fg}: routes {sorted(seen)}")
            assert any(("generic" in r) == fg for r in seen)
        finally:
            H.close()


@pytest.mark.parametrize("family,seed", pm.cases(), ids=[f"{f}-{s}" for f, s in pm.cases()])
def test_interleaved_solo_and_contract_agree_after_every_operation(family, seed):
    t0 = time.perf_counter()
    Case(family, seed).run()
    SLOWEST[(family, seed)] = time.perf_counter() - t0


def test_zz_report_the_slowest_sequence():
    assert SLOWEST, "no sequence was replayed (run with the file)"
    case = max(SLOWEST, key=SLOWEST.get)
    print(f"{len(SLOWEST)} sequences; the slowest: set {case[0]} seed {case[1]}, {SLOWEST[case]:.2f} s")
    for kind in pm.FAMILIES:
        print(f"reads compared with the contract on {kind}: " + ", ".join(f"{r} {k}" for (f, r), k in sorted(CHECKED.items()) if f == kind))
    if len(SLOWEST) == len(pm.cases()):
        for name in pm.READS + ("squantile",):
            assert name in ("fun_info", "mix_info") or any(r == name for _, r in CHECKED), f"no {name} was compared with the contract"
