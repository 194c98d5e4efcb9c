"""GPU: random call sequences over the single-GPU C-ABI (tests/protocol_model.py), replayed on a handle with every deferral and
cache on ("lazy": what the C++ driver uses), on a handle of the same library with every short cut off ("eager") and on the
oracle.  After every operation:

  lazy against eager   the return codes and every value handed back, bit for bit (include/spamtree_hip.h: "identical results"
                       of st_factor_begin, "bit-identical to st_factor's" of the deferred leaf panels, "same results and return
                       codes" of the split sweep).  ONE pair is documented as not bit-identical: a sweep that reads the cached
                       Gram parts against one that recomputes them -- test_gram_cache_gives_identical_sweeps (test_gpu_parity.py):
                       "later sweeps of the caching model take k_sample_lean on reference levels, the other keeps k_sample_mfma:
                       equal up to rounding", asserted there at 1e-12.  From the first such sweep until the next st_set_w, w and
                       what is computed from it (log-densities, statistics, yhat, residuals) are compared at that 1e-12 and with
                       the oracle; everything that depends on theta only (panels, log-determinants) stays bit for bit.
  refusals             a negative code, a text in st_last_error, and the handle's w, log-density components and stored residuals
                       unchanged to the bit; the eager handle and the oracle skip the call, so every later comparison checks it again.
  against the oracle   both handles, with the tolerance test_gpu_parity.py uses for the quantity (REL = 1e-9, H 1e-8; its w is
                       checked "after three sweeps"); beyond three sweeps since the last st_set_w, w and what is computed from it
                       take test_gpu_chain.py's 1e-8.

A failure names the tree, the seed, the index and name of the operation, the model's flags and the operations so far;
`python -m tests.protocol_model --tree T --seed S --upto I` prints that prefix again."""
import numpy as np
import pytest

from tests import protocol_model as pm
from tests.test_gpu_parity import REL, relerr

pytestmark = pytest.mark.gpu

H_TOL = 1e-8            # test_gpu_parity.py: H of a block
CHAIN_TOL = 1e-8        # test_gpu_chain.py: w of a chain
GRAM_CACHE_TOL = 1e-12  # test_gram_cache_gives_identical_sweeps: cached against recomputed Gram parts
OBSERVED = {}           # (tree, quantity) -> largest error against the oracle; (tree, "lazy/eager " + quantity) -> between the handles
PROBLEMS = {}


def problem(tree):
    if tree not in PROBLEMS:
        PROBLEMS[tree] = pm.TREES[tree]["problem"]()
    return PROBLEMS[tree]


def set_env(tree, monkeypatch):
    for k, v in pm.TREES[tree]["env"].items():
        monkeypatch.setenv(k, v)


def note(tree, quantity, err):
    OBSERVED[(tree, quantity)] = max(OBSERVED.get((tree, quantity), 0.0), float(err))


def scalar_err(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


class Case:
    def __init__(self, tree, seed):
        self.tree, self.seed = tree, seed
        self.T = pm.TREES[tree]
        self.inp = pm.Inputs(problem(tree), seed)
        self.ops = pm.sequence(tree, seed)
        self.m = pm.Model(self.T["has_ahead"])
        self.i = 0

    def where(self, what):
        op = self.ops[self.i]
        return (f"{what}\ntree {self.tree} seed {self.seed} operation {self.i} {pm.show(op)}\nflags before it: {self.flags}\n"
                f"python -m tests.protocol_model --tree {self.tree} --seed {self.seed} --upto {self.i}\n"
                + pm.describe(self.ops, self.T["has_ahead"], self.i))

    def same(self, name, a, b, rounding):
        """Two handles' values of one quantity: bit for bit, or (documented, see above) to GRAM_CACHE_TOL."""
        if rounding:
            err = relerr(a, b) if np.ndim(a) else scalar_err(a, b)
            note(self.tree, "lazy/eager " + name, err)
            assert err <= GRAM_CACHE_TOL, self.where(f"lazy and eager differ in {name} by {err:.3g} (cached Gram parts: {GRAM_CACHE_TOL})")
        else:
            assert np.array_equal(a, b), self.where(f"lazy and eager differ in {name}: max |diff| {np.abs(np.asarray(a) - np.asarray(b)).max():.3g}")

    def close(self, who, name, got, want, tol):
        err = relerr(got, want) if np.ndim(want) else scalar_err(got, want)
        note(self.tree, name, err)
        assert err <= tol, self.where(f"{who}: {name} is {err:.3g} from the oracle (tolerance {tol})")

    def against_oracle(self, who, op, o, oo, w_tol):
        n = op.name
        if "ll" in o:
            self.close(who, "log-density", o["ll"], oo["ll"], w_tol)
        if n == "get_w":
            self.close(who, "w", o["w"], oo["w"], w_tol)
        elif n == "yhat":
            self.close(who, "yhat", o["yhat"], oo["yhat"], w_tol)
        elif n == "beta_stats":
            self.close(who, "xty", o["xty"], oo["xty"], w_tol)
        elif n == "tausq_stats":
            self.close(who, "ssq", o["ssq"], oo["ssq"], w_tol)
        elif n == "get_comps":
            self.close(who, "logdet comps", o["logdet"], oo["logdet"], REL)
            self.close(who, "loglik comps", o["loglik"], oo["loglik"], w_tol)
        elif n == "get_block":
            N, Ri = o["N"], o["Ri"]
            if oo["H"] is not None:
                H = -np.linalg.solve(Ri, N) if Ri.ndim == 2 else -N / Ri[:, None]
                self.close(who, "H", H, oo["H"], H_TOL)
            self.close(who, "Ri", Ri, oo["Ri"], REL)
        elif n == "get_resid" and oo["resid"] is not None:
            want = oo["resid"]
            scale = max(np.abs(e).max() for e in want.values())      # tests/test_gpu_gather_g.py: check_resid
            pb = self.inp.pb
            err = max(float(np.abs(o["resid"][pb["indexing"][u]] - e).max()) for u, e in want.items()) / scale
            note(self.tree, "residuals", err)
            assert err <= w_tol, self.where(f"{who}: residuals are {err:.3g} from the oracle (tolerance {w_tol})")

    def run(self):
        T, inp, m = self.T, self.inp, self.m
        lazy = pm.HipExecutor(inp, True, **T["handle"])
        eager = pm.HipExecutor(inp, False, **T["handle"])
        oracle = pm.OracleExecutor(inp)
        bad_code = None
        try:
            assert (lazy.lib.st_factor_ahead_levels(lazy.h) > 0) == T["has_ahead"], "the model's has_ahead is not the tree's"
            if inp.blocks["empty"] is None:
                pytest.fail("the tree has no block without an observed row")
            for self.i, op in enumerate(self.ops):
                self.flags = m.flags()
                cls = m.classify(op)
                assert cls != pm.UNSPECIFIED, self.where("the generator emitted an unspecified operation")
                before = lazy.snapshot(m) if cls == pm.REFUSED else None
                ol, oe, oo = lazy.step(op, m, cls), eager.step(op, m, cls), oracle.step(op, m, cls)
                if cls == pm.REFUSED:
                    assert ol["rc"] < 0 and ol["err"], self.where(f"expected a refusal with a text, got {ol}")
                    after = lazy.snapshot(m)
                    for k in before:
                        assert before[k].tobytes() == after[k].tobytes(), self.where(f"the refused call changed {k}")   # (NaN included)
                    continue
                m.apply(op)
                if oe is None:                          # st_factor_begin, st_factor_ahead_enable: the lazy handle alone
                    assert ol["rc"] == 0, self.where(f"return code {ol['rc']}: {ol.get('err')}")
                    continue
                assert ol["rc"] == oe["rc"] == oo["rc"], self.where(f"return codes: lazy {ol['rc']} ({ol.get('err')}), eager {oe['rc']}, oracle {oo['rc']}")
                assert (ol["rc"] > 0) == (cls == pm.FAILS), self.where(f"the model says {cls}, the code is {ol['rc']}")
                if ol["rc"] > 0:
                    bad_code = ol["rc"]
                    continue
                # which of the handles' values may differ in the last bits (the state after the operation)
                n, s = op.name, op.slot
                rounding = {"factor": m.comps_rounding[s] if s is not None else False, "finish": m.open_rounding,
                            "sweep_end": m.pending_rounding, "get_resid": m.resid_rounding}.get(n, m.w_rounding)
                for k in ol:
                    if k == "rc":
                        continue
                    theta_only = k in ("N", "Ri", "logdet")
                    r = (m.comps_rounding[s] if n == "get_comps" else rounding) and not theta_only
                    self.same(f"{pm.kind(op)}.{k}", ol[k], oe[k], r)
                w_tol = REL if m.w_sweeps <= 3 else CHAIN_TOL
                for who, o in (("lazy", ol), ("eager", oe)):
                    self.against_oracle(who, op, o, oo, w_tol)
        finally:
            lazy.close()
            eager.close()
        return bad_code


def test_the_trees_have_the_machinery_the_sequences_are_about(monkeypatch):
    """Tree a: levels that run ahead of time, a k_factor_quad<.., false, true> leaf level whose T a proposal defers, a
    k_factor_quad<.., true, ..> reference level, blocks without an observed row.  The others: the routes they are here for."""
    import ctypes as C
    want = {"a": (["k_factor_quad<4, 32, 8, true, true>", "k_factor_quad<4, 32, 8, false, true>"], ["k_sample_lean<true>", "k_sample_leaf_seg<4>"]),
            "b": (["k_factor_lchain<96>", "k_factor_ref_finish", "k_factor_bigmfma<3, 5, 34>"], ["k_gram_big"]),
            "c": (["k_factor_wide<WG_JT>"], ["k_gram_big"]),
            "d": (["k_factor<true, MODE_FACTOR>"], ["k_gram_big", "k_sample<true, false>"]),
            "e": (["k_marginal_invchol_wave"], [])}
    for tree, T in pm.TREES.items():
        with monkeypatch.context() as mp:
            set_env(tree, mp)
            inp = pm.Inputs(problem(tree), 0)
            ex = pm.HipExecutor(inp, True, **T["handle"])
            try:
                hm, m = ex.hm, pm.Model(T["has_ahead"])
                ahead = hm.lib.st_factor_ahead_levels(hm.h)
                assert (ahead > 0) == T["has_ahead"], (tree, ahead)
                assert inp.blocks["empty"] is not None, tree
                for op in (pm.Op("factor", slot=0, tid=0), pm.Op("enqueue", slot=1, tid=1), pm.Op("finish")):
                    assert ex.step(op, m, pm.LEGAL)["rc"] == 0
                a_routes = {a for g in hm.route_info()["levels"] for a in g["A"]}
                sweeps = set()
                for key in (1, 2):
                    assert ex.step(pm.Op("sample", key=key), m, pm.LEGAL)["rc"] == 0
                    sweeps |= {x for g in hm.route_info()["levels"] for x in (g["gram"], g["sweep"]) if x}
                print(f"tree {tree}: n {inp.n}, levels ahead {ahead}, phase A {sorted(a_routes)}, sweeps {sorted(sweeps)}")
                assert set(want[tree][0]) <= a_routes and set(want[tree][1]) <= sweeps, (tree, a_routes, sweeps)
                if tree == "a":
                    leaf = hm.route_info()["levels"][-1]["A"]
                    assert leaf == ["k_factor_quad<4, 32, 8, false, true>"], leaf        # the level st_factor_enqueue(1, .) defers
                    ll = C.c_double()
                    assert hm.lib.st_loglik_w(hm.h, 1, C.byref(ll)) == 0                  # ... finished by this reader
            finally:
                ex.close()


@pytest.mark.parametrize("tree,seed", pm.cases(), ids=[f"{t}-{s}" for t, s in pm.cases()])
def test_lazy_eager_and_oracle_agree_after_every_operation(tree, seed, monkeypatch):
    set_env(tree, monkeypatch)
    case = Case(tree, seed)
    bad_code = case.run()
    OBSERVED[(tree, "cases")] = OBSERVED.get((tree, "cases"), 0) + 1
    if bad_code is not None:
        OBSERVED[(tree, "failing theta's code")] = bad_code


def test_zz_report_the_largest_observed_error():
    """Prints, per tree and quantity, the largest error against the oracle and the largest difference between the two handles
    where the cached Gram parts allow one (DESIGN.md records them); fails unless cases ran (run with the file)."""
    assert any(k[1] == "cases" for k in OBSERVED), "no sequence was replayed"
    for (tree, quantity), v in sorted(OBSERVED.items()):
        print(f"tree {tree}  {quantity:38s} {v:.3g}")
    worst = max((v for (t, q), v in OBSERVED.items() if q.startswith("lazy/eager")), default=0.0)
    assert worst <= GRAM_CACHE_TOL
