"""CPU-only: the helper that widens a synthetic problem past eight covariates (tests.util.make_problem builds p <= 8, its
beta_true has eight entries), and the checks of the wide-regression feature that need no GPU: the helper changes nothing it
should keep, the front door of simulate() accepts 1 <= p <= ST_MAX_P, and the extended-precision statistics reference of
tests/test_outputs_reference.py is right on a widened problem.  tests/test_gpu_wide_regression.py imports `widen` from here."""
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import test_outputs_reference as ref
from tests.util import make_problem, oracle_model

ST_MAX_P = 64           # include/spamtree_hip.h
U = 2.0 ** -53


def widen(pb, p, seed=1234):
    """In place: append p - 8 seeded standard-normal columns to the X of a problem built with p = 8 and set pb["p"].  y, the tree
    and the first eight columns stay as they are (y does not depend on the new columns).  Returns pb."""
    assert pb["p"] == 8 and pb["X"].shape[1] == 8 and p > 8
    extra = np.random.default_rng(seed).standard_normal((pb["n"], p - 8))
    pb["X"] = np.ascontiguousarray(np.hstack([pb["X"], extra]))
    pb["p"] = p
    return pb


def test_widen_keeps_y_and_the_first_eight_columns():
    kw = dict(side=6, q=2, seed=3, p=8, missing=0.2)
    base = make_problem(**kw)
    for p in (9, 20, 64):
        pb = widen(make_problem(**kw), p)
        assert pb["p"] == p and pb["X"].shape == (72, p) and np.isfinite(pb["X"]).all()
        assert np.array_equal(pb["y"], base["y"], equal_nan=True) and np.array_equal(pb["X"][:, :8], base["X"])
        assert np.array_equal(pb["mv_id"], base["mv_id"]) and np.array_equal(pb["coords"], base["coords"])
        assert np.all(pb["X"][:, 8:].std(axis=0) > 0.5)
    # the same seed gives the same columns
    assert np.array_equal(widen(make_problem(**kw), 20)["X"], widen(make_problem(**kw), 20)["X"])


def test_header_and_binding_state_the_same_limit():
    import os
    import re
    from spamtree_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spamtree_hip.h")).read()
    assert int(re.search(r"#define\s+ST_MAX_P\s+(\d+)", hdr).group(1)) == ST_MAX_P == _lib.ST_MAX_P


@pytest.mark.parametrize("p,ok", [(1, True), (8, True), (9, True), (64, True), (65, False), (0, False)])
def test_simulate_input_check_accepts_up_to_st_max_p(p, ok, monkeypatch):
    """The front door of simulate(): X with 1 <= p <= ST_MAX_P columns passes the input check (and comes back unchanged with a
    p x q beta), p = 65 is refused with the limit in the text; nothing loads the library before the check."""
    from spamtree_amd import _lib, simulate

    def no_load():
        raise AssertionError("the library was loaded before the inputs were checked")
    monkeypatch.setattr(_lib, "load", no_load)
    rng = np.random.default_rng(p)
    coords, X = rng.uniform(size=(50, 2)), rng.standard_normal((50, p))
    args = (coords, [2.3, 1.0, 1.0, 6.0], None, X, np.arange(p, dtype=np.float64), None, 1)
    if ok:
        out = simulate._check_inputs(*args)
        assert np.array_equal(out[4], X) and out[5].shape == (p, 1)
    else:
        with pytest.raises(ValueError, match=str(ST_MAX_P)):
            simulate._check_inputs(*args)
        with pytest.raises(ValueError, match=str(ST_MAX_P)):
            simulate.simulate(coords, [2.3, 1.0, 1.0, 6.0], X=X, beta=np.zeros(p))


def test_reference_statistics_against_exact_rationals_at_p20():
    """ref_stats, ref_xb and ref_xtx on a widened p = 20 problem of a few dozen rows against exact rational arithmetic, both
    pairings, as test_reference_statistics_against_exact_rationals does at p = 4: the references the GPU tests compare with hold
    beyond eight columns (columns scaled up to 2^19 by scale_problem)."""
    p, q = 20, 3
    pb = ref.scale_problem(widen(make_problem(side=4, q=q, seed=9, p=8, missing=(0.1, 0.3, 0.5)), p))
    assert pb["n"] == 48 and pb["X"].shape == (48, p)
    w, B, _ = ref.scaled_state(pb, 1)
    assert B.shape == (p, q)
    mv0 = pb["mv_id"] - 1
    xb, bxb = ref.ref_xb(pb["X"], mv0, B)
    for i in range(pb["n"]):
        ex = sum(Fraction(pb["X"][i, k]) * Fraction(B[k, mv0[i]]) for k in range(p))
        assert abs(Fraction(xb[i]) - ex) <= Fraction(bxb[i]) / 1000 + Fraction(U) * abs(ex)
    om = oracle_model(pb)
    xtx, btx = ref.ref_xtx(pb["y"], pb["X"], mv0, q)
    for partner in (None, ref.quirk_partner(om, pb["n"])):
        xty, bx, ssq, bs, n_obs = ref.ref_stats(pb["y"], pb["X"], mv0, w, xb, q, partner)
        pr = np.arange(pb["n"]) if partner is None else partner
        for j in range(q):
            rows = [i for i in range(pb["n"]) if mv0[i] == j and math.isfinite(pb["y"][i])]
            assert n_obs[j] == len(rows) > 0
            for k in range(p):
                ex = sum(Fraction(pb["X"][i, k]) * (Fraction(pb["y"][i]) - Fraction(w[pr[i]])) for i in rows)
                assert abs(Fraction(xty[k, j]) - ex) <= Fraction(bx[k, j]) / 1000 + Fraction(U) * abs(ex)
            ex = sum((Fraction(pb["y"][i]) - Fraction(xb[i]) - Fraction(w[i])) ** 2 for i in rows)
            assert abs(Fraction(ssq[j]) - ex) <= Fraction(bs[j]) / 1000 + Fraction(U) * ex
            if partner is None:
                for a in (0, 7, 8, 19):
                    for b in (0, 8, 19):
                        ex = sum(Fraction(pb["X"][i, a]) * Fraction(pb["X"][i, b]) for i in rows)
                        assert abs(Fraction(xtx[j, a, b]) - ex) <= Fraction(btx[j, a, b]) / 1000 + Fraction(U) * abs(ex)
    # the oracle's own statistics at p = 20 agree to its double-precision rounding
    om.w, om.XB = w.copy(), xb.copy()
    oxty, ossq = om.beta_tausq_stats()
    xty, bx, ssq, bs, _ = ref.ref_stats(pb["y"], pb["X"], mv0, w, xb, q, ref.quirk_partner(om, pb["n"]))
    assert np.all(np.abs(oxty - xty) <= 100 * bx) and np.all(np.abs(ossq - ssq) <= 100 * bs)
