"""GPU: more than eight covariates (9 <= p <= ST_MAX_P = 64) through every layer -- the tiled k_stats (one slice of eight columns
of X per grid row), XtX formed on the device by the same kernel body, XB, yhat, the statistics cache, whole chains of both host
drivers against the oracle, new-point prediction and simulation.  Problems are tests.util.make_problem(p = 8) widened by
tests/test_wide_regression_cpu.widen; references and bounds are those of tests/test_outputs_reference.py, unchanged, and the
helpers of tests/test_gpu_outputs.py drive the handle."""
import ctypes as C

import numpy as np
import pytest

from tests import test_gpu_outputs as out
from tests import test_outputs_reference as ref
from tests.test_wide_regression_cpu import ST_MAX_P, widen
from tests.util import make_problem

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble
MISSING6 = out.MISSING6
_dp, _f = out._dp, out._f


def wide_problem(p, **kw):
    return widen(make_problem(p=8, **kw), p)


# ----------------------------------------------------------------------------------------------------------------------
# 1. statistics, XB, yhat, XtX against extended precision
# ----------------------------------------------------------------------------------------------------------------------
# slices of k_stats: p = 9 one column in the second, 16 two full ones, 17 and 33 one column in the last, 64 eight full ones;
# n = 144 q is fewer rows than the 1024 workgroups, 54 rows one block, 16129 = 63 * 256 + 1, 18000 a chunk of 18 rows.
WIDE_CASES = [
    dict(p=9, q=1, side=12, missing=0.12, quirks=1),
    dict(p=16, q=2, side=12, missing=0.0, quirks=0),
    dict(p=17, q=3, side=12, missing=0.12, quirks=1),
    dict(p=33, q=6, side=12, missing=MISSING6, quirks=0),
    dict(p=64, q=6, side=12, missing=MISSING6, quirks=1),             # nq = 390
    dict(p=64, q=6, side=3, missing=0.0, quirks=1),                   # one block, 54 rows
    dict(p=9, q=1, side=127, missing=0.12, quirks=1),                 # n = 16129 = 63 * 256 + 1
    dict(p=40, q=5, side=60, missing=0.12, quirks=0),                 # n = 18000
]


@pytest.mark.parametrize("case", WIDE_CASES, ids=lambda c: "p{p}q{q}s{side}k{quirks}".format(**c))
def test_wide_statistics_xb_yhat_xtx_match_extended_precision(case):
    """The sequence of test_statistics_xb_yhat_xtx_match_extended_precision at p > 8: after st_create, st_set_w and st_set_beta the
    statistics are within ref_stats' (D + 3) 2^-53 sum|t_i| (D = ref.stats_depth(n): the order of additions does not depend on p),
    XB and yhat within (p + 5) 2^-53 sum|t|, XtX within ref_xtx's (n_j + 3) 2^-53 sum|t| and symmetric to the bit, n_obs_by_q
    exact.  Outcome j is scaled by 10^j and column k of X by 2^k, so a wrong slice, column or outcome is an O(1) error."""
    c = dict(case)
    p, q, quirks = c.pop("p"), c.pop("q"), c.pop("quirks")
    pb = ref.scale_problem(wide_problem(p, seed=41, q=q, **c))
    assert pb["X"].shape == (pb["n"], p)
    mv0 = pb["mv_id"] - 1
    n_obs = np.array([np.isfinite(pb["y"][mv0 == j]).sum() for j in range(q)])
    if c["side"] <= 5:
        assert len(pb["block_names"]) == 1 and pb["n"] < 64
    hm = out.hip_model(pb, quirks=bool(quirks))
    partner = out.partner_of(pb, quirks)
    if quirks and np.any(~np.isfinite(pb["y"])):
        assert np.any(partner != np.arange(pb["n"]))
    xtx, bx = ref.ref_xtx(pb["y"], pb["X"], mv0, q)
    for j in range(q):
        err = np.abs(hm.XtX[j] - xtx[j])
        print(f"XtX[{j}] err/bound {np.max(err / np.maximum(bx[j], 1e-300)):.3g}")
        assert hm.XtX[j].shape == (p, p) and np.all(err <= bx[j]), j
        assert np.array_equal(hm.XtX[j], hm.XtX[j].T), j
    assert np.array_equal(hm.n_obs_by_q, n_obs)
    out.assert_stats(hm, pb, partner, "created (w = 0, XB = 0)")
    w, B, tsq_inv = ref.scaled_state(pb, 7)
    hm.set_w(w)
    out.assert_stats(hm, pb, partner, "after st_set_w")
    hm.beta_update(B)
    xb, bxb = ref.ref_xb(pb["X"], mv0, B)
    got = hm.get_XB()
    print(f"XB err/bound {np.max(np.abs(got - xb) / np.maximum(bxb, 1e-300)):.3g}")
    assert np.all(np.abs(got - xb) <= bxb)
    out.assert_stats(hm, pb, partner, "after st_set_beta")
    assert hm.lib.st_set_tausq_inv(hm.h, _dp(tsq_inv)) == 0
    noise = np.random.default_rng(3).standard_normal(pb["n"])
    yh, byh = ref.ref_yhat(pb["X"], mv0, B, w, tsq_inv, noise)
    got = hm.yhat(noise)
    print(f"yhat err/bound {np.max(np.abs(got - yh) / byh):.3g}")
    assert np.all(np.abs(got - yh) <= byh)
    hm.close()


# ----------------------------------------------------------------------------------------------------------------------
# 2. the statistics cache at p = 20 (three slices, nq = 42: fetched on demand, not through the pinned prefetch)
# ----------------------------------------------------------------------------------------------------------------------
def test_wide_statistics_cache_follows_every_change_of_w_and_xb():
    """The pattern of test_statistics_cache_follows_every_change_of_w_and_xb at p = 20, q = 2: after every call that changes w or
    XB the statistics equal the reference for the state the handle holds (and a second request returns the same bits:
    assert_stats asks twice); calls that change no state leave them bit-identical; a reduction started under phase A of a
    proposal is the one for the state at that moment."""
    p, q = 20, 2
    pb = ref.scale_problem(wide_problem(p, side=10, q=q, seed=47, missing=0.15, cell_size=4))
    hm = out.hip_model(pb, quirks=True)
    lib, h = hm.lib, hm.h
    partner = out.partner_of(pb, True)
    w, B, tsq_inv = ref.scaled_state(pb, 9)
    theta = _f(pb["theta"])
    ll = C.c_double()
    s0 = out.assert_stats(hm, pb, partner, "created")
    assert lib.st_set_w(h, _dp(_f(w))) == 0
    s1 = out.assert_stats(hm, pb, partner, "st_set_w")
    assert not np.array_equal(s0[0], s1[0]) and not np.array_equal(s0[1], s1[1])
    assert lib.st_set_beta(h, _dp(B)) == 0
    s2 = out.assert_stats(hm, pb, partner, "st_set_beta")
    assert np.array_equal(s1[0], s2[0]) and not np.array_equal(s1[1], s2[1])       # xty does not read XB, ssq does
    assert lib.st_factor(h, 0, _dp(theta), theta.size, C.byref(ll)) == 0
    out.assert_stats(hm, pb, partner, "st_factor(0)")
    assert lib.st_sample_w(h, None, 11, 1) == 0
    s3 = out.assert_stats(hm, pb, partner, "st_sample_w")
    assert lib.st_sample_w_loglik(h, None, 11, 2, 0, C.byref(ll)) == 0
    s4 = out.assert_stats(hm, pb, partner, "st_sample_w_loglik")
    assert not np.array_equal(s3[0], s4[0])
    # ---- calls that change no state: bit-identical statistics
    buf = np.zeros(pb["n"])
    before = out.raw_stats(hm)
    for name, call in (("st_set_tausq_inv", lambda: lib.st_set_tausq_inv(h, _dp(tsq_inv))),
                       ("st_yhat", lambda: lib.st_yhat(h, None, 11, 4, _dp(buf)))):
        assert call() == 0, name
        after = out.raw_stats(hm)
        assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1]), name
    # ---- the driver's overlap: the reduction starts under phase A of the proposal and is fetched before st_factor_finish
    th2 = _f(theta * 1.01)
    assert lib.st_sample_w(h, None, 11, 5) == 0
    assert lib.st_factor_enqueue(h, 1, _dp(th2), th2.size) == 0
    got = out.raw_stats(hm)
    assert lib.st_factor_finish(h, C.byref(ll)) == 0
    s5 = out.assert_stats(hm, pb, partner, "st_factor_enqueue(1) .. statistics .. st_factor_finish", got=got)
    B2 = np.asfortranarray(B * 0.5 + 1.0)
    assert lib.st_set_beta(h, _dp(B2)) == 0
    s6 = out.assert_stats(hm, pb, partner, "st_set_beta again")
    assert not np.array_equal(s5[1], s6[1])
    hm.close()


# ----------------------------------------------------------------------------------------------------------------------
# 3. the limit
# ----------------------------------------------------------------------------------------------------------------------
def test_more_than_st_max_p_covariates_are_refused():
    from spamtree_amd.model import SpamTreeError
    pb = wide_problem(ST_MAX_P + 1, side=6, q=1, seed=2)
    with pytest.raises(SpamTreeError, match=rf"\(-4\).*\b{ST_MAX_P}\b"):
        out.hip_model(pb)
    hm = out.hip_model(wide_problem(ST_MAX_P, side=6, q=1, seed=2))          # the limit itself is accepted
    assert hm.p == ST_MAX_P and hm.XtX[0].shape == (ST_MAX_P, ST_MAX_P)
    hm.close()


# ----------------------------------------------------------------------------------------------------------------------
# 4. whole chains
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [dict(side=25, q=1, seed=11, missing=0.1, p=12), dict(side=12, q=2, seed=12, p=20)],
                         ids=lambda c: "p{p}q{q}".format(**c))
def test_wide_cpp_and_python_drivers_match_oracle_chain(case):
    """tests/test_gpu_chain.py::test_cpp_and_python_drivers_match_oracle_chain with its settings and tolerances (1e-8 on the
    traces, w and yhat, 1e-7 on paramsd) on widened problems: the beta draw is a p x p Cholesky of tausq_inv XtX + Vi, so XtX from
    the device and beta_mcmc of p x keep x q are both in the comparison."""
    from oracle import spamtree_oracle as so
    from spamtree_amd import fit, mcmc
    from tests.test_gpu_chain import args_of, relerr
    c = dict(case)
    p = c.pop("p")
    pb = wide_problem(p, **c)
    k = pb["theta"].size
    kw = dict(mcmc_keep=4, mcmc_burn=58, mcmc_thin=2, adapting=True, seed=99, main_verbose=False)
    want = so.spamtree_mv_mcmc(*args_of(pb, k), **kw)
    assert np.asarray(want["beta_mcmc"]).size == p * 4 * pb["q"]
    for drv in (fit.spamtree_mv_mcmc, mcmc.spamtree_mv_mcmc):
        got = drv(*args_of(pb, k), **kw)
        assert "None" not in got
        assert np.asarray(got["beta_mcmc"]).shape == np.asarray(want["beta_mcmc"]).shape
        assert relerr(got["theta_mcmc"], want["theta_mcmc"]) < 1e-8
        assert relerr(got["tausq_mcmc"], want["tausq_mcmc"]) < 1e-8
        assert relerr(got["beta_mcmc"], want["beta_mcmc"]) < 1e-8
        assert relerr(got["paramsd"], want["paramsd"]) < 1e-7
        for i in range(4):
            assert relerr(np.asarray(got["w_mcmc"][i]).reshape(-1), want["w_mcmc"][i]) < 1e-8
            assert relerr(np.asarray(got["yhat_mcmc"][i]).reshape(-1), want["yhat_mcmc"][i]) < 1e-8


# ----------------------------------------------------------------------------------------------------------------------
# 5. new points, 6. simulation: the other two readers of p columns
# ----------------------------------------------------------------------------------------------------------------------
def test_new_point_yhat_reads_every_column_of_x_new():
    """st_points_predict in mode 1 (conditional mean, no noise) with X_new of n_new x 12: yhat_new - cond_mean = X_new . B[:, mv]
    within (p + 6) 2^-53 (sum|x b| + |cond_mean|) -- a serial sum of p products and one add, p + 1 roundings, and the rounding
    of the difference formed here is below 2^-64 of the same magnitude."""
    from spamtree_amd.predict import locate
    p, q, n_new = 12, 2, 37
    pb = ref.scale_problem(wide_problem(p, side=20, q=q, seed=5, missing=0.1))
    hm = out.hip_model(pb, tausq=0.2)
    w, B, _ = ref.scaled_state(pb, 6)
    hm.set_w(w)
    hm.beta_update(B)
    assert hm.get_loglik_comps_w(0)
    rng = np.random.default_rng(8)
    lo, hi = pb["coords"].min(axis=0), pb["coords"].max(axis=0)
    pts = lo + (hi - lo) * rng.uniform(size=(n_new, 2))
    mv = rng.integers(1, q + 1, size=n_new)
    X_new = rng.standard_normal((n_new, p)) * 2.0 ** np.arange(p)[None, :]
    hm.set_points(pts, mv, locate(pb["topo"], pts, mv, device=0), X=X_new)
    got = hm.predict_points(mode=1)
    assert np.array_equal(got["w"], got["mean"]) and np.all(np.isfinite(got["yhat"]))
    t = X_new.astype(LD) * B.T[mv - 1].astype(LD)
    want = t.sum(axis=1)
    bound = (p + 6) * U * (np.abs(t).sum(axis=1) + np.abs(got["mean"].astype(LD)))
    err = np.abs(got["yhat"].astype(LD) - got["mean"].astype(LD) - want)
    print(f"new-point XB err/bound {float(np.max(err / bound)):.3g}")
    assert np.all(err <= bound)
    assert float(np.median(np.abs(want) / bound)) > 1e6          # the regression part is really there
    hm.close()


def test_simulated_outcomes_read_every_column_of_x():
    """st_simulate with the caller's z and eps at p = 12, through SpamTreeMV.simulate as tests/test_gpu_simulate.py drives it:
    y_out = XB + w_out + tau_j eps per draw, within ref_yhat's (p + 5) 2^-53 sum|t| for the w_out the call returned."""
    p, q, nd = 12, 2, 2
    pb = ref.scale_problem(wide_problem(p, side=14, q=q, seed=5))
    mv0 = pb["mv_id"] - 1
    hm = out.hip_model(pb, tausq=0.2)
    _, B, _ = ref.scaled_state(pb, 4)
    hm.beta_update(B)
    assert hm.get_loglik_comps_w(0)
    rng = np.random.default_rng(1)
    z, eps = rng.standard_normal((pb["n"], nd)), rng.standard_normal((pb["n"], nd))
    w_out, y_out = hm.simulate(nd, z=z, eps=eps)
    assert w_out.shape == (pb["n"], nd) and np.all(w_out.std(axis=0) > 0)
    for d in range(nd):
        yr, byr = ref.ref_yhat(pb["X"], mv0, B, w_out[:, d], np.full(q, 1.0 / 0.2), eps[:, d])
        print(f"draw {d}: y err/bound {np.max(np.abs(y_out[:, d] - yr) / byr):.3g}")
        assert np.all(np.abs(y_out[:, d] - yr) <= byr)
    hm.close()
