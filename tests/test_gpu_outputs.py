"""GPU: what the chain REPORTS -- the beta / tausq statistics, XB, yhat, XtX, the running means, the quantiles, the per-point
summaries and the exported CrossCovarianceAG10 -- at the shapes where such kernels go wrong, against references that do not share
their code (tests/test_outputs_reference.py: extended-precision restatements of the header's definitions, exact rationals,
oracle.list_summaries.list_qtile).  Every tolerance is a derived bound stated where it is computed (there or here), or a
constant the suite already uses for the same quantity (1e-13 on the device normals, 1e-14 max|ref| on the cross-covariance).

Handles come from spamtree_amd.model.SpamTreeMV as in tests/test_gpu_parity.py; most cases need st_create only.
"""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

from oracle.list_summaries import list_qtile
from tests import test_outputs_reference as ref
from tests.util import make_problem, nice_theta, oracle_model

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
ST_ERR_USAGE, ST_ERR_UNSUPPORTED = -1, -4
MISSING6 = (0.1, 0.3, 0.5, 0.0, 0.9, 0.2)


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def hip_model(pb, quirks=True, tausq=0.25, beta=None):
    from spamtree_amd.model import SpamTreeMV
    return SpamTreeMV(pb["y"], pb["X"], pb["Z"], pb["coords"], pb["mv_id"], pb["blocking"], pb["gix_block"], pb["res_is_ref"],
                      pb["parents"], pb["children"], False, pb["block_names"], pb["block_groups"], pb["indexing"],
                      np.zeros(pb["n"]), np.zeros(pb["p"]) if beta is None else beta, pb["theta"], 1.0 / tausq,
                      reference_quirks=quirks)


def raw_stats(hm):
    """(xty p x q, ssq q, n_obs q) straight from st_beta_stats / st_tausq_stats."""
    xty, ssq, nobs = np.zeros(hm.p * hm.q), np.zeros(hm.q), np.zeros(hm.q, dtype=np.int64)
    assert hm.lib.st_beta_stats(hm.h, _dp(xty)) == 0
    assert hm.lib.st_tausq_stats(hm.h, _dp(ssq), nobs.ctypes.data_as(C.POINTER(C.c_int64))) == 0
    return xty.reshape(hm.q, hm.p).T.copy(), ssq, nobs


def partner_of(pb, quirks):
    return ref.quirk_partner(oracle_model(pb), pb["n"]) if quirks else None


def assert_stats(hm, pb, partner, tag, got=None):
    """The statistics equal the extended-precision reference for the w and XB the handle holds now, per entry within the bound of
    ref_stats ((D + 3) 2^-53 sum |t_i|, D = ref.stats_depth(n)); asking again returns the same bits."""
    xty, ssq, nobs = raw_stats(hm) if got is None else got
    w, xb = hm.get_w(), hm.get_XB()
    rx, bx, rs, bs, rn = ref.ref_stats(pb["y"], pb["X"], pb["mv_id"] - 1, w, xb, pb["q"], partner)
    ex, es = np.abs(xty - rx), np.abs(ssq - rs)
    print(f"{tag}: xty err/bound {np.max(ex / np.maximum(bx, 1e-300)):.3g}  ssq err/bound {np.max(es / np.maximum(bs, 1e-300)):.3g}")
    assert np.array_equal(nobs, rn), tag
    assert np.all(ex <= bx), (tag, xty, rx, bx)
    assert np.all(es <= bs), (tag, ssq, rs, bs)
    again = raw_stats(hm)
    assert np.array_equal(again[0], xty) and np.array_equal(again[1], ssq), tag
    return xty, ssq


# ----------------------------------------------------------------------------------------------------------------------
# 1. statistics, XB, yhat, XtX against extended precision
# ----------------------------------------------------------------------------------------------------------------------
# the (p, q) axis in full at side 12 (n = 144 q: fewer rows than the 1024 workgroups of k_stats), then the other sizes: a
# one-block tree of < 64 rows, n = 16129 = 63 * 256 + 1, and tens of thousands of rows; every missing pattern and both
# pairings at least once.  p * q + q = 2, 8, 9, 40, 42, 54.
STAT_CASES = [
    dict(p=1, q=1, side=12, missing=0.12, quirks=1),
    dict(p=3, q=2, side=12, missing=0.0, quirks=1),
    dict(p=8, q=1, side=12, missing=0.12, quirks=0),
    dict(p=7, q=5, side=12, missing=MISSING6[:5], quirks=1),
    dict(p=6, q=6, side=12, missing=0.12, quirks=1, single_obs=2),
    dict(p=8, q=6, side=12, missing=MISSING6, quirks=0),
    dict(p=3, q=2, side=5, missing=0.0, quirks=0),                    # one block, 50 rows
    dict(p=8, q=6, side=3, missing=0.0, quirks=1),                    # one block, 54 rows
    dict(p=8, q=1, side=127, missing=0.12, quirks=1),                 # n = 16129 = 1 mod 256
    dict(p=7, q=5, side=60, missing=0.12, quirks=0, single_obs=3),    # n = 18000
    dict(p=8, q=6, side=70, missing=MISSING6, quirks=1),              # n = 29400
]


@pytest.mark.parametrize("case", STAT_CASES, ids=lambda c: "p{p}q{q}s{side}k{quirks}".format(**c))
def test_statistics_xb_yhat_xtx_match_extended_precision(case):
    """k_xb, k_stats + k_stats_final, k_yhat and the host XtX against the long-double restatements of the header's definitions.
    Outcome j's y, w, Bcoeff[:, j] and tau_j are scaled by 10^j and column k of X by 2^k, so a wrong outcome or column index is
    an O(1) relative error.  Bounds per entry (derivations in tests/test_outputs_reference.py): statistics (D + 3) 2^-53 sum|t_i|
    with D = ceil(ceil(n / 1024) / 256) + 6 + 4 + 4 + 8 from the code; XB and yhat (p + 5) 2^-53 sum|t| (D = p + 2); XtX
    (n_j + 3) 2^-53 sum|t| (a serial host sum); n_obs_by_q exactly.  No shape was refused by st_create."""
    c = dict(case)
    p, q, quirks = c.pop("p"), c.pop("q"), c.pop("quirks")
    pb = ref.scale_problem(make_problem(seed=41, q=q, p=p, **c))
    mv0 = pb["mv_id"] - 1
    n_obs = np.array([np.isfinite(pb["y"][mv0 == j]).sum() for j in range(q)])
    if c.get("single_obs"):
        assert n_obs[c["single_obs"] - 1] == 1
    if c["side"] <= 5:
        assert len(pb["block_names"]) == 1 and pb["n"] < 64
    hm = hip_model(pb, quirks=bool(quirks))
    partner = partner_of(pb, quirks)
    if quirks and np.any(~np.isfinite(pb["y"])):
        assert np.any(partner != np.arange(pb["n"]))                    # the pairing really differs from the identity
    # XtX and n_obs as st_create computed them
    xtx, bx = ref.ref_xtx(pb["y"], pb["X"], mv0, q)
    for j in range(q):
        assert hm.XtX[j].shape == (p, p) and np.all(np.abs(hm.XtX[j] - xtx[j]) <= bx[j]), j
    assert np.array_equal(hm.n_obs_by_q, n_obs)
    assert_stats(hm, pb, partner, "created (w = 0, XB = 0)")
    w, B, tsq_inv = ref.scaled_state(pb, 7)
    hm.set_w(w)
    assert_stats(hm, pb, partner, "after st_set_w")
    hm.beta_update(B)
    xb, bxb = ref.ref_xb(pb["X"], mv0, B)
    got = hm.get_XB()
    print(f"XB err/bound {np.max(np.abs(got - xb) / np.maximum(bxb, 1e-300)):.3g}")
    assert np.all(np.abs(got - xb) <= bxb)
    assert_stats(hm, pb, partner, "after st_set_beta")
    # yhat with the caller's noise: an exact reference
    assert hm.lib.st_set_tausq_inv(hm.h, _dp(tsq_inv)) == 0
    noise = np.random.default_rng(3).standard_normal(pb["n"])
    yh, byh = ref.ref_yhat(pb["X"], mv0, B, w, tsq_inv, noise)
    got = hm.yhat(noise)
    print(f"yhat err/bound {np.max(np.abs(got - yh) / byh):.3g}")
    assert np.all(np.abs(got - yh) <= byh)
    if q > 1:       # the noise term is what separates the outcomes: with tau_0 everywhere the last outcome would be off by ~ tau_q
        j = q - 1
        assert np.median(np.abs(noise[mv0 == j]) / np.sqrt(tsq_inv[j])) > 1e3 * np.median(byh[mv0 == j])
    hm.close()


@pytest.mark.parametrize("q", [3, 6])
def test_yhat_with_device_noise(q):
    """yhat = XB + w + tau_j normal(stream 5) with the device's own normals, tau^-2 differing by two orders of magnitude from one
    outcome to the next, non-zero XB and w.  Bound: ref_yhat's (p + 5) 2^-53 sum|t| plus tau_j 1e-13, the suite's tolerance on
    the device normals themselves (test_device_normals_match_oracle_stream)."""
    from oracle.spamtree_oracle import StRng
    pb = ref.scale_problem(make_problem(side=12, q=q, p=4, seed=43, missing=0.12))
    mv0 = pb["mv_id"] - 1
    hm = hip_model(pb)
    w, B, tsq_inv = ref.scaled_state(pb, 8)
    hm.set_w(w)
    hm.beta_update(B)
    assert hm.lib.st_set_tausq_inv(hm.h, _dp(tsq_inv)) == 0
    for seed, it in ((2021, 7), (5, 0)):
        noise = StRng(seed).yhat_normals(it, pb["n"])
        yh, byh = ref.ref_yhat(pb["X"], mv0, B, w, tsq_inv, noise)
        got = hm.yhat(None, seed=seed, it=it)
        tol = byh + 1e-13 / np.sqrt(tsq_inv)[mv0]
        assert np.all(np.abs(got - yh) <= tol), np.max(np.abs(got - yh) / tol)
    hm.close()


# ----------------------------------------------------------------------------------------------------------------------
# 2. the statistics cache as a contract
# ----------------------------------------------------------------------------------------------------------------------
def _points_for(hm, pb, n_new, seed):
    from spamtree_amd.predict import locate
    rng = np.random.default_rng(seed)
    lo, hi = pb["coords"].min(axis=0), pb["coords"].max(axis=0)
    pts = lo + (hi - lo) * rng.uniform(size=(n_new, 2))
    mv = rng.integers(1, pb["q"] + 1, size=n_new)
    anchor = locate(pb["topo"], pts, mv, device=0)
    hm.set_points(pts, mv, anchor, X=rng.standard_normal((n_new, pb["p"])))
    return pts, mv


@pytest.mark.parametrize("p,q", [(3, 2), (7, 5), (6, 6), (8, 6)])
@pytest.mark.parametrize("missing", [0.15, 0.0])
def test_statistics_cache_follows_every_change_of_w_and_xb(p, q, missing):
    """After every call that changes w or XB the statistics equal the reference for the state at that moment (w and XB fetched
    from the handle); after every call documented to change no state they are bit-identical to before.  p q + q = 8, 40, 42, 54:
    up to 40 the results of a reduction started under phase A travel to pinned memory behind it, above they are fetched on
    demand.  The problem with missing outcomes exercises st_predict (and has st_simulate refused), the complete one st_simulate.
    reference_quirks = 1: the pairing reads w of NA rows too, so st_predict really changes xty."""
    pb = ref.scale_problem(make_problem(side=10, q=q, p=p, seed=47, missing=missing, cell_size=4))
    assert p * q + q == {(3, 2): 8, (7, 5): 40, (6, 6): 42, (8, 6): 54}[(p, q)]
    hm = hip_model(pb, quirks=True)
    lib, h = hm.lib, hm.h
    partner = partner_of(pb, True)
    rng = np.random.default_rng(2)
    w, B, tsq_inv = ref.scaled_state(pb, 9)
    theta = _f(pb["theta"])
    ll = C.c_double()
    assert_stats(hm, pb, partner, "created")
    assert lib.st_set_w(h, _dp(_f(w))) == 0
    assert_stats(hm, pb, partner, "st_set_w")
    assert lib.st_set_beta(h, _dp(B)) == 0
    assert_stats(hm, pb, partner, "st_set_beta")
    assert lib.st_factor(h, 0, _dp(theta), theta.size, C.byref(ll)) == 0
    assert_stats(hm, pb, partner, "st_factor(0)")
    assert lib.st_sample_w(h, None, 11, 1) == 0
    s1 = assert_stats(hm, pb, partner, "st_sample_w")
    assert lib.st_sample_w_loglik(h, None, 11, 2, 0, C.byref(ll)) == 0
    s2 = assert_stats(hm, pb, partner, "st_sample_w_loglik")
    assert not np.array_equal(s1[0], s2[0])
    assert lib.st_sample_w_loglik_begin(h, None, 11, 3, 0) == 0
    assert lib.st_sample_w_loglik_end(h, C.byref(ll)) == 0
    s3 = assert_stats(hm, pb, partner, "st_sample_w_loglik_begin/_end")
    assert not np.array_equal(s2[1], s3[1])
    if missing:
        w_before = hm.get_w()
        assert lib.st_predict(h, 1) == 0
        na = ~np.isfinite(pb["y"])
        w_after = hm.get_w()
        assert np.any(w_after[na] != w_before[na]) and np.array_equal(w_after[~na], w_before[~na])
        s4 = assert_stats(hm, pb, partner, "st_predict")
        assert not np.array_equal(s3[0], s4[0])            # the quirk pairing reads rows st_predict has just rewritten
    # ---- calls that change no state: bit-identical statistics
    _points_for(hm, pb, 9, 5)
    n = pb["n"]
    buf = [np.zeros(max(n, 16)) for _ in range(4)]
    calls = [
        ("st_set_tausq_inv", lambda: lib.st_set_tausq_inv(h, _dp(tsq_inv))),
        ("st_yhat", lambda: lib.st_yhat(h, None, 11, 4, _dp(buf[0]))),
        ("st_summary_accumulate", lambda: lib.st_summary_accumulate(h, 11, 4)),
        ("st_points_predict", lambda: lib.st_points_predict(h, 0, None, 11, 4, _dp(buf[0]), _dp(buf[1]), _dp(buf[2]), _dp(buf[3]))),
        ("st_points_accumulate", lambda: lib.st_points_accumulate(h, 11, 4, _dp(buf[0]), _dp(buf[1]), _dp(buf[2]), _dp(buf[3]))),
    ]
    before = raw_stats(hm)
    w_before, xb_before = hm.get_w(), hm.get_XB()
    for name, call in calls:
        assert call() == 0, name
        after = raw_stats(hm)
        assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1]), name
    wsim, ysim = np.zeros(n), np.zeros(n)
    rc = lib.st_simulate(h, 1, None, None, 11, 4, _dp(wsim), _dp(ysim))
    assert rc == (ST_ERR_UNSUPPORTED if missing else 0)
    after = raw_stats(hm)
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1]), "st_simulate"
    assert np.array_equal(hm.get_w(), w_before) and np.array_equal(hm.get_XB(), xb_before)
    assert_stats(hm, pb, partner, "after the calls that change nothing")
    # ---- the driver's overlap: the reduction starts under phase A of the proposal and is fetched before st_factor_finish
    th2 = _f(theta * (1.0 + 0.02 * rng.standard_normal(theta.size)))
    assert lib.st_sample_w(h, None, 11, 5) == 0
    assert lib.st_factor_enqueue(h, 1, _dp(th2), th2.size) == 0
    got = raw_stats(hm)
    assert lib.st_factor_finish(h, C.byref(ll)) == 0
    s5 = assert_stats(hm, pb, partner, "st_factor_enqueue(1) .. statistics .. st_factor_finish", got=got)
    # ---- ... and a change of XB after a reduction that has already started under phase A
    assert lib.st_sample_w(h, None, 11, 6) == 0
    assert lib.st_factor(h, 1, _dp(th2), th2.size, C.byref(ll)) == 0
    B2 = np.asfortranarray(B * 0.5 + 1.0)
    assert lib.st_set_beta(h, _dp(B2)) == 0
    s6 = assert_stats(hm, pb, partner, "st_factor(1) -> st_set_beta")
    assert not np.array_equal(s5[1], s6[1])
    hm.close()


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float64)


# ----------------------------------------------------------------------------------------------------------------------
# 3. quantiles: k_qtile through both of its callers
# ----------------------------------------------------------------------------------------------------------------------
_PB625 = []


def problem625():
    if not _PB625:
        _PB625.append(make_problem(side=25, q=1, p=2, seed=51))      # n = 625 = 1 mod 8, mod 4 and mod 2
    return _PB625[0]


def feed(hm, draws, seed=9, it0=0):
    """st_set_w(draw) + st_summary_accumulate per row of draws: the stored w draws are exactly `draws`."""
    for d in range(draws.shape[0]):
        assert hm.lib.st_set_w(hm.h, _dp(draws[d])) == 0
        assert hm.lib.st_summary_accumulate(hm.h, seed, it0 + d) == 0


def assert_qtile(got, draws, q, extra=0.0, tag=None):
    """got == list_qtile(draws, q) per row within ref.qtile_bound: 4 2^-53 (|lower| + |upper|) + 2^-1074."""
    want = list_qtile(list(draws), q)
    tol = ref.qtile_bound(draws, q) + extra
    bad = np.nonzero(~(np.abs(got - want) <= tol))[0]
    assert bad.size == 0, (tag, q, bad[:8], got[bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("keep", [1, 2, 3, 4, 5, 63, 64, 65, 1024, 1025, 2048, 2049, 4097, 8193, 16384])
def test_summary_quantiles_at_every_pad_and_row_count(keep):
    """st_summary_quantile on fed draws: every value of R (8 rows per workgroup up to keep = 2048, then 4, 2, 1), Kpad = keep and
    Kpad > keep, the first launch above 64 KiB of LDS (keep = 1025: 8 x 2048 doubles = 128 KiB) and the largest one, n = 625 not
    a multiple of R; rows of six kinds (ref.qtile_rows); for keep <= 65 every q = k / keep with both neighbours -- among them
    the 351 pairs on which the stepwise rounding of r decides the pick.  w quantiles at every keep; yhat quantiles against
    XB + w + tau StRng.yhat_normals up to keep = 1025 (not at the larger keeps), where the tolerance also carries the
    perturbation of the draws themselves (ref_yhat's bound + tau 1e-13: an order statistic moves by at most the largest
    perturbation of a draw, and the interpolation weights sum to 1).
    lds_limit: hipDeviceAttributeMaxSharedMemoryPerBlock reads 163840 on the MI355X (capped to 160 KiB by st_create), so the
    128 KiB launches of keep > 1024 are within it; the 64 KiB default only applies where the attribute cannot be read."""
    from oracle.spamtree_oracle import StRng
    pb = problem625()
    n = pb["n"]
    beta = np.array([0.7, -1.3])
    hm = hip_model(pb, tausq=0.25, beta=beta)
    draws = ref.qtile_rows(keep, n, seed=keep)
    assert hm.lib.st_summary_reserve(hm.h, keep) == 0
    feed(hm, draws)
    cnt = C.c_int64()
    assert hm.lib.st_summary_get(hm.h, None, None, C.byref(cnt)) == 0 and cnt.value == keep
    with_yhat = keep <= 1025
    if with_yhat:
        B = np.asfortranarray(beta.reshape(2, 1))
        mv0 = np.zeros(n, dtype=np.int64)
        ys, pert = np.zeros((keep, n)), np.zeros(n)
        for d in range(keep):
            ys[d], b = ref.ref_yhat(pb["X"], mv0, B, draws[d], np.array([4.0]), StRng(9).yhat_normals(d, n))
            pert = np.maximum(pert, b + 0.5e-13)
    wq, yq = np.zeros(n), np.zeros(n)
    for q in ref.qtile_qs(keep):
        assert hm.lib.st_summary_quantile(hm.h, q, _dp(wq), None) == 0
        assert_qtile(wq, draws, q, tag="w")
    if with_yhat:
        for q in (0.0, 0.025, 0.5, 0.975, 1.0, (keep // 2) / keep):
            assert hm.lib.st_summary_quantile(hm.h, q, None, _dp(yq)) == 0
            assert_qtile(yq, ys, q, extra=pert, tag="yhat")
    hm.close()


def test_summary_bookkeeping_past_the_reservation_reset_and_reserve_again():
    """Accumulating keep + 5 times with a reservation of keep: quantiles over the first keep draws, means over all keep + 5;
    st_summary_reset then fewer draws than reserved: quantiles over those only (Kpad shrinks from 8 to 4); reserving again
    drops the stored draws (ST_ERR_USAGE); a reservation beyond 16384 is ST_ERR_UNSUPPORTED and leaves the handle usable."""
    pb = problem625()
    n, keep = pb["n"], 5
    hm = hip_model(pb)
    lib, h = hm.lib, hm.h
    draws = np.random.default_rng(4).standard_normal((keep + 5, n)) * 3.0
    assert lib.st_summary_reserve(h, keep) == 0
    feed(hm, draws)
    wq, wm = np.zeros(n), np.zeros(n)
    cnt = C.c_int64()
    for q in (0.0, 0.3, 0.5, 1.0):
        assert lib.st_summary_quantile(h, q, _dp(wq), None) == 0
        assert_qtile(wq, draws[:keep], q)
    assert lib.st_summary_get(h, _dp(wm), None, C.byref(cnt)) == 0 and cnt.value == keep + 5
    want = np.array([math.fsum(draws[:, i]) / (keep + 5) for i in range(n)])
    assert np.all(np.abs(wm - want) <= ref.mean_bound(draws))
    assert lib.st_summary_reset(h) == 0
    assert lib.st_summary_quantile(h, 0.5, _dp(wq), None) == ST_ERR_USAGE
    feed(hm, draws[6:9])
    for q in (0.0, 0.5, 2.0 / 3.0, 1.0):
        assert lib.st_summary_quantile(h, q, _dp(wq), None) == 0
        assert_qtile(wq, draws[6:9], q)
    assert lib.st_summary_get(h, _dp(wm), None, C.byref(cnt)) == 0 and cnt.value == 3
    assert lib.st_summary_reserve(h, 8) == 0
    assert lib.st_summary_quantile(h, 0.5, _dp(wq), None) == ST_ERR_USAGE
    assert lib.st_summary_reserve(h, 16385) == ST_ERR_UNSUPPORTED
    assert lib.st_summary_reserve(h, 2) == 0 and lib.st_summary_reset(h) == 0
    feed(hm, draws[:2])
    assert lib.st_summary_quantile(h, 0.5, _dp(wq), None) == 0
    assert_qtile(wq, draws[:2], 0.5)
    hm.close()


_FITTED = []


def fitted_problem():
    """A bivariate problem with missing outcomes, slot 0 factorised, XB and w non-zero: the state the point set predicts from."""
    if not _FITTED:
        _FITTED.append(make_problem(side=20, q=2, seed=5, missing=0.1, p=2))
    pb = _FITTED[0]
    rng = np.random.default_rng(6)
    hm = hip_model(pb, tausq=0.2)
    hm.set_w(rng.standard_normal(pb["n"]))
    hm.beta_update(np.asfortranarray(rng.standard_normal((2, 2))))
    assert hm.get_loglik_comps_w(0)
    return pb, hm


def points_accumulate(hm, n_new, seed, it):
    out = [np.zeros(n_new) for _ in range(4)]
    assert hm.lib.st_points_accumulate(hm.h, seed, it, *[_dp(o) for o in out]) == 0
    return out     # w_new, cond_mean, cond_var, yhat_new


POINT_QTILE_CASES = [(n_new, keep) for n_new in (1, 7, 9, 33) for keep in (1, 2, 65, 2049)] + [(9, 16384)]


@pytest.mark.parametrize("n_new,keep", POINT_QTILE_CASES)
def test_point_set_quantiles(n_new, keep):
    """k_qtile through st_points_summary_quantile: n_new below, at and above the R = 8, 4, 1 rows of a workgroup (n < R: a single
    partly filled workgroup).  The draws are what st_points_accumulate returned to the host; the reference is list_qtile of
    those, within ref.qtile_bound."""
    pb, hm = fitted_problem()
    _points_for(hm, pb, n_new, 100 + n_new)
    assert hm.lib.st_points_summary_reserve(hm.h, keep) == 0
    ws, ys = np.zeros((keep, n_new)), np.zeros((keep, n_new))
    for d in range(keep):
        ws[d], _, _, ys[d] = points_accumulate(hm, n_new, 13, d)
    assert np.all(np.isfinite(ws)) and np.all(np.isfinite(ys)) and (keep == 1 or np.all(ws.std(axis=0) > 0))
    wq, yq = np.zeros(n_new), np.zeros(n_new)
    for q in sorted(set([0.0, 0.025, 0.5, 0.975, 1.0] + [k / keep for k in range(max(0, keep // 2 - 1), min(keep, keep // 2 + 2) + 1)])):
        assert hm.lib.st_points_summary_quantile(hm.h, q, _dp(wq), _dp(yq)) == 0
        assert_qtile(wq, ws, q, tag="w_new")
        assert_qtile(yq, ys, q, tag="yhat_new")
    hm.close()


def test_point_set_bookkeeping_past_the_reservation_reset_and_reserve_again():
    """The st_summary_* bookkeeping contract for the point set: quantiles over the first keep draws, means over all, reset, fewer
    draws than reserved, re-reserve -> ST_ERR_USAGE, 16385 -> ST_ERR_UNSUPPORTED with the handle still usable."""
    pb, hm = fitted_problem()
    lib, h = hm.lib, hm.h
    n_new, keep = 9, 5
    _points_for(hm, pb, n_new, 3)
    assert lib.st_points_summary_reserve(h, keep) == 0
    ws = np.stack([points_accumulate(hm, n_new, 13, d)[0] for d in range(keep + 5)])
    wq, wm = np.zeros(n_new), np.zeros(n_new)
    cnt = C.c_int64()
    for q in (0.0, 0.3, 0.5, 1.0):
        assert lib.st_points_summary_quantile(h, q, _dp(wq), None) == 0
        assert_qtile(wq, ws[:keep], q)
    assert lib.st_points_summary_get(h, None, None, _dp(wm), None, C.byref(cnt)) == 0 and cnt.value == keep + 5
    want = np.array([math.fsum(ws[:, i]) / (keep + 5) for i in range(n_new)])
    assert np.all(np.abs(wm - want) <= ref.mean_bound(ws))
    assert lib.st_points_summary_reset(h) == 0
    assert lib.st_points_summary_quantile(h, 0.5, _dp(wq), None) == ST_ERR_USAGE
    ws = np.stack([points_accumulate(hm, n_new, 13, 50 + d)[0] for d in range(3)])
    for q in (0.0, 0.5, 2.0 / 3.0, 1.0):
        assert lib.st_points_summary_quantile(h, q, _dp(wq), None) == 0
        assert_qtile(wq, ws, q)
    assert lib.st_points_summary_get(h, None, None, _dp(wm), None, C.byref(cnt)) == 0 and cnt.value == 3
    assert lib.st_points_summary_reserve(h, 8) == 0
    assert lib.st_points_summary_quantile(h, 0.5, _dp(wq), None) == ST_ERR_USAGE
    assert lib.st_points_summary_reserve(h, 16385) == ST_ERR_UNSUPPORTED
    assert lib.st_points_summary_reserve(h, 2) == 0
    ws = np.stack([points_accumulate(hm, n_new, 13, 70 + d)[0] for d in range(2)])
    assert lib.st_points_summary_quantile(h, 0.5, _dp(wq), None) == 0
    assert_qtile(wq, ws, 0.5)
    hm.close()


# ----------------------------------------------------------------------------------------------------------------------
# 4. means and the Welford summaries
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 1000])
def test_running_means_match_exact_sums(N):
    """st_summary_get after N fed draws against math.fsum / N per row: k_axpy_sum adds N - 1 times, the host multiplies by the
    rounded 1 / N, so |got - ref| <= (N + 1) 2^-53 sum|x| / N.  yhat_mean the same way against the yhat draws themselves, which
    st_yhat returns for the same state, seed and iteration (same kernel, same stream 5)."""
    pb = problem625()
    n = pb["n"]
    hm = hip_model(pb, tausq=0.25, beta=np.array([0.7, -1.3]))
    rng = np.random.default_rng(N)
    draws = rng.standard_normal((N, n)) * 10.0 ** rng.integers(-3, 4, n)[None, :]
    ys = np.zeros((N, n))
    for d in range(N):
        assert hm.lib.st_set_w(hm.h, _dp(draws[d])) == 0
        ys[d] = hm.yhat(None, seed=9, it=d)
        assert hm.lib.st_summary_accumulate(hm.h, 9, d) == 0
    wm, ym = np.zeros(n), np.zeros(n)
    cnt = C.c_int64()
    assert hm.lib.st_summary_get(hm.h, _dp(wm), _dp(ym), C.byref(cnt)) == 0 and cnt.value == N
    for got, x in ((wm, draws), (ym, ys)):
        want = np.array([math.fsum(x[:, i]) / N for i in range(n)])
        assert np.all(np.abs(got - want) <= ref.mean_bound(x))
    hm.close()


@pytest.mark.parametrize("case", ["unit", "offset"])
@pytest.mark.parametrize("n_new", [1, 7, 9, 33])
def test_point_summaries_match_exact_moments(case, n_new):
    """st_points_summary_get after N = 300 accumulations, w reset between calls (ref.welford_w: N(0, 1), or 1e6 + 1e-3 N(0, 1) --
    the case a naive sum x^2 - (sum x)^2 / N loses), against exact rational moments of the per-call outputs.
      mean:  Welford's running mean, |err| <= N 2^-53 max|m_k| (one rounding per step, earlier errors damped).
      var = sum var_k / N + M2 / N:  ref.exact_moments' bound on M2 (dominant term N 2^-53 |mean| sum(|d_k| + |x_k - m_k|)) over N,
             + (N + 1) 2^-53 sum var_k / N for the running sum and its division, + 3 2^-53 var for M2 / N and the final sum.
      w_mean, yhat_mean:  (N + 1) 2^-53 sum|x| / N.
    On the conditional means the device returned, the NumPy transcription of k_points_acc's update holds the M2 bound and (in
    the offset case) the naive form exceeds it by more than 100 x at most points: a regression to it could not pass."""
    N = 300
    pb, hm = fitted_problem()
    _points_for(hm, pb, n_new, 200 + n_new)
    outs = []
    for k in range(N):
        hm.set_w(ref.welford_w(case, k, pb["n"]))
        outs.append(points_accumulate(hm, n_new, 17, k))
    ws, cm, cv, ys = (np.stack([o[i] for o in outs]) for i in range(4))
    mean, var, wm, ym = (np.zeros(n_new) for _ in range(4))
    cnt = C.c_int64()
    assert hm.lib.st_points_summary_get(hm.h, _dp(mean), _dp(var), _dp(wm), _dp(ym), C.byref(cnt)) == 0 and cnt.value == N
    e_mean, e_M2, b_M2 = ref.exact_moments(cm)
    sum_var = np.array([float(sum(Fraction(v) for v in cv[:, i])) for i in range(n_new)])
    e_var = np.array([float((sum(Fraction(v) for v in cv[:, i]) + Fraction(e_M2[i])) / N) for i in range(n_new)])
    b_mean = N * U * np.abs(cm).max(axis=0)
    b_var = b_M2 / N + (N + 1) * U * sum_var / N + 3 * U * e_var
    print(f"{case} n_new={n_new}: mean err/bound {np.max(np.abs(mean - e_mean) / b_mean):.3g}  var err/bound "
          f"{np.max(np.abs(var - e_var) / b_var):.3g}  M2/N {np.min(e_M2 / N):.3g}..{np.max(e_M2 / N):.3g}")
    assert np.all(cv >= 0) and np.all(e_M2 > 0)            # the conditional means really vary
    assert np.all(np.abs(mean - e_mean) <= b_mean)
    assert np.all(np.abs(var - e_var) <= b_var)
    for got, x in ((wm, ws), (ym, ys)):
        want = np.array([math.fsum(x[:, i]) / N for i in range(n_new)])
        assert np.all(np.abs(got - want) <= ref.mean_bound(x))
    _, M2w = ref.welford_np(cm)
    assert np.all(np.abs(M2w - e_M2) <= b_M2)
    if case == "offset":
        assert np.all(np.abs(e_mean) > 1e6 * np.sqrt(e_M2 / N))        # a large level with a tiny spread, as intended
        _, M2n = ref.naive_np(cm)
        over = np.abs(M2n - e_M2) >= 100 * b_M2
        assert over.any() and over.mean() >= 0.5, np.abs(M2n - e_M2) / b_M2
        assert np.all(b_var < 1e-2 * e_M2 / N)                          # the bound on var resolves the spread itself
    hm.close()


# ----------------------------------------------------------------------------------------------------------------------
# 5. CrossCovarianceAG10
# ----------------------------------------------------------------------------------------------------------------------
def _ag_params(q):
    from oracle import spamtree_oracle as so
    cp = so.CovarianceParams(2, q, -1)
    cp.transform(nice_theta(q))
    return cp


def _ag_both(p1, m1, p2, m2, q, n_sample=300, seed=0):
    """The device's matrix against the oracle's (1e-14 max|ref|, the suite's constant for this export) and a sample of entries
    against the extended-precision closed form (oracle.extended.covariance, itself pinned to 50 digits), same constant."""
    from oracle import spamtree_oracle as so
    from oracle.extended import covariance
    from spamtree_amd.covariance import CrossCovarianceAG10
    cp = _ag_params(q)
    got = CrossCovarianceAG10(p1, m1, p2, m2, cp.ai1, cp.ai2, cp.phi_i, cp.thetamv, cp.Dmat)
    want = so.CrossCovarianceAG10(p1, m1, p2, m2, cp.ai1, cp.ai2, cp.phi_i, cp.thetamv, cp.Dmat)
    n1, n2 = len(m1), len(m2)
    assert got.shape == (n1, n2) and want.shape == (n1, n2)
    scale = np.abs(want).max()
    assert np.abs(got - want).max() <= 1e-14 * scale
    rng = np.random.default_rng(seed)
    i1, i2 = rng.integers(0, n1, n_sample), rng.integers(0, n2, n_sample)
    allc = np.vstack([p1, p2])
    allv = np.concatenate([np.asarray(m1) - 1, np.asarray(m2) - 1])
    K = covariance(allc, allv, nice_theta(q), q, i1, n1 + i2)
    ext = np.array([K[t, t] for t in range(n_sample)], dtype=np.float64)
    assert np.abs(got[i1, i2] - ext).max() <= 1e-14 * scale
    return got


@pytest.mark.parametrize("q", [2, 3, 4, 5, 6])
@pytest.mark.parametrize("n1", [1, 255, 256, 257])
def test_cross_covariance_outcomes_and_row_counts(q, n1):
    """q = 2..6 and n1 around one workgroup of 256 threads, with coincident (distance 0) and near-coincident (1e-12) points
    across and within outcomes."""
    rng = np.random.default_rng(10 * q + n1)
    n2 = 97
    p1, p2 = rng.uniform(size=(n1, 2)), rng.uniform(size=(n2, 2))
    m1, m2 = rng.integers(1, q + 1, n1), rng.integers(1, q + 1, n2)
    m1[0], m2[:4] = 1, (1, 2, 1, 2)
    p2[0] = p1[0]                                   # coincident, same outcome
    p2[1] = p1[0]                                   # coincident, another outcome
    p2[2] = p1[0] + (1e-12, 0.0)                    # near-coincident, same outcome
    p2[3] = p1[0] + (0.0, 1e-12)                    # near-coincident, another outcome
    got = _ag_both(p1, m1, p2, m2, q, seed=q)
    cp = _ag_params(q)
    assert abs(got[0, 0] - (cp.ai1[0] ** 2 + cp.ai2[0] ** 2)) <= 1e-14 * np.abs(got).max()    # K(0) of outcome 1, D_11 = 0


@pytest.mark.parametrize("n1,n2", [(3, 65535), (3, 65536), (3, 70000), (70000, 3)])
def test_cross_covariance_extents_beyond_one_grid_dimension(n1, n2):
    """The second extent used to go into gridDim.y unchanged, and hipDeviceAttributeMaxGridDimY reads 65536 on the MI355X: the
    launch for n2 = 70000 was refused (ST_ERR_HIP).  k_cross_cov now strides over the columns from a bounded grid."""
    rng = np.random.default_rng(n1 + n2)
    p1, p2 = rng.uniform(size=(n1, 2)), rng.uniform(size=(n2, 2))
    m1, m2 = rng.integers(1, 4, n1), rng.integers(1, 4, n2)
    _ag_both(p1, m1, p2, m2, 3)


def test_cross_covariance_empty_extents():
    """n1 = 0 or n2 = 0: return 0 and write nothing (the reference's empty matrix), through the C entry and the wrapper."""
    from spamtree_amd import _lib
    from spamtree_amd.covariance import CrossCovarianceAG10
    lib = _lib.load()
    cp = _ag_params(3)
    pts = np.asfortranarray(np.random.default_rng(0).uniform(size=(5, 2)))
    mv = np.array([1, 2, 3, 1, 2], dtype=np.int64)
    ip = mv.ctypes.data_as(C.POINTER(C.c_int64))
    D = np.asfortranarray(cp.Dmat)
    out = np.full(8, 7.0)
    for n1, n2 in ((0, 5), (5, 0), (0, 0)):
        rc = lib.st_cross_covariance_ag10(_dp(pts), ip, n1, _dp(pts), ip, n2, _dp(_f(cp.ai1)), _dp(_f(cp.ai2)), _dp(_f(cp.phi_i)),
                                          _dp(_f(cp.thetamv)), _dp(D), 3, 0, _dp(out))
        assert rc == 0 and np.all(out == 7.0), (n1, n2)
    e = np.zeros((0, 2))
    ev = np.zeros(0, dtype=np.int64)
    assert CrossCovarianceAG10(e, ev, pts, mv, cp.ai1, cp.ai2, cp.phi_i, cp.thetamv, cp.Dmat).shape == (0, 5)
    assert CrossCovarianceAG10(pts, mv, e, ev, cp.ai1, cp.ai2, cp.phi_i, cp.thetamv, cp.Dmat).shape == (5, 0)
