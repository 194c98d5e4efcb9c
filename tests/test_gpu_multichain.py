"""GPU: the diagnostics of several chains in one store (st_summary_chain_diagnostics, st_points_summary_chain_diagnostics,
st_points_functionals_chain_diagnostics, st_summary_chain_rank_diagnostics and its two siblings; k_series_diag<true>,
k_series_rank<true>).

The stores are filled through the real calls as tests/test_gpu_diagnostics.py fills them, a store of K = M N draws being M chains
of N draws laid end to end, and the reference (tests/multichain_reference.py: long-double moments, the indicator ESS in Python
integers and exact rationals, 50-digit Phi^-1) is always evaluated on the very draws the device stored.

Tolerances are the single-chain siblings', derived the same way (tests/test_gpu_diagnostics.py, series_bounds; tests/
rank_reference.py, score_bounds): the first-order rounding of the kernel's own addition chains (diag_kernels.hpp, diag_chain_wave),
doubled, with the neglected products asserted below 1e-6.  What the chains add -- multichain_reference.chain_bounds spells every
term out -- is (a) a pooled centring before the per-chain one, so that every later quantity sees values of the size of the spread
and the error of the pooled mean is a common shift that cancels; (b) the chain means nu_c, each behind its own chain of
ceil(N / 64) + 6 additions, entering rho_t through B': nu_c - nb is off by e_b = 2 e_nu + 12 u Y (the butterfly over the M lane
values, a division and a subtraction on top of two means), and since sum_c |nu_c - nb| <= sqrt(M (M - 1) B') the term K B' moves by
at most 2 sqrt(2) e_b / s + 9 u of K (B' + gbar_0), s = sqrt(B' + gbar_0) -- it is added to numerator and denominator of every
rho_t alike, and the lag sums over the chains have ceil(K / 64) + M terms per lane at the most; (c) for R-hat the 2M segment means
carry e_nu on top of the half sums' error, and B = h / (S - 1) sum (m_j - mb)^2 moves by 2 sqrt(h S / (S - 1) B) 2 e_mj to first
order.  Integer-defined outputs (prob, ess_q, ess_tail, ess_exc, mcse_prob) are held to what their siblings are held to: prob bit
for bit, the others within 1e-14 (Num_t are exact integers; only 1 / log10 K, tau's one quotient, the final division and the
square root can differ).  lags and the truncated state are compared wherever the reference's smallest |Gamma_k| exceeds 1e-8.
"""
import ctypes as C
import math

import numpy as np
import pytest

from tests import diag_reference as dref
from tests import multichain_reference as ref
from tests.test_gpu_diagnostics import feed_points, feed_rows, hip_model, points_setup, problem
from tests.test_gpu_rank_diagnostics import thresholds_for

pytestmark = pytest.mark.gpu

ST_ERR_USAGE = -1
INT_RTOL = 1e-14
EPS_PHI = 2 * ref.rr.PHI_ERR_MEASURED
PROBS = (0.1, 0.5)
KEYS = ("ess", "mcse", "sd", "rhat")
SHAPES = [(2, 4), (2, 5), (3, 21), (4, 16), (3, 64), (2, 65), (16, 4), (5, 13)]
OBSERVED = dict(max_err_over_bound=0.0, max_rel_err=0.0, max_int_rel_err=0.0, stores=0, series=0)
N_KINDS = 12


def chain_rows(M, N, n, seed):
    """[M N][n]: column i carries M chains of N draws of kind i mod 12 -- AR(1) chains that agree in level (phi -0.5, 0.5, 0.9);
    AR(1) chains of shifted levels and growing scales; white noise; a constant; every chain constant at a value of its own; one
    constant chain among varying ones; noise on an offset of 1e3; levels 0, 3, 0, 3, ...; identical copies of one chain; a
    three-valued series (ties)."""
    out = np.empty((M * N, n))
    for i in range(n):
        kind, s = i % N_KINDS, seed * 1000 + i * 20
        ar = lambda phi, c, **kw: dref.ar1(N, phi, seed=s + c, **kw)   # noqa: E731
        if kind < 3:
            ch = [ar((-0.5, 0.5, 0.9)[kind], c) for c in range(M)]
        elif kind == 3:
            ch = [ar(0.7, c, scale=1.0 + 0.2 * c) + 0.5 * c for c in range(M)]
        elif kind == 4:
            ch = [ar(0.0, c) for c in range(M)]
        elif kind == 5:
            ch = [np.full(N, 0.1 * (i + 1))] * M
        elif kind == 6:
            ch = [np.full(N, 0.3 * c * c - 1.0) for c in range(M)]
        elif kind == 7:
            ch = [np.full(N, 0.25)] + [ar(0.3, c) for c in range(1, M)]
        elif kind == 8:
            ch = [ar(0.0, c, offset=1e3) for c in range(M)]
        elif kind == 9:
            ch = [ar(0.5, c) + 3.0 * (c % 2) for c in range(M)]
        elif kind == 10:
            ch = [ar(0.6, 0)] * M
        else:
            u = [np.random.default_rng(s + c).uniform(size=N) for c in range(M)]   # (sqrt 2: no pair of lag sums cancels exactly)
            ch = [np.where(v < 0.3 + 0.1 * (c % 3), 1.5, np.where(v > 0.8, math.sqrt(2.0), -1.0)) for c, v in enumerate(u)]
        out[:, i] = np.concatenate(ch)
    return out


def close(a, b, rtol):
    return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= rtol * abs(b)


def note(worst, worst_rel, worst_int, seen):
    for k, v in (("max_err_over_bound", worst), ("max_rel_err", worst_rel), ("max_int_rel_err", worst_int)):
        OBSERVED[k] = max(OBSERVED[k], v)
    OBSERVED["stores"] += 1
    OBSERVED["series"] += seen


def check_plain(got, draws, M, max_lag, tag, cols=None):
    """Every series (or those of ``cols``) of draws[K][n] against the long-double reference: ess, mcse, sd, rhat within
    chain_bounds, lags and the truncated state wherever the reference's smallest |Gamma_k| exceeds 1e-8."""
    K, n = draws.shape
    _, k_max = ref.lag_cap(K // M, max_lag)
    left_out, worst, worst_rel, seen = 0, 0.0, 0.0, 0
    for i in (range(n) if cols is None else cols):
        r = ref.reference(draws[:, i], M, max_lag)
        g = {k: float(got[k][i]) for k in KEYS}
        lags = int(got["lags"][i])
        seen += 1
        if r["den"] == 0.0:
            assert math.isnan(g["ess"]) and math.isnan(g["rhat"]) and g["mcse"] == 0.0 and g["sd"] == 0.0 and lags == 0, (tag, i, g)
            continue
        b = ref.chain_bounds(r, K, lags // 2)
        for k in KEYS:
            if math.isnan(r[k]):
                assert math.isnan(g[k]), (tag, i, k, g[k])
                continue
            err = abs(g[k] - r[k]) / abs(r[k])
            worst, worst_rel = max(worst, err / b[k]), max(worst_rel, err)
            assert err <= b[k], (tag, i, k, g[k], r[k], err, b[k])
        if r["min_abs_gamma"] > 1e-8:
            assert lags == r["lags"] and (lags == 2 * (k_max + 1)) == r["truncated"], (tag, i, lags, r["lags"])
        else:
            left_out += 1
        assert lags % 2 == 0 and 0 <= lags <= 2 * (k_max + 1)
    assert left_out <= 0.02 * seen, (tag, left_out)
    note(worst, worst_rel, 0.0, seen)
    print(f"{tag}: M = {M}, N = {K // M}, n = {seen}, max_lag = {max_lag}: max err / bound {worst:.3g}, max relative err {worst_rel:.3g}, "
          f"left out of the lags comparison {left_out}")


def check_rank(got, draws, M, thr, sides, max_lag, tag, cols=None, probs=PROBS):
    """The rank family of every series (or those of ``cols``) against the reference.  ``thr``: (T, n) values per series."""
    K, n = draws.shape
    _, k_max = ref.lag_cap(K // M, max_lag)
    left_out, worst, worst_rel, worst_int, seen = 0, 0.0, 0.0, 0.0, 0
    for i in (range(n) if cols is None else cols):
        r = ref.rank_reference(draws[:, i], M, probs, [t[i] for t in thr], sides, max_lag)
        seen += 1
        for key, want in (("ess_q", r["ess_q"]), ("ess_exc", r["ess_exc"]), ("mcse_prob", r["mcse_prob"])):
            for k, w in enumerate(want):
                g = float(got[key][k][i])
                assert close(g, w, INT_RTOL), (tag, i, key, k, g, w)
                if not math.isnan(w) and w != 0.0:
                    worst_int = max(worst_int, abs(g - w) / abs(w))
        assert close(float(got["ess_tail"][i]), r["ess_tail"], INT_RTOL), (tag, i, got["ess_tail"][i], r["ess_tail"])
        for t, w in enumerate(r["prob"]):
            assert np.array([got["prob"][t][i]]).tobytes() == np.array([w], dtype=np.float64).tobytes(), (tag, i, t, got["prob"][t][i], w)
        g = {k: float(got[k][i]) for k in ("rhat_rank", "rhat_bulk", "rhat_fold", "ess_bulk")}
        lags = int(got["lags_bulk"][i])
        for part, keys in (("bulk", (("rhat_bulk", "rhat"), ("ess_bulk", "ess"))), ("fold", (("rhat_fold", "rhat"),))):
            rec = r[part]
            if rec["den"] == 0.0:
                assert all(math.isnan(g[a]) for a, _ in keys) and (part != "bulk" or lags == 0), (tag, i, part, g, lags)
                continue
            b = ref.chain_bounds(rec, K, lags // 2, EPS_PHI)
            for a, key in keys:
                if math.isnan(rec[key]):
                    assert math.isnan(g[a]), (tag, i, a, g[a])
                    continue
                err = abs(g[a] - rec[key]) / abs(rec[key])
                worst, worst_rel = max(worst, err / b[key]), max(worst_rel, err)
                assert err <= b[key], (tag, i, a, g[a], rec[key], err, b[key])
        assert np.array([g["rhat_rank"]]).tobytes() == np.array([ref.rr.fmax(g["rhat_bulk"], g["rhat_fold"])]).tobytes(), (tag, i, g)
        if r["bulk"]["den"] != 0.0:
            if r["bulk"]["min_abs_gamma"] > 1e-8:
                assert lags == r["lags_bulk"] and (lags == 2 * (k_max + 1)) == r["truncated"], (tag, i, lags, r["lags_bulk"])
            else:
                left_out += 1
            assert lags % 2 == 0 and 0 <= lags <= 2 * (k_max + 1)
    assert left_out <= 0.02 * seen, (tag, left_out)
    note(worst, worst_rel, worst_int, seen)
    print(f"{tag}: M = {M}, N = {K // M}, n = {seen}, max_lag = {max_lag}: score outputs max err / bound {worst:.3g}, max relative err "
          f"{worst_rel:.3g}; integer-defined outputs max relative err {worst_int:.3g}; left out of the lags comparison {left_out}")


# ---- 1. values ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N", SHAPES)
def test_row_stores_against_the_reference(M, N):
    """n = 81 rows in tiles of 8 (the last holds one), every kind of series; chain boundaries inside a lane stride (N < 64), inside
    a 64-bit word (N = 5, 13, 21, 65), on a word boundary (N = 64), N odd (the middle draw of a chain is dropped); max_lag the
    default, 3 and beyond N; w and yhat, both families from the same store."""
    pb = problem("n81")
    hm = hip_model(pb)
    K = M * N
    draws = chain_rows(M, N, pb["n"], seed=K)
    assert hm.lib.st_summary_reserve(hm.h, K) == 0
    ys = feed_rows(hm, draws)
    for max_lag in (0, 3, N + 5):
        plain = hm.summary_diagnostics(max_lag, n_kept=K, n_chains=M)
        for name, d in (("w", draws), ("yhat", ys)):
            check_plain(plain[name], d, M, max_lag, name)
            assert np.array_equal(plain[name]["truncated"], plain[name]["lags"] == 2 * (ref.lag_cap(N, max_lag)[1] + 1))
            t, per, sides = thresholds_for(d)
            got = hm.summary_rank_diagnostics(PROBS, t, sides, max_lag, n_kept=K, n_chains=M)[name]
            check_rank(got, d, M, per, sides, max_lag, name + " rank")
            assert got["prob"].tobytes() == hm.summary_excursions(K, thresholds=t, side=list(sides))[name]["prob"].tobytes()
        # the pooled sd is the single-chain call's on the same store, bit for bit
        assert plain["w"]["sd"].tobytes() == hm.summary_diagnostics(max_lag)["w"]["sd"].tobytes()
    hm.close()


@pytest.mark.parametrize("M,N", [(4, 4096), (2, 4097)])
def test_row_stores_with_long_series(M, N):
    """K = 16384 as four chains: one series per workgroup at the LDS limit, the scores in the workgroup's global slice; K = 8194 as
    two chains of odd length: the first K beyond the scores' LDS route with a chain boundary inside a word.  n = 64 rows; the
    reference costs seconds per series at these lengths, so it is evaluated on one column of each kind that behaves differently
    (AR(1) with phi -0.5 and 0.9, shifted levels, every chain constant, one constant chain, the offset, levels 0 / 3, the two-valued
    series, the last row) for the plain family and on one of them for the rank family (levels 0 / 3 at K = 16384, shifted levels
    at K = 8194: up to 512 pairs of six indicators in exact integers and of the scores in long double), with the default lag cap."""
    pb = problem("n64")
    hm = hip_model(pb)
    K = M * N
    draws = chain_rows(M, N, pb["n"], seed=7)
    assert hm.lib.st_summary_reserve(hm.h, K) == 0
    ys = feed_rows(hm, draws)
    plain = hm.summary_diagnostics(0, n_kept=K, n_chains=M)
    check_plain(plain["w"], draws, M, 0, "w", cols=[0, 2, 3, 5, 6, 7, 8, 9, 11, 63])
    check_plain(plain["yhat"], ys, M, 0, "yhat", cols=[4, 63])
    t, per, sides = thresholds_for(draws)
    got = hm.summary_rank_diagnostics(PROBS, t, sides, 0, n_kept=K, n_chains=M)["w"]
    check_rank(got, draws, M, per, sides, 0, "w rank", cols=[9 if M == 4 else 3])
    assert got["prob"].tobytes() == hm.summary_excursions(K, thresholds=t, side=list(sides))["w"]["prob"].tobytes()
    hm.close()


def points_handle(pb, n_new=9, seed=5, X=True):
    hm = hip_model(pb)
    assert hm.get_loglik_comps_w(0)
    points_setup(hm, pb, n_new, seed=seed, X=X)
    return hm


@pytest.mark.parametrize("M,N", SHAPES)
def test_point_and_functional_stores_against_the_reference(M, N):
    pb = problem("n64")
    n_new, K = 9, M * N
    hm = points_handle(pb, n_new)
    hm.set_functionals([([0, 1, 2], [1.0, 2.0, -3.0]), ([4], [1.0]), (list(range(n_new)), [1.0 / n_new] * n_new)])
    assert hm.lib.st_points_summary_reserve(hm.h, K) == 0
    ws, ys, fw, fy = feed_points(hm, pb, K, seed=K)
    for max_lag in (0, 3, N + 5):
        plain, fplain = hm.points_diagnostics(max_lag, n_kept=K, n_chains=M), hm.functionals_diagnostics(max_lag, n_kept=K, n_chains=M)
        for name, d, fd in (("w", ws, fw), ("yhat", ys, fy)):
            check_plain(plain[name], d, M, max_lag, name + "*")
            check_plain(fplain[name], fd, M, max_lag, "F_" + name)
            t, per, sides = thresholds_for(d)
            got = hm.points_rank_diagnostics(PROBS, t, sides, max_lag, n_kept=K, n_chains=M)[name]
            check_rank(got, d, M, per, sides, max_lag, name + "* rank")
            fper = [np.median(fd, axis=0), np.quantile(fd, 0.25, axis=0)]   # a threshold value per functional
            got = hm.functionals_rank_diagnostics(PROBS, fper, (1, -1), max_lag, n_kept=K, n_chains=M)[name]
            check_rank(got, fd, M, fper, (1, -1), max_lag, "F_" + name + " rank")
            assert got["truncated"].dtype == bool and got["ess_q"].shape == (2, 3)
    hm.close()


# ---- 2. one chain is the existing call -------------------------------------------------------------------------------------------
def same_bits(a, b, tag):
    for part in ("w", "yhat"):
        assert a[part].keys() == b[part].keys()
        for k in a[part]:
            assert np.asarray(a[part][k]).tobytes() == np.asarray(b[part][k]).tobytes(), (tag, part, k)


def test_one_chain_is_the_existing_call_bit_for_bit():
    """Each of the six calls with n_chains = 1 against its sibling on the same store, two lag caps.  (The Python wrappers take the
    sibling's entry point at n_chains = 1, so the chain entry points are called through the library here.)"""
    from spamtree_amd.model import rank_buffers, rank_spec, series_diag_buffers
    pb = problem("n64")
    n_new, K = 9, 65
    hm = points_handle(pb, n_new)
    hm.set_functionals([([0, 1, 2], [1.0, 2.0, -3.0]), ([4], [1.0])])
    assert hm.lib.st_points_summary_reserve(hm.h, K) == 0 and hm.lib.st_summary_reserve(hm.h, K) == 0
    feed_points(hm, pb, K, seed=2)
    feed_rows(hm, chain_rows(1, K, pb["n"], seed=2))
    lib, h = hm.lib, hm.h

    def plain(call, n, max_lag):
        (dw, sw), (dy, sy) = series_diag_buffers(n), series_diag_buffers(n)
        assert call(h, 1, max_lag, C.byref(sw), C.byref(sy)) == 0
        return dict(w=dw, yhat=dy)

    def rank(call, n, m, thr, max_lag):
        spec, keep, n_prob, n_thr = rank_spec(PROBS, thr, (1, -1), max_lag, m)
        (dw, ow), (dy, oy) = rank_buffers(n, n_prob, n_thr), rank_buffers(n, n_prob, n_thr)
        assert call(h, 1, C.byref(spec), C.byref(ow), C.byref(oy)) == 0
        return dict(w=dw, yhat=dy)

    for max_lag in (0, 7):
        same_bits(plain(lib.st_summary_chain_diagnostics, pb["n"], max_lag), hm.summary_diagnostics(max_lag), "rows")
        same_bits(plain(lib.st_points_summary_chain_diagnostics, n_new, max_lag), hm.points_diagnostics(max_lag), "points")
        same_bits(plain(lib.st_points_functionals_chain_diagnostics, 2, max_lag), hm.functionals_diagnostics(max_lag), "functionals")
        thr = [0.1, -0.4]
        same_bits(rank(lib.st_summary_chain_rank_diagnostics, pb["n"], 1, thr, max_lag),
                  hm.summary_rank_diagnostics(PROBS, thr, (1, -1), max_lag), "rows rank")
        same_bits(rank(lib.st_points_summary_chain_rank_diagnostics, n_new, 1, thr, max_lag),
                  hm.points_rank_diagnostics(PROBS, thr, (1, -1), max_lag), "points rank")
        same_bits(rank(lib.st_points_functionals_chain_rank_diagnostics, 2, 2, thr, max_lag),
                  hm.functionals_rank_diagnostics(PROBS, thr, (1, -1), max_lag), "functionals rank")
    hm.close()


# ---- 3. the outputs of a series do not depend on where it is stored -------------------------------------------------------------
RANK_KEYS = ("rhat_rank", "rhat_bulk", "rhat_fold", "ess_bulk", "ess_tail", "lags_bulk", "ess_q", "ess_exc", "mcse_prob", "prob")


def test_a_series_gives_the_same_bits_wherever_it_is_stored():
    """One series of 3 x 43 draws -- the w* draws of point 3 of a point set -- as that point, as a functional of weight 1 on it, as
    row 0 of the n = 64 handle, as row 37 of the same handle among permuted neighbours and as row 50 of the n = 81 handle (another
    n, another place in its tile): every output of both families agrees bit for bit, for two lag caps."""
    M, N = 3, 43
    K = M * N
    pb = problem("n64")
    hm = points_handle(pb)
    hm.set_functionals([([3], [1.0]), ([0, 1], [0.5, 0.5])])
    assert hm.lib.st_points_summary_reserve(hm.h, K) == 0
    ws, _, fw, _ = feed_points(hm, pb, K, seed=3)
    x = ws[:, 3].copy()
    assert np.array_equal(fw[:, 0], x)
    t, sides = [float(np.median(x)), float(np.quantile(x, 0.2))], (1, -1)
    pick = lambda d, i, keys: {k: np.asarray(d[k])[..., i].copy() for k in keys}   # noqa: E731
    outs = {}
    for max_lag in (0, 7):
        fthr = [np.array([v, v]) for v in t]
        outs[max_lag] = [
            (pick(hm.points_diagnostics(max_lag, n_chains=M)["w"], 3, KEYS + ("lags",)),
             pick(hm.points_rank_diagnostics(PROBS, t, sides, max_lag, n_chains=M)["w"], 3, RANK_KEYS)),
            (pick(hm.functionals_diagnostics(max_lag, n_chains=M)["w"], 0, KEYS + ("lags",)),
             pick(hm.functionals_rank_diagnostics(PROBS, fthr, sides, max_lag, n_chains=M)["w"], 0, RANK_KEYS))]
    for name, row, perm_seed in (("n64", 0, None), ("n64", 37, 4), ("n81", 50, None)):
        pr = problem(name)
        hr = hip_model(pr)
        draws = chain_rows(M, N, pr["n"], seed=11 + row)
        if perm_seed is not None:
            draws = draws[:, np.random.default_rng(perm_seed).permutation(pr["n"])]
        draws[:, row] = x
        assert hr.lib.st_summary_reserve(hr.h, K) == 0
        feed_rows(hr, draws)
        for max_lag in (0, 7):
            outs[max_lag].append((pick(hr.summary_diagnostics(max_lag, n_chains=M)["w"], row, KEYS + ("lags",)),
                                  pick(hr.summary_rank_diagnostics(PROBS, t, sides, max_lag, n_chains=M)["w"], row, RANK_KEYS)))
        hr.close()
    hm.close()
    for max_lag, o in outs.items():
        for other in o[1:]:
            for fam in (0, 1):
                for k in o[0][fam]:
                    assert o[0][fam][k].tobytes() == other[fam][k].tobytes(), (max_lag, k, o[0][fam][k], other[fam][k])
        assert o[0][0]["ess"] > 0 and o[0][0]["lags"] > 0 and o[0][1]["ess_bulk"] > 0 and 0 < o[0][1]["prob"][0] < 1


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    from spamtree_amd import _lib
    from spamtree_amd.model import rank_buffers, series_diag_buffers
    pb = problem("n64")
    hm = hip_model(pb)
    lib, h, n = hm.lib, hm.h, pb["n"]
    dp = C.POINTER(C.c_double)
    d, s = series_diag_buffers(n)
    dr, o = rank_buffers(n, 1, 0)
    prob = np.array([0.5])

    def spec(max_lag=0, n_prob=1):
        return _lib.StRankSpec(max_lag, n_prob, prob.ctypes.data_as(dp), 0, None, None)

    def refused(rc, text):
        assert rc == ST_ERR_USAGE and text in lib.st_last_error(h), (rc, text, lib.st_last_error(h))

    rows, rrows = lib.st_summary_chain_diagnostics, lib.st_summary_chain_rank_diagnostics
    refused(rows(h, 2, 0, C.byref(s), None), b"0 draws stored, the diagnostics need at least 4")       # no reservation
    assert lib.st_summary_reserve(h, 24) == 0
    draws = chain_rows(2, 9, n, seed=1)
    feed_rows(hm, draws[:3])
    refused(rows(h, 0, 0, C.byref(s), None), b"3 draws stored, the diagnostics need at least 4")       # both of step 5: the count first
    feed_rows(hm, draws[3:])
    for call, args in ((rows, lambda M: (M, 0, C.byref(s), None)), (rrows, lambda M: (M, C.byref(spec()), C.byref(o), None))):
        refused(call(h, *args(0)), b"n_chains = 0 must lie in 1 .. 16")
        refused(call(h, *args(-1)), b"n_chains = -1 must lie in 1 .. 16")
        refused(call(h, *args(17)), b"n_chains = 17 must lie in 1 .. 16")
        refused(call(h, *args(4)), b"18 draws stored are not a multiple of n_chains = 4")
        refused(call(h, *args(6)), b"18 draws stored in 6 chains are 3 per chain, the diagnostics need at least 4")
        assert call(h, *args(2)) == 0 and call(h, *args(3)) == 0 and call(h, *args(1)) == 0
    # two faults in one call: step 3 (max_lag) before step 5 (n_chains); inside step 5 the spec before n_chains
    refused(rows(h, 0, -1, C.byref(s), None), b"max_lag must not be negative")
    refused(rrows(h, 0, C.byref(spec(max_lag=-1)), C.byref(o), None), b"max_lag must not be negative")
    refused(rrows(h, 17, C.byref(spec(n_prob=9)), C.byref(o), None), b"n_prob = 9 must lie in 0 .. 8")
    refused(rrows(h, 2, None, C.byref(o), None), b"no spec")
    check_plain(hm.summary_diagnostics(0, n_chains=2)["w"], draws, 2, 0, "after the refusals")          # still answers, and rightly
    # points and functionals: the resolver's refusal first; n_chains (step 5) before yhat without X (step 6)
    pts, fun = lib.st_points_summary_chain_diagnostics, lib.st_points_functionals_chain_diagnostics
    rpts, rfun = lib.st_points_summary_chain_rank_diagnostics, lib.st_points_functionals_chain_rank_diagnostics
    refused(pts(h, 0, 0, C.byref(s), None), b"before st_points_set")
    refused(rfun(h, 0, C.byref(spec()), C.byref(o), None), b"")
    assert hm.get_loglik_comps_w(0)
    points_setup(hm, pb, 9, seed=2, X=False)
    hm.set_functionals([([0, 1], [1.0, 1.0])])
    assert lib.st_points_summary_reserve(h, 12) == 0
    for it in range(10):
        hm.accumulate_points(seed=1, it=it)
    for call in (pts, fun):
        refused(call(h, 3, 0, C.byref(s), C.byref(s)), b"10 draws stored are not a multiple of n_chains = 3")
        refused(call(h, 2, 0, C.byref(s), C.byref(s)), b"needs the regressors X")
        refused(call(h, 5, 0, C.byref(s), None), b"2 per chain")
        assert call(h, 2, 0, C.byref(s), None) == 0
    for call in (rpts, rfun):
        refused(call(h, 20, C.byref(spec()), C.byref(o), C.byref(o)), b"n_chains = 20 must lie in 1 .. 16")
        refused(call(h, 2, C.byref(spec()), C.byref(o), C.byref(o)), b"needs the regressors X")
        assert call(h, 2, C.byref(spec()), C.byref(o), None) == 0
    assert np.all(hm.points_diagnostics(n_chains=2)["w"]["ess"] > 0) and np.all(hm.functionals_rank_diagnostics(n_chains=2)["w"]["ess_tail"] > 0)
    # a point set of size 0 (step 4) with n_chains out of range (step 5): ST_OK, nothing written
    hm.set_points(np.zeros((0, 2)), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))
    d["ess"][:] = -7.0
    dr["ess_bulk"][:] = -7.0
    assert pts(h, 99, 0, C.byref(s), None) == 0 and np.all(d["ess"] == -7.0)
    assert rpts(h, 99, C.byref(spec()), C.byref(o), None) == 0 and np.all(dr["ess_bulk"] == -7.0)
    refused(pts(h, 99, -1, C.byref(s), None), b"max_lag")                                               # step 3 comes before step 4
    check_plain(hm.summary_diagnostics(3, n_chains=3)["w"], draws, 3, 3, "at the end")
    hm.close()


# ---- 5. the driver ----------------------------------------------------------------------------------------------------------------
RK = dict(probs=PROBS, thresholds=(0.0, 0.4), sides=(1, -1))
CHAIN_SEEDS, CHAIN_FACTORS = (23, 101, 7), (1.0, 0.8, 1.25)   # three chains: their seeds and their starts as multiples of theta


def chain_fit(pb, chains=None, seed=None, theta=None, **kw):
    """fit.spamtree_mv_mcmc on the small problem: 12 saved draws per chain after 4 of burn-in, adapting."""
    from spamtree_amd import fit
    from tests.test_gpu_diagnostics import fit_args
    args = list(fit_args(pb))
    if theta is not None:
        args[16] = theta
    run = dict(mcmc_keep=12, mcmc_burn=4, mcmc_thin=1, adapting=True, main_verbose=False)
    if chains is None:
        return fit.spamtree_mv_mcmc(*args, seed=seed, **run, **kw)
    thetas = np.stack([pb["theta"] * f for f in CHAIN_FACTORS[:chains]])
    return fit.spamtree_mv_mcmc(*args, seed=999, chains=chains, chain_seeds=CHAIN_SEEDS[:chains], chain_theta=thetas, **run, **kw)


def driver_points(pb, seed=8):
    from spamtree_amd.predict import locate
    rng = np.random.default_rng(seed)
    n_new = 9
    lo, hi = pb["coords"].min(axis=0), pb["coords"].max(axis=0)
    pts = lo + (hi - lo) * rng.uniform(size=(n_new, 2))
    mv = np.ones(n_new, dtype=np.int64)
    return dict(coords=pts, mv=mv, anchor=locate(pb["topo"], pts, mv, device=0), X=rng.standard_normal((n_new, pb["p"])),
                functionals=[([0, 1, 2], [1.0, 2.0, -3.0]), (list(range(n_new)), [1.0 / n_new] * n_new)])


def stack(lst):
    return np.stack([np.asarray(a).reshape(-1) for a in lst])


def check_slices(res, singles, keep):
    """Chain c's columns of every per-draw output of ``res`` are the single-chain call's, bit for bit."""
    for c, one in enumerate(singles):
        sl = slice(c * keep, (c + 1) * keep)
        for key in ("w_mcmc", "yhat_mcmc"):
            assert stack(res[key])[sl].tobytes() == stack(one[key]).tobytes(), (c, key)
        assert np.ascontiguousarray(res["beta_mcmc"][:, sl, :]).tobytes() == np.ascontiguousarray(one["beta_mcmc"]).tobytes(), c
        for key in ("tausq_mcmc", "theta_mcmc"):
            assert np.ascontiguousarray(res[key][:, sl]).tobytes() == np.ascontiguousarray(one[key]).tobytes(), (c, key)
        assert np.ascontiguousarray(res["paramsd"][:, :, c]).tobytes() == np.ascontiguousarray(one["paramsd"]).tobytes(), c
        if "new" in one:
            for part_r, part_o in ((res["new"], one["new"]), (res["new"]["functionals"], one["new"]["functionals"])):
                for key in ("w", "cond_mean", "cond_var", "yhat"):
                    assert np.ascontiguousarray(part_r[key][:, sl]).tobytes() == np.ascontiguousarray(part_o[key]).tobytes(), (c, key)
    assert np.array_equal(res["chain_id"], np.repeat(np.arange(len(singles)), keep)) and res["n_chains"] == len(singles)


def test_driver_plain_chains_slice_for_slice():
    """Three chains on one handle against the three single-chain calls; the diagnostics of the rows against the reference on the
    returned draws, those of theta, beta and tausq against the host functions; the lean call; chains = 2 without any summary."""
    from spamtree_amd import diagnostics as dg
    pb = problem("n64")
    M, keep = 3, 12
    res = chain_fit(pb, chains=M, diagnostics=True, rank_diagnostics=RK)
    singles = [chain_fit(pb, seed=CHAIN_SEEDS[c], theta=pb["theta"] * CHAIN_FACTORS[c]) for c in range(M)]
    check_slices(res, singles, keep)
    for key, draws in (("w", stack(res["w_mcmc"])), ("yhat", stack(res["yhat_mcmc"]))):
        check_plain(res["diagnostics"][key], draws, M, 0, "driver " + key)
        per = [np.full(draws.shape[1], t) for t in RK["thresholds"]]
        check_rank(res["rank_diagnostics"][key], draws, M, per, RK["sides"], 0, "driver rank " + key)
        assert res["diagnostics"][key]["truncated"].dtype == bool
    assert res["diagnostics"]["n_chains"] == M and res["rank_diagnostics"]["n_chains"] == M
    for j in range(res["theta_mcmc"].shape[0]):
        want = dg.multichain_diagnostics(res["theta_mcmc"][j], M)
        assert all(np.array([want[k]]).tobytes() == np.array([res["diagnostics"]["theta"][k][j]], dtype=np.float64).tobytes() for k in KEYS)
        wr = dg.multichain_rank_diagnostics(res["theta_mcmc"][j], M, probs=RK["probs"])
        assert np.array([wr["rhat_rank"]]).tobytes() == np.array([res["rank_diagnostics"]["theta"]["rhat_rank"][j]]).tobytes()
    assert res["diagnostics"]["beta"]["ess"].shape == (pb["p"], 1) and res["diagnostics"]["tausq"]["ess"].shape == (1,)
    lean = chain_fit(pb, chains=M, diagnostics=True, rank_diagnostics=RK, save_w=False, save_yhat=False)
    assert "w_mcmc" not in lean
    for fam, keys in (("diagnostics", KEYS + ("lags", "truncated")), ("rank_diagnostics", RANK_KEYS + ("truncated",))):
        for part in ("w", "yhat"):
            for k in keys:
                assert np.array_equal(lean[fam][part][k], res[fam][part][k], equal_nan=True), (fam, part, k)
    bare = chain_fit(pb, chains=2)
    check_slices(bare, singles[:2], keep)
    assert "diagnostics" not in bare and bare["chain_time"].shape == (2,) and np.all(bare["chain_time"] > 0)


def test_driver_chains_with_new_points_and_pooled_summaries():
    """Three chains with a point set and functionals: the slices; the pooled device summaries (quantiles, exceedance probability,
    the Rao-Blackwellised mean and variance) against the host on the returned 36 draws, within their own tests' tolerances; the
    multi-chain diagnostics of points and functionals against the reference on the returned draws."""
    pb = problem("n64")
    M, keep = 3, 12
    new_points = driver_points(pb)
    kw = dict(new_points=new_points, new_quantiles=(0.1, 0.5, 0.9))
    res = chain_fit(pb, chains=M, diagnostics=True, rank_diagnostics=RK, excursions=dict(thresholds=[0.0]), **kw)
    singles = [chain_fit(pb, seed=CHAIN_SEEDS[c], theta=pb["theta"] * CHAIN_FACTORS[c], **kw) for c in range(M)]
    check_slices(res, singles, keep)
    new = res["new"]
    K = M * keep
    assert new["w"].shape == (9, K) and new["functionals"]["w"].shape == (2, K)
    # pooled: the device's summaries are those of all 36 draws
    for part in (new, new["functionals"]):
        np.testing.assert_allclose(part["mean"], part["cond_mean"].mean(axis=1), rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(part["var"], part["cond_var"].mean(axis=1) + part["cond_mean"].var(axis=1), rtol=1e-10, atol=1e-14)
        np.testing.assert_allclose(part["w_mean"], part["w"].mean(axis=1), rtol=1e-12, atol=1e-14)
        for qv, (wq, yq) in part["quantiles"].items():
            srt = np.sort(part["w"], axis=1)
            assert np.all((wq >= srt[:, 0]) & (wq <= srt[:, -1]))
            if qv == 0.5:   # 36 draws: the median lies between the two middle order statistics
                assert np.all((wq >= srt[:, K // 2 - 1]) & (wq <= srt[:, K // 2]))
    assert np.array_equal(new["excursions"]["w"]["prob"][0], (new["w"] > 0.0).sum(axis=1) / K) and new["excursions"]["w"]["n_draws"] == K
    assert np.array_equal(res["excursions"]["w"]["prob"][0], (stack(res["w_mcmc"]) > 0.0).sum(axis=0) / K)
    # the multi-chain diagnostics of the points and the functionals
    for part, tag in ((new, "points"), (new["functionals"], "functionals")):
        for key in ("w", "yhat"):
            draws = part[key].T
            check_plain(part["diagnostics"][key], draws, M, 0, f"driver {tag} {key}")
            per = [np.full(draws.shape[1], t) for t in RK["thresholds"]]
            check_rank(part["rank_diagnostics"][key], draws, M, per, RK["sides"], 0, f"driver {tag} rank {key}")
        assert part["diagnostics"]["n_chains"] == M and part["rank_diagnostics"]["n_chains"] == M
    check_plain(res["diagnostics"]["w"], stack(res["w_mcmc"]), M, 0, "driver rows beside points")


def joint_points(pb, seed=12):
    """Nine points in three joint groups of 3, 2 and 4 neighbours (unequal sizes: the packed blocks have different lengths)."""
    from spamtree_amd.predict import locate
    rng = np.random.default_rng(seed)
    lo, hi = pb["coords"].min(axis=0), pb["coords"].max(axis=0)
    labels = np.array([0, 0, 0, 1, 1, 2, 2, 2, 2])
    centres = lo + (hi - lo) * rng.uniform(0.2, 0.8, size=(3, 2))
    pts = centres[labels] + 0.01 * (hi - lo) * rng.standard_normal((9, 2))
    mv = np.ones(9, dtype=np.int64)
    return dict(coords=pts, mv=mv, anchor=locate(pb["topo"], pts, mv, device=0, joint=labels), X=rng.standard_normal((9, pb["p"])), joint=labels)


def chains_without_cond_cov(pb, new_points, M, keep, burn):
    """stm_mcmc_chains through the library with new_cond_var but no new_cond_cov: the driver keeps the packed blocks of all M keep
    draws in a scratch of its own and forms cond_var from their diagonals.  Returns (cond_mean, cond_var, packed cov)."""
    from spamtree_amd import _lib, fit
    from spamtree_amd.model import _dp, _f64, _ip
    from tests.test_gpu_diagnostics import fit_args
    lib = _lib.load()
    a = fit_args(pb)
    spb, hold, n, p, q = fit._problem(a[0], a[1], a[3], a[4], a[7], a[8], a[9], a[11], a[12], a[13])
    pc, pmv, pan, pX, _, labels, _, _, _ = fit._points_inputs(new_points, p, q, ())
    k, K, n_new = pb["theta"].size, M * keep, pc.shape[0]
    bounds, sd = np.asfortranarray(np.asarray(a[14], dtype=np.float64)), np.asfortranarray(np.asarray(a[19], dtype=np.float64))
    opt, fl = _lib.StOptions(0, 1, 0, 1, 0, 0), _lib.StmFlags(1, 1, 1, 1, 1, 1)
    beta_mcmc, tausq_mcmc = np.zeros((p, K, q), order="F"), np.zeros((q, K), order="F")
    theta_mcmc, paramsd, t = np.zeros((k, K), order="F"), np.zeros((k, k), order="F"), C.c_double()
    cond_mean, cond_var = np.zeros((n_new, K), order="F"), np.zeros((n_new, K), order="F")
    cov = np.zeros(int(sum(g * g for g in np.unique(labels, return_counts=True)[1])))
    seeds = np.array(CHAIN_SEEDS[:M], dtype=np.uint64)
    thetas = np.ascontiguousarray(np.stack([pb["theta"] * f for f in CHAIN_FACTORS[:M]]))
    chs = _lib.StmChains(M, seeds.ctypes.data_as(C.POINTER(C.c_uint64)), _dp(thetas), None, None)
    rc = lib.stm_mcmc_chains(C.byref(spb), C.byref(opt), _dp(bounds), _dp(_f64(pb["theta"])), k, _dp(_f64(a[17])), float(a[18]), _dp(sd), keep, burn,
                             1, 999, C.byref(fl), None, None, _dp(beta_mcmc), _dp(tausq_mcmc), _dp(theta_mcmc), _dp(paramsd), C.byref(t),
                             n_new, _dp(pc), _ip(pmv), _ip(pan), _dp(pX), _ip(labels), 0, None, 0,
                             None, _dp(cond_mean), _dp(cond_var), None, None, None, None, None, None, None, None,
                             None, _dp(cov), None, None, None, None, None, C.byref(chs))
    assert rc == 0, (rc, lib.stm_mcmc_chains_last_error())
    del hold
    return cond_mean, cond_var, cov, theta_mcmc


def test_driver_chains_with_a_joint_point_set():
    """Three chains with joint groups of 3, 2 and 4 points.  With the per-draw blocks returned (new_cond_cov): chain c's slice of
    the packed cond_cov, of the cond_var taken from its diagonals and of w, cond_mean and yhat is the single-chain call's, bit for
    bit; the pooled predictive covariance per group is, on the host, the mean of the 36 conditional covariances plus the covariance
    of the 36 conditional means (within 1e-9 of max(1, |cov|), tests/test_gpu_predict_joint.py's tolerance).  Without new_cond_cov
    (through the library: the driver's own scratch of M keep packed blocks) cond_mean, cond_var and cov are the same bits."""
    pb = problem("n64")
    M, keep = 3, 12
    K = M * keep
    jp = joint_points(pb)
    res = chain_fit(pb, chains=M, new_points=jp)
    singles = [chain_fit(pb, seed=CHAIN_SEEDS[c], theta=pb["theta"] * CHAIN_FACTORS[c], new_points=jp) for c in range(M)]
    new = res["new"]
    assert len(new["cond_cov"]) == K and [g.size for g in new["groups"]] == [3, 2, 4] and new["cond_var"].shape == (9, K)
    for c, one in enumerate(singles):
        for s in range(keep):
            for g, (blk, want) in enumerate(zip(new["cond_cov"][c * keep + s], one["new"]["cond_cov"][s])):
                assert blk.shape == want.shape and blk.tobytes() == want.tobytes(), (c, s, g)
        sl = slice(c * keep, (c + 1) * keep)
        for key in ("w", "cond_mean", "cond_var", "yhat"):
            assert np.ascontiguousarray(new[key][:, sl]).tobytes() == np.ascontiguousarray(one["new"][key]).tobytes(), (c, key)
        assert np.ascontiguousarray(res["theta_mcmc"][:, sl]).tobytes() == np.ascontiguousarray(one["theta_mcmc"]).tobytes(), c
    for s in range(K):   # cond_var is the diagonal of the draw's blocks, in the caller's order of the points
        diag = np.empty(9)
        for g, blk in zip(new["groups"], new["cond_cov"][s]):
            diag[g] = np.diagonal(blk)
        assert np.array_equal(new["cond_var"][:, s], np.maximum(diag, 0.0)), s
    for j, g in enumerate(new["groups"]):   # pooled over the three chains
        host = np.mean([new["cond_cov"][s][j] for s in range(K)], axis=0) + np.cov(new["cond_mean"][g], bias=True).reshape(g.size, g.size)
        assert np.abs(new["cov"][j] - host).max() <= 1e-9 * max(1.0, np.abs(host).max()), j
        assert np.array_equal(new["cov"][j], new["cov"][j].T)
    cm, cv, cov, th = chains_without_cond_cov(pb, jp, M, keep, 4)
    assert th.tobytes() == np.asfortranarray(res["theta_mcmc"]).tobytes()
    assert cm.tobytes() == np.asfortranarray(new["cond_mean"]).tobytes() and cv.tobytes() == np.asfortranarray(new["cond_var"]).tobytes()
    assert cov.tobytes() == np.concatenate([np.asarray(b).reshape(-1, order="F") for b in new["cov"]]).tobytes()


# ---- 6. the Python front door ------------------------------------------------------------------------------------------------------
def test_front_door_two_chains_fit_predict_and_the_replay():
    """fit.spamtree_mv_mcmc(chains=2, diagnostics=True, rank_diagnostics=True) with the default seeds (seed, seed + 1) and starts;
    predict.fit_predict(chains=2); predict.predict_new on the concatenated result, unchanged: it replays all 24 draws, and its
    conditional means -- which no draw's normals enter -- are the fit's, column for column; the refusals of the front door."""
    from spamtree_amd import fit
    from spamtree_amd.predict import fit_predict, predict_new
    from tests.test_gpu_diagnostics import fit_args
    pb = problem("n64")
    run = dict(mcmc_keep=12, mcmc_burn=4, mcmc_thin=1, adapting=True, main_verbose=False)
    res = fit.spamtree_mv_mcmc(*fit_args(pb), seed=23, chains=2, diagnostics=True, rank_diagnostics=True, **run)
    singles = [fit.spamtree_mv_mcmc(*fit_args(pb), seed=23 + c, **run) for c in range(2)]
    check_slices(res, singles, 12)
    check_plain(res["diagnostics"]["w"], stack(res["w_mcmc"]), 2, 0, "front door w")
    check_rank(res["rank_diagnostics"]["yhat"], stack(res["yhat_mcmc"]), 2, [], (), 0, "front door rank yhat", probs=())
    assert res["diagnostics"]["n_chains"] == 2 and set(res["diagnostics"]["summary"]) == {"theta", "beta", "tausq", "w", "yhat"}
    pts = driver_points(pb)
    kw = dict(mcmc_keep=12, mcmc_burn=4, mcmc_thin=1, adapting=True, seed=77, device=0)
    out = fit_predict(pb, pts["coords"], pts["mv"], pts["X"], quantiles=(0.5,), diagnostics=True, chains=2, **kw)
    assert out["new"]["w"].shape == (9, 24) and out["n_chains"] == 2 and out["new"]["diagnostics"]["n_chains"] == 2
    one = fit_predict(pb, pts["coords"], pts["mv"], pts["X"], quantiles=(0.5,), **dict(kw, seed=78))
    assert np.ascontiguousarray(out["new"]["w"][:, 12:]).tobytes() == np.ascontiguousarray(one["new"]["w"]).tobytes()
    check_plain(out["new"]["diagnostics"]["w"], out["new"]["w"].T, 2, 0, "fit_predict w*")
    rep = predict_new(pb, out, pts["coords"], pts["mv"], pts["X"], seed=77, device=0, return_moments=True)
    assert rep["w"].shape == (9, 24) and np.array_equal(rep["cond_mean"], out["new"]["cond_mean"])
    assert np.array_equal(rep["w"][:, :12], out["new"]["w"][:, :12])   # chain 0: the replay's seed and counters are the chain's own
    np.testing.assert_allclose(rep["mean"], out["new"]["mean"], rtol=1e-12, atol=1e-14)
    for bad, text in ((dict(chains=2, mcmc_keep=8193), "16384"), (dict(chains=17), "1 .. 16"), (dict(chains=2, criteria=True), "separate drivers"),
                      (dict(chains=2, chain_seeds=(1, 2, 3)), "one seed per chain"), (dict(chain_seeds=(1,)), "need chains > 1"),
                      (dict(chains=2, chain_theta=np.ones((3, pb["theta"].size))), "one start per chain")):
        with pytest.raises(ValueError, match=text):
            fit.spamtree_mv_mcmc(*fit_args(pb), **dict(run, **bad))


def test_zz_report_the_largest_observed_error():
    """Prints the largest error the cases above met, relative and as a fraction of its bound (DESIGN.md section 25 records it)."""
    print(f"largest observed over {OBSERVED['stores']} stores, {OBSERVED['series']} series: err / bound {OBSERVED['max_err_over_bound']:.3g}, "
          f"relative err {OBSERVED['max_rel_err']:.3g}; integer-defined outputs relative err {OBSERVED['max_int_rel_err']:.3g}")
    assert OBSERVED["max_err_over_bound"] <= 1.0 and OBSERVED["max_int_rel_err"] <= INT_RTOL
