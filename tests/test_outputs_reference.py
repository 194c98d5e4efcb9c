"""CPU-only: the references, bounds and input generators of tests/test_gpu_outputs.py, and the checks that they are right.

Nothing here shares code with the library or with oracle.spamtree_oracle: the statistics are restated from the definitions in
include/spamtree_hip.h and accumulated in extended precision (np.longdouble, 64-bit significand: a product of two doubles is
rounded at 2^-64, a pairwise sum of n such terms at about log2(n) 2^-64 of sum |t_i| -- three orders of magnitude below
the bounds they are compared with, which are multiples of 2^-53 sum |t_i|).
"""
import math
from fractions import Fraction

import numpy as np

from oracle.list_summaries import list_qtile
from tests.util import make_problem

LD = np.longdouble
U = 2.0 ** -53
NT, STATS_WG = 256, 1024          # st_device.hpp NT, misc_kernels.hpp STATS_WG


# ----------------------------------------------------------------------------------------------------------------------
# section 1: statistics, XB, yhat, XtX
# ----------------------------------------------------------------------------------------------------------------------
def stats_depth(n):
    """D of k_stats + k_stats_final: the longest chain of additions one term passes through.  k_stats: a workgroup owns a
    chunk of ceil(n / 1024) rows and a thread adds every 256th of them serially (ceil(chunk / 256) additions), wave_sum
    adds over 6 shuffle steps, block_sum adds the 256 / 64 = 4 wave results serially; k_stats_final: a thread adds
    1024 / 256 = 4 partials serially, then an LDS tree of log2(256) = 8 steps."""
    chunk = -(-n // STATS_WG)
    return -(-chunk // NT) + 6 + NT // 64 + STATS_WG // NT + 8


def quirk_partner(om, n_all):
    """Row whose w the Q3 pairing subtracts from y in xty (reference_quirks = 1): the oracle's beta_tausq_stats takes, for the
    t-th available row (positions ix_by_q_a[j] in the available subset), w[t] of the FULL vector."""
    partner = np.arange(n_all)
    partner[om.na_ix_all] = np.arange(om.na_ix_all.size)
    for j in range(om.q):          # the same statement through the per-outcome index sets the oracle really uses
        assert np.array_equal(partner[om.na_ix_all[om.ix_by_q_a[j]]], om.ix_by_q_a[j])
    return partner


def ref_stats(y, X, mv0, w, xb, q, partner=None):
    """(xty p x q, bound_xty, ssq q, bound_ssq, n_obs q) from the header's definitions.  xty[:, j] = X_avail_j' (y_avail_j - w[..])
    (w of the row itself, or of `partner`), ssq_j = sum (y - XB - w)^2 over the observed rows of outcome j.

    Bounds, per entry: |got - ref| <= (D + 3) 2^-53 sum |t_i|, D = stats_depth(n), the + 3 for the roundings inside a term
    (xty: y - w, the product, one spare; ssq: the square and twice the relative error of e).  e = (y - XB) - w is two
    subtractions: the first one's rounding is relative to |y - XB|, not to |e|, and enters e^2 as 2 |e| 2^-53 |y - XB|, so
    the ssq bound carries that term too: (D + 3) 2^-53 sum e^2 + 2 2^-53 sum |e| |y - XB|."""
    n, p = X.shape
    obs = np.isfinite(y)
    partner = np.arange(n) if partner is None else partner
    D = stats_depth(n)
    xty, bx = np.zeros((p, q)), np.zeros((p, q))
    ssq, bs = np.zeros(q), np.zeros(q)
    n_obs = np.zeros(q, dtype=np.int64)
    for j in range(q):
        r = np.nonzero(obs & (mv0 == j))[0]
        n_obs[j] = r.size
        rw = y[r].astype(LD) - w[partner[r]].astype(LD)
        for k in range(p):
            t = X[r, k].astype(LD) * rw
            xty[k, j] = float(t.sum())
            bx[k, j] = (D + 3) * U * float(np.abs(t).sum())
        yx = y[r].astype(LD) - xb[r].astype(LD)
        e = yx - w[r].astype(LD)
        ssq[j] = float((e * e).sum())
        bs[j] = (D + 3) * U * float((e * e).sum()) + 2 * U * float((np.abs(e) * np.abs(yx)).sum())
    return xty, bx, ssq, bs, n_obs


def ref_xb(X, mv0, B):
    """XB = X . Bcoeff[:, mv] per row and its bound (p + 5) 2^-53 sum_k |x_ik b_k| (a serial sum of p products: D = p + 2)."""
    t = X.astype(LD) * B.T[mv0].astype(LD)
    return t.sum(axis=1).astype(np.float64), (X.shape[1] + 5) * U * np.abs(t).sum(axis=1).astype(np.float64)


def ref_yhat(X, mv0, B, w, tausq_inv, noise):
    """yhat = XB + w + tau_j noise, tau_j = tausq_inv_j^(-1/2): p + 2 terms per row, bound (p + 5) 2^-53 sum |t|."""
    t = X.astype(LD) * B.T[mv0].astype(LD)
    last = noise.astype(LD) / np.sqrt(tausq_inv.astype(LD))[mv0]
    val = t.sum(axis=1) + w.astype(LD) + last
    mag = np.abs(t).sum(axis=1) + np.abs(w.astype(LD)) + np.abs(last)
    return val.astype(np.float64), (X.shape[1] + 5) * U * mag.astype(np.float64)


def ref_xtx(y, X, mv0, q):
    """XtX(j) = X_avail_j' X_avail_j (p x p each) and the bound (n_j + 3) 2^-53 sum |x_a x_b| (a serial host sum of n_j terms)."""
    obs = np.isfinite(y)
    p = X.shape[1]
    out, bd = np.zeros((q, p, p)), np.zeros((q, p, p))
    for j in range(q):
        r = np.nonzero(obs & (mv0 == j))[0]
        t = X[r].astype(LD)[:, :, None] * X[r].astype(LD)[:, None, :]
        out[j] = t.sum(axis=0).astype(np.float64)
        bd[j] = (r.size + 3) * U * np.abs(t).sum(axis=0).astype(np.float64)
    return out, bd


def scaled_state(pb, seed):
    """w, Bcoeff (p x q), tausq_inv (q) in which outcome j's values are scaled by 10^j, so that reading another outcome's
    coefficient or tau is an O(1) relative error.  (y and X are scaled by scale_problem.)"""
    rng = np.random.default_rng(seed)
    mv0 = np.asarray(pb["mv_id"]) - 1
    w = rng.standard_normal(pb["n"]) * 10.0 ** mv0
    B = rng.standard_normal((pb["p"], pb["q"])) * 10.0 ** np.arange(pb["q"])[None, :]
    tsq_inv = 4.0 * 100.0 ** -np.arange(pb["q"], dtype=np.float64)       # tau_j = 0.5 10^j
    return w, np.asfortranarray(B), tsq_inv


def scale_problem(pb):
    """In place: outcome j's y times 10^j, column k of X times 2^k (after the tree was built: the tree reads only which y are
    NA).  Returns pb."""
    mv0 = np.asarray(pb["mv_id"]) - 1
    pb["y"] = pb["y"] * 10.0 ** mv0
    pb["X"] = pb["X"] * 2.0 ** np.arange(pb["p"])[None, :]
    return pb


def test_extended_precision_is_extended():
    assert np.finfo(LD).nmant >= 63


def test_make_problem_builds_one_to_eight_covariates_and_keeps_its_old_draws():
    base = make_problem(side=6, q=2, seed=3, p=3)
    for p in range(1, 9):
        pb = make_problem(side=6, q=2, seed=3, p=p)
        assert pb["X"].shape == (72, p) and pb["beta_true"].size == p and np.isfinite(pb["y"]).all()
    assert np.array_equal(make_problem(side=6, q=2, seed=3, p=5)["beta_true"], [-1.0, 0.5, 1.0, 0.25, -0.3])
    again = make_problem(side=6, q=2, seed=3)
    assert np.array_equal(base["y"], again["y"]) and np.array_equal(base["X"], again["X"])
    one = make_problem(side=6, q=3, seed=3, p=2, missing=0.12, single_obs=2)
    assert np.isfinite(one["y"][one["mv_id"] == 2]).sum() == 1 and np.isfinite(one["y"][one["mv_id"] == 1]).sum() > 20


def test_reference_statistics_against_exact_rationals():
    """The long-double restatement against exact rational arithmetic on a small problem, both pairings."""
    from tests.util import oracle_model
    pb = scale_problem(make_problem(side=5, q=3, seed=9, p=4, missing=(0.1, 0.3, 0.5)))
    w, B, _ = scaled_state(pb, 1)
    mv0 = pb["mv_id"] - 1
    xb, _ = ref_xb(pb["X"], mv0, B)
    om = oracle_model(pb)
    for partner in (None, quirk_partner(om, pb["n"])):
        xty, bx, ssq, bs, n_obs = ref_stats(pb["y"], pb["X"], mv0, w, xb, 3, partner)
        pr = np.arange(pb["n"]) if partner is None else partner
        for j in range(3):
            rows = [i for i in range(pb["n"]) if mv0[i] == j and math.isfinite(pb["y"][i])]
            assert n_obs[j] == len(rows)
            for k in range(4):
                ex = sum(Fraction(pb["X"][i, k]) * (Fraction(pb["y"][i]) - Fraction(w[pr[i]])) for i in rows)
                assert abs(Fraction(xty[k, j]) - ex) <= Fraction(bx[k, j]) / 1000 + Fraction(U) * abs(ex)      # (+ its rounding to double)
            ex = sum((Fraction(pb["y"][i]) - Fraction(xb[i]) - Fraction(w[i])) ** 2 for i in rows)
            assert abs(Fraction(ssq[j]) - ex) <= Fraction(bs[j]) / 1000 + Fraction(U) * ex
    # the oracle's own statement of the quirk pairing gives the same numbers (to its double-precision rounding)
    om.w, om.XB = w.copy(), xb.copy()
    oxty, ossq = om.beta_tausq_stats()
    xty, bx, ssq, bs, _ = ref_stats(pb["y"], pb["X"], mv0, w, xb, 3, quirk_partner(om, pb["n"]))
    assert np.all(np.abs(oxty - xty) <= 100 * bx) and np.all(np.abs(ossq - ssq) <= 100 * bs)


# ----------------------------------------------------------------------------------------------------------------------
# section 3: quantiles
# ----------------------------------------------------------------------------------------------------------------------
def qtile_r(q, keep):
    """r of prctile_stl as IEEE doubles compute it step by step: (q * 100) / 100 * keep."""
    return (q * 100.0) / 100.0 * keep


def qtile_picks(draws, q):
    """(lower, upper) -- the two order statistics per row that oracle.list_summaries.prctile_stl interpolates between, for
    draws[keep, n].  Used for the tolerance only; the expected VALUE comes from list_qtile."""
    a = np.sort(draws, axis=0)
    n = a.shape[0]
    r = qtile_r(q, n)
    if r >= n / 2.0:
        lo = int(max(r - 1.0, 0.0))
        return a[lo], (a[lo + 1] if lo < n - 1 else a[lo])
    up = int(math.ceil(max(r - 1.0, 0.0)))
    return (a[up - 1] if up > 0 else a[up]), a[up]


def qtile_bound(draws, q):
    """|got - ref| <= 4 2^-53 (|lower| + |upper|) + 2^-1074: the sort is exact and the pick is the reference's, so what is left
    is two products and a sum, with or without contraction; the last term for subnormal rows."""
    lo, up = qtile_picks(draws, q)
    return 4 * U * (np.abs(lo) + np.abs(up)) + 2.0 ** -1074


def qtile_rows(keep, n, seed):
    """draws[keep, n]; row i (a column here) is of kind i % 6: 0 a random permutation of scale_i (0 .. keep - 1) (well-separated
    order statistics: a wrong pick is off by a whole step), 1 heavy ties (3 levels), 2 constant, 3 mixed signs with +-0.0,
    4 magnitudes 1e-300 .. 1e300, 5 subnormals.  No NaN, no inf."""
    rng = np.random.default_rng(seed)
    d = np.zeros((keep, n))
    for i in range(n):
        kind = i % 6
        if kind == 0:
            d[:, i] = (1.0 + i) * 0.37 * rng.permutation(keep)
        elif kind == 1:
            d[:, i] = rng.integers(0, 3, keep) * 1.5 - 1.5
        elif kind == 2:
            d[:, i] = -2.75 + i
        elif kind == 3:
            v = rng.standard_normal(keep)
            v[rng.uniform(size=keep) < 0.3] = 0.0
            d[:, i] = np.where(rng.uniform(size=keep) < 0.5, -v, v)          # -0.0 and +0.0 both occur
        elif kind == 4:
            d[:, i] = np.where(rng.uniform(size=keep) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-300, 300, keep)
        else:
            d[:, i] = rng.integers(-(1 << 20), 1 << 20, keep) * 2.0 ** -1074
    return d


def qtile_qs(keep):
    """The q grid: keep <= 65: every k / keep, its two neighbours (clipped to [0, 1]) and 0.025, 0.5, 0.975; larger keeps: those
    three, 0, 1 and k / keep for a few k around keep / 2 (the branch r >= len / 2)."""
    if keep <= 65:
        qs = []
        for k in range(keep + 1):
            x = k / keep
            qs += [x, min(1.0, float(np.nextafter(x, 2.0))), max(0.0, float(np.nextafter(x, -1.0)))]
        return sorted(set(qs + [0.025, 0.5, 0.975]))
    return sorted(set([0.0, 0.025, 0.5, 0.975, 1.0] + [k / keep for k in range(keep // 2 - 2, keep // 2 + 3)]))


def test_stepwise_rounding_decides_the_pick_on_many_inputs():
    """For keep = 1..64 and q = k / keep the stepwise r is not the integer k on hundreds of pairs: the inputs where a
    contracted or reordered product picks the other pair.  The GPU test's grid contains every one of them."""
    off = [(keep, k) for keep in range(1, 65) for k in range(keep + 1) if qtile_r(k / keep, keep) != k]
    assert len(off) == 351 and sum(keep + 1 for keep in range(1, 65)) == 2144
    for keep, k in off:
        assert k / keep in qtile_qs(keep)
    # ... and on some of them the pick really differs from the one an exact r = k would make
    differ = 0
    for keep, k in off:
        d = np.arange(keep, dtype=np.float64)[:, None]
        lo, up = qtile_picks(d, k / keep)
        r = float(k)
        if r >= keep / 2.0:
            e_lo = int(max(r - 1.0, 0.0))
        else:
            e_lo = max(int(math.ceil(max(r - 1.0, 0.0))) - 1, 0)
        differ += int(lo[0] != e_lo)
    assert differ > 0


def test_vectorised_picks_are_list_qtile():
    """qtile_picks (used for the tolerance) makes the reference's pick: interpolating its pair reproduces list_qtile bit for bit
    on every kind of row and the whole q grid of small keeps."""
    for keep in (1, 2, 3, 4, 5, 63, 64, 65):
        d = qtile_rows(keep, 13, keep)
        for q in qtile_qs(keep):
            lo, up = qtile_picks(d, q)
            r = qtile_r(q, keep)
            r -= int(r + 0.5)
            want = list_qtile(list(d), q)
            assert np.array_equal((0.5 - r) * lo + (0.5 + r) * up, want), (keep, q)
            assert np.all(np.isfinite(want))
    d = qtile_rows(65, 13, 1)
    step = 0.37 * 1.0                      # row 0: a wrong pick is off by at least half a step, the bound far below it
    assert qtile_bound(d, 0.5)[0] < 1e-12 * step


# ----------------------------------------------------------------------------------------------------------------------
# section 4: means and the Welford summaries
# ----------------------------------------------------------------------------------------------------------------------
def mean_bound(x):
    """Running sum of N draws (N - 1 additions), then one product with the rounded 1 / N: (N + 1) 2^-53 sum |x| / N on the mean.
    x: [N, n]."""
    N = x.shape[0]
    return (N + 1) * U * np.abs(x).sum(axis=0) / N


def exact_mean(x):
    return np.array([float(sum(Fraction(v) for v in x[:, i]) / x.shape[0]) for i in range(x.shape[1])])


def welford_np(x):
    """NumPy transcription of the four-line update of k_points_acc, in doubles: returns (mean, M2) after the rows of x[N, n]."""
    m = np.zeros(x.shape[1])
    M2 = np.zeros(x.shape[1])
    for k in range(x.shape[0]):
        d = x[k] - m
        m1 = m + d / float(k + 1)
        M2 = M2 + d * (x[k] - m1)
        m = m1
    return m, M2


def naive_np(x):
    """The form Welford replaces: M2 = sum x^2 - (sum x)^2 / N in doubles."""
    s, s2 = np.zeros(x.shape[1]), np.zeros(x.shape[1])
    for k in range(x.shape[0]):
        s = s + x[k]
        s2 = s2 + x[k] * x[k]
    return s / x.shape[0], s2 - s * s / x.shape[0]


def exact_moments(x):
    """(mean, M2 = sum (x - mean)^2) per column in exact rationals, and the bound on the device's M2.

    Bound, from the update d = x_k - m_{k-1}; m_k = m_{k-1} + d / k; M2 += d (x_k - m_k): the running mean is rounded once per
    step at 2^-53 |m| and an earlier error is damped, never amplified (the update subtracts it again: factor 1 - 1/k), so
    |err m_k| <= k 2^-53 max|m|.  It enters the increment through both factors: |d_k| err(m_k) + |x_k - m_k| err(m_{k-1}).  The
    increment's own roundings (d, x - m_k, the product) and the N additions to M2 are (N + 3) 2^-53 sum |d_k (x_k - m_k)|.  So
        |err M2| <= N 2^-53 max_k |m_k| sum_k (|d_k| + |x_k - m_k|) + (N + 3) 2^-53 sum_k |d_k (x_k - m_k)|,
    all of it evaluated on the exact sequence, the sums over k >= 2 (the first step rounds nothing).  The first term dominates
    when |mean| is large and the spread tiny."""
    N, n = x.shape
    mean, M2, bound = np.zeros(n), np.zeros(n), np.zeros(n)
    for i in range(n):
        xs = [Fraction(v) for v in x[:, i]]
        m, acc, s1, s2, mmax = Fraction(0), Fraction(0), Fraction(0), Fraction(0), Fraction(0)
        for k, v in enumerate(xs):
            d = v - m
            m = m + d / (k + 1)
            acc += d * (v - m)
            if k == 0:
                continue           # the first step is exact: m_0 = 0, d = x_1, m_1 = x_1, x_1 - m_1 = 0
            s1 += abs(d) + abs(v - m)
            s2 += abs(d * (v - m))
            mmax = max(mmax, abs(m))
        mean[i], M2[i] = float(m), float(acc)
        bound[i] = float(N * Fraction(U) * mmax * s1 + (N + 3) * Fraction(U) * s2)
    return mean, M2, bound


def welford_w(case, k, n, seed=11):
    """The latent field the GPU test sets before accumulation k: "unit": N(0, 1) per row; "offset": 1e6 + 1e-3 N(0, 1) -- a
    large common level with a tiny spread, which the naive variance loses."""
    z = np.random.default_rng([seed, k]).standard_normal(n)
    return z if case == "unit" else 1e6 + 1e-3 * z


def test_welford_holds_its_bound_where_the_naive_form_breaks_it():
    """On N = 300 inputs 1e6 + 1e-3 N(0, 1) (the GPU test's latent fields; it repeats this comparison on the conditional means
    the device returns): the transcription of k_points_acc's update stays within the derived bound, the naive formula
    exceeds it by more than 100 x."""
    x = np.stack([welford_w("offset", k, 7) for k in range(300)])
    mean, M2, bound = exact_moments(x)
    mw, M2w = welford_np(x)
    mn, M2n = naive_np(x)
    assert np.all(np.abs(M2w - M2) <= bound) and np.all(np.abs(mw - mean) <= 300 * U * np.abs(mean))
    assert np.all(np.abs(M2n - M2) >= 100 * bound)
    assert np.all(bound <= 1e-3 * M2)               # the bound itself is sharp enough to mean something
    x = np.stack([welford_w("unit", k, 7) for k in range(300)])
    mean, M2, bound = exact_moments(x)
    mw, M2w = welford_np(x)
    assert np.all(np.abs(M2w - M2) <= bound) and np.all(bound <= 1e-10 * M2)
