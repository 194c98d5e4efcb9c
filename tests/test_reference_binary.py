"""CPU: this repository's restatements against the reference's OWN compiled source.

oracle/_ref/libspamtree_ref.so (oracle/Makefile) is the reference's covariance_functions.cpp, mh_adapt.{h,cpp}, list_mean.cpp
and find_nan.cpp, compiled unchanged against the stand-in oracle/refshim/RcppArmadillo.h; oracle/reflib.py loads it.  Compared
with it here:
  * oracle/spamtree_oracle.py: CovarianceParams.transform, vec_to_symmat, Covariancef, mvCovAG20107, CrossCovarianceAG10 at
    q = 1 to 6 (coincident points, theta at both prior bounds, a zero Dmat entry between different outcomes), the three
    flavours of the q = 1 distance form, and the wide block shapes whose GPU routes are too large for a fixture (75-row
    blocks at q = 3, 100- to 150-row blocks at q = 4 to 6: those kernels are pinned to the oracle by
    tests/test_gpu_many_outcomes.py, test_gpu_deep.py and test_gpu_routes.py, and the oracle to the reference here);
  * oracle/spamtree_oracle.py AND spamtree_amd/mcmc.py: par_huvtransf_*, unif_bounds, calc_jacobian, do_I_accept, RAMAdapt;
  * oracle/list_summaries.py: list_qtile (bitwise) and list_mean;
  * the committed fixtures tests/golden/ref_*.npz: regenerated in memory, byte for byte.

The C++ driver's copy of RAMAdapt (spamtree_amd/csrc/spamtree_fit.cpp) is not called here.  It stays pinned through
tests/test_gpu_chain.py, which compares the driver's paramsd with the oracle chain's, and the oracle's RAMAdapt is pinned here.

The tests against the live library are skipped only where both the library and the reference tree are absent (a machine that
never saw the reference).  Where the tree is present and the library is not, they fail: the build should have produced it.
The last section needs neither: it holds the same restatements to the RECORDED outputs (tests/golden/ref_*.npz), with the
same bounds, so the pin also holds on a machine without the reference.

Tolerances.  Measured on the CPU these tests were written on, as the largest elementwise relative difference
|ours - ref| / max(|ref|, 1e-300) of each group; the test asserts 8 x the measurement (10 x for the RAMAdapt trajectories,
whose repeated Cholesky factorisations compound rounding).  The margin covers only libm against NumPy in exp / log / log1p,
within an ulp or so each.
  covariance, q = 2 to 6 and q = 1 with reference_distance=True     7.5e-16  (q = 1 .. 6: 3.2, 4.2, 7.4, 6.5, 7.2, 6.0 e-16;
                                                                             the q = 1 flavour test: 3.7e-16, against 4.4e-12 for
                                                                             the direct form and 1.1e-5 for the emulated FMA;
                                                                             the recorded covariances: 7.5e-16)
  covariance at the wide block shapes                               7.8e-16  (q = 3: 7.1e-16; q = 4, 5, 6: 7.8e-16)
  par_huvtransf_*, calc_jacobian, both restatements                 0        (the same libm calls on the same bits: exact)
  RAMAdapt paramsd and S over 120 steps, both restatements          5.1e-14  (p = 4: 3.7e-15, p = 10: 1.5e-14, p = 21: 5.1e-14)
All are below the 1e-14 (covariance, helpers) and 1e-10 (trajectories) above which a measurement would be a finding.
list_qtile agrees bitwise; list_mean within keep 2^-52 max|x|; transform, vec_to_symmat, unif_bounds and do_I_accept exactly.
"""
import math
import os

import numpy as np
import pytest

from oracle import list_summaries, reflib
from oracle import spamtree_oracle as so
from spamtree_amd import mcmc as product_mcmc
from tests.golden import make_reference_golden as gen
from tests.util import default_bounds, distinct_theta, make_problem, nice_theta

MEASURED_COV = 7.5e-16
MEASURED_WIDE = 7.8e-16
MEASURED_MH = 0.0
MEASURED_RAM = 5.1e-14

LIB = reflib.load()
GOLDEN = os.path.dirname(os.path.abspath(gen.__file__))


@pytest.fixture(scope="module")
def lib():
    """The live library.  Every test that takes it is skipped where neither it nor the reference tree exists, and fails where
    the tree exists and the library does not."""
    if LIB is None and not reflib.reference_tree_present():
        pytest.skip("neither the reference tree nor the library compiled from it is on this machine")
    assert LIB is not None, "the reference tree is here but oracle/_ref/libspamtree_ref.so is not: run make -C oracle"
    return LIB


def recorded(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def rel(a, b):
    """Largest elementwise |a - b| / max(|b|, 1e-300); b is the reference's."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    if a.size == 0:
        return 0.0
    assert np.array_equal(np.isfinite(a), np.isfinite(b))
    ok = np.isfinite(b)
    return float(np.max(np.abs(a[ok] - b[ok]) / np.maximum(np.abs(b[ok]), 1e-300), initial=0.0))


def check(tag, worst, measured, factor=8.0):
    print(f"{tag}: max relative difference {worst:.3g}")
    assert worst <= factor * measured, (tag, worst, measured)


# ---------------------------------------------------------------------------------------------------------------------
# covariance_functions.{h,cpp}
# ---------------------------------------------------------------------------------------------------------------------
def bound_thetas(q):
    """theta with every entry at its lower, and at its upper, prior bound (tests.util.default_bounds: 1e-3 and 1e3)."""
    b = default_bounds(q)
    return [b[:, 0].copy(), b[:, 1].copy()]


def thetas_of(q):
    if q == 1:
        return [nice_theta(1), gen.MH_START] + bound_thetas(1)
    out = [nice_theta(q), gen.crosscov_theta(q)] + bound_thetas(q)
    if q >= 3:
        out += [distinct_theta(q), gen.crosscov_theta(q, zero_d=True)]
    return out


def points(q, n=46, seed=0):
    """Random points of random outcomes; the last six repeat earlier LOCATIONS (h = 0) with the same and with other outcomes."""
    rng = np.random.default_rng(seed + q)
    c = rng.uniform(size=(n, 2))
    mv = np.concatenate([np.arange(q), rng.integers(0, q, n - q)])
    c[-6:] = c[:6]
    mv[-3:] = mv[3:6]
    rng.shuffle(mv[:-6])
    return c, mv.astype(np.int64)


@pytest.mark.parametrize("q", [1, 2, 3, 4, 5, 6])
def test_transform_and_vec_to_symmat_are_the_references(q, lib):
    """Parameter slicing and the column-wise fill of Dmat, exactly.  At q = 4 the six Dmat entries are distinct and the
    column-wise and the row-wise fill of the triangle differ."""
    for theta in thetas_of(q):
        cp = so.CovarianceParams(2, q, -1)
        cp.transform(theta)
        t = lib.transform(q, theta)
        assert (t["covariance_model"], t["npars"], t["n_cbase"]) == (cp.covariance_model, cp.npars, cp.n_cbase)
        for name in ("ai1", "ai2", "phi_i", "thetamv", "Dmat"):
            assert np.array_equal(getattr(cp, name), t[name]), (name, theta)
    k = q * (q - 1) // 2
    if k:
        x = 1.0 + np.arange(k)
        D = lib.vec_to_symmat(x)
        assert np.array_equal(so.vec_to_symmat(x), D) and np.array_equal(D, D.T) and np.all(np.diag(D) == 0)
        if q == 4:
            assert np.array_equal(D[1:, 0], [1, 2, 3]) and np.array_equal(D[2:, 1], [4, 5]) and D[3, 2] == 6


@pytest.mark.parametrize("q", [1, 2, 3, 4, 5, 6])
def test_covariance_matches_compiled_reference(q, lib):
    """Covariancef and mvCovAG20107 with same true and false, CrossCovarianceAG10 (q >= 2; at q = 1 the reference stops and so
    does the oracle).  q = 1 is the oracle's reference_distance=True flavour (the next test says why)."""
    c, mv = points(q)
    n = c.shape[0]
    every = np.arange(n)
    rng = np.random.default_rng(50 + q)
    i1, i2 = rng.permutation(n)[:30], rng.permutation(n)[:25]
    worst = 0.0
    flavour = True if q == 1 else False
    for theta in thetas_of(q):
        cp = so.CovarianceParams(2, q, -1)
        cp.transform(theta)
        for a, b, same in ((every, every, True), (i1, i1, True), (i1, i2, False), (every, every, False), (i2[:1], i2[:1], True)):
            for ours, theirs in ((so.Covariancef, lib.Covariancef), (so.mvCovAG20107, lib.mvCovAG20107)):
                got = ours(c, mv, a, b, cp, same, flavour)
                ref = theirs(q, theta, c, mv, a, b, same)
                worst = max(worst, rel(got, ref))
        if q >= 2:
            got = so.CrossCovarianceAG10(c[i1], mv[i1] + 1, c[i2], mv[i2] + 1, cp.ai1, cp.ai2, cp.phi_i, cp.thetamv, cp.Dmat)
            ref = lib.CrossCovarianceAG10(c[i1], mv[i1] + 1, c[i2], mv[i2] + 1, cp.ai1, cp.ai2, cp.phi_i, cp.thetamv, cp.Dmat)
            worst = max(worst, rel(got, ref))
        else:
            with pytest.raises(ValueError):
                so.CrossCovarianceAG10(c, mv + 1, c, mv + 1, cp.ai1, cp.ai2, cp.phi_i, cp.thetamv, cp.Dmat)
            with pytest.raises(reflib.ReferenceError_):
                lib.CrossCovarianceAG10(c, mv + 1, c, mv + 1, cp.ai1, cp.ai2, cp.phi_i, cp.thetamv, cp.Dmat)
    check(f"covariance q={q}", worst, MEASURED_COV)


def test_zero_dmat_entry_takes_the_same_variable_branch(lib):
    """A zero Dmat entry between DIFFERENT outcomes: the reference tests v == 0, not i == j, and then uses ai1_i^2, ai2_i^2 and
    phi_i of the ROW's outcome (covariance_functions.cpp:250-255), so the matrix is not symmetric there.  The oracle follows."""
    theta = gen.crosscov_theta(3, zero_d=True)
    t = lib.transform(3, theta)
    assert t["Dmat"][2, 0] == 0.0 and t["Dmat"][0, 2] == 0.0 and t["Dmat"][1, 0] != 0.0
    c = np.array([[0.1, 0.2], [0.6, 0.9]])
    mv = np.array([1, 3])
    ref = lib.CrossCovarianceAG10(c, mv, c, mv, t["ai1"], t["ai2"], t["phi_i"], t["thetamv"], t["Dmat"])
    h = math.hypot(0.5, 0.7)
    for (i, j), o in (((0, 1), 0), ((1, 0), 2)):
        want = t["ai1"][o] ** 2 * math.exp(-t["thetamv"][2] * h) + t["ai2"][o] ** 2 * math.exp(-t["phi_i"][o] * h)
        assert abs(ref[i, j] - want) <= 1e-15 * want
    assert abs(ref[0, 1] - ref[1, 0]) > 0.01
    got = so.CrossCovarianceAG10(c, mv, c, mv, t["ai1"], t["ai2"], t["phi_i"], t["thetamv"], t["Dmat"])
    assert rel(got, ref) <= 8 * MEASURED_COV


def test_q1_reference_distance_flavour_is_the_references(lib):
    """q = 1, phi = 6 and phi ~ 500 on random points: of the oracle's three flavours of the distance form, reference_distance=True
    (|x|^2 + |y|^2 - 2 x.y in plain double arithmetic, in the source's order) is the one that matches the compiled reference
    to rounding.  The direct form sqrt(dx^2 + dy^2) (what the HIP build computes) and the emulated FMA BLAS do not: they
    differ from it by the cancellation itself, orders of magnitude above the bound."""
    rng = np.random.default_rng(9)
    c = rng.uniform(size=(60, 2))
    mv = np.zeros(60, dtype=np.int64)
    every, a, b = np.arange(60), np.arange(0, 40), np.arange(25, 60)
    worst = {True: 0.0, False: 0.0, "fma": 0.0}
    for theta in (nice_theta(1), gen.MH_START):
        cp = so.CovarianceParams(2, 1, -1)
        cp.transform(theta)
        for i1, i2, same in ((every, every, True), (a, b, False)):
            ref = lib.Covariancef(1, theta, c, mv, i1, i2, same)
            for fl in worst:
                worst[fl] = max(worst[fl], rel(so.Covariancef(c, mv, i1, i2, cp, same, fl), ref))
    print("q=1 flavours: reference_distance=True %.3g, direct %.3g, fma %.3g" % (worst[True], worst[False], worst["fma"]))
    check("q=1 reference_distance=True", worst[True], MEASURED_COV)
    assert worst[False] > 100 * 8 * MEASURED_COV and worst["fma"] > 100 * 8 * MEASURED_COV


WIDE = [(3, 12), (4, 10), (5, 10), (6, 10)]


@pytest.mark.parametrize("q,side", WIDE)
def test_covariance_at_the_wide_block_shapes(q, side, lib):
    """75-row blocks at q = 3, 100-, 125- and 150-row blocks at q = 4, 5, 6 (25 locations per cell times q outcomes): every
    block's own covariance (same = true) and its parents-by-block cross-covariance (same = false), as phases A and P ask."""
    pb = make_problem(side=side, q=q, seed=5)
    widths = [len(ix) for ix in pb["indexing"]]
    assert max(widths) == 25 * q
    theta = distinct_theta(q)
    cp = so.CovarianceParams(2, q, -1)
    cp.transform(theta)
    c, mv = pb["coords"], pb["mv_id"] - 1
    worst, crossed = 0.0, 0
    for u, iu in enumerate(pb["indexing"]):
        worst = max(worst, rel(so.Covariancef(c, mv, iu, iu, cp, True), lib.Covariancef(q, theta, c, mv, iu, iu, True)))
        if len(pb["parents"][u]):
            pi = np.concatenate([pb["indexing"][a] for a in pb["parents"][u]])
            worst = max(worst, rel(so.Covariancef(c, mv, pi, iu, cp, False), lib.Covariancef(q, theta, c, mv, pi, iu, False)))
            crossed += 1
    assert crossed >= 4
    check(f"wide q={q}", worst, MEASURED_WIDE)


# ---------------------------------------------------------------------------------------------------------------------
# mh_adapt.{h,cpp}: both restatements
# ---------------------------------------------------------------------------------------------------------------------
RESTATEMENTS = [so, product_mcmc]
IDS = ["oracle", "product_mcmc"]


def mh_params(q, seed):
    """(bounds, values inside them): random, and within 1e-12 of the lower and of the upper bound."""
    b = default_bounds(q)
    rng = np.random.default_rng(seed)
    inside = b[:, 0] + rng.uniform(0.01, 0.99, b.shape[0]) * (b[:, 1] - b[:, 0])
    low, high = b[:, 0] + 1e-12, b[:, 1] - 1e-12
    assert np.all(low > b[:, 0]) and np.all(high < b[:, 1])
    return b, [inside, low, high]


@pytest.mark.parametrize("mod", RESTATEMENTS, ids=IDS)
def test_par_huvtransf_and_jacobian(mod, lib):
    worst = 0.0
    for q in (1, 3, 6):
        b, pars = mh_params(q, q)
        for par in pars:
            f_ref = lib.par_huvtransf_fwd(par, b)
            worst = max(worst, rel(mod.par_huvtransf_fwd(par, b), f_ref))
            for x in (f_ref, np.linspace(-40.0, 40.0, par.size), np.zeros(par.size)):
                worst = max(worst, rel(mod.par_huvtransf_back(x, b), lib.par_huvtransf_back(x, b)))
        for new, old in ((pars[0], pars[1]), (pars[2], pars[0]), (pars[1], pars[2])):
            j_ref = lib.calc_jacobian(new, old, b)
            worst = max(worst, rel(mod.calc_jacobian(new, old, b), j_ref))
    check(f"{mod.__name__} par_huvtransf / calc_jacobian", worst, MEASURED_MH)


@pytest.mark.parametrize("mod", RESTATEMENTS, ids=IDS)
def test_unif_bounds_clamp_and_flag(mod, lib):
    """Below, above, at and inside the bounds: the clamp to bound +- 1e-10 and the returned flag, exactly."""
    b = default_bounds(3)
    n = b.shape[0]
    inside = 0.5 * (b[:, 0] + b[:, 1])
    cases = [inside, b[:, 0].copy(), b[:, 1].copy(), b[:, 0] - 1e-9, b[:, 1] + 1e-9, b[:, 0] - 1e3, b[:, 1] + 1e3]
    mixed = inside.copy()
    mixed[0], mixed[n - 1] = b[0, 0] - 1e-14, b[n - 1, 1] + 1e-13
    cases.append(mixed)
    flags = []
    for par in cases:
        want, want_flag = lib.unif_bounds(par, b)
        got = np.array(par, dtype=np.float64)
        flag = mod.unif_bounds(got, b)
        assert bool(flag) == want_flag and np.array_equal(got, want)
        flags.append(want_flag)
    assert flags == [False, False, False, True, True, True, True, True]
    clamped, _ = lib.unif_bounds(cases[3], b)
    assert np.array_equal(clamped, b[:, 0] + 1e-10)


@pytest.mark.parametrize("mod", RESTATEMENTS, ids=IDS)
def test_do_I_accept_with_injected_uniform(mod, lib):
    """logaccept NaN, +-inf, 0, positive, negative; u at 0, just below and just above exp(logaccept) (or 1)."""
    seen = set()
    for la in (float("nan"), float("inf"), float("-inf"), 0.0, 2.5, -0.7, -30.0, -745.0):
        thr = 0.0 if not math.isfinite(la) else (math.exp(la) if la < 0 else 1.0)
        for u in (0.0, float(np.nextafter(thr, -1.0)), thr, float(np.nextafter(thr, 2.0)), 0.5):
            if u < 0.0:
                continue
            want = lib.do_I_accept(la, u)
            assert bool(mod.do_I_accept(la, u)) == want, (la, u)
            seen.add((la, want))
    assert (0.0, True) in seen and (0.0, False) in seen and (-0.7, True) in seen and (-0.7, False) in seen
    assert not lib.do_I_accept(float("nan"), 0.0) and not lib.do_I_accept(float("inf"), 0.0) and lib.do_I_accept(0.0, 0.0)


@pytest.mark.parametrize("p", gen.RAM_PS)
@pytest.mark.parametrize("mod", RESTATEMENTS, ids=IDS)
def test_ramadapt_trajectory(mod, p, lib):
    """paramsd after every one of 120 steps (across the member g0 = 50, which shadows the file-level 500, and the `started`
    switch), S, started and accept_ratio, on a recorded sequence of U, alpha (NaN and inf among them) and accept flags with
    runs of rejections."""
    S0, U, alpha, accept = gen.ram_inputs(p)
    ref = lib.RAMAdapt(p, S0)
    assert ref.g0 == 50
    P, S, started, ratio = gen.run_ram(ref, U, alpha, accept)
    assert started[49] == 0 and started[50] == 1 and np.all(P[49] == P[0]) and np.any(P[50] != P[0])
    ours = mod.RAMAdapt(p, S0)
    worst = 0.0
    for mc in range(gen.RAM_STEPS):
        ours.count_proposal()
        if accept[mc]:
            ours.count_accepted()
        ours.update_ratios()
        ours.adapt(U[mc], float(alpha[mc]), mc)
        assert bool(ours.started) == bool(started[mc]) and ours.accept_ratio == ratio[mc], mc
        scale = np.abs(P[mc]).max()
        worst = max(worst, float(np.abs(ours.paramsd - P[mc]).max() / scale))
        if started[mc]:
            worst = max(worst, float(np.abs(ours.S - S[mc]).max() / np.abs(S[mc]).max()))
    check(f"{mod.__name__} RAMAdapt p={p}", worst, MEASURED_RAM, factor=10.0)


# ---------------------------------------------------------------------------------------------------------------------
# list_mean.cpp, find_nan.cpp
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep", [1, 2, 3, 7, 8, 40, 65])
def test_list_qtile_bitwise_and_list_mean(keep, lib):
    """oracle.list_summaries against the live list_qtile: selection and one interpolation expression in IEEE double leave
    nothing to round differently, so the bits agree -- on the fixture's draws (ties, constants, repeats) and on the rows and
    the q grid of tests/test_outputs_reference.py (every k / keep with both neighbours: the inputs on which the stepwise
    rounding of r decides the pick).  The draws hold no -0.0: it compares equal to +0.0, so which of the two nth_element
    or a sort puts first is their choice, and with it the sign of a zero quantile.  list_mean within keep 2^-52 max|x|."""
    from tests import test_outputs_reference as outref
    sets = [outref.qtile_rows(keep, 48, seed=keep) + 0.0]      # + 0.0: no -0.0 (see the docstring)
    if keep in gen.KEEPS:
        sets.append(gen.summary_draws(keep))
    for draws in sets:
        x = [draws[i].reshape(-1, 1) for i in range(keep)]
        qs = set(outref.qtile_qs(keep)) | set(gen.REQUIRED_QS) | set(gen.landing_qs(keep))
        for q in sorted(qs):
            want = lib.list_qtile(x, q)
            got = list_summaries.list_qtile(x, q)
            assert got.shape == want.shape and got.tobytes() == want.tobytes(), (keep, q)
        finite_scale = draws[:, np.abs(draws).max(axis=0) < 1e200]
        x = [finite_scale[i].reshape(-1, 1) for i in range(keep)]
        want, got = lib.list_mean(x), list_summaries.list_mean(x)
        assert np.all(np.abs(got - want) <= keep * 2.0 ** -52 * np.abs(finite_scale).max(axis=0).reshape(-1, 1))


def test_landing_quantiles_land_where_they_should():
    for keep in gen.KEEPS:
        whole, half = gen.landing_qs(keep)
        rw, rh = gen.qtile_r(whole, keep), gen.qtile_r(half, keep)
        assert rw == int(rw) and rh - int(rh) == 0.5


def test_find_nan_selects_rows_by_the_first_filter_column(lib):
    rng = np.random.default_rng(3)
    a = [rng.standard_normal((7, 3)) for _ in range(3)]
    f = [rng.standard_normal((7, 2)) for _ in range(3)]
    f[0][[1, 4], 0] = np.nan
    f[1][:, 0] = np.inf
    f[2][3, 1] = np.nan                  # the second column does not filter
    for i, (kept, dropped) in enumerate(zip(lib.find_not_nan(a, f), lib.find_nan(a, f))):
        ok = np.isfinite(f[i][:, 0])
        assert np.array_equal(kept, a[i][ok]) and np.array_equal(dropped, a[i][~ok])


# ---------------------------------------------------------------------------------------------------------------------
# fixture provenance
# ---------------------------------------------------------------------------------------------------------------------
def test_fixtures_are_what_the_library_gives_today(lib):
    """Regenerating every array of every tests/golden/ref_*.npz in memory gives the committed bytes: the fixtures are outputs
    of the compiled reference for exactly the recorded inputs, and nothing else is in those files."""
    files = gen.build_all(lib)
    on_disk = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.startswith("ref_") and f.endswith(".npz"))
    assert on_disk == sorted(files)
    for name, arrays in files.items():
        path = os.path.join(GOLDEN, name + ".npz")
        assert os.path.getsize(path) < 300 * 1024
        with np.load(path) as z:
            assert sorted(z.files) == sorted(arrays), name
            for key, want in arrays.items():
                want, got = np.asarray(want), z[key]
                assert got.dtype == want.dtype and got.shape == want.shape, (name, key)
                assert got.tobytes() == want.tobytes(), (name, key)


# ---------------------------------------------------------------------------------------------------------------------
# the restatements against the RECORDED reference outputs: no library, no reference tree needed
# ---------------------------------------------------------------------------------------------------------------------
def test_oracle_covariance_reproduces_the_recorded_reference():
    """CrossCovarianceAG10 on every recorded case (the oracle's own transform of the recorded theta supplies the parameters, so
    slicing and the Dmat fill are part of what is compared) and the dense Covariancef(., same = true) of every recorded
    problem; q = 1 in the reference_distance=True flavour."""
    f = recorded("ref_crosscov")
    worst = 0.0
    for name, q, _ in gen.CROSSCOV_CASES:
        cp = so.CovarianceParams(2, q, -1)
        cp.transform(f[f"{name}_theta"])
        assert np.array_equal(cp.Dmat, f[f"{name}_Dmat"]) and np.array_equal(cp.ai2, f[f"{name}_ai2"])
        got = so.CrossCovarianceAG10(f[f"{name}_coords1"], f[f"{name}_mv1"], f[f"{name}_coords2"], f[f"{name}_mv2"], cp.ai1, cp.ai2,
                                     cp.phi_i, cp.thetamv, cp.Dmat)
        worst = max(worst, rel(got, f[f"{name}_out"]))
    e = recorded("ref_crosscov_rd")
    got = so.CrossCovarianceAG10(e["cx"], e["mv"], e["cx"], e["mv"], e["ai1"], e["ai2"], e["phi_i"], e["thetamv"], e["Dmat"])
    worst = max(worst, rel(got, gen.from_upper(e["out_upper"], 200)))
    for name, (kw, thetas) in gen.DENSE.items():
        d = recorded("ref_dense_" + name)
        n, q = d["coords"].shape[0], kw["q"]
        rows = np.arange(n)
        for tname in thetas:
            cp = so.CovarianceParams(2, q, -1)
            cp.transform(d["theta_" + tname])
            got = so.Covariancef(d["coords"], d["mv_id"] - 1, rows, rows, cp, True, q == 1)
            worst = max(worst, rel(got, gen.from_upper(d["K_upper_" + tname], n)))
    check("oracle against the recorded covariances", worst, MEASURED_COV)


@pytest.mark.parametrize("p", gen.RAM_PS)
@pytest.mark.parametrize("mod", RESTATEMENTS, ids=IDS)
def test_ramadapt_follows_the_recorded_trajectory(mod, p):
    d = recorded(f"ref_ramadapt_p{p}")
    low = np.tril_indices(p)
    assert d["started"][49] == 0 and d["started"][50] == 1
    ours = mod.RAMAdapt(p, d["S0"])
    worst = 0.0
    for mc in range(gen.RAM_STEPS):
        ours.count_proposal()
        if d["accept"][mc]:
            ours.count_accepted()
        ours.update_ratios()
        ours.adapt(d["U"][mc], float(d["alpha"][mc]), mc)
        assert bool(ours.started) == bool(d["started"][mc]) and ours.accept_ratio == d["accept_ratio"][mc], mc
        assert np.all(np.triu(ours.paramsd, 1) == 0.0)
        want = d["paramsd_lower"][mc]
        worst = max(worst, float(np.abs(ours.paramsd[low] - want).max() / np.abs(want).max()))
    check(f"{mod.__name__} against the recorded RAMAdapt p={p}", worst, MEASURED_RAM, factor=10.0)


def test_list_summaries_reproduce_the_recorded_reference():
    d = recorded("ref_summaries")
    for keep in gen.KEEPS:
        draws = d[f"draws_{keep}"]
        x = [draws[i].reshape(-1, 1) for i in range(keep)]
        for i, q in enumerate(d[f"qs_{keep}"]):
            assert list_summaries.list_qtile(x, float(q)).reshape(-1).tobytes() == d[f"qtile_{keep}"][i].tobytes(), (keep, q)
        got = list_summaries.list_mean(x).reshape(-1)
        assert np.all(np.abs(got - d[f"mean_{keep}"]) <= keep * 2.0 ** -52 * np.abs(draws).max(axis=0))
