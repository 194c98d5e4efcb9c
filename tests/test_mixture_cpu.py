"""CPU: quantiles and the exact CRPS of the mixture predictive at new points (include/spamtree_hip.h, st_points_mixture_*).  The host
restatement spamtree_amd.mixture against the 50-digit reference tests/mixture_reference.py on a fixed list of mixtures; the CRPS
against three independent checks (the closed form of one normal, the integral of (F - 1)^2 by quadrature, its limits); the layout of
the new structs in header and binding; the refusals of stm_fit_run before a chain exists; the host-only launch plan
(tests/mixture_plan_check.cpp over spamtree_amd/csrc/mixture_plan.cpp and store_spec.cpp, plain and under the host sanitizers) and every ValueError of
the front doors."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import mixture_reference as mr
from tests.test_exceed_cpu import fields_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spamtree_amd", "csrc")
USAGE, UNSUPPORTED = -1, -4   # include/spamtree_hip.h: ST_ERR_USAGE, ST_ERR_UNSUPPORTED
PROBS = (1e-6, 0.025, 0.5, 0.975, 1 - 1e-6)

# (means, variances, probabilities beside PROBS)
MIXTURES = {
    "K1": ([0.3], [2.0], ()),
    "K2": ([-1.0, 1.5], [1.0, 0.25], ()),
    "far_modes": ([-50.0, 50.0], [1.0, 1.0], (0.5,)),             # p = 1/2: the quantile sits in the gap, where the density underflows
    "far_modes_3": ([-200.0, 0.0, 300.0], [1.0, 4.0, 1.0], (1 / 3, 2 / 3)),
    "all_equal": ([0.7] * 5, [0.09] * 5, ()),
    "all_degenerate": ([0.3, -0.2, 0.3, 1.0], [0.0] * 4, (0.25, 0.75)),
    "one_jump": ([0.0, 0.1, -0.3, 0.2], [1.0, 0.0, 2.0, 0.5], (0.55, 0.6, 0.7)),   # the point mass at 0.1 carries F from 0.52 to 0.77
    "small_scale": ([1e-8, 2e-8, -1e-8], [1e-16, 4e-16, 1e-18], ()),
    "large_scale": ([1e8, -3e8, 2e8], [1e16, 4e16, 1e14], ()),
    "mixed_scale": ([0.0, 1.0, 1e4], [1e-16, 1.0, 1e16], ()),
    "many": ([0.1 * k - 1.0 for k in range(23)], [0.05 + 0.01 * k * k for k in range(23)], ()),
}


def comps_of(name):
    m, v, extra = MIXTURES[name]
    return np.array(m), np.array(v), mr.components(m, v), tuple(PROBS) + tuple(extra)


# ---- 1. the definition ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MIXTURES))
def test_cdf_and_quantile_against_the_reference(name):
    """mixture.quantile bisects to adjacent doubles, so it is held to the definition as the device is, with the width delta
    replaced by one ulp of the result."""
    from spamtree_amd import mixture as mx
    m, v, comps, probs = comps_of(name)
    for x in list(m) + [float(np.mean(m)), float(m.min() - 3 * np.sqrt(v.max()) - 1), float(m.max() + 2 * np.sqrt(v.max()) + 1)]:
        got, want = mx.cdf(x, m, v), mr.cdf(x, comps)
        assert mr.err(got, want) <= mr.eps_F(x, comps), (name, x, got, float(want))
        assert 0.0 <= got <= 1.0
    last = -math.inf
    for p in sorted(probs):
        x = mx.quantile(p, m, v)
        ulp = math.ulp(x) if x != 0.0 else 5e-324
        eps = max(mr.eps_F(x, comps), mr.eps_F(x - ulp, comps))
        assert float(mr.cdf(x, comps) - p) >= -eps, (name, p, x)                     # F(x) >= p
        assert float(mr.cdf(mr.mp.mpf(x) - ulp, comps) - p) <= eps, (name, p, x)    # ... and F < p one ulp below: x is the infimum
        assert mr.check_quantile(x, p, comps) <= 1.0, (name, p, x)                  # so it passes the device's check too
        assert x >= last, (name, p)
        last = x
        lo, hi = mr.quantile(p, comps)                      # where the reference's own bisection ends: F(lo) < p <= F(hi)
        assert float(hi - lo) <= 1e-30 * max(1.0, abs(x)) and mr.cdf(lo, comps) < p <= mr.cdf(hi, comps)


def test_hand_cases():
    from spamtree_amd import mixture as mx
    assert mx.cdf(0.0, [0.0], [1.0]) == 0.5
    assert mx.cdf(0.1, [0.1], [0.0]) == 1.0 and mx.cdf(math.nextafter(0.1, -1), [0.1], [0.0]) == 0.0   # right-continuous
    assert mx.quantile(0.5, [0.1, 0.1, 7.0], [0.0, 0.0, 0.0]) == 0.1                                     # inf{x : F(x) >= p} at a jump
    assert mx.quantile(0.7, [0.1, 0.1, 7.0], [0.0, 0.0, 0.0]) == 7.0
    assert abs(mx.quantile(0.975, [2.0], [9.0]) - (2.0 + 3.0 * 1.959963984540054)) <= 1e-14
    assert mx.quantile(0.5, [0.0], [0.0]) == 0.0                                                          # an empty functional
    # K = 2, equal variances, symmetric: the median is the midpoint
    assert abs(mx.quantile(0.5, [-1.0, 1.0], [1.0, 1.0])) <= 1e-15
    assert mx.crps(0.3, [0.3], [0.0]) == 0.0 and mx.crps(1.0, [0.0], [0.0]) == 1.0
    assert mx.spread([0.0, 2.0], [0.0, 0.0]) == 0.5      # (2 |0 - 2|) / (2 x 4)
    assert abs(mx.spread([0.0], [1.0]) - 1 / math.sqrt(math.pi)) <= 2.0 ** -52


# ---- 2. the CRPS, three independent checks -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("y", [-3.0, 0.0, 0.4, 25.0])
def test_crps_at_K1_is_the_closed_form_of_a_normal(y):
    from spamtree_amd import mixture as mx
    for m, sd in ((0.3, 1.5), (-2.0, 1e-3), (10.0, 40.0)):
        v = sd * sd                                        # the double that is handed over; its exact root goes into the closed form
        want = mr.crps_normal(y, m, mr.mp.sqrt(mr.mp.mpf(v)))
        comps = mr.components([m], [v])
        ref = mr.crps(y, comps)
        assert abs(ref - want) <= mr.mp.mpf(10) ** -40 * max(1, abs(want))
        got = mx.crps(y, [m], [v])
        bound, _ = mr.crps_bounds(1, mr.t1_mean(y, comps), mr.spread(comps))
        assert mr.err(got, want) <= bound, (y, m, sd, got, float(want), bound)


@pytest.mark.parametrize("name", ["K1", "K2", "all_degenerate", "one_jump", "all_equal", "far_modes"])
def test_crps_is_the_integral_of_the_squared_cdf_difference(name):
    """crps = integral (F(x) - 1(x >= y))^2 dx does not go through A: a wrong closed form fails here in the restatement and in
    spamtree_amd.mixture at once.  K <= 5."""
    from spamtree_amd import mixture as mx
    m, v, comps, _ = comps_of(name)
    assert len(comps) <= 5
    for y in (float(m[0]), float(np.mean(m)) + 0.37, float(m.min()) - 2.0):
        quad = mr.crps_by_quadrature(y, comps)
        ref = mr.crps(y, comps)
        assert abs(ref - quad) <= mr.mp.mpf(10) ** -12 * max(1, abs(quad)), (name, y, float(ref), float(quad))
        got = mx.crps(y, m, v)
        bound, sb = mr.crps_bounds(len(comps), mr.t1_mean(y, comps), mr.spread(comps))
        assert mr.err(got, ref) <= bound, (name, y)
        assert mr.err(mx.spread(m, v), mr.spread(comps)) <= sb, name


def test_crps_is_nonnegative_and_tends_to_the_absolute_error():
    from spamtree_amd import mixture as mx
    rng = np.random.default_rng(3)
    for K in (1, 2, 7, 40):
        m, v = rng.standard_normal(K), rng.uniform(0.0, 2.0, K)
        for y in (-4.0, float(m[0]), 0.1, 9.0):
            assert mx.crps(y, m, v) >= -1e-15
    m = np.array([0.25] * 6)
    for y in (-1.0, 0.25, 3.0):
        last = None
        for s2 in (1.0, 1e-4, 1e-8, 1e-16, 0.0):
            c = mx.crps(y, m, np.full(6, s2))
            assert abs(c - abs(y - 0.25)) <= 0.6 * math.sqrt(s2) + 1e-15      # 0 <= A - |d| <= 0.80 sd and spread = 0.56 sd
            last = c
        assert last == abs(y - 0.25)


# ---- 3. layout -----------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_new_structs_alike(tmp_path):
    from spamtree_amd import _lib
    assert fields_of("spamtree_hip.h", "st_mix_out") == [f[0] for f in _lib.StMixOut._fields_] == ["q", "n_unconverged"]
    assert fields_of("spamtree_fit.h", "stm_mixture") == [f[0] for f in _lib.StmMixture._fields_]
    assert fields_of("spamtree_fit.h", "stm_fit_more") == [f[0] for f in _lib.StmFitMore._fields_] == ["mix"]
    assert _lib.ST_MIX_MAX_DRAWS == 8192 and _lib.ST_MIX_MAX_PROBS == 8
    hdr = open(os.path.join(ROOT, "include", "spamtree_hip.h")).read()
    assert "#define ST_MIX_MAX_DRAWS 8192" in hdr and "#define ST_MIX_MAX_PROBS 8" in hdr
    mxp = C.POINTER(_lib.StMixOut)
    assert _lib.SIGNATURES["st_points_mixture_reserve"] == (C.c_int, [C.c_void_p, C.c_int64])
    assert _lib.SIGNATURES["st_points_mixture_draws"] == (C.c_int, [C.c_void_p] + [_lib.c_dp] * 4 + [_lib.c_ip])
    assert _lib.SIGNATURES["st_points_mixture_quantiles"] == (C.c_int, [C.c_void_p, C.c_int32, _lib.c_dp, mxp, mxp, mxp])
    assert _lib.SIGNATURES["st_points_mixture_crps"] == (C.c_int, [C.c_void_p, _lib.c_dp, _lib.c_dp, _lib.c_ip])
    assert _lib.SIGNATURES["stm_fit_run"] == (C.c_int, [C.POINTER(_lib.StmFit), C.POINTER(_lib.StmFitMore)])
    assert not [s for s in _lib.SIGNATURES if s.startswith("stm_mcmc_") and "mix" in s]
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    src = tmp_path / "mix_layout.cpp"
    lines = ['#include <cstddef>', '#include <cstdio>', '#include "spamtree_fit.h"', "int main() {"]
    want = {}
    for cname, cls in (("st_mix_out", _lib.StMixOut), ("stm_mixture", _lib.StmMixture), ("stm_fit_more", _lib.StmFitMore)):
        lines.append(f'  std::printf("{cname} %zu\\n", sizeof({cname}));')
        want[cname] = C.sizeof(cls)
        for f in cls._fields_:
            lines.append(f'  std::printf("{cname}.{f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
            want[f"{cname}.{f[0]}"] = getattr(cls, f[0]).offset
    src.write_text("\n".join(lines + ["  return 0;", "}"]) + "\n")
    exe = str(tmp_path / "mix_layout")
    subprocess.run([hipcc, "--offload-host-only", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, timeout=600)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, check=True).stdout
    assert {k: int(v) for k, v in (line.split() for line in out.splitlines())} == want


# ---- 4. the driver's refusals ------------------------------------------------------------------------------------------------------
def mix_request(points=True, X=True, fun=False, scores=False, probs=(0.5,), n_probs=None, w=True, yhat=False, fun_w=False, crps=False,
                spread=False, keep=8, chains=1, y_nan=False):
    """(request, stm_fit_more, what they point at) over tests/test_fit_request_cpu.Request."""
    from spamtree_amd import _lib
    from tests.test_fit_request_cpu import N_NEW, Request
    r = Request()
    r.fit.run.mcmc_keep = keep
    if points:
        r.points(X=X)
    if fun:
        r.functionals()
    y = np.full(N_NEW, np.nan)
    if scores:
        r.part("scores", _lib.StmScores(r.dbl_of(y) if y_nan else r.dbl))
    if chains > 1:
        r.chains(chains)
    pr = np.array(probs, dtype=np.float64)
    cnt = [C.c_int64() for _ in range(4)]
    out = lambda want, k: _lib.StMixOut(r.dbl, C.pointer(cnt[k])) if want else _lib.StMixOut()   # noqa: E731
    mix = _lib.StmMixture(pr.ctypes.data_as(_lib.c_dp) if pr.size else None, pr.size if n_probs is None else n_probs, out(w, 0), out(yhat, 1),
                          out(fun_w, 2), r.dbl if crps else None, r.dbl if spread else None, C.pointer(cnt[3]))
    more = _lib.StmFitMore(C.pointer(mix))
    return r, more, (pr, cnt, mix, y)


def test_driver_refuses_before_the_first_factorisation():
    """stm_fit_run returns the refusals of mix before it creates the chain: no device is touched, so they are checked here."""
    from spamtree_amd import _lib
    lib = _lib.load()

    def run(**kw):
        r, more, held = mix_request(**kw)
        rc = lib.stm_fit_run(C.byref(r.fit), C.byref(more))
        assert not r.buf.any() and all(c.value == 0 for c in held[1])        # a refused request writes nothing
        return rc

    nine = [0.1 * (k + 1) for k in range(9)]
    for kw in (dict(points=False),                                       # mix without a point set
               dict(X=False, yhat=True),                                 # a new_yhat output without X_new
               dict(X=False, crps=True), dict(X=False, w=False, spread=True),   # crps / spread without X_new
               dict(crps=True), dict(spread=True),                       # crps without scores
               dict(scores=True, y_nan=True, crps=True), dict(scores=True, y_nan=True, w=False, spread=True),   # ... or with no scored point
               dict(fun_w=True),                                         # fun_w without fun
               dict(probs=nine), dict(probs=(), n_probs=0), dict(n_probs=-1),    # n_probs outside 1 .. 8
               dict(probs=[0.0]), dict(probs=[1.0]), dict(probs=[0.5, -0.1]), dict(probs=[0.5, 1.5]), dict(probs=[np.nan]),
               dict(probs=[0.5, np.inf]),
               dict(probs=[np.nan], keep=8193),                          # the probabilities come before the store's limit
               dict(fun_w=True, keep=8193),                              # ... and so does fun_w without fun
               dict(w=False, probs=[2.0], n_probs=1)):                   # probabilities are read whenever n_probs != 0
        assert run(**kw) == USAGE, kw
    for kw in (dict(keep=8193), dict(keep=4097, chains=2), dict(keep=8193, w=False, probs=(), n_probs=0)):   # chains x mcmc_keep beyond ST_MIX_MAX_DRAWS
        assert run(**kw) == UNSUPPORTED, kw
        assert b"at most 8192" in lib.stm_mcmc_chains_last_error()
    assert run(keep=8193, scores=True, crps=True, X=False) == USAGE      # the order of the checks: X_new before the limit


def test_stm_fit_run_without_more_is_stm_mcmc_fit():
    """Both doors refuse the same requests with the same codes and the same text (tests/test_fit_request_cpu.py's table)."""
    from spamtree_amd import _lib
    from tests.test_fit_request_cpu import CASES, Request
    lib = _lib.load()
    assert lib.stm_fit_run(None, None) == USAGE == lib.stm_mcmc_fit(None)
    n = 0
    for case in CASES:
        symbol, build, rc, text = case.values
        seen = []
        for door in ("stm_mcmc_fit", "stm_fit_run", "stm_fit_run_empty"):
            r = Request()
            build(r)
            more = _lib.StmFitMore()
            got = lib.stm_mcmc_fit(C.byref(r.fit)) if door == "stm_mcmc_fit" else lib.stm_fit_run(C.byref(r.fit), None if door == "stm_fit_run" else C.byref(more))
            seen.append((got, lib.stm_mcmc_chains_last_error().decode()))
            assert not r.buf.any()
        assert seen[0] == seen[1] == seen[2] and seen[0][0] == rc, (symbol, build.__name__, seen)
        n += 1
    assert n >= 20


# ---- 5. the plan ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_plan_check_program(tmp_path, sanitize):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    exe = str(tmp_path / "mixture_plan_check")
    # a stand-alone host program, with the sanitizers on the CPU in its second build: nothing is preloaded
    san = ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.run([hipcc, "--offload-host-only", "-std=c++17", "-O1"] + san + ["-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "mixture_plan_check.cpp"), os.path.join(CSRC, "mixture_plan.cpp"),
                    os.path.join(CSRC, "store_spec.cpp"), "-o", exe], check=True, timeout=600)
    for lim in ("163840", "65536", "4096"):
        r = subprocess.run([exe, lim], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.startswith("OK "), (lim, r.stdout, r.stderr)


def test_the_reference_restates_the_plans_group_size():
    src = open(os.path.join(CSRC, "mixture_plan.cpp")).read()
    assert "K <= 64 ? 64 : K <= 128 ? 128 : MIX_NT" in src
    assert [mr.crps_group(K) for K in (1, 64, 65, 128, 129, 8192)] == [64, 64, 128, 128, 256, 256]
    hdr = open(os.path.join(CSRC, "points_mixture.hpp")).read()
    kern = open(os.path.join(CSRC, "k_points_mixture.hip")).read()
    assert "2^-50 M" in hdr and "2^-51 M" in hdr and "4.440892098500626e-16" in kern and 2.0 ** -51 == 4.440892098500626e-16
    assert mr.DELTA_REL == 2.0 ** -50


# ---- 6. the front doors ----------------------------------------------------------------------------------------------------------------
def test_fit_and_predict_refuse_before_any_device_call():
    from spamtree_amd import fit, predict
    from spamtree_amd import mixture as mx
    from tests.util import make_problem
    pb = make_problem(side=8, q=2, seed=1)
    k = pb["theta"].size
    real = (pb["y"], pb["X"], pb["Z"], pb["coords"], pb["mv_id"], pb["blocking"], pb["gix_block"], pb["res_is_ref"], pb["parents"],
            pb["children"], bool(pb["limited_tree"]), pb["block_names"], pb["block_groups"], pb["indexing"], pb["bounds"],
            np.zeros(pb["n"]), pb["theta"], np.zeros(pb["p"]), 0.1, 0.02 * np.eye(k))
    pts = dict(coords=np.zeros((4, 2)), mv=np.array([1, 2, 1, 2]), anchor=np.zeros(4, dtype=np.int64), X=np.zeros((4, pb["p"])))
    bad = (dict(), dict(probs=None), dict(probs=[0.1] * 9), dict(probs=[]), dict(probs=[0.0]), dict(probs=[1.0]), dict(probs=[np.nan]),
           dict(probs=[0.5, 1.5]), dict(probs=0.5, level=0.1), dict(crps=True), dict(probs=0.5, crps=True), 0.5)
    for spec in bad:                                       # (crps=True without y is refused too)
        with pytest.raises(ValueError):
            fit.spamtree_mv_mcmc(*real, new_points=dict(pts, mixture=spec), mcmc_keep=5, mcmc_burn=1, main_verbose=False)
    with pytest.raises(ValueError):                       # crps with no scored point: known before any chain runs
        fit.spamtree_mv_mcmc(*real, new_points=dict(pts, y=np.full(4, np.nan), mixture=dict(crps=True)), mcmc_keep=5, mcmc_burn=1, main_verbose=False)
    with pytest.raises(ValueError):                       # crps needs X
        fit.spamtree_mv_mcmc(*real, new_points=dict(pts, X=None, mixture=dict(crps=True)), mcmc_keep=5, mcmc_burn=1, main_verbose=False)
    for kw in (dict(mcmc_keep=8193), dict(mcmc_keep=4097, chains=2, chain_seeds=[1, 2])):   # the store's limit, over all chains
        with pytest.raises(ValueError):
            fit.spamtree_mv_mcmc(*real, new_points=dict(pts, mixture=dict(probs=0.5)), mcmc_burn=1, main_verbose=False, **kw)
    draws = dict(w_mcmc=[np.zeros(pb["n"])] * 3, beta_mcmc=np.zeros((pb["p"], 3, 2)), tausq_mcmc=np.ones((2, 3)), theta_mcmc=np.ones((k, 3)))
    for spec in bad:
        with pytest.raises(ValueError):
            predict.fit_predict(pb, pts["coords"], pts["mv"], pts["X"], mixture=spec, mcmc_keep=5)
        with pytest.raises(ValueError):
            predict.predict_new(pb, draws, pts["coords"], pts["mv"], pts["X"], mixture=spec)
    for kw in (dict(z=np.zeros((4, 3))), dict(mode=1)):  # the replay goes through st_points_accumulate: the device's draw only
        with pytest.raises(ValueError):
            predict.predict_new(pb, draws, pts["coords"], pts["mv"], pts["X"], mixture=dict(probs=0.5), **kw)
    probs, crps = mx.check_spec(dict(probs=[0.975, 0.025], crps=True))
    assert probs.tolist() == [0.975, 0.025] and probs.dtype == np.float64 and crps is True
    assert mx.check_spec(dict(crps=True)) == (None, True)
    assert mx.check_spec(dict(crps=True), y=[np.nan, 0.5]) == (None, True)
    with pytest.raises(ValueError):
        mx.check_spec(dict(crps=True), y=[np.nan, np.nan])
    tot, by = mx.point_means([1.0, 2.0, 4.0, 8.0], [0.0, np.nan, 0.0, 0.0], [1, 1, 2, 1], 3)
    assert tot == 13.0 / 3 and by[0] == 4.5 and by[1] == 4.0 and np.isnan(by[2])
    with pytest.raises(ValueError):
        mx.check_spec(dict(probs=0.5), keep=8193)
    with pytest.raises(ValueError):
        mx.quantile(0.0, [0.0], [1.0])
    with pytest.raises(ValueError):
        mx.cdf(0.0, [0.0], [-1.0])
