"""CPU: the Rao-Blackwellised exceedance probabilities at new points (include/spamtree_hip.h, st_points_exceed_*).  The host
restatement spamtree_amd.exceed against the 50-digit reference tests/exceed_reference.py on a fixed list of cases, the layout of the
new structs in header and binding, the refusals of stm_mcmc_fit before a chain exists, and every ValueError of the front doors."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import exceed_reference as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
USAGE = -1   # include/spamtree_hip.h: ST_ERR_USAGE
SUB = 5e-324  # the smallest subnormal


# ---- 1. the definition ---------------------------------------------------------------------------------------------------------------
# (cond_mean per draw, cond_var per draw, threshold)
CASES = [
    ([-1.0, 1.0], [1.0, 1.0], 0.0),                                    # the hand case
    ([0.3], [0.0], 0.5), ([0.5], [0.0], 0.5), ([0.7], [0.0], 0.5),     # v = 0 with m <, =, > c
    ([0.3, 0.5, 0.7, 0.5], [0.0, 0.0, 0.0, 2.0], 0.5),                 # ... mixed with a proper draw
    ([40.0], [1.0], 0.0), ([-40.0], [1.0], 0.0), ([38.0, -38.5], [1.0, 1.0], 0.0),   # |z| up to 40: erfc underflows (gradually from 37.5)
    ([8.0, -8.0, 3.0], [0.04, 0.04, 1e-4], 0.0),                       # |z| = 40 and 300 through small variances
    ([1e-170, -1e-170, 0.0], [SUB, 1e-310, SUB], 0.0),                 # subnormal v: its root is a normal number
    ([1e-162, 2e-162], [SUB, SUB], 1.5e-162),                          # ... with |z| of order 1
    ([0.123456789], [0.75], -0.25),                                    # S = 1
    ([0.1 * k - 1.0 for k in range(23)], [0.05 + 0.01 * k * k for k in range(23)], 0.4),
    ([1e3, -1e3, 0.0], [1.0, 1.0, 1.0], 0.0),                          # far tails both ways in one series
]


@pytest.mark.parametrize("side", [1, -1])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_exceed_py_against_the_reference(case, side):
    from spamtree_amd import exceed as rb
    m, v, c = CASES[case]
    S = len(m)
    got = rb.exceed_w(np.array([m]), np.array([v]), [1], np.array([[c]]), np.array([side]))
    prob, pb, var, vb = er.point_w(m, v, c, side)
    assert got["n_accumulated"] == S and got["prob"].shape == (1, 1)
    ep, ev = er.err(got["prob"][0, 0], prob), er.err(got["prob_var"][0, 0], var)
    assert ep <= pb and ev <= vb, (case, side, ep, pb, ev, vb)
    assert 0.0 <= got["prob"][0, 0] <= 1.0 and 0.0 <= got["prob_var"][0, 0] <= 0.25 + vb
    assert not np.isnan(got["prob"]).any() and not np.isnan(got["prob_var"]).any()
    # the stream does what the one-shot call does, draw by draw
    st = rb.Stream()
    for s in range(S):
        st.update(rb.draw_prob(m[s], v[s], c, side))
    fin = st.finish()
    assert fin["prob"] == got["prob"][0, 0] and fin["prob_var"] == got["prob_var"][0, 0]


def test_the_hand_case_and_the_strict_side():
    from spamtree_amd import exceed as rb
    got = rb.exceed_w(np.array([[-1.0, 1.0]]), np.ones((1, 2)), [1], np.array([[0.0]]), np.array([1]))
    phi1 = 0.5 * math.erfc(-1.0 / math.sqrt(2.0))
    assert abs(got["prob"][0, 0] - 0.5) <= 2 ** -52
    assert abs(got["prob_var"][0, 0] - (phi1 - 0.5) ** 2) <= 2 ** -50
    for side in (1, -1):                                 # v = 0: strict on both sides, exact
        assert rb.draw_prob(0.5, 0.0, 0.5, side) == 0.0
        assert rb.draw_prob(0.7, 0.0, 0.5, side) == (1.0 if side > 0 else 0.0)
        assert rb.draw_prob(0.3, 0.0, 0.5, side) == (0.0 if side > 0 else 1.0)
        assert rb.draw_prob(0.5, 1.0, 0.5, side) == 0.5  # v > 0 at the threshold: a half
    assert rb.draw_prob(1e3, 1.0, 0.0, 1) == 1.0 and rb.draw_prob(1e3, 1.0, 0.0, -1) == 0.0
    assert rb.draw_prob(1e300, SUB, -1e300, 1) == 1.0    # z overflows: the limit, not NaN


def test_the_yhat_target_against_the_reference():
    from spamtree_amd import exceed as rb
    rng = np.random.default_rng(4)
    n, S, p, q, T = 9, 5, 3, 2, 3
    X = rng.standard_normal((n, p))
    mv = rng.integers(1, q + 1, size=n)
    cm, cv = rng.standard_normal((n, S)), rng.uniform(0.0, 2.0, (n, S))
    cv[0] = 0.0                                          # sigma2 = tau2 > 0 all the same
    beta = rng.standard_normal((p, S, q))
    tsi = 1.0 / rng.uniform(0.05, 0.5, (q, S))
    thr = np.array([[-30.0, 30.0], [0.1, -0.2], [1e3, -1e3]])
    side = np.array([1, -1, 1], dtype=np.int32)
    got = rb.exceed_yhat(cm, cv, mv, X, beta, tsi, thr, side)
    refs = [[er.point_yhat(X[i], [beta[:, s, mv[i] - 1] for s in range(S)], cm[i], cv[i], tsi[mv[i] - 1], thr[t, mv[i] - 1], int(side[t]))
             for i in range(n)] for t in range(T)]
    er.check_target(got, refs, "yhat")
    gw = rb.exceed_w(cm, cv, mv, thr, side)
    er.check_target(gw, [[er.point_w(cm[i], cv[i], thr[t, mv[i] - 1], int(side[t])) for i in range(n)] for t in range(T)], "w")
    assert np.all(gw["prob"][2, mv == 1] == 0.0) and np.all(gw["prob"][2, mv == 2] == 1.0)   # the far tails are exact


# ---- 2. layout -----------------------------------------------------------------------------------------------------------------------
def fields_of(header, name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", hdr, flags=re.S).group(1)
    return re.findall(r"[\*\s](\w+)\s*[,;]", body)


def test_header_and_binding_declare_the_new_structs_alike(tmp_path):
    from spamtree_amd import _lib
    assert fields_of("spamtree_hip.h", "st_rb_out") == [f[0] for f in _lib.StRbOut._fields_] == ["prob", "prob_var"]
    assert fields_of("spamtree_fit.h", "stm_rb_exceed") == [f[0] for f in _lib.StmRbExceed._fields_]
    assert fields_of("spamtree_fit.h", "stm_excursions") == [f[0] for f in _lib.StmExcursions._fields_]
    assert _lib.StmExcursions._fields_[-1] == ("rb", C.POINTER(_lib.StmRbExceed))
    assert _lib.SIGNATURES["st_points_exceed_set"] == (C.c_int, [C.c_void_p, C.c_int32, _lib.c_dp, C.POINTER(C.c_int32), _lib.c_dp])
    assert _lib.SIGNATURES["st_points_exceed_get"] == (C.c_int, [C.c_void_p] + [C.POINTER(_lib.StRbOut)] * 3 + [_lib.c_ip])
    xs = _lib.StmExcursions(1)                           # positional constructions keep working; rb defaults to NULL
    assert xs.want_rows == 1 and not xs.rb
    # the compiler's sizes and offsets
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    src = tmp_path / "rb_layout.cpp"
    lines = ['#include <cstddef>', '#include <cstdio>', '#include "spamtree_fit.h"', "int main() {"]
    want = {}
    for cname, cls in (("st_rb_out", _lib.StRbOut), ("stm_rb_exceed", _lib.StmRbExceed), ("stm_excursions", _lib.StmExcursions)):
        lines.append(f'  std::printf("{cname} %zu\\n", sizeof({cname}));')
        want[cname] = C.sizeof(cls)
        for f in cls._fields_:
            lines.append(f'  std::printf("{cname}.{f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
            want[f"{cname}.{f[0]}"] = getattr(cls, f[0]).offset
    src.write_text("\n".join(lines + ["  return 0;", "}"]) + "\n")
    exe = str(tmp_path / "rb_layout")
    subprocess.run([hipcc, "--offload-host-only", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, timeout=600)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, check=True).stdout
    assert {k: int(v) for k, v in (line.split() for line in out.splitlines())} == want


# ---- 3. the driver's refusals ------------------------------------------------------------------------------------------------------
def test_driver_refuses_before_the_first_factorisation():
    """stm_mcmc_fit returns the refusals of rb before it creates the chain: no device is touched, so they are checked here.  Only the
    problem's q is read of the problem; the point set's arrays are not read."""
    from spamtree_amd import _lib
    from tests.test_fit_request_cpu import N_FUN, N_NEW, Request
    lib = _lib.load()

    def run(points=True, X=True, fun=False, n_thr=1, thr=(0.0,), side=None, thr_fun=None, w=True, yhat=False, fun_w=False, keep=8):
        r = Request()
        r.fit.run.mcmc_keep = keep
        if points:
            r.points(X=X)
        if fun:
            r.functionals()
        held = [np.array(thr, dtype=np.float64), None if side is None else np.array(side, dtype=np.int32),
                None if thr_fun is None else np.array(thr_fun, dtype=np.float64), C.c_int64()]
        out = lambda want: _lib.StRbOut(r.dbl, r.dbl) if want else _lib.StRbOut()   # noqa: E731
        rb = _lib.StmRbExceed(n_thr, held[0].ctypes.data_as(_lib.c_dp), None if side is None else held[1].ctypes.data_as(C.POINTER(C.c_int32)),
                              None if thr_fun is None else held[2].ctypes.data_as(_lib.c_dp), out(w), out(yhat), out(fun_w), C.pointer(held[3]))
        xs = r.part("exc", _lib.StmExcursions())
        xs.rb = C.pointer(rb)
        rc = lib.stm_mcmc_fit(C.byref(r.fit))
        assert not r.buf.any()                                           # a refused request writes nothing
        return rc

    nine = [0.0] * 9
    for kw in (dict(points=False),                                       # rb without a point set
               dict(X=False, yhat=True),                                 # a new_yhat output without X_new
               dict(fun=False, fun_w=True, thr_fun=[0.0] * N_FUN),       # fun_w without fun
               dict(fun=True, fun_w=True),                               # fun_w without thr_fun
               dict(fun=False, thr_fun=[0.0] * N_FUN),                   # thr_fun needs functionals
               dict(n_thr=9, thr=nine), dict(n_thr=-1),                  # n_thr outside 1 .. 8
               dict(thr=[np.nan]), dict(thr=[np.inf]), dict(n_thr=2, thr=[0.0, -np.inf]),
               dict(side=[0]), dict(n_thr=2, thr=[0.0, 1.0], side=[1, 2]),
               dict(fun=True, fun_w=True, thr_fun=[0.0, np.nan][:N_FUN]),
               dict(keep=0, thr=[np.nan])):                              # the stores' minimum of draws does not come first: the spec does
        assert run(**kw) == USAGE, kw
    assert N_NEW == 3


# ---- 4. the front doors ----------------------------------------------------------------------------------------------------------------
def test_fit_and_predict_refuse_before_any_device_call():
    from spamtree_amd import exceed as rb
    from spamtree_amd import fit, predict
    from tests.util import make_problem
    pb = make_problem(side=8, q=2, seed=1)
    k = pb["theta"].size
    real = (pb["y"], pb["X"], pb["Z"], pb["coords"], pb["mv_id"], pb["blocking"], pb["gix_block"], pb["res_is_ref"], pb["parents"],
            pb["children"], bool(pb["limited_tree"]), pb["block_names"], pb["block_groups"], pb["indexing"], pb["bounds"],
            np.zeros(pb["n"]), pb["theta"], np.zeros(pb["p"]), 0.1, 0.02 * np.eye(k))
    pts = dict(coords=np.zeros((4, 2)), mv=np.array([1, 2, 1, 2]), anchor=np.zeros(4, dtype=np.int64), X=np.zeros((4, pb["p"])))
    fun = [(np.arange(2), np.ones(2) / 2)]
    bad = (dict(), dict(thresholds=None), dict(thresholds=[0.0] * 9), dict(thresholds=[np.nan]), dict(thresholds=[np.inf]),
           dict(thresholds=0.0, side=0), dict(thresholds=[0.0, 1.0], side=[1, -1, 1]), dict(thresholds=[[0.0, 1.0, 2.0]]),
           dict(thresholds=0.0, level=0.1), dict(thresholds=0.0, thresholds_fun=0.0), 0.5)
    for spec in bad:
        with pytest.raises(ValueError):
            fit.spamtree_mv_mcmc(*real, new_points=dict(pts, exceed=spec), mcmc_keep=5, mcmc_burn=1, main_verbose=False)
    for spec in (dict(thresholds=0.0, thresholds_fun=[[0.0, 1.0]]), dict(thresholds=[0.0, 1.0], thresholds_fun=0.0)):
        with pytest.raises(ValueError):                  # one value per functional; one entry per threshold
            fit.spamtree_mv_mcmc(*real, new_points=dict(pts, functionals=fun, exceed=spec), mcmc_keep=5, mcmc_burn=1, main_verbose=False)
    draws = dict(w_mcmc=[np.zeros(pb["n"])] * 3, beta_mcmc=np.zeros((pb["p"], 3, 2)), tausq_mcmc=np.ones((2, 3)), theta_mcmc=np.ones((k, 3)))
    for spec in bad:
        with pytest.raises(ValueError):
            predict.fit_predict(pb, pts["coords"], pts["mv"], pts["X"], exceed=spec, mcmc_keep=5)
        with pytest.raises(ValueError):
            predict.predict_new(pb, draws, pts["coords"], pts["mv"], pts["X"], exceed=spec)
    for kw in (dict(z=np.zeros((4, 3))), dict(mode=1)):  # the replay goes through st_points_accumulate: the device's draw only
        with pytest.raises(ValueError):
            predict.predict_new(pb, draws, pts["coords"], pts["mv"], pts["X"], exceed=dict(thresholds=0.0), **kw)
    thr, side, thr_fun = rb.check_spec(dict(thresholds=[0.0, [1.0, 2.0]], side=[1, -1], thresholds_fun=[[0.5], -0.5]), 2, 1)
    assert thr.tolist() == [[0.0, 0.0], [1.0, 2.0]] and side.tolist() == [1, -1] and side.dtype == np.int32
    assert thr_fun.tolist() == [[0.5], [-0.5]]
    with pytest.raises(ValueError):
        rb.Stream().finish()
