"""CPU-only: the whole-fit request (include/spamtree_fit.h: stm_run, stm_new_points, stm_fit, stm_mcmc_fit).

Layout: the field names the header declares are the ctypes mirror's, in order, and tests/fit_request_check.cpp -- a host program
that includes the header alone -- prints the sizes and offsets the C++ compiler gives them, which are ctypes' too.
Signatures: the argument list of every positional entry point is the concatenation of the struct fields it is derived from.
Refusals: everything the header says is refused before a chain exists touches no device, so it is checked here.  Each case is sent
once through the narrowest positional entry point that can express it and once through stm_mcmc_fit; the return code is the one
the header documents and both calls leave the same return code and the same stm_mcmc_chains_last_error()."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests.fit_request import LEGACY, POINTS_FAMILY, positional

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
USAGE, UNSUPPORTED = -1, -4   # include/spamtree_hip.h: ST_ERR_USAGE, ST_ERR_UNSUPPORTED


def structs():
    from spamtree_amd import _lib
    return dict(stm_run=_lib.StmRun, stm_new_points=_lib.StmNewPoints, stm_fit=_lib.StmFit)


# ---- layout ------------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_same_fields_in_the_same_order():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spamtree_fit.h")).read(), flags=re.S)
    for name, cls in structs().items():
        body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", hdr, flags=re.S).group(1)
        assert re.findall(r"[\*\s](\w+)\s*[,;]", body) == [f[0] for f in cls._fields_], name
    assert re.search(r"\bint\s+stm_mcmc_fit\s*\(\s*const\s+stm_fit\s*\*\s*\w+\s*\)\s*;", hdr)


def test_the_compiler_and_ctypes_agree_on_sizes_and_offsets(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    src = os.path.join(ROOT, "tests", "fit_request_check.cpp")
    includes = re.findall(r'#include\s+"([^"]+)"', open(src).read())
    assert includes == ["spamtree_fit.h"]
    exe = str(tmp_path / "fit_request_check")
    subprocess.run([hipcc, "--offload-host-only", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True, timeout=600)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, check=True).stdout
    got = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
    want = {}
    for name, cls in structs().items():
        want[name] = C.sizeof(cls)
        want.update({f"{name}.{f[0]}": getattr(cls, f[0]).offset for f in cls._fields_})
    assert got == want
    assert len(want) == 3 + 20 + 22 + 10


# ---- signatures --------------------------------------------------------------------------------------------------------------------
def test_positional_signatures_are_the_struct_fields_concatenated():
    from spamtree_amd import _lib
    run = [t for _, t in _lib.StmRun._fields_]
    pts = dict(_lib.StmNewPoints._fields_)
    part = dict(_lib.StmFit._fields_)
    whole_fit = {s for s in _lib.SIGNATURES if s.startswith("stm_mcmc_")} | {"spamtree_mv_mcmc_c"}
    assert set(LEGACY) == whole_fit - {"stm_mcmc_fit", "stm_mcmc_chains_last_error"} and len(LEGACY) == 11
    for symbol, parts in LEGACY.items():
        res, args = _lib.SIGNATURES[symbol]
        want = list(run)
        if "pts" in parts:
            want += [t for name, t in pts.items() if not (symbol == "stm_mcmc_points" and name in _lib.JOINT_ONLY)]
        want += [part[name] for name in parts if name != "pts"]
        assert res is C.c_int and args == want, symbol
    assert len(_lib.SIGNATURES["spamtree_mv_mcmc_c"][1]) == 20
    assert len(_lib.SIGNATURES["stm_mcmc_points"][1]) == 39 and len(_lib.SIGNATURES["stm_mcmc_points_joint"][1]) == 42
    assert len(_lib.SIGNATURES["stm_mcmc_chains"][1]) == 42 + 6
    assert _lib.SIGNATURES["stm_mcmc_fit"] == (C.c_int, [C.POINTER(_lib.StmFit)])


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
N_NEW, N_FUN = 3, 2


class Request:
    """An stm_fit over the small problem and everything it points at.  ``dbl`` is a buffer any output pointer may name: a refused
    request writes nothing."""

    def __init__(self):
        from spamtree_amd import _lib
        from tests.util import make_problem, problem_arrays, st_problem_struct
        self.arrays = problem_arrays(make_problem(side=8, q=1, seed=1))
        self.pb = st_problem_struct(self.arrays)
        self.opt = _lib.StOptions(0, 1, 0, 1, 0, 0)
        self.flags = _lib.StmFlags(1, 1, 1, 1, 1, 1)
        self.theta = np.ones(4)
        self.buf = np.zeros(64)
        self.dbl = self.buf.ctypes.data_as(_lib.c_dp)
        self.fit = _lib.StmFit()
        self.fit.run = _lib.StmRun(C.pointer(self.pb), C.pointer(self.opt), None, self.dbl_of(self.theta), 4, None, 0.1, None, 8, 1, 1, 1,
                                   C.pointer(self.flags))
        self.held = []

    @staticmethod
    def dbl_of(a):
        from spamtree_amd import _lib
        return a.ctypes.data_as(_lib.c_dp)

    def part(self, name, struct):
        self.held.append(struct)
        setattr(self.fit, name, C.pointer(struct))
        return struct

    def points(self, X=True, **fields):
        """A point set of N_NEW points (nothing reads the coordinates before the chain exists); ``fields`` on top."""
        from spamtree_amd import _lib
        ints = np.zeros(N_NEW, dtype=np.int64)
        self.held.append(ints)
        ip = ints.ctypes.data_as(_lib.c_ip)
        p = self.part("pts", _lib.StmNewPoints(N_NEW, self.dbl, ip, ip, self.dbl if X else None))
        for key, v in fields.items():
            setattr(p, key, v)
        return p

    def functionals(self, **fields):
        from spamtree_amd import _lib
        ints = np.zeros(N_FUN + 1, dtype=np.int64)
        self.held.append(ints)
        ip = ints.ctypes.data_as(_lib.c_ip)
        f = self.part("fun", _lib.StmFunctionals(N_FUN, ip, ip, self.dbl))
        for key, v in fields.items():
            setattr(f, key, v)
        return f

    def chains(self, M, seeds=True):
        from spamtree_amd import _lib
        s = np.arange(1, 17, dtype=np.uint64)
        self.held.append(s)
        return self.part("ch", _lib.StmChains(M, s.ctypes.data_as(C.POINTER(C.c_uint64)) if seeds else None))


def series(r):
    from spamtree_amd import _lib
    return _lib.StSeriesDiag(r.dbl)


def exc_out(r):
    from spamtree_amd import _lib
    return _lib.StExcursionOut(None, r.dbl)          # prob: a threshold output


def rank_out(r):
    from spamtree_amd import _lib
    return _lib.StRankOut(r.dbl)


def summary(kind, r, want_rows=1, **members):
    """One of diag / exc / rk with valid specs and the members named in ``members`` asking for an output."""
    from spamtree_amd import _lib
    if kind == "diag":
        s = r.part("diag", _lib.StmDiagnostics(0, want_rows))
        out = series
    elif kind == "exc":
        s = r.part("exc", _lib.StmExcursions(want_rows))
        out = exc_out
        thr = np.zeros(8)
        r.held.append(thr)
        for spec in (s.rows_spec, s.new_spec, s.fun_spec):
            spec.n_thr, spec.thr = 1, r.dbl_of(thr)
    else:
        s = r.part("rk", _lib.StmRankDiagnostics(want_rows))
        out = rank_out
    for name in members:
        setattr(s, name, out(r))
    return s


SUMMARY_SYMBOL = dict(diag="stm_mcmc_diagnosed", exc="stm_mcmc_excursions", rk="stm_mcmc_ranked")


def summary_cases():
    """For each of diag / exc / rk, what the header lists for all three, in its order, and one refusal of the part's own spec."""
    cases = []
    for kind, symbol in SUMMARY_SYMBOL.items():
        def rows_without_want_rows(r, kind=kind):
            summary(kind, r, want_rows=0, rows_w=1)

        def points_on_a_plain_chain(r, kind=kind):
            summary(kind, r, new_w=1)

        def functionals_without_fun(r, kind=kind):
            r.points()
            summary(kind, r, fun_w=1)

        def yhat_without_X(r, kind=kind):
            r.points(X=False)
            summary(kind, r, new_yhat=1)

        def too_few_draws(r, kind=kind):
            s = summary(kind, r, rows_w=1)
            if kind == "exc":                        # one draw is enough for a threshold, not for a band
                s.rows_spec.want_band = 1
                r.fit.run.mcmc_keep = 1
            else:
                r.fit.run.mcmc_keep = 3              # ST_DIAG_MIN_DRAWS = 4

        def too_many_draws(r, kind=kind):
            summary(kind, r, rows_w=1)
            r.fit.run.mcmc_keep = 16385

        def bad_spec(r, kind=kind):
            s = summary(kind, r, rows_w=1)
            if kind == "diag":
                s.max_lag = -1
            elif kind == "exc":
                s.rows_spec.n_thr = 9                # ST_EXC_MAX_THRESHOLDS = 8
            else:
                s.rows_spec.n_prob = 9               # ST_RANK_MAX_PROBS = 8
        for build, rc in ((rows_without_want_rows, USAGE), (points_on_a_plain_chain, USAGE), (functionals_without_fun, USAGE),
                          (yhat_without_X, USAGE), (too_few_draws, USAGE), (too_many_draws, UNSUPPORTED), (bad_spec, USAGE)):
            cases.append(pytest.param(symbol, build, rc, "stored draws, at most 16384" if rc == UNSUPPORTED else "", id=f"{kind}-{build.__name__}"))
    return cases


def chains_cases():
    def n_chains_out_of_range(r):
        r.chains(17)

    def seeds_null(r):
        r.chains(2, seeds=False)

    def no_saved_draw(r):
        r.chains(2)
        r.fit.run.mcmc_keep = 0

    def theta_null(r):
        r.chains(2)
        r.fit.run.theta = None

    def several_gpus(r):
        r.chains(2)
        r.opt.world = 2

    def too_many_stored_draws(r):
        r.chains(2)
        summary("diag", r, rows_w=1)
        r.fit.run.mcmc_keep = 8193
    return [pytest.param("stm_mcmc_chains", build, rc, text, id=f"chains-{build.__name__}") for build, rc, text in (
        (n_chains_out_of_range, USAGE, "n_chains = 17 must lie in 1 .. 16"), (seeds_null, USAGE, "seeds is NULL"),
        (no_saved_draw, USAGE, "mcmc_keep = 0"), (theta_null, USAGE, "theta is NULL"), (several_gpus, UNSUPPORTED, "world = 2"),
        (too_many_stored_draws, UNSUPPORTED, "2 chains x mcmc_keep = 8193 are 16386 stored draws, at most 16384"))]


def points_cases():
    from spamtree_amd import _lib

    def quantile_outside_0_1(r):
        q = np.array([1.5])
        r.held.append(q)
        r.points(keep_draws=1, quantiles=r.dbl_of(q), n_quantiles=1)

    def quantiles_without_keep_draws(r):
        r.points(keep_draws=0, quantiles=r.dbl, n_quantiles=1)

    def cond_cov_without_labels(r):
        r.points(new_cond_cov=r.dbl)

    def functional_yhat_without_X(r):
        r.points(X=False)
        r.functionals(fun_yhat_mean=r.dbl)

    def scores_without_X(r):
        r.points(X=False)
        r.part("scores", _lib.StmScores(r.dbl, r.dbl))

    def lpd_joint_without_labels(r):
        r.points()
        r.part("scores", _lib.StmScores(r.dbl, None, None, None, r.dbl))

    def crps_without_keep_draws(r):
        r.points(keep_draws=0)
        r.part("scores", _lib.StmScores(r.dbl, None, None, r.dbl))

    def run_without_theta(r):                        # stm_create's own check of its arguments, before st_create
        r.fit.run.theta = None
    return [pytest.param(symbol, build, USAGE, "", id=f"{symbol[9:] or symbol}-{build.__name__}") for symbol, build in (
        ("stm_mcmc_points", quantile_outside_0_1), ("stm_mcmc_points", quantiles_without_keep_draws),
        ("stm_mcmc_points_joint", cond_cov_without_labels), ("stm_mcmc_functionals", functional_yhat_without_X),
        ("stm_mcmc_scored", scores_without_X), ("stm_mcmc_scored", lpd_joint_without_labels), ("stm_mcmc_scored", crps_without_keep_draws),
        ("spamtree_mv_mcmc_c", run_without_theta))]


def criteria_cases():
    from spamtree_amd import _lib

    def hold(r):
        h = np.full(int(r.arrays["n_all"]), np.nan)
        r.held.append(h)
        return r.dbl_of(h)

    def crps_without_want_crps(r):
        r.part("criteria", _lib.StmCriteria(hold(r), 0, None, None, None, None, None, r.dbl))

    def crps_of_too_many_draws(r):
        r.part("criteria", _lib.StmCriteria(hold(r), 1))
        r.fit.run.mcmc_keep = 16385

    def holdout_without_sample_predicts(r):
        r.part("criteria", _lib.StmCriteria(hold(r), 0))
        r.flags.sample_predicts = 0

    def loo_beside_refused_criteria(r):
        crps_without_want_crps(r)
        r.part("loo", _lib.StmLoo(r.dbl))
    return [pytest.param(symbol, build, rc, "", id=f"{symbol[9:]}-{build.__name__}") for symbol, build, rc in (
        ("stm_mcmc_criteria", crps_without_want_crps, USAGE), ("stm_mcmc_criteria", crps_of_too_many_draws, UNSUPPORTED),
        ("stm_mcmc_criteria", holdout_without_sample_predicts, USAGE), ("stm_mcmc_loo", loo_beside_refused_criteria, USAGE))]


CASES = chains_cases() + summary_cases() + points_cases() + criteria_cases()


def test_the_table_has_a_row_for_every_positional_entry_point():
    assert {c.values[0] for c in CASES} == set(LEGACY)


@pytest.mark.parametrize("symbol, build, rc, text", CASES)
def test_refusals_are_the_same_through_either_door(symbol, build, rc, text):
    from spamtree_amd import _lib
    lib = _lib.load()
    seen = []
    for door in ("positional", "request"):
        r = Request()
        build(r)
        got = getattr(lib, symbol)(*positional(symbol, r.fit)) if door == "positional" else lib.stm_mcmc_fit(C.byref(r.fit))
        seen.append((got, lib.stm_mcmc_chains_last_error().decode()))
        assert not r.buf.any()                       # nothing was written
    assert seen[0] == seen[1]
    assert seen[0][0] == rc and text in seen[0][1] and (text or seen[0][1] == "")


@pytest.mark.parametrize("rows_part", ["criteria", "loo"])
@pytest.mark.parametrize("part", POINTS_FAMILY)
def test_parts_of_both_families_are_refused(part, rows_part):
    """New with the request: no positional entry point can say it."""
    from spamtree_amd import _lib
    lib = _lib.load()
    r = Request()
    r.part(rows_part, _lib.StmCriteria() if rows_part == "criteria" else _lib.StmLoo())
    r.part(part, dict(_lib.StmFit._fields_)[part]._type_())
    assert lib.stm_mcmc_fit(C.byref(r.fit)) == USAGE
    assert lib.stm_mcmc_chains_last_error().decode().startswith("stm_mcmc_fit: criteria and loo do not go with")
    # every call clears the text first: a criteria call too, which never sets one
    r = Request()
    r.fit.run.theta = None
    assert lib.stm_mcmc_criteria(*positional("stm_mcmc_criteria", r.fit)) == USAGE and lib.stm_mcmc_chains_last_error() == b""


def test_a_null_request_is_a_usage_error():
    from spamtree_amd import _lib
    assert _lib.load().stm_mcmc_fit(None) == USAGE
