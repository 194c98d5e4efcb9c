"""GPU: every positional whole-fit entry point against stm_mcmc_fit (include/spamtree_fit.h), byte for byte.

For each of the eleven positional entry points the fullest request it can express -- on the 64-row problem with NA rows: nine new
points in joint groups of 3, 2 and 4, two functionals, held-out values at the points and at the NA rows, one quantile, every
output of the diagnostics, excursions (thresholds and band) and rank diagnostics of rows, points and functionals, two chains -- is
run once through that entry point and once through stm_mcmc_fit, each into buffers of its own that start from the same pattern
(NaN, -7 in the integers).  The return codes are 0 and every output buffer and count is the same bytes; only the wall-clock
outputs (mcmc_time, chain_time) are left out."""
import ctypes as C

import numpy as np
import pytest

from tests.fit_request import LEGACY, positional

pytestmark = pytest.mark.gpu

KEEP, BURN = 4, 2     # ST_DIAG_MIN_DRAWS saved draws after two of burn-in
SEEDS = (23, 101)
FILL = -7

_SHARED = {}


def shared():
    """The problem, its st_problem, the point sets (plain and joint anchors) and the held-out values, made once."""
    if not _SHARED:
        from spamtree_amd import fit
        from spamtree_amd.model import functionals_csr
        from spamtree_amd.predict import locate
        from tests.test_gpu_diagnostics import fit_args
        from tests.test_gpu_multichain import joint_points
        from tests.util import make_problem
        pb = make_problem(side=8, q=1, seed=71, p=2, missing=0.2)
        a = fit_args(pb)
        spb, hold, n, p, q = fit._problem(a[0], a[1], a[3], a[4], a[7], a[8], a[9], a[11], a[12], a[13])
        jp = joint_points(pb)
        joint = fit._points_inputs(jp, p, q, ())
        plain = fit._points_inputs(dict(jp, joint=None, anchor=locate(pb["topo"], jp["coords"], jp["mv"], device=0)), p, q, ())
        rng = np.random.default_rng(5)
        _SHARED.update(pb=pb, args=a, spb=spb, hold=hold, n=n, p=p, q=q, joint=joint, plain=plain,
                       fun=functionals_csr([([0, 1, 2], [1.0, 2.0, -3.0]), (list(range(9)), [1.0 / 9] * 9)], 9),
                       y_new=rng.standard_normal(9), y_holdout=np.where(np.isnan(pb["y"]), 0.25, np.nan),
                       theta0=np.ascontiguousarray(np.stack([pb["theta"], 0.8 * pb["theta"]])))
        assert np.isnan(pb["y"]).any() and not np.isnan(pb["y"]).all()
    return _SHARED


class Built:
    """One request with fresh output buffers.  ``out``: every output by name; ``held``: what else the request points at."""

    def __init__(self, parts, joint):
        from spamtree_amd import _lib
        from spamtree_amd.excursions import expand_thresholds
        from spamtree_amd.model import (_dp, _f64, _ip, excursion_buffers, excursion_spec, rank_buffers, rank_spec,
                                        series_diag_buffers)
        s = shared()
        a, n, p, q, k = s["args"], s["n"], s["p"], s["q"], s["pb"]["theta"].size
        M = 2 if "ch" in parts else 1
        K = M * KEEP
        self.out, self.held = {}, []
        held = self.held

        def new(name, shape, dtype=np.float64):
            self.out[name] = b = np.full(shape, np.nan if dtype == np.float64 else FILL, dtype=dtype, order="F")
            return b

        def take(prefix, bufs):          # the buffers a model helper made, refilled with the pattern
            for key, b in bufs.items():
                b.fill(np.nan if b.dtype == np.float64 else FILL)
                self.out[f"{prefix}.{key}"] = b

        def part(name, struct):
            held.append(struct)
            setattr(self.req, name, C.pointer(struct))
            return struct
        self.req = _lib.StmFit()
        held += [np.asfortranarray(np.asarray(a[14], dtype=np.float64)), _f64(s["pb"]["theta"]), _f64(a[17]),
                 np.asfortranarray(np.asarray(a[19], dtype=np.float64)), _lib.StOptions(0, 1, 0, 1, 0, 0), _lib.StmFlags(1, 1, 1, 1, 1, 1),
                 C.c_double()]
        bounds, theta, beta, sd, opt, fl, t = held[-7:]
        self.req.run = _lib.StmRun(C.pointer(s["spb"]), C.pointer(opt), _dp(bounds), _dp(theta), k, _dp(beta), float(a[18]), _dp(sd), KEEP, BURN, 1,
                                   SEEDS[0], C.pointer(fl), _dp(new("w_mcmc", (n, K))), _dp(new("yhat_mcmc", (n, K))),
                                   _dp(new("beta_mcmc", (p, K, q))), _dp(new("tausq_mcmc", (q, K))), _dp(new("theta_mcmc", (k, K))),
                                   _dp(new("paramsd", (k, k))), C.pointer(t))
        if "pts" in parts:
            pc, pmv, pan, pX, _, labels, _, _, _ = s["joint"] if joint else s["plain"]
            n_new = pc.shape[0]
            qs = np.array([0.5])
            held.append(qs)
            per_draw = [_dp(new(f"new_{key}", (n_new, K))) for key in ("w", "cond_mean", "cond_var", "yhat")]
            summ = [_dp(new(f"new_{key}", n_new)) for key in ("mean", "var", "w_mean", "yhat_mean", "w_q", "yhat_q")]
            cov_len = int(sum(g * g for g in np.unique(labels, return_counts=True)[1])) if joint else 0
            part("pts", _lib.StmNewPoints(n_new, _dp(pc), _ip(pmv), _ip(pan), _dp(pX), _ip(labels) if joint else None, KEEP, _dp(qs), 1,
                                          *per_draw, *summ, new("new_route", 1, np.int32).ctypes.data_as(C.POINTER(C.c_int32)),
                                          _dp(new("new_cond_cov", (cov_len, K))) if joint else None, _dp(new("new_cov", cov_len)) if joint else None))
        n_fun = 2
        if "fun" in parts:
            ptr, idx, wt = s["fun"]
            part("fun", _lib.StmFunctionals(n_fun, _ip(ptr), _ip(idx), _dp(wt), *[_dp(new(f"fun_{key}", (n_fun, K))) for key in ("w", "cond_mean", "cond_var", "yhat")],
                                            *[_dp(new(f"fun_{key}", n_fun)) for key in ("mean", "var", "w_mean", "yhat_mean", "w_q", "yhat_q")]))
        if "scores" in parts:
            held.append(s["y_new"])
            part("scores", _lib.StmScores(_dp(s["y_new"]), _dp(new("lpd", 9)), _dp(new("pit", 9)), _dp(new("crps", 9)), _dp(new("lpd_joint", 3)),
                                          _ip(new("n_scored", 1, np.int64)), _ip(new("n_degenerate", 1, np.int64))))
        sizes = dict(rows=n, new=9, fun=n_fun)
        groups = dict(rows=q, new=q, fun=1)   # the domains of a store: the outcomes, or one for the functionals
        values = dict(rows=q, new=q, fun=n_fun)   # the values per threshold
        if "diag" in parts:
            ds = part("diag", _lib.StmDiagnostics(0, 1))
            for where, m in sizes.items():
                for which in ("w", "yhat"):
                    bufs, o = series_diag_buffers(m)
                    take(f"diag.{where}_{which}", bufs)
                    setattr(ds, f"{where}_{which}", o)
        if "exc" in parts:
            xs = part("exc", _lib.StmExcursions(1))
            for where, m in sizes.items():
                spec, keep = excursion_spec(*expand_thresholds((-0.2, 0.3), values[where], (1, -1)), None, True)   # two thresholds and the band
                held.append(keep)
                setattr(xs, f"{where}_spec", spec)
                for which in ("w", "yhat"):
                    bufs, o = excursion_buffers(m, 2, groups[where], K, True)
                    take(f"exc.{where}_{which}", bufs)
                    setattr(xs, f"{where}_{which}", o)
        if "rk" in parts:
            rs = part("rk", _lib.StmRankDiagnostics(1))
            for where, m in sizes.items():
                spec, keep, n_prob, n_thr = rank_spec((0.1, 0.5), (0.0, 0.4), (1, -1), 0, values[where])
                held.append(keep)
                setattr(rs, f"{where}_spec", spec)
                for which in ("w", "yhat"):
                    bufs, o = rank_buffers(m, n_prob, n_thr)
                    take(f"rk.{where}_{which}", bufs)
                    setattr(rs, f"{where}_{which}", o)
        if "ch" in parts:
            seeds = np.array(SEEDS, dtype=np.uint64)
            chain_time = np.zeros(M)
            held += [seeds, chain_time]
            part("ch", _lib.StmChains(M, seeds.ctypes.data_as(C.POINTER(C.c_uint64)), _dp(s["theta0"]), _dp(new("ch.paramsd", (k, k, M))),
                                      _dp(chain_time)))
        if "criteria" in parts:
            held.append(s["y_holdout"])
            part("criteria", _lib.StmCriteria(_dp(s["y_holdout"]), 1, *[_dp(new(f"crit.{key}", n)) for key in ("lppd", "p_waic", "mean_ll", "mu_mean", "pit", "crps")],
                                              _dp(new("crit.obs", (len(_lib.ST_ROWS_OBS), q))), _dp(new("crit.held", (len(_lib.ST_ROWS_HELD), q))),
                                              _ip(new("crit.n_obs", q, np.int64)), _ip(new("crit.n_held", q, np.int64)),
                                              _ip(new("crit.n_accumulated", 1, np.int64))))
        if "loo" in parts:
            part("loo", _lib.StmLoo(*[_dp(new(f"loo.{key}", n)) for key in ("elpd_loo", "pit_loo", "mu_loo", "weight_ess")],
                                    _dp(new("loo.tot", (len(_lib.ST_ROWS_LOO), q))), _ip(new("loo.n_obs", q, np.int64)),
                                    _ip(new("loo.n_accumulated", 1, np.int64)), _ip(new("loo.n_skipped", 1, np.int64))))


@pytest.mark.parametrize("symbol", list(LEGACY))
def test_the_positional_entry_point_and_the_request_write_the_same_bytes(symbol):
    from spamtree_amd import _lib
    lib = _lib.load()
    parts, joint = LEGACY[symbol], symbol != "stm_mcmc_points"
    old, new = Built(parts, joint), Built(parts, joint)
    rc_old = getattr(lib, symbol)(*positional(symbol, old.req))
    rc_new = lib.stm_mcmc_fit(C.byref(new.req))
    assert rc_old == rc_new == 0, (rc_old, rc_new, lib.stm_mcmc_chains_last_error())
    assert sorted(old.out) == sorted(new.out) and len(old.out) >= 6
    for name, b in old.out.items():
        assert b.tobytes() == new.out[name].tobytes(), (symbol, name)
    # the requests wrote: no buffer of the run is still the pattern, and every part left at least one of its own changed
    pattern = {name: np.full(b.shape, np.nan if b.dtype == np.float64 else FILL, dtype=b.dtype).tobytes() for name, b in new.out.items()}
    changed = {name for name, b in new.out.items() if b.tobytes() != pattern[name]}
    assert {"w_mcmc", "yhat_mcmc", "beta_mcmc", "tausq_mcmc", "theta_mcmc", "paramsd"} <= changed
    prefix = dict(pts="new_", fun="fun_", scores="lpd", diag="diag.", exc="exc.", rk="rk.", ch="ch.", criteria="crit.", loo="loo.")
    for p in parts:
        assert any(name.startswith(prefix[p]) for name in changed), (symbol, p)
