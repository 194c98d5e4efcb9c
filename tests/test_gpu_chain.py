"""GPU: whole chains.  The C++ host driver (spamtree_amd/csrc/spamtree_fit.cpp through spamtree_amd/fit.py) and the
Python host driver (spamtree_amd/mcmc.py) against the oracle's restatement of spamtree_mv_mcmc with the same Philox
streams: theta / beta / tausq traces, saved w and yhat."""
import numpy as np
import pytest

from tests.util import make_problem

pytestmark = pytest.mark.gpu


def args_of(pb, k):
    return (pb["y"], pb["X"], pb["Z"], pb["coords"], pb["mv_id"], pb["blocking"], pb["gix_block"], pb["res_is_ref"],
            pb["parents"], pb["children"], pb.get("limited_tree", False), pb["block_names"], pb["block_groups"], pb["indexing"], pb["bounds"],
            np.zeros((pb["n"], 1)), pb["theta"], np.zeros(pb["p"]), 0.1, 0.01 * np.eye(k))


def relerr(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1e-300, np.abs(np.asarray(b)).max()))


@pytest.mark.parametrize("case", [dict(side=25, q=1, seed=11, missing=0.1), dict(side=12, q=2, seed=12),
                                  dict(side=25, q=1, seed=13, missing=0.1, limited_tree=True),
                                  dict(side=10, q=4, seed=14, missing=0.1, signed_sd=2e-4),
                                  dict(side=10, q=6, seed=15, missing=0.1, signed_sd=2e-4)])
def test_cpp_and_python_drivers_match_oracle_chain(case):
    """q = 4 and 6 (a 21- and a 36-entry theta, 100- and 136-row root blocks, NA rows): `signed_sd` is the initial proposal
    scale of ai1[1:], whose bounds are (-1e3, 1e3): at the 0.01 of the other entries a step moves them by about 5, no
    multivariate proposal is ever accepted (logaccept about -500), and the chain would put no theta through the swap.  With
    it both chains accept several proposals during the burn-in (asserted).  That matters for the NA rows as well: the oracle
    restates the reference's predict(need_update), which reads prediction caches that nothing has filled until the first
    accepted theta (H = 0: the rows are drawn from their marginals), while st_predict rebuilds H on every call; a chain with
    NA rows that accepts nothing before its first saved iteration differs there from its first saved beta on (measured at
    q = 3 and 4, side 10, missing 0.1, the 0.01 scale: beta 2e-2 to 1e-1, w of the NA rows O(1))."""
    from oracle import spamtree_oracle as so
    from spamtree_amd import fit, mcmc
    case = dict(case)
    signed_sd = case.pop("signed_sd", None)
    pb = make_problem(**case)
    k = pb["theta"].size

    def args():
        a = list(args_of(pb, k))
        if signed_sd is not None:
            sd = np.full(k, 0.01)
            sd[1:pb["q"]] = signed_sd
            a[19] = np.diag(sd)
        return tuple(a)

    kw = dict(mcmc_keep=4, mcmc_burn=58, mcmc_thin=2, adapting=True, seed=99, main_verbose=False)   # crosses g0 = 50
    ref = so.spamtree_mv_mcmc(*args(), **kw)
    if signed_sd is not None:
        assert not np.array_equal(ref["theta_mcmc"][:, 0], pb["theta"])      # accepted proposals before the first saved draw
    for drv in (fit.spamtree_mv_mcmc, mcmc.spamtree_mv_mcmc):
        got = drv(*args(), **kw)
        assert "None" not in got
        assert relerr(got["theta_mcmc"], ref["theta_mcmc"]) < 1e-8
        assert relerr(got["tausq_mcmc"], ref["tausq_mcmc"]) < 1e-8
        assert relerr(got["beta_mcmc"], ref["beta_mcmc"]) < 1e-8
        assert relerr(got["paramsd"], ref["paramsd"]) < 1e-7
        for i in range(4):
            assert relerr(np.asarray(got["w_mcmc"][i]).reshape(-1), ref["w_mcmc"][i]) < 1e-8
            assert relerr(np.asarray(got["yhat_mcmc"][i]).reshape(-1), ref["yhat_mcmc"][i]) < 1e-8


def test_cpp_chain_steps_and_reports_state():
    from spamtree_amd import fit
    pb = make_problem(side=25, q=1, seed=3)
    ch = fit.Chain(pb["y"], pb["X"], pb["Z"], pb["coords"], pb["mv_id"], pb["blocking"], pb["gix_block"], pb["res_is_ref"],
                   pb["parents"], pb["children"], pb.get("limited_tree", False), pb["block_names"], pb["block_groups"], pb["indexing"],
                   pb["bounds"], pb["theta"], np.zeros(pb["p"]), 0.1, 0.01 * np.eye(4), seed=5)
    ch.step(20)
    st = ch.state()
    assert st["iteration"] == 20 and np.all(np.isfinite(st["theta"])) and np.all(st["tausq_inv"] > 0)
    assert np.isfinite(st["loglik"]) and np.all(np.isfinite(ch.get_w()))
    ch.close()


def test_native_rccl_protocol_single_rank(monkeypatch):
    """The library's own RCCL path (st_comm_init: pack -> ncclAllReduce on the launch stream -> deterministic finish) with a
    one-rank communicator gives the chain of the plain single-GPU path bit for bit.  (More than one rank per GPU is not
    possible with RCCL; the multi-rank protocol itself is covered through gloo in tests/test_gpu_sharded.py.)"""
    from spamtree_amd import fit
    pb = make_problem(side=40, q=1, seed=3, missing=0.05)
    states = []
    monkeypatch.setenv("SPAMTREE_QUAD_MIN", "1")        # quad levels below, so that there are top levels to run ahead
    monkeypatch.setenv("SPAMTREE_QUAD_UNITS", "4")
    for uid in (None, fit.make_unique_id()):
        # the communicator run also starts phase A of the top levels ahead of time, as sharded runs do by default
        monkeypatch.setenv("SPAMTREE_ASYNC_TOP", "0" if uid is None else "1")
        ch = fit.Chain(pb["y"], pb["X"], pb["Z"], pb["coords"], pb["mv_id"], pb["blocking"], pb["gix_block"], pb["res_is_ref"],
                       pb["parents"], pb["children"], False, pb["block_names"], pb["block_groups"], pb["indexing"],
                       pb["bounds"], pb["theta"], np.zeros(pb["p"]), 0.1, 0.01 * np.eye(4), seed=5, unique_id=uid)
        ch.step(12)
        st = ch.state()
        states.append((st["theta"].copy(), st["tausq_inv"].copy(), float(st["loglik"]), ch.get_w().copy()))
        ch.close()
    a, b = states
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and np.array_equal(a[3], b[3])


@pytest.mark.parametrize("async_top", ["1", "0"])
def test_cpp_driver_with_top_levels_ahead_of_time(async_top, monkeypatch):
    """st_factor_begin: the C++ driver starts phase A of the top levels for the proposal before the sweep, on a second
    stream (SPAMTREE_QUAD_MIN=1 gives this small tree quad levels below, hence top levels to run ahead).  Chains with and
    without it (SPAMTREE_ASYNC_TOP=0) equal the oracle's."""
    from oracle import spamtree_oracle as so
    from spamtree_amd import fit
    monkeypatch.setenv("SPAMTREE_QUAD_MIN", "1")
    monkeypatch.setenv("SPAMTREE_QUAD_UNITS", "4")
    monkeypatch.setenv("SPAMTREE_ASYNC_TOP", async_top)
    pb = make_problem(side=40, q=1, seed=21, missing=0.05)
    k = pb["theta"].size
    kw = dict(mcmc_keep=3, mcmc_burn=40, mcmc_thin=1, adapting=True, seed=7, main_verbose=False)
    ref = so.spamtree_mv_mcmc(*args_of(pb, k), **kw)
    got = fit.spamtree_mv_mcmc(*args_of(pb, k), **kw)
    assert relerr(got["theta_mcmc"], ref["theta_mcmc"]) < 1e-8
    assert relerr(got["tausq_mcmc"], ref["tausq_mcmc"]) < 1e-8 and relerr(got["beta_mcmc"], ref["beta_mcmc"]) < 1e-8
    for i in range(3):
        assert relerr(np.asarray(got["w_mcmc"][i]).reshape(-1), ref["w_mcmc"][i]) < 1e-8


def test_deferred_sweep_protocol_failure_and_misuse():
    """st_sample_w_loglik_begin / _end (the C++ driver's default).  A sweep that fails (negative tausq^-1: codes
    10 / 11, spamtree_model.cpp:1056, 1135) surfaces from _end AFTER the proposal's st_factor has run in between; a second
    _begin without _end is refused; the handle is usable afterwards and gives what the synchronous call gives."""
    import ctypes as C
    from tests.test_gpu_parity import hip_model
    pb = make_problem(side=25, q=1, seed=21)
    hm = hip_model(pb, tausq=0.2)
    lib, h = hm.lib, hm.h
    dp = C.POINTER(C.c_double)
    th = np.ascontiguousarray(pb["theta"], dtype=np.float64)
    assert hm.get_loglik_comps_w(0)
    z = np.random.default_rng(0).standard_normal(pb["n"])
    # reference: the synchronous pair (after one warm-up sweep: the first sweep after a factorisation also rebuilds the
    # records' Gram parts and takes other kernels, equal to 1e-12 but not bit for bit)
    ll_sync = C.c_double()
    assert lib.st_sample_w_loglik(h, z.ctypes.data_as(dp), 0, 0, 0, C.byref(ll_sync)) == 0
    hm.set_w(np.zeros(pb["n"]))
    assert lib.st_sample_w_loglik(h, z.ctypes.data_as(dp), 0, 0, 0, C.byref(ll_sync)) == 0
    w_sync = hm.get_w().copy()
    # deferred: the same sweep from the same state, the proposal's phase A in between
    hm.set_w(np.zeros(pb["n"]))
    assert lib.st_sample_w_loglik_begin(h, z.ctypes.data_as(dp), 0, 0, 0) == 0
    assert lib.st_sample_w_loglik_begin(h, z.ctypes.data_as(dp), 0, 0, 0) < 0                  # a second _begin without _end: usage error
    # ... like every other sweep, and whatever reads or replaces w on the host, predicts, swaps or takes a log-density (the
    # header's table next to st_factor_enqueue): refused with a text that names the call, nothing changed -- _end below still
    # hands over the synchronous pair's results
    buf = np.zeros(pb["n"])
    llx = C.c_double()
    zp = z.ctypes.data_as(dp)
    for name, call in [("st_sample_w_loglik_begin", lambda: lib.st_sample_w_loglik_begin(h, zp, 0, 0, 0)),
                       ("st_sample_w", lambda: lib.st_sample_w(h, zp, 0, 0)),
                       ("st_sample_w_loglik", lambda: lib.st_sample_w_loglik(h, zp, 0, 0, 0, C.byref(llx))),
                       ("st_set_w", lambda: lib.st_set_w(h, buf.ctypes.data_as(dp))), ("st_get_w", lambda: lib.st_get_w(h, buf.ctypes.data_as(dp))),
                       ("st_predict", lambda: lib.st_predict(h, 1)), ("st_yhat", lambda: lib.st_yhat(h, zp, 0, 0, buf.ctypes.data_as(dp))),
                       ("st_swap", lambda: lib.st_swap(h)), ("st_loglik_w", lambda: lib.st_loglik_w(h, 0, C.byref(llx)))]:
        assert call() == -1, name
        text = lib.st_last_error(h).decode()
        assert text.startswith(name + " ") and "st_sample_w_loglik_end" in text, (name, text)
    assert np.all(buf == 0.0)
    ll_f = C.c_double()
    assert lib.st_factor(h, 1, th.ctypes.data_as(dp), th.size, C.byref(ll_f)) == 0
    ll_def = C.c_double()
    assert lib.st_sample_w_loglik_end(h, C.byref(ll_def)) == 0
    assert np.array_equal(hm.get_w(), w_sync) and ll_def.value == ll_sync.value
    assert lib.st_sample_w_loglik_end(h, C.byref(ll_def)) < 0                                 # _end without _begin
    # a failing sweep: negative tausq^-1 makes the posterior precision of every block indefinite
    bad = np.array([-50.0])
    assert lib.st_set_tausq_inv(h, bad.ctypes.data_as(dp)) == 0
    assert lib.st_sample_w_loglik_begin(h, z.ctypes.data_as(dp), 0, 1, 0) == 0
    assert lib.st_factor(h, 1, th.ctypes.data_as(dp), th.size, C.byref(ll_f)) == 0
    assert lib.st_sample_w_loglik_end(h, C.byref(ll_def)) in (10, 11)
    # the handle is not poisoned: restore tausq and w, the synchronous sweep reproduces the reference
    good = np.array([1.0 / 0.2])
    assert lib.st_set_tausq_inv(h, good.ctypes.data_as(dp)) == 0
    hm.set_w(np.zeros(pb["n"]))
    ll3 = C.c_double()
    assert lib.st_sample_w_loglik(h, z.ctypes.data_as(dp), 0, 0, 0, C.byref(ll3)) == 0
    assert np.array_equal(hm.get_w(), w_sync) and ll3.value == ll_sync.value
    hm.close()


def test_chain_with_and_without_deferred_sync_are_identical(monkeypatch):
    """SPAMTREE_DEFER_SYNC and SPAMTREE_EARLY_BETA (the tausq / beta draws made under the proposal's factorisation:
    st_factor_enqueue / st_factor_finish) are read when the chain is created: same chain bit for bit."""
    from spamtree_amd import fit
    pb = make_problem(side=25, q=1, seed=3, missing=0.1)
    outs = []
    for defer, early in (("1", "1"), ("0", "1"), ("1", "0")):
        monkeypatch.setenv("SPAMTREE_DEFER_SYNC", defer)
        monkeypatch.setenv("SPAMTREE_EARLY_BETA", early)
        ch = fit.Chain(pb["y"], pb["X"], pb["Z"], pb["coords"], pb["mv_id"], pb["blocking"], pb["gix_block"], pb["res_is_ref"],
                       pb["parents"], pb["children"], False, pb["block_names"], pb["block_groups"], pb["indexing"], pb["bounds"],
                       pb["theta"], np.zeros(pb["p"]), 0.1, 0.01 * np.eye(4), seed=5)
        ch.step(40)
        outs.append(dict(ch.state(), w=ch.get_w()))
        ch.close()
    for o in outs[1:]:
        for k in ("theta", "tausq_inv", "loglik", "w"):
            assert np.array_equal(o[k], outs[0][k]), k


def test_factor_in_two_halves_equals_st_factor():
    """st_factor_enqueue / st_factor_finish (include/spamtree_hip.h): the same return code and log-density as st_factor, with the
    setters -- which no longer synchronise the host -- called in between; misuse is refused."""
    import ctypes as C
    from tests.test_gpu_parity import hip_model
    pb = make_problem(side=25, q=1, seed=4, missing=0.1)
    rng = np.random.default_rng(1)
    w0 = rng.standard_normal(pb["n"])
    hm = hip_model(pb, w=w0, tausq=0.2)
    assert hm.get_loglik_comps_w(0)
    lib, h = hm.lib, hm.h
    dp = C.POINTER(C.c_double)
    th = np.ascontiguousarray(pb["theta"] * 1.1)
    ll0, ll1 = C.c_double(), C.c_double()
    assert lib.st_factor(h, 1, th.ctypes.data_as(dp), th.size, C.byref(ll0)) == 0
    assert lib.st_factor_finish(h, C.byref(ll1)) < 0                      # nothing enqueued
    assert lib.st_factor_enqueue(h, 1, th.ctypes.data_as(dp), th.size) == 0
    assert lib.st_factor_enqueue(h, 1, th.ctypes.data_as(dp), th.size) < 0   # a second one before the first is finished
    # what would read or replace the slot being factorised, sweep, predict or swap is refused with a text that names the call, and
    # changes nothing (the header's table next to st_factor_enqueue): the log-density below still equals st_factor's
    zb = rng.standard_normal(pb["n"]); zp = zb.ctypes.data_as(dp)
    buf, big = np.zeros(pb["n"]), np.zeros(pb["n"] * 8)
    llx = C.c_double()
    thp = th.ctypes.data_as(dp)
    w_before = hm.get_w().copy()
    for name, call in [("st_swap", lambda: lib.st_swap(h)), ("st_sample_w", lambda: lib.st_sample_w(h, zp, 0, 0)),
                       ("st_sample_w_loglik", lambda: lib.st_sample_w_loglik(h, zp, 0, 0, 0, C.byref(llx))),
                       ("st_sample_w_loglik_begin", lambda: lib.st_sample_w_loglik_begin(h, zp, 0, 0, 0)),
                       ("st_predict", lambda: lib.st_predict(h, 1)), ("st_factor", lambda: lib.st_factor(h, 0, thp, th.size, C.byref(llx))),
                       ("st_factor", lambda: lib.st_factor(h, 1, thp, th.size, C.byref(llx))),
                       ("st_factor_begin", lambda: lib.st_factor_begin(h, 1, thp, th.size)),
                       ("st_factor_local", lambda: lib.st_factor_local(h, 1, thp, th.size)),
                       ("st_get_block", lambda: lib.st_get_block(h, 1, 0, big.ctypes.data_as(dp), big.ctypes.data_as(dp))),
                       ("st_get_comps", lambda: lib.st_get_comps(h, 1, buf.ctypes.data_as(dp), buf.ctypes.data_as(dp))),
                       ("st_loglik_w", lambda: lib.st_loglik_w(h, 1, C.byref(llx)))]:
        assert call() == -1, name
        text = lib.st_last_error(h).decode()
        assert text.startswith(name + " ") and "st_factor_finish" in text, (name, text)
    assert lib.st_loglik_w(h, 0, C.byref(llx)) == 0 and abs(llx.value - hm.loglik_w[0]) <= 1e-9 * abs(hm.loglik_w[0])   # the accepted slot stays readable ...
    assert lib.st_get_comps(h, 0, buf.ctypes.data_as(dp), buf.ctypes.data_as(dp)) == 0
    assert np.array_equal(hm.get_w(), w_before)                                           # ... and so does w
    t2 = np.array([1.0 / 0.3]); b2 = np.full(pb["p"], 0.25)
    assert lib.st_set_tausq_inv(h, t2.ctypes.data_as(dp)) == 0 and lib.st_set_beta(h, b2.ctypes.data_as(dp)) == 0
    t2[:] = -1.0; b2[:] = 99.0                                               # the caller's buffers are free on return
    assert lib.st_factor_finish(h, C.byref(ll1)) == 0 and ll1.value == ll0.value
    bad = th.copy(); bad[0] = -1.0                                           # a failing proposal: the reference's errtype through _finish
    assert lib.st_factor_enqueue(h, 1, bad.ctypes.data_as(dp), bad.size) == 0
    assert lib.st_factor_finish(h, C.byref(ll1)) in (1, 2, 3)
    # the uploads arrived: a sweep with the new tausq / beta equals one on a fresh handle that was given them up front
    z = rng.standard_normal(pb["n"])
    hm.deal_with_w(z)
    hr = hip_model(pb, w=w0, tausq=0.3, beta=np.full(pb["p"], 0.25))
    assert hr.get_loglik_comps_w(0)
    hr.deal_with_w(z)
    assert np.array_equal(hm.get_w(), hr.get_w())
    hm.close(); hr.close()


def test_four_ways_to_run_the_sweep_are_bitwise_identical(monkeypatch):
    """One iteration's sweep and the log-density of its w, from the same w, the same supplied normals and the same theta:
    st_sample_w + st_loglik_w, st_sample_w_loglik, st_sample_w_loglik_begin + _end, and the first two again on a second
    handle with a one-rank communicator (the exchange protocol: gather-pack, all-gather, k_pack_comps, all-reduce,
    st_mg_finish / the fused exchange).  They share their steps in the library; w and the log-density are equal to the
    bit.  The tree (side 25, a tenth of the rows missing, SPAMTREE_QUAD_MIN=1) has a reference level and the leaf level
    on k_factor_quad and blocks without observed rows (asserted)."""
    import ctypes as C
    from spamtree_amd import fit
    from tests.test_gpu_parity import hip_model
    monkeypatch.setenv("SPAMTREE_QUAD_MIN", "1")
    pb = make_problem(side=25, q=1, seed=21, missing=0.1)
    rng = np.random.default_rng(8)
    w0, z_warm, z = (rng.standard_normal(pb["n"]) for _ in range(3))
    dp = C.POINTER(C.c_double)
    zp = z.ctypes.data_as(dp)
    n_obs = np.bincount(pb["blocking"] - 1, weights=np.isfinite(pb["y"]).astype(float), minlength=pb["block_names"].size)
    assert np.any(n_obs == 0)                                    # prediction blocks
    results = {}
    for comm in (False, True):
        hm = hip_model(pb, w=w0, tausq=0.2)
        lib, h = hm.lib, hm.h
        if comm:
            buf = C.create_string_buffer(bytes(fit.make_unique_id()), 128)
            assert lib.st_comm_init(h, C.cast(buf, C.c_void_p)) == 0
        assert hm.get_loglik_comps_w(0)
        quad = [any(k.startswith("k_factor_quad<") for k in lv["A"]) for lv in hm.route_info()["levels"]]
        assert quad[-1] and quad[-2], quad                       # the leaf level and the last reference level
        hm.deal_with_w(z_warm)       # (the first sweep after a factorisation also rebuilds the records' Gram parts: other kernels)

        def run(name, sweep):
            hm.set_w(w0)
            ll = sweep()
            results[(name, comm)] = (hm.get_w().copy(), ll)

        def two_calls():
            hm.deal_with_w(z)
            return hm.get_loglik_w(0)

        def one_call():
            ll = C.c_double()
            assert lib.st_sample_w_loglik(h, zp, 0, 0, 0, C.byref(ll)) == 0
            return ll.value

        def two_halves():
            ll = C.c_double()
            assert lib.st_sample_w_loglik_begin(h, zp, 0, 0, 0) == 0
            assert lib.st_sample_w_loglik_end(h, C.byref(ll)) == 0
            return ll.value

        run("st_sample_w + st_loglik_w", two_calls)
        run("st_sample_w_loglik", one_call)
        if not comm:
            run("_begin + _end", two_halves)
        hm.close()
    assert len(results) == 5
    w_ref, ll_ref = results[("st_sample_w + st_loglik_w", False)]
    assert np.isfinite(ll_ref) and not np.array_equal(w_ref, w0)
    for key, (w, ll) in results.items():
        assert np.array_equal(w, w_ref) and ll == ll_ref, key
