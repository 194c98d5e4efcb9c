"""GPU: the full-size configurations bench.py times (#2, #3, #4, #5 and #3 with limited_tree), value by value, block by block,
against the extended-precision reference (oracle/extended.py over a WorkloadView of the workload's arrays).

test_gpu_scale.test_full_size_properties checks these sizes for self-consistency only.  Here, on a sample of blocks per level
(every block of levels with up to 16 blocks; elsewhere the first and last, evenly spaced ones, the longest chain, the fewest
and most rows, partly observed blocks and seeded random ones), with the default routes (no SPAMTREE_* switch).  Each level's
phase-A kernels are printed right after st_factor and its Gram and sweep kernels right after the first sweep, before their
values are checked; that st_factor_enqueue is asynchronous and which configs' top levels st_factor_begin runs ahead (AHEAD)
is asserted, so the driver's path below is the overlapping one where the tree allows it.  Every device value a check reads
must be finite (a NaN is never dropped by a maximum).

  (a) phase A: the stored panel N = -Ri H and Ri (or 1/sqrt(r_ii)) of slot 0 after st_factor at the workload's theta, and of
      the driver's path at a perturbed theta -- st_factor_begin (top levels on the second stream, under a sweep),
      st_factor_enqueue / st_factor_finish on slot 1 with the quad leaf levels' T deferred, then st_swap, which finishes them;
      the logdet and loglik_w components;
  (b) three sweeps with seeded caller normals: the first after a factorisation (the Gram parts rebuilt), one on cached Gram
      parts, and one after the swap to the new theta.  Each sampled observed block is compared with ExtendedBlocks.cond_draw
      given the values before the sweep and its descendants' values after it (what the leaf-to-root sweep conditions it on).
      A block's conditional involves every observed descendant (children = all descendants in a full tree), so the blocks
      whose subtree is too large for the CPU budget (the top levels of full trees) are not drawn here: at most CAP observed
      descendants per block and BUDGET per level.  Rows of prediction blocks stay bitwise unchanged;
  (c) phase C after each sweep: the components of the sampled blocks, and loglik_w against the long-double sum of all
      device components (the final reduction over 87k-556k blocks);
  (d) phase P (configs with NA rows): st_predict after the first sweep, with that sweep's normals, against predict_draw;
  (e) st_beta_stats (X'(y - w) with quirk Q3's pairing) and st_tausq_stats (ssq and n_obs_by_q) over all rows in long double;
  (f) st_simulate with caller normals against prior_draw given the device's own parent values (configs without NA rows:
      st_simulate refuses the others);
  (g) 1e5 seeded new points at #3 (k_points_mfma) and #4 (k_points_generic): the mean and variance of about 512 of them, in
      groups that share a conditioning chain, against point_moments;
  (h) the C++ driver at #3 with bench.py's arguments, stepped until a proposal was accepted (or 100 steps): slot 0's blocks
      at the chain's theta and the components at the chain's w.

Tolerance: values relative to the largest |value| of the level's sampled blocks, TOL = 1e-10; loglik components relative to
the magnitudes of the terms they sum; loglik_w relative to the sum of |component| over all blocks.  No quantity needed more.

Measured on an MI355X, worst over levels and passes (A phase A, B sweep draws, C phase C components, P phase P, E statistics,
F prior draws, G new points, H driver), and the config's wall time, the long-double reference included:
  config          A: N     Ri       logdet   loglik   B: w     C: comp  sum      E: xty   ssq      F/P: w   G: mean  var      time
  #3 (n = 1e6)       4.6e-13  3.0e-13  8.0e-14  8.5e-13  5.9e-13  7.0e-13  3.0e-16  7.0e-17  4.1e-17  5.9e-14  1.1e-13  1.8e-13  102 s
  #2 (n = 1e5)       1.3e-13  5.7e-14  1.0e-14  1.1e-13  1.8e-13  1.4e-13  2.4e-16  4.2e-17  1.0e-16  1.4e-14                      30 s
  #4 (q = 3)         1.0e-12  8.5e-13  2.0e-14  1.2e-12  1.2e-12  6.2e-13  9.2e-17  9.0e-17  8.5e-17  1.1e-13  1.8e-13  1.5e-13   99 s
  #5 (n = 4e6, NA)   1.1e-12  4.1e-13  4.1e-14  1.4e-12  9.2e-13  5.6e-13  1.6e-16  1.2e-16  1.2e-16  2.4e-13 (P)            32 s
  #3 limited         2.7e-13  2.2e-13  1.9e-14  2.0e-13  3.0e-13  1.0e-13  1.9e-16  7.1e-17  5.8e-17  3.2e-14                       4 s
  H (#3 driver, one step: a proposal was accepted): N 5.7e-13, Ri 2.2e-13, logdet 1.8e-14, loglik 5.7e-13.
Sweep coverage (blocks drawn against the reference): every level of #2 and of the limited tree; #3 from level 2 (1 block),
3 (5), 4 (23) down; #4 from level 4 (4 blocks) down; #5 from level 4 (2), 5 (9) down.

Seeded defects (local builds, not committed), each run against this file and the rest of the GPU suite.  The first two pass
the rest of the suite (306 tests) and fail here:
  - k_sample_leaf_wide (#4's leaf sweep, a grid of 16 x CUs workgroups over 16384 blocks) reads the normals of every trip at
    the first trip's base row (zc[j] = z[min(row0 of the workgroup's first block, row0) + j]): config4 fails at its first
    sweep check, the leaf level's draws off by a relative 0.53 (test_full_size_properties still passes: the draws stay
    reproducible, finite and pulled towards y);
  - k_marginal_invchol_wave (the limited tree's marginal factors, a grid of 8 x CUs workgroups of 4 waves) stops after its
    first trip: config3_n1e6_limited fails at its first check, phase A of the leaf level, N off by a relative 1.0 (the panels
    of the blocks past the first trip are never written).
The other two are caught here and by the existing suite as well:
  - k_points_generic keeps v'v and v'u of the previous point of the workgroup (not reset per trip): config4 fails at G, the
    mean off by a relative 5.8; test_gpu_predict_points' deep4 replay catches it as well;
  - k_factor_ref_finish (2 x CUs) stops after its first trip: config4 fails (st_factor reports the unfinished blocks), and
    so does test_gpu_scale.test_full_size_properties[config4].
"""
import ctypes as C
import os
import time

import numpy as np
import pytest

from tests.test_gpu_scale import FULL

pytestmark = pytest.mark.gpu

TOL = 1e-10
HL2PI = 0.918938533204672741780329736405617639861
CONFIGS = [pytest.param(*p.values, False, id=p.id) for p in FULL] + \
          [pytest.param(1000, 1, 25, None, True, id="config3_n1e6_limited")]
# per config: sampled blocks per level, and the sweep's cap on a checked block's observed descendants / their budget per level
# (the blocks whose terms the reference assembles for the sweep check; #4's chains of 525 rows cost the most per block)
PLAN = {1: dict(nper=24, cap=6000, budget=8000), 3: dict(nper=12, cap=100, budget=400)}
PLAN_CELL9 = dict(nper=24, cap=1500, budget=3000)
# (side, q, limited) of the configs whose top levels st_factor_begin runs ahead on the second stream (#4's and the limited
# tree's trees do not qualify: the call is a no-op there)
AHEAD = {(1000, 1, False), (316, 1, False), (1155, 3, False)}


def csr_sum(ptr, vals):
    cs = np.concatenate([[0], np.cumsum(vals)])
    return cs[ptr[1:]] - cs[ptr[:-1]]


def sample_levels(view, nper, seed):
    """{level: (observed blocks sampled, prediction blocks sampled)}."""
    rng = np.random.default_rng(seed)
    labels = np.unique(view.block_groups)
    level = np.searchsorted(labels, view.block_groups)
    m = view.indexing.sizes()
    P = csr_sum(view.parents.ptr, m[view.parents.idx])
    ct = view.block_ct_obs
    out = {}
    for lv in range(labels.size):
        res = []
        for cand in (np.nonzero((level == lv) & (ct > 0))[0], np.nonzero((level == lv) & (ct == 0) & (m > 0))[0]):
            if cand.size <= 16:
                res.append([int(u) for u in cand])
                continue
            pick = [cand[0], cand[-1]] + list(cand[np.linspace(0, cand.size - 1, 10).round().astype(int)])
            pick += [cand[np.argmax(P[cand])], cand[np.argmin(m[cand])], cand[np.argmax(m[cand])]]
            part = cand[(ct[cand] > 0) & (ct[cand] < m[cand])]
            if part.size:
                pick += list(part[np.linspace(0, part.size - 1, min(3, part.size)).round().astype(int)])
            seen = list(dict.fromkeys(int(u) for u in pick))
            rest = np.setdiff1d(cand, seen)
            k = max(0, nper - len(seen))
            seen += [int(u) for u in rng.choice(rest, size=min(k, rest.size), replace=False)]
            res.append(seen)
        if res[0] or res[1]:
            out[lv] = tuple(res)
    return out


def get_block(lib, h, slot, u):
    m, P = C.c_int64(), C.c_int64()
    isref, nobs = C.c_int32(), C.c_int32()
    assert lib.st_block_dims(h, u, C.byref(m), C.byref(P), C.byref(isref), C.byref(nobs)) == 0
    m, P = m.value, P.value
    N = np.zeros(m * max(P, 1))
    Ri = np.zeros(m * m if isref.value else m)
    dp = C.POINTER(C.c_double)
    assert lib.st_get_block(h, slot, u, N.ctypes.data_as(dp), Ri.ctypes.data_as(dp)) == 0
    N = N[: m * P].reshape(P, m).T if P else np.zeros((m, 0))
    return N, (Ri.reshape(m, m).T if isref.value else Ri), bool(isref.value)


def get_comps(lib, h, slot, nb):
    a, b = np.zeros(nb), np.zeros(nb)
    dp = C.POINTER(C.c_double)
    assert lib.st_get_comps(h, slot, a.ctypes.data_as(dp), b.ctypes.data_as(dp)) == 0
    return a, b


class Report:
    """Worst error per (stage, level, quantity), printed at the end of a config."""

    def __init__(self, name):
        self.name, self.rows, self.t0 = name, {}, time.time()

    def add(self, stage, lv, qty, err, n):
        k = (stage, lv, qty)
        e, c = self.rows.get(k, (0.0, 0))
        self.rows[k] = (max(e, err), c + n)
        assert err <= TOL, (self.name, stage, lv, qty, err)

    def show(self):
        print(f"\n[{self.name}] worst relative error per stage / level / quantity (blocks checked), {time.time() - self.t0:.0f} s")
        for (stage, lv, qty), (e, c) in sorted(self.rows.items(), key=lambda kv: (kv[0][0], kv[0][1], kv[0][2])):
            print(f"  {stage:<12} level {lv:>2}  {qty:<8} {e:9.2e}  ({c})")


def worst(errs):
    """The largest of a level's errors; inf if any is not finite (Python's max() would drop a NaN that is not first)."""
    a = np.asarray(errs, dtype=np.float64)
    return float(np.max(a)) if np.all(np.isfinite(a)) else float("inf")


def level_err(pairs):
    """max |dev - ref| / max |ref| over a level's blocks: pairs of (device, reference) arrays; inf if a device value is not
    finite."""
    if not all(np.all(np.isfinite(d)) for d, _ in pairs):
        return float("inf")
    num = worst([float(np.max(np.abs(np.asarray(d, dtype=np.longdouble) - r))) if np.size(r) else 0.0 for d, r in pairs])
    den = worst([float(np.max(np.abs(r))) if np.size(r) else 0.0 for _, r in pairs])
    return num / max(den, 1e-300)


def check_phase_a(rep, stage, lib, h, slot, ex, levels, w):
    nb = ex.om.n_blocks
    ld, qd = get_comps(lib, h, slot, nb)
    obs_all = ex.om.block_ct_obs > 0
    assert np.all(np.isfinite(ld[obs_all])) and np.all(np.isfinite(qd[obs_all])), stage
    for lv, (obs, _) in levels.items():
        if not obs:
            continue
        Np, Rp, cl, cq = [], [], [], []
        for u in obs:
            N, Ri, isref = get_block(lib, h, slot, u)
            b = ex.block(u)
            assert isref == b["isref"], (stage, u)
            Np.append((N, b["N"]))
            Rp.append((Ri, b["Ri"] if isref else b["d"]))
            rl, rq = ex.loglik_comp(u, w)
            diag = np.diag(b["Ri"]) if isref else b["d"]
            cl.append(abs(ld[u] - rl) / max(float(np.sum(np.abs(np.log(diag)))), 1e-300))
            cq.append(abs(qd[u] - rq) / (b["m"] * HL2PI + float(abs(rq + b["m"] * HL2PI))))
        rep.add(stage, lv, "N", level_err(Np), len(obs))
        rep.add(stage, lv, "Ri", level_err(Rp), len(obs))
        rep.add(stage, lv, "logdet", worst(cl), len(obs))
        rep.add(stage, lv, "loglik", worst(cq), len(obs))


def check_phase_c(rep, stage, hm, ex, levels, w):
    ll = hm.get_loglik_w(0)
    ld, qd = hm.comps(0)
    for lv, (obs, _) in levels.items():
        if obs:
            errs = []
            for u in obs:
                b = ex.block(u)
                _, rq = ex.loglik_comp(u, w)
                errs.append(abs(qd[u] - rq) / (b["m"] * HL2PI + float(abs(rq + b["m"] * HL2PI))))
            rep.add(stage, lv, "loglik", worst(errs), len(obs))
    tot = np.sum(ld.astype(np.longdouble)) + np.sum(qd.astype(np.longdouble))
    terms = float(np.sum(np.abs(ld)) + np.sum(np.abs(qd)))
    rep.add(stage, -1, "loglik_w", float(abs(ll - tot)) / terms, int(ld.size))


def check_sweep(rep, stage, ex, levels, plan, w0, w1, z, pred_rows, desc):
    assert np.all(np.isfinite(w1)), stage
    assert np.array_equal(w1[pred_rows], w0[pred_rows]), stage
    om = ex.om
    for lv, (obs, _) in levels.items():
        pairs, spent = [], 0
        for u in obs:
            if desc[u] > plan["cap"] or spent + desc[u] > plan["budget"]:
                continue
            spent += desc[u]
            iu = om.indexing[u]
            pairs.append((w1[iu], ex.cond_draw(u, w0, z[iu], w_desc=w1)))
        if pairs:
            rep.add(stage, lv, "w", level_err(pairs), len(pairs))


def check_stats(rep, stage, hm, view, w):
    xty, ssq = hm.stats()
    nq = np.zeros(view.q, dtype=np.int64)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    s2 = np.zeros(view.q)
    assert hm.lib.st_tausq_stats(hm.h, s2.ctypes.data_as(dp), nq.ctypes.data_as(ip)) == 0
    L = np.longdouble
    oix = np.nonzero(view.obs)[0]
    mv0 = view.mv_id[oix] - 1
    for j in range(view.q):
        ia = np.nonzero(mv0 == j)[0]
        assert nq[j] == ia.size, (stage, j)
        Xa = view.X[oix[ia]].astype(L)
        r = view.y[oix[ia]].astype(L) - w[ia].astype(L)                   # Q3: positions of the subset on the full w
        ref = Xa.T @ r
        mag = np.abs(Xa).T @ np.abs(r)
        rep.add(stage, -1, "xty", float(np.max(np.abs(xty[:, j] - ref) / mag)), 1)
        e = view.y[oix[ia]].astype(L) - view.XB[oix[ia]].astype(L) - w[oix[ia]].astype(L)
        ref = np.sum(e * e)
        rep.add(stage, -1, "ssq", float(abs(ssq[j] - ref) / ref), 1)


@pytest.mark.parametrize("side,q,cell_size,missing,limited", CONFIGS)
def test_full_size_against_extended_precision(side, q, cell_size, missing, limited):
    from oracle.extended import ExtendedBlocks, WorkloadView
    from spamtree_amd.model import SpamTreeMV
    from spamtree_amd.synthetic import make_workload
    assert not [k for k in os.environ if k.startswith("SPAMTREE_")], "the default routes are the ones bench.py times"
    name = f"side={side} q={q} cell={cell_size} missing={missing} limited={limited}"
    rep = Report(name)
    plan = PLAN_CELL9 if cell_size == 9 else PLAN[q]
    wl = make_workload(side, q=q, cell_size=cell_size, missing=missing, device=0, limited_tree=limited)
    n, beta, tsq_inv = wl["n"], wl["beta_true"], 1.0 / 0.15
    view = WorkloadView(wl, beta, tsq_inv, limited_tree=limited)
    view.X, view.obs = np.asarray(wl["X"], dtype=np.float64), np.isfinite(wl["y"])
    levels = sample_levels(view, plan["nper"], seed=side + q)
    obs_ct = (view.block_ct_obs > 0).astype(np.int64)
    desc = csr_sum(view.children.ptr, obs_ct[view.children.idx])
    pred_rows = np.nonzero(~view.obs)[0] if missing is not None else np.zeros(0, dtype=np.int64)
    print(f"\n[{name}] n = {n}, {view.n_blocks} blocks, workload {time.time() - rep.t0:.0f} s; sample (level: observed "
          f"blocks / prediction blocks, sweep-checked):")
    rng = np.random.default_rng(2021)
    w0 = 0.3 * rng.standard_normal(n)
    hm = SpamTreeMV(wl["y"], wl["X"], wl["Z"], wl["coords"], wl["mv_id"], wl["blocking"], wl["gix_block"], wl["res_is_ref"],
                    wl["parents"], wl["children"], limited, wl["block_names"], wl["block_groups"], wl["indexing"], w0,
                    beta, wl["theta"], tsq_inv, device=0)
    try:
        theta0 = wl["theta"]
        theta1 = theta0 * (1.0 + 0.03 * np.linspace(-1.0, 1.0, theta0.size))
        ex0, ex1 = ExtendedBlocks(view, theta0), ExtendedBlocks(view, theta1)
        # (a) slot 0 at the workload's theta
        assert hm.get_loglik_comps_w(0)
        show_routes(hm, levels, desc, plan, sweep=False)
        ahead, is_async = hm.lib.st_factor_ahead_levels(hm.h), hm.lib.st_factor_is_async(hm.h)
        print(f"  top levels factorised ahead by st_factor_begin: {ahead}, st_factor_enqueue asynchronous: {is_async}")
        assert is_async == 1 and (ahead > 0) == ((side, q, limited) in AHEAD), (ahead, is_async)
        check_phase_a(rep, "A slot0", hm.lib, hm.h, 0, ex0, levels, w0)
        # (b, c, d, e) the first sweep after a factorisation, phase P, the statistics
        z = [rng.standard_normal(n) for _ in range(3)]
        hm.deal_with_w(z[0])
        show_routes(hm, levels, desc, plan, sweep=True)
        w1 = hm.get_w()
        check_sweep(rep, "B rebuild", ex0, levels, plan, w0, w1, z[0], pred_rows, desc)
        check_phase_c(rep, "C rebuild", hm, ex0, levels, w1)
        if missing is not None:
            hm.predict(True)
            w1p = hm.get_w()
            assert np.array_equal(w1p[view.obs], w1[view.obs])
            for lv, (_, pred) in levels.items():
                if pred:
                    pairs = [(w1p[view.indexing[u]], ex0.predict_draw(u, w1p, z[0][view.indexing[u]])) for u in pred]
                    rep.add("P predict", lv, "w", level_err(pairs), len(pred))
            print(f"  predict: {hm.route_info()['predict']}")
            w1 = w1p
        check_stats(rep, "E stats", hm, view, w1)
        # (b, c) a sweep on cached Gram parts, while the proposal's top levels run ahead on the second stream
        th1 = np.ascontiguousarray(theta1)
        dp = C.POINTER(C.c_double)
        assert hm.lib.st_factor_begin(hm.h, 1, th1.ctypes.data_as(dp), th1.size) == 0
        hm.deal_with_w(z[1])
        w2 = hm.get_w()
        check_sweep(rep, "B cached", ex0, levels, plan, w1, w2, z[1], pred_rows, desc)
        check_phase_c(rep, "C cached", hm, ex0, levels, w2)
        # (a) the driver's path on slot 1: enqueue / finish with the leaf T deferred, then st_swap finishes it
        assert hm.lib.st_factor_enqueue(hm.h, 1, th1.ctypes.data_as(dp), th1.size) == 0
        ll = C.c_double()
        assert hm.lib.st_factor_finish(hm.h, C.byref(ll)) == 0
        hm.theta_update(1, theta1)
        hm.accept_make_change()
        check_phase_a(rep, "A swapped", hm.lib, hm.h, 0, ex1, levels, w2)
        # (b, c, e) the rebuild sweep after the swap
        hm.deal_with_w(z[2])
        w3 = hm.get_w()
        check_sweep(rep, "B swapped", ex1, levels, plan, w2, w3, z[2], pred_rows, desc)
        check_phase_c(rep, "C swapped", hm, ex1, levels, w3)
        check_stats(rep, "E swapped", hm, view, w3)
        # (f) prior simulation on slot 0 (theta1)
        if missing is None:
            Z = rng.standard_normal((n, 2))
            W, _ = hm.simulate(2, z=Z, outcomes=False)
            assert np.all(np.isfinite(W))
            for lv, (obs, _) in levels.items():
                for d in range(2):
                    pairs = [(W[view.indexing[u], d], ex1.prior_draw(u, W[:, d], Z[view.indexing[u], d])) for u in obs]
                    rep.add("F simulate", lv, "w", level_err(pairs), len(obs))
            print(f"  simulate routes {hm.simulate_info(2)['routes']}")
        # (g) new points
        if not limited and cell_size == 25 and missing is None and side in (1000, 577):
            check_points(rep, hm, wl, view, ex1, w3, rng)
    finally:
        hm.close()
    if side == 1000 and not limited:
        check_driver(rep, wl, view, levels)
    rep.show()


def show_routes(hm, levels, desc, plan, sweep):
    """What ran at each level on the default routes (bench.py's), printed before the values are checked: phase A of the last
    factorisation (sweep=False, right after st_factor), then also the Gram and sweep kernels of the last sweep."""
    ri, li = hm.route_info(), hm.level_info()
    assert len(ri["levels"]) == len(li) and all(lv["A"] and (lv["sweep"] or not sweep) for lv in ri["levels"]), ri
    if not sweep:
        for g, (lv, info) in enumerate(zip(ri["levels"], li)):
            print(f"  level {g}: {info['n_blocks']:>6} blocks, phase A {lv['A']}")
        return
    for g, (lv, info) in enumerate(zip(ri["levels"], li)):
        obs, pred = levels.get(g, ([], []))
        nsw, spent = 0, 0
        for u in obs:
            if desc[u] <= plan["cap"] and spent + desc[u] <= plan["budget"]:
                nsw, spent = nsw + 1, spent + desc[u]
        print(f"  level {g}: {info['n_blocks']:>6} blocks, sampled {len(obs)} observed ({nsw} in the sweep check) / "
              f"{len(pred)} prediction; A={lv['A']} gram={lv['gram']} sweep={lv['sweep']}\n    blocks {obs} / {pred}")


def check_points(rep, hm, wl, view, ex, w, rng):
    from spamtree_amd.predict import locate
    npts = 100000
    lo, hi = wl["coords"].min(axis=0), wl["coords"].max(axis=0)
    pts = lo + (hi - lo) * rng.uniform(size=(npts, 2))
    mv = rng.integers(1, view.q + 1, size=npts)
    anchor = locate(wl["topo"], pts, mv, device=0)
    hm.set_points(pts, mv, anchor)
    out = hm.predict_points(mode=1)
    assert np.all(np.isfinite(out["mean"])) and np.all(np.isfinite(out["var"]))
    routes = hm.points_info()["routes"]
    print(f"  points: {npts}, routes {routes}")
    assert routes == ["k_points_generic"] if view.q == 3 else all(x.startswith("k_points_mfma") for x in routes) and routes
    # ~512 points in groups that share a chain (the reference factorises each chain once): the first and the last point's
    # chains and seeded random ones
    r = np.where(ex.isref[anchor], anchor, [int(view.parents[int(a)][-1]) if view.parents[int(a)].size else int(a)
                                            for a in anchor])
    chains = list(dict.fromkeys([int(r[0]), int(r[-1])] + [int(c) for c in rng.choice(np.unique(r), 30, replace=False)]))
    mp, vp, ck = [], [], 0
    for c in chains[:32]:
        sel = np.nonzero(r == c)[0][:16]
        for i in sel:
            mean, var = ex.point_moments(int(anchor[i]), pts[i:i + 1], mv[i:i + 1], w)
            mp.append((out["mean"][i:i + 1], mean))
            vp.append((out["var"][i:i + 1], var))
        ck += sel.size
    rep.add("G points", -1, "mean", level_err(mp), ck)
    rep.add("G points", -1, "var", level_err(vp), ck)


def check_driver(rep, wl, view, levels):
    from oracle.extended import ExtendedBlocks
    from spamtree_amd import fit
    k = wl["theta"].size
    chain = fit.Chain(wl["y"], wl["X"], wl["Z"], wl["coords"], wl["mv_id"], wl["blocking"], wl["gix_block"], wl["res_is_ref"],
                      wl["parents"], wl["children"], False, wl["block_names"], wl["block_groups"], wl["indexing"], wl["bounds"],
                      wl["theta"], np.zeros(wl["p"]), 0.1, 0.01 * np.eye(k), seed=2021, adapting=True, device=0)
    try:
        steps = 0
        while steps < 100:
            chain.step(1)
            steps += 1
            if chain.state()["accept_ratio"] > 0:
                break
        st = chain.state()
        print(f"  driver: {steps} steps, {'a proposal was accepted' if st['accept_ratio'] > 0 else 'no proposal accepted'}, "
              f"theta {st['theta']}")
        ex = ExtendedBlocks(view, st["theta"])
        check_phase_a(rep, "H driver", chain.lib, chain.h, 0, ex, levels, chain.get_w())
    finally:
        chain.close()
