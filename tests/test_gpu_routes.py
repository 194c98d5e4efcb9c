"""GPU: every phase-A, phase-B and phase-P instantiation of the dispatch table against the NumPy oracle, at the chain
lengths that select it.

Each row of ROUTES is an oracle-size problem (mostly deep strip trees, tests/util.strip_coords with K = (2, 1)) plus the
environment switches that make its small levels take the big-level routes.  The row names the instantiations it must
reach; the test runs the whole device protocol first, proves through st_route_info (what the launch sites actually ran)
that the row reached them, and only then compares with the oracle (tolerances of test_gpu_parity: REL = 1e-9, H 1e-8):

  phase A on both slots (loglik_w, the components, H / Ri of every observed block), three sweeps of w, each followed by
  loglik_w, its per-block components and the beta / tausq statistics, st_predict where the row has NA blocks, then a
  rebuild sweep after an accepted theta (slot 1 factorised at theta', swapped in, swept twice: the Gram parts rebuilt,
  then read from the cache) and st_predict again.  The log-density of a sweep is held to REL relative to the magnitudes
  of the terms it sums.  Rows of one problem share one oracle run.

Route keys: "A" phase A, "gram" the Gram kernel of a rebuild sweep, "sweep" any sweep kernel, "rebuild" / "cached" the
sweep kernel of a sweep that formed / read cached Gram parts ("leaf_rebuild" / "leaf_cached": that of the last level),
"P" st_predict.  NKX (k_factor_quad's
chain tiles) follows the level's longest chain P: 32 up to 128 rows, 38 up to 152, 44 up to 176, 50 up to 200;
WCH=true: blocks of <= 27 rows.
"""
import numpy as np
import pytest

from tests.util import make_problem, oracle_model, strip_coords

pytestmark = pytest.mark.gpu
REL = 1e-9
REL_H = 1e-8


def quad(nkx, isref, wch):
    nkt = {32: 8, 38: 10, 44: 11, 50: 13}[nkx]
    return f"k_factor_quad<4, {nkx}, {nkt}, {'true' if isref else 'false'}, {'true' if wch else 'false'}>"


QUAD_MIN = {"SPAMTREE_QUAD_MIN": "1"}    # oracle-size levels have far fewer than 2 x CUs column groups

# id, strip (nx, ny, q), make_problem keywords, environment, routes the row must reach.  The chain lengths in the comments
# are the levels' longest chains (rows), from the tree the keywords build.
ROUTES = [
    # 30-row reference blocks (no wave elimination): P = 120 / 150; leaf P = 180; NA blocks behind the full chain, P = 180
    dict(id="ref30_leaf50_pred50", strip=(640, 5, 1), kw=dict(cell_size=31, tree_depth=6, missing=0.15), env=QUAD_MIN,
         routes={"A": [quad(32, True, False), quad(38, True, False), quad(50, False, True)],
                 "P": [quad(50, False, True)], "sweep": ["k_sample_leaf_seg<4>", "k_sample_lean<true>"]}),
    # 32-row reference blocks of two outcomes: P = 128 / 160 (the NKX 44 team elimination)
    dict(id="ref32_nkx44", strip=(640, 4, 2), kw=dict(cell_size=16, tree_depth=6), env=QUAD_MIN,
         routes={"A": [quad(32, True, False), quad(44, True, False)], "sweep": ["k_sample_lean<true>"]}),
    # 25-row reference blocks, P = 125 / 150 / 175 (128 blocks): NKX 32 / 38 / 44 with the wave elimination; k_gram on
    # every level of a rebuild sweep
    dict(id="ref25_wch_nkx44", strip=(1280, 5, 1), kw=dict(cell_size=25, tree_depth=8), env=dict(QUAD_MIN, SPAMTREE_SPLIT_GRAM="2"),
         routes={"A": [quad(32, True, True), quad(38, True, True), quad(44, True, True)], "gram": ["k_gram"]}),
    # 24-row reference blocks, leaf and NA blocks with P = 144: leaf and prediction NKX 38; reference levels one block per
    # wave (forced)
    dict(id="leaf38_pred38_wave", strip=(640, 4, 1), kw=dict(cell_size=31, tree_depth=6, missing=0.15),
         env=dict(QUAD_MIN, SPAMTREE_SAMPLE_WAVE="2"),
         routes={"A": [quad(38, False, True)], "P": [quad(38, False, True)], "sweep": ["k_sample_wave", "k_sample_leaf_seg<4>"]}),
    # leaf and NA blocks with P = 168: leaf and prediction NKX 44; SPAMTREE_LEAF_SEG=0: the column-aligned leaf sweep
    dict(id="leaf44_pred44_leafsweep", strip=(1280, 4, 1), kw=dict(cell_size=31, tree_depth=7, missing=0.15),
         env=dict(QUAD_MIN, SPAMTREE_LEAF_SEG="0"),
         routes={"A": [quad(38, True, True), quad(44, False, True)], "P": [quad(44, False, True)], "sweep": ["k_sample_leaf"]}),
    # two outcomes of 9 knots, nine levels: leaf chains of 9 ancestors (k_sample_leaf_seg<6>); the last reference level
    # forms its children's Gram parts itself (k_gram_direct)
    dict(id="seg6_gram_direct", strip=(640, 6, 2), kw=dict(cell_size=9, tree_depth=9), env=dict(QUAD_MIN, SPAMTREE_SPLIT_GRAM="2"),
         routes={"A": [quad(38, True, True)], "sweep": ["k_sample_leaf_seg<6>"], "gram": ["k_gram", "k_gram_direct"]}),
    # the 25 x 25 grid with NA rows (test_gpu_parity's CASES[1]): leaf and prediction chains of <= 78 rows, NKX 32
    dict(id="grid_leaf32_pred32", side=25, kw=dict(missing=0.12), env=QUAD_MIN,
         routes={"A": [quad(32, False, True)], "P": [quad(32, False, True)]}),
    # eight 32-row ancestors: the leaf level's chains are 256 rows, the longest the column-group path takes; no lean kernel
    # there (chains > 255 rows), so its sweeps that read cached Gram parts stay on k_sample_mfma
    dict(id="leaf256_cached_mfma", strip=(1400, 4, 2), kw=dict(cell_size=16, tree_depth=8), env={}, leaf_P_min=256,
         routes={"leaf_cached": ["k_sample_mfma"]}),
]
# instantiations no row reaches, on purpose
EXCLUDED = {
    quad(50, True, True): "never dispatched: a reference level with chains of 177-200 rows takes k_factor_mfma "
                          "(the NKX 50 team elimination spills registers; spamtree_hip.hip, the q_nkx choice)",
    quad(50, True, False): "never dispatched, as above",
}

# ---- the wide-block (scratch-arena) path and the generic kernels: levels of more than 32-row blocks, chains of more than
# 256 rows, force_generic, limited_tree.  Further keys: `force_generic` (the st_options bit), `at` (kernel, lo, hi: a
# level of chains of lo..hi rows takes that kernel), `mirror` (k_gram_big's mode, asserted from the routes of every level),
# `not_routes` (instantiations the row must not reach), `leaf_maxMa`.  Route keys "rebuild" / "leaf_rebuild": the sweep
# kernels of sweeps that formed the Gram parts.
WIDE = dict(strip=(370, 10, 3), kw=dict(tree_depth=7, missing=0.1))   # config #4's blocks (up to 75 rows), NA blocks, n = 11 100
NO_LCHAIN = dict(SPAMTREE_LCHAIN="0", SPAMTREE_LCHAIN_REF="0")
WIDE_ROUTES = [
    # the default routes of config #4's shape: reference levels of <= 74-row blocks on k_factor_lchain + k_factor_ref_finish
    # (P = 67 ... 345 on <96>, level 7 P = 414 on <136>), the leaf level (P = 471, <= 50 columns) on k_factor_lchain<136>;
    # every level on the big path, so k_gram_big writes the lower triangles only (mirror = 0) and the rebuild sweep of the
    # leaf level runs k_sample_leaf_wide on the parts it wrote; the NA blocks (P = 471) on the generic predict kernel
    dict(id="wide4_default_pred", **WIDE, env={}, mirror=0, at=[("k_factor_lchain<96>", 1, 384), ("k_factor_lchain<136>", 385, 544)],
         routes={"A": ["k_factor_lchain<96>", "k_factor_lchain<136>", "k_factor_ref_finish", "k_lchain_scalars"],
                 "gram": ["k_gram_big"], "sweep": ["k_sample<true, false>"], "leaf_rebuild": ["k_sample_leaf_wide"],
                 "leaf_cached": ["k_sample_leaf_wide"], "P": ["k_factor<true, MODE_PREDICT>"]}),
    # SPAMTREE_GRAM_BIG=0: the rebuild sweep forms the Gram parts in the sweep kernels (k_sample<true, true> on the leaf level)
    dict(id="wide4_no_grambig", **WIDE, env=dict(SPAMTREE_GRAM_BIG="0"), not_routes={"gram": ["k_gram_big"]},
         routes={"leaf_rebuild": ["k_sample<true, true>"], "leaf_cached": ["k_sample_leaf_wide"]}),
    # SPAMTREE_LEAF_WIDE=0: the leaf level on k_sample<true, true> in every sweep
    dict(id="wide4_leafwide_off", **WIDE, env=dict(SPAMTREE_LEAF_WIDE="0"), mirror=0,
         not_routes={"sweep": ["k_sample_leaf_wide"]},
         routes={"leaf_rebuild": ["k_sample<true, true>"], "leaf_cached": ["k_sample<true, true>"]}),
    # one block per workgroup: the root and levels 2-6 (67-74 columns) on <5, 3, 24>, level 7 (61) and the leaf level (50)
    # on <4, 5, 34>
    dict(id="wide4_bigmfma", **WIDE, env=dict(NO_LCHAIN, SPAMTREE_WIDE="0"),
         routes={"A": ["k_factor_bigmfma<5, 3, 24>", "k_factor_bigmfma<4, 5, 34>"]}),
    # sibling groups forced onto every level
    dict(id="wide4_sibling_groups", **WIDE, env=dict(NO_LCHAIN, SPAMTREE_WIDE="2"), routes={"A": ["k_factor_wide<WG_JT>"]}),
    # the generic kernels on every level
    dict(id="wide4_generic", **WIDE, env={}, force_generic=True, mirror=0,
         routes={"A": ["k_factor<true, MODE_FACTOR>"], "P": ["k_factor<true, MODE_PREDICT>"], "gram": ["k_gram_big"],
                 "sweep": ["k_sample<true, false>"]}),
    # no NA rows: 75-column reference blocks throughout, level 7 with P = 450 > 384 takes <5, 3, 24>'s second pass over
    # the chain; the leaf level (45 columns, P = 525) <3, 5, 34>
    dict(id="wide4_bigmfma_second_pass", strip=(370, 10, 3), kw=dict(tree_depth=7), env=dict(NO_LCHAIN, SPAMTREE_WIDE="0"),
         at=[("k_factor_bigmfma<5, 3, 24>", 385, 544)], routes={"A": ["k_factor_bigmfma<5, 3, 24>", "k_factor_bigmfma<3, 5, 34>"]}),
    # 96-row reference blocks (32 knots x 3 outcomes; generic factor and sweep kernels, the LDS one at the root) above a
    # leaf level of 48 columns whose chains are exactly 384 rows (the last k_factor_lchain<96> length) and whose widest
    # ancestor has exactly 96 rows (the widest k_sample_leaf_wide takes)
    dict(id="leafwide_edge_ma96_p384", strip=(64, 8, 3), kw=dict(cell_size=(4, 8), tree_depth=4), env={}, mirror=0,
         leaf_maxMa=96, at=[("k_factor_lchain<96>", 384, 384)],
         routes={"A": ["k_factor<false, MODE_FACTOR>", "k_factor<true, MODE_FACTOR>", "k_factor_lchain<96>"],
                 "sweep": ["k_sample<true, false>"], "leaf_rebuild": ["k_sample_leaf_wide"], "leaf_cached": ["k_sample_leaf_wide"]}),
    # config #5's shape (27-row blocks of three outcomes, ten levels) with 10 % of the third outcome NA: levels 9 and 10
    # (P = 213 / 240) beyond k_factor_quad's 200 rows on k_factor_mfma; the NA blocks (P = 239) on the generic LDS kernel
    dict(id="cfg5_mfma_chains_pred", strip=(900, 6, 3), kw=dict(cell_size=9, tree_depth=9, missing=(0.0, 0.0, 0.1)), env={},
         at=[("k_factor_mfma", 201, 230), ("k_factor_mfma", 231, 256)],
         routes={"A": ["k_factor_mfma"], "P": ["k_factor<false, MODE_PREDICT>"]}),
    # the column-group problem of grid_leaf32_pred32 on the generic kernels (every level big: mirror = 0)
    dict(id="grid_generic", side=25, kw=dict(missing=0.12), env={}, force_generic=True, mirror=0,
         routes={"A": ["k_factor<true, MODE_FACTOR>"], "P": ["k_factor<true, MODE_PREDICT>"], "gram": ["k_gram_big"],
                 "sweep": ["k_sample<true, false>"]}),
    # an 88-row root (the LDS generic kernels: wider than k_factor_bigmfma's 80 columns, small enough for LDS), 88- and
    # 75-row reference levels below it on the big path, a 59-column leaf level with P = 251 on k_sample<false>, NA
    # blocks with P = 251 on the LDS generic predict kernel; mixed levels, so k_gram_big writes both triangles
    dict(id="generic_lds", strip=(80, 10, 1), kw=dict(cell_size=(11, 10), tree_depth=3, missing=0.1), env={}, mirror=1,
         routes={"A": ["k_factor<false, MODE_FACTOR>"], "P": ["k_factor<false, MODE_PREDICT>"], "sweep": ["k_sample<false>"],
                 "gram": ["k_gram_big"]}),
    # 16-row reference levels on the column-group kernels above a leftover leaf level of 127-row blocks on the big path:
    # k_gram_big writes both triangles (mirror = 1) for the column-group parents that read them
    dict(id="mixed_colgroup_big_leaf", side=48, kw=dict(cell_size=16, tree_depth=3, missing=0.1), env={}, mirror=1,
         routes={"A": ["k_factor<true, MODE_FACTOR>"], "gram": ["k_gram_big"], "leaf_rebuild": ["k_sample<true, true>"],
                 "leaf_cached": ["k_sample<true, true>"]}),
    # limited_tree: one parent per block, the chain factors of the marginal covariances; 25-row reference blocks one per
    # wave, 63-69-row ones on the workgroup kernel
    dict(id="limited_wave", side=25, kw=dict(missing=0.1, limited_tree=True), env={}, routes={"A": ["k_marginal_invchol_wave"]}),
    dict(id="limited_wide", side=14, q=3, kw=dict(missing=0.1, limited_tree=True), env={}, routes={"A": ["k_marginal_invchol"]}),
]


def build_problem(row):
    if "side" in row:
        return make_problem(side=row["side"], q=row.get("q", 1), seed=11, **row["kw"])
    nx, ny, q = row["strip"]
    coords, mv = strip_coords(nx, ny, q)
    return make_problem(coords=coords, mv_id=mv, q=q, seed=11, K=(2, 1), **row["kw"])


def hip_model(pb, force_generic=False, **kw):
    """beta: p values for every outcome, or p x q (one column per outcome); tausq: one value, or q."""
    from spamtree_amd.model import SpamTreeMV
    beta, tausq = np.asarray(kw["beta"], dtype=np.float64), np.asarray(kw["tausq"], dtype=np.float64)
    hm = SpamTreeMV(pb["y"], pb["X"], pb["Z"], pb["coords"], pb["mv_id"], pb["blocking"], pb["gix_block"],
                    pb["res_is_ref"], pb["parents"], pb["children"], pb.get("limited_tree", False), pb["block_names"],
                    pb["block_groups"], pb["indexing"], kw["w"], beta[:, 0] if beta.ndim == 2 else beta, kw["theta"],
                    1.0 / float(tausq.ravel()[0]), force_generic=force_generic)
    if beta.ndim == 2:
        hm.beta_update(beta)
    if tausq.ndim > 0:
        hm.tausq_inv = 1.0 / tausq
        hm._check(hm.lib.st_set_tausq_inv(hm.h, hm.tausq_inv.ctypes.data_as(hm.lib.st_set_tausq_inv.argtypes[1])))
    return hm


def inputs(pb):
    rng = np.random.default_rng(7)
    return dict(w=rng.standard_normal(pb["n"]), beta=np.array([0.3, -0.2, 0.1]), tausq=0.2, theta=pb["theta"],
                theta2=pb["theta"] * (1.0 + 0.05 * rng.standard_normal(pb["theta"].size)),
                zs=[rng.standard_normal(pb["n"]) for _ in range(5)])


def run_device(pb, inp, force_generic=False):
    """The whole protocol on the device; returns its outputs and the routes every step took."""
    hm = hip_model(pb, force_generic=force_generic, **inp)
    routes = {k: set() for k in ("A", "gram", "sweep", "rebuild", "cached", "leaf_rebuild", "leaf_cached", "P")}
    trace = {}      # route_info() of phase A (slot 0), of the first rebuild sweep and of the first cached sweep, per level

    def note(sweep=None):
        r = hm.route_info()
        trace.setdefault(sweep or "A", r["levels"])
        if sweep in ("rebuild", "cached") and r["levels"][-1]["sweep"]:
            routes["leaf_" + sweep].add(r["levels"][-1]["sweep"])
        for L in r["levels"]:
            if sweep is None:
                routes["A"].update(L["A"])
            else:
                if L["gram"]:
                    routes["gram"].add(L["gram"])
                if L["sweep"]:
                    routes["sweep"].add(L["sweep"])
                    if sweep in ("rebuild", "cached"):
                        routes[sweep].add(L["sweep"])
        if r["predict"]:
            routes["P"].add(r["predict"])

    out = dict(blocks=[{}, {}], levels=hm.level_info())
    out["leaf_P"] = out["levels"][-1]["max_P"]
    has_pred = bool(np.any(~np.isfinite(pb["y"])))
    assert hm.get_loglik_comps_w(0)
    note()
    hm.theta_update(1, inp["theta2"])
    assert hm.get_loglik_comps_w(1)
    note()
    out["loglik_A"] = list(hm.loglik_w)
    out["comps"] = [hm.comps(0), hm.comps(1)]
    observed = [u for u, ix in enumerate(pb["indexing"]) if np.isfinite(pb["y"][ix]).any()]
    for slot in (0, 1):
        for u in observed:
            out["blocks"][slot][u] = hm.block(slot, u)
    ws, lls, ll_comps, xty, ssq = [], [], [], [], []

    def sweep(it):
        hm.deal_with_w(inp["zs"][it])
        note("rebuild" if it in (0, 3) else "cached")
        ws.append(hm.get_w().copy())
        lls.append(hm.get_loglik_w(0))
        ll_comps.append(hm.comps(0)[1].copy())
        st = hm.stats()
        xty.append(st[0])
        ssq.append(st[1])

    for it in range(3):
        sweep(it)
    if has_pred:
        hm.predict(True)
        note("predict")
        ws.append(hm.get_w().copy())
    hm.accept_make_change()
    for it in (3, 4):
        sweep(it)
    if has_pred:
        hm.predict(True)
        ws.append(hm.get_w().copy())
    hm.close()
    out.update(ws=ws, lls=lls, ll_comps=ll_comps, xty=xty, ssq=ssq, routes=routes, trace=trace)
    return out


def relerr(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    if a.size == 0:
        return 0.0
    return float(np.abs(a - b).max() / max(1e-300, np.abs(b).max()))


_ORACLE = {}     # oracle outputs of the protocol, per problem: rows that differ only in environment or options share one run


def oracle_protocol(pb, inp):
    """The protocol of run_device on the NumPy oracle."""
    om = oracle_model(pb, w=inp["w"], beta=inp["beta"], tausq=inp["tausq"])
    assert om.get_loglik_comps_w(om.param_data)
    om.theta_update(om.alter_data, inp["theta2"])
    assert om.get_loglik_comps_w(om.alter_data)
    ref = dict(slots=[], steps=[])
    for pd in (om.param_data, om.alter_data):
        blocks = {}
        for u in range(om.n_blocks):
            if om.block_ct_obs[u] == 0:
                continue
            blocks[u] = (pd.w_cond_mean_K[u] if om.parents[u].size else None,
                         pd.Rcc_invchol[u] if om.block_is_reference[u] else pd.ccholprecdiag[u])
        ref["slots"].append(dict(loglik_w=pd.loglik_w, logdet=pd.logdetCi_comps.copy(), loglik=pd.loglik_w_comps.copy(),
                                 blocks=blocks))
    has_pred = bool(np.any(~np.isfinite(pb["y"])))
    na_ix = om.na_ix_all

    def sweep(z):
        om.gibbs_sample_w(z)
        om.get_loglik_w(om.param_data)
        pd = om.param_data
        xty, ssq = om.beta_tausq_stats()
        ref["steps"].append(dict(kind="sweep", w=om.w[na_ix].copy(), loglik_w=pd.loglik_w, loglik=pd.loglik_w_comps.copy(),
                                 terms=np.abs(pd.logdetCi_comps).sum() + np.abs(pd.loglik_w_comps).sum(), xty=xty, ssq=ssq))

    def predict():
        om.predict(True)
        ref["steps"].append(dict(kind="predict", w=om.w.copy()))

    for it in range(3):
        sweep(inp["zs"][it])
    if has_pred:
        predict()
    om.accept_make_change()
    for it in (3, 4):
        sweep(inp["zs"][it])
    if has_pred:
        predict()
    ref["na_ix"] = na_ix
    return ref


def compare_with_oracle(pb, inp, out, key=None, record=None):
    """out (run_device) against the oracle's run of the same protocol; `key`: the problem's key in the shared cache;
    `record`: a dict that takes the largest error met per compared quantity (each figure goes in before it is asserted)."""
    ref = _ORACLE.get(key) if key is not None else None
    if ref is None:
        ref = oracle_protocol(pb, inp)
        if key is not None:
            _ORACLE[key] = ref

    def held(name, err, bound, ctx):
        if record is not None:
            record[name] = max(record.get(name, 0.0), float(err))
        assert err <= bound, (name, ctx, err)

    for slot, rs in enumerate(ref["slots"]):
        held("loglik_w phase A", abs(out["loglik_A"][slot] - rs["loglik_w"]) / max(1e-300, abs(rs["loglik_w"])), REL, slot)
        ld, ll = out["comps"][slot]
        held("logdet components", relerr(ld, rs["logdet"]), REL, slot)
        held("loglik components", relerr(ll, rs["loglik"]), REL, slot)
        for u, (H_ref, Ri_ref) in rs["blocks"].items():
            H, Ri = out["blocks"][slot][u]
            if H_ref is not None:
                held("H", relerr(H, H_ref), REL_H, (slot, u))
            held("Ri", relerr(Ri, Ri_ref), REL, (slot, u))
    ws, lls, ll_comps = list(out["ws"]), list(out["lls"]), list(out["ll_comps"])
    xty, ssq = list(out["xty"]), list(out["ssq"])
    for k, st in enumerate(ref["steps"]):
        if st["kind"] == "predict":
            held("w after st_predict", relerr(ws.pop(0), st["w"]), REL, k)
            continue
        held("w after a sweep", relerr(ws.pop(0)[ref["na_ix"]], st["w"]), REL, k)
        # per block, then the sum: loglik_w = sum(logdetCi_comps) + sum(loglik_w_comps).  After a sweep the quadratic forms of
        # the posterior draw can nearly cancel the log-determinants (the 256-row leaf chains after an accepted theta:
        # loglik_w = 104 from terms whose magnitudes sum to more than 2.5e4), so the sum is held to REL relative to the
        # terms it adds up, not to its own small value
        held("loglik components of a sweep", relerr(ll_comps.pop(0), st["loglik"]), REL, k)
        held("loglik_w of a sweep / terms", abs(lls.pop(0) - st["loglik_w"]) / max(1e-300, abs(st["loglik_w"]), st["terms"]), REL, k)
        # the sufficient statistics of the beta / tausq updates, reduced on the device from the draw
        held("beta statistics", relerr(xty.pop(0), st["xty"]), REL, k)
        held("tausq statistics", relerr(ssq.pop(0), st["ssq"]), REL, k)
    assert not ws and not lls and not ll_comps and not xty and not ssq


# the sweep kernels of levels on the big (scratch-arena) path: a rebuild sweep forms their Gram parts with k_gram_big
BIG_SWEEP = {"k_sample<true, false>", "k_sample<true, true>", "k_sample_leaf_wide"}
# the chain lengths (P) and block widths (m) each phase-A kernel is dispatched at (st_factor.hip, factor_launch and the
# level geometry: k_factor_quad P <= 200, the column-group path P <= 256, k_factor_lchain<96> / <136> P <= 384 / <= 544,
# k_factor_bigmfma by width: <= 48, <= 64, <= 80 columns)
A_BOUNDS = {
    "k_factor_mfma": dict(P=(0, 256), m=(0, 32)),
    "k_factor_lchain<96>": dict(P=(1, 384), m=(1, 80)),
    "k_factor_lchain<136>": dict(P=(385, 544), m=(1, 80)),
    "k_factor_bigmfma<3, 5, 34>": dict(P=(0, 544), m=(1, 48)),
    "k_factor_bigmfma<4, 5, 34>": dict(P=(0, 544), m=(49, 64)),
    "k_factor_bigmfma<5, 3, 24>": dict(P=(0, 544), m=(65, 80)),
}


def check_routes(row, routes):
    for key, names in row["routes"].items():
        for name in names:
            assert name in routes[key], (row["id"], key, name, sorted(routes[key]))
    for key, names in row.get("not_routes", {}).items():
        for name in names:
            assert name not in routes[key], (row["id"], key, name, sorted(routes[key]))


def check_levels(row, out, pb):
    """The dispatch conditions, from level_info and the per-level routes: every phase-A kernel ran inside its bounds; the
    row's `at` entries (kernel, lo, hi: a level of chains of lo..hi rows on that kernel) are met; `mirror`: the mode of
    k_gram_big, which writes both triangles of the Gram parts (1) unless every observed level is on the big path (0).  The mode
    is asserted here because the draws cannot show it: every kernel that adds a record's Gram part to a posterior precision
    reads its lower triangle only (the column-group kernels forward the upper one, and nothing reads it)."""
    info, trace = out["levels"], out["trace"]
    assert len(info) == len(trace["A"])
    for g, (L, r) in enumerate(zip(info, trace["A"])):
        for name in r["A"]:
            for dim, (lo, hi) in A_BOUNDS.get(name, {}).items():
                v = L["max_" + dim]
                assert lo <= v <= hi, (row["id"], g, name, dim, v)
        for k in ("rebuild", "cached"):
            if trace[k][g]["sweep"] == "k_sample_leaf_wide":
                assert L["max_m"] <= 64, (row["id"], g, L)
    for name, lo, hi in row.get("at", []):
        hits = [L["max_P"] for L, r in zip(info, trace["A"]) if name in r["A"]]
        assert any(lo <= P <= hi for P in hits), (row["id"], name, lo, hi, hits)
    if "mirror" in row:
        rebuild = trace["rebuild"]
        assert any(L["gram"] == "k_gram_big" for L in rebuild), (row["id"], rebuild)
        all_big = all(L["sweep"] in BIG_SWEEP for L in rebuild if L["sweep"])
        assert all_big == (row["mirror"] == 0), (row["id"], [L["sweep"] for L in rebuild])
    if "leaf_maxMa" in row:     # the widest ancestor of the leaf level's blocks (the geometry of spamtree_hip.hip)
        grp = np.asarray(pb["block_groups"])
        obs = [u for u, ix in enumerate(pb["indexing"]) if np.isfinite(pb["y"][ix]).any()]
        leaf = [u for u in obs if grp[u] == grp[obs].max()]
        maxMa = max(len(pb["indexing"][a]) for u in leaf for a in pb["parents"][u])
        assert maxMa == row["leaf_maxMa"], (row["id"], maxMa)


def problem_key(row):
    return repr((row.get("side"), row.get("q", 1), row.get("strip"), sorted(row["kw"].items())))


@pytest.mark.parametrize("row", ROUTES + WIDE_ROUTES, ids=[r["id"] for r in ROUTES + WIDE_ROUTES])
def test_route_matches_oracle(row, monkeypatch):
    for k, v in row["env"].items():
        monkeypatch.setenv(k, v)
    pb = build_problem(row)
    inp = inputs(pb)
    out = run_device(pb, inp, force_generic=row.get("force_generic", False))
    check_routes(row, out["routes"])
    check_levels(row, out, pb)
    assert out["leaf_P"] >= row.get("leaf_P_min", 0), (row["id"], out["leaf_P"])
    compare_with_oracle(pb, inp, out, key=problem_key(row))


# ---- k_sample_lean<false>: the same row with SPAMTREE_SAMPLE_LAT=0, then without it (each handle reads its own switches)
LEAN_ROW = ROUTES[0]


def test_lean_sample_without_latency_variant_matches_oracle_and_is_bitwise_lean_true(monkeypatch):
    for k, v in LEAN_ROW["env"].items():
        monkeypatch.setenv(k, v)
    pb = build_problem(LEAN_ROW)
    inp = inputs(pb)
    monkeypatch.setenv("SPAMTREE_SAMPLE_LAT", "0")
    lean = run_device(pb, inp)
    assert "k_sample_lean<false>" in lean["routes"]["sweep"] and "k_sample_lean<true>" not in lean["routes"]["sweep"]
    monkeypatch.delenv("SPAMTREE_SAMPLE_LAT")
    out = run_device(pb, inp)      # the latency variant on the same levels
    assert "k_sample_lean<true>" in out["routes"]["sweep"]
    for k in ("ws", "lls", "ll_comps", "xty", "ssq"):
        assert np.array_equal(np.array(lean[k]), np.array(out[k])), k
    compare_with_oracle(pb, inp, lean, key=problem_key(LEAN_ROW))


# ---- config #2 at full size (n = 99 856, bench.py --side 316) on its default routes, against oracle/refcpu
CONFIG2_ROUTES = {
    "A": [quad(32, True, True), quad(38, False, True)],    # the 1 024-block reference level (P = 125) / the leaf level (P = 150)
    "sweep": ["k_sample_lean<false>"],                       # that reference level: more groups than 2 x CUs
}


def test_config2_full_size_default_routes_match_refcpu():
    from oracle.refcpu import RefCpu
    from spamtree_amd.model import SpamTreeMV
    from spamtree_amd.synthetic import make_workload
    wl = make_workload(316)
    beta = np.array([-0.5, 0.2, 0.4])
    rng = np.random.default_rng(9)
    w0 = rng.standard_normal(wl["n"])
    th2 = wl["theta"] * (1.0 + 0.05 * rng.standard_normal(wl["theta"].size))
    zs = [rng.standard_normal(wl["n"]) for _ in range(3)]
    hm = SpamTreeMV(wl["y"], wl["X"], wl["Z"], wl["coords"], wl["mv_id"], wl["blocking"], wl["gix_block"], wl["res_is_ref"],
                    wl["parents"], wl["children"], False, wl["block_names"], wl["block_groups"], wl["indexing"], w0, beta,
                    wl["theta"], 1.0 / 0.15)
    info = hm.level_info()
    assert hm.get_loglik_comps_w(0)
    ra = hm.route_info()["levels"]
    comps = hm.comps(0)
    draws = []
    for z in zs[:2]:
        hm.deal_with_w(z)
        draws.append((hm.get_w().copy(), hm.get_loglik_w(0)))
    rb = hm.route_info()["levels"]          # the second sweep: cached Gram parts
    stats = hm.stats()
    hm.theta_update(1, th2)
    assert hm.get_loglik_comps_w(1)
    ll2 = hm.loglik_w[1]
    hm.accept_make_change()
    hm.deal_with_w(zs[2])
    draws.append((hm.get_w().copy(), hm.get_loglik_w(0)))
    hm.close()
    # the routes first: the reference level of 1 024 blocks and the leaf level
    ref = [g for g, L in enumerate(info) if L["n_blocks"] == 1024]
    assert len(ref) == 1 and info[ref[0]]["max_P"] == 125
    leaf = len(info) - 1
    assert info[leaf]["max_P"] == 150
    assert ra[ref[0]]["A"] == [CONFIG2_ROUTES["A"][0]] and ra[leaf]["A"] == [CONFIG2_ROUTES["A"][1]]
    assert rb[ref[0]]["sweep"] == CONFIG2_ROUTES["sweep"][0]
    rc = RefCpu(wl["y"], wl["X"], wl["coords"], wl["mv_id"], wl["res_is_ref"], wl["parents"], wl["children"],
                wl["block_names"], wl["block_groups"], wl["indexing"], threads=16)
    rc.set_w(w0); rc.set_beta(beta[:, None]); rc.set_tausq_inv(1.0 / 0.15)
    code, ll = rc.factor(0, wl["theta"])
    assert code == 0
    ld, lc = rc.comps(0)
    assert relerr(comps[0], ld) <= REL and relerr(comps[1], lc) <= REL
    obs = np.isfinite(wl["y"])
    for it in range(2):
        assert rc.sample_w(zs[it]) == 0
        assert relerr(draws[it][0][obs], rc.get_w()[obs]) <= REL, it
        assert abs(draws[it][1] - rc.loglik_w(0)) <= REL * abs(rc.loglik_w(0)), it
    rxty, rssq = rc.stats()
    assert relerr(stats[0], rxty) <= REL and relerr(stats[1], rssq) <= REL
    code, rll2 = rc.factor(1, th2)
    assert code == 0 and abs(ll2 - rll2) <= REL * abs(rll2)
    rc.swap()
    assert rc.sample_w(zs[2]) == 0
    assert relerr(draws[2][0][obs], rc.get_w()[obs]) <= REL
    assert abs(draws[2][1] - rc.loglik_w(0)) <= REL * abs(rc.loglik_w(0))
    rc.close()


# ---- k_gram_direct eligibility: a leaf block whose last parent is one level above the last reference level
def shallow_leaf_problem():
    """CASES[0] of test_gpu_parity (four levels, the last one the leaf level) with one leaf block re-hung: its parent on the
    last reference level is dropped (parents and children stay consistent), so its direct parent lies one level higher."""
    pb = make_problem(side=25, q=1, seed=53)
    par = [p.copy() for p in pb["parents"]]
    ch = [c.copy() for c in pb["children"]]
    grp = pb["block_groups"]
    leaf = [u for u in range(len(par)) if grp[u] == grp.max() and len(pb["indexing"][u])]
    u = leaf[len(leaf) // 2]
    gp = par[u][-1]
    assert grp[gp] == grp.max() - 1
    par[u] = par[u][:-1]
    ch[gp] = ch[gp][ch[gp] != u]
    assert grp[par[u][-1]] == grp.max() - 2
    pb.update(parents=par, children=ch)
    return pb


@pytest.mark.parametrize("direct", [None, "0"])
def test_gram_direct_with_a_leaf_below_a_shallower_parent(direct, monkeypatch):
    """k_gram_direct lets the last reference level form its children's Gram parts, and the leaf level then writes none.  A
    leaf whose direct parent is shallower would leave that parent's Gram part unwritten: such a tree must keep k_gram (the
    draws differed from the oracle while the eligibility check looked at the last reference level's children only)."""
    monkeypatch.setenv("SPAMTREE_SPLIT_GRAM", "2")
    if direct is None:
        monkeypatch.delenv("SPAMTREE_GRAM_DIRECT", raising=False)
    else:
        monkeypatch.setenv("SPAMTREE_GRAM_DIRECT", direct)
    pb = shallow_leaf_problem()
    inp = inputs(pb)
    out = run_device(pb, inp)
    assert "k_gram" in out["routes"]["gram"]
    assert "k_gram_direct" not in out["routes"]["gram"]    # the last reference level does not hold every leaf's parent
    compare_with_oracle(pb, inp, out)
