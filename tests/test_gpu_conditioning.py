"""GPU: the phase-A and sweep kernels against an extended-precision reference at ill-conditioned theta.

Every other kernel-vs-oracle test runs at nice_theta, where the float64 oracle is accurate to ~1e-14.  At the bottom of the
bounds (phi = 1e-3) K_pa is nearly singular and R = K_uu - V'V cancels: the oracle itself keeps ~6 digits (measured on
make_problem(side=25, q=1, seed=11): Ri 1.3e-6, N 2.1e-6, logdet 1.4e-5 nats; tests/test_extended_reference.py), so
REL = 1e-9 against it says nothing.  The question asked here is whether each kernel loses no more than LAPACK does on the
same problem, with oracle/extended.py (80-bit long double, no LAPACK) as the yardstick:

  for each level l and X in {N (the stored panel -Ri H), Ri (reference) / 1/sqrt(r_ii) (non-reference), logdet component,
  loglik_w component}:  e_dev(l) = max over the level's checked blocks of |X_dev - X_ext|_max / |X_ext|_max (the scalar
  components as one vector per level), e_64(l) the same for the float64 oracle, and e_dev(l) <= C max(e_64(l), 64 eps).

Rows are those of tests/test_gpu_routes.py (ROUTES / WIDE_ROUTES, by id, with their environments); each case first runs the
route table's device protocol at its theta and asserts check_routes, so the row still reaches its instantiations there.
Phase A is read from both slots (factorised at the same theta); the stored panel and Ri come from st_get_block unchanged
(SpamTreeMV.block(raw=True)).  Sweep: one sweep with z = 0 from w0; the draws of the deepest observed level are compared with
the full conditional mean given w0, those of the level above with the mean given w0 and the device's new leaf values
(ExtendedBlocks.cond_mean); the oracle's error is that of om.gibbs_sample_w(zeros) from the same w0.  The sweep therefore
covers the leaf and reference-level sweep kernels each row reaches (route keys "sweep" / "rebuild" of the route table:
k_sample_leaf_seg, k_sample_lean, k_sample_wave, k_sample<...>, k_sample_leaf_wide) and, on its first sweep, the Gram kernels
(k_gram, k_gram_big).

Theta regimes: q = 1 control (nice_theta), phi_mid (0.05), phi_low (1e-3, the lower bound), phi_high (1e3, the upper bound:
K nearly diagonal but -phi h down to ~ -1400, the subnormal and zero paths of the exponentials); near: nice_theta with 5 % of
the rows moved to within 1e-7 of another row of the same outcome in the same block.  q >= 2: control, low (every phi_i and
the AG10 rate at 1e-3), cross (Dmat entries 1e-3 and ai2 = 1e-2 ai1: co-located outcomes, nearly singular q x q blocks).

Failure decision: where the device reports success every stored value is finite; where the extended reference's smallest
relative Schur pivot (min pivot / max K_ii over the checked blocks) is above 1e-10 the device must succeed; below, either
outcome is allowed.  Up to NMAX blocks per level are checked (evenly spaced), so the reference stays within the runtime:
the whole file, oracle and extended reference included, takes about 30 s on an MI355X host (46 cases).

Where this departs from the plain reading of its specification: the near-coincident regime perturbs each row's own problem
(make_problem(random_coords=True) would build a different tree, and the row would lose its routes); the conditioning of a
case is reported as its smallest relative Schur pivot, which is what decides the failure band, not as a condition number;
the scalar components are compared per level with the floor 64 eps max|component|, not the looser 64 eps sum|terms| of the
total loglik_w, which is not compared separately (it is the sum of the per-block components compared here).

Shown to catch real errors (local, uncommitted builds, the whole file each time):
  - cov_exp_tab's polynomial one degree short (~4e-14 per entry): test_gpu_device_math fails, and so does the control case
    of every k_factor_quad row (ratios 13-157) and of wide4_default_pred, whose k_factor_lchain levels use the same
    exponential (ratio 100); the rest of the GPU suite stays green.  phi_mid, phi_low and phi_high cannot catch it: at
    phi_mid / phi_low the oracle's own error (>= 1e-9) is far
    above 4e-14, and at phi_low |phi h| <= 1.4e-3 < ln2/128, so t = 0, r = x and the dropped r^5/120 is below 5e-17, under
    half an ulp of the result; at phi_high the off-diagonal entries that carry the error are negligible;
  - cov_sqrt without its residual correction: test_gpu_device_math fails (this file does not: 4e-15 per distance);
  - R = K_uu - V'V with V'V summed in float32 in the generic factor kernel (k_factor<...>): every grid_generic and
    wide4_generic case but phi_high fails (ratios 4e3 to 9e7; e_dev up to 0.4 at near, 2.6e-2 at phi_low), and at
    wide4_generic-low the device refuses a factorisation whose smallest relative pivot is 5.9e-7.

Observed on an MI355X (every case succeeded on the device and in the oracle): the smallest relative Schur pivot of the
checked blocks, the worst oracle error e_64 and device error e_dev over slots, levels and quantities, and the worst ratio
e_dev / max(e_64, 64 eps).  The device is often far more accurate than the oracle (which forms K_pa^-1 explicitly):
  row                      regime     pivot    e_64     e_dev    ratio
  ref30_leaf50_pred50      control    9.3e-03  6.4e-11  3.7e-13   1.83
  ref30_leaf50_pred50      phi_mid    7.7e-05  8.2e-07  4.6e-11   2.55
  ref30_leaf50_pred50      phi_low    1.5e-06  4.3e-03  2.0e-09   0.64
  ref30_leaf50_pred50      phi_high   9.2e-01  3.0e-15  2.9e-15   0.20
  ref32_nkx44              control    3.3e-03  3.4e-11  5.9e-13   1.57
  ref32_nkx44              low        6.8e-07  9.2e-04  1.9e-09   3.99
  ref32_nkx44              cross      3.6e-05  6.3e-07  1.1e-10   1.38
  ref25_wch_nkx44          control    4.7e-03  2.8e-10  6.9e-13   1.57
  ref25_wch_nkx44          phi_mid    3.9e-05  5.0e-06  9.9e-11   0.62
  ref25_wch_nkx44          phi_low    7.8e-07  1.7e-02  4.8e-09   1.34
  ref25_wch_nkx44          phi_high   6.5e-01  3.6e-15  4.1e-15   0.29
  leaf38_pred38_wave       control    9.3e-03  8.4e-11  3.7e-13   0.84
  leaf38_pred38_wave       phi_mid    7.8e-05  7.6e-07  5.0e-11   3.19
  leaf38_pred38_wave       phi_low    1.6e-06  1.6e-03  2.3e-09   1.02
  leaf38_pred38_wave       phi_high   9.2e-01  3.1e-15  3.1e-15   0.22
  grid_leaf32_pred32       control    1.9e-01  1.5e-14  6.0e-15   0.42
  grid_leaf32_pred32       phi_mid    1.6e-03  1.4e-09  1.6e-12   0.65
  grid_leaf32_pred32       phi_low    3.2e-05  2.3e-06  9.7e-11   0.90
  grid_leaf32_pred32       phi_high   1.0e+00  6.7e-15  6.3e-15   0.44
  grid_leaf32_pred32       near       6.4e-08  1.0e-03  6.5e-07   1.77
  cfg5_mfma_chains_pred    control    1.3e-03  2.5e-10  1.5e-12   2.20
  cfg5_mfma_chains_pred    low        3.4e-07  4.2e-03  6.3e-09   1.20
  cfg5_mfma_chains_pred    cross      4.5e-06  2.5e-05  4.9e-10   1.57
  wide4_default_pred       control    2.4e-03  3.1e-10  1.2e-12   2.59
  wide4_default_pred       low        5.9e-07  1.1e-02  7.7e-09   4.85
  wide4_default_pred       cross      8.0e-06  2.5e-05  8.6e-10   8.32
  wide4_bigmfma            control    2.4e-03  3.1e-10  1.1e-12   2.59
  wide4_bigmfma            low        5.9e-07  1.1e-02  8.7e-09   4.85
  wide4_bigmfma            cross      8.0e-06  2.5e-05  5.7e-10   8.32
  wide4_sibling_groups     control    2.4e-03  3.1e-10  1.2e-12   2.59
  wide4_sibling_groups     low        5.9e-07  1.1e-02  7.0e-09   4.85
  wide4_sibling_groups     cross      8.0e-06  2.5e-05  6.4e-10   8.32
  grid_generic             control    1.9e-01  1.5e-14  7.4e-15   0.52
  grid_generic             phi_mid    1.6e-03  1.4e-09  1.5e-12   0.55
  grid_generic             phi_low    3.2e-05  2.3e-06  9.0e-11   1.04
  grid_generic             phi_high   1.0e+00  6.7e-15  6.8e-15   0.48
  grid_generic             near       6.4e-08  1.0e-03  6.7e-07   0.88
  wide4_generic            control    2.4e-03  3.1e-10  1.1e-12   3.13
  wide4_generic            low        5.9e-07  1.1e-02  4.1e-09   4.19
  wide4_generic            cross      8.0e-06  2.5e-05  4.8e-10  11.51
  limited_wave             control    2.1e-01  3.6e-15  4.5e-15   0.32
  limited_wave             phi_mid    1.7e-03  2.4e-10  9.2e-13   0.65
  limited_wave             phi_low    3.5e-05  3.6e-07  5.2e-11   0.90
  limited_wave             phi_high   1.0e+00  6.9e-15  7.3e-15   0.51
  limited_wave             near       6.4e-08  9.9e-04  1.9e-07   1.16
  limited_wide             control    7.9e-02  9.3e-15  6.0e-15   0.42
  limited_wide             low        2.0e-05  2.5e-07  3.4e-11   2.11
  limited_wide             cross      2.8e-04  1.4e-10  2.6e-12   2.72
"""
import numpy as np
import pytest

from tests.test_gpu_routes import ROUTES, WIDE_ROUTES, build_problem, check_routes, hip_model, inputs, run_device
from tests.util import nice_theta, oracle_model

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
C_BOUND = 8.0
# raised bounds, keyed (row prefix, regime, level, quantity).  The loglik_w component of the root block of config #4's shape
# (75 rows, q = 3, no parent) at the cross regime: measured e_dev / e_64 = 8.32 on both slots of wide4_default_pred,
# wide4_bigmfma and wide4_sibling_groups, and 11.5 on wide4_generic (e_dev ~1e-11).  The identical value on the first three
# is one path: a root level (P = 0, 75 columns) is factorised by k_factor_bigmfma's blocked epilogue on every non-generic
# row (st_factor.hip, the level dispatch), which also forms the quadratic form |Ri w|^2; wide4_generic runs the root on
# k_factor<true, MODE_FACTOR>.  Every other level, regime and quantity of these rows keeps C_BOUND.
C_FAMILY = {("wide4", "cross", 0, "loglik"): 16.0}
NMAX = 6
PIVOT_BAND = 1e-10
ROW = {r["id"]: r for r in ROUTES + WIDE_ROUTES}

Q1_REGIMES = ["control", "phi_mid", "phi_low", "phi_high"]
QM_REGIMES = ["control", "low", "cross"]
CASES = [
    ("ref30_leaf50_pred50", Q1_REGIMES), ("ref32_nkx44", QM_REGIMES), ("ref25_wch_nkx44", Q1_REGIMES),
    ("leaf38_pred38_wave", Q1_REGIMES), ("grid_leaf32_pred32", Q1_REGIMES + ["near"]), ("cfg5_mfma_chains_pred", QM_REGIMES),
    ("wide4_default_pred", QM_REGIMES), ("wide4_bigmfma", QM_REGIMES), ("wide4_sibling_groups", QM_REGIMES),
    ("grid_generic", Q1_REGIMES + ["near"]), ("wide4_generic", QM_REGIMES), ("limited_wave", Q1_REGIMES + ["near"]),
    ("limited_wide", QM_REGIMES),
]
PARAMS = [(rid, reg) for rid, regs in CASES for reg in regs]


def regime_theta(q, regime):
    th = nice_theta(q).copy()
    if q == 1:
        th[3] = {"control": th[3], "near": th[3], "phi_mid": 0.05, "phi_low": 1e-3, "phi_high": 1e3}[regime]
        return th
    nc = 3 if q > 2 else 1
    if regime == "low":
        th[2 * q:3 * q] = 1e-3                  # phi_i
        th[3 * q + nc - 1] = 1e-3               # the AG10 rate (thetamv[2] for q > 2, thetamv[0] for q = 2)
    elif regime == "cross":
        th[q:2 * q] = 1e-2 * th[:q]             # ai2
        th[3 * q + nc:] = 1e-3                  # Dmat entries
    return th


def near_coincident(pb, frac=0.05, seed=5):
    """5 % of the rows moved to within 1e-7 of another row of the same outcome in the same block (the tree is unchanged)."""
    rng = np.random.default_rng(seed)
    coords = pb["coords"].copy()
    mv = pb["mv_id"]
    for ix in pb["indexing"]:
        for i in ix:
            if rng.uniform() >= frac:
                continue
            same = ix[(mv[ix] == mv[i]) & (ix != i)]
            if same.size:
                j = rng.choice(same)
                coords[i] = coords[j] + 1e-7 * rng.uniform(-1.0, 1.0, 2) / np.sqrt(2.0)
    return dict(pb, coords=coords)


_SHARED = {}      # (problem, regime) -> oracle, extended reference and their sweep results, shared by rows of one problem


def checked_blocks(om):
    """Up to NMAX evenly spaced observed blocks per level: {level: [blocks]}."""
    grp = np.asarray(om.block_groups)
    labels = np.unique(grp)
    out = {}
    for lv, lab in enumerate(labels):
        obs = [u for u in np.nonzero(grp == lab)[0] if om.block_ct_obs[u] > 0 and om.indexing[u].size]
        if obs:
            pick = np.unique(np.linspace(0, len(obs) - 1, min(NMAX, len(obs))).round().astype(int))
            out[lv] = [int(obs[k]) for k in pick]
    return out


def reference(key, pb, inp, theta):
    if key in _SHARED:
        return _SHARED[key]
    from oracle.extended import ExtendedBlocks
    om = oracle_model(pb, theta=theta, w=inp["w"], beta=inp["beta"], tausq=inp["tausq"])
    ok64 = om.get_loglik_comps_w(om.param_data)
    ex = ExtendedBlocks(om, theta)
    levels = checked_blocks(om)
    blocks = [u for us in levels.values() for u in us]
    ext = {u: ex.block(u) for u in blocks}
    min_pivot = min(ext[u]["min_pivot"] for u in blocks)
    ref = dict(om=om, ok64=ok64, ex=ex, levels=levels, ext=ext, min_pivot=min_pivot, o64={}, sweep=None)
    if ok64:
        pd = om.param_data
        for u in blocks:
            H = pd.w_cond_mean_K[u] if om.parents[u].size else np.zeros((om.indexing[u].size, 0))
            if ext[u]["isref"]:
                Ri = pd.Rcc_invchol[u]
                N = -Ri @ H
            else:
                Ri = pd.ccholprecdiag[u]
                N = -Ri[:, None] * H
            ref["o64"][u] = dict(N=N, Ri=Ri, logdet=pd.logdetCi_comps[u], loglik=pd.loglik_w_comps[u])
        try:
            om.gibbs_sample_w(np.zeros(pb["n"]))
            ref["w64"] = om.w.copy()
            if np.any(om.block_ct_obs[[u for u in range(om.n_blocks) if om.indexing[u].size]] == 0):
                om.predict(True)          # the rows without observations, from the same z = 0 (predict_errors)
                ref["w64p"] = om.w.copy()
        except RuntimeError:
            ref["w64"] = None
    _SHARED[key] = ref
    return ref


def err(a, b):
    a = np.asarray(a, dtype=np.longdouble).ravel()
    b = np.asarray(b, dtype=np.longdouble).ravel()
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)) if b.size else 0.0


def level_errors(ref, dev):
    """{(level, X): (e_dev, e_64)} over the checked blocks."""
    out = {}
    for lv, us in ref["levels"].items():
        ext = ref["ext"]
        X_ext = dict(N=[ext[u]["N"] for u in us], Ri=[ext[u]["Ri"] if ext[u]["isref"] else ext[u]["d"] for u in us],
                     logdet=[ext[u]["logdet"] for u in us],
                     loglik=[ref["ex"].loglik_comp(u, ref["w0"])[1] for u in us])
        for X, xs in X_ext.items():
            if X == "N":
                e_d = max(err(dev[u]["N"], x) for u, x in zip(us, xs))
                e_o = max(err(ref["o64"][u]["N"], x) for u, x in zip(us, xs))
            elif X == "Ri":
                e_d = max(err(dev[u]["Ri"], x) for u, x in zip(us, xs))
                e_o = max(err(ref["o64"][u]["Ri"], x) for u, x in zip(us, xs))
            else:
                e_d = err([dev[u][X] for u in us], xs)
                e_o = err([ref["o64"][u][X] for u in us], xs)
            out[(lv, X)] = (e_d, e_o)
    return out


def sweep_errors(ref, w_dev):
    """{(level, "sweep"): (e_dev, e_64)} for the deepest observed level and the one above."""
    om, ex, w0 = ref["om"], ref["ex"], ref["w0"]
    lvs = sorted(ref["levels"])[-2:]
    out = {}
    w_mix = w0.copy()
    deepest = lvs[-1]
    grp = np.asarray(om.block_groups)
    labels = np.unique(grp)
    for u in np.nonzero(grp == labels[deepest])[0]:
        if om.block_ct_obs[u] > 0:
            w_mix[om.indexing[u]] = w_dev[om.indexing[u]]
    for lv in reversed(lvs):
        us = ref["levels"][lv]
        base = w0 if lv == deepest else w_mix
        mean = np.concatenate([np.asarray(ex.cond_mean(u, base), dtype=np.longdouble) for u in us])
        rows = np.concatenate([om.indexing[u] for u in us])
        e_d = err(w_dev[rows], mean)
        e_o = err(ref["w64"][rows], mean) if ref.get("w64") is not None else np.inf
        out[(lv, "sweep")] = (e_d, e_o)
    return out


def predict_errors(ref, w_dev):
    """{("P", "predict"): (e_dev, e_64)}: the rows of up to NMAX blocks without observations after st_predict with z = 0, each
    against ExtendedBlocks.predict_draw given the same run's own values of the block's parents."""
    om, ex = ref["om"], ref["ex"]
    na = [u for u in range(om.n_blocks) if om.block_ct_obs[u] == 0 and om.indexing[u].size]
    if not na or ref.get("w64p") is None:
        return {}
    pick = np.unique(np.linspace(0, len(na) - 1, min(NMAX, len(na))).round().astype(int))
    e_d = e_o = 0.0
    for u in (na[k] for k in pick):
        iu = om.indexing[u]
        zero = np.zeros(iu.size)
        e_d = max(e_d, err(w_dev[iu], ex.predict_draw(u, w_dev, zero)))
        e_o = max(e_o, err(ref["w64p"][iu], ex.predict_draw(u, ref["w64p"], zero)))
    return {("P", "predict"): (e_d, e_o)}


def kernels_vs_extended(row, pb, inp, theta, regime, key, raised=C_FAMILY, predict=False):
    """The criterion of this file on one (row, regime): `row`'s environment is set by the caller, inp holds theta = theta2 =
    `theta`, `key` names the problem and regime in the shared cache of references.  `raised`: the raised bounds, keyed
    (row or row prefix, regime, level, quantity).  predict: also the rows without observations after st_predict (predict_errors).  Returns
    (smallest relative pivot, worst e_64, worst e_dev, worst ratio), or None where a refusal inside the band ended it."""
    rid = row["id"]
    ref = reference(key, pb, inp, theta)
    ref["w0"] = inp["w"]
    fg = row.get("force_generic", False)

    # the device: phase A on both slots, the stored blocks, one sweep with z = 0
    hm = hip_model(pb, force_generic=fg, **inp)
    try:
        ok = [hm.get_loglik_comps_w(0)]
        hm.theta_update(1, theta)
        ok.append(hm.get_loglik_comps_w(1))
        assert ok[0] == ok[1], ok
        if not ok[0]:
            assert ref["min_pivot"] <= PIVOT_BAND, (rid, regime, ref["min_pivot"], hm.last_errtype)
            print(f"{rid} {regime}: device refused (errtype {hm.last_errtype}), min pivot {ref['min_pivot']:.2e}")
            return None
        devs = []
        for slot in (0, 1):
            ld, ll = hm.comps(slot)
            dev = {}
            for u in ref["ext"]:
                N, Ri = hm.block(slot, u, raw=True)
                assert np.all(np.isfinite(N)) and np.all(np.isfinite(Ri)), (rid, regime, slot, u)
                dev[u] = dict(N=N, Ri=Ri, logdet=ld[u], loglik=ll[u])
            assert np.all(np.isfinite(ld)) and np.all(np.isfinite(ll)) and np.isfinite(hm.loglik_w[slot])
            devs.append(dev)
        hm.deal_with_w(np.zeros(pb["n"]))
        w_dev = hm.get_w().copy()
        w_pred = None
        if predict and np.any(~np.isfinite(pb["y"])):
            hm.predict(True)
            w_pred = hm.get_w().copy()
    finally:
        hm.close()

    # the row still reaches its instantiations at this theta (the route table's whole protocol)
    out = run_device(pb, inp, force_generic=fg)
    check_routes(row, out["routes"])

    if not ref["ok64"]:
        print(f"{rid} {regime}: the float64 oracle refused; device succeeded (min pivot {ref['min_pivot']:.2e})")
        return None
    errs = {}
    for slot, dev in enumerate(devs):
        for k, v in level_errors(ref, dev).items():
            errs[(slot,) + k] = v
    for k, v in sweep_errors(ref, w_dev).items():
        errs[(0,) + k] = v
    if w_pred is not None:
        assert np.all(np.isfinite(w_pred)), (rid, regime)
        for k, v in predict_errors(ref, w_pred).items():
            errs[(0,) + k] = v
    floor = 64 * EPS
    print(f"{rid} {regime}: min pivot {ref['min_pivot']:.2e}")
    for (slot, lv, X), (e_d, e_o) in sorted(errs.items(), key=str):
        print(f"  slot {slot} level {lv} {X:6s} e_dev {e_d:.2e} e_64 {e_o:.2e} ratio {e_d / max(e_o, floor):.2f}")
    fam = rid.split("_")[0]
    bad = {k: v for k, v in errs.items()
           if not v[0] <= raised.get((rid, regime, k[1], k[2]), raised.get((fam, regime, k[1], k[2]), C_BOUND)) * max(v[1], floor)}
    assert not bad, (rid, regime, bad)
    return (ref["min_pivot"], max(v[1] for v in errs.values()), max(v[0] for v in errs.values()),
            max(v[0] / max(v[1], floor) for v in errs.values()))


@pytest.mark.parametrize("rid,regime", PARAMS, ids=[f"{r}-{g}" for r, g in PARAMS])
def test_kernels_lose_no_more_than_lapack(rid, regime, monkeypatch):
    row = ROW[rid]
    for k, v in row["env"].items():
        monkeypatch.setenv(k, v)
    pb = build_problem(row)
    if regime == "near":
        pb = near_coincident(pb)
    theta = regime_theta(pb["q"], regime)
    inp = dict(inputs(pb), theta=theta, theta2=theta)
    key = (repr((row.get("side"), row.get("q", 1), row.get("strip"), sorted(row["kw"].items()))), regime)
    kernels_vs_extended(row, pb, inp, theta, regime, key)
