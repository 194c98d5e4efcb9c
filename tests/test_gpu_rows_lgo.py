"""GPU: leave-group-out criteria, a group's rows of the latent field integrated out jointly (st_rows_loo_groups_*, the pair part of
k_loo_block, k_lgo_groups / k_lgo_finish).

The references are tests/loo_reference.py (the DAG's precision from the dense covariance matrix: nothing of the device) and
tests/lgo_reference.py (one group's draw in long double).  The rounding bounds are those spamtree_amd/csrc/lgo_kernels.hpp derives.

Not verified here: the refusal of world > 1 handles -- the suite builds no such handle in a single process; it is st_rows_loo_set's,
which has to come first."""
import ctypes as C
import math

import numpy as np
import pytest

from spamtree_amd import loo
from tests import lgo_reference as gr
from tests import loo_reference as lr
from tests.test_gpu_rows_loo import LOO_CASES, fit_args, tausq_rows
from tests.test_gpu_simulate import hip_model
from tests.util import make_problem

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
ST_ERR_USAGE, ST_ERR_UNSUPPORTED = -1, -4
LOO_LAST = ("q_diag", "qw", "cond_mean", "cond_var")
LOO_OUT = ("elpd_loo", "pit_loo", "mu_loo", "weight_ess")


def ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64)) if a is not None else None


def big_group_labels(pb):
    """One 16-member 4 x 4 group in a corner of the grid, every other row a singleton."""
    cells = gr.cell_labels(pb, 4)
    lab = np.arange(pb["n"], dtype=np.int64) + 10
    lab[cells == cells[0]] = 0
    return lab


def strip_labels(pb):
    """Groups of 4 consecutive columns of the 640 x 4 strip (16 members): a group's rows lie on up to eight levels."""
    x = pb["coords"][:, 0]
    return (np.searchsorted(np.unique(x), x) // 4).astype(np.int64)


def missing_na_problem():
    """The `missing` case (prediction blocks) with every seventh observed row's y set to NaN after the problem is built: NA rows
    inside blocks of the density, which stay members of their groups."""
    pb = LOO_CASES["missing"]()
    before = lr.density_blocks(pb)
    pb["y"] = pb["y"].copy()
    pb["y"][np.nonzero(np.isfinite(pb["y"]))[0][::7]] = np.nan
    assert lr.density_blocks(pb) == before
    return pb


def missing_na_labels(pb):
    """2 x 2 cells over every row, rows of prediction blocks included (they are ignored); a cell whose rows of the density have no
    observed y is in no group."""
    lab = gr.cell_labels(pb, 2)
    dens = np.zeros(pb["n"], dtype=bool)
    dens[np.concatenate([pb["indexing"][u] for u in lr.density_blocks(pb)])] = True
    obs = np.isfinite(pb["y"])
    for v in np.unique(lab):
        if not (obs & dens & (lab == v)).any():
            lab[lab == v] = -1
    return lab


CASES = dict(LOO_CASES, missing_na=missing_na_problem)

# (run, case, labels, force_generic)
LABELLINGS = {
    "missing_na-cells2": ("missing_na", missing_na_labels, False),
    "q1_grid-cells2": ("q1_grid", lambda pb: gr.cell_labels(pb, 2), False),
    "q1_grid-big16": ("q1_grid", big_group_labels, False),
    "leaf_reference-cells2": ("leaf_reference", lambda pb: gr.cell_labels(pb, 2), False),
    "q2-sites": ("q2", lambda pb: loo.site_groups(pb["coords"]), False),
    "q3_wide-sites": ("q3_wide", lambda pb: loo.site_groups(pb["coords"]), False),
    "q5-sites": ("q5", lambda pb: loo.site_groups(pb["coords"]), False),
    "strip_deep-columns4": ("strip_deep", strip_labels, False),
    "q1_grid-random": ("q1_grid", lambda pb: gr.random_labels(pb["n"], 3, 11), False),
    "q1_grid-cells2-generic": ("q1_grid", lambda pb: gr.cell_labels(pb, 2), True),
    "q3_wide-sites-generic": ("q3_wide", lambda pb: loo.site_groups(pb["coords"]), True),
}


@pytest.fixture(scope="module")
def dense():
    """Per case: the problem, the dense reference precision, the rows of the density and a random w -- computed once, never changed."""
    out = {}
    for name in sorted({v[0] for v in LABELLINGS.values()}):
        pb = CASES[name]()
        Q, rows = lr.density_precision(pb, pb["theta"])
        w = np.random.default_rng(1).standard_normal(pb["n"])
        out[name] = (pb, Q, rows, w)
    return out


def one_draw(pb, labels, w, generic=False):
    hm = hip_model(pb, force_generic=generic)
    hm.set_w(w)
    hm.rows_loo_set()
    hm.rows_loo_groups_set(labels)
    hm.rows_loo_accumulate()
    return hm


@pytest.mark.parametrize("run", sorted(LABELLINGS))
def test_last_matches_the_dense_reference(dense, run):
    name, make_labels, generic = LABELLINGS[run]
    pb, Q, rows, w = dense[name]
    labels = make_labels(pb)
    label, members = loo.group_index(labels, rows, np.isfinite(pb["y"]))
    hm = one_draw(pb, labels, w, generic)
    ix = hm.rows_loo_groups_index()
    got = hm.rows_loo_groups_last()
    info = hm.rows_loo_info()
    hm.close()
    assert np.array_equal(ix["label"], label) and ix["n_groups"] == len(members) and ix["n_members"] == sum(m.size for m in members)
    for g, m in enumerate(members):
        assert np.array_equal(ix["rows"][ix["ptr"][g]:ix["ptr"][g + 1]], m)
    err = dict(diag=0.0, off=0.0, qw=0.0, cond_mean=0.0, cond_cov=0.0)
    scale = dict(diag=0.0, qw=0.0, cond_mean=0.0, cond_cov=0.0)
    zeros = pairs = 0
    for g, m in enumerate(members):
        A = Q[np.ix_(m, m)]
        ref = gr.group_terms_ld(A, Q[m] @ w, w[m], pb["y"][m], np.zeros(m.size), np.ones(m.size))
        d = np.sqrt(np.diag(A))
        E = np.abs(got["q_gg"][g] - A)
        assert np.array_equal(got["q_gg"][g], got["q_gg"][g].T)
        err["diag"] = max(err["diag"], np.diag(E).max()); scale["diag"] = max(scale["diag"], np.diag(A).max())
        if m.size > 1:
            off = ~np.eye(m.size, dtype=bool)
            err["off"] = max(err["off"], (E / np.outer(d, d))[off].max())
            zeros += int((got["q_gg"][g][off] == 0.0).sum()) // 2
            pairs += m.size * (m.size - 1) // 2
        for k, r in (("qw", Q[m] @ w), ("cond_mean", ref["cond_mean"].astype(np.float64)), ("cond_cov", ref["cond_cov"].astype(np.float64))):
            err[k] = max(err[k], np.abs(got[k][g] - r).max()); scale[k] = max(scale[k], np.abs(r).max())
    for k in scale:
        err[k] /= scale[k]
    print(run, {k: f"{v:.2e}" for k, v in err.items()}, "pairs", pairs, "structural zeros", zeros, "device pairs", ix["n_pairs"])
    assert all(v <= 1e-8 for v in err.values()), (run, err)
    assert ix["n_pairs"] == pairs - zeros
    if run == "q1_grid-random":
        assert zeros > 0               # members on different branches are what the labelling is here for
    if run == "q1_grid-big16":
        assert max(m.size for m in members) == 16
    if run == "missing_na-cells2":       # NA members inside density blocks, and labelled rows of prediction blocks left out
        allm = np.concatenate(members)
        assert (~np.isfinite(pb["y"][allm])).any() and rows.size < pb["n"] and (labels[np.setdiff1d(np.arange(pb["n"]), rows)] >= 0).any()
    plain = hip_model(pb, force_generic=generic)
    plain.rows_loo_set()
    base = plain.rows_loo_info()
    plain.close()
    assert info["routes"] == base["routes"] and info["alg_bytes"] > base["alg_bytes"] and info["flops"] > base["flops"]


def pair_recomputation(pb, hm, members):
    """Per group, in long double from the device's own panels of slot 0: Q_GG, the sums of absolute products, and per pair the
    number of rows that hold both columns plus the blocks that hold both (the additions the earliest term can pass)."""
    LD = np.longdouble
    gid = -np.ones(pb["n"], dtype=np.int64)
    pos = np.zeros(pb["n"], dtype=np.int64)
    for g, m in enumerate(members):
        gid[m] = g
        pos[m] = np.arange(m.size)
    P = [np.zeros((m.size, m.size), dtype=LD) for m in members]
    AP = [np.zeros((m.size, m.size)) for m in members]
    T = [np.zeros((m.size, m.size)) for m in members]
    for u in lr.density_blocks(pb):
        iu, pa = pb["indexing"][u], pb["parents"][u]
        N, Ri = hm.block(0, u, raw=True)
        Lown = np.tril(Ri) if Ri.ndim == 2 else np.diag(Ri)
        cols = np.concatenate([pb["indexing"][a] for a in pa] + [iu]).astype(np.int64)
        L = np.concatenate([N, Lown], axis=1)
        for g in np.unique(gid[cols][gid[cols] >= 0]):
            k = np.nonzero(gid[cols] == g)[0]
            if k.size < 2:
                continue
            sub = L[:, k]
            at = np.ix_(pos[cols[k]], pos[cols[k]])
            P[g][at] += sub.astype(LD).T @ sub.astype(LD)
            AP[g][at] += np.abs(sub).T @ np.abs(sub)
            both = (sub != 0).astype(np.float64)
            T[g][at] += both.T @ both + 1.0
    return P, AP, T


@pytest.mark.parametrize("run", ["q1_grid-cells2", "q3_wide-sites", "strip_deep-columns4", "q1_grid-random"])
def test_pairs_lie_within_the_rounding_bound_of_the_device_panels(dense, run):
    """|p_ij - exact| <= (T_ij + 1) u sum |L[r,i] L[r,j]| (lgo_kernels.hpp), T_ij = the rows holding both columns + the blocks holding both."""
    name, make_labels, generic = LABELLINGS[run]
    pb, _, rows, w = dense[name]
    labels = make_labels(pb)
    _, members = loo.group_index(labels, rows)
    hm = one_draw(pb, labels, w, generic)
    got = hm.rows_loo_groups_last()
    P, AP, T = pair_recomputation(pb, hm, members)
    hm.close()
    worst = 0.0
    for g, m in enumerate(members):
        if m.size < 2:
            continue
        off = ~np.eye(m.size, dtype=bool)
        e = np.abs(got["q_gg"][g] - P[g]).astype(np.float64)[off]
        b = ((T[g] + 1) * U * AP[g])[off]
        assert np.all(e <= b), (run, g)
        worst = max(worst, (e[b > 0] / b[b > 0]).max() if (b > 0).any() else 0.0)
    print(run, "pairs: worst error / bound", worst)


def draw_bound(ref, A, c, wG):
    """The bound of lgo_kernels.hpp (ROUNDING) on one draw of one group, from the reference's own condition numbers: returns
    (dl, dmu per observed member, dz of the members' standardised residuals)."""
    g, go = len(wG), ref["obs"].size
    V = ref["cond_cov"].astype(np.float64)
    nV = np.linalg.norm(V, 2)
    eV = 4.0 * g * (3 * g + 1) * U * ref["kappa_A"]
    dm = (eV + (g + 2) * U) * nV * np.abs(c).sum() + U * np.abs(wG).max()
    Sig = V[np.ix_(ref["obs"], ref["obs"])]
    lam = np.linalg.eigvalsh(Sig + np.diag(ref["sig"] ** 2 - np.diag(Sig))).min()
    eS = eV * nV / lam + 4.0 * go * (3 * go + 1) * U * ref["kappa_S"]
    quad = ref["quad"]
    dmu = dm + 2 * U * np.abs(ref["mu"].astype(np.float64)).max()
    dl = 0.5 * eS * (quad + go) + math.sqrt(quad / lam) * math.sqrt(go) * dmu + U * (abs(float(ref["l"])) + 4 * go + 4)
    dz = dmu / ref["sig"].min() + eS * np.sqrt(quad) + 4 * U * np.sqrt(quad)
    return dl, dmu, dz


@pytest.mark.parametrize("run,S", [("q1_grid-cells2", 1), ("q2-sites", 2), ("q1_grid-big16", 5), ("q3_wide-sites", 7)])
def test_get_and_totals_match_the_long_double_reference(run, S):
    """The reference is fed the device's own Q_GG and c_G of every draw; the outputs' bounds follow test_gpu_rows_loo.get_bounds
    with the per-draw dl, dmu, dPhi of draw_bound."""
    name, make_labels, generic = LABELLINGS[run]
    pb = LOO_CASES[name]()
    n, q = pb["n"], pb["q"]
    labels = make_labels(pb)
    if run == "q3_wide-sites":          # NA members inside density blocks: integrated out with their group, not scored
        pb["y"] = pb["y"].copy()
        pb["y"][np.random.default_rng(4).choice(n, n // 10, replace=False)] = np.nan
        # a site left without any observed member leaves its group
        obs = np.isfinite(pb["y"])
        for v in np.unique(labels):
            if not obs[labels == v].any():
                labels[labels == v] = -1
    hm = hip_model(pb, force_generic=generic)
    hm.rows_loo_set()
    hm.rows_loo_groups_set(labels)
    ix = hm.rows_loo_groups_index()
    members = [ix["rows"][ix["ptr"][g]:ix["ptr"][g + 1]] for g in range(ix["n_groups"])]
    G = len(members)
    xb, tq, y = hm.get_XB(), tausq_rows(pb), pb["y"]
    rng = np.random.default_rng(S)
    base = rng.standard_normal(n)
    refs, dls, dmus, dzs = [], np.zeros((S, G)), np.zeros((S, G)), np.zeros((S, G))
    for s in range(S):
        w = base * (1.0 + 0.5 * s) + 0.3 * rng.standard_normal(n)
        hm.set_w(w)
        hm.rows_loo_accumulate()
        last = hm.rows_loo_groups_last()
        row = []
        for g, m in enumerate(members):
            r = gr.group_terms_ld(last["q_gg"][g], last["qw"][g], w[m], y[m], xb[m], tq[m])
            dls[s, g], dmus[s, g], dzs[s, g] = draw_bound(r, last["q_gg"][g], last["qw"][g], w[m])
            row.append(r)
            # _last's own conditional moments against the same reference
            assert np.all(np.abs(last["cond_mean"][g] - r["cond_mean"].astype(np.float64)) <= dmus[s, g])
        refs.append(row)
    got = hm.rows_loo_groups_get()
    tot = hm.rows_loo_groups_totals()
    hm.close()
    assert got["n_accumulated"] == S and np.all(got["n_skipped"] == 0)
    ls = np.array([[float(r["l"]) for r in row] for row in refs])
    ref, skipped, _ = lr.estimator_ld(np.array([[r["l"] for r in row] for row in refs], dtype=np.longdouble), np.zeros((S, G)), np.zeros((S, G)))
    assert skipped == 0
    dl = dls.max(axis=0)
    dx = 2 * dl + U * (ls.max(axis=0) - ls.min(axis=0)) + 3 * U + S * U
    b_elpd = 4 * (dl + dx + 4 * U * (np.abs(ls).max(axis=0) + math.log(max(S, 2))))
    b_ess = 4 * (4 * dx + 4 * U) * S
    e_elpd, e_ess = np.abs(got["elpd_lgo"] - ref["elpd_loo"]), np.abs(got["weight_ess"] - ref["weight_ess"])
    print(run, S, "elpd_lgo: worst error / bound", (e_elpd / b_elpd).max(), " weight_ess:", (e_ess / b_ess).max())
    assert np.all(e_elpd <= b_elpd) and np.all(e_ess <= b_ess)
    if S == 1:
        assert np.all(got["weight_ess"] == 1.0)
    # the members: mu_lgo and pit_lgo weighted by the group's ratios
    LD = np.longdouble
    worst_mu = worst_pit = 0.0
    scored = np.zeros(n, dtype=bool)
    for g, m in enumerate(members):
        t = np.array([-refs[s][g]["l"] for s in range(S)], dtype=LD)
        x = np.exp(t - t.max())
        ob = refs[0][g]["obs"]
        mus = np.array([refs[s][g]["mu"] for s in range(S)], dtype=LD)
        phis = np.array([refs[s][g]["phi"] for s in range(S)], dtype=LD)
        mu = ((x[:, None] * mus).sum(axis=0) / x.sum()).astype(np.float64)
        pit = ((x[:, None] * phis).sum(axis=0) / x.sum()).astype(np.float64)
        b_mu = 4 * ((2 * dx[g] + 4 * U) * np.abs(mus.astype(np.float64)).max() + dmus[:, g].max())
        b_pit = 4 * (2 * dx[g] + 0.4 * dzs[:, g].max() + 4 * U)
        e_mu, e_pit = np.abs(got["mu_lgo"][m[ob]] - mu), np.abs(got["pit_lgo"][m[ob]] - pit)
        assert np.all(e_mu <= b_mu) and np.all(e_pit <= b_pit), (run, g)
        worst_mu, worst_pit = max(worst_mu, (e_mu / b_mu).max()), max(worst_pit, (e_pit / b_pit).max())
        scored[m[ob]] = True
    print(run, S, "mu_lgo: worst error / bound", worst_mu, " pit_lgo:", worst_pit)
    assert np.array_equal(np.isfinite(got["mu_lgo"]), scored) and np.array_equal(np.isfinite(got["pit_lgo"]), scored)
    if run == "q3_wide-sites":
        assert (~scored[np.concatenate(members)]).any()      # NA members are what the case is here for
    # the totals: fixed trees of additions of the device's own values
    e = got["elpd_lgo"]
    assert tot["n_groups"] == G and abs(tot["elpd_lgo"] - e.sum()) <= G * U * np.abs(e).sum() and tot["lgoic"] == -2.0 * tot["elpd_lgo"]
    assert tot["min_weight_ess"] == got["weight_ess"].min()
    want = loo.group_totals(got, y, pb["mv_id"] - 1, q)
    # se^2 = G css / (G - 1) with css = sum (e - mean)^2 formed centred in a second pass: G + 5 roundings relative to css on either
    # side (the device's and numpy's), halved by the root
    assert abs(tot["se"] - want["se"]) <= (G + 12) * U * want["se"]
    for j in range(q):
        cnt = want["by_outcome"]["count"][j]
        assert tot["by_outcome"]["count"][j] == cnt
        assert abs(tot["by_outcome"]["sqerr"][j] - want["by_outcome"]["sqerr"][j]) <= (cnt + 3) * U * want["by_outcome"]["sqerr"][j]
        assert abs(tot["by_outcome"]["pit"][j] - want["by_outcome"]["pit"][j]) <= cnt * U * want["by_outcome"]["pit"][j]


def test_singleton_groups_reproduce_the_rows():
    """A group of one row is that row's leave-one-out: A = d, V = 1 / d, m = w - c / d (one rounding apart: V c against c / d)."""
    pb = LOO_CASES["missing"]()
    n = pb["n"]
    hm = hip_model(pb)
    hm.rows_loo_set()
    hm.rows_loo_groups_set(np.where(np.isfinite(pb["y"]), np.arange(n), -1).astype(np.int64))
    rng = np.random.default_rng(2)
    for s in range(4):
        hm.set_w(rng.standard_normal(n) * (1 + s))
        hm.rows_loo_accumulate()
    rows, grp = hm.rows_loo_get(), hm.rows_loo_groups_get()
    ix = hm.rows_loo_groups_index()
    hm.close()
    m = ix["rows"]
    assert np.array_equal(m, np.nonzero(np.isfinite(pb["y"]))[0]) and ix["n_pairs"] == 0
    assert np.allclose(grp["elpd_lgo"], rows["elpd_loo"][m], rtol=0, atol=1e-12 * np.abs(rows["elpd_loo"][m]).max())
    assert np.allclose(grp["weight_ess"], rows["weight_ess"][m], rtol=1e-12)
    assert np.allclose(grp["mu_lgo"][m], rows["mu_loo"][m], rtol=0, atol=1e-12 * np.abs(rows["mu_loo"][m]).max())
    assert np.allclose(grp["pit_lgo"][m], rows["pit_loo"][m], rtol=0, atol=1e-12)


def test_a_draw_with_tausq_inv_zero_is_skipped_and_counted():
    pb = LOO_CASES["q1_grid"]()
    n = pb["n"]
    hm = hip_model(pb)
    hm.rows_loo_set()
    hm.rows_loo_groups_set(gr.cell_labels(pb, 2))
    rng = np.random.default_rng(0)
    hm.set_w(rng.standard_normal(n))
    hm.rows_loo_accumulate()
    one = hm.rows_loo_groups_get()
    zero = np.zeros(1)
    assert hm.lib.st_set_tausq_inv(hm.h, zero.ctypes.data_as(C.POINTER(C.c_double))) == 0
    hm.set_w(rng.standard_normal(n))
    hm.rows_loo_accumulate()
    two = hm.rows_loo_groups_get()
    hm.close()
    assert np.all(one["n_skipped"] == 0) and np.all(two["n_skipped"] == 1) and two["n_accumulated"] == 2
    for k in ("elpd_lgo", "weight_ess", "mu_lgo", "pit_lgo"):   # the skipped draw changed nothing
        assert np.array_equal(one[k], two[k], equal_nan=True), k
    assert np.all(np.isfinite(one["elpd_lgo"]))


def test_rows_outputs_are_bitwise_those_without_groups_and_repeatable():
    pb = LOO_CASES["q3_wide"]()
    n = pb["n"]
    labels = loo.site_groups(pb["coords"])
    runs = []
    for mode in ("plain", "groups", "groups"):
        hm = hip_model(pb)
        hm.rows_loo_set()
        if mode == "groups":
            hm.rows_loo_groups_set(labels)
        hm.deal_with_w(None, seed=3, it=0)
        lasts = []
        for it in range(1, 4):
            hm.rows_loo_accumulate()
            lasts.append(hm.rows_loo_last())
            hm.deal_with_w(None, seed=3, it=it)
        out = dict(last=lasts, get=hm.rows_loo_get(), tot=hm.rows_loo_totals(raw=True)[0], w=hm.get_w().copy(), ll=hm.get_loglik_w(0))
        if mode == "groups":
            out["grp"] = hm.rows_loo_groups_get()
            out["glast"] = hm.rows_loo_groups_last()
            out["gtot"] = hm.rows_loo_groups_totals()
        runs.append(out)
        hm.close()
    for other in runs[1:]:
        for a, b in zip(runs[0]["last"], other["last"]):
            assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in LOO_LAST)
        assert all(np.array_equal(runs[0]["get"][k], other["get"][k], equal_nan=True) for k in LOO_OUT)
        assert np.array_equal(runs[0]["tot"], other["tot"]) and np.array_equal(runs[0]["w"], other["w"]) and runs[0]["ll"] == other["ll"]
    a, b = runs[1], runs[2]
    for k in ("elpd_lgo", "weight_ess", "mu_lgo", "pit_lgo", "n_skipped"):
        assert np.array_equal(a["grp"][k], b["grp"][k], equal_nan=True), k
    for k in ("q_gg", "qw", "cond_mean", "cond_cov"):
        assert all(np.array_equal(x, y) for x, y in zip(a["glast"][k], b["glast"][k])), k
    assert a["gtot"]["elpd_lgo"] == b["gtot"]["elpd_lgo"] and a["gtot"]["se"] == b["gtot"]["se"]


def test_refusals_leave_a_text_and_a_usable_handle():
    pb = LOO_CASES["q1_grid"]()
    n = pb["n"]
    hm = hip_model(pb)
    lib, h = hm.lib, hm.h
    cells = gr.cell_labels(pb, 2)
    cnt = C.c_int64()
    calls = [lambda: lib.st_rows_loo_groups_set(h, ip(cells)), lambda: lib.st_rows_loo_groups_clear(h),
             lambda: lib.st_rows_loo_groups_count(h, C.byref(cnt), None, None, None), lambda: lib.st_rows_loo_groups_index(h, None, None, None),
             lambda: lib.st_rows_loo_groups_last(h, None, None, None, None),
             lambda: lib.st_rows_loo_groups_get(h, None, None, None, None, None, C.byref(cnt)),
             lambda: lib.st_rows_loo_groups_totals(h, None, None)]
    for call in calls:                                   # groups without st_rows_loo_set
        assert call() == ST_ERR_USAGE and b"before st_rows_loo_set" in lib.st_last_error(h)
    hm.rows_loo_set()
    for call in calls[1:]:                               # any call before _groups_set
        assert call() == ST_ERR_USAGE and b"before st_rows_loo_groups_set" in lib.st_last_error(h)
    big = gr.cell_labels(pb, 4)
    big[np.nonzero(big == 3)[0][0]] = 0                  # 17 members
    assert lib.st_rows_loo_groups_set(h, ip(big)) == ST_ERR_UNSUPPORTED
    assert b"17 members" in lib.st_last_error(h) and b"16" in lib.st_last_error(h)
    assert calls[2]() == ST_ERR_USAGE                    # nothing was set
    assert calls[0]() == 0 and calls[2]() == 0 and cnt.value == len(np.unique(cells))
    assert lib.st_rows_loo_groups_set(h, ip(big)) == ST_ERR_UNSUPPORTED and calls[2]() == 0 and cnt.value == len(np.unique(cells))
    for call in calls[4:]:                               # _last / _get / _totals before the first accumulate
        assert call() == ST_ERR_USAGE and b"no iteration accumulated" in lib.st_last_error(h)
    assert cnt.value == 0
    hm.rows_loo_accumulate()
    assert calls[0]() == ST_ERR_USAGE and b"after 1 accumulated" in lib.st_last_error(h)      # a late _set
    assert calls[1]() == ST_ERR_USAGE and b"after 1 accumulated" in lib.st_last_error(h)
    assert calls[5]() == 0 and cnt.value == 1 and calls[6]() == 0
    hm.rows_loo_set()                                    # anew: the groups left with the state
    assert calls[2]() == ST_ERR_USAGE and calls[0]() == 0 and calls[1]() == 0 and calls[2]() == ST_ERR_USAGE
    hm.rows_loo_accumulate()
    assert np.all(np.isfinite(hm.rows_loo_get()["elpd_loo"]))
    hm.close()

    na = LOO_CASES["missing"]()                          # a group of NA rows only, inside blocks of the density
    rows = lr.density_precision(na, na["theta"])[1]
    na["y"] = na["y"].copy()
    gone = rows[np.isfinite(na["y"][rows])][[3, 40]]     # two rows lose their y after the problem is built
    na["y"][gone] = np.nan
    assert np.array_equal(lr.density_precision(na, na["theta"])[1], rows)
    lab = -np.ones(na["n"], dtype=np.int64)
    lab[gone] = 5
    hm = hip_model(na)
    hm.rows_loo_set()
    assert hm.lib.st_rows_loo_groups_set(hm.h, ip(lab)) == ST_ERR_USAGE and b"no member with an observed y" in hm.lib.st_last_error(hm.h)
    off = np.setdiff1d(np.arange(na["n"]), rows)         # labelled rows of prediction blocks are ignored
    lab = -np.ones(na["n"], dtype=np.int64)
    lab[off] = 1
    lab[np.nonzero(np.isfinite(na["y"]))[0][:2]] = 1
    assert off.size > 0 and hm.lib.st_rows_loo_groups_set(hm.h, ip(lab)) == 0
    assert hm.rows_loo_groups_index()["n_members"] == 2
    with pytest.raises(ValueError, match="one value per row"):
        hm.rows_loo_groups_set(np.zeros(3, dtype=np.int64))
    hm.close()

    lim = LOO_CASES["limited"]()
    hm = hip_model(lim)
    z = np.zeros(lim["n"], dtype=np.int64)
    assert hm.lib.st_rows_loo_groups_set(hm.h, ip(z)) == ST_ERR_UNSUPPORTED and b"limited_tree" in hm.lib.st_last_error(hm.h)
    assert hm.get_loglik_w(0) == hm.get_loglik_w(0)      # still usable
    hm.close()


def test_end_to_end_total_against_the_exact_leave_group_out_density():
    """Side 12, q = 1, 3 x 3 cells, theta, beta = 0 and tausq = 0.2 fixed, 2000 saved iterations after 200 of burn-in: sum elpd_lgo
    within 2 % of the exact total (-301.40); the same run's sum elpd_loo (exact: -317.33) is more than 2 % from it."""
    from spamtree_amd import fit
    pb = make_problem(side=12, q=1, seed=5)
    n = pb["n"]
    labels = gr.cell_labels(pb, 3)
    Q, rows = lr.density_precision(pb, pb["theta"])
    _, members = loo.group_index(labels, rows, np.isfinite(pb["y"]))
    exact = gr.exact_lgo(pb, Q, rows, np.zeros(n), np.full(n, 0.2), members)
    assert len(members) == 16 and abs(exact.sum() - (-301.40)) < 0.01
    res = fit.spamtree_mv_mcmc(*fit_args(pb, tausq=0.2), loo=True, loo_groups=labels, mcmc_keep=2000, mcmc_burn=200, mcmc_thin=1, seed=5,
                               sample_theta=False, sample_beta=False, sample_tausq=False, save_w=False, save_yhat=False,
                               main_verbose=False)
    lo = res["criteria"]["loo"]
    g = lo["groups"]
    total, rows_total, ess, skip = g["totals"]["elpd_lgo"], lo["totals"]["elpd_loo"], g["weight_ess"], g["n_skipped"]
    assert all(np.array_equal(a, b) for a, b in zip(g["members"], members)) and g["totals"]["n_groups"] == 16
    print("sum elpd_lgo", total, "exact", exact.sum(), "sum elpd_loo", rows_total, "min weight_ess", ess.min())
    assert lo["n_accumulated"] == 2000 and np.all(skip == 0) and lo["n_skipped"] == 0
    assert abs(total - exact.sum()) <= 0.02 * abs(exact.sum())
    assert abs(rows_total - exact.sum()) > 0.02 * abs(exact.sum())


def test_group_khat_is_st_psis_on_the_stored_ratios():
    """With a store the groups' log ratios are kept, the existing PSIS kernel runs on them (one series per group, no companions),
    and nothing else changes: reserved before or after the groups are set."""
    pb = LOO_CASES["q3_wide"]()
    n = pb["n"]
    labels = loo.site_groups(pb["coords"])
    S = 60
    runs = {}
    for order in ("none", "reserve_first", "groups_first"):
        hm = hip_model(pb)
        hm.rows_loo_set()
        if order == "reserve_first":
            hm.rows_loo_reserve(S)
        hm.rows_loo_groups_set(labels)
        if order == "groups_first":
            hm.rows_loo_reserve(S)
        rng = np.random.default_rng(8)
        for s in range(S):
            hm.set_w(rng.standard_normal(n) * (0.5 + rng.uniform()))
            hm.rows_loo_accumulate()
        out = dict(get=hm.rows_loo_groups_get(), rows=hm.rows_loo_get())
        if order == "none":
            assert hm.lib.st_rows_loo_groups_psis(hm.h, None, None, None, None, None) == ST_ERR_USAGE
            assert b"no store reserved" in hm.lib.st_last_error(hm.h)
        else:
            out["t"] = hm.rows_loo_groups_draws()
            out["psis"] = hm.rows_loo_groups_psis()
            out["direct"] = hm.psis(out["t"])
            out["rows_psis"] = hm.rows_loo_psis()
        runs[order] = out
        hm.close()
    a, b, c = runs["none"], runs["reserve_first"], runs["groups_first"]
    for other in (b, c):
        for k in ("elpd_lgo", "weight_ess", "mu_lgo", "pit_lgo", "n_skipped"):
            assert np.array_equal(a["get"][k], other["get"][k], equal_nan=True), k
        assert all(np.array_equal(a["rows"][k], other["rows"][k], equal_nan=True) for k in LOO_OUT)
        for k in ("khat", "elpd_psis", "weight_ess_psis", "tail_len", "n_draws"):
            assert np.array_equal(other["psis"][k], other["direct"][k], equal_nan=True), k
        t = other["t"]
        assert t.shape == (S, a["get"]["elpd_lgo"].size) and np.all(np.isfinite(t)) and np.all(other["psis"]["n_draws"] == S)
        raw = -(np.log(np.exp(t - t.max(axis=0)).sum(axis=0)) + t.max(axis=0) - math.log(S))
        assert np.allclose(raw, a["get"]["elpd_lgo"], rtol=1e-12, atol=1e-12)
        assert np.all(np.isfinite(other["psis"]["khat"])) and np.all(other["psis"]["tail_len"] > 0)
    assert np.array_equal(b["t"], c["t"]) and np.array_equal(b["rows_psis"]["khat"], c["rows_psis"]["khat"], equal_nan=True)
    print("group khat: max", b["psis"]["khat"].max(), "rows' khat: max", np.nanmax(b["rows_psis"]["khat"]))


def test_driver_equals_the_hand_stepped_calls_and_leaves_the_rest_alone():
    from spamtree_amd import fit
    pb = make_problem(side=12, q=3, seed=5, missing=0.1)
    n, q = pb["n"], pb["q"]
    labels = loo.site_groups(pb["coords"])
    keep = 12
    kw = dict(mcmc_keep=keep, mcmc_burn=0, mcmc_thin=1, seed=17, adapting=True, main_verbose=False, sample_predicts=False, save_w=False,
              save_yhat=False)
    res = fit.spamtree_mv_mcmc(*fit_args(pb), loo=True, psis=True, loo_groups=labels, **kw)
    plain = fit.spamtree_mv_mcmc(*fit_args(pb), loo=True, psis=True, **kw)
    raw = fit.spamtree_mv_mcmc(*fit_args(pb), loo=True, loo_groups=labels, **kw)
    for key in ("beta_mcmc", "tausq_mcmc", "theta_mcmc", "paramsd"):
        assert np.array_equal(res[key], plain[key]) and np.array_equal(raw[key], plain[key]), key
    lo, lp = res["criteria"]["loo"], plain["criteria"]["loo"]
    for k in LOO_OUT:                                     # what the request shares with one without groups, bit for bit
        assert np.array_equal(lo[k], lp[k], equal_nan=True), k
    assert np.array_equal(lo["totals"]["by_outcome"]["elpd_loo"], lp["totals"]["by_outcome"]["elpd_loo"])
    for k in ("khat", "elpd_psis", "pit_psis", "mu_psis", "weight_ess_psis"):
        assert np.array_equal(lo["psis"][k], lp["psis"][k], equal_nan=True), k
    assert "groups" not in lp and "khat" not in raw["criteria"]["loo"]["groups"]
    ch = fit.Chain(*fit_args(pb)[:15], pb["theta"], np.zeros(pb["p"]), 0.1, 0.02 * np.eye(pb["theta"].size), seed=17, adapting=True)
    lib = ch.lib
    assert lib.st_rows_loo_set(ch.h) == 0 and lib.st_rows_loo_reserve(ch.h, keep) == 0 and lib.st_rows_loo_groups_set(ch.h, ip(labels)) == 0
    for _ in range(keep):
        ch.step(1)
        assert lib.st_rows_loo_accumulate(ch.h) == 0
    cnt = [C.c_int64() for _ in range(3)]
    assert lib.st_rows_loo_groups_count(ch.h, *[C.byref(v) for v in cnt], None) == 0
    ng, nm = int(cnt[0].value), int(cnt[1].value)
    label, ptr, rows = np.zeros(ng, dtype=np.int64), np.zeros(ng + 1, dtype=np.int64), np.zeros(nm, dtype=np.int64)
    assert lib.st_rows_loo_groups_index(ch.h, ip(label), ip(ptr), ip(rows)) == 0
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
    e, ess, skip, mu, pit = np.zeros(ng), np.zeros(ng), np.zeros(ng, dtype=np.int64), np.zeros(n), np.zeros(n)
    assert lib.st_rows_loo_groups_get(ch.h, dp(e), dp(ess), ip(skip), dp(mu), dp(pit), None) == 0
    tot, by = np.zeros(5), np.zeros((3, q), order="F")
    assert lib.st_rows_loo_groups_totals(ch.h, dp(tot), dp(by)) == 0
    kh, ep, wp = np.zeros(ng), np.zeros(ng), np.zeros(ng)
    assert lib.st_rows_loo_groups_psis(ch.h, dp(kh), dp(ep), dp(wp), None, None) == 0
    ch.close()
    obs = np.isfinite(pb["y"])
    for g in (res["criteria"]["loo"]["groups"], raw["criteria"]["loo"]["groups"]):
        assert np.array_equal(g["label"], label) and len(g["members"]) == ng and g["n_pairs"] == cnt[2].value
        assert all(np.array_equal(g["members"][k], rows[ptr[k]:ptr[k + 1]]) for k in range(ng))
        for k, v in (("elpd_lgo", e), ("weight_ess", ess), ("n_skipped", skip), ("mu_lgo", mu), ("pit_lgo", pit)):
            assert np.array_equal(g[k], v, equal_nan=True), k
        t = g["totals"]
        assert [t[k] for k in ("elpd_lgo", "lgoic", "se", "min_weight_ess")] == list(tot[:4]) and t["n_groups"] == ng == int(tot[4])
        assert all(np.array_equal(t["by_outcome"][k], by[i]) for i, k in enumerate(("sqerr", "pit", "count")))
        scored = np.zeros(n, dtype=bool)
        scored[rows] = True
        assert np.array_equal(np.isfinite(g["mu_lgo"]), scored & obs) and int(by[2].sum()) == int((scored & obs).sum())
    g = res["criteria"]["loo"]["groups"]
    assert np.array_equal(g["khat"], kh) and np.array_equal(g["elpd_psis"], ep) and np.array_equal(g["weight_ess_psis"], wp)
    # the members are the observed rows: NA rows here lie in prediction blocks and are ignored
    assert nm == int(obs.sum()) and ng == np.unique(labels[obs]).size
