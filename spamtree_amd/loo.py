"""Leave-one-out criteria with the latent field integrated out: the definition in float64 NumPy (no device, no library).

The criteria of ``rows_score`` are conditional on w.  Here saved draw s gives an observed row i of margin j the density of y_i with
its own w_i integrated out against the prior full conditional of the tree's DAG, w_i | w_-i, theta ~ N(m_i, v_i):

    v_i = 1 / Q_ii,   m_i = w_i - (Q w)_i / Q_ii,   Q = the DAG's prior precision over the blocks with observed rows,
    mu_s = XB_i + m_i,   sigma2_s = v_i + tausq_j,   l_s = log N(y_i; mu_s, sigma2_s),   Phi_s = Phi((y_i - mu_s) / sigma_s).

Over the S saved draws, with the weights r_s = exp(-l_s):

    elpd_loo_i = -log((1 / S) sum r_s),   pit_loo_i = sum r_s Phi_s / sum r_s,   mu_loo_i = sum r_s mu_s / sum r_s,
    weight_ess_i = (sum r_s)^2 / sum r_s^2.

E_post[1 / p(y_i | w_-i, theta, beta, tausq)] = 1 / p(y_i | y_-i), so elpd_loo_i estimates the leave-one-out log predictive density
log p(y_i | y_-i).  These are the raw weights, with ``weight_ess`` as their diagnostic (on the checks of tests/test_rows_loo_cpu.py it
stayed above 0.17 S); ``spamtree_amd.psis`` smooths their tail and gives k-hat from the per-draw terms the device keeps when asked
(``draw_terms`` below: t_s = -l_s, Phi_s, mu_s).  NA rows get no leave-one-out value: they are leaves, predict them as new points.

The streaming state is what the device keeps (spamtree_amd/csrc/loo_kernels.hpp gives the order of every operation there): the
running maximum M of t_s = -l_s, A1 = sum e^(t - M), A2 = sum e^(2 (t - M)), AP = sum e^(t - M) Phi, AM = sum e^(t - M) mu, rescaled
when M grows, and NS, the number of draws skipped because l_s was not finite.
"""
import math

import numpy as np

HL2PI = -0.91893853320467274178
STATE = ("M", "A1", "A2", "AP", "AM", "NS")


def conditional_moments(Q, w):
    """(q_diag, qw, cond_mean, cond_var) of every row from a precision matrix Q and a field w: Q_ii, (Q w)_i, w_i - (Q w)_i / Q_ii
    and 1 / Q_ii."""
    Q, w = np.asarray(Q, dtype=np.float64), np.asarray(w, dtype=np.float64)
    d = np.diag(Q).copy()
    c = Q @ w
    return d, c, w - c / d, 1.0 / d


def draw_terms(y, xb, cond_mean, cond_var, tausq):
    """(l, Phi, mu) of one draw: the log density of y under N(xb + cond_mean, cond_var + tausq) per row (``tausq`` per row), its
    distribution function at y and its mean."""
    y = np.asarray(y, dtype=np.float64)
    mu = np.asarray(xb, dtype=np.float64) + np.asarray(cond_mean, dtype=np.float64)
    with np.errstate(all="ignore"):
        sig = np.sqrt(np.asarray(cond_var, dtype=np.float64) + np.asarray(tausq, dtype=np.float64))
        z = (y - mu) / sig
        l = -0.5 * z * z - np.log(sig) + HL2PI
    phi = 0.5 * np.array([math.erfc(-v * 0.70710678118654752440) if np.isfinite(v) else np.nan for v in np.ravel(z)]).reshape(np.shape(z))
    return l, phi, mu


def new_state(n):
    return {k: np.zeros(n) for k in STATE}


def update(state, l, phi, mu):
    """One draw into the streaming state (in place; returns it).  Rows whose l is not finite are skipped and counted in NS."""
    l, phi, mu = (np.asarray(a, dtype=np.float64) for a in (l, phi, mu))
    ok = np.isfinite(l)
    state["NS"][~ok] += 1.0
    t = np.where(ok, -l, 0.0)
    M, A1, A2, AP, AM = (state[k] for k in ("M", "A1", "A2", "AP", "AM"))
    first = ok & (A1 == 0.0)
    low = ok & ~first & (t <= M)
    high = ok & ~first & (t > M)
    with np.errstate(all="ignore"):
        x = np.exp(np.where(low, t - M, 0.0))
        A1[low] += x[low]; A2[low] += (x * x)[low]; AP[low] += (x * phi)[low]; AM[low] += (x * mu)[low]
        x = np.exp(np.where(high, M - t, 0.0))
        A1[high] = (A1 * x + 1.0)[high]; A2[high] = (A2 * x * x + 1.0)[high]
        AP[high] = (AP * x + phi)[high]; AM[high] = (AM * x + mu)[high]
        M[high] = t[high]
    M[first] = t[first]; A1[first] = 1.0; A2[first] = 1.0; AP[first] = phi[first]; AM[first] = mu[first]
    return state


def finish(state, S):
    """dict(elpd_loo, pit_loo, mu_loo, weight_ess) after S draws; NaN where every draw was skipped."""
    with np.errstate(all="ignore"):
        Si = S - state["NS"]
        A1 = np.where(Si > 0, state["A1"], np.nan)
        return dict(elpd_loo=-(state["M"] + np.log(A1 / Si)), pit_loo=state["AP"] / A1, mu_loo=state["AM"] / A1,
                    weight_ess=A1 * A1 / state["A2"])


def totals(rows, y, mv, q):
    """Per outcome (``mv`` 0-based) over the rows with a finite elpd_loo: dict(n, elpd_loo, looic, sqerr, pit, min_weight_ess), q
    values each (sums, not means)."""
    y, mv = np.asarray(y, dtype=np.float64), np.asarray(mv)
    out = dict(n=np.zeros(q, dtype=np.int64), elpd_loo=np.zeros(q), looic=np.zeros(q), sqerr=np.zeros(q), pit=np.zeros(q),
               min_weight_ess=np.full(q, np.nan))
    for j in range(q):
        k = (mv == j) & np.isfinite(rows["elpd_loo"])
        out["n"][j] = int(k.sum())
        if not k.any():
            continue
        out["elpd_loo"][j] = rows["elpd_loo"][k].sum()
        out["looic"][j] = -2.0 * out["elpd_loo"][j]
        out["sqerr"][j] = ((y[k] - rows["mu_loo"][k]) ** 2).sum()
        out["pit"][j] = rows["pit_loo"][k].sum()
        out["min_weight_ess"][j] = rows["weight_ess"][k].min()
    return out


# ---- leave-group-out: a group of rows left out together, its rows of w integrated out jointly ---------------------------------
#
# A label per row (int64, negative = in no group); a group is the set of rows with one label among ``rows``, the rows of the density
# (blocks with an observed row).  Groups are numbered by ascending label, members stand in ascending row.  Saved draw s gives group
# G, with o its members with an observed y,
#
#     A = Q_GG,  V = A^-1,  m_G = w_G - V (Q w)_G,  mu_o = XB_o + m_o,  Sigma = V_oo + diag(tausq_{j(a)}),
#     l_s = log N(y_o; mu_o, Sigma),  Phi_a = Phi((y_a - mu_a) / sqrt(Sigma_aa)),
#
# and over the draws, r_s = exp(-l_s): elpd_lgo = -log mean r_s, weight_ess = (sum r)^2 / sum r^2, mu_lgo_a and pit_lgo_a weighted by
# r_s.  E_post[1 / p(y_G | w_-G, theta, beta, tausq)] = 1 / p(y_G | y_-G), so elpd_lgo estimates log p(y_G | y_-G).  A member
# without an observed y is integrated out with the group and not scored.  The streaming state is that of the rows (``update``), one
# (M, A1, A2, NS) per group and (AP, AM) per member; a draw whose l_s is not finite, or whose A or Sigma has a Cholesky pivot that
# is not > 0, is skipped for the group and counted.
LGO_MAX_MEMBERS = 16


def site_groups(coords):
    """One label per distinct location (rows of ``coords``), numbered in the lexicographic order of the locations: all outcomes at
    a site.  One sort of the rows, no Python loop."""
    coords = np.asarray(coords, dtype=np.float64)
    if coords.ndim != 2:
        raise ValueError(f"coords must be n x d, got shape {coords.shape}")
    n = coords.shape[0]
    out = np.zeros(n, dtype=np.int64)
    if n == 0 or coords.shape[1] == 0:
        return out
    order = np.lexsort(coords.T[::-1])                  # by the first column, then the second, ...
    srt = coords[order]
    out[order] = np.concatenate([[0], np.cumsum((srt[1:] != srt[:-1]).any(axis=1))])
    return out


def block_groups(coords, cell):
    """One label per square cell of side ``cell`` (the first two coordinates, cells anchored at their minima): floor((x - min) / cell)."""
    coords = np.asarray(coords, dtype=np.float64)
    if coords.ndim != 2 or coords.shape[1] < 2:
        raise ValueError(f"coords must be n x d with d >= 2, got shape {coords.shape}")
    if not (np.isfinite(cell) and cell > 0):
        raise ValueError(f"cell must be a positive number, got {cell}")
    ij = np.floor((coords[:, :2] - coords[:, :2].min(axis=0)) / float(cell)).astype(np.int64)
    return ij[:, 0] * (ij[:, 1].max() + 1) + ij[:, 1]


def group_index(labels, rows=None, observed=None):
    """(label, members): the groups by ascending label, each an ascending int64 array of rows.  ``rows``: the rows of the density
    (default all).  ValueError: labels not one integer per row, a group beyond LGO_MAX_MEMBERS, or (``observed`` given: a flag per
    row) a group without an observed member."""
    labels = np.asarray(labels)
    if labels.ndim != 1 or not np.issubdtype(labels.dtype, np.integer):
        raise ValueError(f"loo_groups must be one integer label per row, got shape {labels.shape} of {labels.dtype}")
    keep = np.zeros(labels.size, dtype=bool)
    keep[np.arange(labels.size) if rows is None else np.asarray(rows)] = True
    keep &= labels >= 0
    # one stable sort of the kept rows by label: ascending labels, ascending rows inside a label
    idx = np.nonzero(keep)[0].astype(np.int64)
    idx = idx[np.argsort(labels[idx], kind="stable")]
    label, start, count = np.unique(labels[idx], return_index=True, return_counts=True)
    if count.size and count.max() > LGO_MAX_MEMBERS:
        g = int(np.argmax(count > LGO_MAX_MEMBERS))
        raise ValueError(f"loo_groups: the group of label {label[g]} has {count[g]} members, at most {LGO_MAX_MEMBERS} are supported")
    if observed is not None and label.size:
        has = np.add.reduceat(np.asarray(observed, dtype=bool)[idx].astype(np.int64), start) > 0
        if not has.all():
            raise ValueError(f"loo_groups: the group of label {label[int(np.argmin(has))]} has no member with an observed y")
    members = np.split(idx, start[1:])
    if not label.size:
        members = []
    return label.astype(np.int64), members


def group_terms(Q, w, members, y, xb, tausq):
    """One draw of one group from the precision Q and the field w: dict(l, phi, mu, obs, q_gg, qw, cond_mean, cond_cov); phi and mu
    over the observed members ``obs`` (positions in ``members``).  l is NaN where a Cholesky pivot is not > 0."""
    Q, w = np.asarray(Q, dtype=np.float64), np.asarray(w, dtype=np.float64)
    G = np.asarray(members)
    A = Q[np.ix_(G, G)]
    c = Q[G] @ w
    return group_terms_from(A, c, w[G], np.asarray(y, dtype=np.float64)[G], np.asarray(xb, dtype=np.float64)[G],
                            np.asarray(tausq, dtype=np.float64)[G])


def group_terms_from(A, c, wG, yG, xbG, tausqG):
    """``group_terms`` from the group's own A = Q_GG, c = (Q w)_G, w_G, y_G, XB_G and per-member tausq."""
    nan = float("nan")
    g = len(wG)
    ob = np.nonzero(np.isfinite(yG))[0]
    out = dict(l=nan, phi=np.full(ob.size, nan), mu=np.full(ob.size, nan), obs=ob, q_gg=A, qw=c, cond_mean=np.full(g, nan),
               cond_cov=np.full((g, g), nan))
    with np.errstate(all="ignore"):
        try:
            L = np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            return out
        Li = np.linalg.solve(L, np.eye(g))
        V = Li.T @ Li
        m = wG - V @ c
        out["cond_mean"], out["cond_cov"] = m, V
        mu = xbG[ob] + m[ob]
        Sig = V[np.ix_(ob, ob)] + np.diag(tausqG[ob])
        out["mu"] = mu
        try:
            Ls = np.linalg.cholesky(Sig)
        except np.linalg.LinAlgError:
            return out
        z = np.linalg.solve(Ls, yG[ob] - mu)
        out["l"] = -0.5 * float(z @ z) - float(np.log(np.diag(Ls)).sum()) + ob.size * HL2PI
        zs = (yG[ob] - mu) / np.sqrt(np.diag(Sig))
        out["phi"] = 0.5 * np.array([math.erfc(-v * 0.70710678118654752440) if np.isfinite(v) else nan for v in zs])
    return out


def group_terms_batch(Q, W, members, y, xb, tausq):
    """``group_terms`` of one group over the S rows of W, draws that share Q (theta fixed): dict(l (S), phi, mu (S x g_o), obs).
    A, V and Sigma are then the same for every draw; only (Q w)_G and with it the mean move."""
    Q, W = np.asarray(Q, dtype=np.float64), np.asarray(W, dtype=np.float64)
    G = np.asarray(members)
    first = group_terms(Q, W[0], G, y, xb, tausq)
    V, ob = first["cond_cov"], first["obs"]
    yG, xbG, tG = (np.asarray(a, dtype=np.float64)[G] for a in (y, xb, tausq))
    M = W[:, G] - (W @ Q[G].T) @ V.T
    mu = xbG[ob][None, :] + M[:, ob]
    Sig = V[np.ix_(ob, ob)] + np.diag(tG[ob])
    Ls = np.linalg.cholesky(Sig)
    Z = np.linalg.solve(Ls, (yG[ob][None, :] - mu).T).T
    l = -0.5 * (Z * Z).sum(axis=1) - float(np.log(np.diag(Ls)).sum()) + ob.size * HL2PI
    zs = (yG[ob][None, :] - mu) / np.sqrt(np.diag(Sig))[None, :]
    phi = 0.5 * np.vectorize(math.erfc, otypes=[np.float64])(-zs * 0.70710678118654752440)
    return dict(l=l, phi=phi, mu=mu, obs=ob)


def new_group_state(members):
    """The streaming state of the groups: M, A1, A2, NS per group, AP and AM per group over its members (NaN off the observed)."""
    G = len(members)
    return dict(M=np.zeros(G), A1=np.zeros(G), A2=np.zeros(G), NS=np.zeros(G), AP=[np.zeros(len(m)) for m in members],
                AM=[np.zeros(len(m)) for m in members])


def update_groups(state, terms):
    """One draw into the groups' state: ``terms`` is one ``group_terms`` dict per group.  The update of ``update``, the weight
    shared by the group and its members."""
    for g, t in enumerate(terms):
        l = t["l"]
        if not np.isfinite(l):
            state["NS"][g] += 1.0
            continue
        ob, x = t["obs"], -l
        AP, AM = state["AP"][g], state["AM"][g]
        if state["A1"][g] == 0.0:
            state["M"][g], state["A1"][g], state["A2"][g] = x, 1.0, 1.0
            AP[ob], AM[ob] = t["phi"], t["mu"]
        elif x <= state["M"][g]:
            e = math.exp(x - state["M"][g])
            state["A1"][g] += e; state["A2"][g] += e * e
            AP[ob] += e * t["phi"]; AM[ob] += e * t["mu"]
        else:
            e = math.exp(state["M"][g] - x)
            state["A1"][g] = state["A1"][g] * e + 1.0; state["A2"][g] = state["A2"][g] * e * e + 1.0
            AP[ob] = AP[ob] * e + t["phi"]; AM[ob] = AM[ob] * e + t["mu"]
            state["M"][g] = x
    return state


def finish_groups(state, S, members, n, observed):
    """dict(elpd_lgo, weight_ess, n_skipped per group; mu_lgo, pit_lgo per row (n values), NaN off the observed members)."""
    with np.errstate(all="ignore"):
        Sg = S - state["NS"]
        A1 = np.where(Sg > 0, state["A1"], np.nan)
        out = dict(elpd_lgo=-(state["M"] + np.log(A1 / Sg)), weight_ess=A1 * A1 / state["A2"], n_skipped=state["NS"].astype(np.int64),
                   mu_lgo=np.full(n, np.nan), pit_lgo=np.full(n, np.nan))
        observed = np.asarray(observed, dtype=bool)
        for g, m in enumerate(members):
            ob = observed[m]
            out["mu_lgo"][m[ob]] = (state["AM"][g] / A1[g])[ob]
            out["pit_lgo"][m[ob]] = (state["AP"][g] / A1[g])[ob]
    return out


def group_totals(res, y, mv, q):
    """dict(elpd_lgo, lgoic, se, min_weight_ess, n_groups, by_outcome=dict(sqerr, pit, count)) over the groups with a value: se =
    sqrt(G var) of the groups' elpd_lgo, var with divisor G - 1 (NaN below two groups)."""
    e = res["elpd_lgo"][np.isfinite(res["elpd_lgo"])]
    G = e.size
    y, mv = np.asarray(y, dtype=np.float64), np.asarray(mv)
    by = dict(sqerr=np.zeros(q), pit=np.zeros(q), count=np.zeros(q))
    for j in range(q):
        k = (mv == j) & np.isfinite(res["mu_lgo"])
        by["sqerr"][j] = ((y[k] - res["mu_lgo"][k]) ** 2).sum()
        by["pit"][j] = res["pit_lgo"][k].sum()
        by["count"][j] = k.sum()
    return dict(elpd_lgo=float(e.sum()), lgoic=-2.0 * float(e.sum()), se=float(np.sqrt(G * e.var(ddof=1))) if G > 1 else float("nan"),
                min_weight_ess=float(res["weight_ess"][np.isfinite(res["elpd_lgo"])].min()) if G else float("nan"), n_groups=G,
                by_outcome=by)


def accumulate(draws, y, xb, tausq):
    """The whole estimator from an iterable of (cond_mean, cond_var) per draw with fixed xb and per-row tausq: (rows, S)."""
    state, S = None, 0
    for cm, cv in draws:
        if state is None:
            state = new_state(np.size(cm))
        update(state, *draw_terms(y, xb, cm, cv, tausq))
        S += 1
    return finish(state, S), S
