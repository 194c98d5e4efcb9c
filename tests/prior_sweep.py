"""NumPy restatement of the prior sweep of st_simulate, from the oracle's per-block factors (tests only).

For every block u in level order: w_u = H_u w_pa(u) + chol(R_u) z_u, with H_u = w_cond_mean_K[u] and chol(R_u) the inverse of
Rcc_invchol[u] (reference levels) or diag(1 / ccholprecdiag[u]) (non-reference levels)."""
import numpy as np


def prior_sweep(om, Z):
    """Z: n x k normals (the model's sorted row order); returns W (n x k) drawn top-down through `om.param_data`."""
    Z = np.asarray(Z, dtype=np.float64)
    Z = Z[:, None] if Z.ndim == 1 else Z
    d = om.param_data
    W = np.zeros_like(Z)
    labels = np.unique(om.block_groups)
    nb = len(om.indexing)
    order = sorted(range(nb), key=lambda u: int(np.nonzero(labels == om.block_groups[u])[0][0]))
    for u in order:
        iu = om.indexing[u]
        if iu.size == 0:
            continue
        g = int(np.nonzero(labels == om.block_groups[u])[0][0])
        if om.res_is_ref[g] == 1:
            e = np.linalg.solve(np.tril(d.Rcc_invchol[u]), Z[iu])
        else:
            e = Z[iu] / np.asarray(d.ccholprecdiag[u]).reshape(-1, 1)
        if len(om.parents[u]):
            e = e + d.w_cond_mean_K[u] @ W[om.parents_indexing[u]]
        W[iu] = e
    return W
