"""Diagnostic (not part of the product): kernel times of the score step on joint sets, for comparing builds of
k_score_joint_acc -- the 64-bit DPP row broadcasts (the default) against the __shfl form (k_points_score.hip compiled with
-DSC_JOINT_SHFL and linked into a second library, selected with SPAMTREE_LIB).  Config #3's tree, the side x side grid of new
points offset by half a grid step, in joint groups of 4 and then of 16 consecutive cells (k_score_joint_acc<4>, <16>); every point
carries a held-out value; `iters` saved iterations each on one state.  Run it under a kernel trace, once per library:
    [SPAMTREE_LIB=variant.so] rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- \\
        python profiles/micro/score_joint_ab.py [side] [iters] [out.npz]
out.npz receives lpd_joint and lpd of both groupings, to compare the two builds bit for bit."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from spamtree_amd.model import SpamTreeMV  # noqa: E402
from spamtree_amd.predict import locate  # noqa: E402
from spamtree_amd.synthetic import make_workload  # noqa: E402


def main():
    side = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    out = sys.argv[3] if len(sys.argv) > 3 else None
    wl = make_workload(side, device=0)
    g = (np.arange(side) + 0.5) / (side - 1)
    pts = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    n = pts.shape[0]
    rng = np.random.default_rng(3)
    Xn = rng.standard_normal((n, wl["p"]))
    y = Xn @ wl["beta_true"] + 1.5 * rng.standard_normal(n)
    mv = np.ones(n, dtype=np.int64)
    hm = SpamTreeMV(wl["y"], wl["X"], wl["Z"], wl["coords"], wl["mv_id"], wl["blocking"], wl["gix_block"], wl["res_is_ref"],
                    wl["parents"], wl["children"], False, wl["block_names"], wl["block_groups"], wl["indexing"],
                    rng.standard_normal(int(wl["n"])), wl["beta_true"], wl["theta"], 10.0, device=0)
    assert hm.get_loglik_comps_w(0)
    res = {}
    for gsz in (4, 16):
        labels = np.arange(n) // gsz
        hm.set_points(pts, mv, locate(wl["topo"], pts, mv, device=0, joint=labels), Xn, joint=labels)
        hm.set_scores(y)
        for s in range(iters):
            hm._check(hm.lib.st_points_accumulate(hm.h, 11, s, None, None, None, None))
        sc = hm.scores(crps=False)
        res[f"lpd_joint_{gsz}"], res[f"lpd_{gsz}"] = sc["lpd_joint"], sc["lpd"]
        print(f"groups of {gsz}: {len(hm.joint_groups)} groups, mean lpd_joint {np.mean(sc['lpd_joint']):.6f}, "
              f"n_degenerate {sc['n_degenerate']}", flush=True)
    hm.close()
    if out:
        np.savez(out, **res)


if __name__ == "__main__":
    main()
