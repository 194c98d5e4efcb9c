"""Diagnostic (not part of the product): joint new-point prediction (st_points_predict_joint) next to the
per-point st_points_predict on the same points.  Config #3's tree (side x side, q outcomes) and a grid_side x grid_side grid
offset by half a grid step (section 12's point set; q > 1: the q outcomes at every grid node).

    python profiles/micro/predict_joint_time.py [side] [q] [grid_side] [group] [reps]

group = 0: one joint group per site (the q outcomes of a node); group = g > 0: same-anchor runs of g points in anchor order.
The per-point call copies three n-vectors to the host, the joint call w, cond_mean and the packed cond_cov and cond_chol.
Prints device-synchronised wall times (median of reps; calls alternate between the two paths so that drift hits both),
the routes, and the algorithmic flops of st_points_info.  With SPAMTREE_LIB set to another build of the library the per-point
line is the A/B of the unchanged kernels.  For kernel times run it under `rocprofv3 --kernel-trace --stats` in a run of its own."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from spamtree_amd import _lib  # noqa: E402
if os.environ.get("SPAMTREE_LIB"):     # an older build of the library: bind only what it exports (the per-point line still runs)
    import ctypes
    older = ctypes.CDLL(os.environ["SPAMTREE_LIB"])
    for name in [s for s in _lib.SIGNATURES if not hasattr(older, s)]:
        del _lib.SIGNATURES[name]
from spamtree_amd.model import SpamTreeMV  # noqa: E402
from spamtree_amd.predict import group_sites, locate  # noqa: E402
from spamtree_amd.synthetic import make_workload  # noqa: E402

side = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
q = int(sys.argv[2]) if len(sys.argv) > 2 else 1
grid_side = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
group = int(sys.argv[4]) if len(sys.argv) > 4 else 4
reps = int(sys.argv[5]) if len(sys.argv) > 5 else 10

wl = make_workload(side, q=q, device=0) if q > 1 else make_workload(side, device=0)
g = (np.arange(grid_side) + 0.5) / (side - 1)          # the workload's grid step is 1 / (side - 1)
nodes = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
pts, mv = np.repeat(nodes, q, axis=0), np.tile(np.arange(1, q + 1), nodes.shape[0])
n = pts.shape[0]
rng = np.random.default_rng(5)
hm = SpamTreeMV(wl["y"], wl["X"], wl["Z"], wl["coords"], wl["mv_id"], wl["blocking"], wl["gix_block"], wl["res_is_ref"],
                wl["parents"], wl["children"], False, wl["block_names"], wl["block_groups"], wl["indexing"],
                rng.standard_normal(wl["n"]), np.zeros(wl["p"]), wl["theta"], 10.0, device=0)
assert hm.get_loglik_comps_w(0)
has_joint = "st_points_set_joint" in _lib.SIGNATURES
if group == 0:
    labels = group_sites(pts)
    anchor = locate(wl["topo"], pts, mv, device=0, joint=labels) if has_joint else locate(wl["topo"], pts, mv, device=0)
else:
    anchor = locate(wl["topo"], pts, mv, device=0)
    order = np.argsort(anchor, kind="stable")
    run_start = np.concatenate([[True], anchor[order][1:] != anchor[order][:-1]])
    pos = np.arange(n) - np.maximum.accumulate(np.where(run_start, np.arange(n), 0))     # position inside the anchor's run
    new_group = run_start | (pos % group == 0)
    labels = np.empty(n, dtype=np.int64)
    labels[order] = np.cumsum(new_group) - 1
sizes = np.bincount(labels)
print(f"side {side} q {q}: n = {wl['n']}, {n} new points, {sizes.size} joint groups (sizes {sizes.min()}..{sizes.max()}, mean {sizes.mean():.2f})",
      flush=True)


def timed(fn):
    hm.synchronize(); t0 = time.perf_counter()
    fn()
    hm.synchronize()
    return (time.perf_counter() - t0) * 1e3


hm.set_points(pts, mv, anchor)
hm.predict_points(mode=0, seed=1, it=0)
info_p = hm.points_info()
t_point, t_joint, t_lean = [], [], []
for i in range(reps):                                  # alternate: per-point set, joint set (set_points is outside the timing)
    hm.set_points(pts, mv, anchor)
    t_point.append(timed(lambda: hm.predict_points(mode=0, seed=1, it=i)))
    if has_joint:
        hm.set_points(pts, mv, anchor, joint=labels)
        if i == 0:                                     # host buffers once, touched: no page faults inside the timing
            cov, chol, w, mean = (np.full(k, 0.5) for k in (int(hm.joint_offsets[-1]), int(hm.joint_offsets[-1]), n, n))
            dp = lambda a: a.ctypes.data_as(hm.lib.st_points_predict_joint.argtypes[5])   # noqa: E731
            hm._check(hm.lib.st_points_predict_joint(hm.h, 0, None, 1, i, dp(w), dp(mean), dp(cov), dp(chol), None))   # warm-up
        t_joint.append(timed(lambda: hm._check(hm.lib.st_points_predict_joint(hm.h, 0, None, 1, i, dp(w), dp(mean), dp(cov), dp(chol), None))))
        t_lean.append(timed(lambda: hm._check(hm.lib.st_points_predict_joint(hm.h, 0, None, 1, i, dp(w), dp(mean), None, None, None))))
if has_joint:
    info_j = hm.points_info()
print(f"st_points_predict       {np.median(t_point):8.3f} ms (min {np.min(t_point):.3f}, max {np.max(t_point):.3f})  routes {info_p['routes']}  "
      f"{info_p['flops'] / n / 1e3:.1f} kflop / point", flush=True)
if has_joint:
    print(f"st_points_predict_joint {np.median(t_joint):8.3f} ms (min {np.min(t_joint):.3f}, max {np.max(t_joint):.3f})  routes {info_j['routes']}  "
          f"{info_j['flops'] / n / 1e3:.1f} kflop / point; ratio {np.median(t_joint) / np.median(t_point):.2f}", flush=True)
    print(f"   the same without cond_cov / cond_chol ({2 * int(hm.joint_offsets[-1])} doubles less to the host) {np.median(t_lean):8.3f} ms", flush=True)
hm.close()
