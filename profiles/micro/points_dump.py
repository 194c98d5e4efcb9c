"""Diagnostic (not part of the product): everything st_points_* returns on the point sets of tests/test_points_layout_cpu.py
(imported from there, so that the CPU check of the layout and this comparison see the same sets), for the bitwise comparison
of two builds of the library (SPAMTREE_LIB), and the host time of st_points_set / st_points_set_joint.

    python profiles/micro/points_dump.py dump OUT.npz          every output of every row (one process per build)
    python profiles/micro/points_dump.py compare A.npz B.npz   bitwise; exit status 1 at the first difference
    python profiles/micro/points_dump.py time [side] [reps]    st_points_set, st_points_set_joint on side x side points (config #3's tree)

dump, per row: st_points_predict (w, mean, var, yhat from a caller's z) and st_points_info; two st_points_accumulate and
st_points_summary_get; on a joint row the same through st_points_set_joint with st_points_joint_layout, the packed cond_cov and
cond_chol and st_points_summary_get_cov.  (deep5_lds64k is left out: on a device with 160 KB of LDS it is deep5_lds160k.)"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from spamtree_amd.model import SpamTreeMV  # noqa: E402

dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731


def model(pb, force_generic=False):
    rng = np.random.default_rng(6)
    hm = SpamTreeMV(pb["y"], pb["X"], pb["Z"], pb["coords"], pb["mv_id"], pb["blocking"], pb["gix_block"], pb["res_is_ref"],
                    pb["parents"], pb["children"], False, pb["block_names"], pb["block_groups"], pb["indexing"],
                    rng.standard_normal(pb["n"]), rng.standard_normal(pb["p"]), pb["theta"], 5.0, device=0, force_generic=force_generic)
    assert hm.get_loglik_comps_w(0)
    return hm


def summaries(hm, n, joint, res, tag):
    """Two accumulated iterations (seed 11, iterations 0 and 1) and the summaries behind them."""
    lib, h = hm.lib, hm.h
    tot = int(hm.joint_offsets[-1]) if joint else 0
    hm._check(lib.st_points_summary_reset(h))
    for it in range(2):
        o = np.zeros((4, n))
        yh = dp(o[3]) if n else None
        if joint:
            cov, chol = np.zeros(tot), np.zeros(tot)
            hm._check(lib.st_points_accumulate_joint(h, 11, it, dp(o[0]), dp(o[1]), dp(cov), dp(chol), yh))
            res[f"{tag}/acc{it}_cov"], res[f"{tag}/acc{it}_chol"] = cov, chol
        else:
            hm._check(lib.st_points_accumulate(h, 11, it, dp(o[0]), dp(o[1]), dp(o[2]), yh))
        res[f"{tag}/acc{it}"] = o
    if n == 0:
        return
    s = np.zeros((4, n))
    cnt = C.c_int64()
    hm._check(lib.st_points_summary_get(h, dp(s[0]), dp(s[1]), dp(s[2]), dp(s[3]), C.byref(cnt)))
    res[f"{tag}/summary"], res[f"{tag}/n_accumulated"] = s, np.array([cnt.value])
    if joint:
        cov = np.zeros(tot)
        hm._check(lib.st_points_summary_get_cov(h, dp(cov)))
        res[f"{tag}/summary_cov"] = cov


def dump(path):
    from tests.test_points_layout_cpu import CASES
    res = {}
    for rid, (maker, points, joint, _, flags, _) in CASES.items():
        if rid == "deep5_lds64k":
            continue
        pb = maker()
        coords, mv, anchor, labels = points(pb, 7)
        n = anchor.size
        rng = np.random.default_rng(12)
        z, X = rng.standard_normal(n), rng.standard_normal((n, pb["p"]))
        hm = model(pb, "force-generic" in flags)
        for jt in ([False, True] if joint else [False]):
            tag = rid + ("/joint" if jt else "/plain")
            hm.set_points(coords, mv, anchor, X if n else None, joint=labels if jt else None)   # (an empty set keeps no regressors)
            out = hm.predict_points(mode=0, z=z)
            info = hm.points_info()
            for k in ("w", "mean", "var") + (("yhat",) if n else ()) + (("cov_packed", "chol_packed") if jt else ()):
                res[f"{tag}/{k}"] = out[k]
            res[f"{tag}/info"] = np.array([info["n_groups"], info["alg_bytes"], info["flops"]])
            res[f"{tag}/routes"] = np.array(",".join(info["routes"]))
            if jt:
                res[f"{tag}/j_off"] = hm.joint_offsets
                res[f"{tag}/j_members"] = np.concatenate(hm.joint_groups) if hm.joint_groups else np.zeros(0, dtype=np.int64)
                res[f"{tag}/j_sizes"] = np.array([g.size for g in hm.joint_groups])
            summaries(hm, n, jt, res, tag)
            print(f"{tag}: n = {n}, routes {info['routes']}", flush=True)
        hm.close()
    np.savez(path, **res)
    print(f"{len(res)} arrays -> {path}")


def compare(a, b):
    A, B = np.load(a), np.load(b)
    assert sorted(A.files) == sorted(B.files), set(A.files) ^ set(B.files)
    bad = 0
    for k in sorted(A.files):
        x, y = A[k], B[k]
        same = x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()
        print(f"{'same     ' if same else 'DIFFERENT'} {k} {x.dtype} {x.shape}")
        bad += not same
    print(f"{len(A.files)} arrays, {bad} differ")
    return 1 if bad else 0


def time_set(side, reps):
    from spamtree_amd.predict import locate
    from spamtree_amd.synthetic import make_workload
    wl = make_workload(side, device=0)
    hm = model(wl)
    g = (np.arange(side) + 0.5) / (side - 1)
    pts = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    n = pts.shape[0]
    mv = np.ones(n, dtype=np.int64)
    anchor = np.ascontiguousarray(locate(wl["topo"], pts, mv, device=0))
    order = np.argsort(anchor, kind="stable")
    run_start = np.concatenate([[True], anchor[order][1:] != anchor[order][:-1]])
    pos = np.arange(n) - np.maximum.accumulate(np.where(run_start, np.arange(n), 0))     # position inside the anchor's run
    labels = np.empty(n, dtype=np.int64)
    labels[order] = np.cumsum(run_start | (pos % 4 == 0)) - 1                            # same-anchor runs of four points
    c = np.asfortranarray(pts)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))   # noqa: E731
    ts = {"st_points_set": [], "st_points_set_joint": []}
    for _ in range(reps):
        hm.synchronize(); t0 = time.perf_counter()
        hm._check(hm.lib.st_points_set(hm.h, n, dp(c), ip(mv), ip(anchor), None))
        hm.synchronize(); t1 = time.perf_counter()
        hm._check(hm.lib.st_points_set_joint(hm.h, n, dp(c), ip(mv), ip(anchor), None, ip(labels)))
        hm.synchronize(); t2 = time.perf_counter()
        ts["st_points_set"].append((t1 - t0) * 1e3); ts["st_points_set_joint"].append((t2 - t1) * 1e3)
    for k, v in ts.items():
        print(f"{k} side {side} ({n} points): median {np.median(v):.2f} ms (min {np.min(v):.2f}, max {np.max(v):.2f}) over {reps}", flush=True)
    hm.close()


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        time_set(int(sys.argv[2]) if len(sys.argv) > 2 else 1000, int(sys.argv[3]) if len(sys.argv) > 3 else 5)
