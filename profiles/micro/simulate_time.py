"""Diagnostic (not part of the product): time of st_simulate (prior draws from slot 0) at config #3's tree (n = 1e6, q = 1)
and config #4's shape (side 577, q = 3).  Per call: device-synchronised wall time, median of 10, with the draws left on the
device (w_out = y_out = NULL: no copy to the host); nd = 1 and nd = 16.  The algorithmic bytes are st_simulate_info's (every
slot-0 panel once + 8 nd B per row for z, eps, w, y and the ancestor gathers + XB); the fraction is of 8 TB/s.  Kernel times:
run this under `rocprofv3 --kernel-trace --stats` in a separate run.
    python profiles/micro/simulate_time.py [configs...]        (3, 4; default both)  -> one JSON line per (config, nd)"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from spamtree_amd.model import SpamTreeMV  # noqa: E402
from spamtree_amd.synthetic import make_workload  # noqa: E402

CONFIGS = {"3": (1000, 1), "4": (577, 3)}
HBM = 8.0e12


def main(names):
    for name in names:
        side, q = CONFIGS[name]
        wl = make_workload(side, q=q, p=3)
        n = wl["n"]
        hm = SpamTreeMV(wl["y"], wl["X"], wl["Z"], wl["coords"], wl["mv_id"], wl["blocking"], wl["gix_block"], wl["res_is_ref"],
                        wl["parents"], wl["children"], False, wl["block_names"], wl["block_groups"], wl["indexing"],
                        np.zeros(n), wl["beta_true"], wl["theta"], 10.0, device=0)
        assert hm.get_loglik_comps_w(0)
        for nd in (1, 16):
            info = hm.simulate_info(nd)
            t = []
            for r in range(13):
                hm._check(hm.lib.st_synchronize(hm.h))
                t0 = time.perf_counter()
                hm._check(hm.lib.st_simulate(hm.h, nd, None, None, 2021, r * nd, None, None))
                hm._check(hm.lib.st_synchronize(hm.h))
                if r >= 3:
                    t.append(time.perf_counter() - t0)
            ms = float(np.median(t)) * 1e3
            # the timed call writes no y: count the bytes of what it moves (z, w, gathers: 3 x 8 nd per row; no eps / y / XB)
            bytes_ = info["alg_bytes"] - n * (2 * 8.0 * nd + 8.0)
            print(json.dumps(dict(config=name, n=n, q=q, nd=nd, ms_per_call=ms, ms_per_draw=ms / nd, alg_bytes=bytes_,
                                  frac_of_8TBps=bytes_ / (ms * 1e-3) / HBM, routes=info["routes"])), flush=True)
        hm.close()


if __name__ == "__main__":
    main(sys.argv[1:] or ["3", "4"])
