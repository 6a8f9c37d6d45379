"""MANUAL (MI355X): what vg_init_sfm costs.  256 windows of F = 11 frames, 150 features, one non-key frame inside every interval, three
repeats after one warm-up: wall time of the C call (packing outside the timed region) and the device time of its two launches from
events (vg_sfm_out::device_ms).  The project has no host SfM to compare with: no speed-up is claimed; vg_init_align over the same
number of windows takes 2.1 ms (profiles/init_align.json).

usage: python tests/manual/gpu_init_sfm.py [--out profiles/init_sfm_measured.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
N_WIN, F, N_FEAT, REPEATS = 256, 11, 150, 3


def run():
    import numpy as np
    import __graft_entry__ as g
    g.load_package()
    from vins_mono_amd import ba
    import init_sfm_ref as S
    wins = [S.scene(7000 + i, F=F, l=int(i % (F - 1)), n_feat=N_FEAT, nonkey=True) for i in range(N_WIN)]
    h = ba.Handle()
    ins, outs, keep = h.init_sfm_pack(wins, timed=True)
    wall, dev = [], []
    for rep in range(REPEATS + 1):
        t0 = time.perf_counter()
        rc = h.lib.vg_init_sfm(h.h, N_WIN, ins, outs)
        t1 = time.perf_counter()
        assert rc == 0, h.lib.vg_last_error(h.h)
        if rep:
            wall.append((t1 - t0) * 1e3)
            dev.append([float(x) for x in keep[0]['device_ms']])
    status = [int(o.status) for o in outs]
    iters = [int(o.ba_iters) for o in outs]
    res = dict(what=f"vg_init_sfm, {N_WIN} windows, F = {F}, {N_FEAT} features, one non-key frame per interval ({N_WIN * (F - 1)} frame PnPs), "
                    f"{REPEATS} repeats after one warm-up",
               call_wall_ms=wall, device_ms_window_kernel=[d[0] for d in dev], device_ms_frame_kernel=[d[1] for d in dev],
               statuses={str(s): status.count(s) for s in sorted(set(status))}, ba_iterations_mean=float(np.mean(iters)),
               ba_iterations_max=int(np.max(iters)), init_align_ms_same_window_count=2.1)
    h.close()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    r = run()
    print(json.dumps(r, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)
