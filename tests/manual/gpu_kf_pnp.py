"""MANUAL (MI355X): what vg_kf_pnp costs.  256 pairs of 150 matches at 30 % outliers in ONE call (refine 0 and refine 1); the same 256 pairs
one per call; a batch of 256 clean pairs (0 % outliers), which shows what the chunked evaluation saves: a clean pair's bound drops below
KP_CHUNK0 in the first part and the second part's kernels find nothing to do.  One allocating call, reported on its own, then three repeats:
wall time of the C call (the Python packing outside the timed region) and the device time of each launch from events
(vg_kf_pnp_out::device_ms).  The project has no host PnPRANSAC to compare with: no speed-up is claimed.

usage: python tests/manual/gpu_kf_pnp.py [--out profiles/kf_pnp.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
N_PAIRS, N_MATCH, REPEATS = 256, 150, 3


def structs(fe, h, pairs, keep):
    n = len(pairs)
    ins, outs = (fe.KfPnpIn * n)(), (fe.KfPnpOut * n)()
    for i, p in enumerate(pairs):
        a, o = ins[i], outs[i]
        h.lib.vg_kf_pnp_defaults(C.byref(a))
        p3, p2, ids = np.ascontiguousarray(p["point_3d"], np.float32), np.ascontiguousarray(p["old_norm"], np.float32), np.ascontiguousarray(p["point_id"], np.int32)
        a.n, a.point_3d, a.old_norm, a.point_id, a.refine = len(p3), p3.ctypes.data_as(fe._f4), p2.ctypes.data_as(fe._f4), ids.ctypes.data_as(fe._i4), int(p["refine"])
        for k, cnt in (("origin_vio_T", 3), ("origin_vio_R", 9), ("tic", 3), ("qic", 9)):
            setattr(a, k, (C.c_double * cnt)(*np.asarray(p[k], np.float64).reshape(-1)))
        b = (np.zeros(len(p3), np.uint8), np.zeros(len(p3), np.int32), np.zeros(len(p3), np.int32), np.zeros((len(p3), 2), np.float64))
        o.struct_size = C.sizeof(fe.KfPnpOut)
        o.mask, o.matched_index, o.match_id, o.match_xy = b[0].ctypes.data_as(fe._u8), b[1].ctypes.data_as(fe._i4), b[2].ctypes.data_as(fe._i4), b[3].ctypes.data_as(fe._f8)
        keep.append((p3, p2, ids, b))
    return ins, outs


def timed(fe, h, pairs, per_call):
    keep = []
    ins, outs = structs(fe, h, pairs, keep)
    ms = np.zeros(fe.KF_PNP_LAUNCHES, np.float32)
    outs[0].device_ms = ms.ctypes.data_as(fe._f4)
    n = len(pairs)
    wall, dev = [], []
    for rep in range(REPEATS + 1):
        t0 = time.perf_counter()
        if per_call:
            for i in range(n):
                rc = h.lib.vg_kf_pnp(h.h, 1, C.byref(ins, i * C.sizeof(fe.KfPnpIn)), C.byref(outs, i * C.sizeof(fe.KfPnpOut)))
                assert rc == 0, h.lib.vg_last_error(h.h)
        else:
            rc = h.lib.vg_kf_pnp(h.h, n, ins, outs)
            assert rc == 0, h.lib.vg_last_error(h.h)
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append([float(x) for x in ms])
    st = [int(o.status) for o in outs]
    d = dict(allocating_call_wall_ms=wall[0], call_wall_ms=wall[1:], statuses_ok=st.count(0), inliers_min_max=[min(int(o.n_inliers) for o in outs), max(int(o.n_inliers) for o in outs)],
             ransac_bound_min_max=[min(int(o.ransac_bound) for o in outs), max(int(o.ransac_bound) for o in outs)], has_loop=sum(int(o.has_loop) for o in outs),
             # a pair whose winning iteration lies in the second part still had a bound above KP_CHUNK0 (30) after the first: it alone keeps the
             # second sample launch busy for one more dependent chain
             pairs_that_went_on_in_the_second_part=sum(1 for o in outs if int(o.ransac_best) >= 30), last_iteration_max=max(int(o.ransac_iter) for o in outs))
    if per_call:
        d["wall_ms_per_pair"] = [w / n for w in wall[1:]]
        d["device_ms_per_launch_of_the_last_pair"] = dev[1:]
    else:
        d["device_ms_per_launch"] = dev[1:]
        d["device_ms_total"] = [sum(x) for x in dev[1:]]
    return d, outs, keep


def run():
    import __graft_entry__ as g
    g.load_package()
    from vins_mono_amd import ba, fe
    import kf_pnp_ref as K
    h = ba.Handle()
    h.lib.vg_kf_pnp_defaults.argtypes = [C.POINTER(fe.KfPnpIn)]
    h.lib.vg_kf_pnp_defaults.restype = None
    h.lib.vg_kf_pnp.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    res = dict(what=f"vg_kf_pnp, {N_PAIRS} pairs of {N_MATCH} matches; one allocating call, then {REPEATS} repeats", launches=fe.KF_PNP_KERNELS)
    out30 = [K.scene(1000 + i, n=N_MATCH, outlier=0.3) for i in range(N_PAIRS)]
    clean = [K.scene(2000 + i, n=N_MATCH, outlier=0.0) for i in range(N_PAIRS)]
    res["batch_30pct_outliers"], outs, _ = timed(fe, h, out30, False)
    # pair 0 against the reference's decisions
    ref = K.reference(out30[0])
    assert (outs[0].status, outs[0].n_inliers, outs[0].ransac_best, outs[0].ransac_bound, outs[0].has_loop) == \
        (ref['status'], ref['n_inliers'], ref['ransac_best'], ref['ransac_bound'], ref['has_loop'])
    res["batch_30pct_outliers_refine_1"], _, _ = timed(fe, h, [dict(p, refine=1) for p in out30], False)
    res["batch_clean"], _, _ = timed(fe, h, clean, False)
    res["one_pair_per_call_30pct_outliers"], _, _ = timed(fe, h, out30, True)
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
