"""MANUAL (MI355X): what vg_kf_add and vg_kf_match cost.  256 keyframes of 752 x 480 with 150 window points each, max_keypoints 8192, in ONE
vg_kf_add; then 256 pairs (slot i against slot i + 1) in ONE vg_kf_match.  The frames are the first eight of tests/fe_scene.moving_scene,
each used 32 times (the keypoint counts are reported).  One allocating call, reported on its own, then three repeats: wall time of the C
call (the Python packing outside the timed region; the call's own staging of the images inside it) and the device time of each launch
from events (vg_kf_out::device_ms, vg_kf_match_out::device_ms).  For the blur and the FAST score kernels: the bytes they must move (one
read and one write of every pixel) over their time, as a fraction of the 6.3 TB/s of HBM bandwidth that is achievable on this part.
The project has no host KeyFrame to compare with: no speed-up is claimed.

usage: python tests/manual/gpu_kf_brief.py [--out profiles/kf_brief.json]"""
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
N_KF, N_WINDOW, MAX_KP, REPEATS, DISTINCT = 256, 150, 8192, 3, 8
W, H = 752, 480
HBM_ACHIEVABLE = 6.3e12


def run():
    import __graft_entry__ as g
    g.load_package()
    from vins_mono_amd import ba, fe
    import fe_scene
    import kf_brief_ref as K
    scene = fe_scene.moving_scene(DISTINCT)
    imgs = [scene[i % DISTINCT] for i in range(N_KF)]
    cam = K.camera_struct(K.cameras(W)["pinhole"])
    rng = np.random.default_rng(11)
    wins = [np.stack([rng.uniform(20, W - 20, N_WINDOW), rng.uniform(20, H - 20, N_WINDOW)], 1).astype(np.float32) for _ in range(N_KF)]
    res = dict(what=f"vg_kf_add, {N_KF} keyframes of {W} x {H}, {N_WINDOW} window points, max_keypoints {MAX_KP}; vg_kf_match, {N_KF} pairs; one allocating "
                    f"call, then {REPEATS} repeats", launches=fe.KF_KERNELS, frames=f"the first {DISTINCT} frames of fe_scene.moving_scene, each {N_KF // DISTINCT} times")
    h = ba.Handle()
    kf = fe.KeyFrames(h, W, H, MAX_KP, N_WINDOW, N_KF, K.pattern())
    # the structs once, outside the timed region
    ins, outs = (fe.KfIn * N_KF)(), (fe.KfOut * N_KF)()
    ms = np.zeros(fe.KF_ADD_LAUNCHES, np.float32)
    for i in range(N_KF):
        a = ins[i]
        a.struct_size, a.slot, a.img, a.stride = C.sizeof(fe.KfIn), i, imgs[i].ctypes.data_as(fe._u8), W
        a.n_window, a.window_xy, a.camera = N_WINDOW, wins[i].ctypes.data_as(fe._f4), cam
        outs[i].struct_size = C.sizeof(fe.KfOut)
    outs[0].device_ms = ms.ctypes.data_as(fe._f4)
    wall, dev = [], []
    for rep in range(REPEATS + 1):
        t0 = time.perf_counter()
        rc = h.lib.vg_kf_add(h.h, N_KF, ins, outs)
        wall.append((time.perf_counter() - t0) * 1e3)
        assert rc == 0, h.lib.vg_last_error(h.h)
        dev.append([float(x) for x in ms])
    counts = [int(o.n_keypoints) for o in outs]
    ref = [K.fast(scene[i])[0] for i in range(DISTINCT)]
    assert counts[:DISTINCT] == [len(r) for r in ref], "the keypoint counts equal the reference's"
    assert all(int(o.status) == fe.KF_OK for o in outs)
    moved = 2.0 * W * H * N_KF
    res["kf_add"] = dict(allocating_call_wall_ms=wall[0], call_wall_ms=wall[1:], device_ms_per_launch=dev[1:], device_ms_total=[sum(d) for d in dev[1:]],
                         keypoints_of_the_distinct_frames=counts[:DISTINCT], keypoints_min_max=[min(counts), max(counts)],
                         bytes_blur_and_fast_must_move_each=moved,
                         blur_fraction_of_achievable_hbm=[moved / (d[0] * 1e-3) / HBM_ACHIEVABLE for d in dev[1:]],
                         fast_score_fraction_of_achievable_hbm=[moved / (d[1] * 1e-3) / HBM_ACHIEVABLE for d in dev[1:]],
                         upload_bytes=float(W * H * N_KF))
    # one keyframe per call: the per-keyframe use, latency-bound
    one = []
    for rep in range(REPEATS + 1):
        t0 = time.perf_counter()
        rc = h.lib.vg_kf_add(h.h, 1, ins, outs)
        one.append((time.perf_counter() - t0) * 1e3)
        assert rc == 0
    res["kf_add_one_keyframe"] = dict(first_call_wall_ms=one[0], call_wall_ms=one[1:])
    # ---- the match
    pairs, mouts = (fe.KfPair * N_KF)(), (fe.KfMatchOut * N_KF)()
    mms = np.zeros(1, np.float32)
    bufs = []
    for i in range(N_KF):
        pairs[i].struct_size, pairs[i].cur_slot, pairs[i].old_slot = C.sizeof(fe.KfPair), i, (i + 1) % N_KF
        b = (np.zeros(N_WINDOW, np.int32), np.zeros(N_WINDOW, np.int32), np.zeros(N_WINDOW, np.uint8), np.zeros(N_WINDOW, np.int32))
        q = mouts[i]
        q.struct_size = C.sizeof(fe.KfMatchOut)
        q.best_idx, q.best_dist, q.status, q.matched_index = b[0].ctypes.data_as(fe._i4), b[1].ctypes.data_as(fe._i4), b[2].ctypes.data_as(fe._u8), b[3].ctypes.data_as(fe._i4)
        bufs.append(b)
    mouts[0].device_ms = mms.ctypes.data_as(fe._f4)
    wall, dev = [], []
    for rep in range(REPEATS + 1):
        t0 = time.perf_counter()
        rc = h.lib.vg_kf_match(h.h, N_KF, pairs, mouts)
        wall.append((time.perf_counter() - t0) * 1e3)
        assert rc == 0, h.lib.vg_last_error(h.h)
        dev.append(float(mms[0]))
    nm = [int(o.n_matched) for o in mouts]
    # pair 0 against the reference
    r0, r1 = K.keyframe(scene[0], K.cameras(W)["pinhole"], wins[0]), K.keyframe(scene[1], K.cameras(W)["pinhole"], wins[1])
    want = K.match(r0["window_descriptors"], r1["descriptors"], r1["keypoints"], r1["norm"])
    assert np.array_equal(bufs[0][0], want["best_idx"]) and np.array_equal(bufs[0][1], want["best_dist"]) and nm[0] == want["n_matched"]
    res["kf_match"] = dict(allocating_call_wall_ms=wall[0], call_wall_ms=wall[1:], device_ms=dev[1:], n_matched_min_max=[min(nm), max(nm)],
                           descriptor_pairs_per_call=float(sum(N_WINDOW * c for c in counts)))
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
