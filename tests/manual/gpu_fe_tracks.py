"""MANUAL (not collected): vg_fe_tracks_step against what a caller has without it, 256 streams x 150 points, 752x480, CLAHE on, published
and unpublished steps alternating; host clock around calls that end in a synchronise, every leg warmed up first.

  a   vg_fe_read_image_batch + the list bookkeeping of FeatureTracker / the node on the host, in C (vins_host_fe_tracks_leg mode 0 of
      host/host_test_api.cpp: vectors reduced in place, std::map for prev_un_pts_map and the message)
  b   vg_fe_tracks_step (mode 1 of the same loop)
  Both evolve the same lists over the same frames (the message of the last step must agree), in ONE process, interleaved, `--repeats`
  times each, with frames from pageable host memory and with frames resident on the device.
  parent  vg_fe_read_image_batch alone (leg `a` / `b` of tests/manual/gpu_fe_batch_frames.py), this tree's library against the parent
      commit's (--parent-lib), each run in a child process of its own, interleaved.

    python tests/manual/gpu_fe_tracks.py [--parent-lib <libvinsgpu.so of the parent commit>] [--out profiles/fe_tracks.json]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as graft  # noqa: E402

pkg = graft.load_package()
if "--child" in sys.argv and "--parent-lib" in sys.argv:
    pkg.LIB_PATH = sys.argv[sys.argv.index("--parent-lib") + 1]      # (before the first handle loads it)
from vins_mono_amd import ba, fe, synth  # noqa: E402

W, H, NPTS, MIN_DIST = 752, 480, 150, 30
INTR = (461.6, 460.3, 363.0, 248.1, -2.917e-01, 8.228e-02, 5.333e-05, -1.578e-04)
_u8 = C.POINTER(C.c_uint8)


def spread(vals):
    return dict(values=vals, median=float(np.median(vals)), min=float(min(vals)), max=float(max(vals)), spread=float(max(vals) - min(vals)))


def frames_of(S, kinds=16):
    a = [synth.synth_frame(3 + c) for c in range(min(S, kinds))]
    b = [synth.warp_frame(a[c], 4 + c) for c in range(len(a))]
    return [np.ascontiguousarray(np.stack([x[c % len(a)] for c in range(S)])) for x in (a, b)]


def leg(host, buf, S, mode, resident, warm, steps):
    """one run of the C loop on a fresh handle; returns (ms per step, entries of the last message, sum of its ids)"""
    h = ba.Handle()
    fe.FrontEnd(h, W, H, S, NPTS)
    ptrs = (_u8 * (2 * S))(*[C.cast(buf[k].ctypes.data + c * W * H, _u8) for k in range(2) for c in range(S)])
    slots = (C.c_int * 2)(0, 0)
    if resident:
        # frame A into one slot, frame B into the other (an upload fills the slot of the pyramid set the next build fills; the build
        # between the two rotates the sets); the timed calls select a slot and pass no image
        for k in range(2):
            one = (_u8 * S)(*[ptrs[k * S + c] for c in range(S)])
            h._chk(h.lib.vg_fe_upload_frames(h.h, one, W), "upload")
            slots[k] = int(h.lib.vg_fe_frame_slot(h.h))
            if k == 0:
                h._chk(h.lib.vg_fe_build_async(h.h, 1), "build")
        assert slots[0] != slots[1]
    out = (C.c_double * 3)()
    intr = (C.c_double * 8)(*INTR)
    rc = host.vins_host_fe_tracks_leg(h.h, S, mode, None if resident else ptrs, slots, W, NPTS, MIN_DIST, intr, warm, steps, out)
    h._chk(rc, "vins_host_fe_tracks_leg mode %d" % mode)
    h.close()
    return out[0] / steps * 1e3, int(out[1]), int(out[2])


def parent_leg_in_child(S, seconds, lib_path):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", str(S), "--seconds", str(seconds)]
    if lib_path:
        cmd += ["--parent-lib", os.path.abspath(lib_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("child leg failed (%d):\n%s" % (r.returncode, r.stderr[-2000:]))
    return json.loads([line for line in r.stdout.splitlines() if line.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warm", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--child", type=int, default=0)
    a = ap.parse_args()
    if a.child:                                        # vg_fe_read_image_batch alone on the library chosen before anything was loaded
        import gpu_fe_batch_frames as B
        scene = B.Scene(a.child)
        print(json.dumps({m: B.leg_batch(scene, a.seconds, m)["ms_per_step"] for m in ("a", "b")}))
        return
    S = a.streams
    host = C.CDLL(os.path.join(os.path.dirname(pkg.LIB_PATH), "libvins_host.so"))
    host.vins_host_fe_tracks_leg.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(_u8), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int,
                                             C.POINTER(C.c_double), C.c_int, C.c_int, C.POINTER(C.c_double)]
    buf = frames_of(S)
    h = ba.Handle()
    res = dict(what=__doc__.split("\n\n")[0].replace("\n", " "), status="measured",
               shape=dict(streams=S, width=W, height=H, points=NPTS, min_dist=MIN_DIST, equalize=1, steps=a.steps, warm=a.warm, repeats=a.repeats))
    try:
        res["clock_probe"] = h.probe_clocks()
    except Exception as ex:  # noqa: BLE001
        res["clock_probe"] = "unavailable: %r" % (ex,)
    h.close()
    for name, resident in (("frames_from_pageable_host_memory", False), ("frames_resident_on_the_device", True)):
        ms = {0: [], 1: []}
        msg = {}
        for rep in range(a.repeats):
            for mode in (0, 1):
                t, n_msg, id_sum = leg(host, buf, S, mode, resident, a.warm, a.steps)
                ms[mode].append(t)
                msg.setdefault(mode, (n_msg, id_sum))
                assert msg[mode] == (n_msg, id_sum), "a leg is not repeatable"
        assert msg[0] == msg[1] and msg[0][0] > 0, ("the two legs did not end with the same message", msg)
        r = dict(a_batch_plus_host_lists_ms_per_step=spread(ms[0]), b_tracks_step_ms_per_step=spread(ms[1]), last_message_entries=msg[0][0])
        worst = max(r["a_batch_plus_host_lists_ms_per_step"]["spread"], r["b_tracks_step_ms_per_step"]["spread"])
        r["b_minus_a_ms"] = r["b_tracks_step_ms_per_step"]["median"] - r["a_batch_plus_host_lists_ms_per_step"]["median"]
        r["b_not_slower_than_a_by_more_than_the_larger_spread"] = bool(r["b_minus_a_ms"] <= worst)
        res[name] = r
        print(name, json.dumps(r), flush=True)
    if a.parent_lib:
        here, parent = [], []
        for rep in range(a.repeats):
            here.append(parent_leg_in_child(S, a.seconds, None))
            parent.append(parent_leg_in_child(S, a.seconds, a.parent_lib))
        res["read_image_batch_alone_ms_per_step"] = {m: dict(this_tree=spread([x[m] for x in here]), parent=spread([x[m] for x in parent]))
                                                     for m in ("a", "b")}
        print("parent", json.dumps(res["read_image_batch_alone_ms_per_step"]), flush=True)
    else:
        res["read_image_batch_alone_ms_per_step"] = "not run: --parent-lib was not given"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
