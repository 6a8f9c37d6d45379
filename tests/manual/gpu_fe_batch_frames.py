"""MANUAL (not collected): whole readImage frames per second over S camera streams, vg_fe_read_image_batch on one handle against what a
caller had before it -- S single-stream handles driven in a loop -- at 752x480, 150 points, CLAHE on, alternating published and
unpublished steps.  Host clock around calls that end in a synchronise; every shape is warmed up first; every leg runs for at least
`--seconds` of timed work.

  a    vg_fe_read_image_batch, frames in pageable host memory (one buffer for all streams)
  a_reg the same from a buffer registered with vg_host_register
  b    the same with the frames resident on the device (imgs NULL: device work + the small transfers)
  c    S handles, vg_fe_read_image in a loop on ONE host thread, library given by --parent-lib (the build before the batched call)
  c8   the same from 8 host threads
  a and c are repeated three times, alternating, to get the spread.  At S = 1 the single call of this tree runs against the parent's.
  Every leg on the parent's library runs in a child process of its own (--child): the package loads its library with RTLD_GLOBAL, two
  builds of it in one process would bind each other's symbols.

    python tests/manual/gpu_fe_batch_frames.py --parent-lib <libvinsgpu.so of the parent commit> [--out profiles/fe_batch_frames.json]
    python tests/manual/gpu_fe_batch_frames.py --only b --sizes 256        (the leg a kernel trace is taken of; no parent library needed)"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

pkg = graft.load_package()
if "--child" in sys.argv and "--parent-lib" in sys.argv:
    pkg.LIB_PATH = sys.argv[sys.argv.index("--parent-lib") + 1]      # (before the first handle loads it)
from vins_mono_amd import ba, fe, synth  # noqa: E402

W, H, NPTS = 752, 480, 150
INTR = (461.6, 460.3, 363.0, 248.1, -2.917e-01, 8.228e-02, 5.333e-05, -1.578e-04)
_u8, _f4 = C.POINTER(C.c_uint8), C.POINTER(C.c_float)


def single_leg_in_child(S, seconds, lib_path, threads=1):
    """leg_single in a fresh process whose package loads `lib_path` (None: this tree's library)"""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", str(S), "--threads", str(threads), "--seconds", str(seconds)]
    if lib_path:
        cmd += ["--parent-lib", os.path.abspath(lib_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("child leg failed (%d):\n%s" % (r.returncode, r.stderr[-2000:]))
    return json.loads([line for line in r.stdout.splitlines() if line.startswith("{")][-1])


def frame_in(img_ptr, pts, publish):
    f = fe.FrameIn()
    f.struct_size = C.sizeof(fe.FrameIn)
    f.img = img_ptr
    f.stride = W; f.equalize = 1; f.publish = int(publish)
    f.cur_xy = pts.ctypes.data_as(_f4) if len(pts) else None
    f.n = len(pts); f.max_cnt = NPTS; f.min_dist = 30; f.quality = 0.01; f.f_threshold = 1.0; f.focal_length = 460.0
    for i, v in enumerate(INTR):
        f.intr[i] = v
    f.order = C.cast(None, fe.ORDER_FN)
    return f


class Scene:
    """two frames per stream in ONE buffer each, and the corners of either frame (the point lists of the timed steps)"""

    def __init__(self, S, kinds=16):
        a = [synth.synth_frame(3 + c) for c in range(min(S, kinds))]
        b = [synth.warp_frame(a[c], 4 + c) for c in range(len(a))]
        self.S = S
        self.buf = [np.ascontiguousarray(np.stack([x[c % len(a)] for c in range(S)])) for x in (a, b)]
        h = ba.Handle()
        one = fe.FrontEnd(h, W, H, 1, NPTS)
        self.pts = [[], []]
        for c in range(len(a)):
            for k, img in enumerate((a[c], b[c])):
                one = fe.FrontEnd(h, W, H, 1, NPTS)
                self.pts[k].append(np.ascontiguousarray(one.read_image(img, np.zeros((0, 2), np.float32), True, INTR, max_cnt=NPTS, equalize=True)["new_xy"]))
        h.close()
        self.pts = [[p[c % len(a)] for c in range(S)] for p in self.pts]

    def img_ptr(self, k, c):
        return C.cast(self.buf[k].ctypes.data + c * W * H, _u8)

    def inputs(self, resident=False):
        """step 0: frame B with A's corners, published; step 1: frame A with B's corners, not published"""
        out = []
        for step, (k, publish) in enumerate(((1, True), (0, False))):
            arr = (fe.FrameIn * self.S)()
            for c in range(self.S):
                arr[c] = frame_in(None if resident else self.img_ptr(k, c), self.pts[1 - k][c], publish)
            out.append(arr)
        return out


def timed(step_fn, seconds, warm=2):
    for k in range(2 * warm):
        step_fn(k)
    n, t0 = 0, time.perf_counter()
    while True:
        step_fn(n); step_fn(n + 1)
        n += 2
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return n, dt


def chk(h, rc, what):
    h._chk(rc, what)


def leg_batch(scene, seconds, mode):
    S = scene.S
    h = ba.Handle()
    tr = fe.FrontEnd(h, W, H, S, NPTS)
    L = h.lib
    ins = scene.inputs(resident=(mode == "b"))
    outs = (fe.FrameOut * S)()
    first = (fe.FrameIn * S)()
    for c in range(S):
        first[c] = frame_in(scene.img_ptr(0, c), np.zeros((0, 2), np.float32), True)
    chk(h, L.vg_fe_read_image_batch(h.h, S, first, outs), "first frame")
    if mode == "a_reg":
        for b in scene.buf:
            h.host_register(b)
    slots = {}
    if mode == "b":
        for k in (1, 0):
            ptrs = (_u8 * S)(*[scene.img_ptr(k, c) for c in range(S)])
            chk(h, L.vg_fe_upload_frames(h.h, ptrs, W), "upload")
            slots[k] = int(L.vg_fe_frame_slot(h.h))
            chk(h, L.vg_fe_read_image_batch(h.h, S, ins[0 if k == 1 else 1], outs), "resident warm-up")
        assert slots[0] != slots[1]

    def step(n):
        if mode == "b":
            chk(h, L.vg_fe_select_frames(h.h, slots[1 if n % 2 == 0 else 0]), "select")
        chk(h, L.vg_fe_read_image_batch(h.h, S, ins[n % 2], outs), "vg_fe_read_image_batch")

    n, dt = timed(step, seconds)
    tracked = int(np.mean([outs[c].n1 for c in range(S)]))
    if mode == "a_reg":
        for b in scene.buf:
            L.vg_host_unregister(h.h, C.c_void_p(b.ctypes.data))
    h.close()
    return dict(steps=n, seconds=dt, frames_per_s=S * n / dt, ms_per_step=dt / n * 1e3, mean_tracked_last_step=tracked)


def leg_single(scene, seconds, threads=1):
    S = scene.S
    hs = [ba.Handle() for _ in range(S)]
    for h in hs:
        fe.FrontEnd(h, W, H, 1, NPTS)
    ins = scene.inputs()
    outs = [fe.FrameOut() for _ in range(S)]
    for c, h in enumerate(hs):
        f = frame_in(scene.img_ptr(0, c), np.zeros((0, 2), np.float32), True)
        chk(h, h.lib.vg_fe_read_image(h.h, C.byref(f), C.byref(outs[c])), "first frame")

    def some(n, cs):
        arr = ins[n % 2]
        for c in cs:
            h = hs[c]
            rc = h.lib.vg_fe_read_image(h.h, C.byref(arr[c]), C.byref(outs[c]))
            if rc:
                chk(h, rc, "vg_fe_read_image")

    if threads == 1:
        n, dt = timed(lambda k: some(k, range(S)), seconds)
    else:
        T = min(threads, S)
        parts = [range(t, S, T) for t in range(T)]
        for k in range(4):
            some(k, range(S))
        n_steps = [2]
        # (the number of steps is fixed per round so that the threads do the same work; rounds until the time is reached)
        n, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < seconds:
            ts = [threading.Thread(target=lambda p=p: [some(k, p) for k in range(n_steps[0])]) for p in parts]
            for t in ts:
                t.start()
            for t in ts:
                t.join()
            n += n_steps[0]
        dt = time.perf_counter() - t0
    for h in hs:
        h.close()
    return dict(steps=n, seconds=dt, frames_per_s=S * n / dt, ms_per_step=dt / n * 1e3, threads=threads)


def spread(vals):
    return dict(values=vals, median=float(np.median(vals)), min=float(min(vals)), max=float(max(vals)), spread=float(max(vals) - min(vals)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="1,16,64,256")
    ap.add_argument("--only", default=None)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--child", type=int, default=0)
    ap.add_argument("--threads", type=int, default=1)
    a = ap.parse_args()
    if a.child:                                        # one single-stream leg on the library chosen before anything was loaded
        print(json.dumps(leg_single(Scene(a.child), a.seconds, a.threads)))
        return
    res = dict(what=__doc__.split("\n\n")[0].replace("\n", " "), shape=dict(width=W, height=H, points=NPTS, equalize=1), sizes={})
    for S in [int(v) for v in a.sizes.split(",")]:
        scene = Scene(S)
        r = {}
        if a.only:
            r[a.only] = leg_batch(scene, a.seconds, a.only)
        else:
            assert a.parent_lib and os.path.exists(a.parent_lib), "--parent-lib: the library built from the parent commit"
            ra, rc = [], []
            for rep in range(3):
                ra.append(leg_batch(scene, a.seconds, "a"))
                rc.append(single_leg_in_child(S, a.seconds, a.parent_lib))
            r["a"] = spread([x["frames_per_s"] for x in ra]); r["a"]["ms_per_step"] = ra[1]["ms_per_step"]
            r["c"] = spread([x["frames_per_s"] for x in rc]); r["c"]["ms_per_step"] = rc[1]["ms_per_step"]
            r["a_reg"] = leg_batch(scene, a.seconds, "a_reg")
            r["b"] = leg_batch(scene, a.seconds, "b")
            r["c8"] = single_leg_in_child(S, a.seconds, a.parent_lib, threads=8)
            r["factor_a_over_c"] = r["a"]["median"] / r["c"]["median"]
            r["a_beats_c_by_more_than_the_spread"] = bool(r["a"]["min"] > r["c"]["max"])
            if S == 1:
                here, parent = [], []
                for rep in range(3):
                    here.append(single_leg_in_child(S, a.seconds, None)["ms_per_step"])
                    parent.append(single_leg_in_child(S, a.seconds, a.parent_lib)["ms_per_step"])
                r["single_call_ms_this_tree"] = spread(here)
                r["single_call_ms_parent"] = spread(parent)
        res["sizes"][str(S)] = r
        print("S", S, json.dumps(r), flush=True)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
