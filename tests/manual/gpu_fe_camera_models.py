"""MANUAL (not collected): what the camera models cost the front end.  The legs of tests/manual/gpu_fe_batch_frames.py (leg a:
vg_fe_read_image_batch over S streams, frames from pageable host memory; S = 1: vg_fe_read_image) and the step-by-step calls of
tests/manual/gpu_readimage_breakdown.py, each run

  parent              with the library built from the parent commit (--parent-lib), pinhole from intr
  this_tree_pinhole   with this tree's library, pinhole from intr
  this_tree_mei       with this tree's library and the MEI camera A (xi 0.9, the same eight numbers) set on every stream

three repeats each; parent and this_tree_pinhole alternate.  Every leg runs in a child process of its own (the package loads its library
with RTLD_GLOBAL: two builds of it in one process would bind each other's symbols).  Host clock around calls that end in a synchronise.

    python tests/manual/gpu_fe_camera_models.py --parent-lib <libvinsgpu.so of the parent commit> [--sizes 1,256] [--out profiles/fe_camera_models.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gpu_fe_batch_frames as B  # noqa: E402  (with --child and --parent-lib on the command line it selects the parent's library before anything loads)

from vins_mono_amd import ba, fe  # noqa: E402

MEI_A = (0.9,) + B.INTR                                # xi, then gamma1 gamma2 u0 v0 k1 k2 p1 p2


def leg_frames(S, seconds, mei):
    """leg a of gpu_fe_batch_frames.py (S > 1) or its single call (S = 1), with the camera set when `mei`"""
    scene = B.Scene(S)
    h = ba.Handle()
    tr = fe.FrontEnd(h, B.W, B.H, S, B.NPTS)
    if mei:
        for c in range(S):
            tr.set_camera(c, fe.Camera.mei(*MEI_A))
    L = h.lib
    ins = scene.inputs()
    outs = (fe.FrameOut * S)()
    first = (fe.FrameIn * S)()
    for c in range(S):
        first[c] = B.frame_in(scene.img_ptr(0, c), np.zeros((0, 2), np.float32), True)
    if S == 1:
        call = lambda arr: L.vg_fe_read_image(h.h, arr, outs)
    else:
        call = lambda arr: L.vg_fe_read_image_batch(h.h, S, arr, outs)
    B.chk(h, call(first), "first frame")
    n, dt = B.timed(lambda k: B.chk(h, call(ins[k % 2]), "frame"), seconds)
    tracked = int(np.mean([outs[c].n1 for c in range(S)]))
    h.close()
    return dict(steps=n, seconds=dt, frames_per_s=S * n / dt, ms_per_step=dt / n * 1e3, mean_tracked_last_step=tracked)


def leg_breakdown(mei):
    """the loop of gpu_readimage_breakdown.py: median wall time in ms of each step-by-step call of a published frame, one stream"""
    sys.path.insert(0, os.path.dirname(HERE))
    import fe_scene
    h = ba.Handle()
    tr = fe.FrontEnd(h, 752, 480, 1, 600)
    frames = fe_scene.moving_scene(30, seed=3)
    intr = np.array(B.INTR)
    lift = (lambda p: tr.lift(p, fe.Camera.mei(*MEI_A))) if mei else (lambda p: tr.undistort(p, intr))
    T = {}

    def tm(name, f):
        t0 = time.perf_counter(); r = f(); T.setdefault(name, []).append((time.perf_counter() - t0) * 1e3); return r

    tr.push_frames([frames[0]], equalize=True)
    pts = tr.detect(0, 150)
    cnt = np.ones(len(pts), np.int32)
    for k in range(1, 30):
        tm("push_frames", lambda: tr.push_frames([frames[k]], equalize=True))
        nxt, st, err = tm("track", lambda: tr.track(0, pts))
        keep = st.astype(bool)
        cur, nxt = pts[keep], nxt[keep]; cnt = cnt[keep] + 1
        un1 = (tm("lift_cur", lambda: lift(cur)).astype(np.float64) * 460 + [376, 240]).astype(np.float32)
        un2 = (tm("lift_forw", lambda: lift(nxt)).astype(np.float64) * 460 + [376, 240]).astype(np.float32)
        stf = tm("reject_with_f", lambda: tr.reject_with_f(un1, un2, 1.0))[0].astype(bool)
        nxt, cnt = nxt[stf], cnt[stf]
        kept = tm("set_mask", lambda: tr.set_mask([nxt], [cnt], 30))[0]
        nxt, cnt = nxt[kept], cnt[kept]
        new = tm("detect_masked", lambda: tr.detect_masked(0, 150 - len(nxt)))
        pts = np.concatenate([nxt, new]).astype(np.float32); cnt = np.concatenate([cnt, np.ones(len(new), np.int32)])
        tm("lift_final", lambda: lift(pts))
    h.close()
    return {k: float(np.median(v[3:])) for k, v in T.items()}


def in_child(args, lib_path):
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [str(v) for v in args]
    if lib_path:
        cmd += ["--parent-lib", os.path.abspath(lib_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("child leg failed (%d):\n%s" % (r.returncode, r.stderr[-2000:]))
    return json.loads([line for line in r.stdout.splitlines() if line.startswith("{")][-1])


def spread(vals):
    return dict(values=vals, median=float(np.median(vals)), min=float(min(vals)), max=float(max(vals)))


def three_ways(run):
    """run(lib_is_parent, mei) -> result; the three runs of the module's text, three repeats each"""
    runs = dict(parent=[], this_tree_pinhole=[], this_tree_mei=[])
    for rep in range(3):
        runs["parent"].append(run(True, False))
        runs["this_tree_pinhole"].append(run(False, False))
    for rep in range(3):
        runs["this_tree_mei"].append(run(False, True))
    return runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="1,256")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--child", nargs="+", default=None)          # frames S mei | breakdown mei
    a = ap.parse_args()
    if a.child:
        if a.child[0] == "frames":
            print(json.dumps(leg_frames(int(a.child[1]), a.seconds, a.child[2] == "1")))
        else:
            print(json.dumps(leg_breakdown(a.child[1] == "1")))
        return
    assert a.parent_lib and os.path.exists(a.parent_lib), "--parent-lib: the library built from the parent commit"
    import torch
    res = dict(what=__doc__.split("\n\n")[0].replace("\n", " "), box=dict(hostname=os.uname().nodename, device=torch.cuda.get_device_name(0)),
               shape=dict(width=B.W, height=B.H, points=B.NPTS, equalize=1), frames={}, breakdown={})
    for S in [int(v) for v in a.sizes.split(",")]:
        runs = three_ways(lambda parent, mei: in_child(["frames", S, int(mei), "--seconds", a.seconds], a.parent_lib if parent else None))
        r = dict(leg="vg_fe_read_image" if S == 1 else "vg_fe_read_image_batch, frames from pageable host memory")
        for k, v in runs.items():
            r[k] = dict(ms_per_step=spread([x["ms_per_step"] for x in v]), frames_per_s=spread([x["frames_per_s"] for x in v]))
        p, t = r["parent"]["ms_per_step"], r["this_tree_pinhole"]["ms_per_step"]
        r["pinhole_median_within_parent_spread"] = bool(p["min"] <= t["median"] <= p["max"])
        res["frames"][str(S)] = r
        print("S", S, json.dumps(r), flush=True)
    runs = three_ways(lambda parent, mei: in_child(["breakdown", int(mei)], a.parent_lib if parent else None))
    for k, v in runs.items():
        res["breakdown"][k] = {call: spread([x[call] for x in v]) for call in v[0]}
    print("breakdown", json.dumps(res["breakdown"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
