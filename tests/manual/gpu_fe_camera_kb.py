"""MANUAL (not collected): what the camera models cost the batched front end where the lift weighs most: leg b of
tests/manual/gpu_fe_batch_frames.py (vg_fe_read_image_batch over 256 streams x 150 points at 752x480, CLAHE on, frames resident on the
device, published and unpublished steps alternating), run

  a  parent_pinhole   with the library built from the parent commit (--parent-lib), every stream the pinhole of intr
     pinhole          with this tree's library, the same
  b  mei              this tree, the MEI camera A (xi 0.9, the same eight numbers) on every stream
  c  kb               this tree, the Kannala-Brandt camera of config/cla (752x480) on every stream

three repeats each.  Every repeat is a child process of its own (the package loads its library with RTLD_GLOBAL: two builds of it in one
process would bind each other's symbols; the library is chosen as tests/manual/bench_with_lib.py chooses it, by LIB_PATH before the first
handle); the parent's and this tree's children alternate, and a child of this tree runs pinhole, mei and kb one after the other.  Host
clock around calls that end in a synchronise; every leg is warmed up and runs for at least --seconds.  Each leg also reports a CRC of
the last step's lifted points: the pinhole legs of the two libraries must agree.

    python tests/manual/gpu_fe_camera_kb.py --parent-lib <libvinsgpu.so of the parent commit> [--commit <this tree's>] [--out profiles/fe_camera_models.json]

--out: the record goes under the key "resident_256x150" of that JSON file (the file's other keys stay)."""
import argparse
import json
import os
import subprocess
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gpu_fe_batch_frames as B  # noqa: E402  (with --child and --parent-lib on the command line it selects the parent's library before anything loads)

from vins_mono_amd import ba, fe  # noqa: E402

MEI_A = (0.9,) + B.INTR                                # xi, then gamma1 gamma2 u0 v0 k1 k2 p1 p2
KB_CLA = (472.2863830700696, 470.83759684346785, 368.8316828103749, 232.23688706965652,            # mu mv u0 v0
          -0.005740195474458931, 0.02878252863739417, -0.04010621197185408, 0.02008469575876223)   # k2 k3 k4 k5


def leg(scene, seconds, model):
    """leg b of gpu_fe_batch_frames.py with `model` ("pinhole": no camera set, "mei", "kb") on every stream"""
    S = scene.S
    h = ba.Handle()
    tr = fe.FrontEnd(h, B.W, B.H, S, B.NPTS)
    if model != "pinhole":
        cam = fe.Camera.mei(*MEI_A) if model == "mei" else fe.Camera.kannala_brandt(*KB_CLA)
        for c in range(S):
            tr.set_camera(c, cam)
    L = h.lib
    ins = scene.inputs(resident=True)
    outs = (fe.FrameOut * S)()
    first = (fe.FrameIn * S)()
    for c in range(S):
        first[c] = B.frame_in(scene.img_ptr(0, c), np.zeros((0, 2), np.float32), True)
    B.chk(h, L.vg_fe_read_image_batch(h.h, S, first, outs), "first frame")
    slots = {}
    for k in (1, 0):
        ptrs = (B._u8 * S)(*[scene.img_ptr(k, c) for c in range(S)])
        B.chk(h, L.vg_fe_upload_frames(h.h, ptrs, B.W), "upload")
        slots[k] = int(L.vg_fe_frame_slot(h.h))
        B.chk(h, L.vg_fe_read_image_batch(h.h, S, ins[0 if k == 1 else 1], outs), "resident warm-up")
    assert slots[0] != slots[1]

    def step(n):
        B.chk(h, L.vg_fe_select_frames(h.h, slots[1 if n % 2 == 0 else 0]), "select")
        B.chk(h, L.vg_fe_read_image_batch(h.h, S, ins[n % 2], outs), "vg_fe_read_image_batch")

    n, dt = B.timed(step, seconds)
    step(0)                                              # a published step: its lifted lists are what the CRC is taken of
    crc, lifted = 0, 0
    for c in range(S):
        un = np.ctypeslib.as_array(outs[c].un_xy, shape=(outs[c].n_final, 2)) if outs[c].n_final else np.zeros((0, 2), np.float32)
        crc = zlib.crc32(np.ascontiguousarray(un, np.float32).tobytes(), crc)
        lifted += int(outs[c].n_final)
    tracked = int(np.mean([outs[c].n1 for c in range(S)]))
    h.close()
    return dict(steps=n, seconds=dt, ms_per_step=dt / n * 1e3, mean_tracked_last_step=tracked, lifted_last_step=lifted, un_xy_crc32=crc)


def in_child(S, seconds, models, lib_path):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", ",".join(models), "--streams", str(S), "--seconds", str(seconds)]
    if lib_path:
        cmd += ["--parent-lib", os.path.abspath(lib_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("child failed (%d):\n%s" % (r.returncode, r.stderr[-2000:]))
    return json.loads([line for line in r.stdout.splitlines() if line.startswith("{")][-1])


def spread(vals):
    return dict(values=vals, median=float(np.median(vals)), min=float(min(vals)), max=float(max(vals)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--parent-commit", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--child", default=None)                      # the models of one child, comma-separated
    a = ap.parse_args()
    if a.child:
        scene = B.Scene(a.streams)
        print(json.dumps({m: leg(scene, a.seconds, m) for m in a.child.split(",")}))
        return
    assert a.parent_lib and os.path.exists(a.parent_lib), "--parent-lib: the library built from the parent commit"
    import torch
    runs = dict(parent_pinhole=[], pinhole=[], mei=[], kb=[])
    for rep in range(a.repeats):
        runs["parent_pinhole"].append(in_child(a.streams, a.seconds, ["pinhole"], a.parent_lib)["pinhole"])
        here = in_child(a.streams, a.seconds, ["pinhole", "mei", "kb"], None)
        for m in ("pinhole", "mei", "kb"):
            runs[m].append(here[m])
        print("repeat", rep, {k: round(v[-1]["ms_per_step"], 4) for k, v in runs.items()}, flush=True)
    rec = dict(what="vg_fe_read_image_batch, %d streams x %d points at %dx%d, frames resident, ms per step (host clock around synchronised calls)"
                    % (a.streams, B.NPTS, B.W, B.H),
               commits=dict(parent=a.parent_commit, this_tree=a.commit), box=dict(hostname=os.uname().nodename, device=torch.cuda.get_device_name(0)),
               seconds_per_leg=a.seconds, cameras=dict(mei=dict(xi=MEI_A[0], p=MEI_A[1:]), kb=dict(p=KB_CLA)))
    for k, v in runs.items():
        rec[k] = dict(ms_per_step=spread([x["ms_per_step"] for x in v]), mean_tracked_last_step=v[0]["mean_tracked_last_step"],
                      lifted_last_step=v[0]["lifted_last_step"], un_xy_crc32=sorted(set(x["un_xy_crc32"] for x in v)))
    p, t = rec["parent_pinhole"]["ms_per_step"], rec["pinhole"]["ms_per_step"]
    rec["pinhole_difference_ms"] = t["median"] - p["median"]
    rec["pinhole_difference_inside_the_repeat_spread"] = bool(abs(t["median"] - p["median"]) <= max(p["max"] - p["min"], t["max"] - t["min"]))
    rec["pinhole_same_lifted_points_as_parent"] = rec["parent_pinhole"]["un_xy_crc32"] == rec["pinhole"]["un_xy_crc32"]
    rec["kb_over_mei"] = rec["kb"]["ms_per_step"]["median"] / rec["mei"]["ms_per_step"]["median"]
    print(json.dumps(rec), flush=True)
    if a.out:
        doc = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                doc = json.load(f)
        doc["resident_256x150"] = rec
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
