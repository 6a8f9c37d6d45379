"""MANUAL (not collected): what the keyframe message and the point clouds cost a resident sequence, 256 windows of EuRoC shape (K = 11,
about 150 tracks per window) in resident IMU mode (vg_ba_seq_step_imu_async), driven through the Python binding with every frame and
every output struct built beforehand.  One timed step = the step call + vg_ba_batch_download_state (which ends in a synchronise of the
solve) + whatever the variant adds, host clock.

  a   the plain step: this tree's library, and the parent commit's (--parent-lib, a child process of this script per repeat, alternating
      with this tree's) -- the claim is "unchanged"
  b   the step + vg_ba_seq_outputs_async + one vg_ba_seq_get_outputs per window (all six arrays asked for)
  k   vg_ba_seq_outputs_async alone between the handle's timer events (vg_timer_start / vg_timer_stop): ba_seq_publish_kernel AND its one
      download; the binding has no event pair around the kernel alone
  c   what a caller had: the step + vg_ba_seq_get_tracks and vg_ba_seq_export for each of the windows (library calls only: the caller's
      own selection and transform are not counted)

The synthetic tracks thin out after a dozen frames, so a repeat is a chain of short runs (begin, --warm, --frames timed steps).
Bars: a lies inside the parent's repeat spread; b is faster than c by more than the larger of their two spreads.

    python tests/manual/gpu_seq_outputs.py [--parent-lib <the parent commit's libvinsgpu.so>] [--out profiles/seq_outputs.json]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gpu_seq_relo as G  # noqa: E402  (the packed chain of short runs, the spread record)

K = G.K
MP = 256


class Getter:
    """pre-built arguments of the per-window calls"""

    def __init__(self, ba, n):
        self.n = n
        self.f3, self.nm, self.uv, self.pc, self.mg = (np.zeros((MP, c), np.float32) for c in (3, 2, 2, 3, 3))
        self.id = np.zeros(MP, np.int32)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        self.o = ba.SeqOutputs() if hasattr(ba, "SeqOutputs") else None
        if self.o is not None:
            self.o.struct_size = C.sizeof(ba.SeqOutputs)
            self.o.kf_point_3d, self.o.kf_norm, self.o.kf_uv, self.o.cloud_xyz, self.o.margin_xyz = fp(self.f3), fp(self.nm), fp(self.uv), fp(self.pc), fp(self.mg)
            self.o.kf_id = self.id.ctypes.data_as(C.POINTER(C.c_int))
        cap = 512
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        self.t = [np.zeros(cap, np.int32) for _ in range(4)]
        self.dep, self.obs = np.zeros(cap), np.zeros((cap, K, 8))
        self.pose, self.sb, self.ex, self.td = np.zeros((K, 7)), np.zeros((K, 9)), np.zeros(7), np.zeros(1)
        self.nf = C.c_int()
        self.track_args = (cap, C.byref(self.nf), ip(self.t[0]), ip(self.t[1]), ip(self.t[2]), ip(self.t[3]), dp(self.dep), dp(self.obs))
        self.export_args = (dp(self.pose), dp(self.sb), dp(self.ex), dp(self.td), None, None)


def run_variant(h, chain, g, variant, warm, runs):
    """mean ms per timed step over `runs` short runs, and (variant k) the mean ms between the timer events"""
    lib, hh = h.lib, h.h
    step_ms, ev_ms, sizes = [], [], None

    def chk(rc, what):
        if rc:
            raise RuntimeError("%s: %d %s" % (what, rc, lib.vg_last_error(hh).decode()))
    for _ in range(runs):
        chain.begin(h, 0)
        try:
            if variant in ("b", "k"):
                h.seq_outputs_reserve(MP)
            for t in range(chain.steps):
                n, fp = chain.frames[t][0], chain.frames[t][1]
                t0 = time.perf_counter()
                chk(lib.vg_ba_seq_step_imu_async(hh, n, fp), "vg_ba_seq_step_imu_async")
                if variant == "b":
                    chk(lib.vg_ba_seq_outputs_async(hh), "vg_ba_seq_outputs_async")
                rc = h.ba_download_state_raw()
                if rc not in (0, -4):
                    raise RuntimeError("vg_ba_batch_download_state: %d" % rc)
                if variant == "b":
                    for w in range(n):
                        chk(lib.vg_ba_seq_get_outputs(hh, w, C.byref(g.o)), "vg_ba_seq_get_outputs")
                elif variant == "c":
                    for w in range(n):
                        chk(lib.vg_ba_seq_get_tracks(hh, w, *g.track_args), "vg_ba_seq_get_tracks")
                        chk(lib.vg_ba_seq_export(hh, w, *g.export_args), "vg_ba_seq_export")
                t1 = time.perf_counter()
                if variant == "k":
                    h.sync()
                    h.timer_start()
                    chk(lib.vg_ba_seq_outputs_async(hh), "vg_ba_seq_outputs_async")
                    ms = h.timer_stop()
                    if t >= warm:
                        ev_ms.append(ms)
                if t >= warm:
                    step_ms.append((t1 - t0) * 1e3)
            bad = [i['status'] for i in h.seq_info() if i['status'] != 0]
            if bad:
                raise RuntimeError("a window reported status %r" % bad[:4])
            if variant in ("b", "k"):
                o = h.seq_outputs(0)
                sizes = dict(status=o['status'], n_keyframe=o['n_keyframe'], n_cloud=o['n_cloud'], n_margin=o['n_margin'], tracks=len(h.seq_tracks(0, K)['id']))
        finally:
            h.seq_end()
    return float(np.mean(step_ms)), (float(np.mean(ev_ms)) if ev_ms else None), sizes, len(step_ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=256)
    ap.add_argument("--kinds", type=int, default=16)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--lib", default=None, help="(child mode) the library to load")
    ap.add_argument("--only-plain", action="store_true", help="(child mode) print the plain variant's ms per step and leave")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.lib:
        G.pkg.LIB_PATH = os.path.abspath(a.lib)
    from vins_mono_amd import ba
    chain = G.Chain(ba, a.windows, a.kinds, a.warm + a.frames, 1)
    h = ba.Handle()
    g = Getter(ba, a.windows)
    if a.only_plain:
        print("PLAIN", run_variant(h, chain, g, "a", a.warm, a.runs)[0])
        return
    names = dict(a="a_plain", b="b_step_and_outputs", k="k_outputs_async_between_events", c="c_step_and_get_tracks_export")
    ms = {v: [] for v in names}
    ev, parent, extra = [], [], {}
    run_variant(h, chain, g, "b", a.warm, 1)                      # (clocks, allocations)
    for rep in range(a.repeats):
        for v in ("a", "b", "k", "c"):
            m, e, sizes, nsteps = run_variant(h, chain, g, v, a.warm, a.runs)
            ms[v].append(m)
            if e is not None:
                ev.append(e)
            if sizes:
                extra[v] = sizes
            print(rep, names[v], "ms per step", round(m, 4), "" if e is None else "events %.4f ms" % e, flush=True)
            if v == "a" and a.parent_lib:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--lib", a.parent_lib, "--only-plain", "--windows", str(a.windows), "--kinds", str(a.kinds),
                                    "--frames", str(a.frames), "--warm", str(a.warm), "--runs", str(a.runs)], capture_output=True, text=True, timeout=900)
                if r.returncode != 0 or "PLAIN" not in r.stdout:
                    raise RuntimeError("the parent library's run failed:\n" + r.stdout[-1000:] + r.stderr[-2000:])
                parent.append(float(r.stdout.split("PLAIN")[1].split()[0]))
                print(rep, "a_plain_parent_library ms per step", round(parent[-1], 4), flush=True)
    res = dict(what=__doc__.split("\n\n")[0].replace("\n", " "), status="measured",
               shape=dict(windows=a.windows, K=K, landmarks=150, max_points=MP, timed_steps_per_run=a.frames, warm_steps_per_run=a.warm, runs=a.runs, repeats=a.repeats,
                          timed_steps_per_variant_and_repeat=a.frames * a.runs, mode="resident IMU (vg_ba_seq_step_imu_async)", window0_after_the_last_step=extra.get("b")))
    for v in ("a", "b", "c"):
        res[names[v]] = dict(ms_per_step=G.spread(ms[v]))
    res[names["k"]] = dict(ms_kernel_and_download=G.spread(ev))
    if parent:
        res["a_plain_parent_library"] = dict(ms_per_step=G.spread(parent))
        lo, hi = res["a_plain_parent_library"]["ms_per_step"]["min"], res["a_plain_parent_library"]["ms_per_step"]["max"]
        res["a_minus_parent_ms"] = res["a_plain"]["ms_per_step"]["median"] - res["a_plain_parent_library"]["ms_per_step"]["median"]
        res["bar_a_inside_the_parents_repeat_spread"] = bool(lo <= res["a_plain"]["ms_per_step"]["median"] <= hi)
    b, c = res[names["b"]]["ms_per_step"], res[names["c"]]["ms_per_step"]
    res["c_minus_b_ms"] = c["median"] - b["median"]
    res["bar_b_faster_than_c_by_more_than_the_larger_spread"] = bool(c["median"] - b["median"] > max(b["spread"], c["spread"]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
