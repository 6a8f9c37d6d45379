"""MANUAL (not collected): a resident sequence with processIMU on the device (vg_ba_seq_step_imu_async) against what a caller has
without it, 256 windows of EuRoC shape (K = 11, about 150 landmarks), 20 IMU samples per frame.  Both variants are the C++ caller
(host/resident_estimator.cpp through `vins_replay seq`, VINS_REPLAY_TIMING=1): a host clock around processIMU of every estimator plus
solve() (step + state download, ends in a synchronise) per frame.

  a   default path: sample buffers and propagation of Ps / Rs / Vs on the host, ONE batched vg_imu_preintegrate for all windows (plus
      the merged intervals), vg_ba_seq_step_async, vg_ba_batch_download_state
  b   VINS_REPLAY_DEVICE_IMU=1: vg_ba_seq_step_imu_async plus the same download
  c   control: variant a with the parent commit's library (--parent-lib-dir: LD_LIBRARY_PATH of the child), to show what the
      rewritten imu_preint_kernel and the changed step did to the host-fed path
  the device time of ba_seq_imu_kernel and of ba_seq_merge_kernel from HIP events (VINS_REPLAY_KERNEL_TIMES=1), in runs of their own

One run of the tool = hand-over + `--warm` + `--frames` timed frames (the synthetic tracks thin out after that, so a steady state is
a chain of short runs); `--runs` runs per variant and repeat, variants alternating within a repeat.

    python tests/manual/gpu_seq_imu.py [--parent-lib-dir <dir with the parent commit's libvinsgpu.so>] [--out profiles/seq_imu.json]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402

graft.load_package()
import seq_model as M  # noqa: E402
from vins_mono_amd import synth  # noqa: E402


def spread(vals):
    return dict(values=[round(v, 4) for v in vals], median=float(np.median(vals)), min=float(min(vals)), max=float(max(vals)), spread=float(max(vals) - min(vals)))


def run_tool(exe, frames, env, warm):
    """ms per timed frame (processIMU of all estimators + solve()) of one run"""
    with tempfile.NamedTemporaryFile(suffix=".csv") as out:
        r = subprocess.run([exe, "seq", frames, out.name], capture_output=True, text=True, timeout=600, env=dict(os.environ, VINS_REPLAY_TIMING="1", **env))
    if r.returncode != 0:
        raise RuntimeError("vins_replay seq failed (%d):\n%s" % (r.returncode, r.stderr[-2000:]))
    rows = [l.split(",") for l in r.stderr.splitlines() if l.startswith("T,")]
    return [float(x[2]) + float(x[3]) for x in rows[warm:]], [float(x[2]) for x in rows[warm:]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=256)
    ap.add_argument("--kinds", type=int, default=16)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--min-parallax", type=float, default=0.25)
    ap.add_argument("--parent-lib-dir", default=None)
    ap.add_argument("--exe", default=os.path.join(ROOT, "vins-mono_amd", "lib", "vins_replay"), help="the replay tool (e.g. the emulated build, to try the script)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    K, W = 11, a.warm + a.frames
    exe = a.exe
    kinds = [M.FrameSource(synth.SyntheticSequence(900 + s, n_frames=K + W + 1, K=K + W + 1, L=150), noise_seed=900 + s) for s in range(a.kinds)]
    srcs = [kinds[w % a.kinds] for w in range(a.windows)]
    tmp = tempfile.mkdtemp()
    frames = os.path.join(tmp, "frames.bin")
    M.write_seq_file(frames, srcs, K, W, min_parallax=a.min_parallax)
    n_obs = float(np.mean([len(s.image(K - 1 + w)[0]) for s in kinds for w in range(W)]))
    S = kinds[0].seq.imu_per_frame
    res = dict(what=__doc__.split("\n\n")[0].replace("\n", " "), status="measured",
               shape=dict(windows=a.windows, K=K, landmarks=150, samples_per_frame=S, observations_per_frame_mean=n_obs, min_parallax=a.min_parallax,
                          timed_frames_per_run=a.frames, warm_frames_per_run=a.warm, runs=a.runs, repeats=a.repeats,
                          timed_steps_per_variant_and_repeat=a.frames * a.runs),
               upload_doubles_per_window_and_step=dict(a_host_fed=16 + 2 * 472 + 8 * n_obs, b_device_imu=7 * S + 8 * n_obs))
    variants = [("a_host_imu", {}), ("b_device_imu", {"VINS_REPLAY_DEVICE_IMU": "1"})]
    if a.parent_lib_dir:
        variants.append(("c_host_imu_parent_library", {"LD_LIBRARY_PATH": os.path.abspath(a.parent_lib_dir) + os.pathsep + os.environ.get("LD_LIBRARY_PATH", "")}))
    ms = {name: [] for name, _ in variants}
    imu = {name: [] for name, _ in variants}
    for rep in range(a.repeats):
        for name, env in variants:
            tot, host = [], []
            for _ in range(a.runs):
                t, hi = run_tool(exe, frames, env, a.warm)
                tot += t; host += hi
            ms[name].append(float(np.mean(tot)))
            imu[name].append(float(np.mean(host)))
            print(rep, name, "ms per frame", ms[name][-1], "of which processIMU on the host", imu[name][-1], flush=True)
    for name, _ in variants:
        res[name] = dict(ms_per_frame=spread(ms[name]), host_processIMU_ms_per_frame=spread(imu[name]))
    worst = max(res["a_host_imu"]["ms_per_frame"]["spread"], res["b_device_imu"]["ms_per_frame"]["spread"])
    res["b_minus_a_ms"] = res["b_device_imu"]["ms_per_frame"]["median"] - res["a_host_imu"]["ms_per_frame"]["median"]
    res["b_faster_than_a_beyond_the_spreads"] = bool(-res["b_minus_a_ms"] > worst)
    # ---- device time of the two new kernels (all windows of the batch), from HIP events, in runs of their own
    ik, mk = [], []
    for rep in range(a.repeats):
        with tempfile.NamedTemporaryFile(suffix=".csv") as out:
            r = subprocess.run([exe, "seq", frames, out.name], capture_output=True, text=True, timeout=600,
                               env=dict(os.environ, VINS_REPLAY_DEVICE_IMU="1", VINS_REPLAY_KERNEL_TIMES="1"))
        if r.returncode != 0:
            raise RuntimeError("vins_replay seq failed (%d):\n%s" % (r.returncode, r.stderr[-2000:]))
        rows = [l.split(",") for l in r.stderr.splitlines() if l.startswith("K,")][a.warm:]
        ik.append(float(np.mean([float(x[2]) for x in rows])))
        mk.append(float(np.mean([float(x[3]) for x in rows])))
    res["device_ms_per_frame_from_hip_events"] = dict(ba_seq_imu_kernel=spread(ik), ba_seq_merge_kernel=spread(mk), frames_per_repeat=a.frames)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
