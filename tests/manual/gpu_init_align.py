"""MANUAL (MI355X): what vg_init_align costs.  256 windows of F = 11 frames with 20 IMU samples per interval (1 % pose noise), three
repeats after one warm-up: wall time of the C call, and beside it in the same run the two vg_imu_preintegrate calls over the same
rows that a caller needs anyway (integration with the first biases, re-propagation with the solved ones): the difference is what the
alignment adds.  Device time per kernel comes from a second run of this script under `rocprofv3 --kernel-trace --stats` (--profile);
VGPRs / scratch / LDS of the kernels as the compiler reports them for the code object.

usage: python tests/manual/gpu_init_align.py [--out profiles/init_align.json] [--profile]"""
import argparse
import ctypes as C
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
N_WIN, F, SPI, REPEATS = 256, 11, 20, 3
KERNELS = ("init_align_kernel", "init_align_bias_kernel", "imu_preint_kernel")


def run():
    import numpy as np
    import __graft_entry__ as g
    g.load_package()
    from vins_mono_amd import ba
    import init_align_ref as A
    wins = [A.scene(5000 + i, F, SPI, noise=0.01, key='all') for i in range(N_WIN)]
    h = ba.Handle()
    ins, outs, keep = h.init_align_pack(wins)
    ivs = [iv for w in wins for iv in w['intervals']]
    first_bias = [(w['ba0'], w['bg0']) for w in wins for _ in w['intervals']]
    times = dict(init_align_ms=[], imu_preintegrate_twice_ms=[])
    for rep in range(REPEATS + 1):
        t0 = time.perf_counter()
        rc = h.lib.vg_init_align(h.h, N_WIN, ins, outs)
        t1 = time.perf_counter()
        assert rc == 0, h.lib.vg_last_error(h.h)
        if rep:
            times['init_align_ms'].append((t1 - t0) * 1e3)
    res = h.init_align(wins)
    second_bias = [(np.zeros(3), r['bg']) for r, w in zip(res, wins) for _ in w['intervals']]
    # the same packing outside the timed region: time the two C calls only
    n = len(ivs)
    off = np.zeros(n + 1, np.int32)
    rows, first = [], np.zeros((n, 6))
    for k, iv in enumerate(ivs):
        first[k, :3], first[k, 3:] = iv[0][1], iv[0][2]
        rows += [[dt, *a, *gy] for dt, a, gy in iv[1:]]
        off[k + 1] = len(rows)
    smp = np.ascontiguousarray(rows, np.float64)
    nz = np.ascontiguousarray(wins[0]['noise'], np.float64)
    b1 = np.ascontiguousarray([np.concatenate(b) for b in first_bias])
    b2 = np.ascontiguousarray([np.concatenate(b) for b in second_bias])
    out = (ba.ImuPreint * n)()
    for rep in range(REPEATS + 1):
        t0 = time.perf_counter()
        for b in (b1, b2):
            rc = h.lib.vg_imu_preintegrate(h.h, n, ba._ip(off), ba._dp(smp), ba._dp(first), ba._dp(b), ba._dp(nz), out)
            assert rc == 0
        t1 = time.perf_counter()
        if rep:
            times['imu_preintegrate_twice_ms'].append((t1 - t0) * 1e3)
    statuses = [r['status'] for r in res]
    h.close()
    return dict(windows=N_WIN, frames=F, samples_per_interval=SPI, repeats=REPEATS, wall=times,
                statuses={str(s): statuses.count(s) for s in sorted(set(statuses))})


def kernel_notes():
    """VGPRs, SGPRs, scratch and static LDS of the kernels as the compiler reports them for the code object (the library's flags;
    -Rpass-analysis=kernel-resource-usage prints what goes into the kernel descriptors)"""
    src = os.path.join(ROOT, "vins-mono_amd", "csrc", "imu_preint.hip")
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only",
                            "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(d, "dev.o")], capture_output=True, text=True)
    if r.returncode != 0:
        return {"error": r.stderr[-500:]}
    out, cur = {}, None
    keys = {"VGPRs": "vgprs", "TotalSGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane", "LDS Size [bytes/block]": "static_lds_bytes",
            "Occupancy [waves/SIMD]": "occupancy_waves_per_simd"}
    for ln in r.stderr.splitlines():
        m = re.search(r"remark:\s+(Function Name|[A-Za-z][^:]*):\s+(\S+)", ln)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = m.group(2) if m.group(2) in KERNELS else None
            if cur:
                out[cur] = {}
        elif cur and m.group(1) in keys:
            out[cur][keys[m.group(1)]] = int(m.group(2))
    return out


def lds_bytes(frames):
    """the launch's dynamic LDS per frame count, from the carve's own checker (tests/init_align_carve_check.cpp)"""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "carve")
        subprocess.run(["g++", "-std=c++17", os.path.join(ROOT, "tests", "init_align_carve_check.cpp"), "-o", exe], check=True)
        lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
    table = {int(ln.split()[1]): int(ln.split()[-1]) for ln in lines}
    return {f"F={f}": table[f] for f in frames}


def profile():
    """device time per kernel: this script once more under rocprofv3 --kernel-trace --stats (a run of its own)"""
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "align", "--", sys.executable, os.path.abspath(__file__), "--child"],
                           capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            return {"error": r.stderr[-500:]}
        rows = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            import csv
            for row in csv.DictReader(open(path)):
                if row.get("Name") in KERNELS:
                    rows[row["Name"]] = dict(calls=int(row["Calls"]), total_us=float(row["TotalDurationNs"]) / 1e3, average_us=float(row["AverageNs"]) / 1e3,
                                             min_us=float(row["MinNs"]) / 1e3, max_us=float(row["MaxNs"]) / 1e3)
        return rows or {"error": "no kernel_stats.csv rows for the kernels"}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "init_align.json"))
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        run()
        sys.exit(0)
    doc = dict(what=__doc__.split("\n\n")[0], **run())
    doc["kernels"] = kernel_notes()
    doc["dynamic_lds_bytes"] = lds_bytes((11, 32))
    if a.profile:
        doc["device_time"] = profile()
        doc["device_time_note"] = "per launch, all launches of the profiled run (5 vg_init_align calls with two launches of imu_preint_kernel each, 8 vg_imu_preintegrate calls)"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc, indent=1))
