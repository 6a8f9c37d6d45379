"""MANUAL (MI355X): what vg_init_exrot costs.  256 windows of 10 steps, 150 correspondences per step, (a) in ONE call and (b) fed one
step per call, 10 calls that carry records / ric, which is the per-frame use and is latency-bound.  One allocating call, reported on its
own, then three repeats: wall time of the C call (packing outside the timed region) and the device time of its nine launches from
events (vg_exrot_out::device_ms).  (c) 256 steps of 12 correspondences in one call: the LMedS range, where every step is a synchronous estimate of
its own before the upload.  In the same run vg_init_relpose in the shape of profiles/init_relpose.json with its recorded figure
beside it: the two calls share scratch and tables.  The project has no host InitialEXRotation to compare with: no speed-up is claimed.

usage: python tests/manual/gpu_init_exrot.py [--out profiles/init_exrot_measured.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
N_WIN, STEPS, N_CORR, REPEATS = 256, 10, 150, 3
LAUNCHES = ("gather", "samples_1", "counts_1", "bookkeeping_1", "samples_2", "counts_2", "bookkeeping_2", "rotation", "calibration")


def run():
    import __graft_entry__ as g
    g.load_package()
    from vins_mono_amd import ba
    import init_exrot_ref as X
    import init_relpose_ref as R
    wins = [X.scene(9000 + i, [N_CORR] * STEPS, rot_deg=25.0) for i in range(N_WIN)]
    res = dict(what=f"vg_init_exrot, {N_WIN} windows x {STEPS} steps x {N_CORR} correspondences; one allocating call, then {REPEATS} repeats", launches=LAUNCHES)
    h = ba.Handle()
    ins, outs, keep = h.init_exrot_pack(wins, timed=True)
    wall, dev = [], []
    for rep in range(REPEATS + 1):
        t0 = time.perf_counter()
        rc = h.lib.vg_init_exrot(h.h, N_WIN, ins, outs)
        wall.append((time.perf_counter() - t0) * 1e3)
        assert rc == 0, h.lib.vg_last_error(h.h)
        dev.append([float(x) for x in keep[0]['device_ms']])
    first_ok = [int(o.first_ok) for o in outs]
    res['one_call'] = dict(allocating_call_wall_ms=wall[0], call_wall_ms=wall[1:], device_ms_per_launch=dev[1:], device_ms_total=[sum(d) for d in dev[1:]],
                           first_ok={str(v): first_ok.count(v) for v in sorted(set(first_ok))}, status_ok=int(sum(int(o.status) == 0 for o in outs)),
                           fallback_steps=int(sum(int(b['used_fallback'].sum()) for b in keep)))
    whole = [b['ric'].copy() for b in keep]
    # (b) one step per call: the packing of a step needs the records of the step before, so it is inside the loop but outside the timer
    per_frame = []
    for rep in range(REPEATS + 1):
        state, t_calls = [dict(prev=np.zeros((0, 27)), ric_prev=np.eye(3)) for _ in wins], []
        for k in range(STEPS):
            step = [dict(corr=w['corr'][k:k + 1], delta_q=w['delta_q'][k:k + 1], **s) for w, s in zip(wins, state)]
            i2, o2, k2 = h.init_exrot_pack(step)
            t0 = time.perf_counter()
            rc = h.lib.vg_init_exrot(h.h, N_WIN, i2, o2)
            t_calls.append((time.perf_counter() - t0) * 1e3)
            assert rc == 0, h.lib.vg_last_error(h.h)
            state = [dict(prev=np.concatenate([s['prev'], b['records'][:1]]), ric_prev=b['ric'][0].copy()) for s, b in zip(state, k2)]
        assert all(np.array_equal(s['ric_prev'], w[-1]) for s, w in zip(state, whole)), "the per-frame run equals the one call"
        per_frame.append(t_calls)
    res['one_step_per_call'] = dict(first_run_call_wall_ms=per_frame[0], call_wall_ms=per_frame[1:], sum_of_10_calls_ms=[sum(t) for t in per_frame[1:]])
    h.close()
    # (c) the LMedS range: every step of 9 .. 14 correspondences is one synchronous estimate of its own (vg_fe_reject_with_f) before the upload
    h = ba.Handle()
    lwins = [X.scene(9800 + i, [12]) for i in range(N_WIN)]
    ins, outs, keep = h.init_exrot_pack(lwins)
    wall = []
    for rep in range(REPEATS + 1):
        t0 = time.perf_counter()
        rc = h.lib.vg_init_exrot(h.h, N_WIN, ins, outs)
        wall.append((time.perf_counter() - t0) * 1e3)
        assert rc == 0, h.lib.vg_last_error(h.h)
    assert all(int(b['branch'][0]) == 1 for b in keep)
    res['lmeds_256_steps_of_12_points'] = dict(allocating_call_wall_ms=wall[0], call_wall_ms=wall[1:], ms_per_lmeds_step=[w / N_WIN for w in wall[1:]])
    h.close()
    # vg_init_relpose, the first variant of tests/manual/gpu_init_relpose.py, on a handle that has served vg_init_exrot first
    h = ba.Handle()
    h.init_exrot(wins[:4])
    rwins = [R.scene(9000 + i, F=11, n_feat=150) for i in range(N_WIN)]
    ins, outs, keep = h.init_relpose_pack(rwins, timed=True)
    wall, dev = [], []
    for rep in range(REPEATS + 1):
        t0 = time.perf_counter()
        rc = h.lib.vg_init_relpose(h.h, N_WIN, ins, outs)
        wall.append((time.perf_counter() - t0) * 1e3)
        assert rc == 0, h.lib.vg_last_error(h.h)
        dev.append(sum(float(x) for x in keep[0]['device_ms']))
    res['init_relpose_first_candidate_wins'] = dict(allocating_call_wall_ms=wall[0], call_wall_ms=wall[1:], device_ms_total=dev[1:],
                                                    recorded_parent_call_wall_ms=[6.4, 5.5, 5.6], recorded_parent_device_ms=2.0)
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
