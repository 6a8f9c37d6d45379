"""MANUAL (MI355X): what vg_init_relpose costs.  256 windows of F = 11 frames, 150 features, in two variants: every window's FIRST
candidate wins (the usual trajectory: every candidate passes the gate, 2560 RANSACs) and the LAST candidate wins (frames 0 .. F-3 stand
next to F-1, only F-2 passes the gate: 256 RANSACs).  One allocating call, reported on its own, then three repeats: wall time of the C call
(packing outside the timed region) and the device time of its nine launches from events (vg_relpose_out::device_ms).  For scale, in the
same run: vg_init_sfm and vg_init_align over as many windows.  The project has no host relativePose to compare with: no speed-up is
claimed.

usage: python tests/manual/gpu_init_relpose.py [--out profiles/init_relpose_measured.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
N_WIN, F, N_FEAT, REPEATS = 256, 11, 150, 3
LAUNCHES = ("gather", "samples_1", "counts_1", "bookkeeping_1", "samples_2", "counts_2", "bookkeeping_2", "pose", "pick")


def timed_calls(fn, check):
    wall = []
    for rep in range(REPEATS + 1):
        t0 = time.perf_counter()
        rc = fn()
        t1 = time.perf_counter()
        check(rc)
        wall.append((t1 - t0) * 1e3)
    return wall[0], wall[1:]


def run():
    import __graft_entry__ as g
    g.load_package()
    from vins_mono_amd import ba
    import init_align_ref as A
    import init_relpose_ref as R
    import init_sfm_ref as S
    last_xs = [1.3 + 0.001 * i for i in range(F - 2)] + [0.0, 1.3]
    variants = dict(first_candidate_wins=[R.scene(9000 + i, F=F, n_feat=N_FEAT) for i in range(N_WIN)],
                    last_candidate_wins=[R.scene(9500 + i, F=F, n_feat=N_FEAT, xs=last_xs) for i in range(N_WIN)])
    res = dict(what=f"vg_init_relpose, {N_WIN} windows, F = {F}, {N_FEAT} features; one allocating call, then {REPEATS} repeats", launches=LAUNCHES)
    for name, wins in variants.items():
        h = ba.Handle()                                     # (a handle of its own: the first call of each variant allocates)
        ins, outs, keep = h.init_relpose_pack(wins, timed=True)
        dev = []

        def call():
            rc = h.lib.vg_init_relpose(h.h, N_WIN, ins, outs)
            dev.append([float(x) for x in keep[0]['device_ms']])
            return rc

        def ok(rc):
            assert rc == 0, h.lib.vg_last_error(h.h)

        first, wall = timed_calls(call, ok)
        ls = [int(o.l) for o in outs]
        res[name] = dict(allocating_call_wall_ms=first, call_wall_ms=wall, device_ms_per_launch=dev[1:], device_ms_total=[sum(d) for d in dev[1:]],
                         l={str(v): ls.count(v) for v in sorted(set(ls))}, gated_candidates=int(sum(int(b['gate'].sum()) for b in keep)),
                         fallback_candidates=int(sum(int(b['used_fallback'].sum()) for b in keep)))
        h.close()
    # for scale: the two calls behind it over as many windows
    h = ba.Handle()
    swins = [S.scene(7000 + i, F=F, l=int(i % (F - 1)), n_feat=N_FEAT, nonkey=True) for i in range(N_WIN)]
    ins, outs, keep = h.init_sfm_pack(swins)
    first, wall = timed_calls(lambda: h.lib.vg_init_sfm(h.h, N_WIN, ins, outs), lambda rc: None)
    res['init_sfm_same_window_count'] = dict(allocating_call_wall_ms=first, call_wall_ms=wall, recorded_parent_ms=10.8)
    awins = [A.scene(5000 + i, F, 20, noise=0.01, key='all') for i in range(N_WIN)]
    ins2, outs2, keep2 = h.init_align_pack(awins)
    first, wall = timed_calls(lambda: h.lib.vg_init_align(h.h, N_WIN, ins2, outs2), lambda rc: None)
    res['init_align_same_window_count'] = dict(allocating_call_wall_ms=first, call_wall_ms=wall, recorded_parent_ms=2.1)
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
