"""MANUAL (not collected): what relocalisation frames cost a resident sequence, 256 windows of EuRoC shape (K = 11, about 145 landmarks
per window) in resident IMU mode (vg_ba_seq_step_imu_async), driven through the Python binding with every frame packed beforehand.
One timed step = the step call + vg_ba_batch_download_state (which ends in a synchronise of the solve), host clock.

  a   a plain sequence (no reservation): this tree's library, and the parent commit's (--parent-lib, a child process of this script
      per repeat, alternating with this tree's) -- the claim is "unchanged"
  b   reserved (vg_ba_seq_relo_reserve), never armed: the price of the wider camera block (Rc 66 -> 72)
  c   reserved, 1 / 16 / 256 windows armed EVERY step with 25 matches; the vg_ba_seq_set_relo calls are inside the timed step
      (pre-built structs, one ctypes call per armed window) and are reported on their own as well
  d   what a caller had for ONE window of a plain sequence: vg_ba_seq_export + vg_ba_seq_get_tracks, the host's packing, vg_ba_optimize
      with the relocalisation factors on a second handle, vg_ba_seq_import + vg_ba_seq_imu_set -- the stall it puts on the handle.
      The pieces are timed one by one: the packing here is Python and is NOT counted in the sum the expectation is judged with.

The synthetic tracks thin out after a dozen frames, so a repeat is a chain of short runs (begin, --warm, --frames timed steps).
Expectation to confirm or refute: c with one armed window costs less than a + d.

    python tests/manual/gpu_seq_relo.py [--parent-lib <the parent commit's libvinsgpu.so>] [--out profiles/seq_relo.json]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402

pkg = graft.load_package()
K = 11
FRAME = 5           # relo_frame_local_index of every request


def spread(vals):
    return dict(values=[round(v, 4) for v in vals], median=float(np.median(vals)), min=float(min(vals)), max=float(max(vals)), spread=float(max(vals) - min(vals)))


class Chain:
    """the frames of one short run for `windows` windows (a few kinds of synthetic sequence, repeated), packed once"""

    def __init__(self, ba, windows, kinds, steps, matches):
        import seq_imu_model as I
        from vins_mono_amd import synth
        self.I, self.ba, self.n, self.steps = I, ba, windows, steps
        ks = [synth.FrameSource(synth.SyntheticSequence(900 + s, n_frames=K + steps + 1, K=K + steps + 1, L=150), noise_seed=900 + s) for s in range(kinds)]
        self.srcs = [ks[w % kinds] for w in range(windows)]
        kw = [s.initial_window(K, 0) for s in ks]
        for w_ in kw:
            w_['tracks'].sort(key=lambda t: t['id'])            # ascending ids along the list, as in the running system
        self.wins = [kw[w % kinds] for w in range(windows)]
        self.inputs = [synth.sequence_inputs(w_) for w_ in kw]
        self.seeds = [I.seed_of(s, w_, K) for s, w_ in zip(self.srcs, self.wins)]
        self.noise = I.noise_of(ks[0].seq)
        kf = [[I.frame_of(s, K - 1 + t) for s in ks] for t in range(steps)]
        self.frames = [ba.Handle.seq_pack_frames_imu([kf[t][w % kinds] for w in range(windows)]) for t in range(steps)]
        # a request per kind: up to `matches` tracks of the initial window anchored at or before the loop frame, at their first observation
        self.reqs = []
        for w_ in kw:
            tr = [t for t in w_['tracks'] if 1 <= t['start'] <= FRAME and len(t['obs']) >= 4][:matches]
            ids = np.array([t['id'] for t in tr], np.int32)
            xy = np.array([[t['obs'][0][0] + 0.002, t['obs'][0][1] - 0.002] for t in tr], float)
            r = ba.ReloFrame()
            r.struct_size, r.frame, r.pose, r.n_match = C.sizeof(ba.ReloFrame), FRAME, None, len(ids)
            r.match_id, r.match_xy = ids.ctypes.data_as(C.POINTER(C.c_int)), xy.ctypes.data_as(C.POINTER(C.c_double))
            r.prev_relo_r[:] = [1, 0, 0, 0, 1, 0, 0, 0, 1]
            self.reqs.append((r, ids, xy))
        self.kinds = kinds

    def begin(self, h, reserve):
        if reserve:
            h.seq_relo_reserve(reserve)
        probs, trks = zip(*[self.inputs[w % self.kinds] for w in range(self.n)])
        h.seq_begin(list(probs), list(trks), max_features=512, max_new_obs=512, init_depth=5.0, min_parallax=10.0 / 460.0)
        h.seq_imu_begin(self.seeds, self.noise, max_samples=32)
        h.ba_prepare_download()


def run_variant(h, chain, reserve, armed, warm, runs):
    """mean ms per timed step over `runs` short runs; also the mean ms spent in the arming calls and the factors of window 0"""
    lib, hh = h.lib, h.h
    step_ms, arm_ms, nf = [], [], []
    for _ in range(runs):
        chain.begin(h, reserve)
        try:
            for t in range(chain.steps):
                n, fp = chain.frames[t][0], chain.frames[t][1]
                t0 = time.perf_counter()
                for w in range(armed):
                    rc = lib.vg_ba_seq_set_relo(hh, w, C.byref(chain.reqs[w % chain.kinds][0]))
                    if rc:
                        raise RuntimeError("vg_ba_seq_set_relo: %d %s" % (rc, lib.vg_last_error(hh).decode()))
                t1 = time.perf_counter()
                rc = lib.vg_ba_seq_step_imu_async(hh, n, fp)
                if rc:
                    raise RuntimeError("vg_ba_seq_step_imu_async: %d %s" % (rc, lib.vg_last_error(hh).decode()))
                rc = h.ba_download_state_raw()
                t2 = time.perf_counter()
                if rc not in (0, -4):
                    raise RuntimeError("vg_ba_batch_download_state: %d" % rc)
                if t >= warm:
                    step_ms.append((t2 - t0) * 1e3)
                    arm_ms.append((t1 - t0) * 1e3)
            info = h.seq_info()
            bad = [i['status'] for i in info if i['status'] != 0]
            if bad:
                raise RuntimeError("a window reported status %r" % bad[:4])
            if armed:
                nf.append(h.seq_get_relo(0)['n_factors'])
            landmarks = info[0]['n_landmarks']
        finally:
            h.seq_end()
    return float(np.mean(step_ms)), float(np.mean(arm_ms)), (int(np.min(nf)) if nf else 0), landmarks, len(step_ms)


def run_detour(h, h2, chain, warm, runs):
    """d: ms of each piece of the hand-back detour for window 0 of a plain sequence, after `warm` steps"""
    import seq_relo_case as R
    from oracle.window_numpy import SlidingWindow
    from vins_mono_amd import ba
    pieces = dict(export_and_get_tracks=[], python_packing=[], vg_ba_optimize=[], import_and_imu_set=[])
    for _ in range(runs):
        chain.begin(h, 0)
        try:
            for t in range(warm):
                h.seq_step_imu(chain.frames[t])
                h.ba_download_state_raw()
            h.sync()
            base = chain.wins[0]['base']
            t0 = time.perf_counter()
            exp, trk = h.seq_export(0, K)
            seed = h.seq_imu_get(0)
            t1 = time.perf_counter()
            off = np.concatenate([[0], np.cumsum(trk['nobs'])])
            tracks = [dict(id=int(trk['id'][f]), start=int(trk['start'][f]), obs=trk['obs'][off[f]:off[f + 1]], depth=float(trk['depth'][f]), flag=int(trk['solve_flag'][f]))
                      for f in range(len(trk['id']))]
            win = SlidingWindow(K, base, exp['pose'], exp['sb'], exp['imu'], [None] * (K - 1), tracks)
            win.ex, win.td, win.prior = exp['ex'], exp['td'], exp['prior']
            prob = win.problem()
            _, ids, xy = chain.reqs[0]
            prob['relo'], sel, _ = R.host_relo(win, prob, dict(frame=FRAME, pose=None, match_id=ids, match_xy=xy))
            packed = ba.PackedProblem(prob)
            t2 = time.perf_counter()
            h2.ba_upload([packed], [ba.VG_MARGIN_OLD])
            h2.ba_run_async()
            h2.ba_prepare_download()
            h2.ba_download_raw()
            t3 = time.perf_counter()
            full = dict(base)
            full.update(pose=exp['pose'], sb=exp['sb'], ex=exp['ex'], td=exp['td'], imu=exp['imu'], prior=exp['prior'], relo=None, lm_start=np.zeros(0, np.int32),
                        lm_nobs=np.zeros(0, np.int32), obs_off=np.zeros(0, np.int32), obs=np.zeros((0, 7)), inv_depth=np.zeros(0))
            t4 = time.perf_counter()
            h.seq_import(0, full, trk)
            h.seq_imu_set(0, np.concatenate([seed['acc_0'], seed['gyr_0'], seed['g']]))
            t5 = time.perf_counter()
            pieces['export_and_get_tracks'].append((t1 - t0) * 1e3)
            pieces['python_packing'].append((t2 - t1 + t4 - t3) * 1e3)
            pieces['vg_ba_optimize'].append((t3 - t2) * 1e3)
            pieces['import_and_imu_set'].append((t5 - t4) * 1e3)
            n_relo = len(sel)
        finally:
            h.seq_end()
    out = {k: float(np.mean(v)) for k, v in pieces.items()}
    out['library_calls_ms'] = out['export_and_get_tracks'] + out['vg_ba_optimize'] + out['import_and_imu_set']
    out['relocalisation_factors'] = n_relo
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=256)
    ap.add_argument("--kinds", type=int, default=16)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--matches", type=int, default=25)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--lib", default=None, help="(child mode) the library to load")
    ap.add_argument("--only-plain", action="store_true", help="(child mode) print the plain variant's ms per step and leave")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.lib:
        pkg.LIB_PATH = os.path.abspath(a.lib)
    from vins_mono_amd import ba
    chain = Chain(ba, a.windows, a.kinds, a.warm + a.frames, a.matches)
    h = ba.Handle()
    if a.only_plain:
        print("PLAIN", run_variant(h, chain, 0, 0, a.warm, a.runs)[0])
        return
    h2 = ba.Handle()
    variants = [("a_plain", 0, 0), ("b_reserved_idle", a.matches, 0)] + [("c_armed_%d" % n, a.matches, min(n, a.windows)) for n in (1, 16, 256)]
    ms = {v[0]: [] for v in variants}
    arm = {v[0]: [] for v in variants}
    extra = {}
    parent, detour = [], []
    run_variant(h, chain, 0, 0, a.warm, 1)                       # (clocks, allocations)
    for rep in range(a.repeats):
        for name, reserve, armed in variants:
            m, am, nf, lm, nsteps = run_variant(h, chain, reserve, armed, a.warm, a.runs)
            ms[name].append(m); arm[name].append(am)
            extra[name] = dict(relocalisation_factors_window0=nf, landmarks_window0=lm, timed_steps_per_repeat=nsteps)
            print(rep, name, "ms per step", round(m, 4), "arming", round(am, 4), flush=True)
            if name == "a_plain" and a.parent_lib:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--lib", a.parent_lib, "--only-plain", "--windows", str(a.windows), "--kinds", str(a.kinds),
                                    "--frames", str(a.frames), "--warm", str(a.warm), "--runs", str(a.runs)], capture_output=True, text=True, timeout=900)
                if r.returncode != 0 or "PLAIN" not in r.stdout:
                    raise RuntimeError("the parent library's run failed:\n" + r.stdout[-1000:] + r.stderr[-2000:])
                parent.append(float(r.stdout.split("PLAIN")[1].split()[0]))
                print(rep, "a_plain_parent_library ms per step", round(parent[-1], 4), flush=True)
        detour.append(run_detour(h, h2, chain, a.warm, a.runs))
        print(rep, "d_detour", detour[-1], flush=True)
    res = dict(what=__doc__.split("\n\n")[0].replace("\n", " "), status="measured",
               shape=dict(windows=a.windows, K=K, landmarks=150, matches=a.matches, timed_steps_per_run=a.frames, warm_steps_per_run=a.warm, runs=a.runs,
                          repeats=a.repeats, timed_steps_per_variant_and_repeat=a.frames * a.runs, mode="resident IMU (vg_ba_seq_step_imu_async)"))
    for name, _, _ in variants:
        res[name] = dict(ms_per_step=spread(ms[name]), of_which_arming_calls_ms=spread(arm[name]), **extra[name])
    if parent:
        res["a_plain_parent_library"] = dict(ms_per_step=spread(parent))
        worst = max(res["a_plain"]["ms_per_step"]["spread"], res["a_plain_parent_library"]["ms_per_step"]["spread"])
        res["a_minus_parent_ms"] = res["a_plain"]["ms_per_step"]["median"] - res["a_plain_parent_library"]["ms_per_step"]["median"]
        res["a_unchanged_within_the_spreads"] = bool(abs(res["a_minus_parent_ms"]) <= worst)
    res["d_detour_one_window_ms"] = {k: spread([d[k] for d in detour]) for k in detour[0] if k != 'relocalisation_factors'}
    res["d_detour_one_window_ms"]["relocalisation_factors"] = detour[0]['relocalisation_factors']
    am, bm, c1 = (res[k]["ms_per_step"]["median"] for k in ("a_plain", "b_reserved_idle", "c_armed_1"))
    res["b_minus_a_ms"] = bm - am
    res["b_minus_a_beyond_the_spreads"] = bool(abs(bm - am) > max(res["a_plain"]["ms_per_step"]["spread"], res["b_reserved_idle"]["ms_per_step"]["spread"]))
    res["c1_ms"], res["a_plus_d_library_calls_ms"] = c1, am + res["d_detour_one_window_ms"]["library_calls_ms"]["median"]
    res["expectation_c1_below_a_plus_d"] = bool(c1 < res["a_plus_d_library_calls_ms"])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
