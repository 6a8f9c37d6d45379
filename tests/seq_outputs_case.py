"""TEST INFRASTRUCTURE: the keyframe message and the point clouds of a resident sequence (vg_ba_seq_outputs_reserve / _async /
vg_ba_seq_get_outputs; csrc/ba_seq.hip ba_seq_publish_kernel) against tests/seq_outputs_ref.py, which is fed from vg_ba_seq_get_tracks
and vg_ba_seq_export of the same window: the route a caller had before.  tests/test_seq_outputs_simt.py runs the cases on the emulated
kernels, tests/test_seq_outputs_gpu.py on the GPU, at the same shapes."""
import numpy as np

import seq_imu_model as I
import seq_model as M
import seq_outputs_ref as R
from vins_mono_amd import synth

FT = 512                      # max_features of the planted sequences (the largest table holds 300 selected tracks and 100 others)


# ---------------------------------------------------------------------------------------------------------------- planted tables
def plant(K, specs, seed, first_id=1):
    """A track table for vg_ba_seq_begin from (start_frame, n_obs, solve_flag) triples, in that order: ids ascending from first_id with
    gaps, depths in 2 .. 10 (a third of the unsolved ones -1: never triangulated), rows x y z u v vx vy cur_td with z = 1."""
    rng = np.random.default_rng(seed)
    n = len(specs)
    ids = first_id + np.cumsum(rng.integers(1, 4, n)) if n else np.zeros(0, int)
    start = np.array([s for s, _, _ in specs], np.int32)
    nobs = np.array([m for _, m, _ in specs], np.int32)
    flag = np.array([f for _, _, f in specs], np.int32)
    depth = rng.uniform(2.0, 10.0, n)
    depth[(flag == 0) & (np.arange(n) % 3 == 0)] = -1.0
    rows = []
    for m in nobs:
        xy = rng.uniform(-0.5, 0.5, 2) + np.cumsum(rng.normal(0, 0.01, (m, 2)), axis=0)
        for j in range(m):
            x, y = xy[j]
            rows.append([x, y, 1.0, 460.0 * x + 376.0, 460.0 * y + 240.0, rng.normal(0, 0.1), rng.normal(0, 0.1), 0.0])
    return dict(id=ids.astype(np.int32), start=start, nobs=nobs, depth=depth, solve_flag=flag, obs=np.array(rows, float).reshape(-1, 8))


def edge_specs(K):
    """Every (start_frame, n_obs) a table may hold (start + n_obs <= W: the newest slot is the next step's), each with solve_flag 0, 1
    and 2: start_frame on both sides of W - 2 (W - 3 in, W - 2 out), a last frame on both sides of W - 2 (W - 3 out, W - 2 in, W - 1 in),
    n_obs of 1, 2 and 3 at start_frame 0 and 1."""
    W = K - 1
    return [(s, m, f) for s in range(W) for m in range(1, W - s + 1) for f in (0, 1, 2)]


def selected_specs(K, n_sel, n_other, seed):
    """n_sel tracks that the keyframe list and the point cloud select (start 0 .. W - 3, reaching frame W - 2 or W - 1, solved),
    shuffled among n_other tracks that no list selects."""
    W = K - 1
    rng = np.random.default_rng(seed)
    sel = []
    for _ in range(n_sel):
        s = int(rng.integers(0, W - 2))
        last = int(rng.integers(W - 2, W))
        sel.append((s, last - s + 1, 1))
    other = [[(W - 2, 1, 1), (0, 1, 1), (0, 2, 0), (0, 2, 2), (W - 1, 1, 0)][k % 5] for k in range(n_other)]
    specs = sel + other
    order = rng.permutation(len(specs))
    return [specs[i] for i in order]


def all_selected_specs(K, n):
    """Every track in every list it can be in: at K = 4 (W = 3) start 0 with two observations is keyframe, cloud and margin at once; at
    larger K no track is in the keyframe list and the margin cloud together: keyframe + cloud there."""
    W = K - 1
    return [(0, 2, 1)] * n if W == 3 else [(k % (W - 2), W - 1 - k % (W - 2), 1) for k in range(n)]


def _windows(K, n, seed0=31):
    srcs = [synth.FrameSource(synth.SyntheticSequence(seed0 + i, n_frames=K + 2, K=K + 2, L=12), noise_seed=900 + i) for i in range(n)]
    return [synth.sequence_inputs(s.initial_window(K, 0))[0] for s in srcs]


def begin_planted(h, K, tables):
    probs = _windows(K, len(tables))
    h.seq_begin(probs, tables, max_features=FT, max_new_obs=64, max_landmarks=64, init_depth=5.0, min_parallax=10.0 / 460.0)


def check_all(h, K, max_points, where, info=None, mutant=None):
    """seq_outputs of every window against the restatement fed from seq_tracks + seq_export.  Returns ([device dict], [restatement],
    worst ulps)."""
    n = h._seq_n
    got, ref, worst = [], [], 0.0
    for w in range(n):
        t = h.seq_tracks(w, K)
        e = h.seq_export(w, K)[0]
        r = R.restate(t, e['pose'], e['ex'], K, None if info is None else info[w], mutant=mutant)
        g = h.seq_outputs(w)
        worst = max(worst, R.compare(g, r, max_points, (where, 'window', w)))
        got.append(g); ref.append(r)
    return got, ref, worst


PLANTED = {
    # name: K -> list of track tables (one or three windows)
    'edges': lambda K: [plant(K, edge_specs(K), 1), plant(K, [], 2), plant(K, all_selected_specs(K, 40), 3)],
    'lanes': lambda K: [plant(K, selected_specs(K, 1, 7, 4), 4), plant(K, selected_specs(K, 63, 20, 5), 5), plant(K, selected_specs(K, 64, 20, 6), 6)],
    'wide': lambda K: [plant(K, selected_specs(K, 65, 20, 7), 7), plant(K, selected_specs(K, 300, 100, 8), 8, first_id=(1 << 24) - 200),
                       plant(K, edge_specs(K)[::-1], 9)],
    'single': lambda K: [plant(K, edge_specs(K), 10)],
}


def case_planted(h, K, name, mutant=None):
    """Issue case 1: planted tables through vg_ba_seq_begin, vg_ba_seq_outputs_async with no step; keyframe_valid is 0."""
    tables = PLANTED[name](K)
    begin_planted(h, K, tables)
    try:
        h.seq_outputs_reserve(FT)
        h.seq_outputs_async()
        got, ref, worst = check_all(h, K, FT, ('planted', name, K), mutant=mutant)
        for g in got:
            assert g['keyframe_valid'] == 0 and g['status'] == 0
        W = K - 1
        if name == 'edges' and mutant is None:
            t = tables[0]
            # the edges are really there: selected and refused tracks on both sides of every comparison
            kf = set(ref[0]['kf'])
            on = lambda s, m, f: [i for i in range(len(t['id'])) if (t['start'][i], t['nobs'][i], t['solve_flag'][i]) == (s, m, f)]
            assert on(W - 3, 2, 1)[0] in kf and on(W - 3, 1, 1)[0] not in kf and on(W - 2, 1, 1)[0] not in kf
            assert on(W - 3, 2, 0)[0] not in kf and on(W - 3, 2, 2)[0] not in kf
            assert on(0, 1, 1)[0] not in set(ref[0]['cloud']) and on(0, 2, 1)[0] in set(ref[0]['margin']) and on(0, 3, 1)[0] not in set(ref[0]['margin'])
            assert (on(1, 2, 1)[0] in set(ref[0]['cloud'])) == (1 < W - 2) and on(1, 2, 1)[0] not in set(ref[0]['margin'])
            assert got[1]['n_keyframe'] == got[1]['n_cloud'] == got[1]['n_margin'] == 0
            assert got[2]['n_keyframe'] == got[2]['n_cloud'] == 40 and got[2]['n_margin'] == (40 if W == 3 else 0)
        if name == 'lanes' and mutant is None:
            assert [g['n_keyframe'] for g in got] == [1, 63, 64] and [g['n_cloud'] for g in got] == [1, 63, 64]
        if name == 'wide' and mutant is None:
            assert [g['n_keyframe'] for g in got[:2]] == [65, 300] and got[1]['kf_id'].max() > (1 << 24)
        return worst
    finally:
        h.seq_end()


def case_truncation(h, K):
    """Issue case 2: max_points = 64 against 65 and 300 selected tracks, a window with 3 between them."""
    tables = [plant(K, selected_specs(K, 65, 20, 11), 11), plant(K, selected_specs(K, 3, 9, 12), 12), plant(K, selected_specs(K, 300, 100, 13), 13)]
    begin_planted(h, K, tables)
    try:
        h.seq_outputs_reserve(64)
        h.seq_outputs_async()
        got, ref, worst = check_all(h, K, 64, ('truncation', K))
        assert [g['status'] for g in got] == [R.TRUNCATED, 0, R.TRUNCATED]
        assert [g['n_keyframe'] for g in got] == [65, 3, 300] and [g['n_cloud'] for g in got] == [65, 3, 300]
        assert [len(g['kf_id']) for g in got] == [64, 3, 64] and [len(g['cloud_xyz']) for g in got] == [64, 3, 64]
        # a larger reservation replaces the first: everything fits
        h.seq_outputs_reserve(300)
        h.seq_outputs_async()
        got, _, _ = check_all(h, K, 300, ('truncation, reserved again', K))
        assert [g['status'] for g in got] == [0, 0, 0] and len(got[2]['kf_id']) == 300
        return worst
    finally:
        h.seq_end()


# ---------------------------------------------------------------------------------------------------------------- after real steps
def _sources(seeds, Ls, K, n_steps, noise_seed):
    return [synth.FrameSource(synth.SyntheticSequence(s, n_frames=K + n_steps + 1, K=K + n_steps + 1, L=L), noise_seed=noise_seed + s) for s, L in zip(seeds, Ls)]


class HostFed:
    """vg_ba_seq_step_async with what ResidentEstimators does on the host (seq_model.drive_sequence, one frame per call)."""

    def __init__(self, h, srcs, K, min_parallax, max_features, max_landmarks):
        self.h, self.srcs, self.K = h, srcs, K
        wins = [s.initial_window(K, 0) for s in srcs]
        probs, trks = zip(*[synth.sequence_inputs(w) for w in wins])
        h.seq_begin(list(probs), list(trks), max_features=max_features, max_new_obs=max_features, max_landmarks=max_landmarks, init_depth=5.0,
                    min_parallax=min_parallax)
        self.newest = [(w['pose'][K - 1].copy(), w['sb'][K - 1].copy()) for w in wins]
        self.prev = [dict(samples=list(w['samples'][K - 3]), ba=s.seq.ba_lin, bg=s.seq.bg_lin) for w, s in zip(wins, srcs)]
        self.merged = [None] * len(srcs)

    def step(self, g):
        K, frames, cur = self.K, [], []
        for i, src in enumerate(self.srcs):
            smp = src.samples(g - 1)
            sb = self.newest[i][1]
            rec = src.preintegrate(smp, sb[3:6], sb[6:9])
            pose, sbn = M._propagate(self.newest[i][0], sb, smp, src.seq.cfg['g_norm'])
            ids, rows = src.image(g)
            frames.append(dict(pose=pose, sb=sbn, imu_new=rec, imu_merged=self.merged[i], ids=ids, obs=rows))
            cur.append(dict(samples=smp, ba=sb[3:6].copy(), bg=sb[6:9].copy()))
        self.h.seq_step(frames)
        sts, _ = self.h.seq_states(allow_numeric_failure=True)
        info = self.h.seq_info()
        for i, src in enumerate(self.srcs):
            if info[i]['status'] == 0:
                self.newest[i] = (sts[i]['pose'][K - 1].copy(), sts[i]['sb'][K - 1].copy())
            if info[i]['flag'] == M.NEW:
                self.prev[i]['samples'] = self.prev[i]['samples'] + cur[i]['samples'][1:]
                self.merged[i] = src.preintegrate(self.prev[i]['samples'], self.prev[i]['ba'], self.prev[i]['bg'])
            else:
                self.prev[i], self.merged[i] = cur[i], None
        return info


class ImuFed:
    """vg_ba_seq_step_imu_async: raw samples and observations only."""

    def __init__(self, h, srcs, K, min_parallax, max_features, max_landmarks):
        self.h, self.srcs = h, srcs
        wins = [s.initial_window(K, 0) for s in srcs]
        probs, trks = zip(*[synth.sequence_inputs(w) for w in wins])
        h.seq_begin(list(probs), list(trks), max_features=max_features, max_new_obs=max_features, max_landmarks=max_landmarks, init_depth=5.0,
                    min_parallax=min_parallax)
        h.seq_imu_begin([I.seed_of(s, w, K) for s, w in zip(srcs, wins)], I.noise_of(srcs[0].seq), max_samples=20)

    def step(self, g):
        self.h.seq_step_imu([I.frame_of(s, g) for s in self.srcs])
        self.h.seq_states(allow_numeric_failure=True)
        return self.h.seq_info()


def case_steps(h, K, imu, n_steps=4, void=True, mutant=None, min_parallax=0.25):
    """Issue case 3: a small synthetic sequence, the outputs after every step against the restatement, keyframe_valid against
    info[VG_SEQ_FLAG]; both marginalization flags are taken.  void: three windows, the middle one holds more landmarks than
    max_landmarks (its steps are void: VG_ERR_UNSUPPORTED) between two that fit.  Returns (flags per step, worst ulps)."""
    # (L = 70: a frame tracks more than 20 features, below which the key-frame test always says "key frame")
    seeds, Ls = ((22, 24, 23), (70, 150, 70)) if void else ((22,), (70,))
    srcs = _sources(seeds, Ls, K, n_steps, 700)
    drv = (ImuFed if imu else HostFed)(h, srcs, K, min_parallax, 192, 64)
    flags, worst, sizes = [], 0.0, []
    try:
        h.seq_outputs_reserve(128)
        h.seq_outputs_async()                                   # before the first step: the initial window, nothing solved yet
        got, _, _ = check_all(h, K, 128, ('steps', K, imu, 'begin'), mutant=mutant)
        assert all(g['keyframe_valid'] == 0 and g['n_keyframe'] == 0 for g in got)
        for step in range(n_steps):
            info = drv.step(K - 1 + step)
            h.seq_outputs_async()
            got, ref, e = check_all(h, K, 128, ('steps', K, imu, step), info=info, mutant=mutant)
            worst = max(worst, e)
            flags.append([i['flag'] for i in info])
            for w, (g, i) in enumerate(zip(got, info)):
                assert g['keyframe_valid'] == (1 if i['flag'] == M.OLD else 0), (step, w)
                if void and w == 1:
                    assert i['status'] == -3 and g['status'] == -3 and g['n_keyframe'] == g['n_cloud'] == g['n_margin'] == 0, (step, i, g['status'])
                else:
                    assert i['status'] == 0 and g['status'] == 0, (step, w, i)
            sizes.append([(g['n_keyframe'], g['n_cloud'], g['n_margin']) for g in got])
        good = [w for w in range(len(seeds)) if not (void and w == 1)]
        if mutant is None:
            taken = {f[w] for f in flags for w in good}
            assert taken == {M.OLD, M.NEW}, ("the frames must take both marginalization flags", flags)
            assert max(s[w][0] for s in sizes for w in good) >= 5 and max(s[w][1] for s in sizes for w in good) >= 5, sizes
        print("sequence outputs after real steps, K", K, "IMU mode" if imu else "host-fed", "flags", flags, "sizes", sizes, "worst ulps", worst)
        return flags, worst
    finally:
        h.seq_end()


# ---------------------------------------------------------------------------------------------------------------- read-only
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same_window(ha, hb, w, K, where):
    ta, tb = ha.seq_tracks(w, K), hb.seq_tracks(w, K)
    for k in ta:
        assert np.array_equal(_bits(ta[k]), _bits(tb[k])), (where, 'tracks', k)
    ea, eb = ha.seq_export(w, K, raw_imu=True)[0], hb.seq_export(w, K, raw_imu=True)[0]
    for k in ('pose', 'sb', 'ex'):
        assert np.array_equal(_bits(ea[k]), _bits(eb[k])), (where, 'export', k)
    assert ea['td'] == eb['td']
    for ra, rb in zip(ea['imu'], eb['imu']):
        for k in ra:
            assert np.array_equal(_bits(np.asarray(ra[k], np.float64)), _bits(np.asarray(rb[k], np.float64))), (where, 'imu', k)
    pa, pb = ea['prior'], eb['prior']
    assert (pa is None) == (pb is None)
    if pa is not None:
        assert (pa['n'], pa['m'], pa['blocks']) == (pb['n'], pb['m'], pb['blocks']), (where, 'prior blocks')
        for k in ('J0', 'r0'):
            assert np.array_equal(_bits(pa[k]), _bits(pb[k])), (where, 'prior', k)
        for xa, xb in zip(pa['x0'], pb['x0']):
            assert np.array_equal(_bits(xa), _bits(xb)), (where, 'prior x0')


def case_read_only(h_a, h_b, K=11):
    """Issue case 4: two identical handles; vg_ba_seq_outputs_async on one of them only, between two steps: track tables, exports and
    the next step's states are bit-identical."""
    mk = lambda: _sources((22, 23), (30, 30), K, 3, 700)
    da, db = ImuFed(h_a, mk(), K, 0.25, 128, 48), ImuFed(h_b, mk(), K, 0.25, 128, 48)
    try:
        da.step(K - 1); db.step(K - 1)
        for w in range(2):
            _same_window(h_a, h_b, w, K, ('before', w))
        h_a.seq_outputs_reserve(96)
        h_a.seq_outputs_async()
        assert h_a.seq_outputs(0)['n_cloud'] > 0
        for w in range(2):
            _same_window(h_a, h_b, w, K, ('after the call', w))
        h_a.seq_outputs_async()                                 # (and once more right in front of the step, not waited for)
        ia, ib = da.step(K), db.step(K)
        assert ia == ib
        sa, sb = h_a.seq_states()[0], h_b.seq_states()[0]
        for w in range(2):
            for k in ('pose', 'sb', 'ex', 'inv_depth'):
                assert np.array_equal(_bits(sa[w][k]), _bits(sb[w][k])), ('next step', w, k)
            _same_window(h_a, h_b, w, K, ('after the next step', w))
    finally:
        h_a.seq_end(); h_b.seq_end()


# ---------------------------------------------------------------------------------------------------------------- mutations
MUTANT_CASE = {
    # mutant: (named case that must tell it apart, callable)
    'pose_index': ('planted edges K=11', lambda h, m: case_planted(h, 11, 'edges', mutant=m)),
    'no_tic': ('planted edges K=4', lambda h, m: case_planted(h, 4, 'edges', mutant=m)),
    'newest_row': ('planted edges K=11', lambda h, m: case_planted(h, 11, 'edges', mutant=m)),
    'last_frame_gt': ('planted edges K=4', lambda h, m: case_planted(h, 4, 'edges', mutant=m)),
    'solve_nonzero': ('planted edges K=11', lambda h, m: case_planted(h, 11, 'edges', mutant=m)),   # (after a step no track keeps flag 2: removeFailures)
}


def case_mutation(h, mutant):
    """Issue case 5: the mutated restatement does not pass where the true one does."""
    import pytest
    name, run = MUTANT_CASE[mutant]
    # what R.compare reports first for that mutant: the pose of another frame; world points off by tic; another row's x y; a list that
    # loses the tracks ending in frame W - 2 / gains the failed ones
    first = dict(pose_index="'pose'", no_tic="'ulps'", newest_row="'kf_norm'", last_frame_gt="'counts'", solve_nonzero="'counts'")[mutant]
    with pytest.raises(AssertionError, match=first):
        run(h, mutant)
    return name


# ---------------------------------------------------------------------------------------------------------------- the C++ caller
def _parse_outputs(path):
    """<out>.outputs of `vins_replay seq` with VINS_REPLAY_OUTPUTS: {(frame, estimator): dict like Handle.seq_outputs + stamp, R}"""
    recs, cur = {}, None
    for line in open(path).read().strip().splitlines():
        tag, *v = line.split(",")
        if tag == "F":
            cur = dict(keyframe_valid=int(v[2]), status=int(v[3]), n_keyframe=int(v[4]), n_cloud=int(v[5]), n_margin=int(v[6]), stamp=float(v[7]),
                       kf_id=[], kf_point_3d=[], kf_uv=[], kf_norm=[], cloud_xyz=[], margin_xyz=[])
            recs[(int(v[0]), int(v[1]))] = cur
        elif tag == "P":
            cur['T'], cur['R'] = np.array(v[:3], float), np.array(v[3:], float).reshape(3, 3)
        elif tag == "k":
            f = [np.float32(x) for x in v[1:]]
            cur['kf_id'].append(int(v[0])); cur['kf_point_3d'].append(f[:3]); cur['kf_uv'].append(f[3:5]); cur['kf_norm'].append(f[5:7])
        else:
            cur['cloud_xyz' if tag == "c" else 'margin_xyz'].append([np.float32(x) for x in v])
    for r in recs.values():
        r['kf_id'] = np.array(r['kf_id'], np.int32)
        for k, c in (('kf_point_3d', 3), ('kf_uv', 2), ('kf_norm', 2), ('cloud_xyz', 3), ('margin_xyz', 3)):
            r[k] = np.array(r[k], np.float32).reshape(-1, c)
    return recs


def case_cpp(h, exe, tmp_path, timeout=900, K=11, n_frames=4, L=40, min_parallax=10.0 / 460.0, max_points=256):
    """Issue case 8: `vins_replay seq` with VINS_REPLAY_OUTPUTS (ResidentEstimators::usePublishedOutputs, keyframe(), pointCloud(),
    marginCloud(), vg_unpack_keyframe) against the same frames driven through the Python binding, built and driven the way
    seq_relo_case.case_cpp does.  Decisions, counts, ids, order and the copied float32 observations are equal; the world points and the
    pose come from two free-running chains (propagation in C++ / NumPy) that agree to 1e-9 on these frames: they are held to
    compare_replay_csv's bound of 1e-6, relative to max(1, |.|) (measured 3.9e-10; the four-frame data set of seq_relo_case.case_cpp:
    on the three-frame one of the same seeds the two chains part by 1e-5 in frame 2 whatever is published).  Without the switch the
    tool writes no .outputs file and its own output is the same."""
    import os
    import subprocess
    seeds = (22, 23)
    mk = lambda: [M.FrameSource(synth.SyntheticSequence(s, n_frames=K + n_frames + 1, K=K + n_frames + 1, L=L), noise_seed=200 + s) for s in seeds]
    src = mk()
    M.write_seq_file(tmp_path / "frames.bin", src, K, n_frames, min_parallax=min_parallax)
    args = [exe, "seq", str(tmp_path / "frames.bin")]
    r0 = subprocess.run(args + [str(tmp_path / "plain.csv")], capture_output=True, text=True, timeout=timeout)
    assert r0.returncode == 0, r0.stderr[-2000:]
    assert not os.path.exists(str(tmp_path / "plain.csv") + ".outputs")
    r = subprocess.run(args + [str(tmp_path / "out.csv")], capture_output=True, text=True, timeout=timeout,
                       env=dict(os.environ, VINS_REPLAY_OUTPUTS=str(max_points)))
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(tmp_path / "plain.csv").read() == open(tmp_path / "out.csv").read() and r0.stderr == r.stderr      # the tool's own output is unchanged
    got = _parse_outputs(str(tmp_path / "out.csv") + ".outputs")
    src = mk()
    drv = HostFed(h, src, K, min_parallax, 512, 0)
    headers = [[float(s.seq.times[min(k, K - 2)]) for k in range(K)] for s in src]
    worst, seen = 0.0, 0
    close = lambda a, b: float(np.abs(np.asarray(a, float) - np.asarray(b, float)).max() / max(1.0, np.abs(np.asarray(b, float)).max())) if np.size(b) else 0.0
    try:
        h.seq_outputs_reserve(max_points)
        for w in range(n_frames):
            g = K - 1 + w
            info = drv.step(g)
            h.seq_outputs_async()
            for i in range(len(seeds)):
                hd = headers[i]
                hd[K - 1] = float(src[i].seq.times[g])
                headers[i] = hd = (hd[1:] + [hd[K - 1]]) if info[i]['flag'] == M.OLD else (hd[:K - 2] + [hd[K - 1], hd[K - 1]])
                want, c = h.seq_outputs(i), got[(w, i)]
                for k in ('keyframe_valid', 'status', 'n_keyframe', 'n_cloud', 'n_margin'):
                    assert c[k] == want[k], (w, i, k, c[k], want[k])
                assert c['stamp'] == hd[K - 3], (w, i, 'stamp')
                assert np.array_equal(c['kf_id'], want['kf_id']), (w, i, 'ids')
                assert np.array_equal(c['kf_uv'].view(np.uint32), want['kf_uv'].view(np.uint32)) and np.array_equal(c['kf_norm'].view(np.uint32), want['kf_norm'].view(np.uint32))
                e = max(close(c['kf_point_3d'], want['kf_point_3d']), close(c['cloud_xyz'], want['cloud_xyz']), close(c['margin_xyz'], want['margin_xyz']),
                        close(c['T'], want['pose'][:3]), close(c['R'], R.q2R(want['pose'][3:])))
                assert c['cloud_xyz'].shape == want['cloud_xyz'].shape and c['margin_xyz'].shape == want['margin_xyz'].shape
                worst = max(worst, e)
                assert e <= 1e-6, (w, i, e)
                seen += len(c['kf_id']) + len(c['cloud_xyz'])
    finally:
        h.seq_end()
    assert seen > 50, seen
    print("vins_replay seq with VINS_REPLAY_OUTPUTS vs the binding: world points and pose", worst, "over", seen, "rows")
    return worst


# ---------------------------------------------------------------------------------------------------------------- the chain
def case_chain(h_a, h_b, data, min_loop_num=8, max_points=256, reproj_threshold=0.1):
    """Issue case 7: two rigs of tests/vio_bridge_case.py (front end + sequence in IMU mode on one handle each) take the same rendered
    frames through vg_vio_step_async until a keyframe is valid.  Then, for stream 0: the message -> vg_kf_add of the keyframe's image
    (frame W - 2 of the window) with the message's kf_uv as window points -> vg_kf_match against the record of the first frame of the
    run -> vg_kf_pnp with kf_point_3d / kf_id gathered by matched_index, the message's pose and ex_pose -> vg_ba_seq_set_relo -> a
    vg_vio_step_async -> vg_ba_seq_get_relo.  Handle A takes the message from vg_ba_seq_outputs_async behind vg_vio_step_async, handle B
    from the NumPy restatement fed from vg_ba_seq_get_tracks + vg_ba_seq_export: everything downstream is equal bit for bit.
    The frames are those of the bridge's own tests (tests/e2e_vio.Scene): the pair of tests/kf_brief_ref.py that the vg_kf_pnp chain
    test matches is two frames long and has no trajectory, IMU samples or seeded windows to run vg_vio_step_async on.
    The gates of vg_kf_pnp are opened (min_loop_num 8 for 25, reproj_threshold 0.1, no yaw or distance gate): the rigs' windows are
    seeded from noisy guesses and solved with two iterations, so the PnP pose of these world points is not a loop anybody would
    accept (measured on the staged frames: 7.8 m and 71 degrees); what is checked is that the message feeds every call of the chain
    with what the restatement feeds it, and that RANSAC keeps inliers, so that the relocalisation frame carries factors.
    Returns (n_keyframe, n_matched, n_inliers, relocalisation factors)."""
    import kf_brief_ref as KB
    import vio_bridge_case as V
    from vins_mono_amd import fe
    K = data.K
    try:
        for h in (h_a, h_b):
            h.seq_relo_reserve(128)
        a, b = V.Rig(h_a, data), V.Rig(h_b, data)
        h_a.vio_begin(lists=False); h_b.vio_begin(lists=False)
        h_a.seq_outputs_reserve(max_points)
        first = a.f                                              # the frame the first step takes
        msg = None
        for _ in range(len(data.plan) - 1):
            a.vio_step(True); b.vio_step(True)
            h_a.seq_outputs_async()                              # behind vg_vio_step_async
            h_a.seq_states(); h_b.seq_states()
            o = h_a.seq_outputs(0)
            info = h_a.seq_info()
            t, e = h_b.seq_tracks(0, K), h_b.seq_export(0, K)[0]
            r = R.restate(t, e['pose'], e['ex'], K, h_b.seq_info()[0])
            R.compare(o, r, max_points, ('chain', a.f))
            assert o['keyframe_valid'] == (1 if info[0]['flag'] == M.OLD else 0)
            if o['keyframe_valid'] and o['n_keyframe'] > min_loop_num:
                msg = o
                break
        assert msg is not None, "no valid keyframe with enough points on these frames"
        sel = r['kf']
        routes = dict(a=(h_a, msg['kf_uv'], msg['kf_point_3d'], msg['kf_id'], msg['pose'], msg['ex_pose']),
                      b=(h_b, r['kf_uv'][sel], r['world'][sel].astype(np.float32), r['kf_id'][sel], r['pose'], r['ex_pose']))
        img_kf, img_old = data.frames[0][a.f - 2], data.frames[0][data.g0]      # slot W - 2 after a MARGIN_OLD slide holds the frame before the last
        cam = fe.Camera.pinhole(*data.intr)
        reqs, seen = {}, {}
        for name, (h, uv, p3, ids, pose, ex) in routes.items():
            kf = fe.KeyFrames(h, data.W, data.H, 500, max_points, 2, KB.pattern())
            kf.add([0, 1], [img_kf, img_old], [cam] * 2, [np.ascontiguousarray(uv, np.float32), np.zeros((0, 2), np.float32)], arrays=False)
            m = kf.match([(0, 1)])[0]
            n = int(m['n_matched'])
            idx = np.asarray(m['matched_index'][:n], int)
            g = fe.kf_pnp(h, [dict(point_3d=p3[idx], old_norm=np.asarray(m['matched_old_norm'], np.float32)[:n], point_id=ids[idx], origin_vio_T=pose[:3],
                                   origin_vio_R=R.q2R(pose[3:]), tic=ex[:3], qic=R.q2R(ex[3:]), min_loop_num=min_loop_num, reproj_threshold=reproj_threshold, max_yaw_deg=180.0, max_dist=1e3)])[0]
            seen[name] = dict(n_matched=n, idx=idx, status=g['status'], n_inliers=g['n_inliers'], has_loop=g['has_loop'], match_id=np.asarray(g['match_id']),
                              match_xy=np.asarray(g['match_xy'], np.float64), loop_info=np.asarray(g['loop_info'], np.float64))
            order = np.argsort(seen[name]['match_id'], kind='stable')
            reqs[name] = dict(frame=K - 3, pose=None, match_id=seen[name]['match_id'][order].astype(np.int32), match_xy=seen[name]['match_xy'][order],
                              prev_t=np.array([0.3, -0.2, 0.1]), prev_r=np.eye(3))
        sa, sb = seen['a'], seen['b']
        assert sa['n_matched'] == sb['n_matched'] > min_loop_num, (sa['n_matched'], sb['n_matched'])
        for k in ('idx', 'match_id', 'match_xy', 'loop_info'):
            V.same_bits(sa[k], sb[k], ('chain', k))
        assert sa['status'] == sb['status'] == 0 and sa['n_inliers'] == sb['n_inliers'] > min_loop_num and sa['has_loop'] == sb['has_loop'] == 1, (sa, sb)
        assert len(np.unique(sa['match_id'])) == len(sa['match_id'])
        h_a.seq_set_relo(0, reqs['a']); h_b.seq_set_relo(0, reqs['b'])
        a.vio_step(True); b.vio_step(True)
        V.same_snapshot(a.snapshot(), b.snapshot(), ("chain", "armed step"))
        ra, rb = h_a.seq_get_relo(0), h_b.seq_get_relo(0)
        for k in ra:
            V.same_bits(np.asarray(ra[k], np.float64), np.asarray(rb[k], np.float64), ("chain", "relo", k))
        assert ra['armed'] == 1 and ra['n_factors'] >= 2, ra
        out = (int(msg['n_keyframe']), sa['n_matched'], int(sa['n_inliers']), int(ra['n_factors']))
        print("chain from the keyframe message into the relocalisation frame: keyframe points, matches, PnP inliers, factors", out)
        return out
    finally:
        V.release(h_a, h_b)


# ---------------------------------------------------------------------------------------------------------------- stand-alone program
SAN_CASES = {
    # name: (K, tables, max_points): issue cases 1 (edges, an empty table, a full one, K = 4; the lane counts, K = 11) and 2 (truncation)
    'edges4': lambda: (4, PLANTED['edges'](4), FT),
    'lanes11': lambda: (11, PLANTED['lanes'](11), FT),
    'truncation11': lambda: (11, [plant(11, selected_specs(11, 65, 20, 11), 11), plant(11, selected_specs(11, 3, 9, 12), 12),
                                  plant(11, selected_specs(11, 300, 100, 13), 13)], 64),
}


def write_san_case(path, K, tables, max_points):
    """The input of tests/seq_outputs_san_main.cpp: the windows of begin_planted and their tables."""
    probs = _windows(K, len(tables))
    with open(path, "wb") as f:
        f.write(np.array([0x314F5153, len(tables), K, FT, max_points], np.int32).tobytes())
        for p, t in zip(probs, tables):
            for a in (p['pose'], p['sb'], p['ex']):
                f.write(np.ascontiguousarray(a, np.float64).tobytes())
            f.write(np.array([len(t['id'])], np.int32).tobytes())
            for k in ('id', 'start', 'nobs', 'solve_flag'):
                f.write(np.ascontiguousarray(t[k], np.int32).tobytes())
            f.write(np.ascontiguousarray(t['depth'], np.float64).tobytes())
            f.write(np.ascontiguousarray(t['obs'], np.float64).tobytes())


def san_lines(h, K, tables, max_points):
    """What the program prints, from the binding."""
    hx = lambda a: " ".join(f"{int(v):08x}" for v in np.ascontiguousarray(a, np.float32).view(np.uint32).ravel())
    begin_planted(h, K, tables)
    lines = []
    try:
        h.seq_outputs_reserve(max_points)
        h.seq_outputs_async()
        for w in range(len(tables)):
            o = h.seq_outputs(w)
            lines.append(f"W {w} {o['status']} {o['keyframe_valid']} {o['n_keyframe']} {o['n_cloud']} {o['n_margin']}")
            lines.append("pose " + " ".join(f"{int(v):016x}" for v in np.concatenate([o['pose'], o['ex_pose']]).view(np.uint64)))
            lines += [f"k {int(i)} {hx(p)} {hx(n)} {hx(u)}" for i, p, n, u in zip(o['kf_id'], o['kf_point_3d'], o['kf_norm'], o['kf_uv'])]
            lines += ["c " + hx(p) for p in o['cloud_xyz']] + ["m " + hx(p) for p in o['margin_xyz']]
        h.seq_outputs_reserve(1)
        h.seq_outputs_async()
        for w in range(len(tables)):
            o = h.seq_outputs(w)
            lines.append(f"S {w} {o['status']} {o['n_keyframe']} {o['n_cloud']} {o['n_margin']}")
    finally:
        h.seq_end()
    return lines


# ---------------------------------------------------------------------------------------------------------------- refusals
def case_refusals(h, K=4):
    """Issue case 6: every refusal is VG_ERR_BAD_ARG with a text, and moves nothing: the message fetched afterwards is the one from
    before."""
    import pytest

    def refused(fn, text):
        with pytest.raises(RuntimeError, match="status -1.*" + text):
            fn()
    # no live sequence
    refused(lambda: h.seq_outputs_reserve(8), "no running sequence")
    refused(h.seq_outputs_async, "no running sequence")
    refused(lambda: h.seq_outputs(0), "no running sequence")
    begin_planted(h, K, PLANTED['lanes'](K))
    try:
        refused(h.seq_outputs_async, "no reservation")
        refused(lambda: h.seq_outputs(0), "no reservation")
        for bad in (0, -3, 1025):
            refused(lambda: h.seq_outputs_reserve(bad), "max_points")
        refused(h.seq_outputs_async, "no reservation")            # (a refused reservation reserves nothing)
        h.seq_outputs_reserve(80)
        refused(lambda: h.seq_outputs(0), "no vg_ba_seq_outputs_async")
        h.seq_outputs_async()
        before = [h.seq_outputs(w) for w in range(3)]
        refused(lambda: h.seq_outputs(-1), "no such window")
        refused(lambda: h.seq_outputs(3), "no such window")
        refused(lambda: h.seq_outputs(0, struct_size=8), "struct_size")
        refused(lambda: h.seq_outputs_reserve(2000), "max_points")
        after = [h.seq_outputs(w) for w in range(3)]              # (the refused reservation left the old one and its message)
        for a, b in zip(before, after):
            for k in a:
                assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
        check_all(h, K, 80, ('refusals', K))
        h.seq_outputs_reserve(70)                                 # a new reservation: the old message is gone
        refused(lambda: h.seq_outputs(0), "no vg_ba_seq_outputs_async")
    finally:
        h.seq_end()
    refused(h.seq_outputs_async, "no running sequence")           # vg_ba_seq_end freed the reservation with the sequence
    begin_planted(h, K, PLANTED['single'](K))
    try:
        refused(h.seq_outputs_async, "no reservation")            # ... and the next sequence starts without one
    finally:
        h.seq_end()
