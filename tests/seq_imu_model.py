"""TEST INFRASTRUCTURE: drivers of the device-resident sequences that take raw IMU samples (vg_ba_seq_imu_begin /
vg_ba_seq_step_imu_async: Estimator::processIMU and the IMU part of slideWindow() on the device, csrc/ba_seq.hip).

The checked step compares ONE frame's IMU work on identical inputs, per step and window: before the step seq_export gives the newest
state and the record of interval K-3, seq_imu_get the resident measurement; after it seq_imu_get gives the propagated guess and
seq_export the records.  Expected values are computed in NumPy from the device's OWN exported state (seq_model._propagate for the
guess, synth.preintegrate for the records) and once more on the device through Handle.imu_preintegrate.  Bound for records and
guess: 1e-11 x max|expected| per field, the bound of the same arithmetic chain in tests/test_ba_gpu.py
(test_imu_preintegration_on_device); linearisation biases, valid flags and acc_0 / gyr_0 are compared exactly.

On top of that every record is held in its OWN scale (tests/imu_ref.py): record_error against the 80-bit restatement of the same
samples <= M * E64 per field, M the one of tests/test_imu_scale.py.  E64 is the sequence's: what the float64 oracle loses on these
very inputs, and no less than the yardstick of the case table (a single record's e64 is one draw of the rounding noise; the table
is what M was measured against).  The merged record of a MARGIN_SECOND_NEW slide is checked against the 80-bit continuation of the
device's own exported record K-3 and against the 80-bit integration of the concatenated sample list."""
import numpy as np

import imu_ref as R80
import seq_model as M
from seq_model import NEW, OLD, _propagate
from vins_mono_amd import synth

BOUND = 1e-11
REC_FIELDS = ('delta_p', 'delta_q', 'delta_v', 'jacobian', 'covariance')


def noise_of(seq):
    c = seq.cfg
    return (c['acc_n'], c['gyr_n'], c['acc_w'], c['gyr_w'])


def rows_of(samples):
    """(n, 7) rows dt acc gyr of a synth sample list (its entry 0, the first measurement, is not a sample)."""
    return np.array([np.concatenate([[dt], a, g]) for dt, a, g in samples[1:]], float).reshape(-1, 7)


def samples_of(acc_0, gyr_0, rows):
    """The synth sample list of an interval that starts from the measurement acc_0 / gyr_0."""
    return [(0.0, np.array(acc_0, float), np.array(gyr_0, float))] + [(float(r[0]), r[1:4].copy(), r[4:7].copy()) for r in np.asarray(rows, float).reshape(-1, 7)]


class Worst(dict):
    """worst observed difference per kind of check, relative to max|expected| of the field"""

    def note(self, kind, value):
        self[kind] = max(self.get(kind, 0.0), float(value))


def _close(got, want, where, worst, kind):
    got, want = np.asarray(got, float), np.asarray(want, float)
    scale = max(1e-300, np.abs(want).max())
    d = np.abs(got - want).max()
    worst.note(kind, d / scale)
    assert d <= BOUND * scale, (where, kind, d / scale)


def ref80_of(smp, ba=None, bg=None, noise=R80.NOISE, start=None):
    """(80-bit reference, E64 per kind) of one record: integrated from the identity at ba / bg, or continued from `start`"""
    ref = R80.integrate(smp, ba, bg, noise, start=start)
    e64, table = R80.e64_of(smp, ba, bg, noise, start=start, ref=ref), R80.yardstick()
    return ref, {k: max(e64[k], table[k]) for k in R80.KINDS}


def check_record(got, want, where, worst, kind, ref80=None, sum_dt_exact=True):
    """ref80: what ref80_of returned for the samples `want` was integrated from"""
    assert got is not None, where
    _close([got['sum_dt']], [want['sum_dt']], where + ('sum_dt',), worst, kind)
    for key in REC_FIELDS:
        _close(got[key], want[key], where + (key,), worst, kind)
    if ref80 is not None:
        ref, E64 = ref80
        err = R80.record_error(got, ref)
        assert err['lin_ba'] == 0.0 and err['lin_bg'] == 0.0 and (err['sum_dt'] == 0.0 or not sum_dt_exact), (where, kind, err)
        for key, k in R80.KIND_OF.items():
            worst.note(kind + ', ' + k + ' / E64', err[key] / E64[k])
            assert err[key] <= R80.M * E64[k], (where, kind, key, err[key], E64[k])


def begin(h, srcs, K, min_parallax, max_features=128, max_samples=20, wins=None):
    """seq_begin + seq_imu_begin from the initial windows of `srcs`; returns (windows, sample history of record K-3 per window)."""
    wins = wins if wins is not None else [s.initial_window(K, 0) for s in srcs]
    probs, trks = zip(*[synth.sequence_inputs(w) for w in wins])
    h.seq_begin(list(probs), list(trks), max_features=max_features, max_new_obs=max_features, init_depth=5.0, min_parallax=min_parallax)
    seeds = [seed_of(s, w, K) for s, w in zip(srcs, wins)]
    h.seq_imu_begin(seeds, noise_of(srcs[0].seq), max_samples=max_samples)
    return wins, [list(w['samples'][K - 3]) for w in wins]


def seed_of(src, win, K):
    last = win['samples'][K - 3][-1]                        # the measurement at the newest frame of the window
    return np.concatenate([last[1], last[2], [0.0, 0.0, src.seq.cfg['g_norm']]])


def frame_of(src, g, rows=None):
    ids, obs = src.image(g)
    return dict(samples=rows_of(src.samples(g - 1)) if rows is None else rows, ids=ids, obs=obs)


def step_checked(h, K, frames, hist, noise, g_norm, worst, step=0, allow_numeric=False):
    """One vg_ba_seq_step_imu_async with every check of the module docstring; hist[w]: the samples record K-3 of window w was
    integrated from (updated here).  Returns (states, summaries, info)."""
    n = len(frames)
    before = [h.seq_export(w, K, raw_imu=True)[0] for w in range(n)]
    meas = [h.seq_imu_get(w) for w in range(n)]
    h.seq_step_imu(frames)
    sts, sms = h.seq_states(allow_numeric_failure=allow_numeric)
    info = h.seq_info()
    for w in range(n):
        where = (step, w)
        after = h.seq_export(w, K, raw_imu=True)[0]
        got = h.seq_imu_get(w)
        rows = np.asarray(frames[w]['samples'], float).reshape(-1, 7)
        smp = samples_of(meas[w]['acc_0'], meas[w]['gyr_0'], rows)
        pose0, sb0 = before[w]['pose'][K - 1], before[w]['sb'][K - 1]
        ba_, bg_ = sb0[3:6], sb0[6:9]
        # ---- the guess (Ps / Rs / Vs[WINDOW_SIZE]); the biases are copied unchanged
        pe, se = _propagate(pose0, sb0, smp, g_norm)
        _close(got['pose'], pe, where + ('pose',), worst, 'guess')
        _close(got['sb'], se, where + ('sb',), worst, 'guess')
        assert np.array_equal(got['sb'][3:], sb0[3:]), where
        # ---- acc_0 / gyr_0 become the last sample, g stays
        assert np.array_equal(got['acc_0'], rows[-1, 1:4]) and np.array_equal(got['gyr_0'], rows[-1, 4:7]) and np.array_equal(got['g'], meas[w]['g']), where
        # ---- the record of the new interval: K-3 after a MARGIN_OLD slide, still in the newest slot after MARGIN_SECOND_NEW
        want = synth.preintegrate(smp, ba_, bg_, *noise)
        flag = info[w]['flag']
        fresh = after['imu'][K - 3] if flag == OLD else after['imu'][K - 2]
        check_record(fresh, want, where + ('new',), worst, 'record', ref80_of(smp, ba_, bg_, noise))
        check_record(fresh, h.imu_preintegrate([smp], [(ba_, bg_)], noise)[0], where + ('new, vg_imu_preintegrate',), worst, 'record_vs_vg_imu_preintegrate')
        assert np.array_equal(fresh['lin_ba'], ba_) and np.array_equal(fresh['lin_bg'], bg_), where
        if flag == OLD:
            assert fresh['valid'] == (1 if want['sum_dt'] <= 10.0 else 0), where
            hist[w] = smp
        else:
            # ---- the merge: record K-3 continued with this frame's samples = the integration of the concatenated samples at the
            #      OLDER record's biases
            old = before[w]['imu'][K - 3]
            hist[w] = hist[w] + smp[1:]
            wantm = synth.preintegrate(hist[w], old['lin_ba'], old['lin_bg'], *noise)
            merged = after['imu'][K - 3]
            # (the list's sum_dt starts with whatever the caller's first record held: only the continuation's is exact)
            check_record(merged, wantm, where + ('merged',), worst, 'merged_record', ref80_of(hist[w], old['lin_ba'], old['lin_bg'], noise), sum_dt_exact=False)
            check_record(merged, wantm, where + ('merged, continued',), worst, 'merged_continued', ref80_of(smp, noise=noise, start=old))
            check_record(merged, h.imu_preintegrate([hist[w]], [(old['lin_ba'], old['lin_bg'])], noise)[0], where + ('merged, vg_imu_preintegrate',), worst,
                         'merged_vs_vg_imu_preintegrate')
            assert np.array_equal(merged['lin_ba'], old['lin_ba']) and np.array_equal(merged['lin_bg'], old['lin_bg']), where
            assert merged['valid'] == (1 if (old['valid'] and wantm['sum_dt'] <= 10.0) else 0), where
    return sts, sms, info


def run_parity(h, seeds, K=11, L=70, n_steps=4, min_parallax=0.25, max_features=128, max_samples=20, counts=None, dt=None, noise_seed=600,
               allow_numeric=()):
    """Case 1-3: record and guess parity of every step.  counts[w]: IMU samples per frame of window w (default: the 20 of the synthetic
    interval; else the interval re-sampled, with step dt if given); allow_numeric: windows whose solve may report VG_ERR_NUMERIC.
    Returns (flags[step][window], Worst)."""
    srcs = [synth.FrameSource(synth.SyntheticSequence(s, n_frames=K + n_steps + 1, K=K + n_steps + 1, L=L), noise_seed=noise_seed + s) for s in seeds]
    noise, g_norm = noise_of(srcs[0].seq), srcs[0].seq.cfg['g_norm']
    worst = Worst()
    wins, hist = begin(h, srcs, K, min_parallax, max_features, max_samples)
    flags = []
    try:
        for step in range(n_steps):
            g = K - 1 + step
            frames = []
            for w, s in enumerate(srcs):
                rows = None
                if counts is not None and counts[w] != s.seq.imu_per_frame:
                    rows = resampled(s, g - 1, counts[w], dt)
                frames.append(frame_of(s, g, rows))
            sts, sms, info = step_checked(h, K, frames, hist, noise, g_norm, worst, step, allow_numeric=bool(allow_numeric))
            for w in range(len(srcs)):
                ok = (0, -4) if w in allow_numeric else (0,)
                assert info[w]['status'] in ok and sms[w]['status'] in ok, (step, w, info[w]['status'], sms[w]['status'])
            flags.append([i['flag'] for i in info])
    finally:
        h.seq_end()
    print("device IMU, worst difference / max|expected|:", dict(worst))
    return flags, worst


def resampled(src, f, n, dt=None):
    """n samples from frame f on, of step dt (default: frame_dt / n, the whole interval f -> f + 1)."""
    seq = src.seq
    hh = seq.frame_dt / n if dt is None else dt
    return np.array([np.concatenate([[hh], *seq._imu_sample(seq.times[f] + k * hh)]) for k in range(1, n + 1)], float)


# ---------------------------------------------------------------------------------------------------------------------------
class _Twin:
    """What seq_model.check_step asks of its `host`: here a second, host-fed device sequence."""

    def __init__(self, state, summary, info, prior, trk):
        self.last = dict(state=state, summary=summary, prior=prior, n_landmarks=info['n_landmarks'], n_factors=info['n_factors'])
        self.last_track_num = info['n_tracked']
        self._t = trk

    def tracks(self):
        t = self._t
        rows = np.concatenate([t['obs'][f, :n][:, [0, 1, 7, 2, 3, 4, 5, 6]] for f, n in enumerate(t['nobs'])]) if len(t['id']) else np.zeros((0, 8))
        return dict(id=t['id'], start=t['start'], nobs=t['nobs'], solve_flag=t['solve_flag'], depth=t['depth'], obs=rows)


def run_equivalence(h_imu, h_host, seeds, K=11, L=70, n_steps=4, min_parallax=0.25, max_features=128):
    """Case 4: the same frames to a sequence in IMU mode (h_imu) and to a host-fed one (h_host: records from Handle.imu_preintegrate,
    guesses from _propagate, imu_merged carried as seq_model does).  The first step passes seq_model.check_step at its own tolerances;
    the following steps run free and are held to the bar of tests/test_seq_gpu.py test_resident_sequence_free_running (states 1e-4
    relative, identical flags and surviving tracks).  Returns (flags, worst free-running value)."""
    mk = lambda: [synth.FrameSource(synth.SyntheticSequence(s, n_frames=K + n_steps + 1, K=K + n_steps + 1, L=L), noise_seed=700 + s) for s in seeds]
    sa, sb_ = mk(), mk()
    n = len(seeds)
    noise, g_norm = noise_of(sa[0].seq), sa[0].seq.cfg['g_norm']
    wins, _ = begin(h_imu, sa, K, min_parallax, max_features)
    wins_b = [s.initial_window(K, 0) for s in sb_]
    probs, trks = zip(*[synth.sequence_inputs(w) for w in wins_b])
    h_host.seq_begin(list(probs), list(trks), max_features=max_features, max_new_obs=max_features, init_depth=5.0, min_parallax=min_parallax)
    newest = [(w['pose'][K - 1].copy(), w['sb'][K - 1].copy()) for w in wins_b]
    last = [w['samples'][K - 3][-1] for w in wins_b]                       # acc_0 / gyr_0 of the host-side caller
    prev = [dict(samples=list(w['samples'][K - 3]), ba=s.seq.ba_lin, bg=s.seq.bg_lin) for w, s in zip(wins_b, sb_)]
    merged = [None] * n
    flags, worst = [], 0.0
    try:
        for step in range(n_steps):
            g = K - 1 + step
            fa, fb, cur = [], [], []
            for i in range(n):
                f = frame_of(sa[i], g)
                fa.append(f)
                smp = samples_of(last[i][1], last[i][2], f['samples'])
                ba_, bg_ = newest[i][1][3:6].copy(), newest[i][1][6:9].copy()
                rec = h_host.imu_preintegrate([smp], [(ba_, bg_)], noise)[0]
                pose, sb = _propagate(newest[i][0], newest[i][1], smp, g_norm)
                fb.append(dict(pose=pose, sb=sb, imu_new=rec, imu_merged=merged[i], ids=f['ids'], obs=f['obs']))
                cur.append(dict(samples=smp, ba=ba_, bg=bg_))
            h_imu.seq_step_imu(fa)
            h_host.seq_step(fb)
            da, ma = h_imu.seq_states()
            db, mb = h_host.seq_states()
            ia, ib = h_imu.seq_info(), h_host.seq_info()
            pa, pb = (h_imu.seq_priors(), h_host.seq_priors()) if step == 0 else ([None] * n, [None] * n)
            for i in range(n):
                ta, tb = h_imu.seq_tracks(i, K), h_host.seq_tracks(i, K)
                if step == 0:
                    M.check_step(step, i, _Twin(db[i], mb[i], ib[i], pb[i], tb), ib[i]['flag'], dict(state=da[i], summary=ma[i], info=ia[i], prior=pa[i], tracks=ta))
                assert ia[i]['status'] == 0 and ib[i]['status'] == 0 and ia[i]['flag'] == ib[i]['flag'], (step, i)
                for k in ('pose', 'sb'):
                    e = np.abs(da[i][k] - db[i][k]).max() / max(1.0, np.abs(db[i][k]).max())
                    worst = max(worst, e)
                    assert e < 1e-4, (step, i, k, e)
                assert np.array_equal(ta['id'], tb['id']) and np.array_equal(ta['start'], tb['start']) and np.array_equal(ta['nobs'], tb['nobs']), (step, i)
                # the host-side caller's bookkeeping (seq_model.drive_sequence)
                newest[i] = (db[i]['pose'][K - 1].copy(), db[i]['sb'][K - 1].copy())
                last[i] = cur[i]['samples'][-1]
                if ib[i]['flag'] == NEW:
                    prev[i]['samples'] = prev[i]['samples'] + cur[i]['samples'][1:]
                    merged[i] = h_host.imu_preintegrate([prev[i]['samples']], [(prev[i]['ba'], prev[i]['bg'])], noise)[0]
                else:
                    prev[i], merged[i] = cur[i], None
            flags.append([x['flag'] for x in ia])
    finally:
        h_imu.seq_end()
        h_host.seq_end()
    print("device IMU vs host-fed sequence, free-running: worst relative state difference", worst)
    return flags, worst


# ---------------------------------------------------------------------------------------------------------------------------
def run_against_reference(h, min_parallax, n_frames=24):
    """Case 5: seq_model.run_against_reference with the sequence in IMU mode: the reference's OWN processIMU / processImage loop
    (oracle/_ref) against a device that gets nothing but raw samples and observations.  Same frames, same bars."""
    from oracle import ref as R
    K = 11
    ref = R.run_sequence(synth.SyntheticSequence(11, n_frames=26, K=26, L=500), n_frames, L=R.lib(), min_parallax=min_parallax)
    seq = synth.SyntheticSequence(11, n_frames=26, K=26, L=500)
    src = synth.FrameSource(seq, noise_seed=0)
    rng = np.random.default_rng(0)                                  # the draws of R.run_sequence, in its order

    def noisy_state(f):
        th = rng.normal(0, np.radians(0.3), 3)
        Rn = seq.Rm[f] @ (np.eye(3) + np.array([[0, -th[2], th[1]], [th[2], 0, -th[0]], [-th[1], th[0], 0]]))
        q = R.quat_from_R(Rn)
        return np.concatenate([seq.P[f] + rng.normal(0, 0.03, 3), q / np.linalg.norm(q)]), np.concatenate([seq.V[f] + rng.normal(0, 0.03, 3), seq.ba_lin, seq.bg_lin])

    win = src.initial_window(K, 0)
    states = [noisy_state(i) for i in range(K - 1)] + [noisy_state(K - 2)]
    win['pose'], win['sb'] = np.array([s[0] for s in states]), np.array([s[1] for s in states])
    # (slot K-1 of `win` is the reference's second draw for frame K-2; the device starts from a copy of slot K-2, as slideWindow leaves
    #  it -- so slot K-2 takes that draw: the reference propagates from set_frame(K - 1, ...) too)
    win['pose'][K - 2], win['sb'][K - 2] = win['pose'][K - 1].copy(), win['sb'][K - 1].copy()
    begin(h, [src], K, min_parallax, max_features=512, max_samples=seq.imu_per_frame, wins=[win])
    got = []
    try:
        for f in range(K - 1, n_frames):
            h.seq_step_imu([frame_of(src, f)])
            (st,), (sm,) = h.seq_states()
            (info,) = h.seq_info()
            trk = h.seq_tracks(0, K)
            assert info['status'] == 0
            order = list(range(1, K)) + [K - 1] if info['flag'] == OLD else list(range(K - 2)) + [K - 1, K - 1]
            got.append(dict(frame=f, flag=info['flag'], pose=st['pose'][order], sb=st['sb'][order], ids=set(trk['id'].tolist()), n=info['n_after'],
                            iters=sm['num_iterations'], flags=list(sm['it_flags'])))
    finally:
        h.seq_end()
    assert len(ref) == len(got)
    flags = [r['flag'] for r in ref]
    loose, n_flips, worst = 0, 0, 0.0
    for r, g in zip(ref, got):
        assert r['frame'] == g['frame'] and r['solver_flag'] == 1
        assert r['flag'] == g['flag'], r['frame']                                       # same key-frame decision
        assert r['n_features'] == g['n'] and set(r['depth']) == g['ids'], r['frame']    # same tracks survive
        same = r['trace'].shape[0] == g['iters'] and np.array_equal(r['trace'][:, 1].astype(int), (np.array(g['flags'][:g['iters']], int) >> 1) & 1)
        if not same:
            n_flips += 1
            loose = 3
        tol = 2e-3 if loose > 0 else 1e-4
        loose = max(0, loose - 1)
        e = max(np.abs(g['pose'][:, :3] - r['pose'][:, :3]).max() / max(1.0, np.abs(r['pose'][:, :3]).max()), np.abs(g['pose'][:, 3:] - r['pose'][:, 3:]).max(),
                np.abs(g['sb'][:, :3] - r['sb'][:, :3]).max() / max(1.0, np.abs(r['sb'][:, :3]).max()), np.abs(g['sb'][:, 3:] - r['sb'][:, 3:]).max())
        worst = max(worst, e)
        assert e < tol, (r['frame'], e, same, np.abs(g['pose'] - r['pose']).max(axis=1), np.abs(g['sb'] - r['sb']).max(axis=1))
    assert n_flips <= max(1, len(ref) // 4)
    print("device-IMU sequence vs the reference's loop: worst state difference", worst, "trust-region flips", n_flips)
    return flags, worst, n_flips


# ---------------------------------------------------------------------------------------------------------------------------
def run_long_interval(h, K=11, L=70):
    """Case 6: 21 samples of 0.5 s: the record is kept with valid == 0 and meets the record bound; the next ordinary frame is accepted."""
    src = synth.FrameSource(synth.SyntheticSequence(21, n_frames=K + 3, K=K + 3, L=L), noise_seed=621)
    noise, g_norm = noise_of(src.seq), src.seq.cfg['g_norm']
    worst = Worst()
    wins, hist = begin(h, [src], K, 10.0 / 460.0, 128, 32)
    try:
        rows = rows_of(src.samples(K - 2))
        rows = np.vstack([rows, rows[:1]])                         # 21 samples
        rows[:, 0] = 0.5
        sts, sms, info = step_checked(h, K, [frame_of(src, K - 1, rows)], hist, noise, g_norm, worst, 0, allow_numeric=True)
        assert sms[0]['status'] in (0, -4) and info[0]['status'] in (0, -4)
        exp = h.seq_export(0, K, raw_imu=True)[0]
        k = K - 3 if info[0]['flag'] == OLD else K - 2
        assert exp['imu'][k]['valid'] == 0 and exp['imu'][k]['sum_dt'] > 10.0
        h.seq_step_imu([frame_of(src, K)])                         # accepted (what it solves from is the caller's business: see reseed)
        h.seq_states(allow_numeric_failure=True)
    finally:
        h.seq_end()
    print("device IMU, interval of 10.5 s, worst difference / max|expected|:", dict(worst))
    return worst


def run_import(h_a, h_b, seeds, K=11, L=70, n_before=2, min_parallax=0.25):
    """Case 7: two sequences in IMU mode; after n_before frames on h_a its windows are exported and imported (+ seq_imu_set) into
    h_b, whose slots held somebody else's windows; one more frame on both: states, summaries and exported records are equal bit
    for bit (the pattern of seq_model.run_handback)."""
    n = len(seeds)
    mk = lambda off: [synth.FrameSource(synth.SyntheticSequence(s + off, n_frames=K + n_before + 2, K=K + n_before + 2, L=L), noise_seed=800 + s) for s in seeds]
    sa, sother = mk(0), mk(7)
    begin(h_a, sa, K, min_parallax, 256)
    begin(h_b, sother, K, min_parallax, 256)
    try:
        for g in range(K - 1, K - 1 + n_before):
            h_a.seq_step_imu([frame_of(s, g) for s in sa])
            h_a.seq_states()
            h_b.seq_step_imu([frame_of(s, g) for s in sother])
            h_b.seq_states()
        base = sa[0].seq._base()
        for w in range(n):
            e, trk = h_a.seq_export(w, K)
            p = dict(base)
            p.update(pose=e['pose'], sb=e['sb'], ex=e['ex'], td=e['td'], imu=e['imu'], prior=e['prior'], relo=None, lm_start=np.zeros(0, np.int32),
                     lm_nobs=np.zeros(0, np.int32), obs_off=np.zeros(0, np.int32), obs=np.zeros((0, 7)), inv_depth=np.zeros(0))
            h_b.seq_import(w, p, trk)
            m = h_a.seq_imu_get(w)
            h_b.seq_imu_set(w, np.concatenate([m['acc_0'], m['gyr_0'], m['g']]))
        g = K - 1 + n_before
        fr = [frame_of(s, g) for s in sa]
        h_a.seq_step_imu(fr)
        h_b.seq_step_imu(fr)
        ra, rb = h_a.seq_states(), h_b.seq_states()
        ia, ib = h_a.seq_info(), h_b.seq_info()
        for w in range(n):
            for key in ('pose', 'sb', 'ex'):
                assert np.array_equal(ra[0][w][key], rb[0][w][key]), (w, key, np.abs(ra[0][w][key] - rb[0][w][key]).max())
            assert ra[1][w]['final_cost'] == rb[1][w]['final_cost'] and ra[1][w]['num_iterations'] == rb[1][w]['num_iterations']
            assert np.array_equal(ra[1][w]['it_flags'], rb[1][w]['it_flags']) and ia[w] == ib[w]
            ea, eb = h_a.seq_export(w, K, raw_imu=True)[0], h_b.seq_export(w, K, raw_imu=True)[0]
            for k in range(K - 2):
                assert ea['imu'][k]['valid'] == eb['imu'][k]['valid'], (w, k)
                for key in ('sum_dt', 'lin_ba', 'lin_bg') + REC_FIELDS:
                    assert np.array_equal(ea['imu'][k][key], eb['imu'][k][key]), (w, k, key)
            ma, mb = h_a.seq_imu_get(w), h_b.seq_imu_get(w)
            for key in ma:
                assert np.array_equal(ma[key], mb[key]), (w, key)
        return [x['flag'] for x in ia]
    finally:
        h_a.seq_end()
        h_b.seq_end()


def run_refusals(h, K=11, L=40):
    """Case 8: every refusal raises with a message (VG_ERR_BAD_ARG, nothing uploaded), and a correct step afterwards succeeds."""
    import pytest
    src = synth.FrameSource(synth.SyntheticSequence(21, n_frames=K + 3, K=K + 3, L=L), noise_seed=1)
    win = src.initial_window(K, 0)
    prob, tracks = synth.sequence_inputs(win)
    noise = noise_of(src.seq)
    seed = seed_of(src, win, K)
    h.seq_begin([prob], [tracks], max_features=128, max_new_obs=128)
    try:
        good = frame_of(src, K - 1)
        with pytest.raises(RuntimeError, match="status -1.*vg_ba_seq_imu_begin has not been called"):
            h.seq_step_imu([good])
        for ms in (0, 513):
            with pytest.raises(RuntimeError, match="status -1.*max_samples outside"):
                h.seq_imu_begin([seed], noise, max_samples=ms)
        with pytest.raises(RuntimeError, match="status -1.*struct_size"):
            h.seq_imu_begin([seed], noise, max_samples=20, struct_size=8)
        with pytest.raises(RuntimeError, match="status -1.*that many windows"):
            h.seq_imu_begin([seed, seed], noise, max_samples=20)
        h.seq_imu_begin([seed], noise, max_samples=20)
        bad = dict(good, samples=None, n_samples=0)
        with pytest.raises(RuntimeError, match="status -1.*at least one IMU sample"):
            h.seq_step_imu([bad])
        with pytest.raises(RuntimeError, match="status -1.*at least one IMU sample"):
            h.seq_step_imu([dict(good, samples=None, n_samples=5)])                       # NULL samples
        with pytest.raises(RuntimeError, match="status -1.*more samples than"):
            h.seq_step_imu([dict(good, samples=np.vstack([good['samples'], good['samples'][:1]]))])
        for poison in (np.nan, np.inf):
            rows = good['samples'].copy()
            rows[3, 5] = poison
            with pytest.raises(RuntimeError, match="status -1.*not finite"):
                h.seq_step_imu([dict(good, samples=rows)])
        with pytest.raises(RuntimeError, match="status -1.*that many windows"):
            h.seq_step_imu([good, good])
        with pytest.raises(RuntimeError, match="status -1.*strictly ascending"):
            h.seq_step_imu([dict(good, ids=good['ids'][::-1].copy(), obs=good['obs'][::-1].copy())])
        pose, sb = src.guess(K - 1)
        with pytest.raises(RuntimeError, match="status -1.*takes raw IMU samples"):
            h.seq_step([dict(pose=pose, sb=sb, imu_new=src.seq.imu[K - 2], imu_merged=None, ids=good['ids'], obs=good['obs'])])
        h.seq_step_imu([good])                                     # the sequence is still usable
        h.seq_states()
        assert h.seq_info()[0]['status'] == 0
    finally:
        h.seq_end()
    # vg_ba_seq_end drops the IMU state: the next sequence on the handle is host-fed again
    h.seq_begin([prob], [tracks], max_features=128, max_new_obs=128)
    try:
        with pytest.raises(RuntimeError, match="vg_ba_seq_imu_begin has not been called"):
            h.seq_step_imu([good])
    finally:
        h.seq_end()


def run_timing_tap(h, K=11, L=40, positive=True):
    """vg_ba_seq_imu_timing / _times: refused unless the last step was timed; two finite device times (positive on a device with a
    clock) after a timed step; the timed step computes what an untimed one does."""
    import pytest
    states = []
    for timed in (False, True):
        src = synth.FrameSource(synth.SyntheticSequence(21, n_frames=K + 3, K=K + 3, L=L), noise_seed=3)      # (same draws both times)
        begin(h, [src], K, 0.25, 128, 20)
        try:
            with pytest.raises(RuntimeError, match="status -1.*not timed"):
                h.seq_imu_times()
            h.seq_imu_timing(timed)
            for g in (K - 1, K):
                h.seq_step_imu([frame_of(src, g)])
                states.append(h.seq_states()[0][0])
                if timed:
                    a, b = h.seq_imu_times()
                    assert np.isfinite(a) and np.isfinite(b) and a >= 0 and b >= 0 and (not positive or (a > 0 and b > 0)), (a, b)
            if timed:
                h.seq_imu_timing(False)
                with pytest.raises(RuntimeError, match="not timed"):
                    h.seq_imu_times()
        finally:
            h.seq_end()
    for x, y in zip(states[:2], states[2:]):
        assert np.array_equal(x['pose'], y['pose']) and np.array_equal(x['sb'], y['sb'])


def run_cpp(exe, tmp_path, timeout, K=11, n_frames=3, min_parallax=0.25):
    """Case 10: `vins_replay seq` on one write_seq_file input without and with VINS_REPLAY_DEVICE_IMU=1, and once more with the IMU on
    the device AND a hand-back in the middle (VINS_REPLAY_HANDBACK: handBack, handOver + begin, reseed = vg_ba_seq_import +
    vg_ba_seq_imu_set): the comparison of test_cpp_hand_back_and_take_over_again (tests/test_seq_simt.py).  The tool reports which side
    ran processIMU ("M,host" / "M,device" on stderr) and, from vg_ba_seq_imu_get, how far the measurement resident on the device is
    from the last sample the host handed on ("A,<estimator>,<difference>"): only a sequence in IMU mode answers that.
    Returns the worst state difference."""
    import os
    import subprocess
    srcs = [M.FrameSource(synth.SyntheticSequence(s, n_frames=K + n_frames + 1, K=K + n_frames + 1, L=70), noise_seed=200 + s) for s in (21, 22)]
    M.write_seq_file(tmp_path / "frames.bin", srcs, K, n_frames, min_parallax=min_parallax)
    outs = {}
    for tag, env, mode in (("host", {}, "host"), ("device", {"VINS_REPLAY_DEVICE_IMU": "1"}, "device"),
                           ("device_handback", {"VINS_REPLAY_DEVICE_IMU": "1", "VINS_REPLAY_HANDBACK": "0"}, "device")):
        out = tmp_path / f"{tag}.csv"
        r = subprocess.run([exe, "seq", str(tmp_path / "frames.bin"), str(out)], capture_output=True, text=True, timeout=timeout, env=dict(os.environ, **env))
        assert r.returncode == 0, r.stderr[-2000:]
        marks = [l.split(',') for l in r.stderr.splitlines() if l[:2] in ("M,", "A,")]
        assert [m[1] for m in marks if m[0] == "M"] == [mode], (tag, r.stderr[-500:])
        resident = [m for m in marks if m[0] == "A"]
        if mode == "device":
            assert [int(m[1]) for m in resident] == list(range(len(srcs))) and all(float(m[2]) == 0.0 for m in resident), (tag, resident)
        else:
            assert not resident, (tag, resident)
        outs[tag] = [l.split(',') for l in open(out).read().strip().splitlines()]
    a = outs["host"]
    assert len(a) == len(srcs) * n_frames
    flags = [int(l[12]) for l in a]
    assert 0 in flags and 1 in flags                                # (Estimator::MARGIN_OLD = 0, MARGIN_SECOND_NEW = 1)
    worst = 0.0
    for tag in ("device", "device_handback"):
        b = outs[tag]
        assert len(b) == len(a), tag
        for la, lb in zip(a, b):
            assert la[0] == lb[0] and la[12:] == lb[12:], tag       # same estimator, same key-frame decision, tracks, status, no failure
            worst = max(worst, max(abs(float(x) - float(y)) for x, y in zip(la[2:12], lb[2:12])))
    assert worst < 1e-6, worst
    return worst
