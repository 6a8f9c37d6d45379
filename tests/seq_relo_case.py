"""TEST INFRASTRUCTURE: relocalisation frames of a resident sequence (vg_ba_seq_relo_reserve / vg_ba_seq_set_relo / vg_ba_seq_get_relo).
The driver of tests/seq_model.py (`run_both`: the reference's bookkeeping restated on the host + vg_ba_optimize per frame on a second
handle, teacher mode included) with windows armed at chosen steps: the host model's problem of such a frame gets `prob['relo']`
from a NumPy restatement of the reference's cursor walk (estimator.cpp:776-799) and goes through vg_ba_optimize, the sequence gets
the match list keyed by feature id and selects the factors on the device."""
import numpy as np

import seq_model as M
from oracle import ba_numpy as B
from oracle.window_numpy import q2R
from vins_mono_amd import synth

SENTINEL = 10 ** 9      # what the reference reads past the end of match_points (oracle/ref_stubs/ref_driver.cpp: an id no feature has)


def walk(lm_id, lm_start, frame, match_id):
    """estimator.cpp:776-799: [(landmark index, match index)] in landmark order.  Reading past the end means no more matches."""
    mid = [int(v) for v in match_id] + [SENTINEL]
    out, cur = [], 0
    for l, (fid, st) in enumerate(zip(lm_id, lm_start)):
        if st > frame:
            continue
        while mid[cur] < fid:
            cur += 1
        if mid[cur] == fid:
            out.append((l, cur))
            cur += 1
    return out


def ascending(win):
    """prepare= of run(): the track list in ascending feature id, as in the running system (ids are handed out in arrival order and
    new tracks join the list at its end); the synthetic windows come sorted by start frame"""
    win.features.sort(key=lambda ft: ft['id'])


def problem_ids(win):
    """feature ids of the landmarks of win.problem(), in its order"""
    return [ft['id'] for ft in win.features if win.in_problem(ft)]


def project_matches(prob, relo_pose, landmarks):
    """The matched point of landmark l seen from the loop frame (as ba_step_ref.add_relocalisation builds it)."""
    ric, tic = q2R(prob['ex'][3:]), prob['ex'][:3]
    Rr, Pr = B.q2R(relo_pose[3:]), relo_pose[:3]
    xy = []
    for l in landmarks:
        s = int(prob['lm_start'][l])
        o = prob['obs'][int(prob['obs_off'][l])]
        pc = np.array([o[0], o[1], 1.0]) / prob['inv_depth'][l]
        Xw = B.q2R(prob['pose'][s][3:]) @ (ric @ pc + tic) + prob['pose'][s][:3]
        p = ric.T @ (Rr.T @ (Xw - Pr) - tic)
        xy.append((p[0] / p[2], p[1] / p[2]))
    return xy


def standard_request(win, prob, frame=3, n_eligible=8, given_pose=True, offset=(0.05, -0.03, 0.02)):
    """A relocalisation request keyed by feature id: matches for `n_eligible` landmarks anchored at or before `frame` (every other one of
    three of them, so that the cursor passes eligible landmarks without a match), plus ids that are not in the window, ids of tracks outside the
    problem and ids of landmarks anchored behind the loop frame.  About 12 matches."""
    ids = problem_ids(win)
    relo_pose = prob['pose'][frame].copy()
    relo_pose[:3] += offset
    elig = [l for k, l in enumerate(l for l in range(len(ids)) if prob['lm_start'][l] <= frame) if k % 3 != 1][:n_eligible]
    late = [l for l in range(len(ids)) if prob['lm_start'][l] > frame][:2]
    outside = [ft['id'] for ft in win.features if not win.in_problem(ft)][:2]
    known = {ft['id'] for ft in win.features}
    absent = [v for v in (1, max(known) // 2, max(known) + 7) if v not in known][:2]
    entries = {ids[l]: xy for l, xy in zip(elig, project_matches(prob, relo_pose, elig))}
    for k, fid in enumerate([ids[l] for l in late] + outside + absent):
        entries[fid] = (0.01 * (k + 1), -0.02 * (k + 1))
    order = sorted(entries)
    th = np.radians(7.0)
    return dict(frame=frame, pose=relo_pose if given_pose else None, match_id=np.array(order, np.int32), match_xy=np.array([entries[i] for i in order], float),
                prev_t=np.array([0.3, -0.2, 0.1]), prev_r=np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1.0]]),
                expect=dict(eligible=len(elig), late=len(late), outside=len(outside), absent=len(absent)))


def host_relo(win, prob, req):
    """prob['relo'] of the host model for request `req` (None when the walk selects nothing) and the factor list of the walk."""
    sel = walk(problem_ids(win), prob['lm_start'], req['frame'], req['match_id'])
    pose = prob['pose'][req['frame']].copy() if req.get('pose') is None else np.asarray(req['pose'], float)
    relo = dict(pose=pose, match=[(l, float(req['match_xy'][m][0]), float(req['match_xy'][m][1])) for l, m in sel]) if sel else None
    return relo, sel, pose


def gauge_carried(pose, summary, state):
    """relo_Pose of a request without factors after double2vector (estimator.cpp:602-605): through the gauge transform of the solve,
    (relo_t, relo_r); origin_P0 is the solved position of frame 0"""
    rot, p0 = summary['gauge_rot'], summary['gauge_p0']
    return rot @ (pose[:3] - p0) + state['pose'][0][:3], rot @ q2R(pose[3:])


def by_products(state, relo_pose, req):
    """double2vector (estimator.cpp:598-612) in NumPy from downloaded states: Utility::R2ypr / ypr2R / normalizeAngle, degrees"""
    def R2ypr(R):
        y = np.arctan2(R[1, 0], R[0, 0])
        p = np.arctan2(-R[2, 0], R[0, 0] * np.cos(y) + R[1, 0] * np.sin(y))
        r = np.arctan2(R[0, 2] * np.sin(y) - R[1, 2] * np.cos(y), -R[0, 1] * np.sin(y) + R[1, 1] * np.cos(y))
        return np.array([y, p, r]) / np.pi * 180.0

    def norm_angle(a):
        return a - 360.0 * np.floor((a + 180.0) / 360.0) if a > 0 else a + 360.0 * np.floor((-a + 180.0) / 360.0)
    f = req['frame']
    relo_r, relo_t = q2R(relo_pose[3:]), relo_pose[:3]
    Rf, Pf = q2R(state['pose'][f][3:]), state['pose'][f][:3]
    yaw = (R2ypr(np.asarray(req['prev_r']))[0] - R2ypr(relo_r)[0]) / 180.0 * np.pi
    dr = np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1.0]])
    rel = relo_r.T @ Rf
    return dict(drift_r=dr, drift_t=np.asarray(req['prev_t']) - dr @ relo_t, relative_t=relo_r.T @ (Pf - relo_t), relative_R=rel,
                relative_yaw=norm_angle(R2ypr(Rf)[0] - R2ypr(relo_r)[0]))


def same_rotation(q_xyzw, R):
    return np.abs(q2R(q_xyzw) - R).max()


def run(h_seq, h_ref, seeds, arm, K=11, L=40, n_steps=3, max_match=16, min_parallax=10.0 / 460.0, max_features=128, max_factors=0, max_landmarks=0,
        estimate_td=0, check=None, teacher=True, prepare=None, reserve=True, between=None):
    """seq_model.run_both with relocalisation frames.  arm: {(step, window): fn(win, prob) -> request dict}: the window is armed for
    that step.  check(step, w, host window, flag, dev): dev carries 'relo' (vg_ba_seq_get_relo), host.last carries 'relo' (the request,
    the walk's selection `sel`, the input pose, the state's relo_pose of vg_ba_optimize or None).  between(step): called before the
    sequence's step, after the windows are armed (refusal and lifetime cases).  Returns (flags, per step and window dev records)."""
    nwin = len(seeds)
    seqs = [synth.SyntheticSequence(s, n_frames=K + n_steps + 1, K=K + n_steps + 1, L=L, estimate_td=estimate_td) for s in seeds]
    src = [M.FrameSource(q, noise_seed=100 + i) for i, q in enumerate(seqs)]
    hw = [s.initial_host_window(K, 0, 5.0, min_parallax) for s in src]
    if prepare is not None:
        for w_ in hw:
            prepare(w_)
    wins, trks = zip(*[M.window_inputs(w) for w in hw])
    if reserve:
        h_seq.seq_relo_reserve(max_match)
    h_seq.seq_begin(list(wins), list(trks), max_features=max_features, max_new_obs=max_features, max_landmarks=max_landmarks, max_factors=max_factors,
                    init_depth=5.0, min_parallax=min_parallax)
    pending_merge = [None] * nwin
    flags_all, seen = [], []
    try:
        for step in range(n_steps):
            g = K - 1 + step
            frames, flags = [], []
            for w in range(nwin):
                s, win = src[w], hw[w]
                ids, rows = s.image(g)
                pose, sb = s.guess(g)
                smp = s.samples(g - 1)
                rec = s.preintegrate(smp, win.sb[K - 1][3:6], win.sb[K - 1][6:9])
                frames.append(dict(pose=pose, sb=sb, imu_new=rec, imu_merged=pending_merge[w], ids=ids, obs=rows))
                win.pose[K - 1], win.sb[K - 1] = pose, sb
                win.imu[K - 2], win.samples[K - 2] = rec, smp
                flag = win.add_frame(ids, rows)
                win.triangulate(h_ref)
                prob = win.problem()
                relo_rec = None
                if (step, w) in arm:
                    req = arm[(step, w)](win, prob)
                    prob['relo'], sel, pose_in = host_relo(win, prob, req)
                    h_seq.seq_set_relo(w, req)
                    relo_rec = dict(req=req, sel=sel, pose_in=pose_in)
                st, sm, prior = h_ref.ba_optimize(prob, flag)
                if relo_rec is not None:
                    relo_rec['pose'] = st.get('relo_pose')
                    relo_rec['prob'] = prob
                flags.append(flag)
                n_relo = len(relo_rec['sel']) if relo_rec else 0
                win.last = dict(state=st, summary=sm, prior=prior, n_landmarks=len(prob['inv_depth']), n_factors=int((prob['lm_nobs'] - 1).sum()) + n_relo,
                                relo=relo_rec)
            if between is not None:
                between(step)
            h_seq.seq_step(frames)
            dst, dsm = h_seq.seq_states()
            info = h_seq.seq_info()
            pri = h_seq.seq_priors()
            row = []
            for w in range(nwin):
                s, win = src[w], hw[w]
                merged = {}

                def merge(samples, old, s=s, merged=merged):
                    merged['rec'] = s.preintegrate(samples, old['lin_ba'], old['lin_bg'])
                    return merged['rec']
                if teacher and info[w]['flag'] == flags[w] and info[w]['n_landmarks'] == win.last['n_landmarks']:
                    adv = dict(dst[w])
                    adv['inv_depth'] = dst[w]['inv_depth'][:info[w]['n_landmarks']]
                    win.after_solve(adv, pri[w], flags[w], merge)
                else:
                    win.after_solve(win.last['state'], win.last['prior'], flags[w], merge)
                pending_merge[w] = merged.get('rec')
                dev = dict(state=dst[w], summary=dsm[w], info=info[w], prior=pri[w], tracks=h_seq.seq_tracks(w, K),
                           relo=h_seq.seq_get_relo(w) if reserve else None)
                row.append(dev)
                if check:
                    check(step, w, win, flags[w], dev)
            flags_all.append(flags)
            seen.append(row)
    finally:
        h_seq.seq_end()
    return flags_all, seen


def check_relo(step, w, host, dev, tol=1e-9):
    """The loop pose and the factor count of an armed step against vg_ba_optimize with the walk's factors; an idle step reports so."""
    rec, got = host.last['relo'], dev['relo']
    where = f"step {step} window {w}"
    assert np.isfinite(got['pose']).all() and np.isfinite(dev['state']['relo_pose']).all(), where
    assert np.array_equal(got['pose'], dev['state']['relo_pose']), where       # (vg_ba_state::relo_pose is the same download)
    if rec is None:
        assert got['armed'] == 0 and got['n_factors'] == 0, where
        return None
    assert got['armed'] == 1 and got['frame'] == rec['req']['frame'], where
    assert got['n_factors'] == len(rec['sel']), (where, got['n_factors'], len(rec['sel']))
    if rec['sel']:
        e = np.abs(got['pose'] - rec['pose']).max() / max(1.0, np.abs(rec['pose']).max())
        assert e <= tol, (where, 'loop pose', e)
        return e
    return 0.0


# ---------------------------------------------------------------------------------------------------------------- the cases
def _full_check(worst):
    def check(step, w, host, flag, dev):
        M.check_step(step, w, host, flag, dev)
        e = check_relo(step, w, host, dev)
        if e is not None:
            worst['loop_pose'] = max(worst.get('loop_pose', 0.0), e)
    return check


def check_by_products(dev, req, tol=1e-12):
    """vg_ba_seq_get_relo's by-products against the same formulas in NumPy from the downloaded states (issue case 6)."""
    got, want = dev['relo'], by_products(dev['state'], dev['relo']['pose'], req)
    errs = dict(relative_t=np.abs(got['relative_t'] - want['relative_t']).max(), relative_q=same_rotation(got['relative_q'], want['relative_R']),
                relative_yaw=abs(got['relative_yaw'] - want['relative_yaw']), drift_r=np.abs(got['drift_r'] - want['drift_r']).max(),
                drift_t=np.abs(got['drift_t'] - want['drift_t']).max())
    for k, e in errs.items():
        assert e <= tol, (k, e)
    return max(errs.values())


def case_host_bookkeeping(h_seq, h_ref, K=11, estimate_td=0, seeds=(22, 23), with_reference=False):
    """Issue cases 1, 2 and 6: 2 windows, L = 40, 3 steps; window 0 armed at step 1 with frame 3 and about 12 matches (ids outside the
    window, ids of tracks outside the problem and of landmarks anchored behind the loop frame among them), window 1 never armed.  Every
    step passes seq_model.check_step; loop pose to 1e-9, equal n_factors; step 2 (idle again) equals the host model without relo.
    The seeds: windows whose oldest frame anchors tracks.  Where it anchors none (seed 21), the first marginalization removes 15
    states that 15 IMU residuals alone connect to the rest: the new prior is zero in exact arithmetic, rounding noise of 1e-17 .. 1e-7
    in either run, and check_step's comparison of the two priors RELATIVE TO THEIR LARGEST ENTRY compares noise with noise (it passes
    between two runs of one layout only because those agree bit for bit)."""
    worst, armed = {}, {}
    base = _full_check(worst)

    def check(step, w, host, flag, dev):
        base(step, w, host, flag, dev)
        if host.last['relo'] is not None:
            armed[(step, w)] = (host.last['relo'], dev)

    run(h_seq, h_ref, list(seeds), {(1, 0): lambda win, prob: standard_request(win, prob, frame=3)}, K=K, L=40, n_steps=3, estimate_td=estimate_td,
        check=check, prepare=ascending)
    assert list(armed) == [(1, 0)]
    rec, dev = armed[(1, 0)]
    ex = rec['req']['expect']
    assert ex['late'] >= 1 and ex['outside'] >= 1 and ex['absent'] >= 1 and 4 <= len(rec['sel']) < ex['eligible'] + ex['late'] + ex['outside'] + ex['absent']
    assert len(rec['sel']) == ex['eligible']                     # (ascending list: set membership among the eligible landmarks)
    worst['by_products'] = check_by_products(dev, rec['req'])
    if with_reference:
        worst['reference'] = against_reference(rec, dev)
    print("relocalisation frame against host bookkeeping + vg_ba_optimize:", worst)
    return worst


def against_reference(rec, dev, bar=1e-4):
    """The armed step against the reference's own optimization() of that window (oracle/_ref), at the project's parity bar: 1e-4
    relative while the accept / reject traces agree.  The reference leaves relo_Pose itself un-fixed; its gauge-fixed position is
    recovered from its by-products: relo_t = drift_correct_r^T (prev_relo_t - drift_correct_t).
    Measured (MI355X and emulator alike): relative_t 4.5e-13, relative_yaw 1.5e-11, drift_t 4.4e-13, loop position 4.1e-13."""
    from oracle import ref as Rf
    prob, req = dict(rec['prob']), rec['req']
    prob['relo'] = dict(prob['relo'], local_index=req['frame'], prev_t=req['prev_t'], prev_r=req['prev_r'])
    st, trace, _ = Rf.optimization(prob, dev['info']['flag'])
    n = dev['summary']['num_iterations']
    flags = [(1 if it['valid'] else 0) | (2 if it['accepted'] else 0) for it in trace['iterations']]
    assert flags == [int(v) for v in dev['summary']['it_flags'][:n]], ("trust-region decisions differ", flags, dev['summary']['it_flags'][:n])
    got = dev['relo']
    ref_t = st['drift_correct_r'].T @ (req['prev_t'] - st['drift_correct_t'])
    errs = dict(relative_t=np.abs(got['relative_t'] - st['relo_relative_t']).max() / max(1.0, np.abs(st['relo_relative_t']).max()),
                relative_yaw=abs(got['relative_yaw'] - st['relo_relative_yaw']) / max(1.0, abs(st['relo_relative_yaw'])),
                drift_t=np.abs(got['drift_t'] - st['drift_correct_t']).max() / max(1.0, np.abs(st['drift_correct_t']).max()),
                loop_t=np.abs(got['pose'][:3] - ref_t).max() / max(1.0, np.abs(ref_t).max()))
    print("relocalisation by-products against the reference's optimization():", errs)
    for k, e in errs.items():
        assert e <= bar, (k, e)
    return max(errs.values())


def case_walk(h_seq, h_ref, kind):
    """Issue case 3: the factor list of the NumPy walk, exactly (n_factors; the factor tables through the states, which follow
    vg_ba_optimize fed with the walk's list to check_step's bounds)."""
    worst, seen = {}, {}
    base = _full_check(worst)

    def request(win, prob):
        ids = problem_ids(win)
        elig = [l for l in range(len(ids)) if prob['lm_start'][l] <= 3]
        req = standard_request(win, prob, frame=3, n_eligible=len(elig), given_pose=(kind != 'not_ascending'))
        if kind == 'not_ascending':                             # every eligible landmark has a match: what is skipped is skipped by the walk
            pose = prob['pose'][3].copy()
            order = sorted(range(len(elig)), key=lambda k: ids[elig[k]])
            xy = project_matches(prob, pose, elig)
            req.update(match_id=np.array([ids[elig[k]] for k in order], np.int32), match_xy=np.array([xy[k] for k in order], float))
        else:
            lo, hi = min(ids[l] for l in elig), max(ids[l] for l in elig)
            pick = dict(all_below=[lo - 9, lo - 4, lo - 1], all_above=[hi + 1, hi + 5, hi + 11], none=[i + 1 for i in (lo, hi) if i + 1 not in ids][:1] or [hi + 1])[kind]
            req.update(match_id=np.array(pick, np.int32), match_xy=np.full((len(pick), 2), 0.1))
        seen['elig'] = [ids[l] for l in elig]
        return req

    def check(step, w, host, flag, dev):
        base(step, w, host, flag, dev)
        if host.last['relo'] is None:
            return
        rec = host.last['relo']
        seen['n'] = len(rec['sel'])
        if kind == 'not_ascending':
            e = seen['elig']
            assert any(a > b for a, b in zip(e, e[1:])), "the doctored list must hold a larger id in front of a smaller one"
            assert 0 < len(rec['sel']) < len(e)                  # (matches are skipped as in the reference)
        else:
            # no factor: the input pose carried through the gauge transform (estimator.cpp:602-605), the window as if never armed
            # (check_step above compared it with vg_ba_optimize of the problem without relo)
            assert len(rec['sel']) == 0 and dev['relo']['n_factors'] == 0 and dev['relo']['armed'] == 1
            t, Rm = gauge_carried(rec['pose_in'], dev['summary'], dev['state'])
            e = max(np.abs(dev['relo']['pose'][:3] - t).max(), same_rotation(dev['relo']['pose'][3:], Rm))
            worst['carried'] = e
            assert e <= 1e-12, e
            check_by_products(dev, rec['req'])

    run(h_seq, h_ref, [22], {(1, 0): request}, K=11, L=40, n_steps=2, max_match=32, check=check, prepare=None if kind == 'not_ascending' else ascending)
    assert 'n' in seen
    print("relocalisation walk,", kind, ":", seen['n'], "factors", worst)
    return seen['n'], worst


def case_idle(h_a, h_b, seeds=(22, 23), n_steps=3):
    """Issue case 4: a reserved sequence that is never armed next to a plain one: check_step's bounds, finite loop poses.  Returns the
    largest state difference seen (relative to max(1, |.|)).  Measured: 0 on an MI355X, 1.8e-13 on the emulated kernels (the camera system
    of the reserved sequence is six columns wider: other tiles, other summation order)."""
    runs = []
    for reserve in (True, False):
        _, seen = run(h_a, h_b, list(seeds), {}, K=11, L=40, n_steps=n_steps, teacher=False, prepare=ascending, reserve=reserve)
        runs.append(seen)
    worst = 0.0
    for step, (ra, rb) in enumerate(zip(*runs)):
        for w, (a, b) in enumerate(zip(ra, rb)):
            assert np.isfinite(a['relo']['pose']).all() and a['relo']['armed'] == 0 and np.isfinite(a['state']['relo_pose']).all()
            assert 'relo_pose' not in b['state']
            info = b['info']
            twin = _Twin(b['state'], b['summary'], info, b['prior'], b['tracks'])
            M.check_step(step, w, twin, info['flag'], a)
            for k in ('pose', 'sb', 'ex'):
                worst = max(worst, np.abs(a['state'][k] - b['state'][k]).max() / max(1.0, np.abs(b['state'][k]).max()))
    print("reserved, never armed, against a plain sequence: largest state difference", worst)
    return worst


class _Twin:
    """What seq_model.check_step asks of its `host`: here a second device sequence."""

    def __init__(self, state, summary, info, prior, trk):
        self.last = dict(state=state, summary=summary, prior=prior, n_landmarks=info['n_landmarks'], n_factors=info['n_factors'])
        self.last_track_num = info['n_tracked']
        self._t = trk

    def tracks(self):
        t = self._t
        rows = np.concatenate([t['obs'][f, :n][:, [0, 1, 7, 2, 3, 4, 5, 6]] for f, n in enumerate(t['nobs'])]) if len(t['id']) else np.zeros((0, 8))
        return dict(id=t['id'], start=t['start'], nobs=t['nobs'], solve_flag=t['solve_flag'], depth=t['depth'], obs=rows)


def case_fused(h_seq, h_ref, nwin=32, armed=(0, 5, 31)):
    """Issue case 5: from 32 windows on the solve takes the fused factor kernel (four wavefronts); windows 0, 5 and 31 armed at step 1,
    the others idle, each against vg_ba_optimize with the bounds of test_resident_sequence_on_the_fused_factor_kernel."""
    worst = {}

    def check(step, w, host, flag, dev):
        M.check_step(step, w, host, flag, dev, tol=1e-7, tol_depth=1e-6)      # (the two kernels sum in different orders)
        e = check_relo(step, w, host, dev, tol=1e-7)
        if e is not None:
            worst[w] = e
    arm = {(1, w): (lambda win, prob: standard_request(win, prob, frame=3)) for w in armed}
    run(h_seq, h_ref, [100 + 3 * k for k in range(nwin)], arm, K=11, L=40, n_steps=2, check=check, prepare=ascending)
    assert sorted(worst) == sorted(armed)
    print("relocalisation frames on the fused factor kernel: loop pose differences", worst)
    return worst


def case_lifetime(h_seq, h_ref):
    """Issue case 8: every refusal leaves the sequence usable (the steps keep matching the host model, which never saw the refused
    requests); arming twice keeps the second; NULL disarms; vg_ba_seq_import disarms."""
    import pytest
    worst, state = {}, {}
    base = _full_check(worst)

    def good(win, prob):
        state['req'] = standard_request(win, prob, frame=3)
        return state['req']

    def refused(fn):
        with pytest.raises(RuntimeError, match="status -1"):
            fn()

    def between(step):
        if step == 0:
            return
        req = state['req']
        bad = lambda **kw: dict(req, **kw)
        if step == 1:
            # window 0 holds the good request already (armed by the driver): each refusal must leave it as it is
            refused(lambda: h_seq.seq_set_relo(0, req, struct_size=8))
            refused(lambda: h_seq.seq_set_relo(0, bad(frame=-1)))
            refused(lambda: h_seq.seq_set_relo(0, bad(frame=10)))                       # K - 1: the slot the step fills
            refused(lambda: h_seq.seq_set_relo(0, bad(n_match=0)))
            refused(lambda: h_seq.seq_set_relo(0, bad(match_id=np.arange(17, dtype=np.int32), match_xy=np.zeros((17, 2)))))   # max_match = 16
            refused(lambda: h_seq.seq_set_relo(0, bad(match_id=req['match_id'][::-1].copy())))
            refused(lambda: h_seq.seq_set_relo(0, bad(match_id=np.concatenate([req['match_id'][:1], req['match_id'][:-1]]))))   # a repeated id
            for key, val in (('match_xy', np.full_like(req['match_xy'], np.nan)), ('pose', np.array([0, 0, np.inf, 0, 0, 0, 1.0])),
                             ('prev_t', np.array([np.nan, 0, 0])), ('prev_r', np.full((3, 3), np.inf))):
                refused(lambda: h_seq.seq_set_relo(0, bad(**{key: val})))
            refused(lambda: h_seq.seq_set_relo(2, req))
            # armed twice: the second arming counts (the driver armed the first; this one is what the host model solved)
            h_seq.seq_set_relo(0, bad(frame=1, match_id=req['match_id'][:2], match_xy=req['match_xy'][:2] + 0.3))
            h_seq.seq_set_relo(0, req)
            # NULL disarms: window 1 is armed and disarmed again, the host model never armed it
            h_seq.seq_set_relo(1, req)
            h_seq.seq_set_relo(1, None)
        if step == 2:
            # vg_ba_seq_import disarms: window 1 is armed, handed back and re-seeded with its own export
            h_seq.seq_set_relo(1, bad(frame=2))
            exp, trk = h_seq.seq_export(1, 11)
            p = dict(state['base'])
            p.update(pose=exp['pose'], sb=exp['sb'], ex=exp['ex'], td=exp['td'], imu=exp['imu'], prior=exp['prior'], relo=None, lm_start=np.zeros(0, np.int32),
                     lm_nobs=np.zeros(0, np.int32), obs_off=np.zeros(0, np.int32), obs=np.zeros((0, 7)), inv_depth=np.zeros(0))
            h_seq.seq_import(1, p, trk)

    def prepare(win):
        ascending(win)
        state['base'] = win.base

    flags, seen = run(h_seq, h_ref, [22, 23], {(1, 0): good}, K=11, L=40, n_steps=3, check=base, prepare=prepare, between=between)
    assert seen[1][0]['relo']['armed'] == 1 and seen[1][0]['relo']['n_factors'] > 0 and seen[1][1]['relo']['armed'] == 0
    assert seen[2][0]['relo']['armed'] == 0 and seen[2][1]['relo']['armed'] == 0
    return worst


def case_no_reservation(h_seq, h_ref):
    """A sequence begun without vg_ba_seq_relo_reserve refuses a request and goes on; a reservation is consumed by one begin."""
    import pytest
    req = dict(frame=3, match_id=np.array([1, 2], np.int32), match_xy=np.zeros((2, 2)))

    def between(step):
        with pytest.raises(RuntimeError, match="status -1"):
            h_seq.seq_set_relo(0, req)
        with pytest.raises(RuntimeError, match="status -1"):
            h_seq.seq_get_relo(0)
    run(h_seq, h_ref, [22], {}, K=11, L=40, n_steps=1, check=lambda *a: M.check_step(*a), prepare=ascending, reserve=False, between=between)
    for bad in (-1, 1025):
        with pytest.raises(RuntimeError, match="status -1"):
            h_seq.seq_relo_reserve(bad)
    h_seq.seq_relo_reserve(8)
    h_seq.seq_relo_reserve(0)                                     # cancelled: the next sequence is a plain one
    run(h_seq, h_ref, [22], {}, K=11, L=40, n_steps=1, prepare=ascending, reserve=False, between=between)
    h_seq.seq_relo_reserve(8)
    run(h_seq, h_ref, [22], {}, K=11, L=40, n_steps=1, prepare=ascending, reserve=False)      # consumes the reservation ...
    run(h_seq, h_ref, [22], {}, K=11, L=40, n_steps=1, prepare=ascending, reserve=False, between=between)   # ... so this one is plain again


def case_overflow(h_seq, h_ref):
    """Issue case 8, capacities: an armed window whose relocalisation factors do not fit behind its window factors reports
    VG_ERR_UNSUPPORTED in info (the step is void), the other window is untouched, and the request is consumed by the void step."""
    K, MM, frame = 11, 32, 5
    sizes = {}
    run(h_seq, h_ref, [22, 23], {}, K=K, L=40, n_steps=2, prepare=ascending, reserve=False,
        check=lambda step, w, host, flag, dev: sizes.__setitem__((step, w), dev['info']['n_factors']))
    (s0, w0), f0 = max(sizes.items(), key=lambda kv: kv[1])      # the fullest window: every other one fits where it fits
    fcap = (f0 + 15) // 16 * 16                                  # the layout rounds the factor capacity up to 16
    seen = {}

    def request(win, prob):
        ids = problem_ids(win)
        elig = [l for l in range(len(ids)) if prob['lm_start'][l] <= frame]
        req = standard_request(win, prob, frame=frame, n_eligible=len(elig))
        pick = sorted(range(len(elig)), key=lambda k: ids[elig[k]])
        xy = project_matches(prob, req['pose'], elig)
        req.update(match_id=np.array([ids[elig[k]] for k in pick], np.int32), match_xy=np.array([xy[k] for k in pick], float))
        return req

    def check(step, w, host, flag, dev):
        if w != w0:
            M.check_step(step, w, host, flag, dev)
            assert dev['relo']['armed'] == 0
        elif step < s0:
            M.check_step(step, w, host, flag, dev)
        elif step == s0:
            n_relo = len(host.last['relo']['sel'])
            assert f0 + n_relo > fcap, "the request must not fit: " + str((f0, n_relo, fcap))
            assert dev['info']['status'] == -3, dev['info']
            seen['void'] = True
        else:
            assert dev['relo']['armed'] == 0 and dev['relo']['n_factors'] == 0      # consumed by the void step
            seen['consumed'] = True

    run(h_seq, h_ref, [22, 23], {(s0, w0): request}, K=K, L=40, n_steps=s0 + 2, max_match=MM, max_landmarks=64, max_factors=fcap - MM, check=check,
        prepare=ascending, teacher=True)
    assert seen == dict(void=True, consumed=True)


def case_imu_mode(h_imu, h_host, K=11, L=40, seeds=(22, 23)):
    """Issue case 7: the armed step through vg_ba_seq_step_imu_async next to the same step host-fed: states under check_step's bounds, the same factors, loop pose to 1e-9.
    The request names the resident pose (pose = NULL); its matches are the tracks' own observations in the loop frame, moved a little."""
    import seq_imu_model as I
    mk = lambda: [synth.FrameSource(synth.SyntheticSequence(s, n_frames=K + 3, K=K + 3, L=L), noise_seed=700 + s) for s in seeds]
    sa, sb_ = mk(), mk()
    n, frame = len(seeds), 3
    noise, g_norm = I.noise_of(sa[0].seq), sa[0].seq.cfg['g_norm']
    h_imu.seq_relo_reserve(16)
    wins_a, wins_b = [s.initial_window(K, 0) for s in sa], [s.initial_window(K, 0) for s in sb_]
    for w_ in wins_a + wins_b:                                   # (track lists in ascending id, as in the running system: see ascending())
        w_['tracks'].sort(key=lambda tr: tr['id'])
    I.begin(h_imu, sa, K, 10.0 / 460.0, 128, wins=wins_a)
    probs, trks = zip(*[synth.sequence_inputs(w) for w in wins_b])
    h_host.seq_relo_reserve(16)
    h_host.seq_begin(list(probs), list(trks), max_features=128, max_new_obs=128, init_depth=5.0, min_parallax=10.0 / 460.0)
    try:
        t = h_host.seq_tracks(0, K)
        pick = [f for f in range(len(t['id'])) if t['start'][f] <= frame < t['start'][f] + t['nobs'][f] and t['nobs'][f] >= 2]
        pick = pick[:10]
        req = dict(frame=frame, pose=None, match_id=np.array([t['id'][f] for f in pick], np.int32),
                   match_xy=np.array([t['obs'][f, frame - t['start'][f], :2] + 0.002 for f in pick], float), prev_t=np.array([0.3, -0.2, 0.1]),
                   prev_r=np.eye(3))
        h_imu.seq_set_relo(0, req)
        h_host.seq_set_relo(0, req)
        g = K - 1
        fa = [I.frame_of(sa[i], g) for i in range(n)]
        h_imu.seq_step_imu(fa)
        da, ma = h_imu.seq_states()
        ia = h_imu.seq_info()
        # the host-fed twin gets what processIMU produced ON THE DEVICE (the guess of vg_ba_seq_imu_get, the record of the new interval
        # from vg_ba_seq_export: at K-3 after a MARGIN_OLD slide, still in the newest slot otherwise), so that both steps solve identical
        # windows and check_step's bounds for identical inputs apply; the parity of those inputs is tests/test_seq_imu_*.py's subject
        fb = []
        for i in range(n):
            got = h_imu.seq_imu_get(i)
            recs = h_imu.seq_export(i, K, raw_imu=True)[0]['imu']
            rec = dict(recs[K - 3] if ia[i]['flag'] == M.OLD else recs[K - 2])
            rec.pop('valid', None)
            fb.append(dict(pose=got['pose'], sb=got['sb'], imu_new=rec, imu_merged=None, ids=fa[i]['ids'], obs=fa[i]['obs']))
        h_host.seq_step(fb)
        db, mb = h_host.seq_states()
        ib = h_host.seq_info()
        pa, pb = h_imu.seq_priors(), h_host.seq_priors()
        worst = 0.0
        for i in range(n):
            ta, tb = h_imu.seq_tracks(i, K), h_host.seq_tracks(i, K)
            ra, rb = h_imu.seq_get_relo(i), h_host.seq_get_relo(i)
            M.check_step(0, i, _Twin(db[i], mb[i], ib[i], pb[i], tb), ib[i]['flag'], dict(state=da[i], summary=ma[i], info=ia[i], prior=pa[i], tracks=ta))
            assert ra['armed'] == rb['armed'] == (1 if i == 0 else 0) and ra['n_factors'] == rb['n_factors'] and ra['frame'] == rb['frame']
            e = np.abs(ra['pose'] - rb['pose']).max() / max(1.0, np.abs(rb['pose']).max())
            worst = max(worst, e)
            assert e <= 1e-9, (i, e)
            if i == 0:
                assert ra['n_factors'] >= 4, ra
                check_by_products(dict(relo=ra, state=da[i]), req)
                check_by_products(dict(relo=rb, state=db[i]), req)
        print("relocalisation frame in IMU mode against the host-fed step: loop pose difference", worst)
    finally:
        h_imu.seq_end()
        h_host.seq_end()
    return worst


def case_cpp(h_seq, exe, tmp_path, timeout=900, K=11, n_frames=4, L=40, arm_frame=1, min_parallax=10.0 / 460.0):
    """Issue case 9: `vins_replay seq` with a relocalisation side file (ResidentEstimators::useRelocalisation / setReloFrame, which
    resolves the stamp against the class's header mirror) against the same frames and the same request driven through the Python
    binding; the trajectory and the by-products within seq_model.compare_replay_csv's bound.
    Two free-running chains (propagation in C++ / NumPy): they agree to 1e-9 on these frames.  (The three-frame data set of the same
    seeds does not serve: there the two chains part by 1.4e-5 in frame 2 of estimator 0 with or without a relocalisation frame, on
    the parent commit's calls alone.)"""
    import os
    import subprocess
    seeds = (22, 23)
    mk = lambda: [M.FrameSource(synth.SyntheticSequence(s, n_frames=K + n_frames + 1, K=K + n_frames + 1, L=L), noise_seed=200 + s) for s in seeds]
    src = mk()
    wins = M.write_seq_file(tmp_path / "frames.bin", src, K, n_frames, min_parallax=min_parallax)
    # the request for estimator 0, before frame `arm_frame`: the loop frame is named by the stamp of global frame arm_frame + 3; matches
    # for tracks of the initial window that have been seen by then, keyed by id, at the place of their first observation, moved a little
    stamp = float(src[0].seq.times[arm_frame + 3])
    tr = sorted((t for t in wins[0]['tracks'] if 1 <= t['start'] <= 4 and len(t['obs']) >= 3), key=lambda t: t['id'])[:12]
    ids = np.array([t['id'] for t in tr], np.int32)
    xy = np.array([[t['obs'][0][0] + 0.003, t['obs'][0][1] - 0.002] for t in tr], float)
    th = np.radians(5.0)
    prev_t, prev_r = np.array([0.3, -0.2, 0.1]), np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1.0]])
    with open(tmp_path / "relo.txt", "w") as f:
        f.write(f"{arm_frame} 0 {stamp!r} {len(ids)} " + " ".join(repr(float(v)) for v in np.concatenate([prev_t, prev_r.ravel()])) + "\n")
        for (x, y), i in zip(xy, ids):
            f.write(f"{float(x)!r} {float(y)!r} {int(i)}\n")
    r = subprocess.run([exe, "seq", str(tmp_path / "frames.bin"), str(tmp_path / "out.csv")], capture_output=True, text=True, timeout=timeout,
                       env=dict(os.environ, VINS_REPLAY_RELO=str(tmp_path / "relo.txt")))
    assert r.returncode == 0, r.stderr[-2000:]
    got = [float(v) for v in open(str(tmp_path / "out.csv") + ".relo").read().strip().split(",")]
    # ---- the Python-driven run: seq_model.drive_sequence with the header mirror and the request
    src = mk()
    wins = [s.initial_window(K, 0) for s in src]
    n = len(src)
    probs, trks = zip(*[synth.sequence_inputs(w) for w in wins])
    h_seq.seq_relo_reserve(len(ids))
    h_seq.seq_begin(list(probs), list(trks), max_features=512, max_new_obs=512, init_depth=5.0, min_parallax=min_parallax)
    newest = [(w['pose'][K - 1].copy(), w['sb'][K - 1].copy()) for w in wins]
    prev = [dict(samples=list(w['samples'][K - 3]), ba=s.seq.ba_lin, bg=s.seq.bg_lin) for w, s in zip(wins, src)]
    merged = [None] * n
    headers = [[float(s.seq.times[min(k, K - 2)]) for k in range(K)] for s in src]
    out, relo = [], None
    try:
        for w in range(n_frames):
            g = K - 1 + w
            if w == arm_frame:
                found = [k for k in range(K - 1) if headers[0][k] == stamp]
                assert found, "the loop frame must be in the window"
                h_seq.seq_set_relo(0, dict(frame=found[-1], pose=None, match_id=ids, match_xy=xy, prev_t=prev_t, prev_r=prev_r))
            frames, cur = [], []
            for i, s in enumerate(src):
                smp = s.samples(g - 1)
                rec = s.preintegrate(smp, newest[i][1][3:6], newest[i][1][6:9])
                pose, sb = M._propagate(newest[i][0], newest[i][1], smp, s.seq.cfg['g_norm'])
                fid, rows = s.image(g)
                frames.append(dict(pose=pose, sb=sb, imu_new=rec, imu_merged=merged[i], ids=fid, obs=rows))
                cur.append(dict(samples=smp, ba=newest[i][1][3:6].copy(), bg=newest[i][1][6:9].copy()))
                headers[i][K - 1] = float(s.seq.times[g])
            h_seq.seq_step(frames)
            sts, _ = h_seq.seq_states()
            info = h_seq.seq_info()
            if w == arm_frame:
                relo = h_seq.seq_get_relo(0)
                relo['local_index'] = found[-1]
            row = []
            for i, s in enumerate(src):
                st = sts[i]
                newest[i] = (st['pose'][K - 1].copy(), st['sb'][K - 1].copy())
                if info[i]['flag'] == M.NEW:
                    prev[i]['samples'] = prev[i]['samples'] + cur[i]['samples'][1:]
                    merged[i] = s.preintegrate(prev[i]['samples'], prev[i]['ba'], prev[i]['bg'])
                    headers[i][K - 2] = headers[i][K - 1]
                else:
                    prev[i], merged[i] = cur[i], None
                    headers[i] = headers[i][1:] + [headers[i][K - 1]]
                qm = B.R2q(q2R(st['pose'][K - 1][3:]))
                row.append((st['pose'][K - 1][:3].copy(), np.array([qm[3], qm[0], qm[1], qm[2]]), st['sb'][K - 1][:3].copy(), info[i]['flag'], info[i]['n_after']))
            out.append(row)
    finally:
        h_seq.seq_end()
    worst = M.compare_replay_csv(tmp_path / "out.csv", out, n)
    assert relo['armed'] == 1 and relo['n_factors'] >= 4, relo
    assert [int(v) for v in got[:5]] == [arm_frame, 0, 1, relo['n_factors'], relo['local_index']], got[:5]
    q = relo['relative_q'] * (1.0 if np.dot(relo['relative_q'], got[15:19]) >= 0 else -1.0)
    p = np.concatenate([relo['pose'][:3], relo['pose'][3:] * (1.0 if np.dot(relo['pose'][3:], got[8:12]) >= 0 else -1.0)])
    want = np.concatenate([p, relo['relative_t'], q, [relo['relative_yaw']], relo['drift_r'].ravel(), relo['drift_t']])
    e = np.abs(np.array(got[5:]) - want).max()
    assert e < 1e-6, e
    print("vins_replay seq with a relocalisation frame vs the Python-driven sequence: trajectory", worst, "loop pose and by-products", e)
    return worst, e


def case_bridge(h_a, h_b, data, frame=1):
    """Issue case 7, the bridge: the armed step through vg_vio_step_async (handle A) against the two old calls, vg_fe_tracks_step +
    vg_ba_seq_step_imu_async fed from the pinned message (handle B), from the same seeded state: states, summaries, info, track
    tables, IMU state and the relocalisation result to bit patterns, as tests/test_vio_bridge.py holds everything else."""
    import vio_bridge_case as V
    try:
        for h in (h_a, h_b):
            h.seq_relo_reserve(16)
        a, b = V.Rig(h_a, data), V.Rig(h_b, data)
        h_a.vio_begin(lists=False)
        a.vio_step(True); b.old_step(True)                        # one idle frame first: the block stays the unit pose on both paths
        V.same_snapshot(a.snapshot(), b.snapshot(), ("relo bridge", "idle"))
        t = h_b.seq_tracks(0, data.K)
        pick = sorted((f for f in range(len(t['id'])) if t['start'][f] <= frame < t['start'][f] + t['nobs'][f]), key=lambda f: t['id'][f])[:16]
        req = dict(frame=frame, pose=None, match_id=np.array([t['id'][f] for f in pick], np.int32),
                   match_xy=np.array([t['obs'][f, frame - t['start'][f], :2] + 0.002 for f in pick], float), prev_t=np.array([0.3, -0.2, 0.1]), prev_r=np.eye(3))
        h_a.seq_set_relo(0, req); h_b.seq_set_relo(0, req)
        a.vio_step(True); b.old_step(True)
        sa, sb = a.snapshot(), b.snapshot()
        V.same_snapshot(sa, sb, ("relo bridge", "armed"))
        out = []
        for w in range(data.S):
            ra, rb = h_a.seq_get_relo(w), h_b.seq_get_relo(w)
            for k in ra:
                V.same_bits(np.asarray(ra[k], np.float64), np.asarray(rb[k], np.float64), ("relo bridge", w, k))
            V.same_bits(sa["states"][w]["relo_pose"], ra["pose"], ("relo bridge", w, "state relo_pose"))
            out.append((ra['armed'], ra['n_factors']))
        a.vio_step(True); b.old_step(True)                        # consumed: idle again on both
        V.same_snapshot(a.snapshot(), b.snapshot(), ("relo bridge", "after"))
        out.append((h_a.seq_get_relo(0)['armed'], len(pick)))
        return out
    finally:
        V.release(h_a, h_b)
