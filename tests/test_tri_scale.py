"""vg_triangulate (triangulate_kernel) and the triangulation of the resident sequences (ba_seq_tri_kernel), both csrc/tri_dlt.h,
against an 80-bit DLT null vector with a bound per landmark that follows the landmark's own conditioning (tests/tri_ref.py).

The older check holds one scene to rtol 1e-8 against LAPACK: too loose for a well-posed landmark, meaningless for an ill-posed
one.  Here     |depth - d| <= bound = C * eps * (1 + |d|) / |v3| * ( s1 / (s3 - s4) + max(1, max|Ps|) / (s3 - s4) )
with d, v3 and the singular values from the reference alone.  The 0.1 cut of feature_manager.cpp:251 is asserted where the
reference decides it with room: d > 0.1 + bound -> the device returns its depth; d < 0.1 - bound (negative d included) -> it
returns init_depth exactly (two values of init_depth); a landmark inside the margin is not judged.  The table is built so that
at most 2 % of its landmarks are in the margin and at least 60 % have bound <= 1e-10 |d|
(test_table_is_decided_and_mostly_tight).

C is the smallest power of two that the worst measured |depth - d| / bound(C = 1) of emulator and MI355X stays under with a
factor 2 to spare (MEASURED)."""
import numpy as np
import pytest

import tri_ref as T
from oracle import ba_numpy as B
from seq_model import NEW
from vins_mono_amd import ba, synth

C = 1
MEASURED = """worst |depth - d| / bound(C = 1) over the judged landmarks
                                                              CPU fiber emulator      MI355X
    vg_triangulate, 23 scenes / 670 landmarks, 2 init_depths  0.309                   0.269
        (scene of the worst: well_b1.0_n0.001_1 / well_b1.0_n0.001_0; origin 1e4: 0.263 on both)
    block edges, L = 1 / 63 / 64 / 65 / 130                   0.220                   0.222
    ba_seq_tri_kernel, 2 windows                              0.141                   0.160
C = 1: 2 x 0.309 < 1.  On the same table the same Jacobi in float64 (NumPy) reaches 0.341, numpy's LAPACK 4.33 (gesdd on the
float64 matrix; its worst landmarks are the ones with pixel noise, s4 > 0) -- test_float64_restatement_stays_inside_the_bound.
The table: 670 landmarks, 1 in the margin of the 0.1 cut (pure rotation), 584 (87 %) with bound <= 1e-10 |d|.
mutation condition, landmarks beyond 2 x bound out of 670: largest_column 670, point_not_normalised 320, t_by_R1 668,
two_sweeps 574."""
INIT_DEPTHS = (5.0, 7.5)
BLOCK_L = (1, 63, 64, 65, 130)
ULP2 = 2 * 2.0 ** -52


def _device(h, sc, init_depth, table=None):
    st, nb, off, pts = table if table is not None else sc.table()
    return h.triangulate(sc.Ps, sc.Rs.reshape(T.K, 9), T.TIC, T.RIC, st, nb, off, pts, init_depth)


def judge(got, refs, init_depth, c=None, slack=0.0):
    """The assertions of the module docstring on one call's depths; returns (worst |depth - d| / bound(1), judged, in the margin).
    slack: relative allowance on top of the bound (the sequence's round trip through the inverse depth)."""
    c = C if c is None else c
    worst, judged, margin = 0.0, 0, 0
    for l, r in enumerate(refs):
        b, d = T.bound(r, c), float(r['d'])
        if d > 0.1 + b:
            e = abs(T.LD(got[l]) - r['d'])
            assert got[l] != init_depth or abs(d - init_depth) <= b, (l, d, got[l])
            assert e <= b + slack * abs(d), f"landmark {l}: |{got[l]!r} - {d!r}| = {float(e):.3e} > bound {b:.3e} (C = {c})"
            worst = max(worst, float(e) / (b / c))
            judged += 1
        elif d < 0.1 - b:
            assert got[l] == init_depth, (l, d, b, got[l])
            judged += 1
        else:
            margin += 1
    return worst, judged, margin


# ---- the device checks, one body for the emulator and the MI355X ------------------------------------------------------------------
def check_scenes(h, tag):
    worst = {}
    for name, sc in T.scenes().items():
        refs = T.scene_reference(name)
        got = {x: _device(h, sc, x) for x in INIT_DEPTHS}
        for x in INIT_DEPTHS:
            w, judged, margin = judge(got[x], refs, x)
            worst[name] = max(worst.get(name, 0.0), w)
        above = np.array([float(r['d']) > 0.1 + T.bound(r, C) for r in refs])
        assert np.array_equal(got[INIT_DEPTHS[0]][above], got[INIT_DEPTHS[1]][above]), name        # init_depth touches nothing else
        # the same landmarks with the observation blocks laid out in ascending order: bit-identical
        own = [l for l in range(len(sc)) if sc.share[l] is None]
        assert np.array_equal(_device(h, sc, INIT_DEPTHS[0], sc.table(order=own)), got[INIT_DEPTHS[0]]), name
    print(f"tri {tag}: worst |depth - d| / bound(C = 1) per scene: " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    print(f"tri {tag}: worst over all scenes {max(worst.values()):.3f}, C = {C}")
    sc, refs = T.scenes()["cut"], T.scene_reference("cut")
    d = np.array([float(r['d']) for r in refs])
    got = _device(h, sc, 5.0)
    assert np.all(got[d < 0.1] == 5.0) and np.all(np.abs(got[d > 0.1] - d[d > 0.1]) < 1e-9) and (d < 0.1).sum() >= 12 and (d > 0.1).sum() >= 8


def check_block_edges(h, tag):
    """L = 1, 63, 64, 65, 130 in one call each; every depth bit-identical to the same landmark run alone"""
    sc = T.block_scene()
    refs = [T.reference(sc.Ps, sc.Rs, T.TIC, T.RIC, sc.start[l], sc.nobs[l], sc.points_of(l)) for l in range(len(sc))]
    alone = np.array([_device(h, sc.sub([l]), 5.0)[0] for l in range(len(sc))])
    worst = 0.0
    for L in BLOCK_L:
        got = _device(h, sc.sub(range(L)), 5.0)
        assert got.shape == (L,) and np.array_equal(got, alone[:L]), L
        worst = max(worst, judge(got, refs[:L], 5.0)[0])
    print(f"tri {tag}: block edges, worst |depth - d| / bound(C = 1) {worst:.3f}")


def check_refusals(h):
    sc = T.block_scene()
    pts = np.tile([[0.1, 0.2, 1.0]], (13, 1))
    P13, R13 = np.vstack([sc.Ps, sc.Ps[-1:] + 0.3]), np.concatenate([sc.Rs, sc.Rs[-1:]]).reshape(13, 9)
    with pytest.raises(RuntimeError, match="status -3"):          # VG_ERR_UNSUPPORTED
        h.triangulate(P13, R13, T.TIC, T.RIC, [0], [13], [0], pts)
    for start, nobs in ((T.K - 2, 3), (T.K, 1), (-1, 2), (0, 0)):
        with pytest.raises(RuntimeError, match="status -1"):      # VG_ERR_BAD_ARG
            h.triangulate(sc.Ps, sc.Rs.reshape(T.K, 9), T.TIC, T.RIC, [start], [nobs], [0], pts)
    out = np.full(4, -123.0)                                       # L = 0: VG_OK, nothing written
    keep = [np.ascontiguousarray(a, np.float64) for a in (sc.Ps, sc.Rs, T.TIC, T.RIC, pts)]
    tab = np.zeros(1, np.int32)
    rc = h.lib.vg_triangulate(h.h, T.K, *[ba._dp(a) for a in keep[:4]], 0, ba._ip(tab), ba._ip(tab), ba._ip(tab), ba._dp(keep[4]), 5.0, ba._dp(out))
    assert rc == 0 and np.all(out == -123.0)
    assert len(h.triangulate(sc.Ps, sc.Rs.reshape(T.K, 9), T.TIC, T.RIC, [], [], [], pts)) == 0
    one = sc.sub([0])                                              # the handle is still good
    assert np.isfinite(_device(h, one, 5.0)[0])


# ---- ba_seq_tri_kernel: the triangulation of a host-fed resident sequence ---------------------------------------------------------
SEQ_K = 11
SEQ_SEEDS = (31, 32)


def check_sequence(h, tag):
    """Two windows, max_iters = 0 (the solve leaves poses and depths where triangulation put them), min_parallax so large that the
    step chooses MARGIN_SECOND_NEW (no depth is re-anchored).  Every track starts with depth -1."""
    K, WS = SEQ_K, SEQ_K - 1
    srcs = [synth.FrameSource(synth.SyntheticSequence(s, n_frames=K + 3, K=K + 3, L=70), noise_seed=900 + s) for s in SEQ_SEEDS]
    wins = [s.initial_window(K, 0) for s in srcs]
    for w in wins:
        long_ = next(t for t in w['tracks'] if t['start'] == 0 and len(t['obs']) == K - 1)
        row = long_['obs'][3]
        row[0], row[1], row[2] = 2.5 * row[0], 2.5 * row[1], 2.5 * row[2]                     # one observation with z != 1
    probs, trks = zip(*[synth.sequence_inputs(w) for w in wins])
    probs = [dict(p, max_iters=0) for p in probs]
    assert all(np.all(t['depth'] == -1.0) for t in trks)
    frames = []
    for s, w in zip(srcs, wins):
        pose, sb = s.guess(K - 1)
        ids, obs = s.image(K - 1)
        frames.append(dict(pose=pose, sb=sb, imu_new=s.preintegrate(s.samples(K - 2), s.seq.ba_lin, s.seq.bg_lin), imu_merged=None, ids=ids, obs=obs))
    h.seq_begin(probs, list(trks), max_features=128, max_new_obs=128, init_depth=5.0, min_parallax=1e3)
    try:
        h.seq_step(frames)
        _, sms = h.seq_states()
        assert all(m['status'] == 0 and m['num_iterations'] == 0 for m in sms), sms
        info = h.seq_info()
        got = [h.seq_tracks(w, K) for w in range(len(srcs))]
    finally:
        h.seq_end()
    worst = 0.0
    for w, (win, trk, fr) in enumerate(zip(wins, trks, frames)):
        assert info[w]['flag'] == NEW and info[w]['n_tracked'] >= 20, info[w]
        pose = np.vstack([win['pose'][:K - 1], fr['pose'][None]])
        Ps = pose[:, :3]
        Rs = np.array([B.q2R(q / np.sqrt(q @ q)) for q in pose[:, 3:]])                        # normalised as the kernel does
        ex = probs[w]['ex']
        tic, ric = ex[:3], B.q2R(ex[3:] / np.sqrt(ex[3:] @ ex[3:]))
        depth = dict(zip(got[w]['id'].tolist(), got[w]['depth'].tolist()))
        new_obs = dict(zip(fr['ids'].tolist(), fr['obs']))
        refs, out, kinds = [], [], set()
        for t in win['tracks']:
            pts = [r[:3] for r in t['obs']]
            continued = t['id'] in new_obs and t['start'] + len(pts) == WS
            if continued:
                pts.append(new_obs[t['id']][:3])
            n = len(pts)
            admitted = n >= 2 and t['start'] < WS - 2                                          # feature_manager.cpp:206-208
            if not admitted:
                if t['id'] in depth:                                                           # (a track of frame WS - 1 alone is gone)
                    assert depth[t['id']] == -1.0, (w, t['id'], depth[t['id']])
                    kinds.add('start %d' % min(t['start'], WS - 1))
                continue
            kinds.add('%d observations' % n)
            if any(p[2] != 1.0 for p in pts):
                kinds.add('z != 1')
            refs.append(T.reference(Ps, Rs, tic, ric, t['start'], n, np.array(pts)))
            out.append(depth[t['id']])
        assert len(refs) >= 20 and {'2 observations', '%d observations' % (K - 1), 'start %d' % (WS - 2), 'start %d' % (WS - 1), 'z != 1'} <= kinds, kinds
        x, judged, margin = judge(out, refs, 5.0, slack=ULP2)
        assert judged >= 20 and margin <= 2, (judged, margin)
        worst = max(worst, x)
    print(f"tri {tag}: sequence, worst |depth - d| / bound(C = 1) {worst:.3f}")


# ---- the reference, the bound and the table themselves (no device) ----------------------------------------------------------------
def _all_landmarks():
    for name, sc in T.scenes().items():
        for l, r in enumerate(T.scene_reference(name)):
            yield name, sc, l, r


def test_table_is_decided_and_mostly_tight():
    """at most 2 % of the landmarks in the margin of the 0.1 cut, at least 60 % with bound <= 1e-10 |d|; both sides of the cut, negative
    depths, every (nobs, start), both origins occur"""
    n = margin = tight = 0
    seen = set()
    for name, sc, l, r in _all_landmarks():
        b, d = T.bound(r, C), float(r['d'])
        n += 1
        margin += not (d > 0.1 + b or d < 0.1 - b)
        tight += b <= 1e-10 * abs(d)
        seen.add((sc.nobs[l], sc.start[l]))
        seen.add('behind' if d < 0 else ('below' if d < 0.1 - b else ('above' if d < 0.11 and d > 0.1 + b else 'far')))
    print(f"{n} landmarks, {margin} in the margin, {tight} with bound <= 1e-10 |d| ({tight / n:.1%})")
    assert margin <= 0.02 * n and tight >= 0.6 * n, (n, margin, tight)
    assert {(nobs, i0) for nobs in T.NOBS for i0 in range(T.K - nobs + 1)} <= seen and {'behind', 'below', 'above'} <= seen
    assert any(np.abs(sc.Ps).max() > 9e3 for sc in T.scenes().values())


def test_float64_restatement_stays_inside_the_bound():
    """the same Jacobi in float64 and numpy's LAPACK on the float64 matrix, against the 80-bit reference: what the bound is sized by"""
    wj = wl = 0.0
    for name, sc, l, r in _all_landmarks():
        b, d = T.bound(r, 1), float(r['d'])
        if not d > 0.1 + b:
            continue
        m = T.reference(sc.Ps, sc.Rs, T.TIC, T.RIC, sc.start[l], sc.nobs[l], sc.points_of(l), np.float64)
        v = np.linalg.svd(T.dlt_matrix(sc.Ps, sc.Rs, T.TIC, T.RIC, sc.start[l], sc.nobs[l], sc.points_of(l), np.float64))[2][-1]
        wj, wl = max(wj, abs(float(m['d']) - d) / b), max(wl, abs(v[2] / v[3] - d) / b)
    print(f"|d64 - d| / bound(C = 1): Jacobi in float64 {wj:.3f}, LAPACK {wl:.3f}")
    assert wj <= 1.0 and wl <= 8.0, (wj, wl)


@pytest.mark.parametrize("edit", T.EDITS)
def test_each_edit_exceeds_twice_the_bound(edit):
    n = 0
    for name, sc, l, r in _all_landmarks():
        b = T.bound(r, C)
        m = T.reference(sc.Ps, sc.Rs, T.TIC, T.RIC, sc.start[l], sc.nobs[l], sc.points_of(l), np.float64, edit)
        n += np.isfinite(b) and not abs(float(m['d']) - float(r['d'])) <= 2 * b
    print(f"edit {edit}: {n} landmarks beyond 2 x bound")
    assert n >= 1


def test_reference_against_mpmath():
    """Optional cross-check of the 80-bit Jacobi: mpmath.svd_r at 50 digits on the same 80-bit matrix.  1e-17 relative is asked
    wherever 80-bit arithmetic can give it, i.e. where the landmark's own bound, taken with eps = 2^-63, is below 1e-17 |d|; on
    the ill-posed rest of the table (amplifications up to 1e9 by design) no 64-bit mantissa can, and the reference is held to
    that bound instead.  Measured: 3.8e-19 at worst where 1e-17 is asked, 0.13 x bound(eps = 2^-63) at worst overall."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    exact = lambda x: mp.mpf(float(x)) + mp.mpf(float(x - T.LD(float(x))))                  # an 80-bit number as two doubles
    worst_rel, worst_ratio, asked = 0.0, 0.0, 0
    for name, sc, l, r in _all_landmarks():
        b80 = T.bound(r, 1) * 2.0 ** -11
        if l % 3 or not np.isfinite(b80):
            continue
        A = T.dlt_matrix(sc.Ps, sc.Rs, T.TIC, T.RIC, sc.start[l], sc.nobs[l], sc.points_of(l))
        U, S, V = mp.svd_r(mp.matrix([[exact(x) for x in row] for row in A]))
        k = min(range(4), key=lambda i: S[i])
        d = V[k, 2] / V[k, 3]
        e = float(abs(d - exact(r['d'])))
        assert e <= b80, (name, l, e, b80)
        worst_ratio = max(worst_ratio, e / b80)
        if b80 <= 1e-17 * abs(float(d)):
            asked += 1
            worst_rel = max(worst_rel, e / abs(float(d)))
    print(f"80-bit Jacobi vs mpmath.svd_r at 50 digits: {worst_rel:.2e} relative at worst over {asked} landmarks, {worst_ratio:.3f} x bound(eps = 2^-63) overall")
    assert asked >= 60 and worst_rel <= 1e-17, (asked, worst_rel)


# ---- emulated kernels (CPU fiber emulator) ----------------------------------------------------------------------------------------
def test_emulated_scenes(simt_handle):
    check_scenes(simt_handle, 'emulated')


def test_emulated_block_edges(simt_handle):
    check_block_edges(simt_handle, 'emulated')


def test_emulated_refusals(simt_handle):
    check_refusals(simt_handle)


def test_emulated_sequence(simt_handle):
    check_sequence(simt_handle, 'emulated')


# ---- MI355X -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_scenes(handle):
    check_scenes(handle, 'gpu')


@pytest.mark.gpu
def test_block_edges(handle):
    check_block_edges(handle, 'gpu')


@pytest.mark.gpu
def test_refusals(handle):
    check_refusals(handle)


@pytest.mark.gpu
def test_sequence(handle):
    check_sequence(handle, 'gpu')
