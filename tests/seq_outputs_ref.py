"""TEST INFRASTRUCTURE: what the estimator node publishes between two frames, restated in NumPy float64 from the reference's two
functions (vins_estimator/src/utility/visualization.cpp pubKeyframe :348-404, pubPointCloud :240-296), fed from what a caller of a
resident sequence could get before vg_ba_seq_outputs_*: the track table of vg_ba_seq_get_tracks and the states of vg_ba_seq_export.

`mutant` changes the restatement one way at a time (tests/seq_outputs_case.py case_mutations: each must be told apart from the device's
result by a named case):
    'pose_index'     Rs / Ps of the frame behind the right one (a reader of the states from before the slide), in the world point and
                     in the keyframe pose
    'no_tic'         the world point without tic
    'newest_row'     the keyframe row from the track's newest observation instead of the one in frame W - 2
    'last_frame_gt'  start + n_obs - 1 >  W - 2 for >=
    'solve_nonzero'  solve_flag != 0 for == 1
"""
import numpy as np

OLD = 0                       # VG_MARGIN_OLD
TRUNCATED = 1                 # VG_SEQ_OUT_TRUNCATED
MUTANTS = ('pose_index', 'no_tic', 'newest_row', 'last_frame_gt', 'solve_nonzero')


def q2R(q):
    """Quaterniond(w, x, y, z).normalized().toRotationMatrix(), q = x y z w"""
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def restate(tracks, pose, ex, K, info=None, mutant=None):
    """tracks: Handle.seq_tracks (id, start, nobs, solve_flag, depth, obs [f, K, 8] rows x y u v vx vy cur_td z); pose (K, 7), ex (7,):
    Handle.seq_export; info: the window's record of the last step (Handle.seq_info) or None before the first step.
    Returns the un-truncated lists: dict(status, keyframe_valid, pose, ex_pose, kf / cloud / margin: track indices in list order,
    world (n_tracks, 3) float64 world point of every track, kf_norm, kf_uv (float32), kf_id)."""
    W = K - 1
    pose, ex = np.asarray(pose, np.float64).reshape(K, 7), np.asarray(ex, np.float64).reshape(7)
    i_kf = W - 2 + (1 if mutant == 'pose_index' else 0)
    out = dict(status=0, keyframe_valid=0, pose=pose[i_kf].copy(), ex_pose=ex.copy())
    if info is not None:
        out['status'] = int(info['status'])
        out['keyframe_valid'] = 1 if info['flag'] == OLD else 0
    n = len(tracks['id']) if out['status'] == 0 else 0           # a void step: nothing is published
    ric, tic = q2R(ex[3:]), ex[:3]
    kf, cloud, margin = [], [], []
    world = np.zeros((n, 3))
    norm, uv = np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32)
    for f in range(n):
        s, used, flag = int(tracks['start'][f]), int(tracks['nobs'][f]), int(tracks['solve_flag'][f])
        solved = (flag != 0) if mutant == 'solve_nonzero' else (flag == 1)
        rows = tracks['obs'][f]
        point0 = np.array([rows[0][0], rows[0][1], rows[0][7]])
        pts_i = point0 * tracks['depth'][f]
        si = min(s + 1, K - 1) if mutant == 'pose_index' else s
        cam = ric @ pts_i + (0.0 if mutant == 'no_tic' else tic)
        world[f] = q2R(pose[si][3:]) @ cam + pose[si][:3]
        last = s + used - 1
        reaches = (last > W - 2) if mutant == 'last_frame_gt' else (last >= W - 2)
        if s < W - 2 and reaches and solved:                     # pubKeyframe :378
            j = used - 1 if mutant == 'newest_row' else W - 2 - s
            kf.append(f)
            norm[f] = np.float32(rows[j][0]), np.float32(rows[j][1])
            uv[f] = np.float32(rows[j][2]), np.float32(rows[j][3])
        if not (used >= 2 and s < W - 2):                        # pubPointCloud :251 / :276
            continue
        if not (s > W * 3.0 / 4.0 or not solved):                # :253
            cloud.append(f)
        if s == 0 and used <= 2 and solved:                      # :281
            margin.append(f)
    out.update(kf=np.array(kf, int), cloud=np.array(cloud, int), margin=np.array(margin, int), world=world,
               kf_norm=norm, kf_uv=uv, kf_id=np.asarray(tracks['id'], np.int32)[:n])
    return out


def compare(got, ref, max_points, where=""):
    """The device's message of one window (Handle.seq_outputs) against restate(): decisions equal, copied values to the bit, world points
    within one float32 ulp of the float64 value rounded to float32.  Returns the largest world-point difference in ulps."""
    counts = (len(ref['kf']), len(ref['cloud']), len(ref['margin']))
    status = ref['status']
    if max(counts) > max_points:
        status = TRUNCATED
    assert got['status'] == status, (where, 'status', got['status'], status)
    assert got['keyframe_valid'] == ref['keyframe_valid'], (where, 'keyframe_valid', got['keyframe_valid'], ref['keyframe_valid'])
    assert (got['n_keyframe'], got['n_cloud'], got['n_margin']) == counts, (where, 'counts', (got['n_keyframe'], got['n_cloud'], got['n_margin']), counts)
    assert np.array_equal(got['pose'].view(np.uint64), ref['pose'].view(np.uint64)), (where, 'pose', got['pose'], ref['pose'])
    assert np.array_equal(got['ex_pose'].view(np.uint64), ref['ex_pose'].view(np.uint64)), (where, 'ex_pose')
    worst = 0.0
    sel = ref['kf'][:max_points]
    assert len(got['kf_id']) == len(sel), (where, 'stored keyframe rows', len(got['kf_id']), len(sel))
    assert np.array_equal(got['kf_id'], ref['kf_id'][sel]), (where, 'kf_id: selection or order')
    assert got['kf_norm'].dtype == np.float32 and np.array_equal(got['kf_norm'].view(np.uint32), ref['kf_norm'][sel].view(np.uint32)), (where, 'kf_norm')
    assert got['kf_uv'].dtype == np.float32 and np.array_equal(got['kf_uv'].view(np.uint32), ref['kf_uv'][sel].view(np.uint32)), (where, 'kf_uv')
    for key, idx in (('kf_point_3d', sel), ('cloud_xyz', ref['cloud'][:max_points]), ('margin_xyz', ref['margin'][:max_points])):
        g = got[key]
        assert g.dtype == np.float32 and g.shape == (len(idx), 3), (where, key, g.shape, len(idx))
        if not len(idx):
            continue
        want = ref['world'][idx].astype(np.float32)
        ulp = np.spacing(np.abs(want)).astype(np.float64)
        d = np.abs(g.astype(np.float64) - want.astype(np.float64)) / ulp
        worst = max(worst, float(d.max()))
        assert np.isfinite(g).all() and d.max() <= 1.0, (where, key, 'ulps', float(d.max()), int(d.argmax()) // 3)
    return worst
