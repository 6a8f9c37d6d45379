"""vg_fe_tracks_* (track lists resident on the device) against vg_fe_read_image_batch plus the bookkeeping of FeatureTracker restated in
NumPy (TrackBook, from feature_tracker.cpp:118-128, :193-198, :55-68, :71-79, :204-214, :272-305 and feature_tracker_node.cpp:133-150),
and against the reference's own class (oracle/_ref/libvins_ref_fe.so).  Every field of every vg_fe_tracks_out of every frame must be
identical: ints equal, floats and doubles by bit pattern.  No tolerance, no stream or frame left out.

Used by tests/test_fe_tracks.py under the emulator (`not gpu`, in a child process) and on the device (`gpu`)."""
import numpy as np

from vins_mono_amd import fe

import fe_scene
from fe_read_image_case import INTR
from fe_read_image_batch_case import Stream, check_coverage, coverage, run_batch, seven_streams, status_of, unstable_like

# MIN_DIST of the long-list case.  The detection's min-distance grid holds 1024 cells of MIN_DIST pixels (FE_MAX_CELLS, csrc/fe_layout.h):
# at 320x240 a MIN_DIST below 9 is refused with VG_ERR_UNSUPPORTED by the frame path itself (36 x 27 = 972 cells at 9; 40 x 30 at 8), so
# 9 is the smallest spacing the case can run at.  What the case is for stays asserted on the oracle side: a list longer than 256
# entries on every stream.
LONG_MIN_DIST = 9

DIAG = ("n1", "n2", "ransac_ran", "n_kept", "n_new", "fallback", "ransac_best", "ransac_niters")


def stamp_of(c, k):
    """_cur_time of frame k of stream c: a different rate per stream; stream 2 with uneven steps"""
    return 1.0 + k * (0.05 + 0.003 * c) + (0.011 * (k % 3) if c == 2 else 0.0)


class TrackBook:
    """what FeatureTracker keeps besides the points, and what the node makes of it, for ONE stream with its own n_id"""

    def __init__(self):
        self.ids, self.cnt = np.zeros(0, np.int64), np.zeros(0, np.int64)
        self.pts, self.un = np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32)
        self.prev_map, self.n_id, self.prev_time = {}, 0, 0.0
        self.in_map = np.zeros(0, np.uint8)

    def seed(self, pts):
        """a caller that re-seeds its tracks: fresh ids, count 1, no previous map; returns the arguments of tracks_set"""
        n = len(pts)
        self.pts = np.asarray(pts, np.float32).reshape(-1, 2)
        self.ids, self.cnt = np.arange(self.n_id, self.n_id + n, dtype=np.int64), np.ones(n, np.int64)
        self.n_id += n
        self.un, self.prev_map, self.in_map = np.zeros((n, 2), np.float32), {}, np.zeros(n, np.uint8)
        return dict(cur_xy=self.pts.copy(), ids=self.ids.copy(), track_cnt=self.cnt.copy(), n_id=self.n_id, prev_time=self.prev_time)

    def state(self):
        return dict(n=len(self.ids), n_id=self.n_id, prev_time=self.prev_time, cur_xy=self.pts.copy(), ids=self.ids.astype(np.int32),
                    track_cnt=self.cnt.astype(np.int32), un_xy=self.un.copy(), in_map=self.in_map.copy())

    def advance(self, pts_in, publish, out, use_cb, stamp):
        """one frame: `out` is what read_image_batch returned for the list `pts_in`; returns what vg_fe_tracks_out must hold"""
        assert np.array_equal(np.asarray(pts_in, np.float32).view(np.uint32), self.pts.view(np.uint32)), "the book and the caller's list differ"
        st = out["status_lk"] != 0                                        # :115-128 reduceVector
        ids, cnt, pts = self.ids[st], self.cnt[st] + 1, out["forw_xy"][st]   # :129 n++
        if publish:
            if out["ransac_ran"]:                                         # :193-198
                keep = out["status_f"] != 0
                ids, cnt, pts = ids[keep], cnt[keep], pts[keep]
            assert len(ids) == out["n2"]
            order = unstable_like(cnt) if use_cb else np.arange(len(ids))  # :48 the sort, as this caller's platform makes it
            sel = np.asarray(order, np.int64)[out["kept"]]                 # :55-68
            ids, cnt, pts = ids[sel], cnt[sel], pts[sel]
            k = len(out["new_xy"])                                         # :71-79 addPoints
            ids, cnt = np.concatenate([ids, -np.ones(k, np.int64)]), np.concatenate([cnt, np.ones(k, np.int64)])
            pts = np.concatenate([pts, out["new_xy"]]).astype(np.float32).reshape(-1, 2)
        n = len(ids)
        assert n == out["n_final"]
        un = np.asarray(out["un_xy"], np.float32).reshape(-1, 2)          # :262-271
        cur_map = {}
        for i in range(n):
            cur_map.setdefault(int(ids[i]), un[i].copy())                 # (map::insert keeps the first entry of a key)
        vel = np.zeros((n, 2), np.float32)                                # :272-305
        if self.prev_map:
            dt = np.float64(stamp) - np.float64(self.prev_time)
            with np.errstate(all="ignore"):
                for i in range(n):
                    if ids[i] != -1 and int(ids[i]) in self.prev_map:
                        d32 = (un[i] - self.prev_map[int(ids[i])]).astype(np.float32)
                        vel[i] = (d32.astype(np.float64) / dt).astype(np.float32)
        self.prev_map, self.prev_time = cur_map, float(stamp)
        self.in_map = (ids != -1).astype(np.uint8)
        for i in range(n):                                                # :204-214 updateID in list order
            if ids[i] == -1:
                ids[i] = self.n_id
                self.n_id += 1
        self.ids, self.cnt, self.pts, self.un = ids, cnt, pts, un
        m = np.nonzero(cnt > 1)[0]                                        # feature_tracker_node.cpp:133-150, ascending id
        m = m[np.argsort(ids[m], kind="stable")]
        obs = np.zeros((len(m), 7), np.float64)
        if len(m):
            obs[:, 0:2], obs[:, 2], obs[:, 3:5], obs[:, 5:7] = un[m].astype(np.float64), 1.0, pts[m].astype(np.float64), vel[m].astype(np.float64)
        exp = dict(n=n, n_id=self.n_id, n_msg=len(m), ids=ids.astype(np.int32), track_cnt=cnt.astype(np.int32), cur_xy=pts.copy(), un_xy=un.copy(),
                   vel_xy=vel, msg_id=ids[m].astype(np.int32), msg_obs=obs)
        for key in DIAG:
            exp[key] = out[key]
        return exp


def same_tracks_out(got, exp, what):
    for k in ("n", "n_id", "n_msg") + DIAG:
        assert got[k] == exp[k], (what, k, got[k], exp[k])
    for k in ("ids", "track_cnt", "msg_id"):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], exp[k]), (what, k, got[k], exp[k])
    for k in ("cur_xy", "un_xy", "vel_xy"):
        assert got[k].shape == exp[k].shape and np.array_equal(got[k].view(np.uint32), exp[k].view(np.uint32)), (what, k, got[k], exp[k])
    assert got["msg_obs"].shape == exp["msg_obs"].shape and np.array_equal(got["msg_obs"].view(np.uint64), exp["msg_obs"].view(np.uint64)), (what, "msg_obs")


def same_state(got, exp, what):
    for k in ("n", "n_id"):
        assert got[k] == exp[k], (what, k, got[k], exp[k])
    assert np.float64(got["prev_time"]).view(np.uint64) == np.float64(exp["prev_time"]).view(np.uint64), (what, "prev_time")
    for k in ("ids", "track_cnt", "in_map"):
        assert np.array_equal(got[k], exp[k]), (what, k, got[k], exp[k])
    for k in ("cur_xy", "un_xy"):
        assert np.array_equal(got[k].view(np.uint32), exp[k].view(np.uint32)), (what, k)


def oracle(handle, W, H, cap, streams, min_dist, n_frames, stamp=stamp_of):
    """the existing call with the same walk orders + a TrackBook per stream.  Returns (batch log, expected outputs [k][c], seeds {(k, c):
    tracks_set arguments}, states [k][c] after frame k)"""
    log = run_batch(handle, W, H, cap, streams, min_dist, n_frames)
    books = [TrackBook() for _ in streams]
    exp, seeds, states = [], {}, []
    for k in range(n_frames):
        row = []
        for c, (s, b) in enumerate(zip(streams, books)):
            pts, publish, out = log[k][c]
            if k in s.inject:
                seeds[(k, c)] = b.seed(s.inject[k])
            row.append(b.advance(pts, publish, out, s.use_cb, stamp(c, k)))
        exp.append(row)
        states.append([b.state() for b in books])
    return log, exp, seeds, states


def step_args(streams, k, min_dist, stamp=stamp_of):
    return dict(imgs=[s.frames[k] for s in streams], stamps=[stamp(c, k) for c in range(len(streams))], publish_list=[bool(s.pub(k)) for s in streams],
                intr_list=[s.intr for s in streams], max_cnt=[s.max_cnt for s in streams], min_dist=min_dist, equalize=True,
                f_threshold=[s.f_threshold for s in streams], base_masks=[s.base_mask for s in streams],
                orders=[unstable_like if s.use_cb else None for s in streams])


def resident(handle, W, H, cap, streams, min_dist, n_frames, exp, seeds, what, stamp=stamp_of):
    """tracks_begin, then tracks_step per frame (tracks_set where a stream injects); every output against `exp`"""
    tr = fe.FrontEnd(handle, W, H, len(streams), cap)
    tr.tracks_begin()
    for k in range(n_frames):
        for c in range(len(streams)):
            if (k, c) in seeds:
                tr.tracks_set(c, **seeds[(k, c)])
        outs = tr.tracks_step(**step_args(streams, k, min_dist, stamp))
        for c, o in enumerate(outs):
            same_tracks_out(o, exp[k][c], (what, "stream", c, "frame", k))
    return tr


def run_seven(handle, W=320, H=240, n_frames=5):
    """case 1: the seven streams of tests/fe_read_image_batch_case.py"""
    cap = 160
    streams, min_dist = seven_streams(W, H, n_frames)
    log, exp, seeds, _ = oracle(handle, W, H, cap, streams, min_dist, n_frames)
    # ---- what the oracle side alone must show
    seen = coverage([[log[k][c] for k in range(n_frames)] for c in range(len(streams))])
    check_coverage(seen)
    nonzero = sum(int(np.count_nonzero(np.any(e["vel_xy"] != 0, axis=1))) for row in exp for e in row)
    empty_msg = sum(1 for row in exp for e in row if e["n"] > 0 and e["n_msg"] == 0)
    short_msg = sum(1 for row in exp for e in row if 0 < e["n_msg"] < e["n"])
    assert nonzero >= 20 and empty_msg >= 1 and short_msg >= 1, (nonzero, empty_msg, short_msg)
    assert len(seeds) == 2, seeds.keys()
    resident(handle, W, H, cap, streams, min_dist, n_frames, exp, seeds, "seven")
    return dict(nonzero_velocities=nonzero, empty_messages=empty_msg, short_messages=short_msg, ransac_device=seen["ransac_device"],
                fb_lmeds=seen["fb_lmeds"], fb_collinear=seen["fb_collinear"])


def _long_streams(seeds, max_cnt, n_frames, W=320, H=240):
    return [Stream("long%d" % sd, fe_scene.moving_scene(n_frames, seed=sd, width=W, height=H, velocity=(3.1, -1.4)), INTR, mc,
                   lambda k: k % 3 != 2, callback=(j % 2 == 1)) for j, (sd, mc) in enumerate(zip(seeds, max_cnt))]


def run_long(handle):
    """case 2: lists longer than one pass of the compaction (256) and than 1024 / 4 sort keys; one stream, then three; then lists of
    exactly 64 and 65 entries (the wavefront edge)"""
    W, H, cap, n_frames = 320, 240, 320, 4
    longest = {}
    for name, sds in (("one", (4,)), ("three", (4, 5, 6))):
        streams = _long_streams(sds, [300] * len(sds), n_frames)
        _, exp, seeds, _ = oracle(handle, W, H, cap, streams, LONG_MIN_DIST, n_frames)
        for c in range(len(streams)):
            longest[(name, c)] = max(row[c]["n"] for row in exp)
            assert longest[(name, c)] > 256, ("no list longer than 256 entries", name, c, longest)
        resident(handle, W, H, cap, streams, LONG_MIN_DIST, n_frames, exp, seeds, "long-" + name)
    streams = _long_streams((4, 5), (64, 65), n_frames)
    _, exp, seeds, _ = oracle(handle, W, H, cap, streams, 14, n_frames)
    edge = [max(row[c]["n"] for row in exp) for c in range(2)]
    assert edge == [64, 65], edge
    resident(handle, W, H, cap, streams, 14, n_frames, exp, seeds, "edge")
    return dict(longest=sorted(longest.values()), edge=edge)


def run_reference(handle, tmp_dir):
    """case 3: the reference's own FeatureTracker + updateID (oracle/_ref/libvins_ref_fe.so), MAX_CNT 16"""
    import os
    from oracle import ref_fe as RF
    W, H, n_frames, sc = 320, 240, 8, 320.0 / 752.0
    intr4 = tuple(v * sc for v in (4.616e+02, 4.603e+02, 3.630e+02, 2.481e+02))
    dist = (-2.917e-01, 8.228e-02, 5.333e-05, -1.578e-04)
    cfg = RF.write_config(os.path.join(tmp_dir, "fe_tracks_ref_%d.yaml" % os.getpid()), width=W, height=H, max_cnt=16, min_dist=14, equalize=1, intr=intr4)
    frames = fe_scene.moving_scene(n_frames, seed=4, width=W, height=H, velocity=(3.1, -1.4))
    node = RF.Node(RF.lib(), cfg)
    ref = [node.read_image(1.0 + 0.05 * k, frames[k], k % 3 != 2) for k in range(n_frames)]
    # precondition, on the reference's output alone: the platform's std::sort walked the stable order (the surviving ids keep their
    # relative order from the frame before)
    for k in range(1, n_frames):
        before = {int(i): p for p, i in enumerate(ref[k - 1]["ids"])}
        carried = [before[int(i)] for i in ref[k]["ids"] if int(i) in before]
        assert carried == sorted(carried), "precondition: the reference's std::sort left the stable order in frame %d (not the kernel's fault)" % k
    nonzero = sum(int(np.count_nonzero(np.any(r["pts_velocity"] != 0, axis=1))) for r in ref)
    assert nonzero >= 20, nonzero
    tr = fe.FrontEnd(handle, W, H, 1, 32)
    tr.tracks_begin()
    for k in range(n_frames):
        o = tr.tracks_step([frames[k]], [1.0 + 0.05 * k], [k % 3 != 2], [intr4 + dist], max_cnt=16, min_dist=14, equalize=True, f_threshold=1.0,
                           focal_length=460.0)[0]
        r = ref[k]
        assert o["n_id"] == r["n_id"] and o["n"] == len(r["ids"]), (k, o["n_id"], r["n_id"], o["n"], len(r["ids"]))
        assert np.array_equal(o["ids"], r["ids"]) and np.array_equal(o["track_cnt"], r["track_cnt"]), (k, o["ids"], r["ids"], o["track_cnt"], r["track_cnt"])
        for a, b in (("cur_xy", "cur_pts"), ("un_xy", "cur_un_pts"), ("vel_xy", "pts_velocity")):
            assert np.array_equal(o[a].view(np.uint32), r[b].view(np.uint32)), (k, a, o[a], r[b])
    return dict(nonzero_velocities=nonzero, n_id=ref[-1]["n_id"])


def run_export_and_refusals(handle_a, handle_b, W=320, H=240):
    """case 4: export / re-seed of one stream, every refusal with the step after it, a failing callback, refused re-seeds"""
    cap, n_frames = 160, 5
    streams, min_dist = seven_streams(W, H, n_frames)
    S = len(streams)
    _, exp, seeds, states = oracle(handle_b, W, H, cap, streams, min_dist, n_frames)
    done = []

    def refused(name, fn, code=-1):
        try:
            fn()
        except RuntimeError as e:
            assert status_of(e) == code, (name, str(e))
            done.append(name)
            return
        raise AssertionError("not refused: " + name)

    # ---- refusals: each returns VG_ERR_BAD_ARG and the next valid step is the step of a handle that never saw the refused call
    tr = fe.FrontEnd(handle_a, W, H, S, cap)
    refused("step without begin", lambda: tr.tracks_step(**step_args(streams, 0, min_dist)))
    tr.tracks_begin()
    got3 = None
    for k in range(n_frames):
        a = step_args(streams, k, min_dist)
        if k == 0:
            # a non-empty list on a handle without a previous frame
            tr.tracks_set(2, np.array([[20.0, 20.0]], np.float32), [0], [1], 1)
            refused("list without a previous frame", lambda: tr.tracks_step(**a))
            tr.tracks_set(2, np.zeros((0, 2), np.float32), [], [], 0)
        if k == 2:
            refused("wrong struct_size", lambda: tr.tracks_step(struct_size=8, **a))
            refused("n_streams != n_cams", lambda: tr.tracks_step(n_streams=S - 1, **a))
            bad = dict(a); bad["equalize"] = [c != 3 for c in range(S)]
            refused("mixed equalize", lambda: tr.tracks_step(**bad))
            pubs = [c for c in range(S) if a["publish_list"][c]]
            assert len(pubs) >= 2
            bad = dict(a); bad["min_dist"] = [min_dist + (1 if c == pubs[-1] else 0) for c in range(S)]
            refused("mixed min_dist among publishing streams", lambda: tr.tracks_step(**bad))
            bad = dict(a); bad["imgs"] = [None if c == 5 else f for c, f in enumerate(a["imgs"])]
            refused("frames for some streams only", lambda: tr.tracks_step(**bad))
            bad = dict(a); bad["max_cnt"] = [cap + 1 if c == 1 else m for c, m in enumerate(a["max_cnt"])]
            refused("max_cnt > max_points", lambda: tr.tracks_step(**bad))
        for c in range(S):
            if (k, c) in seeds:
                tr.tracks_set(c, **seeds[(k, c)])
        outs = tr.tracks_step(**a)
        for c, o in enumerate(outs):
            same_tracks_out(o, exp[k][c], ("after refusals", c, k))
        for c in range(S):
            same_state(tr.tracks_get(c), states[k][c], ("tracks_get", c, k))
        if k == 2:
            got3 = tr.tracks_get(0)                     # the list of the first stream after the third frame
    # ---- export / re-seed: a second handle takes stream 0 after frame index 2 and gives frames 3 and 4 of the uninterrupted run
    one = fe.FrontEnd(handle_b, W, H, 1, cap)
    one.push_frames([streams[0].frames[2]], equalize=True)
    one.tracks_begin()
    one.tracks_set(0, got3["cur_xy"], got3["ids"], got3["track_cnt"], got3["n_id"], got3["prev_time"], got3["un_xy"], got3["in_map"])
    same_state(one.tracks_get(0), states[2][0], "re-seeded")
    for k in (3, 4):
        o = one.tracks_step(**step_args(streams[:1], k, min_dist))[0]
        same_tracks_out(o, exp[k][0], ("re-seeded", k))
    # ---- refused re-seeds: the list stays
    before = one.tracks_get(0)
    p3 = np.array([[30.0, 30.0], [60.0, 40.0], [90.0, 50.0]], np.float32)
    refused("duplicate id", lambda: one.tracks_set(0, p3, [4, 7, 4], [1, 1, 1], 9))
    refused("n_id too small", lambda: one.tracks_set(0, p3, [4, 7, 8], [1, 1, 1], 8))
    refused("negative id", lambda: one.tracks_set(0, p3, [4, -1, 8], [1, 1, 1], 9))
    same_state(one.tracks_get(0), before, "after refused re-seeds")
    # ---- a callback that fails on stream 3 of 7: VG_ERR_BAD_ARG, the list of every stream unchanged
    tr = fe.FrontEnd(handle_a, W, H, S, cap)
    tr.tracks_begin()
    for k in range(2):
        for c in range(S):
            if (k, c) in seeds:
                tr.tracks_set(c, **seeds[(k, c)])
        tr.tracks_step(**step_args(streams, k, min_dist))
    a = step_args(streams, 2, min_dist)
    assert a["publish_list"][3] and states[1][3]["n"] > 0

    def failing(cnt):
        raise RuntimeError("the caller's sort failed")

    a["orders"] = [failing if c == 3 else o for c, o in enumerate(a["orders"])]
    refused("callback failure", lambda: tr.tracks_step(**a))
    for c in range(S):
        same_state(tr.tracks_get(c), states[1][c], ("after the failed callback", c))
    return done
