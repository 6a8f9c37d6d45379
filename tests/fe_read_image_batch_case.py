"""vg_fe_read_image_batch (readImage of every stream of a handle in one call) against vg_fe_read_image on a single-stream handle, which
tests/test_fe_read_image.py holds to the step-by-step calls and those to the oracle.  EVERY field of every vg_fe_frame_out of the batch must
be identical to what the single-stream handle returns for that stream on the same frames: counts, ransac_ran, status_lk, status_f, kept,
ransac_best, ransac_niters, fallback and the bit patterns of forw_xy, new_xy, un_xy.  No tolerance, no stream left out.

The batch runs first, over all frames; then the streams are replayed ONE AFTER THE OTHER on one single-stream handle (re-configured per
stream), each from its own evolving point list, and every frame is compared -- so 256 streams need two handles, not 257.

Used by tests/test_fe_read_image_batch.py under the emulator (`not gpu`) and on the device (`gpu`)."""
import numpy as np

from vins_mono_amd import fe

import fe_scene
from fe_read_image_case import INTR, INTR_PLAIN

RB_CHUNK0 = 63          # csrc/fe_layout.h: RANSAC iterations the batched call evaluates before its bookkeeping first looks

SCALARS = ("n1", "n2", "ransac_ran", "n_kept", "n_new", "n_final", "ransac_best", "ransac_niters", "fallback")


def same_all(a, b, what):
    """every field of two read_image dictionaries"""
    for k in SCALARS:
        assert a[k] == b[k], (what, k, a[k], b[k])
    for k in ("status_lk", "status_f", "kept"):
        assert (a[k] is None) == (b[k] is None), (what, k)
        if a[k] is not None:
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (what, k, a[k], b[k])
    for k in ("forw_xy", "new_xy", "un_xy"):
        assert (a[k] is None) == (b[k] is None), (what, k)
        if a[k] is not None:
            assert a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (what, k)


def unstable_like(cnt):
    """a walk order that is NOT the stable one: equal counts in reversed order (what an unstable sort may do)"""
    c = np.asarray(cnt)
    return np.lexsort((-np.arange(len(c)), -c))


class Stream:
    """the caller's side of one stream: the point list with its track counts, kept as FeatureTracker keeps them"""

    def __init__(self, name, frames, intr, max_cnt, pub, callback=True, base_mask=None, inject=None, fail_at=None, f_threshold=1.0):
        self.name, self.frames, self.intr, self.max_cnt, self.pub, self.f_threshold = name, frames, intr, max_cnt, pub, f_threshold
        self.use_cb, self.base_mask, self.inject, self.fail_at = callback, base_mask, inject or {}, fail_at
        self.reset()

    def reset(self):
        self.pts, self.cnt, self.k, self._order = np.zeros((0, 2), np.float32), np.zeros(0, np.int64), 0, None

    def begin(self, k):
        """the inputs of frame k: (img, cur_pts, publish)"""
        self.k = k
        if k in self.inject:                              # a point list handed in from outside (as a caller that re-seeds its tracks)
            self.pts = np.asarray(self.inject[k], np.float32)
            self.cnt = np.ones(len(self.pts), np.int64)
        self._order = None
        return self.frames[k], self.pts, bool(self.pub(k))

    def order(self):
        return self._cb if self.use_cb else None

    def _cb(self, st, sf, fw, n2):
        if self.fail_at == self.k:
            raise RuntimeError("the caller's sort failed")
        c = self.cnt[st != 0] + 1
        if sf is not None:
            c = c[sf != 0]
        assert len(c) == n2
        self._order = unstable_like(c)
        return self._order

    def advance(self, out, publish):
        st = out["status_lk"] != 0
        forw, cnt = out["forw_xy"][st], self.cnt[st] + 1
        if publish:
            if out["ransac_ran"]:
                keep = out["status_f"] != 0
                forw, cnt = forw[keep], cnt[keep]
            order = self._order if self._order is not None else np.arange(len(forw))
            forw, cnt = forw[order][out["kept"]], cnt[order][out["kept"]]
            forw = np.concatenate([forw, out["new_xy"]]) if len(forw) + len(out["new_xy"]) else np.zeros((0, 2), np.float32)
            cnt = np.concatenate([cnt, np.ones(len(out["new_xy"]), np.int64)])
        assert len(forw) == out["n_final"]
        self.pts, self.cnt = forw.astype(np.float32), cnt


def seven_streams(W, H, n_frames):
    """one stream of each kind tests/fe_read_image_case.py builds, advancing together; different scenes, cameras, MAX_CNT and publish
    patterns, one MIN_DIST and EQUALIZE (the batched call wants those uniform).  Two streams have a tight F_THRESHOLD: few inliers, so the
    iteration bound of their RANSAC stays in the hundreds or at 1000 and the second part of the batched estimate has work to do (the
    threshold is in pixels of rejectWithF's virtual camera, whose focal length is fixed: the same tracking noise in image pixels is 1 / sc
    of it there, so the threshold scales with 1 / sc to keep the inlier ratio)."""
    sc = W / 320.0
    cam = lambda base, c: tuple(v * (sc if i < 4 else 1.0) * (1.0 + 0.004 * c if i < 2 else 1.0) for i, v in enumerate(base))
    scene = lambda c: fe_scene.moving_scene(n_frames, seed=4 + c, width=W, height=H, velocity=(3.1 - 0.3 * c, -1.4 + 0.2 * c))
    yy, xx = np.mgrid[0:H, 0:W]
    fish = np.where((xx - W / 2) ** 2 + (yy - H / 2) ** 2 < (0.55 * H) ** 2, 255, 0).astype(np.uint8)
    grid = np.array([[x * sc, y * sc] for y in (50.0, 90.0, 130.0, 170.0) for x in np.arange(30.0, 290.0, 20.0)], np.float32)
    gone = np.array([[0.2, 0.3], [W - 0.6, H - 0.7], [0.4, H - 0.8]], np.float32)
    every = lambda k: True
    return [
        Stream("normal", scene(0), cam(INTR, 0), 60, lambda k: k % 2 == 0, f_threshold=0.2 / sc),
        Stream("fisheye", scene(1), cam(INTR, 1), 50, every, base_mask=fish),
        Stream("no-callback", scene(2), cam(INTR, 2), 40, lambda k: k % 3 != 2, callback=False, f_threshold=0.08 / sc),
        Stream("lmeds", scene(3), cam(INTR, 3), 12, every),
        Stream("few", scene(4), cam(INTR, 4), 5, every),
        # cur_pts on four image rows, a camera without distortion: three points of a row stay exactly collinear after the lifting
        Stream("collinear", scene(5), cam(INTR_PLAIN, 0), 70, every, inject={1: grid}),
        # points that all leave the image / fail: nothing survives the tracking on a published frame
        Stream("none", scene(6), cam(INTR, 6), 30, every, inject={1: gone}),
    ], int(round(14 * sc))


def run_batch(handle, W, H, cap, streams, min_dist, n_frames, equalize=True, resident=False):
    """all frames through vg_fe_read_image_batch; returns per frame the list of (inputs, output) per stream"""
    tr = fe.FrontEnd(handle, W, H, len(streams), cap)
    for s in streams:
        s.reset()
    log = []
    for k in range(n_frames):
        ins = [s.begin(k) for s in streams]
        if resident:
            tr.upload_frames([i[0] for i in ins])
        outs = tr.read_image_batch(None if resident else [i[0] for i in ins], [i[1] for i in ins], [i[2] for i in ins], [s.intr for s in streams],
                                   max_cnt=[s.max_cnt for s in streams], min_dist=min_dist, equalize=equalize,
                                   f_threshold=[s.f_threshold for s in streams],
                                   base_masks=[s.base_mask for s in streams], orders=[s.order() for s in streams])
        for s, i, o in zip(streams, ins, outs):
            s.advance(o, i[2])
        log.append([(i[1].copy(), i[2], o) for i, o in zip(ins, outs)])
    return log


def run_single(handle, W, H, cap, stream, min_dist, n_frames, equalize=True):
    """the same frames of ONE stream through vg_fe_read_image on a single-stream handle"""
    one = fe.FrontEnd(handle, W, H, 1, cap)
    stream.reset()
    log = []
    for k in range(n_frames):
        img, pts, publish = stream.begin(k)
        o = one.read_image(img, pts, publish, stream.intr, max_cnt=stream.max_cnt, min_dist=min_dist, equalize=equalize, f_threshold=stream.f_threshold,
                           base_mask=stream.base_mask, order=stream.order())
        stream.advance(o, publish)
        log.append((pts.copy(), publish, o))
    return log


def coverage(single_logs):
    """what the single-stream side went through (the batch is held to it field by field, so it went through the same)"""
    seen = dict(ransac_device=0, niters=[], fb_lmeds=0, fb_collinear=0, published_no_ransac=0, no_input=0, mixed_steps=0)
    n_frames = len(single_logs[0])
    for k in range(n_frames):
        pubs = {log[k][1] for log in single_logs}
        seen["mixed_steps"] += 1 if len(pubs) == 2 else 0
    for log in single_logs:
        for pts, publish, o in log:
            seen["no_input"] += 1 if len(pts) == 0 else 0
            if not publish:
                continue
            if not o["ransac_ran"]:
                seen["published_no_ransac"] += 1
            elif o["fallback"] & 2:
                seen["fb_lmeds"] += 1
            elif o["fallback"] & 1:
                seen["fb_collinear"] += 1
            else:
                seen["ransac_device"] += 1
                seen["niters"].append(o["ransac_niters"])
    return seen


def check_coverage(seen):
    assert seen["ransac_device"] >= 4 and sum(1 for v in seen["niters"] if 0 <= v < 1000) >= 4, seen
    # (a final bound above RB_CHUNK0: the iterations from RB_CHUNK0 on were evaluated by the second part of the batched estimate)
    assert any(v > RB_CHUNK0 for v in seen["niters"]), seen
    assert seen["fb_lmeds"] >= 1 and seen["fb_collinear"] >= 1 and seen["published_no_ransac"] >= 2, seen
    assert seen["no_input"] >= 1 and seen["mixed_steps"] >= 1, seen


def compare(batch_log, single_logs, what=""):
    for c, log in enumerate(single_logs):
        for k, (pts, publish, o) in enumerate(log):
            bp, bpub, bo = batch_log[k][c]
            assert bpub == publish and np.array_equal(bp.view(np.uint32), pts.view(np.uint32)), (what, c, k, "inputs")
            same_all(bo, o, (what, c, k))


def run(handle_batch, handle_single, W=320, H=240, n_frames=5):
    """the seven-stream case; returns the coverage"""
    cap = 160
    streams, min_dist = seven_streams(W, H, n_frames)
    batch_log = run_batch(handle_batch, W, H, cap, streams, min_dist, n_frames)
    single_logs = [run_single(handle_single, W, H, cap, s, min_dist, n_frames) for s in streams]
    compare(batch_log, single_logs, "seven")
    seen = coverage(single_logs)
    # resident frames: imgs=None after upload_frames gives what the call that uploads gives
    res_log = run_batch(handle_batch, W, H, cap, streams, min_dist, min(n_frames, 2), resident=True)
    compare(res_log, [log[:len(res_log)] for log in single_logs], "resident")
    seen["resident_frames"] = len(res_log)
    return seen


def status_of(exc):
    """the vg_status in the message of the binding's RuntimeError"""
    msg = str(exc)
    return int(msg.split("status ")[1].split(":")[0])


def run_refusals(handle_a, handle_b, W=320, H=240):
    """every refusal returns its code, and the NEXT valid call returns what it returns on a handle that never saw the refused call"""
    cap, n_frames = 160, 3
    streams, min_dist = seven_streams(W, H, n_frames)
    S = len(streams)
    clean = run_batch(handle_b, W, H, cap, streams, min_dist, n_frames)
    intr = [s.intr for s in streams]
    mc = [s.max_cnt for s in streams]
    refused = []

    def args(k):
        ins = [s.begin(k) for s in streams]
        return ins, dict(imgs=[i[0] for i in ins], cur_pts_list=[i[1] for i in ins], publish_list=[i[2] for i in ins], intr_list=intr,
                         max_cnt=mc, min_dist=min_dist, equalize=True, f_threshold=[s.f_threshold for s in streams], base_masks=[s.base_mask for s in streams], orders=[s.order() for s in streams])

    def refuse(tr, name, code, **kw):
        try:
            tr.read_image_batch(**kw)
        except RuntimeError as e:
            assert status_of(e) == code, (name, str(e))
            refused.append(name)
            return
        raise AssertionError("not refused: " + name)

    tr = fe.FrontEnd(handle_a, W, H, S, cap)
    for s in streams:
        s.reset()
    # before the first frame: points on a stream without a previous frame
    ins, a = args(0)
    bad = dict(a)
    bad["cur_pts_list"] = [np.array([[20.0, 20.0]], np.float32) if c == 2 else p for c, p in enumerate(a["cur_pts_list"])]
    refuse(tr, "points without a previous frame", -1, **bad)
    for k in range(n_frames):
        ins, a = args(k)
        if k == 1:
            refuse(tr, "n_streams != n_cams", -1, n_streams=S - 1, **a)
            bad = dict(a)
            bad["cur_pts_list"] = [np.full((cap + 1, 2), 30.0, np.float32) if c == 4 else p for c, p in enumerate(a["cur_pts_list"])]
            refuse(tr, "n > max_points", -1, **bad)
            bad = dict(a)
            bad["equalize"] = [c != 3 for c in range(S)]
            refuse(tr, "mixed equalize", -1, **bad)
            pubs = [c for c in range(S) if a["publish_list"][c]]
            assert len(pubs) >= 2
            bad = dict(a)
            bad["min_dist"] = [min_dist + (1 if c == pubs[-1] else 0) for c in range(S)]
            refuse(tr, "mixed min_dist among publishing streams", -1, **bad)
            bad = dict(a)
            bad["imgs"] = [None if c == 5 else f for c, f in enumerate(a["imgs"])]
            refuse(tr, "some-but-not-all img NULL", -1, **bad)
        outs = tr.read_image_batch(**a)
        for c, (s, i, o) in enumerate(zip(streams, ins, outs)):
            same_all(o, clean[k][c][2], ("after refusals", c, k))
            s.advance(o, i[2])
    assert len(refused) == 6, refused
    # a callback that fails on stream 3 of 7: VG_ERR_BAD_ARG, the caller's point lists untouched
    tr = fe.FrontEnd(handle_a, W, H, S, cap)
    for s in streams:
        s.reset()
    for k in range(2):
        ins, a = args(k)
        outs = tr.read_image_batch(**a)
        for s, i, o in zip(streams, ins, outs):
            s.advance(o, i[2])
    ins, a = args(2)
    assert a["publish_list"][3] and len(a["cur_pts_list"][3]) > 0
    before = [(s.pts.copy(), s.cnt.copy()) for s in streams]
    streams[3].fail_at = 2
    try:
        refuse(tr, "callback failure", -1, **a)
    finally:
        streams[3].fail_at = None
    for s, (p, c) in zip(streams, before):
        assert np.array_equal(s.pts.view(np.uint32), p.view(np.uint32)) and np.array_equal(s.cnt, c), s.name
    return refused


def run_headline(handle_batch, handle_single, S=256, W=752, H=480, max_cnt=150):
    """256 streams, 150 points, CLAHE on, two frames: no points / the first frame's corners, both published"""
    from vins_mono_amd import synth
    intr = (461.6, 460.3, 363.0, 248.1, -2.917e-01, 8.228e-02, 5.333e-05, -1.578e-04)
    first = [synth.synth_frame(3 + c) for c in range(S)]
    frames = [[first[c], synth.warp_frame(first[c], 4 + c)] for c in range(S)]
    streams = [Stream("s%d" % c, frames[c], intr, max_cnt, lambda k: True, callback=(c % 2 == 0)) for c in range(S)]
    batch_log = run_batch(handle_batch, W, H, max_cnt, streams, 30, 2)
    ransac = 0
    for c, s in enumerate(streams):
        log = run_single(handle_single, W, H, max_cnt, s, 30, 2)
        for k, (pts, publish, o) in enumerate(log):
            bp, bpub, bo = batch_log[k][c]
            assert np.array_equal(bp.view(np.uint32), pts.view(np.uint32)), (c, k, "inputs")
            same_all(bo, o, ("headline", c, k))
        ransac += 1 if log[1][2]["ransac_ran"] and not log[1][2]["fallback"] else 0
    return dict(streams=S, ransac_device=ransac)
