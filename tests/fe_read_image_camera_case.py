"""vg_fe_read_image on a stream with a MEI camera (vg_fe_set_camera) against the SAME frame composed from the step-by-step entry points on
a second handle, as tests/fe_read_image_case.py does for the pinhole: vg_fe_push_frames, vg_fe_track, the border test,
CataCamera::liftProjective restated in NumPy double for rejectWithF's two point sets (fe_camera_case.lift64, held to the reference's
function by tests/test_fe_camera_lift.py), vg_fe_reject_with_f, vg_fe_set_mask, vg_fe_detect_masked, vg_fe_lift.  Every field
bit-identical, for the cameras A (general) and B (xi == 1.0) on four streams each:

  normal        RANSAC on the device, publish every second frame, an unstable-like walk order from the callback
  lmeds         max_cnt 12: 8 <= survivors < 15, the estimate goes back to the host inside the call with the device's lifted points
  few           max_cnt 5: no rejectWithF
  unpublished   a stream that never publishes: tracking, border test and the lifted survivors only

Used by tests/test_fe_read_image_camera.py under the emulator (`not gpu`) and on the device (`gpu`)."""
import numpy as np

from vins_mono_amd import fe

import fe_camera_case as cc
import fe_scene
from fe_read_image_case import FOCAL, _same


def stepwise(tr, W, H, img, cur, cnt, publish, cam, max_cnt, min_dist, equalize, order_fn):
    """one frame from the fine-grained calls; `cam` = (xi, p8).  Returns the dictionary FrontEnd.read_image returns, the new list, its counts"""
    xi, p = cam
    camera = fe.Camera.mei(xi, *p)
    tr.push_frames([img], equalize=equalize)
    cur = np.asarray(cur, np.float32).reshape(-1, 2)
    n = len(cur)
    out = dict(ransac_ran=False, status_f=None, kept=None, new_xy=None)
    if n:
        forw, st, _ = tr.track(0, cur)
        ix, iy = np.rint(forw[:, 0].astype(np.float64)), np.rint(forw[:, 1].astype(np.float64))          # cvRound
        st = (st != 0) & (1 <= ix) & (ix < W - 1) & (1 <= iy) & (iy < H - 1)
    else:
        forw, st = np.zeros((0, 2), np.float32), np.zeros(0, bool)
    out["status_lk"], out["forw_xy"] = st.astype(np.uint8), forw
    cur1, forw1, cnt1 = cur[st], forw[st], np.asarray(cnt, np.int64)[st] + 1
    out["n1"] = out["n2"] = len(forw1)
    if not publish:
        out["n_final"] = len(forw1)
        out["un_xy"] = tr.lift(forw1, camera) if len(forw1) else np.zeros((0, 2), np.float32)
        return out, forw1, cnt1
    if len(forw1) >= 8:                                          # feature_tracker.cpp:176-187: FOCAL_LENGTH * x / z + COL / 2.0
        cx, cy, cz = cc.lift64(cur1, xi, p)
        fx, fy, fz = cc.lift64(forw1, xi, p)
        p1 = np.stack([FOCAL * cx / cz + W / 2.0, FOCAL * cy / cz + H / 2.0], 1).astype(np.float32)
        p2 = np.stack([FOCAL * fx / fz + W / 2.0, FOCAL * fy / fz + H / 2.0], 1).astype(np.float32)
        sf, _ = tr.reject_with_f(p1, p2, 1.0)
        out["ransac_ran"], out["status_f"] = True, sf
        keep = sf != 0
        forw1, cnt1 = forw1[keep], cnt1[keep]
        out["n2"] = len(forw1)
    order = np.asarray(order_fn(cnt1), np.int64) if len(forw1) else np.zeros(0, np.int64)
    pts_o, cnt_o = forw1[order], cnt1[order]
    kept = tr.set_mask([pts_o], [np.arange(len(cnt_o), 0, -1)], min_dist)[0]
    room = max_cnt - len(kept)
    new = tr.detect_masked(0, room, 0.01, float(min_dist)) if room > 0 else np.zeros((0, 2), np.float32)
    final = np.concatenate([pts_o[kept], new]) if len(kept) + len(new) else np.zeros((0, 2), np.float32)
    out.update(kept=np.asarray(kept, np.int32), new_xy=new, n_kept=len(kept), n_new=len(new), n_final=len(final))
    out["un_xy"] = tr.lift(final, camera) if len(final) else np.zeros((0, 2), np.float32)
    return out, final, np.concatenate([cnt_o[kept], np.ones(len(new), np.int64)])


def unstable_like(cnt):
    """a walk order that is NOT the stable one: equal counts in reversed order (what an unstable sort may do)"""
    c = np.asarray(cnt)
    return np.lexsort((-np.arange(len(c)), -c))


def run(handle_a, handle_b, W=320, H=240, n_frames=5, scale=1.0, names="AB"):
    """returns, per camera, what happened (for the caller's assertions on coverage)"""
    cap = 160
    seen = {}
    frames = fe_scene.moving_scene(n_frames, seed=8, width=W, height=H, velocity=(2.7 * W / 320.0, -1.2 * W / 320.0))
    md = lambda v: int(round(v * W / 320.0))
    for name in names:
        cam = cc.params(name, scale)
        s = seen[name] = dict(ransac_device=0, fb_lmeds=0, fb_collinear=0, no_ransac=0, published=0, unpublished=0, lifted=0)
        # (a new vg_fe_configure per stream: both handles start from scratch, and the configure has cleared the camera)

        def stream(what, frames, max_cnt, min_dist, first_pts=None, pub=lambda k: k % 2 == 0):
            one, ref = fe.FrontEnd(handle_a, W, H, 1, cap), fe.FrontEnd(handle_b, W, H, 1, cap)
            one.set_camera(0, fe.Camera.mei(cam[0], *cam[1]))
            pts, cnt = np.zeros((0, 2), np.float32), np.ones(0, np.int64)
            for k, img in enumerate(frames):
                publish = bool(pub(k))
                if k == 1 and first_pts is not None:                         # (points need a previous frame: they come in with the second one)
                    pts = np.asarray(first_pts, np.float32)
                    cnt = np.ones(len(pts), np.int64)

                def cb(st, sf, fw, n2):
                    c = cnt[st != 0] + 1
                    if sf is not None:
                        c = c[sf != 0]
                    assert len(c) == n2
                    return unstable_like(c)

                # (intr: numbers the stream must ignore)
                got = one.read_image(img, pts, publish, (1.0, 1.0, 0.0, 0.0, 0.3, 0.3, 0.3, 0.3), max_cnt=max_cnt, min_dist=min_dist, equalize=True, order=cb)
                want, pts_next, cnt_next = stepwise(ref, W, H, img, pts, cnt, publish, cam, max_cnt, min_dist, True, unstable_like)
                _same(got, want, (name, what, k))
                s["lifted"] += got["n_final"]
                if publish:
                    s["published"] += 1
                    if got["ransac_ran"]:
                        if got["fallback"] & 2: s["fb_lmeds"] += 1
                        elif got["fallback"] & 1: s["fb_collinear"] += 1
                        else: s["ransac_device"] += 1
                    else:
                        s["no_ransac"] += 1
                else:
                    s["unpublished"] += 1
                pts, cnt = pts_next, cnt_next

        stream("normal", frames, 60, md(14))
        stream("lmeds", frames[:4], 12, md(30))
        stream("few", frames[:3], 5, md(40))
        grid = np.array([[x, y] for y in np.arange(0.15, 0.9, 0.2) * H for x in np.arange(0.1, 0.95, 0.12) * W], np.float32)
        stream("unpublished", frames[:4], 60, md(14), first_pts=grid, pub=lambda k: False)
    return seen


def check(seen, names="AB"):
    for name in names:
        s = seen[name]
        assert s["ransac_device"] >= 1 and s["fb_lmeds"] >= 1 and s["no_ransac"] >= 3 and s["unpublished"] >= 5 and s["lifted"] > 200, (name, s)
    return True
