"""vg_kf_* (keyframe BRIEF descriptors and matching for the pose graph): the NumPy reference, the cases and the check bodies.
tests/test_kf_brief_simt.py runs the bodies through the fiber emulator, tests/test_kf_brief_gpu.py on the MI355X.

The reference holds the four definitions of include/vinsgpu.h written out directly (every arc of FAST, every pair of the match), not the
kernels' shortcuts.  Everything is integer or float32-exact: every comparison below is for equality.

cv::GaussianBlur and cv::FAST are recalled, not pinned; the keypoint counts of tests/fe_scene.moving_scene under the FAST definition are
asserted here (COUNTS), so that a drifting restatement shows.

The rendered match (frame 0's corners as window points against frame 1's record, 100 x 70): the reference alone gives N_RENDERED matches,
above MIN_LOOP_NUM = 25 (119 of 133 window points)."""
import ctypes as C
import os
import subprocess

import numpy as np

import fe_camera_case as mei_case
import fe_kb_case as kb_case
import fe_read_image_case as pin_case
import fe_scene
from vins_mono_amd import fe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERN_FILE = os.path.join(ROOT, "tests", "golden", "brief_pattern.yml")
MIN_LOOP_NUM = 25
TAPS = np.array([7, 17, 32, 46, 52, 46, 32, 17, 7], np.int64)
RING = ((0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3), (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1), (-2, -2), (-1, -3))
# (width, height): keypoints of frame 0, of frame 1, pixels passing the corner test before suppression in frame 0 (None: not recorded)
COUNTS = {(752, 480): (6750, 4930, 31280), (100, 70): (133, 88, None), (67, 41): (29, 27, None)}
BAD_ARG = -1

_pattern = None
_frames = {}
_ref = {}


def pattern():
    global _pattern
    if _pattern is None:
        _pattern = fe.read_brief_pattern(PATTERN_FILE)
        assert _pattern.shape == (4, 256)
    return _pattern


def frames(size):
    """the first two frames of fe_scene.moving_scene at (width, height), rendered once"""
    if size not in _frames:
        _frames[size] = fe_scene.moving_scene(2, width=size[0], height=size[1])
    return _frames[size]


# ---- the definitions ---------------------------------------------------------------------------------------------------------------------
def reflect101(i, n):
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * n - 2 - i, i)


def blur(img):
    H, W = img.shape
    p = img.astype(np.int64)
    xs = reflect101(np.arange(-4, W + 4), W)
    ys = reflect101(np.arange(-4, H + 4), H)
    rows = sum(TAPS[i] * p[:, xs[i:i + W]] for i in range(9))
    assert rows.max() < 65536
    tot = sum(TAPS[j] * rows[ys[j:j + H], :] for j in range(9))
    return ((tot + 32768) >> 16).astype(np.uint8)


def fast_scores(img):
    """the score map (0 where the pixel is no corner) and the number of pixels that pass the corner test"""
    H, W = img.shape
    p = img.astype(np.int32)
    v = p[3:H - 3, 3:W - 3]
    d = np.stack([v - p[3 + dy:H - 3 + dy, 3 + dx:W - 3 + dx] for dx, dy in RING])
    A = np.full(v.shape, -256, np.int32)
    B = np.full(v.shape, -256, np.int32)
    for s in range(16):
        arc = d[[(s + j) % 16 for j in range(9)]]
        A = np.maximum(A, arc.min(0))
        B = np.maximum(B, (-arc).min(0))
    m = np.maximum(A, B)
    score = np.zeros((H, W), np.int32)
    score[3:H - 3, 3:W - 3] = np.where(m > 20, m - 1, 0)
    return score, int((m > 20).sum())


def fast(img):
    """(pt float32 [n, 2], score uint8 [n]) in row-major order, and the count before suppression"""
    score, n_pass = fast_scores(img)
    H, W = score.shape
    q = np.pad(score, 1)
    keep = score > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                keep &= score > q[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    ys, xs = np.nonzero(keep)                                   # row-major: y ascending, then x
    return np.stack([xs, ys], 1).astype(np.float32), score[ys, xs].astype(np.uint8), n_pass


def brief(blurred, pts, pat=None):
    """DVision::BRIEF::compute on the blurred image: uint64 [n, 4]"""
    pat = pattern() if pat is None else pat
    H, W = blurred.shape
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    f = pat.astype(np.float32)
    with np.errstate(all="ignore"):
        c = [np.trunc(pts[:, k % 2, None] + f[k][None, :]) for k in range(4)]          # float32 add, truncation toward zero
    inside = np.ones((len(pts), 256), bool)
    for k, lim in ((0, W), (1, H), (2, W), (3, H)):
        inside &= (c[k] >= 0) & (c[k] < lim)
    ci = [np.where(inside, v, 0).astype(np.int64) for v in c]
    bits = inside & (blurred[ci[1], ci[0]] < blurred[ci[3], ci[2]])
    w = bits.reshape(len(pts), 4, 64).astype(np.uint64) << np.arange(64, dtype=np.uint64)[None, None, :]
    return np.bitwise_or.reduce(w, axis=2)


def lift(pts, cam):
    """keypoints_norm: (float)(x / z), (float)(y / z) of the camera's liftProjective; cam = ('pinhole', p8) | ('mei', xi, p8) | ('kb', p8)"""
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    if len(pts) == 0:
        return np.zeros((0, 2), np.float32)
    if cam[0] == "pinhole":
        x, y = pin_case.lift64(pts, cam[1])
        return np.stack([x, y], 1).astype(np.float32)
    if cam[0] == "mei":
        x, y, z = mei_case.lift64(pts, cam[1], cam[2])
        return np.stack([x / z, y / z], 1).astype(np.float32)
    return kb_case.lifted_xy(pts, cam[1])


def camera_struct(cam):
    if cam[0] == "pinhole":
        return fe.Camera.pinhole(*cam[1])
    if cam[0] == "mei":
        return fe.Camera.mei(cam[1], *cam[2])
    return fe.Camera.kannala_brandt(*cam[1])


def cameras(width):
    """the three models scaled to a frame of that width"""
    s = width / 752.0
    pin = tuple(v * s for v in (461.6, 460.3, 363.0, 248.1)) + (-2.917e-01, 8.228e-02, 5.333e-05, -1.578e-04)
    xi, pm = mei_case.params("A", width / 320.0)
    return {"pinhole": ("pinhole", pin), "mei": ("mei", xi, pm), "kb": ("kb", kb_case.params("cla", width))}


_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def hamming(a, b):
    """popcount of the xor of every pair: int32 [len(a), len(b)]"""
    a8 = np.ascontiguousarray(a, np.uint64).reshape(-1, 4).view(np.uint8).reshape(-1, 1, 32)
    b8 = np.ascontiguousarray(b, np.uint64).reshape(-1, 4).view(np.uint8).reshape(1, -1, 32)
    out = np.zeros((a8.shape[0], b8.shape[1]), np.int32)
    for lo in range(0, a8.shape[0], 16):
        out[lo:lo + 16] = _POP[a8[lo:lo + 16] ^ b8].sum(-1)
    return out


def match(wdesc, odesc, opt, onorm):
    """searchByBRIEFDes + reduceVector"""
    nw, nk = len(wdesc), len(odesc)
    idx, dist = np.full(nw, -1, np.int32), np.full(nw, 128, np.int32)
    if nw and nk:
        d = hamming(wdesc, odesc)
        for w in range(nw):
            best_d, best_i = 128, -1
            cand = np.nonzero(d[w] < 128)[0]
            if len(cand):
                best_i = int(cand[np.argmin(d[w][cand])])           # (argmin: the first, i.e. lowest, index of the smallest distance)
                best_d = int(d[w][best_i])
            idx[w], dist[w] = best_i, best_d
    status = ((idx >= 0) & (dist < 80)).astype(np.uint8)
    m = np.zeros((nw, 2), np.float32)
    mn = np.zeros((nw, 2), np.float32)
    on = status != 0
    m[on], mn[on] = np.asarray(opt, np.float32).reshape(-1, 2)[idx[on]], np.asarray(onorm, np.float32).reshape(-1, 2)[idx[on]]
    keep = np.nonzero(on)[0].astype(np.int32)
    return {"n_window": nw, "n_matched": len(keep), "best_idx": idx, "best_dist": dist, "status": status, "matched_2d_old": m,
            "matched_2d_old_norm": mn, "matched_index": keep, "matched_old_xy": m[keep], "matched_old_norm": mn[keep]}


def keyframe(img, cam, window_xy, max_keypoints=None, pat=None):
    """the record the reference's KeyFrame holds for this image (cached per image identity by the callers)"""
    pts, sc, n_pass = fast(img)
    n_true = len(pts)
    if max_keypoints is not None and n_true > max_keypoints:
        pts, sc = pts[:max_keypoints], sc[:max_keypoints]
    b = blur(img)
    w = np.asarray(window_xy, np.float32).reshape(-1, 2)
    return {"n_keypoints": n_true, "status": fe.KF_TRUNCATED if len(pts) < n_true else fe.KF_OK, "n_kept": len(pts), "keypoints": pts, "scores": sc,
            "norm": lift(pts, cam), "descriptors": brief(b, pts, pat), "window_descriptors": brief(b, w, pat), "n_pass": n_pass, "blur": b}


def scene_ref(size, k, cam_name="pinhole"):
    """the reference record of frame k of the scene at `size`, without window points; computed once"""
    key = (size, k, cam_name)
    if key not in _ref:
        r = keyframe(frames(size)[k], cameras(size[0])[cam_name], np.zeros((0, 2), np.float32))
        want = COUNTS[size]
        assert r["n_keypoints"] == want[k], (size, k, r["n_keypoints"])
        if k == 0 and want[2] is not None:
            assert r["n_pass"] == want[2], (size, r["n_pass"])
        _ref[key] = r
    return _ref[key]


# ---- comparisons ------------------------------------------------------------------------------------------------------------------------
def bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_record(got, ref, what, window=True):
    assert got["n_keypoints"] == ref["n_keypoints"] and got["status"] == ref["status"], (what, got["n_keypoints"], ref["n_keypoints"], got["status"])
    assert np.array_equal(got["keypoints"], ref["keypoints"]), what + ": keypoints"
    assert np.array_equal(got["scores"], ref["scores"]), what + ": scores"
    assert np.array_equal(got["descriptors"], ref["descriptors"]), what + ": descriptors"
    assert np.array_equal(bits32(got["norm"]), bits32(ref["norm"])), what + ": norms"
    if window:
        assert np.array_equal(got["window_descriptors"], ref["window_descriptors"]), what + ": window descriptors"


MATCH_KEYS = ("best_idx", "best_dist", "status", "matched_index")
MATCH_FLOATS = ("matched_2d_old", "matched_2d_old_norm", "matched_old_xy", "matched_old_norm")


def same_match(got, ref, what):
    assert got["n_window"] == ref["n_window"] and got["n_matched"] == ref["n_matched"], (what, got["n_matched"], ref["n_matched"])
    for k in MATCH_KEYS:
        assert np.array_equal(got[k], ref[k]), f"{what}: {k}"
    for k in MATCH_FLOATS:
        assert np.array_equal(bits32(got[k]), bits32(ref[k])), f"{what}: {k}"


def same_get(a, b, what):
    assert set(a) == set(b)
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), f"{what}: {k}"


def device_lift(handle, pts, cam):
    """vg_fe_lift on the same points (a front end of its own size: the lift does not depend on it)"""
    tr = fe.FrontEnd(handle, 320, 240, 1, 1024)
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    out = [tr.lift(pts[lo:lo + 1024], camera_struct(cam)) for lo in range(0, len(pts), 1024)]
    return np.concatenate(out) if out else np.zeros((0, 2), np.float32)


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
def window_points(size, n, seed=1):
    """n window points: the pattern-reach and truncation cases first, then fractional coordinates all over the frame (and a little outside)"""
    W, H = size
    fixed = [(0.25, 0.25), (W - 0.75, H - 0.75), (-200.0, -200.0), (-0.5, 10.5), (W / 2 + 0.5, H / 2 + 0.25), (W - 1.0, 0.0), (0.0, H - 1.0),
             (-0.99, -0.99), (W + 30.5, H / 2.0)]
    rng = np.random.default_rng(seed)
    rnd = np.stack([rng.uniform(-2, W + 2, max(n, 1)), rng.uniform(-2, H + 2, max(n, 1))], 1)
    return np.concatenate([np.array(fixed), rnd]).astype(np.float32)[:n]


def check_frame(handle, size, cam_name="pinhole", n_window=9, max_window=150):
    """both frames of the scene at `size` in one call: the record of each against the reference, through vg_kf_add's arrays and vg_kf_get"""
    cam = cameras(size[0])[cam_name]
    refs = [scene_ref(size, k, cam_name) for k in (0, 1)]
    mk = max(r["n_keypoints"] for r in refs)
    kf = fe.KeyFrames(handle, size[0], size[1], mk, max_window, 3, pattern())
    w = window_points(size, n_window)
    got = kf.add([2, 0], frames(size), [camera_struct(cam)] * 2, [w, w[:1]])
    for k in (0, 1):
        ref = dict(refs[k], window_descriptors=brief(refs[k]["blur"], w if k == 0 else w[:1]))
        same_record(got[k], ref, f"{size} frame {k}")
        rec = kf.get((2, 0)[k])
        assert rec["n_true"] == ref["n_keypoints"] and np.array_equal(rec["window_xy"], w if k == 0 else w[:1])
        for key in ("keypoints", "scores", "descriptors", "window_descriptors"):
            assert np.array_equal(rec[key], ref[key]), key
        assert np.array_equal(bits32(rec["norm"]), bits32(ref["norm"]))
    # the points whose tests all fall outside: a descriptor of 0; the norms against vg_fe_lift on the same points
    assert not got[0]["window_descriptors"][2].any() and got[0]["window_descriptors"][0].any()
    assert np.array_equal(bits32(got[0]["norm"]), bits32(device_lift(handle, got[0]["keypoints"], cam)))
    return got


def check_wide_pattern(handle, size=(100, 70)):
    """the shipped pattern reaches 24 pixels; two others that reach 96 and 32 (more of the tests leave the frame), against the reference"""
    cam = cameras(size[0])["pinhole"]
    w = window_points(size, 12)
    for scale in (4, None):
        pat = pattern() * 4 if scale else np.clip(pattern().astype(np.int32) * 32 // 24, -32, 32).astype(np.int16)
        assert np.abs(pat).max() == (96 if scale else 32)
        ref = keyframe(frames(size)[0], cam, w, pat=pat)
        kf = fe.KeyFrames(handle, size[0], size[1], ref["n_keypoints"], 12, 1, pat)
        same_record(kf.add([0], [frames(size)[0]], [camera_struct(cam)], [w])[0], ref, f"pattern reach {np.abs(pat).max()}")


def border_frame(size, seed=3):
    """0 / 255 structure in the outermost 4 rows and columns (each row and column of the band its own pattern), noise inside"""
    W, H = size
    rng = np.random.default_rng(seed)
    img = rng.integers(90, 160, (H, W)).astype(np.uint8)
    band = (rng.integers(0, 2, (H, W)) * 255).astype(np.uint8)
    m = np.zeros((H, W), bool)
    m[:4], m[-4:], m[:, :4], m[:, -4:] = True, True, True, True
    img[m] = band[m]
    return img


def check_blur_border(handle, size=(67, 41)):
    """a wrong reflection changes the blurred band, hence the descriptors of points whose tests read it: a grid of window points over the
    band and the frame, compared bit for bit"""
    W, H = size
    img = border_frame(size)
    g = np.array([[x + 0.5, y + 0.25] for y in list(range(0, 8)) + list(range(H - 8, H)) + [H // 2] for x in range(0, W, 3)], np.float32)[:150]
    cam = cameras(W)["pinhole"]
    ref = keyframe(img, cam, g)
    b, naive = ref["blur"], blur(np.pad(img, 4, mode="edge"))[4:-4, 4:-4]
    assert (b != naive).sum() > 20, "the case does not tell the border modes apart"
    kf = fe.KeyFrames(handle, W, H, max(ref["n_keypoints"], 1), 150, 1, pattern())
    got = kf.add([0], [img], [camera_struct(cam)], [g])[0]
    same_record(got, ref, "border frame")


def check_window_counts(handle, size=(67, 41), max_window=70):
    """n_window of 0, 1, 64, 65 and max_window_points"""
    cam = cameras(size[0])["pinhole"]
    ref0 = scene_ref(size, 0)
    kf = fe.KeyFrames(handle, size[0], size[1], ref0["n_keypoints"], max_window, 5, pattern())
    ns = (0, 1, 64, 65, max_window)
    ws = [window_points(size, n, seed=2) for n in ns]
    got = kf.add(list(range(5)), [frames(size)[0]] * 5, [camera_struct(cam)] * 5, ws)
    for n, w, g in zip(ns, ws, got):
        assert len(g["window_descriptors"]) == n
        same_record(g, dict(ref0, window_descriptors=brief(ref0["blur"], w)), f"n_window {n}")


def plateau_frame(size=(67, 41)):
    """a bright 2 x 2 block on a dark ground: its four pixels pass the corner test with equal scores, none survives the strict comparison;
    beside it single bright pixels at row 3, column 3, row H - 4 and column W - 4, which are corners"""
    W, H = size
    img = np.full((H, W), 40, np.uint8)
    img[20:22, 30:32] = 200
    for x, y in ((12, 3), (3, 12), (50, H - 4), (W - 4, 25)):
        img[y, x] = 220
    return img


def check_fast_cases(handle, size=(67, 41)):
    W, H = size
    cam = cameras(W)["pinhole"]
    none = np.zeros((0, 2), np.float32)
    kf = fe.KeyFrames(handle, W, H, 16, 4, 2, pattern())
    flat = np.full((H, W), 77, np.uint8)
    got = kf.add([0], [flat], [camera_struct(cam)], [none])[0]
    assert got["n_keypoints"] == 0 and got["status"] == fe.KF_OK and len(got["keypoints"]) == 0
    img = plateau_frame(size)
    ref = keyframe(img, cam, none)
    score, n_pass = fast_scores(img)
    assert n_pass >= 8 and score[20, 30] == score[20, 31] == score[21, 30] == score[21, 31] > 0
    pts = {tuple(p) for p in ref["keypoints"].astype(int).tolist()}
    assert pts == {(12, 3), (3, 12), (50, H - 4), (W - 4, 25)}, pts
    same_record(kf.add([1], [img], [camera_struct(cam)], [none])[0], ref, "plateau frame")


def check_cap(handle, size=(67, 41)):
    """max_keypoints equal to the frame's count (OK) and one less (VG_KF_TRUNCATED, the true count, the kept prefix)"""
    cam = cameras(size[0])["pinhole"]
    full = scene_ref(size, 0)
    n = full["n_keypoints"]
    none = np.zeros((0, 2), np.float32)
    for cap, status in ((n, fe.KF_OK), (n - 1, fe.KF_TRUNCATED)):
        kf = fe.KeyFrames(handle, size[0], size[1], cap, 4, 1, pattern())
        got = kf.add([0], [frames(size)[0]], [camera_struct(cam)], [none])[0]
        ref = dict(full, status=status, **{k: full[k][:cap] for k in ("keypoints", "scores", "norm", "descriptors")})
        same_record(got, ref, f"cap {cap}")
        assert got["status"] == status and got["n_keypoints"] == n and len(got["keypoints"]) == cap
        rec = kf.get(0)
        assert rec["n_true"] == n and len(rec["keypoints"]) == cap


# ---- match on planted records
def flip(desc, bits):
    """desc with the given bit positions flipped"""
    d = np.array(desc, np.uint64).copy()
    for b in bits:
        d[b // 64] ^= np.uint64(1) << np.uint64(b % 64)
    return d


def planted(n_old, seed=4, n_window=8):
    """window descriptors and n_old old ones with the distances of the case list planted wherever n_old has room"""
    rng = np.random.default_rng(seed)
    rnd = lambda n: rng.integers(0, 2 ** 63, (n, 4), dtype=np.int64).astype(np.uint64) ^ (rng.integers(0, 2, (n, 4), dtype=np.int64).astype(np.uint64) << np.uint64(63))
    wd = rnd(n_window)
    od = rnd(n_old)
    order = rng.permutation(256)
    far = lambda d, k: flip(d, order[:k])
    if n_old == 3:                                                  # window 4: 127 is the best there is: found, not accepted
        od[0] = far(wd[4], 127); od[1] = far(wd[4], 128); od[2] = far(wd[4], 200)
    elif n_old >= 1:
        od[n_old - 1] = far(wd[0], 5)                               # window 0: the best match at the last index
    if n_old >= 8:
        od[3] = far(wd[1], 11); od[6] = od[3]                       # window 1: duplicates, the lower index wins
        od[1] = far(wd[2], 79)                                      # window 2: exactly 79: accepted
        od[2] = far(wd[3], 80)                                      # window 3: exactly 80: refused, best_idx kept
        od[5] = far(wd[6], 40); od[7] = far(wd[6], 40 + 2)          # window 6: two candidates, the nearer one
    # window 5: every distance at least 128 -- the complement of an old descriptor is 256 - d away from it, so the far ones are forced
    if n_old:
        d = hamming(wd[5:6], od)[0]
        tries = 0
        while (d < 128).any():
            wd[5] = rnd(1)[0]
            d = hamming(wd[5:6], od)[0]
            tries += 1
            if tries > 64:                                          # (many old descriptors: some random one is always nearer than 128)
                break
    opt = np.stack([np.arange(n_old) * 1.5 + 0.25, np.arange(n_old) * 0.5 + 7.0], 1).astype(np.float32)
    onorm = (opt / np.float32(460.0) - np.float32(0.5)).astype(np.float32)
    wxy = np.stack([np.arange(n_window) + 0.5, np.arange(n_window) * 2.0], 1).astype(np.float32)
    return wd, wxy, od, opt, onorm


def check_planted(handle, max_keypoints=96):
    kf = fe.KeyFrames(handle, 67, 41, max_keypoints, 8, 2, pattern())
    for n_old in (0, 1, 3, 63, 64, 65, max_keypoints):
        wd, wxy, od, opt, onorm = planted(n_old)
        kf.set(0, np.zeros((0, 2)), np.zeros(0), np.zeros((0, 2)), np.zeros((0, 4)), wxy, wd)
        kf.set(1, opt, np.full(n_old, 30, np.uint8), onorm, od, np.zeros((0, 2)), np.zeros((0, 4)))
        ref = match(wd, od, opt, onorm)
        got = kf.match([(0, 1)])[0]
        same_match(got, ref, f"planted, {n_old} old")
        if n_old == 0:
            assert not got["status"].any() and got["n_matched"] == 0 and (got["best_idx"] == -1).all()
        if n_old >= 8:
            assert list(got["best_idx"][:4]) == [n_old - 1, 3, 1, 2] and list(got["best_dist"][:4]) == [5, 11, 79, 80]
            assert list(got["status"][:4]) == [1, 1, 1, 0] and got["best_idx"][6] == 5 and got["best_dist"][6] == 40
        if n_old == 3:
            assert got["best_idx"][4] == 0 and got["best_dist"][4] == 127 and got["status"][4] == 0
            assert got["best_idx"][5] == -1 and got["best_dist"][5] == 128 and got["status"][5] == 0
    # a record against itself: every window descriptor that is also a keypoint descriptor finds distance 0 at its index
    wd, wxy, od, opt, onorm = planted(65)
    kf.set(0, opt, np.full(65, 9, np.uint8), onorm, od, opt[10:18], od[10:18])
    got = kf.match([(0, 0)])[0]
    same_match(got, match(od[10:18], od, opt, onorm), "own record")
    assert (got["best_dist"] == 0).all() and list(got["best_idx"]) == list(range(10, 18))


def rendered_pair(size=(100, 70)):
    """frame 0's corners as window points against frame 1's record"""
    r0, r1 = scene_ref(size, 0), scene_ref(size, 1)
    w = r0["keypoints"][:150]
    return w, brief(r0["blur"], w), match(brief(r0["blur"], w), r1["descriptors"], r1["keypoints"], r1["norm"])


N_RENDERED = 119         # the reference's own count at 100 x 70, seed 5


def check_rendered(handle, size=(100, 70)):
    w, wd, ref = rendered_pair(size)
    assert ref["n_matched"] == N_RENDERED > MIN_LOOP_NUM, ref["n_matched"]
    cam = cameras(size[0])["pinhole"]
    kf = fe.KeyFrames(handle, size[0], size[1], 150, 150, 2, pattern())
    kf.add([0, 1], frames(size), [camera_struct(cam)] * 2, [w, np.zeros((0, 2), np.float32)], arrays=False)
    got = kf.match([(0, 1)])[0]
    same_match(got, ref, "rendered frames")
    return ref["n_matched"]


# ---- batch and state
def check_batch_and_state(handle, size=(67, 41), counts=(1, 3, 33)):
    """a batch of 1, 3 and 33 keyframes equals the single calls (cameras mixed), likewise pairs; refilling a slot leaves the others, bit
    for bit; get after set returns the input"""
    W, H = size
    cams = cameras(W)
    names = ("pinhole", "mei", "kb")
    imgs = frames(size)
    rng = np.random.default_rng(8)
    nmax = max(counts)
    variants = [np.clip(imgs[i % 2].astype(np.int32) + rng.integers(-6, 7, (H, W)), 0, 255).astype(np.uint8) for i in range(nmax)]
    wins = [window_points(size, 3 + i % 5, seed=20 + i) for i in range(nmax)]
    kf = fe.KeyFrames(handle, W, H, 48, 8, nmax + 1, pattern())
    single = []
    for i in range(nmax):
        g = kf.add([i], [variants[i]], [camera_struct(cams[names[i % 3]])], [wins[i]])[0]
        single.append((g, kf.get(i)))
    for i in (0, 1, 2):                                           # each model once against the reference
        ref = keyframe(variants[i], cams[names[i % 3]], wins[i], 48)
        same_record(single[i][0], ref, f"single {names[i % 3]}")
    pairs_all = [(i, (i * 7 + 3) % nmax) for i in range(nmax)]
    single_m = [kf.match([p])[0] for p in pairs_all]
    for n in counts:
        kf2 = fe.KeyFrames(handle, W, H, 48, 8, nmax + 1, pattern())
        slots = list(range(n))[::-1]
        got = kf2.add(slots, [variants[s] for s in slots], [camera_struct(cams[names[s % 3]]) for s in slots], [wins[s] for s in slots])
        for s, g in zip(slots, got):
            same_get(g, single[s][0], f"batch of {n}, slot {s}")
            same_get(kf2.get(s), single[s][1], f"batch of {n}, record {s}")
        pairs = [(i, (i * 7 + 3) % n) for i in range(n)]
        alone = [kf2.match([p])[0] for p in pairs]
        for p, a, g in zip(pairs, alone, kf2.match(pairs)):
            same_get(g, a, f"{n} pairs, pair {p}")
        if n == nmax:
            for a, b in zip(alone, single_m):
                same_get(a, b, "pairs after the batch")
    # (kf2 of the last count holds every slot) refill slot 1: the others stay, bit for bit
    before = [kf2.get(s) for s in range(nmax)]
    g = kf2.add([1], [variants[4]], [camera_struct(cams["mei"])], [wins[2]])[0]
    same_record(g, keyframe(variants[4], cams["mei"], wins[2], 48), "refilled slot")
    for s in range(nmax):
        if s != 1:
            same_get(kf2.get(s), before[s], f"slot {s} after the refill")
    assert kf2.get(1)["descriptors"].tobytes() != before[1]["descriptors"].tobytes()
    # get after set
    wd, wxy, od, opt, onorm = planted(48)
    sc = (np.arange(48) * 5 % 255).astype(np.uint8)
    kf2.set(nmax, opt, sc, onorm, od, wxy, wd, n_true=60)
    rec = kf2.get(nmax)
    want = {"n_true": 60, "keypoints": opt, "scores": sc, "norm": onorm, "descriptors": od, "window_xy": wxy, "window_descriptors": wd}
    same_get(rec, want, "get after set")


# ---- refusals: each through the C entry, with nothing moved
REFUSALS = ("configure_small", "configure_pattern", "configure_null_pattern", "configure_counts", "add_unconfigured", "add_struct_size", "add_out_struct_size",
            "add_slot", "add_same_slot", "add_n_window", "add_null_image", "add_stride", "add_camera_model", "add_camera_focal", "add_camera_nan",
            "get_never_filled", "get_slot", "get_struct_size", "set_counts", "set_null", "set_struct_size", "match_never_filled", "match_slot",
            "match_struct_size", "match_unconfigured")


def _raw_add(kf, ins, outs):
    return kf.lib.vg_kf_add(kf.h, len(ins), ins, outs)


def check_refusal(handle, name, bare_handle=None):
    W, H = 67, 41
    L = handle.lib
    pat = pattern()
    pp = lambda a: a.ctypes.data_as(C.POINTER(C.c_int16))
    if name.startswith("configure"):
        kf = fe.KeyFrames(handle, W, H, 32, 8, 2, pat)
        img = frames((W, H))[0]
        kf.add([0], [img], [camera_struct(cameras(W)["pinhole"])], [window_points((W, H), 3)])
        before = kf.get(0)
        bad = pat.copy()
        bad[2, 17] = 128
        rc = {"configure_small": lambda: L.vg_kf_configure(handle.h, 6, 41, 32, 8, 2, pp(pat)),
              "configure_pattern": lambda: L.vg_kf_configure(handle.h, W, H, 32, 8, 2, pp(bad)),
              "configure_null_pattern": lambda: L.vg_kf_configure(handle.h, W, H, 32, 8, 2, None),
              "configure_counts": lambda: L.vg_kf_configure(handle.h, W, H, 65536, 8, 2, pp(pat)) or L.vg_kf_configure(handle.h, W, H, 32, 1025, 2, pp(pat))
              or L.vg_kf_configure(handle.h, W, H, 32, 8, 0, pp(pat))}[name]()
        assert rc == BAD_ARG and b"vg_kf_configure" in L.vg_last_error(handle.h)
        if name == "configure_counts":
            assert L.vg_kf_configure(handle.h, W, H, 32, 1025, 2, pp(pat)) == BAD_ARG and L.vg_kf_configure(handle.h, W, H, 32, 8, 0, pp(pat)) == BAD_ARG
            assert L.vg_kf_configure(handle.h, W, 6, 32, 8, 2, pp(pat)) == BAD_ARG
        same_get(kf.get(0), before, name + ": the records of the configuration that stands")
        return
    if name.endswith("unconfigured"):
        assert bare_handle is not None
        kf = fe.KeyFrames.__new__(fe.KeyFrames)
        ok = fe.KeyFrames(handle, W, H, 32, 8, 2, pat)             # (sets the argument types on the shared library object)
        kf.hd, kf.lib, kf.h, kf.W, kf.H, kf.MK, kf.MW, kf.NS = bare_handle, bare_handle.lib, bare_handle.h, W, H, 32, 8, 2
        try:
            if name == "add_unconfigured":
                kf.add([0], [frames((W, H))[0]], [camera_struct(cameras(W)["pinhole"])], [np.zeros((0, 2))])
            else:
                kf.match([(0, 0)])
        except RuntimeError as e:
            assert "vg_kf_configure" in str(e)
            return
        raise AssertionError(name + " was not refused")
    kf = fe.KeyFrames(handle, W, H, 32, 8, 3, pat)
    cam = camera_struct(cameras(W)["pinhole"])
    imgs = frames((W, H))
    w = window_points((W, H), 3)
    kf.add([0, 1], imgs, [cam, cam], [w, w])
    before = [kf.get(0), kf.get(1)]

    def entry(slot, img, n_window=3, stride=W, camera=cam, size=None):
        a = fe.KfIn()
        a.struct_size, a.slot, a.stride, a.n_window = C.sizeof(fe.KfIn) if size is None else size, slot, stride, n_window
        a.img = None if img is None else img.ctypes.data_as(fe._u8)
        a.window_xy, a.camera = w.ctypes.data_as(fe._f4), camera
        return a

    def outs(n, size=None):
        o = (fe.KfOut * n)()
        for q in o:
            q.struct_size, q.n_keypoints, q.status = C.sizeof(fe.KfOut) if size is None else size, -77, -77
        return o

    def cam_with(**kw):
        c = camera_struct(cameras(W)["pinhole"])
        for k, v in kw.items():
            if k == "p0":
                c.p[0] = v
            else:
                setattr(c, k, v)
        return c

    img = np.ascontiguousarray(imgs[1])
    if name.startswith("add"):
        good = entry(0, img)
        o = outs(2)
        second = {"add_struct_size": lambda: entry(1, img, size=C.sizeof(fe.KfIn) - 4), "add_out_struct_size": lambda: entry(1, img),
                  "add_slot": lambda: entry(3, img), "add_same_slot": lambda: entry(0, img), "add_n_window": lambda: entry(1, img, n_window=9),
                  "add_null_image": lambda: entry(1, None), "add_stride": lambda: entry(1, img, stride=W - 1),
                  "add_camera_model": lambda: entry(1, img, camera=cam_with(model=2)), "add_camera_focal": lambda: entry(1, img, camera=cam_with(p0=0.0)),
                  "add_camera_nan": lambda: entry(1, img, camera=cam_with(p0=float("nan")))}[name]()
        if name == "add_out_struct_size":
            o[1].struct_size = 8
        ins = (fe.KfIn * 2)(good, second)
        assert _raw_add(kf, ins, o) == BAD_ARG and b"vg_kf_add: entry 1" in L.vg_last_error(handle.h), L.vg_last_error(handle.h)
        assert o[0].n_keypoints == -77 and o[1].status == -77
    elif name.startswith("get") or name.startswith("set"):
        r = fe.KfRecord()
        r.struct_size = C.sizeof(fe.KfRecord)
        if name == "get_never_filled":
            rc = L.vg_kf_get(handle.h, 2, C.byref(r))
        elif name == "get_slot":
            rc = L.vg_kf_get(handle.h, 3, C.byref(r)) or L.vg_kf_get(handle.h, -1, C.byref(r))
        elif name == "get_struct_size":
            r.struct_size -= 8
            rc = L.vg_kf_get(handle.h, 0, C.byref(r))
        else:
            buf = np.zeros(64 * 4, np.uint64)
            for f_, t in (("keypoints_xy", fe._f4), ("scores", fe._u8), ("norm_xy", fe._f4), ("descriptors", fe._u64), ("window_xy", fe._f4), ("window_descriptors", fe._u64)):
                setattr(r, f_, buf.ctypes.data_as(t))
            r.n_keypoints, r.n_window = 4, 2
            if name == "set_counts":
                r.n_keypoints = 33
                rc = L.vg_kf_set(handle.h, 0, C.byref(r))
                r.n_keypoints, r.n_window = 4, 9
                assert L.vg_kf_set(handle.h, 0, C.byref(r)) == BAD_ARG
            elif name == "set_null":
                r.descriptors = None
                rc = L.vg_kf_set(handle.h, 0, C.byref(r))
            else:
                r.struct_size += 8
                rc = L.vg_kf_set(handle.h, 0, C.byref(r))
        assert rc == BAD_ARG and (b"vg_kf_get" in L.vg_last_error(handle.h) or b"vg_kf_set" in L.vg_last_error(handle.h))
    else:
        p = (fe.KfPair * 2)()
        for q, (a, b) in zip(p, ((0, 1), (1, 0))):
            q.struct_size, q.cur_slot, q.old_slot = C.sizeof(fe.KfPair), a, b
        o = (fe.KfMatchOut * 2)()
        for q in o:
            q.struct_size, q.n_matched = C.sizeof(fe.KfMatchOut), -77
        if name == "match_never_filled":
            p[1].old_slot = 2
        elif name == "match_slot":
            p[1].cur_slot = 3
        else:
            p[1].struct_size = 4
        assert L.vg_kf_match(handle.h, 2, p, o) == BAD_ARG and b"vg_kf_match: pair 1" in L.vg_last_error(handle.h)
        assert o[0].n_matched == -77 and o[1].n_matched == -77
    for s in (0, 1):
        same_get(kf.get(s), before[s], f"{name}: slot {s}")
    assert L.vg_kf_get(handle.h, 2, C.byref(fe.KfRecord(struct_size=C.sizeof(fe.KfRecord)))) == BAD_ARG, "slot 2 was never filled"


def check_pattern_file():
    """the yml reader against the fixture: four lists of 256 entries, known first and last entries"""
    p = pattern()
    assert p.shape == (4, 256) and p.dtype == np.int16
    assert [int(p[k, 0]) for k in range(4)] == FIRST and [int(p[k, 255]) for k in range(4)] == LAST, ([int(p[k, 0]) for k in range(4)], [int(p[k, 255]) for k in range(4)])
    assert np.abs(p).max() <= 127


FIRST = [0, -10, 0, -6]      # x1[0] y1[0] x2[0] y2[0] of support_files/brief_pattern.yml
LAST = [0, -3, -1, -2]


# ---- class KeyFrame (host/keyframe.h) through `vins_replay kf`
def write_replay_file(path, size, max_keypoints, max_window, entries, pairs):
    """KFR1; entries: (image, window_xy, cam)"""
    model = {"pinhole": fe.CAM_PINHOLE, "mei": fe.CAM_MEI, "kb": fe.CAM_KANNALA_BRANDT}
    with open(path, "wb") as f:
        np.array([0x3152464B, size[0], size[1], max_keypoints, max_window, len(entries), len(pairs)], np.int32).tofile(f)
        for img, w, cam in entries:
            w = np.ascontiguousarray(w, np.float32).reshape(-1, 2)
            np.array([len(w)], np.int32).tofile(f)
            w.tofile(f)
            np.array([model[cam[0]]], np.int32).tofile(f)
            np.array(list(cam[2] if cam[0] == "mei" else cam[1]) + [cam[1] if cam[0] == "mei" else 0.0], np.float64).tofile(f)
            np.ascontiguousarray(img, np.uint8).tofile(f)
        np.array(pairs, np.int32).reshape(-1, 2).tofile(f)


def replay_expected(size, max_keypoints, entries, pairs):
    """the text `vins_replay kf` must write, from the reference alone"""
    hx = lambda a: " ".join(f"{int(v):08x}" for v in bits32(a).reshape(-1))
    recs, lines = [], []
    for i, (img, w, cam) in enumerate(entries):
        r = keyframe(img, cam, w, max_keypoints)
        recs.append(r)
        lines.append(f"kf {i} {r['n_keypoints']} {r['status']} {r['n_kept']} {len(r['window_descriptors'])}")
        for q in range(r["n_kept"]):
            d = " ".join(f"{int(v):016x}" for v in r["descriptors"][q])
            lines.append(f"k {r['keypoints'][q, 0]:.9g} {r['keypoints'][q, 1]:.9g} {int(r['scores'][q])} {hx(r['norm'][q])} {d}")
        lines += ["w " + " ".join(f"{int(v):016x}" for v in d) for d in r["window_descriptors"]]
    for p, (c, o) in enumerate(pairs):
        m = match(recs[c]["window_descriptors"], recs[o]["descriptors"], recs[o]["keypoints"], recs[o]["norm"])
        lines.append(f"pair {p} {c} {o} {m['n_matched']} {1 if m['n_matched'] > MIN_LOOP_NUM else 0}")
        for w in range(m["n_window"]):
            lines.append(f"s {int(m['status'][w])} {int(m['best_idx'][w])} {int(m['best_dist'][w])} {hx(m['matched_2d_old'][w])} {hx(m['matched_2d_old_norm'][w])}")
        wxy = np.asarray(entries[c][1], np.float32).reshape(-1, 2)
        for k in range(m["n_matched"]):
            lines.append(f"m {int(m['matched_index'][k])} {hx(wxy[m['matched_index'][k]])} {hx(m['matched_old_xy'][k])} {hx(m['matched_old_norm'][k])}")
    return lines


def check_replay(exe, tmp_path):
    """three keyframes (one camera model each, the middle one truncated by the cap) and three pairs, one of them above MIN_LOOP_NUM"""
    size = (100, 70)
    cams = cameras(size[0])
    r0 = scene_ref(size, 0)
    entries = [(frames(size)[0], r0["keypoints"][:100], cams["pinhole"]), (frames(size)[1], window_points(size, 7), cams["mei"]),
               (frames(size)[1], np.zeros((0, 2), np.float32), cams["kb"])]
    pairs = [(0, 1), (1, 0), (0, 2)]
    src, out = os.path.join(str(tmp_path), "kf.bin"), os.path.join(str(tmp_path), "kf.txt")
    write_replay_file(src, size, 100, 100, entries, pairs)
    r = subprocess.run([exe, "kf", src, out, PATTERN_FILE], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    want = replay_expected(size, 100, entries, pairs)
    got = open(out).read().splitlines()
    assert want[0].split()[3] == str(fe.KF_TRUNCATED) and int(want[0].split()[2]) == 133
    assert any(ln.startswith("pair 0 0 1") and ln.endswith(" 1") for ln in want), "a pair above MIN_LOOP_NUM"
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a == b, (a, b)


def check_pattern_reader(exe):
    """BriefExtractor (host/keyframe.h on host/yaml_config.h's block sequences) against the fixture; host only"""
    r = subprocess.run([exe, "kf_pattern", PATTERN_FILE], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    rows = [[int(v) for v in ln.split()] for ln in r.stdout.splitlines()]
    assert len(rows) == 4 and all(len(x) == 256 for x in rows)
    assert [x[0] for x in rows] == FIRST and [x[255] for x in rows] == LAST
    assert np.array_equal(np.array(rows, np.int16), pattern())


# ---- the stand-alone sanitizer program (tests/kf_san_main.cpp): its input file and what it must print
def write_san_case(path, size, img, window_xy, cam, max_keypoints, planted_case):
    """KFS1: W H MK MW | pattern int16[1024] | image | n_window, points | camera p[8] | the planted match: n_old, descriptors, 8 window descriptors"""
    wd, _, od, _, _ = planted_case
    with open(path, "wb") as f:
        np.array([0x3153464B, size[0], size[1], max_keypoints, max(len(window_xy), 8), len(window_xy), len(od)], np.int32).tofile(f)
        pattern().tofile(f)
        np.ascontiguousarray(img, np.uint8).tofile(f)
        np.ascontiguousarray(window_xy, np.float32).tofile(f)
        np.array(cam[1], np.float64).tofile(f)
        np.ascontiguousarray(od, np.uint64).tofile(f)
        np.ascontiguousarray(wd, np.uint64).tofile(f)


def fnv(h, a):
    for b in np.ascontiguousarray(a).tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def san_expected(got_add, got_match):
    """the line kf_san_main prints for a case, from the binding's results on the same input"""
    h = 1469598103934665603
    for k in ("keypoints", "scores", "norm", "descriptors", "window_descriptors"):
        h = fnv(h, got_add[k])
    for k in ("best_idx", "best_dist", "status", "matched_index"):
        h = fnv(h, got_match[k])
    return f"{got_add['n_keypoints']} {got_add['status']} {got_match['n_matched']} {h:016x}"
