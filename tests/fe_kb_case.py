"""Shared by the Kannala-Brandt camera tests (test_fe_kb_*.py, test_fe_read_image_kb.py, test_fe_batch_kb.py): the cameras, the
definition of vins-mono_amd/csrc/fe_camera.h (fe_cam_lift_kb, fe_kb_sincos) restated in NumPy double in the same expression order
(lift64_kb), the reference's EquidistantCamera::liftProjective + backprojectSymmetric (EquidistantCamera.cc:427-442, :715-818) restated
with numpy.linalg.eigvals, arctan2, sin and cos (ref_lift_kb), and the checks that take handles: the `not gpu` tests run them in a child
process on handles of the emulated library (fe_camera_case.run_emulated), the `gpu` tests on the device."""
import ctypes as C
import os

import numpy as np

from vins_mono_amd import fe

import fe_camera_case as cc

HOST = os.path.join(cc.ROOT, "vins-mono_amd", "lib", "libvins_host.so")

# name -> (width, height, (mu mv u0 v0 k2 k3 k4 k5)).  tum, cla, realsense: the projection_parameters of the settings files the
# reference ships (copies under tests/golden/configs).  deg7 (k5 = 0) and deg3 (k2 alone) are synthetic, at 320 x 240 with mu ~ 150 so
# that the corners reach theta ~ 1.3; deg7's principal point is a pair of floats (the r < 1e-10 branch can be hit exactly).  zero: no
# distortion, theta = r.
CAMS = {
    "tum": (512, 512, (190.97847715128717, 190.9733070521226, 254.93170605935475, 256.8974428996504,
                       0.0034823894022493434, 0.0007150348452162257, -0.0020532361418706202, 0.00020293673591811182)),
    "cla": (752, 480, (472.2863830700696, 470.83759684346785, 368.8316828103749, 232.23688706965652,
                       -0.005740195474458931, 0.02878252863739417, -0.04010621197185408, 0.02008469575876223)),
    "realsense": (640, 480, (2.7723712054408202e+02, 2.7699784668734617e+02, 3.3625356873985868e+02, 2.3603924727453901e+02,
                             1.7280355035195181e-02, -2.5505200860040985e-02, 2.2621441637715487e-02, -7.3355871719731113e-03)),
    "deg7": (320, 240, (150.0, 149.5, 160.5, 120.25, -0.012, 0.02, -0.003, 0.0)),
    "deg3": (320, 240, (151.0, 150.5, 158.3, 121.7, 0.025, 0.0, 0.0, 0.0)),
    "zero": (320, 240, (150.5, 150.0, 159.2, 119.6, 0.0, 0.0, 0.0, 0.0)),
}
TABLE = ("tum", "cla", "realsense", "deg7", "deg3")            # the five cameras of the definition test
NEWTON = 10                                                    # FE_KB_NEWTON


def params(name, width=None):
    """the eight numbers of a camera; `width`: the projection parameters scaled to a frame of that width (same aspect)"""
    w, _, p = CAMS[name]
    s = 1.0 if width is None else width / float(w)
    return tuple(v * s for v in p[:4]) + tuple(p[4:])


def camera(name, width=None):
    return fe.Camera.kannala_brandt(*params(name, width))


def points_of(name):
    """fe_camera_case.points at the camera's own frame size"""
    w, h, _ = CAMS[name]
    return cc.points(w, h)


# ---- the definition (csrc/fe_camera.h), same expression order
_S = np.array([-1.0 / 6.0, 1.0 / 120.0, -1.0 / 5040.0, 1.0 / 362880.0, -1.0 / 39916800.0, 1.0 / 6227020800.0, -1.0 / 1307674368000.0,
               1.0 / 355687428096000.0])
_C = np.array([-1.0 / 2.0, 1.0 / 24.0, -1.0 / 720.0, 1.0 / 40320.0, -1.0 / 3628800.0, 1.0 / 479001600.0, -1.0 / 87178291200.0,
               1.0 / 20922789888000.0])


def sincos64(t):
    """fe_kb_sincos"""
    t = np.asarray(t, np.float64)
    with np.errstate(all="ignore"):
        k = np.rint(t * 6.36619772367581382433e-01)
        y = (t - k * 1.57079632673412561417e+00) - k * 6.07710050650619224932e-11
        y2 = y * y
        ps, pc = np.full_like(y, _S[7]), np.full_like(y, _C[7])
        for i in range(6, -1, -1):
            ps = ps * y2 + _S[i]
            pc = pc * y2 + _C[i]
        sy, cy = y + y * y2 * ps, 1.0 + y2 * pc
        kh = k * 0.5
        odd = np.rint(kh) != kh
        jh = np.where(odd, k - 1.0, k) * 0.25
        neg = np.rint(jh) != jh
        s0, c0 = np.where(odd, cy, sy), np.where(odd, sy, cy)
        return np.where(neg, -s0, s0), np.where(neg != odd, -c0, c0)


def theta64_kb(pts, p):
    """(ux, uy, r, theta) of fe_cam_lift_kb for float32 pixels"""
    mu, mv, u0, v0, k2, k3, k4, k5 = [np.float64(v) for v in p]
    q = np.asarray(pts, np.float32).astype(np.float64).reshape(-1, 2)
    ux = (1.0 / mu) * q[:, 0] + (-u0 / mu)
    uy = (1.0 / mv) * q[:, 1] + (-v0 / mv)
    r = np.sqrt(ux * ux + uy * uy)
    d2, d3, d4, d5 = 3.0 * k2, 5.0 * k3, 7.0 * k4, 9.0 * k5
    th = r.copy()
    with np.errstate(all="ignore"):
        for _ in range(NEWTON):
            t2 = th * th
            f = th * ((((k5 * t2 + k4) * t2 + k3) * t2 + k2) * t2 + 1.0) - r
            df = (((d5 * t2 + d4) * t2 + d3) * t2 + d2) * t2 + 1.0
            th = th - f / df
    return ux, uy, r, th


def lift64_kb(pts, p):
    """fe_cam_lift_kb: the ray (x, y, z) of float32 pixels"""
    ux, uy, r, th = theta64_kb(pts, p)
    st, ct = sincos64(th)
    centre = r < 1e-10
    with np.errstate(all="ignore"):
        cphi, sphi = np.where(centre, 1.0, ux / r), np.where(centre, 0.0, uy / r)
    return st * cphi, st * sphi, ct


def lifted_xy(pts, p):
    """(float)(x / z), (float)(y / z): what vg_fe_lift writes"""
    x, y, z = lift64_kb(pts, p)
    with np.errstate(all="ignore"):
        return np.stack([x / z, y / z], 1).astype(np.float32)


# ---- the reference (EquidistantCamera.cc), with NumPy's eigenvalues in the place of Eigen::EigenSolver
def ref_theta_kb(pts, p):
    """(ux, uy, r, theta, phi) of backprojectSymmetric (:715-818)"""
    mu, mv, u0, v0, k2, k3, k4, k5 = [np.float64(v) for v in p]
    q = np.asarray(pts, np.float32).astype(np.float64).reshape(-1, 2)
    ux = (1.0 / mu) * q[:, 0] + (-u0 / mu)                     # :432-433 with the inverse K of :271-274
    uy = (1.0 / mv) * q[:, 1] + (-v0 / mv)
    tol = 1e-10
    r = np.sqrt(ux * ux + uy * uy)                             # p_u.norm()
    phi = np.where(r < 1e-10, 0.0, np.arctan2(uy, ux))
    npow = 9 - 2 * sum(1 for k in (k5, k4, k3, k2) if k == 0.0)
    coeffs = np.zeros(npow + 1)
    coeffs[1] = 1.0
    for power, k in ((3, k2), (5, k3), (7, k4), (9, k5)):
        if npow >= power:
            coeffs[power] = k
    if npow == 1:
        return ux, uy, r, r.copy(), phi
    A = np.zeros((len(r), npow, npow))
    A[:, 1:, :-1] = np.eye(npow - 1)
    A[:, :, -1] = -coeffs[:npow] / coeffs[npow]
    A[:, 0, -1] = r / coeffs[npow]                             # coeffs(0) = -p_u_norm
    ev = np.linalg.eigvals(A)
    t = ev.real.copy()
    ok = (np.abs(ev.imag) <= tol) & (t >= -tol)
    t = np.where(t < 0.0, 0.0, t)
    t = np.where(ok, t, np.inf)
    theta = t.min(axis=1)
    theta = np.where(ok.any(axis=1), theta, r)                 # thetas.empty()
    return ux, uy, r, theta, phi


def ref_lift_kb(pts, p):
    """EquidistantCamera::liftProjective (:427-442)"""
    _, _, _, theta, phi = ref_theta_kb(pts, p)
    return np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)


def first_critical_point(p):
    """the smallest theta > 0 with dr/dtheta = 0 (the end of the lens's first monotone branch), or inf"""
    k2, k3, k4, k5 = p[4:]
    roots = np.roots([9.0 * k5, 7.0 * k4, 5.0 * k3, 3.0 * k2, 1.0])            # in theta^2; leading zeros are dropped by np.roots
    t = [z.real for z in roots if abs(z.imag) <= 1e-12 * max(1.0, abs(z)) and z.real > 0.0]
    return float(np.sqrt(min(t))) if t else float("inf")


# ---- vg_fe_lift point by point (test_fe_kb_lift.py)
BAD_ARG = -1


def _extra_points(name):
    w, h, p = CAMS[name]
    ex = [[np.float32(p[2]), np.float32(p[3])], [0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1]]
    if name == "tum":
        ex.append([480.0, 482.0])                              # 318 pixels from the centre: theta ~ 1.7 > pi / 2
    return np.array(ex, np.float32)


def host_lift(pts, model, p, xi=0.0):
    """CameraModel::liftProjective of the stand-alone host class: rays [n, 3] double"""
    lib = C.CDLL(HOST)
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    rays, p8 = np.zeros((len(pts), 3)), np.array(p, np.float64)
    lib.vins_host_camera_lift.restype = None
    lib.vins_host_camera_lift.argtypes = [C.c_int, C.POINTER(C.c_double), C.c_double, C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_double)]
    lib.vins_host_camera_lift(int(model), p8.ctypes.data_as(C.POINTER(C.c_double)), float(xi), pts.ctypes.data_as(C.POINTER(C.c_float)), len(pts),
                              rays.ctypes.data_as(C.POINTER(C.c_double)))
    return rays


def check_lift(handle, with_host_class=True):
    """vg_fe_lift of every camera bit-identical to lift64_kb on points() of its frame, its principal point, the four corners and (tum) a
    pixel behind the lens; the host class gives the same doubles"""
    cap = 2048
    tr = fe.FrontEnd(handle, 320, 240, 1, cap)
    total = 0
    for name in TABLE + ("zero",):
        p = params(name)
        pts = np.concatenate([points_of(name), _extra_points(name)])
        want = lifted_xy(pts, p)
        got = np.concatenate([tr.lift(pts[i:i + cap], camera(name)) for i in range(0, len(pts), cap)])
        both = np.isfinite(want).all(1) & np.isfinite(got).all(1)
        assert both.mean() > 0.999, (name, both.mean())
        bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(1) & both)
        assert len(bad) == 0, (name, len(bad), pts[bad[:4]], got[bad[:4]], want[bad[:4]])
        x, y, z = lift64_kb(pts, p)
        if name == "tum":
            assert (z[both] < 0.0).sum() >= 1                   # the quadrant swap was compared
        if name == "deg7":
            assert theta64_kb(pts, p)[2].min() < 1e-10          # the centre branch was compared
            i = int(np.argmin(theta64_kb(pts, p)[2]))
            assert got[i, 0] == 0.0 and got[i, 1] == 0.0
        if name == "zero":
            _, _, r, th = theta64_kb(pts, p)
            assert np.array_equal(r, th)
        if with_host_class:
            rays = host_lift(pts, fe.CAM_KANNALA_BRANDT, p)
            assert np.array_equal(rays.view(np.uint64), np.stack([x, y, z], 1).view(np.uint64)), name
        total += int(both.sum())
    return total


def check_refusals(handle):
    """model 3 with a non-finite or zero p[0] / p[1], and the models 2 and 4: refused by both calls, nothing written, the camera kept"""
    tr = fe.FrontEnd(handle, 320, 240, 1, 160)
    lib = handle.lib
    lib.vg_last_error.restype = C.c_char_p
    pts = cc.points(n_random=8)[:64]
    f4 = C.POINTER(C.c_float)
    tr.set_camera(0, camera("deg7"))
    kept = tr.lift(pts, camera("deg7"))
    out = np.full((len(pts), 2), 7.0, np.float32)

    def both(c, why):
        assert lib.vg_fe_set_camera(tr.h, 0, C.byref(c)) == BAD_ARG, why
        assert b"vg_fe_set_camera" in lib.vg_last_error(tr.h), why
        assert lib.vg_fe_lift(tr.h, C.byref(c), pts.ctypes.data_as(f4), len(pts), out.ctypes.data_as(f4)) == BAD_ARG, why
        assert (out == 7.0).all(), why

    for i in range(8):
        for v in (float("nan"), float("inf"), float("-inf")):
            c = camera("deg7"); c.p[i] = v; both(c, "non-finite p[%d]" % i)
    c = camera("deg7"); c.p[0] = 0.0; both(c, "zero p[0]")
    c = camera("deg7"); c.p[1] = -0.0; both(c, "zero p[1]")
    c = camera("deg7"); c.model = 2; both(c, "model 2")
    c = camera("deg7"); c.model = 4; both(c, "model 4")
    c = camera("deg7"); c.xi = float("nan")                     # xi is not inspected for KANNALA_BRANDT
    tr.set_camera(0, c)
    assert cc.same_bits(tr.lift(pts, c), kept)
    return True


# ---- vg_fe_read_image with a KB camera against the step-by-step calls (test_fe_read_image_kb.py)
READ_IMAGE_CAMS = {"deg9": ("realsense", 320), "deg7": ("deg7", None)}       # realsense at half size: 320 x 240


def stepwise(tr, W, H, img, cur, cnt, publish, p, max_cnt, min_dist, equalize, order_fn):
    """fe_read_image_camera_case.stepwise with a KB camera of the eight numbers `p`: one frame from the fine-grained calls, lift64_kb for
    rejectWithF's two point sets.  Returns the dictionary FrontEnd.read_image returns, the new list, its counts"""
    from fe_read_image_case import FOCAL
    cam = fe.Camera.kannala_brandt(*p)
    tr.push_frames([img], equalize=equalize)
    cur = np.asarray(cur, np.float32).reshape(-1, 2)
    out = dict(ransac_ran=False, status_f=None, kept=None, new_xy=None)
    if len(cur):
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
        out["un_xy"] = tr.lift(forw1, cam) if len(forw1) else np.zeros((0, 2), np.float32)
        return out, forw1, cnt1
    if len(forw1) >= 8:                                          # feature_tracker.cpp:176-187: FOCAL_LENGTH * x / z + COL / 2.0
        cx, cy, cz = lift64_kb(cur1, p)
        fx, fy, fz = lift64_kb(forw1, p)
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
    out["un_xy"] = tr.lift(final, cam) if len(final) else np.zeros((0, 2), np.float32)
    return out, final, np.concatenate([cnt_o[kept], np.ones(len(new), np.int64)])


def run_read_image(handle_a, handle_b, W=320, H=240, n_frames=5):
    """the streams normal / lmeds / few / unpublished of fe_read_image_camera_case.run for the two KB cameras; returns, per camera, what
    happened (for check_read_image)"""
    import fe_scene
    from fe_read_image_camera_case import unstable_like
    from fe_read_image_case import _same
    cap = 160
    seen = {}
    frames = fe_scene.moving_scene(n_frames, seed=8, width=W, height=H, velocity=(2.7, -1.2))
    for name, (base, width) in READ_IMAGE_CAMS.items():
        p = params(base, width)
        s = seen[name] = dict(ransac_device=0, fb_lmeds=0, fb_collinear=0, no_ransac=0, published=0, unpublished=0, lifted=0)

        def stream(what, frames, max_cnt, min_dist, first_pts=None, pub=lambda k: k % 2 == 0):
            one, ref = fe.FrontEnd(handle_a, W, H, 1, cap), fe.FrontEnd(handle_b, W, H, 1, cap)
            one.set_camera(0, fe.Camera.kannala_brandt(*p))
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
                want, pts_next, cnt_next = stepwise(ref, W, H, img, pts, cnt, publish, p, max_cnt, min_dist, True, unstable_like)
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

        stream("normal", frames, 60, 14)
        stream("lmeds", frames[:4], 12, 30)
        stream("few", frames[:3], 5, 40)
        grid = np.array([[x, y] for y in np.arange(0.15, 0.9, 0.2) * H for x in np.arange(0.1, 0.95, 0.12) * W], np.float32)
        stream("unpublished", frames[:4], 60, 14, first_pts=grid, pub=lambda k: False)
    return seen


def check_read_image(seen):
    """the coverage assertions of fe_read_image_camera_case.check"""
    import fe_read_image_camera_case as rc
    return rc.check(seen, names=tuple(READ_IMAGE_CAMS))


# ---- mixed models in one batched call, and the resident track lists (test_fe_batch_kb.py)
def check_batch(handle, other, W=320, H=240, n_frames=4):
    """fe_camera_case.check_batch with the streams: no camera (the pinhole of intr), MEI A, KB degree 9, KB degree 3"""
    import fe_scene
    S, cap = 4, 160
    cams = [None, cc.camera("A"), camera("realsense", 320), camera("deg3")]
    scenes = [fe_scene.moving_scene(n_frames, seed=40 + c, width=W, height=H, velocity=(2.0 + 0.4 * c, -1.0 + 0.6 * c)) for c in range(S)]
    kw = dict(max_cnt=60, min_dist=14, equalize=True)
    alone = []
    for c in range(S):
        tr = fe.FrontEnd(other, W, H, 1, cap)
        if cams[c] is not None:
            tr.set_camera(0, cams[c])
        pts, outs = np.zeros((0, 2), np.float32), []
        for k in range(n_frames):
            outs.append(tr.read_image(scenes[c][k], pts, k % 2 == 0, cc.PIN8, **kw))
            pts = cc.next_points(outs[-1], k % 2 == 0)
        alone.append(outs)
    tr = fe.FrontEnd(handle, W, H, S, cap)
    for c in range(S):
        if cams[c] is not None:
            tr.set_camera(c, cams[c])
    pts = [np.zeros((0, 2), np.float32)] * S
    ransac = 0
    for k in range(n_frames):
        pub = k % 2 == 0
        outs = tr.read_image_batch([scenes[c][k] for c in range(S)], pts, [pub] * S, [cc.PIN8] * S, **kw)
        for c in range(S):
            cc.same_frame(outs[c], alone[c][k], ("stream", c, "frame", k))
            ransac += int(outs[c]["ransac_ran"] and not outs[c]["fallback"])
        pts = [cc.next_points(outs[c], pub) for c in range(S)]
    assert ransac >= S                                                          # every stream lifted both point sets for rejectWithF
    assert all(len(alone[c][-1]["un_xy"]) >= 30 for c in range(S))
    # the KB streams lifted with their own cameras: the last list of each is the definition's
    for c, (base, width) in ((2, ("realsense", 320)), (3, ("deg3", None))):
        assert cc.same_bits(alone[c][-1]["un_xy"], lifted_xy(pts[c], params(base, width))), c
    return True


def check_tracks(handle, other, W=320, H=240, n_frames=4):
    """vg_fe_tracks_step on a handle with the streams (pinhole, KB degree 9) against vg_fe_read_image_batch on a second handle with the
    same cameras, fed the lists the steps return: counts and un_xy bit-identical; the KB stream's velocities non-zero from the third
    frame on"""
    import fe_scene
    S, cap = 2, 160
    cams = [fe.Camera.pinhole(*cc.PIN8), camera("realsense", 320)]
    scenes = [fe_scene.moving_scene(n_frames, seed=50 + c, width=W, height=H, velocity=(2.4 + 0.5 * c, -1.1 + 0.7 * c)) for c in range(S)]
    kw = dict(max_cnt=60, min_dist=14, equalize=True)
    a, b = fe.FrontEnd(handle, W, H, S, cap), fe.FrontEnd(other, W, H, S, cap)
    for c in range(S):
        a.set_camera(c, cams[c]); b.set_camera(c, cams[c])
    a.tracks_begin()
    pts = [np.zeros((0, 2), np.float32)] * S
    moving = 0
    for k in range(n_frames):
        imgs = [scenes[c][k] for c in range(S)]
        got = a.tracks_step(imgs, [1.0 + 0.05 * k] * S, [True] * S, [cc.PIN8] * S, **kw)
        want = b.read_image_batch(imgs, pts, [True] * S, [cc.PIN8] * S, **kw)
        for c in range(S):
            assert got[c]["n"] == want[c]["n_final"] and got[c]["n1"] == want[c]["n1"] and got[c]["n2"] == want[c]["n2"], (c, k)
            assert cc.same_bits(got[c]["un_xy"], want[c]["un_xy"]), (c, k)
        assert cc.same_bits(got[1]["un_xy"], lifted_xy(got[1]["cur_xy"], params("realsense", 320))), k
        if k >= 2:
            n = int(np.count_nonzero(np.any(got[1]["vel_xy"] != 0, axis=1)))
            assert n >= 10, (k, n)
            moving += n
        pts = [got[c]["cur_xy"] for c in range(S)]
    return moving
