"""Shared by the camera-model tests (test_fe_camera_*.py, test_fe_read_image*_camera.py, test_fe_standalone_mei.py): the five MEI
cameras, the point set of the per-point check, CataCamera::liftProjective restated in NumPy double (CataCamera.cc:556-626, same expression
order as vins-mono_amd/csrc/fe_camera.h), the checks themselves -- each takes handles, so the `not gpu` tests run it in a child process on
handles of the emulated library and the `gpu` tests on the device -- and the child-process runner."""
import os
import subprocess
import sys

import numpy as np

from vins_mono_amd import fe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INTR = (310.0, 309.0, 158.0, 121.5)                     # gamma1 gamma2 u0 v0 at 320 x 240
DIST = (-0.11, 0.04, 2e-4, -1e-4)
NO_DIST = (0.0, 0.0, 0.0, 0.0)
# name -> (xi, distortion): A the general case, B the xi == 1.0 branch, C 1 - xi * xi < 0, D m_noDistortion, E = the pinhole
CAMS = {"A": (0.9, DIST), "B": (1.0, DIST), "C": (1.5, DIST), "D": (0.9, NO_DIST), "E": (0.0, DIST)}


def params(name, scale=1.0):
    """(xi, the eight numbers of vg_fe_camera::p) of a camera; `scale` multiplies the projection parameters (a larger frame)"""
    xi, dist = CAMS[name]
    return xi, tuple(v * scale for v in INTR) + tuple(dist)


def camera(name, scale=1.0):
    xi, p = params(name, scale)
    return fe.Camera.mei(xi, *p)


def points(width=320, height=240, n_random=512, seed=3):
    """every 8th pixel including the borders and the four corners, then seeded random sub-pixel positions, float32"""
    xs = sorted(set(range(0, width, 8)) | {width - 1})
    ys = sorted(set(range(0, height, 8)) | {height - 1})
    grid = np.array([[x, y] for y in ys for x in xs], np.float32)
    rng = np.random.default_rng(seed)
    rnd = np.stack([rng.uniform(0, width - 1, n_random), rng.uniform(0, height - 1, n_random)], 1).astype(np.float32)
    return np.concatenate([grid, rnd])


def lift64(pts, xi, p):
    """CataCamera::liftProjective in double: the ray (x, y, z) of float32 pixels"""
    g1, g2, u0, v0, k1, k2, p1, p2 = [np.float64(v) for v in p]
    xi = np.float64(xi)
    q = np.asarray(pts, np.float32).astype(np.float64).reshape(-1, 2)
    mx_d = (1.0 / g1) * q[:, 0] + (-u0 / g1)
    my_d = (1.0 / g2) * q[:, 1] + (-v0 / g2)
    mx_u, my_u = mx_d.copy(), my_d.copy()
    if not (k1 == 0.0 and k2 == 0.0 and p1 == 0.0 and p2 == 0.0):
        for _ in range(8):
            mx2, my2, mxy = mx_u * mx_u, my_u * my_u, mx_u * my_u
            rho2 = mx2 + my2
            rad = k1 * rho2 + k2 * rho2 * rho2
            dx = mx_u * rad + 2.0 * p1 * mxy + p2 * (rho2 + 2.0 * mx2)
            dy = my_u * rad + 2.0 * p2 * mxy + p1 * (rho2 + 2.0 * my2)
            mx_u, my_u = mx_d - dx, my_d - dy
    if xi == 1.0:
        z = (1.0 - mx_u * mx_u - my_u * my_u) / 2.0
    else:
        rho2 = mx_u * mx_u + my_u * my_u
        z = 1.0 - xi * (rho2 + 1.0) / (xi + np.sqrt(1.0 + (1.0 - xi * xi) * rho2))
    return mx_u, my_u, z


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- per-point lift (test_fe_camera_lift.py)
def check_lift_against_reference(handle, tmp_dir, names="ABCD"):
    """vg_fe_lift against the reference's CataCamera (oracle/_ref/libvins_ref_fe.so): identical float bit patterns"""
    from oracle import ref_fe as RF
    pts = points()
    tr = fe.FrontEnd(handle, 320, 240, 1, len(pts))
    for name in names:
        xi, p = params(name)
        cfg = RF.write_config(os.path.join(tmp_dir, "cam_%s.yaml" % name), width=320, height=240, intr=p[:4], dist=p[4:], mei_xi=xi)
        ray = RF.Node(RF.lib(), cfg).lift(pts)
        want = np.stack([ray[:, 0] / ray[:, 2], ray[:, 1] / ray[:, 2]], 1).astype(np.float32)
        assert np.isfinite(want).all() and np.isfinite(ray).all(), name                     # fixture condition (on the reference's output)
        # the NumPy restatement the other tests compose frames with is the reference's function too
        x, y, z = lift64(pts, xi, p)
        assert np.array_equal(np.stack([x, y, z], 1).view(np.uint64), ray.view(np.uint64)), name
        got = tr.lift(pts, camera(name))
        bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(1))
        assert len(bad) == 0, (name, len(bad), pts[bad[:4]], got[bad[:4]], want[bad[:4]])
    return len(pts)


def check_lift_xi_zero_is_the_pinhole(handle):
    """camera E: model MEI with xi = 0.0 has z exactly 1.0, so vg_fe_lift equals vg_fe_undistort with the same eight numbers"""
    pts = points()
    tr = fe.FrontEnd(handle, 320, 240, 1, len(pts))
    xi, p = params("E")
    got = tr.lift(pts, camera("E"))
    assert same_bits(got, tr.undistort(pts, p))
    assert same_bits(got, tr.lift(pts, fe.Camera.pinhole(*p)))
    return len(pts)


# ---- the contract of vg_fe_set_camera / vg_fe_lift (test_fe_camera_abi.py)
PIN8 = (196.4, 195.9, 154.5, 124.0, -2.917e-01, 8.228e-02, 5.333e-05, -1.578e-04)       # a pinhole at 320 x 240
BAD_ARG = -1


def next_points(out, publish):
    """cur_pts of the following frame from a read_image result (order == None: the list as it stands)"""
    surv = out["forw_xy"][out["status_lk"] != 0]
    if not publish:
        return surv
    if out["ransac_ran"]:
        surv = surv[out["status_f"] != 0]
    return np.concatenate([surv[out["kept"]], out["new_xy"]]) if len(out["kept"]) + len(out["new_xy"]) else np.zeros((0, 2), np.float32)


def same_frame(a, b, what):
    for k in ("n1", "n2", "ransac_ran", "n_kept", "n_new", "n_final", "fallback", "ransac_best", "ransac_niters"):
        assert a[k] == b[k], (what, k, a[k], b[k])
    for k in ("status_lk", "status_f", "kept"):
        assert (a[k] is None) == (b[k] is None) and (a[k] is None or np.array_equal(a[k], b[k])), (what, k)
    for k in ("forw_xy", "new_xy", "un_xy"):
        assert (a[k] is None) == (b[k] is None) and (a[k] is None or same_bits(a[k], b[k])), (what, k)


def _two_frames(tr, frames, between=None, intr=PIN8):
    """frame 0 (published, no points), `between(tr)`, frame 1 (published, the points of frame 0): the two results"""
    o0 = tr.read_image(frames[0], np.zeros((0, 2), np.float32), True, intr, max_cnt=60, min_dist=14, equalize=True)
    if between is not None:
        between(tr)
    o1 = tr.read_image(frames[1], next_points(o0, True), True, intr, max_cnt=60, min_dist=14, equalize=True)
    assert o1["ransac_ran"] and not o1["fallback"] and o1["n2"] >= 15, o1      # (the frame lifts on every path: rejectWithF and the final list)
    return o0, o1


def check_abi(handle, bare_handle):
    """`bare_handle`: a handle vg_fe_configure has never seen"""
    import ctypes as C
    import fe_scene
    frames = fe_scene.moving_scene(2, seed=6, width=320, height=240, velocity=(2.9, 1.3))
    lib = handle.lib
    new = lambda: fe.FrontEnd(handle, 320, 240, 1, 160)
    pts = points(n_random=8)[:64]
    # the yardsticks: a stream that never had a camera, and one with camera A
    tr = new()
    pin = _two_frames(tr, frames)
    tr = new()
    tr.set_camera(0, camera("A"))
    mei = _two_frames(tr, frames)
    assert not same_bits(pin[1]["un_xy"], mei[1]["un_xy"])                     # (the camera matters)
    lifted = tr.lift(pts, camera("A"))

    def refused(tr):
        good = camera("A")
        out = np.full((len(pts), 2), 7.0, np.float32)
        f4 = C.POINTER(C.c_float)

        lib.vg_last_error.restype = C.c_char_p

        def both(c, why):
            assert lib.vg_fe_set_camera(tr.h, 0, C.byref(c)) == BAD_ARG, why
            assert b"vg_fe_set_camera" in lib.vg_last_error(tr.h), why
            assert lib.vg_fe_lift(tr.h, C.byref(c), pts.ctypes.data_as(f4), len(pts), out.ctypes.data_as(f4)) == BAD_ARG, why
            assert (out == 7.0).all(), why                                     # nothing was written

        c = camera("B"); c.struct_size -= 8; both(c, "struct_size")
        c = camera("B"); c.struct_size = 0; both(c, "struct_size 0")
        c = camera("B"); c.model = 2; both(c, "unknown model")
        c = camera("B"); c.model = -1; both(c, "unknown model")
        for i in range(8):
            for v in (float("nan"), float("inf")):
                c = camera("B"); c.p[i] = v; both(c, "non-finite p[%d]" % i)
        c = camera("B"); c.xi = float("nan"); both(c, "non-finite xi")
        c = camera("B"); c.xi = float("-inf"); both(c, "non-finite xi")
        c = camera("B"); c.p[0] = 0.0; both(c, "zero p[0]")
        c = camera("B"); c.p[1] = -0.0; both(c, "zero p[1]")
        for cam in (-1, 1, 1 << 20):
            assert lib.vg_fe_set_camera(tr.h, cam, C.byref(good)) == BAD_ARG, cam
            assert b"vg_fe_set_camera" in lib.vg_last_error(tr.h), cam
        # a handle that is not configured
        assert lib.vg_fe_set_camera(bare_handle.h, 0, C.byref(good)) == BAD_ARG
        assert lib.vg_fe_lift(bare_handle.h, C.byref(good), pts.ctypes.data_as(f4), len(pts), out.ctypes.data_as(f4)) == BAD_ARG
        assert (out == 7.0).all()
        assert lib.vg_fe_lift(tr.h, None, pts.ctypes.data_as(f4), len(pts), out.ctypes.data_as(f4)) == BAD_ARG
        # vg_fe_lift's capacity rule is vg_fe_undistort's: at most n_cams * max_points points
        assert lib.vg_fe_lift(tr.h, C.byref(good), pts.ctypes.data_as(f4), 161, out.ctypes.data_as(f4)) == BAD_ARG

    # every refusal leaves the stream's camera and state alone: the next frame is the one of a run without the refused calls
    tr = new()
    tr.set_camera(0, camera("A"))
    got = _two_frames(tr, frames, between=refused)
    same_frame(got[0], mei[0], "refused/0"); same_frame(got[1], mei[1], "refused/1")
    assert same_bits(tr.lift(pts, camera("A")), lifted)
    # ... also on a stream that has no camera
    tr = new()
    got = _two_frames(tr, frames, between=refused)
    same_frame(got[1], pin[1], "refused, no camera")
    # set_camera(NULL) returns the stream to the pinhole of intr
    tr = new()
    tr.set_camera(0, camera("A"))
    got = _two_frames(tr, frames, between=lambda t: t.set_camera(0, None))
    same_frame(got[0], mei[0], "null/0"); same_frame(got[1], pin[1], "null/1")
    # so does a fresh vg_fe_configure (`tr` is configured with a camera at this point)
    tr.set_camera(0, camera("C"))
    got = _two_frames(new(), frames)
    same_frame(got[0], pin[0], "configure/0"); same_frame(got[1], pin[1], "configure/1")
    # a PINHOLE vg_fe_camera = the same numbers in intr (which the stream then ignores)
    tr = new()
    c = fe.Camera.pinhole(*PIN8)
    c.xi = float("nan")                                                        # (ignored for PINHOLE, as documented)
    tr.set_camera(0, c)
    got = _two_frames(tr, frames, intr=(1.0, 1.0, 0.0, 0.0, 0.5, 0.5, 0.5, 0.5))
    same_frame(got[0], pin[0], "pinhole/0"); same_frame(got[1], pin[1], "pinhole/1")
    # the camera= argument of the binding is set_camera + the call
    tr = new()
    o0 = tr.read_image(frames[0], np.zeros((0, 2), np.float32), True, None, max_cnt=60, min_dist=14, equalize=True, camera=camera("A"))
    same_frame(o0, mei[0], "camera=")
    return True


# ---- mixed camera models in one batched call (test_fe_read_image_batch_camera.py)
def check_batch(handle, other, W=320, H=240, scale=1.0, n_frames=4):
    """one handle with four streams -- no camera (the pinhole of intr), A, B, D -- through vg_fe_read_image_batch against every stream alone
    through vg_fe_read_image on a single-stream handle with the same camera; publishing and non-publishing steps alternate"""
    import fe_scene
    S, cap = 4, 160
    md = int(round(14 * W / 320.0))
    pin = tuple(v * (scale if i < 4 else 1.0) for i, v in enumerate(PIN8))
    cams = [None, camera("A", scale), camera("B", scale), camera("D", scale)]
    scenes = [fe_scene.moving_scene(n_frames, seed=40 + c, width=W, height=H, velocity=((2.0 + 0.4 * c) * W / 320.0, (-1.0 + 0.6 * c) * W / 320.0))
              for c in range(S)]
    kw = dict(max_cnt=60, min_dist=md, equalize=True)
    alone = []
    for c in range(S):
        tr = fe.FrontEnd(other, W, H, 1, cap)
        if cams[c] is not None:
            tr.set_camera(0, cams[c])
        pts, outs = np.zeros((0, 2), np.float32), []
        for k in range(n_frames):
            outs.append(tr.read_image(scenes[c][k], pts, k % 2 == 0, pin, **kw))
            pts = next_points(outs[-1], k % 2 == 0)
        alone.append(outs)
    tr = fe.FrontEnd(handle, W, H, S, cap)
    for c in range(S):
        if cams[c] is not None:
            tr.set_camera(c, cams[c])
    pts = [np.zeros((0, 2), np.float32)] * S
    ransac = 0
    for k in range(n_frames):
        pub = k % 2 == 0
        outs = tr.read_image_batch([scenes[c][k] for c in range(S)], pts, [pub] * S, [pin] * S, **kw)
        for c in range(S):
            same_frame(outs[c], alone[c][k], ("stream", c, "frame", k))
            ransac += int(outs[c]["ransac_ran"] and not outs[c]["fallback"])
        pts = [next_points(outs[c], pub) for c in range(S)]
    assert ransac >= S                                                          # every stream lifted both point sets for rejectWithF
    # the models made a difference: the same pixels lift differently on the four streams
    last = [alone[c][-1]["un_xy"] for c in range(S)]
    assert all(len(v) >= 30 for v in last)
    return True


# ---- child processes on the emulated library
_CHILD = r"""
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import conftest
import %(module)s as case
H = conftest._simt_handle
print("RESULT", repr(%(call)s))
"""


def run_emulated(module, call, timeout=2400):
    """`call` (an expression over `case` = the module and `H()` = a new handle of the emulated library) in a child process; its value"""
    r = subprocess.run([sys.executable, "-c", _CHILD % dict(root=ROOT, module=module, call=call)], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and "RESULT" in r.stdout, r.stdout[-3000:] + r.stderr[-5000:]
    return eval(r.stdout[r.stdout.index("RESULT") + 6:].strip().splitlines()[0])
