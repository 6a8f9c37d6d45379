"""ctypes binding of the front-end entry points of include/vinsgpu.h (vg_fe_*); no arithmetic lives here."""
import ctypes as C

import numpy as np

_u8 = C.POINTER(C.c_uint8)
_f4 = C.POINTER(C.c_float)
_i4 = C.POINTER(C.c_int)


class FrameOut(C.Structure):
    """vg_fe_frame_out (include/vinsgpu.h)"""
    _fields_ = [("n1", C.c_int), ("n2", C.c_int), ("ransac_ran", C.c_int), ("n_kept", C.c_int), ("n_new", C.c_int), ("n_final", C.c_int),
                ("status_lk", _u8), ("status_f", _u8), ("forw_xy", _f4), ("kept", _i4), ("new_xy", _f4), ("un_xy", _f4),
                ("ransac_best", C.c_int), ("ransac_niters", C.c_int), ("fallback", C.c_int)]


ORDER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(FrameOut), _i4)


class FrameIn(C.Structure):
    """vg_fe_frame_in (include/vinsgpu.h)"""
    _fields_ = [("struct_size", C.c_int), ("img", _u8), ("stride", C.c_int), ("equalize", C.c_int), ("publish", C.c_int), ("cur_xy", _f4),
                ("n", C.c_int), ("max_cnt", C.c_int), ("min_dist", C.c_int), ("quality", C.c_double), ("f_threshold", C.c_double),
                ("focal_length", C.c_double), ("intr", C.c_double * 8), ("base_mask", _u8), ("order", ORDER_FN), ("user", C.c_void_p)]


TRACKS_ORDER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, _i4, _i4)
_f8 = C.POINTER(C.c_double)


class TracksIn(C.Structure):
    """vg_fe_tracks_in (include/vinsgpu.h)"""
    _fields_ = [("struct_size", C.c_int), ("img", _u8), ("stride", C.c_int), ("equalize", C.c_int), ("publish", C.c_int), ("max_cnt", C.c_int),
                ("min_dist", C.c_int), ("quality", C.c_double), ("f_threshold", C.c_double), ("focal_length", C.c_double), ("intr", C.c_double * 8),
                ("base_mask", _u8), ("order", TRACKS_ORDER_FN), ("user", C.c_void_p), ("stamp", C.c_double)]


class TracksOut(C.Structure):
    """vg_fe_tracks_out (include/vinsgpu.h)"""
    _fields_ = [("n", C.c_int), ("n_id", C.c_int), ("n_msg", C.c_int), ("n1", C.c_int), ("n2", C.c_int), ("ransac_ran", C.c_int), ("n_kept", C.c_int),
                ("n_new", C.c_int), ("fallback", C.c_int), ("ransac_best", C.c_int), ("ransac_niters", C.c_int),
                ("ids", _i4), ("track_cnt", _i4), ("cur_xy", _f4), ("un_xy", _f4), ("vel_xy", _f4), ("msg_id", _i4), ("msg_obs", _f8)]


class VioIn(C.Structure):
    """vg_vio_in (include/vinsgpu.h)"""
    _fields_ = [("struct_size", C.c_int), ("n_samples", C.c_int), ("samples", _f8), ("fe", TracksIn)]


class VioOut(C.Structure):
    """vg_vio_out (include/vinsgpu.h)"""
    _fields_ = [("fe", TracksOut)]


VG_VIO_LISTS = 1


class TracksState(C.Structure):
    """vg_fe_tracks_state (include/vinsgpu.h)"""
    _fields_ = [("struct_size", C.c_int), ("n", C.c_int), ("n_id", C.c_int), ("prev_time", C.c_double), ("cur_xy", _f4), ("ids", _i4),
                ("track_cnt", _i4), ("un_xy", _f4), ("in_map", _u8)]


CAM_PINHOLE, CAM_MEI, CAM_KANNALA_BRANDT = 0, 1, 3


class Camera(C.Structure):
    """vg_fe_camera (include/vinsgpu.h): Camera.pinhole(fx, fy, cx, cy, k1, k2, p1, p2), Camera.mei(xi, gamma1, gamma2, u0, v0, k1, k2, p1, p2)
    or Camera.kannala_brandt(mu, mv, u0, v0, k2, k3, k4, k5)"""
    _fields_ = [("struct_size", C.c_int), ("model", C.c_int), ("p", C.c_double * 8), ("xi", C.c_double)]

    @classmethod
    def make(cls, model, p, xi=0.0):
        c = cls()
        c.struct_size, c.model, c.xi = C.sizeof(cls), int(model), float(xi)
        for i, v in enumerate(p):
            c.p[i] = float(v)
        return c

    @classmethod
    def pinhole(cls, *p):
        return cls.make(CAM_PINHOLE, p)

    @classmethod
    def mei(cls, xi, *p):
        return cls.make(CAM_MEI, p, xi)

    @classmethod
    def kannala_brandt(cls, mu, mv, u0, v0, k2, k3, k4, k5):
        return cls.make(CAM_KANNALA_BRANDT, (mu, mv, u0, v0, k2, k3, k4, k5))


class FrontEnd:
    """`n_cams` camera streams on one vg_handle (ba.Handle)."""

    def __init__(self, handle, width, height, n_cams=1, max_points=150):
        self.hd, self.lib, self.h = handle, handle.lib, handle.h
        self.W, self.H, self.cams, self.max_pts = width, height, n_cams, max_points
        L = self.lib
        L.vg_fe_configure.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        L.vg_fe_push_frames.argtypes = [C.c_void_p, C.POINTER(_u8), C.c_int, C.c_int]
        L.vg_fe_upload_frames.argtypes = [C.c_void_p, C.POINTER(_u8), C.c_int]
        L.vg_fe_build_async.argtypes = [C.c_void_p, C.c_int]
        L.vg_fe_select_frames.argtypes = [C.c_void_p, C.c_int]
        L.vg_fe_frame_slot.argtypes = [C.c_void_p]
        L.vg_fe_track.argtypes = [C.c_void_p, C.c_int, _f4, C.c_int, _f4, _u8, _f4]
        L.vg_fe_track_upload.argtypes = [C.c_void_p, _f4, _i4]
        L.vg_fe_track_async.argtypes = [C.c_void_p]
        L.vg_fe_track_download.argtypes = [C.c_void_p, _f4, _u8, _f4]
        L.vg_fe_detect.argtypes = [C.c_void_p, C.c_int, _u8, C.c_int, C.c_double, C.c_double, _f4, _i4]
        L.vg_fe_detect_upload.argtypes = [C.c_void_p, C.POINTER(_u8), _i4]
        L.vg_fe_detect_async.argtypes = [C.c_void_p, C.c_double, C.c_double]
        L.vg_fe_detect_download.argtypes = [C.c_void_p, _f4, _i4]
        L.vg_fe_get_level.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, _u8, _i4, _i4]
        L.vg_fe_get_eig.argtypes = [C.c_void_p, C.c_int, _f4]
        L.vg_fe_keep_eig.argtypes = [C.c_void_p, C.c_int]
        L.vg_fe_set_mask.argtypes = [C.c_void_p, _f4, _i4, _i4, C.POINTER(_u8), C.c_int, _i4, _i4]
        L.vg_fe_detect_masked.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, _f4, _i4]
        L.vg_fe_get_mask.argtypes = [C.c_void_p, C.c_int, _u8]
        L.vg_fe_undistort.argtypes = [C.c_void_p, _f4, C.c_int, C.POINTER(C.c_double), _f4]
        L.vg_fe_reject_with_f.argtypes = [C.c_void_p, _f4, _f4, C.c_int, C.c_double, _u8, _i4, C.POINTER(C.c_double)]
        L.vg_fe_read_image.argtypes = [C.c_void_p, C.POINTER(FrameIn), C.POINTER(FrameOut)]
        if hasattr(L, "vg_fe_read_image_batch"):          # (a library built before the batched call: read_image_batch() raises AttributeError)
            L.vg_fe_read_image_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(FrameIn), C.POINTER(FrameOut)]
        if hasattr(L, "vg_fe_set_camera"):                # (a library built before the camera models: set_camera() / lift() raise AttributeError)
            L.vg_fe_set_camera.argtypes = [C.c_void_p, C.c_int, C.POINTER(Camera)]
            L.vg_fe_lift.argtypes = [C.c_void_p, C.POINTER(Camera), _f4, C.c_int, _f4]
        if hasattr(L, "vg_fe_tracks_step"):               # (a library built before the resident track lists: tracks_*() raise AttributeError)
            L.vg_fe_tracks_begin.argtypes = [C.c_void_p]
            L.vg_fe_tracks_step.argtypes = [C.c_void_p, C.c_int, C.POINTER(TracksIn), C.POINTER(TracksOut)]
            L.vg_fe_tracks_get.argtypes = [C.c_void_p, C.c_int, C.POINTER(TracksState)]
            L.vg_fe_tracks_set.argtypes = [C.c_void_p, C.c_int, C.POINTER(TracksState)]
        if hasattr(L, "vg_vio_step_async"):               # (a library built before the one-call path: vio_step() raises AttributeError)
            L.vg_vio_step_async.argtypes = [C.c_void_p, C.c_int, C.POINTER(VioIn), C.POINTER(VioOut)]
        self.hd._chk(L.vg_fe_configure(self.h, width, height, n_cams, max_points), "vg_fe_configure")

    def _imgs(self, frames):
        self._keep = [np.ascontiguousarray(f, np.uint8) for f in frames]
        assert len(self._keep) == self.cams and all(f.shape == (self.H, self.W) for f in self._keep)
        return (_u8 * self.cams)(*[f.ctypes.data_as(_u8) for f in self._keep])

    def push_frames(self, frames, equalize=False):
        self.hd._chk(self.lib.vg_fe_push_frames(self.h, self._imgs(frames), self.W, int(equalize)), "vg_fe_push_frames")

    def upload_frames(self, frames):
        self.hd._chk(self.lib.vg_fe_upload_frames(self.h, self._imgs(frames), self.W), "vg_fe_upload_frames")

    def frame_slot(self):
        """The frame slot the last upload went into (vg_fe_frame_slot)."""
        return int(self.lib.vg_fe_frame_slot(self.h))

    def select_frames(self, slot):
        self.hd._chk(self.lib.vg_fe_select_frames(self.h, int(slot)), "vg_fe_select_frames")

    def build_async(self, equalize=False):
        self.hd._chk(self.lib.vg_fe_build_async(self.h, int(equalize)), "vg_fe_build_async")

    def track(self, cam, pts):
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
        n = pts.shape[0]
        out, st, err = np.zeros((n, 2), np.float32), np.zeros(n, np.uint8), np.zeros(n, np.float32)
        self.hd._chk(self.lib.vg_fe_track(self.h, cam, pts.ctypes.data_as(_f4), n, out.ctypes.data_as(_f4), st.ctypes.data_as(_u8),
                                          err.ctypes.data_as(_f4)), "vg_fe_track")
        return out, st, err

    def track_upload(self, pts_list):
        buf = np.zeros((self.cams, self.max_pts, 2), np.float32)
        n = np.zeros(self.cams, np.int32)
        for c, p in enumerate(pts_list):
            p = np.asarray(p, np.float32).reshape(-1, 2)
            buf[c, :p.shape[0]] = p
            n[c] = p.shape[0]
        self._n = n
        self.hd._chk(self.lib.vg_fe_track_upload(self.h, buf.ctypes.data_as(_f4), n.ctypes.data_as(_i4)), "vg_fe_track_upload")

    def track_async(self):
        self.hd._chk(self.lib.vg_fe_track_async(self.h), "vg_fe_track_async")

    def track_download(self):
        out = np.zeros((self.cams, self.max_pts, 2), np.float32)
        st = np.zeros((self.cams, self.max_pts), np.uint8)
        err = np.zeros((self.cams, self.max_pts), np.float32)
        self.hd._chk(self.lib.vg_fe_track_download(self.h, out.ctypes.data_as(_f4), st.ctypes.data_as(_u8), err.ctypes.data_as(_f4)), "vg_fe_track_download")
        return [(out[c, :self._n[c]], st[c, :self._n[c]], err[c, :self._n[c]]) for c in range(self.cams)]

    def detect(self, cam, max_corners, quality=0.01, min_dist=30.0, mask=None):
        out = np.zeros((max(max_corners, 1), 2), np.float32)
        n = C.c_int(0)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        self.hd._chk(self.lib.vg_fe_detect(self.h, cam, m.ctypes.data_as(_u8) if m is not None else None, int(max_corners), float(quality),
                                           float(min_dist), out.ctypes.data_as(_f4), C.byref(n)), "vg_fe_detect")
        return out[:n.value].copy()

    def set_mask(self, pts, track_cnt, radius, base_masks=None):
        """FeatureTracker::setMask for every stream: pts[c] (n_c x 2 float32), track_cnt[c] (n_c ints).  Returns the list
        of kept-index arrays (kept order); the final masks stay on the device for detect_masked()."""
        P = np.zeros((self.cams, self.max_pts, 2), np.float32)
        T = np.zeros((self.cams, self.max_pts), np.int32)
        n = np.zeros(self.cams, np.int32)
        for c in range(self.cams):
            p = np.ascontiguousarray(pts[c], np.float32).reshape(-1, 2)
            n[c] = len(p)
            P[c, :len(p)] = p
            T[c, :len(p)] = np.asarray(track_cnt[c], np.int32)
        bp = None
        if base_masks is not None:
            self._bkeep = [None if m is None else np.ascontiguousarray(m, np.uint8) for m in base_masks]
            bp = (_u8 * self.cams)(*[None if m is None else m.ctypes.data_as(_u8) for m in self._bkeep])
        K = np.zeros((self.cams, self.max_pts), np.int32)
        nk = np.zeros(self.cams, np.int32)
        self.hd._chk(self.lib.vg_fe_set_mask(self.h, P.ctypes.data_as(_f4), T.ctypes.data_as(_i4), n.ctypes.data_as(_i4), bp, int(radius),
                                             K.ctypes.data_as(_i4), nk.ctypes.data_as(_i4)), "vg_fe_set_mask")
        return [K[c, :nk[c]].copy() for c in range(self.cams)]

    def detect_masked(self, cam, max_corners, quality=0.01, min_dist=30.0):
        out = np.zeros((max(max_corners, 1), 2), np.float32)
        n = C.c_int(0)
        self.hd._chk(self.lib.vg_fe_detect_masked(self.h, cam, int(max_corners), float(quality), float(min_dist), out.ctypes.data_as(_f4),
                                                  C.byref(n)), "vg_fe_detect_masked")
        return out[:n.value].copy()

    def get_mask(self, cam):
        out = np.zeros((self.H, self.W), np.uint8)
        self.hd._chk(self.lib.vg_fe_get_mask(self.h, cam, out.ctypes.data_as(_u8)), "vg_fe_get_mask")
        return out

    def undistort(self, pts, intr):
        p = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
        out = np.zeros_like(p)
        k = np.ascontiguousarray(intr, np.float64)
        self.hd._chk(self.lib.vg_fe_undistort(self.h, p.ctypes.data_as(_f4), len(p), k.ctypes.data_as(C.POINTER(C.c_double)),
                                              out.ctypes.data_as(_f4)), "vg_fe_undistort")
        return out

    def set_camera(self, cam, camera):
        """vg_fe_set_camera: stream `cam` lifts with `camera` (a Camera) from now on; None: back to the pinhole of the frames' intr."""
        self.hd._chk(self.lib.vg_fe_set_camera(self.h, int(cam), None if camera is None else C.byref(camera)), "vg_fe_set_camera")

    def lift(self, pts, camera):
        """vg_fe_lift: (x / z, y / z) of `camera`'s liftProjective, float32 [n, 2]"""
        p = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
        out = np.zeros_like(p)
        self.hd._chk(self.lib.vg_fe_lift(self.h, C.byref(camera), p.ctypes.data_as(_f4), len(p), out.ctypes.data_as(_f4)), "vg_fe_lift")
        return out

    def reject_with_f(self, p1, p2, threshold=1.0):
        """FeatureTracker::rejectWithF's findFundamentalMat(FM_RANSAC, threshold, 0.99) on the device (deterministic RANSAC).
        p1, p2: [n, 2] float32 virtual-pinhole pixel coordinates.  Returns (status u8 [n], F 3x3)."""
        p1 = np.ascontiguousarray(p1, np.float32).reshape(-1, 2)
        p2 = np.ascontiguousarray(p2, np.float32).reshape(-1, 2)
        n = p1.shape[0]
        st = np.zeros(n, np.uint8)
        Fm = np.zeros(9)
        ni = C.c_int()
        self.hd._chk(self.lib.vg_fe_reject_with_f(self.h, p1.ctypes.data_as(_f4), p2.ctypes.data_as(_f4), n, float(threshold),
                                                  st.ctypes.data_as(_u8), C.byref(ni), Fm.ctypes.data_as(C.POINTER(C.c_double))),
                     "vg_fe_reject_with_f")
        return st, Fm.reshape(3, 3)

    def read_image(self, img, cur_pts, publish, intr, max_cnt=150, min_dist=30, equalize=False, f_threshold=1.0, focal_length=460.0,
                   quality=0.01, base_mask=None, order=None, camera=None):
        """vg_fe_read_image: FeatureTracker::readImage of one stream in one call.  `order(status_lk, status_f or None, forw_xy, n2)` returns
        the walk order of setMask as indices into the n2 survivors (None: the list as it stands).  `camera`: a Camera that is set on the
        stream first (set_camera; it stays), `intr` may then be None.  Returns a dict of numpy copies."""
        if camera is not None:
            self.set_camera(0, camera)
        img = np.ascontiguousarray(img, np.uint8)
        assert img.shape == (self.H, self.W)
        pts = np.ascontiguousarray(cur_pts, np.float32).reshape(-1, 2)
        n = pts.shape[0]
        fin = FrameIn()
        fin.struct_size = C.sizeof(FrameIn)
        fin.img = img.ctypes.data_as(_u8); fin.stride = self.W; fin.equalize = int(equalize); fin.publish = int(publish)
        fin.cur_xy = pts.ctypes.data_as(_f4) if n else None
        fin.n = n; fin.max_cnt = int(max_cnt); fin.min_dist = int(min_dist); fin.quality = float(quality)
        fin.f_threshold = float(f_threshold); fin.focal_length = float(focal_length)
        for i, v in enumerate(intr if intr is not None else ()):
            fin.intr[i] = float(v)
        if base_mask is not None:
            self._base = np.ascontiguousarray(base_mask, np.uint8)
            assert self._base.shape == (self.H, self.W)
            fin.base_mask = self._base.ctypes.data_as(_u8)
        seen = {}

        def _cb(_user, after, out_order):
            a = after.contents
            st = np.ctypeslib.as_array(a.status_lk, (max(n, 1),))[:n].copy()
            sf = np.ctypeslib.as_array(a.status_f, (max(a.n1, 1),))[:a.n1].copy() if a.ransac_ran else None
            fw = np.ctypeslib.as_array(a.forw_xy, (max(n, 1), 2))[:n].copy()
            perm = np.asarray(order(st, sf, fw, a.n2), np.int32)
            seen["n2"] = a.n2
            if perm.shape != (a.n2,):
                return 1
            for q in range(a.n2):
                out_order[q] = int(perm[q])
            return 0

        cb = ORDER_FN(_cb) if order is not None else C.cast(None, ORDER_FN)
        fin.order = cb
        fo = FrameOut()
        self.hd._chk(self.lib.vg_fe_read_image(self.h, C.byref(fin), C.byref(fo)), "vg_fe_read_image")

        def arr(ptr, shape):
            m = int(np.prod(shape))
            return np.ctypeslib.as_array(ptr, shape).copy() if m and ptr else np.zeros(shape, np.float32 if len(shape) == 2 else np.int32)

        out = dict(n1=fo.n1, n2=fo.n2, ransac_ran=bool(fo.ransac_ran), n_kept=fo.n_kept, n_new=fo.n_new, n_final=fo.n_final,
                   ransac_best=fo.ransac_best, ransac_niters=fo.ransac_niters, fallback=fo.fallback)
        out["status_lk"] = arr(fo.status_lk, (n,)).astype(np.uint8)
        out["status_f"] = arr(fo.status_f, (fo.n1,)).astype(np.uint8) if fo.ransac_ran else None
        out["forw_xy"] = arr(fo.forw_xy, (n, 2))
        out["kept"] = arr(fo.kept, (fo.n_kept,)).astype(np.int32) if publish else None
        out["new_xy"] = arr(fo.new_xy, (fo.n_new, 2)) if publish else None
        out["un_xy"] = arr(fo.un_xy, (fo.n_final, 2))
        return out

    def read_image_batch(self, imgs, cur_pts_list, publish_list, intr_list, max_cnt=150, min_dist=30, equalize=False, f_threshold=1.0,
                         focal_length=460.0, quality=0.01, base_masks=None, orders=None, n_streams=None, cameras=None):
        """vg_fe_read_image_batch: FeatureTracker::readImage of every stream of the handle in one call.  imgs: one frame per stream, or None
        for the frames the last upload_frames() left on the device (a list may hold None entries: the library refuses a mixture).
        cur_pts_list / publish_list / intr_list: one entry per stream.  max_cnt, min_dist, equalize, f_threshold, focal_length, quality: one
        value for all streams or a list (the library wants equalize uniform, and quality / min_dist uniform over the publishing streams).
        base_masks / orders: None or lists with None entries; orders[c] as `order` of read_image().  n_streams: what is passed to the
        library (default: the number of list entries).  cameras: None or a list with a Camera (set on that stream first; it stays) or None
        per stream; intr_list[c] may be None for a stream with a camera.  Returns the list of the dictionaries read_image() returns."""
        for c, cam in enumerate(cameras or ()):
            if cam is not None:
                self.set_camera(c, cam)
        S = len(cur_pts_list) if n_streams is None else int(n_streams)
        m = len(cur_pts_list)

        def per(v):
            return list(v) if isinstance(v, (list, tuple, np.ndarray)) else [v] * m

        max_cnt, min_dist, equalize, f_threshold, focal_length, quality = [per(v) for v in (max_cnt, min_dist, equalize, f_threshold, focal_length, quality)]
        frames = [None] * m if imgs is None else [None if f is None else np.ascontiguousarray(f, np.uint8) for f in imgs]
        masks = [None] * m if base_masks is None else [None if b is None else np.ascontiguousarray(b, np.uint8) for b in base_masks]
        orders = [None] * m if orders is None else list(orders)
        pts = [np.ascontiguousarray(p, np.float32).reshape(-1, 2) for p in cur_pts_list]
        assert len(frames) == m and len(publish_list) == m and len(intr_list) == m and len(masks) == m and len(orders) == m
        assert all(f is None or f.shape == (self.H, self.W) for f in frames) and all(b is None or b.shape == (self.H, self.W) for b in masks)
        self._bkeep_batch = masks                      # (the library remembers the mask pointers it has uploaded)
        fin = (FrameIn * m)()
        cbs = []

        def make_cb(c):
            n, order = len(pts[c]), orders[c]

            def _cb(_user, after, out_order):
                try:
                    a = after.contents
                    st = np.ctypeslib.as_array(a.status_lk, (max(n, 1),))[:n].copy()
                    sf = np.ctypeslib.as_array(a.status_f, (max(a.n1, 1),))[:a.n1].copy() if a.ransac_ran else None
                    fw = np.ctypeslib.as_array(a.forw_xy, (max(n, 1), 2))[:n].copy()
                    perm = np.asarray(order(st, sf, fw, a.n2), np.int32)
                    if perm.shape != (a.n2,):
                        return 1
                    for q in range(a.n2):
                        out_order[q] = int(perm[q])
                    return 0
                except Exception:                      # (an exception must not travel through the C frames)
                    return 1

            return ORDER_FN(_cb)

        for c in range(m):
            f = fin[c]
            f.struct_size = C.sizeof(FrameIn)
            f.img = frames[c].ctypes.data_as(_u8) if frames[c] is not None else None
            f.stride = self.W; f.equalize = int(equalize[c]); f.publish = int(bool(publish_list[c]))
            f.cur_xy = pts[c].ctypes.data_as(_f4) if len(pts[c]) else None
            f.n = len(pts[c]); f.max_cnt = int(max_cnt[c]); f.min_dist = int(min_dist[c]); f.quality = float(quality[c])
            f.f_threshold = float(f_threshold[c]); f.focal_length = float(focal_length[c])
            for i, v in enumerate(intr_list[c] if intr_list[c] is not None else ()):
                f.intr[i] = float(v)
            if masks[c] is not None:
                f.base_mask = masks[c].ctypes.data_as(_u8)
            cbs.append(make_cb(c) if orders[c] is not None else C.cast(None, ORDER_FN))
            f.order = cbs[-1]
        fo = (FrameOut * m)()
        self.hd._chk(self.lib.vg_fe_read_image_batch(self.h, S, fin, fo), "vg_fe_read_image_batch")

        def arr(ptr, shape):
            k = int(np.prod(shape))
            return np.ctypeslib.as_array(ptr, shape).copy() if k and ptr else np.zeros(shape, np.float32 if len(shape) == 2 else np.int32)

        outs = []
        for c in range(m):
            o, n, publish = fo[c], len(pts[c]), bool(publish_list[c])
            out = dict(n1=o.n1, n2=o.n2, ransac_ran=bool(o.ransac_ran), n_kept=o.n_kept, n_new=o.n_new, n_final=o.n_final,
                       ransac_best=o.ransac_best, ransac_niters=o.ransac_niters, fallback=o.fallback)
            out["status_lk"] = arr(o.status_lk, (n,)).astype(np.uint8)
            out["status_f"] = arr(o.status_f, (o.n1,)).astype(np.uint8) if o.ransac_ran else None
            out["forw_xy"] = arr(o.forw_xy, (n, 2))
            out["kept"] = arr(o.kept, (o.n_kept,)).astype(np.int32) if publish else None
            out["new_xy"] = arr(o.new_xy, (o.n_new, 2)) if publish else None
            out["un_xy"] = arr(o.un_xy, (o.n_final, 2))
            outs.append(out)
        return outs

    # ---- track lists resident on the device
    def tracks_begin(self):
        """vg_fe_tracks_begin: every stream an empty list, n_id = 0, no previous map"""
        self.hd._chk(self.lib.vg_fe_tracks_begin(self.h), "vg_fe_tracks_begin")

    def tracks_step(self, imgs, stamps, publish_list, intr_list, max_cnt=150, min_dist=30, equalize=False, f_threshold=1.0, focal_length=460.0,
                    quality=0.01, base_masks=None, orders=None, n_streams=None, struct_size=None):
        """vg_fe_tracks_step: one frame for every stream from the resident lists.  imgs / publish_list / intr_list / the scalar options /
        base_masks as read_image_batch; stamps: _cur_time per stream; orders[c]: None or `order(track_cnt[n2]) -> permutation of range(n2)`
        (the incremented counts of the survivors of rejectWithF in list order).  Returns per stream a dict of numpy copies: n, n_id, ids,
        track_cnt, cur_xy, un_xy, vel_xy, msg_id, msg_obs and the diagnostics of vg_fe_tracks_out."""
        m = len(publish_list)
        S = m if n_streams is None else int(n_streams)
        tin, _keep = self._tracks_in(imgs, stamps, publish_list, intr_list, max_cnt, min_dist, equalize, f_threshold, focal_length, quality,
                                     base_masks, orders, struct_size)
        to = (TracksOut * m)()
        self.hd._chk(self.lib.vg_fe_tracks_step(self.h, S, tin, to), "vg_fe_tracks_step")
        return [self._tracks_out(to[c]) for c in range(m)]

    def _tracks_in(self, imgs, stamps, publish_list, intr_list, max_cnt, min_dist, equalize, f_threshold, focal_length, quality, base_masks,
                   orders, struct_size):
        """the vg_fe_tracks_in array of one step and what must outlive the call (frames, masks, callbacks)"""
        m = len(publish_list)

        def per(v):
            return list(v) if isinstance(v, (list, tuple, np.ndarray)) else [v] * m

        max_cnt, min_dist, equalize, f_threshold, focal_length, quality, stamps = [per(v) for v in (max_cnt, min_dist, equalize, f_threshold, focal_length, quality, stamps)]
        frames = [None] * m if imgs is None else [None if f is None else np.ascontiguousarray(f, np.uint8) for f in imgs]
        masks = [None] * m if base_masks is None else [None if b is None else np.ascontiguousarray(b, np.uint8) for b in base_masks]
        orders = [None] * m if orders is None else list(orders)
        assert len(frames) == m and len(intr_list) == m and len(masks) == m and len(orders) == m and len(stamps) == m
        assert all(f is None or f.shape == (self.H, self.W) for f in frames) and all(b is None or b.shape == (self.H, self.W) for b in masks)
        self._bkeep_batch = masks
        tin = (TracksIn * m)()
        cbs = []

        def make_cb(order):
            def _cb(_user, _stream, n2, cnt, out_order):
                try:
                    perm = np.asarray(order(np.ctypeslib.as_array(cnt, (max(n2, 1),))[:n2].copy()), np.int32)
                    if perm.shape != (n2,):
                        return 1
                    for q in range(n2):
                        out_order[q] = int(perm[q])
                    return 0
                except Exception:                      # (an exception must not travel through the C frames)
                    return 1

            return TRACKS_ORDER_FN(_cb)

        for c in range(m):
            f = tin[c]
            f.struct_size = C.sizeof(TracksIn) if struct_size is None else int(struct_size)
            f.img = frames[c].ctypes.data_as(_u8) if frames[c] is not None else None
            f.stride = self.W; f.equalize = int(equalize[c]); f.publish = int(bool(publish_list[c]))
            f.max_cnt = int(max_cnt[c]); f.min_dist = int(min_dist[c]); f.quality = float(quality[c])
            f.f_threshold = float(f_threshold[c]); f.focal_length = float(focal_length[c]); f.stamp = float(stamps[c])
            for i, v in enumerate(intr_list[c] if intr_list[c] is not None else ()):
                f.intr[i] = float(v)
            if masks[c] is not None:
                f.base_mask = masks[c].ctypes.data_as(_u8)
            cbs.append(make_cb(orders[c]) if orders[c] is not None else C.cast(None, TRACKS_ORDER_FN))
            f.order = cbs[-1]
        return tin, (frames, masks, cbs)

    @staticmethod
    def _tracks_out(o, lists=True):
        """numpy copies of one vg_fe_tracks_out; lists False: the counts, and which array pointers were NULL"""

        def arr(ptr, shape, dtype):
            k = int(np.prod(shape))
            return np.ctypeslib.as_array(ptr, shape).copy() if k and ptr else np.zeros(shape, dtype)

        out = {k: int(getattr(o, k)) for k in ("n", "n_id", "n_msg", "n1", "n2", "n_kept", "n_new", "fallback", "ransac_best", "ransac_niters")}
        out["ransac_ran"] = bool(o.ransac_ran)
        if not lists:
            out["null_pointers"] = [k for k in ("ids", "track_cnt", "cur_xy", "un_xy", "vel_xy", "msg_id", "msg_obs") if not getattr(o, k)]
            return out
        out["ids"] = arr(o.ids, (o.n,), np.int32)
        out["track_cnt"] = arr(o.track_cnt, (o.n,), np.int32)
        for k in ("cur_xy", "un_xy", "vel_xy"):
            out[k] = arr(getattr(o, k), (o.n, 2), np.float32)
        out["msg_id"] = arr(o.msg_id, (o.n_msg,), np.int32)
        out["msg_obs"] = arr(o.msg_obs, (o.n_msg, 7), np.float64)
        return out

    def vio_step(self, samples, imgs, stamps, publish_list, intr_list, max_cnt=150, min_dist=30, equalize=False, f_threshold=1.0, focal_length=460.0,
                 quality=0.01, base_masks=None, orders=None, n_streams=None, struct_size=None, vio_struct_size=None, lists=False):
        """vg_vio_step_async: one frame for every stream and, when it publishes, the estimator step of window c from stream c's message
        on the device.  samples[c]: (n, 7) [dt acc gyr] since the previous PUBLISHED frame, None / empty on a frame that does not
        publish; everything else as tracks_step.  lists: the bridge was begun with VG_VIO_LISTS (the dicts of tracks_step); otherwise
        the counts of vg_fe_tracks_out and `null_pointers`, the names of its array pointers that were NULL."""
        m = len(publish_list)
        S = m if n_streams is None else int(n_streams)
        tin, _keep = self._tracks_in(imgs, stamps, publish_list, intr_list, max_cnt, min_dist, equalize, f_threshold, focal_length, quality,
                                     base_masks, orders, struct_size)
        vin, smp = (VioIn * m)(), []
        for c in range(m):
            a = None if samples is None or samples[c] is None else np.ascontiguousarray(samples[c], np.float64).reshape(-1, 7)
            smp.append(a)
            vin[c].struct_size = C.sizeof(VioIn) if vio_struct_size is None else int(vio_struct_size)
            vin[c].n_samples = 0 if a is None else len(a)
            vin[c].samples = a.ctypes.data_as(_f8) if a is not None and a.size else None
            vin[c].fe = tin[c]
        vo = (VioOut * m)()
        self.hd._chk(self.lib.vg_vio_step_async(self.h, S, vin, vo), "vg_vio_step_async")
        return [self._tracks_out(vo[c].fe, lists) for c in range(m)]

    def tracks_get(self, cam):
        """vg_fe_tracks_get: the list of one stream between two frames: dict(n, n_id, prev_time, cur_xy, ids, track_cnt, un_xy, in_map)"""
        cap = self.max_pts
        xy, un = np.zeros((cap, 2), np.float32), np.zeros((cap, 2), np.float32)
        ids, cnt, in_map = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.uint8)
        st = TracksState()
        st.struct_size = C.sizeof(TracksState)
        st.cur_xy, st.ids, st.track_cnt = xy.ctypes.data_as(_f4), ids.ctypes.data_as(_i4), cnt.ctypes.data_as(_i4)
        st.un_xy, st.in_map = un.ctypes.data_as(_f4), in_map.ctypes.data_as(_u8)
        self.hd._chk(self.lib.vg_fe_tracks_get(self.h, int(cam), C.byref(st)), "vg_fe_tracks_get")
        n = st.n
        return dict(n=n, n_id=st.n_id, prev_time=st.prev_time, cur_xy=xy[:n].copy(), ids=ids[:n].copy(), track_cnt=cnt[:n].copy(),
                    un_xy=un[:n].copy(), in_map=in_map[:n].copy())

    def tracks_set(self, cam, cur_xy, ids, track_cnt, n_id, prev_time=0.0, un_xy=None, in_map=None):
        """vg_fe_tracks_set: re-seed one stream between two frames; un_xy None: no previous map"""
        xy = np.ascontiguousarray(cur_xy, np.float32).reshape(-1, 2)
        ids, cnt = np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(track_cnt, np.int32)
        assert len(ids) == len(xy) and len(cnt) == len(xy)
        st = TracksState()
        st.struct_size, st.n, st.n_id, st.prev_time = C.sizeof(TracksState), len(xy), int(n_id), float(prev_time)
        st.cur_xy, st.ids, st.track_cnt = xy.ctypes.data_as(_f4), ids.ctypes.data_as(_i4), cnt.ctypes.data_as(_i4)
        if un_xy is not None:
            un = np.ascontiguousarray(un_xy, np.float32).reshape(-1, 2)
            im = np.ascontiguousarray(in_map, np.uint8)
            assert len(un) == len(xy) and len(im) == len(xy)
            st.un_xy, st.in_map = un.ctypes.data_as(_f4), im.ctypes.data_as(_u8)
        self.hd._chk(self.lib.vg_fe_tracks_set(self.h, int(cam), C.byref(st)), "vg_fe_tracks_set")

    def detect_upload(self, max_corners, masks=None):
        mc = np.ascontiguousarray(max_corners, np.int32)
        mp = None
        if masks is not None:
            self._mkeep = [None if m is None else np.ascontiguousarray(m, np.uint8) for m in masks]
            mp = (_u8 * self.cams)(*[None if m is None else m.ctypes.data_as(_u8) for m in self._mkeep])
        self.hd._chk(self.lib.vg_fe_detect_upload(self.h, mp, mc.ctypes.data_as(_i4)), "vg_fe_detect_upload")

    def detect_async(self, quality=0.01, min_dist=30.0):
        self.hd._chk(self.lib.vg_fe_detect_async(self.h, float(quality), float(min_dist)), "vg_fe_detect_async")

    def detect_download(self):
        out = np.zeros((self.cams, self.max_pts, 2), np.float32)
        n = np.zeros(self.cams, np.int32)
        self.hd._chk(self.lib.vg_fe_detect_download(self.h, out.ctypes.data_as(_f4), n.ctypes.data_as(_i4)), "vg_fe_detect_download")
        return [out[c, :n[c]].copy() for c in range(self.cams)]

    def get_level(self, cam, level, previous=False):
        w, hh = C.c_int(), C.c_int()
        buf = np.zeros(self.W * self.H, np.uint8)
        self.hd._chk(self.lib.vg_fe_get_level(self.h, cam, int(previous), level, buf.ctypes.data_as(_u8), C.byref(w), C.byref(hh)), "vg_fe_get_level")
        return buf[:w.value * hh.value].reshape(hh.value, w.value).copy()

    def keep_eig(self, on=True):
        """the min-eigenvalue map of every following detection is written to device memory too (it is an on-chip intermediate otherwise)"""
        self.hd._chk(self.lib.vg_fe_keep_eig(self.h, 1 if on else 0), "vg_fe_keep_eig")

    def get_eig(self, cam):
        out = np.zeros((self.H, self.W), np.float32)
        self.hd._chk(self.lib.vg_fe_get_eig(self.h, cam, out.ctypes.data_as(_f4)), "vg_fe_get_eig")
        return out


# ---- loop closure: keyframe BRIEF descriptors and matching (vg_kf_*) -------------------------------------------------------------------
_u64 = C.POINTER(C.c_uint64)
KF_OK, KF_TRUNCATED = 0, 1
KF_ADD_LAUNCHES = 7
KF_KERNELS = ("blur", "fast_score", "nonmax_masks", "scan", "scatter", "lift", "brief")


class KfIn(C.Structure):
    """vg_kf_in (include/vinsgpu.h)"""
    _fields_ = [("struct_size", C.c_int), ("slot", C.c_int), ("img", _u8), ("stride", C.c_int), ("n_window", C.c_int), ("window_xy", _f4),
                ("camera", Camera)]


class KfOut(C.Structure):
    """vg_kf_out (include/vinsgpu.h)"""
    _fields_ = [("struct_size", C.c_int), ("n_keypoints", C.c_int), ("status", C.c_int), ("n_kept", C.c_int), ("keypoints_xy", _f4),
                ("scores", _u8), ("norm_xy", _f4), ("descriptors", _u64), ("window_descriptors", _u64), ("device_ms", _f4)]


class KfRecord(C.Structure):
    """vg_kf_record (include/vinsgpu.h)"""
    _fields_ = [("struct_size", C.c_int), ("n_keypoints", C.c_int), ("n_window", C.c_int), ("n_true", C.c_int), ("keypoints_xy", _f4),
                ("scores", _u8), ("norm_xy", _f4), ("descriptors", _u64), ("window_xy", _f4), ("window_descriptors", _u64)]


class KfPair(C.Structure):
    """vg_kf_pair (include/vinsgpu.h)"""
    _fields_ = [("struct_size", C.c_int), ("cur_slot", C.c_int), ("old_slot", C.c_int)]


class KfMatchOut(C.Structure):
    """vg_kf_match_out (include/vinsgpu.h)"""
    _fields_ = [("struct_size", C.c_int), ("n_window", C.c_int), ("n_matched", C.c_int), ("best_idx", _i4), ("best_dist", _i4), ("status", _u8),
                ("matched_2d_old", _f4), ("matched_2d_old_norm", _f4), ("matched_index", _i4), ("matched_old_xy", _f4),
                ("matched_old_norm", _f4), ("device_ms", _f4)]


def read_brief_pattern(path):
    """The four integer lists x1 y1 x2 y2 of an OpenCV-FileStorage yml (support_files/brief_pattern.yml) as int16 [4, 256]."""
    lists, key = {}, None
    with open(path) as f:
        for line in f:
            t = line.strip()
            if t.endswith(":") and not t.startswith("-"):
                key = t[:-1]
                lists[key] = []
            elif t.startswith("- ") and key is not None:
                lists[key].append(int(t[2:]))
    return np.array([lists[k] for k in ("x1", "y1", "x2", "y2")], np.int16)


class KeyFrames:
    """Resident keyframe records of the pose graph on one vg_handle (ba.Handle): vg_kf_configure / _add / _get / _set / _match.
    Independent of FrontEnd.  Arrays in and out are NumPy; descriptors are uint64 [n, 4]."""

    def __init__(self, handle, width, height, max_keypoints, max_window_points, n_slots, pattern):
        self.hd, self.lib, self.h = handle, handle.lib, handle.h
        L = self.lib
        L.vg_kf_configure.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int16)]
        L.vg_kf_add.argtypes = [C.c_void_p, C.c_int, C.POINTER(KfIn), C.POINTER(KfOut)]
        L.vg_kf_get.argtypes = [C.c_void_p, C.c_int, C.POINTER(KfRecord)]
        L.vg_kf_set.argtypes = [C.c_void_p, C.c_int, C.POINTER(KfRecord)]
        L.vg_kf_match.argtypes = [C.c_void_p, C.c_int, C.POINTER(KfPair), C.POINTER(KfMatchOut)]
        self.configure(width, height, max_keypoints, max_window_points, n_slots, pattern)

    def configure(self, width, height, max_keypoints, max_window_points, n_slots, pattern):
        pat = None if pattern is None else np.ascontiguousarray(pattern, np.int16).reshape(4, 256)
        self.hd._chk(self.lib.vg_kf_configure(self.h, int(width), int(height), int(max_keypoints), int(max_window_points), int(n_slots),
                                              None if pat is None else pat.ctypes.data_as(C.POINTER(C.c_int16))), "vg_kf_configure")
        self.W, self.H, self.MK, self.MW, self.NS = int(width), int(height), int(max_keypoints), int(max_window_points), int(n_slots)

    def add(self, slots, images, cameras, window_xy, arrays=True, timed=False):
        """vg_kf_add for len(slots) keyframes in one call.  images[i]: uint8 [H, W] (any row stride); cameras[i]: a Camera;
        window_xy[i]: float32 [n_window, 2].  Returns one dict per entry: n_keypoints (the true count), status, and with `arrays`
        keypoints, scores, norm, descriptors, window_descriptors; with `timed` the first dict also holds device_ms [KF_ADD_LAUNCHES]."""
        n = len(slots)
        ins, outs, keep = (KfIn * n)(), (KfOut * n)(), []
        ms = np.zeros(KF_ADD_LAUNCHES, np.float32)
        for i in range(n):
            img = np.asarray(images[i])
            if img.dtype != np.uint8 or img.ndim != 2 or img.strides[1] != 1:
                img = np.ascontiguousarray(img, np.uint8)
            assert img.shape == (self.H, self.W)
            w = np.ascontiguousarray(window_xy[i], np.float32).reshape(-1, 2)
            a, o = ins[i], outs[i]
            a.struct_size, a.slot, a.img, a.stride = C.sizeof(KfIn), int(slots[i]), img.ctypes.data_as(_u8), img.strides[0]
            a.n_window, a.window_xy, a.camera = len(w), w.ctypes.data_as(_f4), cameras[i]
            o.struct_size = C.sizeof(KfOut)
            bufs = None
            if arrays:
                bufs = (np.zeros((self.MK, 2), np.float32), np.zeros(self.MK, np.uint8), np.zeros((self.MK, 2), np.float32),
                        np.zeros((self.MK, 4), np.uint64), np.zeros((self.MW, 4), np.uint64))
                o.keypoints_xy, o.scores, o.norm_xy = bufs[0].ctypes.data_as(_f4), bufs[1].ctypes.data_as(_u8), bufs[2].ctypes.data_as(_f4)
                o.descriptors, o.window_descriptors = bufs[3].ctypes.data_as(_u64), bufs[4].ctypes.data_as(_u64)
            keep.append((img, w, bufs))
        if timed and n:
            outs[0].device_ms = ms.ctypes.data_as(_f4)
        self.hd._chk(self.lib.vg_kf_add(self.h, n, ins, outs), "vg_kf_add")
        res = []
        for i in range(n):
            o, (_, w, bufs) = outs[i], keep[i]
            d = {"n_keypoints": o.n_keypoints, "status": o.status, "n_kept": o.n_kept}
            if arrays:
                k = o.n_kept
                d.update(keypoints=bufs[0][:k].copy(), scores=bufs[1][:k].copy(), norm=bufs[2][:k].copy(), descriptors=bufs[3][:k].copy(),
                         window_descriptors=bufs[4][:len(w)].copy())
            res.append(d)
        if timed and n:
            res[0]["device_ms"] = ms.copy()
        return res

    def get(self, slot):
        """vg_kf_get: the record of `slot` as a dict of arrays"""
        r = KfRecord()
        r.struct_size = C.sizeof(KfRecord)
        b = (np.zeros((self.MK, 2), np.float32), np.zeros(self.MK, np.uint8), np.zeros((self.MK, 2), np.float32), np.zeros((self.MK, 4), np.uint64),
             np.zeros((self.MW, 2), np.float32), np.zeros((self.MW, 4), np.uint64))
        r.keypoints_xy, r.scores, r.norm_xy = b[0].ctypes.data_as(_f4), b[1].ctypes.data_as(_u8), b[2].ctypes.data_as(_f4)
        r.descriptors, r.window_xy, r.window_descriptors = b[3].ctypes.data_as(_u64), b[4].ctypes.data_as(_f4), b[5].ctypes.data_as(_u64)
        self.hd._chk(self.lib.vg_kf_get(self.h, int(slot), C.byref(r)), "vg_kf_get")
        k, w = r.n_keypoints, r.n_window
        return {"n_true": r.n_true, "keypoints": b[0][:k].copy(), "scores": b[1][:k].copy(), "norm": b[2][:k].copy(), "descriptors": b[3][:k].copy(),
                "window_xy": b[4][:w].copy(), "window_descriptors": b[5][:w].copy()}

    def set(self, slot, keypoints, scores, norm, descriptors, window_xy, window_descriptors, n_true=0):
        """vg_kf_set: upload a whole record (stored keypoints and descriptors, or planted ones)"""
        kp = np.ascontiguousarray(keypoints, np.float32).reshape(-1, 2)
        sc = np.ascontiguousarray(scores, np.uint8).reshape(-1)
        nm = np.ascontiguousarray(norm, np.float32).reshape(-1, 2)
        de = np.ascontiguousarray(descriptors, np.uint64).reshape(-1, 4)
        wx = np.ascontiguousarray(window_xy, np.float32).reshape(-1, 2)
        wd = np.ascontiguousarray(window_descriptors, np.uint64).reshape(-1, 4)
        assert len(kp) == len(sc) == len(nm) == len(de) and len(wx) == len(wd)
        r = KfRecord()
        r.struct_size, r.n_keypoints, r.n_window, r.n_true = C.sizeof(KfRecord), len(kp), len(wx), int(n_true)
        r.keypoints_xy, r.scores, r.norm_xy = kp.ctypes.data_as(_f4), sc.ctypes.data_as(_u8), nm.ctypes.data_as(_f4)
        r.descriptors, r.window_xy, r.window_descriptors = de.ctypes.data_as(_u64), wx.ctypes.data_as(_f4), wd.ctypes.data_as(_u64)
        self.hd._chk(self.lib.vg_kf_set(self.h, int(slot), C.byref(r)), "vg_kf_set")

    def match(self, pairs, timed=False):
        """vg_kf_match for a list of (current slot, old slot).  One dict per pair: best_idx, best_dist, status, matched_2d_old,
        matched_2d_old_norm (per window point) and the compacted matched_index, matched_old_xy, matched_old_norm, n_matched."""
        n = len(pairs)
        ins, outs, keep = (KfPair * n)(), (KfMatchOut * n)(), []
        ms = np.zeros(1, np.float32)
        for i, (c, o) in enumerate(pairs):
            ins[i].struct_size, ins[i].cur_slot, ins[i].old_slot = C.sizeof(KfPair), int(c), int(o)
            b = (np.zeros(self.MW, np.int32), np.zeros(self.MW, np.int32), np.zeros(self.MW, np.uint8), np.zeros((self.MW, 2), np.float32),
                 np.zeros((self.MW, 2), np.float32), np.zeros(self.MW, np.int32), np.zeros((self.MW, 2), np.float32), np.zeros((self.MW, 2), np.float32))
            q = outs[i]
            q.struct_size = C.sizeof(KfMatchOut)
            q.best_idx, q.best_dist, q.status = b[0].ctypes.data_as(_i4), b[1].ctypes.data_as(_i4), b[2].ctypes.data_as(_u8)
            q.matched_2d_old, q.matched_2d_old_norm, q.matched_index = b[3].ctypes.data_as(_f4), b[4].ctypes.data_as(_f4), b[5].ctypes.data_as(_i4)
            q.matched_old_xy, q.matched_old_norm = b[6].ctypes.data_as(_f4), b[7].ctypes.data_as(_f4)
            keep.append(b)
        if timed and n:
            outs[0].device_ms = ms.ctypes.data_as(_f4)
        self.hd._chk(self.lib.vg_kf_match(self.h, n, ins, outs), "vg_kf_match")
        res = []
        for i in range(n):
            b, w, m = keep[i], outs[i].n_window, outs[i].n_matched
            res.append({"n_window": w, "n_matched": m, "best_idx": b[0][:w].copy(), "best_dist": b[1][:w].copy(), "status": b[2][:w].copy(),
                        "matched_2d_old": b[3][:w].copy(), "matched_2d_old_norm": b[4][:w].copy(), "matched_index": b[5][:m].copy(),
                        "matched_old_xy": b[6][:m].copy(), "matched_old_norm": b[7][:m].copy()})
        if timed and n:
            res[0]["device_ms"] = float(ms[0])
        return res


# ---- loop closure: PnPRANSAC and findConnection's loop gate (vg_kf_pnp) ------------------------------------------------------------------
KF_PNP_OK, KF_PNP_SKIPPED, KF_PNP_NO_MODEL, KF_PNP_NUMERIC = 0, 1, 2, 3
KF_PNP_LAUNCHES = 7
KF_PNP_KERNELS = ("sample_0", "count_0", "pick_0", "sample_1", "count_1", "pick_1", "tail")
_f8 = C.POINTER(C.c_double)


class KfPnpIn(C.Structure):
    """vg_kf_pnp_in (include/vinsgpu.h)"""
    _fields_ = [("struct_size", C.c_size_t), ("n", C.c_int), ("point_3d", _f4), ("old_norm", _f4), ("point_id", _i4),
                ("origin_vio_T", C.c_double * 3), ("origin_vio_R", C.c_double * 9), ("tic", C.c_double * 3), ("qic", C.c_double * 9),
                ("min_loop_num", C.c_int), ("max_iters", C.c_int), ("refine", C.c_int), ("reproj_threshold", C.c_double),
                ("confidence", C.c_double), ("max_yaw_deg", C.c_double), ("max_dist", C.c_double)]


class KfPnpOut(C.Structure):
    """vg_kf_pnp_out (include/vinsgpu.h)"""
    _fields_ = [("struct_size", C.c_size_t), ("status", C.c_int), ("n_inliers", C.c_int), ("ransac_best", C.c_int), ("ransac_iter", C.c_int),
                ("ransac_bound", C.c_int), ("refit_iters", C.c_int), ("refit_up", C.c_int), ("has_loop", C.c_int),
                ("sample_rvec", C.c_double * 3), ("sample_tvec", C.c_double * 3), ("rvec", C.c_double * 3), ("tvec", C.c_double * 3),
                ("PnP_R_old", C.c_double * 9), ("PnP_T_old", C.c_double * 3), ("loop_info", C.c_double * 8), ("mask", _u8),
                ("matched_index", _i4), ("match_id", _i4), ("match_xy", _f8), ("device_ms", _f4)]


_KF_PNP_SCALARS = ("min_loop_num", "max_iters", "refine", "reproj_threshold", "confidence", "max_yaw_deg", "max_dist")


def kf_pnp(handle, pairs, timed=False):
    """vg_kf_pnp for a list of pairs on a ba.Handle.  A pair is a dict: point_3d [n, 3] and old_norm [n, 2] (float32), optionally point_id
    [n], origin_vio_T, origin_vio_R, tic, qic and any of min_loop_num, max_iters, refine, reproj_threshold, confidence, max_yaw_deg,
    max_dist (vg_kf_pnp_defaults otherwise); `n` overrides the row count (the refusal tests).  One dict per pair: status, n_inliers, mask,
    the RANSAC taps, sample_rvec / sample_tvec, rvec / tvec, refit_iters / refit_up, PnP_R_old [3, 3], PnP_T_old, loop_info [8], has_loop
    and the compacted matched_index, match_id (int32) and match_xy (float64 [n_inliers, 2]: vg_ba_relo_frame's fields); with `timed`
    the first dict also holds device_ms [KF_PNP_LAUNCHES]."""
    L = handle.lib
    L.vg_kf_pnp_defaults.argtypes = [C.POINTER(KfPnpIn)]
    L.vg_kf_pnp_defaults.restype = None
    L.vg_kf_pnp.argtypes = [C.c_void_p, C.c_int, C.POINTER(KfPnpIn), C.POINTER(KfPnpOut)]
    n = len(pairs)
    ins, outs, keep = (KfPnpIn * max(n, 1))(), (KfPnpOut * max(n, 1))(), []
    ms = np.zeros(KF_PNP_LAUNCHES, np.float32)
    for i, p in enumerate(pairs):
        a, o = ins[i], outs[i]
        L.vg_kf_pnp_defaults(C.byref(a))
        p3 = None if p.get("point_3d") is None else np.ascontiguousarray(p["point_3d"], np.float32).reshape(-1, 3)
        p2 = None if p.get("old_norm") is None else np.ascontiguousarray(p["old_norm"], np.float32).reshape(-1, 2)
        ids = None if p.get("point_id") is None else np.ascontiguousarray(p["point_id"], np.int32).reshape(-1)
        m = int(p["n"]) if "n" in p else len(p3)
        a.n = m
        a.point_3d = None if p3 is None else p3.ctypes.data_as(_f4)
        a.old_norm = None if p2 is None else p2.ctypes.data_as(_f4)
        a.point_id = None if ids is None else ids.ctypes.data_as(_i4)
        for k, cnt in (("origin_vio_T", 3), ("origin_vio_R", 9), ("tic", 3), ("qic", 9)):
            if k in p:
                setattr(a, k, (C.c_double * cnt)(*np.asarray(p[k], np.float64).reshape(-1)))
        for k in _KF_PNP_SCALARS:
            if k in p:
                setattr(a, k, p[k])
        if "struct_size" in p:
            a.struct_size = int(p["struct_size"])
        cap = max(m, 1) if 0 < m <= 1024 else 1
        bufs = (np.zeros(cap, np.uint8), np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros((cap, 2), np.float64))
        o.struct_size = int(p.get("out_struct_size", C.sizeof(KfPnpOut)))
        o.mask, o.matched_index, o.match_id, o.match_xy = (bufs[0].ctypes.data_as(_u8), bufs[1].ctypes.data_as(_i4), bufs[2].ctypes.data_as(_i4),
                                                           bufs[3].ctypes.data_as(_f8))
        keep.append((p3, p2, ids, bufs, m))
    if timed and n:
        outs[0].device_ms = ms.ctypes.data_as(_f4)
    handle._chk(L.vg_kf_pnp(handle.h, n, ins, outs), "vg_kf_pnp")
    res = []
    for i in range(n):
        o, (_, _, _, bufs, m) = outs[i], keep[i]
        k = o.n_inliers
        res.append({"status": o.status, "n_inliers": k, "ransac_best": o.ransac_best, "ransac_iter": o.ransac_iter, "ransac_bound": o.ransac_bound,
                    "refit_iters": o.refit_iters, "refit_up": o.refit_up, "has_loop": o.has_loop,
                    "sample_rvec": np.array(o.sample_rvec), "sample_tvec": np.array(o.sample_tvec), "rvec": np.array(o.rvec), "tvec": np.array(o.tvec),
                    "PnP_R_old": np.array(o.PnP_R_old).reshape(3, 3), "PnP_T_old": np.array(o.PnP_T_old), "loop_info": np.array(o.loop_info),
                    "mask": bufs[0][:m].copy(), "matched_index": bufs[1][:k].copy(), "match_id": bufs[2][:k].copy(), "match_xy": bufs[3][:k].copy()})
    if timed and n:
        res[0]["device_ms"] = ms.copy()
    return res


# ---- loop closure: DBoW2 loop detection (vg_voc_load, vg_bow_*, vg_kf_loop_detect) -----------------------------------------------------------
BOW_TF_IDF, BOW_L1_NORM = 0, 0
BOW_QUERY, BOW_ADD = 1, 2
BOW_STOPPED = 0xFFFFFFFF
BOW_LAUNCHES = 4
BOW_KERNELS = ("walk", "vector", "score", "tail")
_u32 = C.POINTER(C.c_uint32)
VOC_NODE = np.dtype([("node_id", "<i4"), ("parent_id", "<i4"), ("weight", "<f8"), ("descriptor", "<u8", (4,))])      # VINSLoop::Node
VOC_WORD = np.dtype([("node_id", "<i4"), ("word_id", "<i4")])                                                        # VINSLoop::Word


class BowEntry(C.Structure):
    """vg_bow_entry (include/vinsgpu.h)"""
    _fields_ = [("struct_size", C.c_int), ("capacity", C.c_int), ("n_words", C.c_int), ("words", _u32), ("values", _f8)]


class BowIn(C.Structure):
    """vg_bow_in (include/vinsgpu.h)"""
    _fields_ = [("struct_size", C.c_int), ("db", C.c_int), ("slot", C.c_int), ("frame_index", C.c_int), ("flags", C.c_int)]


class BowOut(C.Structure):
    """vg_bow_out (include/vinsgpu.h)"""
    _fields_ = [("struct_size", C.c_int), ("entry_id", C.c_int), ("n_results", C.c_int), ("ids", C.c_int * 4), ("scores", C.c_double * 4),
                ("find_loop", C.c_int), ("loop_index", C.c_int), ("n_words", C.c_int), ("word_of_keypoint", _u32), ("bow_word", _u32),
                ("bow_value", _f8), ("device_ms", _f4)]


def _bow_lib(handle):
    L = handle.lib
    L.vg_voc_load.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    L.vg_bow_configure.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.vg_bow_reset.argtypes = [C.c_void_p, C.c_int]
    L.vg_bow_count.argtypes = [C.c_void_p, C.c_int, _i4, _i4]
    L.vg_bow_get.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(BowEntry)]
    L.vg_kf_loop_detect.argtypes = [C.c_void_p, C.c_int, C.POINTER(BowIn), C.POINTER(BowOut)]
    return L


def read_voc_bin(path):
    """The reference's binary vocabulary (VocabularyBinary.hpp): 6 x int32 k L scoring weighting nNodes nWords, the node records, the
    word records.  Returns (k, L, scoring, weighting, nodes [VOC_NODE], words [VOC_WORD])."""
    with open(path, "rb") as f:
        k, L, scoring, weighting, n_nodes, n_words = np.frombuffer(f.read(24), "<i4")
        nodes = np.frombuffer(f.read(VOC_NODE.itemsize * int(n_nodes)), VOC_NODE)
        words = np.frombuffer(f.read(VOC_WORD.itemsize * int(n_words)), VOC_WORD)
    if len(nodes) != n_nodes or len(words) != n_words:
        raise ValueError(path + ": truncated")
    return int(k), int(L), int(scoring), int(weighting), nodes, words


def voc_load(handle, k, L, nodes, words, scoring=BOW_L1_NORM, weighting=BOW_TF_IDF, n_nodes=None, n_words=None):
    """vg_voc_load: nodes a VOC_NODE array (the file's records, in file order), words a VOC_WORD array"""
    nodes = None if nodes is None else np.ascontiguousarray(nodes, VOC_NODE)
    words = None if words is None else np.ascontiguousarray(words, VOC_WORD)
    nn = (0 if nodes is None else len(nodes)) if n_nodes is None else int(n_nodes)
    nw = (0 if words is None else len(words)) if n_words is None else int(n_words)
    handle._chk(_bow_lib(handle).vg_voc_load(handle.h, int(k), int(L), int(scoring), int(weighting), nn, None if nodes is None else nodes.ctypes.data,
                                             nw, None if words is None else words.ctypes.data), "vg_voc_load")


def bow_configure(handle, n_db, max_entries, pool_words):
    handle._chk(_bow_lib(handle).vg_bow_configure(handle.h, int(n_db), int(max_entries), int(pool_words)), "vg_bow_configure")


def bow_reset(handle, db):
    handle._chk(_bow_lib(handle).vg_bow_reset(handle.h, int(db)), "vg_bow_reset")


def bow_count(handle, db):
    """(entries, pool words in use) of database db"""
    ne, pu = C.c_int(0), C.c_int(0)
    handle._chk(_bow_lib(handle).vg_bow_count(handle.h, int(db), C.byref(ne), C.byref(pu)), "vg_bow_count")
    return ne.value, pu.value


def bow_get(handle, db, entry):
    """vg_bow_get: (words uint32 ascending, values float64) of one entry"""
    L = _bow_lib(handle)
    e = BowEntry()
    e.struct_size = C.sizeof(BowEntry)
    handle._chk(L.vg_bow_get(handle.h, int(db), int(entry), C.byref(e)), "vg_bow_get")
    w, v = np.zeros(max(e.n_words, 1), np.uint32), np.zeros(max(e.n_words, 1), np.float64)
    e.capacity, e.words, e.values = len(w), w.ctypes.data_as(_u32), v.ctypes.data_as(_f8)
    handle._chk(L.vg_bow_get(handle.h, int(db), int(entry), C.byref(e)), "vg_bow_get")
    return w[:e.n_words].copy(), v[:e.n_words].copy()


def kf_loop_detect(handle, requests, taps=None, timed=False):
    """vg_kf_loop_detect for a list of requests (db, slot, frame_index, flags) on a ba.Handle with vg_kf_* records.  taps: the capacity of
    the tap arrays (the records' max_keypoints), or None for no taps.  One dict per request: entry_id, n_results, ids, scores (float64,
    n_results of them), find_loop, loop_index, n_words and with taps word_of_keypoint (capacity-long: the caller knows the record's
    count), bow_word, bow_value; with `timed` the first dict also holds device_ms [BOW_LAUNCHES]."""
    L = _bow_lib(handle)
    n = len(requests)
    ins, outs, keep = (BowIn * max(n, 1))(), (BowOut * max(n, 1))(), []
    ms = np.zeros(BOW_LAUNCHES, np.float32)
    for i, (db, slot, frame_index, flags) in enumerate(requests):
        a, o = ins[i], outs[i]
        a.struct_size, a.db, a.slot, a.frame_index, a.flags = C.sizeof(BowIn), int(db), int(slot), int(frame_index), int(flags)
        o.struct_size = C.sizeof(BowOut)
        bufs = None
        if taps is not None:
            bufs = (np.full(max(int(taps), 1), 0xDEADBEEF, np.uint32), np.zeros(max(int(taps), 1), np.uint32), np.zeros(max(int(taps), 1), np.float64))
            o.word_of_keypoint, o.bow_word, o.bow_value = bufs[0].ctypes.data_as(_u32), bufs[1].ctypes.data_as(_u32), bufs[2].ctypes.data_as(_f8)
        keep.append(bufs)
    if timed and n:
        outs[0].device_ms = ms.ctypes.data_as(_f4)
    handle._chk(L.vg_kf_loop_detect(handle.h, n, ins, outs), "vg_kf_loop_detect")
    res = []
    for i in range(n):
        o, bufs = outs[i], keep[i]
        d = {"entry_id": o.entry_id, "n_results": o.n_results, "ids": np.array(o.ids[:o.n_results], np.int32),
             "scores": np.array(o.scores[:o.n_results], np.float64), "find_loop": o.find_loop, "loop_index": o.loop_index, "n_words": o.n_words}
        if bufs is not None:
            d.update(word_of_keypoint=bufs[0].copy(), bow_word=bufs[1][:o.n_words].copy(), bow_value=bufs[2][:o.n_words].copy())
        res.append(d)
    if timed and n:
        res[0]["device_ms"] = ms.copy()
    return res


# ---- loop closure: 4-DoF pose-graph optimisation (vg_pg_optimize) -----------------------------------------------------------------------
PG_OK, PG_NO_EDGES, PG_NUMERIC = 0, 1, 2
PG_MAX_KEYFRAMES, PG_MAX_ITERS, PG_MAX_CG, PG_LAUNCHES = 2048, 8, 128, 1
PG_KERNELS = ("solve",)


class PgIn(C.Structure):
    """vg_pg_in (include/vinsgpu.h)"""
    _fields_ = [("struct_size", C.c_size_t), ("n_kf", C.c_int), ("n_opt", C.c_int), ("first_looped_index", C.c_int), ("max_iters", C.c_int),
                ("huber_delta", C.c_double), ("index", _i4), ("sequence", _i4), ("has_loop", _i4), ("loop_index", _i4), ("vio_T", _f8),
                ("vio_R", _f8), ("loop_info", _f8)]


class PgOut(C.Structure):
    """vg_pg_out (include/vinsgpu.h)"""
    _fields_ = [("struct_size", C.c_size_t), ("status", C.c_int), ("termination", C.c_int), ("iterations", C.c_int), ("n_edges", C.c_int),
                ("n_loop_edges", C.c_int), ("n_free", C.c_int), ("initial_cost", C.c_double), ("final_cost", C.c_double),
                ("yaw_drift", C.c_double), ("r_drift", C.c_double * 9), ("t_drift", C.c_double * 3),
                ("it_cost", C.c_double * PG_MAX_ITERS), ("it_radius", C.c_double * PG_MAX_ITERS), ("it_cost_cand", C.c_double * PG_MAX_ITERS),
                ("it_model", C.c_double * PG_MAX_ITERS), ("it_flags", C.c_int * PG_MAX_ITERS), ("it_cg", C.c_int * PG_MAX_ITERS),
                ("T", _f8), ("R", _f8), ("device_ms", _f4)]


_PG_TABLES = (("index", np.int32, 1), ("sequence", np.int32, 1), ("has_loop", np.int32, 1), ("loop_index", np.int32, 1),
              ("vio_T", np.float64, 3), ("vio_R", np.float64, 9), ("loop_info", np.float64, 8))


def pg_fill(L, a, o, g):
    """one vg_pg_in / vg_pg_out pair from a graph dict (see pg_optimize); returns the arrays that must outlive the call"""
    L.vg_pg_defaults(C.byref(a))
    keep = []
    for k, dt, w in _PG_TABLES:
        arr = None if g.get(k) is None else np.ascontiguousarray(g[k], dt).reshape(-1)
        setattr(a, k, None if arr is None else arr.ctypes.data_as(_i4 if dt is np.int32 else _f8))
        keep.append(arr)
    a.n_kf = int(g["n_kf"]) if "n_kf" in g else len(keep[0])
    a.n_opt = int(g["n_opt"]) if "n_opt" in g else a.n_kf
    a.first_looped_index = int(g["first_looped_index"])
    for k in ("max_iters", "huber_delta"):
        if k in g:
            setattr(a, k, g[k])
    if "struct_size" in g:
        a.struct_size = int(g["struct_size"])
    cap = a.n_kf if 0 < a.n_kf <= PG_MAX_KEYFRAMES else 1
    T, R = np.zeros((cap, 3), np.float64), np.zeros((cap, 3, 3), np.float64)
    o.struct_size = int(g.get("out_struct_size", C.sizeof(PgOut)))
    o.T, o.R = T.ctypes.data_as(_f8), R.ctypes.data_as(_f8)
    return keep, T, R


def pg_lib(handle):
    L = handle.lib
    L.vg_pg_defaults.argtypes = [C.POINTER(PgIn)]
    L.vg_pg_defaults.restype = None
    L.vg_pg_optimize.argtypes = [C.c_void_p, C.c_int, C.POINTER(PgIn), C.POINTER(PgOut)]
    return L


def pg_optimize(handle, graphs, timed=False):
    """vg_pg_optimize for a list of pose graphs on a ba.Handle.  A graph is a dict: index, sequence, has_loop, loop_index [n_kf] (int32),
    vio_T [n_kf, 3], vio_R [n_kf, 3, 3], loop_info [n_kf, 8], first_looped_index, optionally n_opt (n_kf otherwise), max_iters, huber_delta
    (vg_pg_defaults otherwise); `n_kf` overrides the row count (the refusal tests).  One dict per graph: status, termination, iterations,
    n_edges, n_loop_edges, n_free, initial_cost, final_cost, T [n_kf, 3], R [n_kf, 3, 3], yaw_drift, r_drift [3, 3], t_drift and the trace
    rows it_cost, it_radius, it_cost_cand, it_model, it_flags, it_cg (`iterations` of them); with `timed` the first dict also holds
    device_ms [PG_LAUNCHES]."""
    L = pg_lib(handle)
    n = len(graphs)
    ins, outs, keep = (PgIn * max(n, 1))(), (PgOut * max(n, 1))(), []
    ms = np.zeros(PG_LAUNCHES, np.float32)
    for i, g in enumerate(graphs):
        keep.append(pg_fill(L, ins[i], outs[i], g))
    if timed and n:
        outs[0].device_ms = ms.ctypes.data_as(_f4)
    handle._chk(L.vg_pg_optimize(handle.h, n, ins, outs), "vg_pg_optimize")
    res = []
    for i in range(n):
        o, (_, T, R) = outs[i], keep[i]
        k = o.iterations
        res.append({"status": o.status, "termination": o.termination, "iterations": k, "n_edges": o.n_edges, "n_loop_edges": o.n_loop_edges,
                    "n_free": o.n_free, "initial_cost": o.initial_cost, "final_cost": o.final_cost, "T": T, "R": R, "yaw_drift": o.yaw_drift,
                    "r_drift": np.array(o.r_drift).reshape(3, 3), "t_drift": np.array(o.t_drift),
                    "it_cost": np.array(o.it_cost[:k]), "it_radius": np.array(o.it_radius[:k]), "it_cost_cand": np.array(o.it_cost_cand[:k]),
                    "it_model": np.array(o.it_model[:k]), "it_flags": np.array(o.it_flags[:k], np.int32), "it_cg": np.array(o.it_cg[:k], np.int32)})
    if timed and n:
        res[0]["device_ms"] = ms.copy()
    return res
