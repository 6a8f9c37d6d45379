"""ctypes binding of the BA entry points of include/vinsgpu.h (thin; no arithmetic lives here).

`prob` dicts are the ones produced by `synth.py` (and by the tests): see synth.py's docstring.
"""
import time
import ctypes as C
import numpy as np

from . import lib

VG_MAX_ITERS = 32
VG_MARGIN_OLD, VG_MARGIN_SECOND_NEW, VG_MARGIN_NONE = 0, 1, 2
VG_MARG_SQRT, VG_MARG_EIGEN = 0, 1     # vg_ba_set_marg_mode
# fields of the marginalization path word (vg_ba_batch_marg_info, include/vinsgpu.h VG_MARGPATH_*)
MARGPATH_STAGE1 = (None, 'direct', 'block_lds', 'block_glb', 'vh_eig', 'jacobi_lds', 'jacobi_glb') + (None,) * 9
MARGPATH_CERT = (None, 'passed', 'failed', None)
MARGPATH_SCHUR = (None, 'lds', 'glb', None)
MARGPATH_STAGE2 = (None, 'sqrt', 'sqrt_glb', 'vh_eig', 'jacobi_lds', 'jacobi_glb') + (None,) * 10
VG_IMU_INFO_FACTOR, VG_IMU_INFO_REFERENCE = 0, 1     # vg_ba_set_imu_info_mode
VG_OK = 0
VG_ABI_VERSION = 12         # include/vinsgpu.h
VG_LAUNCH_DIRECT, VG_LAUNCH_GRAPH = 0, 1   # vg_ba_set_launch_mode
VG_LAUNCH_DEFAULT = VG_LAUNCH_DIRECT        # include/vinsgpu.h
VG_PRIOR_RESIDENT = -1
_pd = C.POINTER(C.c_double)
_pi = C.POINTER(C.c_int)


class ImuPreint(C.Structure):
    _fields_ = [("sum_dt", C.c_double), ("delta_p", C.c_double * 3), ("delta_q", C.c_double * 4),
                ("delta_v", C.c_double * 3), ("linearized_ba", C.c_double * 3), ("linearized_bg", C.c_double * 3),
                ("jacobian", C.c_double * 225), ("covariance", C.c_double * 225), ("valid", C.c_int), ("_pad", C.c_int)]


class Problem(C.Structure):
    _fields_ = [("K", C.c_int), ("L", C.c_int), ("n_obs", C.c_int),
                ("pose", _pd), ("speedbias", _pd), ("ex_pose", _pd), ("td", C.c_double), ("inv_depth", _pd),
                ("lm_start", _pi), ("lm_nobs", _pi), ("lm_obs_off", _pi), ("obs", _pd), ("imu", C.POINTER(ImuPreint)),
                ("prior_n", C.c_int), ("prior_nblocks", C.c_int), ("prior_block_kind", _pi), ("prior_block_index", _pi),
                ("prior_J0", _pd), ("prior_r0", _pd), ("prior_x0", _pd),
                ("relo_n", C.c_int), ("relo_pose", _pd), ("relo_lm", _pi), ("relo_xy", _pd),
                ("estimate_extrinsic", C.c_int), ("estimate_td", C.c_int), ("max_iters", C.c_int),
                ("focal", C.c_double), ("tr", C.c_double), ("row", C.c_double), ("g_norm", C.c_double),
                ("max_solver_time_s", C.c_double)]


class State(C.Structure):
    _fields_ = [("pose", _pd), ("speedbias", _pd), ("ex_pose", _pd), ("td", _pd), ("inv_depth", _pd), ("relo_pose", _pd)]


class Summary(C.Structure):
    _fields_ = [("status", C.c_int), ("termination", C.c_int), ("num_iterations", C.c_int), ("num_accepted", C.c_int),
                ("initial_cost", C.c_double), ("final_cost", C.c_double), ("final_radius", C.c_double),
                ("it_cost", C.c_double * VG_MAX_ITERS), ("it_cost_cand", C.c_double * VG_MAX_ITERS),
                ("it_model", C.c_double * VG_MAX_ITERS), ("it_radius", C.c_double * VG_MAX_ITERS),
                ("it_step_norm", C.c_double * VG_MAX_ITERS), ("it_flags", C.c_int * VG_MAX_ITERS), ("prof", C.c_double * 16),
                ("gauge_rot", C.c_double * 9), ("gauge_p0", C.c_double * 3)]


class Prior(C.Structure):
    _fields_ = [("cap", C.c_int), ("cap_blocks", C.c_int), ("n", C.c_int), ("m", C.c_int), ("nblocks", C.c_int),
                ("valid", C.c_int), ("block_kind", _pi), ("block_index", _pi), ("J0", _pd), ("r0", _pd), ("x0", _pd)]


class Tracks(C.Structure):            # vg_ba_tracks
    _fields_ = [("n_features", C.c_int), ("feature_id", _pi), ("start_frame", _pi), ("n_obs", _pi), ("solve_flag", _pi),
                ("depth", _pd), ("obs", _pd)]


class SeqConfig(C.Structure):         # vg_ba_seq_config
    _fields_ = [("max_features", C.c_int), ("max_new_obs", C.c_int), ("max_landmarks", C.c_int), ("max_factors", C.c_int),
                ("init_depth", C.c_double), ("min_parallax", C.c_double)]


class Frame(C.Structure):             # vg_ba_frame
    _fields_ = [("pose", C.c_double * 7), ("speedbias", C.c_double * 9), ("imu_new", C.POINTER(ImuPreint)),
                ("imu_merged", C.POINTER(ImuPreint)), ("n_obs", C.c_int), ("feature_id", _pi), ("obs", _pd)]


class SeqImuConfig(C.Structure):      # vg_ba_seq_imu_config
    _fields_ = [("struct_size", C.c_int), ("max_samples", C.c_int), ("noise", C.c_double * 4)]


class FrameImu(C.Structure):          # vg_ba_frame_imu
    _fields_ = [("n_samples", C.c_int), ("samples", _pd), ("n_obs", C.c_int), ("feature_id", _pi), ("obs", _pd)]


class ReloFrame(C.Structure):         # vg_ba_relo_frame
    _fields_ = [("struct_size", C.c_int), ("frame", C.c_int), ("pose", _pd), ("n_match", C.c_int), ("match_id", _pi), ("match_xy", _pd),
                ("prev_relo_t", C.c_double * 3), ("prev_relo_r", C.c_double * 9)]


class ReloResult(C.Structure):        # vg_ba_relo_result
    _fields_ = [("struct_size", C.c_int), ("armed", C.c_int), ("n_factors", C.c_int), ("frame", C.c_int), ("pose", C.c_double * 7),
                ("relo_relative_t", C.c_double * 3), ("relo_relative_q", C.c_double * 4), ("relo_relative_yaw", C.c_double),
                ("drift_correct_r", C.c_double * 9), ("drift_correct_t", C.c_double * 3)]


_pf = C.POINTER(C.c_float)
VG_SEQ_OUT_TRUNCATED = 1


class SeqOutputs(C.Structure):        # vg_ba_seq_outputs
    _fields_ = [("struct_size", C.c_int), ("status", C.c_int), ("keyframe_valid", C.c_int), ("n_keyframe", C.c_int), ("n_cloud", C.c_int),
                ("n_margin", C.c_int), ("pose", C.c_double * 7), ("ex_pose", C.c_double * 7), ("kf_point_3d", _pf), ("kf_norm", _pf),
                ("kf_uv", _pf), ("kf_id", _pi), ("cloud_xyz", _pf), ("margin_xyz", _pf)]


VG_ALIGN_OK, VG_ALIGN_FAILED_LINEAR, VG_ALIGN_FAILED_REFINE, VG_ALIGN_NUMERIC = 0, 1, 2, 3
VG_ALIGN_MAX_FRAMES = 32


class AlignIn(C.Structure):           # vg_align_in
    _fields_ = [("struct_size", C.c_size_t), ("n_frames", C.c_int), ("R", _pd), ("T", _pd), ("sample_off", _pi), ("samples", _pd),
                ("first", _pd), ("ba0", C.c_double * 3), ("bg0", C.c_double * 3), ("noise", C.c_double * 4), ("tic", C.c_double * 3),
                ("g_norm", C.c_double), ("n_key", C.c_int), ("key", _pi)]


class AlignOut(C.Structure):          # vg_align_out
    _fields_ = [("struct_size", C.c_size_t), ("status", C.c_int), ("delta_bg", C.c_double * 3), ("bg", C.c_double * 3),
                ("g_lin", C.c_double * 3), ("s_lin", C.c_double), ("g_c0", C.c_double * 3), ("s", C.c_double), ("v_body", _pd),
                ("records", C.POINTER(ImuPreint)), ("Ps", _pd), ("Rs", _pd), ("Vs", _pd), ("g_w", C.c_double * 3), ("R0", C.c_double * 9)]


SFM_MAX_ITERS = 50                   # VG_SFM_MAX_ITERS


class SfmIn(C.Structure):             # vg_sfm_in
    _fields_ = [("struct_size", C.c_size_t), ("n_frames", C.c_int), ("l", C.c_int), ("relative_R", C.c_double * 9), ("relative_T", C.c_double * 3),
                ("ric", C.c_double * 9), ("n_feat", C.c_int), ("feature_id", _pi), ("start", _pi), ("nobs", _pi), ("obs_off", _pi), ("points", _pd),
                ("n_all", C.c_int), ("all_key", _pi), ("all_guess", _pi), ("all_off", _pi), ("all_id", _pi), ("all_xy", _pd)]


class SfmOut(C.Structure):            # vg_sfm_out
    _fields_ = [("struct_size", C.c_size_t), ("status", C.c_int), ("q", _pd), ("T", _pd), ("state", _pi), ("position", _pd), ("R_all", _pd),
                ("T_all", _pd), ("is_key", _pi), ("q0", _pd), ("T0", _pd), ("position0", _pd), ("pnp_iters", _pi), ("pnp_up", _pi),
                ("ba_iters", C.c_int), ("ba_termination", C.c_int), ("final_cost", C.c_double), ("it_cost", C.c_double * SFM_MAX_ITERS),
                ("it_cost_cand", C.c_double * SFM_MAX_ITERS), ("it_model", C.c_double * SFM_MAX_ITERS), ("it_radius", C.c_double * SFM_MAX_ITERS),
                ("it_flags", C.c_int * SFM_MAX_ITERS), ("device_ms", _pd)]


RELPOSE_LAUNCHES = 9                 # VG_RELPOSE_LAUNCHES
RELPOSE_OK, RELPOSE_NONE, RELPOSE_NUMERIC = 0, 1, 2
# what the reference hard-codes (estimator.cpp:442-471, solve_5pts.cpp:193-227): the defaults of Handle.init_relpose
RELPOSE_DEFAULTS = dict(ransac_threshold=0.3 / 460, confidence=0.99, min_corres=20, min_inliers=12, parallax_gate=30.0, focal=460.0,
                        cheirality_dist=50.0)
_pu8 = C.POINTER(C.c_uint8)


class RelposeIn(C.Structure):         # vg_relpose_in
    _fields_ = [("struct_size", C.c_size_t), ("n_frames", C.c_int), ("n_feat", C.c_int), ("start", _pi), ("nobs", _pi), ("obs_off", _pi),
                ("points", _pd), ("ransac_threshold", C.c_double), ("confidence", C.c_double), ("min_corres", C.c_int), ("min_inliers", C.c_int),
                ("parallax_gate", C.c_double), ("focal", C.c_double), ("cheirality_dist", C.c_double)]


class RelposeOut(C.Structure):        # vg_relpose_out
    _fields_ = [("struct_size", C.c_size_t), ("status", C.c_int), ("l", C.c_int), ("relative_R", C.c_double * 9), ("relative_T", C.c_double * 3),
                ("n_mask", C.c_int), ("mask", _pu8), ("ransac_mask", _pu8), ("n_corres", _pi), ("avg_parallax", _pd), ("gate", _pi),
                ("ransac_iter", _pi), ("ransac_bound", _pi), ("ransac_inliers", _pi), ("ransac_best", _pi), ("F", _pd), ("good", _pi), ("winner", _pi),
                ("inlier_cnt", _pi), ("used_fallback", _pi), ("device_ms", _pd)]


EXROT_LAUNCHES = 9                   # VG_EXROT_LAUNCHES
EXROT_MAX_STEPS = 64                 # VG_EXROT_MAX_STEPS
EXROT_OK, EXROT_NUMERIC = 0, 1
# what the reference hard-codes (initial_ex_rotation.cpp; cv::findFundamentalMat's defaults): the defaults of Handle.init_exrot
EXROT_DEFAULTS = dict(ransac_threshold=3.0, confidence=0.99, min_points=9, huber_deg=5.0, min_frames=10, cov_threshold=0.25)


class ExrotIn(C.Structure):           # vg_exrot_in
    _fields_ = [("struct_size", C.c_size_t), ("n_steps", C.c_int), ("corr_off", _pi), ("corr", _pd), ("delta_q", _pd), ("n_prev", C.c_int),
                ("prev", _pd), ("ric_prev", _pd), ("ransac_threshold", C.c_double), ("confidence", C.c_double), ("min_points", C.c_int),
                ("huber_deg", C.c_double), ("min_frames", C.c_int), ("cov_threshold", C.c_double)]


class ExrotOut(C.Structure):          # vg_exrot_out
    _fields_ = [("struct_size", C.c_size_t), ("status", C.c_int), ("first_ok", C.c_int), ("calib_ric", C.c_double * 9), ("records", _pd),
                ("ric", _pd), ("sigma", _pd), ("ok", _pi), ("huber", _pd), ("branch", _pi), ("ransac_iter", _pi), ("ransac_bound", _pi),
                ("ransac_inliers", _pi), ("ransac_best", _pi), ("F", _pd), ("front", _pi), ("picked", _pi), ("used_fallback", _pi),
                ("device_ms", _pd)]


SEQ_INFO = ("flag", "n_features", "n_tracked", "n_parallax", "n_landmarks", "n_factors", "status", "n_after")


def imu_struct(m):
    """vg_imu_preint from a pre-integration dict (synth.preintegrate / Handle.imu_preintegrate); None: no factor."""
    q = ImuPreint()
    if m is None:
        q.valid = 0
        return q
    q.sum_dt = float(m['sum_dt'])
    q.delta_p[:] = list(m['delta_p']); q.delta_q[:] = list(m['delta_q']); q.delta_v[:] = list(m['delta_v'])
    q.linearized_ba[:] = list(m['lin_ba']); q.linearized_bg[:] = list(m['lin_bg'])
    q.jacobian[:] = list(np.asarray(m['jacobian'], float).ravel())
    q.covariance[:] = list(np.asarray(m['covariance'], float).ravel())
    q.valid = 1
    return q


def _dp(a):
    return a.ctypes.data_as(_pd)


def _ip(a):
    return a.ctypes.data_as(_pi)


_GS = {0: 7, 1: 9, 2: 7, 3: 1}


class PackedProblem:
    """Owns contiguous copies of a prob dict's arrays and the ctypes struct pointing at them."""

    def __init__(self, prob):
        f8 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        i4 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
        self.K = int(prob['pose'].shape[0])
        self.L = int(prob['inv_depth'].shape[0])
        self.keep = k = {}
        k['pose'], k['sb'], k['ex'] = f8(prob['pose']), f8(prob['sb']), f8(prob['ex'])
        k['lam'] = f8(prob['inv_depth'])
        k['lm_start'], k['lm_nobs'], k['obs_off'] = i4(prob['lm_start']), i4(prob['lm_nobs']), i4(prob['obs_off'])
        k['obs'] = f8(prob['obs']).reshape(-1, 7) if self.L else np.zeros((0, 7))
        imu = (ImuPreint * (self.K - 1))()
        for i, m in enumerate(prob['imu']):
            if m is None:
                imu[i].valid = 0
                continue
            imu[i].sum_dt = float(m['sum_dt'])
            imu[i].delta_p[:] = list(m['delta_p'])
            imu[i].delta_q[:] = list(m['delta_q'])
            imu[i].delta_v[:] = list(m['delta_v'])
            imu[i].linearized_ba[:] = list(m['lin_ba'])
            imu[i].linearized_bg[:] = list(m['lin_bg'])
            imu[i].jacobian[:] = list(np.asarray(m['jacobian'], float).ravel())
            imu[i].covariance[:] = list(np.asarray(m['covariance'], float).ravel())
            imu[i].valid = 1
        k['imu'] = imu
        p = Problem()
        p.K, p.L, p.n_obs = self.K, self.L, int(k['obs'].shape[0])
        p.pose, p.speedbias, p.ex_pose, p.td = _dp(k['pose']), _dp(k['sb']), _dp(k['ex']), float(prob['td'])
        p.inv_depth, p.lm_start, p.lm_nobs, p.lm_obs_off = _dp(k['lam']), _ip(k['lm_start']), _ip(k['lm_nobs']), _ip(k['obs_off'])
        p.obs, p.imu = _dp(k['obs']), imu
        pr = prob.get('prior')
        if isinstance(pr, str) and pr == 'resident':      # the prior the batch slot holds on the device
            p.prior_n = VG_PRIOR_RESIDENT
        elif pr is not None:
            k['pk'] = i4([b[0] for b in pr['blocks']])
            k['pidx'] = i4([b[1] for b in pr['blocks']])
            k['J0'], k['r0'] = f8(pr['J0']), f8(pr['r0'])
            k['x0'] = f8(np.concatenate([np.atleast_1d(np.asarray(v, float)) for v in pr['x0']]))
            p.prior_n, p.prior_nblocks = int(pr['n']), len(pr['blocks'])
            p.prior_block_kind, p.prior_block_index = _ip(k['pk']), _ip(k['pidx'])
            p.prior_J0, p.prior_r0, p.prior_x0 = _dp(k['J0']), _dp(k['r0']), _dp(k['x0'])
        relo = prob.get('relo')
        if relo is not None:
            k['relo_pose'] = f8(relo['pose'])
            k['relo_lm'] = i4([m[0] for m in relo['match']])
            k['relo_xy'] = f8([[m[1], m[2]] for m in relo['match']])
            p.relo_n, p.relo_pose, p.relo_lm, p.relo_xy = len(relo['match']), _dp(k['relo_pose']), _ip(k['relo_lm']), _dp(k['relo_xy'])
        p.estimate_extrinsic, p.estimate_td, p.max_iters = int(prob['estimate_extrinsic']), int(prob['estimate_td']), int(prob['max_iters'])
        p.focal, p.tr, p.row, p.g_norm = float(prob['focal']), float(prob['tr']), float(prob['row']), float(prob['g_norm'])
        p.max_solver_time_s = float(prob.get('max_solver_time_s', 0.0))
        self.struct = p
        self.has_relo = relo is not None


class PackedBatch:
    """The vg_ba_problem* array of a batch, built once: what a native caller holds between frames."""

    def __init__(self, probs):
        self.packed = [p if isinstance(p, PackedProblem) else PackedProblem(p) for p in probs]
        self.arr = (C.POINTER(Problem) * len(self.packed))(*[C.pointer(p.struct) for p in self.packed])


class _Out:
    def __init__(self, K, L, has_relo, want_prior):
        self.pose, self.sb = np.zeros((K, 7)), np.zeros((K, 9))
        self.ex, self.td, self.lam = np.zeros(7), np.zeros(1), np.zeros(max(L, 1))
        self.relo = np.zeros(7)
        self.L = L
        self.state = State(_dp(self.pose), _dp(self.sb), _dp(self.ex), _dp(self.td), _dp(self.lam),
                           _dp(self.relo) if has_relo else None)
        self.prior = None
        if want_prior:
            cap, capb = 6 * K + 32, K + 8
            self.pk, self.pidx = np.zeros(capb, np.int32), np.zeros(capb, np.int32)
            self.J0, self.r0, self.x0 = np.zeros(cap * cap), np.zeros(cap), np.zeros(9 * capb)
            self.prior = Prior(cap, capb, 0, 0, 0, 0, _ip(self.pk), _ip(self.pidx), _dp(self.J0), _dp(self.r0), _dp(self.x0))

    def state_dict(self, has_relo):
        st = dict(pose=self.pose.copy(), sb=self.sb.copy(), ex=self.ex.copy(), td=float(self.td[0]),
                  inv_depth=self.lam[:self.L].copy())
        if has_relo:
            st['relo_pose'] = self.relo.copy()
        return st

    def prior_dict(self):
        q = self.prior
        if q is None or not q.valid:
            return None
        n, nb = q.n, q.nblocks
        blocks = [(int(self.pk[b]), int(self.pidx[b])) for b in range(nb)]
        x0, off = [], 0
        for kind, _ in blocks:
            x0.append(self.x0[off:off + _GS[kind]].copy())
            off += _GS[kind]
        return dict(n=n, m=q.m, blocks=blocks, J0=self.J0[:n * n].reshape(n, n).copy(), r0=self.r0[:n].copy(), x0=x0)


def summary_dict(s):
    n = s.num_iterations
    return dict(status=s.status, termination=s.termination, num_iterations=n, num_accepted=s.num_accepted,
                initial_cost=s.initial_cost, final_cost=s.final_cost, final_radius=s.final_radius,
                it_cost=np.array(s.it_cost[:n]), it_cost_cand=np.array(s.it_cost_cand[:n]),
                it_model=np.array(s.it_model[:n]), it_radius=np.array(s.it_radius[:n]),
                it_step_norm=np.array(s.it_step_norm[:n]), it_flags=np.array(s.it_flags[:n]), prof=np.array(s.prof[:]),
                gauge_rot=np.array(s.gauge_rot[:]).reshape(3, 3), gauge_p0=np.array(s.gauge_p0[:]))


# vg_allreduce_fn(user, device_buf, count, stream) -> 0 on success
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)


class Config(C.Structure):
    """vg_config (include/vinsgpu.h, ABI 12): everything that shapes a handle in one struct; a handle made from it never reads the environment."""
    _fields_ = [("struct_size", C.c_int), ("device", C.c_int), ("launch_mode", C.c_int), ("marg_mode", C.c_int),
                ("fused_min_windows", C.c_int), ("pack_threads", C.c_int), ("imu_info_mode", C.c_int)]


class Handle:
    """vg_create / vg_destroy wrapper; raises RuntimeError with vg_last_error on failures.  config: a dict of vg_config fields
    (device: None = the current one, else the HIP device index; launch_mode = 'graph' | 'direct', marg_mode, fused_min_windows,
    pack_threads, imu_info_mode) -> vg_create_config."""

    def __init__(self, config=None):
        self.lib = lib()
        L = self.lib
        L.vg_create.argtypes = [C.POINTER(C.c_void_p)]
        L.vg_destroy.argtypes = [C.c_void_p]
        L.vg_sync.argtypes = [C.c_void_p]
        L.vg_last_error.argtypes = [C.c_void_p]
        L.vg_last_error.restype = C.c_char_p
        L.vg_timer_start.argtypes = [C.c_void_p]
        L.vg_timer_stop.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        L.vg_ba_batch_upload.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.POINTER(Problem)), _pi]
        L.vg_ba_batch_run_async.argtypes = [C.c_void_p]
        L.vg_ba_batch_download.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.POINTER(State)), C.POINTER(Summary),
                                           C.POINTER(C.POINTER(Prior))]
        L.vg_ba_batch_download_state.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.POINTER(State)), C.POINTER(Summary)]
        L.vg_ba_batch_download_prior.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.POINTER(Prior))]
        L.vg_ba_batch_run_timed.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.vg_ba_batch_run_profiled.argtypes = [C.c_void_p, C.POINTER(C.c_float), _pi]
        L.vg_ba_batch_flops_by_kernel.argtypes = [C.c_void_p, _pd]
        L.vg_ba_batch_info.argtypes = [C.c_void_p, _pd, _pd, _pd, _pi]
        L.vg_ba_batch_flops.argtypes = [C.c_void_p, _pd, _pd]
        L.vg_ba_eval_factors.argtypes = [C.c_void_p, C.POINTER(Problem), _pd, _pd, _pd, _pd, _pd]
        L.vg_ba_set_large_window.argtypes = [C.c_void_p, C.c_int]
        L.vg_ba_set_marg_mode.argtypes = [C.c_void_p, C.c_int]
        L.vg_ba_set_launch_mode.argtypes = [C.c_void_p, C.c_int]
        L.vg_ba_set_fused_min_windows.argtypes = [C.c_void_p, C.c_int]
        L.vg_host_register.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.vg_host_unregister.argtypes = [C.c_void_p, C.c_void_p]
        L.vg_ba_launch_stats.argtypes = [C.c_void_p, _pi, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
        if hasattr(L, 'vg_ba_rccl_init'):            # (absent from the CPU-emulated build of tests/simt)
            L.vg_ba_rccl_init.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p]
            L.vg_ba_rccl_finalize.argtypes = [C.c_void_p]
        L.vg_ba_set_allreduce.argtypes = [C.c_void_p, ALLREDUCE_FN, C.c_void_p]
        L.vg_ba_reduce_layout.argtypes = [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        L.vg_triangulate.argtypes = [C.c_void_p, C.c_int, _pd, _pd, _pd, _pd, C.c_int, _pi, _pi, _pi, _pd, C.c_double, _pd]
        L.vg_imu_preintegrate.argtypes = [C.c_void_p, C.c_int, _pi, _pd, _pd, _pd, _pd, C.POINTER(ImuPreint)]
        L.vg_ba_reserve.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        L.vg_ba_seq_begin.argtypes = [C.c_void_p, C.c_int, C.POINTER(SeqConfig), C.POINTER(C.POINTER(Problem)), C.POINTER(C.POINTER(Tracks))]
        L.vg_ba_seq_step_async.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.POINTER(Frame))]
        L.vg_ba_seq_info.argtypes = [C.c_void_p, C.c_int, _pi]
        L.vg_ba_seq_get_tracks.argtypes = [C.c_void_p, C.c_int, C.c_int, _pi, _pi, _pi, _pi, _pi, _pd, _pd]
        L.vg_ba_seq_end.argtypes = [C.c_void_p]
        L.vg_ba_seq_export.argtypes = [C.c_void_p, C.c_int, _pd, _pd, _pd, _pd, C.POINTER(ImuPreint), C.POINTER(Prior)]
        L.vg_ba_seq_import.argtypes = [C.c_void_p, C.c_int, C.POINTER(Problem), C.POINTER(Tracks)]
        if hasattr(L, "vg_ba_seq_imu_begin"):             # (added within ABI 12: tests/manual/bench_with_lib.py loads older builds)
            L.vg_ba_seq_imu_begin.argtypes = [C.c_void_p, C.c_int, C.POINTER(SeqImuConfig), _pd]
            L.vg_ba_seq_step_imu_async.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.POINTER(FrameImu))]
            L.vg_ba_seq_imu_get.argtypes = [C.c_void_p, C.c_int, _pd, _pd, _pd]
            L.vg_ba_seq_imu_set.argtypes = [C.c_void_p, C.c_int, _pd]
            L.vg_ba_seq_imu_timing.argtypes = [C.c_void_p, C.c_int]
            L.vg_ba_seq_imu_times.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        if hasattr(L, "vg_vio_begin"):                    # (added within ABI 12)
            L.vg_vio_begin.argtypes = [C.c_void_p, C.c_int]
            L.vg_vio_get_frame.argtypes = [C.c_void_p, C.c_int, C.c_int, _pi, _pi, _pd]
            L.vg_vio_end.argtypes = [C.c_void_p]
        if hasattr(L, "vg_ba_seq_set_relo"):              # (added within ABI 12)
            L.vg_ba_seq_relo_reserve.argtypes = [C.c_void_p, C.c_int]
            L.vg_ba_seq_set_relo.argtypes = [C.c_void_p, C.c_int, C.POINTER(ReloFrame)]
            L.vg_ba_seq_get_relo.argtypes = [C.c_void_p, C.c_int, C.POINTER(ReloResult)]
        if hasattr(L, "vg_ba_seq_outputs_async"):         # (added within ABI 12)
            L.vg_ba_seq_outputs_reserve.argtypes = [C.c_void_p, C.c_int]
            L.vg_ba_seq_outputs_async.argtypes = [C.c_void_p]
            L.vg_ba_seq_get_outputs.argtypes = [C.c_void_p, C.c_int, C.POINTER(SeqOutputs)]
        if hasattr(L, "vg_init_align"):                   # (added within ABI 12)
            L.vg_init_align.argtypes = [C.c_void_p, C.c_int, C.POINTER(AlignIn), C.POINTER(AlignOut)]
        if hasattr(L, "vg_init_sfm"):                     # (added within ABI 12)
            L.vg_init_sfm.argtypes = [C.c_void_p, C.c_int, C.POINTER(SfmIn), C.POINTER(SfmOut)]
        if hasattr(L, "vg_init_relpose"):                 # (added within ABI 12)
            L.vg_init_relpose.argtypes = [C.c_void_p, C.c_int, C.POINTER(RelposeIn), C.POINTER(RelposeOut)]
        if hasattr(L, "vg_init_exrot"):                   # (added within ABI 12)
            L.vg_init_exrot.argtypes = [C.c_void_p, C.c_int, C.POINTER(ExrotIn), C.POINTER(ExrotOut)]
        if L.vg_abi_version() != VG_ABI_VERSION:
            raise RuntimeError(f"libvinsgpu.so reports ABI version {L.vg_abi_version()}, this binding was written for {VG_ABI_VERSION}")
        self.h = C.c_void_p()
        if config is None:
            rc = L.vg_create(C.byref(self.h))
        else:
            dev = config.get("device")                      # vg_config::device: 0 = the current device, k + 1 = device k
            cfg = Config(struct_size=C.sizeof(Config), device=0 if dev is None or int(dev) < 0 else int(dev) + 1,
                         launch_mode={None: 0, "direct": 1, "graph": 2}[config.get("launch_mode")], marg_mode=int(config.get("marg_mode", 0)),
                         fused_min_windows=int(config.get("fused_min_windows", 0)), pack_threads=int(config.get("pack_threads", 0)),
                         imu_info_mode=int(config.get("imu_info_mode", 0)))
            L.vg_create_config.argtypes = [C.POINTER(Config), C.POINTER(C.c_void_p)]
            rc = L.vg_create_config(C.byref(cfg), C.byref(self.h))
        if rc != VG_OK:
            raise RuntimeError(f"vg_create failed with status {rc} (no HIP device?)")

    def close(self):
        if self.h:
            self.lib.vg_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != VG_OK:
            raise RuntimeError(f"{what} failed: status {rc}: {self.lib.vg_last_error(self.h).decode()}")

    # ---- timers
    def timer_start(self):
        self._chk(self.lib.vg_timer_start(self.h), "vg_timer_start")

    def timer_stop(self):
        ms = C.c_float()
        self._chk(self.lib.vg_timer_stop(self.h, C.byref(ms)), "vg_timer_stop")
        return float(ms.value)

    def sync(self):
        self._chk(self.lib.vg_sync(self.h), "vg_sync")

    # ---- BA
    def ba_upload(self, probs, margin_flags=None):
        if isinstance(probs, PackedBatch):                # pointer array built once (the boundary loops of bench.py)
            self._packed, arr = probs.packed, probs.arr
            n = len(self._packed)
        else:
            self._packed = [p if isinstance(p, PackedProblem) else PackedProblem(p) for p in probs]
            n = len(self._packed)
            arr = (C.POINTER(Problem) * n)(*[C.pointer(p.struct) for p in self._packed])
        mf = np.ascontiguousarray(margin_flags if margin_flags is not None else [VG_MARGIN_NONE] * n, dtype=np.int32)
        self._margin = mf
        t0 = time.perf_counter()
        self._chk(self.lib.vg_ba_batch_upload(self.h, n, arr, _ip(mf)), "vg_ba_batch_upload")
        self.last_upload_call_ms = (time.perf_counter() - t0) * 1e3        # the C-ABI call alone (pack + H2D + sync)

    def ba_run_async(self):
        self._chk(self.lib.vg_ba_batch_run_async(self.h), "vg_ba_batch_run_async")

    def ba_set_launch_mode(self, mode):
        """VG_LAUNCH_DIRECT (0) / VG_LAUNCH_GRAPH (1): one launch per kernel, or the captured pipeline replayed as a hipGraph."""
        self._chk(self.lib.vg_ba_set_launch_mode(self.h, int(mode)), "vg_ba_set_launch_mode")

    def host_register(self, arr):
        """Page-lock a numpy array that will be handed to the upload entry points repeatedly (vg_host_register)."""
        self._chk(self.lib.vg_host_register(self.h, C.c_void_p(arr.ctypes.data), C.c_size_t(arr.nbytes)), "vg_host_register")

    def host_unregister(self, arr):
        self._chk(self.lib.vg_host_unregister(self.h, C.c_void_p(arr.ctypes.data)), "vg_host_unregister")

    def ba_set_fused_min_windows(self, n):
        """Batches of at least n windows take the fused linearise + accumulate kernel (0 = never; default 32): vg_ba_set_fused_min_windows."""
        self._chk(self.lib.vg_ba_set_fused_min_windows(self.h, int(n)), "vg_ba_set_fused_min_windows")

    def probe_clocks(self):
        """vg_probe_clocks: {ns per dependent FP64 FMA, clock64 ticks per us} with one wavefront / with every CU loaded."""
        out = (C.c_double * 4)()
        self.lib.vg_probe_clocks.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        self._chk(self.lib.vg_probe_clocks(self.h, out), "vg_probe_clocks")
        return {"lone_wave": {"ns_per_dependent_fma": out[0], "clock64_ticks_per_us": out[1]},
                "all_cus_loaded": {"ns_per_dependent_fma": out[2], "clock64_ticks_per_us": out[3]}}

    def ba_launch_stats(self):
        mode, nl, ncap = C.c_int(), C.c_longlong(), C.c_longlong()
        self._chk(self.lib.vg_ba_launch_stats(self.h, C.byref(mode), C.byref(nl), C.byref(ncap)), "vg_ba_launch_stats")
        return {"mode": "graph" if mode.value == VG_LAUNCH_GRAPH else "direct", "graph_launches": nl.value, "graph_captures": ncap.value}

    # ---- large windows / landmark shards (include/vinsgpu.h "Large windows and landmark shards")
    def ba_set_marg_mode(self, mode):
        """VG_MARG_SQRT (0, default) / VG_MARG_EIGEN (1): form of the prior factor (include/vinsgpu.h)."""
        self._chk(self.lib.vg_ba_set_marg_mode(self.h, int(mode)), "vg_ba_set_marg_mode")

    def ba_marg_info(self, window=0):
        """vg_ba_batch_marg_info of a window of the downloaded batch: dict(valid, n, m, nblocks, eig1, eig2, word = the raw path word,
        stage1, cert, schur, stage2 = its fields by name; include/vinsgpu.h VG_MARGPATH_*)."""
        self.lib.vg_ba_batch_marg_info.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        out = (C.c_int * 8)()
        self._chk(self.lib.vg_ba_batch_marg_info(self.h, int(window), out), "vg_ba_batch_marg_info")
        w = int(out[6])
        return dict(valid=int(out[0]), n=int(out[1]), m=int(out[2]), nblocks=int(out[3]), eig1=int(out[4]), eig2=int(out[5]), word=w,
                    stage1=MARGPATH_STAGE1[w & 0xf], cert=MARGPATH_CERT[(w >> 4) & 3], schur=MARGPATH_SCHUR[(w >> 6) & 3],
                    stage2=MARGPATH_STAGE2[(w >> 8) & 0xf])

    def ba_set_imu_info_mode(self, mode):
        """VG_IMU_INFO_FACTOR (0, default) / VG_IMU_INFO_REFERENCE (1): form of the IMU factors' sqrt_info (include/vinsgpu.h)."""
        self.lib.vg_ba_set_imu_info_mode.argtypes = [C.c_void_p, C.c_int]
        self._chk(self.lib.vg_ba_set_imu_info_mode(self.h, int(mode)), "vg_ba_set_imu_info_mode")

    def rccl_unique_id(self):
        """128 bytes from ncclGetUniqueId (rank 0 calls this and broadcasts them)."""
        buf = C.create_string_buffer(128)
        self._chk(self.lib.vg_rccl_unique_id(buf), "vg_rccl_unique_id")
        return buf.raw

    def ba_rccl_init(self, nranks, rank, unique_id):
        """Collective: RCCL communicator on this handle's device + the C all-reduce hook (include/vinsgpu.h)."""
        self._chk(self.lib.vg_ba_rccl_init(self.h, int(nranks), int(rank), bytes(unique_id)), "vg_ba_rccl_init")

    def ba_rccl_finalize(self):
        self._chk(self.lib.vg_ba_rccl_finalize(self.h), "vg_ba_rccl_finalize")

    def ba_set_large_window(self, force=True):
        self._chk(self.lib.vg_ba_set_large_window(self.h, 1 if force else 0), "vg_ba_set_large_window")

    def ba_set_allreduce(self, fn):
        """fn(device_ptr: int, count: int, stream: int) must sum `count` doubles at device_ptr over all ranks in place,
        stream-ordered on the HIP stream `stream`; None removes the hook (single rank)."""
        if fn is None:
            self._hook = None
            self._chk(self.lib.vg_ba_set_allreduce(self.h, ALLREDUCE_FN(), None), "vg_ba_set_allreduce")
            return

        def tramp(user, buf, count, stream):
            try:
                fn(int(buf or 0), int(count), int(stream or 0))
                return 0
            except Exception as exc:                      # an exception must not unwind through the C frame
                self._hook_error = exc
                return 1
        self._hook = ALLREDUCE_FN(tramp)                  # keep the trampoline alive as long as the handle uses it
        self._chk(self.lib.vg_ba_set_allreduce(self.h, self._hook, None), "vg_ba_set_allreduce")

    def ba_reduce_layout(self):
        a, b = C.c_size_t(), C.c_size_t()
        self._chk(self.lib.vg_ba_reduce_layout(self.h, C.byref(a), C.byref(b)), "vg_ba_reduce_layout")
        return int(a.value), int(b.value)

    def ba_run_timed(self):
        """Synchronous run; returns (solve_kernel_ms, marg_kernel_ms) from HIP events on the launch stream."""
        a, b = C.c_float(), C.c_float()
        self._chk(self.lib.vg_ba_batch_run_timed(self.h, C.byref(a), C.byref(b)), "vg_ba_batch_run_timed")
        return float(a.value), float(b.value)

    KERNEL_CLASSES = ("ba_prologue_kernel", "ba_linearize_imu_kernel+ba_linearize_proj_kernel", "ba_accumulate_kernel", "ba_solve_kernel",
                      "ba_final_kernel", "ba_marg_kernel", "ba_big_schur_kernel", "ba_solve_big_kernel", "ba_big_step_kernel")

    def kernel_classes(self):
        """Names of the launch classes of the uploaded batch (VG_BA_KERNEL_*): with the fused projection kernel the accumulate class
        IS ba_linacc_proj_kernel (IMU + prior + projection factors: linearise + accumulate) and the linearize class is left with the
        cost-only pass of the last candidate."""
        k = list(self.KERNEL_CLASSES)
        mode = self.lib.vg_ba_batch_is_fused(self.h)
        if mode == 1:
            k[2] = "ba_linacc_proj_kernel"
        return k

    def ba_run_profiled(self):
        """Synchronous run with a HIP event after every launch: {kernel: (summed ms, launches)}."""
        ms = (C.c_float * len(self.KERNEL_CLASSES))()
        n = (C.c_int * len(self.KERNEL_CLASSES))()
        self._chk(self.lib.vg_ba_batch_run_profiled(self.h, ms, n), "vg_ba_batch_run_profiled")
        return {k: (float(ms[i]), int(n[i])) for i, k in enumerate(self.kernel_classes())}

    def ba_info(self):
        fl, bi, bo, lds = C.c_double(), C.c_double(), C.c_double(), C.c_int()
        self._chk(self.lib.vg_ba_batch_info(self.h, C.byref(fl), C.byref(bi), C.byref(bo), C.byref(lds)), "vg_ba_batch_info")
        fs, fm = C.c_double(), C.c_double()
        self._chk(self.lib.vg_ba_batch_flops(self.h, C.byref(fs), C.byref(fm)), "vg_ba_batch_flops")
        fk = (C.c_double * len(self.KERNEL_CLASSES))()
        self._chk(self.lib.vg_ba_batch_flops_by_kernel(self.h, fk), "vg_ba_batch_flops_by_kernel")
        return dict(flops=fl.value, flops_solve=fs.value, flops_marg=fm.value, bytes_in=bi.value, bytes_out=bo.value,
                    lds_bytes=lds.value, flops_by_kernel={k: float(fk[i]) for i, k in enumerate(self.kernel_classes())})

    def ba_prepare_download(self):
        """Allocate the host output buffers of the uploaded batch once (reused by every ba_download_raw())."""
        n = len(self._packed)
        outs = [_Out(p.K, p.L, p.has_relo, self._margin[i] != VG_MARGIN_NONE) for i, p in enumerate(self._packed)]
        st = (C.POINTER(State) * n)(*[C.pointer(o.state) for o in outs])
        pri = (C.POINTER(Prior) * n)(*[C.pointer(o.prior) if o.prior is not None else None for o in outs])
        sm = (Summary * n)()
        self._dl = (outs, st, pri, sm, list(self._packed))
        return self._dl

    def ba_download_raw(self):
        """vg_ba_batch_download into the buffers of ba_prepare_download(); returns the C-ABI status."""
        outs, st, pri, sm, _ = self._dl
        t0 = time.perf_counter()
        rc = self.lib.vg_ba_batch_download(self.h, len(outs), st, sm, pri)
        self.last_download_call_ms = (time.perf_counter() - t0) * 1e3      # the C-ABI call alone (sync + D2H + unpack)
        return rc

    def ba_download(self, allow_numeric_failure=False):
        outs, st, pri, sm, packed = self.ba_prepare_download()
        n = len(outs)
        rc = self.ba_download_raw()
        if rc != VG_OK and not (allow_numeric_failure and rc == -4):
            self._chk(rc, "vg_ba_batch_download")
        return ([o.state_dict(p.has_relo) for o, p in zip(outs, packed)],
                [summary_dict(sm[i]) for i in range(n)],
                [o.prior_dict() for o in outs])

    def ba_download_state_raw(self, dl=None):
        """vg_ba_batch_download_state into the buffers of ba_prepare_download(): returns while the marginalization runs."""
        outs, st, pri, sm, _ = dl if dl is not None else self._dl
        t0 = time.perf_counter()
        rc = self.lib.vg_ba_batch_download_state(self.h, len(outs), st, sm)
        self.last_download_call_ms = (time.perf_counter() - t0) * 1e3
        return rc

    def ba_download_prior_raw(self):
        outs, st, pri, sm, _ = self._dl
        return self.lib.vg_ba_batch_download_prior(self.h, len(outs), pri)

    def ba_optimize_split(self, prob, margin_flag=VG_MARGIN_NONE):
        """vg_ba_optimize in two parts: returns (state, summary, prior, ms until the states were on the host)."""
        t0 = time.perf_counter()
        self.ba_upload([prob], [margin_flag])
        self.ba_run_async()
        outs, st, pri, sm, packed = self.ba_prepare_download()
        self._chk(self.ba_download_state_raw(), "vg_ba_batch_download_state")
        t_state = (time.perf_counter() - t0) * 1e3
        state, summ = outs[0].state_dict(packed[0].has_relo), summary_dict(sm[0])
        self._chk(self.ba_download_prior_raw(), "vg_ba_batch_download_prior")
        return state, summ, outs[0].prior_dict(), t_state

    def ba_optimize(self, prob, margin_flag=VG_MARGIN_NONE):
        """One Estimator::optimization(): returns (state, summary, new_prior)."""
        self.ba_upload([prob], [margin_flag])
        self.ba_run_async()
        st, sm, pr = self.ba_download()
        return st[0], sm[0], pr[0]

    # ---- windows that stay on the device (include/vinsgpu.h vg_ba_seq_*)
    def ba_reserve(self, max_landmarks=0, max_factors=0, max_obs=0, max_prior_n=0):
        self._chk(self.lib.vg_ba_reserve(self.h, int(max_landmarks), int(max_factors), int(max_obs), int(max_prior_n)), "vg_ba_reserve")

    def seq_begin(self, windows, tracks, max_features=512, max_new_obs=512, max_landmarks=0, max_factors=0, init_depth=5.0,
                  min_parallax=10.0 / 460.0):
        """windows: prob dicts (states, imu, prior, options; landmark tables ignored); tracks[w]: dict(id, start, nobs, depth, obs
        [sum nobs x 8: x y z u v vx vy cur_td], optional solve_flag)."""
        n = len(windows)
        self._packed = [PackedProblem(p) for p in windows]
        arr = (C.POINTER(Problem) * n)(*[C.pointer(p.struct) for p in self._packed])
        self._margin = np.zeros(n, np.int32)
        keep, ts = [], (Tracks * n)()
        for w, t in enumerate(tracks):
            i4 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
            a = dict(id=i4(t['id']), start=i4(t['start']), nobs=i4(t['nobs']), depth=np.ascontiguousarray(t['depth'], dtype=np.float64),
                     obs=np.ascontiguousarray(t['obs'], dtype=np.float64).reshape(-1, 8),
                     flag=i4(t['solve_flag']) if t.get('solve_flag') is not None else None)
            keep.append(a)
            ts[w].n_features = len(a['id'])
            ts[w].feature_id, ts[w].start_frame, ts[w].n_obs = _ip(a['id']), _ip(a['start']), _ip(a['nobs'])
            ts[w].solve_flag = _ip(a['flag']) if a['flag'] is not None else None
            ts[w].depth, ts[w].obs = _dp(a['depth']), _dp(a['obs'])
        tp = (C.POINTER(Tracks) * n)(*[C.pointer(ts[w]) for w in range(n)])
        cfg = SeqConfig(int(max_features), int(max_new_obs), int(max_landmarks), int(max_factors), float(init_depth), float(min_parallax))
        self._seq_relo, reserved = False, getattr(self, "_relo_reserved", 0) > 0
        self._relo_reserved = 0                           # (consumed by this begin, whatever comes of it)
        self._chk(self.lib.vg_ba_seq_begin(self.h, n, C.byref(cfg), arr, tp), "vg_ba_seq_begin")
        self._seq_n = n
        self._seq_relo = reserved
        for p in self._packed:                            # size of the inverse-depth slab a state download fills
            p.L = (int(max_landmarks or max_features) + 15) // 16 * 16
            p.has_relo = reserved                         # (the loop-pose block: seq_states returns relo_pose)

    @staticmethod
    def seq_pack_frames(frames):
        """The vg_ba_frame* array of one step, built once (what a native caller holds): frames[w] = dict(pose (7,), sb (9,), imu_new,
        imu_merged (pre-integration dicts; imu_merged None unless the frame before was dropped as a non-keyframe), ids (n,),
        obs (n, 7) [x y z u v vx vy])."""
        n = len(frames)
        fs, keep = (Frame * n)(), []
        for w, f in enumerate(frames):
            ids = np.ascontiguousarray(f['ids'], dtype=np.int32)
            obs = np.ascontiguousarray(f['obs'], dtype=np.float64).reshape(-1, 7)
            inew = imu_struct(f['imu_new'])
            imrg = imu_struct(f['imu_merged']) if f.get('imu_merged') is not None else None
            keep.append((ids, obs, inew, imrg))
            fs[w].pose[:] = list(np.asarray(f['pose'], float)); fs[w].speedbias[:] = list(np.asarray(f['sb'], float))
            fs[w].imu_new = C.pointer(inew)
            fs[w].imu_merged = C.pointer(imrg) if imrg is not None else None
            fs[w].n_obs = len(ids)
            fs[w].feature_id, fs[w].obs = _ip(ids), _dp(obs)
        fp = (C.POINTER(Frame) * n)(*[C.pointer(fs[w]) for w in range(n)])
        return (n, fp, fs, keep)

    def seq_step(self, frames):
        """One frame for every window (vg_ba_seq_step_async); frames: a list of dicts or the result of seq_pack_frames."""
        packed = frames if isinstance(frames, tuple) else self.seq_pack_frames(frames)
        self._chk(self.lib.vg_ba_seq_step_async(self.h, packed[0], packed[1]), "vg_ba_seq_step_async")

    def seq_states(self, allow_numeric_failure=False):
        """States of the windows as the last step solved them (before the slide) and the summaries."""
        outs, st, pri, sm, packed = self.ba_prepare_download()
        rc = self.ba_download_state_raw()
        if rc != VG_OK and not (allow_numeric_failure and rc == -4):
            self._chk(rc, "vg_ba_batch_download_state")
        return [o.state_dict(getattr(self, "_seq_relo", False)) for o in outs], [summary_dict(sm[i]) for i in range(len(outs))]

    def seq_priors(self):
        """parity tap: the priors the last step's marginalization produced (None where the old one stays)."""
        outs, st, pri, sm, packed = self._dl
        self._chk(self.ba_download_prior_raw(), "vg_ba_batch_download_prior")
        return [o.prior_dict() for o in outs]

    def seq_info(self):
        a = np.zeros((self._seq_n, len(SEQ_INFO)), np.int32)
        self._chk(self.lib.vg_ba_seq_info(self.h, self._seq_n, _ip(a)), "vg_ba_seq_info")
        return [dict(zip(SEQ_INFO, map(int, r))) for r in a]

    def seq_tracks(self, w, K, cap=1024):
        n = C.c_int()
        ids, st, nb, fl = (np.zeros(cap, np.int32) for _ in range(4))
        dep, obs = np.zeros(cap), np.zeros((cap, K, 8))
        self._chk(self.lib.vg_ba_seq_get_tracks(self.h, int(w), cap, C.byref(n), _ip(ids), _ip(st), _ip(nb), _ip(fl), _dp(dep), _dp(obs)),
                  "vg_ba_seq_get_tracks")
        m = n.value
        return dict(id=ids[:m].copy(), start=st[:m].copy(), nobs=nb[:m].copy(), solve_flag=fl[:m].copy(), depth=dep[:m].copy(), obs=obs[:m].copy())

    def seq_export(self, w, K, raw_imu=False):
        """The window of slot w between two frames, as vg_ba_seq_begin takes it: (prob-dict fields, tracks dict).
        raw_imu: parity tap -- every record as the device holds it, with its `valid` flag (otherwise an invalid one is None)."""
        o = _Out(K, 0, False, True)
        imu = (ImuPreint * (K - 1))()
        self._chk(self.lib.vg_ba_seq_export(self.h, int(w), _dp(o.pose), _dp(o.sb), _dp(o.ex), _dp(o.td), imu, C.byref(o.prior)), "vg_ba_seq_export")
        recs = []
        for q in imu:
            recs.append(None if not (q.valid or raw_imu) else dict(
                **(dict(valid=int(q.valid)) if raw_imu else {}), sum_dt=q.sum_dt, delta_p=np.array(q.delta_p), delta_q=np.array(q.delta_q), delta_v=np.array(q.delta_v), lin_ba=np.array(q.linearized_ba),
                lin_bg=np.array(q.linearized_bg), jacobian=np.array(q.jacobian).reshape(15, 15), covariance=np.array(q.covariance).reshape(15, 15)))
        t = self.seq_tracks(w, K)
        rows = np.concatenate([t['obs'][f, :n][:, [0, 1, 7, 2, 3, 4, 5, 6]] for f, n in enumerate(t['nobs'])]) if len(t['id']) else np.zeros((0, 8))
        tracks = dict(id=t['id'], start=t['start'], nobs=t['nobs'], depth=t['depth'], solve_flag=t['solve_flag'], obs=rows)
        return dict(pose=o.pose.copy(), sb=o.sb.copy(), ex=o.ex.copy(), td=float(o.td[0]), imu=recs, prior=o.prior_dict()), tracks

    def seq_import(self, w, prob, tracks):
        """Replace what slot w of the running sequence holds (vg_ba_seq_import); prob / tracks as for seq_begin."""
        p = PackedProblem(prob)
        i4 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
        a = dict(id=i4(tracks['id']), start=i4(tracks['start']), nobs=i4(tracks['nobs']), depth=np.ascontiguousarray(tracks['depth'], dtype=np.float64),
                 obs=np.ascontiguousarray(tracks['obs'], dtype=np.float64).reshape(-1, 8),
                 flag=i4(tracks['solve_flag']) if tracks.get('solve_flag') is not None else None)
        t = Tracks()
        t.n_features = len(a['id'])
        t.feature_id, t.start_frame, t.n_obs = _ip(a['id']), _ip(a['start']), _ip(a['nobs'])
        t.solve_flag = _ip(a['flag']) if a['flag'] is not None else None
        t.depth, t.obs = _dp(a['depth']), _dp(a['obs'])
        self._chk(self.lib.vg_ba_seq_import(self.h, int(w), C.byref(p.struct), C.byref(t)), "vg_ba_seq_import")

    # ---- sequences that take raw IMU samples (include/vinsgpu.h vg_ba_seq_imu_*): processIMU on the device
    def seq_imu_begin(self, seeds, noise, max_samples=64, struct_size=None):
        """After seq_begin, before the first step.  seeds[w] = acc_0 (3), gyr_0 (3), g (3): the newest IMU measurement and the gravity
        vector of window w; noise = (acc_n, gyr_n, acc_w, gyr_w); max_samples: capacity of one frame's sample list (1 .. 512)."""
        s = np.ascontiguousarray(seeds, dtype=np.float64).reshape(-1, 9)
        cfg = SeqImuConfig(C.sizeof(SeqImuConfig) if struct_size is None else int(struct_size), int(max_samples))
        cfg.noise[:] = [float(x) for x in noise]
        self._chk(self.lib.vg_ba_seq_imu_begin(self.h, len(s), C.byref(cfg), _dp(s)), "vg_ba_seq_imu_begin")

    @staticmethod
    def seq_pack_frames_imu(frames):
        """The vg_ba_frame_imu* array of one step: frames[w] = dict(samples (n, 7) [dt acc gyr] in arrival order, ids (m,),
        obs (m, 7) [x y z u v vx vy])."""
        n = len(frames)
        fs, keep = (FrameImu * n)(), []
        for w, f in enumerate(frames):
            ids = np.ascontiguousarray(f['ids'], dtype=np.int32)
            obs = np.ascontiguousarray(f['obs'], dtype=np.float64).reshape(-1, 7)
            smp = None if f['samples'] is None else np.ascontiguousarray(f['samples'], dtype=np.float64).reshape(-1, 7)
            keep.append((ids, obs, smp))
            fs[w].n_samples = int(f['n_samples']) if 'n_samples' in f else (0 if smp is None else len(smp))
            fs[w].samples = _dp(smp) if smp is not None and smp.size else None
            fs[w].n_obs = len(ids)
            fs[w].feature_id, fs[w].obs = _ip(ids), _dp(obs)
        fp = (C.POINTER(FrameImu) * n)(*[C.pointer(fs[w]) for w in range(n)])
        return (n, fp, fs, keep)

    def seq_step_imu(self, frames):
        """One frame for every window from its raw IMU samples and observations (vg_ba_seq_step_imu_async); frames: a list of
        dicts or the result of seq_pack_frames_imu."""
        packed = frames if isinstance(frames, tuple) else self.seq_pack_frames_imu(frames)
        self._chk(self.lib.vg_ba_seq_step_imu_async(self.h, packed[0], packed[1]), "vg_ba_seq_step_imu_async")

    def seq_imu_get(self, w):
        """parity tap: dict(acc_0, gyr_0, g: the resident measurement and gravity; pose (7,), sb (9,): the state guess the LAST step
        propagated)."""
        seed, pose, sb = np.zeros(9), np.zeros(7), np.zeros(9)
        self._chk(self.lib.vg_ba_seq_imu_get(self.h, int(w), _dp(seed), _dp(pose), _dp(sb)), "vg_ba_seq_imu_get")
        return dict(acc_0=seed[:3].copy(), gyr_0=seed[3:6].copy(), g=seed[6:].copy(), pose=pose, sb=sb)

    def seq_imu_set(self, w, seed):
        """acc_0, gyr_0, g of ONE window, after seq_import of that window."""
        s = np.ascontiguousarray(seed, dtype=np.float64).reshape(9)
        self._chk(self.lib.vg_ba_seq_imu_set(self.h, int(w), _dp(s)), "vg_ba_seq_imu_set")

    def seq_imu_timing(self, on=True):
        """HIP events around ba_seq_imu_kernel and ba_seq_merge_kernel of every following step (vg_ba_seq_imu_timing)."""
        self._chk(self.lib.vg_ba_seq_imu_timing(self.h, 1 if on else 0), "vg_ba_seq_imu_timing")

    def seq_imu_times(self):
        """(ms in ba_seq_imu_kernel, ms in ba_seq_merge_kernel) of the last step, all windows of the batch."""
        a, b = C.c_float(), C.c_float()
        self._chk(self.lib.vg_ba_seq_imu_times(self.h, C.byref(a), C.byref(b)), "vg_ba_seq_imu_times")
        return float(a.value), float(b.value)

    # ---- relocalisation frames of a resident sequence (include/vinsgpu.h vg_ba_seq_relo_reserve / set_relo / get_relo)
    def seq_relo_reserve(self, max_match):
        """Before seq_begin: the next sequence gets the loop-pose block and room for max_match (1 .. 1024) relocalisation factors;
        0 cancels."""
        self._chk(self.lib.vg_ba_seq_relo_reserve(self.h, int(max_match)), "vg_ba_seq_relo_reserve")
        self._relo_reserved = int(max_match)

    def seq_set_relo(self, w, relo, struct_size=None):
        """Between two frames: arms window w for the next step.  relo = dict(frame, match_id (n,) ascending, match_xy (n, 2), optional
        pose (7,) [None: the resident pose of that frame], optional prev_t (3,), prev_r (3, 3)); None disarms."""
        if relo is None:
            self._chk(self.lib.vg_ba_seq_set_relo(self.h, int(w), None), "vg_ba_seq_set_relo")
            return
        ids = np.ascontiguousarray(relo['match_id'], dtype=np.int32)
        xy = np.ascontiguousarray(relo['match_xy'], dtype=np.float64).reshape(-1, 2)
        pose = None if relo.get('pose') is None else np.ascontiguousarray(relo['pose'], dtype=np.float64).reshape(7)
        r = ReloFrame()
        r.struct_size = C.sizeof(ReloFrame) if struct_size is None else int(struct_size)
        r.frame, r.n_match = int(relo['frame']), int(relo.get('n_match', len(ids)))
        r.pose = _dp(pose) if pose is not None else None
        r.match_id, r.match_xy = _ip(ids), _dp(xy)
        r.prev_relo_t[:] = [float(x) for x in np.asarray(relo.get('prev_t', np.zeros(3)), float).ravel()]
        r.prev_relo_r[:] = [float(x) for x in np.asarray(relo.get('prev_r', np.eye(3)), float).ravel()]
        self._chk(self.lib.vg_ba_seq_set_relo(self.h, int(w), C.byref(r)), "vg_ba_seq_set_relo")

    def seq_get_relo(self, w):
        """After seq_states of a step: dict(armed, n_factors, frame, pose (7,), relative_t, relative_q (x y z w), relative_yaw [deg],
        drift_r (3, 3), drift_t) of window w in that step."""
        o = ReloResult()
        o.struct_size = C.sizeof(ReloResult)
        self._chk(self.lib.vg_ba_seq_get_relo(self.h, int(w), C.byref(o)), "vg_ba_seq_get_relo")
        return dict(armed=int(o.armed), n_factors=int(o.n_factors), frame=int(o.frame), pose=np.array(o.pose[:]),
                    relative_t=np.array(o.relo_relative_t[:]), relative_q=np.array(o.relo_relative_q[:]), relative_yaw=float(o.relo_relative_yaw),
                    drift_r=np.array(o.drift_correct_r[:]).reshape(3, 3), drift_t=np.array(o.drift_correct_t[:]))

    # ---- keyframe message and point clouds of a resident sequence (include/vinsgpu.h vg_ba_seq_outputs_*)
    def seq_outputs_reserve(self, max_points):
        """Any time a sequence is live: room for max_points (1 .. 1024) rows per list and window; again: replaces."""
        self._chk(self.lib.vg_ba_seq_outputs_reserve(self.h, int(max_points)), "vg_ba_seq_outputs_reserve")
        self._out_mp = int(max_points)

    def seq_outputs_async(self):
        """Enqueue ba_seq_publish_kernel and the one download of every window's header and lists (vg_ba_seq_outputs_async)."""
        self._chk(self.lib.vg_ba_seq_outputs_async(self.h), "vg_ba_seq_outputs_async")

    def seq_outputs(self, window, struct_size=None):
        """What the last seq_outputs_async produced for one window: dict(status, keyframe_valid, n_keyframe, n_cloud, n_margin (true
        counts), pose (7,), ex_pose (7,), kf_point_3d (n, 3), kf_norm (n, 2), kf_uv (n, 2) float32, kf_id (n,) int32, cloud_xyz (n, 3),
        margin_xyz (n, 3) float32), the arrays cut to the stored counts min(n_*, max_points)."""
        mp = max(1, getattr(self, "_out_mp", 0))
        p3, nm, uv = np.zeros((mp, 3), np.float32), np.zeros((mp, 2), np.float32), np.zeros((mp, 2), np.float32)
        ids, pc, mg = np.zeros(mp, np.int32), np.zeros((mp, 3), np.float32), np.zeros((mp, 3), np.float32)
        fp = lambda a: a.ctypes.data_as(_pf)
        o = SeqOutputs()
        o.struct_size = C.sizeof(SeqOutputs) if struct_size is None else int(struct_size)
        o.kf_point_3d, o.kf_norm, o.kf_uv, o.kf_id, o.cloud_xyz, o.margin_xyz = fp(p3), fp(nm), fp(uv), _ip(ids), fp(pc), fp(mg)
        self._chk(self.lib.vg_ba_seq_get_outputs(self.h, int(window), C.byref(o)), "vg_ba_seq_get_outputs")
        nk, nc, nmg = (min(int(v), mp) for v in (o.n_keyframe, o.n_cloud, o.n_margin))
        return dict(status=int(o.status), keyframe_valid=int(o.keyframe_valid), n_keyframe=int(o.n_keyframe), n_cloud=int(o.n_cloud),
                    n_margin=int(o.n_margin), pose=np.array(o.pose[:]), ex_pose=np.array(o.ex_pose[:]), kf_point_3d=p3[:nk].copy(),
                    kf_norm=nm[:nk].copy(), kf_uv=uv[:nk].copy(), kf_id=ids[:nk].copy(), cloud_xyz=pc[:nc].copy(), margin_xyz=mg[:nmg].copy())

    def seq_end(self):
        self._chk(self.lib.vg_ba_seq_end(self.h), "vg_ba_seq_end")
        self._out_mp = 0

    # ---- the front end feeds the sequence on the device, one call per frame (include/vinsgpu.h vg_vio_*)
    def vio_begin(self, lists=False):
        """After tracks_begin (fe.FrontEnd on this handle), seq_begin and seq_imu_begin: stream c feeds window c.  lists: VG_VIO_LISTS,
        every step also returns the lists and the message (otherwise counts only)."""
        self._chk(self.lib.vg_vio_begin(self.h, 1 if lists else 0), "vg_vio_begin")
        self._vio_lists = bool(lists)

    def vio_step(self, front_end, samples, **step_args):
        """vg_vio_step_async: the frame of front_end.tracks_step(**step_args) and, when it publishes, the step of seq_step_imu with
        samples[c] for window c and the observations taken from stream c's message on the device (fe.FrontEnd.vio_step)."""
        return front_end.vio_step(samples, lists=getattr(self, "_vio_lists", False), **step_args)

    def vio_frame(self, w, cap=1024):
        """parity tap: (ids, obs (n, 7)) the last publishing vio_step staged for window w, read from the device"""
        n = C.c_int()
        ids, obs = np.zeros(max(cap, 1), np.int32), np.zeros((max(cap, 1), 7))
        self._chk(self.lib.vg_vio_get_frame(self.h, int(w), int(cap), C.byref(n), _ip(ids), _dp(obs)), "vg_vio_get_frame")
        return ids[:n.value].copy(), obs[:n.value].copy()

    def vio_end(self):
        self._chk(self.lib.vg_vio_end(self.h), "vg_vio_end")

    def imu_preintegrate(self, intervals, biases, noise):
        """Batched IntegrationBase (integration_base.h:30-158).  intervals[k] = [(dt, acc, gyr), ...] with entry 0 =
        (0, acc_0, gyr_0) the first measurement (the layout of synth.preintegrate); biases[k] = (ba, bg);
        noise = (acc_n, gyr_n, acc_w, gyr_w).  Returns the list of pre-integration dicts vg_ba_problem consumes."""
        n = len(intervals)
        off = np.zeros(n + 1, np.int32)
        rows, first = [], np.zeros((n, 6))
        for k, iv in enumerate(intervals):
            first[k, :3], first[k, 3:] = iv[0][1], iv[0][2]
            for dt, a, g in iv[1:]:
                rows.append([dt, a[0], a[1], a[2], g[0], g[1], g[2]])
            off[k + 1] = len(rows)
        smp = np.ascontiguousarray(rows if rows else np.zeros((1, 7)), dtype=np.float64)
        bias = np.ascontiguousarray([np.concatenate([np.asarray(b[0], float), np.asarray(b[1], float)]) for b in biases])
        nz = np.ascontiguousarray(noise, dtype=np.float64)
        out = (ImuPreint * n)()
        self._chk(self.lib.vg_imu_preintegrate(self.h, n, _ip(off), _dp(smp), _dp(np.ascontiguousarray(first)), _dp(bias), _dp(nz), out),
                  "vg_imu_preintegrate")
        res = []
        for q in out:
            res.append(dict(sum_dt=q.sum_dt, delta_p=np.array(q.delta_p), delta_q=np.array(q.delta_q), delta_v=np.array(q.delta_v),
                            lin_ba=np.array(q.linearized_ba), lin_bg=np.array(q.linearized_bg),
                            jacobian=np.array(q.jacobian).reshape(15, 15), covariance=np.array(q.covariance).reshape(15, 15)))
        return res

    @staticmethod
    def init_align_pack(windows):
        """(vg_align_in array, vg_align_out array, the NumPy arrays both point into) for init_align's window dicts"""
        n = len(windows)
        ins, outs, keep = (AlignIn * n)(), (AlignOut * n)(), []
        for w, (a, o) in zip(windows, zip(ins, outs)):
            R = np.array(w['R'], np.float64).reshape(-1, 9)               # (copies: the call never aliases the caller's arrays)
            F = len(R)
            T = np.array(w['T'], np.float64).reshape(F, 3)
            off, rows, first = np.zeros(F, np.int32), [], np.zeros((max(F - 1, 1), 6))
            for k, iv in enumerate(w['intervals']):
                first[k, :3], first[k, 3:] = iv[0][1], iv[0][2]
                for dt, acc, gyr in iv[1:]:
                    rows.append([dt, acc[0], acc[1], acc[2], gyr[0], gyr[1], gyr[2]])
                off[k + 1] = len(rows)
            smp = np.ascontiguousarray(rows if rows else np.zeros((1, 7)), dtype=np.float64)
            key = np.ascontiguousarray(w['key'] if w.get('key') is not None else [], np.int32)
            K = len(key)
            bufs = dict(R=R, T=T, off=off, smp=smp, first=first, key=key, v_body=np.zeros((F, 3)), records=(ImuPreint * max(F - 1, 1))(),
                        Ps=np.zeros((K, 3)), Rs=np.zeros((K, 3, 3)), Vs=np.zeros((K, 3)))
            keep.append(bufs)
            a.struct_size, a.n_frames, a.R, a.T, a.sample_off, a.samples, a.first = C.sizeof(AlignIn), F, _dp(R), _dp(T), _ip(off), _dp(smp), _dp(first)
            a.ba0[:], a.bg0[:] = [float(x) for x in w['ba0']], [float(x) for x in w['bg0']]
            a.noise[:], a.tic[:], a.g_norm = [float(x) for x in w['noise']], [float(x) for x in w['tic']], float(w['g_norm'])
            a.n_key = K
            if K:
                a.key = _ip(key)
                o.Ps, o.Rs, o.Vs = _dp(bufs['Ps']), _dp(bufs['Rs']), _dp(bufs['Vs'])
            o.struct_size, o.v_body, o.records = C.sizeof(AlignOut), _dp(bufs['v_body']), bufs['records']
        return ins, outs, keep

    def init_align(self, windows):
        """VisualIMUAlignment and the state change of visualInitialAlign for a batch of windows (vg_init_align).  A window is a dict:
        R [F][3][3], T [F][3] (ImageFrame::R / T), intervals (F - 1 lists in the layout of imu_preintegrate), ba0, bg0, noise, tic,
        g_norm, key (ascending frame indices of the window, or None).  Returns one dict per window."""
        ins, outs, keep = self.init_align_pack(windows)
        self._chk(self.lib.vg_init_align(self.h, len(windows), ins, outs), "vg_init_align")
        res = []
        for o, b in zip(outs, keep):
            recs = [dict(sum_dt=q.sum_dt, delta_p=np.array(q.delta_p), delta_q=np.array(q.delta_q), delta_v=np.array(q.delta_v),
                         lin_ba=np.array(q.linearized_ba), lin_bg=np.array(q.linearized_bg),
                         jacobian=np.array(q.jacobian).reshape(15, 15), covariance=np.array(q.covariance).reshape(15, 15))
                    for q in b['records'][:len(b['R']) - 1]]
            res.append(dict(status=int(o.status), delta_bg=np.array(o.delta_bg), bg=np.array(o.bg), g_lin=np.array(o.g_lin), s_lin=float(o.s_lin),
                            g_c0=np.array(o.g_c0), s=float(o.s), v_body=b['v_body'], records=recs, Ps=b['Ps'], Rs=b['Rs'], Vs=b['Vs'],
                            g_w=np.array(o.g_w), R0=np.array(o.R0).reshape(3, 3)))
        return res

    @staticmethod
    def init_sfm_pack(windows, timed=False):
        """(vg_sfm_in array, vg_sfm_out array, the NumPy arrays both point into) for init_sfm's window dicts"""
        n = len(windows)
        ins, outs, keep = (SfmIn * n)(), (SfmOut * n)(), []
        i32 = lambda v: np.ascontiguousarray(v, np.int32).reshape(-1)
        for w, (a, o) in zip(windows, zip(ins, outs)):
            F = int(w['n_frames'])
            start, nobs, fid = i32(w['start']), i32(w['nobs']), i32(w['feature_id'])
            nf = len(start)
            off = i32(w['obs_off']) if w.get('obs_off') is not None else i32(np.concatenate([[0], np.cumsum(nobs)[:-1]]))
            points = np.array(w['points'], np.float64).reshape(-1, 3)           # (copies: the call never aliases the caller's arrays)
            all_key, all_guess = i32(w.get('all_key', [])), i32(w.get('all_guess', []))
            na = len(all_key)
            all_off, ids, xy = np.zeros(na + 1, np.int32), [], []
            for e in range(na):
                pts = w['all_pts'][e]
                if all_key[e] < 0 and pts is not None:
                    ids.extend(int(x) for x in pts[0])
                    xy.extend(np.asarray(pts[1], np.float64).reshape(-1, 2).tolist())
                all_off[e + 1] = len(ids)
            ids, xy = i32(ids if ids else [0]), np.ascontiguousarray(xy if xy else np.zeros((1, 2)), np.float64)
            bufs = dict(start=start, nobs=nobs, fid=fid, off=off, points=points, all_key=all_key, all_guess=all_guess, all_off=all_off, ids=ids, xy=xy,
                        q=np.zeros((F, 4)), T=np.zeros((F, 3)), state=np.zeros(nf, np.int32), position=np.zeros((nf, 3)), R_all=np.zeros((na, 3, 3)),
                        T_all=np.zeros((na, 3)), is_key=np.zeros(max(na, 1), np.int32), q0=np.zeros((F, 4)), T0=np.zeros((F, 3)), position0=np.zeros((nf, 3)),
                        pnp_iters=np.zeros(F, np.int32), pnp_up=np.zeros(F, np.int32), device_ms=np.zeros(2))
            keep.append(bufs)
            a.struct_size, a.n_frames, a.l, a.n_feat, a.n_all = C.sizeof(SfmIn), F, int(w['l']), nf, na
            a.relative_R[:] = [float(x) for x in np.asarray(w['relative_R']).reshape(-1)]
            a.relative_T[:] = [float(x) for x in w['relative_T']]
            a.ric[:] = [float(x) for x in np.asarray(w['ric']).reshape(-1)]
            a.feature_id, a.start, a.nobs, a.obs_off, a.points = _ip(fid), _ip(start), _ip(nobs), _ip(off), _dp(points)
            if na:
                a.all_key, a.all_guess, a.all_off, a.all_id, a.all_xy = _ip(all_key), _ip(all_guess), _ip(all_off), _ip(ids), _dp(xy)
            o.struct_size = C.sizeof(SfmOut)
            o.q, o.T, o.state, o.position, o.q0, o.T0, o.position0 = (_dp(bufs['q']), _dp(bufs['T']), _ip(bufs['state']), _dp(bufs['position']),
                                                                       _dp(bufs['q0']), _dp(bufs['T0']), _dp(bufs['position0']))
            o.pnp_iters, o.pnp_up = _ip(bufs['pnp_iters']), _ip(bufs['pnp_up'])
            if na:                                              # (n_all = 0: construct only, every all_* table and output stays NULL)
                o.R_all, o.T_all, o.is_key = _dp(bufs['R_all']), _dp(bufs['T_all']), _ip(bufs['is_key'])
            if timed:
                o.device_ms = _dp(bufs['device_ms'])
        return ins, outs, keep

    def init_sfm(self, windows, timed=False):
        """GlobalSFM::construct and the per-frame PnP of Estimator::initialStructure for a batch of windows (vg_init_sfm).  A window is a
        dict: n_frames, l, relative_R [3][3], relative_T, ric [3][3], feature_id, start, nobs, points (x y z rows, feature after feature;
        obs_off optional), all_key, all_guess, all_pts (per entry None or (ids ascending, xy)).  Returns one dict per window; with
        timed, the first carries device_ms: the device time of the two launches."""
        ins, outs, keep = self.init_sfm_pack(windows, timed)
        self._chk(self.lib.vg_init_sfm(self.h, len(windows), ins, outs), "vg_init_sfm")
        res = []
        for o, b in zip(outs, keep):
            it = int(o.ba_iters)
            d = dict(status=int(o.status), ba_iters=it, ba_termination=int(o.ba_termination), final_cost=float(o.final_cost),
                     it_cost=np.array(o.it_cost)[:it], it_cost_cand=np.array(o.it_cost_cand)[:it], it_model=np.array(o.it_model)[:it],
                     it_radius=np.array(o.it_radius)[:it], it_flags=np.array(o.it_flags)[:it])
            d.update({k: b[k] for k in ('q', 'T', 'state', 'position', 'R_all', 'T_all', 'q0', 'T0', 'position0', 'pnp_iters', 'pnp_up')})
            d['is_key'] = b['is_key'][:len(b['all_key'])]
            if timed:
                d['device_ms'] = b['device_ms']
            res.append(d)
        return res

    RELPOSE_TAPS = ('n_corres', 'avg_parallax', 'gate', 'ransac_iter', 'ransac_bound', 'ransac_inliers', 'ransac_best', 'F', 'good', 'winner', 'inlier_cnt',
                    'used_fallback')

    @staticmethod
    def init_relpose_pack(windows, timed=False):
        """(vg_relpose_in array, vg_relpose_out array, the NumPy arrays both point into) for init_relpose's window dicts"""
        n = len(windows)
        ins, outs, keep = (RelposeIn * n)(), (RelposeOut * n)(), []
        i32 = lambda v: np.ascontiguousarray(v, np.int32).reshape(-1)
        for w, (a, o) in zip(windows, zip(ins, outs)):
            F = int(w['n_frames'])
            start, nobs = i32(w['start']), i32(w['nobs'])
            nf, nc = len(start), max(F - 1, 1)
            off = i32(w['obs_off']) if w.get('obs_off') is not None else i32(np.concatenate([[0], np.cumsum(nobs)[:-1]]))
            points = np.array(w['points'], np.float64).reshape(-1, 3)           # (copies: the call never aliases the caller's arrays)
            bufs = dict(start=start, nobs=nobs, off=off, points=points, mask=np.zeros(max(nf, 1), np.uint8), ransac_mask=np.zeros(max(nf, 1), np.uint8),
                        n_corres=np.zeros(nc, np.int32), avg_parallax=np.zeros(nc), gate=np.zeros(nc, np.int32), ransac_iter=np.zeros(nc, np.int32),
                        ransac_bound=np.zeros(nc, np.int32), ransac_inliers=np.zeros(nc, np.int32), ransac_best=np.zeros(nc, np.int32), F=np.zeros((nc, 3, 3)),
                        good=np.zeros((nc, 4), np.int32), winner=np.zeros(nc, np.int32), inlier_cnt=np.zeros(nc, np.int32),
                        used_fallback=np.zeros(nc, np.int32), device_ms=np.zeros(RELPOSE_LAUNCHES))
            keep.append(bufs)
            a.struct_size, a.n_frames, a.n_feat = C.sizeof(RelposeIn), F, nf
            a.start, a.nobs, a.obs_off, a.points = _ip(start), _ip(nobs), _ip(off), _dp(points)
            for k, v in RELPOSE_DEFAULTS.items():
                setattr(a, k, type(v)(w.get(k, v)))
            o.struct_size = C.sizeof(RelposeOut)
            o.mask, o.ransac_mask = bufs['mask'].ctypes.data_as(_pu8), bufs['ransac_mask'].ctypes.data_as(_pu8)
            for k in Handle.RELPOSE_TAPS:
                setattr(o, k, _dp(bufs[k]) if bufs[k].dtype == np.float64 else _ip(bufs[k]))
            if timed:
                o.device_ms = _dp(bufs['device_ms'])
        return ins, outs, keep

    def init_relpose(self, windows, timed=False):
        """Estimator::relativePose for a batch of windows (vg_init_relpose): the candidate frames 0 .. F-2 against F-1, the first one that
        passes the parallax gate and whose solveRelativeRT succeeds is l.  A window is a dict with the feature tables of init_sfm
        (n_frames, start, nobs, points as x y z rows, obs_off optional) and, optionally, the constants of RELPOSE_DEFAULTS.  Returns one
        dict per window: status (RELPOSE_*), l (-1: none), relative_R [3][3], relative_T, mask / ransac_mask over the correspondences
        of l, and the per-candidate taps of RELPOSE_TAPS; with timed, the first carries device_ms, one figure per launch."""
        ins, outs, keep = self.init_relpose_pack(windows, timed)
        self._chk(self.lib.vg_init_relpose(self.h, len(windows), ins, outs), "vg_init_relpose")
        res = []
        for w, o, b in zip(windows, outs, keep):
            nc = int(w['n_frames']) - 1
            d = dict(status=int(o.status), l=int(o.l), relative_R=np.array(o.relative_R).reshape(3, 3), relative_T=np.array(o.relative_T),
                     mask=b['mask'][:int(o.n_mask)], ransac_mask=b['ransac_mask'][:int(o.n_mask)])
            d.update({k: b[k][:nc] for k in self.RELPOSE_TAPS})
            if timed:
                d['device_ms'] = b['device_ms']
            res.append(d)
        return res

    EXROT_TAPS = ('records', 'ric', 'sigma', 'ok', 'huber', 'branch', 'ransac_iter', 'ransac_bound', 'ransac_inliers', 'ransac_best', 'F', 'front', 'picked',
                  'used_fallback')

    @staticmethod
    def init_exrot_pack(windows, timed=False):
        """(vg_exrot_in array, vg_exrot_out array, the NumPy arrays both point into) for init_exrot's window dicts"""
        n = len(windows)
        ins, outs, keep = (ExrotIn * n)(), (ExrotOut * n)(), []
        for w, (a, o) in zip(windows, zip(ins, outs)):
            steps = [np.asarray(c, np.float64).reshape(-1, 4) for c in w['corr']]
            S, ns = len(steps), max(len(steps), 1)
            corr_off = np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(c) for c in steps])]), np.int32)
            corr = np.ascontiguousarray(np.concatenate(steps + [np.zeros((1, 4))]))     # (never empty: the pointer is not NULL)
            dq = np.array(w['delta_q'], np.float64).reshape(-1, 4)
            prev = np.array(w.get('prev', np.zeros((0, 27))), np.float64).reshape(-1, 27)
            n_prev = len(prev)
            prev = np.ascontiguousarray(np.concatenate([prev, np.zeros((1, 27))]))
            ric_prev = np.array(w.get('ric_prev', np.eye(3)), np.float64).reshape(9)
            bufs = dict(corr_off=corr_off, corr=corr, delta_q=dq, prev=prev, ric_prev=ric_prev, records=np.zeros((ns, 27)), ric=np.zeros((ns, 3, 3)),
                        sigma=np.zeros((ns, 4)), ok=np.zeros(ns, np.int32), huber=np.zeros(ns), branch=np.zeros(ns, np.int32),
                        ransac_iter=np.zeros(ns, np.int32), ransac_bound=np.zeros(ns, np.int32), ransac_inliers=np.zeros(ns, np.int32),
                        ransac_best=np.zeros(ns, np.int32), F=np.zeros((ns, 3, 3)), front=np.zeros((ns, 4), np.int32), picked=np.zeros(ns, np.int32),
                        used_fallback=np.zeros(ns, np.int32), device_ms=np.zeros(EXROT_LAUNCHES))
            keep.append(bufs)
            a.struct_size, a.n_steps, a.n_prev = C.sizeof(ExrotIn), S, n_prev
            a.corr_off, a.corr, a.delta_q, a.prev, a.ric_prev = _ip(corr_off), _dp(corr), _dp(dq), _dp(prev), _dp(ric_prev)
            for k, v in EXROT_DEFAULTS.items():
                setattr(a, k, type(v)(w.get(k, v)))
            o.struct_size = C.sizeof(ExrotOut)
            for k in Handle.EXROT_TAPS:
                setattr(o, k, _dp(bufs[k]) if bufs[k].dtype == np.float64 else _ip(bufs[k]))
            if timed:
                o.device_ms = _dp(bufs['device_ms'])
        return ins, outs, keep

    def init_exrot(self, windows, timed=False):
        """InitialEXRotation::CalibrationExRotation for a batch of windows (vg_init_exrot), a run of consecutive calls per window.  A window
        is a dict with corr (one [n, 4] array x0 y0 x1 y1 per step), delta_q ([S][4], w x y z) and, to resume a run, prev ([n_prev][27]
        records) and ric_prev; optionally the constants of EXROT_DEFAULTS.  Returns one dict per window: status (EXROT_*), first_ok (-1:
        none), calib_ric [3][3] and the per-step arrays of EXROT_TAPS; with timed, the first carries device_ms, one figure per launch."""
        ins, outs, keep = self.init_exrot_pack(windows, timed)
        self._chk(self.lib.vg_init_exrot(self.h, len(windows), ins, outs), "vg_init_exrot")
        res = []
        for w, o, b in zip(windows, outs, keep):
            S = len(w['corr'])
            d = dict(status=int(o.status), first_ok=int(o.first_ok), calib_ric=np.array(o.calib_ric).reshape(3, 3))
            d.update({k: b[k][:S] for k in self.EXROT_TAPS})
            if timed:
                d['device_ms'] = b['device_ms']
            res.append(d)
        return res

    def triangulate(self, Ps, Rs, tic, ric, start, nobs, obs_off, points, init_depth=5.0):
        """FeatureManager::triangulate (feature_manager.cpp:202-257); returns the depth per landmark."""
        Ps = np.ascontiguousarray(Ps, np.float64); Rs = np.ascontiguousarray(Rs, np.float64)
        K, Ln = len(Ps), len(start)
        st = np.ascontiguousarray(start, np.int32); nb = np.ascontiguousarray(nobs, np.int32); oo = np.ascontiguousarray(obs_off, np.int32)
        pts = np.ascontiguousarray(points, np.float64)
        out = np.zeros(max(Ln, 1))
        self._chk(self.lib.vg_triangulate(self.h, K, _dp(Ps), _dp(Rs), _dp(np.ascontiguousarray(tic, np.float64)),
                                          _dp(np.ascontiguousarray(ric, np.float64)), Ln, _ip(st), _ip(nb), _ip(oo), _dp(pts),
                                          float(init_depth), _dp(out)), "vg_triangulate")
        return out[:Ln]

    def ba_eval_factors(self, prob):
        p = PackedProblem(prob)
        F = int((p.keep['lm_nobs'] - 1).sum()) + (len(prob['relo']['match']) if prob.get('relo') else 0)
        K = p.K
        n = int(prob['prior']['n']) if prob.get('prior') is not None else 0
        pr, pJ = np.zeros((F, 2)), np.zeros((F, 2, 20))
        ir, iJ = np.zeros((K - 1, 15)), np.zeros((K - 1, 15, 30))
        qr = np.zeros(max(n, 1))
        self._chk(self.lib.vg_ba_eval_factors(self.h, C.byref(p.struct), _dp(pr), _dp(pJ), _dp(ir), _dp(iJ), _dp(qr)),
                  "vg_ba_eval_factors")
        return dict(proj_r=pr, proj_J=pJ, imu_r=ir, imu_J=iJ, prior_r=qr[:n])
