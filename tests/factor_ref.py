"""80-bit reference, metric, case table, yardstick and edits for the factor level of bundle adjustment: proj_eval, imu_ctx /
imu_raw_col, prior_pass and the sqrt-info prologue (csrc/ba_factors.h, csrc/ba_pipeline.hip), all reached through
Handle.ba_eval_factors (helper module of tests/test_factor_scale.py; no tests in here).

The reference restates, in the requested number format,
    IMUFactor::Evaluate ................. factor/imu_factor.h:19-179  (sqrt_info: imu_factor.h:64)
    IntegrationBase::evaluate ........... factor/integration_base.h:160-186
    ProjectionFactor::Evaluate .......... factor/projection_factor.cpp:21-121
    ProjectionTdFactor::Evaluate ........ factor/projection_td_factor.cpp:34-141
    MarginalizationFactor::Evaluate ..... factor/marginalization_factor.cpp:333-381
    Utility::deltaQ / Qleft / Qright .... utility/utility.h:16-68
The inputs are the float64 inputs, widened: the reference answers for the numbers the device got.  With np.longdouble (80-bit) it is
the reference; with np.float64 it repeats oracle/ba_numpy (imu_factor, projection_factor, projection_td_factor, prior_factor)
operation by operation -- bit-identical, asserted in tests/test_factor_scale.py -- and takes the EDITS of the mutation condition.

The 80-bit IMU weight is U^-1 with covariance = U U^T, U upper triangular: the unique upper factor of covariance^-1, which is what
LLT(covariance.inverse()).matrixL().transpose() of imu_factor.h:64 defines.  numpy.linalg takes no long doubles: the 15 x 15 loops
are written out (upper_factor, upper_inverse).  The float64 route inverts and factorises, as the oracle does.

`*_error(got, ref)` measure a difference against what it subtracts, one number per field kind (KINDS):
    imu_J    D = U_ref J_dev in 80 bits gives the factor's raw Jacobian back; per 3 x 3 block of the 5 x 10 partition
             ([P, R, V, BA, BG] x [P_i, theta_i, V_i, BA_i, BG_i, P_j, theta_j, V_j, BA_j, BG_j]) max|D - Jraw_ref| / max|Jraw_ref| of
             the block; a block the reference has zero is measured against the largest entry of its 3-row band
    imu_r    U_ref r_dev against the raw residual per 3-row band: P against max(|R_i^-1 (..)|, |corrected_delta_p|), V the same with
             v, R against 2, BA / BG against max(|b_i|, |b_j|)
    exact zeros (inf when violated): W is upper triangular, weighted row r combines raw rows >= r only, so a column in which those
             raw rows are all zero holds exact zeros (rows 12-14 outside BG_i / BG_j ...); a skipped factor (sum_dt > 10) is all zero
    proj_J   per factor the 2 x 3 blocks P_i, theta_i, P_j, theta_j, t_ic, theta_ic and the 2 x 1 blocks lambda, td, each against its
             own largest |ref|; a block the reference has zero (td with estimate_td = 0 or zero feature velocities) must be exactly 0
    proj_r   against focal / 1.5 * max(|pcj.xy / z|, |pts_j|)
    prior_r  row i against |r0_i| + sum_k |J0_ik| |dx_k|.  At x0 the reference's own expression q0^-1 q (conjugate / squaredNorm, then the
             product) leaves rounding residue for dx in every number format, so those cases have the kind prior_r_x0; the hand-made
             prior with a dyadic quaternion, where the product is exact, must give r0 bit for bit
Kinds with a conditioning of their own (far positions, lambda blocks that cancel, x0) are listed at KINDS below.

The yardstick: e64(case) = the error of the float64 restatement against the 80-bit one; E64 per kind = the largest over the table.
No device takes part in either."""
import functools

import numpy as np

from oracle import ba_numpy as B
from vins_mono_amd import synth

import ba_step_ref as S
import imu_ref as IR

LD = np.longdouble
# Field kinds.  Where float64 itself loses orders of magnitude more than elsewhere -- by cancellation in the reference's own expressions,
# not by anything a kernel does -- the cases have a kind, and with it an E64, of their own, so that they do not widen the others' bound:
#   *_far           IMU cases with positions near 1e5 m (P_j - P_i cancels five digits before it is rotated)
#   proj_J_lambda   lambda blocks that cancel to less than 1 / LAMBDA_CANCEL of their terms, the point's own |p| / z included (zero
#                   baseline, points kilometres or centimetres away: the reprojection hardly depends on the depth); decided from the
#                   reference, every other lambda block counts as proj_J
#   prior_r_x0      the state equal to x0: dx is what is left of q0^-1 q0 (two rounded products that cancel), carried by J0
KINDS = ('imu_J', 'imu_r', 'imu_J_far', 'imu_r_far', 'proj_J', 'proj_J_lambda', 'proj_r', 'prior_r', 'prior_r_x0')
LAMBDA_CANCEL = 64.0
# the device's bound is M[kind] * E64[kind]; the reference-info mode (inverse() then LLT on the device) has factors of its own
M = dict(imu_J=2, imu_r=4, imu_J_far=4, imu_r_far=4, imu_J_refinfo=4, imu_r_refinfo=4, imu_J_far_refinfo=4, imu_r_far_refinfo=4,
         proj_J=2, proj_J_lambda=8, proj_r=4, prior_r=2, prior_r_x0=1)
O_P, O_R, O_V, O_BA, O_BG = B.O_P, B.O_R, B.O_V, B.O_BA, B.O_BG
G_NORM = synth.EUROC['g_norm']

IMU_EDITS = ('imu_dtheta_i_delta_q', 'imu_dbg_i_corrected_delta_q', 'imu_r_without_dq_dbg', 'imu_r_without_dp_dbg',
             'imu_dtheta_j_qright', 'imu_r_w_flip', 'imu_W_p_bg_entry')
PROJ_EDITS = ('proj_row_term_dropped', 'proj_cur_td_of_j_for_i', 'proj_td_without_vel_j', 'proj_lambda_one_over_lambda',
              'proj_ex_third_skew_dropped', 'proj_reduce_one_over_z')
PRIOR_EDITS = ('prior_sign_flip_dropped', 'prior_factor_2_dropped', 'prior_sb_6_of_9')
EDITS = IMU_EDITS + PROJ_EDITS + PRIOR_EDITS


# --------------------------------------------------------------------------------------------------- helpers in any number format
def _w(v, dtype):
    return np.asarray(v, np.float64).astype(dtype)


def qinv(q):
    """B.qinv without its detour through a Python float (Eigen: conjugate / squaredNorm)"""
    return np.array([-q[0], -q[1], -q[2], q[3]]) / np.dot(q, q)


def qleft(q, dtype):
    """utility.h:51-59, 4 x 4 in (w, x, y, z) order"""
    v, w = q[:3], q[3]
    m = np.zeros((4, 4), dtype)
    m[0, 0] = w
    m[0, 1:] = -v
    m[1:, 0] = v
    m[1:, 1:] = w * np.eye(3, dtype=dtype) + B.skew(v)
    return m


def qright(q, dtype):
    """utility.h:61-68"""
    v, w = q[:3], q[3]
    m = np.zeros((4, 4), dtype)
    m[0, 0] = w
    m[0, 1:] = -v
    m[1:, 0] = v
    m[1:, 1:] = w * np.eye(3, dtype=dtype) - B.skew(v)
    return m


def upper_factor(cov):
    """U upper triangular with cov = U U^T (columns from the last to the first), in cov's own number format"""
    n = cov.shape[0]
    U = np.zeros_like(cov)
    for j in range(n - 1, -1, -1):
        d = cov[j, j]
        for k in range(j + 1, n):
            d = d - U[j, k] * U[j, k]
        assert d > 0, "the covariance is not positive definite"
        U[j, j] = np.sqrt(d)
        for i in range(j):
            s = cov[i, j]
            for k in range(j + 1, n):
                s = s - U[i, k] * U[j, k]
            U[i, j] = s / U[j, j]
    return U


def upper_inverse(U):
    """X = U^-1 (upper triangular), column by column, back substitution upward"""
    n = U.shape[0]
    X = np.zeros_like(U)
    for j in range(n):
        for i in range(j, -1, -1):
            s = U.dtype.type(1 if i == j else 0)
            for k in range(i + 1, j + 1):
                s = s - U[i, k] * X[k, j]
            X[i, j] = s / U[i, i]
    return X


def rot_q(axis, angle):
    """unit quaternion [x, y, z, w] of a rotation by `angle` about `axis`"""
    a = np.asarray(axis, float)
    a = a / np.linalg.norm(a)
    return np.concatenate([a * np.sin(angle / 2), [np.cos(angle / 2)]])


# --------------------------------------------------------------------------------------------------- the IMU factor
def imu_factor(pre, pose_i, sb_i, pose_j, sb_j, g_norm=G_NORM, dtype=LD, edit=None):
    """IMUFactor::Evaluate + IntegrationBase::evaluate.  Returns dict(r, J: weighted 15 / 15 x 30 [pose_i 6 | sb_i 9 | pose_j 6 |
    sb_j 9], r_raw, J_raw, W = sqrt_info, U (80-bit only: covariance = U U^T), scale: the residual's five band scales)."""
    pose_i, sb_i, pose_j, sb_j = (_w(v, dtype) for v in (pose_i, sb_i, pose_j, sb_j))
    G = np.array([0, 0, dtype(np.float64(g_norm))])
    Pi, Qi = pose_i[:3], pose_i[3:]
    Pj, Qj = pose_j[:3], pose_j[3:]
    Vi, Bai, Bgi = sb_i[0:3], sb_i[3:6], sb_i[6:9]
    Vj, Baj, Bgj = sb_j[0:3], sb_j[3:6], sb_j[6:9]
    Jm = _w(pre['jacobian'], dtype).reshape(15, 15)
    delta_p, delta_q, delta_v = _w(pre['delta_p'], dtype), _w(pre['delta_q'], dtype), _w(pre['delta_v'], dtype)
    dp_dba, dp_dbg = Jm[O_P:O_P + 3, O_BA:O_BA + 3], Jm[O_P:O_P + 3, O_BG:O_BG + 3]
    dq_dbg = Jm[O_R:O_R + 3, O_BG:O_BG + 3]
    dv_dba, dv_dbg = Jm[O_V:O_V + 3, O_BA:O_BA + 3], Jm[O_V:O_V + 3, O_BG:O_BG + 3]
    sum_dt = dtype(np.float64(pre['sum_dt']))
    dba, dbg = Bai - _w(pre['lin_ba'], dtype), Bgi - _w(pre['lin_bg'], dtype)
    corrected_delta_q = B.qmul(delta_q, B.deltaQ(dq_dbg @ dbg))                       # integration_base.h:171-174
    corrected_delta_v = delta_v + dv_dba @ dba + dv_dbg @ dbg
    corrected_delta_p = delta_p + dp_dba @ dba + dp_dbg @ dbg
    residual_delta_q, residual_delta_p = corrected_delta_q, corrected_delta_p
    if edit == 'imu_r_without_dq_dbg':
        residual_delta_q = delta_q
    if edit == 'imu_r_without_dp_dbg':
        residual_delta_p = delta_p + dp_dba @ dba
    Qi_inv = qinv(Qi)
    Ri_inv = B.q2R(Qi_inv)
    vP = Ri_inv @ (0.5 * G * sum_dt * sum_dt + Pj - Pi - Vi * sum_dt)
    vV = Ri_inv @ (G * sum_dt + Vj - Vi)
    r = np.zeros(15, dtype)
    r[O_P:O_P + 3] = vP - residual_delta_p                                           # integration_base.h:176-180
    qe = B.qmul(qinv(residual_delta_q), B.qmul(Qi_inv, Qj))
    r[O_R:O_R + 3] = 2 * qe[:3]
    if edit == 'imu_r_w_flip' and qe[3] < 0:
        r[O_R:O_R + 3] = -r[O_R:O_R + 3]
    r[O_V:O_V + 3] = vV - corrected_delta_v
    r[O_BA:O_BA + 3] = Baj - Bai
    r[O_BG:O_BG + 3] = Bgj - Bgi
    Qj_inv = qinv(Qj)
    J0 = np.zeros((15, 6), dtype)                                                     # imu_factor.h:83-106
    J0[O_P:O_P + 3, 0:3] = -Ri_inv
    J0[O_P:O_P + 3, 3:6] = B.skew(vP)
    J0[O_R:O_R + 3, 3:6] = -(qleft(B.qmul(Qj_inv, Qi), dtype)
                             @ qright(delta_q if edit == 'imu_dtheta_i_delta_q' else corrected_delta_q, dtype))[1:, 1:]
    J0[O_V:O_V + 3, 3:6] = B.skew(vV)
    J1 = np.zeros((15, 9), dtype)                                                     # imu_factor.h:107-137
    J1[O_P:O_P + 3, 0:3] = -Ri_inv * sum_dt
    J1[O_P:O_P + 3, 3:6] = -dp_dba
    J1[O_P:O_P + 3, 6:9] = -dp_dbg
    J1[O_R:O_R + 3, 6:9] = -qleft(B.qmul(B.qmul(Qj_inv, Qi), corrected_delta_q if edit == 'imu_dbg_i_corrected_delta_q' else delta_q),
                                  dtype)[1:, 1:] @ dq_dbg
    J1[O_V:O_V + 3, 0:3] = -Ri_inv
    J1[O_V:O_V + 3, 3:6] = -dv_dba
    J1[O_V:O_V + 3, 6:9] = -dv_dbg
    J1[O_BA:O_BA + 3, 3:6] = -np.eye(3, dtype=dtype)
    J1[O_BG:O_BG + 3, 6:9] = -np.eye(3, dtype=dtype)
    J2 = np.zeros((15, 6), dtype)                                                     # imu_factor.h:138-156
    J2[O_P:O_P + 3, 0:3] = Ri_inv
    qj_side = B.qmul(qinv(corrected_delta_q), B.qmul(Qi_inv, Qj))
    J2[O_R:O_R + 3, 3:6] = (qright if edit == 'imu_dtheta_j_qright' else qleft)(qj_side, dtype)[1:, 1:]
    J3 = np.zeros((15, 9), dtype)                                                     # imu_factor.h:157-175
    J3[O_V:O_V + 3, 0:3] = Ri_inv
    J3[O_BA:O_BA + 3, 3:6] = np.eye(3, dtype=dtype)
    J3[O_BG:O_BG + 3, 6:9] = np.eye(3, dtype=dtype)
    out = dict(r_raw=r, J_raw=np.hstack([J0, J1, J2, J3]))
    if dtype is np.float64:
        W = B.imu_sqrt_info(np.asarray(pre['covariance'], np.float64).reshape(15, 15))
    else:
        out['U'] = upper_factor(_w(pre['covariance'], dtype).reshape(15, 15))
        W = upper_inverse(out['U'])
    if edit == 'imu_W_p_bg_entry':
        W = W.copy()
        W[1, 13] = W[1, 13] * (1 + dtype(1e-9))
    out['W'] = W
    out['r'] = W @ r
    out['J'] = np.hstack([W @ J0, W @ J1, W @ J2, W @ J3])
    big = lambda *v: max(float(np.abs(x).max()) for x in v)
    out['scale'] = (big(vP, corrected_delta_p), 2.0, big(vV, corrected_delta_v), big(Bai, Baj), big(Bgi, Bgj))
    out['qe_w'] = float(qe[3])
    if dtype is not np.float64:
        # conditioning of the kinds: the weighted rows combine raw rows through |U| |W|; the P / V bands subtract positions / velocities
        big1 = lambda v: float(np.abs(v).max())
        out['cond'] = max(float((np.abs(out['U']) @ np.abs(W)).max()),
                          (big1(Pi) + big1(Pj) + big1(Vi * sum_dt) + float(0.5 * G[2] * sum_dt * sum_dt)) / out['scale'][0],
                          (big1(Vi) + big1(Vj) + float(G[2] * sum_dt)) / out['scale'][2])
    return out


def imu_error(got, ref, far=False):
    """got: dict(r 15, J 15 x 30) of a device or of the float64 restatement; ref: imu_factor(..., LD) or None for a skipped factor.
    Returns dict(imu_J, imu_r) (far: dict(imu_J_far, imu_r_far)); inf where an exact zero is not one."""
    kJ, kr = ('imu_J_far', 'imu_r_far') if far else ('imu_J', 'imu_r')
    gr, gJ = np.asarray(got['r'], np.float64), np.asarray(got['J'], np.float64).reshape(15, 30)
    if not (np.all(np.isfinite(gr)) and np.all(np.isfinite(gJ))):
        return {kJ: np.inf, kr: np.inf}
    if ref is None:
        return {kJ: 0.0 if not gJ.any() else np.inf, kr: 0.0 if not gr.any() else np.inf}
    U, Jr, rr = ref['U'], ref['J_raw'], ref['r_raw']
    D = U @ gJ.astype(LD)
    eJ = 0.0
    for bi in range(5):
        band = Jr[3 * bi:3 * bi + 3]
        for bj in range(10):
            blk = band[:, 3 * bj:3 * bj + 3]
            m = np.abs(blk).max()
            m = m if m > 0 else np.abs(band).max()
            eJ = max(eJ, float(np.abs(D[3 * bi:3 * bi + 3, 3 * bj:3 * bj + 3] - blk).max() / m))
    for row in range(15):                                                             # exact zeros of the weighted Jacobian
        dead = ~np.any(Jr[row:] != 0, axis=0)
        if np.any(gJ[row, dead] != 0):
            eJ = np.inf
    d = np.abs(U @ gr.astype(LD) - rr)
    er = 0.0
    for b in range(5):
        s, e = ref['scale'][b], float(d[3 * b:3 * b + 3].max())
        er = max(er, e / s if s > 0 else (0.0 if e == 0 else np.inf))
    return {kJ: eJ, kr: er}


# --------------------------------------------------------------------------------------------------- the projection factors
def projection_factor(pose_i, pose_j, ex, inv_dep, td, obs_i, obs_j, focal, tr, row, with_td, dtype=LD, edit=None):
    """ProjectionFactor::Evaluate (with_td = False: td, tr, row and the observations' velocity / row / cur_td are not read) or
    ProjectionTdFactor::Evaluate.  obs_* = [x, y, u, v, vx, vy, cur_td].  Returns dict(r 2, J 2 x 20 [pose_i 6 | pose_j 6 | ex 6 |
    lambda | td], scale: the residual's)."""
    pose_i, pose_j, ex, obs_i, obs_j = (_w(v, dtype) for v in (pose_i, pose_j, ex, obs_i, obs_j))
    inv_dep, focal = dtype(np.float64(inv_dep)), dtype(np.float64(focal))
    sqrt_info = focal / 1.5
    pts_i = np.array([obs_i[0], obs_i[1], dtype(1)])
    pts_j = np.array([obs_j[0], obs_j[1], dtype(1)])
    Pi, Qi = pose_i[:3], pose_i[3:]
    Pj, Qj = pose_j[:3], pose_j[3:]
    tic, qic = ex[:3], ex[3:]
    Ri, Rj, ric = B.q2R(Qi), B.q2R(Qj), B.q2R(qic)
    vel_i = vel_j = None
    if with_td:                                                                       # projection_td_factor.cpp:18-19, :53-56
        td, tr, row = dtype(np.float64(td)), dtype(np.float64(tr)), dtype(np.float64(row))
        vel_i = np.array([obs_i[4], obs_i[5], dtype(0)])
        vel_j = np.array([obs_j[4], obs_j[5], dtype(0)])
        td_i, td_j = obs_i[6], obs_j[6]
        if edit == 'proj_cur_td_of_j_for_i':
            td_i = td_j
        row_i, row_j = obs_i[3] - row / 2, obs_j[3] - row / 2
        if edit == 'proj_row_term_dropped':
            pts_i_td = pts_i - (td - td_i) * vel_i
            pts_j_td = pts_j - (td - td_j) * vel_j
        else:
            pts_i_td = pts_i - (td - td_i + tr / row * row_i) * vel_i
            pts_j_td = pts_j - (td - td_j + tr / row * row_j) * vel_j
    else:
        pts_i_td, pts_j_td = pts_i, pts_j
    pts_camera_i = pts_i_td / inv_dep
    pts_imu_i = ric @ pts_camera_i + tic
    pts_w = Ri @ pts_imu_i + Pi
    pts_imu_j = B.q2R(qinv(Qj)) @ (pts_w - Pj)
    pts_camera_j = B.q2R(qinv(qic)) @ (pts_imu_j - tic)
    dep_j = pts_camera_j[2]
    r = sqrt_info * ((pts_camera_j / dep_j)[:2] - pts_j_td[:2])
    z2 = dep_j if edit == 'proj_reduce_one_over_z' else dep_j * dep_j
    reduce = sqrt_info * np.array([[1.0 / dep_j, 0, -pts_camera_j[0] / z2],
                                   [0, 1.0 / dep_j, -pts_camera_j[1] / (dep_j * dep_j)]])
    jaco_i = np.hstack([ric.T @ Rj.T, ric.T @ Rj.T @ Ri @ -B.skew(pts_imu_i)])
    jaco_j = np.hstack([ric.T @ -Rj.T, ric.T @ B.skew(pts_imu_j)])
    tmp_r = ric.T @ Rj.T @ Ri @ ric
    third = B.skew(ric.T @ (Rj.T @ (Ri @ tic + Pi - Pj) - tic))
    if edit == 'proj_ex_third_skew_dropped':
        third = 0 * third
    jaco_ex = np.hstack([ric.T @ (Rj.T @ Ri - np.eye(3, dtype=dtype)),
                         -tmp_r @ B.skew(pts_camera_i) + B.skew(tmp_r @ pts_camera_i)
                         + third])
    lam2 = inv_dep if edit == 'proj_lambda_one_over_lambda' else inv_dep * inv_dep
    J = np.zeros((2, 20), dtype)
    if with_td:
        j_l = reduce @ tmp_r @ pts_i_td * -1.0 / lam2
        vj = 0 * vel_j[:2] if edit == 'proj_td_without_vel_j' else vel_j[:2]
        J[:, 19] = reduce @ tmp_r @ vel_i / inv_dep * -1.0 + sqrt_info * vj
    else:
        j_l = reduce @ ric.T @ Rj.T @ Ri @ ric @ pts_i * -1.0 / lam2
    J[:, 0:6], J[:, 6:12], J[:, 12:18], J[:, 18] = reduce @ jaco_i, reduce @ jaco_j, reduce @ jaco_ex, j_l
    scale = float(sqrt_info * max(np.abs((pts_camera_j / dep_j)[:2]).max(), np.abs(pts_j_td[:2]).max()))
    lam_terms = np.abs(reduce) @ np.abs(tmp_r @ pts_i_td) / (inv_dep * inv_dep)        # what the lambda block's sum subtracts
    ex_terms = np.abs(reduce) @ (np.abs(tmp_r) @ np.abs(B.skew(pts_camera_i)) + np.abs(B.skew(tmp_r @ pts_camera_i)) + np.abs(third))
    p_over_z = float((np.abs(pts_w).max() + np.abs(Pj).max()) / abs(dep_j))           # what the point in camera j lost on its way there
    return dict(r=r, J=J, scale=scale, dep_j=float(dep_j), lam_cancel=float(lam_terms.max() / np.abs(J[:, 18]).max()) * max(1.0, p_over_z),
                ex_cancel=float(ex_terms.max() / np.abs(J[:, 15:18]).max()), p_over_z=p_over_z)


PROJ_BLOCKS = (('P_i', 0, 3), ('theta_i', 3, 6), ('P_j', 6, 9), ('theta_j', 9, 12), ('t_ic', 12, 15), ('theta_ic', 15, 18),
               ('lambda', 18, 19), ('td', 19, 20))


def proj_error(got, ref):
    gr, gJ = np.asarray(got['r'], np.float64), np.asarray(got['J'], np.float64).reshape(2, 20)
    if not (np.all(np.isfinite(gr)) and np.all(np.isfinite(gJ))):
        return dict(proj_J=np.inf, proj_r=np.inf)
    out = dict(proj_J=0.0, proj_r=float(np.abs(gr.astype(LD) - ref['r']).max() / ref['scale']))
    for name, a, b in PROJ_BLOCKS:
        blk, g = ref['J'][:, a:b], gJ[:, a:b].astype(LD)
        m = np.abs(blk).max()
        if m == 0:
            e = 0.0 if not g.any() else np.inf
        else:
            e = float(np.abs(g - blk).max() / m)
        kind = 'proj_J_lambda' if name == 'lambda' and ref['lam_cancel'] > LAMBDA_CANCEL else 'proj_J'
        out[kind] = max(out.get(kind, 0.0), e)
    return out


# --------------------------------------------------------------------------------------------------- the prior
def prior_factor(prior, blocks_now, dtype=LD, edit=None):
    """MarginalizationFactor::Evaluate: dx per kept block (marginalization_factor.cpp:343-363), r = r0 + J0 dx (:364).  Returns
    dict(r, dx, scale: |r0_i| + sum_k |J0_ik| |dx_k|, dq_w: the w of every pose block's relative quaternion)."""
    dx = np.zeros(prior['n'], dtype)
    off, dq_w = 0, []
    for (kind, _), x, x0 in zip(prior['blocks'], blocks_now, prior['x0']):
        x, x0 = _w(np.atleast_1d(x), dtype), _w(np.atleast_1d(x0), dtype)
        if B.GSIZE[kind] != 7:
            dx[off:off + B.LSIZE[kind]] = x - x0
            if edit == 'prior_sb_6_of_9' and kind == B.KIND_SB:
                dx[off + 6:off + 9] = 0
        else:
            dx[off:off + 3] = x[:3] - x0[:3]
            dq = B.qmul(qinv(x0[3:]), x[3:])
            two = 1.0 if edit == 'prior_factor_2_dropped' else 2.0
            dx[off + 3:off + 6] = two * dq[:3]
            if not (dq[3] >= 0) and edit != 'prior_sign_flip_dropped':
                dx[off + 3:off + 6] = two * -dq[:3]
            dq_w.append(float(dq[3]))
        off += B.LSIZE[kind]
    r0, J0 = _w(prior['r0'], dtype), _w(prior['J0'], dtype)
    return dict(r=r0 + J0 @ dx, dx=dx, scale=np.abs(r0) + np.abs(J0) @ np.abs(dx), dq_w=dq_w)


def prior_error(got_r, ref, at_x0=False):
    kind = 'prior_r_x0' if at_x0 else 'prior_r'
    g = np.asarray(got_r, np.float64)
    if g.shape != ref['r'].shape or not np.all(np.isfinite(g)):
        return {kind: np.inf}
    d, s = np.abs(g.astype(LD) - ref['r']), ref['scale']
    if np.any(d[s == 0] != 0):
        return {kind: np.inf}
    return {kind: float((d[s > 0] / s[s > 0]).max()) if np.any(s > 0) else 0.0}


# --------------------------------------------------------------------------------------------------- the IMU cases
# (imu_ref.CASES' n1 is not here: the covariance of ONE mid-point step has rank 12 -- p and v are both driven by the same six noise
#  terms -- so covariance^-1 and its factor do not exist in any number format; n2 is the shortest record that has a weight)
IMU_RECORDS = ('n2', 'n20', 'n64', 'varying_dt', 'fast_rotation', 'n99_dt0.1', 'n120_dt0.1')
IMU_SKIPPED = 'n120_dt0.1'
# (residual: consistent with the record / off by 0.5 m, 0.2 rad, 1 m/s) x (bias at / 1e-4 from / 0.3, 0.1 from the linearisation point), then
# the special states on the consistent one with the 1e-4 bias and on the perturbed one with the far bias
IMU_STATES = tuple((c, b, 'plain') for c in ('consistent', 'perturbed') for b in ('bias0', 'bias1e-4', 'bias_far')) + \
    tuple((c, b, s) for s in ('antipodal', 'rot178', 'far_position') for (c, b) in (('consistent', 'bias1e-4'), ('perturbed', 'bias_far')))


@functools.lru_cache(maxsize=None)
def imu_record(name):
    """the pre-integration record as the float64 oracle produces it (imu_ref.CASES; n99_dt0.1: one interval just under 10 s)"""
    if name == 'n99_dt0.1':
        rng = np.random.default_rng(20261021)
        iv = IR._interval(rng, 99, 0.1)
        ba, bg = IR._bias(rng)
        return IR.oracle64(iv, ba, bg, IR.NOISE)
    c = IR.CASES[name]
    return IR.oracle64(c['iv'], c['ba'], c['bg'], c['noise'])


def _unit(rng):
    v = rng.normal(0, 1, 3)
    return v / np.linalg.norm(v)


def _imu_state(rng, pre, consistency, bias, special):
    """(pose_i, sb_i, pose_j, sb_j), float64: frame j is what the record, corrected for the bias offset, predicts from frame i (the
    residual is rounding noise and the bias random walk), then perturbed / made special"""
    G = np.array([0, 0, G_NORM])
    Qi = B.qnormalized(rng.normal(0, 1, 4))
    Pi, Vi = rng.normal(0, 3, 3), rng.normal(0, 1, 3)
    dba, dbg = {'bias0': (np.zeros(3), np.zeros(3)), 'bias1e-4': (1e-4 * _unit(rng), 1e-4 * _unit(rng)),
                'bias_far': (0.3 * _unit(rng), 0.1 * _unit(rng))}[bias]
    Bai, Bgi = pre['lin_ba'] + dba, pre['lin_bg'] + dbg
    dba, dbg = Bai - pre['lin_ba'], Bgi - pre['lin_bg']
    Jm, dt = np.asarray(pre['jacobian'], float).reshape(15, 15), float(pre['sum_dt'])
    cdq = B.qmul(pre['delta_q'], B.deltaQ(Jm[3:6, 12:15] @ dbg))
    cdp = pre['delta_p'] + Jm[0:3, 9:12] @ dba + Jm[0:3, 12:15] @ dbg
    cdv = pre['delta_v'] + Jm[6:9, 9:12] @ dba + Jm[6:9, 12:15] @ dbg
    Ri = B.q2R(Qi)
    Pj = Pi + Vi * dt - 0.5 * G * dt * dt + Ri @ cdp
    Vj = Vi - G * dt + Ri @ cdv
    Qj = B.qnormalized(B.qmul(Qi, B.qnormalized(cdq)))
    Baj, Bgj = Bai + rng.normal(0, 1e-4, 3), Bgi + rng.normal(0, 1e-5, 3)
    if consistency == 'perturbed':
        Pj = Pj + 0.5 * _unit(rng)
        Vj = Vj + 1.0 * _unit(rng)
        Qj = B.qnormalized(B.qmul(Qj, rot_q(_unit(rng), 0.2)))
    if special == 'antipodal':
        Qj = -Qj
    elif special == 'rot178':
        Qj = B.qnormalized(B.qmul(Qj, rot_q(_unit(rng), np.radians(178.0))))
    elif special == 'far_position':
        far = 1e5 * np.array([1.0, -0.8, 0.3])
        Pi, Pj = Pi + far, Pj + far
    return np.concatenate([Pi, Qi]), np.concatenate([Vi, Bai, Bgi]), np.concatenate([Pj, Qj]), np.concatenate([Vj, Baj, Bgj])


@functools.lru_cache(maxsize=None)
def imu_cases():
    """name -> dict(record, pre, pose_i, sb_i, pose_j, sb_j, state: (consistency, bias, special))"""
    rng = np.random.default_rng(20261022)
    cases = {}
    for rec in IMU_RECORDS:
        pre = imu_record(rec)
        for st in (IMU_STATES if rec != IMU_SKIPPED else IMU_STATES[4:5]):
            pi, si, pj, sj = _imu_state(rng, pre, *st)
            cases[f"{rec}/{'/'.join(st)}"] = dict(record=rec, pre=pre, pose_i=pi, sb_i=si, pose_j=pj, sb_j=sj, state=st)
    return cases


@functools.lru_cache(maxsize=None)
def imu_reference(name):
    c = imu_cases()[name]
    if c['record'] == IMU_SKIPPED:
        return None
    return imu_factor(c['pre'], c['pose_i'], c['sb_i'], c['pose_j'], c['sb_j'])


def imu_float64(name, edit=None):
    c = imu_cases()[name]
    return imu_factor(c['pre'], c['pose_i'], c['sb_i'], c['pose_j'], c['sb_j'], dtype=np.float64, edit=edit)


def unit_qic():
    """The EuRoC ric as a UNIT quaternion.  The calibration file gives ric to twelve digits, R2q of it has |q|^2 = 1 - 2.3e-13, and for a
    quaternion that is not one the kernel's R(qic)^T is not the reference's R(qic^-1) = R(conj(qic) / |qic|^2): they differ by
    |q|^2 - 1, 1e3 roundings here.  Parameter blocks are normalised by PoseLocalParameterization::Plus after every step, so the factor
    level is tested on unit quaternions (every pose of the tables is normalised as well)."""
    return B.qnormalized(B.R2q(synth.EUROC['ric']))


def _empty_window(K):
    c = synth.EUROC
    return dict(ex=np.concatenate([c['tic'], unit_qic()]), td=0.0, estimate_extrinsic=0, estimate_td=0, max_iters=0, focal=c['focal'], tr=0.0,
                row=float(c['height']), g_norm=G_NORM, prior=None, relo=None, pose=np.zeros((K, 7)), sb=np.zeros((K, 9)),
                inv_depth=np.zeros(0), lm_start=np.zeros(0, np.int32), lm_nobs=np.zeros(0, np.int32), obs_off=np.zeros(0, np.int32),
                obs=np.zeros((0, 7)), imu=[None] * (K - 1))


@functools.lru_cache(maxsize=None)
def imu_windows():
    """The IMU cases two to a window of K = 4 frames, no landmarks: frames 0, 1 hold one case, frames 2, 3 the next, and the factor
    between frames 1 and 2 is absent (vg_imu_preint::valid = 0: its rows stay zero).  [(prob, (name at factor 0, name at factor 2 | None))]"""
    names = list(imu_cases())
    out = []
    for k in range(0, len(names), 2):
        pair = (names[k], names[k + 1] if k + 1 < len(names) else None)
        prob = _empty_window(4 if pair[1] else 2)
        for slot, name in enumerate(pair):
            if name is None:
                continue
            c = imu_cases()[name]
            prob['pose'][2 * slot], prob['pose'][2 * slot + 1] = c['pose_i'], c['pose_j']
            prob['sb'][2 * slot], prob['sb'][2 * slot + 1] = c['sb_i'], c['sb_j']
            prob['imu'][2 * slot] = c['pre']
        out.append((prob, pair))
    return out


# --------------------------------------------------------------------------------------------------- the projection cases
# landmark -> (x, y of the first observation | None: derived, inverse depth | None: derived, feature velocity px-normalised / s,
#              cur_td offsets (i, j) from td, image rows v (i, j) | None: from y, number of observations)
PROJ_CONFIGS = dict(plain=dict(estimate_extrinsic=0, estimate_td=0, tr=0.0), ex=dict(estimate_extrinsic=1, estimate_td=0, tr=0.0),
                    td=dict(estimate_extrinsic=0, estimate_td=1, tr=0.0), ex_td_tr=dict(estimate_extrinsic=1, estimate_td=1, tr=0.02))
PROJ_LANDMARKS = {
    'lambda1e-4': dict(xy=(0.11, -0.07), lam=1e-4), 'lambda1e-3': dict(xy=(-0.21, 0.13), lam=1e-3), 'lambda0.2': dict(xy=(0.31, 0.22), lam=0.2),
    'lambda20': dict(xy=(-0.05, 0.09), lam=20.0, nobs=2),                       # 5 cm in front of camera i: seen across the pure rotation only
    'image_edge': dict(xy=(0.81, 0.51), lam=0.15),
    'z_j0.1': dict(zj=0.1, xyj=(0.2, -0.15)),                                   # 10 cm in front of camera 2
    'td_plus_minus': dict(xy=(0.25, -0.2), lam=0.3, dtd=(-0.03, 0.03)), 'td_minus_plus': dict(xy=(-0.3, 0.1), lam=0.12, dtd=(0.03, -0.03)),
    'row_top': dict(xy=(0.1, None), lam=0.25, rows=(0.0, 0.0)), 'row_bottom': dict(xy=(-0.15, None), lam=0.18, rows=(479.0, 479.0)),
    'velocity0': dict(xy=(0.05, 0.3), lam=0.4, vel=0.0, dtd=(-0.03, 0.03)),
}
PROJ_TD = 0.004


@functools.lru_cache(maxsize=None)
def proj_window(config):
    """K = 3 frames with the EuRoC ric / tic: frame 1 is frame 0 rotated by 4 degrees on the spot (zero baseline), frame 2 lies 0.4 m
    further along camera 0's optical axis (and 5, 3 cm aside), rotated by 3 degrees.  Every landmark starts at frame 0: one factor
    across the zero baseline, one across the forward motion.  Observations in frames 1, 2: the projection plus 1e-3 of noise."""
    c = synth.EUROC
    rng = np.random.default_rng(20261023)
    prob = _empty_window(3)
    prob.update(PROJ_CONFIGS[config])
    prob['td'] = PROJ_TD if prob['estimate_td'] else 0.0
    if prob['estimate_extrinsic']:
        prob['ex'] = prob['ex'].copy()
        prob['ex'][:3] += rng.normal(0, 0.01, 3)
    q0 = B.qnormalized(np.array([0.12, -0.08, 0.31, 0.93]))
    R0 = B.q2R(q0)
    P0 = np.array([1.0, 2.0, 0.5])
    q1 = B.qnormalized(B.qmul(q0, rot_q([0.3, 1.0, -0.2], np.radians(4.0))))
    q2 = B.qnormalized(B.qmul(q0, rot_q([-0.5, 0.2, 1.0], np.radians(3.0))))
    P2 = P0 + R0 @ (c['ric'] @ np.array([0.05, -0.03, 0.4]))
    prob['pose'] = np.array([np.concatenate([P0, q0]), np.concatenate([P0, q1]), np.concatenate([P2, q2])])
    prob['sb'] = np.zeros((3, 9))
    prob['imu'] = [None, None]
    tic, ric = prob['ex'][:3], B.q2R(prob['ex'][3:])
    cam = lambda f, Xw: ric.T @ (B.q2R(prob['pose'][f][3:]).T @ (Xw - prob['pose'][f][:3]) - tic)
    start, nobs, off, obs, lam = [], [], [], [], []
    for name, d in PROJ_LANDMARKS.items():
        n = d.get('nobs', 3)
        rows = d.get('rows')
        if 'zj' in d:
            pcj = np.array([d['xyj'][0], d['xyj'][1], 1.0]) * d['zj']
            Xw = B.q2R(prob['pose'][2][3:]) @ (ric @ pcj + tic) + prob['pose'][2][:3]
            pci = cam(0, Xw)
            xy, lm = pci[:2] / pci[2], 1.0 / pci[2]
        else:
            x, y = d['xy']
            y = (rows[0] - c['cy']) / c['fy'] if y is None else y
            xy, lm = np.array([x, y]), d['lam']
            Xw = R0 @ (ric @ (np.array([xy[0], xy[1], 1.0]) / lm) + tic) + P0
        v = d.get('vel', 2.0)
        dtd = d.get('dtd', (0.0, 0.0))
        start.append(0); nobs.append(n); off.append(len(obs)); lam.append(lm)
        for f in range(n):
            p = cam(f, Xw)
            pxy = xy if f == 0 else p[:2] / p[2] + rng.normal(0, 1e-3, 2)
            row_v = c['fy'] * pxy[1] + c['cy'] if rows is None else rows[min(f, 1)]
            vel = v * np.array([1.0, -0.75]) * (1 if f != 1 else -0.5)
            obs.append([pxy[0], pxy[1], c['fx'] * pxy[0] + c['cx'], row_v, vel[0], vel[1], prob['td'] + dtd[min(f, 1)]])
    prob.update(lm_start=np.array(start, np.int32), lm_nobs=np.array(nobs, np.int32), obs_off=np.array(off, np.int32), obs=np.array(obs, float),
                inv_depth=np.array(lam, float))
    return prob


@functools.lru_cache(maxsize=None)
def relo_window():
    """one relocalisation frame with 8 matches (ba_step_ref.relocalisation_problem, K = 11, 40 landmarks): the first 8 whose track starts
    BEFORE the loop frame (the loop pose is a shifted copy of that frame's: for a track anchored there R_j^T R_i - I, the t_ic block, is
    zero in exact arithmetic and rounding residue in any number format)"""
    prob = S.relocalisation_problem()
    prob['ex'] = np.concatenate([prob['ex'][:3], B.qnormalized(prob['ex'][3:])])
    prob['relo'] = dict(pose=prob['relo']['pose'], match=[m for m in prob['relo']['match'] if prob['lm_start'][m[0]] < 3][:8])
    assert len(prob['relo']['match']) == 8
    return prob


def proj_windows():
    return dict([(k, proj_window(k)) for k in PROJ_CONFIGS] + [('relo', relo_window())])


def proj_factor_names(wname):
    prob = proj_windows()[wname]
    if wname == 'relo':
        nf = int((prob['lm_nobs'] - 1).sum())
        return [f"relo/f{f}" for f in range(nf)] + [f"relo/match{k}" for k in range(8)]
    lms = list(PROJ_LANDMARKS)
    return [f"{wname}/{lms[l]}/0-{fj}" for (l, _, fj, _, _) in B.factor_list(prob)]


def proj_table(prob, dtype=LD, edit=None):
    """every projection factor of the window in B.factor_list's order (the order of Handle.ba_eval_factors): [dict(r, J, scale)]"""
    st = B.state_of(prob)
    K = prob['pose'].shape[0]
    out = []
    for (l, fi, fj, oi, oj) in B.factor_list(prob):
        pj = st['pose'][fj] if fj < K else st['relo_pose']
        out.append(projection_factor(st['pose'][fi], pj, st['ex'], st['inv_depth'][l], st['td'], oi, oj, prob['focal'], prob['tr'], prob['row'],
                                     bool(prob['estimate_td']), dtype, edit))
    return out


def device_order(prob):
    """Row f of Handle.ba_eval_factors' projection tables as an index into B.factor_list: the library keeps the factors landmark-major
    and a landmark's relocalisation factor follows its window factors (B.factor_list, like estimator.cpp:769-801, has them at the end)"""
    facs = B.factor_list(prob)
    relo = prob.get('relo')
    if relo is None:
        return list(range(len(facs)))
    nreg = len(facs) - len(relo['match'])
    relo_of = {int(m[0]): k for k, m in enumerate(relo['match'])}
    order, f = [], 0
    for l in range(len(prob['inv_depth'])):
        n = int(prob['lm_nobs'][l]) - 1
        order += range(f, f + n)
        f += n
        if l in relo_of:
            order.append(nreg + relo_of[l])
    assert sorted(order) == list(range(len(facs)))
    return order


@functools.lru_cache(maxsize=None)
def proj_reference(wname):
    return proj_table(proj_windows()[wname])


# --------------------------------------------------------------------------------------------------- the prior cases
PRIOR_STATES = ('at_x0', 'dx1e-3', 'dx0.3', 'antipodal', 'rot179')


def _small_first(ex, td):
    prob = S.ruled_window(700 + 2 * ex + td, K=4, n_landmarks=8, anchor='all_at_0', length='full', estimate_extrinsic=ex, estimate_td=td)
    if td:
        prob['tr'] = 0.02
    return synth.SyntheticSequence.anchor_prior(prob)


@functools.lru_cache(maxsize=None)
def priors():
    """name -> prior (B.marginalize): MARGIN_OLD of a K = 4 window without / with the extrinsic and td blocks (n = 33, 34: the extrinsic
    block is kept either way), the second-new marginalization of the window after it (n = 27), a hand-made one (n = 15) and the n = 75 prior of the K = 11 fixture of test_factor_parity
    (above the stride of 64 of prior_pass's four-way row split)."""
    out = {}
    for name, (ex, td) in (('old_K4', (0, 0)), ('old_K4_ex_td', (1, 1))):
        prob = _small_first(ex, td)
        out[name] = B.marginalize(prob, B.state_of(prob), B.MARGIN_OLD)
    nxt = dict(_small_first(0, 0))
    nxt['prior'] = out['old_K4']
    out['second_new_K4'] = B.marginalize(nxt, B.state_of(nxt), B.MARGIN_SECOND_NEW)
    seq = synth.SyntheticSequence(21, L=40)
    prob = seq.window(0)
    x, _ = B.solve(prob)
    out['old_K11_n75'] = B.marginalize(prob, B.double2vector(prob, x), B.MARGIN_OLD)
    assert (out['old_K4']['n'], out['old_K4_ex_td']['n'], out['second_new_K4']['n'], out['old_K11_n75']['n']) == (33, 34, 27, 75)
    # a hand-made prior on pose 0 | speed-bias 0 whose quaternion has dyadic entries: q0^-1 q0 is exact with or without fused
    # multiply-adds, so at x0 dx IS zero and prior_r must be r0 bit for bit (with the priors above that holds for no float64
    # implementation of the reference's expression, the oracle included: prior_r_x0)
    rng = np.random.default_rng(20261025)
    x0 = [np.concatenate([rng.normal(0, 3, 3), [0.5, -0.5, 0.5, 0.5]]), rng.normal(0, 0.5, 9)]
    out['dyadic'] = dict(n=15, blocks=[(B.KIND_POSE, 0), (B.KIND_SB, 0)], J0=rng.normal(0, 30, (15, 15)), r0=rng.normal(0, 1, 15), x0=x0)
    return out


def _prior_window(pname, state):
    """a window without landmarks and IMU factors that holds the prior, its kept blocks at the requested state"""
    pr = priors()[pname]
    rng = np.random.default_rng([20261024, sorted(priors()).index(pname), PRIOR_STATES.index(state)])
    K = 11 if pname == 'old_K11_n75' else 4
    kinds = [k for k, _ in pr['blocks']]
    prob = _empty_window(K)
    prob['estimate_extrinsic'], prob['estimate_td'] = int(B.KIND_EX in kinds), int(B.KIND_TD in kinds)
    for f in range(K):
        prob['pose'][f] = np.concatenate([rng.normal(0, 3, 3), B.qnormalized(rng.normal(0, 1, 4))])
        prob['sb'][f] = rng.normal(0, 0.5, 9)
    first_pose = True
    for (kind, idx), x0 in zip(pr['blocks'], pr['x0']):
        x = np.array(x0, float)
        mag = {'at_x0': 0.0, 'dx1e-3': 1e-3, 'dx0.3': 0.3, 'antipodal': 1e-3, 'rot179': 1e-3}[state]
        if B.GSIZE[kind] == 7:
            if mag:
                x[:3] += mag * _unit(rng)
                angle = mag
                if state == 'rot179' and first_pose:
                    angle = np.radians(179.0)
                x[3:] = B.qnormalized(B.qmul(x[3:], rot_q(_unit(rng), angle)))
            if state == 'antipodal':
                x[3:] = -x[3:]
            first_pose = False
        elif mag:
            x += mag * rng.normal(0, 1, x.shape) * (0.01 if kind == B.KIND_TD else 1.0)
        if kind == B.KIND_POSE:
            prob['pose'][idx] = x
        elif kind == B.KIND_SB:
            prob['sb'][idx] = x
        elif kind == B.KIND_EX:
            prob['ex'] = x
        else:
            prob['td'] = float(x[0])
    prob['prior'] = pr
    return prob


@functools.lru_cache(maxsize=None)
def prior_cases():
    """name -> window"""
    return {f"{p}/{s}": _prior_window(p, s) for p in priors() for s in PRIOR_STATES}


def prior_table(prob, dtype=LD, edit=None):
    st = B.state_of(prob)
    return prior_factor(prob['prior'], [B.get_block(st, k, i) for (k, i) in prob['prior']['blocks']], dtype, edit)


@functools.lru_cache(maxsize=None)
def prior_reference(name):
    return prior_table(prior_cases()[name])


# --------------------------------------------------------------------------------------------------- the yardstick
def e64(name, edit=None):
    """{kind: error} of the float64 restatement (edited or not) on a case: an IMU case, a projection window (the worst of its
    factors) or a prior case"""
    if name in imu_cases():
        ref = imu_reference(name)
        return imu_error(imu_float64(name, edit), ref, imu_is_far(name)) if ref is not None else dict(imu_J=0.0, imu_r=0.0)
    if name in proj_windows():
        out = {}
        for got, ref in zip(proj_table(proj_windows()[name], np.float64, edit), proj_reference(name)):
            for k, v in proj_error(got, ref).items():
                out[k] = max(out.get(k, 0.0), v)
        return out
    return prior_error(prior_table(prior_cases()[name], np.float64, edit)['r'], prior_reference(name), prior_is_x0(name))


def imu_is_far(name):
    return name.endswith('/far_position')


def prior_is_x0(name):
    return name.endswith('/at_x0') and not name.startswith('dyadic')


def case_names():
    return list(imu_cases()) + list(proj_windows()) + list(prior_cases())


@functools.lru_cache(maxsize=None)
def yardstick():
    """E64 per kind and the case that sets it: {kind: (value, case)}"""
    out = {k: (0.0, None) for k in KINDS}
    for name in case_names():
        for k, v in e64(name).items():
            if v > out[k][0]:
                out[k] = (v, name)
    return out


@functools.lru_cache(maxsize=None)
def conditioning():
    """What float64 can lose per kind on this table, in roundings, worked out from the 80-bit reference alone (test_yardstick holds
    every E64 under 4 x 2^-52 x this):
        imu_*          the weighted rows combine the raw rows through |U| |W| (1 on the short records, 1e3 on the 9.9 s one), and the P /
                       V bands subtract positions / velocities larger than what is left of them
        proj_J         products of up to five 3 x 3 matrices whose terms cancel like |p| / z (theta_ic: three skew matrices of a point
                       in the camera frame that cancel to the lever arm |tic|); the largest ratio of a block's terms to the block
        proj_J_lambda  the lambda block's terms over the block (lam_cancel)
        proj_r         |p| / z of the point in camera j, times the three rotations it went through
        prior_r        an n-term sum against the sum of its terms' magnitudes: n
        prior_r_x0     the residue of q0^-1 q0 (2^-53 |q0|^2 per product, two products per component) through sum_k |J0_ik| / |r0_i|"""
    out = dict.fromkeys(KINDS, 0.0)
    for name in imu_cases():
        ref = imu_reference(name)
        if ref is not None:
            for k in (('imu_J_far', 'imu_r_far') if imu_is_far(name) else ('imu_J', 'imu_r')):
                out[k] = max(out[k], ref['cond'])
    for wname, prob in proj_windows().items():
        for ref in proj_reference(wname):
            c = max(1.0, ref['lam_cancel'])
            if ref['lam_cancel'] > LAMBDA_CANCEL:
                out['proj_J_lambda'] = max(out['proj_J_lambda'], c)
            else:
                out['proj_J'] = max(out['proj_J'], c)
            out['proj_r'] = max(out['proj_r'], 3 * ref['p_over_z'])
            out['proj_J'] = max(out['proj_J'], ref['ex_cancel'])
    for name, prob in prior_cases().items():
        pr = prob['prior']
        if prior_is_x0(name):
            live = pr['r0'] != 0                                    # (a cut direction is a zero row of J0 with r0 = 0)
            out['prior_r_x0'] = max(out['prior_r_x0'], float((np.abs(pr['J0'][live]).sum(axis=1) / np.abs(pr['r0'][live])).max()))
        else:
            out['prior_r'] = max(out['prior_r'], float(pr['n']))
    return out
