/* vinsgpu.h — C-ABI of libvinsgpu.so: MI355X (gfx950) implementation of VINS-Mono's two compute
 * hot paths.  Plain C, POD structs, raw pointers, int status codes; no torch / Eigen / OpenCV / ROS
 * types cross this boundary.
 *
 * The reference (HKUST-Aerial-Robotics/VINS-Mono) has no FFI/plugin layer; the seam this ABI
 * replaces is two C++ member functions whose state lives in public members:
 *
 *   BA:  void Estimator::optimization()                 vins_estimator/src/estimator.h:47
 *        (body: estimator.cpp:670-1003; state crossing the seam: estimator.h:65-138)
 *   FE:  void FeatureTracker::readImage(const cv::Mat&, double)   feature_tracker/src/feature_tracker.h:33
 *        (body: feature_tracker.cpp:81-167; state: feature_tracker.h:49-62)
 *
 * Every function returns VG_OK (0) or a negative vg_status.  A handle is bound to the HIP device
 * that was current when it was created and must be used by one host thread at a time.
 * Host-pointer entry points are synchronous on return.  The *_async / *_dev entry points only
 * enqueue work on the handle's stream (or the stream given) — pair them with vg_sync().
 */
#ifndef VINSGPU_H
#define VINSGPU_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define VG_ABI_VERSION 12   /* 2: vg_ba_problem::max_solver_time_s, large-window / all-reduce entry points; 3: vg_ba_summary::gauge_*;
                             * 4: VG_PRIOR_RESIDENT; 5: vg_ba_set_launch_mode; 6: vg_ba_reserve, vg_ba_seq_* (windows that stay on the device);
                             * 7: vg_ba_seq_export / vg_ba_seq_import; 8: vg_host_register, vg_ba_set_fused_min_windows, vg_ba_batch_is_fused;
                             * 9: vg_fe_keep_eig (the min-eigenvalue map is no longer written unless asked for);
                             * 10: vg_config / vg_create_config; vg_ba_batch_is_fused no longer returns 2; 11: vg_fe_read_image;
                             * 12: vg_config::device is 0 = current device / k + 1 = device k, vg_config::imu_info_mode, vg_ba_set_imu_info_mode
                             * (added within 12, nothing existing changed: vg_fe_read_image_batch; vg_fe_camera, vg_fe_set_camera, vg_fe_lift;
                             * vg_fe_tracks_begin / _step / _get / _set; vg_ba_seq_imu_begin / _get / _set / _timing / _times, vg_ba_seq_step_imu_async;
                             * vg_vio_begin / _step_async / _get_frame / _end; vg_init_align; vg_init_sfm; vg_init_relpose; vg_init_exrot;
                             * vg_kf_configure / _add / _get / _set / _match; vg_kf_pnp, vg_kf_pnp_defaults; vg_voc_load, vg_bow_configure / _reset / _count / _get,
                             * vg_kf_loop_detect; vg_pg_optimize, vg_pg_defaults; vg_ba_batch_marg_info; vg_ba_seq_outputs_reserve / _async, vg_ba_seq_get_outputs) */
#define VG_MAX_ITERS 32          /* capacity of the per-iteration trace in vg_ba_summary */

typedef enum {
    VG_OK = 0,
    VG_ERR_BAD_ARG = -1,         /* null pointer, negative size, inconsistent tables          */
    VG_ERR_HIP = -2,             /* a HIP runtime call failed (see vg_last_error)             */
    VG_ERR_UNSUPPORTED = -3,     /* problem does not fit the single-workgroup LDS fast path   */
    VG_ERR_NUMERIC = -4,         /* non-finite state / indefinite reduced system on device    */
    VG_ERR_NO_DEVICE = -5
} vg_status;

typedef struct vg_handle vg_handle;

/* ---- lifecycle ------------------------------------------------------------------------------ */
int vg_abi_version(void);
int vg_create(vg_handle** out);                 /* uses the current HIP device, owns one stream  */
/* The same with everything that shapes a handle's behaviour in ONE struct (ABI 10; SURVEY 8(b): vg_create(const vg_config*, ...)).
 * A handle created this way NEVER consults the environment: the development variables VG_BA_LAUNCH_MODE, VG_BA_FUSED,
 * VG_BA_FUSED_MIN, VG_BA_SOLVE_W8_BELOW and VG_PACK_THREADS are defaults of plain vg_create() only (a drop-in library must not change behaviour with
 * its host's environment).  Zero-initialise, set struct_size = sizeof(vg_config), fill what differs from the defaults. */
typedef struct vg_config {
    int struct_size;             /* sizeof(vg_config) of the caller: fields beyond it take their defaults                         */
    int device;                  /* 0 (or negative) = the CURRENT HIP device; k + 1 = device k (hipSetDevice(k) on the caller's
                                  * thread before the streams are created).  ABI 12: a zero-initialised struct no longer means device 0 */
    int launch_mode;             /* VG_LAUNCH_DIRECT + 1 / VG_LAUNCH_GRAPH + 1; 0 = the library's default (vg_ba_set_launch_mode)   */
    int marg_mode;               /* VG_MARG_SQRT (0, default) / VG_MARG_EIGEN: form of the prior factor (vg_ba_set_marg_mode)     */
    int fused_min_windows;       /* batches from this many windows on take the fused factor kernel; 0 = default (32), -1 = never  */
    int pack_threads;            /* host threads that share the packing / unpacking of a batch; 0 = default (8)                   */
    int imu_info_mode;           /* VG_IMU_INFO_FACTOR (0, default) / VG_IMU_INFO_REFERENCE: form of the IMU sqrt_info (vg_ba_set_imu_info_mode) */
} vg_config;
int vg_create_config(const vg_config* cfg, vg_handle** out);
/* What core clock does this box really run at?  out4 = { ns per dependent FP64 FMA with ONE wavefront on the chip, clock64() ticks per
 * microsecond of wall time during that, the same two with every CU loaded }.  The FMA latency is a constant number of core cycles, so
 * the first and third figures are inversely proportional to the clock (lone / under load).  bench.py reports them (`device.clock_probe`). */
int vg_probe_clocks(vg_handle* h, double* out4);
int vg_destroy(vg_handle* h);
int vg_sync(vg_handle* h);                      /* hipStreamSynchronize(handle stream)           */
const char* vg_last_error(vg_handle* h);        /* text of the last failure on this handle       */
/* ABI 8.  Page-lock a host buffer the caller will hand to the upload entry points again and again (an image ring buffer, a staging
 * area): hipHostRegister / hipHostUnregister.  Uploads from registered memory run at the PCIe rate instead of through the runtime's
 * pageable-copy staging (measured for 256 frames of 752x480: bench.py fe.upload_inclusive).  Optional: every entry point takes
 * pageable memory too. */
int vg_host_register(vg_handle* h, void* p, size_t bytes);
int vg_host_unregister(vg_handle* h, void* p);
void* vg_stream(vg_handle* h);                  /* the handle's hipStream_t (as void*)           */
/* HIP-event stopwatch on the handle's stream (used by bench.py for roofline.achieved) */
int vg_timer_start(vg_handle* h);
int vg_timer_stop(vg_handle* h, float* elapsed_ms);   /* records, synchronises, returns ms      */

/* =============================================================================================
 * BA — Estimator::optimization()  (estimator.cpp:670-1003)
 * ============================================================================================= */

/* IMU pre-integration constants of one frame pair, i.e. the members of IntegrationBase read by
 * IMUFactor::Evaluate (factor/imu_factor.h:19-179, factor/integration_base.h:160-186). */
typedef struct {
    double sum_dt;
    double delta_p[3];
    double delta_q[4];           /* x y z w */
    double delta_v[3];
    double linearized_ba[3];
    double linearized_bg[3];
    double jacobian[225];        /* 15x15 row-major, order [p, theta, v, ba, bg] (parameters.h:48-55) */
    double covariance[225];      /* 15x15 row-major */
    int valid;                   /* 0: no factor for this pair (estimator.cpp:714: sum_dt > 10) */
    int _pad;
} vg_imu_preint;

/* Batched IMU pre-integration — replaces IntegrationBase::push_back / propagate / midPointIntegration and, with new
 * linearisation biases, IntegrationBase::repropagate (factor/integration_base.h:30-158), as driven by
 * Estimator::processIMU (estimator.cpp:93-101) and the bias-change re-propagation of estimator.cpp:600-609.
 * Interval k integrates the samples [sample_off[k], sample_off[k+1]) — rows (dt, acc_x, acc_y, acc_z, gyr_x, gyr_y,
 * gyr_z) of `samples` — starting from the measurement first[k] = (acc_0, gyr_0) (IntegrationBase ctor,
 * integration_base.h:15-27) with the biases bias[k] = (linearized_ba, linearized_bg); noise = (ACC_N, GYR_N, ACC_W,
 * GYR_W) of the estimator configuration.  out[k].valid is set to 1 (the sum_dt > 10 s rule of estimator.cpp:714 is
 * applied where the factor is used).  SURVEY.md 8(f) row 2. */
int vg_imu_preintegrate(vg_handle* h, int n_intervals, const int* sample_off, const double* samples, const double* first,
                        const double* bias, const double* noise, vg_imu_preint* out);

/* FeatureManager::triangulate (feature_manager.cpp:202-257) for L landmarks whose depth is
 * not yet known (the used_num >= 2 && start_frame < WINDOW_SIZE - 2 && estimated_depth <= 0 filter of :206-211 is the
 * caller's).  Ps [K x 3], Rs [K x 9 row-major] = body poses of the window, tic / ric = camera extrinsics; landmark l is
 * observed in frames start[l] .. start[l] + nobs[l] - 1 with feature_per_frame.point = points[obs_off[l] + j] (x y z).
 * depth[l] = svd_V[2] / svd_V[3] of the 2n x 4 DLT system, or init_depth (INIT_DEPTH) when that is < 0.1 (:245-254). */
int vg_triangulate(vg_handle* h, int K, const double* Ps, const double* Rs, const double* tic, const double* ric, int L,
                   const int* start, const int* nobs, const int* obs_off, const double* points, double init_depth, double* depth);

/* ---- Initialisation: visual-inertial alignment, batched (added within ABI 12, nothing existing changed) -----------------------------
 * VisualIMUAlignment (initial/initial_aligment.cpp:3-207: solveGyroscopeBias, LinearAlignment, RefineGravity) and the state change of
 * Estimator::visualInitialAlign that follows it (estimator.cpp:376-435) for n_windows independent windows in one synchronous call: one
 * upload, one kernel (one workgroup per window, FP64), one download.  A window is one all_image_frame map: F ImageFrames in stamp order
 * with their SfM poses and the raw IMU rows between them; the F - 1 records are integrated on the device through the per-sample body
 * of vg_imu_preintegrate, first with (ba0, bg0), then again with (0, bg0 + delta_bg).
 *
 * The reference is followed, quirks included:
 *   - the re-propagation passes a ZERO accelerometer bias (repropagate(Vector3d::Zero(), Bgs[0]), :35), whatever ba0 was;
 *   - A and b of LinearAlignment are multiplied by 1000, the scale column holds (T_j - T_i) / 100, so s = x[n - 1] / 100;
 *     it fails (VG_ALIGN_FAILED_LINEAR) when | |g| - g_norm | > 1 or s < 0; nothing after it is computed then, g_lin / s_lin are returned;
 *   - RefineGravity clears its A and b ONCE before its four passes, not per pass, and multiplies them by 1000 at the end of every pass:
 *     pass k solves the sum of the passes so far, the older ones weighted 1000^(k - j);
 *   - TangentBasis compares the normalised gravity with (0, 0, 1) exactly; g0 <- normalised(g0 + lxly dg) g_norm after every pass;
 *     s = x[n - 1] / 100 afterwards, s < 0 gives VG_ALIGN_FAILED_REFINE;
 *   - Vs[k] = R[key[k]] * x.segment<3>(3 k): the reference indexes x by the KEY-FRAME counter kv, not by the frame's position in
 *     all_image_frame (estimator.cpp:406-415); with non-key frames in front of a key frame that is another frame's velocity.
 * Deviations:
 *   - the solves are an unpivoted LDL^T where the reference calls Eigen's pivoted ldlt() (the systems are symmetric positive
 *     semi-definite); a pivot that is not a positive finite number gives VG_ALIGN_NUMERIC for that window only, as does F < 4
 *     (6 (F - 1) rows for 3 F + 4 unknowns: singular by count; delta_bg, bg and the records are still returned);
 *   - R0 = g2R(g) uses Quaterniond::FromTwoVectors in its regular branch; when g is so close to -z that Eigen would take its SVD
 *     branch (1 + g.z / |g| < 1e-12) the window gets VG_ALIGN_NUMERIC.
 * Window stage (n_key > 0 and status OK): Rs[k] = R[key[k]], Ps[k] = s T[key[k]] - Rs[k] tic - (s T[key[0]] - Rs[0] tic), Vs as
 * above; R0 = g2R(g) with the yaw of R0 Rs[0] removed; g_w = R0 g; Ps, Rs, Vs <- R0 ...  Clearing the depths, triangulate with a
 * zero tic and estimated_depth *= s (:386-397, :416-422) stay the caller's: vg_triangulate and one multiplication.
 * Refused with VG_ERR_BAD_ARG before anything is uploaded (vg_last_error says which; no output is touched, the handle stays usable):
 * a wrong struct_size, F outside 2 .. VG_ALIGN_MAX_FRAMES, a NULL table, sample_off not ascending or an empty interval, a key list
 * that does not ascend or leaves [0, F), n_key of 1 or above F, a non-finite input.  An interval longer than vg_imu_preintegrate's
 * practice is integrated like there.  What is not computed for a window's status is returned as zeros. */
enum { VG_ALIGN_OK = 0, VG_ALIGN_FAILED_LINEAR = 1, VG_ALIGN_FAILED_REFINE = 2, VG_ALIGN_NUMERIC = 3 };
#define VG_ALIGN_MAX_FRAMES 32

typedef struct {                 /* one window = one all_image_frame map */
    size_t struct_size;          /* sizeof(vg_align_in) */
    int n_frames;                /* F, 2 .. VG_ALIGN_MAX_FRAMES: ImageFrame entries in stamp order */
    const double* R;             /* [F][9] row-major, ImageFrame::R (body rotation in the SfM frame c0) */
    const double* T;             /* [F][3] ImageFrame::T (camera position in c0, unscaled) */
    const int* sample_off;       /* [F] interval k (frame k -> k + 1) integrates rows [sample_off[k], sample_off[k + 1]) */
    const double* samples;       /* rows dt acc gyr, as vg_imu_preintegrate */
    const double* first;         /* [F - 1][6] acc_0 gyr_0 of every interval */
    double ba0[3], bg0[3];       /* biases the records are FIRST integrated with (Bas / Bgs during initialisation) */
    double noise[4];             /* ACC_N GYR_N ACC_W GYR_W */
    double tic[3];               /* TIC[0] */
    double g_norm;               /* G.norm() */
    int n_key;                   /* K, 0 or 2 .. F: frames of the window (Headers[0 .. frame_count]) */
    const int* key;              /* [K] ascending indices into the F frames */
} vg_align_in;

typedef struct {
    size_t struct_size;          /* sizeof(vg_align_out), set by the caller */
    int status;                  /* VG_ALIGN_* */
    double delta_bg[3], bg[3];   /* solveGyroscopeBias; bg = bg0 + delta_bg */
    double g_lin[3], s_lin;      /* LinearAlignment before RefineGravity (s already / 100) */
    double g_c0[3], s;           /* after RefineGravity (the status is OK or FAILED_REFINE) */
    double* v_body;              /* [F][3] x.segment<3>(3 i) after RefineGravity, or NULL */
    vg_imu_preint* records;      /* [F - 1] the records re-propagated with (0, bg), or NULL */
    double *Ps, *Rs, *Vs;        /* [K][3] [K][9] [K][3] the window after estimator.cpp:376-435, or NULL when n_key == 0 */
    double g_w[3], R0[9];        /* g = R0 g, rot_diff */
} vg_align_out;

int vg_init_align(vg_handle* h, int n_windows, const vg_align_in* in, vg_align_out* out);

/* ---- Initialisation: global SfM and the per-frame PnP, batched (added within ABI 12, nothing existing changed) -------------------------
 * The part of Estimator::initialStructure between relativePose() and visualInitialAlign() (estimator.cpp:250-353, initial/initial_sfm.cpp,
 * ReprojectionError3D of initial/initial_sfm.h:25-54) for n_windows independent windows in one synchronous call: one upload, two launches
 * (one workgroup per window: GlobalSFM::construct with its full BA; then one workgroup per non-key frame: its PnP), one download, FP64.
 * R_all / T_all are ImageFrame::R / T, the inputs of vg_align_in::R / T.  l, relative_R, relative_T are inputs: relativePose / solveRelativeRT
 * is vg_init_relpose (below), whose outputs they are; ric may be what vg_init_exrot (below) calibrated.  The IMU-excitation check of
 * :222-248 (which has no effect in the reference) is NOT part of either call.
 *
 * construct, statement by statement:
 *   - q[l] = identity, T[l] = 0, q[F-1] = q[l] * Quaterniond(relative_R) (Eigen's matrix-to-quaternion conversion), T[F-1] = relative_T;
 *     c_Quat = q.inverse() (conjugate over squared norm), c_Rotation = toRotationMatrix, c_Translation = -(c_Rotation T);
 *   - stages 1 to 5 in the reference's order (:158-217): for i = l .. F-2: (i > l: PnP of i from the pose of i-1) then
 *     triangulateTwoFrames(i, F-1); for i = l+1 .. F-2: triangulateTwoFrames(l, i); for i = l-1 .. 0: PnP of i from i+1, then
 *     triangulateTwoFrames(i, l); last, every feature still without a position and with two observations or more from its first and its
 *     LAST observation.  triangulateTwoFrames touches only features whose state is false and makes no depth or cheirality test.  A feature
 *     with one observation is never triangulated: it stays out of the BA and out of sfm_tracked_points (state 0);
 *   - triangulatePoint: the right singular vector of the 4x4 design matrix for the smallest singular value (one-sided Jacobi SVD, as
 *     vg_triangulate), divided by its last component;
 *   - solveFrameByPnP: the points are the features with state 1 seen in the frame, in feature order; fewer than 10 give
 *     VG_SFM_FAILED_PNP (:45-50).  The 2-D and 3-D inputs are ROUNDED TO FLOAT32 (cv::Point2f / Point3f) and then used in double.
 * cv::solvePnP(..., useExtrinsicGuess = 1, SOLVEPNP_ITERATIVE) is third-party and unpinned; this is its definition here (OpenCV 3.3.1's
 * guess branch of cvFindExtrinsicCameraParams2, restated): CvLevMarq over (rvec, t), at most 20 iterations; lambda = 10^k, k starting
 * at -3; normal equations JtJ, JtErr over all points with the diagonal of JtJ multiplied by 1 + lambda; param = prevParam - solution; when
 * the error norm grew: k + 1 and, while k <= 16, a re-solve from the same JtJ (counted in pnp_up); else, and past the cap, the step is
 * kept and k - 1 (floor -16); stop when |param - prevParam| / (|prevParam| + DBL_EPSILON) < FLT_EPSILON; the residual is projected minus
 * observed with K = I and no distortion, the Jacobian the exact derivative through Rodrigues; the result is always "success".
 * The full BA is Ceres' TrustRegionMinimizer with the LEVENBERG_MARQUARDT strategy at the defaults the reference leaves in place: at most
 * 50 iterations (accepted, rejected and invalid ones counted); gradient tolerance 1e-10 on the max-norm of the unscaled gradient in the
 * tangent space, checked at the start and after every accepted step; parameter tolerance |dx| <= 1e-8 (|x| + 1e-8) and function tolerance
 * |cost - candidate| <= 1e-6 cost, checked in this order BEFORE the step is judged (the point stays where it was, as in the dogleg
 * restatement of vg_ba_optimize); radius 1e4 at first, at most 1e16, below 1e-32 after a rejected step ends with CONVERGENCE; a step is
 * accepted when (cost - candidate) / model change > 1e-3 (monotonic); LM diagonal D = sqrt(clamp(diag(JtJ), 1e-6, 1e32) / radius) of the
 * Jacobi-scaled Jacobian (scale 1 / (1 + column norm) from the FIRST Jacobian), D * D added to the diagonal; radius / max(1/3, 1 - (2 rho -
 * 1)^3) on success; / decrease_factor (2 at first and after every success, doubling) on a rejected or invalid step; 5 invalid steps in a
 * row (a point block or the reduced system not positive definite, a model change that is not positive) end with FAILURE.  Blocks: a
 * 4-parameter quaternion (w x y z) with QuaternionParameterization (Plus = [cos|d|, sin|d| / |d| d] * q), a translation per frame, 3 per
 * triangulated feature; constant: the rotation of l, the translations of l and F-1 (x and |x| leave them out).  One ReprojectionError3D
 * per observation of every triangulated feature; QuaternionRotatePoint normalises the quaternion inside the cost, the Jacobian is what
 * auto-diff gives times the 4x3 plus-Jacobian.  The points are eliminated first (DENSE_SCHUR), the reduced camera system (6 F - 9) by
 * Cholesky.  VG_SFM_FAILED_BA: not CONVERGENCE and final_cost >= 5e-3 (:281-289).  Afterwards q[i] = inverse(), T[i] = -(q[i] * c_t).
 * Frames: a key entry gets R = Q[i] ric^T, T = T[i]; a non-key entry starts from Q[g]^-1, -R T[g] (g = all_guess), takes the ids of its
 * map found among the features with state 1, in the map's order (fewer than 6: VG_SFM_FAILED_FRAME, :333), and gets R = R_pnp^T ric^T,
 * T = -R_pnp^T t.
 * Deviations:
 *   - max_solver_time_in_seconds = 0.2 is NOT enforced (as SOLVER_TIME for vg_ba_optimize: a wall-clock cap is not reproducible);
 *   - a triangulated coordinate that is not finite (division by w = 0) gives VG_SFM_NUMERIC where the reference goes on with it;
 *   - Rodrigues in both directions is the regular branch (theta < DBL_EPSILON included), without OpenCV's SVD re-orthogonalisation of the
 *     matrix; the near-pi branch (sin part below 1e-5 with a trace part that is not positive) gives VG_SFM_NUMERIC;
 *   - the 6x6 solve of a PnP step is an unpivoted LDL^T where OpenCV takes an SVD solve: a pivot that is not positive and finite, or an
 *     error norm that is not finite, gives VG_SFM_NUMERIC;
 *   - every non-key entry is solved on its own: an entry behind a failed one is still returned; the status is that of the FIRST failed
 *     entry in stamp order (the reference returns at it).
 * What a status leaves uncomputed comes back as zeros: FAILED_PNP / NUMERIC inside construct return pnp_iters / pnp_up of the frames done
 * and nothing else; FAILED_BA returns the taps, state[] and the BA trace; FAILED_FRAME / NUMERIC of a frame return everything but that
 * entry's R_all / T_all.  A window's status never touches its neighbours; a batch equals the single calls bit for bit.
 * Refused with VG_ERR_BAD_ARG before anything is uploaded (vg_last_error names the cause; no output is touched, the handle stays usable): a
 * wrong struct_size, F outside 3 .. VG_SFM_MAX_FRAMES, l outside [0, F-2], n_feat outside 1 .. VG_SFM_MAX_FEATURES, a NULL table, start +
 * nobs > F or nobs < 1, obs_off not ascending (rows that overlap), duplicate feature_id, all_key not ascending over its non-negative
 * entries or not covering 0 .. F-1 exactly once when n_all > 0, all_guess outside [0, F), all_off not ascending, a non-finite input. */
enum { VG_SFM_OK = 0, VG_SFM_FAILED_PNP = 1, VG_SFM_FAILED_BA = 2, VG_SFM_FAILED_FRAME = 3, VG_SFM_NUMERIC = 4 };
#define VG_SFM_MAX_FRAMES 16     /* the reduced camera system of 6 F - 9 unknowns sits in LDS beside the per-feature blocks */
#define VG_SFM_MAX_FEATURES 1024 /* 15 doubles of LDS per feature: csrc/init_sfm_carve.h */
#define VG_SFM_MAX_ITERS 50      /* Ceres' max_num_iterations default */

typedef struct {                 /* one window: f_manager.feature and all_image_frame at the time of initialStructure() */
    size_t struct_size;          /* sizeof(vg_sfm_in) */
    int n_frames;                /* F = frame_count + 1, 3 .. VG_SFM_MAX_FRAMES (the reference runs 11) */
    int l;                       /* the reference frame relativePose() chose, 0 .. F-2 */
    double relative_R[9];        /* row-major */
    double relative_T[3];
    double ric[9];               /* RIC[0], row-major */
    int n_feat;                  /* 1 .. VG_SFM_MAX_FEATURES */
    const int* feature_id;       /* [n_feat] distinct */
    const int* start;            /* [n_feat] the layout of vg_triangulate: feature j is seen in frames start[j] .. start[j] + nobs[j] - 1 */
    const int* nobs;
    const int* obs_off;          /* [n_feat] ascending: the feature's first row of points */
    const double* points;        /* x y z rows (feature_per_frame.point; x and y are used) */
    int n_all;                   /* entries of all_image_frame in stamp order; 0: construct only */
    const int* all_key;          /* [n_all] the index i of the key frame (Headers[i]) this entry IS, or -1 */
    const int* all_guess;        /* [n_all] for a non-key entry: the i whose pose is its guess (the walk of estimator.cpp:290-306) */
    const int* all_off;          /* [n_all + 1] a non-key entry's map is rows all_off[a] .. all_off[a + 1] - 1 of all_id / all_xy */
    const int* all_id;           /* feature ids, ascending inside an entry (the order of the frame's points map) */
    const double* all_xy;        /* x y of camera 0 */
} vg_sfm_in;

typedef struct {                 /* every pointer may be NULL */
    size_t struct_size;          /* sizeof(vg_sfm_out), set by the caller */
    int status;                  /* VG_SFM_* */
    double* q;                   /* [F][4] (w x y z) Q after construct */
    double* T;                   /* [F][3] */
    int* state;                  /* [n_feat] sfm_f[j].state: the set bits are sfm_tracked_points */
    double* position;            /* [n_feat][3] sfm_f[j].position after the BA (zeros where state is 0) */
    double* R_all;               /* [n_all][9] ImageFrame::R */
    double* T_all;               /* [n_all][3] ImageFrame::T */
    int* is_key;                 /* [n_all] ImageFrame::is_key_frame */
    /* taps for the tests */
    double *q0, *T0;             /* [F][4] [F][3] c_Quat, c_Translation right before the full BA */
    double* position0;           /* [n_feat][3] the triangulated positions right before the full BA */
    int *pnp_iters, *pnp_up;     /* [F] iterations, and lambda increases, of each chain PnP (0 for l and F-1) */
    int ba_iters, ba_termination;/* VG_TERM_* */
    double final_cost;
    double it_cost[VG_SFM_MAX_ITERS], it_cost_cand[VG_SFM_MAX_ITERS], it_model[VG_SFM_MAX_ITERS], it_radius[VG_SFM_MAX_ITERS];
    int it_flags[VG_SFM_MAX_ITERS];      /* the trace of vg_ba_summary: bit0 valid, bit1 accepted */
    double* device_ms;           /* read on out[0] only: [2] device time of the two launches from events, or NULL (no events) */
} vg_sfm_out;

int vg_init_sfm(vg_handle* h, int n_windows, const vg_sfm_in* in, vg_sfm_out* out);

/* ---- Initialisation: relativePose (RANSAC + recoverPose), batched (added within ABI 12, nothing existing changed) ----------------------
 * Estimator::relativePose (estimator.cpp:442-471) for n_windows independent windows in one synchronous call: FeatureManager::
 * getCorresponding (feature_manager.cpp:120), the parallax gate, MotionEstimator::solveRelativeRT (initial/solve_5pts.cpp:193-227) with the
 * file's own recoverPose / decomposeEssentialMat (:4-190), over the candidate frames i = 0 .. F-2 against frame F-1.  The outputs l,
 * relative_R, relative_T are the inputs of vg_sfm_in under the same names and layout, and the feature tables are those of vg_sfm_in: one
 * packing serves both calls.  One upload, nine launches, one download on the ordinary path (a second small submission when a candidate
 * needs the exact sample schedule, see 4).
 *
 * Statement by statement, quirks kept:
 *   1. Correspondences.  Candidate i gets the features with start <= i and start + nobs - 1 >= F-1, in feature order, as pairs (point at
 *      i, point at F-1); x and y of the rows are used.
 *   2. Gate.  It passes when n_corres > min_corres (20) and average_parallax * focal (460) > parallax_gate (30), both strict.  The
 *      parallax of a pair is sqrt(dx dx + dy dy) on the DOUBLE x, y; average_parallax = sum / n_corres.  The sum runs in ONE FIXED ORDER,
 *      which is not the reference's left-to-right one: with d[k] the parallax of pair k, s[t] = d[t] + d[t + 256] + d[t + 512] + ...
 *      (ascending, t = 0 .. 255, missing terms are +0), then seven halving steps s[t] += s[t + h], h = 128, 64, .. 1; the sum is s[0].
 *      Any order of these positive terms lies within n_corres 2^-53 relative of any other.
 *   3. Rounding.  ll, rr are the pairs rounded to float32 (cv::Point2f); everything after the gate uses them, widened to double.
 *   4. RANSAC.  cv::findFundamentalMat(ll, rr, FM_RANSAC, ransac_threshold (0.3 / 460), 0.99, mask) is this library's deterministic
 *      RANSAC of vg_fe_reject_with_f (oracle/ASSUMPTIONS.md F9) at this threshold: the sample schedule of cv::RNG((uint64)-1), run7Point
 *      on the raw points, the models of a sample ranked best first, the float error against threshold^2, a model replacing the best one
 *      when it has more inliers than max(best, 6), the bound RANSACUpdateNumIters(0.99, ...) after every improvement.  The model goes out
 *      unchanged (OpenCV 3.3's registrator does not refit) and is used as E: the points are normalised.  The device runs the schedule as
 *      far as it depends on n alone; a candidate in whose schedule a sample would have been REDRAWN by OpenCV (its last point collinear
 *      with two earlier ones) is repeated with the exact schedule, made on the host, through the same kernels; its results are those of
 *      the exact schedule and used_fallback is 1.  min_corres >= 14, so a gated candidate always has the 15 points of the RANSAC branch.
 *   5. decomposeEssentialMat.  The SVD of the 3x3 matrix here is a one-sided Jacobi on its columns (pairs (0,1), (0,2), (1,2) in turn,
 *      a pair is rotated while |a.b| > 1e-15 |a||b|; at most 40 sweeps; only rotations between two columns above 1e-13 of the Frobenius
 *      norm keep the sweeps going).  Singular values: the column norms, descending (stable).  Vt: the accumulated rotations in that
 *      order, negated when its determinant is negative.  U: u0, u1 the first two columns over their norms, u2 = u0 x u1 (so det U = +1;
 *      the third column of a matrix of rank 2 is rounding noise and is not used).  R1 = U W Vt, R2 = U Wt Vt, t = u2.  The set
 *      {R1, R2} x {t, -t} does not depend on this convention; the ORDER does, and with it the >= tie-break of :152-181 -- a LAPACK SVD
 *      may name R1 what is R2 here.
 *   6. Four triangulations, (R1, t), (R2, t), (R1, -t), (R2, -t) against P0 = [I|0].  cv::triangulatePoints is third-party and unpinned.
 *      RECALLED for OpenCV 3.3.1, NOT PINNED: per point a 6x4 design matrix, three rows per view (x P[2] - P[0], y P[2] - P[1],
 *      x P[1] - y P[0]), and the right singular vector of the smallest singular value -- here by the one-sided Jacobi of vg_triangulate
 *      (threshold 1e-16, at most 40 sweeps) on the four columns.  (Later OpenCV releases build a 4x4 matrix from two rows per view; the
 *      null vector of exact data is the same, of noisy data it is not.)  Masks in exactly the order of :80-88: Q.z Q.w > 0; Q divided by
 *      Q.w; z < dist (50); z' = (P Q).z summed left to right; z' > 0; z' < dist.  ANDed with the RANSAC mask.  The winner by the chain
 *      good1 >= the others, else good2 >= the others, else good3, else the fourth.  relative_R = R^T, relative_T = -(R^T t) of the
 *      winner; success is inlier_cnt > min_inliers (12).
 *   7. Pick.  l is the first i in ascending order whose gate passes and whose solveRelativeRT succeeds.
 * Deviations:
 *   - the candidates are evaluated in parallel; every gated one is computed whatever an earlier one returned, so the taps are the same
 *     from run to run and do not depend on l;
 *   - a triangulated value that is not finite (Q.w = 0) fails every comparison it enters, as cv::compare has it: the point counts for no
 *     candidate;
 *   - a RANSAC that finds no model (no sample with more than 6 inliers) makes the candidate fail with zero taps, where the reference
 *     hands an empty matrix to recoverPose and aborts;
 *   - a 3x3 SVD that does not converge inside the sweep cap makes the candidate numeric; when the walk of 7 meets such a candidate before
 *     a success the window ends with VG_RELPOSE_NUMERIC (l = -1).  That window only: its neighbours are untouched.
 * Taps of a candidate that is not gated are zero.  ransac_iter is the iteration the bookkeeping ended on, the last one its loop looked at (the larger of the
 * winning iteration and bound - 1; -1: the schedule was empty), ransac_bound the bound it ended with, ransac_best the iteration whose model
 * won (-1: none).  A batch equals the single calls bit for bit.
 * Refused with VG_ERR_BAD_ARG before anything is uploaded (vg_last_error names the cause; no output is touched, the handle stays usable): a
 * wrong struct_size, F outside 3 .. VG_SFM_MAX_FRAMES, n_feat outside 1 .. VG_SFM_MAX_FEATURES, a NULL table, start + nobs > F or nobs <
 * 1, obs_off not ascending, a non-finite input, a threshold, gate, focal or distance that is not positive, min_corres < 14 or min_inliers <
 * 0, a confidence other than 0.99 (the bound table is built for it), more than VG_RELPOSE_MAX_STREAMS candidates in one call.
 * NOT part of it: re-initialisation inside vg_vio_*, a drop-in against the reference's headers.  (InitialEXRotation::
 * CalibrationExRotation, which keeps state across frames and uses another findFundamentalMat mode, is vg_init_exrot below.) */
enum { VG_RELPOSE_OK = 0, VG_RELPOSE_NONE = 1, VG_RELPOSE_NUMERIC = 2 };
#define VG_RELPOSE_LAUNCHES 9         /* gather | RANSAC part 1: samples, counts, bookkeeping | part 2: the same | pose | pick */
#define VG_RELPOSE_MAX_STREAMS 4096   /* (window, candidate) pairs of one call: each holds the models of 1000 iterations on the device */

typedef struct {
    size_t struct_size;          /* sizeof(vg_relpose_in) */
    int n_frames;                /* F = frame_count + 1, 3 .. VG_SFM_MAX_FRAMES */
    int n_feat;                  /* 1 .. VG_SFM_MAX_FEATURES */
    const int* start;            /* [n_feat] the tables of vg_sfm_in */
    const int* nobs;
    const int* obs_off;
    const double* points;        /* x y z rows; x and y are used */
    /* what the reference hard-codes; its values are the defaults a caller should set */
    double ransac_threshold;     /* 0.3 / 460 */
    double confidence;           /* 0.99 (nothing else is accepted) */
    int min_corres;              /* 20 */
    int min_inliers;             /* 12 */
    double parallax_gate;        /* 30 */
    double focal;                /* 460 */
    double cheirality_dist;      /* 50 */
} vg_relpose_in;

typedef struct {                 /* every pointer may be NULL */
    size_t struct_size;          /* sizeof(vg_relpose_out), set by the caller */
    int status;                  /* VG_RELPOSE_* */
    int l;                       /* -1 when none */
    double relative_R[9];        /* row-major; zeros when none */
    double relative_T[3];
    int n_mask;                  /* n_corres of l */
    unsigned char* mask;         /* [n_feat] the first n_mask: the final mask (RANSAC and cheirality) over the correspondences of l */
    unsigned char* ransac_mask;  /* [n_feat] the first n_mask: the mask findFundamentalMat returned for l (a tap) */
    /* taps per candidate, [F-1] each */
    int* n_corres;
    double* avg_parallax;
    int* gate;
    int *ransac_iter, *ransac_bound, *ransac_inliers, *ransac_best;
    double* F;                   /* [F-1][9] */
    int* good;                   /* [F-1][4] */
    int *winner, *inlier_cnt, *used_fallback;
    double* device_ms;           /* read on out[0] only: [VG_RELPOSE_LAUNCHES] device time per launch from events, or NULL.  The second
                                  * submission of the candidates that need the exact schedule (used_fallback) is NOT in these figures */
} vg_relpose_out;

int vg_init_relpose(vg_handle* h, int n_windows, const vg_relpose_in* in, vg_relpose_out* out);

/* ---- Initialisation: extrinsic-rotation calibration, batched (added within ABI 12, nothing existing changed) ---------------------------
 * InitialEXRotation::CalibrationExRotation (initial/initial_ex_rotation.cpp, the whole file) for n_windows independent windows in one
 * synchronous call; every window gets a run of S = n_steps consecutive calls of the reference's member.  Step k (k = 1 .. S) is the call
 * with frame_count = n_prev + k.  One upload, nine launches, one download on the ordinary path; a step in the LMedS range costs one small
 * estimate of its own before the upload, a step that needs the exact sample schedule a second small submission (see 3, 4).  With it every
 * stage of vins_estimator/src/initial/ has its call: a caller with estimate_extrinsic: 2 feeds calib_ric to vg_sfm_in::ric / vg_align_in.
 *
 * Statement by statement, quirks kept:
 *   1. solveRelativeR, small inputs.  Fewer than min_points (9) correspondences give Rc = identity (branch 0); F and the other taps are 0.
 *   2. Rounding.  ll, rr are the pairs rounded to float32 (cv::Point2f); everything after uses them, widened to double.
 *   3. Fundamental matrix, 15 points or more (branch 2): cv::findFundamentalMat(ll, rr) is FM_RANSAC at threshold 3.0, confidence 0.99 --
 *      this library's deterministic RANSAC exactly as in vg_init_relpose item 4: the cv::RNG((uint64)-1) schedule, run7Point on the raw
 *      points, the float error against threshold squared, no refit, and the second submission with the exact schedule (used_fallback)
 *      for a step whose n-only schedule holds a redrawn sample.  CONSEQUENCE, kept: the points are normalised coordinates, so at 3.0
 *      almost every point is an inlier of almost any model; the bookkeeping usually ends at iteration 0 with bound 0 and the matrix is
 *      that of the FIRST sample, and where that sample's cubic has several real roots every root's model takes all points and the tie
 *      may go to a spurious one, whose Rc is degrees off (about every second step of a rendered window).  That is the reference's
 *      behaviour.  ransac_threshold is a field: in the units of the points (solveRelativeRT passes 0.3 / 460) the RANSAC separates them.
 *   4. Fundamental matrix, 9 to 14 points (branch 1): OpenCV switches to LMedS.  It is the front end's LMedS (vg_fe_reject_with_f, csrc/
 *      fe_ransac.hip, oracle/ASSUMPTIONS.md F9) run on the step's float32 points at this threshold, through that call's kernels, before the
 *      upload, as the front end's fall-back streams run; ransac_* are 0 for it.  These estimates are NOT batched: one synchronous round trip
 *      per such step, 0.2 ms each on an MI355X (profiles/init_exrot.json), outside device_ms.
 *   5. decomposeE.  The SVD is vg_init_relpose item 5 (rp_decompose): R1 = U W Vt, R2 = U Wt Vt, t1 = u2, t2 = -u2.  det U = det Vt = +1
 *      by construction, so det R1 = +1 and the E = -E branch of :83-87 is never taken; the set {R1, R2} x {t, -t} does not depend on
 *      this.  The ORDER does depend on the convention, and with it the strict ratio1 > ratio2 of :90.
 *   6. testTriangulation, in the order (R1,t1) (R1,t2) (R2,t1) (R2,t2) (front[4]).  P1 is a Matx34f: R and t are rounded to float32 and
 *      widened.  cv::triangulatePoints is the 6x4 form of vg_init_relpose item 6 with the same Jacobi, in double, on the widened P1 and
 *      points (RECALLED, NOT PINNED).  Its result is stored as float32: q = float32(Q).  RECALLED for OpenCV 3.3.1, NOT PINNED, and exactly
 *      what the kernel does: col / normal_factor is a float32 scaling, inv = float32(1.0 / double(q.w)), a = q * inv in float32 (four
 *      products); each of the two products P a is one row, z = float32(P[2][0] a.x + P[2][1] a.y + P[2][2] a.z + P[2][3] a.w) summed
 *      left to right in double over the widened float32 operands (the products are exact) and rounded once.  front counts the points
 *      with z_l > 0 and z_r > 0; a comparison with a non-finite value is false.  ratio = front / n in double.  The result is R1 when
 *      max(ratio(R1,t1), ratio(R1,t2)) > max(ratio(R2,t1), ratio(R2,t2)), else R2 (picked 1 or 2; the double R, not its float32
 *      rounding), and it goes out TRANSPOSED (:93-95): that is Rc of the step.
 *   7. CalibrationExRotation.  Rimu = delta_q.toRotationMatrix() (not normalised, as Eigen).  Rc_g = (ric^-1 Rimu) ric, products left to
 *      right, ric^-1 Eigen's 3x3 cofactor inverse (cofactors times 1 / det, det = (c00 m00 + c10 m10) + c20 m20), not a transpose.
 *      Quaterniond(Matrix3d) is the conversion restated for vg_init_sfm.  angularDistance in Eigen 3.3's form, 2 atan2(|vec(d)|, |w(d)|)
 *      with d = r1 * conj(r2) (UNPINNED: Eigen 3.2 takes 2 acos); in degrees by (180 / M_PI) *.  The Huber weight is huber_deg / angle
 *      above huber_deg (5) degrees, else 1.  L and R exactly as :32-47, the vector part first and w last; the block of record i is
 *      huber (L - R) entry by entry, and A is 4 (n_prev + k) x 4.  A record's block depends on the record alone.
 *      JacobiSVD is third-party; here it is a one-sided Jacobi on the four columns of A itself, not on A^T A: the pairs (0,1) (0,2) (0,3)
 *      (1,2) (1,3) (2,3) in turn; al = |a_p|^2, be = |a_q|^2, ga = a_p . a_q, each the sum over a record's four rows in ascending order
 *      from 0, then over the 64 record slots (absent ones are 0) by six butterfly steps s += s[slot ^ h], h = 32 .. 1; the pair is rotated
 *      when |ga| > 1e-16 sqrt(al be) and ga != 0, with zeta = (be - al) / (2 ga), t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)), c = 1 /
 *      sqrt(1 + t^2), s = c t; the sweeps go on while a sweep met a pair with |ga| > 1e-13 sqrt(al be) between two columns above 1e-26 of
 *      the squared Frobenius norm; at most 40 sweeps.  Singular values: the column norms, sorted descending (sigma); x is the column of V
 *      of the smallest.  Quaterniond(x) reads x as (x y z w); ric = toRotationMatrix(x)^-1, the cofactor inverse again, no normalisation.
 *      ok = (n_prev + k >= min_frames (10)) && sigma[2] > cov_threshold (0.25), strict: the test is on the THIRD singular value, the
 *      result is the vector of the FOURTH.
 * Deviations:
 *   - every step is computed even after a success, where the reference's caller stops calling: first_ok = n_prev + k of the first step
 *     with ok (-1: none) tells where it stopped, calib_ric is ric of that step (zeros when none);
 *   - a 3x3 or 4N x 4 Jacobi that does not end inside its cap, or a RANSAC / LMedS that finds no model (the reference aborts inside
 *     OpenCV on the empty matrix; here the step's Rc is the identity), gives VG_EXROT_NUMERIC for that window only, with first_ok -1;
 *   - a batch equals the single calls bit for bit; a run split at any step and resumed with prev = the earlier records (carried and
 *     returned, in order) and ric_prev = ric of the last step equals the unsplit run bit for bit.
 * Refused with VG_ERR_BAD_ARG before anything is uploaded (vg_last_error names the cause; no output is touched, the handle stays usable): a
 * wrong struct_size, n_steps < 1, n_prev < 0, n_prev + n_steps above VG_EXROT_MAX_STEPS, a NULL table, corr_off not ascending, a step over
 * VG_SFM_MAX_FEATURES pairs, a non-finite input, a delta_q of zero norm, a threshold, huber_deg or cov_threshold that is not positive, a
 * confidence other than 0.99, min_points < 9, more than VG_RELPOSE_MAX_STREAMS (window, step) pairs in one call (they use its scratch).
 * NOT part of it: a drop-in against the reference's headers. */
enum { VG_EXROT_OK = 0, VG_EXROT_NUMERIC = 1 };
#define VG_EXROT_LAUNCHES 9           /* gather | RANSAC part 1: samples, counts, bookkeeping | part 2: the same | rotation | calibration */
#define VG_EXROT_MAX_STEPS 64         /* n_prev + n_steps: one record per lane of the calibration stage's wavefront */

typedef struct {
    size_t struct_size;          /* sizeof(vg_exrot_in) */
    int n_steps;                 /* S >= 1 */
    const int* corr_off;         /* [S + 1] ascending: step k's correspondences are rows corr_off[k-1] .. corr_off[k] - 1 of corr */
    const double* corr;          /* x0 y0 x1 y1 rows: corres[i].first(0,1) / .second(0,1) of getCorresponding(frame_count - 1, frame_count) */
    const double* delta_q;       /* [S][4] (w x y z) pre_integrations[frame_count]->delta_q */
    /* the carried state: a caller who feeds one frame at a time gets what one long call gives */
    int n_prev;                  /* records before this call (0: the reference's constructor) */
    const double* prev;          /* [n_prev][27] the records Rc | Rimu | Rc_g, row-major, in order */
    const double* ric_prev;      /* [9] ric after the last earlier step; the identity when n_prev = 0, as the constructor sets it */
    /* what the reference hard-codes; its values are the defaults a caller should set */
    double ransac_threshold;     /* 3.0, cv::findFundamentalMat's default */
    double confidence;           /* 0.99 (nothing else is accepted) */
    int min_points;              /* 9 */
    double huber_deg;            /* 5.0 */
    int min_frames;              /* 10 (WINDOW_SIZE) */
    double cov_threshold;        /* 0.25 */
} vg_exrot_in;

typedef struct {                 /* every pointer may be NULL */
    size_t struct_size;          /* sizeof(vg_exrot_out), set by the caller */
    int status;                  /* VG_EXROT_* */
    int first_ok;                /* n_prev + k of the first step the reference would have returned true at, or -1 */
    double calib_ric[9];         /* ric of that step, row-major; zeros when none */
    /* per step, [S] each */
    double* records;             /* [S][27] Rc | Rimu | Rc_g: append to prev to resume */
    double* ric;                 /* [S][9] */
    double* sigma;               /* [S][4] descending */
    int* ok;
    double* huber;               /* the weight of the step's OWN record */
    /* taps per step */
    int* branch;                 /* 0 identity, 1 LMedS, 2 RANSAC */
    int *ransac_iter, *ransac_bound, *ransac_inliers, *ransac_best;     /* as vg_relpose_out; 0 outside branch 2 */
    double* F;                   /* [S][9] */
    int* front;                  /* [S][4] (R1,t1) (R1,t2) (R2,t1) (R2,t2) */
    int *picked, *used_fallback; /* 1 or 2 (0: identity) */
    double* device_ms;           /* read on out[0] only: [VG_EXROT_LAUNCHES] device time per launch from events, or NULL.  The LMedS
                                  * estimates and the second submission (used_fallback) are NOT in these figures */
} vg_exrot_out;

int vg_init_exrot(vg_handle* h, int n_windows, const vg_exrot_in* in, vg_exrot_out* out);

/* block kinds of the marginalization prior (MarginalizationInfo::keep_block_*) */
enum { VG_BLK_POSE = 0, VG_BLK_SPEEDBIAS = 1, VG_BLK_EXPOSE = 2, VG_BLK_TD = 3 };
enum { VG_MARGIN_OLD = 0, VG_MARGIN_SECOND_NEW = 1, VG_MARGIN_NONE = 2 };

/* The optimisation problem exactly as Estimator::optimization() assembles it from
 * para_Pose / para_SpeedBias / para_Ex_Pose / para_Feature / para_Td (estimator.cpp:486-528),
 * f_manager.feature (:719-764), pre_integrations[] (:711-718) and last_marginalization_info (:703-709).
 * All arrays are caller-owned host memory, read-only. */
#define VG_PRIOR_RESIDENT (-1)
typedef struct {
    int K;                       /* frames in the window = WINDOW_SIZE + 1                        */
    int L;                       /* landmarks that pass used_num>=2 && start_frame<WINDOW_SIZE-2  */
    int n_obs;                   /* rows of `obs`                                                 */
    const double* pose;          /* K x 7  [px py pz qx qy qz qw]                                  */
    const double* speedbias;     /* K x 9  [v ba bg]                                               */
    const double* ex_pose;       /* 7      camera-in-IMU extrinsic                                 */
    double td;
    const double* inv_depth;     /* L      inverse depth in the landmark's first observing frame   */
    const int* lm_start;         /* L      start_frame                                             */
    const int* lm_nobs;          /* L      feature_per_frame.size()  (consecutive frames)          */
    const int* lm_obs_off;       /* L      first row of this landmark in `obs`                     */
    const double* obs;           /* n_obs x 7  [x y u v vx vy cur_td]; x,y normalised (z = 1)      */
    const vg_imu_preint* imu;    /* K-1    factor k links frame k -> k+1                           */
    /* prior (MarginalizationFactor, marginalization_factor.cpp:321-381); prior_n == 0: none.
     * prior_n == VG_PRIOR_RESIDENT: the prior this window slot (index in the batch) holds ON THE DEVICE -- the result of the
     * marginalization of the handle's last run for that slot if it produced one (flag != VG_MARGIN_NONE, vg_ba_prior.valid),
     * else the prior the slot was last given.  The reference keeps last_marginalization_info in place between two calls of
     * optimization() (estimator.cpp:703-709, :836-870); this is the same thing for a prior that lives in HBM: nothing of it
     * crosses the host boundary (download the states with out_priors = NULL).  The other prior_* fields are ignored.  Needs
     * the same K and the same batch slot as the run that produced it; VG_ERR_BAD_ARG if the slot holds nothing.          */
    int prior_n;                 /* rows of the prior = sum of local block sizes                   */
    int prior_nblocks;
    const int* prior_block_kind; /* VG_BLK_*                                                       */
    const int* prior_block_index;/* frame index for POSE / SPEEDBIAS, 0 otherwise                  */
    const double* prior_J0;      /* prior_n x prior_n row-major linearized_jacobians               */
    const double* prior_r0;      /* prior_n           linearized_residuals                          */
    const double* prior_x0;      /* concatenated keep_block_data (global sizes 7/9/7/1)            */
    /* relocalisation factors (estimator.cpp:769-801); relo_n == 0: none */
    int relo_n;
    const double* relo_pose;     /* 7                                                              */
    const int* relo_lm;          /* relo_n  landmark index                                         */
    const double* relo_xy;       /* relo_n x 2 matched normalised point in the loop frame          */
    /* options */
    int estimate_extrinsic;      /* 0: ex_pose constant (SetParameterBlockConstant, :686-689)      */
    int estimate_td;             /* 1: ProjectionTdFactor + td block (:694-698, :741-746)          */
    int max_iters;               /* NUM_ITERATIONS                                                  */
    double focal;                /* FOCAL_LENGTH: sqrt_info = focal/1.5 * I (estimator.cpp:17-18)   */
    double tr;                   /* TR  rolling-shutter read-out time                               */
    double row;                  /* ROW image height                                                */
    double g_norm;               /* G = (0,0,g_norm)                                                */
    double max_solver_time_s;    /* SOLVER_TIME (estimator.cpp:812-815: options.max_solver_time_in_seconds); 0 = no
                                  * cap.  Checked on the device clock before every trust-region iteration, like Ceres does
                                  * on the host clock: termination stays NO_CONVERGENCE.  A cap makes the result depend on
                                  * timing; it is ignored while an all-reduce hook is installed (ranks must agree).        */
} vg_ba_problem;

/* Optimised state, AFTER Estimator::double2vector()'s gauge fix and the vector2double() repack
 * (estimator.cpp:530-619, :486-528).  Caller-owned buffers sized as in vg_ba_problem. */
typedef struct {
    double* pose;                /* K x 7 */
    double* speedbias;           /* K x 9 */
    double* ex_pose;             /* 7     */
    double* td;                  /* 1     */
    double* inv_depth;           /* L     (a negative value => FeatureManager::setDepth marks solve_flag = 2) */
    double* relo_pose;           /* 7 or NULL */
} vg_ba_state;

enum { VG_TERM_NO_CONVERGENCE = 0, VG_TERM_CONVERGENCE = 1, VG_TERM_FAILURE = 2 };

typedef struct {
    int status;                  /* vg_status of this window                                      */
    int termination;             /* VG_TERM_*                                                     */
    int num_iterations;          /* trust-region iterations performed (accepted + rejected)       */
    int num_accepted;
    double initial_cost;
    double final_cost;
    double final_radius;
    /* per-iteration trace (first num_iterations entries) */
    double it_cost[VG_MAX_ITERS];       /* cost at the current point before the step             */
    double it_cost_cand[VG_MAX_ITERS];  /* cost at the candidate                                   */
    double it_model[VG_MAX_ITERS];      /* model cost change                                       */
    double it_radius[VG_MAX_ITERS];     /* trust-region radius used                                */
    double it_step_norm[VG_MAX_ITERS];  /* dogleg step norm (scaled space)                         */
    int it_flags[VG_MAX_ITERS];         /* bit0 valid, bit1 accepted                               */
    double prof[16];                    /* device phase timers (shader cycles of lane 0); zero unless the library
                                           was built with -DBA_PROFILE                                  */
    /* the gauge transform double2vector() applied (estimator.cpp:541-577): x_fixed = gauge_rot (x - gauge_p0) + Ps[0]_before,
     * R_fixed = gauge_rot R; gauge_rot = rot_diff (3x3 row-major), gauge_p0 = para_Pose[0] position right after the solve.
     * For quantities outside the window, e.g. relo_Pose when no matched landmark put it into the problem (:598-603).   */
    double gauge_rot[9];
    double gauge_p0[3];
} vg_ba_summary;

/* New marginalization prior (MarginalizationInfo after marginalize() + getParameterBlocks(),
 * marginalization_factor.cpp:174-319), blocks already re-labelled for the slid window
 * (addr_shift, estimator.cpp:913-930 / :969-996).  Caller allocates J0[cap*cap], r0[cap],
 * x0[9*cap_blocks] (global block sizes: 7 pose / 9 speed-bias / 7 extrinsic / 1 td), block_kind/index[cap_blocks] and sets
 * cap / cap_blocks. */
typedef struct {
    int cap;                     /* in: capacity (rows) of J0 / r0                                */
    int cap_blocks;              /* in: capacity of the block arrays                              */
    int n;                       /* out: kept dimension  (0: no prior produced)                   */
    int m;                       /* out: marginalised dimension                                   */
    int nblocks;                 /* out */
    int valid;                   /* out: 1 if a new prior was produced, 0 if the old one stays    */
    int* block_kind;
    int* block_index;
    double* J0;                  /* n x n row-major */
    double* r0;
    double* x0;                  /* concatenated, global sizes */
} vg_ba_prior;

/* One synchronous Estimator::optimization(): solve + gauge fix (+ marginalization if
 * margin_flag != VG_MARGIN_NONE; out_prior may be NULL then). */
int vg_ba_optimize(vg_handle* h, const vg_ba_problem* in, int margin_flag,
                   vg_ba_state* out_state, vg_ba_summary* out_summary, vg_ba_prior* out_prior);

/* Batch of independent windows (BASELINE.json configs[3]); staged so that benchmarks can time the
 * device work alone with inputs resident in HBM:
 *   upload   : pack + H2D (synchronous on return)
 *   run_async: enqueue the solve pipeline (+ marginalization kernel) for every uploaded window
 *   download : D2H + unpack (synchronises first)
 * All windows of a batch must share K, estimate_extrinsic, estimate_td and relo presence. */
int vg_ba_batch_upload(vg_handle* h, int nwin, const vg_ba_problem* const* in, const int* margin_flags);
int vg_ba_batch_run_async(vg_handle* h);
/* same as run_async but synchronous and timed with HIP events on the handle's stream: the solve pipeline (all its
 * launches) and the marginalization kernel */
int vg_ba_batch_run_timed(vg_handle* h, float* solve_ms, float* marg_ms);
int vg_ba_batch_download(vg_handle* h, int nwin, vg_ba_state* const* out_states,
                         vg_ba_summary* out_summaries, vg_ba_prior* const* out_priors);
/* The download in two parts.  The states and summaries are final as soon as the solve pipeline has finished; the
 * marginalization kernel that follows on the stream only reads them, and its result is consumed by the NEXT frame's
 * optimization (estimator.cpp:703-709).  download_state returns while the marginalization is still running (it waits for
 * an event recorded behind the solve pipeline and copies on a second stream); download_prior waits for the whole stream.
 * Collect the priors before the handle's next upload. */
int vg_ba_batch_download_state(vg_handle* h, int nwin, vg_ba_state* const* out_states, vg_ba_summary* out_summaries);
int vg_ba_batch_download_prior(vg_handle* h, int nwin, vg_ba_prior* const* out_priors);
/* vg_ba_optimize in the same two parts (one window): begin = upload + run + download_state */
int vg_ba_optimize_begin(vg_handle* h, const vg_ba_problem* in, int margin_flag, vg_ba_state* out_state, vg_ba_summary* out_summary);
int vg_ba_optimize_prior(vg_handle* h, vg_ba_prior* out_prior);
/* one synchronous run with a HIP event after every launch of the solve pipeline: ms[k] = summed duration and n[k] =
 * number of launches of kernel class k (both arrays VG_BA_KERNEL_COUNT long) */
enum { VG_BA_KERNEL_PROLOGUE = 0, VG_BA_KERNEL_LINEARIZE, VG_BA_KERNEL_ACCUMULATE, VG_BA_KERNEL_SOLVE, VG_BA_KERNEL_FINAL,
       VG_BA_KERNEL_MARG,
       /* large-window path: landmark Schur kernel; reduced solve (+ the preceding all-reduce); dogleg step (+ its all-reduce) */
       VG_BA_KERNEL_BIG_SCHUR, VG_BA_KERNEL_BIG_SOLVE, VG_BA_KERNEL_BIG_STEP, VG_BA_KERNEL_COUNT };
int vg_ba_batch_run_profiled(vg_handle* h, float* ms, int* n);
/* the SURVEY.md 8(d) flop model of one run of the uploaded batch, split per kernel class (VG_BA_KERNEL_COUNT doubles) */
int vg_ba_batch_flops_by_kernel(vg_handle* h, double* flops);
/* algorithmic work of the uploaded batch for roofline accounting (SURVEY.md 8(d) flop model) */
int vg_ba_batch_info(vg_handle* h, double* flops_per_run, double* bytes_in, double* bytes_out, int* lds_bytes);
/* the same flop model split per launch: ba_solve_kernel (solve + prior J^T J) and ba_marg_kernel (the marginalization term) */
int vg_ba_batch_flops(vg_handle* h, double* solve_flops, double* marg_flops);

/* ---- Large windows and landmark shards (BASELINE.json configs[4]) --------------------------------
 * The reference fixes WINDOW_SIZE = 10 and NUM_OF_F = 1000 at compile time (vins_estimator/src/parameters.h:12,14) and
 * walks every factor in one thread (estimator.cpp:719-764); here both are runtime sizes.  A window whose camera part is
 * wider than the single-workgroup pipeline's tiling (more than ~13 frames) automatically takes the LARGE-WINDOW PATH: the
 * landmark Schur complement is formed by a multi-workgroup kernel into a reduce buffer, the reduced system is factorised
 * out of HBM / LDS by one workgroup.  The same path shards a window over ranks: every rank uploads the SAME frames, IMU
 * factors and prior but only ITS contiguous share of the landmarks (with their observations), installs an all-reduce
 * hook, and calls vg_ba_batch_run_async as usual (on this path the call waits for the stream once or a few times near the end of
 * the solve: the rounds that only exist for retried factorisations are issued on demand, after a look at the windows' DONE flags);
 * after the run every rank holds the identical frame states and the inverse depths of its own landmarks.  Marginalization: a large
 * window on ONE rank is marginalized like any other (margin_flags); with an all-reduce hook installed margin_flags must be NONE --
 * a MARGIN_OLD marginalization only involves the tracks anchored at frame 0, so the ranks all-gather those (a few KB) and every rank
 * marginalizes the same reduced single-rank problem (all frames at the solved states, imu[], the old prior, those tracks,
 * max_iters = 0) on a second handle without a hook: identical result everywhere (vins-mono_amd/shard.py marginalize_sharded).
 *
 * The hook is called on the host, twice per trust-region round, between two kernel launches: it must enqueue on `stream`
 * (a hipStream_t) an in-place SUM over all ranks of `count` doubles at `device_buf` -- with RCCL:
 *     ncclAllReduce(device_buf, device_buf, count, ncclDouble, ncclSum, comm, (hipStream_t)stream)
 * -- and return 0.  No host synchronisation is needed or wanted.  count is the same on every rank (it depends only on the
 * window's frame count and flags): vg_ba_reduce_layout reports both counts (reduced system; step norms). */
typedef int (*vg_allreduce_fn)(void* user, double* device_buf, size_t count, void* stream);
int vg_ba_set_allreduce(vg_handle* h, vg_allreduce_fn fn, void* user);       /* fn == NULL: single rank */
int vg_ba_set_large_window(vg_handle* h, int force);     /* force != 0: take the large-window path whatever the size */

/* The same hook bound to RCCL over xGMI inside the library (csrc/vg_rccl.hip; librccl is opened with dlopen at the first call,
 * VG_ERR_UNSUPPORTED if it cannot be).  One process per GPU: rank 0 calls vg_rccl_unique_id and hands the 128 bytes to the
 * other ranks by whatever channel the application has (torch.distributed / MPI broadcast); every rank then calls
 * vg_ba_rccl_init(handle, nranks, rank, id) — collective, it creates the communicator on the handle's device and installs
 * ncclAllReduce(buf, buf, count, ncclDouble, ncclSum, comm, launch stream) as the hook.  vg_ba_rccl_finalize (also run by
 * vg_destroy) removes the hook and destroys the communicator. */
#define VG_RCCL_ID_BYTES 128
int vg_rccl_unique_id(char* id128);
int vg_ba_rccl_init(vg_handle* h, int nranks, int rank, const char* id128);
int vg_ba_rccl_finalize(vg_handle* h);

/* How vg_ba_batch_run_async / vg_ba_optimize* issue the solve pipeline (prologue, max_iters x {linearise IMU + prior,
 * linearise projections, accumulate, solve}, cost pass, final: 4 * max_iters + 4 launches):
 *   VG_LAUNCH_DIRECT  one hipLaunchKernelGGL per kernel;
 *   VG_LAUNCH_GRAPH   the sequence is captured from the handle's stream into a hipGraph the first time a given combination of
 *                     device buffers, grid sizes and round count is run, and replayed by ONE hipGraphLaunch afterwards (the
 *                     kernel arguments of a batch do not change from run to run; a re-allocation or a different size class
 *                     re-captures).  Same kernels, same results, bit for bit.
 * Default: environment VG_BA_LAUNCH_MODE = "graph" | "direct", else VG_LAUNCH_DEFAULT.  The large-window path (all-reduce hook
 * between launches) and the profiled run always launch directly.  vg_ba_launch_stats reports the mode in effect and how many
 * graph launches / captures the handle has made. */
enum { VG_LAUNCH_DIRECT = 0, VG_LAUNCH_GRAPH = 1 };
#ifndef VG_LAUNCH_DEFAULT
#define VG_LAUNCH_DEFAULT VG_LAUNCH_DIRECT
#endif
int vg_ba_set_launch_mode(vg_handle* h, int mode);
int vg_ba_launch_stats(vg_handle* h, int* mode, long long* graph_launches, long long* graph_captures);
/* ABI 8.  From how many windows per batch on the factors of a round are linearised AND accumulated by ONE kernel with one workgroup per
 * window (ba_linacc_proj_kernel: IMU factors, prior and projection factors; the projection records stay in LDS, J^T J of the camera
 * blocks on MFMA) instead of by ba_linearize_imu / ba_linearize_proj / ba_accumulate spread over many workgroups per window.  With few
 * windows the spread form is faster (the chip is empty), with a full batch the fused one (+18 % solves/s at 256 windows).  Default:
 * environment VG_BA_FUSED_MIN, else 32; 0 = never.  Windows with extrinsic / td columns or on the large-window path always take the
 * spread form.  Takes effect at the next upload. */
int vg_ba_set_fused_min_windows(vg_handle* h, int min_windows);
int vg_ba_batch_is_fused(vg_handle* h);      /* uploaded batch: 0 = spread kernels; 1 = fused factor kernel (counted as VG_BA_KERNEL_ACCUMULATE) + solve kernel;
                                              * < 0: error.  (2 = one merged launch per round was an experiment of ABI 8-9; removed) */

/* Capacities the layout of every later batch is built for at least (landmarks, projection factors and observation rows per window,
 * rows of the prior): a caller whose windows fluctuate from frame to frame keeps one layout -- no re-allocation, and in
 * VG_LAUNCH_GRAPH mode no re-capture.  Zero leaves a capacity to the data.  Takes effect at the next upload. */
int vg_ba_reserve(vg_handle* h, int max_landmarks, int max_factors, int max_obs, int max_prior_n);

/* ---- Windows that stay on the device from frame to frame ------------------------------------------------
 * The reference keeps the sliding window in host members between two calls of optimization(): f_manager.feature (every track,
 * also the ones not yet in the problem), Ps / Rs / Vs / Bas / Bgs, pre_integrations[], last_marginalization_info.  Around
 * optimization() it runs, per frame (Estimator::processImage, estimator.cpp:120-215):
 *     f_manager.addFeatureCheckParallax   (feature_manager.cpp:45-107)   new observations, key-frame decision
 *     f_manager.triangulate               (feature_manager.cpp:202-257)  depth of the tracks that enter the problem
 *     optimization()                      (estimator.cpp:670-1003)       solve + marginalization
 *     slideWindow()                       (estimator.cpp:1005-1126)      state / pre-integration shift,
 *                                         FeatureManager::removeBackShiftDepth / removeFront (feature_manager.cpp:275-351)
 *     f_manager.removeFailures            (feature_manager.cpp:161-171)
 * A sequence does all of that on the device for a batch of independent windows: the track tables, the states, the IMU constants
 * and the prior never leave HBM; per frame the host sends the new frame's observations (id + 7 doubles each) and EITHER its
 * state guess (what processIMU propagated) and the pre-integration of the new interval (vg_ba_seq_step_async) OR the raw IMU
 * samples since the frame before (vg_ba_seq_step_imu_async: processIMU runs on the device too, see below), and reads back the
 * states.  No per-frame packing, no re-upload of the window.  Relocalisation frames are taken by a sequence begun after
 * vg_ba_seq_relo_reserve (below: vg_ba_seq_set_relo); the large-window path is not offered in a sequence.                    */
typedef struct {
    int n_features;              /* f_manager.feature.size(), list order                                                     */
    const int* feature_id;       /* FeaturePerId::feature_id                                                                 */
    const int* start_frame;
    const int* n_obs;            /* feature_per_frame.size() (consecutive frames from start_frame)                           */
    const int* solve_flag;       /* may be NULL (all 0)                                                                      */
    const double* depth;         /* estimated_depth (-1: not triangulated yet)                                               */
    const double* obs;           /* sum(n_obs) rows, feature-major: [x y z u v vx vy cur_td] (FeaturePerFrame)                */
} vg_ba_tracks;

typedef struct {
    int max_features;            /* capacity of a window's track table                                                       */
    int max_new_obs;             /* capacity of one frame's observation list                                                 */
    int max_landmarks;           /* tracks in the problem at once (0: max_features)                                           */
    int max_factors;             /* projection factors at once (0: 6 x max_landmarks)                                         */
    double init_depth;           /* INIT_DEPTH   (vins_estimator/src/parameters.cpp:3)                                       */
    double min_parallax;         /* MIN_PARALLAX (keyframe_parallax / FOCAL_LENGTH, parameters.cpp:79-80)                    */
} vg_ba_seq_config;

/* The new frame of one window: what Estimator::processImage receives (the `image` map in ascending feature id: one
 * observation per feature, rows [x y z u v vx vy]) plus what Estimator::processIMU has produced since the last frame: the
 * propagated state of the newest frame (Ps / Rs / Vs [WINDOW_SIZE], biases copied from the frame before) and
 * pre_integrations[WINDOW_SIZE].  imu_merged: after a frame that was NOT a key frame (margin flag VG_MARGIN_SECOND_NEW)
 * slideWindow folds the dropped interval's samples into pre_integrations[WINDOW_SIZE - 1] (estimator.cpp:1069-1085); the
 * caller re-integrates that interval (vg_imu_preintegrate over the concatenated samples) and hands it over here; NULL otherwise. */
typedef struct {
    double pose[7];
    double speedbias[9];
    const vg_imu_preint* imu_new;
    const vg_imu_preint* imu_merged;
    int n_obs;
    const int* feature_id;       /* ascending                                                                                */
    const double* obs;           /* n_obs x 7                                                                                */
} vg_ba_frame;

/* per-window record of the last step (vg_ba_seq_info) */
enum { VG_SEQ_FLAG = 0,          /* marginalization flag the key-frame test chose (VG_MARGIN_OLD: the frame before was a key frame) */
       VG_SEQ_N_FEATURES,        /* tracks in the table after the new observations were added                                 */
       VG_SEQ_N_TRACKED,         /* last_track_num                                                                            */
       VG_SEQ_N_PARALLAX,        /* parallax_num                                                                              */
       VG_SEQ_N_LANDMARKS,       /* tracks in the problem                                                                     */
       VG_SEQ_N_FACTORS,
       VG_SEQ_STATUS,            /* VG_OK or VG_ERR_UNSUPPORTED: a capacity of vg_ba_seq_config was exceeded (the step is void)  */
       VG_SEQ_N_AFTER,           /* tracks left after slideWindow + removeFailures                                            */
       VG_SEQ_INFO_INTS = 8 };

/* windows[w]: states of the K frames, imu[K-1], prior, options of window w as in vg_ba_optimize (its landmark tables are ignored;
 * frame K-1 and imu[K-2] are placeholders that the first step overwrites); tracks[w]: its track table.  This is the state
 * the reference is in between two frames (after slideWindow).  All windows share K and the estimate_* options. */
int vg_ba_seq_begin(vg_handle* h, int nwin, const vg_ba_seq_config* cfg, const vg_ba_problem* const* windows,
                    const vg_ba_tracks* const* tracks);
/* One frame for every window: add + key-frame test + triangulate + problem tables + solve + marginalization + slide, all
 * enqueued on the handle's stream. */
int vg_ba_seq_step_async(vg_handle* h, int nwin, const vg_ba_frame* const* frames);
/* States of the window as solved by the last step (before the slide) and its summaries: vg_ba_batch_download_state;
 * vg_ba_state::inv_depth, if not NULL, must hold max_landmarks rounded up to a multiple of 16 values (the first
 * info[VG_SEQ_N_LANDMARKS] are the problem's, in track-list order).  info: [nwin][VG_SEQ_INFO_INTS]. */
int vg_ba_seq_info(vg_handle* h, int nwin, int* info);
/* parity tap: the track table of one window as the last step left it; arrays of capacity cap (obs may be NULL; else
 * cap x K x 8 doubles, rows [x y u v vx vy cur_td z] of feature f at obs + (f * K + j) * 8) */
int vg_ba_seq_get_tracks(vg_handle* h, int window, int cap, int* n_features, int* feature_id, int* start_frame, int* n_obs,
                         int* solve_flag, double* depth, double* obs);
/* Hand-back and re-seed of ONE window of a running sequence, between two frames (after a step):
 *   export  the window of slot `window` in the form vg_ba_seq_begin takes it -- states (K x 7, K x 9, 7, 1), the K-1 pre-integration
 *           records (the newest one is the placeholder the next step fills: valid = 0), the prior (caller-allocated as for
 *           vg_ba_optimize; n = 0: none; after a step that chose VG_MARGIN_SECOND_NEW the record of interval K-3 is still the
 *           un-merged one -- the merged record reaches the device with the next frame's imu_merged; a sequence in IMU mode holds the merged one already) -- together with vg_ba_seq_get_tracks this is everything the reference keeps in
 *           Ps / Rs / Vs / Bas / Bgs, pre_integrations[], f_manager.feature and last_marginalization_info: a host Estimator can
 *           take the window back (a checkpoint; a failure re-start; a relocalisation frame needs no hand-back: vg_ba_seq_set_relo);
 *   import  replaces what slot `window` holds (same K and estimate_* options as the sequence; prior from the host or none) while
 *           the other windows stay where they are.  Any output pointer of export may be NULL. */
int vg_ba_seq_export(vg_handle* h, int window, double* pose, double* speedbias, double* ex_pose, double* td, vg_imu_preint* imu,
                     vg_ba_prior* prior);
int vg_ba_seq_import(vg_handle* h, int window, const vg_ba_problem* in, const vg_ba_tracks* tracks);
int vg_ba_seq_end(vg_handle* h);

/* ---- Sequences that take raw IMU samples: Estimator::processIMU on the device (added within ABI 12) ------------------------------
 * With vg_ba_seq_step_async the caller still does Estimator::processIMU (estimator.cpp:84-118) and the IMU part of slideWindow()
 * (:1069-1095) on the host: it keeps the sample buffers of the last two intervals, propagates Ps / Rs / Vs[WINDOW_SIZE],
 * pre-integrates the new interval (vg_imu_preintegrate, a synchronous round trip), re-integrates the merged one after a dropped
 * non-keyframe, and uploads two records of 472 doubles per window and frame.  The device holds every input of that work (the
 * solved newest state, its biases, the record of the interval before), so a sequence switched to IMU mode takes, per frame and
 * window, ONLY the observations and the raw samples (dt acc gyr) that arrived since the frame before -- what the estimator node
 * receives from its two topics -- and nothing of the window's IMU data ever leaves HBM.  One vg_ba_seq_step_imu_async does
 *   processIMU   for every sample in order: pre_integrations[WINDOW_SIZE]->push_back into a fresh record, linearised at the biases
 *                of slot K-1 as the last slide left them and started from the resident acc_0 / gyr_0 (the arithmetic of
 *                vg_imu_preintegrate, one shared text); the mid-point propagation of Ps / Rs / Vs[WINDOW_SIZE] (:107-114) from the
 *                solved state of slot K-1.  The record goes to interval K-2 (valid = sum_dt <= 10), the guess to state slot K-1,
 *                the biases of slot K-1 stay, acc_0 / gyr_0 become the last sample.
 *                Rs: the matrix of the NORMALISED quaternion of slot K-1, multiplied per sample by the matrix of the NORMALISED
 *                deltaQ(un_gyr dt) = (theta / 2, 1) / |.|, converted back and normalised: the project's restatement of processIMU
 *                (oracle/window_numpy.py propagate, against which the device is tested to 1e-11).  The reference (and
 *                host/resident_estimator.cpp on its default path) multiplies by the UN-normalised deltaQ matrix, which is not a
 *                rotation; the two guesses differ by |theta|^3 / 4 per sample (4e-8 in the quaternion over 20 samples of a 200 Hz
 *                EuRoC-like interval), far below what the solve that follows it resolves.
 *   the step     of vg_ba_seq_step_async, unchanged: add, key-frame test, triangulate, build, solve, marginalization, slide.
 *   the merge    after a step that chose VG_MARGIN_SECOND_NEW the record that is at K-3 after the slide is CONTINUED with this
 *                frame's samples (push_back from the stored sum_dt, delta_p / q / v, jacobian, covariance, with the record's own
 *                linearisation biases and the measurement that ended it, as estimator.cpp:1069-1081 does); valid is re-evaluated
 *                on the merged sum_dt.  Difference to the host-fed mode: vg_ba_seq_export returns the MERGED record right after
 *                such a step (host-fed: the un-merged one until the next frame brings imu_merged).
 * The states come back as before (vg_ba_batch_download_state, vg_ba_seq_info). */
typedef struct vg_ba_seq_imu_config {
    int struct_size;             /* sizeof(vg_ba_seq_imu_config)                                                             */
    int max_samples;             /* capacity of one frame's sample list, 1 .. 512                                            */
    double noise[4];             /* ACC_N GYR_N ACC_W GYR_W, as vg_imu_preintegrate                                          */
} vg_ba_seq_imu_config;
/* After vg_ba_seq_begin, before the first step: switches the running sequence to IMU mode.  seed[w] = acc_0(3) gyr_0(3) g(3):
 * the newest IMU measurement (Estimator::acc_0 / gyr_0) and Estimator::g of that estimator (per window: the reference refines
 * it at initialisation).  State slot K-2 is copied into K-1 on the device (what slideWindow leaves; vg_ba_seq_import does the
 * same in this mode), so the "frame K-1 is a placeholder" rule of vg_ba_seq_begin keeps holding for the caller. */
int vg_ba_seq_imu_begin(vg_handle* h, int nwin, const vg_ba_seq_imu_config* cfg, const double* seed /* [nwin][9] */);
typedef struct vg_ba_frame_imu {
    int n_samples;               /* 1 .. max_samples.  ONE sample makes a singular covariance (the position rows of V are dt / 2
                                  * times its velocity rows, integration_base.h:113-124): the record is exact, the solve of a
                                  * window that holds such an interval may report VG_ERR_NUMERIC                              */
    const double* samples;       /* n_samples x 7: dt acc gyr, in arrival order                                              */
    int n_obs;
    const int* feature_id;       /* ascending                                                                                */
    const double* obs;           /* n_obs x 7, as vg_ba_frame                                                                */
} vg_ba_frame_imu;
/* Refused with VG_ERR_BAD_ARG before anything is uploaded (vg_last_error says why; the sequence stays usable): no
 * vg_ba_seq_imu_begin, n_samples < 1 or > max_samples, samples NULL, a sample that is not finite, nwin other than the sequence's,
 * ids not ascending.  vg_ba_seq_step_async is refused on a sequence in IMU mode (it would leave the resident measurement stale). */
int vg_ba_seq_step_imu_async(vg_handle* h, int nwin, const vg_ba_frame_imu* const* frames);
/* Parity tap and re-seed of ONE window between two frames.
 *   get  seed9: the last measurement + g; guess_pose7 / guess_sb9: the state guess the LAST step propagated.  Any pointer may be NULL.
 *   set  seed9, after vg_ba_seq_import of that window. */
int vg_ba_seq_imu_get(vg_handle* h, int window, double* seed9, double* guess_pose7, double* guess_sb9);
int vg_ba_seq_imu_set(vg_handle* h, int window, const double* seed9);
/* Measurement tap: with timing on, every step records HIP events around ba_seq_imu_kernel and around ba_seq_merge_kernel (all
 * windows of the batch); vg_ba_seq_imu_times waits for the last step's merge and returns the two device times in ms (either
 * pointer may be NULL).  VG_ERR_BAD_ARG without a sequence in IMU mode, or when the last step was not timed. */
int vg_ba_seq_imu_timing(vg_handle* h, int on);
int vg_ba_seq_imu_times(vg_handle* h, float* imu_kernel_ms, float* merge_kernel_ms);

/* ---- Relocalisation frames of a resident sequence (added within ABI 12, nothing existing changed) ---------------------------------
 * When the pose graph reports a loop, Estimator::setReloFrame (estimator.cpp:1128-1147) leaves match_points, relo_Pose and
 * relo_frame_local_index for the NEXT optimization(), which adds one pose block and one ProjectionFactor per matched landmark
 * (:769-801) and whose double2vector() forms the relative pose and the drift correction (:598-612).  A sequence does the same
 * without handing its window back: the matches go up with the next step's staging, the factors are selected from the resident
 * track table on the device (the reference's cursor walk, reproduced for track lists that are not ascending too), the loop pose
 * is the K+1-th pose block of the window.
 *   vg_ba_seq_relo_reserve  before vg_ba_seq_begin, like vg_ba_reserve: with 1 <= max_match <= 1024 the NEXT vg_ba_seq_begin lays out
 *                           the loop-pose block and adds max_match to its factor and observation-row capacities; the reservation
 *                           is consumed by that begin.  0 cancels it.  Without a reservation vg_ba_seq_begin builds the layout it
 *                           always built.  Between relocalisation frames the block is idle: it holds the unit pose 0 0 0 0 0 0 1
 *                           and no factor.  vg_ba_seq_begin refuses (VG_ERR_UNSUPPORTED) a K whose wider camera part leaves the
 *                           single-workgroup pipeline, and keeps refusing windows that arrive with relo_n != 0.
 *   vg_ba_seq_set_relo      between two frames: arms window `window` for the NEXT step only, whichever of vg_ba_seq_step_async,
 *                           vg_ba_seq_step_imu_async and vg_vio_step_async that is (relocalization_info is consumed by one
 *                           optimization()).  r == NULL disarms; arming twice keeps the second; vg_ba_seq_import of that window,
 *                           vg_ba_seq_end and vg_ba_seq_begin disarm.  VG_ERR_BAD_ARG before anything is touched (the sequence
 *                           stays usable): a sequence begun without a reservation, a wrong struct_size, frame outside 0 .. K-2,
 *                           n_match outside 1 .. max_match, ids that are not strictly ascending, a number that is not finite.
 *                           The call itself neither uploads nor synchronises; a step with no armed window uploads nothing extra.
 *                           An armed window whose factors or rows exceed the capacities reports VG_ERR_UNSUPPORTED in
 *                           info[VG_SEQ_STATUS] like every other capacity: the step is void, the relocalisation is consumed.
 *   vg_ba_seq_get_relo      after the states of a step are down (vg_ba_batch_download_state; vg_ba_state::relo_pose returns the
 *                           loop pose there too): the relocalisation outcome of that step for one window.  n_factors == 0 is
 *                           legal (no matched landmark is in the problem): the input pose is carried through the gauge transform,
 *                           which is what the reference computes.  The by-products are formed on the host, in double, from the
 *                           downloaded states with the reference's expressions (Utility::R2ypr / ypr2R / normalizeAngle, degrees).
 * info[VG_SEQ_N_FACTORS] counts the relocalisation factors too. */
typedef struct vg_ba_relo_frame {
    int struct_size;             /* sizeof(vg_ba_relo_frame)                                                                 */
    int frame;                   /* relo_frame_local_index, 0 .. K-2: index into the window as it stands between two frames
                                  * (what setReloFrame's loop over Headers[0 .. WINDOW_SIZE) finds; the sequence keeps no stamps) */
    const double* pose;          /* 7: the initial relo_Pose; NULL: the resident pose of window frame `frame` at the start of the step */
    int n_match;                 /* 1 .. max_match                                                                            */
    const int* match_id;         /* strictly ascending feature ids (match_points[k].z())                                      */
    const double* match_xy;      /* n_match x 2 normalised points in the loop frame                                           */
    double prev_relo_t[3];
    double prev_relo_r[9];       /* row-major                                                                                 */
} vg_ba_relo_frame;
typedef struct vg_ba_relo_result {
    int struct_size;             /* sizeof(vg_ba_relo_result), set by the caller                                              */
    int armed;                   /* 0 / 1: the window was armed for that step (0: everything below but pose is zero)          */
    int n_factors;               /* relocalisation factors in the problem                                                     */
    int frame;
    double pose[7];              /* the gauge-fixed loop pose (relo_r as a quaternion x y z w, relo_t)                         */
    double relo_relative_t[3];
    double relo_relative_q[4];   /* x y z w                                                                                   */
    double relo_relative_yaw;
    double drift_correct_r[9];   /* row-major                                                                                 */
    double drift_correct_t[3];
} vg_ba_relo_result;
int vg_ba_seq_relo_reserve(vg_handle* h, int max_match);
int vg_ba_seq_set_relo(vg_handle* h, int window, const vg_ba_relo_frame* r);
int vg_ba_seq_get_relo(vg_handle* h, int window, vg_ba_relo_result* out);

/* ---- What the estimator publishes between two frames: keyframe message and point clouds (added within ABI 12, nothing existing changed) ---
 * After every frame the estimator node (estimator_node.cpp:321-328) calls pubKeyframe (vins_estimator/src/utility/visualization.cpp:
 * 348-404) and pubPointCloud (:240-296); the pose graph builds its KeyFrame from the first.  A sequence forms both on the device
 * (ba_seq_publish_kernel, csrc/ba_seq.hip) from the CURRENT track table and the window's states as they stand between two frames --
 * after slideWindow() and removeFailures(), i.e. what vg_ba_seq_get_tracks and vg_ba_seq_export return -- and changes nothing resident.
 * With W = WINDOW_SIZE = K - 1, per window, every list in track-list order:
 *   keyframe list   tracks with start_frame < W - 2 && start_frame + n_obs - 1 >= W - 2 && solve_flag == 1 (:378): the world point,
 *                   the observation in frame W - 2 (row W - 2 - start_frame of the track: normalised x y, pixel u v) and the feature id.
 *                   The reference sends the id through a float channel (:397); here it stays the int it is: the two agree below 2^24.
 *   point cloud     n_obs >= 2 && start_frame < W - 2 && !(start_frame > W * 3.0 / 4.0) && solve_flag == 1 (:251-254): the world point
 *   margin cloud    n_obs >= 2 && start_frame < W - 2 && start_frame == 0 && n_obs <= 2 && solve_flag == 1 (:276-282): the world point
 *   world point     Rs[s] (ric (point0 estimated_depth) + tic) + Ps[s], s = start_frame, point0 = the first observation (x, y, z);
 *                   Rs / ric are the matrices of the normalised state quaternions.  Formed in double, rounded to float once, by the
 *                   store (geometry_msgs::Point32, ChannelFloat32; KeyFrame takes cv::Point3f / cv::Point2f).
 *   pose            of frame W - 2 (px py pz qx qy qz qw) and ex_pose (tic, ric), the resident doubles as they are.
 *   keyframe_valid  1 iff the last step of the sequence chose VG_MARGIN_OLD for this window (info[VG_SEQ_FLAG]): the
 *                   marginalization_flag == 0 gate of :351.  0 before the first step.  The keyframe list is formed either way; the flag
 *                   says whether the reference would publish it.  The caller owns the stamps (Headers[W - 2]): a sequence keeps none.
 *   status          VG_OK; the status of the window's last step when that step was void (info[VG_SEQ_STATUS] != VG_OK): the three
 *                   counts are 0 then; VG_SEQ_OUT_TRUNCATED when a list selects more tracks than max_points: the first max_points
 *                   of that list are stored, in list order, and n_* still report the true counts.
 *   vg_ba_seq_outputs_reserve  any time a sequence is live, 1 <= max_points <= 1024 (the kernels' track capacity): the device block
 *                              and the pinned staging for max_points rows per list and window.  Again: replaces the reservation
 *                              (what an earlier _async produced is gone).  The call WAITS for the handle's stream (a step
 *                              enqueued before it finishes first): reserve once, outside the frame loop.  vg_ba_seq_end frees it;
 *                              vg_ba_seq_begin starts without one.
 *   vg_ba_seq_outputs_async    enqueues the kernel and ONE download (headers + packed lists of every window) on the handle's stream,
 *                              behind whatever step was enqueued last; works after vg_ba_seq_step_async, vg_ba_seq_step_imu_async and
 *                              vg_vio_step_async alike, and right after vg_ba_seq_begin / vg_ba_seq_import.  On demand: no step
 *                              launches it, and the step's launches, downloads and results are what they were.
 *   vg_ba_seq_get_outputs      waits for the last _async (not for anything enqueued behind it) and copies one window: the scalars
 *                              always, each array that is not NULL for min(n_*, max_points) rows.  Arrays must hold max_points rows.
 * VG_ERR_BAD_ARG with a vg_last_error text and nothing moved: any of the three without a live sequence; _async or _get without a
 * reservation; _get before any _async since the reservation; a window out of range; a wrong struct_size; max_points out of range. */
#define VG_SEQ_OUT_TRUNCATED 1
typedef struct vg_ba_seq_outputs {
    int struct_size;             /* sizeof(vg_ba_seq_outputs), set by the caller                                              */
    int status;                  /* VG_OK / the void step's status / VG_SEQ_OUT_TRUNCATED                                     */
    int keyframe_valid;
    int n_keyframe, n_cloud, n_margin;   /* true counts (may exceed max_points: status says so)                               */
    double pose[7];              /* frame W - 2: px py pz qx qy qz qw                                                         */
    double ex_pose[7];           /* tic, ric (x y z w)                                                                        */
    float* kf_point_3d;          /* [max_points][3]   every array may be NULL                                                 */
    float* kf_norm;              /* [max_points][2]   normalised x y in frame W - 2                                           */
    float* kf_uv;                /* [max_points][2]   pixel u v in frame W - 2                                                */
    int* kf_id;                  /* [max_points]                                                                              */
    float* cloud_xyz;            /* [max_points][3]                                                                           */
    float* margin_xyz;           /* [max_points][3]                                                                           */
} vg_ba_seq_outputs;
int vg_ba_seq_outputs_reserve(vg_handle* h, int max_points);
int vg_ba_seq_outputs_async(vg_handle* h);
int vg_ba_seq_get_outputs(vg_handle* h, int window, vg_ba_seq_outputs* out);

/* Form of the prior factor the marginalization hands back (marginalization_factor.cpp:285-296 builds J0 = S^1/2 V^T,
 * r0 = S^-1/2 V^T b' from the eigen-decomposition A' = V S V^T of the kept system).  Everything downstream uses the factor
 * only through J0^T J0, J0^T r0 and |r0|^2, which do not change under an orthogonal transformation from the left:
 *   VG_MARG_SQRT  (default)  J0 = L^T, r0 = L^-1 b' from the diagonally pivoted Cholesky factor of A', cut where no remaining
 *                            pivot exceeds eps = 1e-8 (the reference cuts eigenvalues at the same eps);
 *   VG_MARG_EIGEN            the reference's eigen form (rows ordered by ascending eigenvalue).
 * Takes effect at the next upload / vg_ba_optimize. */
enum { VG_MARG_SQRT = 0, VG_MARG_EIGEN = 1 };
int vg_ba_set_marg_mode(vg_handle* h, int mode);
/* Added within ABI 12, nothing existing changed.  Which variants of the marginalization kernel a window of the uploaded batch ran
 * through -- read-only, for tests and diagnosis; valid once the priors of the run are on the host (vg_ba_batch_download with priors,
 * vg_ba_batch_download_prior, vg_ba_optimize), VG_ERR_BAD_ARG before.  out[0..3] = prior valid, n, m, kept blocks; out[4] = sweeps |
 * attempts << 8 of the eigen-decomposition of the dropped block (0: it left by elimination); out[5] = rank << 16 of the square-root
 * factor, or sweeps | attempts << 8 of the kept block's eigen-decomposition; out[6] = the path word below (0 for a window that
 * produced no prior; builds with -DBA_PROFILE keep a cycle stamp there instead); out[7] = 0.
 *   stage 1, the dropped block leaves (VG_MARGPATH_S1_MASK):  _DIRECT two-stage elimination on the matrix cores, A' written into the
 *       square root's tile; _BLOCK_LDS / _BLOCK_GLB certified block elimination with its right-hand sides staged in LDS / read from
 *       global memory; _VH_EIG / _JACOBI_LDS / _JACOBI_GLB eigen pseudo-inverse (16-lane groups / one-sided Jacobi in LDS / in global memory);
 *   certificate lambda_min(Amm) > 1e-7 (VG_MARGPATH_CERT_MASK): 0 not evaluated, _PASSED, _FAILED (every elimination that evaluated it was
 *       refused: the eigen pseudo-inverse ran);
 *   Schur product A' = Arr - Arm Amm^+ Amr behind stage 1 (VG_MARGPATH_SCHUR_MASK): 0 none (_DIRECT forms A' itself), _LDS, _GLB operands;
 *   stage 2, the factor of the kept block (VG_MARGPATH_S2_MASK): _SQRT / _SQRT_GLB pivoted Cholesky in LDS / global memory,
 *       _VH_EIG / _JACOBI_LDS / _JACOBI_GLB the eigen form. */
enum { VG_MARGPATH_S1_MASK = 0xf, VG_MARGPATH_S1_DIRECT = 1, VG_MARGPATH_S1_BLOCK_LDS = 2, VG_MARGPATH_S1_BLOCK_GLB = 3, VG_MARGPATH_S1_VH_EIG = 4,
       VG_MARGPATH_S1_JACOBI_LDS = 5, VG_MARGPATH_S1_JACOBI_GLB = 6,
       VG_MARGPATH_CERT_MASK = 0x30, VG_MARGPATH_CERT_PASSED = 0x10, VG_MARGPATH_CERT_FAILED = 0x20,
       VG_MARGPATH_SCHUR_MASK = 0xc0, VG_MARGPATH_SCHUR_LDS = 0x40, VG_MARGPATH_SCHUR_GLB = 0x80,
       VG_MARGPATH_S2_MASK = 0xf00, VG_MARGPATH_S2_SQRT = 0x100, VG_MARGPATH_S2_SQRT_GLB = 0x200, VG_MARGPATH_S2_VH_EIG = 0x300,
       VG_MARGPATH_S2_JACOBI_LDS = 0x400, VG_MARGPATH_S2_JACOBI_GLB = 0x500 };
int vg_ba_batch_marg_info(vg_handle* h, int window, int out[8]);
/* ABI 12.  Form of the IMU factors' weight sqrt_info = LLT(covariance^-1).matrixL()^T (factor/imu_factor.h:64).  The Cholesky factor of
 * the inverse is unique, so both forms are the same matrix up to rounding -- the covariance is badly conditioned, and the rounding of
 * this factor is one of the inputs of the trust-region decisions (profiles/r06_flip_stats.json):
 *   VG_IMU_INFO_FACTOR     (default)  U^-1 of covariance = U U^T (U upper): the inverse is never formed;
 *   VG_IMU_INFO_REFERENCE             covariance.inverse() by partial-pivot LU, then the LLT of its lower triangle, as the reference
 *                                     spells it (operation order of oracle/ref_stubs' stand-in Eigen, no contraction).
 * Takes effect at the next upload / vg_ba_optimize. */
enum { VG_IMU_INFO_FACTOR = 0, VG_IMU_INFO_REFERENCE = 1 };
int vg_ba_set_imu_info_mode(vg_handle* h, int mode);
int vg_ba_reduce_layout(vg_handle* h, size_t* count_system, size_t* count_norms);

/* Batched factor evaluation for parity tests (rows B2-B5 of SURVEY.md 8(a)): evaluates every
 * projection / IMU / prior factor of the problem at its input state WITHOUT the robust-loss
 * correction and returns residuals and tangent-space Jacobians.
 *   proj_r  [F x 2], proj_J [F x 2 x 20] columns = [pose_i(6) pose_j(6) ex(6) lambda(1) td(1)]
 *   imu_r   [(K-1) x 15], imu_J [(K-1) x 15 x 30] columns = [pose_i(6) sb_i(9) pose_j(6) sb_j(9)]
 *   prior_r [prior_n]
 * F = sum(lm_nobs - 1) + relo_n, landmark by landmark; a landmark's relocalisation factor follows its
 * window factors.  Any output pointer may be NULL.  The rows of an IMU factor the solve leaves out
 * (valid == 0 or sum_dt > 10) are zero. */
int vg_ba_eval_factors(vg_handle* h, const vg_ba_problem* in, double* proj_r, double* proj_J,
                       double* imu_r, double* imu_J, double* prior_r);

/* =============================================================================================
 * FE — FeatureTracker::readImage()  (feature_tracker/src/feature_tracker.cpp:81-167)
 *
 * The handle holds `n_cams` independent camera streams (trackerData[NUM_OF_CAM] in
 * feature_tracker_node.cpp:21; also used as the batch dimension of BASELINE.json configs[1]).  Per stream the
 * device keeps the pyramids of the previous and the current frame (cur_img / forw_img of feature_tracker.h:52).
 *
 *   vg_fe_push_frames   <- `forw_img = img` incl. the optional CLAHE (:87-104)  + the pyramid build that
 *                          cv::calcOpticalFlowPyrLK does internally; the former current frame becomes previous
 *   vg_fe_track         <- cv::calcOpticalFlowPyrLK(cur_img, forw_img, cur_pts, forw_pts, status, err,
 *                          cv::Size(21,21), 3)                                    (:113)
 *   vg_fe_detect        <- cv::goodFeaturesToTrack(forw_img, n_pts, max_corners, 0.01, MIN_DIST, mask)  (:149)
 *
 * Staged variants (*_upload / *_async / *_download) let a benchmark time the device work with inputs resident in HBM.
 * ============================================================================================= */
int vg_fe_configure(vg_handle* h, int width, int height, int n_cams, int max_points);
/* imgs[cam] = top-left pixel of an 8-bit single-channel frame with row stride `stride` bytes; every stream needs a frame
 * (the batched streams advance together: a NULL entry is VG_ERR_BAD_ARG and leaves the device state untouched).  equalize != 0 applies CLAHE(3.0, 8x8) first (EQUALIZE of feature_tracker/src/parameters.cpp:59). */
int vg_fe_push_frames(vg_handle* h, const uint8_t* const* imgs, int stride, int equalize);
int vg_fe_upload_frames(vg_handle* h, const uint8_t* const* imgs, int stride);     /* H2D only            */
int vg_fe_build_async(vg_handle* h, int equalize);                                 /* CLAHE + pyramids    */
/* Two device-resident frame slots, one per pyramid set.  upload_frames fills the slot of the set the NEXT build will fill and
 * selects it; a frame that is not equalized then IS level 0 of its pyramid (no copy).  Consequence: after upload_frames the
 * older of the two pyramids is incomplete until build_async has run — upload, build, then track (push_frames does the first
 * two).  frame_slot returns the selected slot; select_frames re-selects a slot that was uploaded earlier (benchmarks alternate
 * between two resident frames; building from the slot the current pyramid already uses falls back to a copy). */
int vg_fe_frame_slot(vg_handle* h);
int vg_fe_select_frames(vg_handle* h, int slot);
/* Pyramidal LK from the previous to the current frame of stream `cam`.  prev_xy / next_xy are (x, y) float pairs.
 * status / err have OpenCV's meaning (the inBorder() filter of feature_tracker.cpp:115-117 is the caller's). */
int vg_fe_track(vg_handle* h, int cam, const float* prev_xy, int n, float* next_xy, uint8_t* status, float* err);
int vg_fe_track_upload(vg_handle* h, const float* prev_xy /* [n_cams][max_points][2] */, const int* n /* [n_cams] */);
int vg_fe_track_async(vg_handle* h);
int vg_fe_track_download(vg_handle* h, float* next_xy, uint8_t* status, float* err);
/* Shi-Tomasi corners of the CURRENT frame of stream `cam`; mask is height x width (0 = excluded) or NULL.
 * out_xy must hold max_corners pairs; corners are integer pixel positions in acceptance order. */
int vg_fe_detect(vg_handle* h, int cam, const uint8_t* mask, int max_corners, double quality, double min_dist,
                 float* out_xy, int* out_n);
int vg_fe_detect_upload(vg_handle* h, const uint8_t* const* masks /* per cam or NULL */, const int* max_corners);
int vg_fe_detect_async(vg_handle* h, double quality, double min_dist);
int vg_fe_detect_download(vg_handle* h, float* out_xy /* [n_cams][max_points][2] */, int* out_n /* [n_cams] */);
/* FeatureTracker::setMask() (feature_tracker.cpp:36-69) for all streams: the points of stream c
 * (pts_xy[c][i], track_cnt[c][i], i < n[c]; arrays are [n_cams][max_points]) are visited by track_cnt descending
 * (stable), a point is kept iff the mask at its rounded position is still 255, and every kept point blanks the filled
 * disc of `radius` (MIN_DIST) around it.  base_masks[c] = the FISHEYE mask (:38-41) or NULL (all 255); base_masks may
 * be NULL.  kept_index[c][k] = index of the k-th kept point, n_kept[c] their number.  The final mask stays on the
 * device as the mask of stream c for vg_fe_detect_masked(). */
int vg_fe_set_mask(vg_handle* h, const float* pts_xy, const int* track_cnt, const int* n, const uint8_t* const* base_masks,
                   int radius, int* kept_index, int* n_kept);
/* cv::goodFeaturesToTrack(forw_img, n_pts, max_corners, quality, min_dist, mask) (:149) with the mask left on the
 * device by vg_fe_set_mask: no mask upload */
int vg_fe_detect_masked(vg_handle* h, int cam, int max_corners, double quality, double min_dist, float* out_xy, int* out_n);
/* FeatureTracker::undistortedPoints() lifting (:258-271): PinholeCamera::liftProjective with the 8-step recursive
 * distortion model (camera_model PinholeCamera.cc:450-510, :646-661).  intr = fx fy cx cy k1 k2 p1 p2; out = (x/z, y/z)
 * as float (cv::Point2f).  The same as vg_fe_lift with a VG_CAM_PINHOLE camera of these eight numbers. */
int vg_fe_undistort(vg_handle* h, const float* pts_xy, int n, const double* intr, float* out_xy);
/* ---- Camera models (added within ABI 12).  The models whose liftProjective runs on the device, in double.  The first two in the
 * reference's expression order (bit-identical to camodocal's):
 *   VG_CAM_PINHOLE  PinholeCamera (PinholeCamera.cc:450-510): what vg_fe_frame_in::intr and vg_fe_undistort describe
 *   VG_CAM_MEI      CataCamera, the unified model (CataCamera.cc:556-626): the pinhole lift with gamma1 gamma2 u0 v0, then
 *                   z = 1 - xi (rho2 + 1) / (xi + sqrt(1 + (1 - xi^2) rho2)), or (1 - rho2) / 2 when xi == 1.0
 *   VG_CAM_KANNALA_BRANDT  EquidistantCamera, the equidistant fisheye (EquidistantCamera.cc:427-442, :715-818); p = mu mv u0 v0 k2 k3
 *                   k4 k5, xi is ignored.  With (ux, uy) = ((1 / mu) px - u0 / mu, (1 / mv) py - v0 / mv) and r = |(ux, uy)|, theta is
 *                   the root of theta + k2 theta^3 + k3 theta^5 + k4 theta^7 + k5 theta^9 = r that 10 Newton steps from theta = r
 *                   reach (a fixed count; polynomial and derivative by Horner in theta^2), and the ray is (sin theta ux / r,
 *                   sin theta uy / r, cos theta) -- (sin theta, 0, cos theta) when r < 1e-10 -- with the library's own sine and cosine
 *                   (a Cody-Waite reduction by pi / 2 and Taylor polynomials, absolute error about 1e-16): emulated kernels, device and
 *                   host class give the same bits.  The reference finds theta as the smallest non-negative real eigenvalue of the
 *                   polynomial's companion matrix: the same number (to about 1e-14) wherever r(theta) is monotone up to the pixel, and
 *                   (float)(x / z), (float)(y / z) then equal camodocal's up to a float ulp (tests/test_fe_kb_definition.py).  What it is
 *                   NOT: for a pixel beyond the first maximum of r(theta), or one for which the reference finds no admissible root, the
 *                   reference returns another branch's root or r itself; this function returns whatever Newton reaches.  Such pixels lie
 *                   outside the calibrated image circle; the settings the reference ships (config/tum, config/cla,
 *                   config/realsense/realsense_fisheye) have none inside their frames.
 * The value 2 is no model.  SCARAMUZZA is not offered. */
#define VG_CAM_PINHOLE 0
#define VG_CAM_MEI     1
#define VG_CAM_KANNALA_BRANDT 3
typedef struct vg_fe_camera {
    int struct_size;             /* sizeof(vg_fe_camera) */
    int model;                   /* VG_CAM_* */
    double p[8];                 /* PINHOLE: fx fy cx cy k1 k2 p1 p2;  MEI: gamma1 gamma2 u0 v0 k1 k2 p1 p2;  KANNALA_BRANDT: mu mv u0 v0 k2 k3 k4 k5 */
    double xi;                   /* MEI: mirror_parameters.xi; ignored for PINHOLE and KANNALA_BRANDT */
} vg_fe_camera;
/* Set the camera of stream `cam` of a configured handle: from then on vg_fe_read_image / vg_fe_read_image_batch lift that stream's
 * points with it (rejectWithF's two point sets and undistortedPoints' list) and ignore vg_fe_frame_in::intr for that stream.
 * camera == NULL returns the stream to "pinhole from intr"; vg_fe_configure clears every stream's camera; a stream that never had a
 * camera set behaves as it always did.  Refused with VG_ERR_BAD_ARG before anything is touched (the stream keeps the camera it had;
 * vg_last_error says why): a wrong struct_size, an unknown model, cam outside [0, n_cams), a handle that is not configured, a
 * non-finite parameter, p[0] or p[1] zero.  No device work, no allocation: the camera travels with the next frame's one upload. */
int vg_fe_set_camera(vg_handle* h, int cam, const vg_fe_camera* camera);
/* vg_fe_undistort for any model: out = ((float)(x / z), (float)(y / z)) of `camera`'s liftProjective for n points, n at most
 * n_cams * max_points of vg_fe_configure.  Independent of the streams' cameras.  The same refusals as vg_fe_set_camera. */
int vg_fe_lift(vg_handle* h, const vg_fe_camera* camera, const float* pts_xy, int n, float* out_xy);
/* FeatureTracker::rejectWithF() (feature_tracker.cpp:169-202): cv::findFundamentalMat(un_cur_pts, un_forw_pts, FM_RANSAC,
 * threshold, 0.99, status) on n >= 8 correspondences given in the pixel coordinates of the virtual pinhole camera
 * (FOCAL_LENGTH * x/z + COL/2, ...).  Follows OpenCV 3.3's registrators as recalled (oracle/ASSUMPTIONS.md F9): cv::RNG((uint64)-1)
 * sample schedule, 7-point solver, error = max of the two squared point-to-epipolar-line distances (float) <= threshold^2, adaptive
 * iteration bound, LMedS instead of RANSAC below 15 points.  status[i] = 1 for the inliers of the winning model; if no model is
 * found every status is 1 (nothing is rejected).  n_inliers / F_out (row-major 3x3, F33 = 1) may be NULL.  A pure function of the
 * input.  SURVEY.md 8(f) row 3. */
int vg_fe_reject_with_f(vg_handle* h, const float* cur_un_xy, const float* forw_un_xy, int n, double threshold, uint8_t* status,
                        int* n_inliers, double* F_out);
/* debugging / parity taps: copy a pyramid level of the current (which = 0) or previous (1) frame, or the
 * min-eigenvalue map of the last detect, to host memory.  The map (cv::cornerMinEigenVal inside cv::goodFeaturesToTrack,
 * feature_tracker.cpp:149) is an on-chip intermediate of the detection: vg_fe_keep_eig(h, 1) makes every FOLLOWING detection
 * write it to device memory as well (4 bytes per pixel and stream, allocated at that call); vg_fe_get_eig without it is
 * VG_ERR_BAD_ARG. */
int vg_fe_get_level(vg_handle* h, int cam, int which, int level, uint8_t* out, int* w, int* hgt);
int vg_fe_keep_eig(vg_handle* h, int on);
int vg_fe_get_eig(vg_handle* h, int cam, float* out);
int vg_fe_get_mask(vg_handle* h, int cam, uint8_t* out);          /* current device mask of the stream */

/* ---- One call per frame (ABI 11): FeatureTracker::readImage() of ONE stream (a handle configured with n_cams == 1) from `forw_img = img`
 * to undistortedPoints(), feature_tracker.cpp:81-167, without the host between the steps:
 *   upload (frame + cur_pts, one block) -> CLAHE -> pyramid -> calcOpticalFlowPyrLK -> status && inBorder -> reduceVector
 *   publish:      -> liftProjective of both point sets -> findFundamentalMat (RANSAC; sample schedule and iteration bounds resident on the
 *                    device) -> reduceVector -> [status download, `order` callback, order upload] -> setMask walk -> goodFeaturesToTrack
 *                    with MAX_CNT - kept corners -> addPoints -> liftProjective of the final list -> ONE download
 *   not publish:  -> liftProjective of the survivors -> ONE download
 * The one thing a published frame still asks the host in the middle is the ORDER of setMask's walk: the reference sorts by track_cnt with
 * std::sort (:48), which is not stable -- the order among equal counts is whatever the platform's sort makes of the sequence, so the
 * caller's own std::sort call decides it (feature_tracker_readimage.cpp passes a callback that runs the reference's sort).  order == NULL:
 * the list is walked as it stands -- which IS the stable order by count for a caller that keeps the reference's list discipline (kept
 * points in walk order, then new points with count 1: the counts are then non-increasing along the list at all times).
 * Two cases go back to the host inside the call (same results, more round trips): 8 <= survivors < 15 (findFundamentalMat switches to
 * LMedS) and a RANSAC sample OpenCV would have redrawn for collinearity (its schedule then depends on the points).
 * All pointers of vg_fe_frame_out point into pinned buffers of the handle and stay valid until the next vg_fe_* call on it.
 * This call IS vg_fe_read_image_batch (below) with one stream: one implementation, one resident state per handle, so the two calls may
 * be mixed on a handle with n_cams == 1.  What it keeps of its own: img == NULL is VG_ERR_BAD_ARG (the batch reads that as "the resident
 * frames"), a handle with n_cams != 1 is VG_ERR_UNSUPPORTED, and all 1000 RANSAC iterations are evaluated in one launch per step.
 * The FIRST call on a handle builds its resident tables: the RANSAC schedules for every point count up to max_points (28 KB each, tens
 * of milliseconds of host time once) and the per-stream tables of the batch (about 0.45 MB of device memory per stream: the models,
 * inlier counts and inlier sets of all iterations; a few tens of KB before the two calls were one).  Limits: n_cams == 1,
 * max_points <= 2048, rejectWithF on at most 1024 tracking survivors. */
typedef struct vg_fe_frame_out {
    int n1;                      /* survivors of tracking + border test                                           (:115-124) */
    int n2;                      /* survivors of rejectWithF (== n1 when it did not run)                          (:193-198) */
    int ransac_ran;              /* publish && n1 >= 8                                                            (:171)     */
    int n_kept, n_new;           /* setMask's survivors, new corners (publish only)                               (:64, :149) */
    int n_final;                 /* length of the list the frame ends with: n_kept + n_new, or n1 when not published          */
    const uint8_t* status_lk;    /* [n]   calcOpticalFlowPyrLK status && inBorder(forw_pts[i])                               */
    const uint8_t* status_f;     /* [n1]  findFundamentalMat's mask over the tracking survivors (ransac_ran only)            */
    const float* forw_xy;        /* [n][2] tracked position of every input point                                             */
    const int* kept;             /* [n_kept] positions IN THE WALK ORDER of the points setMask kept                          */
    const float* new_xy;         /* [n_new][2] goodFeaturesToTrack's corners                                                 */
    const float* un_xy;          /* [n_final][2] liftProjective (x/z, y/z) of the final list: kept points in walk order, then new ones */
    int ransac_best, ransac_niters, fallback;   /* diagnostics: winning iteration, iterations that counted, RI_FB_* bits that sent the
                                                   estimate back to the host                                                 */
} vg_fe_frame_out;
/* called once per published frame after rejectWithF: `after` holds n1, n2, status_lk, status_f, forw_xy; write the walk order into
 * order[0 .. n2) as indices into the list of the n2 survivors (a permutation); return 0 (anything else aborts the frame with
 * VG_ERR_BAD_ARG).
 * Failure semantics (ABI 12): every error that follows from the arguments alone -- sizes, a point list without a previous frame -- is
 * returned BEFORE the frame is uploaded: the stream is untouched.  An error after that (the callback's, a detection overflow, a HIP
 * error) leaves the device stream one frame ahead of the caller; the callback must therefore not change the caller's own state
 * (work on copies, apply the statuses after VG_OK -- host/dropin/feature_tracker_readimage.cpp), and the caller re-starts the stream
 * (vg_fe_configure) before it tracks again. */
typedef int (*vg_fe_order_fn)(void* user, const vg_fe_frame_out* after, int* order);
typedef struct vg_fe_frame_in {
    int struct_size;             /* sizeof(vg_fe_frame_in) */
    const uint8_t* img;          /* the frame, width x height of vg_fe_configure */
    int stride;                  /* bytes per row */
    int equalize;                /* EQUALIZE */
    int publish;                 /* PUB_THIS_FRAME */
    const float* cur_xy;         /* [n][2] cur_pts */
    int n;
    int max_cnt;                 /* MAX_CNT  (<= max_points of vg_fe_configure) */
    int min_dist;                /* MIN_DIST */
    double quality;              /* goodFeaturesToTrack qualityLevel: 0.01 at :149 */
    double f_threshold;          /* F_THRESHOLD */
    double focal_length;         /* FOCAL_LENGTH (rejectWithF's virtual camera, :178) */
    double intr[8];              /* PinholeCamera: fx fy cx cy k1 k2 p1 p2 (ignored for a stream with a vg_fe_set_camera camera) */
    const uint8_t* base_mask;    /* fisheye_mask (height x width, contiguous) or NULL; uploaded when the pointer changes */
    vg_fe_order_fn order;        /* or NULL */
    void* user;
} vg_fe_frame_in;
int vg_fe_read_image(vg_handle* h, const vg_fe_frame_in* in, vg_fe_frame_out* out);

/* ---- The same for EVERY stream of a handle in one call (added within ABI 12): readImage of in[c] for stream c of a handle configured
 * with n_cams == n_streams (any other n_streams: VG_ERR_BAD_ARG; the batched streams advance together), out[c] with exactly the
 * meaning, the values and the lifetime of the single call's result for that stream -- the single call is this one with n_streams == 1.
 * One upload, one launch per step over all streams (tracking, image build, stamping and detection are indexed by stream; the steps
 * between them run one workgroup per stream; with more than one stream the RANSAC runs in two parts around the iteration bookkeeping
 * instead of 1000 iterations per stream), one download after rejectWithF, one after the detection.  When to use which: one camera ->
 * vg_fe_read_image (lowest latency: one launch per RANSAC step); many cameras or many sequences replayed together -> one handle with
 * n_cams streams and this call.
 *   per stream  (from in[c]):  img / stride, cur_xy / n, publish, max_cnt, intr, focal_length, f_threshold, base_mask, order / user.
 *               Streams that publish and streams that do not may be mixed; one that does not costs the detection an early exit.
 *               The camera is per stream too (vg_fe_set_camera, else the pinhole of in[c].intr): streams of different models may
 *               be mixed in one call.
 *   uniform     equalize over all streams; quality and min_dist over the streams that publish (the batched image build and the
 *               detection take ONE value each): a call that mixes them is VG_ERR_BAD_ARG.
 *   frames      every in[c].img NULL: the frames are the ones the last vg_fe_upload_frames put into the selected slot (nothing is
 *               uploaded; benchmarks time the device work this way).  Some NULL, some not: VG_ERR_BAD_ARG.
 *   walk order  after rejectWithF of all streams ONE download, then the `order` callbacks on the calling thread in ascending stream
 *               order (streams that publish, have n2 > 0 and a callback), then ONE upload of all orders.
 *   host cases  8 <= survivors < 15 (LMedS) and a sample OpenCV would have redrawn go back to the host per stream.
 * Failure semantics as for the single call: everything that follows from the arguments alone (sizes, a point list on a handle without
 * a previous frame, mixed uniform fields, n_streams, frames for some streams only) is refused BEFORE any frame is uploaded and no stream
 * has moved; an error after that (a callback's, a detection overflow, a HIP error) leaves ALL streams one frame ahead of the caller,
 * who re-starts them with vg_fe_configure.  Limits: max_points <= 2048, rejectWithF on at most 1024 tracking survivors per stream;
 * the first call allocates the per-stream tables (about 0.45 MB of device memory per stream). */
int vg_fe_read_image_batch(vg_handle* h, int n_streams, const vg_fe_frame_in* in /* [n_streams] */, vg_fe_frame_out* out /* [n_streams] */);

/* ---- Track lists resident on the device (added within ABI 12, nothing existing changed).  vg_fe_read_image_batch takes cur_pts from
 * the host every frame and leaves the bookkeeping of FeatureTracker to every caller: ids / track_cnt and reduceVector over them
 * (feature_tracker.cpp:118-128, :193-198), setMask's re-ordering (:55-68), addPoints (:71-79), updateID (:204-214, driven from
 * feature_tracker_node.cpp:103-111), prev_un_pts_map / pts_velocity (:272-305) and the message filter track_cnt > 1
 * (feature_tracker_node.cpp:133-150).  These calls keep all of that on the device, per stream:
 *   n, cur_xy[n] (cur_pts), ids[n] (all >= 0 between two frames), track_cnt[n], un_xy[n] (cur_un_pts), in_map[n] (the point is in
 *   prev_un_pts_map under its own id), n_id, prev_time
 * and a frame returns what the estimator consumes: per feature  id, x, y, z, u, v, vx, vy.
 * IDS ARE PER STREAM: every stream counts its own n_id from 0, as a node with NUM_OF_CAM == 1 does.  The reference's process-wide static
 * FeatureTracker::n_id, interleaved over the cameras of one node, is NOT reproduced.
 * The state is allocated by the first vg_fe_tracks_begin (capacity max_points per stream); vg_fe_configure drops it.
 *
 * vg_fe_tracks_begin   every stream: an empty list, n_id = 0, no previous map.  Also the restart after a failed step.
 * vg_fe_tracks_step    one frame for every stream: the frame of vg_fe_read_image_batch (image build, calcOpticalFlowPyrLK, rejectWithF,
 *                      setMask, goodFeaturesToTrack, liftProjective -- the same kernels) with cur_pts read from the resident list, then
 *                      ONE kernel that commits the frame: reduceVector / the walk order / addPoints over ids and counts, track_cnt + 1,
 *                      pts_velocity, updateID, and the message.  The upload carries the control block and the cameras only.
 *     velocity (:272-305)  a carried point whose in_map was set: v = (float)((double)(un - prev_un) / (stamp - prev_time)) per
 *                      component (float difference, double division, as the reference's Point2f arithmetic); every other point (0, 0).
 *                      Points detected in a frame enter the reference's map under the key -1 (the map is built BEFORE updateID), so
 *                      they are not found one frame later: in_map = (id != -1) before this frame's ids are assigned.  stamp ==
 *                      prev_time gives what IEEE gives.
 *     message          entries with track_cnt > 1, ascending by id: msg_id[n_msg], msg_obs[n_msg][7] = x y 1.0 u v vx vy (the floats
 *                      widened to double as estimator_node.cpp widens them): vg_ba_frame::feature_id / obs may point straight at them.
 *   The rules of vg_fe_read_image_batch carry over: equalize uniform; quality / min_dist uniform over the streams that publish; img of
 *   all streams or of none (the resident frames); n_streams == n_cams; cameras per stream (vg_fe_set_camera, else the pinhole of
 *   intr); the LMedS range and a redrawn sample finish on the host.
 *   walk order  `order` (optional) receives the incremented counts of the n2 survivors of rejectWithF in list order -- the keys setMask
 *               sorts by -- and writes a permutation of [0, n2); it runs on the calling thread, streams in ascending order; anything
 *               but 0 aborts the step with VG_ERR_BAD_ARG, as does an order that is no permutation.  NULL walks the list as it stands:
 *               the counts of a resident list are non-increasing along the list between two frames (kept points in walk order, then
 *               new ones with count 1), so that IS the stable order by count.  The reference's std::sort is not stable: a caller
 *               that must reproduce one platform's order among equal counts passes its own sort here.
 *   failure     VG_ERR_BAD_ARG before anything is uploaded, no stream moved: a step without vg_fe_tracks_begin, a wrong struct_size,
 *               mixed uniform fields, frames for some streams only, n_streams != n_cams, max_cnt > max_points, a non-empty list on a
 *               handle without a previous frame.  An error after the upload (a callback's, a detection overflow, a HIP error) leaves
 *               every LIST exactly as it was (the commit kernel runs last and writes a second copy) but the FRAMES one ahead: restart
 *               with vg_fe_tracks_begin or vg_fe_configure.
 *   do not mix  a vg_fe_read_image* / vg_fe_push_frames call between two steps moves the frames but not the lists.
 *   All pointers of vg_fe_tracks_out point into pinned buffers of the handle and stay valid until the next vg_fe_* call on it.
 * vg_fe_tracks_get / vg_fe_tracks_set   export and re-seed of ONE stream between two frames; the other streams stay where they are.
 *   get: arrays of capacity max_points, any of them may be NULL.  set: n <= max_points; ids distinct and >= 0 and n_id greater than
 *   every id, else VG_ERR_BAD_ARG; un_xy == NULL: no previous map (in_map is ignored, the next frame's velocities are 0); with un_xy,
 *   in_map is required. */
typedef int (*vg_fe_tracks_order_fn)(void* user, int stream, int n2, const int* track_cnt /* [n2] */, int* order /* [n2] */);
typedef struct vg_fe_tracks_in {
    int struct_size;             /* sizeof(vg_fe_tracks_in) */
    const uint8_t* img;          /* as vg_fe_frame_in, without cur_xy / n */
    int stride;
    int equalize;
    int publish;
    int max_cnt;
    int min_dist;
    double quality;
    double f_threshold;
    double focal_length;
    double intr[8];
    const uint8_t* base_mask;
    vg_fe_tracks_order_fn order; /* or NULL */
    void* user;
    double stamp;                /* _cur_time of readImage */
} vg_fe_tracks_in;
typedef struct vg_fe_tracks_out {
    int n;                       /* the list the frame ends with, after updateID */
    int n_id;
    int n_msg;
    int n1, n2, ransac_ran, n_kept, n_new, fallback, ransac_best, ransac_niters;   /* as vg_fe_frame_out */
    const int* ids;              /* [n] */
    const int* track_cnt;        /* [n] */
    const float* cur_xy;         /* [n][2] */
    const float* un_xy;          /* [n][2] */
    const float* vel_xy;         /* [n][2] pts_velocity */
    const int* msg_id;           /* [n_msg] ascending */
    const double* msg_obs;       /* [n_msg][7] x y 1.0 u v vx vy */
} vg_fe_tracks_out;
typedef struct vg_fe_tracks_state {
    int struct_size;             /* sizeof(vg_fe_tracks_state) */
    int n;
    int n_id;
    double prev_time;
    float* cur_xy;               /* [n][2] */
    int* ids;                    /* [n] */
    int* track_cnt;              /* [n] */
    float* un_xy;                /* [n][2] */
    uint8_t* in_map;             /* [n] */
} vg_fe_tracks_state;
int vg_fe_tracks_begin(vg_handle* h);
int vg_fe_tracks_step(vg_handle* h, int n_streams, const vg_fe_tracks_in* in /* [n_streams] */, vg_fe_tracks_out* out /* [n_streams] */);
int vg_fe_tracks_get(vg_handle* h, int cam, vg_fe_tracks_state* state);
int vg_fe_tracks_set(vg_handle* h, int cam, const vg_fe_tracks_state* state);

/* ---- Front end feeds resident sequences on the device: one call per frame (added within ABI 12, nothing existing changed) -----------
 * vg_fe_tracks_step builds the estimator's message (msg_id / msg_obs) in HBM and vg_ba_seq_step_imu_async reads a frame's observations
 * from HBM; between the two calls the message travels to the pinned mirror, through the caller and up again.  These calls join the two on
 * ONE handle that runs n_cams camera + IMU streams, stream c feeding window c: images and IMU samples go up, states come down, the tracks
 * and the observations stay on the device.
 *
 * vg_vio_begin       needs, else VG_ERR_BAD_ARG with a vg_last_error text: resident lists begun (vg_fe_tracks_begin); a running sequence
 *                    in IMU mode (vg_ba_seq_begin + vg_ba_seq_imu_begin) on the same handle; n_cams == nwin; max_points <=
 *                    vg_ba_seq_config::max_new_obs; flags of VG_VIO_*.  The lists may hold tracks and the windows a seeded state -- the
 *                    normal case: the caller runs the first K-1 frames through vg_fe_tracks_step, initialises from the collected
 *                    messages (vg_init_exrot while estimate_extrinsic is 2, then vg_init_relpose, vg_init_sfm and vg_init_align, each
 *                    one call for all windows), seeds the sequence from the result and switches to vg_vio_step_async
 *                    (the ids stay consistent because the list is resident).
 * vg_vio_step_async  one frame for every stream.  The frame of vg_fe_tracks_step (same kernels, same host finish of RANSAC and
 *                    detection); fe.publish must be uniform over the streams of one call.  On a frame that publishes, one kernel
 *                    (ba_seq_bridge_kernel) moves every stream's message from the commit kernel's output into the staging
 *                    ba_seq_add_kernel reads, and the step of vg_ba_seq_step_imu_async follows; only the samples and their counts are
 *                    uploaded.  On a frame that does not publish only the front end runs and n_samples must be 0: the caller keeps
 *                    accumulating samples until the next published frame.
 *                    out[c].fe: the counts of vg_fe_tracks_out; its array pointers are NULL unless the bridge was begun with
 *                    VG_VIO_LISTS -- without it the download after the commit kernel carries the header block only, neither the lists
 *                    nor the message.
 *   refused with VG_ERR_BAD_ARG before anything is uploaded or launched (no stream and no window moves): no bridge; struct_size; n
 *                    other than n_cams; mixed publish; n_samples outside 1 .. max_samples on a frame that publishes or not 0 on one
 *                    that does not; samples NULL; a sample that is not finite; everything vg_fe_tracks_step refuses.
 *   failure after the front end's upload (a callback's, a detection overflow): the estimator part is NOT launched, the windows stay;
 *                    the lists behave as vg_fe_tracks_step documents.
 *   States come back as before: vg_ba_batch_download_state, vg_ba_seq_info.
 * vg_vio_get_frame   parity tap: what the last publishing step staged for one window -- n_obs, ids, rows of 7 doubles -- read from the
 *                    sequence's staging buffers on the device; arrays of capacity cap (either may be NULL).
 * vg_vio_end         ends the bridge; lists and sequence go on.
 * Mixing: vg_fe_tracks_step and vg_ba_seq_step_imu_async stay legal between two vg_vio_step_async calls (the same state).
 * vg_ba_seq_end, vg_ba_seq_begin, vg_ba_seq_imu_begin (it replaces the staging and may change max_samples), vg_fe_configure and
 * vg_fe_tracks_begin end the bridge: a later vg_vio_step_async is refused until vg_vio_begin is called again.
 * Relocalisation: a publishing vg_vio_step_async honours a window armed with vg_ba_seq_set_relo (it shares the step: the request
 * travels in the sample block's header); a frame that does not publish leaves the request armed for the next one that does. */
typedef struct vg_vio_in {
    int struct_size;             /* sizeof(vg_vio_in)                                                                          */
    int n_samples;               /* IMU rows since the previous PUBLISHED frame, as estimator_node's getMeasurements pairs them */
    const double* samples;       /* n_samples x 7: dt acc gyr                                                                  */
    vg_fe_tracks_in fe;          /* exactly what vg_fe_tracks_step takes for this stream                                       */
} vg_vio_in;
typedef struct vg_vio_out {
    vg_fe_tracks_out fe;         /* counts; the array pointers are NULL unless VG_VIO_LISTS                                    */
} vg_vio_out;
enum { VG_VIO_LISTS = 1 };
int vg_vio_begin(vg_handle* h, int flags);
int vg_vio_step_async(vg_handle* h, int n, const vg_vio_in* in /* [n] */, vg_vio_out* out /* [n] */);
int vg_vio_get_frame(vg_handle* h, int window, int cap, int* n_obs, int* feature_id, double* obs7);
int vg_vio_end(vg_handle* h);

/* ---- Loop closure: keyframe BRIEF descriptors and matching (added within ABI 12, nothing existing changed) ----------------------------
 * The integer-exact, batchable part of the pose graph's KeyFrame (pose_graph/src/keyframe.cpp): computeWindowBRIEFPoint and
 * computeBRIEFPoint with keypoints_norm (vg_kf_add), searchByBRIEFDes with the reduceVector step of findConnection:301-312
 * (vg_kf_match).  PnPRANSAC and the loop_info arithmetic behind it are vg_kf_pnp (the next block), DBoW2 loop detection is vg_kf_loop_detect (the
 * block after it).  NOT here: the 4-DoF
 * pose-graph optimisation, thumbnails and debug images.  Independent of vg_fe_configure: the pose graph's image is not the front
 * end's current frame.
 *
 * DVision::BRIEF is read from the reference as the definition.  cv::GaussianBlur and cv::FAST are RECALLED, NOT PINNED (no OpenCV to
 * compare with; SURVEY.md Appendix B.6 and DESIGN.md section 4 list them).  Everything is integer or float32-exact:
 *   blur    cv::GaussianBlur(img, im, Size(9, 9), 2, 2) on CV_8UC1, BORDER_REFLECT_101, as OpenCV's fixed-point separable path:
 *           taps k = 7 17 32 46 52 46 32 17 7 (sum 256), out(x, y) = (sum_j k_j (sum_i k_i p(x + i - 4, y + j - 4)) + 32768) >> 16,
 *           indices reflected without repeating the edge pixel (-1 -> 1, W -> W - 2)
 *   FAST    cv::FAST(image, keypoints, 20, true) on the image that is NOT blurred.  Ring (dx, dy) clockwise from the top: (0,-3) (1,-3)
 *           (2,-2) (3,-1) (3,0) (3,1) (2,2) (1,3) (0,3) (-1,3) (-2,2) (-3,1) (-3,0) (-3,-1) (-2,-2) (-1,-3); d_k = v - ring_k; A = max
 *           over the 16 arcs of 9 contiguous ring pixels of min d_k, B the same for -d_k.  A pixel with 3 <= x < W - 3, 3 <= y < H - 3
 *           is a corner iff max(A, B) > 20, its score max(A, B) - 1 (cornerScore<16> of a pixel that passed); every other pixel scores
 *           0.  Kept iff the score is strictly greater than each of its 8 neighbours'.  Listed row-major (y, then x), pt = (float x,
 *           float y), the score as the response.  The ORDER is part of the result: the match breaks ties by index.
 *   BRIEF   DVision::BRIEF::compute (BRIEF.cpp:39-106) with the 256 tests of `pattern` on the blurred image: x1 = (int)(pt.x +
 *           (float)pattern_x1[i]) (a float32 add, truncation toward zero: a coordinate in (-1, 0) is 0 and inside), likewise y1 x2 y2; bit
 *           i = all four inside the image && im(y1, x1) < im(y2, x2).  A descriptor is 4 little-endian 64-bit words, bit i in word i / 64
 *           at position i % 64.
 *   lift    keypoints_norm = vg_fe_lift of the entry's camera on the keypoints.
 *   match   searchInAera: for window descriptor w the smallest (Hamming distance, index) among the old record's descriptors with
 *           distance < 128: best_dist, best_idx (128, -1: none); status = best_idx >= 0 && best_dist < 80; matched_2d_old(_norm) = the
 *           old pt / norm at best_idx where status, else (0, 0).  The compacted lists are the status-1 entries in window order.
 *
 * vg_kf_configure  allocates n_slots resident keyframe records: max_keypoints x (descriptor, pt, norm, score), max_window_points x
 *                  (descriptor, pt), the counts.  pattern: int16[4][256] = x1 y1 x2 y2.  Calling it again replaces everything.
 *                  Refused: width or height < 7, max_keypoints outside 1 .. VG_KF_MAX_KEYPOINTS, max_window_points outside 1 ..
 *                  VG_KF_MAX_WINDOW, n_slots < 1, pattern NULL or an offset outside +-127.
 * vg_kf_add        n keyframes in one call: one upload (images, cameras, window points), seven launches over the batch, one download.
 *                  A frame with more than max_keypoints corners keeps the first max_keypoints in row-major order, reports the true
 *                  count in n_keypoints and status VG_KF_TRUNCATED (the reference has no cap).  The output arrays are optional
 *                  (NULL: not copied); their capacities are max_keypoints / max_window_points.
 * vg_kf_get / set  download a record / upload one whole (the KeyFrame constructor of loadPoseGraph).  vg_kf_get fills the counts and the
 *                  arrays whose pointers are non-NULL; vg_kf_set takes every array of a non-zero count.
 * vg_kf_match      n_pairs of (current slot, old slot), pairs may share slots: the current record's window descriptors against the old
 *                  record's keypoint descriptors.  An old record without keypoints gives all-zero status.  One launch, one download.
 * Refused with VG_ERR_BAD_ARG before anything is touched (vg_last_error says why): a handle without vg_kf_configure, a wrong struct_size,
 * a slot out of range or (get, match) never filled, the same slot twice in one vg_kf_add, n_window or a count of vg_kf_set above its
 * capacity, a NULL image, stride < width, a NULL table of a non-zero count, a camera vg_fe_set_camera would refuse. */
#define VG_KF_MAX_KEYPOINTS 65535    /* the match key is (distance << 16) | index */
#define VG_KF_MAX_WINDOW 1024
#define VG_KF_OK 0
#define VG_KF_TRUNCATED 1
#define VG_KF_ADD_LAUNCHES 7         /* blur, FAST score, non-max masks, scan, scatter, lift, BRIEF */
typedef struct vg_kf_in {
    int struct_size;             /* sizeof(vg_kf_in) */
    int slot;
    const uint8_t* img;          /* height rows of width raw 8-bit pixels, `stride` bytes apart */
    int stride;
    int n_window;                /* point_2d_uv.size() */
    const float* window_xy;      /* n_window x 2: point_2d_uv */
    vg_fe_camera camera;         /* m_camera of keypoints_norm */
} vg_kf_in;
typedef struct vg_kf_out {
    int struct_size;             /* sizeof(vg_kf_out) */
    int n_keypoints;             /* corners cv::FAST lists: the TRUE count, the record keeps min(n_keypoints, max_keypoints) */
    int status;                  /* VG_KF_OK / VG_KF_TRUNCATED */
    int n_kept;
    float* keypoints_xy;         /* [max_keypoints][2] or NULL */
    uint8_t* scores;             /* [max_keypoints] */
    float* norm_xy;              /* [max_keypoints][2] */
    uint64_t* descriptors;       /* [max_keypoints][4] */
    uint64_t* window_descriptors;/* [max_window_points][4] */
    float* device_ms;            /* out[0] only: VG_KF_ADD_LAUNCHES event intervals of the batch, or NULL */
} vg_kf_out;
typedef struct vg_kf_record {
    int struct_size;             /* sizeof(vg_kf_record) */
    int n_keypoints, n_window;   /* what the record holds */
    int n_true;                  /* corners before the cap (vg_kf_set: 0 means n_keypoints) */
    float* keypoints_xy;
    uint8_t* scores;
    float* norm_xy;
    uint64_t* descriptors;
    float* window_xy;
    uint64_t* window_descriptors;
} vg_kf_record;
typedef struct vg_kf_pair {
    int struct_size;             /* sizeof(vg_kf_pair) */
    int cur_slot, old_slot;
} vg_kf_pair;
typedef struct vg_kf_match_out {
    int struct_size;             /* sizeof(vg_kf_match_out) */
    int n_window;                /* window points of the current record */
    int n_matched;               /* entries of the compacted lists; the caller compares it with MIN_LOOP_NUM */
    int* best_idx;               /* [max_window_points] each, or NULL */
    int* best_dist;
    uint8_t* status;
    float* matched_2d_old;       /* [..][2] */
    float* matched_2d_old_norm;  /* [..][2] */
    int* matched_index;          /* the surviving window indices, ascending: gathers matched_2d_cur, point_3d, point_id */
    float* matched_old_xy;       /* [..][2] compacted */
    float* matched_old_norm;     /* [..][2] compacted */
    float* device_ms;            /* out[0] only: the launch's event interval, or NULL */
} vg_kf_match_out;
int vg_kf_configure(vg_handle* h, int width, int height, int max_keypoints, int max_window_points, int n_slots, const int16_t* pattern);
int vg_kf_add(vg_handle* h, int n, const vg_kf_in* in /* [n] */, vg_kf_out* out /* [n] */);
int vg_kf_get(vg_handle* h, int slot, vg_kf_record* rec);
int vg_kf_set(vg_handle* h, int slot, const vg_kf_record* rec);
int vg_kf_match(vg_handle* h, int n_pairs, const vg_kf_pair* in /* [n_pairs] */, vg_kf_match_out* out /* [n_pairs] */);

/* ---- Loop closure: PnPRANSAC and findConnection's loop gate, batched (added within ABI 12, nothing existing changed) -------------------
 * What KeyFrame::findConnection runs between searchByBRIEFDes (vg_kf_match) and the lists it publishes (vg_ba_seq_set_relo):
 * KeyFrame::PnPRANSAC (pose_graph/src/keyframe.cpp:200-256), the second reduceVector round (:406-415) and the loop_info arithmetic
 * with its yaw / distance gate (:472-516), for n_pairs (current, old) pairs in one call.  Needs no vg_kf_configure; plain arrays in
 * and out.  Synchronous: one upload, VG_KF_PNP_LAUNCHES launches over the whole batch, one download.  A pair's status never touches
 * its neighbours; a batch equals the single calls bit for bit.
 *
 * cv::solvePnPRansac is third-party and not pinned here: everything below is RECALLED for OpenCV 3.3-era solvepnp.cpp / epnp.cpp /
 * ptsetreg.cpp, NOT PINNED.  Parts marked [FIXED] are this library's choice where the
 * recalled code leaves the result to rounding noise or to a general-purpose solver; [DEVIATION] where it knowingly differs.
 *  1 Camera   K = I, no distortion.  R_inital = (origin_vio_R qic)^-1 (3x3 inverse by cofactors over the determinant, as Eigen's),
 *             P_inital = -(R_inital (origin_vio_T + origin_vio_R tic)), rvec0 = Rodrigues(R_inital) (regular branch, as vg_init_sfm
 *             states it; the near-pi branch is VG_KF_PNP_NUMERIC).  They enter step 5 and the NO_MODEL case only.
 *  2 Registrator  5 model points.  Samples: cv::RNG((uint64)-1), five rng.uniform(0, n) per sample, an index already in the sample is
 *             redrawn; PnPRansacCallback has no checkSubset, so the schedule depends on n alone (no host fallback path).  At most
 *             max_iters iterations.  A model replaces the best one when its inlier count exceeds max(best, 4); then niters =
 *             RANSACUpdateNumIters(0.99, (n - good) / n, 5, niters).  Iterations at or beyond niters do not count.
 *  3 Error    of a model (rvec, tvec) at point i: R = Rodrigues(rvec); X = R P_i + tvec in double (P_i widened from float32);
 *             z = X[2] != 0 ? 1 / X[2] : 1; the projection (X[0] z, X[1] z) rounded to float32; dx, dy = its float32 difference to the
 *             float32 observation; err = (float)((double)dx dx + (double)dy dy); inlier iff err <= (float)(threshold threshold).
 *  4 runKernel  solvePnP(SOLVEPNP_EPNP) on the five points widened to double (the guess is ignored by EPnP):
 *             control points: c0 = the centroid, c_i = c0 + sqrt(lambda_i / 5) e_i for the eigenpairs of PW0^T PW0 (PW0 = the
 *               centred points) in descending lambda.  [FIXED] The 3x3 eigenproblem is the one-sided Jacobi of vg_init_relpose on
 *               the columns of PW0^T PW0 (lambda = the column norm); each e_i has its largest-magnitude entry positive (lowest index
 *               on a tie).  Barycentric coordinates through the 3x3 inverse (cofactors over the determinant) of [c1-c0 c2-c0 c3-c0].
 *             M (10 x 12) with fu = fv = 1, uc = vc = 0: rows [a_j, 0, -a_j u] and [0, a_j, -a_j v] per control point j.
 *               [FIXED] The eigenvectors of M^T M for its four smallest eigenvalues are the right singular vectors of M by the
 *               one-sided Jacobi on its 12 columns (pairs (i, j) with i + j = r mod 12 in round r = 0 .. 11 of a sweep, threshold
 *               1e-15, at most 40 sweeps, eigenvalue = squared column norm, ascending, lowest index on a tie): v1 the smallest .. v4.
 *             [DEVIATION] the null-space basis.  M^T M of 5 points has rank at most 10: v1, v2 are an arbitrary orthonormal basis of a
 *               plane, in OpenCV whatever rounding noise its SVD leaves, and the non-converged Gauss-Newton makes the pose depend on
 *               it.  Here, with (a, b) the computed pair, k the row of largest a[k]^2 + b[k]^2 (lowest index first) and r its root:
 *               v1 = (b[k] a - a[k] b) / r (0 at row k), v2 = (a[k] a + b[k] b) / r (r > 0 at row k); then every one of v1 .. v4 has
 *               its largest-magnitude entry made positive.  This is the library's choice: no OpenCV build is reproduced bit for bit at
 *               this step; the result depends continuously on the input wherever the row choice is not tied.
 *             compute_L_6x10, compute_rho as recalled; find_betas_approx_1 / 2 / 3 ([FIXED] their 6x4, 6x3, 6x5 least-squares solves
 *               are by the Householder QR of qr_solve, where OpenCV calls cvSolve(CV_SVD)), each followed by gauss_newton (5
 *               iterations, the 6x4 step by qr_solve) and compute_R_and_t: solve_for_sign, Arun's 3x3 SVD ([FIXED] the same one-sided
 *               Jacobi, U from the normalised columns, singular values descending) with R = U V^T, its third ROW negated when det R <
 *               0, t = pc0 - R pw0.  The candidate of the smallest mean reprojection error wins (2 against 1, then 3 against the
 *               better of them, strict <).  rvec = Rodrigues(R), regular branch.
 *             [DEVIATION] A sample whose control-point matrix has a determinant that is zero or not finite, a QR column that is all
 *               zero, a Rodrigues in the near-pi branch, or any value of rvec / tvec that is not finite yields NO model (count -1).
 *               The reference goes on with a pseudo-inverse.
 *  5 Returned pose  `refine` selects (recollections of the 3.x releases differ and nothing here can settle it):
 *             0  the winning sample's model goes out unchanged: recalled for the releases (3.2 - 3.4.x) that refit the inliers by
 *                solvePnP(EPNP / no guess) and then return the sample's model when the call is made through the RANSAC result;
 *             1  solvePnP(inliers, useExtrinsicGuess = 1, SOLVEPNP_ITERATIVE) started from R_inital / P_inital: recalled for 3.0 - 3.1
 *                and for builds that pass the caller's flags to the final solvePnP.  Exactly vg_init_sfm's PnP over the inliers in input
 *                order (points rounded to float32); VG_SFM_NUMERIC there is VG_KF_PNP_NUMERIC here.  That PnP hands its rotation on as a
 *                matrix: the returned rvec is its Rodrigues vector (regular branch; near pi: VG_KF_PNP_NUMERIC).
 *             The refit WITHOUT a guess (DLT / homography start of SOLVEPNP_ITERATIVE) is NOT offered.
 *             No model at all: solvePnPRansac returns false and leaves the caller's rvec0 / P_inital in place; so does this call
 *             (VG_KF_PNP_NO_MODEL, mask all zero, n_inliers 0).
 *  6 After the pose  :245-254 as written: r = Rodrigues(rvec); R_w_c_old = r^T; T_w_c_old = R_w_c_old (-tvec); PnP_R_old = R_w_c_old
 *             qic^T; PnP_T_old = T_w_c_old - PnP_R_old tic.  n_inliers > min_loop_num gates loop_info: relative_t = PnP_R_old^T
 *             (origin_vio_T - PnP_T_old); relative_q = the library's R_to_q (Eigen's Quaterniond(Matrix3d)) of PnP_R_old^T origin_vio_R,
 *             negated as a whole when w < 0 (w >= 0 on output), as w x y z; relative_yaw = normalizeAngle(R2ypr(origin_vio_R).x -
 *             R2ypr(PnP_R_old).x) in degrees.  has_loop = |relative_yaw| < max_yaw_deg && |relative_t| < max_dist, both strict.
 *             Without the gate loop_info is zero and has_loop 0.  The compacted lists (the inliers in input order) are filled whenever
 *             the RANSAC found a model, whatever has_loop says.
 * n <= min_loop_num: findConnection never calls PnPRANSAC: VG_KF_PNP_SKIPPED, everything else zero.
 * Refused with VG_ERR_BAD_ARG before anything is uploaded, no output touched, the handle usable: a wrong struct_size, n outside 6 ..
 * VG_KF_MAX_WINDOW, a NULL table (point_3d, old_norm), a non-finite input, reproj_threshold / max_yaw_deg / max_dist not positive,
 * min_loop_num < 0, max_iters outside 1 .. VG_KF_PNP_MAX_ITERS, a confidence other than 0.99, refine outside {0, 1}. */
#define VG_KF_PNP_OK 0
#define VG_KF_PNP_SKIPPED 1
#define VG_KF_PNP_NO_MODEL 2
#define VG_KF_PNP_NUMERIC 3
#define VG_KF_PNP_MAX_ITERS 1000
#define VG_KF_PNP_LAUNCHES 7         /* samples, counts, bookkeeping of the first chunk; the same of the rest; mask + refit + pose tail */
typedef struct vg_kf_pnp_in {
    size_t struct_size;          /* sizeof(vg_kf_pnp_in); vg_kf_pnp_defaults sets it */
    int n;                       /* matched_2d_cur.size() after vg_kf_match, 6 .. VG_KF_MAX_WINDOW */
    const float* point_3d;       /* [n][3] matched_3d (cv::Point3f) */
    const float* old_norm;       /* [n][2] matched_2d_old_norm (matched_old_norm of vg_kf_match) */
    const int* point_id;         /* [n] matched_id, or NULL: match_id is then the input index */
    double origin_vio_T[3], origin_vio_R[9], tic[3], qic[9];      /* row-major */
    int min_loop_num;            /* 25 (MIN_LOOP_NUM) */
    int max_iters;               /* 100 */
    int refine;                  /* step 5; default 0 */
    double reproj_threshold;     /* 10.0 / 460.0 */
    double confidence;           /* 0.99; nothing else is accepted */
    double max_yaw_deg;          /* 30 */
    double max_dist;             /* 20 */
} vg_kf_pnp_in;
typedef struct vg_kf_pnp_out {
    size_t struct_size;          /* sizeof(vg_kf_pnp_out), set by the caller */
    int status;                  /* VG_KF_PNP_* */
    int n_inliers;
    int ransac_best;             /* iteration whose model won, -1: none */
    int ransac_iter;             /* the last iteration the loop looked at */
    int ransac_bound;            /* the bound niters ended with */
    int refit_iters, refit_up;   /* refine == 1: iterations and lambda raises of the PnP (pnp_iters / pnp_up of vg_init_sfm) */
    int has_loop;
    double sample_rvec[3], sample_tvec[3];     /* the winning sample's model */
    double rvec[3], tvec[3];                   /* the returned pose */
    double PnP_R_old[9], PnP_T_old[3];
    double loop_info[8];         /* relative_t 3 | relative_q w x y z | relative_yaw (degrees) */
    unsigned char* mask;         /* [n] status of PnPRANSAC, or NULL */
    int* matched_index;          /* [n] capacity each, or NULL: the n_inliers surviving input indices, ascending */
    int* match_id;               /* point_id of the survivors: vg_ba_relo_frame::match_id */
    double* match_xy;            /* [..][2] old_norm of the survivors widened: vg_ba_relo_frame::match_xy */
    float* device_ms;            /* out[0] only: VG_KF_PNP_LAUNCHES event intervals of the batch, or NULL */
} vg_kf_pnp_out;
void vg_kf_pnp_defaults(vg_kf_pnp_in* in);        /* zero, struct_size and the defaults above; qic and origin_vio_R the identity */
int vg_kf_pnp(vg_handle* h, int n_pairs, const vg_kf_pnp_in* in /* [n_pairs] */, vg_kf_pnp_out* out /* [n_pairs] */);

/* ---- Loop closure: DBoW2 loop detection, batched (added within ABI 12, nothing existing changed) ----------------------------------------
 * PoseGraph::detectLoop (pose_graph/src/pose_graph.cpp:304-386) and addKeyFrameIntoVoc for a batch of pose graphs: the vocabulary tree,
 * one resident database per pose graph, the query, the decision and the add.  The input of a request is a filled vg_kf_* record: its
 * `descriptors` are brief_descriptors of computeBRIEFPoint and never leave the device.  The returned loop_index goes to vg_kf_match as
 * the old keyframe (the caller maps the database's entry ids, which are the keyframe indices when every keyframe is added in order, to
 * its slots).  optimize4DoF is vg_pg_optimize (the last block).  NOT offered, and left with the caller: thumbnails and debug images.
 *
 * DBoW2 is vendored in the reference (pose_graph/src/ThirdParty/DBoW, VocabularyBinary.*): READ from the reference as the definition, not
 * recalled, and restated in tests/kf_bow_ref.py (the reference's DBoW2 is not compiled into the oracle).  Only what PoseGraph uses is
 * offered: weighting TF_IDF (enum value 0), scoring L1_NORM (0), no direct index (db.setVocabulary(*voc, false, 0)).  That the shipped
 * brief_k10L6.bin carries TF_IDF / L1_NORM is DBoW2's default and UNVERIFIED here (the file was not available).
 *
 *   vocabulary  (VocabularyBinary.hpp, TemplatedVocabulary::loadBin:1509-1561) the file's records: vg_voc_node x n_nodes, vg_voc_word x
 *               n_words.  Node 0 is the root and has no record.  The children of a node are the records naming it as parent, IN RECORD
 *               ORDER.  A node without children is a leaf.  Bit i of a descriptor is word i / 64, position i % 64, as in vg_kf_*.  The
 *               tree need not be uniform.
 *   word        (transform:1217-1258) start at the root; among the current node's children take the one with the smallest Hamming
 *               distance to the descriptor, on a tie the FIRST in child order (the reference updates on d < best_d only); repeat until the
 *               chosen node is a leaf: its word_id and weight.
 *   BoW vector  (transform:1065-1121, BowVector::addWeight, normalize) over the descriptors in keypoint order: a word whose weight is not
 *               > 0 is skipped ("stopped"), else v[word] += weight: for a word seen c times c - 1 sequential additions of the same
 *               double, NOT c * weight.  Then norm = sum of fabs(v) in ascending word id, sequentially from 0; every value is divided by
 *               norm if norm > 0.
 *   query       (queryL1:656-723, db.query(desc, ret, 4, frame_index - 50)) max_id = frame_index - 50; entry e takes part iff e < max_id ||
 *               max_id == -1 || e == n_entries - 1, n_entries counted BEFORE this frame is added: the last entry added always takes
 *               part (ret[0], "the nearest neighbour's score"), and frame_index == 49 admits every entry.  For an entry with at least
 *               one word in common, value = the sum over the common words in ascending word id of fabs(q - d) - fabs(q) - fabs(d),
 *               accumulated sequentially, starting from the first term.  Entries without a common word do not appear.  Sorted ascending
 *               by value, the first 4 kept; Score = -value / 2.0.  std::sort leaves the order of equal values to the platform: THIS
 *               LIBRARY breaks ties by ascending entry id.
 *   decision    (detectLoop:348-385) find_loop = n_results >= 1 && Score[0] > 0.05 && some i >= 1 has Score[i] > 0.015.  If find_loop &&
 *               frame_index > 50: min_index = Id[0] unconditionally, lowered to every Id[i] < min_index with Score[i] > 0.015; loop_index =
 *               min_index.  Otherwise loop_index = -1.
 *   add         (db.add) the frame's vector becomes entry n_entries++, after the query.
 * Additions, fabs, one division per word and one halving: nothing is multiplied and added in one expression, and the device result
 * equals a float64 restatement bit for bit.
 *
 * vg_voc_load       validates on the host, then uploads the tree renumbered so that the children of a node are contiguous and in child
 *                   order (one sibling group = one contiguous read of n_children x 32 bytes).  Word ids that leave the library are the
 *                   file's.  k and L are the file's header: no node may have more than k children (k <= 65535), no leaf may lie deeper
 *                   than L.  A second call replaces the vocabulary and empties every database.  Refused before anything is touched: a
 *                   node id outside 1 .. n_nodes or repeated, a parent that is not a node or the root, a node not reachable from the
 *                   root, a word on a node with children, a leaf without a word or with two, a word id outside 0 .. n_words - 1 or
 *                   repeated, an empty root, more than k children, a leaf below level L, k or L < 1, a scoring / weighting other than
 *                   VG_BOW_L1_NORM / VG_BOW_TF_IDF, a NULL table.
 * vg_bow_configure  n_db independent resident databases (one pose graph each) of at most max_entries entries; a database stores its
 *                   entries back to back in a pool of pool_words (word id, value) pairs with an offset table.  Calling it again replaces
 *                   them.  Needs a vocabulary.  Refused: n_db, max_entries or pool_words < 1.
 * vg_bow_reset      empties database db.
 * vg_bow_get        one entry's vector (savePoseGraph, tests): n_words always; words / values (ascending word id) when non-NULL, refused
 *                   when `capacity` is below n_words.
 * vg_kf_loop_detect n requests in one call: one upload (the requests), VG_BOW_LAUNCHES launches over the batch, one download.
 *                   flags: VG_BOW_QUERY | VG_BOW_ADD is detectLoop, VG_BOW_ADD alone is addKeyFrameIntoVoc, VG_BOW_QUERY alone queries
 *                   without adding.  A record with no keypoints gives an empty vector: no results, and an empty entry if ADD.  The pool
 *                   advances by the true word count.  Refused with VG_ERR_BAD_ARG before anything is touched: no vocabulary, no
 *                   vg_bow_configure, no vg_kf_configure, a wrong struct_size, flags without QUERY and ADD or with other bits, db or slot
 *                   out of range, a slot never filled, the same db twice in one call (the order would matter), ADD on a database with
 *                   max_entries entries or with fewer free pool words than the record's keypoints (the upper bound of its distinct
 *                   words, known before the launch). */
#define VG_BOW_TF_IDF 0              /* DBoW2::WeightingType */
#define VG_BOW_L1_NORM 0             /* DBoW2::ScoringType */
#define VG_BOW_QUERY 1
#define VG_BOW_ADD 2
#define VG_BOW_MAX_RESULTS 4
#define VG_BOW_STOPPED 0xFFFFFFFFu   /* word_of_keypoint of a descriptor that lands on a word whose weight is not > 0 */
#define VG_BOW_LAUNCHES 4            /* walk, vector, score, tail */
typedef struct vg_voc_node {         /* VINSLoop::Node, the file's record */
    int32_t node_id, parent_id;
    double weight;
    uint64_t descriptor[4];
} vg_voc_node;
typedef struct vg_voc_word {         /* VINSLoop::Word */
    int32_t node_id, word_id;
} vg_voc_word;
typedef struct vg_bow_entry {
    int struct_size;             /* sizeof(vg_bow_entry) */
    int capacity;                /* of words / values */
    int n_words;                 /* out */
    uint32_t* words;             /* ascending, or NULL */
    double* values;              /* or NULL */
} vg_bow_entry;
typedef struct vg_bow_in {
    int struct_size;             /* sizeof(vg_bow_in) */
    int db;
    int slot;                    /* a filled vg_kf_* record */
    int frame_index;             /* detectLoop's frame_index (VG_BOW_QUERY) */
    int flags;                   /* VG_BOW_QUERY | VG_BOW_ADD */
} vg_bow_in;
typedef struct vg_bow_out {
    int struct_size;             /* sizeof(vg_bow_out), set by the caller */
    int entry_id;                /* the entry this frame became, -1 without VG_BOW_ADD */
    int n_results;               /* 0 .. VG_BOW_MAX_RESULTS (0 without VG_BOW_QUERY) */
    int ids[VG_BOW_MAX_RESULTS]; /* ret[i].Id, -1 beyond n_results */
    double scores[VG_BOW_MAX_RESULTS];   /* ret[i].Score, 0 beyond n_results */
    int find_loop;
    int loop_index;              /* detectLoop's return value */
    int n_words;                 /* entries of the frame's BoW vector */
    uint32_t* word_of_keypoint;  /* [n_keypoints of the record] taps, or NULL: the file's word id or VG_BOW_STOPPED */
    uint32_t* bow_word;          /* [n_keypoints] capacity: the vector's word ids, ascending */
    double* bow_value;           /* [n_keypoints] capacity: its values */
    float* device_ms;            /* out[0] only: VG_BOW_LAUNCHES event intervals of the batch, or NULL */
} vg_bow_out;
int vg_voc_load(vg_handle* h, int k, int L, int scoring, int weighting, int n_nodes, const vg_voc_node* nodes /* [n_nodes] */, int n_words,
                const vg_voc_word* words /* [n_words] */);
int vg_bow_configure(vg_handle* h, int n_db, int max_entries, int pool_words);
int vg_bow_reset(vg_handle* h, int db);
int vg_bow_count(vg_handle* h, int db, int* n_entries, int* pool_used);     /* what database db holds (either pointer may be NULL) */
int vg_bow_get(vg_handle* h, int db, int entry, vg_bow_entry* out);
int vg_kf_loop_detect(vg_handle* h, int n, const vg_bow_in* in /* [n] */, vg_bow_out* out /* [n] */);

/* ---- Loop closure: 4-DoF pose-graph optimisation, batched (added within ABI 12, nothing existing changed) -------------------------------
 * One pass of the body of PoseGraph::optimize4DoF (pose_graph/src/pose_graph.cpp:403-579) for n_graphs independent pose graphs in one
 * call: the graph, the solve, updatePose of the optimised keyframes, the drift, and the drift applied to the keyframes behind cur_index.
 * Plain arrays in and out, no configure call.  Synchronous: one upload, VG_PG_LAUNCHES launch over the whole batch (one workgroup per
 * graph, all iterations inside it), one download; device scratch grows on demand inside the handle.  A graph's status never touches its
 * neighbours; a batch equals the single calls bit for bit.
 *
 * The graph and the cost functors are READ from the reference; Ceres (problem, loss corrector, trust region) is RECALLED, NOT PINNED, as
 * for vg_init_sfm.  [FIXED]: this library's choice where Ceres leaves the result to a general-purpose solver; [DEVIATION]: knowingly
 * different.
 *  input     The slice of keyframelist that optimize4DoF walks, in list order: the n_kf keyframes with index >= first_looped_index
 *            through the END of the list; the first n_opt of them (up to and including cur_index) are optimised, the others only receive
 *            the drift (:562-571).  loop_info is vg_kf_pnp_out::loop_info: relative_t | relative_q | relative_yaw (degrees); has_loop,
 *            loop_index and loop_info are read for the optimised keyframes only.
 *  graph     (:445-519) local index i over the optimised keyframes.  Variables per node: yaw_i (degrees) and t_i; pitch_i, roll_i are
 *            constants; (yaw, pitch, roll) = Utility::R2ypr(vio_R_i), t_i = vio_T_i.  A node is CONSTANT when index == first_looped_index or
 *            sequence == 0.  Chain edges (i-j) -> i for j = 1 .. 4 while i-j >= 0 and the sequences are equal: relative_t = vio_R_{i-j}^T
 *            (t_i - t_{i-j}), relative_yaw = yaw_i - yaw_{i-j}, NOT normalised, no loss.  Loop edge of a node with has_loop: from the node
 *            whose index == loop_index to i, relative_t = loop_info[0..2], relative_yaw = loop_info[7], HuberLoss(huber_delta).  Edge slot
 *            5 i + (j - 1) is the chain edge from i-j, slot 5 i + 4 the loop edge; a slot without an edge counts as zero everywhere.
 *            [DEVIATION] the reference passes vio_R through a quaternion and back (tmp_q = tmp_r; q.toRotationMatrix(); q.inverse() * v):
 *            the matrix is used directly, the difference is rounding.
 *  residual  (pose_graph.h:88-247, as written) edge a -> b with R = YawPitchRollToRotationMatrix(yaw_a, pitch_a, roll_a) (degrees,
 *            x / 180 * pi): e[c] = (R[c] d0 + R[3+c] d1 + R[6+c] d2) - relative_t[c], d = t_b - t_a; e[3] = NormalizeAngle(yaw_b - yaw_a -
 *            relative_yaw), divided by 10 on a loop edge (FourDOFWeightError, weight 1).  NormalizeAngle is the reference's one
 *            conditional wrap (> 180: - 360; < -180: + 360), slope 1.  Parameters of a node in the order yaw, t.  The Jacobian is the exact
 *            derivative: d e[c] / d t_b = (R[c], R[3+c], R[6+c]) = -d e[c] / d t_a; d e[c] / d yaw_a = (R[c] d1 - R[3+c] d0) (pi / 180);
 *            d e[3] / d yaw_b = 1 (loop: 1 / 10) = -d e[3] / d yaw_a.  AngleLocalParameterization: Plus = NormalizeAngle(yaw + delta),
 *            Jacobian 1.
 *  loss      s = e.e (ascending).  Huber: s <= delta^2: rho = s, rho' = 1; else rho = 2 delta sqrt(s) - delta^2, rho' = max(DBL_MIN,
 *            delta / sqrt(s)).  rho'' <= 0 everywhere, so Ceres' Corrector takes its first branch: residual and Jacobian rows times
 *            sqrt(rho'), no alpha term.  cost = (sum of rho over the edge slots) / 2; edges between two constant nodes count in the cost.
 *  sums      [FIXED] a SUM OVER A LIST (edge slots, parameters) is: thread t of 256 adds the entries t, t + 256, ... in ascending order;
 *            the 256 partial sums are folded by halves (p[t] += p[t + h], h = 128, 64 .. 1).  A product of small matrices sums its inner
 *            index ascending from the first term.  The terms of a node are gathered in the order: its own edge slots 0 .. 4 (as b), the
 *            chain edges leaving it to i+1 .. i+4 (as a), the loop edges arriving at it in ascending source (as a); every term is formed
 *            first and then added.  Nothing is multiplied and added in one rounding (-ffp-contract=off).
 *  minimiser Exactly the loop of the vg_init_sfm block with the cap max_iters: radius 1e4, Jacobi scale 1 / (1 + column norm) from the
 *            FIRST Jacobian, D = sqrt(clamp(diag, 1e-6, 1e32) / radius) and D D added, gradient tolerance 1e-10 (unscaled, max-norm over the
 *            free nodes) at the start and after every accepted step, parameter tolerance 1e-8 and function tolerance 1e-6 in this order
 *            before the step is judged, rho > 1e-3, the radius rules, five invalid steps in a row: FAILURE.  x and |x| run over the free
 *            nodes.  [FIXED] the blocks of JtJ are formed from the unscaled Jacobian and scaled afterwards, s_p (A_pq s_q), the diagonal
 *            blocks mirrored from their lower triangle; the model change is -sum over the edge slots of u.(r + u / 2), u = Ja da + Jb db
 *            with d = scale * y the step in the parameters.  max_solver_time stays out, as in the reference (commented out).
 *  step      [FIXED] (Ceres: SPARSE_NORMAL_CHOLESKY; the step is the same to the residual below.)  A = JtJ + D D over the free nodes in
 *            list order, 4x4 blocks.  M = the block band of A of half-width 4 blocks: every chain edge in full, both diagonal blocks of
 *            every loop edge, its off-diagonal block only inside the band; positive definite as a sum of positive semidefinite terms
 *            plus D D > 0.  Band block (f, f-d): the chain edge between the two nodes, then the loop edge.  Unpivoted Cholesky of M as a
 *            scalar band of half-width 19, column by column (every entry loses its products in ascending column order): a pivot that is
 *            not positive and finite makes the step invalid; the inverse 1 / sqrt(pivot) is kept and MULTIPLIED with, in the
 *            factorisation and in both sweeps.  A y = -g by conjugate gradients preconditioned with M from y = 0: r = b, z = M^-1 r,
 *            p = z; per iteration q = A p, alpha = r.z / p.q (p.q not > 0: invalid), y += alpha p, r -= alpha q, z = M^-1 r, done when
 *            r.z <= 1e-24 r0.z0 (sqrt(r.z) <= 1e-12 sqrt(r0.z0)), else p = z + (r.z / previous r.z) p.  VG_PG_MAX_CG iterations without
 *            that make the step invalid.  q = A p by rows: band blocks d = 4 .. 1, the diagonal block, the transposed blocks of the rows
 *            f+1 .. f+4, the node's own out-of-band loop block, the transposed ones of the loops arriving in ascending source, D D p.
 *  after     (:532-571) T = t_i, R = Utility::ypr2R(yaw_i, pitch_i, roll_i) ((Rz Ry) Rx) for the optimised keyframes, constant ones
 *            included; yaw_drift = R2ypr(R_cur).x - R2ypr(vio_R_cur).x, r_drift = ypr2R(yaw_drift, 0, 0), t_drift = t_cur - r_drift
 *            vio_T_cur; behind cur_index T = r_drift vio_T + t_drift, R = r_drift vio_R.
 * status: VG_PG_OK; VG_PG_NO_EDGES nothing is free: the poses are the VIO poses through the same formulas, the drift is computed all the
 * same, iterations 0; VG_PG_NUMERIC the initial cost or a returned number is not finite: T, R and the drift come back as zeros.
 * VG_PG_OK says that the numbers are finite, not that the solve went well: five invalid steps in a row (VG_PG_MAX_CG iterations without
 * convergence is one way to an invalid step) end with VG_PG_OK and termination VG_TERM_FAILURE; read termination and it_cg.
 * Refused with VG_ERR_BAD_ARG before anything is uploaded (vg_last_error names the cause; no output is touched, the handle stays usable): a
 * wrong struct_size, n_kf outside 1 .. VG_PG_MAX_KEYFRAMES, n_opt outside 1 .. n_kf, a NULL table, index not strictly ascending, a first
 * keyframe below first_looped_index, sequence < 0, a loop_index below first_looped_index, not in the slice or not before its own
 * keyframe, a non-finite input, max_iters outside 1 .. VG_PG_MAX_ITERS, huber_delta not positive.
 * NOT offered, and left with the caller: the thread around the pass and its 2 s sleep, thumbnails, debug images, map save / load, ROS. */
#define VG_PG_OK 0
#define VG_PG_NO_EDGES 1
#define VG_PG_NUMERIC 2
#define VG_PG_MAX_KEYFRAMES 2048
#define VG_PG_MAX_ITERS 8
#define VG_PG_MAX_CG 128
#define VG_PG_LAUNCHES 1
typedef struct vg_pg_in {
    size_t struct_size;          /* sizeof(vg_pg_in); vg_pg_defaults sets it */
    int n_kf;                    /* 1 .. VG_PG_MAX_KEYFRAMES */
    int n_opt;                   /* 1 .. n_kf: the keyframes up to and including cur_index */
    int first_looped_index;
    int max_iters;               /* 5 */
    double huber_delta;          /* 0.1 */
    const int* index;            /* [n_kf] strictly ascending */
    const int* sequence;         /* [n_kf] */
    const int* has_loop;         /* [n_kf] */
    const int* loop_index;       /* [n_kf] a global index (read where has_loop) */
    const double* vio_T;         /* [n_kf][3] */
    const double* vio_R;         /* [n_kf][9] row-major */
    const double* loop_info;     /* [n_kf][8] (read where has_loop) */
} vg_pg_in;
typedef struct vg_pg_out {
    size_t struct_size;          /* sizeof(vg_pg_out), set by the caller */
    int status;                  /* VG_PG_* */
    int termination;             /* VG_TERM_* */
    int iterations;
    int n_edges, n_loop_edges, n_free;
    double initial_cost, final_cost;
    double yaw_drift, r_drift[9], t_drift[3];
    double it_cost[VG_PG_MAX_ITERS], it_radius[VG_PG_MAX_ITERS], it_cost_cand[VG_PG_MAX_ITERS], it_model[VG_PG_MAX_ITERS];
    int it_flags[VG_PG_MAX_ITERS];       /* bit0 valid, bit1 accepted */
    int it_cg[VG_PG_MAX_ITERS];          /* conjugate-gradient iterations of the row's solve */
    double* T;                   /* [n_kf][3] what updatePose receives, or NULL */
    double* R;                   /* [n_kf][9] or NULL */
    float* device_ms;            /* out[0] only: VG_PG_LAUNCHES event intervals of the batch, or NULL */
} vg_pg_out;
void vg_pg_defaults(vg_pg_in* in);                /* zero, struct_size, max_iters 5, huber_delta 0.1 */
int vg_pg_optimize(vg_handle* h, int n_graphs, const vg_pg_in* in /* [n_graphs] */, vg_pg_out* out /* [n_graphs] */);

#ifdef __cplusplus
}
#endif
#endif /* VINSGPU_H */
