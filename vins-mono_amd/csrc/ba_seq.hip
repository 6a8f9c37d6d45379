// ba_seq.hip — windows that stay on the device from frame to frame (include/vinsgpu.h: vg_ba_seq_*).
//
// What the reference does on the host around Estimator::optimization(), once per frame (Estimator::processImage,
// vins_estimator/src/estimator.cpp:120-215), done here by four small kernels on the window's own tables in HBM:
//
//   ba_seq_add_kernel    FeatureManager::addFeatureCheckParallax (feature_manager.cpp:45-107): the new frame's observations join
//                        their tracks (linear search by feature id, first match, like the find_if of :58), unknown ids open new
//                        tracks at the end of the list in the order they arrive; last_track_num; the key-frame test by the
//                        mean parallax between the second and third newest frames (compensatedParallax2, :352-382) decides the
//                        marginalization flag (estimator.cpp:124-127).  Also takes in what processIMU produced: the state guess of
//                        the new frame and the pre-integration of the new (and, after a dropped non-keyframe, the merged) interval.
//   ba_seq_tri_kernel    FeatureManager::triangulate (feature_manager.cpp:202-257) for the tracks that are in the problem and have
//                        no depth yet (tri_dlt.h).
//   ba_seq_build_kernel  what optimization() walks f_manager.feature for (estimator.cpp:719-764) and vector2double() (:486-528):
//                        the landmark list (used_num >= 2 && start_frame < WINDOW_SIZE - 2, list order), inverse depths,
//                        observation rows, the factor list and its (anchor, target)-sorted slot table, the prior's block table --
//                        exactly the tables csrc/ba_host.hip pack_window builds on the host for an uploaded window.  In a window
//                        armed with a relocalisation frame (vg_ba_seq_set_relo) also what optimization() adds for
//                        relocalization_info (:769-801): the walk over match_points, one factor per matched landmark against
//                        the loop pose, block K of the window.
//   [ the solve pipeline and the marginalization kernel of ba_pipeline.hip / ba_marg.hip, unchanged ]
//   ba_seq_slide_kernel  double2vector's setDepth (feature_manager.cpp:141-159), slideWindow() (estimator.cpp:1005-1126: state and
//                        pre-integration shift for both flags), FeatureManager::removeBackShiftDepth / removeFront
//                        (feature_manager.cpp:275-351), removeFailures (:161-171); the new prior's block table.
//
// A sequence that takes raw IMU samples (vg_ba_seq_imu_begin) runs ba_seq_imu_kernel in front of all this and ba_seq_merge_kernel
// behind it: Estimator::processIMU (estimator.cpp:84-118) and the IMU part of slideWindow() (:1069-1095) on the device.
//
// A sequence fed by the front end on the same handle (vg_vio_step_async) runs ba_seq_bridge_kernel in front of all that: the message
// fe_tk_commit_kernel left in HBM becomes the frame staging ba_seq_add_kernel reads, without a trip through the host.
//
// One workgroup per window.  The track table is a plain ordered list (ints: id, start_frame, n_obs, solve_flag, landmark index in
// the current problem; doubles: estimated_depth and K rows of 8 per track); the slide writes the surviving tracks, compacted in
// order, into the window's second table, so no kernel moves rows in place.  Order matters: it is the order of para_Feature.
#include <hip/hip_runtime.h>
#include "ba_math.h"
#include "tri_dlt.h"
#include "ba_layout.h"
#include "imu_step.h"
#include "vg_handle.h"
#include "fe_layout.h"
#include "../../include/vinsgpu.h"

#define SEQ_NT 256
#define SEQ_HDR 8                 // ints in front of a track table: [0] number of tracks
#define SEQ_FT_MAX 1024           // tracks per window (LDS tables of the kernels)
#define SEQ_NIN_MAX 1024          // observations per frame
#define SEQ_L_MAX 1024            // landmarks in the problem
#define SEQ_MM_MAX 1024           // matched points of a relocalisation frame
#define SEQ_IMU 472               // doubles per pre-integration record (= BA_IMU_STRIDE)
#define SEQ_IN_POSE 0
#define SEQ_IN_SB 7
#define SEQ_IN_IMU_NEW 16
#define SEQ_IN_IMU_MERGED (16 + SEQ_IMU)
#define SEQ_IN_ROWS (16 + 2 * SEQ_IMU)

struct SeqTab {
    int* hdr; int* id; int* start; int* nobs; int* sflag; int* lm;
    double* depth; double* obs;
};
DEV SeqTab seq_table(const SeqDev& S, int which, int w) {
    SeqTab t;
    int* ti = S.ft_i[which] + (size_t)w * S.fi_stride;
    double* td = S.ft_d[which] + (size_t)w * S.fd_stride;
    t.hdr = ti; t.id = ti + SEQ_HDR; t.start = t.id + S.FT; t.nobs = t.start + S.FT; t.sflag = t.nobs + S.FT; t.lm = t.sflag + S.FT;
    t.depth = td; t.obs = td + S.FT;
    return t;
}

// Ordered compaction by the first wavefront: dst[f] = rank of f among the flagged entries (flag[f] != 0), -1 otherwise.
// Returns the count to the first wavefront's lanes (others must read it from LDS after a barrier).
DEV int seq_compact(const int* flag, int* dst, int n, int tid) {
    int base = 0;
    if (tid < 64) {
        for (int c = 0; c < n; c += 64) {
            const int f = c + tid;
            const int on = (f < n) && flag[f];
            const unsigned long long mask = __ballot(on);
            if (f < n) dst[f] = on ? base + __popcll(mask & ((1ull << tid) - 1ull)) : -1;
            base += __popcll(mask);
        }
    }
    return base;
}

// ---------------------------------------------------------------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(SEQ_NT) void ba_seq_add_kernel(const BaLayout* __restrict__ Lp, BaPtrs P, SeqDev S, int cur) {
    __shared__ int s_id[SEQ_FT_MAX];
    __shared__ int s_match[SEQ_NIN_MAX];
    __shared__ int s_isnew[SEQ_NIN_MAX];
    __shared__ int s_cond[SEQ_FT_MAX];
    __shared__ double s_val[SEQ_FT_MAX];
    __shared__ int s_misc[4];
    const BaLayout& L = *Lp;
    const int w = blockIdx.x, tid = threadIdx.x, K = S.K, WS = K - 1;
    SeqTab T = seq_table(S, cur, w);
    int* ia = P.iarr + (size_t)w * L.istride;
    double* di = P.din + (size_t)w * L.dstride;
    const int* ii = S.in_i + (size_t)w * S.ii_stride;
    const double* idd = S.in_d + (size_t)w * S.id_stride;
    const int* inid = ii + 8;
    const double* rows = idd + S.rows_off;
    int* info = S.info + (size_t)w * VG_SEQ_INFO_INTS;
    const int n = T.hdr[0];
    int nin = ii[0];
    int status = VG_OK;
    if (nin > S.NIN) { nin = S.NIN; status = VG_ERR_UNSUPPORTED; }
    for (int f = tid; f < n; f += SEQ_NT) s_id[f] = T.id[f];
    __syncthreads();
    // ---- find_if(feature.begin(), feature.end(), id == feature_id): first match in list order
    for (int i = tid; i < nin; i += SEQ_NT) {
        const int id = inid[i];
        int m = -1;
        for (int j = 0; j < n; ++j) if (s_id[j] == id) { m = j; break; }
        s_match[i] = m;
        s_isnew[i] = m < 0;
    }
    __syncthreads();
    // ---- unknown ids: new tracks behind the list, in arrival order (feature.push_back, :62-65)
    {
        const int cnt = seq_compact(s_isnew, s_isnew, nin, tid);          // (in place: an entry is read and written by the same lane)
        if (tid == 0) s_misc[0] = cnt;
    }
    __syncthreads();
    const int n_new = s_misc[0];
    int ntot = n + n_new;
    if (ntot > S.FT) { ntot = S.FT; status = VG_ERR_UNSUPPORTED; }
    const double td_cur = di[L.do_td];
    for (int i = tid; i < nin; i += SEQ_NT) {
        int f = s_match[i], j = 0;
        if (f >= 0) {
            j = T.nobs[f];
            if (j >= K) continue;                                         // (cannot happen: a track spans consecutive frames of the window)
            T.nobs[f] = j + 1;
        } else {
            f = n + s_isnew[i];
            if (f >= S.FT) continue;
            T.id[f] = inid[i]; T.start[f] = WS; T.nobs[f] = 1; T.sflag[f] = 0; T.lm[f] = -1;
            T.depth[f] = -1.0;                                            // FeaturePerId ctor (feature_manager.h:57-61)
        }
        const double* r = rows + (size_t)i * 8;                           // [x y z u v vx vy]
        double* o = T.obs + ((size_t)f * K + j) * 8;                      // [x y u v vx vy cur_td z]
        o[0] = r[0]; o[1] = r[1]; o[2] = r[3]; o[3] = r[4]; o[4] = r[5]; o[5] = r[6]; o[6] = td_cur; o[7] = r[2];
    }
    __syncthreads();
    // ---- key-frame test (:73-106): parallax between frames WS - 2 and WS - 1 of every track that has both
    const int last_track_num = nin - n_new;
    const int fc = WS;
    for (int f = tid; f < ntot; f += SEQ_NT) {
        const int st = T.start[f], no = T.nobs[f];
        const int on = (st <= fc - 2) && (st + no - 1 >= fc - 1);
        double ans = 0.0;
        if (on) {
            const double* fi = T.obs + ((size_t)f * K + (fc - 2 - st)) * 8;
            const double* fj = T.obs + ((size_t)f * K + (fc - 1 - st)) * 8;
            const double u_j = fj[0], v_j = fj[1];
            const double dep_i = fi[7];
            const double u_i = fi[0] / dep_i, v_i = fi[1] / dep_i;
            const double du = u_i - u_j, dv = v_i - v_j;
            ans = fmax(0.0, sqrt(fmin(du * du + dv * dv, du * du + dv * dv)));       // (p_i_comp = p_i, :369)
        }
        s_cond[f] = on;
        s_val[f] = ans;
    }
    __syncthreads();
    if (tid == 0) {
        double sum = 0.0;
        int num = 0;
        for (int f = 0; f < ntot; ++f) if (s_cond[f]) { sum += s_val[f]; ++num; }       // list order, like the reference's loop
        int flag = VG_MARGIN_OLD;                                          // addFeatureCheckParallax() == true
        if (!(fc < 2 || last_track_num < 20) && num != 0) flag = (sum / num >= S.min_parallax) ? VG_MARGIN_OLD : VG_MARGIN_SECOND_NEW;
        ia[L.io_hdr + H_MARGIN] = flag;
        T.hdr[0] = ntot;
        info[VG_SEQ_FLAG] = flag; info[VG_SEQ_N_FEATURES] = ntot; info[VG_SEQ_N_TRACKED] = last_track_num; info[VG_SEQ_N_PARALLAX] = num;
        info[VG_SEQ_STATUS] = status;
    }
    // ---- what processIMU produced (estimator.cpp:83-117): state of the new frame, pre_integrations[WINDOW_SIZE]; after a dropped
    //      non-keyframe also the merged pre_integrations[WINDOW_SIZE - 1] (:1069-1085)
    //      (a sequence that takes raw samples has all of this from ba_seq_imu_kernel / ba_seq_merge_kernel already: its staging
    //      holds samples where a host-fed one holds the records)
    if (S.imu_mode) return;
    if (tid < 7) di[L.do_pose + 7 * WS + tid] = idd[SEQ_IN_POSE + tid];
    if (tid >= 32 && tid < 41) di[L.do_sb + 9 * WS + (tid - 32)] = idd[SEQ_IN_SB + (tid - 32)];
    for (int e = tid; e < 467; e += SEQ_NT) di[L.do_imu + (size_t)(K - 2) * BA_IMU_STRIDE + e] = idd[SEQ_IN_IMU_NEW + e];
    if (tid == 64) ia[L.io_imu_valid + (K - 2)] = (ii[2] && idd[SEQ_IN_IMU_NEW] <= 10.0) ? 1 : 0;
    if (ii[1] && K >= 3) {
        for (int e = tid; e < 467; e += SEQ_NT) di[L.do_imu + (size_t)(K - 3) * BA_IMU_STRIDE + e] = idd[SEQ_IN_IMU_MERGED + e];
        if (tid == 65) ia[L.io_imu_valid + (K - 3)] = (ii[3] && idd[SEQ_IN_IMU_MERGED] <= 10.0) ? 1 : 0;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// grid (nwin, FT / 64), one thread per track
extern "C" __global__ __launch_bounds__(64) void ba_seq_tri_kernel(const BaLayout* __restrict__ Lp, BaPtrs P, SeqDev S, int cur) {
    __shared__ double A[TRI_ROWS * 4][64];
    __shared__ double s_P[3 * TRI_MAXOBS], s_R[9 * TRI_MAXOBS];
    const BaLayout& L = *Lp;
    const int w = blockIdx.x, t = threadIdx.x, K = S.K, WS = K - 1;
    SeqTab T = seq_table(S, cur, w);
    const int n = T.hdr[0];
    if ((int)blockIdx.y * 64 >= n) return;
    const double* di = P.din + (size_t)w * L.dstride;
    if (t < K) {                                                          // Ps / Rs of the window (vector members of the Estimator)
        const double* x = di + L.do_pose + 7 * t;
        double q[4] = {x[3], x[4], x[5], x[6]};
        q_normalize(q);
        q_to_R(q, s_R + 9 * t);
        s_P[3 * t] = x[0]; s_P[3 * t + 1] = x[1]; s_P[3 * t + 2] = x[2];
    }
    __syncthreads();
    const int f = blockIdx.y * 64 + t;
    if (f >= n) return;
    const int st = T.start[f], no = T.nobs[f];
    if (!(no >= 2 && st < WS - 2)) return;                                // :206-208
    if (T.depth[f] > 0) return;                                           // :210-211
    double Ric[9], Tic[3];
    {
        const double* ex = di + L.do_ex;
        double q[4] = {ex[3], ex[4], ex[5], ex[6]};
        q_normalize(q);
        q_to_R(q, Ric);
        Tic[0] = ex[0]; Tic[1] = ex[1]; Tic[2] = ex[2];
    }
    const double* ob = T.obs + (size_t)f * K * 8;
    T.depth[f] = tri_dlt_depth(A, t, s_P, s_R, Ric, Tic, st, no,
                               [ob](int j, double* p) { p[0] = ob[8 * j]; p[1] = ob[8 * j + 1]; p[2] = ob[8 * j + 7]; }, S.init_depth);
}

// ---------------------------------------------------------------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(SEQ_NT) void ba_seq_build_kernel(const BaLayout* __restrict__ Lp, BaPtrs P, SeqDev S, int cur) {
    __shared__ int s_in[SEQ_FT_MAX];           // track is in the problem
    __shared__ int s_lm[SEQ_FT_MAX];           // its landmark index
    __shared__ int s_ls[SEQ_L_MAX], s_ln[SEQ_L_MAX], s_feat[SEQ_L_MAX];
    __shared__ int s_fbeg[SEQ_L_MAX + 1], s_off[SEQ_L_MAX + 1];
    __shared__ int s_pair[BA_MAX_K * BA_MAX_K + 1];
    __shared__ int s_mid[SEQ_MM_MAX];          // relocalisation frame: ids of the matched points,
    __shared__ int s_lid[SEQ_L_MAX];           // feature id of landmark l,
    __shared__ int s_rel[SEQ_L_MAX];           // its match (rank among the matched landmarks << 10 | index in the match list) or -1
    __shared__ int s_misc[4];
    const BaLayout& L = *Lp;
    const int w = blockIdx.x, tid = threadIdx.x, K = S.K, WS = K - 1, Kp = L.Kp;
    SeqTab T = seq_table(S, cur, w);
    int* ia = P.iarr + (size_t)w * L.istride;
    double* di = P.din + (size_t)w * L.dstride;
    int* info = S.info + (size_t)w * VG_SEQ_INFO_INTS;
    const int* sp = S.sp + (size_t)w * S.sp_stride;
    const int n = T.hdr[0];
    const int margin = ia[L.io_hdr + H_MARGIN];
    // ---- relocalisation frame of this step (staging header [5 .. 7]; a sequence without the loop-pose block never looks)
    const int* ii = S.in_i + (size_t)w * S.ii_stride;
    int n_match = (Kp > K && S.MM) ? ii[5] : 0;
    if (n_match < 0 || n_match > S.MM) n_match = 0;                        // (the host refuses such a request)
    const int relo_frame = n_match ? ii[6] : 0;
    for (int k = tid; k < n_match; k += SEQ_NT) s_mid[k] = S.relo_i[(size_t)w * S.MM + k];
    __syncthreads();
    // ---- clear the tables a host pack would have zero-filled (the IMU validity flags and the owner task list stay)
    for (int k = tid; k < BA_HDR_INTS; k += SEQ_NT) ia[L.io_hdr + k] = 0;
    for (int k = L.io_lm_start + tid; k < L.io_task_list; k += SEQ_NT) ia[k] = 0;        // lm_start .. pair_ptr
    for (int k = L.io_pb_kind + tid; k < L.istride; k += SEQ_NT) ia[k] = 0;
    // ---- the landmark list: used_num >= 2 && start_frame < WINDOW_SIZE - 2, in list order (estimator.cpp:722-725)
    for (int f = tid; f < n; f += SEQ_NT) s_in[f] = (T.nobs[f] >= 2 && T.start[f] < WS - 2) ? 1 : 0;
    __syncthreads();
    {
        const int cnt = seq_compact(s_in, s_lm, n, tid);
        if (tid == 0) s_misc[0] = cnt;
    }
    __syncthreads();
    int nL = s_misc[0];
    int status = info[VG_SEQ_STATUS];
    if (nL > L.Lcap || nL > SEQ_L_MAX) { nL = 0; status = VG_ERR_UNSUPPORTED; }
    for (int f = tid; f < n; f += SEQ_NT) {
        const int l = nL ? s_lm[f] : -1;
        T.lm[f] = l;
        if (l >= 0) { s_ls[l] = T.start[f]; s_ln[l] = T.nobs[f]; s_feat[l] = f; s_lid[l] = T.id[f]; }
    }
    __syncthreads();
    if (tid == 0) {
        // the offsets of every landmark's factors and rows; beside them the reference's walk over match_points (estimator.cpp:776-799):
        // landmarks in list order, only those anchored at or before the loop frame; the cursor moves on while the match id is below the
        // feature id, an equal id takes the match and moves on.  Past the end means "no more matches" (the reference reads past the end
        // there; oracle/ref_stubs/ref_driver.cpp defines that memory as ids no feature has).  With ids ascending along the list this
        // is set membership; along a list that is not ascending, matches are skipped exactly as the reference skips them.
        int fb = 0, ob = 0, cursor = 0, nrel = 0;
        for (int l = 0; l < nL; ++l) {
            int r = -1;
            if (n_match && s_ls[l] <= relo_frame) {
                const int id = s_lid[l];
                while (cursor < n_match && s_mid[cursor] < id) ++cursor;
                if (cursor < n_match && s_mid[cursor] == id) { r = (nrel << 10) | cursor; ++cursor; ++nrel; }
            }
            s_rel[l] = r;
            s_fbeg[l] = fb; s_off[l] = ob; fb += s_ln[l] - 1 + (r >= 0 ? 1 : 0); ob += s_ln[l];
        }
        s_fbeg[nL] = fb; s_off[nL] = ob;
        s_misc[1] = fb; s_misc[2] = ob; s_misc[3] = nrel;
    }
    __syncthreads();
    int F = s_misc[1], nobs_tot = s_misc[2], n_relo = s_misc[3];
    if (F > L.Fcap || nobs_tot + n_relo > L.Ocap) { nL = 0; F = 0; nobs_tot = 0; n_relo = 0; status = VG_ERR_UNSUPPORTED; }
    const bool armed = n_match != 0;                                      // (a void step consumes the relocalisation frame too)
    // ---- per landmark: start frame, first factor, inverse depth (vector2double: 1 / estimated_depth, :519-522), observation rows,
    //      factors (first observation -> every later one, :732-763)
    for (int l = tid; l < nL; l += SEQ_NT) {
        const int f = s_feat[l], s = s_ls[l], no = s_ln[l], o = s_off[l], fb = s_fbeg[l];
        ia[L.io_lm_start + l] = s;
        ia[L.io_lm_fbeg + l] = fb;
        di[L.do_lam + l] = 1.0 / T.depth[f];
        for (int k = 1; k < no; ++k) {
            const int q = fb + k - 1;
            ia[L.io_fac_i + q] = s; ia[L.io_fac_j + q] = s + k; ia[L.io_fac_lm + q] = l;
            ia[L.io_fac_oi + q] = o; ia[L.io_fac_oj + q] = o + k;
        }
        if (s_rel[l] >= 0) {                                              // ProjectionFactor(first observation, matched point) on
            const int q = fb + no - 1, rank = s_rel[l] >> 10, m = s_rel[l] & 1023;      // (para_Pose[start], relo_Pose, ex, depth): behind
            const int row = nobs_tot + rank;                              // the landmark's window factors, its row behind the window's rows
            ia[L.io_fac_i + q] = s; ia[L.io_fac_j + q] = K; ia[L.io_fac_lm + q] = l;
            ia[L.io_fac_oi + q] = o; ia[L.io_fac_oj + q] = row;
            const double* xy = S.relo_d + (size_t)w * (8 + 2 * S.MM) + 8 + 2 * m;
            double* d = di + L.do_obs + (size_t)row * BA_OBS_STRIDE;
            d[0] = xy[0]; d[1] = xy[1];
            for (int c = 2; c < BA_OBS_STRIDE; ++c) d[c] = 0.0;
        }
    }
    if (tid == 0) ia[L.io_lm_fbeg + nL] = F;
    for (int l = nL + tid; l < L.Lcap; l += SEQ_NT) di[L.do_lam + l] = 0.0;
    for (int e = tid; e < nobs_tot * 8; e += SEQ_NT) {                    // rows [x y u v vx vy cur_td | 0]
        const int row = e >> 3, c = e & 7;
        // landmark of this row: binary search in the offsets
        int lo = 0, hi = nL - 1;
        while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (s_off[mid] <= row) lo = mid; else hi = mid - 1; }
        const int f = s_feat[lo], j = row - s_off[lo];
        di[L.do_obs + (size_t)row * BA_OBS_STRIDE + c] = (c < 7) ? T.obs[((size_t)f * K + j) * 8 + c] : 0.0;
    }
    for (int e = (nobs_tot + n_relo) * 8 + tid; e < L.Ocap * BA_OBS_STRIDE; e += SEQ_NT) di[L.do_obs + e] = 0.0;
    // ---- the loop pose, block K: relo_Pose as given, or the resident pose of the loop frame as this step found it (the add kernel
    //      writes slot K - 1 only); the unit pose while the window is not armed, every step, as pack_window writes it
    if (Kp > K && tid < 7) {
        double v = tid == 6 ? 1.0 : 0.0;
        if (armed) v = ii[7] ? S.relo_d[(size_t)w * (8 + 2 * S.MM) + tid] : di[L.do_pose + 7 * relo_frame + tid];
        di[L.do_pose + 7 * K + tid] = v;
    }
    // ---- slot table: records sorted by (anchor, target) pair, landmark order inside a pair (pack_window)
    //      (target K is the loop pose: a landmark has a factor there when the walk gave it a match, not by its length)
    for (int p = tid; p < Kp * Kp; p += SEQ_NT) {
        const int i = p / Kp, j = p % Kp, d = j - i;
        int c = 0;
        if (d > 0) for (int l = 0; l < nL; ++l) c += (s_ls[l] == i && (j < K ? s_ln[l] > d : s_rel[l] >= 0)) ? 1 : 0;
        s_pair[p] = c;
    }
    __syncthreads();
    if (tid == 0) {
        int acc = 0;
        for (int p = 0; p < Kp * Kp; ++p) { const int c = s_pair[p]; s_pair[p] = acc; acc += c; }
        s_pair[Kp * Kp] = acc;
    }
    __syncthreads();
    for (int p = tid; p <= Kp * Kp; p += SEQ_NT) ia[L.io_pair_ptr + p] = s_pair[p];
    for (int p = tid; p < Kp * Kp; p += SEQ_NT) {
        const int i = p / Kp, j = p % Kp, d = j - i;
        if (d <= 0) continue;
        int cursor = s_pair[p];
        for (int l = 0; l < nL; ++l)
            if (s_ls[l] == i && (j < K ? s_ln[l] > d : s_rel[l] >= 0)) ia[L.io_fac_slot + s_fbeg[l] + (j < K ? d : s_ln[l]) - 1] = cursor++;
    }
    if (tid == 0) {
        // wavefront owner tasks (pack_window): every block except the diagonal pose blocks and the blocks among ex / td
        const int nb = Kp + L.e + L.t;
        int q = 0;
        for (int br = 0; br < nb; ++br)
            for (int bc = 0; bc <= br; ++bc)
                if (!(br == bc && br < Kp) && !(bc >= Kp)) ia[L.io_task_list + q++] = br * (br + 1) / 2 + bc;
        // the prior's block table: where the rows / columns of J0 sit in the solver's ordering
        const int pn = sp[0], pnb = pn ? sp[1] : 0;
        int off = 0, x0off = 0;
        for (int b = 0; b < pnb; ++b) {
            const int kind = sp[2 + b], idx = sp[2 + (K + 4) + b];
            ia[L.io_pb_kind + b] = kind; ia[L.io_pb_idx + b] = idx; ia[L.io_pb_off + b] = off; ia[L.io_pb_x0off + b] = x0off;
            int col = -1;
            if (kind == VG_BLK_POSE) col = 6 * idx;
            else if (kind == VG_BLK_SPEEDBIAS) col = L.Rc + 9 * idx;
            else if (kind == VG_BLK_EXPOSE) col = L.e ? 6 * Kp : -1;
            else col = L.t ? 6 * Kp + 6 * L.e : -1;
            ia[L.io_pb_col + b] = col;
            off += kind == VG_BLK_SPEEDBIAS ? 9 : (kind == VG_BLK_TD ? 1 : 6);
            x0off += kind == VG_BLK_SPEEDBIAS ? 9 : (kind == VG_BLK_TD ? 1 : 7);
        }
        int* hdr = ia + L.io_hdr;
        hdr[H_L] = nL; hdr[H_F] = F; hdr[H_NPRIOR] = pn; hdr[H_NBLK] = pnb; hdr[H_MAXIT] = S.max_iters; hdr[H_NCHUNK] = 1;
        hdr[H_MARGIN] = margin; hdr[H_STATUS] = 0; hdr[H_MARGMODE] = S.marg_mode;
        info[VG_SEQ_N_LANDMARKS] = nL; info[VG_SEQ_N_FACTORS] = F; info[VG_SEQ_STATUS] = status;
        if (S.MM) {
            int* ro = S.relo_out + (size_t)w * 4;
            ro[0] = armed ? 1 : 0; ro[1] = n_relo; ro[2] = armed ? relo_frame : 0; ro[3] = 0;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(SEQ_NT) void ba_seq_slide_kernel(const BaLayout* __restrict__ Lp, BaPtrs P, SeqDev S, int cur) {
    __shared__ int s_alive[SEQ_FT_MAX], s_dst[SEQ_FT_MAX], s_ns[SEQ_FT_MAX], s_nn[SEQ_FT_MAX], s_src[SEQ_FT_MAX], s_skip[SEQ_FT_MAX];
    __shared__ int s_fl[SEQ_FT_MAX];
    __shared__ double s_dep[SEQ_FT_MAX];
    __shared__ double s_tf[24];                // R0 (9), P0 (3), R1 (9), P1 (3) of removeBackShiftDepth
    __shared__ int s_misc[4];
    const BaLayout& L = *Lp;
    const int w = blockIdx.x, tid = threadIdx.x, K = S.K, WS = K - 1;
    SeqTab T = seq_table(S, cur, w), N = seq_table(S, cur ^ 1, w);
    int* ia = P.iarr + (size_t)w * L.istride;
    double* di = P.din + (size_t)w * L.dstride;
    const double* out = P.out + (size_t)w * L.ostride;
    int* info = S.info + (size_t)w * VG_SEQ_INFO_INTS;
    const int n = T.hdr[0];
    const int flag = ia[L.io_hdr + H_MARGIN];
    if (tid == 0) {
        // slideWindowOld (estimator.cpp:1115-1126): R0 = back_R0 ric, P0 = back_P0 + back_R0 tic; R1 = Rs[0] ric, P1 = Ps[0] + Rs[0] tic
        // with back_* = frame 0 and Rs[0] / Ps[0] = frame 1 of the window just solved, ric / tic as solved
        double qe[4] = {out[L.oo_ex + 3], out[L.oo_ex + 4], out[L.oo_ex + 5], out[L.oo_ex + 6]}, Ric[9];
        q_normalize(qe);
        q_to_R(qe, Ric);
        const double Tic[3] = {out[L.oo_ex], out[L.oo_ex + 1], out[L.oo_ex + 2]};
        for (int k = 0; k < 2; ++k) {
            const double* x = out + L.oo_pose + 7 * k;
            double q[4] = {x[3], x[4], x[5], x[6]}, R[9], t[3];
            q_normalize(q);
            q_to_R(q, R);
            m3_mul(R, Ric, s_tf + 12 * k);
            m3_vec(R, Tic, t);
            for (int c = 0; c < 3; ++c) s_tf[12 * k + 9 + c] = x[c] + t[c];
        }
    }
    __syncthreads();
    // ---- per track: setDepth, then removeBackShiftDepth / removeFront, then removeFailures
    for (int f = tid; f < n; f += SEQ_NT) {
        const int st = T.start[f], no = T.nobs[f], l = T.lm[f];
        double dep = T.depth[f];
        int fl = T.sflag[f];
        if (l >= 0) {                                                     // FeatureManager::setDepth (feature_manager.cpp:141-159)
            dep = 1.0 / out[L.oo_lam + l];
            fl = dep < 0 ? 2 : 1;
        }
        int alive = 1, ns = st, nn = no, src = 0, skip = -1;
        if (flag == VG_MARGIN_OLD) {
            if (st != 0) ns = st - 1;
            else {
                nn = no - 1; src = 1;
                if (nn < 2) alive = 0;
                else {
                    const double* r = T.obs + (size_t)f * K * 8;
                    const double pi[3] = {r[0] * dep, r[1] * dep, r[7] * dep};           // uv_i * estimated_depth
                    double wp[3], d[3], pj[3];
                    m3_vec(s_tf, pi, wp);
                    for (int c = 0; c < 3; ++c) d[c] = wp[c] + s_tf[9 + c] - s_tf[21 + c];   // marg_R pts_i + marg_P - new_P
                    m3t_vec(s_tf + 12, d, pj);
                    dep = pj[2] > 0 ? pj[2] : S.init_depth;
                }
            }
        } else {                                                          // removeFront(frame_count = WINDOW_SIZE)
            if (st == WS) ns = st - 1;
            else {
                const int j = WS - 1 - st;
                if (no - 1 >= j) { skip = j; nn = no - 1; if (nn == 0) alive = 0; }
            }
        }
        if (fl == 2) alive = 0;                                           // removeFailures
        s_alive[f] = alive; s_ns[f] = ns; s_nn[f] = nn; s_src[f] = src; s_skip[f] = skip; s_dep[f] = dep; s_fl[f] = fl;
    }
    __syncthreads();
    {
        const int cnt = seq_compact(s_alive, s_dst, n, tid);
        if (tid == 0) { s_misc[0] = cnt; N.hdr[0] = cnt; info[VG_SEQ_N_AFTER] = cnt; }
    }
    __syncthreads();
    for (int f = tid; f < n; f += SEQ_NT) {
        const int d = s_dst[f];
        if (d < 0) continue;
        N.id[d] = T.id[f]; N.start[d] = s_ns[f]; N.nobs[d] = s_nn[f]; N.sflag[d] = s_fl[f]; N.lm[d] = -1; N.depth[d] = s_dep[f];
    }
    for (int e = tid; e < n * K * 8; e += SEQ_NT) {
        const int f = e / (K * 8), r = e - f * (K * 8), jj = r >> 3, c = r & 7;
        const int d = s_dst[f];
        if (d < 0 || jj >= s_nn[f]) continue;
        int sj = s_src[f] + jj;
        if (s_skip[f] >= 0 && sj >= s_skip[f]) ++sj;
        N.obs[((size_t)d * K + jj) * 8 + c] = T.obs[((size_t)f * K + sj) * 8 + c];
    }
    // ---- states and pre-integrations (estimator.cpp:1010-1050 / :1069-1099); the newest slot keeps a copy of the newest frame
    for (int e = tid; e < 7 * K; e += SEQ_NT) {
        const int k = e / 7, c = e - 7 * k;
        int from;
        if (flag == VG_MARGIN_OLD) from = k < K - 1 ? k + 1 : K - 1;
        else from = k <= K - 3 ? k : K - 1;
        di[L.do_pose + e] = out[L.oo_pose + 7 * from + c];
    }
    for (int e = tid; e < 9 * K; e += SEQ_NT) {
        const int k = e / 9, c = e - 9 * k;
        int from;
        if (flag == VG_MARGIN_OLD) from = k < K - 1 ? k + 1 : K - 1;
        else from = k <= K - 3 ? k : K - 1;
        di[L.do_sb + e] = out[L.oo_sb + 9 * from + c];
    }
    if (tid < 7) di[L.do_ex + tid] = out[L.oo_ex + tid];
    if (tid == 7) di[L.do_td] = out[L.oo_td];
    if (flag == VG_MARGIN_OLD) {
        for (int e = tid; e < 467; e += SEQ_NT)
            for (int k = 0; k + 1 < K - 1; ++k)
                di[L.do_imu + (size_t)k * BA_IMU_STRIDE + e] = di[L.do_imu + (size_t)(k + 1) * BA_IMU_STRIDE + e];
        if (tid == 0) for (int k = 0; k + 1 < K - 1; ++k) ia[L.io_imu_valid + k] = ia[L.io_imu_valid + k + 1];
    }
    // ---- the new prior's block table (the factor itself is moved by ba_carry_prior_kernel); none produced: the old one stays
    const int* mi = P.miout + (size_t)w * L.mi_stride;
    int* sp = S.sp + (size_t)w * S.sp_stride;
    if (mi[0]) {
        if (tid == 0) { sp[0] = mi[1]; sp[1] = mi[3]; }
        for (int b = tid; b < K + 4; b += SEQ_NT) { sp[2 + b] = mi[8 + b]; sp[2 + (K + 4) + b] = mi[8 + (K + 4) + b]; }
    } else if (flag == VG_MARGIN_OLD) {
        // A MARGIN_OLD step whose marginalization produced nothing (a non-finite solve): the frames and tracks have been shifted
        // above, the old prior still names the un-shifted blocks -- it must not survive (the drop-in drops last_marginalization_info
        // in the same situation, host/dropin/estimator_optimization.cpp).  The window goes on without a prior and the
        // step reports VG_ERR_NUMERIC in info[VG_SEQ_STATUS], so that the caller can re-seed it (vg_ba_seq_import).
        // (MARGIN_SECOND_NEW without Pose[WINDOW_SIZE - 1] in the prior legitimately produces nothing: the old prior stays, its
        //  blocks keep their slots, estimator.cpp:933-936.)
        if (tid == 0) {
            sp[0] = 0; sp[1] = 0;
            int* info = S.info + (size_t)w * VG_SEQ_INFO_INTS;
            if (info[VG_SEQ_STATUS] == VG_OK) info[VG_SEQ_STATUS] = VG_ERR_NUMERIC;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Estimator::processIMU (estimator.cpp:84-118) for the samples of one frame, one wavefront per window, in front of ba_seq_add_kernel:
// pre_integrations[WINDOW_SIZE]->push_back into a fresh record (csrc/imu_step.h: the arithmetic of vg_imu_preintegrate) linearised at
// the biases of slot K-1 and started from the resident acc_0 / gyr_0, beside it the mid-point propagation of Ps / Rs / Vs[WINDOW_SIZE]
// (:107-114; wave-uniform 3x3 work that the compiler schedules into the LDS waits of the 15x15 products).  Rs is the matrix of the
// normalised quaternion of slot K-1, multiplied per sample by the matrix of the normalised deltaQ (the project's restatement,
// oracle/window_numpy.py propagate), and goes back as a normalised quaternion.
// rotation matrix -> quaternion with w >= 0 wherever w resolves (the convention of the project's restatement, synth._R2q: a
// guess whose quaternion keeps its sign from frame to frame; Eigen's conversion (R_to_q) takes over for w < 1e-3)
DEV void R_to_q_wpos(const double* m, double* q) {
    const double w = sqrt(fmax(1e-300, 1 + m[0] + m[4] + m[8])) / 2;
    if (w > 1e-3) {
        q[0] = (m[7] - m[5]) / (4 * w); q[1] = (m[2] - m[6]) / (4 * w); q[2] = (m[3] - m[1]) / (4 * w); q[3] = w;
    } else {
        int i = 0;
        if (m[4] > m[0]) i = 1;
        if (m[8] > m[i * 4]) i = 2;
        const int j = (i + 1) % 3, k = (i + 2) % 3;
        double t = sqrt(m[i * 4] - m[j * 4] - m[k * 4] + 1.0);
        q[i] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (m[k * 3 + j] - m[j * 3 + k]) * t;
        q[j] = (m[j * 3 + i] + m[i * 3 + j]) * t;
        q[k] = (m[k * 3 + i] + m[i * 3 + k]) * t;
    }
}

extern "C" __global__ __launch_bounds__(64) void ba_seq_imu_kernel(const BaLayout* __restrict__ Lp, BaPtrs P, SeqDev S) {
    __shared__ ImuPreLds s;
    const BaLayout& L = *Lp;
    const int w = blockIdx.x, lane = threadIdx.x, K = S.K;
    int* ia = P.iarr + (size_t)w * L.istride;
    double* di = P.din + (size_t)w * L.dstride;
    const double* smp = S.in_d + (size_t)w * S.id_stride;
    double* st = S.imu_st + (size_t)w * SEQ_IMU_ST;
    double* xp = di + L.do_pose + 7 * (K - 1);
    double* xs = di + L.do_sb + 9 * (K - 1);
    int ns = S.in_i[(size_t)w * S.ii_stride + 4];
    if (ns > S.MS) ns = S.MS;                                             // (the host refuses such a frame)
    double first[6], bias[6], g[3], Pw[3], Vw[3], R[9];
#pragma unroll
    for (int i = 0; i < 6; ++i) { first[i] = st[i]; bias[i] = xs[3 + i]; }
#pragma unroll
    for (int i = 0; i < 3; ++i) { g[i] = st[6 + i]; Pw[i] = xp[i]; Vw[i] = xs[i]; }
    {
        double q[4] = {xp[3], xp[4], xp[5], xp[6]};
        q_normalize(q);
        q_to_R(q, R);
    }
    ImuRun r;
    imu_enter(s, r, nullptr, first, bias, S.noise[0], S.noise[1], S.noise[2], S.noise[3], lane);
    for (int k = 0; k < ns; ++k) {
        const double* sm = smp + (size_t)k * 7;
        {   // Ps / Rs / Vs[WINDOW_SIZE] (:107-114), from acc_0 / gyr_0 as they are BEFORE push_back moves them on
            const double dt = sm[0];
            const double a0[3] = {r.acc0[0] - r.ba[0], r.acc0[1] - r.ba[1], r.acc0[2] - r.ba[2]};
            const double a1[3] = {sm[1] - r.ba[0], sm[2] - r.ba[1], sm[3] - r.ba[2]};
            double u0[3], u1[3], dR[9], Rn[9];
            m3_vec(R, a0, u0);
            double dq[4] = {(0.5 * (r.gyr0[0] + sm[4]) - r.bg[0]) * dt / 2, (0.5 * (r.gyr0[1] + sm[5]) - r.bg[1]) * dt / 2,
                            (0.5 * (r.gyr0[2] + sm[6]) - r.bg[2]) * dt / 2, 1.0};
            q_normalize(dq);
            q_to_R(dq, dR);
            m3_mul(R, dR, Rn);
            m3_vec(Rn, a1, u1);
#pragma unroll
            for (int i = 0; i < 9; ++i) R[i] = Rn[i];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double ua = 0.5 * ((u0[i] - g[i]) + (u1[i] - g[i]));
                Pw[i] = Pw[i] + dt * Vw[i] + 0.5 * dt * dt * ua;
                Vw[i] = Vw[i] + dt * ua;
            }
        }
        imu_push_back(s, r, sm, lane);
    }
    imu_leave(s, r, di + L.do_imu + (size_t)(K - 2) * BA_IMU_STRIDE, lane);
    if (lane == 1) ia[L.io_imu_valid + (K - 2)] = (r.sum_dt <= 10.0) ? 1 : 0;
    if (lane == 0) {
        double q[4];
        R_to_q_wpos(R, q);
        q_normalize(q);
        for (int i = 0; i < 3; ++i) { xp[i] = Pw[i]; xs[i] = Vw[i]; st[16 + i] = Pw[i]; st[23 + i] = Vw[i]; }
        for (int i = 0; i < 4; ++i) { xp[3 + i] = q[i]; st[19 + i] = q[i]; }
        for (int i = 0; i < 6; ++i) { st[26 + i] = bias[i]; st[9 + i] = first[i]; }
        for (int i = 0; i < 3; ++i) { st[i] = r.acc0[i]; st[3 + i] = r.gyr0[i]; }
    }
}

// The IMU part of slideWindow() after a dropped non-keyframe (estimator.cpp:1069-1081): pre_integrations[WINDOW_SIZE - 1] -- record
// K-3 after the slide -- takes this frame's samples.  No sample history: the stored record IS the state push_back continues from
// (sum_dt, delta_p / q / v, jacobian, covariance, its own linearisation biases), the samples are still in the frame staging, and the
// measurement that ended the record is the one ba_seq_imu_kernel kept.  Windows that marginalized the oldest frame leave at once.
extern "C" __global__ __launch_bounds__(64) void ba_seq_merge_kernel(const BaLayout* __restrict__ Lp, BaPtrs P, SeqDev S) {
    __shared__ ImuPreLds s;
    const BaLayout& L = *Lp;
    const int w = blockIdx.x, lane = threadIdx.x, K = S.K;
    if (S.info[(size_t)w * VG_SEQ_INFO_INTS + VG_SEQ_FLAG] != VG_MARGIN_SECOND_NEW) return;
    int* ia = P.iarr + (size_t)w * L.istride;
    double* rec = P.din + (size_t)w * L.dstride + L.do_imu + (size_t)(K - 3) * BA_IMU_STRIDE;
    const double* smp = S.in_d + (size_t)w * S.id_stride;
    const double* st = S.imu_st + (size_t)w * SEQ_IMU_ST;
    int ns = S.in_i[(size_t)w * S.ii_stride + 4];
    if (ns > S.MS) ns = S.MS;
    ImuRun r;
    imu_enter(s, r, rec, st + 9, nullptr, S.noise[0], S.noise[1], S.noise[2], S.noise[3], lane);
    for (int k = 0; k < ns; ++k) imu_push_back(s, r, smp + (size_t)k * 7, lane);
    imu_leave(s, r, rec, lane);
    if (lane == 1) ia[L.io_imu_valid + (K - 3)] = (ia[L.io_imu_valid + (K - 3)] && r.sum_dt <= 10.0) ? 1 : 0;
}

// what slideWindow() leaves in the newest slot: a copy of the frame before it (vg_ba_seq_imu_begin / vg_ba_seq_import in IMU mode)
extern "C" __global__ __launch_bounds__(64) void ba_seq_imu_seed_kernel(const BaLayout* __restrict__ Lp, BaPtrs P, SeqDev S, int w0) {
    const BaLayout& L = *Lp;
    const int w = w0 + blockIdx.x, t = threadIdx.x, K = S.K;
    double* di = P.din + (size_t)w * L.dstride;
    if (t < 7) di[L.do_pose + 7 * (K - 1) + t] = di[L.do_pose + 7 * (K - 2) + t];
    else if (t < 16) di[L.do_sb + 9 * (K - 1) + (t - 7)] = di[L.do_sb + 9 * (K - 2) + (t - 7)];
}

// ---------------------------------------------------------------------------------------------------------------------------
// vg_vio_step_async: the message the front end's commit kernel (fe_tk_commit_kernel, fe_frame.hip) left in HBM for stream w goes to
// where ba_seq_add_kernel reads the frame of window w, in front of ba_seq_imu_kernel.  One workgroup per stream / window.
//   ints     ii[0] = n_msg, ii[4] = n_samples, ii[5 .. 7] = the relocalisation request (vg_ba_seq_set_relo; 0 without one), the rest of the header 0; ids behind it (16-byte copies when max_points is a multiple of 4:
//            the streams' id lists are max_points ints apart)
//   doubles  the samples from the step's packed upload to the front of the staging; the rows [x y z u v vx vy] -> [x y z u v vx vy 0]
//            at rows_off: 64 rows at a time through LDS -- 224 16-byte loads of the packed 7-double rows (two scalar loads where the
//            stream's rows start at an odd double) and 256 16-byte stores, one quarter row per thread
// The staging is at the CAPACITY strides of vg_ba_seq_imu_begin: the host does not know n_msg before the launch.  n_msg is written as
// it is and the copy clamped at NIN: ba_seq_add_kernel reports the over-capacity frame, as on the host-fed path.
extern "C" __global__ __launch_bounds__(SEQ_NT) void ba_seq_bridge_kernel(SeqDev S, const int* __restrict__ tk_hdr, const int* __restrict__ msg_id,
                                                                         const double* __restrict__ msg_obs, int cap,
                                                                         const double* __restrict__ smp, int smp_stride) {
    __shared__ double s_row[64 * 7];
    const int w = blockIdx.x, tid = threadIdx.x;
    int* ii = S.in_i + (size_t)w * S.ii_stride;
    double* idd = S.in_d + (size_t)w * S.id_stride;
    const double* sw = smp + (size_t)w * smp_stride;
    const int n_msg = tk_hdr[(size_t)w * TK_HDR_INTS + TK_NMSG];
    const int ns_in = *(const int*)sw;
    const int ns = ns_in < 0 ? 0 : (ns_in > S.MS ? S.MS : ns_in);         // (the host refuses such a frame)
    const int nin = n_msg < 0 ? 0 : (n_msg > S.NIN ? S.NIN : n_msg);
    // (ints 1 .. 3 of the sample block's header: the relocalisation request of this step, zero in every other step)
    if (tid < 8) ii[tid] = tid == 0 ? n_msg : (tid == 4 ? ns_in : (tid >= 5 ? ((const int*)sw)[tid - 4] : 0));
    // ---- samples: 7 ns doubles, pairs (an odd count takes the zero the host padded with; rows_off >= up8(7 MS))
    for (int k = tid; k < (7 * ns + 1) >> 1; k += SEQ_NT) ((double2*)idd)[k] = ((const double2*)(sw + 8))[k];
    // ---- ids
    const int* mid = msg_id + (size_t)w * cap;
    const int nq = (cap & 3) == 0 ? nin >> 2 : 0;
    for (int k = tid; k < nq; k += SEQ_NT) ((int4*)(ii + 8))[k] = ((const int4*)mid)[k];
    for (int i = 4 * nq + tid; i < nin; i += SEQ_NT) ii[8 + i] = mid[i];
    // ---- rows
    const double* src = msg_obs + (size_t)w * cap * 7;
    double* rows = idd + S.rows_off;
    const bool al = (((size_t)w * cap * 7) & 1) == 0;                     // (msg_obs itself is 256-byte aligned; 64 rows are 448 doubles)
    for (int r0 = 0; r0 < nin; r0 += 64) {
        const int rem = (nin - r0 < 64 ? nin - r0 : 64) * 7;
        const double* p = src + (size_t)r0 * 7;
        const int e = 2 * tid;
        if (e + 1 < rem && al) {
            const double2 v = *(const double2*)(p + e);
            s_row[e] = v.x; s_row[e + 1] = v.y;
        } else {
            if (e < rem) s_row[e] = p[e];
            if (e + 1 < rem) s_row[e + 1] = p[e + 1];
        }
        __syncthreads();
        const int r = tid >> 2, q = tid & 3;
        if (r0 + r < nin) {
            double2 v;
            v.x = s_row[7 * r + 2 * q];
            v.y = q < 3 ? s_row[7 * r + 2 * q + 1] : 0.0;
            *(double2*)(rows + (size_t)(r0 + r) * 8 + 2 * q) = v;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// vg_ba_seq_outputs_async: what the estimator node publishes between two frames (estimator_node.cpp:321-328), from the window as it
// stands in HBM.  pubKeyframe (vins_estimator/src/utility/visualization.cpp:348-404): the pose of frame WINDOW_SIZE - 2 and, for every
// solved track seen in that frame, its world point, the observation in that frame and the id; pubPointCloud (:240-296): the world
// points of the solved landmarks and the margin cloud.  One workgroup per window.  Reads the CURRENT track table (the one the last slide
// wrote, or vg_ba_seq_begin / vg_ba_seq_import filled) and the states of the input slab (after slideWindow() and removeFailures());
// writes only the window's block of `out`: nothing resident changes.
//   keyframe list   start < W - 2 && start + n_obs - 1 >= W - 2 && solve_flag == 1                              (:378)
//   point cloud     n_obs >= 2 && start < W - 2 && !(start > W * 3.0 / 4.0) && solve_flag == 1                  (:251-254)
//                   (the 3/4 test is vacuous for every K a sequence accepts: start <= W - 3 <= 0.75 W whenever W <= 12; it is evaluated
//                    all the same, as the reference writes it)
//   margin cloud    n_obs >= 2 && start < W - 2 && start == 0 && n_obs <= 2 && solve_flag == 1                  (:276-282)
// each in track-list order (seq_compact).  World point, in FP64, rounded to float32 only by the store (the messages carry Point32):
//   w = Rs[s] (ric (point0 depth) + tic) + Ps[s],  s = start_frame, point0 = first observation (x, y, z),
// Rs / ric the matrices of the normalised quaternions, as ba_seq_tri_kernel takes them.
// The window's block, in 4-byte words (vg_ba_seq_get_outputs unpacks it):
//   [0] status  [1] keyframe_valid  [2] n_keyframe  [3] n_cloud  [4] n_margin (true counts)  [5 .. 7] 0
//   [8 .. 36)   14 doubles: pose of frame W - 2 (px py pz qx qy qz qw), ex_pose (tic, ric as stored)
//   [36 ..)     keyframe rows, 8 words each: w (3 float) | x y u v of the observation in frame W - 2 (4 float) | id (int)
//   then        cloud rows, then margin rows, 3 floats each; every list has room for MP rows
// More selected tracks than MP: the first MP of the list are stored, the count stays the true one, status = VG_SEQ_OUT_TRUNCATED.
// A window whose last step was void reports that step's status and three zero counts.  stepped = 0 (no step since vg_ba_seq_begin):
// the info words are not a step's, keyframe_valid = 0 and the status starts from VG_OK.
#define SEQ_OUT_HDR 36
extern "C" __global__ __launch_bounds__(SEQ_NT) void ba_seq_publish_kernel(const BaLayout* __restrict__ Lp, BaPtrs P, SeqDev S, int cur, int stepped,
                                                                          int* __restrict__ out, int MP, int ostride) {
    __shared__ int s_kf[SEQ_FT_MAX], s_pc[SEQ_FT_MAX], s_mg[SEQ_FT_MAX];
    __shared__ double s_R[9 * BA_MAX_K], s_P[3 * BA_MAX_K], s_ex[12];       // Rs, Ps; ric (9) tic (3)
    __shared__ int s_cnt[3];
    const BaLayout& L = *Lp;
    const int w = blockIdx.x, tid = threadIdx.x, K = S.K, WS = K - 1;
    SeqTab T = seq_table(S, cur, w);
    const double* di = P.din + (size_t)w * L.dstride;
    const int* info = S.info + (size_t)w * VG_SEQ_INFO_INTS;
    int* o = out + (size_t)w * ostride;
    const int step_status = stepped ? info[VG_SEQ_STATUS] : VG_OK;
    const int n = step_status == VG_OK ? T.hdr[0] : 0;
    if (tid < K) {
        const double* x = di + L.do_pose + 7 * tid;
        double q[4] = {x[3], x[4], x[5], x[6]};
        q_normalize(q);
        q_to_R(q, s_R + 9 * tid);
        s_P[3 * tid] = x[0]; s_P[3 * tid + 1] = x[1]; s_P[3 * tid + 2] = x[2];
    } else if (tid == K) {                                                 // (the thread behind the K that take the poses)
        const double* ex = di + L.do_ex;
        double q[4] = {ex[3], ex[4], ex[5], ex[6]};
        q_normalize(q);
        q_to_R(q, s_ex);
        s_ex[9] = ex[0]; s_ex[10] = ex[1]; s_ex[11] = ex[2];
    }
    for (int f = tid; f < n; f += SEQ_NT) {
        const int st = T.start[f], no = T.nobs[f];
        const int solved = T.sflag[f] == 1;
        const int in_problem = no >= 2 && st < WS - 2;
        s_kf[f] = (st < WS - 2 && st + no - 1 >= WS - 2 && solved) ? 1 : 0;
        s_pc[f] = (in_problem && !((double)st > WS * 3.0 / 4.0) && solved) ? 1 : 0;
        s_mg[f] = (in_problem && st == 0 && no <= 2 && solved) ? 1 : 0;
    }
    __syncthreads();
    {
        const int c0 = seq_compact(s_kf, s_kf, n, tid);                    // (in place: an entry is read and written by the same lane)
        const int c1 = seq_compact(s_pc, s_pc, n, tid);
        const int c2 = seq_compact(s_mg, s_mg, n, tid);
        if (tid == 0) { s_cnt[0] = c0; s_cnt[1] = c1; s_cnt[2] = c2; }
    }
    __syncthreads();
    // ---- the header
    if (tid == 0) {
        int status = step_status;
        if (s_cnt[0] > MP || s_cnt[1] > MP || s_cnt[2] > MP) status = VG_SEQ_OUT_TRUNCATED;
        o[0] = status;
        o[1] = (stepped && info[VG_SEQ_FLAG] == VG_MARGIN_OLD) ? 1 : 0;   // marginalization_flag == 0 (:351)
        o[2] = s_cnt[0]; o[3] = s_cnt[1]; o[4] = s_cnt[2]; o[5] = 0; o[6] = 0; o[7] = 0;
    }
    double* od = (double*)(o + 8);
    if (tid < 7) od[tid] = di[L.do_pose + 7 * (WS - 2) + tid];
    else if (tid < 14) od[tid] = di[L.do_ex + (tid - 7)];
    // ---- the rows
    float* kf = (float*)(o + SEQ_OUT_HDR);
    float* pc = kf + (size_t)8 * MP;
    float* mg = pc + (size_t)3 * MP;
    for (int f = tid; f < n; f += SEQ_NT) {
        const int dk = s_kf[f], dp = s_pc[f], dm = s_mg[f];
        const bool k_on = dk >= 0 && dk < MP, p_on = dp >= 0 && dp < MP, m_on = dm >= 0 && dm < MP;
        if (!(k_on || p_on || m_on)) continue;
        const int st = T.start[f];
        const double dep = T.depth[f];
        const double* r0 = T.obs + (size_t)f * K * 8;                      // [x y u v vx vy cur_td z]
        const double px = r0[0] * dep, py = r0[1] * dep, pz = r0[7] * dep;
        const double cx = s_ex[0] * px + s_ex[1] * py + s_ex[2] * pz + s_ex[9];
        const double cy = s_ex[3] * px + s_ex[4] * py + s_ex[5] * pz + s_ex[10];
        const double cz = s_ex[6] * px + s_ex[7] * py + s_ex[8] * pz + s_ex[11];
        const double* R = s_R + 9 * st;
        const float wx = (float)(R[0] * cx + R[1] * cy + R[2] * cz + s_P[3 * st]);
        const float wy = (float)(R[3] * cx + R[4] * cy + R[5] * cz + s_P[3 * st + 1]);
        const float wz = (float)(R[6] * cx + R[7] * cy + R[8] * cz + s_P[3 * st + 2]);
        if (k_on) {
            const double* rj = r0 + (size_t)(WS - 2 - st) * 8;
            float* d = kf + (size_t)8 * dk;
            d[0] = wx; d[1] = wy; d[2] = wz;
            d[3] = (float)rj[0]; d[4] = (float)rj[1]; d[5] = (float)rj[2]; d[6] = (float)rj[3];
            ((int*)d)[7] = T.id[f];
        }
        if (p_on) { float* d = pc + (size_t)3 * dp; d[0] = wx; d[1] = wy; d[2] = wz; }
        if (m_on) { float* d = mg + (size_t)3 * dm; d[0] = wx; d[1] = wy; d[2] = wz; }
    }
}
extern "C" int ba_seq_out_stride(int max_points) { return (SEQ_OUT_HDR + 14 * max_points + 3) / 4 * 4; }     // words per window, a multiple of 16 bytes
extern "C" int ba_seq_out_hdr_words() { return SEQ_OUT_HDR; }
extern "C" hipError_t ba_seq_launch_publish(const BaLayout& L, const BaLayout* dL, const BaPtrs& P, const SeqDev& S, int cur, int stepped, int* out,
                                            int max_points, hipStream_t stream) {
    hipLaunchKernelGGL(ba_seq_publish_kernel, dim3(L.nwin), dim3(SEQ_NT), 0, stream, dL, P, S, cur, stepped, out, max_points, ba_seq_out_stride(max_points));
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------------
extern "C" hipError_t ba_seq_launch_bridge(const BaLayout& L, const SeqDev& S, const int* tk_hdr, const int* msg_id, const double* msg_obs, int cap,
                                           const double* smp, int smp_stride, hipStream_t stream) {
    hipLaunchKernelGGL(ba_seq_bridge_kernel, dim3(L.nwin), dim3(SEQ_NT), 0, stream, S, tk_hdr, msg_id, msg_obs, cap, smp, smp_stride);
    return hipGetLastError();
}
extern "C" hipError_t ba_seq_launch_imu(const BaLayout& L, const BaLayout* dL, const BaPtrs& P, const SeqDev& S, hipStream_t stream) {
    hipLaunchKernelGGL(ba_seq_imu_kernel, dim3(L.nwin), dim3(64), 0, stream, dL, P, S);
    return hipGetLastError();
}
extern "C" hipError_t ba_seq_launch_merge(const BaLayout& L, const BaLayout* dL, const BaPtrs& P, const SeqDev& S, hipStream_t stream) {
    hipLaunchKernelGGL(ba_seq_merge_kernel, dim3(L.nwin), dim3(64), 0, stream, dL, P, S);
    return hipGetLastError();
}
extern "C" hipError_t ba_seq_launch_imu_seed(const BaLayout* dL, const BaPtrs& P, const SeqDev& S, int w0, int n, hipStream_t stream) {
    hipLaunchKernelGGL(ba_seq_imu_seed_kernel, dim3(n), dim3(64), 0, stream, dL, P, S, w0);
    return hipGetLastError();
}
extern "C" hipError_t ba_seq_launch_front(const BaLayout& L, const BaLayout* dL, const BaPtrs& P, const SeqDev& S, int cur, hipStream_t stream) {
    hipLaunchKernelGGL(ba_seq_add_kernel, dim3(L.nwin), dim3(SEQ_NT), 0, stream, dL, P, S, cur);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ba_seq_tri_kernel, dim3(L.nwin, (S.FT + 63) / 64), dim3(64), 0, stream, dL, P, S, cur);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(ba_seq_build_kernel, dim3(L.nwin), dim3(SEQ_NT), 0, stream, dL, P, S, cur);
    return hipGetLastError();
}
extern "C" hipError_t ba_seq_launch_slide(const BaLayout& L, const BaLayout* dL, const BaPtrs& P, const SeqDev& S, int cur, hipStream_t stream) {
    hipLaunchKernelGGL(ba_seq_slide_kernel, dim3(L.nwin), dim3(SEQ_NT), 0, stream, dL, P, S, cur);
    return hipGetLastError();
}
extern "C" int ba_seq_relo_max_match() { return SEQ_MM_MAX < 1024 ? SEQ_MM_MAX : 1024; }     // (a match index takes 10 bits of s_rel)
extern "C" int ba_seq_limits(int* ft_max, int* nin_max, int* hdr_ints, int* in_rows_off) {
    if (ft_max) *ft_max = SEQ_FT_MAX;
    if (nin_max) *nin_max = SEQ_NIN_MAX;
    if (hdr_ints) *hdr_ints = SEQ_HDR;
    if (in_rows_off) *in_rows_off = SEQ_IN_ROWS;
    return SEQ_L_MAX;
}
