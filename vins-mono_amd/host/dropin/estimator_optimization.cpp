// estimator_optimization.cpp — THE drop-in for the back end: `void Estimator::optimization()` of the REFERENCE class
// (vins_estimator/src/estimator.h:47, body at estimator.cpp:670-1003) on the MI355X path.
//
// How it is used.  This file includes the reference's own "estimator.h" and defines exactly one member function of the
// reference's `class Estimator`.  In a catkin workspace: add this file, include/vinsgpu.h and host/vg_pack.h (header-only: the
// packers it shares with the project's own classes) to vins_estimator, link libvinsgpu.so, and remove (or
// `objcopy --weaken-symbol=_ZN9Estimator12optimizationEv`) the definition in estimator.cpp —
// nothing else of the package changes: processIMU / processImage / solveOdometry / slideWindow / vector2double /
// double2vector / FeatureManager / MarginalizationInfo are the reference's, and they call this body where they called
// Ceres.  Here (no Eigen / Ceres / ROS in the image) oracle/Makefile target `ref_gpu` does precisely that against the
// header stand-ins of oracle/ref_stubs and produces oracle/_ref/libvins_ref_gpu.so; tests/test_dropin_gpu.py drives the
// reference's processIMU / processImage loop through it and through the all-reference build side by side.
//
// What the body does instead of estimator.cpp:670-1003:
//   :672-701  ceres::Problem + parameter blocks      -> vector2double() (the reference's), then plain tables
//   :703-801  AddResidualBlock (prior, IMU, projection, relocalisation factors) -> vg_ba_problem (same selection rules)
//   :803-818  ceres::Solve(DENSE_SCHUR, DOGLEG)      -> vg_ba_optimize_begin: solve + gauge fix on the device, states back
//   :823      double2vector()                        -> the reference's own (its yaw / position fix is idempotent on the
//                                                       already fixed states; it also forms the relocalisation by-products)
//   :825-1000 MarginalizationInfo machinery          -> runs on the device BEHIND the state download; picked up at the next
//                                                       call (or by vins_gpu_collect_prior) and stored into the reference's
//                                                       own MarginalizationInfo / last_marginalization_parameter_blocks
// State the reference class has no member for (device handle, pending prior) lives in a side table keyed by `this`.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "estimator.h"
#include "vinsgpu.h"
#include "vg_pack.h"

namespace {

struct VgSide {
    vg_handle* vg = nullptr;
    bool prior_pending = false;   // optimization() has returned, its marginalization result is still on the device
    bool solver_failed = false;   // the device reported a non-finite solve
    // What the window looked like when the result was left on the device: the pending prior belongs to the window that
    // CONTINUES that one.  Both slides leave the newest frame of then at index WINDOW_SIZE - 1 (estimator.cpp:1037-1041,
    // :1078-1079), and optimization() itself is the only writer of last_marginalization_info besides clearState() (:70-76).
    double pending_stamp = 0;                               // Headers[WINDOW_SIZE].stamp at that time
    const MarginalizationInfo* pending_lmi = nullptr;       // last_marginalization_info at that time (not yet replaced)
    vg_ba_summary last;           // trace of the last solve (the reference only logs Summary::BriefReport)
    // run-time behaviour switches (vins_gpu_set_option)
    bool solver_time_cap = false; // forward SOLVER_TIME as max_solver_time_in_seconds (estimator.cpp:812-815)
    bool marg_eigen = false;      // the reference's eigen form of the prior instead of the pivoted-Cholesky square root
    bool marg_mode_dirty = false;
    bool imu_info_reference = false, imu_info_dirty = false;
};
std::mutex g_mu;
std::unordered_map<const Estimator*, VgSide> g_side;
VgSide& side_of(const Estimator* e) {
    std::lock_guard<std::mutex> lock(g_mu);
    return g_side[e];             // (references into an unordered_map stay valid across inserts)
}

// The marginalization result of the last optimization() -> last_marginalization_info / ..._parameter_blocks
// (estimator.cpp:926-929 / :992-996), as the reference's own types.
void collect_prior(Estimator& e, VgSide& s) {
    if (!s.prior_pending) return;
    s.prior_pending = false;
    // (before the caller's slideWindow() the frame is still at WINDOW_SIZE; afterwards both slides leave it at WINDOW_SIZE - 1)
    const bool continues = e.Headers[WINDOW_SIZE - 1].stamp.toSec() == s.pending_stamp || e.Headers[WINDOW_SIZE].stamp.toSec() == s.pending_stamp;
    if (e.last_marginalization_info != s.pending_lmi || !continues) {
        // clearState() ran in between (failureDetection() in processImage, estimator.cpp:190-200, or the restart callback,
        // estimator_node.cpp:182-198): it freed last_marginalization_info and the window now on the host is a fresh one.  The
        // result on the device describes the trajectory before the reset -- the reference has no prior here, so neither do we.
        // (Nothing to fetch: the next upload is ordered behind the marginalization kernel on the handle's stream.)
        return;
    }
    vg_pack::PriorOut buf(WINDOW_SIZE + 1);
    vg_ba_prior& pr = buf.pr;
    if (vg_ba_optimize_prior(s.vg, &pr) != VG_OK) throw std::runtime_error(std::string("vg_ba_optimize_prior: ") + vg_last_error(s.vg));
    if (s.solver_failed) {
        // no new prior exists, and the old one must not survive the caller's slideWindow() (it names un-shifted blocks)
        if (e.last_marginalization_info) delete e.last_marginalization_info;
        e.last_marginalization_info = nullptr;
        e.last_marginalization_parameter_blocks.clear();
        return;
    }
    if (!pr.valid) return;        // MARGIN_SECOND_NEW without Pose[WINDOW_SIZE-1] in the prior: the old prior stays (:935-936)
    vg_pack::install_prior(e, pr, pr.m);
    // the members only the reference's MarginalizationInfo has: ~MarginalizationInfo frees the linearisation points through
    // parameter_block_data (marginalization_factor.cpp:71-87), so every installed block is entered there, keyed by its address
    MarginalizationInfo* mi = e.last_marginalization_info;
    mi->sum_block_size = 0;
    for (size_t b = 0; b < mi->keep_block_data.size(); ++b) {
        const long addr = reinterpret_cast<long>(e.last_marginalization_parameter_blocks[b]);
        mi->parameter_block_data[addr] = mi->keep_block_data[b];
        mi->parameter_block_size[addr] = mi->keep_block_size[b];
        mi->parameter_block_idx[addr] = mi->keep_block_idx[b];
        mi->sum_block_size += mi->keep_block_size[b];
    }
}

}  // namespace

void Estimator::optimization() {
    VgSide& s = side_of(this);
    if (vg_abi_version() != VG_ABI_VERSION) throw std::runtime_error("libvinsgpu.so was built from another include/vinsgpu.h (ABI version mismatch)");
    if (!s.vg) {
        if (vg_create(&s.vg) != VG_OK) throw std::runtime_error("vg_create failed: no MI355X / libvinsgpu (no CPU fallback)");
    }
    // form of the prior factor the marginalization hands to the next frame: the pivoted-Cholesky square root (default) or the
    // reference's eigen form (marginalization_factor.cpp:285-296) -- vins_gpu_set_option(e, VINS_GPU_OPT_MARG_EIGEN, 1); include/vinsgpu.h
    if (s.marg_mode_dirty) { vg_ba_set_marg_mode(s.vg, s.marg_eigen ? VG_MARG_EIGEN : VG_MARG_SQRT); s.marg_mode_dirty = false; }
    if (s.imu_info_dirty) { vg_ba_set_imu_info_mode(s.vg, s.imu_info_reference ? VG_IMU_INFO_REFERENCE : VG_IMU_INFO_FACTOR); s.imu_info_dirty = false; }
    collect_prior(*this, s);                                    // the previous frame's marginalization result, if still on the device
    vector2double();                                            // estimator.cpp:701
    const int K = WINDOW_SIZE + 1;
    // ---- factor tables instead of problem.AddResidualBlock (:719-764, same filter), relocalisation factors (:769-801)
    vg_pack::FactorTables ft;
    vg_pack::collect_factors(*this, WINDOW_SIZE, ft);
    const int L = (int)ft.lm_start.size();
    // ---- IMUFactor(pre_integrations[j]), j = i + 1 (:711-718)
    std::vector<vg_imu_preint> imu(K - 1);
    for (int i = 0; i < WINDOW_SIZE; i++) vg_pack::preint_to_abi(imu[i], pre_integrations[i + 1]);
    vg_ba_problem pb;
    memset(&pb, 0, sizeof(pb));
    pb.K = K; pb.L = L; pb.n_obs = (int)ft.obs.size() / 7;
    pb.pose = &para_Pose[0][0]; pb.speedbias = &para_SpeedBias[0][0]; pb.ex_pose = &para_Ex_Pose[0][0]; pb.td = ESTIMATE_TD ? para_Td[0][0] : td;
    pb.inv_depth = &para_Feature[0][0];
    pb.lm_start = ft.lm_start.data(); pb.lm_nobs = ft.lm_nobs.data(); pb.lm_obs_off = ft.lm_off.data(); pb.obs = ft.obs.data(); pb.imu = imu.data();
    // ---- MarginalizationFactor(last_marginalization_info) on last_marginalization_parameter_blocks (:703-709)
    vg_pack::PriorIn prior;
    vg_pack::prior_to_problem(*this, prior, pb);
    const bool relo_in_problem = relocalization_info && !ft.relo_lm.empty();
    if (relo_in_problem) {
        pb.relo_n = (int)ft.relo_lm.size(); pb.relo_pose = relo_Pose; pb.relo_lm = ft.relo_lm.data(); pb.relo_xy = ft.relo_xy.data();
    }
    pb.estimate_extrinsic = ESTIMATE_EXTRINSIC ? 1 : 0; pb.estimate_td = ESTIMATE_TD ? 1 : 0; pb.max_iters = NUM_ITERATIONS;
    pb.focal = FOCAL_LENGTH; pb.tr = TR; pb.row = ROW; pb.g_norm = G.z();
    // options.max_solver_time_in_seconds (:812-815): a wall-clock cap makes the result depend on timing (oracle/ASSUMPTIONS.md C7)
    // and 40 ms is 30 x what a solve takes here, so it is NOT forwarded unless the caller asks for the reference's contract to the
    // letter: vins_gpu_set_option(e, VINS_GPU_OPT_SOLVER_TIME_CAP, 1) (a run-time switch)
    if (s.solver_time_cap) pb.max_solver_time_s = marginalization_flag == MARGIN_OLD ? SOLVER_TIME * 4.0 / 5.0 : SOLVER_TIME;
    // ---- outputs
    std::vector<double> lam(L > 0 ? L : 1);
    double td_out = td;
    vg_ba_state st;
    st.pose = &para_Pose[0][0]; st.speedbias = &para_SpeedBias[0][0]; st.ex_pose = &para_Ex_Pose[0][0]; st.td = ESTIMATE_TD ? &para_Td[0][0] : &td_out;
    st.inv_depth = lam.data(); st.relo_pose = pb.relo_n ? relo_Pose : nullptr;
    const int flag = marginalization_flag == MARGIN_OLD ? VG_MARGIN_OLD : VG_MARGIN_SECOND_NEW;
    const int rc = vg_ba_optimize_begin(s.vg, &pb, flag, &st, &s.last);
    if (rc != VG_OK && rc != VG_ERR_NUMERIC) throw std::runtime_error(std::string("vg_ba_optimize_begin: ") + vg_last_error(s.vg));
    for (int l = 0; l < L; ++l) para_Feature[l][0] = lam[l];
    if (relocalization_info && !relo_in_problem) {
        // relo_Pose carried no factor: the reference leaves it untouched by the solve and gauge-fixes it in double2vector
        // (:598-603) with the rot_diff / para_Pose[0] it derives there; the device has applied that transform to the window
        // already, so it is applied to relo_Pose here (vg_ba_summary::gauge_*) and double2vector's own transform is the identity
        Matrix3d rot;
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) rot(r, c) = s.last.gauge_rot[3 * r + c];
        const Matrix3d Rr = rot * Quaterniond(relo_Pose[6], relo_Pose[3], relo_Pose[4], relo_Pose[5]).normalized().toRotationMatrix();
        const Vector3d tr = rot * Vector3d(relo_Pose[0] - s.last.gauge_p0[0], relo_Pose[1] - s.last.gauge_p0[1], relo_Pose[2] - s.last.gauge_p0[2])
                            + Vector3d(para_Pose[0][0], para_Pose[0][1], para_Pose[0][2]);
        const Quaterniond q(Rr);
        relo_Pose[0] = tr.x(); relo_Pose[1] = tr.y(); relo_Pose[2] = tr.z();
        relo_Pose[3] = q.x(); relo_Pose[4] = q.y(); relo_Pose[5] = q.z(); relo_Pose[6] = q.w();
    }
    double2vector();                                            // :823 (the reference's)
    s.solver_failed = rc == VG_ERR_NUMERIC;
    s.prior_pending = true;
    s.pending_stamp = Headers[WINDOW_SIZE].stamp.toSec();
    s.pending_lmi = last_marginalization_info;
    if (s.solver_failed) collect_prior(*this, s);              // (drops the priors, see there)
}

// ---- C entry points for the surrounding code (the reference class has no member to hang these on)
extern "C" {
// fetch the marginalization result of the last optimization() now (tests, serialisation of last_marginalization_info)
void vins_gpu_collect_prior(Estimator* e) { collect_prior(*e, side_of(e)); }
// forget a pending marginalization result: for callers that reset the estimator by other means than clearState()
void vins_gpu_reset(Estimator* e) {
    VgSide& s = side_of(e);
    s.prior_pending = false; s.solver_failed = false;
}
// behaviour switches of one Estimator (run time, no environment variables): VINS_GPU_OPT_SOLVER_TIME_CAP forwards SOLVER_TIME as
// max_solver_time_in_seconds (estimator.cpp:812-815; default off), VINS_GPU_OPT_MARG_EIGEN asks for the reference's eigen form of
// the prior instead of the square root (default off), VINS_GPU_OPT_IMU_INFO_REFERENCE (3) for the IMU factors' sqrt_info formed as
// imu_factor.h:64 spells it, inverse() then LLT (vg_ba_set_imu_info_mode; default off).  Takes effect at the next optimization().  Returns 0, -1 for an unknown option.
int vins_gpu_set_option(Estimator* e, int option, int value) {
    VgSide& s = side_of(e);
    if (option == 1) { s.solver_time_cap = value != 0; return 0; }                                       // VINS_GPU_OPT_SOLVER_TIME_CAP
    if (option == 2) { s.marg_eigen = value != 0; s.marg_mode_dirty = true; return 0; }                  // VINS_GPU_OPT_MARG_EIGEN
    if (option == 3) { s.imu_info_reference = value != 0; s.imu_info_dirty = true; return 0; }           // VINS_GPU_OPT_IMU_INFO_REFERENCE
    return -1;
}
// trace of the last solve
const vg_ba_summary* vins_gpu_last_summary(Estimator* e) { return &side_of(e).last; }
int vins_gpu_last_iterations(Estimator* e) { return side_of(e).last.num_iterations; }
// release the device handle of an Estimator that is about to be destroyed
void vins_gpu_release(Estimator* e) {
    std::lock_guard<std::mutex> lock(g_mu);
    auto it = g_side.find(e);
    if (it == g_side.end()) return;
    if (it->second.vg) vg_destroy(it->second.vg);
    g_side.erase(it);
}
}
