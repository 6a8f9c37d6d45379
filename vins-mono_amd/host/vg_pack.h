// vg_pack.h — the packers between the classes' members and the C-ABI (include/vinsgpu.h), ONCE, for the project's classes
// (estimator.h / feature_tracker.h on compat/) and for the drop-ins written against the reference's own headers (host/dropin/).
//
// Header-only, C++14, standard library + vinsgpu.h only: every function is a template over the class types (E an Estimator, IB an
// IntegrationBase, T a FeatureTracker; the point type is taken from T's own lists), so both sets of types instantiate the same body.
// Include it AFTER the class header.  Of the member types only x() / y() / z() / w(), operator(), rows() / cols(), resize(), data()
// and the (w, x, y, z) quaternion constructor are used.  What the callers do differently on purpose (side tables, camera, gauge
// transform of relo_Pose, configuration globals) stays in their own files.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <type_traits>
#include <utility>
#include <vector>
#include "vinsgpu.h"

namespace vg_pack {

// =================================================================================================================== back end

// IntegrationBase -> vg_imu_preint (what IMUFactor reads); a null pointer = no factor for this pair (valid = 0, all zero)
template <class IB> void preint_to_abi(vg_imu_preint& m, const IB* p) {
    std::memset(&m, 0, sizeof(m));
    if (!p) return;
    m.valid = 1; m.sum_dt = p->sum_dt;
    for (int k = 0; k < 3; ++k) { m.delta_p[k] = p->delta_p(k); m.delta_v[k] = p->delta_v(k); m.linearized_ba[k] = p->linearized_ba(k); m.linearized_bg[k] = p->linearized_bg(k); }
    m.delta_q[0] = p->delta_q.x(); m.delta_q[1] = p->delta_q.y(); m.delta_q[2] = p->delta_q.z(); m.delta_q[3] = p->delta_q.w();
    for (int r = 0; r < 15; ++r)                                // Eigen is column-major, the C-ABI row-major: convert explicitly
        for (int c = 0; c < 15; ++c) { m.jacobian[r * 15 + c] = p->jacobian(r, c); m.covariance[r * 15 + c] = p->covariance(r, c); }
}

// vg_imu_preint -> the record fields of an IntegrationBase; the raw samples (dt_buf / acc_buf / gyr_buf, linearized_acc / _gyr) stay
// with the callers that have them
template <class IB> void preint_from_abi(IB& p, const vg_imu_preint& m) {
    typedef typename std::decay<decltype(p.delta_q)>::type Quat;
    p.sum_dt = m.sum_dt;
    for (int k = 0; k < 3; ++k) { p.delta_p(k) = m.delta_p[k]; p.delta_v(k) = m.delta_v[k]; p.linearized_ba(k) = m.linearized_ba[k]; p.linearized_bg(k) = m.linearized_bg[k]; }
    p.delta_q = Quat(m.delta_q[3], m.delta_q[0], m.delta_q[1], m.delta_q[2]);
    for (int r = 0; r < 15; ++r)
        for (int c = 0; c < 15; ++c) { p.jacobian(r, c) = m.jacobian[r * 15 + c]; p.covariance(r, c) = m.covariance[r * 15 + c]; }
}

// sizes of a parameter block: global (para_* doubles) and local (columns of the prior; the pose blocks lose one)
inline int block_global_size(int kind) { return kind == VG_BLK_SPEEDBIAS ? 9 : (kind == VG_BLK_TD ? 1 : 7); }
inline int local_size(int global_size) { return global_size == 7 ? 6 : global_size; }

// (kind, frame index) of a parameter-block address inside para_Pose / para_SpeedBias / para_Ex_Pose / para_Td, and back
template <class E> bool block_of(E& e, const double* addr, int& kind, int& index) {
    const int frames = (int)(sizeof(e.para_Pose) / sizeof(e.para_Pose[0]));
    for (int i = 0; i < frames; ++i) {
        if (addr == e.para_Pose[i]) { kind = VG_BLK_POSE; index = i; return true; }
        if (addr == e.para_SpeedBias[i]) { kind = VG_BLK_SPEEDBIAS; index = i; return true; }
    }
    if (addr == e.para_Ex_Pose[0]) { kind = VG_BLK_EXPOSE; index = 0; return true; }
    if (addr == e.para_Td[0]) { kind = VG_BLK_TD; index = 0; return true; }
    return false;
}
template <class E> double* block_addr(E& e, int kind, int index) {
    return kind == VG_BLK_POSE ? e.para_Pose[index] : kind == VG_BLK_SPEEDBIAS ? e.para_SpeedBias[index] : kind == VG_BLK_EXPOSE ? e.para_Ex_Pose[0] : e.para_Td[0];
}

// The factor tables of optimization() instead of problem.AddResidualBlock (estimator.cpp:719-801)
struct FactorTables {
    std::vector<int> lm_start, lm_nobs, lm_off;     // per optimised landmark: first frame, observations, first row of obs
    std::vector<double> obs;                        // rows of 7: point x y, uv, velocity, cur_td
    std::vector<int> relo_lm;                       // relocalisation factors: landmark index ...
    std::vector<double> relo_xy;                    // ... and matched point
};
template <class E> void collect_factors(E& e, int window_size, FactorTables& t) {
    for (auto& it : e.f_manager.feature) {          // the filter of FeatureManager::getFeatureCount / getDepthVector
        it.used_num = it.feature_per_frame.size();
        if (!(it.used_num >= 2 && it.start_frame < window_size - 2)) continue;
        t.lm_start.push_back(it.start_frame);
        t.lm_nobs.push_back((int)it.feature_per_frame.size());
        t.lm_off.push_back((int)t.obs.size() / 7);
        for (auto& f : it.feature_per_frame) {
            const double row[7] = {f.point.x(), f.point.y(), f.uv.x(), f.uv.y(), f.velocity.x(), f.velocity.y(), f.cur_td};
            t.obs.insert(t.obs.end(), row, row + 7);
        }
    }
    // relocalisation factors (:769-801): ProjectionFactor(first observation, matched point) on (para_Pose[start], relo_Pose, ex, depth)
    // for every optimised landmark that started at or before the loop frame and has a match (match_points are sorted by feature id,
    // like f_manager.feature)
    if (!e.relocalization_info) return;
    size_t retrive = 0;
    int feature_index = -1;
    for (auto& it : e.f_manager.feature) {
        if (!(it.used_num >= 2 && it.start_frame < window_size - 2)) continue;
        ++feature_index;
        if (it.start_frame > e.relo_frame_local_index) continue;
        while (retrive < e.match_points.size() && (int)e.match_points[retrive].z() < it.feature_id) ++retrive;
        if (retrive < e.match_points.size() && (int)e.match_points[retrive].z() == it.feature_id) {
            t.relo_lm.push_back(feature_index);
            t.relo_xy.push_back(e.match_points[retrive].x());
            t.relo_xy.push_back(e.match_points[retrive].y());
            ++retrive;
        }
    }
}

// MarginalizationFactor(last_marginalization_info) on last_marginalization_parameter_blocks (:703-709) -> the prior fields of a
// vg_ba_problem.  The blocks are identified by their para_* ADDRESSES, as in the reference; the C-ABI wants (kind, frame index).  The
// columns of linearized_jacobians are addressed through keep_block_idx - m (marginalization_factor.cpp:343-378): they are gathered
// into the block order of last_marginalization_parameter_blocks.  `b` owns what pb then points to.
struct PriorIn {
    std::vector<int> kind, index;
    std::vector<double> J0, r0, x0;
};
template <class E> void prior_to_problem(E& e, PriorIn& b, vg_ba_problem& pb) {
    if (!e.last_marginalization_info) return;
    auto* mi = e.last_marginalization_info;
    const int n = mi->n, nb = (int)mi->keep_block_size.size();
    const int ncols = (int)mi->linearized_jacobians.cols();
    b.J0.assign((size_t)n * n, 0.0);
    int col = 0;
    for (int k = 0; k < nb; ++k) {
        int kind, index;
        if (!block_of(e, e.last_marginalization_parameter_blocks[k], kind, index)) throw std::runtime_error("prior block address outside the para_* arrays");
        b.kind.push_back(kind); b.index.push_back(index);
        const int gs = mi->keep_block_size[k], ls = local_size(gs), src = mi->keep_block_idx[k] - mi->m;
        b.x0.insert(b.x0.end(), mi->keep_block_data[k], mi->keep_block_data[k] + gs);
        if (src < 0 || src + ls > ncols || col + ls > n) throw std::runtime_error("prior block outside linearized_jacobians");
        for (int r = 0; r < n; ++r)
            for (int c = 0; c < ls; ++c) b.J0[(size_t)r * n + col + c] = mi->linearized_jacobians(r, src + c);
        col += ls;
    }
    if (col != n) throw std::runtime_error("prior: kept blocks do not cover the n columns");
    b.r0.resize(n);
    for (int r = 0; r < n; ++r) b.r0[r] = mi->linearized_residuals(r);
    pb.prior_n = n; pb.prior_nblocks = nb;
    pb.prior_block_kind = b.kind.data(); pb.prior_block_index = b.index.data();
    pb.prior_J0 = b.J0.data(); pb.prior_r0 = b.r0.data(); pb.prior_x0 = b.x0.data();
}

// Download buffers of a vg_ba_prior for a window of K frames (x0 holds 9 doubles per block at most: speed-bias); `pr` is the view
struct PriorOut {
    std::vector<int> kind, index;
    std::vector<double> J0, r0, x0;
    vg_ba_prior pr;
    explicit PriorOut(int K) : kind(K + 8), index(K + 8), J0((size_t)(6 * K + 32) * (6 * K + 32)), r0(6 * K + 32), x0(9 * (K + 8)) {
        std::memset(&pr, 0, sizeof(pr));
        pr.cap = 6 * K + 32; pr.cap_blocks = K + 8; pr.block_kind = kind.data(); pr.block_index = index.data();
        pr.J0 = J0.data(); pr.r0 = r0.data(); pr.x0 = x0.data();
    }
    PriorOut(const PriorOut&) = delete;
    PriorOut& operator=(const PriorOut&) = delete;
};

// last_marginalization_info = marginalization_info (estimator.cpp:926-929 / :992-996) from a vg_ba_prior: a new MarginalizationInfo
// (n, m, Jacobian, residuals, keep_block_size / idx / data; every keep_block_data[b] is a new double[]) and the blocks' addresses in
// the SLID window (addr_shift, :913-924 / :969-990: the device already re-labelled them).  The old MarginalizationInfo is deleted.
template <class E> void install_prior(E& e, const vg_ba_prior& pr, int m) {
    typedef typename std::remove_pointer<typename std::decay<decltype(e.last_marginalization_info)>::type>::type Info;
    Info* mi = new Info();
    mi->n = pr.n; mi->m = m;
    mi->linearized_jacobians.resize(pr.n, pr.n);
    mi->linearized_residuals.resize(pr.n);
    for (int r = 0; r < pr.n; ++r) {
        mi->linearized_residuals(r) = pr.r0[r];
        for (int c = 0; c < pr.n; ++c) mi->linearized_jacobians(r, c) = pr.J0[(size_t)r * pr.n + c];
    }
    std::vector<double*> blocks;
    int off = 0, x0o = 0;
    for (int b = 0; b < pr.nblocks; ++b) {
        const int gs = block_global_size(pr.block_kind[b]);
        mi->keep_block_size.push_back(gs);
        mi->keep_block_idx.push_back(m + off);
        double* d = new double[gs];
        std::memcpy(d, pr.x0 + x0o, sizeof(double) * gs);
        mi->keep_block_data.push_back(d);
        blocks.push_back(block_addr(e, pr.block_kind[b], pr.block_index[b]));
        off += local_size(gs); x0o += gs;
    }
    delete e.last_marginalization_info;
    e.last_marginalization_info = mi;
    e.last_marginalization_parameter_blocks = blocks;
}

// ---- initialisation: VisualIMUAlignment + the state change of visualInitialAlign (vg_init_align)
// all_image_frame -> vg_align_in.  Map: std::map<double, ImageFrame> of either set of types (second.R / second.T / second.pre_integration
// with dt_buf / acc_buf / gyr_buf / linearized_acc / linearized_gyr); interval k is the pre_integration of frame k + 1.  stamps: the
// n_stamps key frames of the window (Headers[0 .. frame_count].stamp.toSec()), 0 for none; each must be a key of the map.  `p` owns
// what p.in points to.
struct AlignIn {
    std::vector<double> R, T, samples, first;
    std::vector<int> off, key;
    vg_align_in in;
};
template <class Map, class V3>
void pack_align(const Map& frames, const double* stamps, int n_stamps, const V3& ba0, const V3& bg0, const double* noise, const V3& tic, double g_norm, AlignIn& p) {
    const int F = (int)frames.size();
    p.R.clear(); p.T.clear(); p.samples.clear(); p.first.clear(); p.off.assign(1, 0); p.key.clear();
    int k = 0;
    for (auto it = frames.begin(); it != frames.end(); ++it, ++k) {
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) p.R.push_back(it->second.R(r, c));
        for (int r = 0; r < 3; ++r) p.T.push_back(it->second.T(r));
        if (k == 0) continue;
        const auto* pre = it->second.pre_integration;
        if (!pre) throw std::runtime_error("pack_align: an ImageFrame behind the first has no pre_integration");
        for (int r = 0; r < 3; ++r) p.first.push_back(pre->linearized_acc(r));
        for (int r = 0; r < 3; ++r) p.first.push_back(pre->linearized_gyr(r));
        for (size_t i = 0; i < pre->dt_buf.size(); ++i) {
            p.samples.push_back(pre->dt_buf[i]);
            for (int r = 0; r < 3; ++r) p.samples.push_back(pre->acc_buf[i](r));
            for (int r = 0; r < 3; ++r) p.samples.push_back(pre->gyr_buf[i](r));
        }
        p.off.push_back((int)(p.samples.size() / 7));              // F entries: sample_off[k + 1] ends interval k
    }
    for (int i = 0; i < n_stamps; ++i) {
        const auto it = frames.find(stamps[i]);
        if (it == frames.end()) throw std::runtime_error("pack_align: a window stamp is not in all_image_frame");
        int pos = 0;
        for (auto jt = frames.begin(); jt != it; ++jt) ++pos;
        p.key.push_back(pos);
    }
    if (p.samples.empty()) p.samples.assign(7, 0.0);
    std::memset(&p.in, 0, sizeof(p.in));
    p.in.struct_size = sizeof(p.in);
    p.in.n_frames = F;
    p.in.R = p.R.data(); p.in.T = p.T.data(); p.in.sample_off = p.off.data(); p.in.samples = p.samples.data(); p.in.first = p.first.data();
    for (int r = 0; r < 3; ++r) { p.in.ba0[r] = ba0(r); p.in.bg0[r] = bg0(r); p.in.tic[r] = tic(r); }
    for (int r = 0; r < 4; ++r) p.in.noise[r] = noise[r];
    p.in.g_norm = g_norm;
    p.in.n_key = n_stamps; p.in.key = p.key.data();
}
// the download buffers of one window with F frames, K of them in the window; `out` is the view
struct AlignOut {
    std::vector<double> v_body, Ps, Rs, Vs;
    std::vector<vg_imu_preint> records;
    vg_align_out out;
    AlignOut(int F, int K) : v_body(3 * (size_t)F), Ps(3 * (size_t)K), Rs(9 * (size_t)K), Vs(3 * (size_t)K), records(F > 1 ? F - 1 : 1) {
        std::memset(&out, 0, sizeof(out));
        out.struct_size = sizeof(out);
        out.v_body = v_body.data(); out.records = records.data();
        if (K > 0) { out.Ps = Ps.data(); out.Rs = Rs.data(); out.Vs = Vs.data(); }
    }
    AlignOut(const AlignOut&) = delete;
    AlignOut& operator=(const AlignOut&) = delete;
};

// the walk over f_manager.feature that vg_sfm_in and vg_relpose_in share: one row of (id, start, nobs, obs_off) per feature, its points behind
template <class Features>
void pack_feature_tables(const Features& features, std::vector<int>& id, std::vector<int>& start, std::vector<int>& nobs, std::vector<int>& off,
                         std::vector<double>& points) {
    for (const auto& f : features) {
        id.push_back(f.feature_id); start.push_back(f.start_frame); nobs.push_back((int)f.feature_per_frame.size());
        off.push_back((int)(points.size() / 3));
        for (const auto& o : f.feature_per_frame)
            for (int r = 0; r < 3; ++r) points.push_back(o.point(r));
    }
}

// ---- initialisation: GlobalSFM::construct + the per-frame PnP of initialStructure (vg_init_sfm)
// f_manager.feature and all_image_frame -> vg_sfm_in.  Features: a list of FeaturePerId (feature_id, start_frame, feature_per_frame with
// .point); Map: std::map<double, ImageFrame> whose entries carry `points` (id -> vector of (camera, x y z u v vx vy)); stamps: the
// n_stamps key frames Headers[0 .. frame_count].stamp.toSec().  all_key / all_guess come from the walk of estimator.cpp:290-306: a
// counter i over the stamps; an entry whose stamp equals stamps[i] IS key frame i (i moves on); any other entry moves i on once when
// its stamp is past stamps[i], and takes the pose of i as its guess.  `p` owns what p.in points to.
struct SfmIn {
    std::vector<int> id, start, nobs, off, all_key, all_guess, all_off, all_id;
    std::vector<double> points, all_xy;
    vg_sfm_in in;
};
template <class Features, class Map, class M3, class V3>
void pack_sfm(const Features& features, const Map& frames, const double* stamps, int n_stamps, int l, const M3& relative_R, const V3& relative_T,
              const M3& ric, SfmIn& p) {
    p.id.clear(); p.start.clear(); p.nobs.clear(); p.off.clear(); p.points.clear();
    p.all_key.clear(); p.all_guess.clear(); p.all_off.assign(1, 0); p.all_id.clear(); p.all_xy.clear();
    pack_feature_tables(features, p.id, p.start, p.nobs, p.off, p.points);
    int i = 0;
    for (auto it = frames.begin(); it != frames.end(); ++it) {
        if (i < n_stamps && it->first == stamps[i]) {
            p.all_key.push_back(i); p.all_guess.push_back(i);
            ++i;
        } else {
            if (i < n_stamps && it->first > stamps[i]) ++i;
            if (i >= n_stamps) throw std::runtime_error("pack_sfm: a frame of all_image_frame lies behind the last window stamp");
            p.all_key.push_back(-1); p.all_guess.push_back(i);
            for (const auto& id_pts : it->second.points) {                     // (a std::map: ascending ids)
                if (id_pts.second.empty()) continue;
                p.all_id.push_back(id_pts.first);
                p.all_xy.push_back(id_pts.second[0].second(0, 0)); p.all_xy.push_back(id_pts.second[0].second(1, 0));
            }
        }
        p.all_off.push_back((int)p.all_id.size());
    }
    if (p.all_id.empty()) { p.all_id.assign(1, 0); p.all_xy.assign(2, 0.0); }
    std::memset(&p.in, 0, sizeof(p.in));
    p.in.struct_size = sizeof(p.in);
    p.in.n_frames = n_stamps; p.in.l = l;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) { p.in.relative_R[3 * r + c] = relative_R(r, c); p.in.ric[3 * r + c] = ric(r, c); }
        p.in.relative_T[r] = relative_T(r);
    }
    p.in.n_feat = (int)p.id.size();
    p.in.feature_id = p.id.data(); p.in.start = p.start.data(); p.in.nobs = p.nobs.data(); p.in.obs_off = p.off.data(); p.in.points = p.points.data();
    p.in.n_all = (int)p.all_key.size();
    p.in.all_key = p.all_key.data(); p.in.all_guess = p.all_guess.data(); p.in.all_off = p.all_off.data(); p.in.all_id = p.all_id.data();
    p.in.all_xy = p.all_xy.data();
}
// the download buffers of one window with F key frames, n features and A entries of all_image_frame; `out` is the view
struct SfmOut {
    std::vector<double> q, T, position, R_all, T_all;
    std::vector<int> state, is_key;
    vg_sfm_out out;
    SfmOut(int F, int n, int A) : q(4 * (size_t)F), T(3 * (size_t)F), position(3 * (size_t)n), R_all(9 * (size_t)A + 1), T_all(3 * (size_t)A + 1), state(n), is_key(A + 1) {
        std::memset(&out, 0, sizeof(out));
        out.struct_size = sizeof(out);
        out.q = q.data(); out.T = T.data(); out.position = position.data(); out.state = state.data();
        out.R_all = R_all.data(); out.T_all = T_all.data(); out.is_key = is_key.data();
    }
    SfmOut(const SfmOut&) = delete;
    SfmOut& operator=(const SfmOut&) = delete;
};

// ---- initialisation: Estimator::relativePose (vg_init_relpose) over the same feature tables; the constants are the reference's
struct RelposeIn {
    std::vector<int> id, start, nobs, off;
    std::vector<double> points;
    vg_relpose_in in;
};
template <class Features>
void pack_relpose(const Features& features, int n_frames, RelposeIn& p) {
    p.id.clear(); p.start.clear(); p.nobs.clear(); p.off.clear(); p.points.clear();
    pack_feature_tables(features, p.id, p.start, p.nobs, p.off, p.points);
    std::memset(&p.in, 0, sizeof(p.in));
    p.in.struct_size = sizeof(p.in);
    p.in.n_frames = n_frames; p.in.n_feat = (int)p.id.size();
    p.in.start = p.start.data(); p.in.nobs = p.nobs.data(); p.in.obs_off = p.off.data(); p.in.points = p.points.data();
    p.in.ransac_threshold = 0.3 / 460; p.in.confidence = 0.99; p.in.min_corres = 20; p.in.min_inliers = 12;      // solve_5pts.cpp:204, :221, estimator.cpp:449
    p.in.parallax_gate = 30; p.in.focal = 460; p.in.cheirality_dist = 50;                                        // estimator.cpp:460, solve_5pts.cpp:77
}
struct RelposeOut {
    vg_relpose_out out;
    RelposeOut() {
        std::memset(&out, 0, sizeof(out));
        out.struct_size = sizeof(out);
    }
};

// ---- initialisation: InitialEXRotation::CalibrationExRotation (vg_init_exrot), ONE step: the correspondences of (frame_count - 1,
// frame_count), the interval's delta_q, and the state the earlier steps left (records of 27 doubles each, ric); the constants are the
// reference's (initial_ex_rotation.cpp, cv::findFundamentalMat's defaults)
struct ExrotIn {
    int off[2];
    std::vector<double> corr, prev;
    double dq[4], ric[9];
    vg_exrot_in in;
};
template <class Corres, class Q, class M3>
void pack_exrot(const Corres& corres, const Q& delta_q, const std::vector<double>& records, const M3& ric, ExrotIn& p) {
    p.corr.assign(4 * corres.size() + 4, 0.0);                 // (never empty: the pointer is not NULL)
    for (size_t i = 0; i < corres.size(); ++i) {
        p.corr[4 * i] = corres[i].first(0); p.corr[4 * i + 1] = corres[i].first(1);
        p.corr[4 * i + 2] = corres[i].second(0); p.corr[4 * i + 3] = corres[i].second(1);
    }
    p.off[0] = 0; p.off[1] = (int)corres.size();
    p.dq[0] = delta_q.w(); p.dq[1] = delta_q.x(); p.dq[2] = delta_q.y(); p.dq[3] = delta_q.z();
    p.prev = records;
    for (int e = 0; e < 9; ++e) p.ric[e] = ric(e / 3, e % 3);
    std::memset(&p.in, 0, sizeof(p.in));
    p.in.struct_size = sizeof(p.in);
    p.in.n_steps = 1; p.in.corr_off = p.off; p.in.corr = p.corr.data(); p.in.delta_q = p.dq;
    p.in.n_prev = (int)(records.size() / 27); p.in.prev = p.prev.empty() ? nullptr : p.prev.data(); p.in.ric_prev = p.ric;
    p.in.ransac_threshold = 3.0; p.in.confidence = 0.99; p.in.min_points = 9;                   // initial_ex_rotation.cpp:71, :79
    p.in.huber_deg = 5.0; p.in.min_frames = 10; p.in.cov_threshold = 0.25;                      // :30, :60
}
struct ExrotOut {
    vg_exrot_out out;
    double records[27], ric[9], sigma[4], huber = 0;
    int ok = 0;
    ExrotOut() {
        std::memset(&out, 0, sizeof(out));
        out.struct_size = sizeof(out);
        out.records = records; out.ric = ric; out.sigma = sigma; out.huber = &huber; out.ok = &ok;
    }
    ExrotOut(const ExrotOut&) = delete;
    ExrotOut& operator=(const ExrotOut&) = delete;
};

// ================================================================================================================== front end

// reduceVector (feature_tracker.cpp:13-29) for any element type
template <class V> void reduce_vector(V& v, const std::vector<uint8_t>& status) {
    int j = 0;
    for (int i = 0; i < int(v.size()); i++)
        if (status[i]) v[j++] = v[i];
    v.resize(j);
}

template <class T> struct OrderCtx {
    typedef typename std::decay<decltype(std::declval<T&>().forw_pts)>::type::value_type Point2f;
    typedef std::vector<std::pair<int, std::pair<Point2f, int>>> SortedList;
    T* t;
    int n_in;
    SortedList sorted;               // setMask's cnt_pts_id (:43), the third field holding the list index instead of the id
};

// The reference's sort call (:47-51): same element type, same comparator, same std::sort.  std::sort by track_cnt is not stable: the
// order among equal counts is what the platform's std::sort makes of the sequence; the permutation depends on the outcomes of the
// comparisons only, and those look at the counts (tests/test_fe_dropin.py holds it against the reference's node).
template <class Point2f> void sort_by_count(std::vector<std::pair<int, std::pair<Point2f, int>>>& cnt_pts_id) {
    using std::pair;
    std::sort(cnt_pts_id.begin(), cnt_pts_id.end(),
              [](const pair<int, pair<Point2f, int>>& a, const pair<int, pair<Point2f, int>>& b) { return a.first > b.first; });
}

// vg_fe_order_fn with user = OrderCtx<T>*: the order of setMask's walk
template <class T> int order_callback(void* user, const vg_fe_frame_out* after, int* order) {
    typedef typename OrderCtx<T>::Point2f Point2f;
    OrderCtx<T>* c = static_cast<OrderCtx<T>*>(user);
    // The survivors with their counts (:115-128, :193-198: track_cnt++ after the tracking), formed ON THE SIDE: the tracker's own vectors
    // are only touched once the library call has returned VG_OK, so a frame that fails later (detection overflow, a HIP error) leaves
    // the tracker as it was
    c->sorted.clear();
    for (int i = 0, k = 0, idx = 0; i < c->n_in; i++) {
        if (!after->status_lk[i]) continue;
        const bool keep = !after->ransac_ran || after->status_f[k];
        k++;
        if (keep) c->sorted.push_back(std::make_pair(c->t->track_cnt[i] + 1, std::make_pair(Point2f(after->forw_xy[2 * i], after->forw_xy[2 * i + 1]), idx++)));
    }
    if ((int)c->sorted.size() != after->n2) return 1;
    sort_by_count(c->sorted);
    for (int q = 0; q < after->n2; q++) order[q] = c->sorted[q].second.second;
    return 0;
}

// What readImage does with the statuses of a frame (:115-128, :193-198): forw_pts as the tracking left them, reduceVector by
// `status && inBorder`, track_cnt++, reduceVector by findFundamentalMat's mask
template <class T> void apply_statuses(T& t, const vg_fe_frame_out& a, int n_in) {
    typedef typename OrderCtx<T>::Point2f Point2f;
    t.forw_pts.resize(n_in);
    for (int i = 0; i < n_in; i++) t.forw_pts[i] = Point2f(a.forw_xy[2 * i], a.forw_xy[2 * i + 1]);
    if (n_in > 0) {
        const std::vector<uint8_t> status(a.status_lk, a.status_lk + n_in);
        reduce_vector(t.prev_pts, status);
        reduce_vector(t.cur_pts, status);
        reduce_vector(t.forw_pts, status);
        reduce_vector(t.ids, status);
        reduce_vector(t.cur_un_pts, status);
        reduce_vector(t.track_cnt, status);
    }
    for (auto& n : t.track_cnt) n++;
    if (a.ransac_ran) {
        const std::vector<uint8_t> status(a.status_f, a.status_f + a.n1);
        reduce_vector(t.prev_pts, status);
        reduce_vector(t.cur_pts, status);
        reduce_vector(t.forw_pts, status);
        reduce_vector(t.cur_un_pts, status);
        reduce_vector(t.ids, status);
        reduce_vector(t.track_cnt, status);
    }
}

// A published frame after apply_statuses: setMask's outcome (:53-68), the kept points in the order of the walk (`sorted`: the list the
// order callback made), then the new corners through addPoints() (:144-156)
template <class T> void apply_published(T& t, const vg_fe_frame_out& out, const typename OrderCtx<T>::SortedList& sorted) {
    typedef typename OrderCtx<T>::Point2f Point2f;
    std::vector<Point2f> kept_pts;
    std::vector<int> kept_ids, kept_cnt;
    for (int k = 0; k < out.n_kept; k++) {
        const auto& it = sorted[out.kept[k]];
        kept_pts.push_back(it.second.first);
        kept_ids.push_back(t.ids[it.second.second]);
        kept_cnt.push_back(it.first);
    }
    t.forw_pts = kept_pts; t.ids = kept_ids; t.track_cnt = kept_cnt;
    t.n_pts.clear();
    for (int k = 0; k < out.n_new; k++) t.n_pts.push_back(Point2f(out.new_xy[2 * k], out.new_xy[2 * k + 1]));
    t.addPoints();
}

// undistortedPoints() (:262-304) given the lifted (x / z, y / z) pairs of cur_pts: cur_un_pts, the map, the velocities
template <class T> void lifted_points(T& t, const float* un) {
    typedef typename OrderCtx<T>::Point2f Point2f;
    t.cur_un_pts.clear();
    t.cur_un_pts_map.clear();
    const int n = (int)t.cur_pts.size();
    for (int i = 0; i < n; i++) {
        t.cur_un_pts.push_back(Point2f(un[2 * i], un[2 * i + 1]));
        t.cur_un_pts_map.insert(std::make_pair(t.ids[i], Point2f(un[2 * i], un[2 * i + 1])));
    }
    if (!t.prev_un_pts_map.empty()) {
        double dt = t.cur_time - t.prev_time;
        t.pts_velocity.clear();
        for (unsigned int i = 0; i < t.cur_un_pts.size(); i++) {
            if (t.ids[i] != -1) {
                auto it = t.prev_un_pts_map.find(t.ids[i]);
                if (it != t.prev_un_pts_map.end()) {
                    double v_x = (t.cur_un_pts[i].x - it->second.x) / dt;
                    double v_y = (t.cur_un_pts[i].y - it->second.y) / dt;
                    t.pts_velocity.push_back(Point2f((float)v_x, (float)v_y));
                } else
                    t.pts_velocity.push_back(Point2f(0, 0));
            } else
                t.pts_velocity.push_back(Point2f(0, 0));
        }
    } else {
        for (unsigned int i = 0; i < t.cur_pts.size(); i++) t.pts_velocity.push_back(Point2f(0, 0));      // (as the reference: not cleared)
    }
    t.prev_un_pts_map = t.cur_un_pts_map;
}

// The arguments of one frame that every caller sets alike: the image, cur_pts and the configuration values (the reference's globals
// PUB_THIS_FRAME, EQUALIZE, MAX_CNT, MIN_DIST, F_THRESHOLD, FOCAL_LENGTH, handed in by the caller whose header declares them).  intr,
// base_mask and the order callback stay with the caller.
template <class T, class Image>
void fill_frame_in(T& t, const Image& img, bool publish, int equalize, int max_cnt, int min_dist, double f_threshold, double focal_length, vg_fe_frame_in& in) {
    std::memset(&in, 0, sizeof(in));
    in.struct_size = (int)sizeof(in);
    in.img = img.data; in.stride = (int)img.step; in.equalize = equalize; in.publish = publish ? 1 : 0;
    in.cur_xy = t.cur_pts.empty() ? nullptr : &t.cur_pts[0].x; in.n = (int)t.cur_pts.size();
    in.max_cnt = max_cnt; in.min_dist = min_dist; in.quality = 0.01; in.f_threshold = f_threshold; in.focal_length = focal_length;
}

// setMask() (:36-69) up to the library call: cnt_pts_id sorted the reference's way (:43-51), packed as vg_fe_set_mask takes it (the
// device's own sort by count is stable, i.e. the identity on an already sorted list)
template <class T>
void sorted_for_setmask(T& t, int capacity, std::vector<float>& xy, std::vector<int>& cnt, typename OrderCtx<T>::SortedList& cnt_pts_id) {
    const int n = (int)t.forw_pts.size();
    if (n > capacity) throw std::runtime_error("FeatureTracker::setMask: more points than the configured capacity");
    for (int i = 0; i < n; i++) cnt_pts_id.push_back(std::make_pair(t.track_cnt[i], std::make_pair(t.forw_pts[i], t.ids[i])));
    sort_by_count(cnt_pts_id);
    xy.assign((size_t)capacity * 2, 0.f);
    cnt.assign((size_t)capacity, 0);
    for (int i = 0; i < n; ++i) { xy[2 * i] = cnt_pts_id[i].second.first.x; xy[2 * i + 1] = cnt_pts_id[i].second.first.y; cnt[i] = cnt_pts_id[i].first; }
}
// ... and after it (:53-68): the points the walk kept, in its order
template <class T> void take_setmask_result(T& t, const typename OrderCtx<T>::SortedList& cnt_pts_id, const int* kept, int nk) {
    t.forw_pts.clear(); t.ids.clear(); t.track_cnt.clear();
    for (int k = 0; k < nk; ++k) {
        const auto& it = cnt_pts_id[kept[k]];
        t.forw_pts.push_back(it.second.first); t.ids.push_back(it.second.second); t.track_cnt.push_back(it.first);
    }
}

// ---- vg_kf_*: the pose graph's KeyFrame (host/keyframe.h, or the reference's own class with a slot beside it)
// one entry of vg_kf_add from a keyframe's image and point_2d_uv
template <class KF>
void pack_kf(const KF& kf, int slot, const vg_fe_camera& camera, vg_kf_in& in) {
    std::memset(&in, 0, sizeof(in));
    in.struct_size = (int)sizeof(in);
    in.slot = slot; in.img = kf.image.data; in.stride = (int)kf.image.step;
    in.n_window = (int)kf.point_2d_uv.size(); in.window_xy = kf.point_2d_uv.empty() ? nullptr : &kf.point_2d_uv[0].x;
    in.camera = camera;
}
// a whole record for vg_kf_set from stored keypoints, keypoints_norm and brief_descriptors (the constructor of loadPoseGraph); the
// vectors of `r` hold what rec points to
struct KfRecord {
    std::vector<float> kp, nm;
    std::vector<uint8_t> sc;
    std::vector<uint64_t> de;
    vg_kf_record rec;
};
template <class KF>
void pack_kf_record(const KF& kf, KfRecord& r) {
    const size_t n = kf.keypoints.size();
    if (kf.keypoints_norm.size() != n || kf.brief_descriptors.size() != n) throw std::runtime_error("pack_kf_record: the three lists differ in length");
    r.kp.assign(2 * n + 2, 0.f); r.nm.assign(2 * n + 2, 0.f); r.sc.assign(n + 1, 0); r.de.assign(4 * n + 4, 0);
    for (size_t i = 0; i < n; ++i) {
        r.kp[2 * i] = kf.keypoints[i].pt.x; r.kp[2 * i + 1] = kf.keypoints[i].pt.y;
        r.nm[2 * i] = kf.keypoints_norm[i].pt.x; r.nm[2 * i + 1] = kf.keypoints_norm[i].pt.y;
        r.sc[i] = (uint8_t)kf.keypoints[i].response;
        for (int q = 0; q < 4; ++q) r.de[4 * i + q] = kf.brief_descriptors[i][q];
    }
    std::memset(&r.rec, 0, sizeof(r.rec));
    r.rec.struct_size = (int)sizeof(r.rec);
    r.rec.n_keypoints = (int)n;
    r.rec.keypoints_xy = r.kp.data(); r.rec.scores = r.sc.data(); r.rec.norm_xy = r.nm.data(); r.rec.descriptors = r.de.data();
}

// one entry of vg_kf_pnp from the lists findConnection holds behind its first reduceVector round (cv::Point3f / cv::Point2f are three / two
// packed floats; the vectors must outlive the call) and the keyframe's origin_vio_T / origin_vio_R, tic, qic; matched_id: ints, the
// reference's vector<double> narrowed by the caller.  Everything else keeps the defaults of vg_kf_pnp_defaults.
template <class KF, class P3, class P2>
void pack_kf_pnp(const KF& kf, const std::vector<P3>& matched_3d, const std::vector<P2>& matched_2d_old_norm, const std::vector<int>& matched_id, vg_kf_pnp_in& in) {
    static_assert(sizeof(P3) == 3 * sizeof(float) && sizeof(P2) == 2 * sizeof(float), "packed float points");
    if (matched_3d.size() != matched_2d_old_norm.size() || (!matched_id.empty() && matched_id.size() != matched_3d.size()))
        throw std::runtime_error("pack_kf_pnp: the lists differ in length");
    vg_kf_pnp_defaults(&in);
    in.n = (int)matched_3d.size();
    in.point_3d = matched_3d.empty() ? nullptr : &matched_3d[0].x;
    in.old_norm = matched_2d_old_norm.empty() ? nullptr : &matched_2d_old_norm[0].x;
    in.point_id = matched_id.empty() ? nullptr : matched_id.data();
    for (int r = 0; r < 3; ++r) {
        in.origin_vio_T[r] = kf.origin_vio_T(r); in.tic[r] = kf.tic(r);
        for (int c = 0; c < 3; ++c) { in.origin_vio_R[3 * r + c] = kf.origin_vio_R(r, c); in.qic[3 * r + c] = kf.qic(r, c); }
    }
}

// the estimator's keyframe message (vg_ba_seq_get_outputs of one window, its kf_* arrays filled, max_points rows each) as the arguments of
// the KeyFrame constructors of host/keyframe.h: point_3d, point_2d_uv, point_2d_norm and point_id per window point (the id as the double the
// reference's class keeps), vio_T_w_i, vio_R_w_i = the matrix of the normalised pose quaternion.  P3 / P2: three / two packed floats
// (cv::Point3f / cv::Point2f).  The stamp and the image are the caller's.  Returns the number of points (min(n_keyframe, max_points)).
template <class P3, class P2, class V3, class M3>
int unpack_keyframe(const vg_ba_seq_outputs& o, int max_points, std::vector<P3>& point_3d, std::vector<P2>& point_2d_uv, std::vector<P2>& point_2d_norm,
                    std::vector<double>& point_id, V3& vio_T_w_i, M3& vio_R_w_i) {
    static_assert(sizeof(P3) == 3 * sizeof(float) && sizeof(P2) == 2 * sizeof(float), "packed float points");
    const int n = std::max(0, std::min(o.n_keyframe, max_points));
    if (n && (!o.kf_point_3d || !o.kf_uv || !o.kf_norm || !o.kf_id)) throw std::runtime_error("unpack_keyframe: the kf_* arrays of vg_ba_seq_outputs are not all there");
    point_3d.resize(n); point_2d_uv.resize(n); point_2d_norm.resize(n); point_id.resize(n);
    if (n) {
        std::memcpy(&point_3d[0], o.kf_point_3d, sizeof(P3) * n);
        std::memcpy(&point_2d_uv[0], o.kf_uv, sizeof(P2) * n);
        std::memcpy(&point_2d_norm[0], o.kf_norm, sizeof(P2) * n);
    }
    for (int k = 0; k < n; ++k) point_id[k] = (double)o.kf_id[k];
    const double* p = o.pose;
    const double qn = std::sqrt(p[3] * p[3] + p[4] * p[4] + p[5] * p[5] + p[6] * p[6]);
    const double x = p[3] / qn, y = p[4] / qn, z = p[5] / qn, w = p[6] / qn;
    const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                         2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)};
    for (int r = 0; r < 3; ++r) {
        vio_T_w_i(r) = p[r];
        for (int c = 0; c < 3; ++c) vio_R_w_i(r, c) = R[3 * r + c];
    }
    return n;
}

// one request of vg_kf_loop_detect for a keyframe whose record is resident (kf.slot): flags VG_BOW_QUERY | VG_BOW_ADD is detectLoop,
// VG_BOW_ADD alone addKeyFrameIntoVoc.  `out` is zeroed and gets its struct_size; the caller adds tap arrays if it wants them.
template <class KF>
void pack_bow(const KF& kf, int db, int frame_index, int flags, vg_bow_in& in, vg_bow_out& out) {
    std::memset(&in, 0, sizeof(in));
    std::memset(&out, 0, sizeof(out));
    in.struct_size = (int)sizeof(in); out.struct_size = (int)sizeof(out);
    in.db = db; in.slot = kf.slot; in.frame_index = frame_index; in.flags = flags;
}

// one graph of vg_pg_optimize: the slice of keyframelist (a list of pointers to keyframes with index, sequence, has_loop, loop_index,
// loop_info, vio_T_w_i, vio_R_w_i) that optimize4DoF walks -- index >= first_looped_index through the END of the list; the keyframes up
// to and including cur_index are the optimised ones.  Sets local_index as the reference does.  The tables live in `p`.
struct PgIn {
    vg_pg_in in;
    std::vector<int> index, sequence, has_loop, loop_index;
    std::vector<double> T, R, info;
};
template <class List>
void pack_pg(List& keyframelist, int first_looped_index, int cur_index, PgIn& p) {
    p.index.clear(); p.sequence.clear(); p.has_loop.clear(); p.loop_index.clear(); p.T.clear(); p.R.clear(); p.info.clear();
    int n_opt = 0;
    bool past = false;                  // behind cur_index: the keyframes that only receive the drift
    for (auto it = keyframelist.begin(); it != keyframelist.end(); ++it) {
        auto& kf = **it;
        if (kf.index < first_looped_index) continue;
        if (!past) { kf.local_index = n_opt++; past = kf.index == cur_index; }
        p.index.push_back(kf.index); p.sequence.push_back(kf.sequence); p.has_loop.push_back(kf.has_loop ? 1 : 0); p.loop_index.push_back(kf.loop_index);
        for (int r = 0; r < 3; ++r) p.T.push_back(kf.vio_T_w_i(r));
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) p.R.push_back(kf.vio_R_w_i(r, c));
        for (int k = 0; k < 8; ++k) p.info.push_back(kf.has_loop ? kf.loop_info(k, 0) : 0.0);
    }
    if (!past) throw std::runtime_error("pack_pg: cur_index is not in the slice");
    vg_pg_defaults(&p.in);
    p.in.n_kf = (int)p.index.size(); p.in.n_opt = n_opt; p.in.first_looped_index = first_looped_index;
    p.in.index = p.index.data(); p.in.sequence = p.sequence.data(); p.in.has_loop = p.has_loop.data(); p.in.loop_index = p.loop_index.data();
    p.in.vio_T = p.T.data(); p.in.vio_R = p.R.data(); p.in.loop_info = p.info.data();
}

}  // namespace vg_pack

// (the packer of vg_pg_optimize under the name the integration guide uses)
template <class List>
void vg_pack_pg(List& keyframelist, int first_looped_index, int cur_index, vg_pack::PgIn& p) {
    vg_pack::pack_pg(keyframelist, first_looped_index, cur_index, p);
}
// (the packer of vg_kf_loop_detect under the name the integration guide uses)
template <class KF>
void vg_pack_bow(const KF& kf, int db, int frame_index, int flags, vg_bow_in& in, vg_bow_out& out) {
    vg_pack::pack_bow(kf, db, frame_index, flags, in, out);
}
// (the packer of vg_kf_pnp under the name the integration guide uses)
template <class KF, class P3, class P2>
void vg_pack_kf_pnp(const KF& kf, const std::vector<P3>& matched_3d, const std::vector<P2>& matched_2d_old_norm, const std::vector<int>& matched_id, vg_kf_pnp_in& in) {
    vg_pack::pack_kf_pnp(kf, matched_3d, matched_2d_old_norm, matched_id, in);
}
// (the unpacker of vg_ba_seq_get_outputs' keyframe message under the name the integration guide uses)
template <class P3, class P2, class V3, class M3>
int vg_unpack_keyframe(const vg_ba_seq_outputs& o, int max_points, std::vector<P3>& point_3d, std::vector<P2>& point_2d_uv, std::vector<P2>& point_2d_norm,
                       std::vector<double>& point_id, V3& vio_T_w_i, M3& vio_R_w_i) {
    return vg_pack::unpack_keyframe(o, max_points, point_3d, point_2d_uv, point_2d_norm, point_id, vio_T_w_i, vio_R_w_i);
}
// (the packer of vg_kf_add under the name the integration guide uses)
template <class KF>
void vg_pack_kf(const KF& kf, int slot, const vg_fe_camera& camera, vg_kf_in& in) {
    vg_pack::pack_kf(kf, slot, camera, in);
}
// (the packer of vg_init_sfm under the name the integration guide uses)
template <class Features, class Map, class M3, class V3>
void vg_pack_sfm(const Features& features, const Map& frames, const double* stamps, int n_stamps, int l, const M3& relative_R, const V3& relative_T,
                 const M3& ric, vg_pack::SfmIn& p) {
    vg_pack::pack_sfm(features, frames, stamps, n_stamps, l, relative_R, relative_T, ric, p);
}
// (the packer of vg_init_relpose under the name the integration guide uses)
template <class Features>
void vg_pack_relpose(const Features& features, int n_frames, vg_pack::RelposeIn& p) {
    vg_pack::pack_relpose(features, n_frames, p);
}
// (the packer of vg_init_exrot under the name the integration guide uses)
template <class Corres, class Q, class M3>
void vg_pack_exrot(const Corres& corres, const Q& delta_q, const std::vector<double>& records, const M3& ric, vg_pack::ExrotIn& p) {
    vg_pack::pack_exrot(corres, delta_q, records, ric, p);
}
// (the packer of vg_init_align under the name the integration guide uses)
template <class Map, class V3>
void vg_pack_align(const Map& frames, const double* stamps, int n_stamps, const V3& ba0, const V3& bg0, const double* noise, const V3& tic, double g_norm, vg_pack::AlignIn& p) {
    vg_pack::pack_align(frames, stamps, n_stamps, ba0, bg0, noise, tic, g_norm, p);
}
