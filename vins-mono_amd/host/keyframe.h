// keyframe.h — the pose graph's KeyFrame (pose_graph/src/keyframe.h, keyframe.cpp) with its findConnection, on the device through
// vg_kf_* (include/vinsgpu.h): computeWindowBRIEFPoint, computeBRIEFPoint with keypoints_norm, searchByBRIEFDes and the reduceVector step
// behind it (vg_kf_add, vg_kf_match), PnPRANSAC, the second reduceVector round and the loop_info arithmetic with its gate (vg_kf_pnp).
// Stand-alone and header-only; the reference's member names.  A KeyFrame owns one SLOT of the handle's resident records
// (KeyFrame::configure allocates them once); its descriptors stay on the device, the members below are the host copies the reference's
// callers read.  Where the reference publishes a ROS message (pub_match_points) the class fills the plain struct match_points.
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>
#include "../../include/vinsgpu.h"
#include "compat/cv_compat.h"
#include "compat/eigen_compat.h"
#include "vg_pack.h"
#include "yaml_config.h"

// BriefExtractor(pattern_file): the four lists x1 y1 x2 y2 of an OpenCV-FileStorage yml (support_files/brief_pattern.yml).  It only
// reads the pattern: the descriptors are computed by the library, which gets the pattern through vg_kf_configure.
class BriefExtractor {
  public:
    int16_t pattern[4][256];
    explicit BriefExtractor(const std::string& pattern_file) {
        VinsYaml y;
        if (!y.load(pattern_file)) throw std::runtime_error("Could not open file " + pattern_file);
        const char* keys[4] = {"x1", "y1", "x2", "y2"};
        for (int k = 0; k < 4; ++k) {
            const std::vector<double>* v = y.sequence(keys[k]);
            if (!v || v->size() != 256) throw std::runtime_error(pattern_file + ": " + keys[k] + " is not a list of 256 numbers");
            for (int i = 0; i < 256; ++i) pattern[k][i] = (int16_t)(*v)[i];
        }
    }
};

namespace BRIEF { typedef std::array<uint64_t, 4> bitset; }      // bit i of a descriptor: word i / 64, position i % 64

class KeyFrame {
  public:
    static const int MIN_LOOP_NUM = 25;
    // once per handle, before the first KeyFrame
    static void configure(vg_handle* h, const BriefExtractor& extractor, int width, int height, int max_keypoints, int max_window_points, int n_slots) {
        if (vg_kf_configure(h, width, height, max_keypoints, max_window_points, n_slots, &extractor.pattern[0][0]) != VG_OK)
            throw std::runtime_error(vg_last_error(h));
        capacity(h, max_keypoints, max_window_points, true);
    }

    KeyFrame(vg_handle* h_, int slot_, double _time_stamp, int _index, const cv::Mat& _image, const std::vector<cv::Point2f>& _point_2d_uv,
             const vg_fe_camera& _camera)
        : time_stamp(_time_stamp), index(_index), image(_image), point_2d_uv(_point_2d_uv), camera(_camera), slot(slot_), h(h_) {
        computeWindowBRIEFPoint();
        computeBRIEFPoint();
    }
    // the reference's second constructor (loadPoseGraph): stored keypoints and descriptors go up as they are
    KeyFrame(vg_handle* h_, int slot_, double _time_stamp, int _index, const std::vector<cv::KeyPoint>& _keypoints, const std::vector<cv::KeyPoint>& _keypoints_norm,
             const std::vector<BRIEF::bitset>& _brief_descriptors)
        : time_stamp(_time_stamp), index(_index), keypoints(_keypoints), keypoints_norm(_keypoints_norm), brief_descriptors(_brief_descriptors), slot(slot_), h(h_) {
        vg_pack::KfRecord r;
        vg_pack::pack_kf_record(*this, r);
        if (vg_kf_set(h, slot, &r.rec) != VG_OK) throw std::runtime_error(vg_last_error(h));
        n_true = (int)keypoints.size();
        added = true;
    }

    // a keyframe that only verifies: the members PnPRANSAC and findConnection's second half read, no record on the device
    KeyFrame(vg_handle* h_, double _time_stamp, int _index, const Eigen::Vector3d& _vio_T_w_i, const Eigen::Matrix3d& _vio_R_w_i,
             const std::vector<cv::Point3f>& _point_3d, const std::vector<double>& _point_id)
        : time_stamp(_time_stamp), index(_index), point_3d(_point_3d), point_id(_point_id), vio_T_w_i(_vio_T_w_i), vio_R_w_i(_vio_R_w_i), T_w_i(_vio_T_w_i),
          R_w_i(_vio_R_w_i), origin_vio_T(_vio_T_w_i), origin_vio_R(_vio_R_w_i), slot(-1), h(h_) { added = true; }

    // KeyFrame::PnPRANSAC (keyframe.cpp:200-256) with the reference's signature: status is appended to, as there.  One vg_kf_pnp; the
    // call's loop gate is set below the list's length so that the member always runs (findConnection tests MIN_LOOP_NUM before it)
    void PnPRANSAC(const std::vector<cv::Point2f>& matched_2d_old_norm, const std::vector<cv::Point3f>& matched_3d, std::vector<uchar>& status,
                   Eigen::Vector3d& PnP_T_old, Eigen::Matrix3d& PnP_R_old) {
        pnp(matched_2d_old_norm, matched_3d, std::vector<int>(), std::min((int)MIN_LOOP_NUM, (int)matched_3d.size() - 1));
        for (size_t i = 0; i < matched_3d.size(); ++i) status.push_back(p_mask[i]);
        for (int r = 0; r < 3; ++r) { PnP_T_old(r) = pout.PnP_T_old[r]; for (int c = 0; c < 3; ++c) PnP_R_old(r, c) = pout.PnP_R_old[3 * r + c]; }
    }
    // findConnection (keyframe.cpp:259-520) as the reference declares it: the match, the first reduceVector round, PnPRANSAC with the
    // second, loop_info and the gate; sets has_loop, loop_index, loop_info and match_points.  point_3d / point_id are per window point.
    bool findConnection(KeyFrame* old_kf) {
        std::vector<cv::Point2f> matched_2d_cur, matched_2d_old, matched_2d_old_norm;
        std::vector<int> matched_index;
        std::vector<cv::Point3f> matched_3d;
        std::vector<double> matched_id;
        if (point_3d.size() != point_2d_uv.size() || point_id.size() != point_2d_uv.size()) throw std::runtime_error("KeyFrame::findConnection: point_3d / point_id per window point");
        findConnection(*old_kf, matched_2d_cur, matched_2d_old, matched_2d_old_norm, matched_index);
        for (int i : matched_index) { matched_3d.push_back(point_3d[i]); matched_id.push_back(point_id[i]); }
        return findConnection(old_kf, matched_2d_old_norm, matched_3d, matched_id);
    }
    // its second half (:401-520) from the lists the first reduceVector round left; the lists are reduced in place as there
    bool findConnection(KeyFrame* old_kf, std::vector<cv::Point2f>& matched_2d_old_norm, std::vector<cv::Point3f>& matched_3d, std::vector<double>& matched_id) {
        pnp_status = VG_KF_PNP_SKIPPED;
        if ((int)matched_3d.size() <= MIN_LOOP_NUM) return false;
        std::vector<int> ids;
        for (double v : matched_id) ids.push_back((int)v);
        pnp(matched_2d_old_norm, matched_3d, ids, MIN_LOOP_NUM);
        std::vector<cv::Point2f> n2;
        std::vector<cv::Point3f> n3;
        std::vector<double> nid;
        for (int k = 0; k < pout.n_inliers; ++k) { n2.push_back(matched_2d_old_norm[p_index[k]]); n3.push_back(matched_3d[p_index[k]]); nid.push_back(matched_id[p_index[k]]); }
        matched_2d_old_norm.swap(n2); matched_3d.swap(n3); matched_id.swap(nid);
        if (!pout.has_loop) return false;
        has_loop = true;
        loop_index = old_kf->index;
        for (int k = 0; k < 8; ++k) loop_info(k, 0) = pout.loop_info[k];
        // FAST_RELOCALIZATION: what pub_match_points carries, ready for vg_ba_relo_frame (match_id / match_xy)
        match_points.stamp = time_stamp;
        match_points.match_id.assign(p_id.begin(), p_id.begin() + pout.n_inliers);
        match_points.match_xy.assign(p_xy.begin(), p_xy.begin() + 2 * (size_t)pout.n_inliers);
        const Eigen::Quaterniond Q(old_kf->R_w_i);
        const double tq[8] = {old_kf->T_w_i.x(), old_kf->T_w_i.y(), old_kf->T_w_i.z(), Q.w(), Q.x(), Q.y(), Q.z(), (double)index};
        for (int k = 0; k < 8; ++k) match_points.t_q_index[k] = tq[k];
        return true;
    }

    void computeWindowBRIEFPoint() {
        add();
        window_keypoints.clear();
        for (const cv::Point2f& p : point_2d_uv) { cv::KeyPoint key; key.pt = p; window_keypoints.push_back(key); }
    }
    void computeBRIEFPoint() { add(); }

    // searchByBRIEFDes(matched_2d_old, matched_2d_old_norm, status, old_kf's descriptors / keypoints / keypoints_norm): the old record is
    // resident, so the old KeyFrame stands for its three lists
    void searchByBRIEFDes(std::vector<cv::Point2f>& matched_2d_old, std::vector<cv::Point2f>& matched_2d_old_norm, std::vector<uchar>& status, const KeyFrame& old_kf) {
        match(old_kf);
        const size_t n = (size_t)mout.n_window;
        for (size_t i = 0; i < n; ++i) {
            status.push_back(m_status[i]);
            matched_2d_old.push_back(cv::Point2f(m_old[2 * i], m_old[2 * i + 1]));
            matched_2d_old_norm.push_back(cv::Point2f(m_old_norm[2 * i], m_old_norm[2 * i + 1]));
        }
    }
    // findConnection up to the MIN_LOOP_NUM test (keyframe.cpp:262-312 ... :356): the lists after reduceVector, in window order;
    // matched_index gathers what the caller owns (point_3d, point_id, point_2d_norm).  Returns (int)matched_2d_cur.size() > MIN_LOOP_NUM.
    bool findConnection(const KeyFrame& old_kf, std::vector<cv::Point2f>& matched_2d_cur, std::vector<cv::Point2f>& matched_2d_old,
                        std::vector<cv::Point2f>& matched_2d_old_norm, std::vector<int>& matched_index) {
        match(old_kf);
        matched_2d_cur.clear(); matched_2d_old.clear(); matched_2d_old_norm.clear(); matched_index.clear();
        for (int k = 0; k < mout.n_matched; ++k) {
            matched_index.push_back(m_index[k]);
            matched_2d_cur.push_back(point_2d_uv[m_index[k]]);
            matched_2d_old.push_back(cv::Point2f(c_old[2 * k], c_old[2 * k + 1]));
            matched_2d_old_norm.push_back(cv::Point2f(c_old_norm[2 * k], c_old_norm[2 * k + 1]));
        }
        return (int)matched_2d_cur.size() > MIN_LOOP_NUM;
    }

    // the pose members PoseGraph::addKeyFrame and optimize4DoF go through (keyframe.cpp:522-575)
    void getVioPose(Eigen::Vector3d& _T_w_i, Eigen::Matrix3d& _R_w_i) const { _T_w_i = vio_T_w_i; _R_w_i = vio_R_w_i; }
    void getPose(Eigen::Vector3d& _T_w_i, Eigen::Matrix3d& _R_w_i) const { _T_w_i = T_w_i; _R_w_i = R_w_i; }
    void updatePose(const Eigen::Vector3d& _T_w_i, const Eigen::Matrix3d& _R_w_i) { T_w_i = _T_w_i; R_w_i = _R_w_i; }
    void updateVioPose(const Eigen::Vector3d& _T_w_i, const Eigen::Matrix3d& _R_w_i) { vio_T_w_i = _T_w_i; vio_R_w_i = _R_w_i; T_w_i = vio_T_w_i; R_w_i = vio_R_w_i; }
    Eigen::Vector3d getLoopRelativeT() const { return Eigen::Vector3d(loop_info(0, 0), loop_info(1, 0), loop_info(2, 0)); }
    Eigen::Quaterniond getLoopRelativeQ() const { return Eigen::Quaterniond(loop_info(3, 0), loop_info(4, 0), loop_info(5, 0), loop_info(6, 0)); }
    double getLoopRelativeYaw() const { return loop_info(7, 0); }

    double time_stamp;
    int index;
    int local_index = 0;                // optimize4DoF's position in its slice
    int sequence = 1;
    cv::Mat image;
    std::vector<cv::Point2f> point_2d_uv;
    std::vector<cv::KeyPoint> keypoints, keypoints_norm, window_keypoints;
    std::vector<BRIEF::bitset> brief_descriptors, window_brief_descriptors;
    vg_fe_camera camera = {};
    int slot;
    std::vector<cv::Point3f> point_3d;  // per window point, like point_2d_uv (from a resident sequence: vg_unpack_keyframe, host/vg_pack.h)
    std::vector<double> point_id;
    Eigen::Vector3d vio_T_w_i, T_w_i, origin_vio_T, tic;
    Eigen::Matrix3d vio_R_w_i, R_w_i, origin_vio_R, qic;          // (tic / qic: the reference's globals, per keyframe here)
    bool has_loop = false;
    int loop_index = -1;
    Eigen::Matrix<double, 8, 1> loop_info;
    struct MatchPoints {                // sensor_msgs::PointCloud of pub_match_points as plain data
        double stamp = 0.0;
        std::vector<int> match_id;      // points[k].z
        std::vector<double> match_xy;   // points[k].x, .y
        double t_q_index[8] = {0, 0, 0, 1, 0, 0, 0, 0};      // the old keyframe's T_w_i, Q (w x y z), this keyframe's index
    } match_points;
    int pnp_refine = 0;                 // vg_kf_pnp_in::refine
    int pnp_status = VG_KF_PNP_SKIPPED; // VG_KF_PNP_* of the last PnPRANSAC
    vg_kf_pnp_out pout = {};            // the last vg_kf_pnp (taps included); its pointers are the class's own
    int n_true = 0;                     // corners cv::FAST lists; above max_keypoints the record keeps the first max_keypoints (kf_status)
    int kf_status = VG_KF_OK;
    std::vector<int> best_idx, best_dist;      // of the last match, per window point

  private:
    vg_handle* h;
    bool added = false;
    vg_kf_match_out mout = {};
    std::vector<uchar> m_status;
    std::vector<float> m_old, m_old_norm, c_old, c_old_norm;
    std::vector<int> m_index;

    std::vector<uchar> p_mask;
    std::vector<int> p_index, p_id;
    std::vector<double> p_xy;
    void pnp(const std::vector<cv::Point2f>& norm, const std::vector<cv::Point3f>& p3, const std::vector<int>& ids, int min_loop_num) {
        vg_kf_pnp_in in;
        vg_pack_kf_pnp(*this, p3, norm, ids, in);
        in.min_loop_num = min_loop_num; in.refine = pnp_refine;
        const size_t n = p3.size();
        p_mask.assign(n + 1, 0); p_index.assign(n + 1, 0); p_id.assign(n + 1, 0); p_xy.assign(2 * n + 2, 0.0);
        std::memset(&pout, 0, sizeof(pout));
        pout.struct_size = sizeof(pout); pout.mask = p_mask.data(); pout.matched_index = p_index.data(); pout.match_id = p_id.data(); pout.match_xy = p_xy.data();
        if (vg_kf_pnp(h, 1, &in, &pout) != VG_OK) throw std::runtime_error(vg_last_error(h));
        pnp_status = pout.status;
    }
    // (max_keypoints, max_window_points) of the handle's configuration
    static std::pair<int, int> capacity(vg_handle* h, int mk = 0, int mw = 0, bool set = false) {
        static std::vector<std::pair<vg_handle*, std::pair<int, int>>> table;
        for (auto& e : table)
            if (e.first == h) { if (set) e.second = {mk, mw}; return e.second; }
        if (!set) throw std::runtime_error("KeyFrame: KeyFrame::configure was not called for this handle");
        table.push_back({h, {mk, mw}});
        return {mk, mw};
    }
    // the one vg_kf_add that fills both descriptor sets
    void add() {
        if (added) return;
        const std::pair<int, int> cap = capacity(h);
        vg_kf_in in;
        vg_pack_kf(*this, slot, camera, in);
        std::vector<float> kp(2 * (size_t)cap.first), nm(2 * (size_t)cap.first);
        std::vector<uint8_t> sc((size_t)cap.first);
        std::vector<uint64_t> de(4 * (size_t)cap.first), wde(4 * (size_t)cap.second);
        vg_kf_out out;
        std::memset(&out, 0, sizeof(out));
        out.struct_size = (int)sizeof(out); out.keypoints_xy = kp.data(); out.scores = sc.data(); out.norm_xy = nm.data(); out.descriptors = de.data();
        out.window_descriptors = wde.data();
        if (vg_kf_add(h, 1, &in, &out) != VG_OK) throw std::runtime_error(vg_last_error(h));
        n_true = out.n_keypoints; kf_status = out.status;
        keypoints.clear(); keypoints_norm.clear(); brief_descriptors.clear(); window_brief_descriptors.clear();
        for (int i = 0; i < out.n_kept; ++i) {
            cv::KeyPoint k, n;
            k.pt = cv::Point2f(kp[2 * i], kp[2 * i + 1]); k.response = (float)sc[i];
            n.pt = cv::Point2f(nm[2 * i], nm[2 * i + 1]);
            keypoints.push_back(k); keypoints_norm.push_back(n);
            brief_descriptors.push_back(BRIEF::bitset{de[4 * i], de[4 * i + 1], de[4 * i + 2], de[4 * i + 3]});
        }
        for (size_t i = 0; i < point_2d_uv.size(); ++i) window_brief_descriptors.push_back(BRIEF::bitset{wde[4 * i], wde[4 * i + 1], wde[4 * i + 2], wde[4 * i + 3]});
        added = true;
    }
    void match(const KeyFrame& old_kf) {
        const int mw = capacity(h).second;
        best_idx.assign(mw, 0); best_dist.assign(mw, 0); m_status.assign(mw, 0); m_index.assign(mw, 0);
        m_old.assign(2 * (size_t)mw, 0.f); m_old_norm.assign(2 * (size_t)mw, 0.f); c_old.assign(2 * (size_t)mw, 0.f); c_old_norm.assign(2 * (size_t)mw, 0.f);
        vg_kf_pair pr;
        pr.struct_size = (int)sizeof(pr); pr.cur_slot = slot; pr.old_slot = old_kf.slot;
        std::memset(&mout, 0, sizeof(mout));
        mout.struct_size = (int)sizeof(mout); mout.best_idx = best_idx.data(); mout.best_dist = best_dist.data(); mout.status = m_status.data();
        mout.matched_2d_old = m_old.data(); mout.matched_2d_old_norm = m_old_norm.data(); mout.matched_index = m_index.data();
        mout.matched_old_xy = c_old.data(); mout.matched_old_norm = c_old_norm.data();
        if (vg_kf_match(h, 1, &pr, &mout) != VG_OK) throw std::runtime_error(vg_last_error(h));
        best_idx.resize(mout.n_window); best_dist.resize(mout.n_window);
    }
};
