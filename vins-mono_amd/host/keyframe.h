// keyframe.h — the pose graph's KeyFrame (pose_graph/src/keyframe.h, keyframe.cpp) up to the MIN_LOOP_NUM test of findConnection, on the
// device through vg_kf_* (include/vinsgpu.h): computeWindowBRIEFPoint, computeBRIEFPoint with keypoints_norm, searchByBRIEFDes and the
// reduceVector step behind it.  Stand-alone and header-only; the reference's member names.  A KeyFrame owns one SLOT of the handle's
// resident records (KeyFrame::configure allocates them once); its descriptors stay on the device, the members below are the host copies
// the reference's callers read.  What follows in the reference's findConnection -- PnPRANSAC and the loop_info arithmetic -- stays with
// the caller, who gets the compacted lists.
#pragma once
#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>
#include "../../include/vinsgpu.h"
#include "compat/cv_compat.h"
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

    double time_stamp;
    int index;
    cv::Mat image;
    std::vector<cv::Point2f> point_2d_uv;
    std::vector<cv::KeyPoint> keypoints, keypoints_norm, window_keypoints;
    std::vector<BRIEF::bitset> brief_descriptors, window_brief_descriptors;
    vg_fe_camera camera = {};
    int slot;
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
