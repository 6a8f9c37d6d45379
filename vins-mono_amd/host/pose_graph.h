// pose_graph.h — the loop detection of the pose graph's PoseGraph (pose_graph/src/pose_graph.h, pose_graph.cpp:304-410) on the device
// through vg_voc_load / vg_bow_* / vg_kf_loop_detect (include/vinsgpu.h): loadVocabulary, detectLoop and addKeyFrameIntoVoc with the
// reference's signatures, over the resident record of a KeyFrame (host/keyframe.h).  Stand-alone and header-only.  A PoseGraph owns one
// DATABASE of the handle (PoseGraph::configure allocates them once, after the vocabulary is loaded).  addKeyFrame keeps the reference's pose
// bookkeeping (:44-62, :82-136, without the ROS messages) and keyframelist; optimize4DoF is ONE pass of the reference's loop body (:407-573)
// through vg_pg_optimize: drain optimize_buf, solve, write the poses back, set the drift.  The thread around it and its 2 s sleep stay the
// caller's, and so do the locks: the class is not thread-safe.  The thumbnails, the debug images, map save / load and the ROS publishing
// are not here.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <list>
#include <queue>
#include <stdexcept>
#include <string>
#include <vector>
#include "../../include/vinsgpu.h"
#include "keyframe.h"
#include "vg_pack.h"

// BriefVocabulary(path): the reference's binary vocabulary (VocabularyBinary.hpp): 6 x int32 k, L, scoringType, weightingType, nNodes,
// nWords, then the node records, then the word records.  It only reads the file: the tree is built by the library (vg_voc_load).
class BriefVocabulary {
  public:
    int32_t k = 0, L = 0, scoring = 0, weighting = 0;
    std::vector<vg_voc_node> nodes;
    std::vector<vg_voc_word> words;
    explicit BriefVocabulary(const std::string& path) {
        FILE* f = fopen(path.c_str(), "rb");
        if (!f) throw std::runtime_error("Could not open file " + path);
        int32_t hdr[6];
        bool ok = fread(hdr, sizeof(int32_t), 6, f) == 6 && hdr[4] >= 0 && hdr[5] >= 0;
        if (ok) {
            k = hdr[0]; L = hdr[1]; scoring = hdr[2]; weighting = hdr[3];
            nodes.resize((size_t)hdr[4]); words.resize((size_t)hdr[5]);
            ok = fread(nodes.data(), sizeof(vg_voc_node), nodes.size(), f) == nodes.size() && fread(words.data(), sizeof(vg_voc_word), words.size(), f) == words.size();
        }
        fclose(f);
        if (!ok) throw std::runtime_error(path + ": not a binary vocabulary (truncated)");
    }
};
static_assert(sizeof(vg_voc_node) == 48 && sizeof(vg_voc_word) == 8, "the file's record layout");

class PoseGraph {
  public:
    // once per handle, after loadVocabulary: n_db pose graphs of at most max_entries keyframes, pool_words (word, value) pairs each
    static void configure(vg_handle* h, int n_db, int max_entries, int pool_words) {
        if (vg_bow_configure(h, n_db, max_entries, pool_words) != VG_OK) throw std::runtime_error(vg_last_error(h));
    }
    PoseGraph(vg_handle* h_, int db_) : t_drift(0, 0, 0), w_t_vio(0, 0, 0), r_drift(yawRotation(0.0)), w_r_vio(yawRotation(0.0)), h(h_), db(db_) {}
    // (the vocabulary is the handle's: one load serves every PoseGraph on it, and empties their databases)
    void loadVocabulary(const std::string& voc_path) {
        const BriefVocabulary voc(voc_path);
        if (vg_voc_load(h, voc.k, voc.L, voc.scoring, voc.weighting, (int)voc.nodes.size(), voc.nodes.data(), (int)voc.words.size(), voc.words.data()) != VG_OK)
            throw std::runtime_error(vg_last_error(h));
    }
    // detectLoop (pose_graph.cpp:304-386): query, then add; the index of the loop candidate or -1.  `last` holds the whole answer.
    int detectLoop(KeyFrame* keyframe, int frame_index) {
        run(keyframe, frame_index, VG_BOW_QUERY | VG_BOW_ADD);
        return last.loop_index;
    }
    // addKeyFrameIntoVoc (pose_graph.cpp:388-410)
    void addKeyFrameIntoVoc(KeyFrame* keyframe) { run(keyframe, keyframe->index, VG_BOW_ADD); }
    vg_bow_out last = {};

    // addKeyFrame (pose_graph.cpp:42-136 and the push_back of :196): the three parts below in the reference's order around detectLoop /
    // findConnection.  A caller that has its loops from elsewhere (a stored pose graph, the replay tool) calls the parts itself.
    void addKeyFrame(KeyFrame* cur_kf, bool flag_detect_loop) {
        shiftToBase(cur_kf);
        int loop_index = -1;
        if (flag_detect_loop) loop_index = detectLoop(cur_kf, cur_kf->index);
        else addKeyFrameIntoVoc(cur_kf);
        if (loop_index != -1) {
            KeyFrame* old_kf = getKeyFrame(loop_index);
            if (old_kf && cur_kf->findConnection(old_kf)) addLoop(cur_kf, old_kf);
        }
        appendKeyFrame(cur_kf);
    }
    // :44-64: a new sequence resets the shift and the drift; the VIO pose goes to the base frame; the keyframe gets its global index
    void shiftToBase(KeyFrame* cur_kf) {
        if (sequence_cnt != cur_kf->sequence) {
            sequence_cnt++;
            sequence_loop.push_back(0);
            w_t_vio = Eigen::Vector3d(0, 0, 0); w_r_vio = yawRotation(0.0);
            t_drift = Eigen::Vector3d(0, 0, 0); r_drift = yawRotation(0.0);
        }
        Eigen::Vector3d vio_P_cur;
        Eigen::Matrix3d vio_R_cur;
        cur_kf->getVioPose(vio_P_cur, vio_R_cur);
        vio_P_cur = w_r_vio * vio_P_cur + w_t_vio;
        vio_R_cur = w_r_vio * vio_R_cur;
        cur_kf->updateVioPose(vio_P_cur, vio_R_cur);
        cur_kf->index = global_index;
        global_index++;
    }
    // :82-128 behind a successful findConnection (cur_kf carries has_loop, loop_index, loop_info)
    void addLoop(KeyFrame* cur_kf, KeyFrame* old_kf) {
        const int loop_index = old_kf->index;
        if (earliest_loop_index > loop_index || earliest_loop_index == -1) earliest_loop_index = loop_index;
        Eigen::Vector3d w_P_old, w_P_cur, vio_P_cur;
        Eigen::Matrix3d w_R_old, w_R_cur, vio_R_cur;
        old_kf->getVioPose(w_P_old, w_R_old);
        cur_kf->getVioPose(vio_P_cur, vio_R_cur);
        const Eigen::Vector3d relative_t = cur_kf->getLoopRelativeT();
        const Eigen::Matrix3d relative_q = cur_kf->getLoopRelativeQ().toRotationMatrix();
        w_P_cur = w_R_old * relative_t + w_P_old;
        w_R_cur = w_R_old * relative_q;
        const double shift_yaw = yawOf(w_R_cur) - yawOf(vio_R_cur);
        const Eigen::Matrix3d shift_r = yawRotation(shift_yaw);
        const Eigen::Vector3d shift_t = w_P_cur - w_R_cur * vio_R_cur.transpose() * vio_P_cur;
        if (old_kf->sequence != cur_kf->sequence && sequence_loop[cur_kf->sequence] == 0) {      // shift the whole sequence to the world frame
            w_r_vio = shift_r; w_t_vio = shift_t;
            vio_P_cur = w_r_vio * vio_P_cur + w_t_vio;
            vio_R_cur = w_r_vio * vio_R_cur;
            cur_kf->updateVioPose(vio_P_cur, vio_R_cur);
            for (KeyFrame* kf : keyframelist)
                if (kf->sequence == cur_kf->sequence) {
                    Eigen::Vector3d P;
                    Eigen::Matrix3d R;
                    kf->getVioPose(P, R);
                    P = w_r_vio * P + w_t_vio;
                    R = w_r_vio * R;
                    kf->updateVioPose(P, R);
                }
            sequence_loop[cur_kf->sequence] = 1;
        }
        optimize_buf.push(cur_kf->index);
    }
    // :130-136, :196: the drift-corrected pose, then the list
    void appendKeyFrame(KeyFrame* cur_kf) {
        Eigen::Vector3d P;
        Eigen::Matrix3d R;
        cur_kf->getVioPose(P, R);
        P = r_drift * P + t_drift;
        R = r_drift * R;
        cur_kf->updatePose(P, R);
        keyframelist.push_back(cur_kf);
    }
    KeyFrame* getKeyFrame(int index) {
        for (KeyFrame* kf : keyframelist)
            if (kf->index == index) return kf;
        return nullptr;
    }
    // ONE pass of optimize4DoF's loop body (:407-573); false: optimize_buf was empty.  `pg` holds the whole answer of the last pass.
    bool optimize4DoF() {
        int cur_index = -1, first_looped_index = -1;
        while (!optimize_buf.empty()) {
            cur_index = optimize_buf.front();
            first_looped_index = earliest_loop_index;
            optimize_buf.pop();
        }
        if (cur_index == -1) return false;
        vg_pack::PgIn p;
        vg_pack_pg(keyframelist, first_looped_index, cur_index, p);
        std::vector<double> T(3 * (size_t)p.in.n_kf), R(9 * (size_t)p.in.n_kf);
        pg = vg_pg_out();
        pg.struct_size = sizeof(pg); pg.T = T.data(); pg.R = R.data();
        if (vg_pg_optimize(h, 1, &p.in, &pg) != VG_OK) throw std::runtime_error(vg_last_error(h));
        pg.T = nullptr; pg.R = nullptr;
        if (pg.status == VG_PG_NUMERIC) return true;            // (nothing is written back: the poses and the drift stay)
        size_t k = 0;
        for (KeyFrame* kf : keyframelist) {
            if (kf->index < first_looped_index) continue;
            Eigen::Vector3d t(T[3 * k], T[3 * k + 1], T[3 * k + 2]);
            Eigen::Matrix3d r;
            for (int e = 0; e < 9; ++e) r(e / 3, e % 3) = R[9 * k + e];
            kf->updatePose(t, r);
            ++k;
        }
        yaw_drift = pg.yaw_drift;
        for (int e = 0; e < 9; ++e) r_drift(e / 3, e % 3) = pg.r_drift[e];
        t_drift = Eigen::Vector3d(pg.t_drift[0], pg.t_drift[1], pg.t_drift[2]);
        return true;
    }
    std::list<KeyFrame*> keyframelist;
    std::queue<int> optimize_buf;
    int earliest_loop_index = -1, global_index = 0, sequence_cnt = 0;
    std::vector<int> sequence_loop = std::vector<int>(1, 0);
    Eigen::Vector3d t_drift, w_t_vio;
    Eigen::Matrix3d r_drift, w_r_vio;                          // (the identity at first: set entry by entry, no default is relied on)
    double yaw_drift = 0.0;
    vg_pg_out pg = {};

  private:
    vg_handle* h;
    int db;
    static double yawOf(const Eigen::Matrix3d& R) { return std::atan2(R(1, 0), R(0, 0)) / M_PI * 180.0; }      // Utility::R2ypr(R).x()
    static Eigen::Matrix3d yawRotation(double yaw) {                                                            // Utility::ypr2R({yaw, 0, 0})
        const double y = yaw / 180.0 * M_PI;
        Eigen::Matrix3d R;
        R(0, 0) = std::cos(y); R(0, 1) = -std::sin(y); R(0, 2) = 0.0;
        R(1, 0) = std::sin(y); R(1, 1) = std::cos(y); R(1, 2) = 0.0;
        R(2, 0) = 0.0; R(2, 1) = 0.0; R(2, 2) = 1.0;
        return R;
    }
    void run(KeyFrame* keyframe, int frame_index, int flags) {
        vg_bow_in in;
        vg_pack_bow(*keyframe, db, frame_index, flags, in, last);
        if (vg_kf_loop_detect(h, 1, &in, &last) != VG_OK) throw std::runtime_error(vg_last_error(h));
    }
};
