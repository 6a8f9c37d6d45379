// replay_main.cpp — ROS-free replay harness for the drop-in classes (SURVEY.md 8(d) configs[0] substitute).
//
//   vins_replay fe <frames.bin> <out.txt> [config.yaml]   frames.bin = int32 n, w, h, pub_every ; n * w*h bytes
//     feeds the frames through FeatureTracker::readImage exactly as img_callback does (feature_tracker_node.cpp:86-111:
//     readImage, then updateID for every feature) and dumps, per frame, ids / cur_pts / track_cnt / cur_un_pts / velocity.
//     With config.yaml the front-end parameters and the camera (model_type PINHOLE or MEI) come from that file, through
//     readFeatureTrackerParameters and FeatureTracker::readIntrinsicParameter as in the node (feature_tracker_node.cpp:205-208);
//     without it: the built-in EuRoC values.  `fe_batch <list.txt> <out_prefix> [config.yaml]` takes the same argument for all streams.
//
//   vins_replay ba <sequence.bin> <out.csv>
//     N consecutive sliding windows through the drop-in Estimator the way process() drives it once the system is
//     initialised (estimator.cpp:120-170): IMU pre-integration of the new frame interval (here: vg_imu_preintegrate on
//     the device instead of processIMU's sample-by-sample push_back), Estimator::optimization() (solve + MARGIN_OLD
//     marginalization, prior carried over through last_marginalization_info / ..._parameter_blocks) and
//     Estimator::slideWindow() (state shift + removeBackShiftDepth).  Writes one line per window in the format of
//     pubOdometry's result file (utility/visualization.cpp:157-172): stamp[ns], P, Q(w x y z), V of frame WINDOW_SIZE.
//     sequence.bin is written by tests/replay_util.py.
//
//   vins_replay seq <frames.bin> <out.csv>
//     N estimators whose windows stay ON THE DEVICE (ResidentEstimators, resident_estimator.h): the file holds, per estimator, the
//     window as it stands between two frames (states, the IMU samples of its intervals, every track) and then W frames at the level
//     of the node's callbacks: the IMU samples since the last frame (processIMU) and the `image` map (processImage).  One line per
//     frame and estimator: index, stamp[ns], P, Q(w x y z), V of frame WINDOW_SIZE as solved, the key-frame decision, tracks left.
//
//   vins_replay vio <window.bin> <frames.bin> <out.csv>
//     Both drop-ins in one process, wired the way the two nodes are (feature_tracker_node.cpp:86-160 publishes id / undistorted
//     point / pixel / velocity of every feature with track_cnt > 1; estimator_node.cpp:286-306 turns that message into the `image`
//     map of processImage): `seq` for one estimator whose tracks are NOT in the file (window.bin holds states and IMU samples only,
//     L = 0 and n = 0) but come from FeatureTracker::readImage over frames.bin -- the first WINDOW_SIZE frames fill the window that
//     is handed over, every further frame is one processImage + solve.  tests/e2e_vio.py renders the frames.
//
//   vins_replay align <in.bin> <out.txt>
//     Estimator::visualInitialAlign() (vg_init_align, vg_triangulate with a zero tic, the depth scaling) over one all_image_frame map
//     from a file; writes the status, Bgs[0], g, the window's Ps / Rs / Vs and the landmarks' depths (replay_align below).
//
//   vins_replay sfm <in.bin> <out.txt>
//     Estimator::initialStructure(l, relative_R, relative_T) (vg_init_sfm, then visualInitialAlign) over f_manager.feature and one
//     all_image_frame map from a file; writes the statuses, every entry's is_key_frame / R / T and what `align` writes (replay_sfm below).
//
//   vins_replay kf <in.bin> <out.txt> <brief_pattern.yml>
//     keyframes and loop candidates of the pose graph through class KeyFrame (host/keyframe.h, vg_kf_*; replay_kf below).
//   vins_replay kf_pattern <brief_pattern.yml>
//     host only: prints the four lists of 256 integers that BriefExtractor reads from the yml.
//   vins_replay exrot <in.bin> <out.txt>
//     the extrinsic-rotation calibration of processImage, one vg_init_exrot call per frame (replay_exrot below).
//   vins_replay bow <voc.bin> <frames.bin> <out.txt>
//     BriefVocabulary and PoseGraph::loadVocabulary / detectLoop (host/pose_graph.h, vg_kf_loop_detect through vg_pack_bow; replay_bow below).
//   vins_replay kfpnp <in.bin> <out.txt>
//     KeyFrame::PnPRANSAC and findConnection's second half (vg_kf_pnp through vg_pack_kf_pnp) over the matched lists of a file
//     (replay_kfpnp below).
//   vins_replay pgo <in.bin> <out.txt>
//     PoseGraph's pose bookkeeping and ONE pass of optimize4DoF (host/pose_graph.h, vg_pg_optimize through vg_pack_pg) over the slice of
//     a keyframe list from a file: every keyframe goes through shiftToBase / addLoop / appendKeyFrame, then the pass (replay_pgo below).
//   vins_replay relpose <in.bin> <out.txt>
//     Estimator::relativePose(relative_R, relative_T, l) (vg_init_relpose) over f_manager.feature from a file; writes the return value,
//     the VG_RELPOSE_* status, l, relative_R and relative_T and, when no frame passes, what the zero-argument initialStructure() returns
//     and leaves in marginalization_flag (replay_relpose below).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <stdexcept>
#include <vector>
#include "estimator.h"
#include "feature_tracker.h"
#include "keyframe.h"
#include "pose_graph.h"
#include "resident_estimator.h"
#include "vg_pack.h"

// the front-end globals of a configuration file; the frames of the replay must have its image size, and there is no fisheye mask here
static void replay_fe_config(const char* config, int w, int h) {
    readFeatureTrackerParameters(config);
    if (COL != w || ROW != h) throw std::runtime_error("the configuration file's image size differs from the frames'");
    if (FISHEYE) throw std::runtime_error("fisheye: 1 needs the mask image, which the replay does not load");
}

static int replay_fe(const char* in, const char* out, const char* config) {
    FILE* f = fopen(in, "rb");
    if (!f) { perror("frames"); return 2; }
    int hdr[4];
    if (fread(hdr, sizeof(int), 4, f) != 4) return 2;
    const int n = hdr[0], w = hdr[1], h = hdr[2], pub_every = hdr[3];
    COL = w; ROW = h;
    std::vector<unsigned char> buf((size_t)w * h);
    FeatureTracker tracker;
    if (config) {
        replay_fe_config(config, w, h);
        tracker.readIntrinsicParameter(config);
    }
    FILE* o = fopen(out, "w");
    for (int k = 0; k < n; ++k) {
        if (fread(buf.data(), 1, buf.size(), f) != buf.size()) return 2;
        PUB_THIS_FRAME = (k % pub_every) == 0;
        cv::Mat img(h, w, cv::CV_8UC1, buf.data(), (size_t)w);
        tracker.readImage(img, 0.05 * k);
        for (unsigned int i = 0;; i++) if (!tracker.updateID(i)) break;
        fprintf(o, "frame %d n %zu\n", k, tracker.cur_pts.size());
        for (size_t i = 0; i < tracker.cur_pts.size(); ++i)
            fprintf(o, "%d %d %.9g %.9g %.9g %.9g %.9g %.9g\n", tracker.ids[i], tracker.track_cnt[i], tracker.cur_pts[i].x, tracker.cur_pts[i].y,
                    tracker.cur_un_pts[i].x, tracker.cur_un_pts[i].y, tracker.pts_velocity[i].x, tracker.pts_velocity[i].y);
    }
    fclose(o);
    fclose(f);
    return 0;
}

// `fe` for S streams advancing together on one handle (FeatureTrackerBatch): list.txt names S files of the `fe` input format with the
// same size, frame count and pub_every; stream c's lines go to <out_prefix><c>.txt in the `fe` output format
static int replay_fe_batch(const char* list, const char* out_prefix, const char* config) {
    std::vector<std::string> names;
    {
        FILE* l = fopen(list, "r");
        if (!l) { perror("list"); return 2; }
        char line[4096];
        while (fgets(line, sizeof(line), l)) {
            std::string s(line);
            while (!s.empty() && (s.back() == '\n' || s.back() == '\r' || s.back() == ' ')) s.pop_back();
            if (!s.empty()) names.push_back(s);
        }
        fclose(l);
    }
    const int S = (int)names.size();
    if (S < 1) { fprintf(stderr, "vins_replay fe_batch: empty list\n"); return 2; }
    std::vector<FILE*> f((size_t)S, nullptr), o((size_t)S, nullptr);
    int n = 0, w = 0, h = 0, pub_every = 1;
    for (int c = 0; c < S; ++c) {
        f[c] = fopen(names[c].c_str(), "rb");
        if (!f[c]) { perror(names[c].c_str()); return 2; }
        int hdr[4];
        if (fread(hdr, sizeof(int), 4, f[c]) != 4) return 2;
        if (c == 0) { n = hdr[0]; w = hdr[1]; h = hdr[2]; pub_every = hdr[3]; }
        else if (hdr[0] != n || hdr[1] != w || hdr[2] != h || hdr[3] != pub_every) {
            fprintf(stderr, "vins_replay fe_batch: %s differs from the first file in size, frame count or pub_every\n", names[c].c_str());
            return 2;
        }
        o[c] = fopen((std::string(out_prefix) + std::to_string(c) + ".txt").c_str(), "w");
        if (!o[c]) { perror("output"); return 2; }
    }
    COL = w; ROW = h;
    std::vector<std::vector<unsigned char>> buf((size_t)S, std::vector<unsigned char>((size_t)w * h));
    FeatureTrackerBatch batch(S);
    if (config) {
        replay_fe_config(config, w, h);
        for (int c = 0; c < S; ++c) batch.trackers[c].readIntrinsicParameter(config);
    }
    std::vector<cv::Mat> imgs;
    std::vector<double> stamps((size_t)S);
    for (int k = 0; k < n; ++k) {
        imgs.clear();
        for (int c = 0; c < S; ++c) {
            if (fread(buf[c].data(), 1, buf[c].size(), f[c]) != buf[c].size()) return 2;
            imgs.push_back(cv::Mat(h, w, cv::CV_8UC1, buf[c].data(), (size_t)w));
            stamps[c] = 0.05 * k;
        }
        PUB_THIS_FRAME = (k % pub_every) == 0;
        batch.readImages(imgs, stamps);
        for (int c = 0; c < S; ++c) {
            FeatureTracker& tracker = batch.trackers[c];
            for (unsigned int i = 0;; i++) if (!tracker.updateID(i)) break;
            fprintf(o[c], "frame %d n %zu\n", k, tracker.cur_pts.size());
            for (size_t i = 0; i < tracker.cur_pts.size(); ++i)
                fprintf(o[c], "%d %d %.9g %.9g %.9g %.9g %.9g %.9g\n", tracker.ids[i], tracker.track_cnt[i], tracker.cur_pts[i].x, tracker.cur_pts[i].y,
                        tracker.cur_un_pts[i].x, tracker.cur_un_pts[i].y, tracker.pts_velocity[i].x, tracker.pts_velocity[i].y);
        }
    }
    for (int c = 0; c < S; ++c) { fclose(o[c]); fclose(f[c]); }
    return 0;
}

namespace {
struct Reader {
    FILE* f;
    void d(double* p, int n) { if (fread(p, sizeof(double), n, f) != (size_t)n) throw std::runtime_error("sequence file truncated"); }
    void i(int* p, int n) { if (fread(p, sizeof(int), n, f) != (size_t)n) throw std::runtime_error("sequence file truncated"); }
};
struct FrameInit { double t, pose[7], sb[9]; };

void set_frame(Estimator& e, int i, const FrameInit& fr) {
    e.Ps[i] = Vector3d(fr.pose[0], fr.pose[1], fr.pose[2]);
    e.Rs[i] = Quaterniond(fr.pose[6], fr.pose[3], fr.pose[4], fr.pose[5]).toRotationMatrix();
    e.Vs[i] = Vector3d(fr.sb[0], fr.sb[1], fr.sb[2]);
    e.Bas[i] = Vector3d(fr.sb[3], fr.sb[4], fr.sb[5]);
    e.Bgs[i] = Vector3d(fr.sb[6], fr.sb[7], fr.sb[8]);
}

// one frame interval: (acc_0, gyr_0) + S samples (dt, acc, gyr) -> IntegrationBase on the device
IntegrationBase* preintegrate(vg_handle* h, Reader& rd, int S, const double* bias, const double* noise) {
    double first[6];
    rd.d(first, 6);
    std::vector<double> smp((size_t)S * 7);
    rd.d(smp.data(), S * 7);
    const int off[2] = {0, S};
    vg_imu_preint out;
    if (vg_imu_preintegrate(h, 1, off, smp.data(), first, bias, noise, &out) != VG_OK) throw std::runtime_error(vg_last_error(h));
    IntegrationBase* p = new IntegrationBase();
    p->linearized_acc = Vector3d(first[0], first[1], first[2]);          // raw samples: slideWindow(MARGIN_SECOND_NEW) merges intervals
    p->linearized_gyr = Vector3d(first[3], first[4], first[5]);
    for (int i = 0; i < S; ++i) {
        p->dt_buf.push_back(smp[7 * i]);
        p->acc_buf.push_back(Vector3d(smp[7 * i + 1], smp[7 * i + 2], smp[7 * i + 3]));
        p->gyr_buf.push_back(Vector3d(smp[7 * i + 4], smp[7 * i + 5], smp[7 * i + 6]));
    }
    vg_pack::preint_from_abi(*p, out);
    return p;
}
}  // namespace

static int replay_ba(const char* in, const char* out) {
    Reader rd{fopen(in, "rb")};
    if (!rd.f) { perror("sequence"); return 2; }
    int hdr[4];
    rd.i(hdr, 4);
    if (hdr[0] != 0x31414256) { fprintf(stderr, "not a VBA1 sequence file\n"); return 2; }
    const int W = hdr[1], K = hdr[2], S = hdr[3];
    if (K != WINDOW_SIZE + 1) { fprintf(stderr, "sequence has K = %d, the Estimator is built for %d\n", K, WINDOW_SIZE + 1); return 2; }
    double ex[7], noise[4], par[2], bias[6];
    rd.d(ex, 7); rd.d(noise, 4); rd.d(par, 2); rd.d(bias, 6);
    G_NORM = par[0]; FOCAL_LENGTH_D = par[1]; ESTIMATE_EXTRINSIC = 0; ESTIMATE_TD = 0; NUM_ITERATIONS = 8;
    ACC_N = noise[0]; GYR_N = noise[1]; ACC_W = noise[2]; GYR_W = noise[3];
    vg_handle* h = nullptr;
    if (vg_create(&h) != VG_OK) { fprintf(stderr, "vg_create failed (no CPU fallback)\n"); return 3; }
    Estimator est;
    est.tic[0] = Vector3d(ex[0], ex[1], ex[2]);
    est.ric[0] = Quaterniond(ex[6], ex[3], ex[4], ex[5]).toRotationMatrix();
    std::vector<double> stamp(K);
    for (int i = 0; i < K; ++i) {
        FrameInit fr;
        rd.d(&fr.t, 1); rd.d(fr.pose, 7); rd.d(fr.sb, 9);
        set_frame(est, i, fr);
        stamp[i] = fr.t;
    }
    for (int i = 0; i + 1 < K; ++i) est.pre_integrations[i + 1] = preintegrate(h, rd, S, bias, noise);
    FILE* o = fopen(out, "w");
    for (int w = 0; w < W; ++w) {
        if (w > 0) {
            est.marginalization_flag = Estimator::MARGIN_OLD;
            est.slideWindow();                                           // (deletes the IntegrationBase that rotated out, like the reference)
            for (int i = 0; i + 1 < K; ++i) stamp[i] = stamp[i + 1];
            FrameInit fr;
            rd.d(&fr.t, 1); rd.d(fr.pose, 7); rd.d(fr.sb, 9);
            set_frame(est, WINDOW_SIZE, fr);
            stamp[K - 1] = fr.t;
            est.pre_integrations[WINDOW_SIZE] = preintegrate(h, rd, S, bias, noise);
        }
        // features of this window: tracks from the file, depths carried over by removeBackShiftDepth where the track existed
        std::map<int, double> carried;
        for (auto& f : est.f_manager.feature) carried[f.feature_id] = f.estimated_depth;
        est.f_manager.feature.clear();
        int L;
        rd.i(&L, 1);
        for (int l = 0; l < L; ++l) {
            int meta[3];
            double init_inv_depth;
            rd.i(meta, 3);
            rd.d(&init_inv_depth, 1);
            FeaturePerId f;
            f.feature_id = meta[0]; f.start_frame = meta[1];
            for (int k = 0; k < meta[2]; ++k) {
                double r[7];
                rd.d(r, 7);
                FeaturePerFrame fr;
                fr.point = Vector3d(r[0], r[1], 1.0); fr.uv.x() = r[2]; fr.uv.y() = r[3]; fr.velocity.x() = r[4]; fr.velocity.y() = r[5]; fr.cur_td = r[6];
                f.feature_per_frame.push_back(fr);
            }
            auto it = carried.find(f.feature_id);
            f.estimated_depth = it != carried.end() ? it->second : 1.0 / init_inv_depth;
            est.f_manager.feature.push_back(f);
        }
        est.marginalization_flag = Estimator::MARGIN_OLD;
        est.optimization();
        const Quaterniond q(est.Rs[WINDOW_SIZE]);
        fprintf(o, "%.0f,%.5f,%.5f,%.5f,%.5f,%.5f,%.5f,%.5f,%.5f,%.5f,%.5f,\n", stamp[K - 1] * 1e9, est.Ps[WINDOW_SIZE].x(), est.Ps[WINDOW_SIZE].y(),
                est.Ps[WINDOW_SIZE].z(), q.w(), q.x(), q.y(), q.z(), est.Vs[WINDOW_SIZE].x(), est.Vs[WINDOW_SIZE].y(), est.Vs[WINDOW_SIZE].z());
    }
    for (int k = 0; k <= WINDOW_SIZE; ++k) { delete est.pre_integrations[k]; est.pre_integrations[k] = nullptr; }   // (the harness owns them, like the reference's clearState)
    fclose(o);
    fclose(rd.f);
    vg_destroy(h);
    return 0;
}

// vins_replay align <in.bin> <out.txt>: Estimator::visualInitialAlign() over one all_image_frame map from a file
// (tests/init_align_ref.write_replay): int32 'VAL1', F, K, L; doubles ba0 3, bg0 3, noise 4, tic 3, ric 9, g_norm, init_depth; per
// frame stamp, R 9 (row-major), T 3; per interval int32 n, then acc_0 gyr_0 and n rows dt acc gyr; K int32 frame indices of the
// window; per landmark int32 start_frame, n_obs and n_obs points x y z.  Writes the return value and the VG_ALIGN_* status, Bgs[0], g,
// per window frame P, R, V, and every landmark's estimated_depth, all with 17 digits.
static int replay_align(const char* in, const char* out) {
    Reader rd{fopen(in, "rb")};
    if (!rd.f) { perror("align file"); return 2; }
    int hdr[4];
    rd.i(hdr, 4);
    if (hdr[0] != 0x314C4156) { fprintf(stderr, "not a VAL1 file\n"); return 2; }
    const int F = hdr[1], K = hdr[2], L = hdr[3];
    if (K < 2 || K > WINDOW_SIZE + 1 || F < K) { fprintf(stderr, "K = %d, F = %d: the Estimator holds 2 .. %d window frames\n", K, F, WINDOW_SIZE + 1); return 2; }
    double b[6], noise[4], ex[12], par[2];
    rd.d(b, 6); rd.d(noise, 4); rd.d(ex, 12); rd.d(par, 2);
    ACC_N = noise[0]; GYR_N = noise[1]; ACC_W = noise[2]; GYR_W = noise[3]; G_NORM = par[0]; INIT_DEPTH = par[1];
    Estimator est;
    est.tic[0] = Vector3d(ex[0], ex[1], ex[2]);
    for (int e = 0; e < 9; ++e) est.ric[0](e / 3, e % 3) = ex[3 + e];
    for (int i = 0; i <= WINDOW_SIZE; ++i) { est.Bas[i] = Vector3d(b[0], b[1], b[2]); est.Bgs[i] = Vector3d(b[3], b[4], b[5]); }
    std::vector<double> stamp(F);
    std::vector<std::unique_ptr<IntegrationBase>> owned;
    for (int k = 0; k < F; ++k) {
        double fr[13];
        rd.d(fr, 13);
        stamp[k] = fr[0];
        ImageFrame& f = est.all_image_frame[fr[0]];
        for (int e = 0; e < 9; ++e) f.R(e / 3, e % 3) = fr[1 + e];
        f.T = Vector3d(fr[10], fr[11], fr[12]);
    }
    for (int k = 1; k < F; ++k) {
        int n;
        double first[6];
        rd.i(&n, 1); rd.d(first, 6);
        std::vector<double> smp((size_t)n * 7);
        rd.d(smp.data(), n * 7);
        owned.emplace_back(new IntegrationBase());
        IntegrationBase* p = owned.back().get();
        p->linearized_acc = Vector3d(first[0], first[1], first[2]);
        p->linearized_gyr = Vector3d(first[3], first[4], first[5]);
        for (int i = 0; i < n; ++i) {
            p->dt_buf.push_back(smp[7 * i]);
            p->acc_buf.push_back(Vector3d(smp[7 * i + 1], smp[7 * i + 2], smp[7 * i + 3]));
            p->gyr_buf.push_back(Vector3d(smp[7 * i + 4], smp[7 * i + 5], smp[7 * i + 6]));
        }
        est.all_image_frame[stamp[k]].pre_integration = p;
    }
    std::vector<int> key(K);
    rd.i(key.data(), K);
    est.frame_count = K - 1;
    for (int i = 0; i < K; ++i) est.Headers[i] = stamp[key[i]];
    for (int l = 0; l < L; ++l) {
        int meta[2];
        rd.i(meta, 2);
        FeaturePerId f;
        f.feature_id = l; f.start_frame = meta[0];
        for (int k = 0; k < meta[1]; ++k) {
            double r[3];
            rd.d(r, 3);
            FeaturePerFrame fr;
            fr.point = Vector3d(r[0], r[1], r[2]);
            f.feature_per_frame.push_back(fr);
        }
        est.f_manager.feature.push_back(f);
    }
    fclose(rd.f);
    const bool ok = est.visualInitialAlign();
    FILE* o = fopen(out, "w");
    if (!o) { perror("out"); return 2; }
    fprintf(o, "result %d %d\n", ok ? 1 : 0, est.align_status);
    fprintf(o, "bg %.17g %.17g %.17g\n", est.Bgs[0].x(), est.Bgs[0].y(), est.Bgs[0].z());
    fprintf(o, "g %.17g %.17g %.17g\n", est.g.x(), est.g.y(), est.g.z());
    for (int i = 0; ok && i < K; ++i) {
        fprintf(o, "frame %.17g %.17g %.17g", est.Ps[i].x(), est.Ps[i].y(), est.Ps[i].z());
        for (int e = 0; e < 9; ++e) fprintf(o, " %.17g", est.Rs[i](e / 3, e % 3));
        fprintf(o, " %.17g %.17g %.17g\n", est.Vs[i].x(), est.Vs[i].y(), est.Vs[i].z());
    }
    for (auto& f : est.f_manager.feature) fprintf(o, "depth %.17g\n", f.estimated_depth);
    fclose(o);
    return 0;
}

// vins_replay sfm <in.bin> <out.txt>: Estimator::initialStructure(l, relative_R, relative_T) over f_manager.feature and one
// all_image_frame map from a file (tests/init_sfm_ref.write_replay): int32 'VSR1', A (entries of all_image_frame), K (window frames), L
// (features), l; doubles ba0 3, bg0 3, noise 4, tic 3, ric 9, g_norm, init_depth, relative_R 9, relative_T 3; per entry its stamp, int32
// n and n times (int32 id, double x y): its points map; per interval int32 n, then acc_0 gyr_0 and n rows dt acc gyr; K int32 entry
// indices of the window; per feature int32 id, start_frame, n_obs and n_obs points x y z.  Writes the return value, the VG_SFM_* and
// VG_ALIGN_* statuses and marginalization_flag, per entry is_key_frame, R, T, then what `align` writes, all with 17 digits.
static int replay_sfm(const char* in, const char* out) {
    Reader rd{fopen(in, "rb")};
    if (!rd.f) { perror("sfm file"); return 2; }
    int hdr[5];
    rd.i(hdr, 5);
    if (hdr[0] != 0x31525356) { fprintf(stderr, "not a VSR1 file\n"); return 2; }
    const int A = hdr[1], K = hdr[2], L = hdr[3], l = hdr[4];
    if (K < 3 || K > WINDOW_SIZE + 1 || A < K) { fprintf(stderr, "K = %d, A = %d: the Estimator holds 3 .. %d window frames\n", K, A, WINDOW_SIZE + 1); return 2; }
    double b[6], noise[4], ex[12], par[2], rel[12];
    rd.d(b, 6); rd.d(noise, 4); rd.d(ex, 12); rd.d(par, 2); rd.d(rel, 12);
    ACC_N = noise[0]; GYR_N = noise[1]; ACC_W = noise[2]; GYR_W = noise[3]; G_NORM = par[0]; INIT_DEPTH = par[1];
    Estimator est;
    est.tic[0] = Vector3d(ex[0], ex[1], ex[2]);
    Matrix3d relative_R;
    for (int e = 0; e < 9; ++e) { est.ric[0](e / 3, e % 3) = ex[3 + e]; relative_R(e / 3, e % 3) = rel[e]; }
    const Vector3d relative_T(rel[9], rel[10], rel[11]);
    for (int i = 0; i <= WINDOW_SIZE; ++i) { est.Bas[i] = Vector3d(b[0], b[1], b[2]); est.Bgs[i] = Vector3d(b[3], b[4], b[5]); }
    std::vector<double> stamp(A);
    std::vector<std::unique_ptr<IntegrationBase>> owned;
    for (int k = 0; k < A; ++k) {
        int n;
        rd.d(&stamp[k], 1); rd.i(&n, 1);
        ImageFrame& f = est.all_image_frame[stamp[k]];
        for (int i = 0; i < n; ++i) {
            int id;
            double xy[2];
            rd.i(&id, 1); rd.d(xy, 2);
            Eigen::Matrix<double, 7, 1> m;
            m(0, 0) = xy[0]; m(1, 0) = xy[1]; m(2, 0) = 1.0;
            f.points[id].emplace_back(0, m);
        }
    }
    for (int k = 1; k < A; ++k) {
        int n;
        double first[6];
        rd.i(&n, 1); rd.d(first, 6);
        std::vector<double> smp((size_t)n * 7);
        rd.d(smp.data(), n * 7);
        owned.emplace_back(new IntegrationBase());
        IntegrationBase* p = owned.back().get();
        p->linearized_acc = Vector3d(first[0], first[1], first[2]);
        p->linearized_gyr = Vector3d(first[3], first[4], first[5]);
        for (int i = 0; i < n; ++i) {
            p->dt_buf.push_back(smp[7 * i]);
            p->acc_buf.push_back(Vector3d(smp[7 * i + 1], smp[7 * i + 2], smp[7 * i + 3]));
            p->gyr_buf.push_back(Vector3d(smp[7 * i + 4], smp[7 * i + 5], smp[7 * i + 6]));
        }
        est.all_image_frame[stamp[k]].pre_integration = p;
    }
    std::vector<int> key(K);
    rd.i(key.data(), K);
    est.frame_count = K - 1;
    for (int i = 0; i < K; ++i) est.Headers[i] = stamp[key[i]];
    for (int j = 0; j < L; ++j) {
        int meta[3];
        rd.i(meta, 3);
        FeaturePerId f;
        f.feature_id = meta[0]; f.start_frame = meta[1];
        for (int k = 0; k < meta[2]; ++k) {
            double r[3];
            rd.d(r, 3);
            FeaturePerFrame fr;
            fr.point = Vector3d(r[0], r[1], r[2]);
            f.feature_per_frame.push_back(fr);
        }
        est.f_manager.feature.push_back(f);
    }
    fclose(rd.f);
    est.marginalization_flag = Estimator::MARGIN_SECOND_NEW;    // (so that the MARGIN_OLD of a construct failure shows)
    const bool ok = est.initialStructure(l, relative_R, relative_T);
    FILE* o = fopen(out, "w");
    if (!o) { perror("out"); return 2; }
    fprintf(o, "result %d %d %d %d\n", ok ? 1 : 0, est.sfm_status, est.align_status, (int)est.marginalization_flag);
    for (auto& kv : est.all_image_frame) {
        fprintf(o, "entry %d", kv.second.is_key_frame ? 1 : 0);
        for (int e = 0; e < 9; ++e) fprintf(o, " %.17g", kv.second.R(e / 3, e % 3));
        fprintf(o, " %.17g %.17g %.17g\n", kv.second.T.x(), kv.second.T.y(), kv.second.T.z());
    }
    fprintf(o, "bg %.17g %.17g %.17g\n", est.Bgs[0].x(), est.Bgs[0].y(), est.Bgs[0].z());
    fprintf(o, "g %.17g %.17g %.17g\n", est.g.x(), est.g.y(), est.g.z());
    for (int i = 0; ok && i < K; ++i) {
        fprintf(o, "frame %.17g %.17g %.17g", est.Ps[i].x(), est.Ps[i].y(), est.Ps[i].z());
        for (int e = 0; e < 9; ++e) fprintf(o, " %.17g", est.Rs[i](e / 3, e % 3));
        fprintf(o, " %.17g %.17g %.17g\n", est.Vs[i].x(), est.Vs[i].y(), est.Vs[i].z());
    }
    for (auto& f : est.f_manager.feature) fprintf(o, "depth %.17g\n", f.estimated_depth);
    fclose(o);
    return 0;
}

// vins_replay relpose <in.bin> <out.txt>: Estimator::relativePose over f_manager.feature from a file (tests/init_relpose_ref.write_file):
// int32 'VRP1', F (window frames), L (features), rows; L int32 start_frame, L int32 n_obs, L int32 first row; rows x y z.  Writes
// "result <return value> <VG_RELPOSE_*> <l>", "R" with nine numbers, "T" with three (17 digits) and, when relativePose returned false,
// "structure <return value of initialStructure()> <marginalization_flag>".
static int replay_relpose(const char* in, const char* out) {
    Reader rd{fopen(in, "rb")};
    if (!rd.f) { perror("relpose file"); return 2; }
    int hdr[4];
    rd.i(hdr, 4);
    if (hdr[0] != 0x31505256) { fprintf(stderr, "not a VRP1 file\n"); return 2; }
    const int K = hdr[1], L = hdr[2], rows = hdr[3];
    if (K < 3 || K > WINDOW_SIZE + 1) { fprintf(stderr, "K = %d: the Estimator holds 3 .. %d window frames\n", K, WINDOW_SIZE + 1); return 2; }
    std::vector<int> start(L), nobs(L), off(L);
    std::vector<double> pts((size_t)rows * 3);
    rd.i(start.data(), L); rd.i(nobs.data(), L); rd.i(off.data(), L); rd.d(pts.data(), rows * 3);
    fclose(rd.f);
    Estimator est;
    est.frame_count = K - 1;
    for (int j = 0; j < L; ++j) {
        FeaturePerId f;
        f.feature_id = j; f.start_frame = start[j];
        for (int k = 0; k < nobs[j]; ++k) {
            FeaturePerFrame fr;
            const double* r = &pts[3 * ((size_t)off[j] + k)];
            fr.point = Vector3d(r[0], r[1], r[2]);
            f.feature_per_frame.push_back(fr);
        }
        est.f_manager.feature.push_back(f);
    }
    Matrix3d relative_R;
    for (int e = 0; e < 9; ++e) relative_R(e / 3, e % 3) = 0.0;
    Vector3d relative_T(0.0, 0.0, 0.0);
    int l = -2;
    const bool ok = est.relativePose(relative_R, relative_T, l);
    FILE* o = fopen(out, "w");
    if (!o) { perror("out"); return 2; }
    fprintf(o, "result %d %d %d\n", ok ? 1 : 0, est.relpose_status, l);
    fprintf(o, "R");
    for (int e = 0; e < 9; ++e) fprintf(o, " %.17g", relative_R(e / 3, e % 3));
    fprintf(o, "\nT %.17g %.17g %.17g\n", relative_T.x(), relative_T.y(), relative_T.z());
    if (!ok) {
        est.marginalization_flag = Estimator::MARGIN_SECOND_NEW;    // (initialStructure() must leave it alone when no frame passes)
        const bool st = est.initialStructure();
        fprintf(o, "structure %d %d\n", st ? 1 : 0, (int)est.marginalization_flag);
    }
    fclose(o);
    return 0;
}

// vins_replay kf <in.bin> <out.txt> <brief_pattern.yml>: class KeyFrame (host/keyframe.h, BriefExtractor, vg_pack_kf) over a file of
// keyframes and pairs (tests/kf_brief_ref.write_replay_file): int32 'KFR1', W, H, max_keypoints, max_window_points, n_frames, n_pairs; per
// frame int32 n_window, the points (float32), int32 camera model, p[8] and xi (float64), the image; then the pairs (current, old).  Writes
// per keyframe "kf <i> <true count> <status> <kept> <n_window>", a "k" line per keypoint (x y score, the norm's bits, the four words) and a
// "w" line per window descriptor; per pair "pair <p> <cur> <old> <n_matched> <findConnection's return value>", an "s" line per window
// point (status, best index and distance, the matched point and norm as bits) and an "m" line per survivor of reduceVector.
static unsigned kf_bits(float v) { unsigned u; memcpy(&u, &v, 4); return u; }
static int replay_kf(const char* in, const char* out, const char* pattern_file) {
    Reader rd{fopen(in, "rb")};
    if (!rd.f) { perror("kf file"); return 2; }
    int hdr[7];
    rd.i(hdr, 7);
    if (hdr[0] != 0x3152464B) { fprintf(stderr, "not a KFR1 file\n"); return 2; }
    const int W = hdr[1], H = hdr[2], MK = hdr[3], MW = hdr[4], NF = hdr[5], NP = hdr[6];
    if (W < 1 || H < 1 || NF < 1 || NP < 0) { fprintf(stderr, "bad header\n"); return 2; }
    vg_handle* h = nullptr;
    if (vg_create(&h) != VG_OK) { fprintf(stderr, "vg_create failed\n"); return 1; }
    FILE* o = fopen(out, "w");
    if (!o) { perror("out"); return 2; }
    {
        BriefExtractor extractor(pattern_file);
        KeyFrame::configure(h, extractor, W, H, MK, MW, NF);
        std::vector<std::unique_ptr<KeyFrame>> kfs;
        for (int i = 0; i < NF; ++i) {
            int nw = 0, model = 0;
            rd.i(&nw, 1);
            std::vector<cv::Point2f> uv((size_t)nw);
            if (nw && fread(uv.data(), sizeof(cv::Point2f), nw, rd.f) != (size_t)nw) throw std::runtime_error("kf file truncated");
            rd.i(&model, 1);
            vg_fe_camera cam;
            memset(&cam, 0, sizeof(cam));
            cam.struct_size = (int)sizeof(cam); cam.model = model;
            rd.d(cam.p, 8); rd.d(&cam.xi, 1);
            cv::Mat img(H, W, cv::CV_8UC1, (uchar)0);
            if (fread(img.data, 1, (size_t)W * H, rd.f) != (size_t)W * H) throw std::runtime_error("kf file truncated");
            kfs.emplace_back(new KeyFrame(h, i, 0.05 * i, i, img, uv, cam));
            const KeyFrame& k = *kfs.back();
            fprintf(o, "kf %d %d %d %d %d\n", i, k.n_true, k.kf_status, (int)k.keypoints.size(), (int)k.window_brief_descriptors.size());
            for (size_t q = 0; q < k.keypoints.size(); ++q) {
                const BRIEF::bitset& d = k.brief_descriptors[q];
                fprintf(o, "k %.9g %.9g %d %08x %08x %016llx %016llx %016llx %016llx\n", k.keypoints[q].pt.x, k.keypoints[q].pt.y, (int)k.keypoints[q].response,
                        kf_bits(k.keypoints_norm[q].pt.x), kf_bits(k.keypoints_norm[q].pt.y), (unsigned long long)d[0], (unsigned long long)d[1],
                        (unsigned long long)d[2], (unsigned long long)d[3]);
            }
            for (const BRIEF::bitset& d : k.window_brief_descriptors)
                fprintf(o, "w %016llx %016llx %016llx %016llx\n", (unsigned long long)d[0], (unsigned long long)d[1], (unsigned long long)d[2], (unsigned long long)d[3]);
        }
        for (int p = 0; p < NP; ++p) {
            int pr[2];
            rd.i(pr, 2);
            if (pr[0] < 0 || pr[0] >= NF || pr[1] < 0 || pr[1] >= NF) throw std::runtime_error("a pair names no keyframe");
            KeyFrame& cur = *kfs[pr[0]];
            std::vector<cv::Point2f> m_old, m_old_norm, c_cur, c_old, c_old_norm;
            std::vector<uchar> status;
            std::vector<int> index;
            cur.searchByBRIEFDes(m_old, m_old_norm, status, *kfs[pr[1]]);
            const bool ok = cur.findConnection(*kfs[pr[1]], c_cur, c_old, c_old_norm, index);
            fprintf(o, "pair %d %d %d %d %d\n", p, pr[0], pr[1], (int)index.size(), ok ? 1 : 0);
            for (size_t w = 0; w < status.size(); ++w)
                fprintf(o, "s %d %d %d %08x %08x %08x %08x\n", (int)status[w], cur.best_idx[w], cur.best_dist[w], kf_bits(m_old[w].x), kf_bits(m_old[w].y),
                        kf_bits(m_old_norm[w].x), kf_bits(m_old_norm[w].y));
            for (size_t k = 0; k < index.size(); ++k)
                fprintf(o, "m %d %08x %08x %08x %08x %08x %08x\n", index[k], kf_bits(c_cur[k].x), kf_bits(c_cur[k].y), kf_bits(c_old[k].x), kf_bits(c_old[k].y),
                        kf_bits(c_old_norm[k].x), kf_bits(c_old_norm[k].y));
        }
    }
    fclose(rd.f);
    fclose(o);
    vg_destroy(h);
    return 0;
}

// vins_replay exrot <in.bin> <out.txt>: the ESTIMATE_EXTRINSIC == 2 block of processImage (Estimator::calibrateExtrinsicRotation, class
// InitialEXRotation, vg_pack_exrot) fed ONE FRAME AT A TIME from a file (tests/init_exrot_ref.write_file): int32 'VEX1', S (steps), rows;
// S + 1 int32 first rows; rows x0 y0 x1 y1; S rows w x y z.  Per step it writes "step <k> <return value> <VG_EXROT_*> <ESTIMATE_EXTRINSIC
// after>", "ric" with nine numbers and "sigma" with four (17 digits); after a success the block no longer applies, as in the reference, and
// the remaining steps are written as "skipped <k>"; "calib" is ric[0] at the end.
static int replay_exrot(const char* in, const char* out) {
    Reader rd{fopen(in, "rb")};
    if (!rd.f) { perror("exrot file"); return 2; }
    int hdr[3];
    rd.i(hdr, 3);
    if (hdr[0] != 0x31584556) { fprintf(stderr, "not a VEX1 file\n"); return 2; }
    const int S = hdr[1], rows = hdr[2];
    if (S < 1 || rows < 0) { fprintf(stderr, "S = %d, rows = %d\n", S, rows); return 2; }
    std::vector<int> off(S + 1);
    std::vector<double> corr((size_t)rows * 4 + 4), dq((size_t)S * 4);
    rd.i(off.data(), S + 1); rd.d(corr.data(), rows * 4); rd.d(dq.data(), S * 4);
    fclose(rd.f);
    FILE* o = fopen(out, "w");
    if (!o) { perror("out"); return 2; }
    Estimator est;
    ESTIMATE_EXTRINSIC = 2;                                     // as readEstimatorParameters leaves the globals for estimate_extrinsic: 2
    RIC.assign(1, Matrix3d());
    TIC.assign(1, Vector3d());
    IntegrationBase ib;
    for (int k = 0; k < S; ++k) {
        if (ESTIMATE_EXTRINSIC != 2) { fprintf(o, "skipped %d\n", k); continue; }
        // the two newest frames of a window: every correspondence is a feature seen in both
        est.frame_count = 1;
        est.f_manager.feature.clear();
        for (int j = off[k]; j < off[k + 1]; ++j) {
            FeaturePerId f;
            f.feature_id = j; f.start_frame = 0;
            FeaturePerFrame a, b;
            a.point = Vector3d(corr[4 * (size_t)j], corr[4 * (size_t)j + 1], 1.0);
            b.point = Vector3d(corr[4 * (size_t)j + 2], corr[4 * (size_t)j + 3], 1.0);
            f.feature_per_frame.push_back(a); f.feature_per_frame.push_back(b);
            est.f_manager.feature.push_back(f);
        }
        ib.delta_q = Quaterniond(dq[4 * (size_t)k], dq[4 * (size_t)k + 1], dq[4 * (size_t)k + 2], dq[4 * (size_t)k + 3]);
        est.pre_integrations[1] = &ib;
        const bool ok = est.calibrateExtrinsicRotation();
        est.pre_integrations[1] = nullptr;
        fprintf(o, "step %d %d %d %d\nric", k, ok ? 1 : 0, est.exrot_status, ESTIMATE_EXTRINSIC);
        for (int e = 0; e < 9; ++e) fprintf(o, " %.17g", est.initial_ex_rotation.ric(e / 3, e % 3));
        fprintf(o, "\nsigma");
        for (int e = 0; e < 4; ++e) fprintf(o, " %.17g", est.initial_ex_rotation.sigma[e]);
        fprintf(o, "\n");
    }
    fprintf(o, "calib");
    for (int e = 0; e < 9; ++e) fprintf(o, " %.17g", est.ric[0](e / 3, e % 3));
    fprintf(o, "\n");
    fclose(o);
    return 0;
}

namespace {
// the front end of `vio`: one frame through readImage + updateID, returned as the `image` map (features seen at least twice)
struct FrontEnd {
    FILE* f = nullptr;
    int n = 0, w = 0, h = 0, k = 0;
    std::vector<unsigned char> buf;
    std::unique_ptr<FeatureTracker> tracker;
    bool open(const char* path) {
        f = fopen(path, "rb");
        int hdr[4];
        if (!f || fread(hdr, sizeof(int), 4, f) != 4) return false;
        n = hdr[0]; w = hdr[1]; h = hdr[2];
        COL = w; ROW = h;
        buf.resize((size_t)w * h);
        tracker.reset(new FeatureTracker());
        return true;
    }
    ResidentEstimators::Image next() {
        if (k >= n || fread(buf.data(), 1, buf.size(), f) != buf.size()) throw std::runtime_error("frames file exhausted");
        PUB_THIS_FRAME = true;
        cv::Mat img(h, w, cv::CV_8UC1, buf.data(), (size_t)w);
        tracker->readImage(img, 0.05 * k++);
        for (unsigned int i = 0;; i++) if (!tracker->updateID(i)) break;
        ResidentEstimators::Image image;
        for (size_t i = 0; i < tracker->cur_pts.size(); ++i) {
            if (tracker->track_cnt[i] <= 1) continue;
            Eigen::Matrix<double, 7, 1> p;
            p(0, 0) = tracker->cur_un_pts[i].x; p(1, 0) = tracker->cur_un_pts[i].y; p(2, 0) = 1.0;
            p(3, 0) = tracker->cur_pts[i].x; p(4, 0) = tracker->cur_pts[i].y;
            p(5, 0) = tracker->pts_velocity[i].x; p(6, 0) = tracker->pts_velocity[i].y;
            image[tracker->ids[i]].emplace_back(0, p);
        }
        return image;
    }
    ~FrontEnd() { if (f) fclose(f); }
};
}  // namespace

static int replay_seq(const char* in, const char* out, const char* frames = nullptr) {
    Reader rd{fopen(in, "rb")};
    if (!rd.f) { perror("frames"); return 2; }
    FrontEnd fe;
    if (frames && !fe.open(frames)) { perror("images"); return 2; }
    int hdr[5];
    rd.i(hdr, 5);
    if (hdr[0] != 0x31515356) { fprintf(stderr, "not a VSQ1 file\n"); return 2; }
    const int N = hdr[1], W = hdr[2], K = hdr[3], S = hdr[4];
    if (K != WINDOW_SIZE + 1) { fprintf(stderr, "file has K = %d, the Estimator is built for %d\n", K, WINDOW_SIZE + 1); return 2; }
    double noise[4], par[4];
    rd.d(noise, 4); rd.d(par, 4);
    G_NORM = par[0]; FOCAL_LENGTH_D = par[1]; MIN_PARALLAX = par[2]; INIT_DEPTH = par[3];
    ESTIMATE_EXTRINSIC = 0; ESTIMATE_TD = 0; NUM_ITERATIONS = 8;
    ACC_N = noise[0]; GYR_N = noise[1]; ACC_W = noise[2]; GYR_W = noise[3];
    vg_handle* h = nullptr;
    if (vg_create(&h) != VG_OK) { fprintf(stderr, "vg_create failed (no CPU fallback)\n"); return 3; }
    std::unique_ptr<ResidentEstimators> resp(new ResidentEstimators(N, 512, 512));
    // VINS_REPLAY_HANDBACK=<frame>: after that frame every window is handed back into a host Estimator (handBack), a NEW batch
    // takes them over (handOver + begin) and estimator 0 is re-seeded once more in place (reseed): the rest of the run must not notice
    const char* hb_env = getenv("VINS_REPLAY_HANDBACK");
    const int handback_frame = hb_env ? atoi(hb_env) : -1;
    // VINS_REPLAY_DEVICE_IMU=1: processIMU on the device too (ResidentEstimators::useDeviceImu)
    const char* di_env = getenv("VINS_REPLAY_DEVICE_IMU");
    const bool device_imu = di_env && atoi(di_env) != 0;
    if (device_imu) resp->useDeviceImu();
    // VINS_REPLAY_TIMING=1: per frame "T,<frame>,<ms in processIMU>,<ms in solve()>" on stderr (tests/manual/gpu_seq_imu.py)
    const bool timing = getenv("VINS_REPLAY_TIMING") != nullptr;
    // VINS_REPLAY_RELO=<file>: relocalisation records, text: "frame estimator stamp n_match  prev_relo_t (3)  prev_relo_r (9, row-major)"
    // followed by n_match lines "x y feature_id".  Before that frame of the file setReloFrame() is called for the estimator
    // (ResidentEstimators::useRelocalisation), and after its solve() the by-products go to <out>.relo, one line per record:
    // frame,estimator,found,n_factors,local_index,relo_Pose (7),relo_relative_t (3),relo_relative_q (x y z w),relo_relative_yaw,
    // drift_correct_r (9),drift_correct_t (3)
    struct ReloRec { int frame, est; double stamp; Vector3d t; Matrix3d r; std::vector<Vector3d> match; bool found = false; };
    std::vector<ReloRec> relo;
    if (const char* rl_env = getenv("VINS_REPLAY_RELO")) {
        FILE* rf = fopen(rl_env, "r");
        if (!rf) { perror("relocalisation records"); return 2; }
        ReloRec q;
        int n = 0, max_match = 1;
        double t[3], r[9];
        while (fscanf(rf, "%d %d %lf %d %lf %lf %lf %lf %lf %lf %lf %lf %lf %lf %lf %lf", &q.frame, &q.est, &q.stamp, &n, &t[0], &t[1], &t[2], &r[0], &r[1], &r[2],
                      &r[3], &r[4], &r[5], &r[6], &r[7], &r[8]) == 16) {
            q.t = Vector3d(t[0], t[1], t[2]);
            for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) q.r(a, b) = r[3 * a + b];
            q.match.clear();
            for (int k = 0; k < n; ++k) {
                double x, y; int id;
                if (fscanf(rf, "%lf %lf %d", &x, &y, &id) != 3) { fprintf(stderr, "relocalisation records: short match list\n"); return 2; }
                q.match.push_back(Vector3d(x, y, id));
            }
            max_match = std::max(max_match, n);
            relo.push_back(q);
        }
        fclose(rf);
        resp->useRelocalisation(max_match);
    }
    // VINS_REPLAY_OUTPUTS=<max_points>: what the estimator node publishes after every frame (ResidentEstimators::usePublishedOutputs:
    // pubKeyframe / pubPointCloud formed on the device) goes to <out>.outputs, per frame and estimator:
    //   "F,frame,estimator,keyframe_valid,status,n_keyframe,n_cloud,n_margin,stamp of frame WINDOW_SIZE - 2"
    //   "P,vio_T_w_i (3),vio_R_w_i (9, row-major)"       17 digits
    //   "k,id,point_3d (3),uv (2),norm (2)"              per stored keyframe row; floats with 9 digits (they are float32)
    //   "c,x,y,z" per point of the cloud, "m,x,y,z" per point of the margin cloud
    const char* po_env = getenv("VINS_REPLAY_OUTPUTS");
    const int pub_points = po_env ? atoi(po_env) : 0;
    if (pub_points) resp->usePublishedOutputs(pub_points);
    std::vector<std::vector<double>> stamps0(N);
    for (int i = 0; i < N; ++i) {
        // the estimator as the reference's code would hold it between two frames, then handed over
        Estimator est;
        double ex[7], bias[6], last[6];
        rd.d(ex, 7); rd.d(bias, 6);
        est.tic[0] = Vector3d(ex[0], ex[1], ex[2]);
        est.ric[0] = Quaterniond(ex[6], ex[3], ex[4], ex[5]).toRotationMatrix();
        for (int k = 0; k < K; ++k) {
            FrameInit fr;
            rd.d(&fr.t, 1); rd.d(fr.pose, 7); rd.d(fr.sb, 9);
            set_frame(est, k, fr);
            stamps0[i].push_back(fr.t);
        }
        for (int k = 0; k + 2 < K; ++k) est.pre_integrations[k + 1] = preintegrate(h, rd, S, bias, noise);
        rd.d(last, 6);
        int L;
        rd.i(&L, 1);
        for (int l = 0; l < L; ++l) {
            int meta[3];
            double depth;
            rd.i(meta, 3); rd.d(&depth, 1);
            FeaturePerId f;
            f.feature_id = meta[0]; f.start_frame = meta[1]; f.estimated_depth = depth;
            for (int k = 0; k < meta[2]; ++k) {
                double r[8];
                rd.d(r, 8);
                FeaturePerFrame fr;
                fr.point = Vector3d(r[0], r[1], r[2]); fr.uv.x() = r[3]; fr.uv.y() = r[4]; fr.velocity.x() = r[5]; fr.velocity.y() = r[6]; fr.cur_td = r[7];
                f.feature_per_frame.push_back(fr);
            }
            est.f_manager.feature.push_back(f);
        }
        if (frames) {
            // the window's tracks from the front end: frame k of the window = image k (what addFeatureCheckParallax would have
            // collected, feature_manager.cpp:45-73, before the first solve of this replay)
            if (N != 1 || L != 0) { fprintf(stderr, "vio: window.bin must hold one estimator without tracks\n"); return 2; }
            std::map<int, FeaturePerId*> at;            // list nodes stay where they are
            for (int k = 0; k < WINDOW_SIZE; ++k) {
                const ResidentEstimators::Image image = fe.next();
                for (const auto& id_pts : image) {
                    auto it = at.find(id_pts.first);
                    if (it == at.end()) {
                        FeaturePerId f;
                        f.feature_id = id_pts.first; f.start_frame = k; f.estimated_depth = -1.0;
                        est.f_manager.feature.push_back(f);
                        it = at.emplace(id_pts.first, &est.f_manager.feature.back()).first;
                    }
                    const Eigen::Matrix<double, 7, 1>& r = id_pts.second[0].second;
                    FeaturePerFrame fr;
                    fr.point = Vector3d(r(0, 0), r(1, 0), r(2, 0)); fr.uv.x() = r(3, 0); fr.uv.y() = r(4, 0);
                    fr.velocity.x() = r(5, 0); fr.velocity.y() = r(6, 0); fr.cur_td = 0.0;
                    it->second->feature_per_frame.push_back(fr);
                }
            }
        }
        resp->handOver(i, est, Vector3d(last[0], last[1], last[2]), Vector3d(last[3], last[4], last[5]));
        for (int k = 0; k <= WINDOW_SIZE; ++k) (*resp)[i].Headers[k] = stamps0[i][k];
        for (int k = 0; k <= WINDOW_SIZE; ++k) { delete est.pre_integrations[k]; est.pre_integrations[k] = nullptr; }
    }
    resp->begin();
    FILE* orelo = relo.empty() ? nullptr : fopen((std::string(out) + ".relo").c_str(), "w");
    FILE* opub = pub_points ? fopen((std::string(out) + ".outputs").c_str(), "w") : nullptr;
    // VINS_REPLAY_KERNEL_TIMES=1 (with the IMU on the device): per frame "K,<frame>,<ms in ba_seq_imu_kernel>,<ms in ba_seq_merge_kernel>"
    // on stderr, from HIP events; asking for them waits for the merge, so such a run is not one to take host times from
    const bool kernel_times = device_imu && getenv("VINS_REPLAY_KERNEL_TIMES") != nullptr;
    if (kernel_times) resp->deviceImuTiming(true);
    FILE* o = fopen(out, "w");
    std::vector<double> smp((size_t)S * 7);
    double fe_ms = 0;
    for (int w = 0; w < W; ++w) {
        std::vector<double> stamp(N);
        double imu_ms = 0;
        for (ReloRec& q : relo)
            if (q.frame == w) q.found = resp->setReloFrame(q.est, q.stamp, 0, q.match, q.t, q.r);
        for (int i = 0; i < N; ++i) {
            rd.d(&stamp[i], 1);
            rd.d(smp.data(), S * 7);
            const auto t_imu = std::chrono::steady_clock::now();
            for (int s = 0; s < S; ++s)
                resp->processIMU(i, smp[7 * s], Vector3d(smp[7 * s + 1], smp[7 * s + 2], smp[7 * s + 3]), Vector3d(smp[7 * s + 4], smp[7 * s + 5], smp[7 * s + 6]));
            imu_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_imu).count();
            int n;
            rd.i(&n, 1);
            ResidentEstimators::Image image;
            for (int k = 0; k < n; ++k) {
                int id;
                double r[7];
                rd.i(&id, 1); rd.d(r, 7);
                Eigen::Matrix<double, 7, 1> p;
                for (int c = 0; c < 7; ++c) p(c, 0) = r[c];
                image[id].emplace_back(0, p);
            }
            if (frames) {
                const auto t0 = std::chrono::steady_clock::now();
                image = fe.next();
                fe_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            }
            resp->processImage(i, image, stamp[i]);
        }
        const auto t_solve = std::chrono::steady_clock::now();
        resp->solve();
        const double solve_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_solve).count();
        if (timing) fprintf(stderr, "T,%d,%.4f,%.4f\n", w, imu_ms, solve_ms);
        if (kernel_times) {
            float ik = 0, mk = 0;
            resp->deviceImuTimes(ik, mk);
            fprintf(stderr, "K,%d,%.5f,%.5f\n", w, ik, mk);
        }
        for (int i = 0; i < N; ++i) {
            // (the mirror is post-slide: the frame just solved sits in slot WINDOW_SIZE either way)
            const ResidentEstimators::One& e = (*resp)[i];
            const Quaterniond q(e.Rs[WINDOW_SIZE]);
            fprintf(o, "%d,%.0f,%.9f,%.9f,%.9f,%.9f,%.9f,%.9f,%.9f,%.9f,%.9f,%.9f,%d,%d,%d,%d\n", i, stamp[i] * 1e9, e.Ps[WINDOW_SIZE].x(), e.Ps[WINDOW_SIZE].y(),
                    e.Ps[WINDOW_SIZE].z(), q.w(), q.x(), q.y(), q.z(), e.Vs[WINDOW_SIZE].x(), e.Vs[WINDOW_SIZE].y(), e.Vs[WINDOW_SIZE].z(),
                    (int)e.marginalization_flag, e.n_features, e.status, e.failure_occur ? 1 : 0);
            if (frames) fprintf(o, "t,%d,%.3f,%.3f\n", i, fe_ms, solve_ms);      // vio: wall time of readImage / of processImage's solve, ms
        }
        for (const ReloRec& q : relo) {
            if (q.frame != w) continue;
            const ResidentEstimators::One& e = (*resp)[q.est];
            fprintf(orelo, "%d,%d,%d,%d,%d", w, q.est, q.found ? 1 : 0, q.found ? e.relo_n_factors : 0, q.found ? e.relo_frame_local_index : -1);
            for (int k = 0; k < 7; ++k) fprintf(orelo, ",%.12g", e.relo_Pose[k]);
            fprintf(orelo, ",%.12g,%.12g,%.12g", e.relo_relative_t.x(), e.relo_relative_t.y(), e.relo_relative_t.z());
            fprintf(orelo, ",%.12g,%.12g,%.12g,%.12g,%.12g", e.relo_relative_q.x(), e.relo_relative_q.y(), e.relo_relative_q.z(), e.relo_relative_q.w(), e.relo_relative_yaw);
            for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) fprintf(orelo, ",%.12g", e.drift_correct_r(a, b));
            fprintf(orelo, ",%.12g,%.12g,%.12g\n", e.drift_correct_t.x(), e.drift_correct_t.y(), e.drift_correct_t.z());
        }
        for (int i = 0; i < N && opub; ++i) {
            const ResidentEstimators::Keyframe& kf = resp->keyframe(i);
            const ResidentEstimators::Cloud& pc = resp->pointCloud(i);
            const ResidentEstimators::Cloud& mg = resp->marginCloud(i);
            fprintf(opub, "F,%d,%d,%d,%d,%d,%d,%d,%.17g\n", w, i, kf.valid ? 1 : 0, kf.status, kf.count, pc.count, mg.count, kf.stamp);
            fprintf(opub, "P,%.17g,%.17g,%.17g", kf.vio_T_w_i.x(), kf.vio_T_w_i.y(), kf.vio_T_w_i.z());
            for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) fprintf(opub, ",%.17g", kf.vio_R_w_i(a, b));
            fprintf(opub, "\n");
            for (size_t k = 0; k < kf.point_id.size(); ++k)
                fprintf(opub, "k,%d,%.9g,%.9g,%.9g,%.9g,%.9g,%.9g,%.9g\n", (int)kf.point_id[k], kf.point_3d[3 * k], kf.point_3d[3 * k + 1], kf.point_3d[3 * k + 2],
                        kf.point_2d_uv[2 * k], kf.point_2d_uv[2 * k + 1], kf.point_2d_norm[2 * k], kf.point_2d_norm[2 * k + 1]);
            for (size_t k = 0; k + 2 < pc.xyz.size(); k += 3) fprintf(opub, "c,%.9g,%.9g,%.9g\n", pc.xyz[k], pc.xyz[k + 1], pc.xyz[k + 2]);
            for (size_t k = 0; k + 2 < mg.xyz.size(); k += 3) fprintf(opub, "m,%.9g,%.9g,%.9g\n", mg.xyz[k], mg.xyz[k + 1], mg.xyz[k + 2]);
        }
        if (w == handback_frame) {
            std::unique_ptr<ResidentEstimators> next(new ResidentEstimators(N, 512, 512));
            if (device_imu) next->useDeviceImu();
            if (pub_points) next->usePublishedOutputs(pub_points);
            if (!relo.empty()) { int mm = 1; for (const ReloRec& q : relo) mm = std::max(mm, (int)q.match.size()); next->useRelocalisation(mm); }
            std::vector<std::unique_ptr<Estimator>> back;
            for (int i = 0; i < N; ++i) {
                back.emplace_back(new Estimator());
                resp->handBack(i, *back[i]);
                next->handOver(i, *back[i], (*resp)[i].acc_0, (*resp)[i].gyr_0);
                for (int k = 0; k <= WINDOW_SIZE; ++k) (*next)[i].Headers[k] = (*resp)[i].Headers[k];
            }
            next->begin();
            next->reseed(0, *back[0], (*resp)[0].acc_0, (*resp)[0].gyr_0);
            for (auto& e : back)
                for (int k = 0; k <= WINDOW_SIZE; ++k) { delete e->pre_integrations[k]; e->pre_integrations[k] = nullptr; }
            resp = std::move(next);
            if (kernel_times) resp->deviceImuTiming(true);
        }
    }
    // which side ran processIMU, and (device) how far the resident acc_0 / gyr_0 are from the last sample the host handed on
    fprintf(stderr, "M,%s\n", resp->deviceImu() ? "device" : "host");
    if (resp->deviceImu())
        for (int i = 0; i < N; ++i) {
            double s[9];
            resp->residentMeasurement(i, s);
            const ResidentEstimators::One& e = (*resp)[i];
            const double m[6] = {e.acc_0.x(), e.acc_0.y(), e.acc_0.z(), e.gyr_0.x(), e.gyr_0.y(), e.gyr_0.z()};
            double worst = 0;
            for (int k = 0; k < 6; ++k) worst = std::max(worst, std::fabs(s[k] - m[k]));
            fprintf(stderr, "A,%d,%.3g\n", i, worst);
        }
    fclose(o);
    if (orelo) fclose(orelo);
    if (opub) fclose(opub);
    fclose(rd.f);
    vg_destroy(h);
    return 0;
}

// vins_replay kfpnp <in.bin> <out.txt>: KeyFrame::PnPRANSAC and the second half of KeyFrame::findConnection (host/keyframe.h,
// vg_pack_kf_pnp) over a KPN1 file (tests/kf_pnp_ref.write_file: the lists findConnection holds behind its first reduceVector round).
// The file's min_loop_num must be KeyFrame::MIN_LOOP_NUM and its other gates the defaults, which is what the class passes.  Writes
// "pnp <VG_KF_PNP_*> <inliers>", "status" with the mask, "R" nine and "T" three numbers of PnPRANSAC (17 digits); then of findConnection
// "connection <return value> <VG_KF_PNP_*> <has_loop> <loop_index> <survivors>", "loop_info" with eight numbers, "taps" (best, last
// iteration, bound, refit iterations and raises), "pose" (rvec, tvec), an "m <id> <x> <y>" line per entry of match_points and "tq" with its eight numbers.
static int replay_kfpnp(const char* in, const char* out) {
    Reader rd{fopen(in, "rb")};
    if (!rd.f) { perror("kfpnp file"); return 2; }
    int hdr[5];
    double d[27];
    rd.i(hdr, 5); rd.d(d, 27);
    if (hdr[0] != 0x314E504B) { fprintf(stderr, "not a KPN1 file\n"); return 2; }
    const int n = hdr[1];
    if (n < 0 || hdr[2] != KeyFrame::MIN_LOOP_NUM || hdr[3] != 100) { fprintf(stderr, "the class runs MIN_LOOP_NUM %d and 100 iterations\n", (int)KeyFrame::MIN_LOOP_NUM); return 2; }
    std::vector<cv::Point3f> p3((size_t)n);
    std::vector<cv::Point2f> p2((size_t)n);
    std::vector<int> ids((size_t)n);
    if (n && (fread(p3.data(), sizeof(cv::Point3f), n, rd.f) != (size_t)n || fread(p2.data(), sizeof(cv::Point2f), n, rd.f) != (size_t)n))
        throw std::runtime_error("kfpnp file truncated");
    rd.i(ids.data(), n);
    fclose(rd.f);
    vg_handle* h = nullptr;
    if (vg_create(&h) != VG_OK) { fprintf(stderr, "vg_create failed\n"); return 1; }
    FILE* o = fopen(out, "w");
    if (!o) { perror("out"); return 2; }
    {
        Vector3d T(d[3], d[4], d[5]), tic(d[15], d[16], d[17]);
        Matrix3d R, qic;
        for (int e = 0; e < 9; ++e) { R(e / 3, e % 3) = d[6 + e]; qic(e / 3, e % 3) = d[18 + e]; }
        std::vector<double> pid(ids.begin(), ids.end());
        KeyFrame cur(h, 1.5, 7, T, R, p3, pid), old_kf(h, 0.5, 3, Vector3d(0.1, 0.2, 0.3), Matrix3d(), std::vector<cv::Point3f>(), std::vector<double>());
        cur.tic = tic; cur.qic = qic; cur.pnp_refine = hdr[4];
        std::vector<uchar> status;
        Vector3d PT;
        Matrix3d PR;
        if (n >= 6) {
            cur.PnPRANSAC(p2, p3, status, PT, PR);
            fprintf(o, "pnp %d %d\nstatus", cur.pnp_status, cur.pout.n_inliers);
            for (uchar s : status) fprintf(o, " %d", (int)s);
            fprintf(o, "\nR");
            for (int e = 0; e < 9; ++e) fprintf(o, " %.17g", PR(e / 3, e % 3));
            fprintf(o, "\nT %.17g %.17g %.17g\n", PT.x(), PT.y(), PT.z());
        }
        std::vector<cv::Point2f> m2 = p2;
        std::vector<cv::Point3f> m3 = p3;
        std::vector<double> mid = pid;
        const bool ok = cur.findConnection(&old_kf, m2, m3, mid);
        fprintf(o, "connection %d %d %d %d %d\nloop_info", ok ? 1 : 0, cur.pnp_status, cur.has_loop ? 1 : 0, cur.loop_index, (int)m3.size());
        for (int k = 0; k < 8; ++k) fprintf(o, " %.17g", cur.has_loop ? cur.loop_info(k, 0) : 0.0);
        const vg_kf_pnp_out& q = cur.pout;
        fprintf(o, "\ntaps %d %d %d %d %d\n", q.ransac_best, q.ransac_iter, q.ransac_bound, q.refit_iters, q.refit_up);
        fprintf(o, "pose %.17g %.17g %.17g %.17g %.17g %.17g\n", q.rvec[0], q.rvec[1], q.rvec[2], q.tvec[0], q.tvec[1], q.tvec[2]);
        for (size_t k = 0; k < cur.match_points.match_id.size(); ++k)
            fprintf(o, "m %d %.17g %.17g\n", cur.match_points.match_id[k], cur.match_points.match_xy[2 * k], cur.match_points.match_xy[2 * k + 1]);
        fprintf(o, "tq");
        for (int k = 0; k < 8; ++k) fprintf(o, " %.17g", cur.match_points.t_q_index[k]);
        fprintf(o, "\n");
    }
    fclose(o);
    vg_destroy(h);
    return 0;
}

// vins_replay bow <voc.bin> <frames.bin> <out.txt>: BriefVocabulary, PoseGraph::loadVocabulary and PoseGraph::detectLoop (host/pose_graph.h,
// vg_pack_bow) over a BOW1 file (tests/kf_bow_ref.write_frames: int32 'BOW1', n_frames, the first frame_index; per frame n and n x 4
// 64-bit words).  Every frame becomes a KeyFrame of stored descriptors in slot 0 and goes through detectLoop on one database.  A line per
// frame: frame_index, the return value, find_loop, the entry id, n_words, n_results, then id:score (the double's bits, hexadecimal) each.
static int replay_bow(const char* voc_path, const char* in, const char* out) {
    Reader rd{fopen(in, "rb")};
    if (!rd.f) { perror("bow file"); return 2; }
    int hdr[3];
    rd.i(hdr, 3);
    if (hdr[0] != 0x31574F42 || hdr[1] < 0) { fprintf(stderr, "not a BOW1 file\n"); return 2; }
    std::vector<std::vector<BRIEF::bitset>> frames((size_t)hdr[1]);
    size_t most = 1, total = 1;
    for (auto& fr : frames) {
        int n = 0;
        rd.i(&n, 1);
        if (n < 0) throw std::runtime_error("bow file: a negative count");
        fr.resize((size_t)n);
        if (n && fread(fr.data(), sizeof(BRIEF::bitset), n, rd.f) != (size_t)n) throw std::runtime_error("bow file truncated");
        most = std::max(most, (size_t)n); total += (size_t)n;
    }
    fclose(rd.f);
    vg_handle* h = nullptr;
    if (vg_create(&h) != VG_OK) { fprintf(stderr, "vg_create failed\n"); return 1; }
    FILE* o = fopen(out, "w");
    if (!o) { perror("out"); return 2; }
    int rc = 0;
    try {
        int16_t pattern[1024] = {0};
        if (vg_kf_configure(h, 64, 64, (int)most, 1, 1, pattern) != VG_OK) throw std::runtime_error(vg_last_error(h));
        PoseGraph pg(h, 0);
        pg.loadVocabulary(voc_path);
        PoseGraph::configure(h, 1, (int)frames.size() + 1, (int)total);
        for (size_t i = 0; i < frames.size(); ++i) {
            const std::vector<cv::KeyPoint> kp(frames[i].size());
            KeyFrame kf(h, 0, 0.05 * (double)i, hdr[2] + (int)i, kp, kp, frames[i]);
            const int loop = pg.detectLoop(&kf, kf.index);
            const vg_bow_out& q = pg.last;
            fprintf(o, "%d %d %d %d %d %d", kf.index, loop, q.find_loop, q.entry_id, q.n_words, q.n_results);
            for (int k = 0; k < q.n_results; ++k) {
                unsigned long long u;
                memcpy(&u, &q.scores[k], 8);
                fprintf(o, " %d:%016llx", q.ids[k], u);
            }
            fprintf(o, "\n");
        }
    } catch (const std::exception& e) { fprintf(stderr, "vins_replay bow: %s\n", e.what()); rc = 1; }
    fclose(o);
    vg_destroy(h);
    return rc;
}

// The graph file of tests/kf_pgo_ref.write_file: int32 n_kf n_opt first_looped_index max_iters, float64 huber_delta, the tables.  The
// class runs the reference's 5 iterations and HuberLoss(0.1).
static int replay_pgo(const char* in, const char* out) {
    Reader rd{fopen(in, "rb")};
    if (!rd.f) { perror("pgo file"); return 2; }
    int hdr[4];
    double delta;
    rd.i(hdr, 4); rd.d(&delta, 1);
    const int n = hdr[0];
    if (n < 1 || hdr[3] != 5 || delta != 0.1) { fprintf(stderr, "the class runs 5 iterations and HuberLoss(0.1)\n"); return 2; }
    std::vector<int> index(n), sequence(n), has_loop(n), loop_index(n);
    std::vector<double> T(3 * (size_t)n), R(9 * (size_t)n), info(8 * (size_t)n);
    rd.i(index.data(), n); rd.i(sequence.data(), n); rd.i(has_loop.data(), n); rd.i(loop_index.data(), n);
    rd.d(T.data(), 3 * n); rd.d(R.data(), 9 * n); rd.d(info.data(), 8 * n);
    fclose(rd.f);
    vg_handle* h = nullptr;
    if (vg_create(&h) != VG_OK) { fprintf(stderr, "vg_create failed\n"); return 1; }
    FILE* o = fopen(out, "w");
    if (!o) { perror("out"); return 2; }
    {
        PoseGraph pg(h, 0);
        pg.earliest_loop_index = hdr[2];                        // (an earlier pass found it: the file holds the slice from there on)
        std::vector<std::unique_ptr<KeyFrame>> kfs;
        for (int i = 0; i < n; ++i) {
            Vector3d t(T[3 * i], T[3 * i + 1], T[3 * i + 2]);
            Matrix3d r;
            for (int e = 0; e < 9; ++e) r(e / 3, e % 3) = R[9 * (size_t)i + e];
            kfs.emplace_back(new KeyFrame(h, 0.1 * i, index[i], t, r, std::vector<cv::Point3f>(), std::vector<double>()));
            KeyFrame* kf = kfs.back().get();
            kf->sequence = sequence[i];
            pg.global_index = index[i];                         // (the file's indices need not be consecutive)
            pg.shiftToBase(kf);
            if (has_loop[i] && i < hdr[1]) {
                KeyFrame* old_kf = pg.getKeyFrame(loop_index[i]);
                if (!old_kf) throw std::runtime_error("pgo file: a loop_index that is not an earlier keyframe");
                kf->has_loop = true; kf->loop_index = loop_index[i];
                for (int k = 0; k < 8; ++k) kf->loop_info(k, 0) = info[8 * (size_t)i + k];
                pg.addLoop(kf, old_kf);
            }
            pg.appendKeyFrame(kf);
        }
        const bool ran = pg.optimize4DoF();
        const vg_pg_out& q = pg.pg;
        fprintf(o, "pass %d %d %d %d %d %d %d\n", ran ? 1 : 0, q.status, q.termination, q.iterations, q.n_edges, q.n_loop_edges, q.n_free);
        fprintf(o, "cost %.17g %.17g\ndrift %.17g", q.initial_cost, q.final_cost, pg.yaw_drift);
        for (int e = 0; e < 9; ++e) fprintf(o, " %.17g", pg.r_drift(e / 3, e % 3));
        fprintf(o, " %.17g %.17g %.17g\n", pg.t_drift.x(), pg.t_drift.y(), pg.t_drift.z());
        for (KeyFrame* kf : pg.keyframelist) {
            Vector3d t;
            Matrix3d r;
            kf->getPose(t, r);
            fprintf(o, "kf %d %d %.17g %.17g %.17g", kf->index, kf->local_index, t.x(), t.y(), t.z());
            for (int e = 0; e < 9; ++e) fprintf(o, " %.17g", r(e / 3, e % 3));
            fprintf(o, "\n");
        }
    }
    fclose(o);
    vg_destroy(h);
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 4 && !strcmp(argv[1], "pgo")) {
        try { return replay_pgo(argv[2], argv[3]); }
        catch (const std::exception& e) { fprintf(stderr, "vins_replay pgo: %s\n", e.what()); return 1; }
    }
    if (argc >= 5 && !strcmp(argv[1], "bow")) {
        try { return replay_bow(argv[2], argv[3], argv[4]); }
        catch (const std::exception& e) { fprintf(stderr, "vins_replay bow: %s\n", e.what()); return 1; }
    }
    if (argc >= 4 && !strcmp(argv[1], "kfpnp")) {
        try { return replay_kfpnp(argv[2], argv[3]); }
        catch (const std::exception& e) { fprintf(stderr, "vins_replay kfpnp: %s\n", e.what()); return 1; }
    }
    if (argc >= 4 && !strcmp(argv[1], "fe")) {
        try { return replay_fe(argv[2], argv[3], argc >= 5 ? argv[4] : nullptr); }
        catch (const std::exception& e) { fprintf(stderr, "vins_replay fe: %s\n", e.what()); return 1; }
    }
    if (argc >= 4 && !strcmp(argv[1], "fe_batch")) {
        try { return replay_fe_batch(argv[2], argv[3], argc >= 5 ? argv[4] : nullptr); }
        catch (const std::exception& e) { fprintf(stderr, "vins_replay fe_batch: %s\n", e.what()); return 1; }
    }
    if (argc >= 4 && !strcmp(argv[1], "ba")) {
        try { return replay_ba(argv[2], argv[3]); }
        catch (const std::exception& e) { fprintf(stderr, "vins_replay ba: %s\n", e.what()); return 1; }
    }
    if (argc >= 4 && !strcmp(argv[1], "seq")) {
        try { return replay_seq(argv[2], argv[3]); }
        catch (const std::exception& e) { fprintf(stderr, "vins_replay seq: %s\n", e.what()); return 1; }
    }
    if (argc >= 5 && !strcmp(argv[1], "vio")) {
        try { return replay_seq(argv[2], argv[4], argv[3]); }
        catch (const std::exception& e) { fprintf(stderr, "vins_replay vio: %s\n", e.what()); return 1; }
    }
    if (argc >= 4 && !strcmp(argv[1], "align")) {
        try { return replay_align(argv[2], argv[3]); }
        catch (const std::exception& e) { fprintf(stderr, "vins_replay align: %s\n", e.what()); return 1; }
    }
    if (argc >= 3 && !strcmp(argv[1], "kf_pattern")) {          // host only: the four lists BriefExtractor reads, one line each
        try {
            BriefExtractor extractor(argv[2]);
            for (int k = 0; k < 4; ++k) {
                for (int i = 0; i < 256; ++i) printf("%d%c", (int)extractor.pattern[k][i], i == 255 ? '\n' : ' ');
            }
            return 0;
        } catch (const std::exception& e) { fprintf(stderr, "vins_replay kf_pattern: %s\n", e.what()); return 1; }
    }
    if (argc >= 5 && !strcmp(argv[1], "kf")) {
        try { return replay_kf(argv[2], argv[3], argv[4]); }
        catch (const std::exception& e) { fprintf(stderr, "vins_replay kf: %s\n", e.what()); return 1; }
    }
    if (argc >= 4 && !strcmp(argv[1], "exrot")) {
        try { return replay_exrot(argv[2], argv[3]); }
        catch (const std::exception& e) { fprintf(stderr, "vins_replay exrot: %s\n", e.what()); return 1; }
    }
    if (argc >= 4 && !strcmp(argv[1], "relpose")) {
        try { return replay_relpose(argv[2], argv[3]); }
        catch (const std::exception& e) { fprintf(stderr, "vins_replay relpose: %s\n", e.what()); return 1; }
    }
    if (argc >= 4 && !strcmp(argv[1], "sfm")) {
        try { return replay_sfm(argv[2], argv[3]); }
        catch (const std::exception& e) { fprintf(stderr, "vins_replay sfm: %s\n", e.what()); return 1; }
    }
    fprintf(stderr, "usage: vins_replay fe <frames.bin> <out.txt> [config.yaml] | vins_replay fe_batch <list.txt> <out_prefix> [config.yaml] | vins_replay ba <sequence.bin> <out.csv> | vins_replay seq <frames.bin> <out.csv> | vins_replay vio <window.bin> <frames.bin> <out.csv> | vins_replay align <in.bin> <out.txt> | vins_replay sfm <in.bin> <out.txt> | vins_replay relpose <in.bin> <out.txt> | vins_replay exrot <in.bin> <out.txt> | vins_replay kf <in.bin> <out.txt> <brief_pattern.yml> | vins_replay kfpnp <in.bin> <out.txt> | vins_replay bow <voc.bin> <frames.bin> <out.txt> | vins_replay pgo <in.bin> <out.txt>\n");
    return 2;
}
