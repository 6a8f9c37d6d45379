// feature_tracker_readimage.cpp — THE drop-in for the front end: four member functions of the REFERENCE'S `class FeatureTracker`
// (feature_tracker/src/feature_tracker.h:28-65), on the MI355X path:
//     void FeatureTracker::readImage(const cv::Mat&, double)    feature_tracker.cpp:81-167
//     void FeatureTracker::setMask()                            feature_tracker.cpp:36-69
//     void FeatureTracker::rejectWithF()                        feature_tracker.cpp:169-202
//     void FeatureTracker::undistortedPoints()                  feature_tracker.cpp:258-306
//
// How it is used.  This file includes the reference's own "feature_tracker.h" — `camodocal::CameraPtr m_camera`, the cv::Mat
// members, `showUndistortion`, the globals of parameters.h all stay what they are — and defines exactly those four members.  In a
// catkin workspace: add this file, include/vinsgpu.h and host/vg_pack.h (the packers it shares with the project's own classes;
// header-only) to feature_tracker, link libvinsgpu.so, and remove the four definitions
// from feature_tracker.cpp (or weaken them:  objcopy --weaken-symbol=_ZN14FeatureTracker9readImageERKN2cv3MatEd
// --weaken-symbol=_ZN14FeatureTracker7setMaskEv --weaken-symbol=_ZN14FeatureTracker11rejectWithFEv
// --weaken-symbol=_ZN14FeatureTracker17undistortedPointsEv).  feature_tracker_node.cpp, parameters.cpp, addPoints / updateID /
// readIntrinsicParameter / showUndistortion / inBorder / reduceVector and all of camera_model stay the reference's.  Here (no
// OpenCV / ROS in the image) oracle/Makefile target `ref_fe` does precisely that against the header stand-ins of
// oracle/ref_stubs_fe and produces oracle/_ref/libvins_ref_fe_gpu.so; tests/test_fe_dropin_*.py drive the reference's
// img_callback() through it and through the all-reference build side by side.
//
// readImage() itself is ONE library call per frame, vg_fe_read_image (include/vinsgpu.h): frame and cur_pts go up in one block, the
// device runs :87-125 (CLAHE, pyramid, LK, border test, reduceVector) and, on a published frame, rejectWithF, setMask's walk, the
// detection, addPoints and the lifting of undistortedPoints without the host in between; the results come back in one block.  The one
// question a published frame still puts to the host is the ORDER of setMask's walk: the reference's std::sort by track_cnt (:48) is not
// stable, so the order among equal counts is whatever this translation unit's std::sort makes of the sequence -- the callback
// (vg_pack::order_callback, instantiated here) runs that very sort call and hands the permutation down.  A camera that is not a
// camodocal::PinholeCamera takes the step-by-step members (its lifting runs on the host).
//
// What the step-by-step bodies (setMask / rejectWithF / undistortedPoints as members, and readImage for other camera models) do instead
// of the reference's:
//   :87-93   cv::createCLAHE(3.0, Size(8,8))->apply          -> vg_fe_push_frames(.., EQUALIZE): upload + CLAHE + pyramid on the device
//   :113     cv::calcOpticalFlowPyrLK(cur_img, forw_img, ..)  -> vg_fe_track (the pyramid of cur_img is still on the device)
//   :149     cv::goodFeaturesToTrack(forw_img, .., mask)      -> vg_fe_detect_masked (the mask setMask() built stays on the device)
//   :191     cv::findFundamentalMat(.., FM_RANSAC, ..)        -> vg_fe_reject_with_f
//   :48-68   std::sort by track_cnt + mask walk + cv::circle  -> the SAME std::sort call on the host (the order among equal counts is
//                                                                whatever the platform's std::sort gives: the reference's too), then
//                                                                vg_fe_set_mask walks that order on the device
//   :262-267 m_camera->liftProjective per point               -> vg_fe_undistort for a camodocal::PinholeCamera (the EuRoC / default
//                                                                model); any other camera model lifts through m_camera on the host
// Differences a caller can see: `forw_img` / `cur_img` / `prev_img` refer to the image as it came in (the equalized image lives on
// the device: vg_fe_get_level(.., 0, ..) returns it) and `mask` is left empty (vg_fe_get_mask).  The node reads neither.
// State the reference class has no member for (the device handle) lives in a side table keyed by `this`.
#include <algorithm>
#include <cstring>
#include <mutex>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "feature_tracker.h"
#include "vinsgpu.h"
#include "vg_pack.h"

namespace {

struct FeSide {
    vg_handle* vg = nullptr;
    int capacity = 0, width = 0, height = 0;
    bool pinhole = false;          // m_camera is a camodocal::PinholeCamera: lifting runs on the device
    double intr[8];                // fx fy cx cy k1 k2 p1 p2
    const void* camera = nullptr;  // the camera object `intr` was read from
    std::vector<uint8_t> base_copy;   // the fisheye mask without row padding, when the cv::Mat has some
    int stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // vins_fe_gpu_stats
};
std::mutex g_mu;
std::unordered_map<const FeatureTracker*, FeSide> g_side;
FeSide& side_of(const FeatureTracker* t) {
    std::lock_guard<std::mutex> lock(g_mu);
    return g_side[t];
}
void chk(int rc, vg_handle* h, const char* what) {
    if (rc != VG_OK) throw std::runtime_error(std::string(what) + ": " + (h ? vg_last_error(h) : "no handle") + " (no CPU fallback)");
}
// the device side of one tracker: created at the first call, re-configured when the image size or MAX_CNT changes
FeSide& ensure(FeatureTracker* t, int w, int h) {
    FeSide& s = side_of(t);
    if (vg_abi_version() != VG_ABI_VERSION) throw std::runtime_error("libvinsgpu.so was built from another include/vinsgpu.h (ABI version mismatch)");
    if (!s.vg) chk(vg_create(&s.vg), s.vg, "vg_create");
    // vg_fe_read_image takes streams of up to 2048 points; a list never exceeds MAX_CNT (:144-156), the factor is slack.  MAX_CNT
    // beyond 2048 takes the step-by-step branch of readImage.
    const int cap = MAX_CNT <= 2048 ? std::min(std::max(MAX_CNT, 1) * 4, 2048) : MAX_CNT;
    if (s.capacity < cap || s.width != w || s.height != h) {
        chk(vg_fe_configure(s.vg, w, h, 1, cap), s.vg, "vg_fe_configure");
        s.capacity = cap; s.width = w; s.height = h;
    }
    if (s.camera != t->m_camera.get()) {
        s.camera = t->m_camera.get();
        camodocal::PinholeCameraPtr pin = boost::dynamic_pointer_cast<camodocal::PinholeCamera>(t->m_camera);
        s.pinhole = static_cast<bool>(pin);
        if (pin) {
            const camodocal::PinholeCamera::Parameters& p = pin->getParameters();
            const double v[8] = {p.fx(), p.fy(), p.cx(), p.cy(), p.k1(), p.k2(), p.p1(), p.p2()};
            std::memcpy(s.intr, v, sizeof(v));
        }
    }
    return s;
}

}  // namespace

void FeatureTracker::setMask() {                                      // feature_tracker.cpp:36-69
    FeSide& s = ensure(this, COL, ROW);
    // prefer to keep features that are tracked for long time (:43-51): the reference's own sort, verbatim semantics
    std::vector<float> xy;
    std::vector<int> cnt, kept((size_t)s.capacity, 0);
    vg_pack::OrderCtx<FeatureTracker>::SortedList cnt_pts_id;
    vg_pack::sorted_for_setmask(*this, s.capacity, xy, cnt, cnt_pts_id);
    const int n = (int)cnt_pts_id.size();
    // :38-41: the fisheye mask or all-255 is the canvas; the walk in sorted order (the device's own sort by count is stable, i.e. the
    // identity on an already sorted list) keeps a point iff the canvas is still 255 under it and blanks a disc of MIN_DIST around it
    std::vector<uint8_t> base;
    const uint8_t* basep[1] = {nullptr};
    if (FISHEYE) {
        if (fisheye_mask.rows != ROW || fisheye_mask.cols != COL) throw std::runtime_error("FeatureTracker::setMask: fisheye_mask is not ROW x COL");
        base.resize((size_t)ROW * COL);
        for (int y = 0; y < ROW; ++y) std::memcpy(base.data() + (size_t)y * COL, fisheye_mask.data + (size_t)y * fisheye_mask.step, (size_t)COL);
        basep[0] = base.data();
    }
    int nk = 0;
    chk(vg_fe_set_mask(s.vg, xy.data(), cnt.data(), &n, basep, MIN_DIST, kept.data(), &nk), s.vg, "vg_fe_set_mask");
    vg_pack::take_setmask_result(*this, cnt_pts_id, kept.data(), nk);
}

namespace {
void undistorted_points(FeatureTracker* t, FeSide& s, const float* lifted);
}  // namespace

void FeatureTracker::readImage(const cv::Mat& _img, double _cur_time) {     // feature_tracker.cpp:81-167
    cur_time = _cur_time;
    // the reference assumes the configured size (COL / ROW: setMask, inBorder, the fisheye mask); a frame of another size would make
    // this member and the other three re-configure the device side against each other every frame -- tracking would degrade silently
    if (_img.cols != COL || _img.rows != ROW)
        throw std::runtime_error("FeatureTracker::readImage: frame is " + std::to_string(_img.cols) + "x" + std::to_string(_img.rows) +
                                 ", the configuration says " + std::to_string(COL) + "x" + std::to_string(ROW));
    FeSide& s = ensure(this, COL, ROW);
    const float* lifted = nullptr;
    if (s.pinhole && s.capacity <= 2048) {
        // ---- one call per frame
        vg_fe_frame_in in;
        vg_pack::fill_frame_in(*this, _img, PUB_THIS_FRAME, EQUALIZE, MAX_CNT, MIN_DIST, F_THRESHOLD, FOCAL_LENGTH, in);
        std::memcpy(in.intr, s.intr, sizeof(in.intr));
        if (FISHEYE && PUB_THIS_FRAME) {                                     // :38-41: the fisheye mask is setMask's canvas
            if (fisheye_mask.rows != ROW || fisheye_mask.cols != COL) throw std::runtime_error("FeatureTracker::readImage: fisheye_mask is not ROW x COL");
            if ((int)fisheye_mask.step == COL)
                in.base_mask = fisheye_mask.data;
            else {
                s.base_copy.resize((size_t)ROW * COL);
                for (int y = 0; y < ROW; ++y) std::memcpy(s.base_copy.data() + (size_t)y * COL, fisheye_mask.data + (size_t)y * fisheye_mask.step, (size_t)COL);
                in.base_mask = s.base_copy.data();
            }
        }
        vg_pack::OrderCtx<FeatureTracker> ctx{this, in.n, {}};
        in.order = vg_pack::order_callback<FeatureTracker>; in.user = &ctx;
        if (in.n > s.capacity) throw std::runtime_error("FeatureTracker::readImage: more points than the configured capacity");
        vg_fe_frame_out out;
        chk(vg_fe_read_image(s.vg, &in, &out), s.vg, "vg_fe_read_image");
        s.stats[0]++; s.stats[1] += in.publish; s.stats[2] += out.ransac_ran; s.stats[3] += (out.fallback & 1) ? 1 : 0;
        s.stats[4] += (out.fallback & 2) ? 1 : 0; s.stats[5] += out.ransac_niters;
        if (forw_img.empty())
            prev_img = cur_img = forw_img = _img;
        else
            forw_img = _img;
        vg_pack::apply_statuses(*this, out, in.n);                           // only now: the call returned VG_OK
        if (PUB_THIS_FRAME) vg_pack::apply_published(*this, out, ctx.sorted);   // (its addPoints() is the reference's, :71-79)
        if ((int)forw_pts.size() != out.n_final) throw std::runtime_error("FeatureTracker::readImage: list length differs from the device's");
        lifted = out.un_xy;
    } else {
        // ---- step by step (camera models whose lifting runs through camodocal on the host)
        s.stats[6]++;
        // EQUALIZE (:85-95) and `forw_img = img` (:97-104): the frame goes to the device, where the (optional) CLAHE and the pyramid
        // that calcOpticalFlowPyrLK would build of it are formed; the previous frame's pyramid stays where it is
        const uint8_t* planes[1] = {_img.data};
        chk(vg_fe_push_frames(s.vg, planes, (int)_img.step, EQUALIZE), s.vg, "vg_fe_push_frames");
        if (forw_img.empty())
            prev_img = cur_img = forw_img = _img;
        else
            forw_img = _img;

        forw_pts.clear();

        if (cur_pts.size() > 0) {                                            // :108-125
            vector<uchar> status(cur_pts.size());
            vector<float> err(cur_pts.size());
            forw_pts.resize(cur_pts.size());
            chk(vg_fe_track(s.vg, 0, &cur_pts[0].x, (int)cur_pts.size(), &forw_pts[0].x, status.data(), err.data()), s.vg, "vg_fe_track");
            for (int i = 0; i < int(forw_pts.size()); i++)
                if (status[i] && !inBorder(forw_pts[i])) status[i] = 0;
            reduceVector(prev_pts, status);
            reduceVector(cur_pts, status);
            reduceVector(forw_pts, status);
            reduceVector(ids, status);
            reduceVector(cur_un_pts, status);
            reduceVector(track_cnt, status);
        }

        for (auto& n : track_cnt) n++;                                       // :127-128

        if (PUB_THIS_FRAME) {                                                // :130-158
            rejectWithF();
            setMask();
            int n_max_cnt = MAX_CNT - static_cast<int>(forw_pts.size());
            if (n_max_cnt > 0) {
                n_pts.resize(n_max_cnt);
                int n = 0;
                chk(vg_fe_detect_masked(s.vg, 0, n_max_cnt, 0.01, (double)MIN_DIST, &n_pts[0].x, &n), s.vg, "vg_fe_detect_masked");
                n_pts.resize(n);
            } else
                n_pts.clear();
            addPoints();                                                     // the reference's (:71-79)
        }
    }
    prev_img = cur_img;                                                      // :160-166
    prev_pts = cur_pts;
    prev_un_pts = cur_un_pts;
    cur_img = forw_img;
    cur_pts = forw_pts;
    undistorted_points(this, s, lifted);
    prev_time = cur_time;
}

void FeatureTracker::rejectWithF() {                                        // feature_tracker.cpp:169-202
    if (forw_pts.size() >= 8) {
        FeSide& s = ensure(this, COL, ROW);
        // :175-188 as the reference has it: 2 x <= 150 points through camodocal on the host, in double (the float pair handed to the
        // RANSAC is rounded from FOCAL_LENGTH * x / z + COL / 2)
        vector<cv::Point2f> un_cur_pts(cur_pts.size()), un_forw_pts(forw_pts.size());
        for (unsigned int i = 0; i < cur_pts.size(); i++) {
            Eigen::Vector3d tmp_p;
            m_camera->liftProjective(Eigen::Vector2d(cur_pts[i].x, cur_pts[i].y), tmp_p);
            tmp_p.x() = FOCAL_LENGTH * tmp_p.x() / tmp_p.z() + COL / 2.0;
            tmp_p.y() = FOCAL_LENGTH * tmp_p.y() / tmp_p.z() + ROW / 2.0;
            un_cur_pts[i] = cv::Point2f(tmp_p.x(), tmp_p.y());

            m_camera->liftProjective(Eigen::Vector2d(forw_pts[i].x, forw_pts[i].y), tmp_p);
            tmp_p.x() = FOCAL_LENGTH * tmp_p.x() / tmp_p.z() + COL / 2.0;
            tmp_p.y() = FOCAL_LENGTH * tmp_p.y() / tmp_p.z() + ROW / 2.0;
            un_forw_pts[i] = cv::Point2f(tmp_p.x(), tmp_p.y());
        }
        const int n = (int)forw_pts.size();
        vector<uchar> status(n);
        chk(vg_fe_reject_with_f(s.vg, &un_cur_pts[0].x, &un_forw_pts[0].x, n, F_THRESHOLD, status.data(), nullptr, nullptr), s.vg, "vg_fe_reject_with_f");
        reduceVector(prev_pts, status);
        reduceVector(cur_pts, status);
        reduceVector(forw_pts, status);
        reduceVector(cur_un_pts, status);
        reduceVector(ids, status);
        reduceVector(track_cnt, status);
    }
}

namespace {
// undistortedPoints() (feature_tracker.cpp:258-306); `lifted` = the (x / z, y / z) pairs of cur_pts when the device already formed them
void undistorted_points(FeatureTracker* t, FeSide& s, const float* lifted) {
    const vector<cv::Point2f>& cur_pts = t->cur_pts;
    const int n = (int)cur_pts.size();
    std::vector<float> un_own;
    const float* un = lifted;
    if (!un) {
        un_own.resize((size_t)std::max(n, 1) * 2);
        if (n > 0 && s.pinhole)
            chk(vg_fe_undistort(s.vg, &cur_pts[0].x, n, s.intr, un_own.data()), s.vg, "vg_fe_undistort");
        else
            for (int i = 0; i < n; i++) {                                    // MEI / KANNALA_BRANDT / SCARAMUZZA: camodocal on the host (:262-266)
                Eigen::Vector2d a(cur_pts[i].x, cur_pts[i].y);
                Eigen::Vector3d b;
                t->m_camera->liftProjective(a, b);
                un_own[2 * i] = (float)(b.x() / b.z());
                un_own[2 * i + 1] = (float)(b.y() / b.z());
            }
        un = un_own.data();
    }
    vg_pack::lifted_points(*t, un);                                          // cur_un_pts, the map, the velocities (:267-304)
}
}  // namespace

void FeatureTracker::undistortedPoints() { undistorted_points(this, ensure(this, COL, ROW), nullptr); }

// ---- C entry points for the surrounding code (the reference class has no member to hang these on)
extern "C" {
// release the device handle of a FeatureTracker that is about to be destroyed or re-used for another stream
void vins_fe_gpu_release(FeatureTracker* t) {
    std::lock_guard<std::mutex> lock(g_mu);
    auto it = g_side.find(t);
    if (it == g_side.end()) return;
    if (it->second.vg) vg_destroy(it->second.vg);
    g_side.erase(it);
}
// how the frames of this tracker ran: [0] frames through vg_fe_read_image, [1] of them published, [2] with rejectWithF, [3] / [4] whose
// estimate went back to the host (a RANSAC sample OpenCV would have redrawn / the LMedS range), [5] sum of the RANSAC iterations that
// counted, [6] frames through the step-by-step members
void vins_fe_gpu_stats(FeatureTracker* t, int* out8) { std::memcpy(out8, side_of(t).stats, sizeof(int) * 8); }
// the device handle (e.g. for vg_fe_get_mask / vg_fe_get_level: the members `mask` and the equalized `cur_img` stay on the device)
vg_handle* vins_fe_gpu_handle(FeatureTracker* t) { return side_of(t).vg; }
}
