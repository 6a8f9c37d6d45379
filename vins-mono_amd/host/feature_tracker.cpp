// feature_tracker.cpp — see feature_tracker.h.  Control flow follows feature_tracker/src/feature_tracker.cpp of the
// reference (cited per block); the arithmetic runs on the GPU through libvinsgpu.so.
#include "feature_tracker.h"
#include "vg_pack.h"
#include <cstring>
#include "yaml_config.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <stdexcept>

int ROW = 480, COL = 752, MAX_CNT = 150, MIN_DIST = 30, EQUALIZE = 1, FISHEYE = 0, FOCAL_LENGTH = 460;
bool PUB_THIS_FRAME = false;
double F_THRESHOLD = 1.0;
int FREQ = 10, SHOW_TRACK = 1, FE_WINDOW_SIZE = 20;
std::string IMAGE_TOPIC, FE_IMU_TOPIC, FISHEYE_MASK;

void readFeatureTrackerParameters(const std::string& config_file, const std::string& vins_folder) {   // feature_tracker/src/parameters.cpp:37-74
    VinsYaml fs;
    if (!fs.load(config_file)) throw std::runtime_error("ERROR: Wrong path to settings: " + config_file);
    IMAGE_TOPIC = fs.str("image_topic");
    FE_IMU_TOPIC = fs.str("imu_topic");
    MAX_CNT = (int)fs.number("max_cnt");
    MIN_DIST = (int)fs.number("min_dist");
    ROW = (int)fs.number("image_height");
    COL = (int)fs.number("image_width");
    FREQ = (int)fs.number("freq");
    F_THRESHOLD = fs.number("F_threshold");
    SHOW_TRACK = (int)fs.number("show_track");
    EQUALIZE = (int)fs.number("equalize");
    FISHEYE = (int)fs.number("fisheye");
    if (FISHEYE == 1) FISHEYE_MASK = vins_folder + "config/fisheye_mask.jpg";
    FE_WINDOW_SIZE = 20;
    FOCAL_LENGTH = 460;
    PUB_THIS_FRAME = false;
    if (FREQ == 0) FREQ = 100;
}
int FeatureTracker::n_id = 0;

static int cvRoundf(float v) { return (int)std::lrintf(v); }

bool inBorder(const cv::Point2f& pt) {                       // feature_tracker.cpp:5-11
    const int BORDER_SIZE = 1;
    int img_x = cvRoundf(pt.x);
    int img_y = cvRoundf(pt.y);
    return BORDER_SIZE <= img_x && img_x < COL - BORDER_SIZE && BORDER_SIZE <= img_y && img_y < ROW - BORDER_SIZE;
}

void reduceVector(vector<cv::Point2f>& v, vector<uchar> status) {   // :13-20
    int j = 0;
    for (int i = 0; i < int(v.size()); i++)
        if (status[i]) v[j++] = v[i];
    v.resize(j);
}
void reduceVector(vector<int>& v, vector<uchar> status) {           // :22-29
    int j = 0;
    for (int i = 0; i < int(v.size()); i++)
        if (status[i]) v[j++] = v[i];
    v.resize(j);
}

void CameraModel::liftProjective(float u, float v, double& x, double& y, double& z) const {
    FeCamera c;
    c.model = model == VG_CAM_MEI ? FE_CAM_MEI : model == VG_CAM_KANNALA_BRANDT ? FE_CAM_KB : FE_CAM_PINHOLE;
    for (int i = 0; i < 8; ++i) c.p[i] = p[i];
    c.xi = xi;
    fe_cam_lift(c, u, v, x, y, z);
}
vg_fe_camera CameraModel::abi() const {
    vg_fe_camera c;
    std::memset(&c, 0, sizeof(c));
    c.struct_size = (int)sizeof(c); c.model = model; c.xi = xi;
    for (int i = 0; i < 8; ++i) c.p[i] = p[i];
    return c;
}

FeatureTracker::FeatureTracker() : cur_time(0), prev_time(0) {}
FeatureTracker::~FeatureTracker() { if (vg_) vg_destroy(vg_); }

static void chk(int rc, vg_handle* h, const char* what) {
    if (rc != VG_OK) throw std::runtime_error(std::string(what) + ": " + (h ? vg_last_error(h) : "no handle") + " (no CPU fallback)");
}

void FeatureTracker::setMask() {                             // feature_tracker.cpp:36-69, on the device (vg_fe_set_mask)
    // The reference orders the points with std::sort by track_cnt (:48-51): the order among equal counts is whatever the platform's
    // std::sort gives.  The same call is made here, and the device walks the list in that order (its own sort by count is stable,
    // i.e. the identity on a sorted list) -- the result is the reference's on the platform this is built on (tests/test_fe_dropin.py).
    // `mask` itself stays on the device: goodFeaturesToTrack below consumes it there (vg_fe_detect_masked).
    std::vector<float> xy;
    std::vector<int> cnt, kept((size_t)fe_capacity_, 0);
    vg_pack::OrderCtx<FeatureTracker>::SortedList cnt_pts_id;
    vg_pack::sorted_for_setmask(*this, fe_capacity_, xy, cnt, cnt_pts_id);
    const int n = (int)cnt_pts_id.size();
    const uint8_t* base[1] = {FISHEYE ? fisheye_mask.data : nullptr};
    int nk = 0;
    chk(vg_fe_set_mask(vg_, xy.data(), cnt.data(), &n, base, MIN_DIST, kept.data(), &nk), vg_, "vg_fe_set_mask");
    vg_pack::take_setmask_result(*this, cnt_pts_id, kept.data(), nk);
}

void FeatureTracker::addPoints() {                            // :71-79
    for (auto& p : n_pts) {
        forw_pts.push_back(p);
        ids.push_back(-1);
        track_cnt.push_back(1);
    }
}

typedef vg_pack::OrderCtx<FeatureTracker> OrderCtx;

// readImage around the library call: the arguments of a tracker's frame ...
static void frame_input(FeatureTracker& t, const cv::Mat& _img, vg_fe_frame_in& in, OrderCtx& ctx) {
    vg_pack::fill_frame_in(t, _img, PUB_THIS_FRAME, EQUALIZE, MAX_CNT, MIN_DIST, F_THRESHOLD, FOCAL_LENGTH, in);
    std::memcpy(in.intr, t.m_camera.p, sizeof(in.intr));                                // (the stream lifts with its vg_fe_set_camera camera)
    in.base_mask = (FISHEYE && PUB_THIS_FRAME) ? t.fisheye_mask.data : nullptr;         // :38-41 (contiguous ROW x COL, readFeatureTrackerParameters)
    ctx.t = &t; ctx.n_in = in.n;
    in.order = vg_pack::order_callback<FeatureTracker>; in.user = &ctx;
}

// ... and everything readImage does once the call has returned VG_OK (ctx.sorted: setMask's list as the order callback made it).
// FeatureTrackerBatch runs the two for S trackers around ONE call.
static void apply_frame(FeatureTracker& t, const cv::Mat& _img, const vg_fe_frame_out& out, const OrderCtx& ctx) {
    if (t.forw_img.empty()) t.prev_img = t.cur_img = t.forw_img = _img;
    else t.forw_img = _img;
    vg_pack::apply_statuses(t, out, ctx.n_in);                               // only now: the call returned VG_OK
    if (PUB_THIS_FRAME) vg_pack::apply_published(t, out, ctx.sorted);
    if ((int)t.forw_pts.size() != out.n_final) throw std::runtime_error("FeatureTracker::readImage: list length differs from the device's");
    t.prev_img = t.cur_img;                                                  // :160-166
    t.prev_pts = t.cur_pts;
    t.prev_un_pts = t.cur_un_pts;
    t.cur_img = t.forw_img;
    t.cur_pts = t.forw_pts;
    vg_pack::lifted_points(t, out.un_xy);
    t.prev_time = t.cur_time;
}

// ONE library call per frame (vg_fe_read_image): the frame and cur_pts go up in one block; CLAHE, pyramid, LK, the border test,
// reduceVector and -- on a published frame -- rejectWithF, setMask's walk, goodFeaturesToTrack, addPoints and the lifting of
// undistortedPoints run on the device without the host in between; the members setMask() / rejectWithF() / undistortedPoints() remain
// for callers that drive the steps themselves.
void FeatureTracker::readImage(const cv::Mat& _img, double _cur_time) {    // :81-167
    cur_time = _cur_time;
    if (!configured_) {
        chk(vg_create(&vg_), vg_, "vg_create");
        // vg_fe_read_image takes streams of up to 2048 points; a list never exceeds MAX_CNT (:144-156), the factor is slack
        if (MAX_CNT > 2048) throw std::runtime_error("FeatureTracker::readImage: max_cnt > 2048 is not offered (vg_fe_read_image)");
        fe_capacity_ = std::min(std::max(MAX_CNT, 1) * 4, 2048);
        chk(vg_fe_configure(vg_, COL, ROW, 1, fe_capacity_), vg_, "vg_fe_configure");
        configured_ = true;
        camera_sent_ = false;                                                // (vg_fe_configure clears the stream's camera)
    }
    if (!camera_sent_) {
        const vg_fe_camera cam = m_camera.abi();
        chk(vg_fe_set_camera(vg_, 0, &cam), vg_, "vg_fe_set_camera");
        camera_sent_ = true;
    }
    if ((int)cur_pts.size() > fe_capacity_) throw std::runtime_error("FeatureTracker::readImage: more points than the configured capacity");
    vg_fe_frame_in in;
    OrderCtx ctx;
    frame_input(*this, _img, in, ctx);
    vg_fe_frame_out out;
    chk(vg_fe_read_image(vg_, &in, &out), vg_, "vg_fe_read_image");
    apply_frame(*this, _img, out, ctx);
}

void FeatureTracker::rejectWithF() {                                       // feature_tracker.cpp:169-202
    if (forw_pts.size() >= 8) {
        const int n = (int)forw_pts.size();
        vector<cv::Point2f> un_cur_pts(cur_pts.size()), un_forw_pts(forw_pts.size());
        for (unsigned int i = 0; i < cur_pts.size(); i++) {
            double x, y, z;
            m_camera.liftProjective(cur_pts[i].x, cur_pts[i].y, x, y, z);
            x = FOCAL_LENGTH * x / z + COL / 2.0;
            y = FOCAL_LENGTH * y / z + ROW / 2.0;
            un_cur_pts[i] = cv::Point2f((float)x, (float)y);
            m_camera.liftProjective(forw_pts[i].x, forw_pts[i].y, x, y, z);
            x = FOCAL_LENGTH * x / z + COL / 2.0;
            y = FOCAL_LENGTH * y / z + ROW / 2.0;
            un_forw_pts[i] = cv::Point2f((float)x, (float)y);
        }
        vector<uchar> status(n);
        // cv::findFundamentalMat(un_cur_pts, un_forw_pts, cv::FM_RANSAC, F_THRESHOLD, 0.99, status) on the device
        chk(vg_fe_reject_with_f(vg_, &un_cur_pts[0].x, &un_forw_pts[0].x, n, F_THRESHOLD, status.data(), nullptr, nullptr), vg_, "vg_fe_reject_with_f");
        reduceVector(prev_pts, status);
        reduceVector(cur_pts, status);
        reduceVector(forw_pts, status);
        reduceVector(cur_un_pts, status);
        reduceVector(ids, status);
        reduceVector(track_cnt, status);
    }
}

bool FeatureTracker::updateID(unsigned int i) {                              // :204-214
    if (i < ids.size()) {
        if (ids[i] == -1) ids[i] = n_id++;
        return true;
    }
    return false;
}

void FeatureTracker::readIntrinsicParameter(const string& calib_file) {
    // feature_tracker.cpp:216-220 -> CameraFactory::generateCameraFromYamlFile ->
    //   model_type PINHOLE: PinholeCamera::Parameters::readFromYamlFile (PinholeCamera.cc:144-183): distortion_parameters k1 k2 p1 p2,
    //                       projection_parameters fx fy cx cy
    //   model_type MEI:     CataCamera::Parameters::readFromYamlFile (CataCamera.cc:161-203): mirror_parameters xi,
    //                       distortion_parameters k1 k2 p1 p2, projection_parameters gamma1 gamma2 u0 v0
    // KANNALA_BRANDT and SCARAMUZZA are refused by name here; readCameraModel below reads KANNALA_BRANDT as well (it lifts on the
    // device too, csrc/fe_camera.h) for a caller that assigns m_camera.
    VinsYaml fs;
    if (!fs.load(calib_file)) throw std::runtime_error("readIntrinsicParameter: cannot read " + calib_file);
    const std::string model = fs.str("model_type", "PINHOLE");
    const bool mei = model == "MEI";
    if (model != "PINHOLE" && !mei)
        throw std::runtime_error("readIntrinsicParameter: camera model " + model + " is not supported (PINHOLE and MEI lift on the device)");
    CameraModel c;
    c.model = mei ? VG_CAM_MEI : VG_CAM_PINHOLE;
    c.xi = mei ? fs.number("mirror_parameters.xi") : 0.0;
    c.p[0] = fs.number(mei ? "projection_parameters.gamma1" : "projection_parameters.fx");
    c.p[1] = fs.number(mei ? "projection_parameters.gamma2" : "projection_parameters.fy");
    c.p[2] = fs.number(mei ? "projection_parameters.u0" : "projection_parameters.cx");
    c.p[3] = fs.number(mei ? "projection_parameters.v0" : "projection_parameters.cy");
    c.p[4] = fs.number("distortion_parameters.k1"); c.p[5] = fs.number("distortion_parameters.k2");
    c.p[6] = fs.number("distortion_parameters.p1"); c.p[7] = fs.number("distortion_parameters.p2");
    m_camera = c;
    camera_sent_ = false;                                                    // (a configured stream gets it with its next frame)
}

CameraModel readCameraModel(const std::string& file) {
    // CameraFactory::generateCameraFromYamlFile with the models that lift on the device: PINHOLE and MEI as readIntrinsicParameter above,
    // KANNALA_BRANDT as EquidistantCamera::Parameters::readFromYamlFile (EquidistantCamera.cc:146-182): projection_parameters k2 k3 k4 k5
    // mu mv u0 v0, stored as vg_fe_camera::p takes them (mu mv u0 v0 k2 k3 k4 k5)
    VinsYaml fs;
    if (!fs.load(file)) throw std::runtime_error("readCameraModel: cannot read " + file);
    const std::string model = fs.str("model_type", "PINHOLE");
    if (model == "KANNALA_BRANDT") {
        CameraModel c;
        c.model = VG_CAM_KANNALA_BRANDT;
        c.xi = 0.0;
        const char* keys[8] = {"mu", "mv", "u0", "v0", "k2", "k3", "k4", "k5"};
        for (int i = 0; i < 8; ++i) c.p[i] = fs.number(std::string("projection_parameters.") + keys[i]);
        return c;
    }
    if (model != "PINHOLE" && model != "MEI")
        throw std::runtime_error("readCameraModel: camera model " + model + " is not supported (PINHOLE, MEI and KANNALA_BRANDT lift on the device)");
    FeatureTracker tr;
    tr.readIntrinsicParameter(file);
    return tr.m_camera;
}

void FeatureTracker::undistortedPoints() {                                   // :258-306, lifting on the device
    const int n = (int)cur_pts.size();
    std::vector<float> un((size_t)std::max(n, 1) * 2);
    const vg_fe_camera cam = m_camera.abi();
    if (n > 0) chk(vg_fe_lift(vg_, &cam, &cur_pts[0].x, n, un.data()), vg_, "vg_fe_lift");
    vg_pack::lifted_points(*this, un.data());
}

// ---- FeatureTrackerBatch: the node's loop over trackerData[i].readImage (feature_tracker_node.cpp:82-101) with one library call
FeatureTrackerBatch::FeatureTrackerBatch(int n_streams) : trackers((size_t)std::max(n_streams, 1)) {}
FeatureTrackerBatch::~FeatureTrackerBatch() { if (vg_) vg_destroy(vg_); }

void FeatureTrackerBatch::readImages(const vector<cv::Mat>& imgs, const vector<double>& stamps) {
    const int S = size();
    if ((int)imgs.size() != S || (int)stamps.size() != S) throw std::runtime_error("FeatureTrackerBatch::readImages: one image and one stamp per stream");
    if (!configured_) {
        chk(vg_create(&vg_), vg_, "vg_create");
        if (MAX_CNT > 2048) throw std::runtime_error("FeatureTrackerBatch::readImages: max_cnt > 2048 is not offered (vg_fe_read_image_batch)");
        fe_capacity_ = std::min(std::max(MAX_CNT, 1) * 4, 2048);
        chk(vg_fe_configure(vg_, COL, ROW, S, fe_capacity_), vg_, "vg_fe_configure");
        for (int c = 0; c < S; c++) trackers[c].camera_sent_ = false;        // (vg_fe_configure clears every stream's camera)
        configured_ = true;
    }
    for (int c = 0; c < S; c++) {                                            // every tracker keeps its own camera: the models may differ
        if (trackers[c].camera_sent_) continue;
        const vg_fe_camera cam = trackers[c].m_camera.abi();
        chk(vg_fe_set_camera(vg_, c, &cam), vg_, "vg_fe_set_camera");
        trackers[c].camera_sent_ = true;
    }
    vector<vg_fe_frame_in> in((size_t)S);
    vector<vg_fe_frame_out> out((size_t)S);
    vector<OrderCtx> ctx((size_t)S);
    for (int c = 0; c < S; c++) {
        if ((int)trackers[c].cur_pts.size() > fe_capacity_) throw std::runtime_error("FeatureTrackerBatch::readImages: more points than the configured capacity");
        frame_input(trackers[c], imgs[c], in[c], ctx[c]);
    }
    chk(vg_fe_read_image_batch(vg_, S, in.data(), out.data()), vg_, "vg_fe_read_image_batch");
    for (int c = 0; c < S; c++) {                                            // only now: the call returned VG_OK
        trackers[c].cur_time = stamps[c];
        apply_frame(trackers[c], imgs[c], out[c], ctx[c]);
    }
}
