// feature_tracker.h — drop-in FeatureTracker for the MI355X path: same class name, members and method signatures as
// feature_tracker/src/feature_tracker.h:28-65 of the reference.  readImage() is ONE library call per frame, vg_fe_read_image
// (include/vinsgpu.h); the members setMask / rejectWithF / undistortedPoints keep the step-by-step entry points
// of feature_tracker.cpp:81-167 for callers that drive the steps themselves:
//   cv::createCLAHE(...)->apply      -> vg_fe_push_frames(.., equalize)     (:87-93)
//   cv::calcOpticalFlowPyrLK         -> vg_fe_track                          (:113)
//   cv::goodFeaturesToTrack          -> vg_fe_detect                         (:149)
//   cv::findFundamentalMat(RANSAC)   -> vg_fe_reject_with_f                  (:191; deterministic RANSAC, ASSUMPTIONS F9)
// Differences (documented in INTEGRATION.md): the camera model is CameraModel below -- PinholeCamera and CataCamera (MEI) restated
// from camera_model/src/camera_models/{PinholeCamera,CataCamera}.cc, EquidistantCamera (KANNALA_BRANDT) by the definition of
// csrc/fe_camera.h, the function the kernels lift with -- instead of camodocal::CameraPtr.
#pragma once
#include <map>
#include <string>
#include <vector>
#include "compat/cv_compat.h"
#include "../../include/vinsgpu.h"
#include "../csrc/fe_camera.h"

using namespace std;

// globals of feature_tracker/src/parameters.h (same names)
extern int ROW, COL, MAX_CNT, MIN_DIST, EQUALIZE, FISHEYE, FOCAL_LENGTH;
extern bool PUB_THIS_FRAME;
extern double F_THRESHOLD;
extern int FREQ, SHOW_TRACK, FE_WINDOW_SIZE;
extern std::string IMAGE_TOPIC, FE_IMU_TOPIC, FISHEYE_MASK;
// feature_tracker/src/parameters.cpp:37-74 without the ROS node handle: the path of the configuration file is passed directly
void readFeatureTrackerParameters(const std::string& config_file, const std::string& vins_folder = "");

bool inBorder(const cv::Point2f& pt);
void reduceVector(vector<cv::Point2f>& v, vector<uchar> status);
void reduceVector(vector<int>& v, vector<uchar> status);

// camodocal::PinholeCamera, camodocal::CataCamera or camodocal::EquidistantCamera parameters; the default is config/euroc/euroc_config.yaml:13-22
struct CameraModel {
    int model = VG_CAM_PINHOLE;
    double p[8] = {461.6, 460.3, 363.0, 248.1, -2.917e-01, 8.228e-02, 5.333e-05, -1.578e-04};   // fx fy cx cy | gamma1 gamma2 u0 v0, then k1 k2 p1 p2; KANNALA_BRANDT: mu mv u0 v0 k2 k3 k4 k5
    double xi = 0.0;             // MEI: mirror_parameters.xi
    void liftProjective(float u, float v, double& x, double& y, double& z) const;     // the projective ray, as the kernels compute it
    vg_fe_camera abi() const;    // what vg_fe_set_camera / vg_fe_lift take
};

// The camera of a settings file, for a caller to assign to FeatureTracker::m_camera: PINHOLE and MEI as
// FeatureTracker::readIntrinsicParameter reads them, and KANNALA_BRANDT (EquidistantCamera::Parameters::readFromYamlFile:
// projection_parameters k2 k3 k4 k5 mu mv u0 v0).  Throws, naming the model, for anything else.
CameraModel readCameraModel(const std::string& file);

class FeatureTracker {
  public:
    FeatureTracker();
    ~FeatureTracker();

    void readImage(const cv::Mat& _img, double _cur_time);
    void setMask();
    void addPoints();
    bool updateID(unsigned int i);
    void readIntrinsicParameter(const string& calib_file);   // PINHOLE or MEI section of the configuration file (host/yaml_config.h)
    void rejectWithF();
    void undistortedPoints();

    cv::Mat mask;
    cv::Mat fisheye_mask;
    cv::Mat prev_img, cur_img, forw_img;
    vector<cv::Point2f> n_pts;
    vector<cv::Point2f> prev_pts, cur_pts, forw_pts;
    vector<cv::Point2f> prev_un_pts, cur_un_pts;
    vector<cv::Point2f> pts_velocity;
    vector<int> ids;
    vector<int> track_cnt;
    map<int, cv::Point2f> cur_un_pts_map;
    map<int, cv::Point2f> prev_un_pts_map;
    CameraModel m_camera;
    double cur_time;
    double prev_time;

    static int n_id;

  private:
    vg_handle* vg_ = nullptr;      // owns the device-side pyramids of cur_img / forw_img
    int fe_capacity_ = 0;
    bool configured_ = false;
    bool camera_sent_ = false;     // m_camera has gone to the stream that runs this tracker's frames (vg_fe_set_camera)
    friend class FeatureTrackerBatch;
};

// S stand-alone trackers on ONE handle: readImages() is the loop of the reference's node over trackerData[i].readImage(...)
// (feature_tracker_node.cpp:82-101) made with one library call, vg_fe_read_image_batch.  Every tracker keeps its own camera and its own
// lists; COL, ROW, MAX_CNT, MIN_DIST, EQUALIZE, F_THRESHOLD and PUB_THIS_FRAME are the process-wide globals they already are (so all
// streams publish or none does).  No tracker is touched before the call has returned VG_OK.
class FeatureTrackerBatch {
  public:
    explicit FeatureTrackerBatch(int n_streams);
    ~FeatureTrackerBatch();
    FeatureTrackerBatch(const FeatureTrackerBatch&) = delete;
    FeatureTrackerBatch& operator=(const FeatureTrackerBatch&) = delete;
    void readImages(const vector<cv::Mat>& imgs, const vector<double>& stamps);
    int size() const { return (int)trackers.size(); }
    vector<FeatureTracker> trackers;

  private:
    vg_handle* vg_ = nullptr;
    int fe_capacity_ = 0;
    bool configured_ = false;
};
