// resident_estimator.h — N estimators in their NON_LINEAR phase whose sliding windows live on the device between frames
// (include/vinsgpu.h: vg_ba_seq_*; csrc/ba_seq.hip).  The two callbacks keep the reference's signatures
// (vins_estimator/src/estimator.h:32-33) with the estimator's index in front:
//     processIMU(i, dt, linear_acceleration, angular_velocity)        estimator.cpp:83-117
//     processImage(i, image)                                          estimator.cpp:120-215 (solver_flag == NON_LINEAR branch)
// processIMU does what the reference's does on the host (unless useDeviceImu() moved that to the device as well): it keeps the raw samples of the running interval (dt_buf / acc_buf /
// gyr_buf of IntegrationBase) and propagates Ps / Rs / Vs of the newest frame.  processImage only stores the frame;
// solve() then runs ONE device step for all estimators (addFeatureCheckParallax, triangulate, optimization(), slideWindow(),
// removeFailures(): vg_ba_seq_step_async) and brings the states back.  f_manager, para_*, pre_integrations[] and
// last_marginalization_info have no host copy: that is the point.
#pragma once
#include <map>
#include <utility>
#include <vector>
#include "estimator.h"

class ResidentEstimators {
  public:
    typedef std::map<int, std::vector<std::pair<int, Eigen::Matrix<double, 7, 1>>>> Image;   // feature_id -> [(camera_id, x y z u v vx vy)]
    struct Interval {                         // what IntegrationBase keeps of one frame interval (integration_base.h:188-208)
        Vector3d linearized_acc, linearized_gyr, linearized_ba, linearized_bg;
        std::vector<double> samples;          // rows (dt, acc, gyr)
    };
    struct One {
        Vector3d Ps[WINDOW_SIZE + 1], Vs[WINDOW_SIZE + 1], Bas[WINDOW_SIZE + 1], Bgs[WINDOW_SIZE + 1];   // as the last solve + slide left them
        Matrix3d Rs[WINDOW_SIZE + 1];
        Matrix3d ric;
        Vector3d tic;
        double td = 0;
        Vector3d acc_0, gyr_0, g;
        bool first_imu = false;
        Estimator::MarginalizationFlag marginalization_flag = Estimator::MARGIN_OLD;   // of the last solve()
        vg_ba_summary last_summary;
        int n_features = 0, status = 0;       // tracks left after the slide; VG_OK or VG_ERR_UNSUPPORTED (a capacity was exceeded)
        int last_track_num = 0;               // f_manager.last_track_num of the last frame
        // Estimator::failureDetection() (estimator.cpp:621-667) on the window as solved, BEFORE its slide, against last_P / last_R
        // of the frame before (:205-208).  The reference reboots on failure (clearState + setParameter, :193-199).  Here the flag is
        // raised and the caller decides: the windows of a batch begin together (vg_ba_seq_begin), so re-initialising ONE estimator
        // means handing the batch over again (a per-window re-seed of a running sequence is not offered yet).
        bool failure_occur = false;
        Vector3d last_P, last_P0;
        Matrix3d last_R, last_R0;
        // Headers[k].stamp.toSec() of the window (estimator.h:95): set by the caller after handOver() for the frames handed over, by
        // processImage(i, image, stamp) for every further frame, shifted with the window; what setReloFrame() resolves its stamp against
        double Headers[WINDOW_SIZE + 1] = {};
        // relocalisation (estimator.h:125-138).  setReloFrame() arms the next solve(); after it the by-products of double2vector()
        // (estimator.cpp:598-612) are here, relo_Pose is the gauge-fixed loop pose and relo_n_factors the factors the problem held
        bool relocalization_info = false;
        int relo_frame_local_index = 0, relo_n_factors = 0;
        double relo_frame_stamp = 0, relo_Pose[7] = {0, 0, 0, 0, 0, 0, 1}, relo_relative_yaw = 0;
        int relo_frame_index = 0;
        Matrix3d drift_correct_r;
        Vector3d drift_correct_t, relo_relative_t;
        Quaterniond relo_relative_q;
        bool relo_solved = false;             // the LAST solve() carried a relocalisation frame for this estimator
        // ---- internal
        Interval cur, prev;                   // pre_integrations[WINDOW_SIZE] (running) and [WINDOW_SIZE - 1] (may take cur's samples, estimator.cpp:1069-1085)
        bool merge_pending = false;
        std::vector<int> ids;                 // the stored frame
        std::vector<double> rows;
        bool have_frame = false;
    };

    ResidentEstimators(int n, int max_features, int max_new_obs);
    ~ResidentEstimators();
    ResidentEstimators(const ResidentEstimators&) = delete;
    ResidentEstimators& operator=(const ResidentEstimators&) = delete;

    // Hand-over of estimator i between two frames (after slideWindow()): its states, pre_integrations[1 .. WINDOW_SIZE - 1] (the
    // last one with its raw samples), f_manager.feature and last_marginalization_info; acc_0 / gyr_0 = the newest IMU sample.
    void handOver(int i, Estimator& e, const Vector3d& acc_0, const Vector3d& gyr_0);
    // Opt-in, before begin(): Estimator::processIMU and the IMU part of slideWindow() run on the device (vg_ba_seq_imu_begin /
    // vg_ba_seq_step_imu_async).  processIMU then only buffers the samples (no propagation, no integration), solve() sends them with
    // the observations, and Ps / Rs / Vs[WINDOW_SIZE] of the mirror are filled from the downloaded states as before.  The raw samples
    // stay buffered on the host for handBack.
    // max_samples: the most IMU samples one frame may bring (1 .. 512; a capacity, the step uploads what a frame holds).
    void useDeviceImu(int max_samples = 512);
    bool deviceImu() const { return device_imu_; }
    // parity tap in that mode: acc_0 (3), gyr_0 (3), g (3) as the DEVICE holds them for estimator i (vg_ba_seq_imu_get)
    void residentMeasurement(int i, double seed9[9]);
    // measurement taps in that mode (vg_ba_seq_imu_timing / _times): device time of the IMU kernel and of the merge of the last solve(), ms
    void deviceImuTiming(bool on);
    void deviceImuTimes(float& imu_kernel_ms, float& merge_kernel_ms);
    // Opt-in, before begin(): the windows get the loop-pose block and room for max_match (1 .. 1024) relocalisation factors
    // (vg_ba_seq_relo_reserve), and setReloFrame() may be called between two frames.
    void useRelocalisation(int max_match);
    // Estimator::setReloFrame (estimator.cpp:1128-1147) of estimator i: the stamp is looked up in Headers[0 .. WINDOW_SIZE); where it is
    // found, the NEXT solve() carries the loop pose (initially the pose of that frame) and one factor per matched landmark
    // (match_points[k] = x, y, feature id; ids ascending), selected on the device (vg_ba_seq_set_relo).  Returns whether it was found.
    bool setReloFrame(int i, double frame_stamp, int frame_index, const std::vector<Vector3d>& match_points, const Vector3d& relo_t, const Matrix3d& relo_r);
    // Opt-in, before or after begin(): every solve() also forms, on the device, what the estimator node publishes after the frame
    // (pubKeyframe / pubPointCloud, visualization.cpp:348-404 / :240-296; vg_ba_seq_outputs_*): room for max_points (1 .. 1024)
    // rows per list and estimator.  The lists of the LAST solve() are in keyframe(i), pointCloud(i), marginCloud(i); right after
    // begin() (or this call on a running batch) they are those of the windows as handed over.
    struct Keyframe {                         // the arguments of host/keyframe.h's KeyFrame constructors, packed floats (cv::Point3f / Point2f)
        bool valid = false;                   // marginalization_flag == 0 after the last solve(): the reference would publish it (:351)
        int status = 0, count = 0;            // vg_ba_seq_outputs::status, n_keyframe (the true count; the vectors hold min(count, max_points))
        double stamp = 0;                     // Headers[WINDOW_SIZE - 2] of the mirror (the sequence keeps no stamps)
        Vector3d vio_T_w_i;
        Matrix3d vio_R_w_i;
        std::vector<float> point_3d, point_2d_uv, point_2d_norm;     // 3 / 2 / 2 floats per point
        std::vector<double> point_id;
    };
    struct Cloud {
        int status = 0, count = 0;
        std::vector<float> xyz;               // 3 floats per point
    };
    void usePublishedOutputs(int max_points);
    const Keyframe& keyframe(int i) const { return pub_.at(i).kf; }
    const Cloud& pointCloud(int i) const { return pub_.at(i).cloud; }
    const Cloud& marginCloud(int i) const { return pub_.at(i).margin; }
    void begin();                             // vg_ba_seq_begin once every estimator has been handed over
    // The way back, between two frames: window i of the running sequence into the members of a host Estimator (Ps / Rs / Vs / Bas /
    // Bgs, ric / tic / td, pre_integrations[1 .. WINDOW_SIZE - 1] -- the last one with its raw samples --, f_manager.feature,
    // last_marginalization_info + parameter blocks): vg_ba_seq_export + vg_ba_seq_get_tracks.  For a checkpoint or a re-start after
    // failureDetection().  The device keeps its copy; reseed() replaces it.
    void handBack(int i, Estimator& e);
    void reseed(int i, Estimator& e, const Vector3d& acc_0, const Vector3d& gyr_0);     // vg_ba_seq_import: estimator i only
    void processIMU(int i, double dt, const Vector3d& linear_acceleration, const Vector3d& angular_velocity);
    void processImage(int i, const Image& image);
    void processImage(int i, const Image& image, double stamp);      // with header.stamp.toSec(): Headers[WINDOW_SIZE] of the mirror
    void solve();                             // one frame for every estimator (all must have received their image)
    One& operator[](int i) { return est_[i]; }
    int size() const { return (int)est_.size(); }

  private:
    struct Window;                            // the hand-over arrays of one estimator (alive until begin())
    Window* pack(int i, Estimator& e, const Vector3d& acc_0, const Vector3d& gyr_0);
    std::vector<One> est_;
    std::vector<Window*> win_;
    vg_handle* vg_ = nullptr;
    int max_features_, max_new_obs_;
    bool begun_ = false;
    bool device_imu_ = false;
    int max_samples_ = 512;
    int max_match_ = 0;
    struct Published { Keyframe kf; Cloud cloud, margin; };
    std::vector<Published> pub_;
    int max_points_ = 0;                      // usePublishedOutputs (0: not asked for)
    void reservePublished();                  // vg_ba_seq_outputs_reserve + the lists of the windows as they stand
    void fetchPublished();                    // vg_ba_seq_get_outputs of every estimator into pub_
    void stepFromHost();                      // solve(): the host-fed step (pre-integration + propagated guess from here)
    void finishStep();                        // solve(): download, mirror, sample buffers
};
