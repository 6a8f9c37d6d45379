// fe_camera.h — the camera models the front end lifts pixels with, as ONE function for the device kernels (fe_frame.hip,
// fe_kernels.hip), the host of the library (fe_host.hip) and the stand-alone host class (host/feature_tracker.cpp):
//   FE_CAM_PINHOLE  PinholeCamera::liftProjective (camera_model/src/camera_models/PinholeCamera.cc:450-510, distortion :646-661)
//   FE_CAM_MEI      CataCamera::liftProjective    (CataCamera.cc:556-626, distortion :766-782, inverse K :320-323): the pinhole
//                   lift followed by the unified model's z
// Every expression is the reference's, in its order, in double.  A file that includes this header must be compiled without
// floating-point contraction (-ffp-contract=off, or a target without fused multiply-add): a contracted a * b + c rounds once.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(VINS_SIMT)
#define FE_CAM_FN __host__ __device__ __forceinline__
#else
#define FE_CAM_FN inline
#endif

#define FE_CAM_PINHOLE 0            // = VG_CAM_PINHOLE (include/vinsgpu.h)
#define FE_CAM_MEI 1                // = VG_CAM_MEI

struct FeCamera {
    int model;                      // FE_CAM_*
    double p[8];                    // PINHOLE: fx fy cx cy k1 k2 p1 p2;  MEI: gamma1 gamma2 u0 v0 k1 k2 p1 p2
    double xi;                      // MEI: mirror_parameters.xi
};

// pixel -> projective ray (x, y, z).  `c.model` is uniform wherever this is called from a kernel (one camera per stream, one workgroup
// or launch per stream): the model test is a scalar branch.  PINHOLE: z = 1.0.
FE_CAM_FN void fe_cam_lift(const FeCamera& c, float px, float py, double& x, double& y, double& z) {
    const double fx = c.p[0], fy = c.p[1], cx = c.p[2], cy = c.p[3], k1 = c.p[4], k2 = c.p[5], p1 = c.p[6], p2 = c.p[7];
    const double mx_d = (1.0 / fx) * (double)px + (-cx / fx), my_d = (1.0 / fy) * (double)py + (-cy / fy);
    double mx_u = mx_d, my_u = my_d;
    // CataCamera's m_noDistortion (:307-317); PinholeCamera has the same switch but the pinhole path here never took it
    const bool skip = c.model == FE_CAM_MEI && k1 == 0.0 && k2 == 0.0 && p1 == 0.0 && p2 == 0.0;
    if (!skip) {
#pragma unroll 1
        for (int it = 0; it < 8; ++it) {                            // recursive distortion model, n = 8
            const double mx2 = mx_u * mx_u, my2 = my_u * my_u, mxy = mx_u * my_u, rho2 = mx2 + my2;
            const double rad = k1 * rho2 + k2 * rho2 * rho2;
            const double dx = mx_u * rad + 2.0 * p1 * mxy + p2 * (rho2 + 2.0 * mx2);
            const double dy = my_u * rad + 2.0 * p2 * mxy + p1 * (rho2 + 2.0 * my2);
            mx_u = mx_d - dx; my_u = my_d - dy;
        }
    }
    x = mx_u; y = my_u;
    if (c.model != FE_CAM_MEI) { z = 1.0; return; }
    const double xi = c.xi;                                         // :615-625
    if (xi == 1.0)
        z = (1.0 - mx_u * mx_u - my_u * my_u) / 2.0;
    else {
        const double rho2 = mx_u * mx_u + my_u * my_u;
        z = 1.0 - xi * (rho2 + 1.0) / (xi + sqrt(1.0 + (1.0 - xi * xi) * rho2));
    }
}

// (x / z, y / z) as undistortedPoints() stores them (cv::Point2f); the pinhole's z is 1.0: no division
FE_CAM_FN void fe_cam_lift_xy(const FeCamera& c, float px, float py, float& ox, float& oy) {
    double x, y, z;
    fe_cam_lift(c, px, py, x, y, z);
    if (c.model == FE_CAM_MEI) { ox = (float)(x / z); oy = (float)(y / z); }
    else { ox = (float)x; oy = (float)y; }
}
