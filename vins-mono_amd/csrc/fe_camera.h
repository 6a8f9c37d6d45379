// fe_camera.h — the camera models the front end lifts pixels with, as ONE function for the device kernels (fe_frame.hip,
// fe_kernels.hip), the host of the library (fe_host.hip) and the stand-alone host class (host/feature_tracker.cpp):
//   FE_CAM_PINHOLE  PinholeCamera::liftProjective (camera_model/src/camera_models/PinholeCamera.cc:450-510, distortion :646-661)
//   FE_CAM_MEI      CataCamera::liftProjective    (CataCamera.cc:556-626, distortion :766-782, inverse K :320-323): the pinhole
//                   lift followed by the unified model's z
//   FE_CAM_KB       EquidistantCamera::liftProjective (EquidistantCamera.cc:427-442, backprojectSymmetric :715-818, inverse K
//                   :271-274): the Kannala-Brandt (equidistant) lens, fe_cam_lift_kb below
// PINHOLE and MEI: every expression is the reference's, in its order, in double.  KB: the reference's quantity -- the root theta of
// theta + k2 theta^3 + k3 theta^5 + k4 theta^7 + k5 theta^9 = r on the lens's first monotone branch -- by a route of its own
// (a fixed Newton count and a sine / cosine written out here), so that the emulated kernels, the device and the NumPy restatement
// of the tests agree bit for bit.  A file that includes this header must be compiled without floating-point contraction
// (-ffp-contract=off, or a target without fused multiply-add): a contracted a * b + c rounds once.
#pragma once
#include <math.h>
#include <cmath>

#if defined(__HIPCC__) || defined(VINS_SIMT)
#define FE_CAM_FN __host__ __device__ __forceinline__
#else
#define FE_CAM_FN inline
#endif

#define FE_CAM_PINHOLE 0            // = VG_CAM_PINHOLE (include/vinsgpu.h)
#define FE_CAM_MEI 1                // = VG_CAM_MEI
#define FE_CAM_KB 3                 // = VG_CAM_KANNALA_BRANDT (2 is no model)

struct FeCamera {
    int model;                      // FE_CAM_*
    double p[8];                    // PINHOLE: fx fy cx cy k1 k2 p1 p2;  MEI: gamma1 gamma2 u0 v0 k1 k2 p1 p2;  KB: mu mv u0 v0 k2 k3 k4 k5
    double xi;                      // MEI: mirror_parameters.xi
};

#define FE_KB_NEWTON 10             // Newton steps of fe_cam_lift_kb: a fixed count, as the 8 distortion passes of the pinhole are

// sin(t) and cos(t) from + - * rint, compares and selects alone (no libm: the host's and the device's would have to agree bit for
// bit): k = rint(t * 2 / pi), y = t - k * pi / 2 by a two-constant Cody-Waite reduction (fdlibm's pio2_1, 33 bits: k * pio2_1 is exact
// for |k| < 2^20; pio2_1t its tail), the Taylor polynomials of degree 17 and 16 on |y| <= pi / 4 (first dropped terms 8e-20 and 2e-18),
// then the quadrant.  Meant for the |t| of a lens (a few radians); absolute error <= 1.2e-16 on [0, 3.2].  The coefficients sit in
// two tables walked by a loop that is not unrolled: as literals in straight-line code they cost the kernels of fe_frame.hip spills.
FE_CAM_FN void fe_kb_sincos(double t, double& s, double& c) {
    static constexpr double S[8] = {-1.0 / 6.0, 1.0 / 120.0, -1.0 / 5040.0, 1.0 / 362880.0, -1.0 / 39916800.0, 1.0 / 6227020800.0,
                                    -1.0 / 1307674368000.0, 1.0 / 355687428096000.0};                 // y^3 ... y^17
    static constexpr double C[8] = {-1.0 / 2.0, 1.0 / 24.0, -1.0 / 720.0, 1.0 / 40320.0, -1.0 / 3628800.0, 1.0 / 479001600.0,
                                    -1.0 / 87178291200.0, 1.0 / 20922789888000.0};                    // y^2 ... y^16
    const double k = rint(t * 6.36619772367581382433e-01);
    const double y = (t - k * 1.57079632673412561417e+00) - k * 6.07710050650619224932e-11;
    const double y2 = y * y;
    double ps = S[7], pc = C[7];
#pragma unroll 1
    for (int i = 6; i >= 0; --i) { ps = ps * y2 + S[i]; pc = pc * y2 + C[i]; }
    const double sy = y + y * y2 * ps, cy = 1.0 + y2 * pc;
    // k mod 4 without an integer: odd = k is odd; neg = (k - odd) / 2 is odd
    const double kh = k * 0.5;
    const bool odd = rint(kh) != kh;
    const double jh = (odd ? k - 1.0 : k) * 0.25;
    const bool neg = rint(jh) != jh;
    const double s0 = odd ? cy : sy, c0 = odd ? sy : cy;
    s = neg ? -s0 : s0;
    c = neg != odd ? -c0 : c0;
}

// EquidistantCamera::liftProjective: the ray (sin theta cos phi, sin theta sin phi, cos theta) of the pixel whose normalised
// position has the norm r = theta + k2 theta^3 + k3 theta^5 + k4 theta^7 + k5 theta^9.  theta: FE_KB_NEWTON Newton steps from
// theta = r, polynomial and derivative by Horner in theta^2; cos phi = ux / r, sin phi = uy / r ((1, 0) below the reference's 1e-10).
// Where r(theta) is monotone up to the pixel's theta this is the reference's smallest non-negative real root; beyond the first
// maximum of r(theta) it is whatever Newton reaches (include/vinsgpu.h).
FE_CAM_FN void fe_cam_lift_kb(const FeCamera& c, float px, float py, double& x, double& y, double& z) {
    const double mu = c.p[0], mv = c.p[1], u0 = c.p[2], v0 = c.p[3], k2 = c.p[4], k3 = c.p[5], k4 = c.p[6], k5 = c.p[7];
    const double ux = (1.0 / mu) * (double)px + (-u0 / mu), uy = (1.0 / mv) * (double)py + (-v0 / mv);
    const double r = sqrt(ux * ux + uy * uy);
    const double d2 = 3.0 * k2, d3 = 5.0 * k3, d4 = 7.0 * k4, d5 = 9.0 * k5;
    double th = r;
#pragma unroll 1
    for (int it = 0; it < FE_KB_NEWTON; ++it) {
        const double t2 = th * th;
        const double f = th * ((((k5 * t2 + k4) * t2 + k3) * t2 + k2) * t2 + 1.0) - r;
        const double df = (((d5 * t2 + d4) * t2 + d3) * t2 + d2) * t2 + 1.0;
        th = th - f / df;
    }
    double st, ct;
    fe_kb_sincos(th, st, ct);
    const bool centre = r < 1e-10;
    const double cphi = centre ? 1.0 : ux / r, sphi = centre ? 0.0 : uy / r;
    x = st * cphi; y = st * sphi; z = ct;
}

// pixel -> projective ray (x, y, z).  `c.model` is uniform wherever this is called from a kernel (one camera per stream, one workgroup
// or launch per stream): the model test is a scalar branch.  PINHOLE: z = 1.0.
FE_CAM_FN void fe_cam_lift(const FeCamera& c, float px, float py, double& x, double& y, double& z) {
    if (c.model == FE_CAM_KB) { fe_cam_lift_kb(c, px, py, x, y, z); return; }
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
    if (c.model != FE_CAM_PINHOLE) { ox = (float)(x / z); oy = (float)(y / z); }
    else { ox = (float)x; oy = (float)y; }
}

// a caller's vg_fe_camera (include/vinsgpu.h; a template so that this header needs no other) -> FeCamera, or the reason it is refused:
// the rules of vg_fe_set_camera, vg_fe_lift and vg_kf_add
template <typename VgCamera>
inline const char* fe_camera_check(const VgCamera* in, FeCamera* out) {
    if (in->struct_size != (int)sizeof(VgCamera)) return "struct_size is not sizeof(vg_fe_camera)";
    if (in->model != FE_CAM_PINHOLE && in->model != FE_CAM_MEI && in->model != FE_CAM_KB) return "unknown camera model";
    for (int i = 0; i < 8; ++i)
        if (!std::isfinite(in->p[i])) return "a camera parameter is not finite";
    if (in->model == FE_CAM_MEI && !std::isfinite(in->xi)) return "xi is not finite";
    if (in->p[0] == 0.0 || in->p[1] == 0.0) return "a zero focal length (p[0] / p[1])";
    out->model = in->model;
    for (int i = 0; i < 8; ++i) out->p[i] = in->p[i];
    out->xi = in->model == FE_CAM_MEI ? in->xi : 0.0;
    return nullptr;
}
