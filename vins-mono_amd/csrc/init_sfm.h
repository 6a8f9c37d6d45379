// init_sfm.h — device functions of init_sfm_kernel and init_sfm_frame_kernel (csrc/triangulate.hip: vg_init_sfm): GlobalSFM::construct
// (vins_estimator/src/initial/initial_sfm.cpp), cv::solvePnP's guess branch restated, the full BA (Ceres' trust-region loop with the
// LEVENBERG_MARQUARDT strategy, points eliminated first) and the per-frame PnP of Estimator::initialStructure (estimator.cpp:286-353),
// for ONE window run by the SFM_NT threads of ONE workgroup that owns the carve of init_sfm_carve.h.  include/vinsgpu.h is the
// definition; this file follows it statement by statement.
//
// Everything small is workgroup-uniform (every thread evaluates it from the same LDS words).  Feature j belongs to thread j mod SFM_NT in
// every pass; sums over features are taken per thread in ascending j, then over the 64 lanes by the DPP tree of ba_math.h, then over
// the wavefronts in ascending order: no atomics, the same bits run to run and in any batch.
#pragma once
#include "ba_math.h"
#include "init_sfm_carve.h"

#define SF_OK 0                 // VG_SFM_* of include/vinsgpu.h
#define SF_FAILED_PNP 1
#define SF_FAILED_BA 2
#define SF_FAILED_FRAME 3
#define SF_NUMERIC 4
#define SF_RES 8                // status | ba_iters | ba_termination | final_cost | pad
#define SF_FR 16                // per frame: q 4 | T 3 | q0 4 | T0 3 | pnp_iters | pnp_up
#define SF_FT 7                 // per feature: state | position 3 | position0 3
#define SF_TR 5                 // per BA iteration: cost | candidate cost | model cost change | radius | flags (1 valid, 2 accepted)
#define SF_AL 14                // per all_image_frame entry: R 9 | T 3 | is_key | status
#define SF_PAR 21               // relative_R 9 | relative_T 3 | ric 9
#define SF_WI 8                 // ints per window: F | l | n_feat | n_all | first feature | first observation | first frame | first entry

DEV bool sf_finite(double v) { return v > -1.79e308 && v < 1.79e308; }
DEV bool sf_pos_finite(double v) { return v > 0.0 && v < 1.79e308; }
DEV double sf_f32(double v) { return (double)(float)v; }      // cv::Point2f / Point3f

// ---- the workgroup reductions.  v[N] of every thread -> totals red[SFM_NW * SFM_NRED + i], the same in every thread's view after
// the call; two barriers, and the totals stay valid until the next call's first barrier
template <int N> DEV void sf_reduce(double* v, double* red, int tid) {
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = wave_sum_all(v[i]);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int i = 0; i < N; ++i) red[(tid >> 6) * SFM_NRED + i] = v[i];
    }
    __syncthreads();
    if (tid < N) {
        double s = red[tid];
        for (int w = 1; w < SFM_NW; ++w) s += red[w * SFM_NRED + tid];
        red[SFM_NW * SFM_NRED + tid] = s;
    }
    __syncthreads();
}
DEV double sf_total(const double* red, int i) { return red[SFM_NW * SFM_NRED + i]; }
DEV double sf_reduce_max(double v, double* red, int tid) {
    v = wave_max_all(v);
    if ((tid & 63) == 0) red[(tid >> 6) * SFM_NRED] = v;
    __syncthreads();
    if (tid == 0) {
        double s = red[0];
        for (int w = 1; w < SFM_NW; ++w) s = fmax(s, red[w * SFM_NRED]);
        red[SFM_NW * SFM_NRED] = s;
    }
    __syncthreads();
    return red[SFM_NW * SFM_NRED];
}

// ---- quaternions (w x y z), Eigen's conventions
DEV void sf_q_to_R(const double* q, double* R) { const double e[4] = {q[1], q[2], q[3], q[0]}; q_to_R(e, R); }
DEV void sf_R_to_q(const double* R, double* q) { double e[4]; R_to_q(R, e); q[0] = e[3]; q[1] = e[0]; q[2] = e[1]; q[3] = e[2]; }
DEV void sf_q_inverse(const double* q, double* o) {          // the conjugate over the squared norm
    const double n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    o[0] = q[0] / n2; o[1] = -q[1] / n2; o[2] = -q[2] / n2; o[3] = -q[3] / n2;
}
DEV void sf_q_mul(const double* a, const double* b, double* o) {
    o[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
    o[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
    o[2] = a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3];
    o[3] = a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1];
}

// ---- GlobalSFM::triangulatePoint (initial_sfm.cpp:5-19): the right singular vector of the 4x4 design matrix for the smallest singular
// value by a one-sided (Hestenes) Jacobi SVD on its columns, in registers, divided by its last component.  false: a coordinate is not
// finite
DEV bool sf_tri_point(const double* R0, const double* t0, const double* R1, const double* t1, const double* p0, const double* p1, double* X) {
    double D[16], V[16];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        D[c] = p0[0] * R0[6 + c] - R0[c];      D[4 + c] = p0[1] * R0[6 + c] - R0[3 + c];
        D[8 + c] = p1[0] * R1[6 + c] - R1[c];  D[12 + c] = p1[1] * R1[6 + c] - R1[3 + c];
    }
    D[3] = p0[0] * t0[2] - t0[0];  D[7] = p0[1] * t0[2] - t0[1];
    D[11] = p1[0] * t1[2] - t1[0]; D[15] = p1[1] * t1[2] - t1[1];
#pragma unroll
    for (int k = 0; k < 16; ++k) V[k] = (k % 5 == 0) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 60; ++sweep) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
                for (int r = 0; r < 4; ++r) { const double a = D[r * 4 + p], b = D[r * 4 + q]; alpha += a * a; beta += b * b; gamma += a * b; }
                if (gamma != 0.0 && fabs(gamma) > 1e-16 * sqrt(alpha * beta)) {
                    rotated = true;
                    const double zeta = (beta - alpha) / (2.0 * gamma);
                    const double tn = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                    const double c = 1.0 / sqrt(1.0 + tn * tn), s = c * tn;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const double a = D[r * 4 + p], b = D[r * 4 + q];
                        D[r * 4 + p] = c * a - s * b; D[r * 4 + q] = s * a + c * b;
                        const double va = V[r * 4 + p], vb = V[r * 4 + q];
                        V[r * 4 + p] = c * va - s * vb; V[r * 4 + q] = s * va + c * vb;
                    }
                }
            }
        if (!rotated) break;
    }
    double best = 0.0, v[4] = {0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        double s2 = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) s2 += D[r * 4 + c] * D[r * 4 + c];
        if (c == 0 || s2 < best) { best = s2; v[0] = V[c]; v[1] = V[4 + c]; v[2] = V[8 + c]; v[3] = V[12 + c]; }
    }
    X[0] = v[0] / v[3]; X[1] = v[1] / v[3]; X[2] = v[2] / v[3];
    return sf_finite(X[0]) && sf_finite(X[1]) && sf_finite(X[2]);
}

// ---- cv::Rodrigues, regular branches only
// matrix -> rvec; false in the near-pi branch (sin part below 1e-5 with a negative trace part)
DEV bool sf_rodrigues_R2r(const double* R, double* rv) {
    const double r[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
    const double s = sqrt((r[0] * r[0] + r[1] * r[1] + r[2] * r[2]) * 0.25);
    double c = (R[0] + R[4] + R[8] - 1.0) * 0.5;
    c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
    const double theta = acos(c);
    if (s < 1e-5) {
        if (!(c > 0)) return false;
        rv[0] = rv[1] = rv[2] = 0.0;
        return true;
    }
    const double vth = theta / (2.0 * s);
    rv[0] = r[0] * vth; rv[1] = r[1] * vth; rv[2] = r[2] * vth;
    return true;
}
// the Levi-Civita symbol of (a, b, i) in 0 .. 2: d [r]x[a][b] / d r_i = -eps(a, b, i)
DEV double sf_eps(int a, int b, int i) { return (double)((a - b) * (b - i) * (i - a) / 2); }
// rvec -> R and, with JAC, dR [3][9]: dR / d rvec_i
template <bool JAC> DEV void sf_rodrigues_r2R(const double* rv, double* R, double* dR) {
    const double theta = sqrt(rv[0] * rv[0] + rv[1] * rv[1] + rv[2] * rv[2]);
    if (theta < 2.220446049250313e-16) {
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                R[a * 3 + b] = (a == b) ? 1.0 : 0.0;
                if constexpr (JAC) {
#pragma unroll
                    for (int i = 0; i < 3; ++i) dR[i * 9 + a * 3 + b] = -sf_eps(a, b, i);
                }
            }
        return;
    }
    const double c = cos(theta), s = sin(theta), it = 1.0 / theta, c1 = 1.0 - c;
    const double r[3] = {rv[0] * it, rv[1] * it, rv[2] * it};
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const double rrt = r[a] * r[b], rx = -(sf_eps(a, b, 0) * r[0] + sf_eps(a, b, 1) * r[1] + sf_eps(a, b, 2) * r[2]);
            const double I = (a == b) ? 1.0 : 0.0;
            R[a * 3 + b] = c * I + c1 * rrt + s * rx;
            if constexpr (JAC) {
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const double ri = r[i];
                    const double a0 = -s * ri, a1 = (s - 2 * c1 * it) * ri, a2 = c1 * it, a3 = (c - s * it) * ri, a4 = s * it;
                    const double drrt = (a == i ? r[b] : 0.0) + (b == i ? r[a] : 0.0);
                    dR[i * 9 + a * 3 + b] = a0 * I + a1 * rrt + a2 * drrt + a3 * rx - a4 * sf_eps(a, b, i);
                }
            }
        }
}

// unpivoted LDL^T solve of the symmetric 6x6 system given by its lower triangle A[21] (row i at i (i + 1) / 2) with the diagonal
// multiplied by mul; false: a pivot is not a positive finite number
DEV bool sf_ldlt6(const double* A, double mul, const double* b, double* x) {
    double W[21];
#pragma unroll
    for (int k = 0; k < 21; ++k) W[k] = A[k];
#pragma unroll
    for (int i = 0; i < 6; ++i) W[SFM_TRI(i) + i] *= mul;
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const double d = W[SFM_TRI(j) + j];
        ok = ok && sf_pos_finite(d);
        double col[6];
#pragma unroll
        for (int i = j + 1; i < 6; ++i) col[i] = W[SFM_TRI(i) + j] / d;
#pragma unroll
        for (int i = j + 1; i < 6; ++i)
#pragma unroll
            for (int k = j + 1; k <= i; ++k) W[SFM_TRI(i) + k] -= W[SFM_TRI(i) + j] * col[k];
#pragma unroll
        for (int i = j + 1; i < 6; ++i) W[SFM_TRI(i) + j] = col[i];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) x[i] = b[i];
#pragma unroll
    for (int j = 0; j < 5; ++j)
#pragma unroll
        for (int i = j + 1; i < 6; ++i) x[i] -= W[SFM_TRI(i) + j] * x[j];
#pragma unroll
    for (int i = 0; i < 6; ++i) x[i] /= W[SFM_TRI(i) + i];
#pragma unroll
    for (int j = 5; j > 0; --j)
#pragma unroll
        for (int i = 0; i < j; ++i) x[i] -= W[SFM_TRI(j) + i] * x[j];
    return ok;
}

// ---- cv::solvePnP(..., useExtrinsicGuess, SOLVEPNP_ITERATIVE) as include/vinsgpu.h restates it, by the whole workgroup.
// point(k, P, p) -> bool: whether entry k of 0 .. n - 1 takes part, and its 3-D / 2-D point ALREADY rounded to float32.
// Rg, tg: the guess.  Returns SF_OK or SF_NUMERIC; R, t, iters, ups are uniform.
template <typename PointFn>
DEV int sf_pnp(double* red, int n, PointFn point, const double* Rg, const double* tg, double* R, double* t, int* iters_out, int* ups_out, int tid) {
    double par[6], prev[6];
    if (!sf_rodrigues_R2r(Rg, par)) return SF_NUMERIC;
    par[3] = tg[0]; par[4] = tg[1]; par[5] = tg[2];
    int k10 = -3, iters = 0, ups = 0;
    double prev_norm = 0.0;
    for (;;) {
        double dR[27], acc[28];
        sf_rodrigues_r2R<true>(par, R, dR);
#pragma unroll
        for (int i = 0; i < 28; ++i) acc[i] = 0.0;
        for (int k = tid; k < n; k += SFM_NT) {
            double P[3], p[2];
            if (!point(k, P, p)) continue;
            double X[3], J[12];
            m3_vec(R, P, X);
            X[0] += par[3]; X[1] += par[4]; X[2] += par[5];
            const double z = 1.0 / X[2], x = X[0] * z, y = X[1] * z;
            const double e0 = x - p[0], e1 = y - p[1];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                double dX[3];
                m3_vec(dR + 9 * i, P, dX);
                J[i] = z * (dX[0] - x * dX[2]);
                J[6 + i] = z * (dX[1] - y * dX[2]);
            }
            J[3] = z; J[4] = 0.0; J[5] = -x * z;
            J[9] = 0.0; J[10] = z; J[11] = -y * z;
#pragma unroll
            for (int a = 0; a < 6; ++a) {
#pragma unroll
                for (int b = 0; b <= a; ++b) acc[SFM_TRI(a) + b] += J[a] * J[b] + J[6 + a] * J[6 + b];
                acc[21 + a] += J[a] * e0 + J[6 + a] * e1;
            }
            acc[27] += e0 * e0 + e1 * e1;
        }
        sf_reduce<28>(acc, red, tid);
        double JtJ[21], Jte[6];
#pragma unroll
        for (int i = 0; i < 21; ++i) JtJ[i] = sf_total(red, i);
#pragma unroll
        for (int i = 0; i < 6; ++i) Jte[i] = sf_total(red, 21 + i);
        if (iters == 0) prev_norm = sqrt(sf_total(red, 27));
#pragma unroll
        for (int i = 0; i < 6; ++i) prev[i] = par[i];
        double nrm = 0.0;
        for (;;) {
            // step(): lambda = 10^k, the diagonal of JtJ times 1 + lambda, param = prevParam - solution
            double lam = 1.0, d[6];
            const int ak = k10 < 0 ? -k10 : k10;
            for (int i = 0; i < ak; ++i) lam *= 10.0;
            if (k10 < 0) lam = 1.0 / lam;
            if (!sf_ldlt6(JtJ, 1.0 + lam, Jte, d)) return SF_NUMERIC;
#pragma unroll
            for (int i = 0; i < 6; ++i) { par[i] = prev[i] - d[i]; if (!sf_finite(par[i])) return SF_NUMERIC; }
            sf_rodrigues_r2R<false>(par, R, nullptr);
            double e2[1] = {0.0};
            for (int k = tid; k < n; k += SFM_NT) {
                double P[3], p[2];
                if (!point(k, P, p)) continue;
                double X[3];
                m3_vec(R, P, X);
                X[0] += par[3]; X[1] += par[4]; X[2] += par[5];
                const double z = 1.0 / X[2], e0 = X[0] * z - p[0], e1 = X[1] * z - p[1];
                e2[0] += e0 * e0 + e1 * e1;
            }
            sf_reduce<1>(e2, red, tid);
            nrm = sqrt(sf_total(red, 0));
            if (!sf_finite(nrm)) return SF_NUMERIC;
            if (nrm > prev_norm) {
                ++k10;
                if (k10 <= 16) { ++ups; continue; }
            }
            break;
        }
        k10 = k10 - 1 < -16 ? -16 : k10 - 1;
        ++iters;
        double dd = 0.0, pp = 0.0;
#pragma unroll
        for (int i = 0; i < 6; ++i) { dd += (par[i] - prev[i]) * (par[i] - prev[i]); pp += prev[i] * prev[i]; }
        if (iters >= 20 || sqrt(dd) / (sqrt(pp) + 2.220446049250313e-16) < 1.1920928955078125e-07) break;
        prev_norm = nrm;
    }
    sf_rodrigues_r2R<false>(par, R, nullptr);
    t[0] = par[3]; t[1] = par[4]; t[2] = par[5];
    *iters_out = iters; *ups_out = ups;
    return SF_OK;
}

// ---- ReprojectionError3D (initial_sfm.h:25-54) with ceres::QuaternionRotatePoint, which normalises the quaternion, and the Jacobians
// auto-diff gives: Jc [2][6] (rotation through the 4x3 plus-Jacobian of QuaternionParameterization | translation), Jp [2][3]
DEV void sf_residual(const double* q, const double* t, const double* X, double u, double v, bool jac, double* r, double* Jc, double* Jp) {
    const double s = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double a = q[0] * s, b = q[1] * s, c = q[2] * s, d = q[3] * s;
    const double t2 = a * b, t3 = a * c, t4 = a * d, t5 = -b * b, t6 = b * c, t7 = b * d, t8 = -c * c, t9 = c * d, t1 = -d * d;
    const double Mx[9] = {t8 + t1, t6 - t4, t3 + t7, t4 + t6, t5 + t1, t9 - t2, t7 - t3, t2 + t9, t5 + t8};
    double p[3];
    m3_vec(Mx, X, p);
    p[0] = 2.0 * p[0] + X[0] + t[0]; p[1] = 2.0 * p[1] + X[1] + t[1]; p[2] = 2.0 * p[2] + X[2] + t[2];
    const double iz = 1.0 / p[2], xp = p[0] * iz, yp = p[1] * iz;
    r[0] = xp - u; r[1] = yp - v;
    if (!jac) return;
    const double X0 = X[0], X1 = X[1], X2 = X[2];
    // G [3][4] = d (2 M(u) X + X) / d u
    double G[12] = {2 * (c * X2 - d * X1), 2 * (c * X1 + d * X2), 2 * (-2 * c * X0 + b * X1 + a * X2), 2 * (-2 * d * X0 - a * X1 + b * X2),
                    2 * (d * X0 - b * X2), 2 * (c * X0 - 2 * b * X1 - a * X2), 2 * (b * X0 + d * X2), 2 * (a * X0 - 2 * d * X1 + c * X2),
                    2 * (b * X1 - c * X0), 2 * (d * X0 + a * X1 - 2 * b * X2), 2 * (-a * X0 + d * X1 - 2 * c * X2), 2 * (b * X0 + c * X1)};
    const double uq[4] = {a, b, c, d};
#pragma unroll
    for (int i = 0; i < 3; ++i) {                            // du / dq = s (I - u u^T)
        const double gu = G[4 * i] * a + G[4 * i + 1] * b + G[4 * i + 2] * c + G[4 * i + 3] * d;
#pragma unroll
        for (int k = 0; k < 4; ++k) G[4 * i + k] = s * (G[4 * i + k] - gu * uq[k]);
    }
    // the plus-Jacobian at the (unnormalised) q: rows [-x -y -z; w z -y; -z w x; y -x w]
    const double w_ = q[0], x_ = q[1], y_ = q[2], z_ = q[3];
    const double Pj[12] = {-x_, -y_, -z_, w_, z_, -y_, -z_, w_, x_, y_, -x_, w_};
    double GP[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) GP[3 * i + k] = G[4 * i] * Pj[k] + G[4 * i + 1] * Pj[3 + k] + G[4 * i + 2] * Pj[6 + k] + G[4 * i + 3] * Pj[9 + k];
    const double d02 = -xp * iz, d12 = -yp * iz;            // dr / dp = [iz 0 d02; 0 iz d12]
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        Jc[k] = iz * GP[k] + d02 * GP[6 + k];
        Jc[6 + k] = iz * GP[3 + k] + d12 * GP[6 + k];
        const double R0k = 2.0 * Mx[k] + (k == 0 ? 1.0 : 0.0), R1k = 2.0 * Mx[3 + k] + (k == 1 ? 1.0 : 0.0), R2k = 2.0 * Mx[6 + k] + (k == 2 ? 1.0 : 0.0);
        Jp[k] = iz * R0k + d02 * R2k;
        Jp[3 + k] = iz * R1k + d12 * R2k;
    }
    Jc[3] = iz; Jc[4] = 0.0; Jc[5] = d02;
    Jc[9] = 0.0; Jc[10] = iz; Jc[11] = d12;
}

// ceres::QuaternionParameterization::Plus
DEV void sf_quat_plus(const double* q, const double* d, double* o) {
    const double n = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    if (n > 0.0) {
        const double s = sin(n) / n;
        const double dq[4] = {cos(n), s * d[0], s * d[1], s * d[2]};
        sf_q_mul(dq, q, o);
    } else {
        o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; o[3] = q[3];
    }
}

// the window as the device sees it
struct SfWin {
    int F, l, n, n_all;
    const int *start, *nobs, *off;      // [n]; off: the feature's first row of obs
    const double* obs;                  // x y rows
    double *res, *fr, *ft, *tr;         // the output blocks of this window (SF_RES, [F] SF_FR, [n] SF_FT, [SFM_MAX_ITERS] SF_TR)
};

// reduced index of camera column (f, c), -1 when constant: the rotation of l, the translations of l and F - 1
DEV int sf_cidx(int f, int c, int l, int F) {
    if (f == l || (f == F - 1 && c >= 3)) return -1;
    return 6 * f + c - (f > l ? 6 : 0);
}
DEV bool sf_sees(const SfWin& w, int j, int f) { return f >= w.start[j] && f < w.start[j] + w.nobs[j]; }
DEV const double* sf_obs(const SfWin& w, int j, int f) { return w.obs + 2 * (size_t)(w.off[j] + f - w.start[j]); }

// triangulateTwoFrames (initial_sfm.cpp:74-110): features whose state is still false, seen in both frames.  false: a coordinate that is
// not finite (uniform)
DEV bool sf_two_frames(const SfWin& w, double* L, const SfmLds& c, int f0, int f1, int tid) {
    double bad[1] = {0.0};
    for (int j = tid; j < w.n; j += SFM_NT) {
        if (w.ft[SF_FT * j] != 0.0 || !sf_sees(w, j, f0) || !sf_sees(w, j, f1)) continue;
        double X[3];
        if (!sf_tri_point(L + c.cR + 9 * f0, L + c.ct + 3 * f0, L + c.cR + 9 * f1, L + c.ct + 3 * f1, sf_obs(w, j, f0), sf_obs(w, j, f1), X)) bad[0] += 1.0;
        w.ft[SF_FT * j] = 1.0;
        L[c.pos + 3 * j] = X[0]; L[c.pos + 3 * j + 1] = X[1]; L[c.pos + 3 * j + 2] = X[2];
    }
    sf_reduce<1>(bad, L + c.red, tid);
    return sf_total(L + c.red, 0) == 0.0;
}

// solveFrameByPnP (initial_sfm.cpp:22-72) of frame i from the pose of frame g
DEV int sf_chain_pnp(const SfWin& w, double* L, const SfmLds& c, int i, int g, int tid) {
    double cnt[1] = {0.0};
    for (int j = tid; j < w.n; j += SFM_NT)
        if (w.ft[SF_FT * j] != 0.0 && sf_sees(w, j, i)) cnt[0] += 1.0;
    sf_reduce<1>(cnt, L + c.red, tid);
    if (sf_total(L + c.red, 0) < 10.0) return SF_FAILED_PNP;
    double Rg[9], tg[3], R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) Rg[k] = L[c.cR + 9 * g + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) tg[k] = L[c.ct + 3 * g + k];
    int iters = 0, ups = 0;
    const double* pos = L + c.pos;
    const int st = sf_pnp(L + c.red, w.n, [&](int j, double* P, double* p) {
        if (w.ft[SF_FT * j] == 0.0 || !sf_sees(w, j, i)) return false;
        const double* o = sf_obs(w, j, i);
        P[0] = sf_f32(pos[3 * j]); P[1] = sf_f32(pos[3 * j + 1]); P[2] = sf_f32(pos[3 * j + 2]);
        p[0] = sf_f32(o[0]); p[1] = sf_f32(o[1]);
        return true;
    }, Rg, tg, R, t, &iters, &ups, tid);
    if (st != SF_OK) return st;
    __syncthreads();
    if (tid == 0) {
        double q[4];
        sf_R_to_q(R, q);
        for (int k = 0; k < 9; ++k) L[c.cR + 9 * i + k] = R[k];
        for (int k = 0; k < 3; ++k) L[c.ct + 3 * i + k] = t[k];
        for (int k = 0; k < 4; ++k) L[c.cq + 4 * i + k] = q[k];
        w.fr[SF_FR * i + 14] = (double)iters; w.fr[SF_FR * i + 15] = (double)ups;
    }
    __syncthreads();
    return SF_OK;
}

// ---- the linearisation at the current point.  mode 0: the Jacobi scales sc / sp from the unscaled column norms; mode 1: everything an
// iteration needs: vinv, gp (scaled), the diagonal blocks of S with D^2, gc (scaled).  Totals left by the last reduction are consumed
// here; returns through *cost, *xx (sum of squares of the free parameters), *bad (a point block that cannot be inverted).
DEV void sf_linearise(const SfWin& w, double* L, const SfmLds& c, int mode, double radius, double* cost, double* xx, bool* bad, int tid) {
    const int F = w.F, l = w.l;
    double acc3[3] = {0.0, 0.0, 0.0};
    if (mode == 1)                                          // (the blocks between different frames start from zero; the barriers of the
        for (int e = tid; e < SFM_TRI(SFM_NC(F)); e += SFM_NT) L[c.S + e] = 0.0;      //  reduction below come before the diagonal blocks are written)
    for (int j = tid; j < w.n; j += SFM_NT) {
        if (w.ft[SF_FT * j] == 0.0) continue;
        const double X[3] = {L[c.pos + 3 * j], L[c.pos + 3 * j + 1], L[c.pos + 3 * j + 2]};
        const double s0 = L[c.sp + 3 * j], s1 = L[c.sp + 3 * j + 1], s2 = L[c.sp + 3 * j + 2];
        double V[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0};
        const int f0 = w.start[j], nf = w.nobs[j];
        for (int k = 0; k < nf; ++k) {
            const int f = f0 + k;
            const double* o = sf_obs(w, j, f);
            double r[2], Jc[12], Jp[6];
            sf_residual(L + c.cq + 4 * f, L + c.ct + 3 * f, X, o[0], o[1], true, r, Jc, Jp);
            Jp[0] *= s0; Jp[1] *= s1; Jp[2] *= s2; Jp[3] *= s0; Jp[4] *= s1; Jp[5] *= s2;
            V[0] += Jp[0] * Jp[0] + Jp[3] * Jp[3];
            V[1] += Jp[1] * Jp[0] + Jp[4] * Jp[3]; V[2] += Jp[1] * Jp[1] + Jp[4] * Jp[4];
            V[3] += Jp[2] * Jp[0] + Jp[5] * Jp[3]; V[4] += Jp[2] * Jp[1] + Jp[5] * Jp[4]; V[5] += Jp[2] * Jp[2] + Jp[5] * Jp[5];
            g[0] += Jp[0] * r[0] + Jp[3] * r[1]; g[1] += Jp[1] * r[0] + Jp[4] * r[1]; g[2] += Jp[2] * r[0] + Jp[5] * r[1];
            acc3[0] += r[0] * r[0] + r[1] * r[1];
        }
        acc3[2] += X[0] * X[0] + X[1] * X[1] + X[2] * X[2];
        if (mode == 0) {
            L[c.sp + 3 * j] = 1.0 / (1.0 + sqrt(V[0])); L[c.sp + 3 * j + 1] = 1.0 / (1.0 + sqrt(V[2])); L[c.sp + 3 * j + 2] = 1.0 / (1.0 + sqrt(V[5]));
            continue;
        }
        L[c.gp + 3 * j] = g[0]; L[c.gp + 3 * j + 1] = g[1]; L[c.gp + 3 * j + 2] = g[2];
        // LM diagonal sqrt(clamp(diag, 1e-6, 1e32) / radius), added squared; then the inverse by the adjugate
        const double D0 = sqrt(fmin(fmax(V[0], 1e-6), 1e32) / radius), D1 = sqrt(fmin(fmax(V[2], 1e-6), 1e32) / radius), D2 = sqrt(fmin(fmax(V[5], 1e-6), 1e32) / radius);
        const double a = V[0] + D0 * D0, b = V[1], cc = V[2] + D1 * D1, d = V[3], e = V[4], f = V[5] + D2 * D2;
        const double c00 = cc * f - e * e, c10 = d * e - b * f, c20 = b * e - cc * d;
        const double det = a * c00 + b * c10 + d * c20;
        if (!sf_pos_finite(det)) acc3[1] += 1.0;
        double* vi = L + c.vinv + 6 * j;
        vi[0] = c00 / det; vi[1] = c10 / det; vi[2] = (a * f - d * d) / det; vi[3] = c20 / det; vi[4] = (b * d - a * e) / det; vi[5] = (a * cc - b * b) / det;
    }
    sf_reduce<3>(acc3, L + c.red, tid);
    *cost = sf_total(L + c.red, 0) / 2.0;
    *bad = sf_total(L + c.red, 1) != 0.0;
    double x2 = sf_total(L + c.red, 2);
    for (int f = 0; f < F; ++f) {
        if (f != l)
            for (int k = 0; k < 4; ++k) x2 += L[c.cq + 4 * f + k] * L[c.cq + 4 * f + k];
        if (f != l && f != F - 1)
            for (int k = 0; k < 3; ++k) x2 += L[c.ct + 3 * f + k] * L[c.ct + 3 * f + k];
    }
    *xx = x2;
    // ---- the camera blocks, frame by frame: 21 + 6 sums over the features that see the frame
    for (int f = 0; f < F; ++f) {
        double acc[27];
#pragma unroll
        for (int i = 0; i < 27; ++i) acc[i] = 0.0;
        double sc6[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) sc6[k] = L[c.sc + 6 * f + k];
        for (int j = tid; j < w.n; j += SFM_NT) {
            if (w.ft[SF_FT * j] == 0.0 || !sf_sees(w, j, f)) continue;
            const double* o = sf_obs(w, j, f);
            double r[2], Jc[12], Jp[6];
            sf_residual(L + c.cq + 4 * f, L + c.ct + 3 * f, L + c.pos + 3 * j, o[0], o[1], true, r, Jc, Jp);
#pragma unroll
            for (int k = 0; k < 6; ++k) { Jc[k] *= sc6[k]; Jc[6 + k] *= sc6[k]; }
#pragma unroll
            for (int a = 0; a < 6; ++a) {
#pragma unroll
                for (int b = 0; b <= a; ++b) acc[SFM_TRI(a) + b] += Jc[a] * Jc[b] + Jc[6 + a] * Jc[6 + b];
                acc[21 + a] += Jc[a] * r[0] + Jc[6 + a] * r[1];
            }
        }
        sf_reduce<27>(acc, L + c.red, tid);
        const double* tot = L + c.red + SFM_NW * SFM_NRED;
        if (mode == 0) {
            if (tid < 6) L[c.sc + 6 * f + tid] = 1.0 / (1.0 + sqrt(tot[SFM_TRI(tid) + tid]));
        } else {
            if (tid < 21) {
                int a, b;
                tri_decode(tid, a, b);
                const int ia = sf_cidx(f, a, l, F), ib = sf_cidx(f, b, l, F);
                if (ia >= 0 && ib >= 0) {
                    double v = tot[tid];
                    if (a == b) { const double D = sqrt(fmin(fmax(v, 1e-6), 1e32) / radius); v += D * D; }
                    L[c.S + SFM_TRI(ia) + ib] = v;
                }
            } else if (tid < 27) {
                L[c.gc + 6 * f + tid - 21] = tot[tid];
            }
        }
        // (the next reduction's first barrier comes after these reads)
    }
    __syncthreads();
}

// in-place Cholesky of the packed lower triangle S (n x n); false: a pivot is not a positive finite number (uniform)
DEV bool sf_cholesky(double* S, double* col, int n, int tid) {
    for (int j = 0; j < n; ++j) {
        const double d = S[SFM_TRI(j) + j];
        if (!sf_pos_finite(d)) return false;
        const double piv = sqrt(d);
        __syncthreads();                                    // (every thread has read the pivot before it is overwritten)
        for (int i = j + tid; i < n; i += SFM_NT) { const double v = (i == j) ? piv : S[SFM_TRI(i) + j] / piv; col[i] = v; S[SFM_TRI(i) + j] = v; }
        __syncthreads();
        const int m = n - 1 - j, cnt = SFM_TRI(m);
        for (int e = tid; e < cnt; e += SFM_NT) {
            int a, b;
            tri_decode(e, a, b);
            S[SFM_TRI(j + 1 + a) + j + 1 + b] -= col[j + 1 + a] * col[j + 1 + b];
        }
        __syncthreads();
    }
    return true;
}
// x <- (L L^T)^-1 x
DEV void sf_chol_solve(const double* S, double* x, int n, int tid) {
    for (int j = 0; j < n; ++j) {
        if (tid == 0) x[j] /= S[SFM_TRI(j) + j];
        __syncthreads();
        const double xj = x[j];
        for (int i = j + 1 + tid; i < n; i += SFM_NT) x[i] -= S[SFM_TRI(i) + j] * xj;
        __syncthreads();
    }
    for (int j = n - 1; j >= 0; --j) {
        if (tid == 0) x[j] /= S[SFM_TRI(j) + j];
        __syncthreads();
        const double xj = x[j];
        for (int i = tid; i < j; i += SFM_NT) x[i] -= S[SFM_TRI(j) + i] * xj;
        __syncthreads();
    }
}

// S -= sum_j W_j (V_j + D^2)^-1 W_j^T and rhs = gc - sum_j W_j (V_j + D^2)^-1 gp_j, feature after feature in ascending j: `ch` features are
// staged (W and Y = W Vinv of every frame of the span), then every thread takes the products of its own entries.  The coupling blocks
// are recomputed from the observations, not kept: at the capacity they would be 18 doubles for each of 16384 observations.
DEV void sf_schur(const SfWin& w, double* L, const SfmLds& c, int tid) {
    const int F = w.F, l = w.l, nc = SFM_NC(F), per = SFM_STAGE_PER(F), ntri = SFM_TRI(nc);
    for (int e = tid; e < nc; e += SFM_NT) { const int full = e < 6 * l ? e : e + 6; L[c.rhs + e] = L[c.gc + full]; }
    __syncthreads();
    for (int j0 = 0; j0 < w.n; j0 += c.ch) {
        const int nj = w.n - j0 < c.ch ? w.n - j0 : c.ch;
        // one thread per (staged feature, frame of its span)
        for (int e = tid; e < nj * F; e += SFM_NT) {
            const int cj = e / F, k = e - cj * F, j = j0 + cj;
            if (w.ft[SF_FT * j] == 0.0 || k >= w.nobs[j]) continue;
            const int f = w.start[j] + k;
            const double* o = sf_obs(w, j, f);
            double r[2], Jc[12], Jp[6];
            sf_residual(L + c.cq + 4 * f, L + c.ct + 3 * f, L + c.pos + 3 * j, o[0], o[1], true, r, Jc, Jp);
            const double* vi = L + c.vinv + 6 * j;
            const double Vi[9] = {vi[0], vi[1], vi[3], vi[1], vi[2], vi[4], vi[3], vi[4], vi[5]};
#pragma unroll
            for (int m = 0; m < 3; ++m) { const double s = L[c.sp + 3 * j + m]; Jp[m] *= s; Jp[3 + m] *= s; }
            double* Wd = L + c.stage + cj * per + 36 * k;
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                const double s = L[c.sc + 6 * f + a];
                const double ja = Jc[a] * s, jb = Jc[6 + a] * s;
                const double w0 = ja * Jp[0] + jb * Jp[3], w1 = ja * Jp[1] + jb * Jp[4], w2 = ja * Jp[2] + jb * Jp[5];
                Wd[3 * a] = w0; Wd[3 * a + 1] = w1; Wd[3 * a + 2] = w2;
#pragma unroll
                for (int m = 0; m < 3; ++m) Wd[18 + 3 * a + m] = w0 * Vi[m] + w1 * Vi[3 + m] + w2 * Vi[6 + m];
            }
        }
        __syncthreads();
        for (int e = tid; e < ntri + nc; e += SFM_NT) {
            int ia, ib = -1;
            if (e < ntri) tri_decode(e, ia, ib); else ia = e - ntri;
            const int fa_ = ia < 6 * l ? ia : ia + 6, fa = fa_ / 6, ra = fa_ - 6 * fa;
            int fb = 0, rb = 0;
            if (ib >= 0) { const int fb_ = ib < 6 * l ? ib : ib + 6; fb = fb_ / 6; rb = fb_ - 6 * fb; }
            double v = e < ntri ? L[c.S + e] : L[c.rhs + ia];
            for (int cj = 0; cj < nj; ++cj) {
                const int j = j0 + cj;
                if (w.ft[SF_FT * j] == 0.0 || !sf_sees(w, j, fa)) continue;
                const double* Y = L + c.stage + cj * per + 36 * (fa - w.start[j]) + 18 + 3 * ra;
                if (ib >= 0) {
                    if (!sf_sees(w, j, fb)) continue;
                    const double* Wb = L + c.stage + cj * per + 36 * (fb - w.start[j]) + 3 * rb;
                    v -= Y[0] * Wb[0] + Y[1] * Wb[1] + Y[2] * Wb[2];
                } else {
                    const double* g = L + c.gp + 3 * j;
                    v -= Y[0] * g[0] + Y[1] * g[1] + Y[2] * g[2];
                }
            }
            if (e < ntri) L[c.S + e] = v; else L[c.rhs + ia] = v;
        }
        __syncthreads();
    }
}

// GlobalSFM::construct up to the full BA, the BA, and the key entries of all_image_frame.  Returns the status (uniform).
DEV int sf_window(const SfWin& w, double* L, const double* par, const int* allkey, double* al, int tid) {
    const int F = w.F, l = w.l, n = w.n;
    const SfmLds c = sfm_lds(F, n);
    double* red = L + c.red;
    // ---- q[l] = identity, q[F - 1] = q[l] * Quaterniond(relative_R); the camera frames c_Quat = inverse, c_Translation = -(R T)
    if (tid == 0) {
        for (int ii = 0; ii < 2; ++ii) {
            const int i = ii ? F - 1 : l;
            double q[4] = {1.0, 0.0, 0.0, 0.0}, T[3] = {0.0, 0.0, 0.0}, cq[4], R[9], t[3];
            if (ii) {
                const double ql[4] = {1.0, 0.0, 0.0, 0.0};
                double qr[4];
                sf_R_to_q(par, qr);
                sf_q_mul(ql, qr, q);
                T[0] = par[9]; T[1] = par[10]; T[2] = par[11];
            }
            sf_q_inverse(q, cq);
            sf_q_to_R(cq, R);
            m3_vec(R, T, t);
            for (int k = 0; k < 4; ++k) L[c.cq + 4 * i + k] = cq[k];
            for (int k = 0; k < 9; ++k) L[c.cR + 9 * i + k] = R[k];
            for (int k = 0; k < 3; ++k) L[c.ct + 3 * i + k] = -t[k];
        }
    }
    __syncthreads();
    // ---- stages 1 and 2: PnP of l + 1 .. F - 2 along the chain, each triangulated with F - 1
    for (int i = l; i < F - 1; ++i) {
        if (i > l) { const int st = sf_chain_pnp(w, L, c, i, i - 1, tid); if (st != SF_OK) return st; }
        if (!sf_two_frames(w, L, c, i, F - 1, tid)) return SF_NUMERIC;
    }
    // ---- stage 3: l with l + 1 .. F - 2
    for (int i = l + 1; i < F - 1; ++i)
        if (!sf_two_frames(w, L, c, l, i, tid)) return SF_NUMERIC;
    // ---- stage 4: PnP of l - 1 .. 0, each triangulated with l
    for (int i = l - 1; i >= 0; --i) {
        const int st = sf_chain_pnp(w, L, c, i, i + 1, tid);
        if (st != SF_OK) return st;
        if (!sf_two_frames(w, L, c, i, l, tid)) return SF_NUMERIC;
    }
    // ---- stage 5: everything else with two observations or more, from its first and its LAST observation
    {
        double bad[1] = {0.0};
        for (int j = tid; j < n; j += SFM_NT) {
            if (w.ft[SF_FT * j] != 0.0 || w.nobs[j] < 2) continue;
            const int f0 = w.start[j], f1 = f0 + w.nobs[j] - 1;
            double X[3];
            if (!sf_tri_point(L + c.cR + 9 * f0, L + c.ct + 3 * f0, L + c.cR + 9 * f1, L + c.ct + 3 * f1, sf_obs(w, j, f0), sf_obs(w, j, f1), X)) bad[0] += 1.0;
            w.ft[SF_FT * j] = 1.0;
            L[c.pos + 3 * j] = X[0]; L[c.pos + 3 * j + 1] = X[1]; L[c.pos + 3 * j + 2] = X[2];
        }
        sf_reduce<1>(bad, red, tid);
        if (sf_total(red, 0) != 0.0) return SF_NUMERIC;
    }
    // ---- the taps: c_Quat, c_Translation and the positions right before the BA
    for (int e = tid; e < 7 * F; e += SFM_NT) {
        const int f = e / 7, k = e - 7 * f;
        w.fr[SF_FR * f + 7 + k] = k < 4 ? L[c.cq + 4 * f + k] : L[c.ct + 3 * f + k - 4];
    }
    for (int j = tid; j < n; j += SFM_NT) {
        const bool on = w.ft[SF_FT * j] != 0.0;
        for (int k = 0; k < 3; ++k) { if (!on) L[c.pos + 3 * j + k] = 0.0; w.ft[SF_FT * j + 4 + k] = L[c.pos + 3 * j + k]; }
        L[c.sp + 3 * j] = L[c.sp + 3 * j + 1] = L[c.sp + 3 * j + 2] = 1.0;
    }
    for (int e = tid; e < 6 * F; e += SFM_NT) L[c.sc + e] = 1.0;
    __syncthreads();                                        // (cR is dead from here on: S takes its place)
    // ---- the full BA
    const int nc = SFM_NC(F);
    double cost = 0.0, xx = 0.0, radius = 1e4, dec = 2.0;
    bool bad = false, check_grad = true;
    int it = 0, invalid = 0, term = 0;                      // VG_TERM_NO_CONVERGENCE
    sf_linearise(w, L, c, 0, radius, &cost, &xx, &bad, tid);
    for (;;) {
        sf_linearise(w, L, c, 1, radius, &cost, &xx, &bad, tid);
        if (check_grad) {
            // max |gradient|, unscaled, over the free columns
            double g = 0.0;
            for (int e = tid; e < nc; e += SFM_NT) { const int full = e < 6 * l ? e : e + 6; g = fmax(g, fabs(L[c.gc + full] / L[c.sc + full])); }
            for (int j = tid; j < n; j += SFM_NT) {
                if (w.ft[SF_FT * j] == 0.0) continue;
                for (int k = 0; k < 3; ++k) g = fmax(g, fabs(L[c.gp + 3 * j + k] / L[c.sp + 3 * j + k]));
            }
            if (sf_reduce_max(g, red, tid) <= 1e-10) { term = 1; break; }
            check_grad = false;
        }
        if (it >= SFM_MAX_ITERS) break;
        ++it;
        double* tr = w.tr + SF_TR * (it - 1);
        bool solved = !bad;
        if (solved) {
            sf_schur(w, L, c, tid);
            solved = sf_cholesky(L + c.S, L + c.col, nc, tid);
            if (solved) sf_chol_solve(L + c.S, L + c.rhs, nc, tid);
        }
        __syncthreads();
        // the step: -solution, unscaled (dcam takes gc's place); the candidate cameras
        for (int e = tid; e < 6 * F; e += SFM_NT) {
            const int f = e / 6, k = e - 6 * f, r = sf_cidx(f, k, l, F);
            L[c.dcam + e] = (r >= 0 && solved) ? -L[c.rhs + r] * L[c.sc + e] : 0.0;
        }
        __syncthreads();
        if (tid < F) {
            const int f = tid;
            if (f != l) sf_quat_plus(L + c.cq + 4 * f, L + c.dcam + 6 * f, L + c.cq2 + 4 * f);
            else for (int k = 0; k < 4; ++k) L[c.cq2 + 4 * f + k] = L[c.cq + 4 * f + k];
            for (int k = 0; k < 3; ++k) L[c.ct2 + 3 * f + k] = (f != l && f != F - 1) ? L[c.ct + 3 * f + k] + L[c.dcam + 6 * f + 3 + k] : L[c.ct + 3 * f + k];
        }
        __syncthreads();
        // back-substitution of the points, the model cost change -(J step) . (r + J step / 2) and the candidate's cost
        double acc[3] = {0.0, 0.0, 0.0};
        for (int j = tid; j < n && solved; j += SFM_NT) {
            if (w.ft[SF_FT * j] == 0.0) continue;
            const double X[3] = {L[c.pos + 3 * j], L[c.pos + 3 * j + 1], L[c.pos + 3 * j + 2]};
            const double sp3[3] = {L[c.sp + 3 * j], L[c.sp + 3 * j + 1], L[c.sp + 3 * j + 2]};
            const int f0 = w.start[j], nf = w.nobs[j];
            double tv[3] = {L[c.gp + 3 * j], L[c.gp + 3 * j + 1], L[c.gp + 3 * j + 2]};
            for (int k = 0; k < nf; ++k) {
                const int f = f0 + k;
                const double* o = sf_obs(w, j, f);
                double r[2], Jc[12], Jp[6];
                sf_residual(L + c.cq + 4 * f, L + c.ct + 3 * f, X, o[0], o[1], true, r, Jc, Jp);
                double v0 = 0.0, v1 = 0.0;                  // Jc_scaled * yc_f = -(Jc * dcam_f)
#pragma unroll
                for (int a = 0; a < 6; ++a) { const double y = -L[c.dcam + 6 * f + a]; v0 += Jc[a] * y; v1 += Jc[6 + a] * y; }
#pragma unroll
                for (int m = 0; m < 3; ++m) tv[m] -= (Jp[m] * v0 + Jp[3 + m] * v1) * sp3[m];
            }
            const double* vi = L + c.vinv + 6 * j;
            const double dp[3] = {-(vi[0] * tv[0] + vi[1] * tv[1] + vi[3] * tv[2]) * sp3[0], -(vi[1] * tv[0] + vi[2] * tv[1] + vi[4] * tv[2]) * sp3[1],
                                  -(vi[3] * tv[0] + vi[4] * tv[1] + vi[5] * tv[2]) * sp3[2]};
            L[c.gp + 3 * j] = dp[0]; L[c.gp + 3 * j + 1] = dp[1]; L[c.gp + 3 * j + 2] = dp[2];
            const double X2[3] = {X[0] + dp[0], X[1] + dp[1], X[2] + dp[2]};
            for (int k = 0; k < nf; ++k) {
                const int f = f0 + k;
                const double* o = sf_obs(w, j, f);
                double r[2], r2[2], Jc[12], Jp[6];
                sf_residual(L + c.cq + 4 * f, L + c.ct + 3 * f, X, o[0], o[1], true, r, Jc, Jp);
                double s0 = Jp[0] * dp[0] + Jp[1] * dp[1] + Jp[2] * dp[2], s1 = Jp[3] * dp[0] + Jp[4] * dp[1] + Jp[5] * dp[2];
#pragma unroll
                for (int a = 0; a < 6; ++a) { const double y = L[c.dcam + 6 * f + a]; s0 += Jc[a] * y; s1 += Jc[6 + a] * y; }
                acc[0] -= s0 * (r[0] + s0 / 2.0) + s1 * (r[1] + s1 / 2.0);
                sf_residual(L + c.cq2 + 4 * f, L + c.ct2 + 3 * f, X2, o[0], o[1], false, r2, nullptr, nullptr);
                acc[1] += r2[0] * r2[0] + r2[1] * r2[1];
            }
            acc[2] += (X[0] - X2[0]) * (X[0] - X2[0]) + (X[1] - X2[1]) * (X[1] - X2[1]) + (X[2] - X2[2]) * (X[2] - X2[2]);
        }
        sf_reduce<3>(acc, red, tid);
        const double model = sf_total(red, 0), cost2 = sf_total(red, 1) / 2.0;
        double dx2 = sf_total(red, 2);
        if (!solved || !(model > 0.0)) {
            if (tid == 0) { tr[0] = cost; tr[1] = 0.0; tr[2] = solved ? model : 0.0; tr[3] = radius; tr[4] = 0.0; }
            if (++invalid >= 5) { term = 2; break; }
            radius /= dec; dec *= 2.0;
            continue;
        }
        invalid = 0;
        for (int f = 0; f < F; ++f) {
            for (int k = 0; k < 4; ++k) { const double d = L[c.cq + 4 * f + k] - L[c.cq2 + 4 * f + k]; if (f != l) dx2 += d * d; }
            for (int k = 0; k < 3; ++k) { const double d = L[c.ct + 3 * f + k] - L[c.ct2 + 3 * f + k]; if (f != l && f != F - 1) dx2 += d * d; }
        }
        const double used = radius;
        int flags = 1;
        bool stop = false;
        if (sqrt(dx2) <= 1e-8 * (sqrt(xx) + 1e-8)) { term = 1; stop = true; }                  // parameter tolerance
        else if (fabs(cost - cost2) <= 1e-6 * cost) { term = 1; stop = true; }                 // function tolerance
        else {
            const double rho = (cost - cost2) / model;
            if (rho > 1e-3) {
                flags = 3;
                __syncthreads();
                for (int j = tid; j < n; j += SFM_NT) {
                    if (w.ft[SF_FT * j] == 0.0) continue;
                    for (int k = 0; k < 3; ++k) L[c.pos + 3 * j + k] += L[c.gp + 3 * j + k];
                }
                if (tid < F) {
                    for (int k = 0; k < 4; ++k) L[c.cq + 4 * tid + k] = L[c.cq2 + 4 * tid + k];
                    for (int k = 0; k < 3; ++k) L[c.ct + 3 * tid + k] = L[c.ct2 + 3 * tid + k];
                }
                __syncthreads();
                const double t = 2.0 * rho - 1.0;
                radius = fmin(radius / fmax(1.0 / 3.0, 1.0 - t * t * t), 1e16);
                dec = 2.0;
                check_grad = true;
            } else {
                radius /= dec; dec *= 2.0;
                if (radius < 1e-32) { term = 1; stop = true; }
            }
        }
        if (tid == 0) { tr[0] = cost; tr[1] = cost2; tr[2] = model; tr[3] = used; tr[4] = (double)flags; }
        if (stop) break;
    }
    __syncthreads();
    if (tid == 0) { w.res[1] = (double)it; w.res[2] = (double)term; w.res[3] = cost; }
    if (term != 1 && !(cost < 5e-3)) return SF_FAILED_BA;
    // ---- q[i] = inverse, T[i] = -(q[i] * c_t); positions; the key entries R = Q[i] ric^T, T = T[i]
    if (tid < F) {
        double q[4], R[9], t[3];
        sf_q_inverse(L + c.cq + 4 * tid, q);
        sf_q_to_R(q, R);
        m3_vec(R, L + c.ct + 3 * tid, t);
        for (int k = 0; k < 4; ++k) w.fr[SF_FR * tid + k] = q[k];
        for (int k = 0; k < 3; ++k) w.fr[SF_FR * tid + 4 + k] = -t[k];
    }
    for (int j = tid; j < n; j += SFM_NT)
        for (int k = 0; k < 3; ++k) w.ft[SF_FT * j + 1 + k] = L[c.pos + 3 * j + k];
    __syncthreads();
    for (int a = tid; a < w.n_all; a += SFM_NT) {
        const int i = allkey[a];
        if (i < 0) continue;
        double R[9], Ro[9];
        sf_q_to_R(w.fr + SF_FR * i, R);
        m3_mul_t(R, par + 12, Ro);
        double* o = al + SF_AL * a;
        for (int k = 0; k < 9; ++k) o[k] = Ro[k];
        for (int k = 0; k < 3; ++k) o[9 + k] = w.fr[SF_FR * i + 4 + k];
        o[12] = 1.0;
    }
    return SF_OK;
}

// One non-key entry of all_image_frame (estimator.cpp:302-352) by one workgroup: the guess is Q[g]^-1, -R T[g]; the points are the
// frame's ids found among the tracked features, in the frame's order; R = R_pnp^T ric^T, T = -R_pnp^T t.
// feat [npt]: the feature each id names, or -1; xy [npt][2].
DEV int sf_frame(double* red, int npt, const int* feat, const double* xy, const double* fr_g, const double* ft, const double* ric, double* o, int tid) {
    double cnt[1] = {0.0};
    for (int k = tid; k < npt; k += SFM_NT)
        if (feat[k] >= 0 && ft[SF_FT * feat[k]] != 0.0) cnt[0] += 1.0;
    sf_reduce<1>(cnt, red, tid);
    if (sf_total(red, 0) < 6.0) return SF_FAILED_FRAME;
    double qi[4], Rg[9], tg[3], R[9], t[3];
    sf_q_inverse(fr_g, qi);
    sf_q_to_R(qi, Rg);
    m3_vec(Rg, fr_g + 4, tg);
    tg[0] = -tg[0]; tg[1] = -tg[1]; tg[2] = -tg[2];
    int iters = 0, ups = 0;
    const int st = sf_pnp(red, npt, [&](int k, double* P, double* p) {
        const int j = feat[k];
        if (j < 0 || ft[SF_FT * j] == 0.0) return false;
        P[0] = sf_f32(ft[SF_FT * j + 1]); P[1] = sf_f32(ft[SF_FT * j + 2]); P[2] = sf_f32(ft[SF_FT * j + 3]);
        p[0] = sf_f32(xy[2 * k]); p[1] = sf_f32(xy[2 * k + 1]);
        return true;
    }, Rg, tg, R, t, &iters, &ups, tid);
    if (st != SF_OK) return st;
    if (tid == 0) {
        double Ro[9], Rt[9], T[3];
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) Rt[3 * a + b] = R[3 * b + a];
        m3_mul_t(Rt, ric, Ro);
        const double mt[3] = {-t[0], -t[1], -t[2]};
        m3_vec(Rt, mt, T);
        for (int k = 0; k < 9; ++k) o[k] = Ro[k];
        for (int k = 0; k < 3; ++k) o[9 + k] = T[k];
    }
    return SF_OK;
}
