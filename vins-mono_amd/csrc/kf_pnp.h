// kf_pnp.h — vg_kf_pnp: KeyFrame::PnPRANSAC (pose_graph/src/keyframe.cpp:200-256), the second reduceVector round and the loop_info gate of
// findConnection (:406-415, :472-516) for N pairs at once.  include/vinsgpu.h defines the call statement by statement (cv::solvePnPRansac
// RECALLED, NOT PINNED; the [FIXED] and [DEVIATION] parts are marked there); this file is its device code and its host entry.  Included
// behind kf_brief.h at the END of fe_ransac.hip: it uses that file's CvRng and update_num_iters and init_relpose.h's scratch block, and is
// compiled with -ffp-contract=off like the rest of the unit.
//
// Launches on the handle's stream between one upload and one download (VG_KF_PNP_LAUNCHES):
//   kp_sample_kernel   \  iterations [0, KP_CHUNK0) of every pair that runs: one EPnP model per group of 12 lanes (the 12 columns of M in
//   kp_count_kernel     > the one-sided Jacobi, five samples per wavefront), one wavefront per (pair, iteration) for the inlier count by
//   kp_pick_kernel     /  ballots, the registrator's sequential walk per pair; a second round of the three for [KP_CHUNK0, bound): the
//                         two-part scheme of vg_init_relpose (fe_ransac.hip has the argument why two parts give the outputs of one)
//   kp_tail_kernel     one workgroup per pair: the winner's mask by ballots, the ordered compaction (prefix counts, no atomics), the refit
//                      (sf_pnp of init_sfm.h over the inliers), the pose algebra, loop_info and the gate
// The schedule and the bound table depend on n alone: the host builds one of each per distinct n of the call and uploads them with the input.
#pragma once
#include "init_sfm.h"

#define KP_GROUP 12                 // lanes per sample: one per column of M
#define KP_PER_WAVE (64 / KP_GROUP) // 5 samples per wavefront; lanes 60 .. 63 idle
#define KP_CHUNK0 30                // iterations every running pair evaluates before the bookkeeping first looks (6 wavefronts of 5)
#define KP_P2_WAVES 16              // wavefronts per pair of the second part's sample kernel (each takes 5 iterations in turn)
#define KP_P2_COUNT 32              // wavefronts per pair of the second part's count kernel
#define KP_MODEL 8                  // doubles per model: rvec 3 | tvec 3 | valid | -
enum { KP_N = 0, KP_PT0, KP_SCHED, KP_TAB, KP_MAXIT, KP_MINLOOP, KP_REFINE, KP_RUN, KP_PI = 8 };     // ints per pair (input)
enum { KP_BEST = 0, KP_NITERS, KP_MAXGOOD, KP_NIN, KP_STATUS, KP_RIT, KP_RUP, KP_LOOP, KP_CTL = 8 };  // ints per pair (output)
#define KP_PAR 28                   // doubles per pair: thresh2 (a float, widened) | max_yaw | max_dist | origin_vio_T 3 | origin_vio_R 9 | tic 3 | qic 9 | -
#define KP_RES 32                   // doubles per pair: sample rvec 3 tvec 3 | rvec 3 tvec 3 | PnP_R_old 9 | PnP_T_old 3 | loop_info 8

struct KpDev {
    int P, stride, words_n;         // pairs, iterations a pair has room for, mask words a pair has room for
    const int* pi;                  // [P][KP_PI]
    const double* par;              // [P][KP_PAR]
    const float* p3;                // x y z rows of all pairs
    const float* p2;                // x y rows
    const int* tabs;                // the schedules [iterations][5] and bound tables [n + 1] of the distinct n, at pi[KP_SCHED] / pi[KP_TAB]
    int* ctl;                       // [P][KP_CTL]
    double* res;                    // [P][KP_RES]
    unsigned long long* mask;       // [P][words_n]
    int* midx;                      // matched_index, at the pair's first point
    double* models;                 // [P][stride][KP_MODEL]
    int* count;                     // [P][stride]
};

// what one sample keeps in LDS: everything that is indexed by a loop variable
struct KpLds {
    double pw[15], us[10], cw[12], al[20], v[48], L[60], rho[6], A[30], b[6], x[5], betas[4], ccs[12], pcs[15], m[9], mv[9], R[27], t[9];
};

// Utility::R2ypr(R).x() (utility.h:70-85), degrees
DEV double kp_yaw_deg(const double* R) { return atan2(R[3], R[0]) / M_PI * 180.0; }

// one-sided Jacobi of a 3x3 matrix in LDS (the rotation, threshold and sweep cap of rp_decompose): A V = U Sigma in place, columns then
// ordered by descending norm (stable); sv: the squared column norms
DEV void kp_jacobi3(double* A, double* V, double* sv) {
    for (int k = 0; k < 9; ++k) V[k] = (k % 4 == 0) ? 1.0 : 0.0;
    double fro = 0.0;
    for (int k = 0; k < 9; ++k) fro += A[k] * A[k];
    const double signal = 1e-26 * fro;
    bool conv = false;
    for (int sweep = 0; sweep < 40 && !conv; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                double al = 0.0, be = 0.0, ga = 0.0;
                for (int r = 0; r < 3; ++r) { const double x = A[3 * r + p], y = A[3 * r + q]; al += x * x; be += y * y; ga += x * y; }
                if (fabs(ga) > 1e-15 * sqrt(al * be) && ga != 0.0) {
                    rotated = rotated || (al > signal && be > signal);
                    const double zeta = (be - al) / (2.0 * ga);
                    const double tn = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                    const double cs = 1.0 / sqrt(1.0 + tn * tn), sn = cs * tn;
                    for (int r = 0; r < 3; ++r) {
                        const double x = A[3 * r + p], y = A[3 * r + q];
                        A[3 * r + p] = cs * x - sn * y; A[3 * r + q] = sn * x + cs * y;
                        const double vx = V[3 * r + p], vy = V[3 * r + q];
                        V[3 * r + p] = cs * vx - sn * vy; V[3 * r + q] = sn * vx + cs * vy;
                    }
                }
            }
        conv = !rotated;
    }
    for (int c = 0; c < 3; ++c) sv[c] = A[c] * A[c] + A[3 + c] * A[3 + c] + A[6 + c] * A[6 + c];
    for (int st = 0; st < 3; ++st) {
        const int a = st == 1 ? 1 : 0, b = a + 1;
        if (sv[b] > sv[a]) {
            const double ts = sv[a]; sv[a] = sv[b]; sv[b] = ts;
            for (int r = 0; r < 3; ++r) {
                const double x = A[3 * r + a]; A[3 * r + a] = A[3 * r + b]; A[3 * r + b] = x;
                const double y = V[3 * r + a]; V[3 * r + a] = V[3 * r + b]; V[3 * r + b] = y;
            }
        }
    }
}

// qr_solve of epnp.cpp for a 6 x nc system in LDS (A row-major with row length nc, overwritten; b overwritten); false: a column that is
// all zero
DEV bool kp_qr_solve(double* A, double* b, double* X, const int nc) {
    const int nr = 6;
    double A1[5], A2[5];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        double a1 = 0.0, a2 = 0.0;
        if (k < nc) {
            double mx = 0.0;
            for (int i = k; i < nr; ++i) { const double a = fabs(A[i * nc + k]); if (a > mx) mx = a; }
            if (mx == 0.0) ok = false;
            else {
                const double inv = 1.0 / mx;
                double sum = 0.0;
                for (int i = k; i < nr; ++i) { A[i * nc + k] *= inv; sum += A[i * nc + k] * A[i * nc + k]; }
                double sigma = sqrt(sum);
                if (A[k * nc + k] < 0) sigma = -sigma;
                A[k * nc + k] += sigma;
                a1 = sigma * A[k * nc + k]; a2 = -mx * sigma;
                for (int j = k + 1; j < nc; ++j) {
                    double s = 0.0;
                    for (int i = k; i < nr; ++i) s += A[i * nc + k] * A[i * nc + j];
                    const double tau = s / a1;
                    for (int i = k; i < nr; ++i) A[i * nc + j] -= tau * A[i * nc + k];
                }
            }
        }
        A1[k] = a1; A2[k] = a2;
    }
    if (!ok) return false;
#pragma unroll
    for (int j = 0; j < 5; ++j)
        if (j < nc) {
            double tau = 0.0;
            for (int i = j; i < nr; ++i) tau += A[i * nc + j] * b[i];
            tau /= A1[j];
            for (int i = j; i < nr; ++i) b[i] -= tau * A[i * nc + j];
        }
#pragma unroll
    for (int i = 4; i >= 0; --i)
        if (i < nc) {
            double s = 0.0;
            for (int j = i + 1; j < nc; ++j) s += A[i * nc + j] * X[j];
            X[i] = (b[i] - s) / A2[i];
        }
    return true;
}

// the columns c0 .. of L_6x10 against rho by qr_solve -> S.x
DEV bool kp_ls(KpLds& S, const int c0, const int c1, const int c2, const int c3, const int c4, const int nc) {
    for (int i = 0; i < 6; ++i) {
        S.A[i * nc] = S.L[10 * i + c0]; S.A[i * nc + 1] = S.L[10 * i + c1]; S.A[i * nc + 2] = S.L[10 * i + c2];
        if (nc > 3) S.A[i * nc + 3] = S.L[10 * i + c3];
        if (nc > 4) S.A[i * nc + 4] = S.L[10 * i + c4];
        S.b[i] = S.rho[i];
    }
    return kp_qr_solve(S.A, S.b, S.x, nc);
}

// gauss_newton (5 iterations) on S.betas
DEV bool kp_gauss_newton(KpLds& S) {
    for (int it = 0; it < 5; ++it) {
        const double b0 = S.betas[0], b1 = S.betas[1], b2 = S.betas[2], b3 = S.betas[3];
        for (int i = 0; i < 6; ++i) {
            const double* l = S.L + 10 * i;
            S.A[4 * i] = 2 * l[0] * b0 + l[1] * b1 + l[3] * b2 + l[6] * b3;
            S.A[4 * i + 1] = l[1] * b0 + 2 * l[2] * b1 + l[4] * b2 + l[7] * b3;
            S.A[4 * i + 2] = l[3] * b0 + l[4] * b1 + 2 * l[5] * b2 + l[8] * b3;
            S.A[4 * i + 3] = l[6] * b0 + l[7] * b1 + l[8] * b2 + 2 * l[9] * b3;
            S.b[i] = S.rho[i] - (l[0] * b0 * b0 + l[1] * b0 * b1 + l[2] * b1 * b1 + l[3] * b0 * b2 + l[4] * b1 * b2 + l[5] * b2 * b2 + l[6] * b0 * b3 +
                                 l[7] * b1 * b3 + l[8] * b2 * b3 + l[9] * b3 * b3);
        }
        if (!kp_qr_solve(S.A, S.b, S.x, 4)) return false;
        for (int i = 0; i < 4; ++i) S.betas[i] += S.x[i];
    }
    return true;
}

// compute_R_and_t -> S.R + 9 * slot, S.t + 3 * slot; returns reprojection_error
DEV double kp_R_and_t(KpLds& S, const int slot) {
    double* R = S.R + 9 * slot;
    double* t = S.t + 3 * slot;
    for (int k = 0; k < 12; ++k) S.ccs[k] = 0.0;
    for (int i = 0; i < 4; ++i)
        for (int k = 0; k < 12; ++k) S.ccs[k] += S.betas[i] * S.v[12 * i + k];
    for (int i = 0; i < 5; ++i)
        for (int j = 0; j < 3; ++j)
            S.pcs[3 * i + j] = S.al[4 * i] * S.ccs[j] + S.al[4 * i + 1] * S.ccs[3 + j] + S.al[4 * i + 2] * S.ccs[6 + j] + S.al[4 * i + 3] * S.ccs[9 + j];
    if (S.pcs[2] < 0.0) {                                       // solve_for_sign
        for (int k = 0; k < 12; ++k) S.ccs[k] = -S.ccs[k];
        for (int k = 0; k < 15; ++k) S.pcs[k] = -S.pcs[k];
    }
    double pc0[3] = {0.0, 0.0, 0.0}, pw0[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < 5; ++i) {
        pc0[0] += S.pcs[3 * i]; pc0[1] += S.pcs[3 * i + 1]; pc0[2] += S.pcs[3 * i + 2];
        pw0[0] += S.pw[3 * i]; pw0[1] += S.pw[3 * i + 1]; pw0[2] += S.pw[3 * i + 2];
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) { pc0[j] /= 5.0; pw0[j] /= 5.0; }
    for (int k = 0; k < 9; ++k) S.m[k] = 0.0;
    for (int i = 0; i < 5; ++i) {
        const double w0 = S.pw[3 * i] - pw0[0], w1 = S.pw[3 * i + 1] - pw0[1], w2 = S.pw[3 * i + 2] - pw0[2];
        const double c0 = S.pcs[3 * i] - pc0[0], c1 = S.pcs[3 * i + 1] - pc0[1], c2 = S.pcs[3 * i + 2] - pc0[2];
        S.m[0] += c0 * w0; S.m[1] += c0 * w1; S.m[2] += c0 * w2;
        S.m[3] += c1 * w0; S.m[4] += c1 * w1; S.m[5] += c1 * w2;
        S.m[6] += c2 * w0; S.m[7] += c2 * w1; S.m[8] += c2 * w2;
    }
    double sv[3];
    kp_jacobi3(S.m, S.mv, sv);
    for (int c = 0; c < 3; ++c) {                                // U: the normalised columns
        const double nn = sqrt(c == 0 ? sv[0] : (c == 1 ? sv[1] : sv[2]));
        for (int r = 0; r < 3; ++r) S.m[3 * r + c] = S.m[3 * r + c] / nn;
    }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[3 * i + j] = S.m[3 * i] * S.mv[3 * j] + S.m[3 * i + 1] * S.mv[3 * j + 1] + S.m[3 * i + 2] * S.mv[3 * j + 2];
    const double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] - R[2] * R[4] * R[6] - R[1] * R[3] * R[8] - R[0] * R[5] * R[7];
    if (det < 0) { R[6] = -R[6]; R[7] = -R[7]; R[8] = -R[8]; }
    for (int i = 0; i < 3; ++i) t[i] = (i == 0 ? pc0[0] : (i == 1 ? pc0[1] : pc0[2])) - (R[3 * i] * pw0[0] + R[3 * i + 1] * pw0[1] + R[3 * i + 2] * pw0[2]);
    double sum = 0.0;
    for (int i = 0; i < 5; ++i) {
        const double* pw = S.pw + 3 * i;
        const double Xc = R[0] * pw[0] + R[1] * pw[1] + R[2] * pw[2] + t[0], Yc = R[3] * pw[0] + R[4] * pw[1] + R[5] * pw[2] + t[1];
        const double iz = 1.0 / (R[6] * pw[0] + R[7] * pw[1] + R[8] * pw[2] + t[2]);
        const double du = S.us[2 * i] - Xc * iz, dv = S.us[2 * i + 1] - Yc * iz;
        sum += sqrt(du * du + dv * dv);
    }
    return sum / 5.0;
}

// a vector's largest-magnitude entry made positive (lowest index on a tie)
DEV void kp_sign(double* v, const int n) {
    double m = 0.0;
    for (int e = 0; e < n; ++e) if (fabs(v[e]) > fabs(m)) m = v[e];
    if (m < 0.0) for (int e = 0; e < n; ++e) v[e] = -v[e];
}

// choose_control_points and compute_barycentric_coordinates of the sample in S.pw; false: the control-point matrix cannot be inverted
DEV bool kp_control_points(KpLds& S) {
    double c0[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < 5; ++i) { c0[0] += S.pw[3 * i]; c0[1] += S.pw[3 * i + 1]; c0[2] += S.pw[3 * i + 2]; }
#pragma unroll
    for (int j = 0; j < 3; ++j) { c0[j] /= 5.0; S.cw[j] = c0[j]; }
    for (int k = 0; k < 9; ++k) S.m[k] = 0.0;
    for (int i = 0; i < 5; ++i) {
        const double d0 = S.pw[3 * i] - c0[0], d1 = S.pw[3 * i + 1] - c0[1], d2 = S.pw[3 * i + 2] - c0[2];
        S.m[0] += d0 * d0; S.m[1] += d0 * d1; S.m[2] += d0 * d2;
        S.m[3] += d1 * d0; S.m[4] += d1 * d1; S.m[5] += d1 * d2;
        S.m[6] += d2 * d0; S.m[7] += d2 * d1; S.m[8] += d2 * d2;
    }
    double sv[3];
    kp_jacobi3(S.m, S.mv, sv);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double e[3] = {S.mv[i], S.mv[3 + i], S.mv[6 + i]};
        double m = 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) if (fabs(e[j]) > fabs(m)) m = e[j];
        const double sg = m < 0.0 ? -1.0 : 1.0;
        const double k = sqrt(sqrt(sv[i]) / 5.0);
#pragma unroll
        for (int j = 0; j < 3; ++j) S.cw[3 * (i + 1) + j] = c0[j] + k * (sg * e[j]);
    }
    // CC[i][j - 1] = cws[j][i] - cws[0][i]; its inverse by cofactors over the determinant
    double C[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) C[3 * i + j] = S.cw[3 * (j + 1) + i] - S.cw[i];
    const double k00 = C[4] * C[8] - C[5] * C[7], k01 = C[5] * C[6] - C[3] * C[8], k02 = C[3] * C[7] - C[4] * C[6];
    const double det = C[0] * k00 + C[1] * k01 + C[2] * k02;
    if (det == 0.0 || !sf_finite(det)) return false;
    const double id = 1.0 / det;
    const double I0 = k00 * id, I1 = (C[2] * C[7] - C[1] * C[8]) * id, I2 = (C[1] * C[5] - C[2] * C[4]) * id;
    const double I3 = k01 * id, I4 = (C[0] * C[8] - C[2] * C[6]) * id, I5 = (C[2] * C[3] - C[0] * C[5]) * id;
    const double I6 = k02 * id, I7 = (C[1] * C[6] - C[0] * C[7]) * id, I8 = (C[0] * C[4] - C[1] * C[3]) * id;
    for (int i = 0; i < 5; ++i) {
        const double d0 = S.pw[3 * i] - S.cw[0], d1 = S.pw[3 * i + 1] - S.cw[1], d2 = S.pw[3 * i + 2] - S.cw[2];
        const double a1 = I0 * d0 + I1 * d1 + I2 * d2, a2 = I3 * d0 + I4 * d1 + I5 * d2, a3 = I6 * d0 + I7 * d1 + I8 * d2;
        S.al[4 * i] = 1.0 - a1 - a2 - a3; S.al[4 * i + 1] = a1; S.al[4 * i + 2] = a2; S.al[4 * i + 3] = a3;
    }
    return true;
}

// everything of compute_pose behind the eigenvectors (S.v: v1 .. v4 as the Jacobi left them) -> model[KP_MODEL]
DEV void kp_solve(KpLds& S, double* model) {
    // the canonical basis of the null plane, then the signs
    {
        double* a = S.v;
        double* b = S.v + 12;
        int k = 0;
        double best = -1.0;
        for (int e = 0; e < 12; ++e) { const double s = a[e] * a[e] + b[e] * b[e]; if (s > best) { best = s; k = e; } }
        const double ak = a[k], bk = b[k], r = sqrt(best);
        for (int e = 0; e < 12; ++e) {
            const double x = a[e], y = b[e];
            a[e] = (bk * x - ak * y) / r; b[e] = (ak * x + bk * y) / r;
        }
        a[k] = 0.0;
        for (int i = 0; i < 4; ++i) kp_sign(S.v + 12 * i, 12);
    }
    // compute_L_6x10 (dv[i][pair] = v_i at control point a minus v_i at control point b, pairs 01 02 03 12 13 23), compute_rho
    {
        int a = 0, b = 1;
        for (int pr = 0; pr < 6; ++pr) {
            double d[4][3];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int k = 0; k < 3; ++k) d[i][k] = S.v[12 * i + 3 * a + k] - S.v[12 * i + 3 * b + k];
#define KP_DOT(p, q) (d[p][0] * d[q][0] + d[p][1] * d[q][1] + d[p][2] * d[q][2])
            double* row = S.L + 10 * pr;
            row[0] = KP_DOT(0, 0); row[1] = 2.0 * KP_DOT(0, 1); row[2] = KP_DOT(1, 1); row[3] = 2.0 * KP_DOT(0, 2); row[4] = 2.0 * KP_DOT(1, 2);
            row[5] = KP_DOT(2, 2); row[6] = 2.0 * KP_DOT(0, 3); row[7] = 2.0 * KP_DOT(1, 3); row[8] = 2.0 * KP_DOT(2, 3); row[9] = KP_DOT(3, 3);
#undef KP_DOT
            const double r0 = S.cw[3 * a] - S.cw[3 * b], r1 = S.cw[3 * a + 1] - S.cw[3 * b + 1], r2 = S.cw[3 * a + 2] - S.cw[3 * b + 2];
            S.rho[pr] = r0 * r0 + r1 * r1 + r2 * r2;
            ++b;
            if (b > 3) { ++a; b = a + 1; }
        }
    }
    bool ok = true;
    double err0 = 0.0, err1 = 0.0, err2 = 0.0;
    // find_betas_approx_1: B11 B12 B13 B14
    ok = kp_ls(S, 0, 1, 3, 6, 0, 4);
    if (ok) {
        const double sg = S.x[0] < 0 ? -1.0 : 1.0;
        S.betas[0] = sqrt(sg * S.x[0]);
        S.betas[1] = sg * S.x[1] / S.betas[0]; S.betas[2] = sg * S.x[2] / S.betas[0]; S.betas[3] = sg * S.x[3] / S.betas[0];
        ok = kp_gauss_newton(S);
        if (ok) err0 = kp_R_and_t(S, 0);
    }
    // find_betas_approx_2: B11 B12 B22;  _3: B11 B12 B22 B13 B23
    for (int ap = 1; ap < 3 && ok; ++ap) {
        ok = kp_ls(S, 0, 1, 2, 3, 4, ap == 1 ? 3 : 5);
        if (!ok) break;
        if (S.x[0] < 0) { S.betas[0] = sqrt(-S.x[0]); S.betas[1] = S.x[2] < 0 ? sqrt(-S.x[2]) : 0.0; }
        else { S.betas[0] = sqrt(S.x[0]); S.betas[1] = S.x[2] > 0 ? sqrt(S.x[2]) : 0.0; }
        if (S.x[1] < 0) S.betas[0] = -S.betas[0];
        S.betas[2] = ap == 1 ? 0.0 : S.x[3] / S.betas[0];
        S.betas[3] = 0.0;
        ok = kp_gauss_newton(S);
        if (ok) { const double e = kp_R_and_t(S, ap); if (ap == 1) err1 = e; else err2 = e; }
    }
    int N = 0;
    if (err1 < err0) N = 1;
    if (err2 < (N == 1 ? err1 : err0)) N = 2;
    double rv[3] = {0.0, 0.0, 0.0};
    ok = ok && sf_rodrigues_R2r(S.R + 9 * N, rv);
    const double* t = S.t + 3 * N;
    ok = ok && sf_finite(rv[0]) && sf_finite(rv[1]) && sf_finite(rv[2]) && sf_finite(t[0]) && sf_finite(t[1]) && sf_finite(t[2]) &&
         sf_finite(err0) && sf_finite(err1) && sf_finite(err2);
    model[0] = ok ? rv[0] : 0.0; model[1] = ok ? rv[1] : 0.0; model[2] = ok ? rv[2] : 0.0;
    model[3] = ok ? t[0] : 0.0; model[4] = ok ? t[1] : 0.0; model[5] = ok ? t[2] : 0.0;
    model[6] = ok ? 1.0 : 0.0; model[7] = 0.0;
}

// end of the iterations of a launch: `end`, cut to the pair's max_iters and, behind the first part, to the bound it left
DEV int kp_end(const int* pi, const int* ctl, const int first, int end) {
    if (first > 0 && ctl[KP_NITERS] < end) end = ctl[KP_NITERS];
    return pi[KP_MAXIT] < end ? pi[KP_MAXIT] : end;
}

extern "C" __global__ __launch_bounds__(64) void kp_sample_kernel(KpDev b, int first, int end) {
    __shared__ KpLds lds[KP_PER_WAVE];
    __shared__ int okc[KP_PER_WAVE];
    const int pair = blockIdx.y;
    const int* pi = b.pi + (size_t)pair * KP_PI;
    if (pi[KP_RUN] == 0) return;
    const int lane = threadIdx.x, g = lane / KP_GROUP, c = lane - KP_GROUP * g;
    const bool member = g < KP_PER_WAVE;
    const int gb = member ? KP_GROUP * g : 0;              // first lane of the group (lanes 60 .. 63 read group 0's lanes; their results are dropped)
    KpLds& S = lds[member ? g : 0];
    const int nsched = kp_end(pi, b.ctl + (size_t)pair * KP_CTL, first, end);
    const int* __restrict__ sched = b.tabs + pi[KP_SCHED];
    const float* __restrict__ p3 = b.p3 + 3 * (size_t)pi[KP_PT0];
    const float* __restrict__ p2 = b.p2 + 2 * (size_t)pi[KP_PT0];
    double* __restrict__ models = b.models + (size_t)pair * b.stride * KP_MODEL;
#pragma unroll 1
    for (int k0 = first + blockIdx.x * KP_PER_WAVE; k0 < nsched; k0 += gridDim.x * KP_PER_WAVE) {
        const int k = k0 + g;
        const bool live = member && k < nsched;
        if (live && c == 0) {
            for (int i = 0; i < 5; ++i) {
                const int id = sched[(size_t)k * 5 + i];
                S.pw[3 * i] = p3[3 * id]; S.pw[3 * i + 1] = p3[3 * id + 1]; S.pw[3 * i + 2] = p3[3 * id + 2];
                S.us[2 * i] = p2[2 * id]; S.us[2 * i + 1] = p2[2 * id + 1];
            }
            okc[g] = kp_control_points(S) ? 1 : 0;
        }
        __syncthreads();
        // column c of M (rows 2i, 2i + 1 of point i: [a_j, 0, -a_j u], [0, a_j, -a_j v] at control point j = c / 3) and of the identity
        const bool run = live && okc[member ? g : 0] != 0;
        double a[10], v[12];
        {
            const int j = c / 3, m = c - 3 * j;
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const double aj = run ? S.al[4 * i + j] : 0.0, u = run ? S.us[2 * i] : 0.0, w = run ? S.us[2 * i + 1] : 0.0;
                a[2 * i] = m == 0 ? aj : (m == 1 ? 0.0 : aj * (0.0 - u));
                a[2 * i + 1] = m == 0 ? 0.0 : (m == 1 ? aj : aj * (0.0 - w));
            }
        }
#pragma unroll
        for (int e = 0; e < 12; ++e) v[e] = (e == c) ? 1.0 : 0.0;
        double scale2 = 0.0, nn = 0.0;
#pragma unroll
        for (int r = 0; r < 10; ++r) nn += a[r] * a[r];
#pragma unroll
        for (int q = 0; q < KP_GROUP; ++q) scale2 += __shfl(nn, gb + q);
        const double signal = 1e-26 * scale2;
        const unsigned long long gmask = 0xfffull << gb;
        bool active = run;                                  // (uniform over the group)
        for (int sweep = 0; sweep < 40; ++sweep) {
            bool rotated = false;
#pragma unroll 1
            for (int rd = 0; rd < KP_GROUP; ++rd) {
                int p = rd - c;
                p = p < 0 ? p + KP_GROUP : p;
                const bool lo = c < p;
                double bb[10], w[12];
#pragma unroll
                for (int r = 0; r < 10; ++r) bb[r] = __shfl(a[r], gb + p);
#pragma unroll
                for (int e = 0; e < 12; ++e) w[e] = __shfl(v[e], gb + p);
                // (al, be, ga) of the pair as the column with the smaller index sees them: both lanes form the same sums
                double al = 0.0, be = 0.0, ga = 0.0;
#pragma unroll
                for (int r = 0; r < 10; ++r) {
                    const double x = lo ? a[r] : bb[r], y = lo ? bb[r] : a[r];
                    al += x * x; be += y * y; ga += x * y;
                }
                if (active && p != c && fabs(ga) > 1e-15 * sqrt(al * be) && ga != 0.0) {
                    rotated = rotated || (al > signal && be > signal);
                    const double zeta = (be - al) / (2.0 * ga);
                    const double tn = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                    const double cs = 1.0 / sqrt(1.0 + tn * tn), sn = cs * tn;
#pragma unroll
                    for (int r = 0; r < 10; ++r) a[r] = lo ? cs * a[r] - sn * bb[r] : sn * bb[r] + cs * a[r];
#pragma unroll
                    for (int e = 0; e < 12; ++e) v[e] = lo ? cs * v[e] - sn * w[e] : sn * w[e] + cs * v[e];
                }
            }
            const unsigned long long bal = __ballot(rotated);      // (every lane takes part, whatever its group's state)
            active = active && (bal & gmask) != 0ull;
            if (!__any(active)) break;
        }
        // the four columns of the smallest norms, ascending (lowest index on a tie): rank of this lane's column among the group's
        nn = 0.0;
#pragma unroll
        for (int r = 0; r < 10; ++r) nn += a[r] * a[r];
        int rank = 0;
#pragma unroll
        for (int q = 0; q < KP_GROUP; ++q) {
            const double o = __shfl(nn, gb + q);
            rank += (o < nn || (o == nn && q < c)) ? 1 : 0;
        }
        if (run && rank < 4)
#pragma unroll
            for (int e = 0; e < 12; ++e) S.v[12 * rank + e] = v[e];
        __syncthreads();
        if (live && c == 0) {
            double* model = models + (size_t)k * KP_MODEL;
            if (run) kp_solve(S, model);
            else
                for (int e = 0; e < KP_MODEL; ++e) model[e] = 0.0;
        }
        __syncthreads();
    }
}

// error of step 3 for one point; R: Rodrigues(rvec)
DEV float kp_error(const double* R, const double* t, const float* P, const float* q) {
    const double Pd[3] = {(double)P[0], (double)P[1], (double)P[2]};
    double X[3];
    m3_vec(R, Pd, X);
    X[0] += t[0]; X[1] += t[1]; X[2] += t[2];
    const double z = X[2] != 0.0 ? 1.0 / X[2] : 1.0;
    const float px = (float)(X[0] * z), py = (float)(X[1] * z);
    const float dx = px - q[0], dy = py - q[1];
    return (float)((double)dx * (double)dx + (double)dy * (double)dy);
}

extern "C" __global__ __launch_bounds__(64) void kp_count_kernel(KpDev b, int first, int end) {
    const int pair = blockIdx.y, lane = threadIdx.x;
    const int* pi = b.pi + (size_t)pair * KP_PI;
    if (pi[KP_RUN] == 0) return;
    const int n = pi[KP_N];
    const float* __restrict__ p3 = b.p3 + 3 * (size_t)pi[KP_PT0];
    const float* __restrict__ p2 = b.p2 + 2 * (size_t)pi[KP_PT0];
    const float thresh2 = (float)b.par[(size_t)KP_PAR * pair];
    end = kp_end(pi, b.ctl + (size_t)pair * KP_CTL, first, end);
#pragma unroll 1
    for (int k = first + blockIdx.x; k < end; k += gridDim.x) {
        const double* model = b.models + ((size_t)pair * b.stride + k) * KP_MODEL;
        int cnt = -1;
        if (model[6] != 0.0) {
            double R[9];
            const double rv[3] = {model[0], model[1], model[2]}, t[3] = {model[3], model[4], model[5]};
            sf_rodrigues_r2R<false>(rv, R, nullptr);
            cnt = 0;
            for (int i0 = 0; i0 < n; i0 += 64) {
                const int i = i0 + lane;
                const bool in = i < n && kp_error(R, t, p3 + 3 * (i < n ? i : 0), p2 + 2 * (i < n ? i : 0)) <= thresh2;
                cnt += __popcll(__ballot(in));
            }
        }
        if (lane == 0) b.count[(size_t)pair * b.stride + k] = cnt;
    }
}

// The registrator's loop over the iterations [it0, stop) (rp_pick_kernel with 5 model points), one wavefront per pair
extern "C" __global__ __launch_bounds__(64) void kp_pick_kernel(KpDev b, int it0, int stop) {
    const int pair = blockIdx.x, lane = threadIdx.x;
    if (pair >= b.P) return;
    const int* pi = b.pi + (size_t)pair * KP_PI;
    if (pi[KP_RUN] == 0) return;
    int* ctl = b.ctl + (size_t)pair * KP_CTL;
    const int* count = b.count + (size_t)pair * b.stride;
    const int* tab = b.tabs + pi[KP_TAB];
    int niters = pi[KP_MAXIT], max_good = 0, best = -1;
    if (it0 > 0) { niters = ctl[KP_NITERS]; max_good = ctl[KP_MAXGOOD]; best = ctl[KP_BEST]; }
    if (stop > pi[KP_MAXIT]) stop = pi[KP_MAXIT];
    for (int base = it0; base < stop && base < niters; base += 64) {
        // (only what the count kernel wrote is read: it evaluated the iterations below the bound this walk starts from, and the bound only shrinks)
        const int mine = (base + lane < stop && base + lane < niters) ? count[base + lane] : -1;
        for (int j = 0; j < 64 && base + j < niters && base + j < stop; ++j) {
            const int c = __shfl(mine, j);
            if (c > (max_good > 4 ? max_good : 4)) {
                best = base + j; max_good = c;
                const int t = tab[c];
                niters = t < niters ? t : niters;
            }
        }
    }
    if (lane == 0) { ctl[KP_BEST] = best; ctl[KP_NITERS] = niters; ctl[KP_MAXGOOD] = max_good; }
}

// One workgroup per pair: the winner's mask, the ordered compaction, the refit, :245-254, loop_info and the gate.
extern "C" __global__ __launch_bounds__(SFM_NT) void kp_tail_kernel(KpDev b) {
    __shared__ double red[(SFM_NW + 1) * SFM_NRED];
    __shared__ unsigned long long wds[VG_KF_MAX_WINDOW / 64];
    const int pair = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (pair >= b.P) return;
    const int* pi = b.pi + (size_t)pair * KP_PI;
    int* ctl = b.ctl + (size_t)pair * KP_CTL;
    double* res = b.res + (size_t)KP_RES * pair;
    if (pi[KP_RUN] == 0) {                                   // findConnection never calls PnPRANSAC: everything stays zero
        if (tid == 0) ctl[KP_STATUS] = VG_KF_PNP_SKIPPED;
        return;
    }
    const int n = pi[KP_N], nw = (n + 63) >> 6, best = ctl[KP_BEST];
    const double* par = b.par + (size_t)KP_PAR * pair;
    const float* __restrict__ p3 = b.p3 + 3 * (size_t)pi[KP_PT0];
    const float* __restrict__ p2 = b.p2 + 2 * (size_t)pi[KP_PT0];
    const double *oT = par + 3, *oR = par + 6, *tic = par + 15, *qic = par + 18;
    // ---- R_inital, P_inital, rvec0
    double Rg[9], tg[3], rv0[3];
    bool guess_ok;
    {
        double Rwc[9], Twc[3];
        m3_mul(oR, qic, Rwc);
        m3_vec(oR, tic, Twc);
        Twc[0] = oT[0] + Twc[0]; Twc[1] = oT[1] + Twc[1]; Twc[2] = oT[2] + Twc[2];
        const double k00 = Rwc[4] * Rwc[8] - Rwc[5] * Rwc[7], k01 = Rwc[5] * Rwc[6] - Rwc[3] * Rwc[8], k02 = Rwc[3] * Rwc[7] - Rwc[4] * Rwc[6];
        const double id = 1.0 / (Rwc[0] * k00 + Rwc[1] * k01 + Rwc[2] * k02);
        Rg[0] = k00 * id; Rg[1] = (Rwc[2] * Rwc[7] - Rwc[1] * Rwc[8]) * id; Rg[2] = (Rwc[1] * Rwc[5] - Rwc[2] * Rwc[4]) * id;
        Rg[3] = k01 * id; Rg[4] = (Rwc[0] * Rwc[8] - Rwc[2] * Rwc[6]) * id; Rg[5] = (Rwc[2] * Rwc[3] - Rwc[0] * Rwc[5]) * id;
        Rg[6] = k02 * id; Rg[7] = (Rwc[1] * Rwc[6] - Rwc[0] * Rwc[7]) * id; Rg[8] = (Rwc[0] * Rwc[4] - Rwc[1] * Rwc[3]) * id;
        m3_vec(Rg, Twc, tg);
        tg[0] = -tg[0]; tg[1] = -tg[1]; tg[2] = -tg[2];
        guess_ok = sf_rodrigues_R2r(Rg, rv0);
#pragma unroll
        for (int k = 0; k < 3; ++k) guess_ok = guess_ok && sf_finite(rv0[k]) && sf_finite(tg[k]);
    }
    // ---- the winner's mask by ballots, wavefront wv takes the words wv, wv + SFM_NW, ...
    double ms[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (best >= 0) {
        const double* model = b.models + ((size_t)pair * b.stride + best) * KP_MODEL;
#pragma unroll
        for (int k = 0; k < 6; ++k) ms[k] = model[k];
        double R[9];
        sf_rodrigues_r2R<false>(ms, R, nullptr);
        const float thresh2 = (float)par[0];
        for (int w = wv; w < nw; w += SFM_NW) {
            const int i = 64 * w + lane;
            const bool in = i < n && kp_error(R, ms + 3, p3 + 3 * (i < n ? i : 0), p2 + 2 * (i < n ? i : 0)) <= thresh2;
            const unsigned long long bal = __ballot(in);
            if (lane == 0) { wds[w] = bal; b.mask[(size_t)pair * b.words_n + w] = bal; }
        }
    }
    __syncthreads();
    // ---- the ordered compaction: thread w owns word w, its first slot is the count of the words before it
    int n_in = 0;
    if (best >= 0) {
        for (int w = 0; w < nw; ++w) n_in += __popcll(wds[w]);
        if (tid < nw) {
            int pos = 0;
            for (int w = 0; w < tid; ++w) pos += __popcll(wds[w]);
            int* midx = b.midx + pi[KP_PT0];
            unsigned long long m = wds[tid];
            while (m) {
                const int bit = __ffsll((long long)m) - 1;
                midx[pos++] = 64 * tid + bit;
                m &= m - 1ull;
            }
        }
    }
    // ---- the returned pose
    int status = best >= 0 ? VG_KF_PNP_OK : VG_KF_PNP_NO_MODEL;
    double rv[3] = {0.0, 0.0, 0.0}, tv[3] = {0.0, 0.0, 0.0};
    int rit = 0, rup = 0;
    if (best < 0) {
        if (!guess_ok) status = VG_KF_PNP_NUMERIC;
#pragma unroll
        for (int k = 0; k < 3; ++k) { rv[k] = rv0[k]; tv[k] = tg[k]; }
    } else if (pi[KP_REFINE] == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { rv[k] = ms[k]; tv[k] = ms[3 + k]; }
    } else {
        int st = guess_ok ? SF_OK : SF_NUMERIC;
        double R[9];
        if (st == SF_OK)
            st = sf_pnp(red, n, [&](int k, double* P, double* p) {
                if (((wds[k >> 6] >> (k & 63)) & 1ull) == 0ull) return false;
                P[0] = p3[3 * k]; P[1] = p3[3 * k + 1]; P[2] = p3[3 * k + 2];
                p[0] = p2[2 * k]; p[1] = p2[2 * k + 1];
                return true;
            }, Rg, tg, R, tv, &rit, &rup, tid);
        // (the PnP hands its rotation on as a matrix: the returned rvec is its Rodrigues vector, regular branch)
        if (st == SF_OK && !sf_rodrigues_R2r(R, rv)) st = SF_NUMERIC;
        if (st != SF_OK) status = VG_KF_PNP_NUMERIC;
    }
    if (tid != 0) return;
    ctl[KP_STATUS] = status; ctl[KP_NIN] = n_in; ctl[KP_RIT] = rit; ctl[KP_RUP] = rup; ctl[KP_LOOP] = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) res[k] = ms[k];
    if (status == VG_KF_PNP_NUMERIC) return;               // (the block was zeroed before the launches)
    // ---- :245-254
    double r[9], Rold[9], Told[3], PR[9], PT[3];
    sf_rodrigues_r2R<false>(rv, r, nullptr);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Rold[3 * i + j] = r[3 * j + i];
    const double mt[3] = {-tv[0], -tv[1], -tv[2]};
    m3_vec(Rold, mt, Told);
    m3_mul_t(Rold, qic, PR);
    m3_vec(PR, tic, PT);
    PT[0] = Told[0] - PT[0]; PT[1] = Told[1] - PT[1]; PT[2] = Told[2] - PT[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) { res[6 + k] = rv[k]; res[9 + k] = tv[k]; res[21 + k] = PT[k]; }
#pragma unroll
    for (int k = 0; k < 9; ++k) res[12 + k] = PR[k];
    if (status != VG_KF_PNP_OK || !(n_in > pi[KP_MINLOOP])) return;
    // ---- :474-480
    const double d[3] = {oT[0] - PT[0], oT[1] - PT[1], oT[2] - PT[2]};
    double rt[3], rq[4], rel[9];
    m3t_vec(PR, d, rt);
    m3t_mul(PR, oR, rel);
    sf_R_to_q(rel, rq);
    if (rq[0] < 0.0) { rq[0] = -rq[0]; rq[1] = -rq[1]; rq[2] = -rq[2]; rq[3] = -rq[3]; }
    const double a = kp_yaw_deg(oR) - kp_yaw_deg(PR);
    const double yaw = a > 0 ? a - 360.0 * floor((a + 180.0) / 360.0) : a + 360.0 * floor((-a + 180.0) / 360.0);
    res[24] = rt[0]; res[25] = rt[1]; res[26] = rt[2]; res[27] = rq[0]; res[28] = rq[1]; res[29] = rq[2]; res[30] = rq[3]; res[31] = yaw;
    ctl[KP_LOOP] = (fabs(yaw) < par[1] && sqrt(rt[0] * rt[0] + rt[1] * rt[1] + rt[2] * rt[2]) < par[2]) ? 1 : 0;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
extern "C" void vg_kf_pnp_defaults(vg_kf_pnp_in* in) {
    if (!in) return;
    *in = vg_kf_pnp_in();
    in->struct_size = sizeof(vg_kf_pnp_in);
    in->origin_vio_R[0] = in->origin_vio_R[4] = in->origin_vio_R[8] = 1.0;
    in->qic[0] = in->qic[4] = in->qic[8] = 1.0;
    in->min_loop_num = 25; in->max_iters = 100; in->refine = 0;
    in->reproj_threshold = 10.0 / 460.0; in->confidence = 0.99; in->max_yaw_deg = 30.0; in->max_dist = 20.0;
}

extern "C" int vg_kf_pnp(vg_handle* h, int n_pairs, const vg_kf_pnp_in* in, vg_kf_pnp_out* out) {
    VG_RANGE("vg_kf_pnp");
    if (!h) return VG_ERR_BAD_ARG;
    auto bad = [&](int w, const char* what) {
        h->err = "vg_kf_pnp: pair " + std::to_string(w) + ": " + what;
        return VG_ERR_BAD_ARG;
    };
    if (n_pairs <= 0 || !in || !out) { h->err = "vg_kf_pnp: n_pairs <= 0 or a NULL argument"; return VG_ERR_BAD_ARG; }
    // ---- everything that follows from the arguments alone, before anything is uploaded or written
    const int P = n_pairs;
    size_t nPts = 0;
    int nmax = 0, stride = 1;
    for (int w = 0; w < P; ++w) {
        const vg_kf_pnp_in& a = in[w];
        if (a.struct_size != sizeof(vg_kf_pnp_in)) return bad(w, "vg_kf_pnp_in::struct_size");
        if (out[w].struct_size != sizeof(vg_kf_pnp_out)) return bad(w, "vg_kf_pnp_out::struct_size");
        if (a.n < 6 || a.n > VG_KF_MAX_WINDOW) return bad(w, "n outside 6 .. VG_KF_MAX_WINDOW");
        if (!a.point_3d || !a.old_norm) return bad(w, "a NULL table");
        if (!(a.reproj_threshold > 0) || !(a.max_yaw_deg > 0) || !(a.max_dist > 0) || !std::isfinite(a.reproj_threshold) ||
            !std::isfinite(a.max_yaw_deg) || !std::isfinite(a.max_dist))
            return bad(w, "reproj_threshold, max_yaw_deg or max_dist is not positive");
        if (a.min_loop_num < 0) return bad(w, "min_loop_num < 0");
        if (a.max_iters < 1 || a.max_iters > VG_KF_PNP_MAX_ITERS) return bad(w, "max_iters outside 1 .. VG_KF_PNP_MAX_ITERS");
        if (a.confidence != 0.99) return bad(w, "a confidence other than 0.99");
        if (a.refine != 0 && a.refine != 1) return bad(w, "refine outside {0, 1}");
        if (!rp_finite(a.origin_vio_T, 3) || !rp_finite(a.origin_vio_R, 9) || !rp_finite(a.tic, 3) || !rp_finite(a.qic, 9)) return bad(w, "a non-finite input");
        for (int i = 0; i < 3 * a.n; ++i) if (!std::isfinite(a.point_3d[i])) return bad(w, "a non-finite input");
        for (int i = 0; i < 2 * a.n; ++i) if (!std::isfinite(a.old_norm[i])) return bad(w, "a non-finite input");
        nPts += a.n;
        nmax = std::max(nmax, a.n);
        stride = std::max(stride, a.max_iters);
    }
    const int words_n = (int)rp_up(nmax, 64) / 64;
    // ---- the schedule and the bound table of every distinct n among the pairs that run (to the most iterations such a pair asks for)
    std::vector<int> tabs, need_it(VG_KF_MAX_WINDOW + 1, 0), at_s(VG_KF_MAX_WINDOW + 1, -1), at_t(VG_KF_MAX_WINDOW + 1, -1);
    for (int w = 0; w < P; ++w)
        if (in[w].n > in[w].min_loop_num) need_it[in[w].n] = std::max(need_it[in[w].n], in[w].max_iters);
    for (int n = 6; n <= nmax; ++n) {
        if (!need_it[n]) continue;
        at_s[n] = (int)tabs.size();
        tabs.resize(tabs.size() + (size_t)need_it[n] * 5);
        CvRng rng((unsigned long long)-1);
        for (int it = 0; it < need_it[n]; ++it) {
            int* idx = tabs.data() + at_s[n] + (size_t)it * 5;
            for (int i = 0; i < 5;) {                       // getSubset: an index already in the sample is drawn again
                const int c = idx[i] = rng.uniform(0, n);
                int j = 0;
                for (; j < i; ++j) if (c == idx[j]) break;
                if (j == i) ++i;
            }
        }
        at_t[n] = (int)tabs.size();
        for (int c = 0; c <= n; ++c) tabs.push_back(update_num_iters(0.99, (double)(n - c) / n, 5, VG_KF_PNP_MAX_ITERS));
    }
    if (tabs.empty()) tabs.push_back(0);
    // ---- the host image of the upload: doubles [par], floats [p3 | p2], ints [pi | tabs]
    const size_t n_f = rp_up(5 * nPts, 2), n_i = rp_up((size_t)KP_PI * P + tabs.size(), 2);
    std::vector<double> hpar((size_t)KP_PAR * P, 0.0);
    std::vector<float> hf(n_f, 0.f);
    std::vector<int> hi(n_i, 0);
    {
        size_t pt = 0;
        for (int w = 0; w < P; ++w) {
            const vg_kf_pnp_in& a = in[w];
            int* q = hi.data() + (size_t)KP_PI * w;
            const bool run = a.n > a.min_loop_num;
            q[KP_N] = a.n; q[KP_PT0] = (int)pt; q[KP_SCHED] = run ? KP_PI * P + at_s[a.n] : 0; q[KP_TAB] = run ? KP_PI * P + at_t[a.n] : 0;
            q[KP_MAXIT] = a.max_iters; q[KP_MINLOOP] = a.min_loop_num; q[KP_REFINE] = a.refine; q[KP_RUN] = run ? 1 : 0;
            double* p = hpar.data() + (size_t)KP_PAR * w;
            p[0] = (double)(float)(a.reproj_threshold * a.reproj_threshold); p[1] = a.max_yaw_deg; p[2] = a.max_dist;
            std::copy(a.origin_vio_T, a.origin_vio_T + 3, p + 3); std::copy(a.origin_vio_R, a.origin_vio_R + 9, p + 6);
            std::copy(a.tic, a.tic + 3, p + 15); std::copy(a.qic, a.qic + 9, p + 18);
            std::copy(a.point_3d, a.point_3d + 3 * (size_t)a.n, hf.data() + 3 * pt);
            std::copy(a.old_norm, a.old_norm + 2 * (size_t)a.n, hf.data() + 3 * nPts + 2 * pt);
            pt += a.n;
        }
        std::copy(tabs.begin(), tabs.end(), hi.begin() + (size_t)KP_PI * P);
    }
    // the download, in 8-byte units: ctl (ints) | res | mask | midx (ints)
    const size_t d_ctl = 0, d_res = d_ctl + (size_t)P * KP_CTL / 2, d_mask = d_res + (size_t)KP_RES * P, d_mi = d_mask + (size_t)P * words_n,
                 n_out = d_mi + rp_up(nPts, 2) / 2;
    std::vector<double> hout(n_out);
    hipError_t e = hipSetDevice(h->device);
    auto fail = [&](hipError_t err) { h->err = std::string("vg_kf_pnp: ") + hipGetErrorString(err); return VG_ERR_HIP; };
    if (e != hipSuccess) return fail(e);
    // ---- device block (the scratch block of vg_init_relpose, grown on demand): [out | par | floats | ints | models | count]
    const size_t b_out = 0, b_par = b_out + n_out * 8, b_f = b_par + hpar.size() * 8, b_i = b_f + n_f * 4, b_md = rp_up(b_i + n_i * 4, 256);
    const size_t b_ct = b_md + (size_t)P * stride * KP_MODEL * 8, total = b_ct + (size_t)P * stride * 4;
    if ((e = rp_scratch(h, total)) != hipSuccess) return fail(e);
    char* base = (char*)h->relpose_buf;
    double* d_out = (double*)(base + b_out);
    KpDev b;
    b.P = P; b.stride = stride; b.words_n = words_n;
    b.par = (const double*)(base + b_par);
    b.p3 = (const float*)(base + b_f); b.p2 = b.p3 + 3 * nPts;
    b.pi = (const int*)(base + b_i); b.tabs = b.pi;          // (KP_SCHED / KP_TAB count from the start of the int block)
    b.ctl = (int*)(d_out + d_ctl); b.res = d_out + d_res; b.mask = (unsigned long long*)(d_out + d_mask); b.midx = (int*)(d_out + d_mi);
    b.models = (double*)(base + b_md); b.count = (int*)(base + b_ct);
    if ((e = hipMemcpyAsync(base + b_par, hpar.data(), hpar.size() * 8, hipMemcpyHostToDevice, h->stream)) != hipSuccess) return fail(e);
    if ((e = hipMemcpyAsync(base + b_f, hf.data(), n_f * 4, hipMemcpyHostToDevice, h->stream)) != hipSuccess) return fail(e);
    if ((e = hipMemcpyAsync(base + b_i, hi.data(), n_i * 4, hipMemcpyHostToDevice, h->stream)) != hipSuccess) return fail(e);
    if ((e = hipMemsetAsync(d_out, 0, n_out * 8, h->stream)) != hipSuccess) return fail(e);
    struct Events {                                         // destroyed on every way out
        hipEvent_t ev[VG_KF_PNP_LAUNCHES + 1] = {};
        ~Events() { for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x); }
    } evs;
    const bool timed = out[0].device_ms != nullptr;
    if (timed)
        for (int i = 0; i <= VG_KF_PNP_LAUNCHES; ++i)
            if ((e = hipEventCreate(&evs.ev[i])) != hipSuccess) return fail(e);
    int mark = 0;
    auto stamp = [&]() { return timed ? hipEventRecord(evs.ev[mark++], h->stream) : hipSuccess; };
    if ((e = stamp()) != hipSuccess) return fail(e);
    hipLaunchKernelGGL(kp_sample_kernel, dim3(KP_CHUNK0 / KP_PER_WAVE, (unsigned)P), dim3(64), 0, h->stream, b, 0, KP_CHUNK0);
    if ((e = stamp()) != hipSuccess) return fail(e);
    hipLaunchKernelGGL(kp_count_kernel, dim3(KP_CHUNK0, (unsigned)P), dim3(64), 0, h->stream, b, 0, KP_CHUNK0);
    if ((e = stamp()) != hipSuccess) return fail(e);
    hipLaunchKernelGGL(kp_pick_kernel, dim3((unsigned)P), dim3(64), 0, h->stream, b, 0, KP_CHUNK0);
    if ((e = stamp()) != hipSuccess) return fail(e);
    hipLaunchKernelGGL(kp_sample_kernel, dim3(KP_P2_WAVES, (unsigned)P), dim3(64), 0, h->stream, b, KP_CHUNK0, VG_KF_PNP_MAX_ITERS);
    if ((e = stamp()) != hipSuccess) return fail(e);
    hipLaunchKernelGGL(kp_count_kernel, dim3(KP_P2_COUNT, (unsigned)P), dim3(64), 0, h->stream, b, KP_CHUNK0, VG_KF_PNP_MAX_ITERS);
    if ((e = stamp()) != hipSuccess) return fail(e);
    hipLaunchKernelGGL(kp_pick_kernel, dim3((unsigned)P), dim3(64), 0, h->stream, b, KP_CHUNK0, VG_KF_PNP_MAX_ITERS);
    if ((e = stamp()) != hipSuccess) return fail(e);
    hipLaunchKernelGGL(kp_tail_kernel, dim3((unsigned)P), dim3(SFM_NT), 0, h->stream, b);
    if ((e = stamp()) != hipSuccess) return fail(e);
    if ((e = hipGetLastError()) != hipSuccess) return fail(e);
    if ((e = hipMemcpyAsync(hout.data(), d_out, n_out * 8, hipMemcpyDeviceToHost, h->stream)) != hipSuccess) return fail(e);
    if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return fail(e);
    if (timed)
        for (int i = 0; i < VG_KF_PNP_LAUNCHES; ++i) {
            float ms = 0.f;
            if ((e = hipEventElapsedTime(&ms, evs.ev[i], evs.ev[i + 1])) != hipSuccess) return fail(e);
            out[0].device_ms[i] = ms;
        }
    const int* ctl = (const int*)(hout.data() + d_ctl);
    const unsigned long long* mask = (const unsigned long long*)(hout.data() + d_mask);
    const int* midx = (const int*)(hout.data() + d_mi);
    size_t pt = 0;
    for (int w = 0; w < P; ++w) {
        const vg_kf_pnp_in& a = in[w];
        vg_kf_pnp_out& o = out[w];
        const int* c = ctl + (size_t)w * KP_CTL;
        const double* r = hout.data() + d_res + (size_t)KP_RES * w;
        const bool ran = c[KP_STATUS] != VG_KF_PNP_SKIPPED;
        o.status = c[KP_STATUS]; o.n_inliers = c[KP_NIN]; o.refit_iters = c[KP_RIT]; o.refit_up = c[KP_RUP]; o.has_loop = c[KP_LOOP];
        // the last iteration the loop looked at: the bound can drop below the iteration that lowered it
        const int reach = std::min(c[KP_NITERS], a.max_iters) - 1;
        o.ransac_best = ran ? c[KP_BEST] : 0; o.ransac_bound = ran ? c[KP_NITERS] : 0; o.ransac_iter = ran ? std::max(c[KP_BEST], reach) : 0;
        std::copy(r, r + 3, o.sample_rvec); std::copy(r + 3, r + 6, o.sample_tvec); std::copy(r + 6, r + 9, o.rvec); std::copy(r + 9, r + 12, o.tvec);
        std::copy(r + 12, r + 21, o.PnP_R_old); std::copy(r + 21, r + 24, o.PnP_T_old); std::copy(r + 24, r + 32, o.loop_info);
        if (o.mask)
            for (int k = 0; k < a.n; ++k) o.mask[k] = (unsigned char)((mask[(size_t)w * words_n + (k >> 6)] >> (k & 63)) & 1ull);
        for (int k = 0; k < o.n_inliers; ++k) {
            const int i = midx[pt + k];
            if (o.matched_index) o.matched_index[k] = i;
            if (o.match_id) o.match_id[k] = a.point_id ? a.point_id[i] : i;
            if (o.match_xy) { o.match_xy[2 * k] = a.old_norm[2 * i]; o.match_xy[2 * k + 1] = a.old_norm[2 * i + 1]; }
        }
        pt += a.n;
    }
    return VG_OK;
}
