// init_align.h — device functions of init_align_kernel (csrc/imu_preint.hip: vg_init_align): VisualIMUAlignment
// (vins_estimator/src/initial/initial_aligment.cpp:3-207) and the state change of Estimator::visualInitialAlign (estimator.cpp:376-435)
// for ONE window, run by the 64 lanes of ONE wavefront that owns the carve of init_align_carve.h.  The records come from
// imu_preint_kernel: the host launches it over the intervals of all windows before al_gyro_bias and again before al_window.
// Everything small is wave-uniform (every lane evaluates it); the lanes share the assembly, the factorisation and the
// substitutions entry-wise.  Sums over the pairs run pair 0 first, one pair after the other: no atomics, the result is the same
// run to run.
//
// The reference's quirks are kept (include/vinsgpu.h lists them): A and b times 1000, the scale column divided by 100, A and b of
// RefineGravity cleared ONCE before its four passes and multiplied by 1000 at the end of every pass, TangentBasis' exact comparison,
// the re-propagation with a zero accelerometer bias, Vs indexed by the key-frame counter.
// The solves are an unpivoted LDL^T of the packed lower triangle (the systems are symmetric positive semi-definite; the reference
// calls Eigen's pivoted ldlt()): a pivot that is not a positive finite number ends the window with AL_NUMERIC.
#pragma once
#include "ba_math.h"
#include "imu_step.h"
#include "init_align_carve.h"

#define AL_OK 0                 // VG_ALIGN_* of include/vinsgpu.h
#define AL_FAILED_LINEAR 1
#define AL_FAILED_REFINE 2
#define AL_NUMERIC 3
#define AL_RES 28               // status | delta_bg 3 | bg 3 | g_lin 3 | s_lin | g_c0 3 | s | g_w 3 | R0 9 | pad
#define AL_PAR 14               // ba0 3 | bg0 3 | noise 4 | tic 3 | g_norm
#define AL_WIN 15               // Ps 3 | Rs 9 | Vs 3

DEV bool al_pos_finite(double v) { return v > 0.0 && v < 1.79e308; }
DEV bool al_finite(double v) { return v > -1.79e308 && v < 1.79e308; }

// Eigen normalized(): divide by the norm
DEV void al_normalized(const double* v, double* o) {
    const double n = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    o[0] = v[0] / n; o[1] = v[1] / n; o[2] = v[2] / n;
}

// Utility::R2ypr(R).x() (utility.h:70-85), degrees
DEV double al_yaw_deg(const double* R) { return atan2(R[3], R[0]) / M_PI * 180.0; }
// Utility::ypr2R({yaw, 0, 0}) * R (utility.h:88-112; Ry = Rx = I exactly)
DEV void al_yaw_times(double yaw_deg, const double* R, double* o) {
    const double y = yaw_deg / 180.0 * M_PI, c = cos(y), s = sin(y);
    const double Rz[9] = {c, -s, 0.0, s, c, 0.0, 0.0, 0.0, 1.0};
    m3_mul(Rz, R, o);
}

// in-place unpivoted LDL^T of the packed lower triangle W (n x n): L below the diagonal, D on it.  false: a pivot is not a positive
// finite number (wave-uniform, every lane returns together)
DEV bool al_factor(double* W, double* col, int n, int lane) {
    for (int j = 0; j < n; ++j) {
        const double d = W[AL_TRI(j) + j];
        if (!al_pos_finite(d)) return false;
        for (int i = j + 1 + lane; i < n; i += 64) col[i] = W[AL_TRI(i) + j] / d;
        __syncthreads();
        const int m = n - 1 - j, cnt = AL_TRI(m);
        for (int e = lane; e < cnt; e += 64) {
            int a, b;
            tri_decode(e, a, b);
            const int i = j + 1 + a, k = j + 1 + b;
            W[AL_TRI(i) + k] -= W[AL_TRI(i) + j] * col[k];
        }
        __syncthreads();
        for (int i = j + 1 + lane; i < n; i += 64) W[AL_TRI(i) + j] = col[i];
        __syncthreads();
    }
    return true;
}
// x <- (L D L^T)^-1 x
DEV void al_solve(const double* W, double* x, int n, int lane) {
    for (int j = 0; j < n - 1; ++j) {
        const double xj = x[j];
        for (int i = j + 1 + lane; i < n; i += 64) x[i] -= W[AL_TRI(i) + j] * xj;
        __syncthreads();
    }
    for (int i = lane; i < n; i += 64) x[i] /= W[AL_TRI(i) + i];
    __syncthreads();
    for (int j = n - 1; j > 0; --j) {
        const double xj = x[j];
        for (int i = lane; i < j; i += 64) x[i] -= W[AL_TRI(j) + i] * xj;
        __syncthreads();
    }
}

// One pair's tmp_A^T tmp_A and tmp_A^T tmp_b added to acc / b (initial_aligment.cpp:75-113 with refine, :138-175 without).
// Ri, Rj, Ti, Tj: the two ImageFrames; pr: sum_dt dp dv of frame_j's record; nc = 10 (columns v_i v_j g s) or 9 (v_i v_j dg s).
DEV void al_add_pair(double* acc, double* bv, double* tA, const double* Ri, const double* Rj, const double* Ti, const double* Tj,
                     const double* pr, const double* tic, bool refine, const double* lx, const double* ly, const double* g0, int i,
                     int n, int lane) {
    const int nc = refine ? 9 : 10, ng = nc - 7;            // ng: gravity columns
    double* tb = tA + 6 * AL_TC;
    const double dt = pr[0];
    if (lane < 6 * nc) {
        const int r = lane / nc, a = lane - nc * r, rr = r < 3 ? r : r - 3;
        double v = 0.0;
        if (a < 3) v = (a == rr) ? (r < 3 ? -dt : -1.0) : 0.0;
        else if (a < 6) {
            if (r >= 3) { const int c = a - 3; v = Ri[rr] * Rj[c] + Ri[3 + rr] * Rj[3 + c] + Ri[6 + rr] * Rj[6 + c]; }
        } else if (a < 6 + ng) {
            // R_i^T * dt * dt / 2 (position rows) or R_i^T * dt (velocity rows), times lxly in RefineGravity
            double m[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) m[k] = r < 3 ? Ri[3 * k + rr] * dt * dt / 2 : Ri[3 * k + rr] * dt;
            if (refine) { const double* l = (a == 6) ? lx : ly; v = m[0] * l[0] + m[1] * l[1] + m[2] * l[2]; }
            else v = m[a - 6];
        } else if (r < 3) {
            v = (Ri[rr] * (Tj[0] - Ti[0]) + Ri[3 + rr] * (Tj[1] - Ti[1]) + Ri[6 + rr] * (Tj[2] - Ti[2])) / 100.0;
        }
        tA[r * AL_TC + a] = v;
    }
    if (lane >= 58) {                                       // tmp_b (six lanes the entries above leave free)
        const int r = lane - 58, rr = r < 3 ? r : r - 3;
        double v;
        if (r < 3) {
            double RtR[3];                                  // row rr of R_i^T R_j
#pragma unroll
            for (int c = 0; c < 3; ++c) RtR[c] = Ri[rr] * Rj[c] + Ri[3 + rr] * Rj[3 + c] + Ri[6 + rr] * Rj[6 + c];
            v = pr[1 + rr] + (RtR[0] * tic[0] + RtR[1] * tic[1] + RtR[2] * tic[2]) - tic[rr];
            if (refine) v -= Ri[rr] * dt * dt / 2 * g0[0] + Ri[3 + rr] * dt * dt / 2 * g0[1] + Ri[6 + rr] * dt * dt / 2 * g0[2];
        } else {
            v = pr[4 + rr];
            if (refine) v -= Ri[rr] * dt * g0[0] + Ri[3 + rr] * dt * g0[1] + Ri[6 + rr] * dt * g0[2];
        }
        tb[r] = v;
    }
    __syncthreads();
    for (int e = lane; e < nc * nc; e += 64) {
        const int a = e / nc, c = e - nc * a;
        if (c > a) continue;                                // the lower triangle (the column map below ascends)
        double v = 0.0;
#pragma unroll
        for (int r = 0; r < 6; ++r) v += tA[r * AL_TC + a] * tA[r * AL_TC + c];
        const int ga = a < 6 ? 3 * i + a : n - (nc - 6) + (a - 6), gc = c < 6 ? 3 * i + c : n - (nc - 6) + (c - 6);
        acc[AL_TRI(ga) + gc] += v;
    }
    if (lane < nc) {
        double v = 0.0;
#pragma unroll
        for (int r = 0; r < 6; ++r) v += tA[r * AL_TC + lane] * tb[r];
        bv[lane < 6 ? 3 * i + lane : n - (nc - 6) + (lane - 6)] += v;
    }
    __syncthreads();
}

// A = A * 1000, b = b * 1000; the copy; x = A.ldlt().solve(b)
DEV bool al_scale_solve(const AlignLds& c, double* L, int n, int lane) {
    const int tri = AL_TRI(n);
    for (int e = lane; e < tri; e += 64) { const double v = L[c.acc + e] * 1000.0; L[c.acc + e] = v; L[c.fac + e] = v; }
    for (int e = lane; e < n; e += 64) { const double v = L[c.b + e] * 1000.0; L[c.b + e] = v; L[c.x + e] = v; }
    __syncthreads();
    if (!al_factor(L + c.fac, L + c.col, n, lane)) return false;
    al_solve(L + c.fac, L + c.x, n, lane);
    return true;
}

// MatrixXd TangentBasis(Vector3d& g0) (initial_aligment.cpp:40-53)
DEV void al_tangent_basis(const double* g0, double* b, double* cc) {
    double a[3];
    al_normalized(g0, a);
    double tmp[3] = {0.0, 0.0, 1.0};
    if (a[0] == 0.0 && a[1] == 0.0 && a[2] == 1.0) { tmp[0] = 1.0; tmp[2] = 0.0; }      // if (a == tmp) tmp << 1, 0, 0
    const double at = a[0] * tmp[0] + a[1] * tmp[1] + a[2] * tmp[2];
    const double u[3] = {tmp[0] - a[0] * at, tmp[1] - a[1] * at, tmp[2] - a[2] * at};
    al_normalized(u, b);
    cc[0] = a[1] * b[2] - a[2] * b[1]; cc[1] = a[2] * b[0] - a[0] * b[2]; cc[2] = a[0] * b[1] - a[1] * b[0];
}

// solveGyroscopeBias (:3-26) of one window from its F - 1 records integrated with (ba0, bg0): A += J^T J, b += J^T 2 vec(dq^-1 (x) q_ij),
// pair 0 first; every lane evaluates it (wave-uniform).  Writes delta_bg / bg into res and the biases (0, bg0 + delta_bg) of the
// re-propagation into bias [F - 1][6]; AL_NUMERIC: a pivot or the solution is not finite (the biases stay what they were).
DEV int al_gyro_bias(int F, const double* R, const double* rec, const double* par, double* res, double* bias, int lane) {
    double A3[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, b3[3] = {0, 0, 0};
    for (int k = 0; k < F - 1; ++k) {
        const double* o = rec + (size_t)k * IMU_OUT;
        double J[9], RtR[9], qij[4], qi[4], q[4];
#pragma unroll
        for (int e = 0; e < 9; ++e) J[e] = o[17 + (3 + e / 3) * 15 + 12 + e % 3];           // jacobian.block<3, 3>(O_R, O_BG)
        m3t_mul(R + 9 * k, R + 9 * (k + 1), RtR);
        R_to_q(RtR, qij);
        q_inv(o + 4, qi);
        q_mul(qi, qij, q);
        const double tb[3] = {2 * q[0], 2 * q[1], 2 * q[2]};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int b = 0; b < 3; ++b) A3[a * 3 + b] += J[a] * J[b] + J[3 + a] * J[3 + b] + J[6 + a] * J[6 + b];
            b3[a] += J[a] * tb[0] + J[3 + a] * tb[1] + J[6 + a] * tb[2];
        }
    }
    double dbg[3];
    {   // 3x3 LDL^T
        const double d0 = A3[0];
        if (!al_pos_finite(d0)) return AL_NUMERIC;
        const double l10 = A3[3] / d0, l20 = A3[6] / d0;
        const double d1 = A3[4] - l10 * A3[3];
        if (!al_pos_finite(d1)) return AL_NUMERIC;
        const double l21 = (A3[7] - l20 * A3[3]) / d1;
        const double d2 = A3[8] - l20 * A3[6] - l21 * l21 * d1;
        if (!al_pos_finite(d2)) return AL_NUMERIC;
        const double y0 = b3[0], y1 = b3[1] - l10 * y0, y2 = b3[2] - l20 * y0 - l21 * y1;
        dbg[2] = y2 / d2;
        dbg[1] = y1 / d1 - l21 * dbg[2];
        dbg[0] = y0 / d0 - l10 * dbg[1] - l20 * dbg[2];
        if (!(al_finite(dbg[0]) && al_finite(dbg[1]) && al_finite(dbg[2]))) return AL_NUMERIC;
    }
    const double bg[3] = {par[3] + dbg[0], par[4] + dbg[1], par[5] + dbg[2]};
    if (lane == 0)
        for (int i = 0; i < 3; ++i) { res[1 + i] = dbg[i]; res[4 + i] = bg[i]; }
    // repropagate(Vector3d::Zero(), Bgs[0]) (:32-36): the accelerometer bias is ZERO
    for (int e = lane; e < 6 * (F - 1); e += 64) bias[e] = (e % 6 < 3) ? 0.0 : bg[e % 6 - 3];
    return AL_OK;
}

// LinearAlignment, RefineGravity and the window stage of one window.  L: the carve; the tables are the window's own (R, T [F]; rec
// [F - 1] the records re-propagated with (0, bg); key [K]).  Returns the status; res [AL_RES] is written by lane 0 as far as the status
// reaches, everything behind it stays as the host cleared it.
DEV int al_window(double* L, int F, int K, const double* R, const double* T, const double* rec, const int* key, const double* par,
                  double* res, double* vbody, double* win, int lane) {
    const AlignLds c = align_lds(F);
    const double* tic = par + 10;
    const double g_norm = par[13];
    for (int k = lane; k < F - 1; k += 64) {
        const double* o = rec + (size_t)k * IMU_OUT;
        double* pr = L + c.pr + AL_PR * k;
        pr[0] = o[0];
        for (int i = 0; i < 3; ++i) { pr[1 + i] = o[1 + i]; pr[4 + i] = o[8 + i]; }
    }
    __syncthreads();
    if (F < AL_MIN_FRAMES_SOLVE) return AL_NUMERIC;
    // ---- LinearAlignment (:125-187)
    int n = AL_N_LIN(F);
    for (int e = lane; e < AL_TRI(n); e += 64) L[c.acc + e] = 0.0;
    for (int e = lane; e < n; e += 64) L[c.b + e] = 0.0;
    __syncthreads();
    for (int i = 0; i < F - 1; ++i)
        al_add_pair(L + c.acc, L + c.b, L + c.tA, R + 9 * i, R + 9 * (i + 1), T + 3 * i, T + 3 * (i + 1), L + c.pr + AL_PR * i, tic, false,
                    nullptr, nullptr, nullptr, i, n, lane);
    if (!al_scale_solve(c, L, n, lane)) return AL_NUMERIC;
    const double* x = L + c.x;
    double g[3] = {x[n - 4], x[n - 3], x[n - 2]};
    double sc = x[n - 1] / 100.0;
    if (!(al_finite(g[0]) && al_finite(g[1]) && al_finite(g[2]) && al_finite(sc))) return AL_NUMERIC;
    if (lane == 0) { res[7] = g[0]; res[8] = g[1]; res[9] = g[2]; res[10] = sc; }
    if (fabs(sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]) - g_norm) > 1.0 || sc < 0) return AL_FAILED_LINEAR;
    __syncthreads();                                        // (x is read above, cleared below)
    // ---- RefineGravity (:55-123): A and b are cleared once, NOT per pass
    n = n - 1;
    double g0[3];
    al_normalized(g, g0);
    g0[0] *= g_norm; g0[1] *= g_norm; g0[2] *= g_norm;
    for (int e = lane; e < AL_TRI(n); e += 64) L[c.acc + e] = 0.0;
    for (int e = lane; e < n; e += 64) L[c.b + e] = 0.0;
    __syncthreads();
    for (int pass = 0; pass < 4; ++pass) {
        double lx[3], ly[3];
        al_tangent_basis(g0, lx, ly);
        for (int i = 0; i < F - 1; ++i)
            al_add_pair(L + c.acc, L + c.b, L + c.tA, R + 9 * i, R + 9 * (i + 1), T + 3 * i, T + 3 * (i + 1), L + c.pr + AL_PR * i, tic,
                        true, lx, ly, g0, i, n, lane);
        if (!al_scale_solve(c, L, n, lane)) return AL_NUMERIC;
        const double d0 = x[n - 3], d1 = x[n - 2];
        const double u[3] = {g0[0] + (lx[0] * d0 + ly[0] * d1), g0[1] + (lx[1] * d0 + ly[1] * d1), g0[2] + (lx[2] * d0 + ly[2] * d1)};
        al_normalized(u, g0);
        g0[0] *= g_norm; g0[1] *= g_norm; g0[2] *= g_norm;
        if (!(al_finite(g0[0]) && al_finite(g0[1]) && al_finite(g0[2]))) return AL_NUMERIC;
        __syncthreads();                                    // (every lane has read dg before the next pass overwrites x)
    }
    sc = x[n - 1] / 100.0;
    if (!al_finite(sc)) return AL_NUMERIC;
    if (lane == 0) { res[11] = g0[0]; res[12] = g0[1]; res[13] = g0[2]; res[14] = sc; }
    for (int e = lane; e < 3 * F; e += 64) vbody[e] = x[e];
    if (sc < 0.0) return AL_FAILED_REFINE;
    if (K <= 0) return AL_OK;
    // ---- the window (estimator.cpp:376-435)
    double gn[3], R0[9], Rt[9];
    al_normalized(g0, gn);
    if (1.0 + gn[2] < 1e-12) return AL_NUMERIC;             // FromTwoVectors' SVD branch is not restated
    {   // Utility::g2R: Quaterniond::FromTwoVectors(ng1, (0, 0, 1)) in its regular branch, then its own yaw removed
        double v0[3];
        al_normalized(gn, v0);
        const double sq = sqrt((1.0 + v0[2]) * 2.0), invs = 1.0 / sq;
        const double q[4] = {v0[1] * invs, -v0[0] * invs, 0.0 * invs, sq * 0.5};
        q_to_R(q, Rt);
        al_yaw_times(-al_yaw_deg(Rt), Rt, R0);
    }
    const double* Rs0 = R + 9 * key[0];
    m3_mul(R0, Rs0, Rt);
    {
        double R1[9];
        al_yaw_times(-al_yaw_deg(Rt), R0, R1);
#pragma unroll
        for (int e = 0; e < 9; ++e) R0[e] = R1[e];
    }
    if (lane == 0) {
        double gw[3];
        m3_vec(R0, g0, gw);
        for (int i = 0; i < 3; ++i) res[15 + i] = gw[i];
        for (int e = 0; e < 9; ++e) res[18 + e] = R0[e];
    }
    if (lane < K) {
        const int f = key[lane], f0 = key[0];
        const double* Rk = R + 9 * f;
        double a[3], a0[3], P[3], V[3], o[3];
        m3_vec(Rk, tic, a);
        m3_vec(Rs0, tic, a0);
#pragma unroll
        for (int i = 0; i < 3; ++i) P[i] = sc * T[3 * f + i] - a[i] - (sc * T[3 * f0 + i] - a0[i]);
        // Vs[kv] = frame.R * x.segment<3>(kv * 3): x is indexed by the KEY-FRAME counter, not by the frame's position (:406-415)
        const double xv[3] = {x[3 * lane], x[3 * lane + 1], x[3 * lane + 2]};
        m3_vec(Rk, xv, V);
        double* w = win + AL_WIN * lane;
        m3_vec(R0, P, o);
        w[0] = o[0]; w[1] = o[1]; w[2] = o[2];
        m3_mul(R0, Rk, Rt);
#pragma unroll
        for (int e = 0; e < 9; ++e) w[3 + e] = Rt[e];
        m3_vec(R0, V, o);
        w[12] = o[0]; w[13] = o[1]; w[14] = o[2];
    }
    return AL_OK;
}
