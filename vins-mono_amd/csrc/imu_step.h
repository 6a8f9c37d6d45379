// imu_step.h — one text for IntegrationBase::push_back (integration_base.h:30-158), shared by imu_preint_kernel
// (csrc/imu_preint.hip: vg_imu_preintegrate), ba_seq_imu_kernel and ba_seq_merge_kernel (csrc/ba_seq.hip: sequences that take raw
// IMU samples).  One wavefront per interval: the 15x15 jacobian and covariance live in LDS; per sample every lane evaluates the
// (tiny, wave-uniform) mid-point update and the 3x3 blocks of F (15x15) and V (15x18) redundantly, then the lanes share
//   jacobian <- F jacobian,   covariance <- F covariance F^T + V diag(noise) V^T
// entry-wise (225 entries over 64 lanes, k ascending like a plain triple loop); three barriers per sample.
//   imu_enter      the state a push_back starts from: the identity (a fresh IntegrationBase) or a stored record (the continuation
//                  of pre_integrations[WINDOW_SIZE - 1] in slideWindow, estimator.cpp:1069-1081)
//   imu_push_back  one sample
//   imu_leave      the record, in the layout of IMU_OUT
// All three are called by the 64 lanes of ONE wavefront that owns `s` (they contain block barriers).
#pragma once
#include "ba_math.h"

#define IMU_OUT 467     // sum_dt | dp 3 | dq 4 | dv 3 | ba 3 | bg 3 | jacobian 225 | covariance 225

struct ImuPreLds {
    double J[2][225], P[225], T[225], F[225], V[15 * 18], nz[18];      // J: the current jacobian is J[ImuRun::jb]
};

// what the lanes keep in registers between two samples (wave-uniform)
struct ImuRun {
    double acc0[3], gyr0[3];        // the measurement the next sample starts from (acc_0 / gyr_0)
    double ba[3], bg[3];            // linearized_ba / linearized_bg
    double dp[3], dv[3], dq[4], sum_dt;
    int jb;                         // which half of ImuPreLds::J holds the jacobian
};

// rec: nullptr (identity) or a stored record [IMU_OUT]; then the biases are the record's own and `bias` is not read
DEV void imu_enter(ImuPreLds& s, ImuRun& r, const double* rec, const double* first, const double* bias,
                   double acc_n, double gyr_n, double acc_w, double gyr_w, int lane) {
    for (int e = lane; e < 225; e += 64) {
        s.J[0][e] = rec ? rec[17 + e] : ((e / 15 == e % 15) ? 1.0 : 0.0);
        s.P[e] = rec ? rec[242 + e] : 0.0;
        s.F[e] = 0.0;
    }
    for (int e = lane; e < 15 * 18; e += 64) s.V[e] = 0.0;
    if (lane < 18) {
        // noise = diag(ACC_N^2 I, GYR_N^2 I, ACC_N^2 I, GYR_N^2 I, ACC_W^2 I, GYR_W^2 I)  (integration_base.h:18-26)
        const int b = lane / 3;
        s.nz[lane] = (b == 0 || b == 2) ? acc_n * acc_n : ((b == 1 || b == 3) ? gyr_n * gyr_n : (b == 4 ? acc_w * acc_w : gyr_w * gyr_w));
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        r.acc0[i] = first[i]; r.gyr0[i] = first[3 + i];
        r.ba[i] = rec ? rec[11 + i] : bias[i]; r.bg[i] = rec ? rec[14 + i] : bias[3 + i];
        r.dp[i] = rec ? rec[1 + i] : 0.0; r.dv[i] = rec ? rec[8 + i] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) r.dq[i] = rec ? rec[4 + i] : (i == 3 ? 1.0 : 0.0);
    r.sum_dt = rec ? rec[0] : 0.0;
    r.jb = 0;
    __syncthreads();
}

// sm: dt acc(3) gyr(3)
DEV void imu_push_back(ImuPreLds& s, ImuRun& run, const double* sm, int lane) {
    double* const acc0 = run.acc0; double* const gyr0 = run.gyr0;
    const double* const ba = run.ba; const double* const bg = run.bg;
    double* const dp = run.dp; double* const dv = run.dv; double* const dq = run.dq;
    const double dt = sm[0];
    const double acc1[3] = {sm[1], sm[2], sm[3]}, gyr1[3] = {sm[4], sm[5], sm[6]};
    // ---- midPointIntegration (integration_base.h:62-72), wave-uniform
    double Rq[9], Rr[9], rq[4];
    q_to_R(dq, Rq);
    const double w[3] = {0.5 * (gyr0[0] + gyr1[0]) - bg[0], 0.5 * (gyr0[1] + gyr1[1]) - bg[1], 0.5 * (gyr0[2] + gyr1[2]) - bg[2]};
    const double hq[4] = {w[0] * dt / 2, w[1] * dt / 2, w[2] * dt / 2, 1.0};
    q_mul(dq, hq, rq);
    q_to_R(rq, Rr);                                   // un-normalised result_delta_q, as the reference uses it
    const double a0[3] = {acc0[0] - ba[0], acc0[1] - ba[1], acc0[2] - ba[2]};
    const double a1[3] = {acc1[0] - ba[0], acc1[1] - ba[1], acc1[2] - ba[2]};
    double u0[3], u1[3];
    m3_vec(Rq, a0, u0);
    m3_vec(Rr, a1, u1);
    const double ua[3] = {0.5 * (u0[0] + u1[0]), 0.5 * (u0[1] + u1[1]), 0.5 * (u0[2] + u1[2])};
    double np_[3], nv[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) { np_[i] = dp[i] + dv[i] * dt + 0.5 * ua[i] * dt * dt; nv[i] = dv[i] + ua[i] * dt; }
    // ---- F, V blocks (integration_base.h:76-129)
    double Rw[9], Ra0[9], Ra1[9], IRw[9], RqA0[9], RrA1[9], RrA1I[9];
    skew3(w, Rw); skew3(a0, Ra0); skew3(a1, Ra1);
#pragma unroll
    for (int i = 0; i < 9; ++i) IRw[i] = ((i % 4 == 0) ? 1.0 : 0.0) - Rw[i] * dt;
    m3_mul(Rq, Ra0, RqA0);
    m3_mul(Rr, Ra1, RrA1);
    m3_mul(RrA1, IRw, RrA1I);
    if (lane < 9) {
        const int r = lane / 3, c = lane % 3, i = lane;
        const double id = (r == c) ? 1.0 : 0.0;
        double* F = s.F;
        double* V = s.V;
        F[(0 + r) * 15 + 0 + c] = id;
        F[(0 + r) * 15 + 3 + c] = -0.25 * RqA0[i] * dt * dt + -0.25 * RrA1I[i] * dt * dt;
        F[(0 + r) * 15 + 6 + c] = id * dt;
        F[(0 + r) * 15 + 9 + c] = -0.25 * (Rq[i] + Rr[i]) * dt * dt;
        F[(0 + r) * 15 + 12 + c] = -0.25 * RrA1[i] * dt * dt * -dt;
        F[(3 + r) * 15 + 3 + c] = IRw[i];
        F[(3 + r) * 15 + 12 + c] = -1.0 * id * dt;
        F[(6 + r) * 15 + 3 + c] = -0.5 * RqA0[i] * dt + -0.5 * RrA1I[i] * dt;
        F[(6 + r) * 15 + 6 + c] = id;
        F[(6 + r) * 15 + 9 + c] = -0.5 * (Rq[i] + Rr[i]) * dt;
        F[(6 + r) * 15 + 12 + c] = -0.5 * RrA1[i] * dt * -dt;
        F[(9 + r) * 15 + 9 + c] = id;
        F[(12 + r) * 15 + 12 + c] = id;
        V[(0 + r) * 18 + 0 + c] = 0.25 * Rq[i] * dt * dt;
        V[(0 + r) * 18 + 3 + c] = 0.25 * -RrA1[i] * dt * dt * 0.5 * dt;
        V[(0 + r) * 18 + 6 + c] = 0.25 * Rr[i] * dt * dt;
        V[(0 + r) * 18 + 9 + c] = 0.25 * -RrA1[i] * dt * dt * 0.5 * dt;
        V[(3 + r) * 18 + 3 + c] = 0.5 * id * dt;
        V[(3 + r) * 18 + 9 + c] = 0.5 * id * dt;
        V[(6 + r) * 18 + 0 + c] = 0.5 * Rq[i] * dt;
        V[(6 + r) * 18 + 3 + c] = 0.5 * -RrA1[i] * dt * 0.5 * dt;
        V[(6 + r) * 18 + 6 + c] = 0.5 * Rr[i] * dt;
        V[(6 + r) * 18 + 9 + c] = 0.5 * -RrA1[i] * dt * 0.5 * dt;
        V[(9 + r) * 18 + 12 + c] = id * dt;
        V[(12 + r) * 18 + 15 + c] = id * dt;
    }
    __syncthreads();
    // ---- jacobian = F * jacobian (into the other jacobian buffer) ; T = F * covariance
    // (a rolled loop over the lane's entries: fully unrolled, the 4 x 45 LDS operands of a lane are all in flight at once and
    //  the kernel spills)
    const double* const Jo = s.J[run.jb];
    double* const Jn = s.J[run.jb ^ 1];
#pragma unroll 1
    for (int e = lane; e < 225; e += 64) {
        const int i = e / 15, j = e - 15 * i;
        double a = 0.0, b = 0.0;
#pragma unroll
        for (int t = 0; t < 15; ++t) { const double f = s.F[i * 15 + t]; a += f * Jo[t * 15 + j]; b += f * s.P[t * 15 + j]; }
        Jn[e] = a; s.T[e] = b;
    }
    __syncthreads();
    // ---- covariance = T * F^T + V * noise * V^T
#pragma unroll 1
    for (int e = lane; e < 225; e += 64) {
        const int i = e / 15, j = e - 15 * i;
        double a = 0.0, b = 0.0;
#pragma unroll
        for (int t = 0; t < 15; ++t) a += s.T[i * 15 + t] * s.F[j * 15 + t];
#pragma unroll
        for (int t = 0; t < 18; ++t) b += s.V[i * 18 + t] * s.nz[t] * s.V[j * 18 + t];
        s.P[e] = a + b;
    }
    // ---- propagate() tail (integration_base.h:147-155)
#pragma unroll
    for (int i = 0; i < 3; ++i) { dp[i] = np_[i]; dv[i] = nv[i]; acc0[i] = acc1[i]; gyr0[i] = gyr1[i]; }
    dq[0] = rq[0]; dq[1] = rq[1]; dq[2] = rq[2]; dq[3] = rq[3];
    {   // Eigen normalize(): divide by the norm
        const double nrm = sqrt(dq[0] * dq[0] + dq[1] * dq[1] + dq[2] * dq[2] + dq[3] * dq[3]);
        dq[0] /= nrm; dq[1] /= nrm; dq[2] /= nrm; dq[3] /= nrm;
    }
    run.sum_dt += dt;
    run.jb ^= 1;
    __syncthreads();                                  // F, V and the old jacobian buffer are free again
}

// o: [IMU_OUT]
DEV void imu_leave(const ImuPreLds& s, const ImuRun& r, double* o, int lane) {
    if (lane == 0) {
        o[0] = r.sum_dt;
        for (int i = 0; i < 3; ++i) { o[1 + i] = r.dp[i]; o[8 + i] = r.dv[i]; o[11 + i] = r.ba[i]; o[14 + i] = r.bg[i]; }
        for (int i = 0; i < 4; ++i) o[4 + i] = r.dq[i];
    }
    for (int e = lane; e < 225; e += 64) { o[17 + e] = s.J[r.jb][e]; o[242 + e] = s.P[e]; }
}
