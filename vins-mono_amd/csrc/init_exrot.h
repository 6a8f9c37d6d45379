// init_exrot.h — vg_init_exrot: InitialEXRotation::CalibrationExRotation (initial/initial_ex_rotation.cpp) for N windows, a run of S
// consecutive calls of the reference's member per window.  include/vinsgpu.h defines the call statement by statement; this file is its
// device code and its host entry.  It is included at the END of fe_ransac.hip, after init_relpose.h, whose RANSAC kernels, decomposition
// and triangulation it uses as they are.  Compiled with -ffp-contract=off like the rest of the unit.
//
// A STREAM is one (window, step) pair; NS of them in a call.  Launches on the handle's stream between one upload and one download:
//   ex_gather_kernel     one wavefront per stream: the float32 point sets, the branch (identity / LMedS / RANSAC), the control block
//   rp_ransac7_kernel    \
//   rp_count_kernel       > init_relpose.h's three kernels in its chunked two-part scheme, over the streams of the RANSAC branch
//   rp_pick_kernel       /
//   ex_rot_kernel        one wavefront per stream: rp_decompose uniformly, the lanes over the points, four front counts by ballots, the pick
//   ex_calib_kernel      one wavefront per window, sequential over its steps: record i is the 4x4 block of lane i, the column products of
//                        the one-sided Jacobi are wavefront reductions
// A stream of the LMedS branch (9 .. 14 correspondences) gets its model from vg_fe_reject_with_f's kernels BEFORE the upload, as the front
// end's fall-back streams do; a stream whose n-only schedule holds a redrawn sample is repeated with the exact schedule, as in
// vg_init_relpose, and the rotation and calibration stages run once more.
#pragma once

#define EX_WI 4                     // ints per window: S | n_prev | first stream | first row of prev
#define EX_BRANCH 17                // a free slot of the relpose control block: 0 identity, 1 LMedS, 2 RANSAC
// doubles per window in RpDev::par (RP_PAR): thresh2 (a float, widened) | min_points | huber_deg | min_frames | cov_threshold | - | - | -
static_assert(EX_BRANCH > RP_MAXIT && EX_BRANCH < RP_CTL_INTS, "the branch slot is free");

struct ExDev {
    int NS, W, cap;
    const int* wi;                  // [W][EX_WI]
    const int* swin;                // [NS][2] window, step
    const int* cn;                  // [NS] correspondences of the stream
    const int* coff;                // [NS] its first row of corr
    const double* par;              // [W][RP_PAR]
    const double* ricp;             // [W][9] ric_prev
    const double* prev;             // [][27] the carried records, window after window
    const double* dq;               // [NS][4] w x y z
    const double* fin;              // [NS][9] the model of a stream of the LMedS branch (zeros: none)
    const double* corr;             // x0 y0 x1 y1 rows
    int* ctl;                       // [NS][RP_CTL_INTS]
    double* res;                    // [NS][RP_RES] F 9 | -
    float *p1, *p2;                 // [NS][cap][2]
    double* rec;                    // [NS][27] Rc | Rimu | Rc_g
    double* ric;                    // [NS][9]
    double* sig;                    // [NS][4]
    double* hub;                    // [NS]
    int* okc;                       // [NS][2] ok | the 4N x 4 Jacobi ended inside its cap
    int* wout;                      // [W][2] status, first_ok
    double* calib;                  // [W][9]
};

extern "C" __global__ __launch_bounds__(64) void ex_gather_kernel(ExDev b) {
    const int c = blockIdx.x, lane = threadIdx.x;
    if (c >= b.NS) return;
    const int n = b.cn[c];
    const double* r = b.corr + 4 * (size_t)b.coff[c];
    float* p1 = b.p1 + (size_t)c * b.cap * 2;
    float* p2 = b.p2 + (size_t)c * b.cap * 2;
    for (int k = lane; k < n; k += 64) {
        p1[2 * k] = (float)r[4 * k]; p1[2 * k + 1] = (float)r[4 * k + 1]; p2[2 * k] = (float)r[4 * k + 2]; p2[2 * k + 1] = (float)r[4 * k + 3];
    }
    const int min_points = (int)b.par[(size_t)RP_PAR * b.swin[2 * c] + 1];
    const int branch = n < min_points ? 0 : (n < 15 ? 1 : 2);
    int* ctl = b.ctl + (size_t)c * RP_CTL_INTS;
    double* res = b.res + (size_t)RP_RES * c;
    const double* fin = b.fin + 9 * (size_t)c;
    if (lane < 9) res[lane] = branch == 1 ? fin[lane] : 0.0;
    if (lane == 0) {
        for (int k = 0; k < RP_CTL_INTS; ++k) ctl[k] = 0;
        bool have = false;
        for (int k = 0; k < 9; ++k) have = have || fin[k] != 0.0;
        ctl[RP_N] = n; ctl[RP_GATE] = branch == 2 ? 1 : 0; ctl[RP_RUN] = ctl[RP_GATE]; ctl[RP_XS] = -1; ctl[RP_MAXIT] = FE_RANSAC_MAXIT;
        ctl[RP_BEST] = (branch == 1 && have) ? 0 : -1;
        ctl[EX_BRANCH] = branch;
    }
}

// Eigen's 3x3 inverse (compute_inverse_size3): cofactors over the determinant, the determinant from the first column
DEV void ex_inv3(const double* m, double* o) {
#define EX_COF(i, j) (m[3 * (((i) + 1) % 3) + ((j) + 1) % 3] * m[3 * (((i) + 2) % 3) + ((j) + 2) % 3] - m[3 * (((i) + 1) % 3) + ((j) + 2) % 3] * m[3 * (((i) + 2) % 3) + ((j) + 1) % 3])
    const double c00 = EX_COF(0, 0), c10 = EX_COF(1, 0), c20 = EX_COF(2, 0);
    const double det = (c00 * m[0] + c10 * m[3]) + c20 * m[6];
    const double invdet = 1.0 / det;
    o[0] = c00 * invdet; o[1] = c10 * invdet; o[2] = c20 * invdet;
    o[3] = EX_COF(0, 1) * invdet; o[4] = EX_COF(1, 1) * invdet; o[5] = EX_COF(2, 1) * invdet;
    o[6] = EX_COF(0, 2) * invdet; o[7] = EX_COF(1, 2) * invdet; o[8] = EX_COF(2, 2) * invdet;
#undef EX_COF
}

// Quaterniond(Matrix3d) (ba_math.h: R_to_q) with the three cases of its second branch written out: q is x y z w, nothing is indexed at
// run time
DEV void ex_R_to_q(const double* m, double* q) {
    double t = m[0] + m[4] + m[8];
    if (t > 0) {
        t = sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m[7] - m[5]) * t; q[1] = (m[2] - m[6]) * t; q[2] = (m[3] - m[1]) * t;
    } else if (!(m[4] > m[0]) && !(m[8] > m[0])) {             // i = 0, j = 1, k = 2
        t = sqrt(m[0] - m[4] - m[8] + 1.0);
        q[0] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (m[7] - m[5]) * t; q[1] = (m[3] + m[1]) * t; q[2] = (m[6] + m[2]) * t;
    } else if (m[4] > m[0] && !(m[8] > m[4])) {                // i = 1, j = 2, k = 0
        t = sqrt(m[4] - m[8] - m[0] + 1.0);
        q[1] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (m[2] - m[6]) * t; q[2] = (m[7] + m[5]) * t; q[0] = (m[1] + m[3]) * t;
    } else {                                                   // i = 2, j = 0, k = 1
        t = sqrt(m[8] - m[0] - m[4] + 1.0);
        q[2] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (m[3] - m[1]) * t; q[0] = (m[2] + m[6]) * t; q[1] = (m[5] + m[7]) * t;
    }
}

// huber * (L - R) of one record (initial_ex_rotation.cpp:23-49), row-major 4x4; returns the Huber weight
DEV double ex_block(const double* Rc, const double* Rimu, const double* Rcg, const double huber_deg, double* B) {
    double a[4], g[4], m[4];                                   // x y z w
    ex_R_to_q(Rc, a); ex_R_to_q(Rcg, g); ex_R_to_q(Rimu, m);
    // d = r1 * r2.conjugate(), Eigen's product
    const double bw = g[3], bx = -g[0], by = -g[1], bz = -g[2];
    const double dw = a[3] * bw - a[0] * bx - a[1] * by - a[2] * bz;
    const double dx = a[3] * bx + a[0] * bw + a[1] * bz - a[2] * by;
    const double dy = a[3] * by + a[1] * bw + a[2] * bx - a[0] * bz;
    const double dz = a[3] * bz + a[2] * bw + a[0] * by - a[1] * bx;
    const double ang = (180.0 / 3.14159265358979323846) * (2.0 * atan2(sqrt(dx * dx + dy * dy + dz * dz), fabs(dw)));
    const double huber = ang > huber_deg ? huber_deg / ang : 1.0;
    const double w = a[3], x = a[0], y = a[1], z = a[2], W = m[3], X = m[0], Y = m[1], Z = m[2];
    B[0] = huber * (w - W);    B[1] = huber * (-z - Z);   B[2] = huber * (y - -Y);   B[3] = huber * (x - X);
    B[4] = huber * (z - -Z);   B[5] = huber * (w - W);    B[6] = huber * (-x - X);   B[7] = huber * (y - Y);
    B[8] = huber * (-y - Y);   B[9] = huber * (x - -X);   B[10] = huber * (w - W);   B[11] = huber * (z - Z);
    B[12] = huber * (-x - -X); B[13] = huber * (-y - -Y); B[14] = huber * (-z - -Z); B[15] = huber * (w - W);
    return huber;
}

// the sum of one value per lane over the wavefront: six butterfly steps, every lane ends with the same bits
DEV double ex_wave_sum(double s) {
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) s += __shfl_xor(s, h);
    return s;
}

// One wavefront per stream: solveRelativeR after findFundamentalMat (decomposeE, four testTriangulation, the pick), Rc transposed.
// `second`: the submission that repeats the streams with an exact schedule; the others keep what they have.
extern "C" __global__ __launch_bounds__(64) void ex_rot_kernel(ExDev b, int second) {
    const int cam = blockIdx.x, lane = threadIdx.x;
    if (cam >= b.NS) return;
    int* ctl = b.ctl + (size_t)cam * RP_CTL_INTS;
    if (second && ctl[RP_RUN] == 0) return;
    double* rc = b.rec + 27 * (size_t)cam;
    const int branch = ctl[EX_BRANCH];
    if (branch == 0 || ctl[RP_BEST] < 0) {                 // identity; a branch that found no model is numeric
        if (lane < 9) rc[lane] = (lane % 4 == 0) ? 1.0 : 0.0;
        if (lane == 0) { ctl[RP_NUMERIC] = branch != 0 ? 1 : 0; ctl[RP_WINNER] = 0; ctl[RP_GOOD] = ctl[RP_GOOD + 1] = ctl[RP_GOOD + 2] = ctl[RP_GOOD + 3] = 0; }
        return;
    }
    const int n = ctl[RP_N], nw = (n + 63) >> 6;
    const float* __restrict__ p1 = b.p1 + (size_t)cam * b.cap * 2;
    const float* __restrict__ p2 = b.p2 + (size_t)cam * b.cap * 2;
    const double* res = b.res + (size_t)RP_RES * cam;
    double E[9], R1[9], R2[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) E[k] = res[k];
    const bool conv = rp_decompose(E, R1, R2, t);
    // P1 is a Matx34f: R and t rounded to float32 and widened
    double R1f[9], R2f[9], tf[3], tmf[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) { R1f[k] = (double)(float)R1[k]; R2f[k] = (double)(float)R2[k]; }
#pragma unroll
    for (int k = 0; k < 3; ++k) { tf[k] = (double)(float)t[k]; tmf[k] = -tf[k]; }
    int front[4] = {0, 0, 0, 0};                           // (R1,t1) (R1,t2) (R2,t1) (R2,t2)
    for (int w = 0; w < nw; ++w) {
        const int i = 64 * w + lane;
        const bool valid = i < n;
        const double x0 = valid ? (double)p1[2 * i] : 0.0, y0 = valid ? (double)p1[2 * i + 1] : 0.0;
        const double x1 = valid ? (double)p2[2 * i] : 0.0, y1 = valid ? (double)p2[2 * i + 1] : 0.0;
#pragma unroll
        for (int cand = 0; cand < 4; ++cand) {
            const double* R = cand >= 2 ? R2f : R1f;
            const double* tt = (cand & 1) ? tmf : tf;
            double Q[4];
            rp_triangulate(R, tt, x0, y0, x1, y1, Q);
            // the point cloud is CV_32F; col / normal_factor is a float32 scaling by the float32 reciprocal; P (col / w) is summed in
            // double over the widened operands, left to right, and stored as float32
            const float q0 = (float)Q[0], q1 = (float)Q[1], q2 = (float)Q[2], q3 = (float)Q[3];
            const float inv = (float)(1.0 / (double)q3);
            const float a0 = q0 * inv, a1 = q1 * inv, a2 = q2 * inv, a3 = q3 * inv;
            const float zl = (float)(0.0 * (double)a0 + 0.0 * (double)a1 + 1.0 * (double)a2 + 0.0 * (double)a3);
            const float zr = (float)(R[6] * (double)a0 + R[7] * (double)a1 + R[8] * (double)a2 + tt[2] * (double)a3);
            front[cand] += __popcll(__ballot(valid && zl > 0.f && zr > 0.f));
        }
    }
    const double r11 = (double)front[0] / n, r12 = (double)front[1] / n, r21 = (double)front[2] / n, r22 = (double)front[3] / n;
    const double ratio1 = r11 > r12 ? r11 : r12, ratio2 = r21 > r22 ? r21 : r22;
    const bool first = ratio1 > ratio2;
    if (lane < 9) {
        const int rr = lane / 3, cc = lane % 3;            // ans_R_eigen(j, i) = ans_R_cv(i, j)
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < 9; ++k) v = (k == 3 * cc + rr) ? (first ? R1[k] : R2[k]) : v;
        rc[lane] = v;
    }
    if (lane == 0) {
        ctl[RP_NUMERIC] = conv ? 0 : 1; ctl[RP_WINNER] = first ? 1 : 2;
        ctl[RP_GOOD] = front[0]; ctl[RP_GOOD + 1] = front[1]; ctl[RP_GOOD + 2] = front[2]; ctl[RP_GOOD + 3] = front[3];
    }
}

// One wavefront per window, the steps in turn (Rc_g of a step needs ric of the step before).  Record i of the run (the carried ones
// first) is lane i: its 4x4 block huber (L - R) does not change once the record exists, so a step adds one block and decomposes a copy.
extern "C" __global__ __launch_bounds__(64) void ex_calib_kernel(ExDev b) {
    const int w = blockIdx.x, lane = threadIdx.x;
    if (w >= b.W) return;
    const int* q = b.wi + EX_WI * w;
    const int S = q[0], np = q[1], s0 = q[2];
    const double* par = b.par + (size_t)RP_PAR * w;
    const double huber_deg = par[2], cov = par[4];
    const int min_frames = (int)par[3];
    double B[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) B[k] = 0.0;
    if (lane < np) {
        const double* r = b.prev + 27 * ((size_t)q[3] + lane);
        double Rc[9], Ri[9], Rg[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) { Rc[k] = r[k]; Ri[k] = r[9 + k]; Rg[k] = r[18 + k]; }
        ex_block(Rc, Ri, Rg, huber_deg, B);
    }
    double ric[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) ric[k] = b.ricp[9 * (size_t)w + k];
    int status = VG_EXROT_OK, first_ok = -1;
    for (int k = 0; k < S; ++k) {
        const int c = s0 + k, m = np + k + 1;
        double* rec = b.rec + 27 * (size_t)c;
        if (b.ctl[(size_t)c * RP_CTL_INTS + RP_NUMERIC] != 0) status = VG_EXROT_NUMERIC;
        double Rc[9], Ri[9], Rg[9], T[9], inv[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) Rc[e] = rec[e];
        {
            const double* dq = b.dq + 4 * (size_t)c;
            const double e[4] = {dq[1], dq[2], dq[3], dq[0]};
            q_to_R(e, Ri);
        }
        ex_inv3(ric, inv);
        m3_mul(inv, Ri, T);
        m3_mul(T, ric, Rg);
        double blk[16];
        const double huber = ex_block(Rc, Ri, Rg, huber_deg, blk);
        const bool mine = lane == m - 1;
#pragma unroll
        for (int e = 0; e < 16; ++e) B[e] = mine ? blk[e] : B[e];
        if (lane == 0) {
            for (int e = 0; e < 9; ++e) { rec[9 + e] = Ri[e]; rec[18 + e] = Rg[e]; }
            b.hub[c] = huber;
        }
        // ---- the singular values and the last right singular vector of the 4 m x 4 matrix: one-sided Jacobi on its four columns
        double A[16], V[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) { A[e] = lane < m ? B[e] : 0.0; V[e] = (e % 5 == 0) ? 1.0 : 0.0; }
        double fro = 0.0;
#pragma unroll
        for (int e = 0; e < 16; ++e) fro += A[e] * A[e];
        fro = ex_wave_sum(fro);
        const double signal = 1e-26 * fro;
        bool conv = false;
        for (int sweep = 0; sweep < 40 && !conv; ++sweep) {
            bool big = false;
#pragma unroll
            for (int p = 0; p < 3; ++p)
#pragma unroll
                for (int qq = p + 1; qq < 4; ++qq) {
                    double al = 0.0, be = 0.0, ga = 0.0;
#pragma unroll
                    for (int r = 0; r < 4; ++r) { const double x = A[4 * r + p], y = A[4 * r + qq]; al += x * x; be += y * y; ga += x * y; }
                    al = ex_wave_sum(al); be = ex_wave_sum(be); ga = ex_wave_sum(ga);
                    const double lim = sqrt(al * be);
                    if (fabs(ga) > 1e-16 * lim && ga != 0.0) {
                        big = big || (fabs(ga) > 1e-13 * lim && al > signal && be > signal);
                        const double zeta = (be - al) / (2.0 * ga);
                        const double tn = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                        const double cs = 1.0 / sqrt(1.0 + tn * tn), sn = cs * tn;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const double x = A[4 * r + p], y = A[4 * r + qq];
                            A[4 * r + p] = cs * x - sn * y; A[4 * r + qq] = sn * x + cs * y;
                            const double vx = V[4 * r + p], vy = V[4 * r + qq];
                            V[4 * r + p] = cs * vx - sn * vy; V[4 * r + qq] = sn * vx + cs * vy;
                        }
                    }
                }
            conv = !big;
        }
        double sv[4];
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
            double s2 = 0.0;
#pragma unroll
            for (int r = 0; r < 4; ++r) s2 += A[4 * r + cc] * A[4 * r + cc];
            sv[cc] = ex_wave_sum(s2);
        }
        // descending: the five compare-exchanges (0,1) (2,3) (0,2) (1,3) (1,2), the columns of V along (no index, nothing goes to scratch)
#pragma unroll
        for (int st = 0; st < 5; ++st) {
            const int a = (st == 0 || st == 2) ? 0 : (st == 1 ? 2 : 1), bq = st == 0 ? 1 : (st == 1 || st == 3 ? 3 : 2);
            const bool sw = sv[bq] > sv[a];
            const double ta = sv[a];
            sv[a] = sw ? sv[bq] : ta; sv[bq] = sw ? ta : sv[bq];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double vx = V[4 * r + a], vy = V[4 * r + bq];
                V[4 * r + a] = sw ? vy : vx; V[4 * r + bq] = sw ? vx : vy;
            }
        }
        // Quaterniond(x): the coefficients x y z w; ric = toRotationMatrix().inverse()
        const double xq[4] = {V[3], V[7], V[11], V[15]};
        double Rx[9];
        q_to_R(xq, Rx);
        ex_inv3(Rx, ric);
        const double s2v = sqrt(sv[2]);
        const bool ok = m >= min_frames && s2v > cov;
        if (!conv) status = VG_EXROT_NUMERIC;
        if (ok && first_ok < 0) {
            first_ok = m;
            if (lane == 0) for (int e = 0; e < 9; ++e) b.calib[9 * (size_t)w + e] = ric[e];
        }
        if (lane == 0) {
            for (int e = 0; e < 9; ++e) b.ric[9 * (size_t)c + e] = ric[e];
            b.sig[4 * (size_t)c] = sqrt(sv[0]); b.sig[4 * (size_t)c + 1] = sqrt(sv[1]); b.sig[4 * (size_t)c + 2] = s2v; b.sig[4 * (size_t)c + 3] = sqrt(sv[3]);
            b.okc[2 * (size_t)c] = ok ? 1 : 0; b.okc[2 * (size_t)c + 1] = conv ? 1 : 0;
        }
    }
    if (lane == 0) {
        if (status != VG_EXROT_OK) {
            first_ok = -1;
            for (int e = 0; e < 9; ++e) b.calib[9 * (size_t)w + e] = 0.0;
        } else if (first_ok < 0) {
            for (int e = 0; e < 9; ++e) b.calib[9 * (size_t)w + e] = 0.0;
        }
        b.wout[2 * w] = status; b.wout[2 * w + 1] = first_ok;
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
extern "C" int vg_init_exrot(vg_handle* h, int n_windows, const vg_exrot_in* in, vg_exrot_out* out) {
    VG_RANGE("vg_init_exrot");
    if (!h) return VG_ERR_BAD_ARG;
    auto bad = [&](int w, const char* what) {
        h->err = "vg_init_exrot: window " + std::to_string(w) + ": " + what;
        return VG_ERR_BAD_ARG;
    };
    if (n_windows <= 0 || !in || !out) { h->err = "vg_init_exrot: n_windows <= 0 or a NULL argument"; return VG_ERR_BAD_ARG; }
    // ---- everything that follows from the arguments alone, before anything is uploaded or written
    size_t NS = 0, nRows = 0, nPrev = 0;
    int nmax = 15;
    for (int w = 0; w < n_windows; ++w) {
        const vg_exrot_in& a = in[w];
        if (a.struct_size != sizeof(vg_exrot_in)) return bad(w, "vg_exrot_in::struct_size");
        if (out[w].struct_size != sizeof(vg_exrot_out)) return bad(w, "vg_exrot_out::struct_size");
        const int S = a.n_steps;
        if (S < 1) return bad(w, "n_steps < 1");
        if (a.n_prev < 0) return bad(w, "n_prev < 0");
        if ((long long)a.n_prev + S > VG_EXROT_MAX_STEPS) return bad(w, "n_prev + n_steps above VG_EXROT_MAX_STEPS");
        if (!a.corr_off || !a.delta_q || !a.ric_prev || (a.n_prev > 0 && !a.prev)) return bad(w, "a NULL table");
        if (a.corr_off[0] < 0) return bad(w, "corr_off[0] < 0");
        for (int k = 0; k < S; ++k) {
            if (a.corr_off[k + 1] < a.corr_off[k]) return bad(w, "corr_off does not ascend");
            if (a.corr_off[k + 1] - a.corr_off[k] > VG_SFM_MAX_FEATURES) return bad(w, "a step with more than VG_SFM_MAX_FEATURES correspondences");
            nmax = std::max(nmax, a.corr_off[k + 1] - a.corr_off[k]);
        }
        const size_t rows = (size_t)(a.corr_off[S] - a.corr_off[0]);
        if (rows > 0 && !a.corr) return bad(w, "a NULL table");
        if (!(a.ransac_threshold > 0) || !std::isfinite(a.ransac_threshold)) return bad(w, "ransac_threshold is not positive");
        if (a.confidence != 0.99) return bad(w, "a confidence other than 0.99");
        if (!(a.huber_deg > 0) || !std::isfinite(a.huber_deg) || !(a.cov_threshold > 0) || !std::isfinite(a.cov_threshold))
            return bad(w, "huber_deg or cov_threshold is not positive");
        if (a.min_points < 9) return bad(w, "min_points < 9");
        if (rows > 0 && !rp_finite(a.corr + 4 * (size_t)a.corr_off[0], 4 * rows)) return bad(w, "a non-finite input");
        if (!rp_finite(a.delta_q, 4 * (size_t)S) || !rp_finite(a.ric_prev, 9) || (a.n_prev > 0 && !rp_finite(a.prev, 27 * (size_t)a.n_prev)))
            return bad(w, "a non-finite input");
        for (int k = 0; k < S; ++k) {
            const double* dq = a.delta_q + 4 * (size_t)k;
            if (!(dq[0] * dq[0] + dq[1] * dq[1] + dq[2] * dq[2] + dq[3] * dq[3] > 0)) return bad(w, "a delta_q of zero norm");
        }
        NS += S; nRows += rows; nPrev += a.n_prev;
    }
    if (NS > VG_RELPOSE_MAX_STREAMS) { h->err = "vg_init_exrot: more than VG_RELPOSE_MAX_STREAMS (window, step) pairs in one call"; return VG_ERR_BAD_ARG; }
    if (nRows > (size_t)0x1fffffff) { h->err = "vg_init_exrot: too many correspondences for one call"; return VG_ERR_BAD_ARG; }
    const int W = n_windows, cap = (int)rp_up(nmax, 64), words_n = cap / 64;
    // ---- the host image of the upload: ints [wi | swin | cn | coff], doubles [par | ricp | prev | dq | fin | corr]
    const size_t i_wi = 0, i_sw = i_wi + (size_t)EX_WI * W, i_cn = i_sw + 2 * NS, i_co = i_cn + NS, n_int = rp_up(i_co + NS, 2);
    const size_t o_par = 0, o_rp = o_par + (size_t)RP_PAR * W, o_pv = o_rp + 9 * (size_t)W, o_dq = o_pv + 27 * nPrev, o_fin = o_dq + 4 * NS,
                 o_corr = o_fin + 9 * NS, n_in = o_corr + 4 * nRows;
    // the download, in 8-byte units: ctl (ints) | wout (ints) | okc (ints) | res | rec | ric | sig | hub | calib
    const size_t d_ctl = 0, d_wo = d_ctl + NS * RP_CTL_INTS / 2, d_ok = d_wo + W, d_res = d_ok + NS, d_rec = d_res + (size_t)RP_RES * NS, d_ric = d_rec + 27 * NS,
                 d_sig = d_ric + 9 * NS, d_hub = d_sig + 4 * NS, d_cal = d_hub + NS, n_out = d_cal + 9 * (size_t)W;
    std::vector<int> hint(n_int, 0);
    std::vector<double> hin(n_in, 0.0), hout(n_out);
    std::vector<int> lmeds;                                 // the streams of the LMedS branch
    {
        size_t s = 0, row = 0, pv = 0;
        for (int w = 0; w < W; ++w) {
            const vg_exrot_in& a = in[w];
            const int S = a.n_steps;
            int* wi = hint.data() + i_wi + (size_t)EX_WI * w;
            wi[0] = S; wi[1] = a.n_prev; wi[2] = (int)s; wi[3] = (int)pv;
            double* p = hin.data() + o_par + (size_t)RP_PAR * w;
            p[0] = (double)(float)(a.ransac_threshold * a.ransac_threshold);
            p[1] = a.min_points; p[2] = a.huber_deg; p[3] = a.min_frames; p[4] = a.cov_threshold;
            std::copy(a.ric_prev, a.ric_prev + 9, hin.data() + o_rp + 9 * (size_t)w);
            if (a.n_prev > 0) std::copy(a.prev, a.prev + 27 * (size_t)a.n_prev, hin.data() + o_pv + 27 * pv);
            std::copy(a.delta_q, a.delta_q + 4 * (size_t)S, hin.data() + o_dq + 4 * s);
            const size_t rows = (size_t)(a.corr_off[S] - a.corr_off[0]);
            if (rows > 0) std::copy(a.corr + 4 * (size_t)a.corr_off[0], a.corr + 4 * (size_t)a.corr_off[S], hin.data() + o_corr + 4 * row);
            for (int k = 0; k < S; ++k) {
                const int n = a.corr_off[k + 1] - a.corr_off[k];
                hint[i_sw + 2 * (s + k)] = w; hint[i_sw + 2 * (s + k) + 1] = k;
                hint[i_cn + s + k] = n; hint[i_co + s + k] = (int)row + (a.corr_off[k] - a.corr_off[0]);
                if (n >= a.min_points && n < 15) lmeds.push_back((int)(s + k));
            }
            s += S; row += rows; pv += a.n_prev;
        }
    }
    // the float32 point sets of stream s as ex_gather_kernel makes them, the two sets 2 * cap apart
    std::vector<float> pts((size_t)cap * 4);
    auto host_points = [&](size_t s) {
        const int n = hint[i_cn + s];
        const double* r = hin.data() + o_corr + 4 * (size_t)hint[i_co + s];
        for (int k = 0; k < n; ++k) {
            pts[2 * k] = (float)r[4 * k]; pts[2 * k + 1] = (float)r[4 * k + 1];
            pts[2 * cap + 2 * k] = (float)r[4 * k + 2]; pts[2 * cap + 2 * k + 1] = (float)r[4 * k + 3];
        }
        return n;
    };
    // ---- the LMedS branch: the front end's estimate, one stream at a time, before the upload (its model travels with it)
    for (int s : lmeds) {
        const int n = host_points((size_t)s);
        std::vector<uint8_t> st((size_t)n);
        int n_in_l = 0;
        const int rc = vg_fe_reject_with_f(h, pts.data(), pts.data() + 2 * cap, n, in[hint[i_sw + 2 * (size_t)s]].ransac_threshold, st.data(), &n_in_l,
                                           hin.data() + o_fin + 9 * (size_t)s);
        if (rc != VG_OK) return rc;
    }
    hipError_t e = hipSetDevice(h->device);
    auto fail = [&](hipError_t err) { h->err = std::string("vg_init_exrot: ") + hipGetErrorString(err); return VG_ERR_HIP; };
    if (e != hipSuccess) return fail(e);
    // ---- the resident tables and the scratch of vg_init_relpose (its helpers)
    if ((e = rp_resident_tables(h, nmax)) != hipSuccess) return fail(e);
    // ---- device block: [out | in doubles | ints | scratch]
    const size_t b_out = 0, b_in = b_out + n_out * 8, b_int = b_in + n_in * 8, b_p1 = rp_up(b_int + n_int * 4, 256), b_p2 = b_p1 + NS * cap * 2 * sizeof(float);
    const size_t b_md = rp_up(b_p2 + NS * cap * 2 * sizeof(float), 256), b_F = b_md + NS * FE_RANSAC_MAXIT * 27 * 8, b_me = b_F + NS * FE_RANSAC_MAXIT * 9 * 8;
    const size_t b_wd = b_me + NS * FE_RANSAC_MAXIT * 8, b_rm = b_wd + NS * FE_RANSAC_MAXIT * (size_t)words_n * 8, b_ct = b_rm + NS * (size_t)words_n * 8;
    const size_t b_xs = rp_up(b_ct + NS * FE_RANSAC_MAXIT * 4, 256);
    const size_t xs_cap = RP_XS_CAP;
    if ((e = rp_scratch(h, b_xs + xs_cap * FE_RANSAC_MAXIT * 7 * 4)) != hipSuccess) return fail(e);
    char* base = (char*)h->relpose_buf;
    double* d_out = (double*)(base + b_out);
    double* d_in = (double*)(base + b_in);
    int* d_int = (int*)(base + b_int);
    ExDev x;
    x.NS = (int)NS; x.W = W; x.cap = cap;
    x.wi = d_int + i_wi; x.swin = d_int + i_sw; x.cn = d_int + i_cn; x.coff = d_int + i_co;
    x.par = d_in + o_par; x.ricp = d_in + o_rp; x.prev = d_in + o_pv; x.dq = d_in + o_dq; x.fin = d_in + o_fin; x.corr = d_in + o_corr;
    x.ctl = (int*)(d_out + d_ctl); x.res = d_out + d_res; x.p1 = (float*)(base + b_p1); x.p2 = (float*)(base + b_p2);
    x.rec = d_out + d_rec; x.ric = d_out + d_ric; x.sig = d_out + d_sig; x.hub = d_out + d_hub; x.okc = (int*)(d_out + d_ok);
    x.wout = (int*)(d_out + d_wo); x.calib = d_out + d_cal;
    RpDev b = {};                                           // what the three RANSAC kernels read and write; the rest stays null
    b.NS = (int)NS; b.W = W; b.cap = cap; b.words_n = words_n;
    rp_table_pointers(h, b);
    b.swin = x.swin; b.par = x.par; b.ctl = x.ctl; b.res = x.res; b.p1 = x.p1; b.p2 = x.p2;
    b.rmask = (unsigned long long*)(base + b_rm);
    b.xsched = (const int*)(base + b_xs);
    b.models = (double*)(base + b_md); b.Fit = (double*)(base + b_F); b.med = (double*)(base + b_me);
    b.words = (unsigned long long*)(base + b_wd); b.count = (int*)(base + b_ct);
    if ((e = hipMemcpyAsync(d_in, hin.data(), n_in * 8, hipMemcpyHostToDevice, h->stream)) != hipSuccess) return fail(e);
    if ((e = hipMemcpyAsync(d_int, hint.data(), n_int * 4, hipMemcpyHostToDevice, h->stream)) != hipSuccess) return fail(e);
    if ((e = hipMemsetAsync(d_out, 0, n_out * 8, h->stream)) != hipSuccess) return fail(e);
    struct Events {                                         // destroyed on every way out
        hipEvent_t ev[VG_EXROT_LAUNCHES + 1] = {};
        ~Events() { for (hipEvent_t v : ev) if (v) (void)hipEventDestroy(v); }
    } evs;
    const bool timed = out[0].device_ms != nullptr;
    if (timed)
        for (int i = 0; i <= VG_EXROT_LAUNCHES; ++i)
            if ((e = hipEventCreate(&evs.ev[i])) != hipSuccess) return fail(e);
    int mark = 0;
    auto stamp = [&](bool on) { return on ? hipEventRecord(evs.ev[mark++], h->stream) : hipSuccess; };
    // the RANSAC stage of the streams whose RP_RUN is set, the rotation stage, the calibration of every window
    auto stages = [&](bool on, int second) -> hipError_t {
        hipError_t r;
        if ((r = rp_ransac_launches(h, b, NS, [&] { return stamp(on); })) != hipSuccess) return r;
        hipLaunchKernelGGL(ex_rot_kernel, dim3((unsigned)NS), dim3(64), 0, h->stream, x, second);
        if ((r = stamp(on)) != hipSuccess) return r;
        hipLaunchKernelGGL(ex_calib_kernel, dim3((unsigned)W), dim3(64), 0, h->stream, x);
        if ((r = stamp(on)) != hipSuccess) return r;
        return hipGetLastError();
    };
    if ((e = stamp(timed)) != hipSuccess) return fail(e);
    hipLaunchKernelGGL(ex_gather_kernel, dim3((unsigned)NS), dim3(64), 0, h->stream, x);
    if ((e = stamp(timed)) != hipSuccess) return fail(e);
    if ((e = stages(timed, 0)) != hipSuccess) return fail(e);
    if ((e = hipMemcpyAsync(hout.data(), d_out, n_out * 8, hipMemcpyDeviceToHost, h->stream)) != hipSuccess) return fail(e);
    if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return fail(e);
    int* ctl = (int*)(hout.data() + d_ctl);
    // ---- the streams whose n-only schedule holds a sample OpenCV would have redrawn: once more with the exact schedule
    std::vector<int> again;
    for (size_t s = 0; s < NS; ++s)
        if (ctl[s * RP_CTL_INTS + RP_GATE] && ctl[s * RP_CTL_INTS + RP_FB]) again.push_back((int)s);
    void* xs_own = nullptr;
    struct Free { void*& p; ~Free() { if (p) (void)hipFree(p); } } xs_free{xs_own};
    if (!again.empty()) {
        std::vector<int> xs;
        rp_exact_schedules(again, ctl, NS, cap, xs, [&](size_t s, float* p) {
            const int n = host_points(s);
            std::copy(pts.begin(), pts.end(), p);
            return n;
        });
        if (again.size() > xs_cap) {
            if ((e = hipMalloc(&xs_own, xs.size() * 4)) != hipSuccess) return fail(e);
            b.xsched = (const int*)xs_own;
        }
        if ((e = hipMemcpyAsync((void*)b.xsched, xs.data(), xs.size() * 4, hipMemcpyHostToDevice, h->stream)) != hipSuccess) return fail(e);
        if ((e = hipMemcpyAsync(b.ctl, ctl, NS * RP_CTL_INTS * 4, hipMemcpyHostToDevice, h->stream)) != hipSuccess) return fail(e);
        if ((e = stages(false, 1)) != hipSuccess) return fail(e);
        if ((e = hipMemcpyAsync(hout.data(), d_out, n_out * 8, hipMemcpyDeviceToHost, h->stream)) != hipSuccess) return fail(e);
        if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return fail(e);
    }
    if (timed)
        for (int i = 0; i < VG_EXROT_LAUNCHES; ++i) {
            float ms = 0.f;
            if ((e = hipEventElapsedTime(&ms, evs.ev[i], evs.ev[i + 1])) != hipSuccess) return fail(e);
            out[0].device_ms[i] = ms;
        }
    const int* wout = (const int*)(hout.data() + d_wo);
    const int* okc = (const int*)(hout.data() + d_ok);
    size_t s0 = 0;
    for (int w = 0; w < W; ++w) {
        const int S = in[w].n_steps;
        vg_exrot_out& o = out[w];
        o.status = wout[2 * w]; o.first_ok = wout[2 * w + 1];
        std::copy(hout.data() + d_cal + 9 * (size_t)w, hout.data() + d_cal + 9 * (size_t)w + 9, o.calib_ric);
        for (int k = 0; k < S; ++k) {
            const size_t s = s0 + k;
            const int* c = ctl + s * RP_CTL_INTS;
            const bool g = c[EX_BRANCH] == 2;
            if (o.records) std::copy(hout.data() + d_rec + 27 * s, hout.data() + d_rec + 27 * s + 27, o.records + 27 * (size_t)k);
            if (o.ric) std::copy(hout.data() + d_ric + 9 * s, hout.data() + d_ric + 9 * s + 9, o.ric + 9 * (size_t)k);
            if (o.sigma) std::copy(hout.data() + d_sig + 4 * s, hout.data() + d_sig + 4 * s + 4, o.sigma + 4 * (size_t)k);
            if (o.ok) o.ok[k] = okc[2 * s];
            if (o.huber) o.huber[k] = hout[d_hub + s];
            if (o.branch) o.branch[k] = c[EX_BRANCH];
            // (as vg_init_relpose: the last iteration the loop looked at)
            const int reach = (c[RP_NITERS] < c[RP_MAXIT] ? c[RP_NITERS] : c[RP_MAXIT]) - 1;
            if (o.ransac_iter) o.ransac_iter[k] = g ? (c[RP_BEST] > reach ? c[RP_BEST] : reach) : 0;
            if (o.ransac_best) o.ransac_best[k] = g ? c[RP_BEST] : 0;
            if (o.ransac_bound) o.ransac_bound[k] = g ? c[RP_NITERS] : 0;
            if (o.ransac_inliers) o.ransac_inliers[k] = g ? c[RP_NIN] : 0;
            if (o.F) for (int q = 0; q < 9; ++q) o.F[9 * (size_t)k + q] = hout[d_res + (size_t)RP_RES * s + q];
            if (o.front) for (int q = 0; q < 4; ++q) o.front[4 * (size_t)k + q] = c[RP_GOOD + q];
            if (o.picked) o.picked[k] = c[RP_WINNER];
            if (o.used_fallback) o.used_fallback[k] = (g && c[RP_XS] >= 0) ? 1 : 0;
        }
        s0 += S;
    }
    return VG_OK;
}
