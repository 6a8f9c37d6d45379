// init_relpose.h — vg_init_relpose: Estimator::relativePose (estimator.cpp:442-471) for N windows, every candidate frame of every
// window at once.  include/vinsgpu.h defines the call statement by statement; this file is its device code and its host entry.  It is
// included at the END of fe_ransac.hip: the RANSAC stage compiles the two bodies of that file (fe_ransac7_body.h,
// fe_ransac_count_body.h) once more with a (window, candidate) pair as the stream, and the host part uses that file's schedule and bound
// functions (get_subset, update_num_iters, fe_ransac_tables).  Compiled with -ffp-contract=off like the rest of the unit.
//
// A STREAM is one (window, candidate i) pair; NS of them in a call.  Launches on the handle's stream between one upload and one download:
//   rp_gather_kernel     one workgroup per stream: getCorresponding by ballots and prefix counts in feature order, the float32 point
//                        sets, n_corres, the parallax sum in the fixed order the header names, the gate
//   rp_ransac7_kernel    \  iterations [0, RP_CHUNK0) of every gated stream and the collinearity test of its whole schedule, then the
//   rp_count_kernel       > bookkeeping; a second round of the three for [RP_CHUNK0, bound): the two-part scheme of
//   rp_pick_kernel       /  vg_fe_read_image_batch (fe_ransac.hip has the argument why two parts give the outputs of one)
//   rp_pose_kernel       one wavefront per gated stream: the 3x3 SVD uniformly, the lanes over the points, four null vectors per point,
//                        masks and counts by ballots
//   rp_window_kernel     one thread per window: the first candidate in ascending order that is gated and succeeded
// No atomics in any sum (the one atomicOr raises the collinearity flag).
#pragma once

#define RP_CHUNK0 63                // iterations every gated stream evaluates before the bookkeeping first looks (9 wavefronts of 7)
#define RP_P2_WAVES 24              // wavefronts per stream of the second part's sample kernel (each takes 7 iterations in turn)
#define RP_P2_COUNT 64              // wavefronts per stream of the second part's count kernel
#define RP_NT 256                   // threads of the gather workgroup
static_assert(FE_RANSAC_MAXPTS >= VG_SFM_MAX_FEATURES, "a candidate's correspondences fit the RANSAC kernels' point capacity");
enum {
    RP_N = 0,          // n_corres
    RP_GATE,           // the gate passed
    RP_RUN,            // this submission runs the stream's RANSAC and pose stages
    RP_FB,             // a sample of the n-only schedule would have been redrawn (RI_FB_COLLINEAR)
    RP_BEST,           // iteration whose model won (-1: none)
    RP_NITERS,         // the bound
    RP_MAXGOOD,        // carried between the two parts of the bookkeeping
    RP_XS,             // slot of the stream's exact schedule (-1: the row of the n-only table)
    RP_NIN,            // inliers of the winning model
    RP_NUMERIC,        // the 3x3 SVD did not converge
    RP_WINNER,         // 0 .. 3
    RP_CNT,            // inlier_cnt
    RP_GOOD,           // [4]
    RP_MAXIT = 16,     // iterations of the stream's schedule (FE_RANSAC_MAXIT unless the exact schedule ran out of samples)
    RP_CTL_INTS = 20
};
#define RP_WI 6                     // ints per window: F | n_feat | first feature | first observation row | first stream | -
#define RP_PAR 8                    // doubles per window: thresh2 (a float, widened) | min_corres | gate | focal | min_inliers | dist | - | -
#define RP_RES 24                   // doubles per stream: F 9 | relative_R 9 | relative_T 3 | -

struct RpDev {
    int NS, W, cap, words_n, tab_stride;
    const int* wi;                  // [W][RP_WI]
    const int* swin;                // [NS][2] window, candidate
    const int *start, *nobs, *off;  // the windows' feature tables, one after the other
    const double* par;              // [W][RP_PAR]
    const double* obs;              // x y rows
    int* ctl;                       // [NS][RP_CTL_INTS]
    int* wout;                      // [W][2] l, status
    double* avg;                    // [NS] average_parallax
    double* res;                    // [NS][RP_RES]
    unsigned long long* rmask;      // [NS][words_n] the RANSAC mask
    unsigned long long* mask;       // [NS][words_n] the winner's mask (RANSAC and cheirality)
    float *p1, *p2;                 // [NS][cap][2]
    const int* sched;               // [nmax - 14][FE_RANSAC_MAXIT][7] the n-only schedules
    const int* niters_tab;          // [nmax + 1][tab_stride]
    const int* xsched;              // [slots][FE_RANSAC_MAXIT][7] exact schedules of the second submission
    double* models;                 // [NS][FE_RANSAC_MAXIT][3][9]
    double* Fit;                    // [NS][FE_RANSAC_MAXIT][9]
    double* med;                    // [NS][FE_RANSAC_MAXIT] (what the count body writes beside the model; not read)
    int* count;                     // [NS][FE_RANSAC_MAXIT]
    unsigned long long* words;      // [NS][FE_RANSAC_MAXIT][words_n]
    unsigned long long* mask4;      // [NS][4][words_n] the masks of the four candidates of recoverPose
};

extern "C" __global__ __launch_bounds__(RP_NT) void rp_gather_kernel(RpDev b) {
    __shared__ double term[FE_RANSAC_MAXPTS];
    __shared__ double red[RP_NT];
    __shared__ int wcnt[RP_NT / 64];
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (c >= b.NS) return;
    const int w = b.swin[2 * c], i = b.swin[2 * c + 1];
    const int* q = b.wi + RP_WI * w;
    const int F = q[0], n = q[1];
    const int *start = b.start + q[2], *nobs = b.nobs + q[2], *off = b.off + q[2];
    const double* obs = b.obs + 2 * (size_t)q[3];
    float* p1 = b.p1 + (size_t)c * b.cap * 2;
    float* p2 = b.p2 + (size_t)c * b.cap * 2;
    int base = 0;
    for (int j0 = 0; j0 < n; j0 += RP_NT) {
        const int j = j0 + tid;
        bool in = false;
        double x0 = 0, y0 = 0, x1 = 0, y1 = 0;
        if (j < n) {
            const int s = start[j], k = nobs[j];
            in = s <= i && s + k - 1 >= F - 1;
            if (in) {
                const double* r = obs + 2 * (size_t)off[j];
                x0 = r[2 * (i - s)]; y0 = r[2 * (i - s) + 1]; x1 = r[2 * (F - 1 - s)]; y1 = r[2 * (F - 1 - s) + 1];
            }
        }
        const unsigned long long bal = __ballot(in);
        if (lane == 0) wcnt[wv] = __popcll(bal);
        __syncthreads();
        int pos = base + __popcll(bal & ((1ull << lane) - 1ull));
        for (int u = 0; u < RP_NT / 64; ++u) { if (u < wv) pos += wcnt[u]; base += wcnt[u]; }
        if (in) {
            p1[2 * pos] = (float)x0; p1[2 * pos + 1] = (float)y0; p2[2 * pos] = (float)x1; p2[2 * pos + 1] = (float)y1;
            const double dx = x0 - x1, dy = y0 - y1;
            term[pos] = sqrt(dx * dx + dy * dy);
        }
        __syncthreads();
    }
    // the parallax sum: s[t] = d[t] + d[t + 256] + ..., then the halving tree
    double s = 0.0;
    for (int k = tid; k < base; k += RP_NT) s += term[k];
    red[tid] = s;
    __syncthreads();
    for (int h = RP_NT / 2; h >= 1; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    if (tid == 0) {
        const double* par = b.par + (size_t)RP_PAR * w;
        const double avg = base > 0 ? red[0] / base : 0.0;
        const bool gate = base > (int)par[1] && avg * par[3] > par[2];
        int* ctl = b.ctl + (size_t)c * RP_CTL_INTS;
        for (int k = 0; k < RP_CTL_INTS; ++k) ctl[k] = 0;
        ctl[RP_N] = base; ctl[RP_GATE] = gate ? 1 : 0; ctl[RP_RUN] = gate ? 1 : 0; ctl[RP_BEST] = -1; ctl[RP_XS] = -1;
        ctl[RP_MAXIT] = FE_RANSAC_MAXIT;
        b.avg[c] = avg;
    }
}

// the stream's schedule and the end of this launch's iterations (fe_ransac.hip: rb_ransac_end)
DEV const int* rp_sched(const RpDev& b, const int* ctl) {
    return ctl[RP_XS] >= 0 ? b.xsched + (size_t)ctl[RP_XS] * 7 * FE_RANSAC_MAXIT : b.sched + (size_t)(ctl[RP_N] - 15) * 7 * FE_RANSAC_MAXIT;
}
DEV int rp_end(const int* ctl, const int first, int end) {
    if (first > 0 && ctl[RP_NITERS] < end) end = ctl[RP_NITERS];
    return ctl[RP_MAXIT] < end ? ctl[RP_MAXIT] : end;
}

extern "C" __global__ __launch_bounds__(64) void rp_ransac7_kernel(RpDev b, int first, int end) {
    const int cam = blockIdx.y;
    int* const sctl = b.ctl + (size_t)cam * RP_CTL_INTS;
    if (sctl[RP_RUN] == 0) return;
    const int* __restrict__ sched = rp_sched(b, sctl);
    const float* __restrict__ p1 = b.p1 + (size_t)cam * b.cap * 2;
    const float* __restrict__ p2 = b.p2 + (size_t)cam * b.cap * 2;
    double* __restrict__ models = b.models + (size_t)cam * FE_RANSAC_MAXIT * 27;
    if (first == 0 && sctl[RP_XS] < 0)
        for (int q = blockIdx.x * 64 + threadIdx.x; q < FE_RANSAC_MAXIT; q += gridDim.x * 64) {
            int idx[7];
#pragma unroll
            for (int i = 0; i < 7; ++i) idx[i] = sched[(size_t)q * 7 + i];
            if (fr_last_collinear(p1, idx) || fr_last_collinear(p2, idx)) atomicOr(&sctl[RP_FB], RI_FB_COLLINEAR);
        }
    const int nsched = rp_end(sctl, first, end);
#pragma unroll 1
    for (int k0 = first + blockIdx.x * FR_PER_WAVE; k0 < nsched; k0 += gridDim.x * FR_PER_WAVE) {
#define FR_FIRST_SAMPLE k0
#include "fe_ransac7_body.h"
#undef FR_FIRST_SAMPLE
    }
}

extern "C" __global__ __launch_bounds__(64) void rp_count_kernel(RpDev b, int first, int end) {
    const int cam = blockIdx.y, lane = threadIdx.x;
    const int* sctl = b.ctl + (size_t)cam * RP_CTL_INTS;
    if (sctl[RP_RUN] == 0) return;
    const int n = sctl[RP_N];
    const float* __restrict__ p1 = b.p1 + (size_t)cam * b.cap * 2;
    const float* __restrict__ p2 = b.p2 + (size_t)cam * b.cap * 2;
    const double* __restrict__ models = b.models + (size_t)cam * FE_RANSAC_MAXIT * 27;
    double* __restrict__ Fout = b.Fit + (size_t)cam * FE_RANSAC_MAXIT * 9;
    double* __restrict__ median = b.med + (size_t)cam * FE_RANSAC_MAXIT;
    int* __restrict__ count = b.count + (size_t)cam * FE_RANSAC_MAXIT;
    // (a row of ceil(n / 64) words per iteration, as the body lays them out; words_n is the capacity)
    unsigned long long* __restrict__ inl_words = b.words + (size_t)cam * FE_RANSAC_MAXIT * b.words_n;
    const float thresh2 = (float)b.par[(size_t)RP_PAR * b.swin[2 * cam]];
    const int lmeds = 0;
    end = rp_end(sctl, first, end);
#pragma unroll 1
    for (int k0 = first + blockIdx.x; k0 < end; k0 += gridDim.x) {
        const int k = k0;
#include "fe_ransac_count_body.h"
    }
}

// The registrator's loop over the iterations [it0, stop) (fe_frame.hip: ri_pick_body), one wavefront per stream; `final`: the last part,
// which also hands the winner's model, inlier count and inlier words on.
extern "C" __global__ __launch_bounds__(64) void rp_pick_kernel(RpDev b, int it0, int stop, int final) {
    const int cam = blockIdx.x, lane = threadIdx.x;
    if (cam >= b.NS) return;
    int* ctl = b.ctl + (size_t)cam * RP_CTL_INTS;
    if (ctl[RP_RUN] == 0) return;
    const int n = ctl[RP_N];
    const int* count = b.count + (size_t)cam * FE_RANSAC_MAXIT;
    int niters = ctl[RP_MAXIT], max_good = 0, best = -1;
    if (it0 > 0) { niters = ctl[RP_NITERS]; max_good = ctl[RP_MAXGOOD]; best = ctl[RP_BEST]; }
    if (stop > ctl[RP_MAXIT]) stop = ctl[RP_MAXIT];
    const int* tab = b.niters_tab + (size_t)n * b.tab_stride;
    for (int base = it0; base < stop && base < niters; base += 64) {
        const int mine = base + lane < stop ? count[base + lane] : -1;
        for (int j = 0; j < 64 && base + j < niters && base + j < stop; ++j) {
            const int c = __shfl(mine, j);
            if (c > (max_good > 6 ? max_good : 6)) {
                best = base + j; max_good = c;
                const int t = tab[c];
                niters = t < niters ? t : niters;
            }
        }
    }
    if (lane == 0) { ctl[RP_BEST] = best; ctl[RP_NITERS] = niters; ctl[RP_MAXGOOD] = max_good; }
    if (!final) return;
    const int nw = (n + 63) >> 6;
    double* res = b.res + (size_t)RP_RES * cam;
    if (lane < 9) res[lane] = best < 0 ? 0.0 : b.Fit[((size_t)cam * FE_RANSAC_MAXIT + best) * 9 + lane];
    if (lane < nw)
        b.rmask[(size_t)cam * b.words_n + lane] = best < 0 ? 0ull : b.words[(size_t)cam * FE_RANSAC_MAXIT * b.words_n + (size_t)best * nw + lane];
    if (lane == 0) ctl[RP_NIN] = best < 0 ? 0 : max_good;
}

// ---- the pose stage ----------------------------------------------------------------------------------------------------------------
// decomposeEssentialMat with the SVD the header states; false: the sweeps did not end inside the cap
DEV bool rp_decompose(const double* E, double* R1, double* R2, double* t) {
    double A[9], V[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) { A[k] = E[k]; V[k] = (k % 4 == 0) ? 1.0 : 0.0; }
    double fro = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) fro += A[k] * A[k];
    const double signal = 1e-26 * fro;
    bool conv = false;
    for (int sweep = 0; sweep < 40 && !conv; ++sweep) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int q = p + 1; q < 3; ++q) {
                double al = 0.0, be = 0.0, ga = 0.0;
#pragma unroll
                for (int r = 0; r < 3; ++r) { const double x = A[3 * r + p], y = A[3 * r + q]; al += x * x; be += y * y; ga += x * y; }
                if (fabs(ga) > 1e-15 * sqrt(al * be) && ga != 0.0) {
                    rotated = rotated || (al > signal && be > signal);
                    const double zeta = (be - al) / (2.0 * ga);
                    const double tn = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                    const double cs = 1.0 / sqrt(1.0 + tn * tn), sn = cs * tn;
#pragma unroll
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
    // singular values descending, stable: three compare-exchanges of whole columns (no index, so nothing goes to scratch)
    double sv[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int r = 0; r < 3; ++r) { sv[0] += A[3 * r] * A[3 * r]; sv[1] += A[3 * r + 1] * A[3 * r + 1]; sv[2] += A[3 * r + 2] * A[3 * r + 2]; }
#pragma unroll
    for (int st = 0; st < 3; ++st) {
        const int a = st == 1 ? 1 : 0, bq = a + 1;
        const bool sw = sv[bq] > sv[a];
        const double ta = sv[a];
        sv[a] = sw ? sv[bq] : ta; sv[bq] = sw ? ta : sv[bq];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double x = A[3 * r + a], y = A[3 * r + bq], vx = V[3 * r + a], vy = V[3 * r + bq];
            A[3 * r + a] = sw ? y : x; A[3 * r + bq] = sw ? x : y;
            V[3 * r + a] = sw ? vy : vx; V[3 * r + bq] = sw ? vx : vy;
        }
    }
    double u0[3], u1[3], u2[3], v0[3], v1[3], v2[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) { u0[r] = A[3 * r]; u1[r] = A[3 * r + 1]; v0[r] = V[3 * r]; v1[r] = V[3 * r + 1]; v2[r] = V[3 * r + 2]; }
    const double n0 = sqrt(u0[0] * u0[0] + u0[1] * u0[1] + u0[2] * u0[2]), n1 = sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);
#pragma unroll
    for (int r = 0; r < 3; ++r) { u0[r] = u0[r] / n0; u1[r] = u1[r] / n1; }
    u2[0] = u0[1] * u1[2] - u0[2] * u1[1]; u2[1] = u0[2] * u1[0] - u0[0] * u1[2]; u2[2] = u0[0] * u1[1] - u0[1] * u1[0];
    // det Vt = v0 . (v1 x v2)
    const double det = v0[0] * (v1[1] * v2[2] - v1[2] * v2[1]) + v0[1] * (v1[2] * v2[0] - v1[0] * v2[2]) + v0[2] * (v1[0] * v2[1] - v1[1] * v2[0]);
    if (det < 0)
#pragma unroll
        for (int r = 0; r < 3; ++r) { v0[r] = -v0[r]; v1[r] = -v1[r]; v2[r] = -v2[r]; }
    // U W = [-u1 | u0 | u2], U Wt = [u1 | -u0 | u2]; R = (U W) Vt = sum over k of column k times row k of Vt
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            R1[3 * r + c] = -u1[r] * v0[c] + u0[r] * v1[c] + u2[r] * v2[c];
            R2[3 * r + c] = u1[r] * v0[c] - u0[r] * v1[c] + u2[r] * v2[c];
        }
    t[0] = u2[0]; t[1] = u2[1]; t[2] = u2[2];
    return conv;
}

// cv::triangulatePoints for one point and P1 = [R | t] against P0 = [I | 0] (the header's recalled 6x4 form): the right singular vector
// of the smallest singular value by the one-sided Jacobi of tri_dlt.h (same rotation, same threshold and sweep cap), the matrix in
// registers here where tri_dlt.h keeps its 24 rows in an LDS column
DEV void rp_triangulate(const double* R, const double* t, double x0, double y0, double x1, double y1, double* Q) {
    double A[24], V[16];
    A[0] = -1.0; A[1] = 0.0; A[2] = x0; A[3] = 0.0;
    A[4] = 0.0; A[5] = -1.0; A[6] = y0; A[7] = 0.0;
    A[8] = -y0; A[9] = x0; A[10] = 0.0; A[11] = 0.0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const double P0 = c < 3 ? R[c] : t[0], P1 = c < 3 ? R[3 + c] : t[1], P2 = c < 3 ? R[6 + c] : t[2];
        A[12 + c] = x1 * P2 - P0; A[16 + c] = y1 * P2 - P1; A[20 + c] = x1 * P1 - y1 * P0;
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) V[k] = (k % 5 == 0) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 40; ++sweep) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
                for (int r = 0; r < 6; ++r) { const double a = A[r * 4 + p], bb = A[r * 4 + q]; alpha += a * a; beta += bb * bb; gamma += a * bb; }
                if (fabs(gamma) > 1e-16 * sqrt(alpha * beta) && gamma != 0.0) {
                    rotated = true;
                    const double zeta = (beta - alpha) / (2.0 * gamma);
                    const double tn = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                    const double c = 1.0 / sqrt(1.0 + tn * tn), s = c * tn;
#pragma unroll
                    for (int r = 0; r < 6; ++r) {
                        const double a = A[r * 4 + p], bb = A[r * 4 + q];
                        A[r * 4 + p] = c * a - s * bb; A[r * 4 + q] = s * a + c * bb;
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const double a = V[r * 4 + p], bb = V[r * 4 + q];
                        V[r * 4 + p] = c * a - s * bb; V[r * 4 + q] = s * a + c * bb;
                    }
                }
            }
        if (!rotated) break;
    }
    double best = 0.0;
    int bi = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        double s2 = 0.0;
#pragma unroll
        for (int r = 0; r < 6; ++r) s2 += A[r * 4 + c] * A[r * 4 + c];
        if (c == 0 || s2 < best) { best = s2; bi = c; }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) Q[r] = bi == 0 ? V[4 * r] : (bi == 1 ? V[4 * r + 1] : (bi == 2 ? V[4 * r + 2] : V[4 * r + 3]));
}

// One wavefront per stream (DESIGN.md says why not a workgroup): 64 points per pass.
extern "C" __global__ __launch_bounds__(64) void rp_pose_kernel(RpDev b) {
    const int cam = blockIdx.x, lane = threadIdx.x;
    if (cam >= b.NS) return;
    int* ctl = b.ctl + (size_t)cam * RP_CTL_INTS;
    if (ctl[RP_RUN] == 0) return;
    double* res = b.res + (size_t)RP_RES * cam;
    if (ctl[RP_BEST] < 0) {                                // no model: the candidate fails, its taps stay zero
        if (lane < RP_RES - 9) res[9 + lane] = 0.0;
        if (lane == 0) { ctl[RP_NUMERIC] = 0; ctl[RP_WINNER] = 0; ctl[RP_CNT] = 0; ctl[RP_GOOD] = ctl[RP_GOOD + 1] = ctl[RP_GOOD + 2] = ctl[RP_GOOD + 3] = 0; }
        for (int w = lane; w < b.words_n; w += 64) b.mask[(size_t)cam * b.words_n + w] = 0ull;
        return;
    }
    const int n = ctl[RP_N], nw = (n + 63) >> 6;
    const double dist = b.par[(size_t)RP_PAR * b.swin[2 * cam] + 5];
    const float* __restrict__ p1 = b.p1 + (size_t)cam * b.cap * 2;
    const float* __restrict__ p2 = b.p2 + (size_t)cam * b.cap * 2;
    unsigned long long* mask = b.mask + (size_t)cam * b.words_n;
    const unsigned long long* rmask = b.rmask + (size_t)cam * b.words_n;
    unsigned long long* mask4 = b.mask4 + (size_t)cam * 4 * b.words_n;
    double E[9], R1[9], R2[9], t[3], tm[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) E[k] = res[k];
    const bool conv = rp_decompose(E, R1, R2, t);
    tm[0] = -t[0]; tm[1] = -t[1]; tm[2] = -t[2];
    int good[4] = {0, 0, 0, 0};
    for (int w = 0; w < nw; ++w) {
        const int i = 64 * w + lane;
        const bool valid = i < n;
        const double x0 = valid ? (double)p1[2 * i] : 0.0, y0 = valid ? (double)p1[2 * i + 1] : 0.0;
        const double x1 = valid ? (double)p2[2 * i] : 0.0, y1 = valid ? (double)p2[2 * i + 1] : 0.0;
        const bool rin = valid && ((rmask[w] >> lane) & 1ull) != 0ull;
#pragma unroll
        for (int cand = 0; cand < 4; ++cand) {
            const double* R = (cand & 1) ? R2 : R1;
            const double* tt = cand >= 2 ? tm : t;
            double Q[4];
            rp_triangulate(R, tt, x0, y0, x1, y1, Q);
            bool m = Q[2] * Q[3] > 0;
            const double X = Q[0] / Q[3], Y = Q[1] / Q[3], Z = Q[2] / Q[3], Wq = Q[3] / Q[3];
            m = (Z < dist) && m;
            const double z1 = R[6] * X + R[7] * Y + R[8] * Z + tt[2] * Wq;
            m = (z1 > 0) && m;
            m = (z1 < dist) && m;
            const unsigned long long bal = __ballot(m && rin);
            good[cand] += __popcll(bal);
            if (lane == 0) mask4[(size_t)cand * b.words_n + w] = bal;
        }
    }
    int win = 3;
    if (good[0] >= good[1] && good[0] >= good[2] && good[0] >= good[3]) win = 0;
    else if (good[1] >= good[0] && good[1] >= good[2] && good[1] >= good[3]) win = 1;
    else if (good[2] >= good[0] && good[2] >= good[1] && good[2] >= good[3]) win = 2;
    double R[9], tt[3];                                    // (selected by value: a pointer chosen at run time would put R1 / R2 into scratch)
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = (win & 1) ? R2[k] : R1[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) tt[k] = win >= 2 ? tm[k] : t[k];
    if (lane == 0) {
        // Rotation = R^T, Translation = -(R^T t)
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) res[9 + 3 * r + c] = R[3 * c + r];
            res[18 + r] = -(R[r] * tt[0] + R[3 + r] * tt[1] + R[6 + r] * tt[2]);
        }
        const int cnt = win == 0 ? good[0] : (win == 1 ? good[1] : (win == 2 ? good[2] : good[3]));
        ctl[RP_NUMERIC] = conv ? 0 : 1; ctl[RP_WINNER] = win; ctl[RP_CNT] = cnt;
        ctl[RP_GOOD] = good[0]; ctl[RP_GOOD + 1] = good[1]; ctl[RP_GOOD + 2] = good[2]; ctl[RP_GOOD + 3] = good[3];
        // (the words lane 0 itself stored above)
        for (int w = 0; w < nw; ++w) mask[w] = mask4[(size_t)win * b.words_n + w];
    }
}

extern "C" __global__ __launch_bounds__(64) void rp_window_kernel(RpDev b) {
    const int w = blockIdx.x * 64 + threadIdx.x;
    if (w >= b.W) return;
    const int* q = b.wi + RP_WI * w;
    const int min_in = (int)b.par[(size_t)RP_PAR * w + 4];
    int l = -1, status = VG_RELPOSE_NONE;
    for (int i = 0; i < q[0] - 1; ++i) {
        const int* ctl = b.ctl + (size_t)(q[4] + i) * RP_CTL_INTS;
        if (ctl[RP_GATE] == 0) continue;
        if (ctl[RP_NUMERIC] != 0) { status = VG_RELPOSE_NUMERIC; break; }
        if (ctl[RP_BEST] >= 0 && ctl[RP_CNT] > min_in) { l = i; status = VG_RELPOSE_OK; break; }
    }
    b.wout[2 * w] = l; b.wout[2 * w + 1] = status;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
namespace {
inline size_t rp_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
bool rp_finite(const double* p, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(p[i])) return false;
    return true;
}
// ---- what vg_init_relpose and vg_init_exrot (init_exrot.h) share on the host: one text for the tables, the scratch, the six RANSAC
// launches and the exact schedules, so that the two entries cannot drift apart
// the resident tables: built once per handle up to the largest point count seen, rebuilt larger when a call exceeds it
hipError_t rp_resident_tables(vg_handle* h, int nmax) {
    if (nmax <= h->relpose_nmax) return hipSuccess;
    hipError_t e;
    std::vector<int> sched, tab;
    const int stride = nmax + 1;
    fe_ransac_tables(nmax, sched, tab, stride);
    if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return e;
    (void)hipFree(h->relpose_tab);
    h->relpose_tab = nullptr; h->relpose_nmax = 0;
    if ((e = hipMalloc(&h->relpose_tab, sizeof(int) * (sched.size() + tab.size()))) != hipSuccess) return e;
    if ((e = hipMemcpy(h->relpose_tab, sched.data(), sizeof(int) * sched.size(), hipMemcpyHostToDevice)) != hipSuccess) return e;
    if ((e = hipMemcpy((int*)h->relpose_tab + sched.size(), tab.data(), sizeof(int) * tab.size(), hipMemcpyHostToDevice)) != hipSuccess) return e;
    h->relpose_nmax = nmax;
    return hipSuccess;
}
// the scratch block, grown on demand
hipError_t rp_scratch(vg_handle* h, size_t need) {
    if (need <= h->relpose_cap) return hipSuccess;
    hipError_t e;
    if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return e;
    (void)hipFree(h->relpose_buf);
    h->relpose_buf = nullptr; h->relpose_cap = 0;
    if ((e = hipMalloc(&h->relpose_buf, need)) != hipSuccess) return e;
    h->relpose_cap = need;
    return hipSuccess;
}
// the schedule and bound pointers of a control block from the resident tables
void rp_table_pointers(const vg_handle* h, RpDev& b) {
    const int tmax = h->relpose_nmax;
    b.tab_stride = tmax + 1;
    b.sched = (const int*)h->relpose_tab; b.niters_tab = b.sched + (size_t)(tmax - 14) * FE_RANSAC_MAXIT * 7;
}
// the RANSAC stage of the streams whose RP_RUN is set: the chunked two-part scheme, six launches; stamp() after each
template <class Stamp>
hipError_t rp_ransac_launches(vg_handle* h, const RpDev& b, size_t NS, Stamp&& stamp) {
    hipError_t r;
    hipLaunchKernelGGL(rp_ransac7_kernel, dim3(RP_CHUNK0 / FR_PER_WAVE, (unsigned)NS), dim3(64), 0, h->stream, b, 0, RP_CHUNK0);
    if ((r = stamp()) != hipSuccess) return r;
    hipLaunchKernelGGL(rp_count_kernel, dim3(RP_CHUNK0, (unsigned)NS), dim3(64), 0, h->stream, b, 0, RP_CHUNK0);
    if ((r = stamp()) != hipSuccess) return r;
    hipLaunchKernelGGL(rp_pick_kernel, dim3((unsigned)NS), dim3(64), 0, h->stream, b, 0, RP_CHUNK0, 0);
    if ((r = stamp()) != hipSuccess) return r;
    hipLaunchKernelGGL(rp_ransac7_kernel, dim3(RP_P2_WAVES, (unsigned)NS), dim3(64), 0, h->stream, b, RP_CHUNK0, FE_RANSAC_MAXIT);
    if ((r = stamp()) != hipSuccess) return r;
    hipLaunchKernelGGL(rp_count_kernel, dim3(RP_P2_COUNT, (unsigned)NS), dim3(64), 0, h->stream, b, RP_CHUNK0, FE_RANSAC_MAXIT);
    if ((r = stamp()) != hipSuccess) return r;
    hipLaunchKernelGGL(rp_pick_kernel, dim3((unsigned)NS), dim3(64), 0, h->stream, b, RP_CHUNK0, FE_RANSAC_MAXIT, 1);
    return stamp();
}
// The second submission's control blocks and exact schedules: only the streams of `again` run; points(s, pts) fills the stream's float32
// point sets (the two sets 2 * cap apart) and returns their count.  xs gets one schedule per stream of `again`.
template <class Points>
void rp_exact_schedules(const std::vector<int>& again, int* ctl, size_t NS, int cap, std::vector<int>& xs, Points&& points) {
    xs.assign(again.size() * FE_RANSAC_MAXIT * 7, 0);
    std::vector<float> pts((size_t)cap * 4);
    for (size_t s = 0; s < NS; ++s) ctl[s * RP_CTL_INTS + RP_RUN] = 0;
    for (size_t k = 0; k < again.size(); ++k) {
        const size_t s = again[k];
        int* c = ctl + s * RP_CTL_INTS;
        const int n = points(s, pts.data());
        CvRng rng((unsigned long long)-1);
        int nsched = 0;
        for (; nsched < FE_RANSAC_MAXIT; ++nsched)
            if (!get_subset(rng, pts.data(), pts.data() + 2 * cap, n, xs.data() + (k * FE_RANSAC_MAXIT + nsched) * 7, 10000)) break;
        c[RP_RUN] = 1; c[RP_XS] = (int)k; c[RP_MAXIT] = nsched; c[RP_BEST] = -1; c[RP_NITERS] = 0; c[RP_MAXGOOD] = 0;
    }
}
#define RP_XS_CAP 64                // exact schedules the scratch block has room for; more: a block of their own
}  // namespace

extern "C" int vg_init_relpose(vg_handle* h, int n_windows, const vg_relpose_in* in, vg_relpose_out* out) {
    VG_RANGE("vg_init_relpose");
    if (!h) return VG_ERR_BAD_ARG;
    auto bad = [&](int w, const char* what) {
        h->err = "vg_init_relpose: window " + std::to_string(w) + ": " + what;
        return VG_ERR_BAD_ARG;
    };
    if (n_windows <= 0 || !in || !out) { h->err = "vg_init_relpose: n_windows <= 0 or a NULL argument"; return VG_ERR_BAD_ARG; }
    // ---- everything that follows from the arguments alone, before anything is uploaded or written
    size_t nFeat = 0, nObs = 0, NS = 0;
    int nmax = 15;
    for (int w = 0; w < n_windows; ++w) {
        const vg_relpose_in& a = in[w];
        if (a.struct_size != sizeof(vg_relpose_in)) return bad(w, "vg_relpose_in::struct_size");
        if (out[w].struct_size != sizeof(vg_relpose_out)) return bad(w, "vg_relpose_out::struct_size");
        const int F = a.n_frames, n = a.n_feat;
        if (F < 3 || F > VG_SFM_MAX_FRAMES) return bad(w, "n_frames outside 3 .. VG_SFM_MAX_FRAMES");
        if (n < 1 || n > VG_SFM_MAX_FEATURES) return bad(w, "n_feat outside 1 .. VG_SFM_MAX_FEATURES");
        if (!a.start || !a.nobs || !a.obs_off || !a.points) return bad(w, "a NULL table");
        if (!(a.ransac_threshold > 0) || !std::isfinite(a.ransac_threshold)) return bad(w, "ransac_threshold is not positive");
        if (a.confidence != 0.99) return bad(w, "a confidence other than 0.99");
        if (!(a.parallax_gate > 0) || !(a.focal > 0) || !(a.cheirality_dist > 0) || !std::isfinite(a.parallax_gate) || !std::isfinite(a.focal) ||
            !std::isfinite(a.cheirality_dist))
            return bad(w, "parallax_gate, focal or cheirality_dist is not positive");
        if (a.min_corres < 14 || a.min_inliers < 0) return bad(w, "min_corres < 14 or min_inliers < 0");
        if (a.obs_off[0] < 0) return bad(w, "obs_off[0] < 0");
        size_t no = 0;
        for (int j = 0; j < n; ++j) {
            if (a.nobs[j] < 1 || a.start[j] < 0 || a.start[j] + a.nobs[j] > F) return bad(w, "start + nobs > n_frames or nobs < 1");
            if (j > 0 && a.obs_off[j] < a.obs_off[j - 1] + a.nobs[j - 1]) return bad(w, "obs_off does not ascend");
            if (!rp_finite(a.points + 3 * (size_t)a.obs_off[j], 3 * (size_t)a.nobs[j])) return bad(w, "a non-finite input");
            no += a.nobs[j];
        }
        nFeat += n; nObs += no; NS += F - 1;
        nmax = std::max(nmax, n);
    }
    if (NS > VG_RELPOSE_MAX_STREAMS) { h->err = "vg_init_relpose: more than VG_RELPOSE_MAX_STREAMS candidates in one call"; return VG_ERR_BAD_ARG; }
    if (nObs > (size_t)0x3fffffff) { h->err = "vg_init_relpose: too many observations for one call"; return VG_ERR_BAD_ARG; }
    const int W = n_windows, cap = (int)rp_up(nmax, 64), words_n = cap / 64;
    // ---- the host image of the upload: ints [wi | swin | start | nobs | off], doubles [par | obs]
    const size_t i_wi = 0, i_sw = i_wi + (size_t)RP_WI * W, i_st = i_sw + 2 * NS, i_nb = i_st + nFeat, i_of = i_nb + nFeat, n_int = rp_up(i_of + nFeat, 2);
    const size_t o_par = 0, o_obs = o_par + (size_t)RP_PAR * W, n_in = o_obs + 2 * nObs;
    // the download, in 8-byte units: ctl (ints) | wout (ints) | avg | res | rmask | mask
    const size_t d_ctl = 0, d_wo = d_ctl + NS * RP_CTL_INTS / 2, d_avg = d_wo + W, d_res = d_avg + NS, d_rm = d_res + (size_t)RP_RES * NS,
                 d_mask = d_rm + NS * words_n, n_out = d_mask + NS * words_n;
    std::vector<int> hint(n_int, 0);
    std::vector<double> hin(n_in, 0.0), hout(n_out);
    {
        size_t ft = 0, ob = 0, s = 0;
        for (int w = 0; w < W; ++w) {
            const vg_relpose_in& a = in[w];
            const int F = a.n_frames, n = a.n_feat;
            int* wi = hint.data() + i_wi + (size_t)RP_WI * w;
            wi[0] = F; wi[1] = n; wi[2] = (int)ft; wi[3] = (int)ob; wi[4] = (int)s;
            double* p = hin.data() + o_par + (size_t)RP_PAR * w;
            p[0] = (double)(float)(a.ransac_threshold * a.ransac_threshold);
            p[1] = a.min_corres; p[2] = a.parallax_gate; p[3] = a.focal; p[4] = a.min_inliers; p[5] = a.cheirality_dist;
            for (int i = 0; i < F - 1; ++i) { hint[i_sw + 2 * (s + i)] = w; hint[i_sw + 2 * (s + i) + 1] = i; }
            int no = 0;
            for (int j = 0; j < n; ++j) {
                hint[i_st + ft + j] = a.start[j]; hint[i_nb + ft + j] = a.nobs[j]; hint[i_of + ft + j] = no;
                for (int k = 0; k < a.nobs[j]; ++k) {
                    const double* r = a.points + 3 * ((size_t)a.obs_off[j] + k);
                    hin[o_obs + 2 * (ob + no + k)] = r[0]; hin[o_obs + 2 * (ob + no + k) + 1] = r[1];
                }
                no += a.nobs[j];
            }
            ft += n; ob += no; s += F - 1;
        }
    }
    hipError_t e = hipSetDevice(h->device);
    auto fail = [&](hipError_t err) { h->err = std::string("vg_init_relpose: ") + hipGetErrorString(err); return VG_ERR_HIP; };
    if (e != hipSuccess) return fail(e);
    // ---- the resident tables: built once per handle up to the largest n_feat seen, rebuilt larger when a call exceeds it
    if ((e = rp_resident_tables(h, nmax)) != hipSuccess) return fail(e);
    // ---- device block: [out | in doubles | ints | scratch]
    const size_t b_out = 0, b_in = b_out + n_out * 8, b_int = b_in + n_in * 8, b_p1 = rp_up(b_int + n_int * 4, 256), b_p2 = b_p1 + NS * cap * 2 * sizeof(float);
    const size_t b_md = rp_up(b_p2 + NS * cap * 2 * sizeof(float), 256), b_F = b_md + NS * FE_RANSAC_MAXIT * 27 * 8, b_me = b_F + NS * FE_RANSAC_MAXIT * 9 * 8;
    const size_t b_wd = b_me + NS * FE_RANSAC_MAXIT * 8, b_m4 = b_wd + NS * FE_RANSAC_MAXIT * (size_t)words_n * 8, b_ct = b_m4 + NS * 4 * (size_t)words_n * 8;
    const size_t b_xs = rp_up(b_ct + NS * FE_RANSAC_MAXIT * 4, 256);
    const size_t xs_cap = RP_XS_CAP;
    if ((e = rp_scratch(h, b_xs + xs_cap * FE_RANSAC_MAXIT * 7 * 4)) != hipSuccess) return fail(e);
    char* base = (char*)h->relpose_buf;
    double* d_out = (double*)(base + b_out);
    double* d_in = (double*)(base + b_in);
    int* d_int = (int*)(base + b_int);
    RpDev b;
    b.NS = (int)NS; b.W = W; b.cap = cap; b.words_n = words_n;
    rp_table_pointers(h, b);
    b.wi = d_int + i_wi; b.swin = d_int + i_sw; b.start = d_int + i_st; b.nobs = d_int + i_nb; b.off = d_int + i_of;
    b.par = d_in + o_par; b.obs = d_in + o_obs;
    b.ctl = (int*)(d_out + d_ctl); b.wout = (int*)(d_out + d_wo); b.avg = d_out + d_avg; b.res = d_out + d_res;
    b.rmask = (unsigned long long*)(d_out + d_rm); b.mask = (unsigned long long*)(d_out + d_mask);
    b.p1 = (float*)(base + b_p1); b.p2 = (float*)(base + b_p2);
    b.xsched = (const int*)(base + b_xs);
    b.models = (double*)(base + b_md); b.Fit = (double*)(base + b_F); b.med = (double*)(base + b_me);
    b.words = (unsigned long long*)(base + b_wd); b.mask4 = (unsigned long long*)(base + b_m4); b.count = (int*)(base + b_ct);
    if ((e = hipMemcpyAsync(d_in, hin.data(), n_in * 8, hipMemcpyHostToDevice, h->stream)) != hipSuccess) return fail(e);
    if ((e = hipMemcpyAsync(d_int, hint.data(), n_int * 4, hipMemcpyHostToDevice, h->stream)) != hipSuccess) return fail(e);
    if ((e = hipMemsetAsync(d_out, 0, n_out * 8, h->stream)) != hipSuccess) return fail(e);
    struct Events {                                         // destroyed on every way out
        hipEvent_t ev[VG_RELPOSE_LAUNCHES + 1] = {};
        ~Events() { for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x); }
    } evs;
    const bool timed = out[0].device_ms != nullptr;
    if (timed)
        for (int i = 0; i <= VG_RELPOSE_LAUNCHES; ++i)
            if ((e = hipEventCreate(&evs.ev[i])) != hipSuccess) return fail(e);
    int mark = 0;
    auto stamp = [&](bool on) { return on ? hipEventRecord(evs.ev[mark++], h->stream) : hipSuccess; };
    // the RANSAC and pose stages of the streams whose RP_RUN is set, then the pick over every window
    auto stages = [&](bool on) -> hipError_t {
        hipError_t r;
        if ((r = rp_ransac_launches(h, b, NS, [&] { return stamp(on); })) != hipSuccess) return r;
        hipLaunchKernelGGL(rp_pose_kernel, dim3((unsigned)NS), dim3(64), 0, h->stream, b);
        if ((r = stamp(on)) != hipSuccess) return r;
        hipLaunchKernelGGL(rp_window_kernel, dim3((unsigned)(W + 63) / 64), dim3(64), 0, h->stream, b);
        if ((r = stamp(on)) != hipSuccess) return r;
        return hipGetLastError();
    };
    if ((e = stamp(timed)) != hipSuccess) return fail(e);
    hipLaunchKernelGGL(rp_gather_kernel, dim3((unsigned)NS), dim3(RP_NT), 0, h->stream, b);
    if ((e = stamp(timed)) != hipSuccess) return fail(e);
    if ((e = stages(timed)) != hipSuccess) return fail(e);
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
        // the stream's float32 point sets, gathered here from the caller's tables as rp_gather_kernel gathers them (no copy back)
        std::vector<int> xs;
        rp_exact_schedules(again, ctl, NS, cap, xs, [&](size_t s, float* pts) {
            const int w = hint[i_sw + 2 * s], i = hint[i_sw + 2 * s + 1], n = ctl[s * RP_CTL_INTS + RP_N];
            const vg_relpose_in& a = in[w];
            int k = 0;
            for (int j = 0; j < a.n_feat && k < n; ++j) {
                const int s0 = a.start[j];
                if (!(s0 <= i && s0 + a.nobs[j] - 1 >= a.n_frames - 1)) continue;
                const double* r = a.points + 3 * (size_t)a.obs_off[j];
                pts[2 * k] = (float)r[3 * (i - s0)]; pts[2 * k + 1] = (float)r[3 * (i - s0) + 1];
                pts[2 * cap + 2 * k] = (float)r[3 * (a.n_frames - 1 - s0)]; pts[2 * cap + 2 * k + 1] = (float)r[3 * (a.n_frames - 1 - s0) + 1];
                ++k;
            }
            return n;
        });
        if (again.size() > xs_cap) {
            if ((e = hipMalloc(&xs_own, xs.size() * 4)) != hipSuccess) return fail(e);
            b.xsched = (const int*)xs_own;
        }
        if ((e = hipMemcpyAsync((void*)b.xsched, xs.data(), xs.size() * 4, hipMemcpyHostToDevice, h->stream)) != hipSuccess) return fail(e);
        if ((e = hipMemcpyAsync(b.ctl, ctl, NS * RP_CTL_INTS * 4, hipMemcpyHostToDevice, h->stream)) != hipSuccess) return fail(e);
        if ((e = stages(false)) != hipSuccess) return fail(e);
        if ((e = hipMemcpyAsync(hout.data(), d_out, n_out * 8, hipMemcpyDeviceToHost, h->stream)) != hipSuccess) return fail(e);
        if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return fail(e);
    }
    if (timed)
        for (int i = 0; i < VG_RELPOSE_LAUNCHES; ++i) {
            float ms = 0.f;
            if ((e = hipEventElapsedTime(&ms, evs.ev[i], evs.ev[i + 1])) != hipSuccess) return fail(e);
            out[0].device_ms[i] = ms;
        }
    const int* wout = (const int*)(hout.data() + d_wo);
    const unsigned long long* mask = (const unsigned long long*)(hout.data() + d_mask);
    const unsigned long long* rmask = (const unsigned long long*)(hout.data() + d_rm);
    size_t s0 = 0;
    for (int w = 0; w < W; ++w) {
        const int F = in[w].n_frames;
        vg_relpose_out& o = out[w];
        o.l = wout[2 * w]; o.status = wout[2 * w + 1];
        for (int k = 0; k < 9; ++k) o.relative_R[k] = 0.0;
        for (int k = 0; k < 3; ++k) o.relative_T[k] = 0.0;
        o.n_mask = 0;
        if (o.mask) std::fill(o.mask, o.mask + in[w].n_feat, (unsigned char)0);
        if (o.ransac_mask) std::fill(o.ransac_mask, o.ransac_mask + in[w].n_feat, (unsigned char)0);
        for (int i = 0; i < F - 1; ++i) {
            const int* c = ctl + (s0 + i) * RP_CTL_INTS;
            const double* r = hout.data() + d_res + (size_t)RP_RES * (s0 + i);
            const bool g = c[RP_GATE] != 0;
            if (o.n_corres) o.n_corres[i] = c[RP_N];
            if (o.avg_parallax) o.avg_parallax[i] = hout[d_avg + s0 + i];
            if (o.gate) o.gate[i] = c[RP_GATE];
            // the last iteration the loop looked at: the bound can drop below the iteration that lowered it; an exact schedule can run out
            const int reach = (c[RP_NITERS] < c[RP_MAXIT] ? c[RP_NITERS] : c[RP_MAXIT]) - 1;
            if (o.ransac_iter) o.ransac_iter[i] = g ? (c[RP_BEST] > reach ? c[RP_BEST] : reach) : 0;
            if (o.ransac_best) o.ransac_best[i] = g ? c[RP_BEST] : 0;
            if (o.ransac_bound) o.ransac_bound[i] = g ? c[RP_NITERS] : 0;
            if (o.ransac_inliers) o.ransac_inliers[i] = g ? c[RP_NIN] : 0;
            if (o.F) for (int k = 0; k < 9; ++k) o.F[9 * i + k] = g ? r[k] : 0.0;
            if (o.good) for (int k = 0; k < 4; ++k) o.good[4 * i + k] = g ? c[RP_GOOD + k] : 0;
            if (o.winner) o.winner[i] = g ? c[RP_WINNER] : 0;
            if (o.inlier_cnt) o.inlier_cnt[i] = g ? c[RP_CNT] : 0;
            if (o.used_fallback) o.used_fallback[i] = (g && c[RP_XS] >= 0) ? 1 : 0;
            if (i == o.l) {
                std::copy(r + 9, r + 18, o.relative_R);
                std::copy(r + 18, r + 21, o.relative_T);
                o.n_mask = c[RP_N];
                if (o.mask)
                    for (int k = 0; k < c[RP_N]; ++k) o.mask[k] = (unsigned char)((mask[(s0 + i) * words_n + (k >> 6)] >> (k & 63)) & 1ull);
                if (o.ransac_mask)
                    for (int k = 0; k < c[RP_N]; ++k) o.ransac_mask[k] = (unsigned char)((rmask[(s0 + i) * words_n + (k >> 6)] >> (k & 63)) & 1ull);
            }
        }
        s0 += F - 1;
    }
    return VG_OK;
}
