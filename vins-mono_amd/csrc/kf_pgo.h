// kf_pgo.h — vg_pg_optimize: one pass of the body of PoseGraph::optimize4DoF (pose_graph/src/pose_graph.cpp:403-579) for a batch of pose
// graphs.  include/vinsgpu.h defines the call statement by statement (the graph and the functors READ from the reference, Ceres RECALLED,
// NOT PINNED; the [FIXED] and [DEVIATION] parts are marked there); this file is its device code and its host entry.  Included behind
// kf_bow.h at the END of fe_ransac.hip: it uses init_relpose.h's scratch block and is compiled with -ffp-contract=off like the rest of the
// unit.
//
// One launch, one workgroup of PG_NT threads per graph, every iteration inside it; no workgroup waits for another, there are no atomics,
// and every loop is bounded by a constant or by an input count.  Everything a graph needs lies in its own carve of global scratch.
//   all wavefronts   the edge measurements, residuals and Jacobians (a thread per edge slot), the per-node gathers of the blocks and the
//                    gradient (a thread per free node, the terms in the header's order), q = A p (a thread per row), the sums (pg_sum:
//                    strided partial sums, then a fold by halves)
//   wavefront 0      the banded Cholesky (a 20 x 20 window of the band in LDS slides down the diagonal: per column the pivot, the scaled
//                    column, the rank-1 update of the window by 190 entry pairs over the lanes; the next row's operands are read from
//                    global memory while the column is factored) and the two triangular sweeps (lane = row mod 32 keeps the row's running
//                    right-hand side in a register, the solved entry goes round by readlane, the operands of the next step are read
//                    while this step's chain runs; wavefronts 1 .. 3 stage the next 128 rows of the factor into LDS meanwhile)
// This is latency-bound by design: a graph keeps one CU busy and the sweeps are a chain of 4 n_free dependent steps; throughput comes
// from the batch.
#pragma once
#include <cfloat>
#include "kf_pnp.h"

#define PG_NT 256
#define PG_KD 19                    // scalar half-bandwidth of M: 4 blocks of 4 and the block's own triangle
#define PG_BW (PG_KD + 1)           // entries a band row keeps: [0] 1 / L(i, i), [o] L(i, i - o)
#define PG_PAIRS (PG_KD * PG_BW / 2)// entries (i, k), j < k <= i <= j + 19, a column updates
#define PG_CH 128                   // rows of the factor a sweep keeps in LDS per chunk
#define PG_CHR (PG_CH + PG_KD)
#define PG_RH 32                    // a sweep's look-ahead in the right-hand side: the row a lane takes when its row is solved
enum { PG_N = 0, PG_NKF, PG_NF, PG_MAXIT, PG_NLP, PG_GI = 8 };            // ints per graph
enum { PG_O_INT = 0, PG_O_IN, PG_O_SCR, PG_O_OUT, PG_GO = 4 };            // offsets per graph (ints, doubles, doubles, doubles)
#define PG_OUT_HDR 48               // doubles: initial | final | yaw_drift | r_drift 9 | t_drift 3 | - | trace [8][4]: cost radius candidate model
#define PG_OUT_INT 24               // ints behind them: status | termination | iterations | - | flags 8 | cg 8 | - 4
#define PG_SCR_N 435                // scratch doubles per optimised keyframe (pg_carve)

struct PgDev {
    int G;
    const int* gi;                  // [G][PG_GI]
    const long long* go;            // [G][PG_GO]
    const double* delta;            // [G] huber_delta
    const int* ints;                // per graph: fidx [N] | nof [N] | ea [5 N] | lp_off [N + 1] | lp_src [N]
    const double* in;               // per graph: vio_T [NKF][3] | vio_R [NKF][9] | loop measurement [N][4]
    double* scratch;
    double* out;                    // per graph: PG_OUT_HDR | PG_OUT_INT ints | T [NKF][3] | R [NKF][9]
};

// the carve of a graph's scratch (doubles), N optimised keyframes
struct PgCarve {
    double *yaw, *pr, *t, *cyaw, *ct, *meas, *res, *Ja, *Jb, *ev, *Ab, *LB, *g, *gs, *scale, *dcl, *dd, *Lb, *x, *r, *z, *p, *q, *w;
};
DEV PgCarve pg_carve(double* s, const int N) {
    PgCarve c;
    c.yaw = s; s += N; c.pr = s; s += 2 * N; c.t = s; s += 3 * N; c.cyaw = s; s += N; c.ct = s; s += 3 * N;
    c.meas = s; s += 20 * N; c.res = s; s += 20 * N; c.Ja = s; s += 80 * N; c.Jb = s; s += 80 * N; c.ev = s; s += 5 * N;
    c.Ab = s; s += 80 * N; c.LB = s; s += 16 * N; c.g = s; s += 4 * N; c.gs = s; s += 4 * N; c.scale = s; s += 4 * N; c.dcl = s; s += 4 * N;
    c.dd = s; s += 4 * N; c.Lb = s; s += 80 * N; c.x = s; s += 4 * N; c.r = s; s += 4 * N; c.z = s; s += 4 * N; c.p = s; s += 4 * N;
    c.q = s; s += 4 * N; c.w = s; s += 4 * N;                  // 435 N
    return c;
}

DEV double pg_normalize(const double a) { return a > 180.0 ? a - 360.0 : (a < -180.0 ? a + 360.0 : a); }

// Utility::R2ypr (utility.h:70-85), degrees
DEV void pg_R2ypr(const double* R, double* ypr) {
    const double y = atan2(R[3], R[0]);
    const double p = atan2(-R[6], R[0] * cos(y) + R[3] * sin(y));
    const double r = atan2(R[2] * sin(y) - R[5] * cos(y), -R[1] * sin(y) + R[4] * cos(y));
    ypr[0] = y / M_PI * 180.0; ypr[1] = p / M_PI * 180.0; ypr[2] = r / M_PI * 180.0;
}
// Utility::ypr2R (utility.h:88-112): (Rz Ry) Rx
DEV void pg_ypr2R(const double yaw, const double pitch, const double roll, double* R) {
    const double y = yaw / 180.0 * M_PI, p = pitch / 180.0 * M_PI, r = roll / 180.0 * M_PI;
    const double Rz[9] = {cos(y), -sin(y), 0.0, sin(y), cos(y), 0.0, 0.0, 0.0, 1.0};
    const double Ry[9] = {cos(p), 0.0, sin(p), 0.0, 1.0, 0.0, -sin(p), 0.0, cos(p)};
    const double Rx[9] = {1.0, 0.0, 0.0, 0.0, cos(r), -sin(r), 0.0, sin(r), cos(r)};
    double zy[9];
    m3_mul(Rz, Ry, zy);
    m3_mul(zy, Rx, R);
}

// FourDOFError / FourDOFWeightError with the loss corrector for the edge a -> b; returns rho.  With JAC the corrected residual res[4] and
// the corrected Jacobians Ja, Jb [4][4] (rows: residuals, columns: yaw t) are stored; without, nothing is
template <bool JAC>
DEV double pg_edge(const double ya, const double pa, const double ra, const double* ta, const double yb, const double* tb, const double* m,
                   const bool loop, const double delta, double* res, double* Ja, double* Jb) {
    const double y = ya / 180.0 * M_PI, p = pa / 180.0 * M_PI, r = ra / 180.0 * M_PI;
    const double cy = cos(y), sy = sin(y), cp = cos(p), sp = sin(p), cr = cos(r), sr = sin(r);
    const double R[9] = {cy * cp, -sy * cr + cy * sp * sr, sy * sr + cy * sp * cr, sy * cp, cy * cr + sy * sp * sr, -cy * sr + sy * sp * cr, -sp, cp * sr, cp * cr};
    const double d0 = tb[0] - ta[0], d1 = tb[1] - ta[1], d2 = tb[2] - ta[2];
    double e[4];
#pragma unroll
    for (int c = 0; c < 3; ++c) e[c] = (R[c] * d0 + R[3 + c] * d1 + R[6 + c] * d2) - m[c];
    const double ang = pg_normalize(yb - ya - m[3]);
    e[3] = loop ? ang / 10.0 : ang;
    const double s = e[0] * e[0] + e[1] * e[1] + e[2] * e[2] + e[3] * e[3];
    double rho = s, sc = 1.0;
    if (loop && s > delta * delta) {
        const double rt = sqrt(s);
        rho = 2.0 * delta * rt - delta * delta;
        sc = sqrt(fmax(DBL_MIN, delta / rt));
    }
    if (JAC) {
        // (a candidate's evaluation, !JAC, stores nothing: after a rejected step the residuals of the current point are still needed)
#pragma unroll
        for (int c = 0; c < 4; ++c) res[c] = sc * e[c];
        const double w = loop ? 1.0 / 10.0 : 1.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double dy = (R[c] * d1 - R[3 + c] * d0) * (M_PI / 180.0);
            Ja[4 * c] = sc * dy; Ja[4 * c + 1] = sc * -R[c]; Ja[4 * c + 2] = sc * -R[3 + c]; Ja[4 * c + 3] = sc * -R[6 + c];
            Jb[4 * c] = 0.0; Jb[4 * c + 1] = sc * R[c]; Jb[4 * c + 2] = sc * R[3 + c]; Jb[4 * c + 3] = sc * R[6 + c];
        }
        Ja[12] = sc * -w; Ja[13] = 0.0; Ja[14] = 0.0; Ja[15] = 0.0;
        Jb[12] = sc * w; Jb[13] = 0.0; Jb[14] = 0.0; Jb[15] = 0.0;
    }
    return rho;
}

// the header's SUM OVER A LIST of f(0) .. f(n - 1); every thread of the workgroup calls it and gets the sum
template <typename F>
DEV double pg_sum(double* red, const int n, const int tid, F f) {
    double s = 0.0;
    for (int k = tid; k < n; k += PG_NT) s += f(k);
    red[tid] = s;
    __syncthreads();
#pragma unroll 1
    for (int h = PG_NT / 2; h > 0; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}
template <typename F>
DEV double pg_max(double* red, const int n, const int tid, F f) {
    double s = 0.0;
    for (int k = tid; k < n; k += PG_NT) s = fmax(s, f(k));
    red[tid] = s;
    __syncthreads();
#pragma unroll 1
    for (int h = PG_NT / 2; h > 0; h >>= 1) {
        if (tid < h) red[tid] = fmax(red[tid], red[tid + h]);
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// C [4][4] += A^T B over the residual index (the product first, then the addition)
DEV void pg_add_AtB(double* C, const double* A, const double* B) {
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            double t = A[p] * B[q];
            t += A[4 + p] * B[4 + q]; t += A[8 + p] * B[8 + q]; t += A[12 + p] * B[12 + q];
            C[4 * p + q] += t;
        }
}
DEV void pg_add_Atr(double* g, const double* A, const double* r) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        double t = A[p] * r[0];
        t += A[4 + p] * r[1]; t += A[8 + p] * r[2]; t += A[12 + p] * r[3];
        g[p] += t;
    }
}

// what the kernel keeps in LDS
struct PgLds {
    double red[PG_NT];
    double W[PG_BW * PG_BW];            // the window of the factorisation: entry (i, k) at [i % 20][k % 20]
    double Lc[2][PG_CHR * PG_BW];       // a sweep's rows of the factor, two chunks
    double Rc[2][PG_CH + PG_RH];        // and of its right-hand side
    unsigned char pi[PG_PAIRS], pk[PG_PAIRS];
    int flag;
};

// residuals (and with JAC Jacobians) of every edge slot at (yaw, t) -> ev[slot] = rho; returns the cost
template <bool JAC>
DEV double pg_evaluate(PgLds& S, const PgCarve& c, const int* ea, const int N, const double delta, const double* yaw, const double* t, const int tid) {
    for (int e = tid; e < 5 * N; e += PG_NT) {
        const int a = ea[e], b = e / 5;
        double rho = 0.0;
        if (a >= 0) rho = pg_edge<JAC>(yaw[a], c.pr[2 * a], c.pr[2 * a + 1], t + 3 * a, yaw[b], t + 3 * b, c.meas + 4 * e, e - 5 * b == 4, delta,
                                       c.res + 4 * e, c.Ja + 16 * e, c.Jb + 16 * e);
        c.ev[e] = rho;
    }
    __syncthreads();
    const double* ev = c.ev;
    return pg_sum(S.red, 5 * N, tid, [&](int k) { return ev[k]; }) / 2.0;
}

// M(i, i - o) of the LM system: the band blocks of As plus D D on the diagonal (zero outside the block band)
DEV double pg_band_entry(const double* Ab, const double* dd, const int i, const int o) {
    const int k = i - o, f = i >> 2, pp = i & 3, fk = k >> 2, qq = k & 3, d = f - fk;
    if (d > 4) return 0.0;
    const double v = Ab[(size_t)f * 80 + 16 * d + 4 * pp + qq];
    return o == 0 ? v + dd[i] : v;
}

// Unpivoted banded Cholesky of M by wavefront 0 -> Lb [n][PG_BW]; S.flag = 0 when a pivot is not positive and finite
DEV void pg_factor(PgLds& S, const PgCarve& c, const int n, const int tid) {
    if (tid == 0) S.flag = 1;
    if (tid < 64) {
        const int lane = tid;
        for (int k = lane; k < PG_BW * PG_BW; k += 64) S.W[k] = 0.0;
        __builtin_amdgcn_wave_barrier();
        if (lane < PG_BW)
            for (int i = lane; i < PG_BW && i < n; ++i) S.W[i * PG_BW + (i - lane)] = pg_band_entry(c.Ab, c.dd, i, lane);      // (i, i - lane)
        __builtin_amdgcn_wave_barrier();
        bool ok = true;
#pragma unroll 1
        for (int j = 0; j < n && ok; ++j) {
            const int jm = j % PG_BW, in = j + PG_BW;
            // the operands of the row that enters behind this column, in flight while the column is factored
            const double pre = (lane < PG_BW && in < n) ? pg_band_entry(c.Ab, c.dd, in, lane) : 0.0;
            const double piv = S.W[jm * PG_BW + jm];
            ok = piv > 0.0 && sf_finite(piv);
            if (!ok) break;
            const double inv = 1.0 / sqrt(piv);
            if (lane == 0) c.Lb[(size_t)j * PG_BW] = inv;
            else if (lane < PG_BW && j + lane < n) {
                const int i = j + lane, at = (i % PG_BW) * PG_BW + jm;
                const double v = S.W[at] * inv;
                S.W[at] = v;
                c.Lb[(size_t)i * PG_BW + lane] = v;
            }
            __builtin_amdgcn_wave_barrier();
            for (int q = lane; q < PG_PAIRS; q += 64) {
                const int i = j + S.pi[q], k = j + S.pk[q];
                if (i < n) {
                    const int ri = (i % PG_BW) * PG_BW, rk = (k % PG_BW) * PG_BW;
                    S.W[ri + k % PG_BW] -= S.W[ri + jm] * S.W[rk + jm];
                }
            }
            __builtin_amdgcn_wave_barrier();
            if (lane < PG_BW && in < n) S.W[jm * PG_BW + (in - lane) % PG_BW] = pre;
            __builtin_amdgcn_wave_barrier();
        }
        if (!ok && lane == 0) S.flag = 0;
    }
    __syncthreads();
}

// rows [r0, r0 + nl) of the factor and [s0, s0 + ns) of the right-hand side into chunk `buf` (rows outside 0 .. n - 1 are left out)
DEV void pg_stage(PgLds& S, const double* Lb, const double* rhs, const int n, const int buf, const int r0, const int nl, const int s0, const int ns,
                  const int t, const int nt) {
    const int rows = r0 + nl <= n ? nl : n - r0;
    const double* src = Lb + (size_t)r0 * PG_BW;
    for (int k = t; k < rows * PG_BW; k += nt) S.Lc[buf][k] = src[k];
    for (int k = t; k < ns; k += nt) {
        const int i = s0 + k;
        if (i >= 0 && i < n) S.Rc[buf][k] = rhs[i];
    }
}

// FWD: L z = rhs, else L^T z = rhs (rhs and z are different vectors).  Wavefront 0 sweeps; lane l keeps the running right-hand side of the
// row = l (mod 32) in `acc`: when its row is solved the lane takes the row 32 further on, whose first update is 13 steps away.  Nothing in
// a step branches per lane, the LDS operands of step j + 1 are read while step j's chain (readlane, three multiply / subtract) runs, and
// the solved entries leave 32 at a time.
template <bool FWD>
DEV void pg_sweep(PgLds& S, const double* Lb, const double* rhs, double* z, const int n, const int tid) {
    const int nchunk = (n + PG_CH - 1) / PG_CH;
    {
        const int c0 = FWD ? 0 : nchunk - 1, r0 = c0 * PG_CH;
        pg_stage(S, Lb, rhs, n, c0 & 1, r0, FWD ? PG_CHR : PG_CH, FWD ? r0 : r0 - PG_RH, PG_CH + PG_RH, tid, PG_NT);
    }
    __syncthreads();
    double acc = 0.0, zo = 0.0;
#pragma unroll 1
    for (int cc = 0; cc < nchunk; ++cc) {
        const int ch = FWD ? cc : nchunk - 1 - cc, r0 = ch * PG_CH, buf = ch & 1;
        if (tid >= 64) {
            if (cc + 1 < nchunk) {
                const int nx = FWD ? ch + 1 : ch - 1, x0 = nx * PG_CH;
                pg_stage(S, Lb, rhs, n, nx & 1, x0, FWD ? PG_CHR : PG_CH, FWD ? x0 : x0 - PG_RH, PG_CH + PG_RH, tid - 64, PG_NT - 64);
            }
        } else {
            const int lane = tid, rend = r0 + PG_CH < n ? r0 + PG_CH : n;
            const double* L = S.Lc[buf];
            const double* Rr = S.Rc[buf];
            // the three LDS operands of step j: 1 / L(j, j), this lane's entry of the column (FWD) or row (else) and the right-hand side
            // of the row the solving lane takes next; a lane without an entry, and a step outside the chunk, read slot 0
            auto operands = [&](const int j, double& inv, double& lv, double& nxt) {
                const bool in = j >= r0 && j < rend;
                const int o = FWD ? (lane - j) & 31 : (j - lane) & 31, i = FWD ? j + o : j - o;
                const bool has = in && o >= 1 && o <= PG_KD && (FWD ? i < n : i >= 0);
                const bool more = in && (FWD ? j + PG_RH < n : j - PG_RH >= 0);
                inv = L[in ? (j - r0) * PG_BW : 0];
                lv = L[has ? (FWD ? (i - r0) * PG_BW + o : (j - r0) * PG_BW + o) : 0];
                nxt = Rr[more ? (FWD ? j + PG_RH - r0 : j - r0) : 0];
            };
            if (cc == 0) {
                const int row = FWD ? (lane & 31) : n - 1 - ((n - 1 - lane) & 31);
                acc = (row >= 0 && row < n) ? Rr[FWD ? row : row - (r0 - PG_RH)] : 0.0;
            }
            double inv, lv, nxt;
            operands(FWD ? r0 : rend - 1, inv, lv, nxt);
#pragma unroll 1
            for (int s = 0; s < rend - r0; ++s) {
                const int j = FWD ? r0 + s : rend - 1 - s;
                double inv_n, lv_n, nxt_n;
                operands(FWD ? j + 1 : j - 1, inv_n, lv_n, nxt_n);
                const int o = FWD ? (lane - j) & 31 : (j - lane) & 31, i = FWD ? j + o : j - o;
                const bool has = o >= 1 && o <= PG_KD && (FWD ? i < n : i >= 0);
                const double zj = readlane_f64(acc, j & 31) * inv;
                const double upd = acc - lv * zj;
                zo = o == 0 ? zj : zo;
                acc = o == 0 ? nxt : (has ? upd : acc);
                if (FWD ? ((j & 31) == 31 || j == rend - 1) : (j & 31) == 0) {
                    const int row = (j & ~31) + lane;
                    if (lane < 32 && (FWD ? row <= j : row < rend)) z[row] = zo;
                }
                inv = inv_n; lv = lv_n; nxt = nxt_n;
            }
        }
        __syncthreads();
    }
}

// q = A p over the free nodes, a thread per row, in the header's order
DEV void pg_matvec(const PgCarve& c, const int* fidx, const int* nof, const int* ea, const int* lp_off, const int* lp_src, const int NF, const double* p,
                   double* q, const int tid) {
    for (int i = tid; i < 4 * NF; i += PG_NT) {
        const int f = i >> 2, pp = i & 3;
        double acc = 0.0;
        for (int d = 4; d >= 1; --d)
            if (f - d >= 0) {
                const double* B = c.Ab + (size_t)f * 80 + 16 * d + 4 * pp;
                const double* v = p + 4 * (f - d);
                double t = B[0] * v[0];
                t += B[1] * v[1]; t += B[2] * v[2]; t += B[3] * v[3];
                acc += t;
            }
        {
            const double* B = c.Ab + (size_t)f * 80 + 4 * pp;
            const double* v = p + 4 * f;
            double t = B[0] * v[0];
            t += B[1] * v[1]; t += B[2] * v[2]; t += B[3] * v[3];
            acc += t;
        }
        for (int d = 1; d <= 4; ++d)
            if (f + d < NF) {
                const double* B = c.Ab + (size_t)(f + d) * 80 + 16 * d + pp;
                const double* v = p + 4 * (f + d);
                double t = B[0] * v[0];
                t += B[4] * v[1]; t += B[8] * v[2]; t += B[12] * v[3];
                acc += t;
            }
        const int n = nof[f], a = ea[5 * n + 4];
        if (a >= 0 && fidx[a] >= 0 && f - fidx[a] > 4) {
            const double* B = c.LB + 16 * n + 4 * pp;
            const double* v = p + 4 * fidx[a];
            double t = B[0] * v[0];
            t += B[1] * v[1]; t += B[2] * v[2]; t += B[3] * v[3];
            acc += t;
        }
        for (int k = lp_off[n]; k < lp_off[n + 1]; ++k) {
            const int s = lp_src[k], fs = fidx[s];
            if (fs >= 0 && fs - f > 4) {
                const double* B = c.LB + 16 * s + pp;
                const double* v = p + 4 * fs;
                double t = B[0] * v[0];
                t += B[4] * v[1]; t += B[8] * v[2]; t += B[12] * v[3];
                acc += t;
            }
        }
        acc += c.dd[i] * p[i];
        q[i] = acc;
    }
    __syncthreads();
}

extern "C" __global__ __launch_bounds__(PG_NT) void pg_solve_kernel(PgDev b) {
    __shared__ PgLds S;
    const int g = blockIdx.x, tid = threadIdx.x;
    if (g >= b.G) return;
    const int* gi = b.gi + (size_t)g * PG_GI;
    const long long* go = b.go + (size_t)g * PG_GO;
    const int N = gi[PG_N], NKF = gi[PG_NKF], NF = gi[PG_NF], max_it = gi[PG_MAXIT];
    const double delta = b.delta[g];
    const int* fidx = b.ints + go[PG_O_INT];
    const int* nof = fidx + N;
    const int* ea = nof + N;
    const int* lp_off = ea + 5 * N;
    const int* lp_src = lp_off + N + 1;
    const double* vT = b.in + go[PG_O_IN];
    const double* vR = vT + 3 * NKF;
    const double* lmeas = vR + 9 * NKF;
    double* od = b.out + go[PG_O_OUT];
    int* oi = (int*)(od + PG_OUT_HDR);
    double* oT = od + PG_OUT_HDR + PG_OUT_INT / 2;
    double* oR = oT + 3 * NKF;
    const PgCarve c = pg_carve(b.scratch + go[PG_O_SCR], N);
    // the pairs (i - j, k - j), 1 <= k - j <= i - j <= 19, of a column's update
    for (int q = tid; q < PG_PAIRS; q += PG_NT) {
        int li = 1, rest = q;
        while (rest >= li) { rest -= li; ++li; }
        S.pi[q] = (unsigned char)li; S.pk[q] = (unsigned char)(rest + 1);
    }
    // ---- the nodes, the measurements
    for (int i = tid; i < N; i += PG_NT) {
        double ypr[3];
        pg_R2ypr(vR + 9 * i, ypr);
        c.yaw[i] = ypr[0]; c.pr[2 * i] = ypr[1]; c.pr[2 * i + 1] = ypr[2];
        c.t[3 * i] = vT[3 * i]; c.t[3 * i + 1] = vT[3 * i + 1]; c.t[3 * i + 2] = vT[3 * i + 2];
    }
    __syncthreads();
    for (int e = tid; e < 5 * N; e += PG_NT) {
        const int a = ea[e], i = e / 5;
        double* m = c.meas + 4 * e;
        if (a < 0) { m[0] = m[1] = m[2] = m[3] = 0.0; continue; }
        if (e - 5 * i == 4) { m[0] = lmeas[4 * i]; m[1] = lmeas[4 * i + 1]; m[2] = lmeas[4 * i + 2]; m[3] = lmeas[4 * i + 3]; continue; }
        const double d[3] = {c.t[3 * i] - c.t[3 * a], c.t[3 * i + 1] - c.t[3 * a + 1], c.t[3 * i + 2] - c.t[3 * a + 2]};
        m3t_vec(vR + 9 * a, d, m);
        m[3] = c.yaw[i] - c.yaw[a];
    }
    __syncthreads();
    double cost = pg_evaluate<true>(S, c, ea, N, delta, c.yaw, c.t, tid);
    const double cost0 = cost;
    int it = 0, term = 0, invalid = 0;                          // VG_TERM_NO_CONVERGENCE
    const bool finite0 = sf_finite(cost0);
    if (NF > 0 && finite0) {
        const int n = 4 * NF;
        double radius = 1e4, dec = 2.0, x_norm = 0.0;
        bool relin = true, first = true;
        const double *yw = c.yaw, *tt = c.t, *cy = c.cyaw, *ctt = c.ct, *gp = c.g;
#pragma unroll 1
        while (true) {
            if (relin) {
                // ---- the gathers: diagonal block, gradient, band blocks, out-of-band loop block of every free node
                for (int f = tid; f < NF; f += PG_NT) {
                    const int nd = nof[f];
                    double D[16], gg[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                    for (int k = 0; k < 16; ++k) D[k] = 0.0;
                    for (int k = 0; k < 5; ++k) {
                        const int e = 5 * nd + k;
                        if (ea[e] >= 0) { pg_add_AtB(D, c.Jb + 16 * e, c.Jb + 16 * e); pg_add_Atr(gg, c.Jb + 16 * e, c.res + 4 * e); }
                    }
                    for (int j = 1; j <= 4; ++j)
                        if (nd + j < N) {
                            const int e = 5 * (nd + j) + j - 1;
                            if (ea[e] >= 0) { pg_add_AtB(D, c.Ja + 16 * e, c.Ja + 16 * e); pg_add_Atr(gg, c.Ja + 16 * e, c.res + 4 * e); }
                        }
                    for (int k = lp_off[nd]; k < lp_off[nd + 1]; ++k) {
                        const int e = 5 * lp_src[k] + 4;
                        pg_add_AtB(D, c.Ja + 16 * e, c.Ja + 16 * e); pg_add_Atr(gg, c.Ja + 16 * e, c.res + 4 * e);
                    }
                    double* A = c.Ab + (size_t)f * 80;
#pragma unroll
                    for (int k = 0; k < 16; ++k) A[k] = D[k];
#pragma unroll
                    for (int k = 0; k < 4; ++k) c.g[4 * f + k] = gg[k];
                    for (int d = 1; d <= 4; ++d) {
#pragma unroll
                        for (int k = 0; k < 16; ++k) D[k] = 0.0;
                        if (f - d >= 0) {
                            const int q = nof[f - d], dist = nd - q;
                            if (dist <= 4 && ea[5 * nd + dist - 1] >= 0) { const int e = 5 * nd + dist - 1; pg_add_AtB(D, c.Jb + 16 * e, c.Ja + 16 * e); }
                            if (ea[5 * nd + 4] == q) { const int e = 5 * nd + 4; pg_add_AtB(D, c.Jb + 16 * e, c.Ja + 16 * e); }
                        }
#pragma unroll
                        for (int k = 0; k < 16; ++k) A[16 * d + k] = D[k];
                    }
#pragma unroll
                    for (int k = 0; k < 16; ++k) D[k] = 0.0;
                    const int la = ea[5 * nd + 4];
                    if (la >= 0 && fidx[la] >= 0 && f - fidx[la] > 4) { const int e = 5 * nd + 4; pg_add_AtB(D, c.Jb + 16 * e, c.Ja + 16 * e); }
#pragma unroll
                    for (int k = 0; k < 16; ++k) c.LB[16 * nd + k] = D[k];
                }
                __syncthreads();
                if (first)
                    for (int i = tid; i < n; i += PG_NT) c.scale[i] = 1.0 / (1.0 + sqrt(c.Ab[(size_t)(i >> 2) * 80 + 5 * (i & 3)]));
                // |x| over the free nodes; the gradient tolerance, at the start and after every accepted step
                x_norm = sqrt(pg_sum(S.red, n, tid, [&](int i) { const int nd = nof[i >> 2]; const double v = (i & 3) ? tt[3 * nd + (i & 3) - 1] : yw[nd]; return v * v; }));
                if (pg_max(S.red, n, tid, [&](int i) { return fabs(gp[i]); }) <= 1e-10) { term = 1; break; }
                // ---- the Jacobi scale on both sides, the clamped diagonal
                for (int f = tid; f < NF; f += PG_NT) {
                    double* A = c.Ab + (size_t)f * 80;
                    const double* sr = c.scale + 4 * f;
                    for (int pp = 0; pp < 4; ++pp)
                        for (int qq = 0; qq <= pp; ++qq) {
                            const double v = sr[pp] * (A[4 * pp + qq] * sr[qq]);
                            A[4 * pp + qq] = v; A[4 * qq + pp] = v;
                        }
                    for (int d = 1; d <= 4; ++d)
                        if (f - d >= 0) {
                            const double* sq = c.scale + 4 * (f - d);
                            for (int pp = 0; pp < 4; ++pp)
                                for (int qq = 0; qq < 4; ++qq) A[16 * d + 4 * pp + qq] = sr[pp] * (A[16 * d + 4 * pp + qq] * sq[qq]);
                        }
                    const int nd = nof[f], la = ea[5 * nd + 4];
                    if (la >= 0 && fidx[la] >= 0 && f - fidx[la] > 4) {
                        const double* sq = c.scale + 4 * fidx[la];
                        for (int pp = 0; pp < 4; ++pp)
                            for (int qq = 0; qq < 4; ++qq) c.LB[16 * nd + 4 * pp + qq] = sr[pp] * (c.LB[16 * nd + 4 * pp + qq] * sq[qq]);
                    }
                    for (int pp = 0; pp < 4; ++pp) {
                        c.gs[4 * f + pp] = c.g[4 * f + pp] * sr[pp];
                        c.dcl[4 * f + pp] = fmin(fmax(A[5 * pp], 1e-6), 1e32);
                    }
                }
                __syncthreads();
                relin = false; first = false;
            }
            if (it >= max_it) break;
            ++it;
            const int row = it - 1;
            for (int i = tid; i < n; i += PG_NT) { const double D = sqrt(c.dcl[i] / radius); c.dd[i] = D * D; }
            __syncthreads();
            // ---- the step: Cholesky of the band, conjugate gradients
            pg_factor(S, c, n, tid);
            bool valid = S.flag != 0;
            int cg = 0;
            double model = 0.0;
            if (valid) {
                for (int i = tid; i < n; i += PG_NT) { c.x[i] = 0.0; c.r[i] = -c.gs[i]; }
                __syncthreads();
                pg_sweep<true>(S, c.Lb, c.r, c.w, n, tid);
                pg_sweep<false>(S, c.Lb, c.w, c.z, n, tid);
                for (int i = tid; i < n; i += PG_NT) c.p[i] = c.z[i];
                const double *rr = c.r, *zz = c.z, *ppv = c.p, *qq = c.q;
                double rz = pg_sum(S.red, n, tid, [&](int i) { return rr[i] * zz[i]; });
                const double rz0 = rz;
                bool done = false;
                valid = rz0 > 0.0 && sf_finite(rz0);
#pragma unroll 1
                while (valid && !done && cg < VG_PG_MAX_CG) {
                    ++cg;
                    pg_matvec(c, fidx, nof, ea, lp_off, lp_src, NF, c.p, c.q, tid);
                    const double pq = pg_sum(S.red, n, tid, [&](int i) { return ppv[i] * qq[i]; });
                    if (!(pq > 0.0) || !sf_finite(pq)) { valid = false; break; }
                    const double alpha = rz / pq;
                    for (int i = tid; i < n; i += PG_NT) { c.x[i] += alpha * c.p[i]; c.r[i] -= alpha * c.q[i]; }
                    __syncthreads();
                    pg_sweep<true>(S, c.Lb, c.r, c.w, n, tid);
                    pg_sweep<false>(S, c.Lb, c.w, c.z, n, tid);
                    const double rzn = pg_sum(S.red, n, tid, [&](int i) { return rr[i] * zz[i]; });
                    if (!(rzn > -1.79e308 && rzn < 1.79e308)) { valid = false; break; }
                    if (rzn <= 1e-24 * rz0) { done = true; break; }
                    const double beta = rzn / rz;
                    for (int i = tid; i < n; i += PG_NT) c.p[i] = c.z[i] + beta * c.p[i];
                    __syncthreads();
                    rz = rzn;
                }
                valid = valid && done;
            }
            if (valid) {
                // the step in the parameters (kept in w), the model change
                for (int i = tid; i < n; i += PG_NT) c.w[i] = c.scale[i] * c.x[i];
                __syncthreads();
                for (int e = tid; e < 5 * N; e += PG_NT) {
                    const int a = ea[e], bn = e / 5;
                    double m = 0.0;
                    if (a >= 0) {
                        const int fa = fidx[a], fb = fidx[bn];
                        double u[4] = {0.0, 0.0, 0.0, 0.0};
                        if (fa >= 0) {
                            const double* J = c.Ja + 16 * e; const double* v = c.w + 4 * fa;
                            for (int r = 0; r < 4; ++r) { double t = J[4 * r] * v[0]; t += J[4 * r + 1] * v[1]; t += J[4 * r + 2] * v[2]; t += J[4 * r + 3] * v[3]; u[r] += t; }
                        }
                        if (fb >= 0) {
                            const double* J = c.Jb + 16 * e; const double* v = c.w + 4 * fb;
                            for (int r = 0; r < 4; ++r) { double t = J[4 * r] * v[0]; t += J[4 * r + 1] * v[1]; t += J[4 * r + 2] * v[2]; t += J[4 * r + 3] * v[3]; u[r] += t; }
                        }
                        const double* r4 = c.res + 4 * e;
                        m = u[0] * (r4[0] + u[0] / 2.0);
                        m += u[1] * (r4[1] + u[1] / 2.0); m += u[2] * (r4[2] + u[2] / 2.0); m += u[3] * (r4[3] + u[3] / 2.0);
                    }
                    c.ev[e] = m;
                }
                __syncthreads();
                const double* ev = c.ev;
                model = -pg_sum(S.red, 5 * N, tid, [&](int k) { return ev[k]; });
                valid = model > 0.0;
            }
            if (tid == 0) {
                od[16 + 4 * row] = cost; od[16 + 4 * row + 1] = radius; od[16 + 4 * row + 2] = 0.0; od[16 + 4 * row + 3] = model;
                oi[4 + row] = 0; oi[12 + row] = cg;
            }
            if (!valid) {
                if (++invalid >= 5) { term = 2; break; }
                radius = radius / dec; dec = dec * 2.0;
                continue;
            }
            invalid = 0;
            // ---- the candidate
            for (int i = tid; i < N; i += PG_NT) {
                const int f = fidx[i];
                c.cyaw[i] = f >= 0 ? pg_normalize(c.yaw[i] + c.w[4 * f]) : c.yaw[i];
                for (int k = 0; k < 3; ++k) c.ct[3 * i + k] = f >= 0 ? c.t[3 * i + k] + c.w[4 * f + 1 + k] : c.t[3 * i + k];
            }
            __syncthreads();
            const double cost2 = pg_evaluate<false>(S, c, ea, N, delta, c.cyaw, c.ct, tid);
            const double dxn = sqrt(pg_sum(S.red, n, tid, [&](int i) {
                const int nd = nof[i >> 2], k = i & 3;
                const double v = k ? tt[3 * nd + k - 1] - ctt[3 * nd + k - 1] : yw[nd] - cy[nd];
                return v * v;
            }));
            if (tid == 0) { od[16 + 4 * row + 2] = cost2; oi[4 + row] = 1; }
            if (dxn <= 1e-8 * (x_norm + 1e-8)) { term = 1; break; }
            if (fabs(cost - cost2) <= 1e-6 * cost) { term = 1; break; }
            const double rho = (cost - cost2) / model;
            if (rho > 1e-3) {
                if (tid == 0) oi[4 + row] = 3;
                for (int i = tid; i < N; i += PG_NT) {
                    c.yaw[i] = c.cyaw[i];
                    for (int k = 0; k < 3; ++k) c.t[3 * i + k] = c.ct[3 * i + k];
                }
                __syncthreads();
                cost = pg_evaluate<true>(S, c, ea, N, delta, c.yaw, c.t, tid);
                const double t3 = 2.0 * rho - 1.0;
                radius = fmin(radius / fmax(1.0 / 3.0, 1.0 - t3 * t3 * t3), 1e16);
                dec = 2.0;
                relin = true;                                   // (the gathers, |x| and the gradient tolerance at the head of the loop)
            } else {
                radius = radius / dec; dec = dec * 2.0;
                if (radius < 1e-32) { term = 1; break; }
            }
        }
    } else if (finite0) term = 1;
    __syncthreads();
    // ---- updatePose of the optimised keyframes, the drift, the keyframes behind cur_index
    for (int i = tid; i < N; i += PG_NT) {
        pg_ypr2R(c.yaw[i], c.pr[2 * i], c.pr[2 * i + 1], oR + 9 * i);
        oT[3 * i] = c.t[3 * i]; oT[3 * i + 1] = c.t[3 * i + 1]; oT[3 * i + 2] = c.t[3 * i + 2];
    }
    __syncthreads();
    double rd[9], td[3], yd;
    {
        const int cur = N - 1;
        double yc[3], yv[3], rv[3];
        pg_R2ypr(oR + 9 * cur, yc);
        pg_R2ypr(vR + 9 * cur, yv);
        yd = yc[0] - yv[0];
        pg_ypr2R(yd, 0.0, 0.0, rd);
        m3_vec(rd, vT + 3 * cur, rv);
        td[0] = oT[3 * cur] - rv[0]; td[1] = oT[3 * cur + 1] - rv[1]; td[2] = oT[3 * cur + 2] - rv[2];
    }
    for (int i = N + tid; i < NKF; i += PG_NT) {
        double P[3];
        m3_vec(rd, vT + 3 * i, P);
        oT[3 * i] = P[0] + td[0]; oT[3 * i + 1] = P[1] + td[1]; oT[3 * i + 2] = P[2] + td[2];
        m3_mul(rd, vR + 9 * i, oR + 9 * i);
    }
    __syncthreads();
    const double bad = pg_max(S.red, 12 * NKF, tid, [&](int k) { return sf_finite(oT[k]) ? 0.0 : 1.0; });      // (T and R lie back to back)
    bool numeric = !finite0 || bad != 0.0 || !sf_finite(cost) || !sf_finite(yd);
    for (int k = 0; k < 3; ++k) numeric = numeric || !sf_finite(td[k]);
    if (numeric) {
        for (int k = tid; k < 12 * NKF; k += PG_NT) oT[k] = 0.0;
    }
    if (tid == 0) {
        od[0] = cost0; od[1] = cost; od[2] = numeric ? 0.0 : yd;
        for (int k = 0; k < 9; ++k) od[3 + k] = numeric ? 0.0 : rd[k];
        for (int k = 0; k < 3; ++k) od[12 + k] = numeric ? 0.0 : td[k];
        oi[0] = numeric ? VG_PG_NUMERIC : (NF > 0 ? VG_PG_OK : VG_PG_NO_EDGES); oi[1] = term; oi[2] = it;
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
extern "C" void vg_pg_defaults(vg_pg_in* in) {
    if (!in) return;
    *in = vg_pg_in();
    in->struct_size = sizeof(vg_pg_in);
    in->max_iters = 5; in->huber_delta = 0.1;
}

extern "C" int vg_pg_optimize(vg_handle* h, int n_graphs, const vg_pg_in* in, vg_pg_out* out) {
    VG_RANGE("vg_pg_optimize");
    if (!h) return VG_ERR_BAD_ARG;
    auto bad = [&](int w, const char* what) {
        h->err = "vg_pg_optimize: graph " + std::to_string(w) + ": " + what;
        return VG_ERR_BAD_ARG;
    };
    if (n_graphs <= 0 || !in || !out) { h->err = "vg_pg_optimize: n_graphs <= 0 or a NULL argument"; return VG_ERR_BAD_ARG; }
    // ---- everything that follows from the arguments alone, before anything is uploaded or written
    const int G = n_graphs;
    std::vector<int> hgi((size_t)PG_GI * G, 0), hint, stat((size_t)3 * G, 0);
    std::vector<long long> hgo((size_t)PG_GO * G, 0);
    std::vector<double> hdelta(G), hin;
    size_t n_scr = 0, n_out = 0;
    for (int w = 0; w < G; ++w) {
        const vg_pg_in& a = in[w];
        if (a.struct_size != sizeof(vg_pg_in)) return bad(w, "vg_pg_in::struct_size");
        if (out[w].struct_size != sizeof(vg_pg_out)) return bad(w, "vg_pg_out::struct_size");
        if (a.n_kf < 1 || a.n_kf > VG_PG_MAX_KEYFRAMES) return bad(w, "n_kf outside 1 .. VG_PG_MAX_KEYFRAMES");
        if (a.n_opt < 1 || a.n_opt > a.n_kf) return bad(w, "n_opt outside 1 .. n_kf");
        if (!a.index || !a.sequence || !a.has_loop || !a.loop_index || !a.vio_T || !a.vio_R || !a.loop_info) return bad(w, "a NULL table");
        if (a.max_iters < 1 || a.max_iters > VG_PG_MAX_ITERS) return bad(w, "max_iters outside 1 .. VG_PG_MAX_ITERS");
        if (!(a.huber_delta > 0) || !std::isfinite(a.huber_delta)) return bad(w, "huber_delta is not positive");
        const int N = a.n_opt, NKF = a.n_kf;
        if (a.index[0] < a.first_looped_index) return bad(w, "the first keyframe lies below first_looped_index");
        for (int i = 1; i < NKF; ++i) if (a.index[i] <= a.index[i - 1]) return bad(w, "index is not strictly ascending");
        for (int i = 0; i < NKF; ++i) if (a.sequence[i] < 0) return bad(w, "sequence < 0");
        if (!rp_finite(a.vio_T, 3 * (size_t)NKF) || !rp_finite(a.vio_R, 9 * (size_t)NKF)) return bad(w, "a non-finite input");
        const size_t i0 = hint.size(), d0 = hin.size();
        hint.resize(i0 + (size_t)9 * N + 1, -1);
        int* fidx = hint.data() + i0;
        int* nof = fidx + N;
        int* ea = nof + N;
        int* lp_off = ea + 5 * N;
        int* lp_src = lp_off + N + 1;
        int NF = 0, n_edges = 0, n_loop = 0;
        for (int i = 0; i < N; ++i) {
            const bool constant = a.index[i] == a.first_looped_index || a.sequence[i] == 0;
            fidx[i] = constant ? -1 : NF;
            if (!constant) nof[NF++] = i;
        }
        std::fill(lp_off, lp_off + N + 1, 0);
        for (int i = 0; i < N; ++i) {
            for (int j = 1; j <= 4; ++j)
                if (i - j >= 0 && a.sequence[i] == a.sequence[i - j]) { ea[5 * i + j - 1] = i - j; ++n_edges; }
            if (!a.has_loop[i]) continue;
            if (a.loop_index[i] < a.first_looped_index) return bad(w, "a loop_index below first_looped_index");
            const int* at = std::lower_bound(a.index, a.index + NKF, a.loop_index[i]);
            if (at == a.index + NKF || *at != a.loop_index[i]) return bad(w, "a loop_index that is not in the slice");
            const int la = (int)(at - a.index);
            if (la >= i) return bad(w, "a loop_index that is not before its own keyframe");
            if (!rp_finite(a.loop_info + 8 * (size_t)i, 8)) return bad(w, "a non-finite input");
            ea[5 * i + 4] = la; ++n_edges; ++n_loop;
            ++lp_off[la + 1];
        }
        for (int i = 0; i < N; ++i) lp_off[i + 1] += lp_off[i];
        {
            std::vector<int> fill(lp_off, lp_off + N);
            for (int i = 0; i < N; ++i)
                if (ea[5 * i + 4] >= 0) lp_src[fill[ea[5 * i + 4]]++] = i;           // (ascending source: i ascends)
        }
        hin.resize(d0 + (size_t)12 * NKF + 4 * N, 0.0);
        std::copy(a.vio_T, a.vio_T + 3 * (size_t)NKF, hin.begin() + d0);
        std::copy(a.vio_R, a.vio_R + 9 * (size_t)NKF, hin.begin() + d0 + 3 * (size_t)NKF);
        for (int i = 0; i < N; ++i)
            if (a.has_loop[i]) {
                double* m = hin.data() + d0 + (size_t)12 * NKF + 4 * i;
                m[0] = a.loop_info[8 * i]; m[1] = a.loop_info[8 * i + 1]; m[2] = a.loop_info[8 * i + 2]; m[3] = a.loop_info[8 * i + 7];
            }
        int* q = hgi.data() + (size_t)PG_GI * w;
        q[PG_N] = N; q[PG_NKF] = NKF; q[PG_NF] = NF; q[PG_MAXIT] = a.max_iters; q[PG_NLP] = n_loop;
        long long* o = hgo.data() + (size_t)PG_GO * w;
        o[PG_O_INT] = (long long)i0; o[PG_O_IN] = (long long)d0; o[PG_O_SCR] = (long long)n_scr; o[PG_O_OUT] = (long long)n_out;
        n_scr += (size_t)PG_SCR_N * N;
        n_out += PG_OUT_HDR + PG_OUT_INT / 2 + (size_t)12 * NKF;
        hdelta[w] = a.huber_delta;
        stat[3 * w] = n_edges; stat[3 * w + 1] = n_loop; stat[3 * w + 2] = NF;
    }
    if (hint.size() & 1) hint.push_back(0);
    std::vector<double> hout(n_out);
    hipError_t e = hipSetDevice(h->device);
    auto fail = [&](hipError_t err) { h->err = std::string("vg_pg_optimize: ") + hipGetErrorString(err); return VG_ERR_HIP; };
    if (e != hipSuccess) return fail(e);
    // ---- device block (the scratch block of vg_init_relpose, grown on demand): [out | in | delta | go | gi | ints | scratch]
    const size_t b_out = 0, b_in = b_out + n_out * 8, b_dl = b_in + hin.size() * 8, b_go = b_dl + (size_t)G * 8, b_gi = b_go + hgo.size() * 8;
    const size_t b_it = b_gi + hgi.size() * 4, b_sc = rp_up(b_it + hint.size() * 4, 256), total = b_sc + n_scr * 8;
    if ((e = rp_scratch(h, total)) != hipSuccess) return fail(e);
    char* base = (char*)h->relpose_buf;
    PgDev b;
    b.G = G;
    b.out = (double*)(base + b_out); b.in = (const double*)(base + b_in); b.delta = (const double*)(base + b_dl);
    b.go = (const long long*)(base + b_go); b.gi = (const int*)(base + b_gi); b.ints = (const int*)(base + b_it); b.scratch = (double*)(base + b_sc);
    if ((e = hipMemcpyAsync(base + b_in, hin.data(), hin.size() * 8, hipMemcpyHostToDevice, h->stream)) != hipSuccess) return fail(e);
    if ((e = hipMemcpyAsync(base + b_dl, hdelta.data(), (size_t)G * 8, hipMemcpyHostToDevice, h->stream)) != hipSuccess) return fail(e);
    if ((e = hipMemcpyAsync(base + b_go, hgo.data(), hgo.size() * 8, hipMemcpyHostToDevice, h->stream)) != hipSuccess) return fail(e);
    if ((e = hipMemcpyAsync(base + b_gi, hgi.data(), hgi.size() * 4, hipMemcpyHostToDevice, h->stream)) != hipSuccess) return fail(e);
    if ((e = hipMemcpyAsync(base + b_it, hint.data(), hint.size() * 4, hipMemcpyHostToDevice, h->stream)) != hipSuccess) return fail(e);
    if ((e = hipMemsetAsync(b.out, 0, n_out * 8, h->stream)) != hipSuccess) return fail(e);
    struct Events {                                         // destroyed on every way out
        hipEvent_t ev[VG_PG_LAUNCHES + 1] = {};
        ~Events() { for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x); }
    } evs;
    const bool timed = out[0].device_ms != nullptr;
    if (timed)
        for (int i = 0; i <= VG_PG_LAUNCHES; ++i)
            if ((e = hipEventCreate(&evs.ev[i])) != hipSuccess) return fail(e);
    if (timed && (e = hipEventRecord(evs.ev[0], h->stream)) != hipSuccess) return fail(e);
    hipLaunchKernelGGL(pg_solve_kernel, dim3((unsigned)G), dim3(PG_NT), 0, h->stream, b);
    if (timed && (e = hipEventRecord(evs.ev[1], h->stream)) != hipSuccess) return fail(e);
    if ((e = hipGetLastError()) != hipSuccess) return fail(e);
    if ((e = hipMemcpyAsync(hout.data(), b.out, n_out * 8, hipMemcpyDeviceToHost, h->stream)) != hipSuccess) return fail(e);
    if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return fail(e);
    if (timed) {
        float ms = 0.f;
        if ((e = hipEventElapsedTime(&ms, evs.ev[0], evs.ev[1])) != hipSuccess) return fail(e);
        out[0].device_ms[0] = ms;
    }
    for (int w = 0; w < G; ++w) {
        vg_pg_out& o = out[w];
        const int NKF = in[w].n_kf;
        const double* od = hout.data() + hgo[(size_t)PG_GO * w + PG_O_OUT];
        const int* oi = (const int*)(od + PG_OUT_HDR);
        o.status = oi[0]; o.termination = oi[1]; o.iterations = oi[2];
        o.n_edges = stat[3 * w]; o.n_loop_edges = stat[3 * w + 1]; o.n_free = stat[3 * w + 2];
        o.initial_cost = od[0]; o.final_cost = od[1]; o.yaw_drift = od[2];
        std::copy(od + 3, od + 12, o.r_drift); std::copy(od + 12, od + 15, o.t_drift);
        for (int k = 0; k < VG_PG_MAX_ITERS; ++k) {
            o.it_cost[k] = od[16 + 4 * k]; o.it_radius[k] = od[16 + 4 * k + 1]; o.it_cost_cand[k] = od[16 + 4 * k + 2]; o.it_model[k] = od[16 + 4 * k + 3];
            o.it_flags[k] = oi[4 + k]; o.it_cg[k] = oi[12 + k];
        }
        const double* T = od + PG_OUT_HDR + PG_OUT_INT / 2;
        if (o.T) std::copy(T, T + 3 * (size_t)NKF, o.T);
        if (o.R) std::copy(T + 3 * (size_t)NKF, T + 12 * (size_t)NKF, o.R);
    }
    return VG_OK;
}
