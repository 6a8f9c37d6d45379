// init_sfm_carve.h — how init_sfm_kernel (csrc/triangulate.hip, csrc/init_sfm.h) cuts its dynamic LDS: ONE definition, read by the
// kernel, by the host that sizes the launch (vg_init_sfm) and by the stand-alone checker tests/init_sfm_carve_check.cpp.  Plain
// structs over uniform inputs, offsets in doubles, in the manner of init_align_carve.h.  F frames, n features, NC = 6 F - 9 free camera
// unknowns (the rotation of l and the translations of l and F - 1 are constant).
//   red    partial sums of the workgroup reductions: [SFM_NW][SFM_NRED] and the totals [SFM_NRED]
//   cq ct  c_Quat (w x y z) / c_Translation per frame
//   sc     Jacobi scale of the 6 F camera columns
//   gc     the camera gradient (scaled) until the right-hand side is built, then the camera step (unscaled): dcam
//   S      the reduced camera system, packed lower triangle (row i at i (i + 1) / 2), then its Cholesky factor in place; during
//          construct, before any system exists, the rotation matrices of the chain: cR
//   rhs    right-hand side, then the solution
//   col    one scaled column of the factor; after the solve the candidate of the step: cq2, ct2
//   pos    positions | vinv the symmetric (V_j + D^2)^-1, 6 per feature | gp the point gradient (scaled), then the point step
//   sp     Jacobi scale of the point columns
//   stage  `ch` features at a time: the coupling blocks W_jf [6][3] and Y_jf = W_jf (V_j + D^2)^-1 of every frame of the feature's
//          span, from which every thread takes the products of its own entries of S
// state[] stays in the output block in HBM: feature j is always handled by thread j mod SFM_NT.
// The per-feature part is 15 n doubles: n = 1024 takes 120 KB of the 160 KB, the camera part at F = 16 another 36 KB, which leaves room
// for ONE staged feature (ch = 1, 4.5 KB); the usual window (F = 11, 150 features) has 31 KB of fixed parts and stages 9 features at
// once inside 64 KB.  VG_SFM_MAX_FEATURES is therefore 1024.
#pragma once

#ifdef __HIPCC__
#define SFM_HD __host__ __device__ inline
#else
#define SFM_HD inline
#endif

#define SFM_MAX_FRAMES 16             // VG_SFM_MAX_FRAMES
#define SFM_MIN_FRAMES 3
#define SFM_MAX_FEATURES 1024         // VG_SFM_MAX_FEATURES
#define SFM_MAX_ITERS 50              // VG_SFM_MAX_ITERS
#define SFM_NT 256                    // threads of a workgroup
#define SFM_NW (SFM_NT / 64)          // wavefronts
#define SFM_NRED 28                   // the widest reduction: 21 + 6 + 1 sums of a PnP iteration
#define SFM_MAX_STAGE 32              // features staged at once, at most
#define SFM_CU_LDS (160 * 1024)       // bytes of LDS of a CU
#define SFM_SMALL_LDS (64 * 1024)     // what a window takes when its fixed parts leave room for SFM_MIN_STAGE staged features below this
#define SFM_MIN_STAGE 8
#define SFM_NC(F) (6 * (F) - 9)
#define SFM_TRI(n) ((n) * ((n) + 1) / 2)
#define SFM_STAGE_PER(F) (36 * (F))   // doubles of one staged feature: W and Y, 18 per frame each

struct SfmLds { int red, cq, ct, sc, gc, dcam, S, cR, rhs, col, cq2, ct2, pos, vinv, gp, sp, stage, ch, end; };
SFM_HD SfmLds sfm_lds(int F, int n) {
    const int nc = SFM_NC(F), ev = (n + 1) & ~1, c7 = 7 * F + 2 > nc + 1 ? 7 * F + 2 : nc + 1;
    SfmLds c;
    c.red = 0;
    c.cq = c.red + (SFM_NW + 1) * SFM_NRED; c.ct = c.cq + 4 * F; c.sc = c.ct + 3 * F + (F & 1);
    c.gc = c.sc + 6 * F; c.dcam = c.gc;
    c.S = c.gc + 6 * F; c.cR = c.S;
    c.rhs = c.S + ((SFM_TRI(nc) + 1) & ~1); c.col = c.rhs + nc + 1;
    c.cq2 = c.col; c.ct2 = c.cq2 + 4 * F;
    c.pos = c.col + c7 + (c7 & 1);
    c.vinv = c.pos + 3 * ev; c.gp = c.vinv + 6 * ev; c.sp = c.gp + 3 * ev;
    c.stage = c.sp + 3 * ev;
    const int per = SFM_STAGE_PER(F);
    int ch = (SFM_SMALL_LDS / 8 - c.stage) / per;         // inside 64 KB when that stages SFM_MIN_STAGE features or more, else what the CU has
    if (ch < SFM_MIN_STAGE) ch = (SFM_CU_LDS / 8 - c.stage) / per;
    ch = ch > SFM_MAX_STAGE ? SFM_MAX_STAGE : ch;
    c.ch = ch;                        // < 1: the window does not fit (the carve check shows it never happens within the capacities)
    c.end = c.stage + (ch > 0 ? ch : 1) * per;
    return c;
}
