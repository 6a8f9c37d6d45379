// init_align_carve.h — how init_align_kernel (csrc/imu_preint.hip, csrc/init_align.h) cuts its dynamic LDS: ONE definition, read by
// the kernel, by the host that sizes the launch (vg_init_align) and by the stand-alone checker tests/init_align_carve_check.cpp.
// Plain structs over uniform inputs, offsets in doubles, in the manner of ba_carve.h.
//   acc   the normal matrix A as the reference accumulates it, packed lower triangle (row i at i (i + 1) / 2); RefineGravity keeps it
//         across its four passes, so the factorisation works on a copy:
//   fac   packed lower triangle: the copy, then L below the diagonal and D on it
//   b     the right-hand side (accumulated like A) | x  the copy the solve runs in (the solution) | col  one scaled column of the factor
//   pr    per pair: sum_dt, delta_p, delta_v of the re-propagated record (AL_PR doubles)
//   tA    tmp_A [6][AL_TC] and tmp_b [6] of the pair being added
#pragma once

#ifdef __HIPCC__
#define AL_HD __host__ __device__ inline
#else
#define AL_HD inline
#endif

#define AL_MAX_FRAMES 32              // VG_ALIGN_MAX_FRAMES
#define AL_MIN_FRAMES_SOLVE 4         // 6 (F - 1) rows for 3 F + 4 unknowns: below this the linear system is singular by count
#define AL_PR 8                       // sum_dt | delta_p 3 | delta_v 3 | pad
#define AL_TC 10                      // columns of tmp_A (LinearAlignment: 10; RefineGravity uses 9 of them)
#define AL_CU_LDS (160 * 1024)        // bytes of LDS of a CU
#define AL_N_LIN(F) (3 * (F) + 4)     // unknowns of LinearAlignment; RefineGravity has one fewer
#define AL_TRI(n) ((n) * ((n) + 1) / 2)

struct AlignLds { int acc, fac, b, x, col, pr, tA, end; };
AL_HD AlignLds align_lds(int F) {
    const int n = AL_N_LIN(F), tri = (AL_TRI(n) + 1) & ~1, nv = (n + 1) & ~1;
    AlignLds c;
    c.acc = 0; c.fac = c.acc + tri;
    c.b = c.fac + tri; c.x = c.b + nv; c.col = c.x + nv;
    c.pr = c.col + nv; c.tA = c.pr + AL_PR * (F - 1);
    c.end = c.tA + 6 * AL_TC + 6;
    return c;
}
