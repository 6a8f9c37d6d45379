// ba_carve.h — how the BA kernels cut their dynamic LDS and their HBM scratch into arrays: ONE definition per carve, read by
// the kernel that takes its pointers from it, by the host (ba_layout_fn.h: launch sizes, capacity decisions, refusals) and by
// the stand-alone checker tests/layout/ba_layout_check.cpp.  Plain structs and inline builders over uniform inputs; offsets in
// doubles unless a field says otherwise.  A region that several phases reuse is sized by the maximum of their named needs.
// Included at the end of ba_layout.h.
#pragma once

#ifdef __HIPCC__
#define BA_HD __host__ __device__ inline
#else
#define BA_HD inline
#endif
BA_HD int ba_up(int v, int m) { return (v + m - 1) / m * m; }
BA_HD int ba_max(int a, int b) { return a > b ? a : b; }
BA_HD int ba_min(int a, int b) { return a < b ? a : b; }

#define BA_CU_LDS (160 * 1024)        // bytes of LDS of a CU: the most a workgroup's dynamic and static group segments take together
#define BA_LDS_STATIC (8192 + 512)    // allowance for a kernel's static group segment (the per-round kernels report 8 KB: their non-inlined phases)
#define BA_LDS_MAX_LINACC (159 * 1024)   // hipFuncAttributeMaxDynamicSharedMemorySize of ba_linacc_proj_kernel
#define BA_LDS_MAX_LIN (128 * 1024)   // ... of ba_linearize_imu_kernel / ba_eval_factors_kernel; a prior's J0 is staged in LDS below this size

#define IMU_U 225                     // doubles of one IMU factor's 15x15 sqrt_info
#define IMU_PANEL 480                 // doubles of one IMU factor's weighted Jacobian panel [15][32]
#define PRO_WS 256                    // prologue: doubles of scratch per wavefront of imu_sqrt_info (15x15 factor) ...
#define PRO_WS_REF 512                // ... and of imu_sqrt_info_ref (LU / L [225] | inverse [225] | permutation [15])
#define MG_REC 42                     // doubles per projection record of the marginalization kernel
#define MG_PRV_PAD 480                // marginalization scratch: slack behind the prior residual / dx vectors
#define BA_NST(K, Kp) ba_up(7 * (Kp) + 9 * (K) + 8, 2)     // doubles of one state copy [pose Kp*7 | sb K*9 | ex 7 | td 1]

// ---- linearisation kernels (ba_linearize_imu_kernel, ba_eval_factors_kernel; imu_pass / prior_pass wherever they run)
struct LinLds { int U, panels, dx, part, end, need_imu, need_prior; };      // imu_pass: U [nb][IMU_U] | panels [nb][IMU_PANEL]; prior_pass: dx [Ncap] | part [4 Ncap]
BA_HD LinLds lin_lds(int nb, int Ncap) {
    LinLds c;
    c.U = 0; c.panels = ba_up(nb * IMU_U, 2);
    c.dx = 0; c.part = Ncap;
    c.need_imu = c.panels + nb * IMU_PANEL; c.need_prior = c.part + 4 * Ncap;
    c.end = ba_max(c.need_imu, c.need_prior);
    return c;
}

// ---- fused factor kernel (ba_linacc_proj_kernel)
#define LA_NT BA_NT               // (imu_pass / prior_pass are written for BA_NT threads)
#define LA_RS 33                  // doubles per staged record: rows at 0 and 16, odd stride (conflict-free b64 stores by thread)
#define LA_NPW 6                  // wavefronts that own pair blocks; the other two of the workgroup take the landmark sums
#define LA_MAXP 13                // pairs per pair wavefront: Kp (Kp - 1) / 2 <= 78 for Kp <= 13
#define LA_QCAP 80                // pairs a window can have (78 for Kp = 13), padded
#define LA_PAIR 90                // kept doubles of a pair block: ii 21 | jj 21 | ji 36 (row = target's column, col = anchor's) | gi 6 | gj 6
#define LA_NCH 64                 // entries of the chunk table: at most LA_NCH - 2 landmark chunks and the end marker
#define LA_MAXCHF 512             // staged records: one thread evaluates one factor of a chunk
static_assert(LA_QCAP <= 128, "the pair prefix of ba_linacc_proj_kernel takes two pairs per lane of one wavefront");
// records [chf][LA_RS] | pair blocks [npair][LA_PAIR] | ints: key [chf] lstart [LA_NCH] posx [chf] pstart [LA_QCAP + 2]
// wcnt [LA_NT / 64][LA_QCAP] | state [nst].  The prior and IMU passes run before anything is staged: their scratch is [0, x).
struct LinaccLds {
    int rec, P, key, x, end;
    int i_lstart, i_posx, i_pstart, i_wcnt, i_end;      // ints behind `key`
    int need_imu, need_prior;                           // imu_pass (LinLds) and prior_pass; prior_staged tests its own need against P
};
#define LA_FIXED_INTS (LA_NCH + LA_QCAP + 2 + LA_NT / 64 * LA_QCAP)
// the most records that leave the carve inside the CU: per factor a record, a key and a position (2 ints)
BA_HD int linacc_chf(int K, int Kp) {
    const int avail = (BA_CU_LDS - BA_LDS_STATIC) / 8, per = LA_RS + 1;
    const int chf = (avail - BA_NST(K, Kp) - Kp * (Kp - 1) / 2 * LA_PAIR - per - LA_FIXED_INTS / 2) / per;
    return ba_min(chf & ~1, LA_MAXCHF);
}

BA_HD LinaccLds linacc_lds(int K, int Kp, int chf, int Ncap) {
    LinaccLds c;
    c.rec = 0; c.P = ba_up(chf * LA_RS, 2);
    c.key = c.P + ba_up(Kp * (Kp - 1) / 2 * LA_PAIR, 2);
    c.i_lstart = chf; c.i_posx = c.i_lstart + LA_NCH; c.i_pstart = c.i_posx + chf; c.i_wcnt = c.i_pstart + LA_QCAP + 2;
    c.i_end = c.i_wcnt + LA_NT / 64 * LA_QCAP;
    c.x = ba_up(c.key + (c.i_end + 1) / 2 + 2, 2);
    c.end = c.x + BA_NST(K, Kp);
    const LinLds l = lin_lds(ba_min(K - 1, BA_IMU_BATCH), Ncap);
    c.need_imu = l.need_imu; c.need_prior = l.need_prior;
    return c;
}

// ---- prologue (ba_prologue_kernel): scratch per wavefront of the sqrt_info factorisation, or the prior's J0 [Ncap][Ncap] when it fits
struct ProLds { int wave, need_sqrt, need_J0, end; };
BA_HD ProLds pro_lds(int imu_info, int Ncap) {
    ProLds c;
    c.wave = imu_info ? PRO_WS_REF : PRO_WS;
    c.need_sqrt = BA_NW * c.wave;
    c.need_J0 = 8 * Ncap * Ncap <= BA_LDS_MAX_LIN ? Ncap * Ncap : 0;
    c.end = ba_max(c.need_sqrt, c.need_J0);
    return c;
}
// workgroups per window of the prologue: side by side (BaLayout::pro_split) the gauge, BA_NW IMU factors each, the prior's two pieces
BA_HD int pro_grid_y(int pro_split, int K) { return pro_split ? 1 + (K - 1 + BA_NW - 1) / BA_NW + 2 : 1; }

// ---- single-workgroup solve (ba_solve_kernel / ba_solve_w8_kernel): the carve itself travels in BaLayout::l_*.  The ring of
//      coupling rows [2][SV_RING_ROWS][ldc] is reused outside the chain: `stage` is its second slot, `wd` (the staged landmark
//      tile [RcPad][SCHUR_LD]) and the small scratch uses alias its start.  The 8-wavefront build keeps the tile behind the carve.
#define SV_RING_ROWS 18
#define SCHUR_LW 32                               // landmarks per staged tile
#define SCHUR_LD (SCHUR_LW + 1)
struct SolveRing { int size, stage, need_stage, need_tile, need_threads, need_small; };
BA_HD SolveRing solve_ring(int K, int RcPad, int ldc) {
    SolveRing c;
    c.size = 2 * SV_RING_ROWS * ldc; c.stage = SV_RING_ROWS * ldc; c.need_stage = c.stage + 2 * 9 * 18;
    c.need_tile = RcPad * SCHUR_LD; c.need_threads = 2 * SV_NT; c.need_small = ba_max(9 * K, 162);
    return c;
}

// ---- marginalization (ba_marg_kernel), LDS: eigM [ld][ld] | eigV [ld][ld] | cs | red [32] | state | int tables (MGI_*)
struct MargCs { int jacobi, generic, fast, vh_eig, amm, size; };      // the phases that use `cs`
BA_HD MargCs marg_cs(int mcap, int posmax, int Lcap) {
    MargCs c;
    c.jacobi = 2 * mcap;                                // rotation pairs
    c.generic = 3 * (posmax / 2 + 2);                   // generic sweep: one table of 3 * half doubles
    c.fast = 2 * (3 * ((mcap + 2) / 2) + 2) + 2;        // fast path: two of them (double-buffered)
    c.vh_eig = ba_up(5 * mcap + 8, 2);                  // vh_eig: running diagonal, norms, eigenvalues, flags
    c.amm = ba_up(Lcap + 512, 2);                       // Amm block elimination: landmark diagonal + 2 x 256
    c.size = ba_max(ba_up(ba_max(ba_max(c.jacobi, c.generic), c.fast), 2), ba_max(c.vh_eig, c.amm));
    return c;
}
struct MargLds { int eM, eV, cs, red, x, ints, end; };
BA_HD MargLds marg_lds(int K, int ld, int cs_size) {
    MargLds c;
    c.eM = 0; c.eV = ld * ld; c.cs = 2 * ld * ld;
    c.red = c.cs + cs_size; c.x = c.red + 32; c.ints = c.x + 16 * K + 8;      // state [pose K*7 | sb K*9 | ex 7 | td 1]
    c.end = c.ints + BA_MARG_LDS_INTS / 2 + 2;         // (+ 2: the launch has always asked for two doubles more than the kernel cuts)
    return c;
}
// ---- marginalization, HBM scratch per window (doubles; lm / l0 are int tables)
struct MargScratch { long A, bv, rec, T1, T2, gM, gV, g2M, g2V, prv, lm, l0, end; };
BA_HD MargScratch marg_scratch(int posmax, int Fcap, int mcap, int Ncap, int Lcap) {
    const long pm = posmax;
    MargScratch c;
    c.A = 0; c.bv = pm * pm;                            // posmax x posmax, rhs
    c.rec = c.bv + pm;                                  // [Fcap][MG_REC] projection records
    c.T1 = c.rec + (long)Fcap * MG_REC;                 // posmax x (mcap + 1), twice
    c.T2 = c.T1 + pm * (mcap + 1);
    c.gM = c.T2 + pm * (mcap + 1);                      // staging / eig fallback: posmax^2, twice
    c.gV = c.gM + pm * pm;
    c.g2M = c.gV + pm * pm;                             // second-eig fallback: mcap^2, twice
    c.g2V = c.g2M + (long)mcap * mcap;
    c.prv = c.g2V + (long)mcap * mcap;                  // prior residual [Ncap] + dx [Ncap]
    c.lm = c.prv + 2 * Ncap + MG_PRV_PAD;               // int [Lcap]: landmark -> column
    c.l0 = c.lm + Lcap / 2;                             // int [Lcap + ...]: the landmarks anchored at frame 0
    c.end = c.lm + Lcap + 64 + Lcap / 2 + 8;
    return c;
}
