// ba_layout_fn.h — the device layout of a batch of windows as a function of its shape alone: no handle, no HIP, no environment
// (host only; ba_host.hip's build_layout scans the problems and resolves the switches, tests/layout/ba_layout_check.cpp walks a
// grid of shapes through it).  Every LDS / scratch size comes from the carves of ba_carve.h.
#pragma once
#include <cstring>
#include "ba_layout.h"
#include "../../include/vinsgpu.h"

struct BaShape {
    int nwin, K;
    int relo;                      // the relocalisation pose block is part of the windows
    int e, t;                      // estimate_extrinsic / estimate_td
    int Lmax, Fmax, Omax, Nmax, NBmax;   // maxima over the windows (and the reservations): landmarks, factors, observations, prior rows / blocks
    int imu_info_mode, force_large;
    int fused_min;                 // resolved switches: windows from which ba_linacc_proj_kernel runs (1 << 30: never) ...
    int w8_below;                  // ... and below which ba_solve_w8_kernel does
};

// returns VG_OK, or a refusal and its text in *err
inline int ba_layout_from_shape(const BaShape& s, BaLayout& L, const char** err) {
#define BA_REFUSE(text) do { *err = text; return VG_ERR_UNSUPPORTED; } while (0)
    const auto up = ba_up;
    memset(&L, 0, sizeof(L));
    L.nwin = s.nwin;
    L.K = s.K;
    L.Kp = L.K + (s.relo ? 1 : 0);
    L.e = s.e ? 1 : 0;
    L.t = s.t ? 1 : 0;
    L.Rc = 6 * L.Kp + 6 * L.e + L.t;
    L.RcPad = up(L.Rc + 1, 16);                  // + the augmented rhs row / column
    L.R = L.Rc + 9 * L.K;
    L.Rpad = up(L.R + 1, 8);
    L.Lcap = up(s.Lmax, 16);
    L.Fcap = up(s.Fmax, 16);
    L.Ocap = up(s.Omax, 8);
    L.Ncap = up(ba_max(s.Nmax, 1), 8);
    L.NBcap = up(ba_max(s.NBmax, 1), 8);
    L.REC = 28 + 12 * L.e + 2 * L.t;
    L.nst = BA_NST(L.K, L.Kp);
    L.imu_info = s.imu_info_mode;
    // one workgroup solves a window out of LDS while the camera part fits its tiling; wider windows (and windows the
    // caller shards over ranks) take the large-window path
    L.big = (L.RcPad > 96 || L.Rc > 127 || L.K + 1 > BA_MAX_K || s.force_large) ? 1 : 0;
    if (L.big && L.Rc + 10 > 256) BA_REFUSE("camera part wider than the large-window solve kernel's tiling");
    // ---- workgroups per window
    L.nbf = (L.Fcap + BA_LIN_NT - 1) / BA_LIN_NT;
    // IMU / prior linearisation: spread over workgroups only while all of them fit the chip at once (latency mode)
    {
        const int nsplit = (L.K - 1 + BA_IMU_GROUP - 1) / BA_IMU_GROUP;
        const bool split = (long)s.nwin * (nsplit + 1) <= 256;
        L.igs = split ? BA_IMU_GROUP : L.K - 1;
        L.nig = split ? nsplit : 1;
        L.nprw = split ? 1 : 0;
        L.pro_split = split ? 1 : 0;                   // (ba_prologue_kernel: its pieces side by side, see the kernel)
    }
    L.nbl = L.nbf + L.nig + L.nprw;
    {
        const int nb = L.Kp + L.e + L.t;
        L.ntask = nb * (nb + 1) / 2;
        const int per = BA_ACC_NT / 64;
        const int ng = L.e + L.t, nglob = ng * (ng + 1) / 2;      // blocks among ex / td: they visit EVERY factor
        // diagonal pose blocks get a workgroup each, the ex / td blocks share one (if present), wavefront tasks after them
        L.nba = L.Kp + (ng ? 1 : 0) + (L.ntask - L.Kp - nglob + (L.Lcap + 63) / 64 + per - 1) / per;
    }
    // ---- LDS carve of the solve kernel (large-window path: only S, red and 1/L_jj are LDS offsets, the others are
    //      offsets into the HBM scratch at so_bigm)
    int bigm_doubles = 0;
    {
        // XC leading dimension: rows p and p+1 of an MFMA operand read must fall on different halves of the 64 banks
        int ldc = L.RcPad;
        if ((2 * ldc) % 64 != 32) ldc += 16;
        L.ldc = ldc;
        const SolveRing ring = solve_ring(L.K, L.RcPad, ldc);
        int o = 0, ob = 0;
        int& oo = L.big ? ob : o;                    // where the movable arrays are carved from
        L.l_S = o; o += up((L.Rc + 1) * (L.Rc + 2) / 2, 2);
        L.l_XC = 0; L.l_ring = 0; L.l_pinv = 0;
        if (L.big) { L.l_XC = oo; oo += up(9 * L.K, 8) * ldc; }    // (large path: two k-steps per trip of schur_chain_big)
        else {
            // single-workgroup path (round 5): the coupling rows are not held for the whole solve any more (100 rows x ldc = 64 KB of
            // the former 134 KB carve).  Two slots of 18 rows -- the block pair being eliminated and the pair before it -- are all the
            // chain elimination reads; finished rows are parked in HBM (so_xp) for the back substitution.  The staged landmark tile
            // of the Schur sweep (l_wd) and the small scratch uses of `wd` alias the ring: they are only live outside the chain.
            L.l_ring = o; o += ring.size;
        }
        L.l_D = oo; oo += up(81 * L.K, 2);
        L.l_E = oo; oo += up(81 * L.K, 2);
        L.l_dinv = oo; oo += up(9 * L.K, 2);
        L.l_vec = oo; oo += 9 * L.Rpad;
        L.l_red = o; o += 32;
        if (L.big) { L.l_wd = oo; oo += up(ring.need_small, 2); }
        else L.l_wd = L.l_ring;                                    // (SolveRing: the tile, SV_NT and the small scratch uses fit, below)
        L.l_z = oo; oo += up(36 * L.K, 2);
        if (L.big) { L.l_pmap = oo; oo += up(L.Ncap, 4) / 2; }
        else { L.l_pmap = 0; L.l_pinv = o; o += up(L.R, 4) / 2; }
        if (L.big) { L.l_di = o; o += up(L.Rc + 1, 2); L.l_cz = o; o += 6 * 96; }
        L.l_Sg = 0;
        if (L.big) { L.l_Sg = oo; oo += up((L.Rc + 1) * (L.Rc + 2) / 2, 2); }      // S between the halves of the reduced solve
        L.lds_solve = o * 8;
        bigm_doubles = ob;
        if (!L.big && L.Rc + 10 - 64 > 32) BA_REFUSE("solve kernel: more column tasks than three wavefronts");
        if (!L.big && ring.size < ba_max(ba_max(ring.need_tile, ring.need_threads), ring.need_small)) BA_REFUSE("solve kernel: scratch does not fit the coupling-row ring");
        if (L.lds_solve > BA_CU_LDS) BA_REFUSE("solve kernel LDS carve exceeds 160 KB");
        L.lds_lin = 8 * lin_lds(ba_min(ba_min(L.K - 1, BA_IMU_BATCH), L.igs), L.Ncap).end;
        L.lds_pro = 8 * pro_lds(L.imu_info, L.Ncap).end;
        if (L.lds_lin > BA_LDS_MAX_LIN) BA_REFUSE("prior too large for the linearisation kernel");
        // fused projection kernel (ba_linacc_proj_kernel, LinaccLds).  Few windows: the chip is empty and the separate kernels spread
        // a window over many workgroups (single window: 28 us per round against 52 us for the one fused workgroup); from a few dozen
        // windows on (fused_min) the fused kernel wins
        {
            const int chf = linacc_chf(L.K, L.Kp);
            const LinaccLds la = linacc_lds(L.K, L.Kp, chf, L.Ncap);
            L.la_on = (L.nwin >= s.fused_min && !L.big && !L.e && !L.t && L.Kp <= 13 && chf >= 96 && (L.Fcap + chf - 17) / (chf - 16) <= LA_NCH - 2) ? 1 : 0;
            L.la_chf = chf; L.la_chq = chf - 16;
            L.la_P = la.P; L.la_key = la.key; L.la_x = la.x;
            L.lds_linacc = la.end * 8;
        }
        // which build of the per-round solve kernel: 4 wavefronts per window (two windows per CU, the batch) or 8 (ba_solve_w8.hip: a
        // few windows on an otherwise empty chip).  Below 32 windows -- where the factor side is in its latency
        // mode as well -- the second window per CU does not exist and the wavefront slots go to the same window.
        // (the 8-wavefront build stages the landmark tile of its Schur phase behind the carve -- the ring it aliases in the 4-wavefront
        //  kernel is live beside it there; a shape that leaves no room keeps the 4-wavefront kernel)
        L.sv_w8 = (!L.big && L.nwin < s.w8_below) ? 1 : 0;
        L.l_wd8 = L.lds_solve / 8;
        L.lds_solve_w8 = L.lds_solve + 8 * ring.need_tile;
        if (L.lds_solve_w8 > BA_CU_LDS) L.sv_w8 = 0;
    }
    if (L.big) {
        const int nt = (L.Rc + 1 + 15) / 16;
        L.nts = nt * (nt + 1) / 2;
        const int ntri = L.Rc * (L.Rc + 1) / 2;
        L.rb1_T = up(ntri + L.Rc, 2);
        L.rb1_scal = L.rb1_T + up((L.Rc + 1) * (L.Rc + 2) / 2, 2);
        L.rb1_len = L.rb1_scal + RB1_NSCAL;
    }
    // ---- int arrays
    int o = 0;
    L.io_hdr = o; o += BA_HDR_INTS;
    L.io_lm_start = o; o += L.Lcap;
    L.io_lm_fbeg = o; o += L.Lcap + 8;
    L.io_fac_i = o; o += L.Fcap;
    L.io_fac_j = o; o += L.Fcap;
    L.io_fac_lm = o; o += L.Fcap;
    L.io_fac_oi = o; o += L.Fcap;
    L.io_fac_oj = o; o += L.Fcap;
    L.io_fac_slot = o; o += L.Fcap;
    L.io_pair_ptr = o; o += up(L.Kp * L.Kp + 1, 8);
    L.io_task_list = o; o += up(L.ntask, 8);
    L.io_imu_valid = o; o += up(L.K, 8);
    L.io_pb_kind = o; o += L.NBcap;
    L.io_pb_idx = o; o += L.NBcap;
    L.io_pb_col = o; o += L.NBcap;
    L.io_pb_off = o; o += L.NBcap;
    L.io_pb_x0off = o; o += L.NBcap;
    L.istride = up(o, 8);
    // ---- double inputs
    o = 0;
    L.do_pose = o; o += up(7 * L.Kp, 2);
    L.do_sb = o; o += up(9 * L.K, 2);
    L.do_ex = o; o += 8;
    L.do_td = o; o += 2;
    L.do_lam = o; o += L.Lcap;
    L.do_obs = o; o += L.Ocap * BA_OBS_STRIDE;
    L.do_imu = o; o += (L.K - 1) * BA_IMU_STRIDE;
    L.do_par = o; o += P_NPAR;
    L.dstride = up(o, 8);
    // ---- prior factor: a buffer of its own whose layout depends on K alone as long as the prior is one the marginalization
    //      can have produced (n <= 6K + 25, <= K + 4 blocks) -- so that a prior can stay where it is between frames
    L.pld = ba_max(up(6 * L.K + 9 * 2 + 6 + 1, 8), L.Ncap);
    L.po_x0 = 0;
    L.po_r0 = 9 * ba_max(up(L.K + 4, 8), L.NBcap);
    L.po_J0 = L.po_r0 + L.pld;
    L.pstride = up(L.po_J0 + L.pld * L.pld, 8);
    // ---- scratch
    o = 0;
    L.so_ctl = o; o += C_NCTL;
    L.so_part = o; o += up(L.nbl, 8);
    L.so_x = o; o += 2 * L.nst;
    L.so_lam = o; o += 2 * L.Lcap;
    L.so_imuU = o; o += up((L.K - 1) * IMU_U, 2);
    L.so_Hp = o; o += L.Ncap * L.Ncap;
    L.so_J0t = o; o += L.Ncap * L.Ncap;
    L.so_rec = o; o += L.Fcap * L.REC;
    L.so_sc = o; o += L.Rpad;
    L.so_sl = o; o += L.Lcap;
    L.so_dg = o; o += L.Rpad + L.Lcap;
    L.so_gt = o; o += L.Rpad + L.Lcap;
    L.so_gn = o; o += L.Rpad + L.Lcap;
    L.so_yl = o; o += L.Lcap;
    L.so_lsc = o; o += L.Lcap;
    L.so_xp = 0;
    if (!L.big) { L.so_xp = o; o += up(9 * L.K, 4) * L.ldc; }
    if (L.big) {
        L.so_bigm = o; o += up(bigm_doubles, 8);
        L.so_dgl = o; o += 2 * L.Lcap;
        L.so_gtl = o; o += 2 * L.Lcap;
    }
    {
        int b = 0;
        L.bo_Sp = b; b += up(L.Rc * (L.Rc + 1) / 2, 2);
        L.bo_gp = b; b += L.RcPad;
        L.bo_h = b; b += L.Lcap;
        L.bo_b = b; b += L.Lcap;
        L.bo_Wt = b; b += L.RcPad * L.Lcap;
        L.bo_imuJ = b; b += (L.K - 1) * 512;       // per factor: 465 lower Hessian entries + 30 gradient entries
        L.bo_pr = b; b += L.Ncap;
        L.bo_gpr = b; b += L.Ncap;
        L.buf_stride = up(b, 8);
    }
    L.so_buf = o; o += 2 * L.buf_stride;
    L.sstride = up(o, 8);
    // gather plan of assemble_small behind the device copy of this struct (build_asm_plan)
    L.pl_off = (int)((sizeof(BaLayout) + 255) / 256 * 256);
    L.pl_n = L.big ? 0 : L.Rc * (L.Rc + 1) / 2 + L.Rpad + 2 * 81 * L.K;
    // ---- outputs
    o = 0;
    L.oo_pose = o; o += up(7 * L.Kp, 2);
    L.oo_sb = o; o += up(9 * L.K, 2);
    L.oo_ex = o; o += 8;
    L.oo_td = o; o += 2;
    L.oo_lam = o; o += L.Lcap;
    L.oo_sum = o; o += BA_SUM_DOUBLES;
    L.oo_trace = o; o += 5 * VG_MAX_ITERS + 16;
    L.ostride = up(o, 8);
    L.oi_stride = up(4 + VG_MAX_ITERS, 8);
    // ---- marginalization: kept dimension <= 6K + 2*9 + 6 + 1; blocks <= K + 4.  Both paths: the kernel's LDS tables are
    //      sized for BA_MAX_K_LARGE frames; a kept block wider than the LDS tile is factored in global memory.
    L.mcap = up(6 * L.K + 9 * 2 + 6 + 1, 8);
    if (L.mcap > 256) BA_REFUSE("kept dimension of the marginalization beyond the kernel's tables");
    const int mcap = L.mcap;
    L.mo_J0 = 0;
    L.mo_r0 = mcap * mcap;
    L.mo_x0 = L.mo_r0 + mcap;
    L.mo_stride = up(L.mo_x0 + (L.K + 4) * 9, 8);
    L.mi_stride = up(8 + 2 * (L.K + 4) + 16, 8);   // + 16 phase stamps (BA_PROFILE builds)
    L.mg_posmax = up(mcap + 15 + L.Lcap, 2);
    {
        L.mg_cs = marg_cs(mcap, L.mg_posmax, L.Lcap).size;
        int ld = mcap + 1;                           // big enough for the kept part; also used for Amm when m <= ld.  ODD:
                                                     // the symmetric-storage Jacobi walks columns (stride ld doubles) and
                                                     // an even stride folds them onto a few LDS banks (96 -> one bank)
        while (marg_lds(L.K, ld, L.mg_cs).end > BA_CU_LDS / 8) ld -= 2;
        L.mg_ld = ld;
        L.mg_lds_bytes = marg_lds(L.K, ld, L.mg_cs).end * 8;
        if (ld < 8) BA_REFUSE("marginalization LDS carve failed");
        L.ms_stride = (int)up((int)marg_scratch(L.mg_posmax, L.Fcap, mcap, L.Ncap, L.Lcap).end, 8);
    }
    return VG_OK;
#undef BA_REFUSE
}
