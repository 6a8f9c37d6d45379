// TEST INFRASTRUCTURE: vg_ba_seq_outputs_* as a program of its own, for a sanitizer build with the EMULATED kernels (tests/test_seq_outputs_simt.py
// builds it with -fsanitize=address,undefined next to the kernel sources and tests/simt/simt_runtime.cpp; no Python in the process).
//
//   seq_outputs_san <case.bin>
// case.bin (tests/seq_outputs_case.write_san_case): ints magic 'SQO1', nwin, K, max_features, max_points; per window K x 7 pose, K x 9
// speed / bias, 7 extrinsic doubles, then the track table: int n, n ids, n start frames, n observation counts, n solve flags, n depths,
// sum(n_obs) x 8 rows [x y z u v vx vy cur_td].
// Runs vg_ba_seq_begin on the planted windows, vg_ba_seq_outputs_reserve(max_points), vg_ba_seq_outputs_async and vg_ba_seq_get_outputs
// of every window, and prints the message with the bit patterns of its floats; seq_outputs_case.san_lines prints the same from the binding.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../include/vinsgpu.h"

struct Window {
    std::vector<double> pose, sb, ex, depth, obs;
    std::vector<int> id, start, nobs, flag;
    std::vector<vg_imu_preint> imu;
    vg_ba_problem prob;
    vg_ba_tracks tracks;
};

template <class T> static bool rd(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}
static uint32_t bits(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }
static uint64_t bits(double v) { uint64_t u; memcpy(&u, &v, 8); return u; }

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: seq_outputs_san <case.bin>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    int hdr[5];
    if (!f || fread(hdr, sizeof(int), 5, f) != 5 || hdr[0] != 0x314F5153) { fprintf(stderr, "not an SQO1 file\n"); return 2; }
    const int nwin = hdr[1], K = hdr[2], FT = hdr[3], MP = hdr[4];
    std::vector<Window> win(nwin);
    for (Window& w : win) {
        int n = 0;
        if (!rd(f, w.pose, 7 * (size_t)K) || !rd(f, w.sb, 9 * (size_t)K) || !rd(f, w.ex, 7) || fread(&n, sizeof(int), 1, f) != 1 || n < 0) return 2;
        if (!rd(f, w.id, n) || !rd(f, w.start, n) || !rd(f, w.nobs, n) || !rd(f, w.flag, n) || !rd(f, w.depth, n)) return 2;
        size_t rows = 0;
        for (int v : w.nobs) rows += (size_t)v;
        if (!rd(f, w.obs, rows * 8)) return 2;
        w.imu.resize(K - 1);
        memset(w.imu.data(), 0, sizeof(vg_imu_preint) * w.imu.size());
        memset(&w.prob, 0, sizeof(w.prob));
        w.prob.K = K; w.prob.pose = w.pose.data(); w.prob.speedbias = w.sb.data(); w.prob.ex_pose = w.ex.data(); w.prob.imu = w.imu.data();
        w.prob.max_iters = 8; w.prob.focal = 460.0; w.prob.row = 480.0; w.prob.g_norm = 9.81;
        memset(&w.tracks, 0, sizeof(w.tracks));
        w.tracks.n_features = n; w.tracks.feature_id = w.id.data(); w.tracks.start_frame = w.start.data(); w.tracks.n_obs = w.nobs.data();
        w.tracks.solve_flag = w.flag.data(); w.tracks.depth = w.depth.data(); w.tracks.obs = w.obs.data();
    }
    fclose(f);
    vg_handle* h = nullptr;
    if (vg_create(&h) != VG_OK) { fprintf(stderr, "vg_create failed\n"); return 1; }
    std::vector<const vg_ba_problem*> pb;
    std::vector<const vg_ba_tracks*> tr;
    for (Window& w : win) { pb.push_back(&w.prob); tr.push_back(&w.tracks); }
    vg_ba_seq_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.max_features = FT; cfg.max_new_obs = 64; cfg.max_landmarks = 64; cfg.init_depth = 5.0; cfg.min_parallax = 10.0 / 460.0;
    int rc = vg_ba_seq_begin(h, nwin, &cfg, pb.data(), tr.data());
    if (rc == VG_OK) rc = vg_ba_seq_outputs_reserve(h, MP);
    if (rc == VG_OK) rc = vg_ba_seq_outputs_async(h);
    if (rc != VG_OK) { fprintf(stderr, "status %d: %s\n", rc, vg_last_error(h)); return 1; }
    // exactly max_points rows per array: a row too many written by the library is a heap overflow here
    std::vector<float> p3(3 * (size_t)MP), nm(2 * (size_t)MP), uv(2 * (size_t)MP), pc(3 * (size_t)MP), mg(3 * (size_t)MP);
    std::vector<int> id(MP);
    for (int w = 0; w < nwin; ++w) {
        vg_ba_seq_outputs o;
        memset(&o, 0, sizeof(o));
        o.struct_size = (int)sizeof(o);
        o.kf_point_3d = p3.data(); o.kf_norm = nm.data(); o.kf_uv = uv.data(); o.kf_id = id.data(); o.cloud_xyz = pc.data(); o.margin_xyz = mg.data();
        rc = vg_ba_seq_get_outputs(h, w, &o);
        if (rc != VG_OK) { fprintf(stderr, "status %d: %s\n", rc, vg_last_error(h)); return 1; }
        printf("W %d %d %d %d %d %d\n", w, o.status, o.keyframe_valid, o.n_keyframe, o.n_cloud, o.n_margin);
        printf("pose");
        for (int k = 0; k < 7; ++k) printf(" %016" PRIx64, bits(o.pose[k]));
        for (int k = 0; k < 7; ++k) printf(" %016" PRIx64, bits(o.ex_pose[k]));
        printf("\n");
        const int nk = o.n_keyframe < MP ? o.n_keyframe : MP, nc = o.n_cloud < MP ? o.n_cloud : MP, nmg = o.n_margin < MP ? o.n_margin : MP;
        for (int k = 0; k < nk; ++k)
            printf("k %d %08x %08x %08x %08x %08x %08x %08x\n", id[k], bits(p3[3 * k]), bits(p3[3 * k + 1]), bits(p3[3 * k + 2]), bits(nm[2 * k]), bits(nm[2 * k + 1]),
                   bits(uv[2 * k]), bits(uv[2 * k + 1]));
        for (int k = 0; k < nc; ++k) printf("c %08x %08x %08x\n", bits(pc[3 * k]), bits(pc[3 * k + 1]), bits(pc[3 * k + 2]));
        for (int k = 0; k < nmg; ++k) printf("m %08x %08x %08x\n", bits(mg[3 * k]), bits(mg[3 * k + 1]), bits(mg[3 * k + 2]));
    }
    // with only the scalars asked for, and once more after a second reservation that is smaller than every list
    vg_ba_seq_outputs o;
    memset(&o, 0, sizeof(o));
    o.struct_size = (int)sizeof(o);
    rc = vg_ba_seq_get_outputs(h, 0, &o);
    if (rc == VG_OK) rc = vg_ba_seq_outputs_reserve(h, 1);
    if (rc == VG_OK) rc = vg_ba_seq_outputs_async(h);
    o.kf_point_3d = p3.data(); o.kf_id = id.data(); o.cloud_xyz = pc.data();
    for (int w = 0; w < nwin && rc == VG_OK; ++w) {
        rc = vg_ba_seq_get_outputs(h, w, &o);
        printf("S %d %d %d %d %d\n", w, o.status, o.n_keyframe, o.n_cloud, o.n_margin);
    }
    if (rc != VG_OK) { fprintf(stderr, "status %d: %s\n", rc, vg_last_error(h)); return 1; }
    vg_ba_seq_end(h);
    vg_destroy(h);
    return 0;
}
