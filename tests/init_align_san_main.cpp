// init_align_san_main.cpp — stand-alone driver of vg_init_align for a sanitizer build on the CPU (tests/test_init_align_simt.py builds it
// with -fsanitize=address,undefined together with the emulated kernels of csrc/imu_preint.hip and runs it; nothing is loaded into
// Python).  Every argument is a VAL1 file (tests/init_align_ref.write_replay); all of them go into ONE call, then each alone.  Prints
// one line per window: status, s, and a checksum of everything the call wrote.
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>
#include "../include/vinsgpu.h"

// Linked with vg_core, imu_preint and the emulator's runtime only: vg_destroy's hooks into the units that are left out (state this
// program never creates)
struct FeState;
extern "C" void fe_state_destroy(FeState*) {}
extern "C" void ba_graph_release(vg_handle*) {}
extern "C" void ba_seq_release(vg_handle*) {}

namespace {
struct Window {
    std::vector<double> R, T, samples, first, v_body, Ps, Rs, Vs;
    std::vector<int> off, key;
    std::vector<vg_imu_preint> records;
    vg_align_in in;
    vg_align_out out;
};
void rd(FILE* f, void* p, size_t bytes) { if (fread(p, 1, bytes, f) != bytes) throw std::runtime_error("file truncated"); }

void load(const char* path, Window& w) {
    FILE* f = fopen(path, "rb");
    if (!f) throw std::runtime_error(std::string("cannot open ") + path);
    int hdr[4];
    rd(f, hdr, sizeof(hdr));
    if (hdr[0] != 0x314C4156) throw std::runtime_error("not a VAL1 file");
    const int F = hdr[1], K = hdr[2];
    double head[24];                                        // ba0 3, bg0 3, noise 4, tic 3, ric 9, g_norm, init_depth
    rd(f, head, sizeof(head));
    w.R.resize(9 * F); w.T.resize(3 * F); w.off.assign(1, 0);
    for (int k = 0; k < F; ++k) {
        double fr[13];
        rd(f, fr, sizeof(fr));
        memcpy(&w.R[9 * k], fr + 1, 9 * sizeof(double));
        memcpy(&w.T[3 * k], fr + 10, 3 * sizeof(double));
    }
    for (int k = 1; k < F; ++k) {
        int n;
        double first[6];
        rd(f, &n, sizeof(n)); rd(f, first, sizeof(first));
        w.first.insert(w.first.end(), first, first + 6);
        const size_t at = w.samples.size();
        w.samples.resize(at + 7 * (size_t)n);
        rd(f, w.samples.data() + at, 7 * (size_t)n * sizeof(double));
        w.off.push_back((int)(w.samples.size() / 7));
    }
    w.key.resize(K);
    if (K) rd(f, w.key.data(), K * sizeof(int));
    fclose(f);
    w.v_body.assign(3 * F, 0.0); w.Ps.assign(3 * K, 0.0); w.Rs.assign(9 * K, 0.0); w.Vs.assign(3 * K, 0.0);
    w.records.resize(F - 1);
    memset(&w.in, 0, sizeof(w.in));
    w.in.struct_size = sizeof(w.in); w.in.n_frames = F;
    w.in.R = w.R.data(); w.in.T = w.T.data(); w.in.sample_off = w.off.data(); w.in.samples = w.samples.data(); w.in.first = w.first.data();
    memcpy(w.in.ba0, head, 3 * sizeof(double)); memcpy(w.in.bg0, head + 3, 3 * sizeof(double));
    memcpy(w.in.noise, head + 6, 4 * sizeof(double)); memcpy(w.in.tic, head + 10, 3 * sizeof(double));
    w.in.g_norm = head[22];
    w.in.n_key = K; w.in.key = K ? w.key.data() : nullptr;
    memset(&w.out, 0, sizeof(w.out));
    w.out.struct_size = sizeof(w.out);
    w.out.v_body = w.v_body.data(); w.out.records = w.records.data();
    if (K) { w.out.Ps = w.Ps.data(); w.out.Rs = w.Rs.data(); w.out.Vs = w.Vs.data(); }
}

double checksum(const Window& w) {
    double c = w.out.s + w.out.s_lin;
    for (int i = 0; i < 3; ++i) c += w.out.bg[i] + w.out.g_lin[i] + w.out.g_c0[i] + w.out.g_w[i];
    for (double v : w.v_body) c += v;
    for (double v : w.Ps) c += v;
    for (double v : w.Rs) c += v;
    for (double v : w.Vs) c += v;
    for (const vg_imu_preint& r : w.records) c += r.sum_dt + r.covariance[224] + r.jacobian[0];
    return c;
}
}  // namespace

int main(int argc, char** argv) {
    try {
        std::vector<Window> w(argc - 1);
        for (int i = 1; i < argc; ++i) load(argv[i], w[i - 1]);
        vg_handle* h = nullptr;
        if (vg_create(&h) != VG_OK) { fprintf(stderr, "vg_create failed\n"); return 3; }
        std::vector<vg_align_in> in;
        std::vector<vg_align_out> out;
        for (auto& x : w) { in.push_back(x.in); out.push_back(x.out); }
        if (vg_init_align(h, (int)in.size(), in.data(), out.data()) != VG_OK) { fprintf(stderr, "%s\n", vg_last_error(h)); return 1; }
        for (size_t i = 0; i < w.size(); ++i) {
            w[i].out = out[i];
            printf("batch %zu status %d s %.17g sum %.17g\n", i, out[i].status, out[i].s, checksum(w[i]));
        }
        for (size_t i = 0; i < w.size(); ++i) {
            if (vg_init_align(h, 1, &w[i].in, &w[i].out) != VG_OK) { fprintf(stderr, "%s\n", vg_last_error(h)); return 1; }
            printf("alone %zu status %d s %.17g sum %.17g\n", i, w[i].out.status, w[i].out.s, checksum(w[i]));
        }
        vg_destroy(h);
    } catch (const std::exception& e) { fprintf(stderr, "%s\n", e.what()); return 2; }
    return 0;
}
