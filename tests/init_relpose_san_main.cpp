// init_relpose_san_main.cpp — stand-alone driver of vg_init_relpose for a sanitizer build on the CPU (tests/test_init_relpose_simt.py builds
// it with -fsanitize=address,undefined together with the emulated kernels of csrc/fe_ransac.hip and runs it; nothing is loaded into
// Python).  Every argument is a VRP1 file (tests/init_relpose_ref.write_file); all of them go into ONE call, then each alone.  Prints one
// line per window: F, status, l, and a checksum of everything the call wrote.
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>
#include "../include/vinsgpu.h"

// Linked with vg_core, fe_ransac and the emulator's runtime only: vg_destroy's hooks into the units that are left out (state this
// program never creates)
struct FeState;
extern "C" void fe_state_destroy(FeState*) {}
extern "C" void ba_graph_release(vg_handle*) {}
extern "C" void ba_seq_release(vg_handle*) {}

namespace {
struct Window {
    std::vector<int> start, nobs, off, n_corres, gate, it, bound, nin, best, good, winner, cnt, fb;
    std::vector<double> points, avg, F;
    std::vector<unsigned char> mask, rmask;
    vg_relpose_in in;
    vg_relpose_out out;
};
void rd(FILE* f, void* p, size_t bytes) { if (bytes && fread(p, 1, bytes, f) != bytes) throw std::runtime_error("file truncated"); }

void load(const char* path, Window& w) {
    FILE* f = fopen(path, "rb");
    if (!f) throw std::runtime_error(std::string("cannot open ") + path);
    int hdr[4];                                             // magic, F, n_feat, rows of points
    rd(f, hdr, sizeof(hdr));
    if (hdr[0] != 0x31505256) throw std::runtime_error("not a VRP1 file");
    const int F = hdr[1], n = hdr[2], rows = hdr[3], C = F - 1;
    w.start.resize(n); w.nobs.resize(n); w.off.resize(n); w.points.resize(3 * (size_t)rows);
    rd(f, w.start.data(), sizeof(int) * n); rd(f, w.nobs.data(), sizeof(int) * n); rd(f, w.off.data(), sizeof(int) * n);
    rd(f, w.points.data(), sizeof(double) * 3 * rows);
    fclose(f);
    std::memset(&w.in, 0, sizeof(w.in));
    std::memset(&w.out, 0, sizeof(w.out));
    w.in.struct_size = sizeof(w.in); w.in.n_frames = F; w.in.n_feat = n;
    w.in.start = w.start.data(); w.in.nobs = w.nobs.data(); w.in.obs_off = w.off.data(); w.in.points = w.points.data();
    w.in.ransac_threshold = 0.3 / 460; w.in.confidence = 0.99; w.in.min_corres = 20; w.in.min_inliers = 12;
    w.in.parallax_gate = 30; w.in.focal = 460; w.in.cheirality_dist = 50;
    for (auto* v : {&w.n_corres, &w.gate, &w.it, &w.bound, &w.nin, &w.best, &w.winner, &w.cnt, &w.fb}) v->assign(C, 0);
    w.good.assign(4 * C, 0); w.avg.assign(C, 0.0); w.F.assign(9 * C, 0.0); w.mask.assign(n, 0); w.rmask.assign(n, 0);
    w.out.struct_size = sizeof(w.out);
    w.out.mask = w.mask.data(); w.out.ransac_mask = w.rmask.data(); w.out.n_corres = w.n_corres.data(); w.out.avg_parallax = w.avg.data();
    w.out.gate = w.gate.data(); w.out.ransac_iter = w.it.data(); w.out.ransac_bound = w.bound.data(); w.out.ransac_inliers = w.nin.data();
    w.out.ransac_best = w.best.data();
    w.out.F = w.F.data(); w.out.good = w.good.data(); w.out.winner = w.winner.data(); w.out.inlier_cnt = w.cnt.data();
    w.out.used_fallback = w.fb.data();
}

unsigned long long sum_bits(const void* p, size_t bytes, unsigned long long h) {
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i < bytes; ++i) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}
void print(const char* tag, const Window& w) {
    unsigned long long h = 1469598103934665603ull;
    for (const auto* v : {&w.avg, &w.F}) h = sum_bits(v->data(), v->size() * sizeof(double), h);
    for (const auto* v : {&w.n_corres, &w.gate, &w.it, &w.bound, &w.nin, &w.best, &w.good, &w.winner, &w.cnt, &w.fb}) h = sum_bits(v->data(), v->size() * sizeof(int), h);
    for (const auto* v : {&w.mask, &w.rmask}) h = sum_bits(v->data(), v->size(), h);
    h = sum_bits(w.out.relative_R, sizeof(w.out.relative_R), h); h = sum_bits(w.out.relative_T, sizeof(w.out.relative_T), h);
    std::printf("%s %d %d %d %d %016llx\n", tag, w.in.n_frames, w.out.status, w.out.l, w.out.n_mask, h);
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s window.bin ...\n", argv[0]); return 2; }
    try {
        const int n = argc - 1;
        std::vector<Window> wins(n);
        for (int i = 0; i < n; ++i) load(argv[1 + i], wins[i]);
        vg_handle* h = nullptr;
        if (vg_create(&h) != VG_OK) throw std::runtime_error("vg_create failed");
        std::vector<vg_relpose_in> ins(n);
        std::vector<vg_relpose_out> outs(n);
        for (int i = 0; i < n; ++i) { ins[i] = wins[i].in; outs[i] = wins[i].out; }
        if (vg_init_relpose(h, n, ins.data(), outs.data()) != VG_OK) throw std::runtime_error(vg_last_error(h));
        for (int i = 0; i < n; ++i) { wins[i].out = outs[i]; print("batch", wins[i]); }
        for (int i = 0; i < n; ++i) {
            if (vg_init_relpose(h, 1, &wins[i].in, &wins[i].out) != VG_OK) throw std::runtime_error(vg_last_error(h));
            print("alone", wins[i]);
        }
        vg_destroy(h);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "init_relpose_san_main: %s\n", e.what());
        return 1;
    }
    return 0;
}
