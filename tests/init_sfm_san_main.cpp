// init_sfm_san_main.cpp — stand-alone driver of vg_init_sfm for a sanitizer build on the CPU (tests/test_init_sfm_simt.py builds it with
// -fsanitize=address,undefined together with the emulated kernels of csrc/triangulate.hip and runs it; nothing is loaded into Python).
// Every argument is a VSF1 file (tests/init_sfm_ref.write_file); all of them go into ONE call, then each alone.  Prints one line per
// window: status, BA iterations, final cost, and a checksum of everything the call wrote.
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>
#include "../include/vinsgpu.h"

// Linked with vg_core, triangulate and the emulator's runtime only: vg_destroy's hooks into the units that are left out (state this
// program never creates)
struct FeState;
extern "C" void fe_state_destroy(FeState*) {}
extern "C" void ba_graph_release(vg_handle*) {}
extern "C" void ba_seq_release(vg_handle*) {}

namespace {
struct Window {
    std::vector<int> fid, start, nobs, off, all_key, all_guess, all_off, all_id, state, is_key, pnp_iters, pnp_up;
    std::vector<double> points, all_xy, q, T, position, R_all, T_all, q0, T0, position0;
    vg_sfm_in in;
    vg_sfm_out out;
};
void rd(FILE* f, void* p, size_t bytes) { if (bytes && fread(p, 1, bytes, f) != bytes) throw std::runtime_error("file truncated"); }

void load(const char* path, Window& w) {
    FILE* f = fopen(path, "rb");
    if (!f) throw std::runtime_error(std::string("cannot open ") + path);
    int hdr[7];                                             // magic, F, l, n_feat, rows of points, n_all, rows of all_xy
    rd(f, hdr, sizeof(hdr));
    if (hdr[0] != 0x31465356) throw std::runtime_error("not a VSF1 file");
    const int F = hdr[1], n = hdr[3], no = hdr[4], na = hdr[5], np = hdr[6];
    std::memset(&w.in, 0, sizeof(w.in));
    std::memset(&w.out, 0, sizeof(w.out));
    rd(f, w.in.relative_R, sizeof(double) * 9); rd(f, w.in.relative_T, sizeof(double) * 3); rd(f, w.in.ric, sizeof(double) * 9);
    w.fid.resize(n); w.start.resize(n); w.nobs.resize(n); w.off.resize(n); w.points.resize(3 * (size_t)no);
    rd(f, w.fid.data(), sizeof(int) * n); rd(f, w.start.data(), sizeof(int) * n); rd(f, w.nobs.data(), sizeof(int) * n); rd(f, w.off.data(), sizeof(int) * n);
    rd(f, w.points.data(), sizeof(double) * 3 * no);
    w.all_key.resize(na + 1); w.all_guess.resize(na + 1); w.all_off.resize(na + 1); w.all_id.resize(np + 1); w.all_xy.resize(2 * (size_t)np + 2);
    rd(f, w.all_key.data(), sizeof(int) * na); rd(f, w.all_guess.data(), sizeof(int) * na); rd(f, w.all_off.data(), sizeof(int) * (na + 1));
    rd(f, w.all_id.data(), sizeof(int) * np); rd(f, w.all_xy.data(), sizeof(double) * 2 * np);
    fclose(f);
    w.in.struct_size = sizeof(w.in); w.in.n_frames = F; w.in.l = hdr[2]; w.in.n_feat = n; w.in.n_all = na;
    w.in.feature_id = w.fid.data(); w.in.start = w.start.data(); w.in.nobs = w.nobs.data(); w.in.obs_off = w.off.data(); w.in.points = w.points.data();
    w.in.all_key = w.all_key.data(); w.in.all_guess = w.all_guess.data(); w.in.all_off = w.all_off.data(); w.in.all_id = w.all_id.data();
    w.in.all_xy = w.all_xy.data();
    w.q.resize(4 * F); w.T.resize(3 * F); w.q0.resize(4 * F); w.T0.resize(3 * F); w.pnp_iters.resize(F); w.pnp_up.resize(F);
    w.state.resize(n); w.position.resize(3 * n); w.position0.resize(3 * n);
    w.R_all.resize(9 * na + 1); w.T_all.resize(3 * na + 1); w.is_key.resize(na + 1);
    w.out.struct_size = sizeof(w.out);
    w.out.q = w.q.data(); w.out.T = w.T.data(); w.out.q0 = w.q0.data(); w.out.T0 = w.T0.data(); w.out.pnp_iters = w.pnp_iters.data();
    w.out.pnp_up = w.pnp_up.data(); w.out.state = w.state.data(); w.out.position = w.position.data(); w.out.position0 = w.position0.data();
    w.out.R_all = w.R_all.data(); w.out.T_all = w.T_all.data(); w.out.is_key = w.is_key.data();
}

unsigned long long sum_bits(const void* p, size_t bytes, unsigned long long h) {
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i < bytes; ++i) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}
void print(const char* tag, const Window& w) {
    unsigned long long h = 1469598103934665603ull;
    for (const auto* v : {&w.q, &w.T, &w.position, &w.R_all, &w.T_all, &w.q0, &w.T0, &w.position0}) h = sum_bits(v->data(), v->size() * sizeof(double), h);
    for (const auto* v : {&w.state, &w.is_key, &w.pnp_iters, &w.pnp_up}) h = sum_bits(v->data(), v->size() * sizeof(int), h);
    h = sum_bits(w.out.it_cost, sizeof(w.out.it_cost), h); h = sum_bits(w.out.it_cost_cand, sizeof(w.out.it_cost_cand), h);
    h = sum_bits(w.out.it_flags, sizeof(w.out.it_flags), h);
    std::printf("%s %d %d %d %.17g %016llx\n", tag, w.in.n_frames, w.out.status, w.out.ba_iters, w.out.final_cost, h);
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
        std::vector<vg_sfm_in> ins(n);
        std::vector<vg_sfm_out> outs(n);
        for (int i = 0; i < n; ++i) { ins[i] = wins[i].in; outs[i] = wins[i].out; }
        if (vg_init_sfm(h, n, ins.data(), outs.data()) != VG_OK) throw std::runtime_error(vg_last_error(h));
        for (int i = 0; i < n; ++i) { wins[i].out = outs[i]; print("batch", wins[i]); }
        for (int i = 0; i < n; ++i) {
            if (vg_init_sfm(h, 1, &wins[i].in, &wins[i].out) != VG_OK) throw std::runtime_error(vg_last_error(h));
            print("alone", wins[i]);
        }
        vg_destroy(h);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "init_sfm_san_main: %s\n", e.what());
        return 1;
    }
    return 0;
}
