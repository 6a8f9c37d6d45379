// kf_pgo_san_main.cpp — stand-alone driver of vg_pg_optimize for a sanitizer build on the CPU (tests/test_kf_pgo_simt.py builds it with
// -fsanitize=address,undefined together with the emulated kernels of csrc/fe_ransac.hip and runs it; nothing is loaded into Python).
// Every argument is a graph file (tests/kf_pgo_ref.write_file).  All files go through one batched call, then each alone; one line per
// graph and call: batch|alone, status, termination, iterations, n_edges, n_loop_edges, n_free, final_cost and yaw_drift (hex floats) and a
// checksum of everything written.
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
void rd(FILE* f, void* p, size_t bytes) { if (bytes && fread(p, 1, bytes, f) != bytes) throw std::runtime_error("file truncated"); }
unsigned long long fnv(unsigned long long h, const void* p, size_t bytes) {
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i < bytes; ++i) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}
struct Graph {
    vg_pg_in in;
    std::vector<int> index, sequence, has_loop, loop_index;
    std::vector<double> T, R, info;
};
struct Out {
    vg_pg_out o;
    std::vector<double> T, R;
    explicit Out(int n) : T(3 * (size_t)n), R(9 * (size_t)n) {              // exactly n_kf rows each: an overrun is a report
        std::memset(&o, 0, sizeof(o));
        o.struct_size = sizeof(o); o.T = T.data(); o.R = R.data();
    }
};
void load(const char* path, Graph& g) {
    FILE* f = fopen(path, "rb");
    if (!f) throw std::runtime_error(std::string("cannot open ") + path);
    int hdr[4];
    double delta;
    rd(f, hdr, sizeof(hdr)); rd(f, &delta, sizeof(delta));
    const size_t n = (size_t)hdr[0];
    g.index.resize(n); g.sequence.resize(n); g.has_loop.resize(n); g.loop_index.resize(n); g.T.resize(3 * n); g.R.resize(9 * n); g.info.resize(8 * n);
    rd(f, g.index.data(), 4 * n); rd(f, g.sequence.data(), 4 * n); rd(f, g.has_loop.data(), 4 * n); rd(f, g.loop_index.data(), 4 * n);
    rd(f, g.T.data(), 24 * n); rd(f, g.R.data(), 72 * n); rd(f, g.info.data(), 64 * n);
    fclose(f);
    vg_pg_defaults(&g.in);
    g.in.n_kf = hdr[0]; g.in.n_opt = hdr[1]; g.in.first_looped_index = hdr[2]; g.in.max_iters = hdr[3]; g.in.huber_delta = delta;
    g.in.index = g.index.data(); g.in.sequence = g.sequence.data(); g.in.has_loop = g.has_loop.data(); g.in.loop_index = g.loop_index.data();
    g.in.vio_T = g.T.data(); g.in.vio_R = g.R.data(); g.in.loop_info = g.info.data();
}
void line(const char* tag, const Out& r) {
    const vg_pg_out& o = r.o;
    unsigned long long s = 1469598103934665603ull;
    s = fnv(s, &o.initial_cost, sizeof(double) * (2 + 13 + 4 * VG_PG_MAX_ITERS));      // initial_cost .. it_model: contiguous doubles
    s = fnv(s, o.it_flags, sizeof(int) * 2 * VG_PG_MAX_ITERS);
    s = fnv(s, r.T.data(), 8 * r.T.size()); s = fnv(s, r.R.data(), 8 * r.R.size());
    std::printf("%s %d %d %d %d %d %d %a %a %016llx\n", tag, o.status, o.termination, o.iterations, o.n_edges, o.n_loop_edges, o.n_free, o.final_cost,
                o.yaw_drift, s);
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s graph.bin ...\n", argv[0]); return 2; }
    try {
        vg_handle* h = nullptr;
        if (vg_create(&h) != VG_OK) throw std::runtime_error("vg_create failed");
        const int n = argc - 1;
        std::vector<Graph> gs(n);
        for (int i = 0; i < n; ++i) load(argv[i + 1], gs[i]);
        std::vector<vg_pg_in> ins;
        std::vector<Out> outs;
        std::vector<vg_pg_out> os;
        for (int i = 0; i < n; ++i) { ins.push_back(gs[i].in); outs.emplace_back(gs[i].in.n_kf); }
        for (int i = 0; i < n; ++i) os.push_back(outs[i].o);
        if (vg_pg_optimize(h, n, ins.data(), os.data()) != VG_OK) throw std::runtime_error(vg_last_error(h));
        for (int i = 0; i < n; ++i) { outs[i].o = os[i]; line("batch", outs[i]); }
        for (int i = 0; i < n; ++i) {
            Out one(gs[i].in.n_kf);
            if (vg_pg_optimize(h, 1, &gs[i].in, &one.o) != VG_OK) throw std::runtime_error(vg_last_error(h));
            line("alone", one);
        }
        vg_destroy(h);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "kf_pgo_san_main: %s\n", e.what());
        return 1;
    }
    return 0;
}
