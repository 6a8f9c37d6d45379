// kf_pnp_san_main.cpp — stand-alone driver of vg_kf_pnp for a sanitizer build on the CPU (tests/test_kf_pnp_simt.py builds it with
// -fsanitize=address,undefined together with the emulated kernels of csrc/fe_ransac.hip and runs it; nothing is loaded into Python).
// Every argument is a KPN1 file (tests/kf_pnp_ref.write_file).  All files go through one batched call, then each alone; one line per
// pair and call: batch|alone, status, n_inliers, ransac_best, ransac_iter, ransac_bound, has_loop and a checksum of everything written.
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
struct Pair {
    vg_kf_pnp_in in;
    std::vector<float> p3, p2;
    std::vector<int> ids;
};
struct Out {
    vg_kf_pnp_out o;
    std::vector<unsigned char> mask;
    std::vector<int> mi, id;
    std::vector<double> xy;
    explicit Out(int n) : mask(n), mi(n), id(n), xy(2 * (size_t)n) {        // exactly n entries each: an overrun is a report
        std::memset(&o, 0, sizeof(o));
        o.struct_size = sizeof(o); o.mask = mask.data(); o.matched_index = mi.data(); o.match_id = id.data(); o.match_xy = xy.data();
    }
};
void load(const char* path, Pair& p) {
    FILE* f = fopen(path, "rb");
    if (!f) throw std::runtime_error(std::string("cannot open ") + path);
    int hdr[5];
    double d[27];
    rd(f, hdr, sizeof(hdr)); rd(f, d, sizeof(d));
    if (hdr[0] != 0x314E504B) throw std::runtime_error("not a KPN1 file");
    const int n = hdr[1];
    p.p3.resize(3 * (size_t)n); p.p2.resize(2 * (size_t)n); p.ids.resize(n);
    rd(f, p.p3.data(), 4 * p.p3.size()); rd(f, p.p2.data(), 4 * p.p2.size()); rd(f, p.ids.data(), 4 * p.ids.size());
    fclose(f);
    vg_kf_pnp_defaults(&p.in);
    p.in.n = n; p.in.min_loop_num = hdr[2]; p.in.max_iters = hdr[3]; p.in.refine = hdr[4];
    p.in.reproj_threshold = d[0]; p.in.max_yaw_deg = d[1]; p.in.max_dist = d[2];
    std::memcpy(p.in.origin_vio_T, d + 3, 24); std::memcpy(p.in.origin_vio_R, d + 6, 72); std::memcpy(p.in.tic, d + 15, 24); std::memcpy(p.in.qic, d + 18, 72);
    p.in.point_3d = p.p3.data(); p.in.old_norm = p.p2.data(); p.in.point_id = p.ids.data();
}
void line(const char* tag, const Out& r) {
    const vg_kf_pnp_out& o = r.o;
    unsigned long long s = 1469598103934665603ull;
    s = fnv(s, o.sample_rvec, sizeof(double) * 32);           // sample_rvec .. loop_info: 32 contiguous doubles
    s = fnv(s, r.mask.data(), r.mask.size()); s = fnv(s, r.mi.data(), 4 * (size_t)o.n_inliers); s = fnv(s, r.id.data(), 4 * (size_t)o.n_inliers);
    s = fnv(s, r.xy.data(), 16 * (size_t)o.n_inliers);
    std::printf("%s %d %d %d %d %d %d %d %d %016llx\n", tag, o.status, o.n_inliers, o.ransac_best, o.ransac_iter, o.ransac_bound, o.has_loop, o.refit_iters,
                o.refit_up, s);
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s case.bin ...\n", argv[0]); return 2; }
    try {
        vg_handle* h = nullptr;
        if (vg_create(&h) != VG_OK) throw std::runtime_error("vg_create failed");
        const int n = argc - 1;
        std::vector<Pair> prs(n);
        for (int i = 0; i < n; ++i) load(argv[i + 1], prs[i]);
        std::vector<vg_kf_pnp_in> ins;
        std::vector<Out> outs;
        std::vector<vg_kf_pnp_out> os;
        for (int i = 0; i < n; ++i) { ins.push_back(prs[i].in); outs.emplace_back(prs[i].in.n); }
        for (int i = 0; i < n; ++i) os.push_back(outs[i].o);
        if (vg_kf_pnp(h, n, ins.data(), os.data()) != VG_OK) throw std::runtime_error(vg_last_error(h));
        for (int i = 0; i < n; ++i) { outs[i].o = os[i]; line("batch", outs[i]); }
        for (int i = 0; i < n; ++i) {
            Out one(prs[i].in.n);
            if (vg_kf_pnp(h, 1, &prs[i].in, &one.o) != VG_OK) throw std::runtime_error(vg_last_error(h));
            line("alone", one);
        }
        vg_destroy(h);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "kf_pnp_san_main: %s\n", e.what());
        return 1;
    }
    return 0;
}
