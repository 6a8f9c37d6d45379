// init_exrot_san_main.cpp — stand-alone driver of vg_init_exrot for a sanitizer build on the CPU (tests/test_init_exrot_simt.py builds it
// with -fsanitize=address,undefined together with the emulated kernels of csrc/fe_ransac.hip and runs it; nothing is loaded into Python).
// Every argument is a VEX1 file (tests/init_exrot_ref.write_file); all of them go into ONE call, then each alone, then each run of two
// steps or more split after its first step and resumed through records / ric.  Prints one line per window: S, status, first_ok, and a
// checksum of everything the call wrote ("split": of the two parts' outputs joined, which must be the unsplit run's).
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
    int S = 0;
    std::vector<int> off, ok, branch, it, bound, nin, best, front, picked, fb;
    std::vector<double> corr, dq, prev, records, ric, sigma, huber, F;
    double ric_prev[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    vg_exrot_in in;
    vg_exrot_out out;
    // (re)point the structs at the vectors: steps [lo, hi) of the file carrying `prev`
    void bind(int lo, int hi) {
        const int n = hi - lo;
        std::memset(&in, 0, sizeof(in));
        std::memset(&out, 0, sizeof(out));
        in.struct_size = sizeof(in); in.n_steps = n; in.corr_off = off.data() + lo; in.corr = corr.data(); in.delta_q = dq.data() + 4 * (size_t)lo;
        in.n_prev = (int)(prev.size() / 27); in.prev = prev.empty() ? nullptr : prev.data(); in.ric_prev = ric_prev;
        in.ransac_threshold = 3.0; in.confidence = 0.99; in.min_points = 9; in.huber_deg = 5.0; in.min_frames = 10; in.cov_threshold = 0.25;
        for (auto* v : {&ok, &branch, &it, &bound, &nin, &best, &picked, &fb}) v->assign(n, 0);
        front.assign(4 * (size_t)n, 0); records.assign(27 * (size_t)n, 0.0); ric.assign(9 * (size_t)n, 0.0); sigma.assign(4 * (size_t)n, 0.0);
        huber.assign(n, 0.0); F.assign(9 * (size_t)n, 0.0);
        out.struct_size = sizeof(out);
        out.records = records.data(); out.ric = ric.data(); out.sigma = sigma.data(); out.ok = ok.data(); out.huber = huber.data();
        out.branch = branch.data(); out.ransac_iter = it.data(); out.ransac_bound = bound.data(); out.ransac_inliers = nin.data();
        out.ransac_best = best.data(); out.F = F.data(); out.front = front.data(); out.picked = picked.data(); out.used_fallback = fb.data();
    }
};
void rd(FILE* f, void* p, size_t bytes) { if (bytes && fread(p, 1, bytes, f) != bytes) throw std::runtime_error("file truncated"); }

void load(const char* path, Window& w) {
    FILE* f = fopen(path, "rb");
    if (!f) throw std::runtime_error(std::string("cannot open ") + path);
    int hdr[3];                                             // magic, S, rows of corr
    rd(f, hdr, sizeof(hdr));
    if (hdr[0] != 0x31584556) throw std::runtime_error("not a VEX1 file");
    w.S = hdr[1];
    const int rows = hdr[2];
    w.off.resize(w.S + 1); w.corr.resize(4 * (size_t)rows + 4); w.dq.resize(4 * (size_t)w.S);
    rd(f, w.off.data(), sizeof(int) * (w.S + 1)); rd(f, w.corr.data(), sizeof(double) * 4 * rows); rd(f, w.dq.data(), sizeof(double) * 4 * w.S);
    fclose(f);
    w.bind(0, w.S);
}

unsigned long long sum_bits(const void* p, size_t bytes, unsigned long long h) {
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i < bytes; ++i) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}
// the per-step outputs, array after array (so that two parts joined array by array hash like the whole)
struct Joined {
    std::vector<double> d[5];
    std::vector<int> i[9];
    void add(const Window& w) {
        const std::vector<double>* dv[5] = {&w.records, &w.ric, &w.sigma, &w.huber, &w.F};
        const std::vector<int>* iv[9] = {&w.ok, &w.branch, &w.it, &w.bound, &w.nin, &w.best, &w.front, &w.picked, &w.fb};
        for (int k = 0; k < 5; ++k) d[k].insert(d[k].end(), dv[k]->begin(), dv[k]->end());
        for (int k = 0; k < 9; ++k) i[k].insert(i[k].end(), iv[k]->begin(), iv[k]->end());
    }
    unsigned long long hash() const {
        unsigned long long h = 1469598103934665603ull;
        for (const auto& v : d) h = sum_bits(v.data(), v.size() * sizeof(double), h);
        for (const auto& v : i) h = sum_bits(v.data(), v.size() * sizeof(int), h);
        return h;
    }
};
void print(const char* tag, int S, int status, int first_ok, const double* calib, const Joined& j) {
    std::printf("%s %d %d %d %016llx\n", tag, S, status, first_ok, sum_bits(calib, 9 * sizeof(double), j.hash()));
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
        std::vector<vg_exrot_in> ins(n);
        std::vector<vg_exrot_out> outs(n);
        for (int i = 0; i < n; ++i) { ins[i] = wins[i].in; outs[i] = wins[i].out; }
        if (vg_init_exrot(h, n, ins.data(), outs.data()) != VG_OK) throw std::runtime_error(vg_last_error(h));
        for (int i = 0; i < n; ++i) {
            wins[i].out = outs[i];
            Joined j; j.add(wins[i]);
            print("batch", wins[i].S, outs[i].status, outs[i].first_ok, outs[i].calib_ric, j);
        }
        for (int i = 0; i < n; ++i) {
            if (vg_init_exrot(h, 1, &wins[i].in, &wins[i].out) != VG_OK) throw std::runtime_error(vg_last_error(h));
            Joined j; j.add(wins[i]);
            print("alone", wins[i].S, wins[i].out.status, wins[i].out.first_ok, wins[i].out.calib_ric, j);
        }
        for (int i = 0; i < n; ++i) {
            Window& w = wins[i];
            if (w.S < 2) continue;
            Joined j;
            w.bind(0, 1);
            if (vg_init_exrot(h, 1, &w.in, &w.out) != VG_OK) throw std::runtime_error(vg_last_error(h));
            j.add(w);
            int first_ok = w.out.first_ok, status = w.out.status;
            double calib[9];
            std::memcpy(calib, w.out.calib_ric, sizeof(calib));
            const std::vector<double> rec = w.records, ric = w.ric;
            w.prev = rec;
            std::memcpy(w.ric_prev, ric.data(), sizeof(w.ric_prev));
            w.bind(1, w.S);
            if (vg_init_exrot(h, 1, &w.in, &w.out) != VG_OK) throw std::runtime_error(vg_last_error(h));
            j.add(w);
            if (w.out.status != VG_EXROT_OK) status = w.out.status;
            if (first_ok < 0) { first_ok = w.out.first_ok; std::memcpy(calib, w.out.calib_ric, sizeof(calib)); }
            print("split", w.S, status, status == VG_EXROT_OK ? first_ok : -1, calib, j);
        }
        vg_destroy(h);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "init_exrot_san_main: %s\n", e.what());
        return 1;
    }
    return 0;
}
