// kf_san_main.cpp — stand-alone driver of vg_kf_* for a sanitizer build on the CPU (tests/test_kf_brief_simt.py builds it with
// -fsanitize=address,undefined together with the emulated kernels of csrc/fe_ransac.hip and runs it; nothing is loaded into Python).
// Every argument is a KFS1 file (tests/kf_brief_ref.write_san_case): one frame with its window points and camera, the capacities, and a
// planted match (old descriptors, 8 window descriptors).  Per file: vg_kf_configure, vg_kf_add, then a second configuration with room for
// the planted records, vg_kf_set twice and vg_kf_match.  Prints one line per file: the true keypoint count, the status, n_matched and a
// checksum of every array the two calls wrote.
#include <algorithm>
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
void ok(vg_handle* h, int rc) { if (rc != VG_OK) throw std::runtime_error(vg_last_error(h)); }

void run(vg_handle* h, const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) throw std::runtime_error(std::string("cannot open ") + path);
    int hdr[7];                                             // magic, W, H, max_keypoints, max_window_points, n_window, n_old
    rd(f, hdr, sizeof(hdr));
    if (hdr[0] != 0x3153464B) throw std::runtime_error("not a KFS1 file");
    const int W = hdr[1], H = hdr[2], MK = hdr[3], MW = hdr[4], nw = hdr[5], n_old = hdr[6];
    std::vector<int16_t> pat(1024);
    std::vector<uint8_t> img((size_t)W * H);
    std::vector<float> wxy(2 * (size_t)nw);
    double p[8];
    std::vector<uint64_t> od(4 * (size_t)n_old), wd(32);
    rd(f, pat.data(), 2048); rd(f, img.data(), img.size()); rd(f, wxy.data(), 4 * wxy.size()); rd(f, p, sizeof(p));
    rd(f, od.data(), 8 * od.size()); rd(f, wd.data(), 8 * wd.size());
    fclose(f);
    // ---- the frame
    ok(h, vg_kf_configure(h, W, H, MK, MW, 1, pat.data()));
    vg_kf_in in;
    std::memset(&in, 0, sizeof(in));
    in.struct_size = sizeof(in); in.slot = 0; in.img = img.data(); in.stride = W; in.n_window = nw; in.window_xy = wxy.data();
    in.camera.struct_size = sizeof(vg_fe_camera); in.camera.model = VG_CAM_PINHOLE;
    std::copy(p, p + 8, in.camera.p);
    std::vector<float> kp(2 * (size_t)MK), nm(2 * (size_t)MK);
    std::vector<uint8_t> sc((size_t)MK);
    std::vector<uint64_t> de(4 * (size_t)MK), wde(4 * (size_t)MW);
    vg_kf_out out;
    std::memset(&out, 0, sizeof(out));
    out.struct_size = sizeof(out); out.keypoints_xy = kp.data(); out.scores = sc.data(); out.norm_xy = nm.data(); out.descriptors = de.data();
    out.window_descriptors = wde.data();
    ok(h, vg_kf_add(h, 1, &in, &out));
    unsigned long long s = 1469598103934665603ull;
    const size_t k = (size_t)out.n_kept;
    s = fnv(s, kp.data(), 8 * k); s = fnv(s, sc.data(), k); s = fnv(s, nm.data(), 8 * k); s = fnv(s, de.data(), 32 * k); s = fnv(s, wde.data(), 32 * (size_t)nw);
    // ---- the planted match: slot 1 holds the 8 window descriptors, slot 2 the old descriptors
    const int MK2 = std::max(MK, n_old), MW2 = std::max(MW, 8);
    ok(h, vg_kf_configure(h, W, H, MK2, MW2, 3, pat.data()));
    std::vector<float> zero(2 * (size_t)std::max(MK2, MW2), 0.f), w8(16);
    std::vector<uint8_t> zsc((size_t)MK2, 0);
    for (int i = 0; i < 8; ++i) { w8[2 * i] = i + 0.5f; w8[2 * i + 1] = 2.0f * i; }
    vg_kf_record r;
    std::memset(&r, 0, sizeof(r));
    r.struct_size = sizeof(r); r.n_window = 8; r.window_xy = w8.data(); r.window_descriptors = wd.data();
    ok(h, vg_kf_set(h, 1, &r));
    std::memset(&r, 0, sizeof(r));
    r.struct_size = sizeof(r); r.n_keypoints = n_old; r.keypoints_xy = zero.data(); r.scores = zsc.data(); r.norm_xy = zero.data(); r.descriptors = od.data();
    ok(h, vg_kf_set(h, 2, &r));
    vg_kf_pair pr;
    pr.struct_size = sizeof(pr); pr.cur_slot = 1; pr.old_slot = 2;
    std::vector<int> bi((size_t)MW2), bd((size_t)MW2), mi((size_t)MW2);
    std::vector<uint8_t> st((size_t)MW2);
    vg_kf_match_out mo;
    std::memset(&mo, 0, sizeof(mo));
    mo.struct_size = sizeof(mo); mo.best_idx = bi.data(); mo.best_dist = bd.data(); mo.status = st.data(); mo.matched_index = mi.data();
    ok(h, vg_kf_match(h, 1, &pr, &mo));
    s = fnv(s, bi.data(), 4 * (size_t)mo.n_window); s = fnv(s, bd.data(), 4 * (size_t)mo.n_window); s = fnv(s, st.data(), (size_t)mo.n_window);
    s = fnv(s, mi.data(), 4 * (size_t)mo.n_matched);
    std::printf("%d %d %d %016llx\n", out.n_keypoints, out.status, mo.n_matched, s);
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s case.bin ...\n", argv[0]); return 2; }
    try {
        vg_handle* h = nullptr;
        if (vg_create(&h) != VG_OK) throw std::runtime_error("vg_create failed");
        for (int i = 1; i < argc; ++i) run(h, argv[i]);
        vg_destroy(h);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "kf_san_main: %s\n", e.what());
        return 1;
    }
    return 0;
}
