// kf_bow_san_main.cpp — a stand-alone program over the EMULATED kernels of vg_voc_load / vg_bow_* / vg_kf_loop_detect (csrc/kf_bow.h), built
// with -fsanitize=address,undefined by tests/test_kf_bow_simt.py::test_standalone_sanitizer_run and run as a subprocess.
//   kf_bow_san <voc.bin> <frames.bin>
// voc.bin: the reference's binary vocabulary layout; frames.bin: BOW1 (tests/kf_bow_ref.write_frames).  Every frame is planted with
// vg_kf_set and goes through vg_kf_loop_detect (QUERY | ADD) on database 0 with the taps on; a second database gets the same stream in the
// same calls from the second frame on (a batch of two).  Prints, per frame, the line tests/kf_bow_ref.result_line builds.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../include/vinsgpu.h"

// Linked with vg_core, fe_ransac and the emulator's runtime only: vg_destroy's hooks into the units that are left out (state this
// program never creates)
struct FeState;
extern "C" void fe_state_destroy(FeState*) {}
extern "C" void ba_graph_release(vg_handle*) {}
extern "C" void ba_seq_release(vg_handle*) {}

static bool read_all(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: kf_bow_san <voc.bin> <frames.bin>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror("voc"); return 2; }
    int32_t vh[6];
    if (!read_all(f, vh, sizeof(vh)) || vh[4] < 1 || vh[5] < 1) { fprintf(stderr, "bad vocabulary header\n"); return 2; }
    std::vector<vg_voc_node> nodes((size_t)vh[4]);
    std::vector<vg_voc_word> words((size_t)vh[5]);
    if (!read_all(f, nodes.data(), nodes.size() * sizeof(vg_voc_node)) || !read_all(f, words.data(), words.size() * sizeof(vg_voc_word))) { fprintf(stderr, "vocabulary truncated\n"); return 2; }
    fclose(f);
    f = fopen(argv[2], "rb");
    if (!f) { perror("frames"); return 2; }
    int32_t fh[3];
    if (!read_all(f, fh, sizeof(fh)) || fh[0] != 0x31574F42 || fh[1] < 0) { fprintf(stderr, "not a BOW1 file\n"); return 2; }
    std::vector<std::vector<uint64_t>> frames((size_t)fh[1]);
    size_t most = 1, total = 1;
    for (auto& fr : frames) {
        int32_t n = 0;
        if (!read_all(f, &n, 4) || n < 0) { fprintf(stderr, "frames truncated\n"); return 2; }
        fr.resize(4 * (size_t)n);
        if (n && !read_all(f, fr.data(), 32 * (size_t)n)) { fprintf(stderr, "frames truncated\n"); return 2; }
        if ((size_t)n > most) most = (size_t)n;
        total += (size_t)n;
    }
    fclose(f);
    vg_handle* h = nullptr;
    if (vg_create(&h) != VG_OK) { fprintf(stderr, "vg_create failed\n"); return 1; }
    auto die = [&](const char* what) { fprintf(stderr, "%s: %s\n", what, vg_last_error(h)); return 1; };
    int16_t pattern[1024] = {0};
    if (vg_kf_configure(h, 64, 64, (int)most, 1, 1, pattern) != VG_OK) return die("vg_kf_configure");
    if (vg_voc_load(h, vh[0], vh[1], vh[2], vh[3], vh[4], nodes.data(), vh[5], words.data()) != VG_OK) return die("vg_voc_load");
    if (vg_bow_configure(h, 2, (int)frames.size() + 1, (int)total) != VG_OK) return die("vg_bow_configure");
    std::vector<float> xy(2 * most, 0.f);
    std::vector<uint8_t> sc(most, 0);
    std::vector<uint32_t> wok(2 * most), bw(2 * most);
    std::vector<double> bv(2 * most);
    int rc = 0;
    for (size_t i = 0; i < frames.size(); ++i) {
        const int n = (int)(frames[i].size() / 4);
        vg_kf_record rec;
        memset(&rec, 0, sizeof(rec));
        rec.struct_size = (int)sizeof(rec); rec.n_keypoints = n;
        rec.keypoints_xy = xy.data(); rec.scores = sc.data(); rec.norm_xy = xy.data(); rec.descriptors = frames[i].data();
        if (vg_kf_set(h, 0, &rec) != VG_OK) return die("vg_kf_set");
        vg_bow_in in[2];
        vg_bow_out out[2];
        memset(in, 0, sizeof(in)); memset(out, 0, sizeof(out));
        const int nreq = i >= 1 ? 2 : 1;
        for (int r = 0; r < nreq; ++r) {
            in[r].struct_size = (int)sizeof(vg_bow_in); in[r].db = r; in[r].slot = 0; in[r].frame_index = fh[2] + (int)i; in[r].flags = VG_BOW_QUERY | VG_BOW_ADD;
            out[r].struct_size = (int)sizeof(vg_bow_out);
            out[r].word_of_keypoint = wok.data() + most * r; out[r].bow_word = bw.data() + most * r; out[r].bow_value = bv.data() + most * r;
        }
        if (vg_kf_loop_detect(h, nreq, in, out) != VG_OK) return die("vg_kf_loop_detect");
        const vg_bow_out& q = out[0];
        printf("%d %d %d %d %d %d", in[0].frame_index, q.loop_index, q.find_loop, q.entry_id, q.n_words, q.n_results);
        for (int k = 0; k < q.n_results; ++k) {
            unsigned long long u;
            memcpy(&u, &q.scores[k], 8);
            printf(" %d:%016llx", q.ids[k], u);
        }
        printf("\n");
        if (nreq == 2 && (out[1].n_words != q.n_words || memcmp(bw.data(), bw.data() + most, 4 * (size_t)q.n_words) || memcmp(bv.data(), bv.data() + most, 8 * (size_t)q.n_words))) {
            fprintf(stderr, "frame %zu: the two databases' vectors differ\n", i);
            rc = 1;
        }
        vg_bow_entry e;
        memset(&e, 0, sizeof(e));
        e.struct_size = (int)sizeof(e); e.capacity = (int)most; e.words = wok.data() + most; e.values = bv.data() + most;
        if (vg_bow_get(h, 0, q.entry_id, &e) != VG_OK) return die("vg_bow_get");
        if (e.n_words != q.n_words || memcmp(e.values, bv.data(), 8 * (size_t)q.n_words)) { fprintf(stderr, "frame %zu: vg_bow_get differs from the tap\n", i); rc = 1; }
    }
    if (vg_bow_reset(h, 1) != VG_OK) return die("vg_bow_reset");
    vg_destroy(h);
    return rc;
}
