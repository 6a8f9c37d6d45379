// pose_graph.h — the loop detection of the pose graph's PoseGraph (pose_graph/src/pose_graph.h, pose_graph.cpp:304-410) on the device
// through vg_voc_load / vg_bow_* / vg_kf_loop_detect (include/vinsgpu.h): loadVocabulary, detectLoop and addKeyFrameIntoVoc with the
// reference's signatures, over the resident record of a KeyFrame (host/keyframe.h).  Stand-alone and header-only.  A PoseGraph owns one
// DATABASE of the handle (PoseGraph::configure allocates them once, after the vocabulary is loaded).  optimize4DoF, the thumbnails and the
// debug images are not here.
#pragma once
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>
#include "../../include/vinsgpu.h"
#include "keyframe.h"
#include "vg_pack.h"

// BriefVocabulary(path): the reference's binary vocabulary (VocabularyBinary.hpp): 6 x int32 k, L, scoringType, weightingType, nNodes,
// nWords, then the node records, then the word records.  It only reads the file: the tree is built by the library (vg_voc_load).
class BriefVocabulary {
  public:
    int32_t k = 0, L = 0, scoring = 0, weighting = 0;
    std::vector<vg_voc_node> nodes;
    std::vector<vg_voc_word> words;
    explicit BriefVocabulary(const std::string& path) {
        FILE* f = fopen(path.c_str(), "rb");
        if (!f) throw std::runtime_error("Could not open file " + path);
        int32_t hdr[6];
        bool ok = fread(hdr, sizeof(int32_t), 6, f) == 6 && hdr[4] >= 0 && hdr[5] >= 0;
        if (ok) {
            k = hdr[0]; L = hdr[1]; scoring = hdr[2]; weighting = hdr[3];
            nodes.resize((size_t)hdr[4]); words.resize((size_t)hdr[5]);
            ok = fread(nodes.data(), sizeof(vg_voc_node), nodes.size(), f) == nodes.size() && fread(words.data(), sizeof(vg_voc_word), words.size(), f) == words.size();
        }
        fclose(f);
        if (!ok) throw std::runtime_error(path + ": not a binary vocabulary (truncated)");
    }
};
static_assert(sizeof(vg_voc_node) == 48 && sizeof(vg_voc_word) == 8, "the file's record layout");

class PoseGraph {
  public:
    // once per handle, after loadVocabulary: n_db pose graphs of at most max_entries keyframes, pool_words (word, value) pairs each
    static void configure(vg_handle* h, int n_db, int max_entries, int pool_words) {
        if (vg_bow_configure(h, n_db, max_entries, pool_words) != VG_OK) throw std::runtime_error(vg_last_error(h));
    }
    PoseGraph(vg_handle* h_, int db_) : h(h_), db(db_) {}
    // (the vocabulary is the handle's: one load serves every PoseGraph on it, and empties their databases)
    void loadVocabulary(const std::string& voc_path) {
        const BriefVocabulary voc(voc_path);
        if (vg_voc_load(h, voc.k, voc.L, voc.scoring, voc.weighting, (int)voc.nodes.size(), voc.nodes.data(), (int)voc.words.size(), voc.words.data()) != VG_OK)
            throw std::runtime_error(vg_last_error(h));
    }
    // detectLoop (pose_graph.cpp:304-386): query, then add; the index of the loop candidate or -1.  `last` holds the whole answer.
    int detectLoop(KeyFrame* keyframe, int frame_index) {
        run(keyframe, frame_index, VG_BOW_QUERY | VG_BOW_ADD);
        return last.loop_index;
    }
    // addKeyFrameIntoVoc (pose_graph.cpp:388-410)
    void addKeyFrameIntoVoc(KeyFrame* keyframe) { run(keyframe, keyframe->index, VG_BOW_ADD); }
    vg_bow_out last = {};

  private:
    vg_handle* h;
    int db;
    void run(KeyFrame* keyframe, int frame_index, int flags) {
        vg_bow_in in;
        vg_pack_bow(*keyframe, db, frame_index, flags, in, last);
        if (vg_kf_loop_detect(h, 1, &in, &last) != VG_OK) throw std::runtime_error(vg_last_error(h));
    }
};
