// kf_bow.h — vg_voc_load / vg_bow_* / vg_kf_loop_detect: DBoW2 loop detection of the pose graph (PoseGraph::detectLoop, addKeyFrameIntoVoc)
// for a batch of pose graphs: the vocabulary tree, one resident database per pose graph, the query, the decision and the add.
// include/vinsgpu.h defines every stage (DBoW2 is vendored in the reference and READ there); this file is the device code and the host
// entries.  It is included at the END of fe_ransac.hip (after kf_pnp.h), compiled with -ffp-contract=off like the rest of the unit.  The
// input of a request is a resident record of kf_brief.h: nothing goes up but the request.
//
// THE TREE on the device is renumbered breadth first, so that the children of a node are contiguous and in child order:
//   vdesc [n_tot][4]  the descriptors, 32 bytes a node (the root's are zero and never read)
//   vkid  [n_tot]     (first child, number of children); a leaf: (the FILE's word id, 0)
//   vweight [n_words] by the file's word id
// A DATABASE is pool_w / pool_v [pool_words] with off [max_entries + 1]: entry e is [off[e], off[e + 1]), word ids ascending.  The host
// keeps the same offsets (it learns the word count of every add from the download), so every capacity is checked before a launch.
//
// vg_kf_loop_detect, four launches over the batch between one upload and one download:
//   bow_walk_kernel    16 lanes per descriptor, a lane per child: two 16-byte loads, four popcounts, the minimum of (distance << 16 | child)
//                      over the group by four shuffles; a node with more than 16 children takes more rounds.  The descriptor stays in
//                      registers for all levels.  Every loop is uniform over the wavefront (a finished group idles along).
//   bow_vector_kernel  a workgroup per request: bitonic sort of the word ids (in LDS up to BOW_SORT_LDS, in global scratch beyond), the
//                      heads of the runs ranked by ballots, the repeated addition per run, the sequential norm by one thread, the division
//   bow_score_kernel   a wavefront per (request, eligible entry): a lane per entry word looks its word up in the query vector by bisection;
//                      the terms of the found words are then added in ascending word order by ONE chain (ballot, shuffle per set bit)
//   bow_tail_kernel    a wavefront per request: the smallest 4 by (value, entry id), the halving, the decision, the append into the pool
// No floating-point atomic anywhere, and no atomic at all.
#pragma once
#include <cstring>

#define BOW_GROUP 16
#define BOW_NONE 0xFFFFFFFFu
#define BOW_SORT_LDS 8192             // word ids a workgroup sorts in LDS (32 KB); longer lists are sorted in global scratch
#define BOW_VEC_THREADS 1024
#define BOW_HDR 16                    // ints per request that come down: n_words n_results ids[4] find_loop loop_index entry_id

struct BowDev {
    int n, stride, sort_stride, emax, ME, PW;
    unsigned rec_bytes, r_desc;
    const char* rec;
    const unsigned long long* vdesc;
    const int2* vkid;
    const double* vweight;
    unsigned* pool_w;                 // [n_db][PW]
    double* pool_v;                   // [n_db][PW]
    int* off;                         // [n_db][ME + 1]
    const int* req;                   // [n][8] db slot frame_index flags n_entries - - -
    unsigned* wok;                    // [n][stride] word of keypoint
    unsigned* sorted;                 // [n][sort_stride] (sort_stride 0: every list fits LDS)
    unsigned* sw;                     // [n][stride] the frame's vector
    double* sv;
    double* score;                    // [n][emax]
    int* has;                         // [n][emax]
    int* hdr;                         // [n][BOW_HDR]
    double* outd;                     // [n][4]
};

extern "C" __global__ __launch_bounds__(256) void bow_walk_kernel(BowDev b) {
    const int tid = threadIdx.x, sub = tid & (BOW_GROUP - 1), r = blockIdx.y;
    const int i = blockIdx.x * (256 / BOW_GROUP) + tid / BOW_GROUP;
    const char* rec = b.rec + (size_t)b.req[8 * r + 1] * b.rec_bytes;
    const int nk = min(((const int*)rec)[0], b.stride);
    bool done = i >= nk;
    unsigned long long d0 = 0, d1 = 0, d2 = 0, d3 = 0;
    if (!done) {
        const ulonglong2* dp = (const ulonglong2*)(rec + b.r_desc) + 2 * (size_t)i;
        const ulonglong2 lo = dp[0], hi = dp[1];
        d0 = lo.x; d1 = lo.y; d2 = hi.x; d3 = hi.y;
    }
    int node = 0, word = -1;
    while (true) {
        int first = 0, cnt = 0;
        if (!done) {
            const int2 kc = b.vkid[node];
            first = kc.x; cnt = kc.y;
            if (cnt == 0) { done = true; word = first; }
        }
        if (!__any(!done)) break;
        unsigned key = 0xFFFFFFFFu;
        for (int c0 = 0; __any(!done && c0 < cnt); c0 += BOW_GROUP) {
            const int c = c0 + sub;
            if (!done && c < cnt) {
                const ulonglong2* np = (const ulonglong2*)b.vdesc + 2 * (size_t)(first + c);
                const ulonglong2 lo = np[0], hi = np[1];
                const int dist = __popcll(d0 ^ lo.x) + __popcll(d1 ^ lo.y) + __popcll(d2 ^ hi.x) + __popcll(d3 ^ hi.y);
                key = min(key, ((unsigned)dist << 16) | (unsigned)c);
            }
        }
#pragma unroll
        for (int m = BOW_GROUP / 2; m >= 1; m >>= 1) key = min(key, (unsigned)__shfl_xor((int)key, m, BOW_GROUP));
        if (!done) node = first + (int)(key & 0xFFFFu);
    }
    if (i < nk && sub == 0) b.wok[(size_t)r * b.stride + i] = b.vweight[word] > 0.0 ? (unsigned)word : BOW_NONE;
}

extern "C" __global__ __launch_bounds__(BOW_VEC_THREADS) void bow_vector_kernel(BowDev b) {
    __shared__ unsigned lds_a[BOW_SORT_LDS];
    __shared__ double lds_d[BOW_VEC_THREADS];
    __shared__ int wcnt[BOW_VEC_THREADS / 64];
    __shared__ double s_norm;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = blockIdx.x;
    const char* rec = b.rec + (size_t)b.req[8 * r + 1] * b.rec_bytes;
    const int nk = min(((const int*)rec)[0], b.stride);
    int P = 1;
    while (P < nk) P <<= 1;
    unsigned* a = P <= BOW_SORT_LDS ? lds_a : b.sorted + (size_t)r * b.sort_stride;
    const unsigned* wok = b.wok + (size_t)r * b.stride;
    for (int i = tid; i < P; i += BOW_VEC_THREADS) a[i] = i < nk ? wok[i] : BOW_NONE;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += BOW_VEC_THREADS) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned x = a[i], y = a[l];
                    if ((x > y) == ((i & k) == 0)) { a[i] = y; a[l] = x; }
                }
            }
            __syncthreads();
        }
    // the heads of the runs, ranked in order; a head adds its word's weight c - 1 times
    unsigned* sw = b.sw + (size_t)r * b.stride;
    double* sv = b.sv + (size_t)r * b.stride;
    int base = 0;
    for (int i0 = 0; i0 < nk; i0 += BOW_VEC_THREADS) {
        const int i = i0 + tid;
        const unsigned x = i < nk ? a[i] : BOW_NONE;
        const bool head = x != BOW_NONE && (i == 0 || a[i - 1] != x);
        const unsigned long long bal = __ballot(head);
        if (lane == 0) wcnt[wave] = __popcll(bal);
        __syncthreads();
        int pre = base + __popcll(bal & ((1ull << lane) - 1ull)), tot = 0;
        for (int q = 0; q < BOW_VEC_THREADS / 64; ++q) { const int v = wcnt[q]; pre += q < wave ? v : 0; tot += v; }
        if (head) {
            int c = 1;
            while (i + c < nk && a[i + c] == x) ++c;
            const double w = b.vweight[x];
            double v = w;
            for (int t = 1; t < c; ++t) v += w;
            sw[pre] = x; sv[pre] = v;
        }
        base += tot;
        __syncthreads();
    }
    const int nw = base;
    // norm: the sum of fabs(v) in ascending word id by ONE chain; the values pass through LDS a chunk at a time
    double norm = 0.0;
    for (int i0 = 0; i0 < nw; i0 += BOW_VEC_THREADS) {
        if (i0 + tid < nw) lds_d[tid] = fabs(sv[i0 + tid]);
        __syncthreads();
        if (tid == 0) {
            const int m = min(BOW_VEC_THREADS, nw - i0);
            for (int q = 0; q < m; ++q) norm += lds_d[q];
        }
        __syncthreads();
    }
    if (tid == 0) { s_norm = norm; b.hdr[BOW_HDR * r] = nw; }
    __syncthreads();
    norm = s_norm;
    if (norm > 0.0)
        for (int i = tid; i < nw; i += BOW_VEC_THREADS) sv[i] = sv[i] / norm;
}

extern "C" __global__ __launch_bounds__(256) void bow_score_kernel(BowDev b) {
    const int lane = threadIdx.x & 63, r = blockIdx.y, e = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= b.emax) return;                                    // (the whole wavefront, here and below)
    const int* rq = b.req + 8 * r;
    const int db = rq[0], max_id = rq[2] - 50, ne = rq[4];
    const bool takes_part = (rq[3] & VG_BOW_QUERY) && e < ne && (e < max_id || max_id == -1 || e == ne - 1);
    if (!takes_part) {
        if (lane == 0) b.has[(size_t)r * b.emax + e] = 0;
        return;
    }
    const int* off = b.off + (size_t)db * (b.ME + 1);
    const int o0 = off[e], nd = off[e + 1] - o0, nq = b.hdr[BOW_HDR * r];
    const unsigned* dw = b.pool_w + (size_t)db * b.PW + o0;
    const double* dv = b.pool_v + (size_t)db * b.PW + o0;
    const unsigned* qw = b.sw + (size_t)r * b.stride;
    const double* qv = b.sv + (size_t)r * b.stride;
    double acc = 0.0;
    bool have = false;
    for (int j0 = 0; j0 < nd; j0 += 64) {
        const int j = j0 + lane;
        bool found = false;
        double term = 0.0;
        if (j < nd) {
            const unsigned w = dw[j];
            int lo = 0, hi = nq;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (qw[mid] < w) lo = mid + 1; else hi = mid;
            }
            if (lo < nq && qw[lo] == w) {
                const double q = qv[lo], d = dv[j];
                found = true;
                term = fabs(q - d) - fabs(q) - fabs(d);
            }
        }
        unsigned long long mask = __ballot(found);
        while (mask) {                                          // ascending lane = ascending word id: one chain, the same in every lane
            const int src = __ffsll((long long)mask) - 1;
            const double t = __shfl(term, src);
            acc = have ? acc + t : t;
            have = true;
            mask &= mask - 1ull;
        }
    }
    if (lane == 0) {
        b.has[(size_t)r * b.emax + e] = have ? 1 : 0;
        b.score[(size_t)r * b.emax + e] = acc;
    }
}

extern "C" __global__ __launch_bounds__(64) void bow_tail_kernel(BowDev b) {
    const int lane = threadIdx.x, r = blockIdx.x;
    const int* rq = b.req + 8 * r;
    const int db = rq[0], frame_index = rq[2], flags = rq[3], ne = rq[4];
    const double* score = b.score + (size_t)r * b.emax;
    const int* has = b.has + (size_t)r * b.emax;
    int ids[VG_BOW_MAX_RESULTS] = {-1, -1, -1, -1}, nres = 0;
    double sc[VG_BOW_MAX_RESULTS] = {0.0, 0.0, 0.0, 0.0};
    if (flags & VG_BOW_QUERY) {
#pragma unroll 1
        for (int k = 0; k < VG_BOW_MAX_RESULTS; ++k) {
            double bv = 0.0;
            int bi = 0x7FFFFFFF;
            for (int e = lane; e < ne; e += 64) {
                if (!has[e] || e == ids[0] || e == ids[1] || e == ids[2]) continue;
                const double v = score[e];
                if (bi == 0x7FFFFFFF || v < bv) { bv = v; bi = e; }       // (e ascends: an equal value keeps the smaller id)
            }
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                const double ov = __shfl_xor(bv, m);
                const int oi = __shfl_xor(bi, m);
                if (oi != 0x7FFFFFFF && (bi == 0x7FFFFFFF || ov < bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
            }
            if (bi == 0x7FFFFFFF) break;                        // (uniform: every lane holds the same minimum)
            ids[k] = bi; sc[k] = -bv / 2.0; nres = k + 1;
        }
    }
    bool find_loop = false;
    if (nres >= 1 && sc[0] > 0.05)
        for (int k = 1; k < nres; ++k) find_loop = find_loop || sc[k] > 0.015;
    int loop_index = -1;
    if (find_loop && frame_index > 50) {
        loop_index = ids[0];
        for (int k = 1; k < nres; ++k)
            if (ids[k] < loop_index && sc[k] > 0.015) loop_index = ids[k];
    }
    int entry = -1;
    if (flags & VG_BOW_ADD) {
        int* off = b.off + (size_t)db * (b.ME + 1);
        const int o0 = off[ne], nw = b.hdr[BOW_HDR * r];
        unsigned* pw = b.pool_w + (size_t)db * b.PW + o0;
        double* pv = b.pool_v + (size_t)db * b.PW + o0;
        const unsigned* sw = b.sw + (size_t)r * b.stride;
        const double* sv = b.sv + (size_t)r * b.stride;
        for (int i = lane; i < nw; i += 64) { pw[i] = sw[i]; pv[i] = sv[i]; }
        if (lane == 0) off[ne + 1] = o0 + nw;
        entry = ne;
    }
    if (lane == 0) {
        int* hd = b.hdr + BOW_HDR * r;
        hd[1] = nres;
        for (int k = 0; k < VG_BOW_MAX_RESULTS; ++k) { hd[2 + k] = ids[k]; b.outd[4 * r + k] = sc[k]; }
        hd[6] = find_loop ? 1 : 0; hd[7] = loop_index; hd[8] = entry;
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
struct BowState {
    int k = 0, L = 0, n_tot = 0, n_words = 0;                   // the vocabulary (n_tot: the nodes with the root)
    char* voc = nullptr;                                        // vdesc | vkid | vweight
    size_t v_kid = 0, v_weight = 0;
    int n_db = 0, ME = 0, PW = 0;
    char* db = nullptr;                                         // pool_w | pool_v | off
    size_t d_v = 0, d_off = 0;
    std::vector<std::vector<int>> off;                          // per database: the offsets of its entries, off[0] = 0 (the device's table, mirrored)
    char* buf = nullptr;
    size_t buf_cap = 0;
    PinnedBuf<char> h_up, h_down;
};

static void bow_release_db(BowState* s) {
    (void)hipFree(s->db);
    s->db = nullptr; s->n_db = s->ME = s->PW = 0;
    s->off.clear();
}

extern "C" void bow_release(vg_handle* h) {
    BowState* s = (BowState*)h->bow;
    if (!s) return;
    (void)hipFree(s->voc);
    bow_release_db(s);
    (void)hipFree(s->buf);
    s->h_up.release(); s->h_down.release();
    delete s;
    h->bow = nullptr;
}

extern "C" int vg_voc_load(vg_handle* h, int k, int L, int scoring, int weighting, int n_nodes, const vg_voc_node* nodes, int n_words, const vg_voc_word* words) {
    if (!h) return VG_ERR_BAD_ARG;
    auto bad = [&](const std::string& what) { h->err = "vg_voc_load: " + what; return VG_ERR_BAD_ARG; };
    if (scoring != VG_BOW_L1_NORM || weighting != VG_BOW_TF_IDF) return bad("only L1_NORM scoring with TF_IDF weighting is offered");
    if (k < 1 || k > 65535 || L < 1) return bad("k outside 1 .. 65535 or L < 1");
    if (n_nodes < 1 || n_words < 1 || !nodes || !words) return bad("an empty or NULL table");
    if (n_nodes > 0x3fffffff) return bad("too many nodes");
    // ---- the tree as the file states it: the children of a node in record order
    const size_t NT = (size_t)n_nodes + 1;
    std::vector<int> rec_of(NT, -1), n_child(NT, 0), start(NT + 1, 0), child((size_t)n_nodes), word_of(NT, -1);
    for (int i = 0; i < n_nodes; ++i) {
        const int id = nodes[i].node_id, p = nodes[i].parent_id;
        if (id < 1 || id > n_nodes) return bad("record " + std::to_string(i) + ": a node id outside 1 .. n_nodes");
        if (rec_of[id] >= 0) return bad("record " + std::to_string(i) + ": the node id is repeated");
        if (p < 0 || p > n_nodes) return bad("record " + std::to_string(i) + ": the parent is neither a node nor the root");
        rec_of[id] = i;
        ++n_child[p];
    }
    if (n_child[0] == 0) return bad("the root has no children");
    for (size_t v = 0; v < NT; ++v) {
        if (n_child[v] > k) return bad("node " + std::to_string(v) + " has more than k children");
        start[v + 1] = start[v] + n_child[v];
    }
    {
        std::vector<int> fill(start.begin(), start.end() - 1);
        for (int i = 0; i < n_nodes; ++i) child[fill[nodes[i].parent_id]++] = nodes[i].node_id;
    }
    std::vector<char> seen_word((size_t)n_words, 0);
    for (int i = 0; i < n_words; ++i) {
        const int id = words[i].node_id, w = words[i].word_id;
        if (id < 1 || id > n_nodes) return bad("word record " + std::to_string(i) + ": a node id outside 1 .. n_nodes");
        if (w < 0 || w >= n_words) return bad("word record " + std::to_string(i) + ": a word id outside 0 .. n_words - 1");
        if (seen_word[w]) return bad("word record " + std::to_string(i) + ": the word id is repeated");
        if (n_child[id] > 0) return bad("word record " + std::to_string(i) + ": a word on a node with children");
        if (word_of[id] >= 0) return bad("word record " + std::to_string(i) + ": a second word on the same leaf");
        seen_word[w] = 1; word_of[id] = w;
    }
    // ---- breadth first from the root: new ids, the children of a node side by side in child order
    std::vector<int> order, level(NT, -1);                     // order[new id] = the file's id
    order.reserve(NT);
    order.push_back(0); level[0] = 0;
    for (size_t q = 0; q < order.size(); ++q) {
        const int v = order[q];
        for (int c = start[v]; c < start[v + 1]; ++c) {
            if (level[child[c]] >= 0) return bad("the records do not form a tree");
            level[child[c]] = level[v] + 1;
            order.push_back(child[c]);
        }
    }
    if (order.size() != NT) return bad("a node is not reachable from the root");
    for (size_t v = 1; v < NT; ++v)
        if (n_child[v] == 0) {
            if (word_of[v] < 0) return bad("leaf " + std::to_string(v) + " has no word");
            if (level[v] > L) return bad("leaf " + std::to_string(v) + " lies below level L");
        }
    std::vector<unsigned long long> vdesc(4 * NT, 0ull);
    std::vector<int> vkid(2 * NT, 0);
    std::vector<double> vweight((size_t)n_words, 0.0);
    {
        size_t next = 1;                                        // the new id of the first child of order[q]
        for (size_t q = 0; q < NT; ++q) {
            const int v = order[q];
            if (v > 0) memcpy(&vdesc[4 * q], nodes[rec_of[v]].descriptor, 32);
            if (n_child[v] > 0) { vkid[2 * q] = (int)next; vkid[2 * q + 1] = n_child[v]; next += (size_t)n_child[v]; }
            else { vkid[2 * q] = word_of[v]; vkid[2 * q + 1] = 0; vweight[word_of[v]] = nodes[rec_of[v]].weight; }
        }
    }
    // ---- only now the device
    auto fail = [&](hipError_t err) { h->err = std::string("vg_voc_load: ") + hipGetErrorString(err); return VG_ERR_HIP; };
    hipError_t e = hipSetDevice(h->device);
    if (e != hipSuccess) return fail(e);
    if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return fail(e);
    BowState* s = (BowState*)h->bow;
    if (!s) { s = new BowState(); h->bow = s; }
    (void)hipFree(s->voc);
    s->voc = nullptr; s->n_tot = 0; s->n_words = 0;
    for (auto& o : s->off) o.assign(1, 0);                      // every database is empty again
    const size_t v_kid = kf_up(32 * NT), v_weight = kf_up(v_kid + 8 * NT), n_all = kf_up(v_weight + 8 * (size_t)n_words);
    if ((e = hipMalloc((void**)&s->voc, n_all)) != hipSuccess) return fail(e);
    if ((e = hipMemcpy(s->voc, vdesc.data(), 32 * NT, hipMemcpyHostToDevice)) != hipSuccess) return fail(e);
    if ((e = hipMemcpy(s->voc + v_kid, vkid.data(), 8 * NT, hipMemcpyHostToDevice)) != hipSuccess) return fail(e);
    if ((e = hipMemcpy(s->voc + v_weight, vweight.data(), 8 * (size_t)n_words, hipMemcpyHostToDevice)) != hipSuccess) return fail(e);
    s->k = k; s->L = L; s->n_tot = (int)NT; s->n_words = n_words; s->v_kid = v_kid; s->v_weight = v_weight;
    return VG_OK;
}

extern "C" int vg_bow_configure(vg_handle* h, int n_db, int max_entries, int pool_words) {
    if (!h) return VG_ERR_BAD_ARG;
    auto bad = [&](const char* what) { h->err = std::string("vg_bow_configure: ") + what; return VG_ERR_BAD_ARG; };
    BowState* s = (BowState*)h->bow;
    if (!s || !s->voc) return bad("the handle has no vocabulary (vg_voc_load)");
    if (n_db < 1 || max_entries < 1 || pool_words < 1) return bad("n_db, max_entries or pool_words < 1");
    if (max_entries > 0x3fffffff) return bad("max_entries is too large");
    auto fail = [&](hipError_t err) { h->err = std::string("vg_bow_configure: ") + hipGetErrorString(err); return VG_ERR_HIP; };
    hipError_t e = hipSetDevice(h->device);
    if (e != hipSuccess) return fail(e);
    if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return fail(e);
    bow_release_db(s);
    const size_t d_v = kf_up(4 * (size_t)n_db * pool_words), d_off = kf_up(d_v + 8 * (size_t)n_db * pool_words),
                 n_all = d_off + kf_up(4 * (size_t)n_db * ((size_t)max_entries + 1));
    if ((e = hipMalloc((void**)&s->db, n_all)) != hipSuccess) return fail(e);
    if ((e = hipMemset(s->db + d_off, 0, n_all - d_off)) != hipSuccess) return fail(e);          // off[db][0] = 0, for good
    s->n_db = n_db; s->ME = max_entries; s->PW = pool_words; s->d_v = d_v; s->d_off = d_off;
    s->off.assign((size_t)n_db, std::vector<int>(1, 0));
    return VG_OK;
}

extern "C" int vg_bow_reset(vg_handle* h, int db) {
    if (!h) return VG_ERR_BAD_ARG;
    BowState* s = (BowState*)h->bow;
    if (!s || !s->db) { h->err = "vg_bow_reset: the handle has no databases (vg_bow_configure)"; return VG_ERR_BAD_ARG; }
    if (db < 0 || db >= s->n_db) { h->err = "vg_bow_reset: db out of range"; return VG_ERR_BAD_ARG; }
    s->off[db].assign(1, 0);
    return VG_OK;
}

extern "C" int vg_bow_count(vg_handle* h, int db, int* n_entries, int* pool_used) {
    if (!h) return VG_ERR_BAD_ARG;
    BowState* s = (BowState*)h->bow;
    if (!s || !s->db) { h->err = "vg_bow_count: the handle has no databases (vg_bow_configure)"; return VG_ERR_BAD_ARG; }
    if (db < 0 || db >= s->n_db) { h->err = "vg_bow_count: db out of range"; return VG_ERR_BAD_ARG; }
    if (n_entries) *n_entries = (int)s->off[db].size() - 1;
    if (pool_used) *pool_used = s->off[db].back();
    return VG_OK;
}

extern "C" int vg_bow_get(vg_handle* h, int db, int entry, vg_bow_entry* out) {
    if (!h) return VG_ERR_BAD_ARG;
    auto bad = [&](const char* what) { h->err = std::string("vg_bow_get: ") + what; return VG_ERR_BAD_ARG; };
    BowState* s = (BowState*)h->bow;
    if (!s || !s->db) return bad("the handle has no databases (vg_bow_configure)");
    if (!out) return bad("a NULL argument");
    if (out->struct_size != (int)sizeof(vg_bow_entry)) return bad("vg_bow_entry::struct_size");
    if (db < 0 || db >= s->n_db) return bad("db out of range");
    const std::vector<int>& off = s->off[db];
    if (entry < 0 || entry >= (int)off.size() - 1) return bad("entry out of range");
    const int o0 = off[entry], nw = off[entry + 1] - o0;
    if ((out->words || out->values) && out->capacity < nw) return bad("capacity below the entry's word count");
    auto fail = [&](hipError_t err) { h->err = std::string("vg_bow_get: ") + hipGetErrorString(err); return VG_ERR_HIP; };
    hipError_t e = hipSetDevice(h->device);
    if (e != hipSuccess) return fail(e);
    if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return fail(e);
    const size_t at = (size_t)db * s->PW + o0;
    if (out->words && nw && (e = hipMemcpy(out->words, s->db + 4 * at, 4 * (size_t)nw, hipMemcpyDeviceToHost)) != hipSuccess) return fail(e);
    if (out->values && nw && (e = hipMemcpy(out->values, s->db + s->d_v + 8 * at, 8 * (size_t)nw, hipMemcpyDeviceToHost)) != hipSuccess) return fail(e);
    out->n_words = nw;
    return VG_OK;
}

extern "C" int vg_kf_loop_detect(vg_handle* h, int n, const vg_bow_in* in, vg_bow_out* out) {
    VG_RANGE("vg_kf_loop_detect");
    if (!h) return VG_ERR_BAD_ARG;
    BowState* s = (BowState*)h->bow;
    KfState* kf = (KfState*)h->kf;
    auto bad = [&](int r, const char* what) { h->err = "vg_kf_loop_detect: request " + std::to_string(r) + ": " + what; return VG_ERR_BAD_ARG; };
    if (!s || !s->voc) { h->err = "vg_kf_loop_detect: the handle has no vocabulary (vg_voc_load)"; return VG_ERR_BAD_ARG; }
    if (!s->db) { h->err = "vg_kf_loop_detect: the handle has no databases (vg_bow_configure)"; return VG_ERR_BAD_ARG; }
    if (!kf) { h->err = "vg_kf_loop_detect: the handle has no keyframe records (vg_kf_configure)"; return VG_ERR_BAD_ARG; }
    if (n <= 0 || !in || !out) { h->err = "vg_kf_loop_detect: n <= 0 or a NULL argument"; return VG_ERR_BAD_ARG; }
    // ---- everything that follows from the arguments and the host's mirror, before anything is uploaded or written
    std::vector<char> seen((size_t)s->n_db, 0);
    int stride = 1, emax = 1;
    bool taps = false;
    for (int r = 0; r < n; ++r) {
        const vg_bow_in& a = in[r];
        if (a.struct_size != (int)sizeof(vg_bow_in)) return bad(r, "vg_bow_in::struct_size");
        if (out[r].struct_size != (int)sizeof(vg_bow_out)) return bad(r, "vg_bow_out::struct_size");
        if ((a.flags & ~(VG_BOW_QUERY | VG_BOW_ADD)) || !(a.flags & (VG_BOW_QUERY | VG_BOW_ADD))) return bad(r, "flags");
        if (a.db < 0 || a.db >= s->n_db) return bad(r, "db out of range");
        if (seen[a.db]) return bad(r, "the database appears twice in the call");
        seen[a.db] = 1;
        if (a.slot < 0 || a.slot >= kf->NS) return bad(r, "slot out of range");
        if (!kf->filled[a.slot]) return bad(r, "the slot was never filled");
        const std::vector<int>& off = s->off[a.db];
        const int ne = (int)off.size() - 1, nk = kf->kept[a.slot];
        if (a.flags & VG_BOW_ADD) {
            if (ne >= s->ME) return bad(r, "the database is full (max_entries)");
            if (s->PW - off.back() < nk) return bad(r, "fewer free pool words than the record has keypoints");
        }
        stride = std::max(stride, nk); emax = std::max(emax, ne);
        taps = taps || out[r].word_of_keypoint || out[r].bow_word || out[r].bow_value;
    }
    hipError_t e = hipSetDevice(h->device);
    auto fail = [&](hipError_t err) { h->err = std::string("vg_kf_loop_detect: ") + hipGetErrorString(err); return VG_ERR_HIP; };
    if (e != hipSuccess) return fail(e);
    stride = (stride + 3) / 4 * 4;
    int sort_stride = 0;
    if (stride > BOW_SORT_LDS) { sort_stride = 1; while (sort_stride < stride) sort_stride <<= 1; }
    // scratch: [requests | score | has | sorted || hdr | outd | wok | sw | sv]; what follows || comes down (the three lists only for the taps)
    const size_t N = (size_t)n, S = (size_t)stride;
    const size_t b_score = kf_up(32 * N), b_has = kf_up(b_score + 8 * N * emax), b_sorted = kf_up(b_has + 4 * N * emax),
                 b_hdr = kf_up(b_sorted + 4 * N * sort_stride), b_outd = b_hdr + kf_up(4 * BOW_HDR * N), b_wok = b_outd + kf_up(32 * N),
                 b_sw = b_wok + kf_up(4 * N * S), b_sv = b_sw + kf_up(4 * N * S), n_all = b_sv + kf_up(8 * N * S);
    const size_t n_down = (taps ? n_all : b_wok) - b_hdr;
    if (n_all > s->buf_cap) {                               // (half as much again: a database that grows by an entry per call must not reallocate per call)
        if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return fail(e);
        (void)hipFree(s->buf);
        s->buf = nullptr; s->buf_cap = 0;
        const size_t cap = n_all + n_all / 2;
        if ((e = hipMalloc((void**)&s->buf, cap)) != hipSuccess) return fail(e);
        s->buf_cap = cap;
    }
    if ((e = s->h_up.resize(32 * N)) != hipSuccess) return fail(e);
    if ((e = s->h_down.resize(n_down)) != hipSuccess) return fail(e);
    int* rq = (int*)s->h_up.data();
    for (int r = 0; r < n; ++r) {
        int* q = rq + 8 * r;
        q[0] = in[r].db; q[1] = in[r].slot; q[2] = in[r].frame_index; q[3] = in[r].flags; q[4] = (int)s->off[in[r].db].size() - 1; q[5] = q[6] = q[7] = 0;
    }
    BowDev b;
    b.n = n; b.stride = stride; b.sort_stride = sort_stride; b.emax = emax; b.ME = s->ME; b.PW = s->PW;
    b.rec_bytes = kf->rec_bytes; b.r_desc = kf->r_desc; b.rec = kf->rec;
    b.vdesc = (const unsigned long long*)s->voc; b.vkid = (const int2*)(s->voc + s->v_kid); b.vweight = (const double*)(s->voc + s->v_weight);
    b.pool_w = (unsigned*)s->db; b.pool_v = (double*)(s->db + s->d_v); b.off = (int*)(s->db + s->d_off);
    char* base = s->buf;
    b.req = (const int*)base; b.score = (double*)(base + b_score); b.has = (int*)(base + b_has); b.sorted = (unsigned*)(base + b_sorted);
    b.hdr = (int*)(base + b_hdr); b.outd = (double*)(base + b_outd); b.wok = (unsigned*)(base + b_wok); b.sw = (unsigned*)(base + b_sw); b.sv = (double*)(base + b_sv);
    if ((e = hipMemcpyAsync(base, rq, 32 * N, hipMemcpyHostToDevice, h->stream)) != hipSuccess) return fail(e);
    struct Events {                                         // destroyed on every way out
        hipEvent_t ev[VG_BOW_LAUNCHES + 1] = {};
        ~Events() { for (hipEvent_t v : ev) if (v) (void)hipEventDestroy(v); }
    } evs;
    const bool timed = out[0].device_ms != nullptr;
    if (timed)
        for (int i = 0; i <= VG_BOW_LAUNCHES; ++i)
            if ((e = hipEventCreate(&evs.ev[i])) != hipSuccess) return fail(e);
    int mark = 0;
    auto stamp = [&]() { return timed ? hipEventRecord(evs.ev[mark++], h->stream) : hipSuccess; };
    if ((e = stamp()) != hipSuccess) return fail(e);
    hipLaunchKernelGGL(bow_walk_kernel, dim3((stride + 256 / BOW_GROUP - 1) / (256 / BOW_GROUP), n), dim3(256), 0, h->stream, b);
    if ((e = stamp()) != hipSuccess) return fail(e);
    hipLaunchKernelGGL(bow_vector_kernel, dim3(n), dim3(BOW_VEC_THREADS), 0, h->stream, b);
    if ((e = stamp()) != hipSuccess) return fail(e);
    hipLaunchKernelGGL(bow_score_kernel, dim3((emax + 3) / 4, n), dim3(256), 0, h->stream, b);
    if ((e = stamp()) != hipSuccess) return fail(e);
    hipLaunchKernelGGL(bow_tail_kernel, dim3(n), dim3(64), 0, h->stream, b);
    if ((e = stamp()) != hipSuccess) return fail(e);
    if ((e = hipGetLastError()) != hipSuccess) return fail(e);
    char* down = s->h_down.data();
    if ((e = hipMemcpyAsync(down, base + b_hdr, n_down, hipMemcpyDeviceToHost, h->stream)) != hipSuccess) return fail(e);
    if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return fail(e);
    if (timed)
        for (int i = 0; i < VG_BOW_LAUNCHES; ++i) {
            float ms = 0.f;
            if ((e = hipEventElapsedTime(&ms, evs.ev[i], evs.ev[i + 1])) != hipSuccess) return fail(e);
            out[0].device_ms[i] = ms;
        }
    for (int r = 0; r < n; ++r) {
        const int* hd = (const int*)down + BOW_HDR * r;
        const double* od = (const double*)(down + (b_outd - b_hdr)) + 4 * r;
        vg_bow_out& o = out[r];
        o.n_words = hd[0]; o.n_results = hd[1]; o.find_loop = hd[6]; o.loop_index = hd[7]; o.entry_id = hd[8];
        for (int k = 0; k < VG_BOW_MAX_RESULTS; ++k) { o.ids[k] = hd[2 + k]; o.scores[k] = od[k]; }
        if (in[r].flags & VG_BOW_ADD) { std::vector<int>& off = s->off[in[r].db]; off.push_back(off.back() + hd[0]); }
        const size_t nk = (size_t)kf->kept[in[r].slot], nw = (size_t)hd[0];
        if (o.word_of_keypoint && nk) memcpy(o.word_of_keypoint, down + (b_wok - b_hdr) + 4 * S * r, 4 * nk);
        if (o.bow_word && nw) memcpy(o.bow_word, down + (b_sw - b_hdr) + 4 * S * r, 4 * nw);
        if (o.bow_value && nw) memcpy(o.bow_value, down + (b_sv - b_hdr) + 8 * S * r, 8 * nw);
    }
    return VG_OK;
}
