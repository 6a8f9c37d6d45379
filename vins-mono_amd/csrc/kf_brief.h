// kf_brief.h — vg_kf_*: the integer-exact part of the pose graph's KeyFrame (pose_graph/src/keyframe.cpp) for a batch of keyframes:
// computeWindowBRIEFPoint, computeBRIEFPoint with keypoints_norm (vg_kf_add), searchByBRIEFDes with findConnection's reduceVector step
// (vg_kf_match), and the resident records between the two (vg_kf_configure / _get / _set).  include/vinsgpu.h defines every stage; this
// file is the device code and the host entries.  It is included at the END of fe_ransac.hip (after init_exrot.h), compiled with
// -ffp-contract=off like the rest of the unit: the lift is fe_camera.h's, the one vg_fe_lift runs.
//
// RECALLED, NOT PINNED: cv::GaussianBlur's fixed-point 9x9 path and cv::FAST(20, true) with cornerScore<16> are written from the
// statement in include/vinsgpu.h; there is no OpenCV to compare with.  DVision::BRIEF::compute is read from the reference.
//
// A RECORD is one block of rec_bytes per slot: counts (n_keypoints kept, n_window, true corner count, filled) | descriptors [MK][4] |
// pt [MK][2] | norm [MK][2] | window descriptors [MW][4] | window pt [MW][2] | scores [MK].  vg_kf_get / vg_kf_set move it whole.
//
// vg_kf_add, seven launches over the batch between one upload and one download:
//   kf_blur_kernel     64 x 32 tile + 4-pixel halo in LDS (uint8), the row pass into LDS (uint16), the column pass out (uint8)
//   kf_fast_kernel     64 x 32 tile + 3-pixel halo in LDS, a thread takes 8 pixels: A / B by min / max doubling over the 16 differences
//   kf_nms_kernel      a wavefront per SEGMENT of 64 consecutive pixels in row-major order: the ballot of "kept" is the segment's mask
//                      (a wavefront walks KF_SEGS segments: a workgroup per four segments is bound by the dispatch rate, not by HBM)
//   kf_scan_kernel     a workgroup per frame: exclusive scan of the masks' popcounts, the record's counts, the window points
//   kf_scatter_kernel  a wavefront per segment: rank = segment offset + popcount of the lower lanes; pt and score
//   kf_lift_kernel     a thread per kept corner: keypoints_norm
//   kf_brief_kernel    a wavefront per point (window points, then corners): lane l takes tests 64 r + l, the four ballots are the words
// No atomic decides an order anywhere.  vg_kf_match is one launch, a workgroup per pair.
#pragma once
#include <cstring>

#define KF_TW 64
#define KF_TH 32
#define KF_SEGS 8                     // segments a wavefront of the non-max and scatter kernels walks
#define KF_ITEMS 4                    // points a wavefront of the BRIEF kernel walks
#define KF_MATCH_THREADS 512
#define KF_CHUNK 512                  // old descriptors staged in LDS at a time (16 KB)
#define KF_NONE ((128u << 16) | 0xFFFFu)

struct KfDev {
    int W, H, n, MK, MW, nseg;
    unsigned rec_bytes, r_desc, r_pt, r_norm, r_wdesc, r_wpt, r_score;
    char* rec;                        // [n_slots][rec_bytes]
    const short* pat;                 // [256][4] x1 y1 x2 y2 of test i (interleaved at vg_kf_configure)
    const FeCamera* cam;              // [n]
    const int* slot;                  // [n]
    const int* nwin;                  // [n]
    const float* wxy;                 // [n][MW][2]
    const uint8_t* img;               // [n][H][W]
    uint8_t* blur;
    uint8_t* score;
    unsigned long long* mask;         // [n][nseg]
    int* segoff;                      // [n][nseg]
    int* hdr;                         // [n][4] true count, status, kept, n_window
    char* stage;                      // [n][rec_bytes] (or null)
};

// BORDER_REFLECT_101 for an index up to 4 outside [0, n), n >= 7; clamped beyond (a tile that hangs over the edge: never stored)
DEV int kf_reflect(int i, int n) {
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * n - 2 - i : i;
    return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

extern "C" __global__ __launch_bounds__(256) void kf_blur_kernel(KfDev b) {
    __shared__ uint8_t raw[KF_TH + 8][KF_TW + 8];
    __shared__ unsigned short hs[KF_TH + 8][KF_TW];
    const int tid = threadIdx.x, x0 = blockIdx.x * KF_TW, y0 = blockIdx.y * KF_TH, W = b.W, H = b.H;
    const size_t frame = (size_t)blockIdx.z * W * H;
    const uint8_t* __restrict__ img = b.img + frame;
    for (int i = tid; i < (KF_TH + 8) * (KF_TW + 8); i += 256) {
        const int r = i / (KF_TW + 8), c = i % (KF_TW + 8);
        raw[r][c] = img[(size_t)kf_reflect(y0 + r - 4, H) * W + kf_reflect(x0 + c - 4, W)];
    }
    __syncthreads();
    const int k[9] = {7, 17, 32, 46, 52, 46, 32, 17, 7};
    for (int i = tid; i < (KF_TH + 8) * KF_TW; i += 256) {
        const int r = i / KF_TW, c = i % KF_TW;
        int s = 0;
#pragma unroll
        for (int j = 0; j < 9; ++j) s += k[j] * (int)raw[r][c + j];
        hs[r][c] = (unsigned short)s;                          // at most 255 * 256
    }
    __syncthreads();
    for (int i = tid; i < KF_TH * KF_TW; i += 256) {
        const int r = i / KF_TW, c = i % KF_TW;
        int s = 0;
#pragma unroll
        for (int j = 0; j < 9; ++j) s += k[j] * (int)hs[r + j][c];
        if (x0 + c < W && y0 + r < H) b.blur[frame + (size_t)(y0 + r) * W + (x0 + c)] = (uint8_t)((s + 32768) >> 16);
    }
}

// max over the 16 arcs of 9 contiguous ring entries of the arc's minimum, by doubling: m2 m4 m8 then the ninth
DEV int kf_arc_max_min(const int* d) {
    int m2[16], m4[16], best = -255;
#pragma unroll
    for (int i = 0; i < 16; ++i) m2[i] = min(d[i], d[(i + 1) & 15]);
#pragma unroll
    for (int i = 0; i < 16; ++i) m4[i] = min(m2[i], m2[(i + 2) & 15]);
#pragma unroll
    for (int i = 0; i < 16; ++i) best = max(best, min(min(m4[i], m4[(i + 4) & 15]), d[(i + 8) & 15]));
    return best;
}

extern "C" __global__ __launch_bounds__(256) void kf_fast_kernel(KfDev b) {
    __shared__ uint8_t t[KF_TH + 6][KF_TW + 8];
    const int tid = threadIdx.x, x0 = blockIdx.x * KF_TW, y0 = blockIdx.y * KF_TH, W = b.W, H = b.H;
    const size_t frame = (size_t)blockIdx.z * W * H;
    const uint8_t* __restrict__ img = b.img + frame;
    for (int i = tid; i < (KF_TH + 6) * (KF_TW + 6); i += 256) {
        const int r = i / (KF_TW + 6), c = i % (KF_TW + 6);
        const int y = min(max(y0 + r - 3, 0), H - 1), x = min(max(x0 + c - 3, 0), W - 1);     // (clamped: only interior pixels are scored)
        t[r][c] = img[(size_t)y * W + x];
    }
    __syncthreads();
    const int c = tid & 63;
#pragma unroll 1
    for (int q = 0; q < KF_TH / 4; ++q) {
        const int r = (tid >> 6) + 4 * q, x = x0 + c, y = y0 + r;
        if (x >= W || y >= H) continue;
        int s = 0;
        if (x >= 3 && x < W - 3 && y >= 3 && y < H - 3) {
            const int v = t[r + 3][c + 3];
            const int dx[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
            const int dy[16] = {-3, -3, -2, -1, 0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3};
            int d[16], e[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) { d[i] = v - (int)t[r + 3 + dy[i]][c + 3 + dx[i]]; e[i] = -d[i]; }
            const int m = max(kf_arc_max_min(d), kf_arc_max_min(e));
            s = m > 20 ? m - 1 : 0;
        }
        b.score[frame + (size_t)y * W + x] = (uint8_t)s;
    }
}

extern "C" __global__ __launch_bounds__(256) void kf_nms_kernel(KfDev b) {
    const int lane = threadIdx.x & 63, W = b.W, H = b.H;
    const uint8_t* __restrict__ sc = b.score + (size_t)blockIdx.y * W * H;
    const int seg0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * KF_SEGS;
#pragma unroll 1
    for (int q = 0; q < KF_SEGS; ++q) {
        const int seg = seg0 + q;
        if (seg >= b.nseg) return;                              // (the whole wavefront)
        const int p = seg * 64 + lane;
        bool keep = false;
        if (p < W * H) {
            const int s = sc[p];
            if (s > 0) {                                        // a scored pixel is 3 or more inside: its neighbours exist
                const uint8_t* a = sc + p - W;
                const uint8_t* c = sc + p + W;
                keep = s > a[-1] && s > a[0] && s > a[1] && s > sc[p - 1] && s > sc[p + 1] && s > c[-1] && s > c[0] && s > c[1];
            }
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) b.mask[(size_t)blockIdx.y * b.nseg + seg] = m;
    }
}

extern "C" __global__ __launch_bounds__(256) void kf_scan_kernel(KfDev b) {
    __shared__ int sums[256];
    const int tid = threadIdx.x, e = blockIdx.x, nseg = b.nseg;
    const unsigned long long* __restrict__ mk = b.mask + (size_t)e * nseg;
    int* off = b.segoff + (size_t)e * nseg;
    const int chunk = (nseg + 255) / 256, lo = min(tid * chunk, nseg), hi = min(lo + chunk, nseg);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += __popcll(mk[i]);
    sums[tid] = s;
    __syncthreads();
    int base = 0, total = 0;
    for (int i = 0; i < 256; ++i) { const int v = sums[i]; base += i < tid ? v : 0; total += v; }
    for (int i = lo; i < hi; ++i) { off[i] = base; base += __popcll(mk[i]); }
    char* rec = b.rec + (size_t)b.slot[e] * b.rec_bytes;
    const int nw = b.nwin[e];
    float* wpt = (float*)(rec + b.r_wpt);
    for (int i = tid; i < 2 * nw; i += 256) wpt[i] = b.wxy[(size_t)e * b.MW * 2 + i];
    if (tid == 0) {
        const int kept = min(total, b.MK);
        int* cnt = (int*)rec;
        cnt[0] = kept; cnt[1] = nw; cnt[2] = total; cnt[3] = 1;
        int* hd = b.hdr + 4 * e;
        hd[0] = total; hd[1] = total > b.MK ? VG_KF_TRUNCATED : VG_KF_OK; hd[2] = kept; hd[3] = nw;
    }
}

extern "C" __global__ __launch_bounds__(256) void kf_scatter_kernel(KfDev b) {
    const int lane = threadIdx.x & 63, e = blockIdx.y, W = b.W;
    const int seg0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * KF_SEGS;
    char* rec = b.rec + (size_t)b.slot[e] * b.rec_bytes;
#pragma unroll 1
    for (int q = 0; q < KF_SEGS; ++q) {
        const int seg = seg0 + q;
        if (seg >= b.nseg) return;
        const unsigned long long m = b.mask[(size_t)e * b.nseg + seg];
        if (!((m >> lane) & 1ull)) continue;
        const int rank = b.segoff[(size_t)e * b.nseg + seg] + __popcll(m & ((1ull << lane) - 1ull));
        if (rank >= b.MK) continue;
        const int p = seg * 64 + lane;
        float* pt = (float*)(rec + b.r_pt) + 2 * rank;
        pt[0] = (float)(p % W); pt[1] = (float)(p / W);
        ((uint8_t*)(rec + b.r_score))[rank] = b.score[(size_t)e * W * b.H + p];
    }
}

// keypoints_norm: a thread per kept corner (dense: the scatter's lanes are one in sixty-four)
extern "C" __global__ __launch_bounds__(256) void kf_lift_kernel(KfDev b) {
    const int k = blockIdx.x * 256 + threadIdx.x, e = blockIdx.y;
    char* rec = b.rec + (size_t)b.slot[e] * b.rec_bytes;
    if (k >= ((const int*)rec)[0]) return;
    const float* pt = (const float*)(rec + b.r_pt) + 2 * k;
    float* nm = (float*)(rec + b.r_norm) + 2 * k;
    const FeCamera cam = b.cam[e];
    float nx, ny;
    fe_cam_lift_xy(cam, pt[0], pt[1], nx, ny);
    nm[0] = nx; nm[1] = ny;
}

// (int)(f) is inside [0, n) exactly when -1 < f < n (truncation toward zero); -1 for everything else, a NaN included
DEV int kf_coord(float f, int n) { return (f > -1.0f && f < (float)n) ? (int)f : -1; }

// (Measured: copying the point's window of the blurred image into LDS first, a row per load, took 2.2 ms where these gathers take
// 1.1 ms for 256 frames: the gathers stay.)
extern "C" __global__ __launch_bounds__(256) void kf_brief_kernel(KfDev b) {
    const int lane = threadIdx.x & 63, e = blockIdx.y, W = b.W, H = b.H;
    char* rec = b.rec + (size_t)b.slot[e] * b.rec_bytes;
    const int* cnt = (const int*)rec;
    const uint8_t* __restrict__ im = b.blur + (size_t)e * W * H;
    const short4* __restrict__ pat = (const short4*)b.pat;      // [256] x1 y1 x2 y2
    const int item0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * KF_ITEMS;
#pragma unroll 1
    for (int q = 0; q < KF_ITEMS; ++q) {
        const int item = item0 + q;
        const float* pt;
        unsigned long long* dst;
        if (item < b.MW) {
            if (item >= cnt[1]) continue;                       // (the whole wavefront)
            pt = (const float*)(rec + b.r_wpt) + 2 * item;
            dst = (unsigned long long*)(rec + b.r_wdesc) + 4 * item;
        } else {
            const int k = item - b.MW;
            if (k >= cnt[0]) return;
            pt = (const float*)(rec + b.r_pt) + 2 * k;
            dst = (unsigned long long*)(rec + b.r_desc) + 4 * k;
        }
        const float px = pt[0], py = pt[1];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const short4 t = pat[64 * r + lane];
            const int x1 = kf_coord(px + (float)t.x, W), y1 = kf_coord(py + (float)t.y, H);
            const int x2 = kf_coord(px + (float)t.z, W), y2 = kf_coord(py + (float)t.w, H);
            bool bit = false;
            if ((x1 | y1 | x2 | y2) >= 0) bit = im[(size_t)y1 * W + x1] < im[(size_t)y2 * W + x2];
            const unsigned long long word = __ballot(bit);
            if (lane == 0) dst[r] = word;
        }
    }
}

// the records of the batch, whole, one after another (the download of an entry that asks for its arrays)
extern "C" __global__ __launch_bounds__(256) void kf_gather_kernel(KfDev b) {
    const uint4* src = (const uint4*)(b.rec + (size_t)b.slot[blockIdx.y] * b.rec_bytes);
    uint4* dst = (uint4*)(b.stage + (size_t)blockIdx.y * b.rec_bytes);
    const unsigned i = blockIdx.x * 256 + threadIdx.x;
    if (i < b.rec_bytes / 16) dst[i] = src[i];
}

struct KfMatchDev {
    int MW;
    unsigned rec_bytes, r_desc, r_pt, r_norm, r_wdesc;
    const char* rec;
    const int* pairs;                 // [np][2] current slot, old slot
    int* out;                         // [np][4 + 12 MW]: n_window n_matched - - | best_idx | best_dist | status | m2d 2 | m2dn 2 | index | c2d 2 | c2dn 2
};

// A workgroup per pair.  The old record's descriptors pass through LDS once, KF_CHUNK at a time, word-major (a lane's four 64-bit reads
// are bank-conflict free); a wavefront takes window descriptor w, w + 8, ...: its lanes stride over the chunk, the key (distance << 16) |
// index goes through a butterfly minimum.  Then the statuses, and the survivors' ranks by a ballot prefix within the workgroup.
extern "C" __global__ __launch_bounds__(KF_MATCH_THREADS) void kf_match_kernel(KfMatchDev b) {
    __shared__ unsigned long long od[4 * KF_CHUNK];
    __shared__ unsigned best[VG_KF_MAX_WINDOW];
    __shared__ int wcnt[KF_MATCH_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, p = blockIdx.x, MW = b.MW;
    const char* cur = b.rec + (size_t)b.pairs[2 * p] * b.rec_bytes;
    const char* old = b.rec + (size_t)b.pairs[2 * p + 1] * b.rec_bytes;
    const int nw = ((const int*)cur)[1], nk = ((const int*)old)[0];
    const unsigned long long* __restrict__ wdesc = (const unsigned long long*)(cur + b.r_wdesc);
    const unsigned long long* __restrict__ odesc = (const unsigned long long*)(old + b.r_desc);
    for (int w = tid; w < nw; w += KF_MATCH_THREADS) best[w] = KF_NONE;
    __syncthreads();
    for (int c0 = 0; c0 < nk; c0 += KF_CHUNK) {
        const int m = min(KF_CHUNK, nk - c0);
        for (int i = tid; i < 4 * m; i += KF_MATCH_THREADS) od[(i & 3) * KF_CHUNK + (i >> 2)] = odesc[4 * (size_t)c0 + i];
        __syncthreads();
        for (int w = wave; w < nw; w += KF_MATCH_THREADS / 64) {
            const unsigned long long w0 = wdesc[4 * w], w1 = wdesc[4 * w + 1], w2 = wdesc[4 * w + 2], w3 = wdesc[4 * w + 3];
            unsigned key = KF_NONE;
            for (int j = lane; j < m; j += 64) {
                const int dist = __popcll(w0 ^ od[j]) + __popcll(w1 ^ od[KF_CHUNK + j]) + __popcll(w2 ^ od[2 * KF_CHUNK + j]) + __popcll(w3 ^ od[3 * KF_CHUNK + j]);
                key = min(key, ((unsigned)dist << 16) | (unsigned)(c0 + j));
            }
#pragma unroll
            for (int h = 32; h >= 1; h >>= 1) key = min(key, (unsigned)__shfl_xor((int)key, h));
            if (lane == 0) best[w] = min(best[w], key);
        }
        __syncthreads();
    }
    int* out = b.out + (size_t)p * (4 + 12 * MW);
    int* o_idx = out + 4;
    int* o_dist = o_idx + MW;
    int* o_st = o_dist + MW;
    float* o_m = (float*)(o_st + MW);
    float* o_mn = o_m + 2 * MW;
    int* o_ci = (int*)(o_mn + 2 * MW);
    float* o_c = (float*)(o_ci + MW);
    float* o_cn = o_c + 2 * MW;
    const float* opt = (const float*)(old + b.r_pt);
    const float* onm = (const float*)(old + b.r_norm);
    int base = 0;
    for (int w0 = 0; w0 < nw; w0 += KF_MATCH_THREADS) {
        const int w = w0 + tid;
        const bool valid = w < nw;
        const unsigned key = valid ? best[w] : KF_NONE;
        const int idx = (key >> 16) < 128u ? (int)(key & 0xFFFFu) : -1;
        const int dist = idx >= 0 ? (int)(key >> 16) : 128;
        const bool st = valid && idx >= 0 && dist < 80;
        const unsigned long long bal = __ballot(st);
        if (lane == 0) wcnt[wave] = __popcll(bal);
        __syncthreads();
        int pre = base + __popcll(bal & ((1ull << lane) - 1ull)), tot = 0;
        for (int q = 0; q < KF_MATCH_THREADS / 64; ++q) { const int v = wcnt[q]; pre += q < wave ? v : 0; tot += v; }
        if (valid) {
            const float mx = st ? opt[2 * idx] : 0.f, my = st ? opt[2 * idx + 1] : 0.f, nx = st ? onm[2 * idx] : 0.f, ny = st ? onm[2 * idx + 1] : 0.f;
            o_idx[w] = idx; o_dist[w] = dist; o_st[w] = st ? 1 : 0;
            o_m[2 * w] = mx; o_m[2 * w + 1] = my; o_mn[2 * w] = nx; o_mn[2 * w + 1] = ny;
            if (st) { o_ci[pre] = w; o_c[2 * pre] = mx; o_c[2 * pre + 1] = my; o_cn[2 * pre] = nx; o_cn[2 * pre + 1] = ny; }
        }
        base += tot;
        __syncthreads();
    }
    if (tid == 0) { out[0] = nw; out[1] = base; out[2] = 0; out[3] = 0; }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
struct KfState {
    int W = 0, H = 0, MK = 0, MW = 0, NS = 0, nseg = 0;
    unsigned rec_bytes = 0, r_desc = 0, r_pt = 0, r_norm = 0, r_wdesc = 0, r_wpt = 0, r_score = 0;
    char* rec = nullptr;              // the records, then the pattern
    short* pat = nullptr;
    std::vector<char> filled;
    std::vector<int> kept;            // per slot: the record's n_keypoints as the host last saw it (vg_kf_add / vg_kf_set; kf_bow.h sizes by it)
    char* buf = nullptr;              // scratch of vg_kf_add / vg_kf_match, grown on demand
    size_t buf_cap = 0;
    PinnedBuf<char> h_up, h_down;
};

extern "C" void kf_release(vg_handle* h) {
    KfState* s = (KfState*)h->kf;
    if (!s) return;
    (void)hipFree(s->rec);
    (void)hipFree(s->buf);
    s->h_up.release(); s->h_down.release();
    delete s;
    h->kf = nullptr;
}

static size_t kf_up(size_t v) { return (v + 255) / 256 * 256; }

static hipError_t kf_scratch(KfState* s, size_t need) {
    if (need <= s->buf_cap) return hipSuccess;
    (void)hipFree(s->buf);
    s->buf = nullptr; s->buf_cap = 0;
    const hipError_t e = hipMalloc((void**)&s->buf, need);
    if (e == hipSuccess) s->buf_cap = need;
    return e;
}

extern "C" int vg_kf_configure(vg_handle* h, int width, int height, int max_keypoints, int max_window_points, int n_slots, const int16_t* pattern) {
    if (!h) return VG_ERR_BAD_ARG;
    auto bad = [&](const char* what) { h->err = std::string("vg_kf_configure: ") + what; return VG_ERR_BAD_ARG; };
    if (width < 7 || height < 7) return bad("width or height below 7");
    if ((long long)width * height > 0x3fffffffLL) return bad("the frame is too large");
    if (max_keypoints < 1 || max_keypoints > VG_KF_MAX_KEYPOINTS) return bad("max_keypoints outside 1 .. VG_KF_MAX_KEYPOINTS");
    if (max_window_points < 1 || max_window_points > VG_KF_MAX_WINDOW) return bad("max_window_points outside 1 .. VG_KF_MAX_WINDOW");
    if (n_slots < 1) return bad("n_slots < 1");
    if (!pattern) return bad("pattern is NULL");
    for (int i = 0; i < 1024; ++i)
        if (pattern[i] < -127 || pattern[i] > 127) return bad("a pattern offset outside +-127");
    hipError_t e = hipSetDevice(h->device);
    auto fail = [&](hipError_t err) { h->err = std::string("vg_kf_configure: ") + hipGetErrorString(err); return VG_ERR_HIP; };
    if (e != hipSuccess) return fail(e);
    if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return fail(e);
    kf_release(h);
    KfState* s = new KfState();
    s->W = width; s->H = height; s->MK = max_keypoints; s->MW = max_window_points; s->NS = n_slots;
    s->nseg = (width * height + 63) / 64;
    const unsigned MK = (unsigned)max_keypoints, MW = (unsigned)max_window_points;
    s->r_desc = 16; s->r_pt = s->r_desc + 32 * MK; s->r_norm = s->r_pt + 8 * MK; s->r_wdesc = s->r_norm + 8 * MK;
    s->r_wpt = s->r_wdesc + 32 * MW; s->r_score = s->r_wpt + 8 * MW;
    s->rec_bytes = (s->r_score + MK + 15) / 16 * 16;
    const size_t recs = kf_up((size_t)s->rec_bytes * n_slots);
    if ((e = hipMalloc((void**)&s->rec, recs + 1024 * sizeof(short))) != hipSuccess) { delete s; return fail(e); }
    s->pat = (short*)(s->rec + recs);
    h->kf = s;
    s->filled.assign(n_slots, 0);
    s->kept.assign(n_slots, 0);
    if ((e = hipMemsetAsync(s->rec, 0, recs, h->stream)) != hipSuccess) return fail(e);
    short pat4[1024];                                       // test i: x1 y1 x2 y2 side by side, one 8-byte load
    for (int i = 0; i < 256; ++i)
        for (int k = 0; k < 4; ++k) pat4[4 * i + k] = pattern[256 * k + i];
    if ((e = hipMemcpyAsync(s->pat, pat4, sizeof(pat4), hipMemcpyHostToDevice, h->stream)) != hipSuccess) return fail(e);
    if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return fail(e);
    return VG_OK;
}

// what the host reads of a record block
struct KfView {
    const int* cnt; const unsigned long long* desc; const float* pt; const float* norm; const unsigned long long* wdesc; const float* wpt; const uint8_t* score;
    KfView(const KfState* s, const char* r)
        : cnt((const int*)r), desc((const unsigned long long*)(r + s->r_desc)), pt((const float*)(r + s->r_pt)), norm((const float*)(r + s->r_norm)),
          wdesc((const unsigned long long*)(r + s->r_wdesc)), wpt((const float*)(r + s->r_wpt)), score((const uint8_t*)(r + s->r_score)) {}
};

extern "C" int vg_kf_add(vg_handle* h, int n, const vg_kf_in* in, vg_kf_out* out) {
    VG_RANGE("vg_kf_add");
    if (!h) return VG_ERR_BAD_ARG;
    KfState* s = (KfState*)h->kf;
    auto bad = [&](int e, const char* what) { h->err = "vg_kf_add: entry " + std::to_string(e) + ": " + what; return VG_ERR_BAD_ARG; };
    if (!s) { h->err = "vg_kf_add: the handle has no keyframe records (vg_kf_configure)"; return VG_ERR_BAD_ARG; }
    if (n <= 0 || !in || !out) { h->err = "vg_kf_add: n <= 0 or a NULL argument"; return VG_ERR_BAD_ARG; }
    const int W = s->W, H = s->H, MK = s->MK, MW = s->MW;
    // ---- everything that follows from the arguments alone, before anything is uploaded or written
    std::vector<FeCamera> cams((size_t)n);
    std::vector<char> seen((size_t)s->NS, 0);
    bool want = false;
    for (int e = 0; e < n; ++e) {
        const vg_kf_in& a = in[e];
        if (a.struct_size != (int)sizeof(vg_kf_in)) return bad(e, "vg_kf_in::struct_size");
        if (out[e].struct_size != (int)sizeof(vg_kf_out)) return bad(e, "vg_kf_out::struct_size");
        if (a.slot < 0 || a.slot >= s->NS) return bad(e, "slot out of range");
        if (seen[a.slot]) return bad(e, "the slot appears twice in the call");
        seen[a.slot] = 1;
        if (!a.img) return bad(e, "a NULL image");
        if (a.stride < W) return bad(e, "stride below the width");
        if (a.n_window < 0 || a.n_window > MW) return bad(e, "n_window above max_window_points");
        if (a.n_window > 0 && !a.window_xy) return bad(e, "a NULL window_xy");
        if (const char* why = fe_camera_check(&a.camera, &cams[e])) return bad(e, why);
        want = want || out[e].keypoints_xy || out[e].scores || out[e].norm_xy || out[e].descriptors || out[e].window_descriptors;
    }
    hipError_t e = hipSetDevice(h->device);
    auto fail = [&](hipError_t err) { h->err = std::string("vg_kf_add: ") + hipGetErrorString(err); return VG_ERR_HIP; };
    if (e != hipSuccess) return fail(e);
    const size_t WH = (size_t)W * H, nseg = (size_t)s->nseg;
    // upload: [cameras | slots | n_window | window points | images]; behind it the scratch
    const size_t u_cam = 0, u_slot = kf_up(u_cam + sizeof(FeCamera) * n), u_nw = u_slot + 4 * (size_t)n, u_wxy = kf_up(u_nw + 4 * (size_t)n),
                 u_img = kf_up(u_wxy + 8 * (size_t)MW * n), n_up = kf_up(u_img + WH * n);
    const size_t b_blur = n_up, b_score = kf_up(b_blur + WH * n), b_mask = kf_up(b_score + WH * n), b_off = kf_up(b_mask + 8 * nseg * n),
                 b_hdr = kf_up(b_off + 4 * nseg * n), b_stage = b_hdr + 16 * (size_t)n, n_all = b_stage + (want ? (size_t)s->rec_bytes * n : 0);
    if ((e = kf_scratch(s, n_all)) != hipSuccess) return fail(e);
    if ((e = s->h_up.resize(n_up)) != hipSuccess) return fail(e);
    const size_t n_down = 16 * (size_t)n + (want ? (size_t)s->rec_bytes * n : 0);
    if ((e = s->h_down.resize(n_down)) != hipSuccess) return fail(e);
    char* up = s->h_up.data();
    memcpy(up + u_cam, cams.data(), sizeof(FeCamera) * n);
    for (int k = 0; k < n; ++k) {
        ((int*)(up + u_slot))[k] = in[k].slot;
        ((int*)(up + u_nw))[k] = in[k].n_window;
        float* w = (float*)(up + u_wxy) + 2 * (size_t)MW * k;
        if (in[k].n_window > 0) memcpy(w, in[k].window_xy, 8 * (size_t)in[k].n_window);
        memset(w + 2 * in[k].n_window, 0, 8 * (size_t)(MW - in[k].n_window));
        char* d = up + u_img + WH * k;
        if (in[k].stride == W) memcpy(d, in[k].img, WH);
        else for (int y = 0; y < H; ++y) memcpy(d + (size_t)y * W, in[k].img + (size_t)y * in[k].stride, W);
    }
    KfDev b;
    b.W = W; b.H = H; b.n = n; b.MK = MK; b.MW = MW; b.nseg = s->nseg;
    b.rec_bytes = s->rec_bytes; b.r_desc = s->r_desc; b.r_pt = s->r_pt; b.r_norm = s->r_norm; b.r_wdesc = s->r_wdesc; b.r_wpt = s->r_wpt; b.r_score = s->r_score;
    b.rec = s->rec; b.pat = s->pat;
    char* base = s->buf;
    b.cam = (const FeCamera*)(base + u_cam); b.slot = (const int*)(base + u_slot); b.nwin = (const int*)(base + u_nw); b.wxy = (const float*)(base + u_wxy);
    b.img = (const uint8_t*)(base + u_img); b.blur = (uint8_t*)(base + b_blur); b.score = (uint8_t*)(base + b_score);
    b.mask = (unsigned long long*)(base + b_mask); b.segoff = (int*)(base + b_off); b.hdr = (int*)(base + b_hdr); b.stage = want ? base + b_stage : nullptr;
    if ((e = hipMemcpyAsync(base, up, n_up, hipMemcpyHostToDevice, h->stream)) != hipSuccess) return fail(e);
    struct Events {                                         // destroyed on every way out
        hipEvent_t ev[VG_KF_ADD_LAUNCHES + 1] = {};
        ~Events() { for (hipEvent_t v : ev) if (v) (void)hipEventDestroy(v); }
    } evs;
    const bool timed = out[0].device_ms != nullptr;
    if (timed)
        for (int i = 0; i <= VG_KF_ADD_LAUNCHES; ++i)
            if ((e = hipEventCreate(&evs.ev[i])) != hipSuccess) return fail(e);
    int mark = 0;
    auto stamp = [&]() { return timed ? hipEventRecord(evs.ev[mark++], h->stream) : hipSuccess; };
    const dim3 tiles((W + KF_TW - 1) / KF_TW, (H + KF_TH - 1) / KF_TH, n), segs((s->nseg + 4 * KF_SEGS - 1) / (4 * KF_SEGS), n);
    if ((e = stamp()) != hipSuccess) return fail(e);
    hipLaunchKernelGGL(kf_blur_kernel, tiles, dim3(256), 0, h->stream, b);
    if ((e = stamp()) != hipSuccess) return fail(e);
    hipLaunchKernelGGL(kf_fast_kernel, tiles, dim3(256), 0, h->stream, b);
    if ((e = stamp()) != hipSuccess) return fail(e);
    hipLaunchKernelGGL(kf_nms_kernel, segs, dim3(256), 0, h->stream, b);
    if ((e = stamp()) != hipSuccess) return fail(e);
    hipLaunchKernelGGL(kf_scan_kernel, dim3(n), dim3(256), 0, h->stream, b);
    if ((e = stamp()) != hipSuccess) return fail(e);
    hipLaunchKernelGGL(kf_scatter_kernel, segs, dim3(256), 0, h->stream, b);
    if ((e = stamp()) != hipSuccess) return fail(e);
    hipLaunchKernelGGL(kf_lift_kernel, dim3((MK + 255) / 256, n), dim3(256), 0, h->stream, b);
    if ((e = stamp()) != hipSuccess) return fail(e);
    hipLaunchKernelGGL(kf_brief_kernel, dim3((MW + MK + 4 * KF_ITEMS - 1) / (4 * KF_ITEMS), n), dim3(256), 0, h->stream, b);
    if ((e = stamp()) != hipSuccess) return fail(e);
    if ((e = hipGetLastError()) != hipSuccess) return fail(e);
    for (int k = 0; k < n; ++k) s->filled[in[k].slot] = 1;
    // the download: the headers and, right behind them, the records when an entry asks for arrays
    if (want) {
        hipLaunchKernelGGL(kf_gather_kernel, dim3((s->rec_bytes / 16 + 255) / 256, n), dim3(256), 0, h->stream, b);
        if ((e = hipGetLastError()) != hipSuccess) return fail(e);
    }
    char* down = s->h_down.data();
    if ((e = hipMemcpyAsync(down, base + b_hdr, n_down, hipMemcpyDeviceToHost, h->stream)) != hipSuccess) return fail(e);
    if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return fail(e);
    if (timed)
        for (int i = 0; i < VG_KF_ADD_LAUNCHES; ++i) {
            float ms = 0.f;
            if ((e = hipEventElapsedTime(&ms, evs.ev[i], evs.ev[i + 1])) != hipSuccess) return fail(e);
            out[0].device_ms[i] = ms;
        }
    const int* hd = (const int*)down;
    for (int k = 0; k < n; ++k) {
        vg_kf_out& o = out[k];
        o.n_keypoints = hd[4 * k]; o.status = hd[4 * k + 1]; o.n_kept = hd[4 * k + 2];
        s->kept[in[k].slot] = o.n_kept;
        if (!want) continue;
        const KfView v(s, down + 16 * (size_t)n + (size_t)s->rec_bytes * k);
        const size_t nk = (size_t)o.n_kept, nw = (size_t)in[k].n_window;
        if (o.keypoints_xy) memcpy(o.keypoints_xy, v.pt, 8 * nk);
        if (o.scores) memcpy(o.scores, v.score, nk);
        if (o.norm_xy) memcpy(o.norm_xy, v.norm, 8 * nk);
        if (o.descriptors) memcpy(o.descriptors, v.desc, 32 * nk);
        if (o.window_descriptors) memcpy(o.window_descriptors, v.wdesc, 32 * nw);
    }
    return VG_OK;
}

extern "C" int vg_kf_get(vg_handle* h, int slot, vg_kf_record* rec) {
    if (!h) return VG_ERR_BAD_ARG;
    KfState* s = (KfState*)h->kf;
    auto bad = [&](const char* what) { h->err = std::string("vg_kf_get: ") + what; return VG_ERR_BAD_ARG; };
    if (!s) return bad("the handle has no keyframe records (vg_kf_configure)");
    if (!rec) return bad("a NULL argument");
    if (rec->struct_size != (int)sizeof(vg_kf_record)) return bad("vg_kf_record::struct_size");
    if (slot < 0 || slot >= s->NS) return bad("slot out of range");
    if (!s->filled[slot]) return bad("the slot was never filled");
    auto fail = [&](hipError_t err) { h->err = std::string("vg_kf_get: ") + hipGetErrorString(err); return VG_ERR_HIP; };
    hipError_t e = hipSetDevice(h->device);
    if (e != hipSuccess) return fail(e);
    if ((e = s->h_down.resize(s->rec_bytes)) != hipSuccess) return fail(e);
    if ((e = hipMemcpyAsync(s->h_down.data(), s->rec + (size_t)slot * s->rec_bytes, s->rec_bytes, hipMemcpyDeviceToHost, h->stream)) != hipSuccess) return fail(e);
    if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return fail(e);
    const KfView v(s, s->h_down.data());
    const size_t nk = (size_t)v.cnt[0], nw = (size_t)v.cnt[1];
    rec->n_keypoints = v.cnt[0]; rec->n_window = v.cnt[1]; rec->n_true = v.cnt[2];
    if (rec->keypoints_xy) memcpy(rec->keypoints_xy, v.pt, 8 * nk);
    if (rec->scores) memcpy(rec->scores, v.score, nk);
    if (rec->norm_xy) memcpy(rec->norm_xy, v.norm, 8 * nk);
    if (rec->descriptors) memcpy(rec->descriptors, v.desc, 32 * nk);
    if (rec->window_xy) memcpy(rec->window_xy, v.wpt, 8 * nw);
    if (rec->window_descriptors) memcpy(rec->window_descriptors, v.wdesc, 32 * nw);
    return VG_OK;
}

extern "C" int vg_kf_set(vg_handle* h, int slot, const vg_kf_record* rec) {
    if (!h) return VG_ERR_BAD_ARG;
    KfState* s = (KfState*)h->kf;
    auto bad = [&](const char* what) { h->err = std::string("vg_kf_set: ") + what; return VG_ERR_BAD_ARG; };
    if (!s) return bad("the handle has no keyframe records (vg_kf_configure)");
    if (!rec) return bad("a NULL argument");
    if (rec->struct_size != (int)sizeof(vg_kf_record)) return bad("vg_kf_record::struct_size");
    if (slot < 0 || slot >= s->NS) return bad("slot out of range");
    if (rec->n_keypoints < 0 || rec->n_keypoints > s->MK) return bad("n_keypoints above max_keypoints");
    if (rec->n_window < 0 || rec->n_window > s->MW) return bad("n_window above max_window_points");
    if (rec->n_true != 0 && rec->n_true < rec->n_keypoints) return bad("n_true below n_keypoints");
    if (rec->n_keypoints > 0 && (!rec->keypoints_xy || !rec->scores || !rec->norm_xy || !rec->descriptors)) return bad("a NULL table of a non-zero count");
    if (rec->n_window > 0 && (!rec->window_xy || !rec->window_descriptors)) return bad("a NULL table of a non-zero count");
    auto fail = [&](hipError_t err) { h->err = std::string("vg_kf_set: ") + hipGetErrorString(err); return VG_ERR_HIP; };
    hipError_t e = hipSetDevice(h->device);
    if (e != hipSuccess) return fail(e);
    if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return fail(e);        // (the staging may still be in flight)
    if ((e = s->h_up.resize(s->rec_bytes)) != hipSuccess) return fail(e);
    char* r = s->h_up.data();
    memset(r, 0, s->rec_bytes);
    const size_t nk = (size_t)rec->n_keypoints, nw = (size_t)rec->n_window;
    int* cnt = (int*)r;
    cnt[0] = rec->n_keypoints; cnt[1] = rec->n_window; cnt[2] = rec->n_true ? rec->n_true : rec->n_keypoints; cnt[3] = 1;
    if (nk) {
        memcpy(r + s->r_desc, rec->descriptors, 32 * nk); memcpy(r + s->r_pt, rec->keypoints_xy, 8 * nk);
        memcpy(r + s->r_norm, rec->norm_xy, 8 * nk); memcpy(r + s->r_score, rec->scores, nk);
    }
    if (nw) { memcpy(r + s->r_wdesc, rec->window_descriptors, 32 * nw); memcpy(r + s->r_wpt, rec->window_xy, 8 * nw); }
    if ((e = hipMemcpyAsync(s->rec + (size_t)slot * s->rec_bytes, r, s->rec_bytes, hipMemcpyHostToDevice, h->stream)) != hipSuccess) return fail(e);
    if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return fail(e);
    s->filled[slot] = 1;
    s->kept[slot] = rec->n_keypoints;
    return VG_OK;
}

extern "C" int vg_kf_match(vg_handle* h, int n_pairs, const vg_kf_pair* in, vg_kf_match_out* out) {
    VG_RANGE("vg_kf_match");
    if (!h) return VG_ERR_BAD_ARG;
    KfState* s = (KfState*)h->kf;
    auto bad = [&](int p, const char* what) { h->err = "vg_kf_match: pair " + std::to_string(p) + ": " + what; return VG_ERR_BAD_ARG; };
    if (!s) { h->err = "vg_kf_match: the handle has no keyframe records (vg_kf_configure)"; return VG_ERR_BAD_ARG; }
    if (n_pairs <= 0 || !in || !out) { h->err = "vg_kf_match: n_pairs <= 0 or a NULL argument"; return VG_ERR_BAD_ARG; }
    for (int p = 0; p < n_pairs; ++p) {
        if (in[p].struct_size != (int)sizeof(vg_kf_pair)) return bad(p, "vg_kf_pair::struct_size");
        if (out[p].struct_size != (int)sizeof(vg_kf_match_out)) return bad(p, "vg_kf_match_out::struct_size");
        if (in[p].cur_slot < 0 || in[p].cur_slot >= s->NS || in[p].old_slot < 0 || in[p].old_slot >= s->NS) return bad(p, "slot out of range");
        if (!s->filled[in[p].cur_slot] || !s->filled[in[p].old_slot]) return bad(p, "a slot that was never filled");
    }
    auto fail = [&](hipError_t err) { h->err = std::string("vg_kf_match: ") + hipGetErrorString(err); return VG_ERR_HIP; };
    hipError_t e = hipSetDevice(h->device);
    if (e != hipSuccess) return fail(e);
    const size_t MW = (size_t)s->MW, stride = 4 + 12 * MW, n_out = 4 * stride * n_pairs, b_out = kf_up(8 * (size_t)n_pairs);
    if ((e = kf_scratch(s, b_out + n_out)) != hipSuccess) return fail(e);
    if ((e = s->h_up.resize(8 * (size_t)n_pairs)) != hipSuccess) return fail(e);
    if ((e = s->h_down.resize(n_out)) != hipSuccess) return fail(e);
    int* pr = (int*)s->h_up.data();
    for (int p = 0; p < n_pairs; ++p) { pr[2 * p] = in[p].cur_slot; pr[2 * p + 1] = in[p].old_slot; }
    KfMatchDev b;
    b.MW = s->MW; b.rec_bytes = s->rec_bytes; b.r_desc = s->r_desc; b.r_pt = s->r_pt; b.r_norm = s->r_norm; b.r_wdesc = s->r_wdesc;
    b.rec = s->rec; b.pairs = (const int*)s->buf; b.out = (int*)(s->buf + b_out);
    if ((e = hipMemcpyAsync(s->buf, pr, 8 * (size_t)n_pairs, hipMemcpyHostToDevice, h->stream)) != hipSuccess) return fail(e);
    struct Events {
        hipEvent_t ev[2] = {};
        ~Events() { for (hipEvent_t v : ev) if (v) (void)hipEventDestroy(v); }
    } evs;
    const bool timed = out[0].device_ms != nullptr;
    if (timed)
        for (int i = 0; i < 2; ++i)
            if ((e = hipEventCreate(&evs.ev[i])) != hipSuccess) return fail(e);
    if (timed && (e = hipEventRecord(evs.ev[0], h->stream)) != hipSuccess) return fail(e);
    hipLaunchKernelGGL(kf_match_kernel, dim3(n_pairs), dim3(KF_MATCH_THREADS), 0, h->stream, b);
    if (timed && (e = hipEventRecord(evs.ev[1], h->stream)) != hipSuccess) return fail(e);
    if ((e = hipGetLastError()) != hipSuccess) return fail(e);
    if ((e = hipMemcpyAsync(s->h_down.data(), s->buf + b_out, n_out, hipMemcpyDeviceToHost, h->stream)) != hipSuccess) return fail(e);
    if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return fail(e);
    if (timed) {
        float ms = 0.f;
        if ((e = hipEventElapsedTime(&ms, evs.ev[0], evs.ev[1])) != hipSuccess) return fail(e);
        out[0].device_ms[0] = ms;
    }
    for (int p = 0; p < n_pairs; ++p) {
        const int* r = (const int*)s->h_down.data() + stride * p;
        vg_kf_match_out& o = out[p];
        const size_t nw = (size_t)r[0], nm = (size_t)r[1];
        o.n_window = r[0]; o.n_matched = r[1];
        const int* idx = r + 4;
        const int* dist = idx + MW;
        const int* st = dist + MW;
        const int* m = st + MW;
        const int* mn = m + 2 * MW;
        const int* ci = mn + 2 * MW;
        const int* c = ci + MW;
        const int* cn = c + 2 * MW;
        if (o.best_idx) memcpy(o.best_idx, idx, 4 * nw);
        if (o.best_dist) memcpy(o.best_dist, dist, 4 * nw);
        if (o.status) for (size_t w = 0; w < nw; ++w) o.status[w] = (uint8_t)st[w];
        if (o.matched_2d_old) memcpy(o.matched_2d_old, m, 8 * nw);
        if (o.matched_2d_old_norm) memcpy(o.matched_2d_old_norm, mn, 8 * nw);
        if (o.matched_index) memcpy(o.matched_index, ci, 4 * nm);
        if (o.matched_old_xy) memcpy(o.matched_old_xy, c, 8 * nm);
        if (o.matched_old_norm) memcpy(o.matched_old_norm, cn, 8 * nm);
    }
    return VG_OK;
}
