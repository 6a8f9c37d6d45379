// fe_frame.hip — what FeatureTracker::readImage (feature_tracker/src/feature_tracker.cpp:81-167) does BETWEEN its OpenCV calls, on
// the device, so that vg_fe_read_image / vg_fe_read_image_batch (fe_host.hip) run a frame without handing intermediate results to the
// host.  The work on ONE stream is a body (ri_*_body) over the stream's view RiDev:
//   :115-124  status[i] && inBorder(forw_pts[i]) + reduceVector        -> ri_after_lk_body (ordered compaction = reduceVector)
//   :175-188  liftProjective of cur_pts / forw_pts for findFundamentalMat -> the same body (the stream's camera, double, reference order)
//   :191-198  the registrator's sequential bookkeeping over the RANSAC iterations + reduceVector by its mask -> ri_pick_body
//   :36-69    setMask's walk in the order the host's sort produced     -> ri_setmask_body (+ fe_stamp_kernel of fe_kernels.hip)
//   :144      n_max_cnt = MAX_CNT - forw_pts.size()                    -> written by the same body where fe_select_kernel reads it
//   :71-79, :258-268  addPoints + undistortedPoints (liftProjective of the final list) -> ri_finish_body
// All of them work on <= a few hundred points: what matters is that they need no round trip, not their arithmetic.  Compiled with
// -ffp-contract=off: the lifting (fe_camera.h) evaluates the reference's double expressions as written.
//
// The kernels (fe_rb_*, at the end of this file) run the frame for the S streams of a handle -- S = 1 is vg_fe_read_image: one
// workgroup (the walk: one wavefront) PER STREAM, which rebuilds the stream's RiDev from the device tables of RbDev and runs the body.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "vg_target.h"
#include "fe_layout.h"

#define FDEV __device__ __forceinline__

// liftProjective of the stream's camera (fe_camera.h: PinholeCamera, CataCamera or EquidistantCamera, the same function as fe_lift_kernel of
// fe_kernels.hip).  r.cam.model is uniform over the workgroup.
FDEV void ri_lift(const RiDev& r, float px, float py, double& x, double& y, double& z) { fe_cam_lift(r.cam, px, py, x, y, z); }
// FOCAL_LENGTH * x / z + COL / 2.0 (feature_tracker.cpp:176-187), rounded to float by cv::Point2f; the pinhole's z is 1.0
FDEV void ri_virtual(const RiDev& r, float px, float py, float* out) {
    double x, y, z;
    ri_lift(r, px, py, x, y, z);
    if (r.cam.model != FE_CAM_PINHOLE) { out[0] = (float)(r.focal * x / z + r.half_w); out[1] = (float)(r.focal * y / z + r.half_h); }
    else { out[0] = (float)(r.focal * x + r.half_w); out[1] = (float)(r.focal * y + r.half_h); }
}

// ordered compaction of a flag over [0, n) by one workgroup of 256 threads: dst[rank of i among the set flags] = src ? src[i] : i.
// Returns the number of set flags (uniform).  `wsum` = 4 ints of LDS.
FDEV int ri_compact(const uint8_t* flag, int n, const int* src, int* dst, int* wsum) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + tid;
        const bool f = i < n && flag[i] != 0;
        const unsigned long long bal = __ballot(f);
        if (lane == 0) wsum[wave] = __popcll(bal);
        __syncthreads();
        int before = base;
        for (int q = 0; q < wave; ++q) before += wsum[q];
        if (f) dst[before + __popcll(bal & ((1ull << lane) - 1ull))] = src ? src[i] : i;
        base += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
    return base;
}

// After the tracking kernel.  One workgroup.
FDEV void ri_after_lk_body(const FeDev& d, const RiDev& r, int* wsum) {
    const int tid = threadIdx.x;
    const int n = r.ctl[RI_N], publish = r.ctl[RI_PUBLISH];
    // :115-117  status[i] && inBorder(forw_pts[i])  (BORDER_SIZE 1, cvRound = round half to even)
    for (int i = tid; i < n; i += 256) {
        const float x = d.next_xy[2 * i], y = d.next_xy[2 * i + 1];
        const int ix = __float2int_rn(x), iy = __float2int_rn(y);
        const bool ok = d.status[i] != 0 && 1 <= ix && ix < d.W - 1 && 1 <= iy && iy < d.H - 1;
        r.a_status_lk[i] = ok ? 1 : 0;
        r.a_forw_xy[2 * i] = x; r.a_forw_xy[2 * i + 1] = y;
    }
    __threadfence_block();
    __syncthreads();
    const int n1 = ri_compact(r.a_status_lk, n, nullptr, r.idx1, wsum);
    __threadfence_block();
    __syncthreads();
    const bool ransac = publish && n1 >= 8;                         // rejectWithF: `if (forw_pts.size() >= 8)` (:171)
    for (int k = tid; k < n1; k += 256) {
        const int i = r.idx1[k];
        if (!publish) {                                             // undistortedPoints of the list this frame ends with (:262-267)
            fe_cam_lift_xy(r.cam, d.next_xy[2 * i], d.next_xy[2 * i + 1], r.a_un_xy[2 * k], r.a_un_xy[2 * k + 1]);
        } else {
            if (ransac) {                                           // :176-187
                ri_virtual(r, d.next_xy[2 * i], d.next_xy[2 * i + 1], r.p2 + 2 * k);
                ri_virtual(r, r.xy_in[2 * i], r.xy_in[2 * i + 1], r.p1 + 2 * k);
            } else
                r.idx2[k] = i;
        }
    }
    if (tid == 0) {
        r.ctl[RI_N1] = n1;
        r.ctl[RI_RANSAC] = ransac ? 1 : 0;
        int fb = 0;
        if (ransac && n1 < 15) fb |= RI_FB_LMEDS;
        if (ransac && n1 > FE_RANSAC_MAXPTS) fb |= RI_FB_RANGE;
        r.ctl[RI_FALLBACK] = fb;
        r.ctl[RI_BEST] = -1;
        r.ctl[RI_NITERS] = 0;
        if (!ransac) r.ctl[RI_N2] = n1;
        if (!ransac || fb) {                                        // (fb: the host finishes rejectWithF; the header tells it so)
            r.a_hdr[RI_N] = n; r.a_hdr[RI_PUBLISH] = publish; r.a_hdr[RI_N1] = n1; r.a_hdr[RI_N2] = n1; r.a_hdr[RI_FALLBACK] = fb;
            r.a_hdr[RI_RANSAC] = ransac ? 1 : 0; r.a_hdr[RI_BEST] = -1; r.a_hdr[RI_NITERS] = 0;
        }
    }
}

// After fe_rb_ransac7_kernel / fe_rb_count_kernel: the registrator's loop over the iterations (ptsetreg.cpp RANSACPointSetRegistrator::run
// as restated in fe_ransac.hip: a model replaces the best one if it has more inliers than max(best, 6); after every improvement the
// iteration bound shrinks to RANSACUpdateNumIters(...), read from the host-made table; iterations at or beyond the bound do not
// count), then the mask of the winning model and reduceVector by it.  One workgroup; the loop itself runs on one wavefront with the
// counts of 64 iterations in a register each (v_readlane in sequence: the bound usually ends the loop inside the first chunk).
// More than one stream: the loop runs in two parts with RANSAC work between them, iterations [it0, stop) per part, the state (bound,
// best count, best iteration) carried in ctl; `final`: the last part, which also makes the mask.  One stream: (0, FE_RANSAC_MAXIT, true).
FDEV void ri_pick_body(const RiDev& r, const int it0, const int stop, const bool final, int* wsum, int& sbest) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int n1 = r.ctl[RI_N1];
    if (r.ctl[RI_PUBLISH] == 0 || r.ctl[RI_RANSAC] == 0) return;
    int fb = r.ctl[RI_FALLBACK];
    if (fb & (RI_FB_LMEDS | RI_FB_RANGE)) return;                   // (header already written by ri_after_lk_body)
    if (tid < 64) {
        int niters = FE_RANSAC_MAXIT, max_good = 0, best = -1;
        if (it0 > 0) { niters = r.ctl[RI_NITERS]; max_good = r.ctl[RI_MAXGOOD]; best = r.ctl[RI_BEST]; }
        const int* tab = r.niters_tab + (size_t)n1 * r.tab_stride;
        for (int base = it0; base < stop && base < niters; base += 64) {
            const int mine = base + lane < stop ? r.count[base + lane] : -1;
            for (int j = 0; j < 64 && base + j < niters && base + j < stop; ++j) {
                const int c = __shfl(mine, j);
                if (c > (max_good > 6 ? max_good : 6)) {
                    best = base + j; max_good = c;
                    const int t = tab[c];
                    niters = t < niters ? t : niters;
                }
            }
        }
        if (lane == 0) { sbest = best; r.ctl[RI_BEST] = best; r.ctl[RI_NITERS] = niters; if (!final) r.ctl[RI_MAXGOOD] = max_good; }
    }
    if (!final) return;
    __syncthreads();
    const int best = sbest;
    const int nw = (n1 + 63) >> 6;
    // the mask: inlier set of the winning iteration's model; no model at all -> nothing is rejected (fe_ransac.hip, ASSUMPTIONS F9)
    for (int k = tid; k < n1; k += 256)
        r.a_status_f[k] = best < 0 ? 1 : (uint8_t)((r.words[(size_t)best * nw + (k >> 6)] >> (k & 63)) & 1ull);
    __threadfence_block();
    __syncthreads();
    const int n2 = ri_compact(r.a_status_f, n1, r.idx1, r.idx2, wsum);
    if (tid == 0) {
        fb = r.ctl[RI_FALLBACK];
        r.ctl[RI_N2] = n2;
        r.a_hdr[RI_N] = r.ctl[RI_N]; r.a_hdr[RI_PUBLISH] = 1; r.a_hdr[RI_N1] = n1; r.a_hdr[RI_N2] = n2; r.a_hdr[RI_FALLBACK] = fb;
        r.a_hdr[RI_RANSAC] = 1; r.a_hdr[RI_BEST] = best; r.a_hdr[RI_NITERS] = r.ctl[RI_NITERS];
    }
}

// setMask (:36-69) in a given order: position q of the walk is survivor order[q] (order == nullptr: the list as it stands).  A point is
// kept iff its rounded position is inside the image, the base mask there is 255 and no previously kept point's filled disc covers it
// (fe_setmask_kernel of fe_kernels.hip has the derivation).  One wavefront, 64 positions of the walk at a time, one per lane:
//   1. every lane tests ITS point against the points kept in earlier chunks (their coordinates are read from LDS at a uniform address);
//   2. inside the chunk the walk is sequential over the lanes that are still alive (s_ff1 over the ballot): the first one is kept, its
//      coordinates go to all lanes through v_readlane, every later lane it covers drops out -- ten instructions per kept point instead of
//      an LDS round trip per candidate (48 us -> see DESIGN.md for 150 points);
//   3. the kept lanes store their results side by side (prefix popcount).
// Also: n_max_cnt = MAX_CNT - kept (:144) for the detection.
#define RI_SETMASK_MAX 2048
FDEV void ri_setmask_body(const FeDev& d, const RiDev& r, short* kx, short* ky) {
    const int lane = threadIdx.x, W = d.W, H = d.H;
    const int n2 = r.ctl[RI_N2];
    const int r2 = r.radius * r.radius;
    int nk = 0;
    for (int base = 0; base < n2; base += 64) {
        const int q = base + lane;
        int px = 0, py = 0;
        bool alive = false;
        if (q < n2) {
            const int i = r.idx2[r.order ? r.order[q] : q];
            px = __float2int_rn(d.next_xy[2 * i]); py = __float2int_rn(d.next_xy[2 * i + 1]);      // Point2f -> Point: round half to even
            alive = px >= 0 && py >= 0 && px < W && py < H;
            if (alive && r.base_mask) alive = r.base_mask[(size_t)py * W + px] == 255;
        }
        for (int j = 0; j < nk; ++j) {
            const int dx = px - kx[j], dy = py - ky[j];
            alive = alive && !(dx * dx + dy * dy <= r2);
        }
        unsigned long long am = __ballot(alive), keptm = 0ull;
        while (am) {
            const int j = __ffsll((long long)am) - 1;
            keptm |= 1ull << j;
            const int jx = __shfl(px, j), jy = __shfl(py, j);
            const int dx = px - jx, dy = py - jy;
            alive = alive && lane > j && !(dx * dx + dy * dy <= r2);
            am = __ballot(alive);
        }
        if ((keptm >> lane) & 1ull) {
            const int k = nk + __popcll(keptm & ((1ull << lane) - 1ull));
            kx[k] = (short)px; ky[k] = (short)py;
            r.b_kept[k] = q;
            r.kept_xy[2 * k] = px; r.kept_xy[2 * k + 1] = py;
        }
        nk += __popcll(keptm);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    if (lane == 0) {
        r.ctl[RI_NK] = nk;
        const int room = r.max_cnt - nk;
        const_cast<int*>(d.max_corners)[0] = room > 0 ? (room < d.max_pts ? room : d.max_pts) : 0;
    }
}

// addPoints (:71-79) + undistortedPoints (:262-267): the list the frame ends with = the kept points in the walk's order, then the new
// corners; every point lifted.
FDEV void ri_finish_body(const FeDev& d, const RiDev& r) {
    const int tid = threadIdx.x;
    const int nk = r.ctl[RI_NK];
    const int nc = d.ncorners[0];
    const int nnew = nc < 0 ? 0 : nc;
    for (int k = tid; k < nk + nnew; k += 256) {
        float x, y;
        if (k < nk) {
            const int q = r.b_kept[k];
            const int i = r.idx2[r.order ? r.order[q] : q];
            x = d.next_xy[2 * i]; y = d.next_xy[2 * i + 1];
        } else {
            x = d.corners[2 * (k - nk)]; y = d.corners[2 * (k - nk) + 1];
            r.b_new_xy[2 * (k - nk)] = x; r.b_new_xy[2 * (k - nk) + 1] = y;
        }
        fe_cam_lift_xy(r.cam, x, y, r.b_un_xy[2 * k], r.b_un_xy[2 * k + 1]);
    }
    if (tid == 0) {
        r.ctl[RI_NNEW] = nc;
        r.b_hdr[RI_NK] = nk; r.b_hdr[RI_NNEW] = nc; r.b_hdr[RI_N2] = r.ctl[RI_N2];
    }
}

// ================================================================================================ the kernels: a workgroup per stream
// Stream c as the bodies see a stream: its slices of the per-stream arrays of FeDev (next_xy, status, corners, the detection's
// counters) and an RiDev made from the tables.  Everything here is uniform over the workgroup.
FDEV void rb_stream(const RbDev& b, const int c, FeDev& d, RiDev& r) {
    const size_t cap = (size_t)b.cap, mp = (size_t)d.max_pts;
    d.next_xy += c * mp * 2; d.status += c * mp; d.corners += c * mp * 2; d.max_corners += c; d.ncorners += c;
    const RiCam& k = b.cam[c];
    r.ctl = b.ctl + (size_t)c * RI_CTL_INTS; r.xy_in = b.xy_in + c * cap * 2; r.cap = b.cap;
    r.idx1 = b.idx1 + c * cap; r.idx2 = b.idx2 + c * cap; r.p1 = b.p1 + c * cap * 2; r.p2 = b.p2 + c * cap * 2;
    r.order = b.ord_flag[c] ? b.order + c * cap : nullptr;
    char* a = b.a + c * b.a_stride;
    r.a_hdr = (int*)a; r.a_status_lk = (uint8_t*)(a + b.a_st); r.a_status_f = (uint8_t*)(a + b.a_sf); r.a_forw_xy = (float*)(a + b.a_fw);
    r.a_un_xy = b.a_un + c * cap * 2;
    char* q = b.b + c * b.b_stride;
    r.b_hdr = (int*)q; r.b_kept = (int*)(q + b.b_k); r.b_new_xy = (float*)(q + b.b_nw); r.b_un_xy = (float*)(q + b.b_un);
    r.niters_tab = b.niters_tab; r.tab_stride = b.tab_stride;
    r.count = b.count + (size_t)c * FE_RANSAC_MAXIT; r.words = b.words + (size_t)c * FE_RANSAC_MAXIT * b.words_n;
    r.focal = k.focal; r.half_w = k.half_w; r.half_h = k.half_h;
    r.cam = k.cam;
    r.max_cnt = k.max_cnt; r.radius = k.radius;
    r.kept_xy = b.kept_xy + c * cap * 2;
    r.base_mask = (b.base && k.has_base) ? b.base + (size_t)c * d.W * d.H : nullptr;
}

// grid (S), 256 threads.  Besides the body: every stream starts the frame with no kept point and NO detection (a
// negative corner budget: fe_mineig_kernel / fe_select_kernel leave at once); fe_rb_setmask_kernel sets both for the streams that publish.
extern "C" __global__ __launch_bounds__(256) void fe_rb_after_lk_kernel(FeDev d, RbDev b) {
    __shared__ int wsum[4];
    const int c = blockIdx.x;
    RiDev r;
    rb_stream(b, c, d, r);
    if (threadIdx.x == 0) { b.nk[c] = 0; const_cast<int*>(d.max_corners)[0] = -1; }
    ri_after_lk_body(d, r, wsum);
}
// grid (S), 256 threads; the bookkeeping over iterations [first, end) (fe_ransac.hip); the part that ends at FE_RANSAC_MAXIT makes the mask
extern "C" __global__ __launch_bounds__(256) void fe_rb_pick_kernel(FeDev d, RbDev b, int first, int end) {
    __shared__ int wsum[4];
    __shared__ int sbest;
    RiDev r;
    rb_stream(b, blockIdx.x, d, r);
    ri_pick_body(r, first, end, end >= FE_RANSAC_MAXIT, wsum, sbest);
}
// grid (S), one wavefront
extern "C" __global__ __launch_bounds__(64) void fe_rb_setmask_kernel(FeDev d, RbDev b) {
    __shared__ short kx[RI_SETMASK_MAX], ky[RI_SETMASK_MAX];
    const int c = blockIdx.x;
    RiDev r;
    rb_stream(b, c, d, r);
    if (r.ctl[RI_PUBLISH] == 0) return;
    ri_setmask_body(d, r, kx, ky);
    if (threadIdx.x == 0) b.nk[c] = r.ctl[RI_NK];          // (lane 0 wrote it)
}
// grid (S), 256 threads
extern "C" __global__ __launch_bounds__(256) void fe_rb_finish_kernel(FeDev d, RbDev b) {
    RiDev r;
    rb_stream(b, blockIdx.x, d, r);
    if (r.ctl[RI_PUBLISH] == 0) return;
    ri_finish_body(d, r);
}

// ================================================================================================ vg_fe_tracks_step: the frame's last kernel
// grid (S), 256 threads, after fe_rb_finish_kernel (after fe_rb_after_lk_kernel when no stream publishes).  The bookkeeping of
// FeatureTracker that vg_fe_read_image_batch leaves to its caller, on the resident lists (TkDev, fe_layout.h), from `from` into `to`:
//   :118-128, :193-198, :55-68  reduceVector / setMask's re-ordering over ids, track_cnt, cur_un_pts: final position -> input position
//                               is idx1 (not published) or idx2[order[b_kept]] (published), which the frame's kernels left behind
//   :129                        track_cnt + 1
//   :71-79                      addPoints: the new corners, count 1
//   :272-305                    pts_velocity against prev_un_pts_map: float difference, double division by dt, rounded to float
//   :204-214                    updateID: the list's ids are >= 0 between the frames, so the entries that take n_id++ in list order are
//                               exactly the new corners, which stand at the end: id = n_id + (position among them)
//   feature_tracker_node.cpp:133-150  the message: track_cnt > 1, here ascending by id (the order Estimator::processImage's map has)
// A detection overflow on ANY stream voids the step for all of them: `to` gets TK_NNEW = -1 and nothing else.
extern "C" __global__ __launch_bounds__(256) void fe_tk_commit_kernel(FeDev d, RbDev b, TkDev t) {
    __shared__ int wsum[4];
    __shared__ int s_bad;
    __shared__ uint8_t flag[TK_MAX];
    __shared__ int pos[TK_MAX];
    __shared__ unsigned long long key[TK_MAX];
    const int c = blockIdx.x, tid = threadIdx.x;
    const size_t cap = (size_t)b.cap;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    for (int s = tid; s < b.S; s += 256)
        if (b.ctl[(size_t)s * RI_CTL_INTS + RI_PUBLISH] != 0 && d.ncorners[s] < 0) s_bad = 1;
    __syncthreads();
    int* th = t.to.hdr + (size_t)c * TK_HDR_INTS;
    if (s_bad) {
        if (tid == 0) th[TK_NNEW] = -1;
        return;
    }
    RiDev r;
    rb_stream(b, c, d, r);
    const int* fh = t.from.hdr + (size_t)c * TK_HDR_INTS;
    const int* f_ids = t.from.ids + c * cap;
    const int* f_cnt = t.from.cnt + c * cap;
    const float* f_un = t.from.un_xy + c * cap * 2;
    const uint8_t* f_map = t.from.in_map + c * cap;
    int* t_ids = t.to.ids + c * cap;
    int* t_cnt = t.to.cnt + c * cap;
    float* t_xy = t.to.cur_xy + c * cap * 2;
    float* t_un = t.to.un_xy + c * cap * 2;
    float* t_vel = t.to.vel + c * cap * 2;
    uint8_t* t_map = t.to.in_map + c * cap;
    const int publish = r.ctl[RI_PUBLISH];
    const int ncar = publish ? r.ctl[RI_NK] : r.ctl[RI_N1];                 // carried over
    int nnew = publish ? d.ncorners[0] : 0;
    nnew = nnew < b.cap - ncar ? nnew : b.cap - ncar;                       // (max_cnt <= max_points: never cuts)
    const int n = ncar + nnew;
    const double stamp = *(const double*)(r.ctl + RI_STAMP);
    const double dt = stamp - *(const double*)(fh + TK_TIME);
    const int n_id = fh[TK_NID];
    const float* un = publish ? r.b_un_xy : r.a_un_xy;                      // the lifted list the frame path made
    for (int k = tid; k < n; k += 256) {
        const float ux = un[2 * k], uy = un[2 * k + 1];
        float x, y, vx = 0.f, vy = 0.f;
        int id, cnt;
        if (k < ncar) {
            int i;
            if (publish) {
                const int q = r.b_kept[k];
                i = r.idx2[r.order ? r.order[q] : q];
            } else
                i = r.idx1[k];
            x = d.next_xy[2 * i]; y = d.next_xy[2 * i + 1];
            id = f_ids[i]; cnt = f_cnt[i] + 1;
            if (f_map[i]) {
                vx = (float)((double)(ux - f_un[2 * i]) / dt);
                vy = (float)((double)(uy - f_un[2 * i + 1]) / dt);
            }
        } else {
            const int j = k - ncar;
            x = d.corners[2 * j]; y = d.corners[2 * j + 1];
            id = n_id + j; cnt = 1;
        }
        t_ids[k] = id; t_cnt[k] = cnt;
        t_xy[2 * k] = x; t_xy[2 * k + 1] = y;
        t_un[2 * k] = ux; t_un[2 * k + 1] = uy;
        t_vel[2 * k] = vx; t_vel[2 * k + 1] = vy;
        t_map[k] = k < ncar ? 1 : 0;                                        // (id != -1) before updateID
        flag[k] = cnt > 1 ? 1 : 0;
    }
    __threadfence_block();
    __syncthreads();
    // ---- the message: positions with track_cnt > 1 (ordered compaction), then (id, position) pairs sorted by one workgroup: bitonic
    // over the next power of two, padded with keys above every id
    const int nm = ri_compact(flag, n, nullptr, pos, wsum);
    __syncthreads();
    int P = 1;
    while (P < nm) P <<= 1;
    for (int k = tid; k < P; k += 256)
        key[k] = k < nm ? (((unsigned long long)(unsigned)t_ids[pos[k]] << 32) | (unsigned long long)(unsigned)pos[k]) : ~0ull;
    for (int k2 = 2; k2 <= P; k2 <<= 1)
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int i = tid; i < P; i += 256) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned long long a = key[i], z = key[l];
                    if ((a > z) == ((i & k2) == 0)) { key[i] = z; key[l] = a; }
                }
            }
        }
    __syncthreads();
    int* m_id = t.to.msg_id + c * cap;
    double* m_obs = t.to.msg_obs + c * cap * 7;
    for (int m = tid; m < nm; m += 256) {
        const int p = (int)(key[m] & 0xffffffffull);
        m_id[m] = (int)(key[m] >> 32);
        double* o = m_obs + (size_t)m * 7;
        o[0] = (double)t_un[2 * p]; o[1] = (double)t_un[2 * p + 1]; o[2] = 1.0;
        o[3] = (double)t_xy[2 * p]; o[4] = (double)t_xy[2 * p + 1];
        o[5] = (double)t_vel[2 * p]; o[6] = (double)t_vel[2 * p + 1];
    }
    if (tid == 0) {
        th[TK_N] = n; th[TK_NID] = n_id + nnew; th[TK_NMSG] = nm; th[TK_NK] = publish ? ncar : 0; th[TK_NNEW] = nnew;
        *(double*)(th + TK_TIME) = stamp;
    }
}
