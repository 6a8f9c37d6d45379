// fe_host.hip — host side of the front-end path behind the C-ABI (include/vinsgpu.h, vg_fe_*): owns the per-camera
// pyramids / point / corner buffers in HBM, launches the kernels of fe_kernels.hip on the handle's stream.
// Replaces the OpenCV calls of FeatureTracker::readImage (feature_tracker/src/feature_tracker.cpp:87-93, :113, :149).
#include "vg_range.h"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include "fe_layout.h"
#include "vg_handle.h"
#include "../../include/vinsgpu.h"

#define HIPCHK(h, expr)                                                                            \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) {                                                                    \
            (h)->err = std::string(#expr) + ": " + hipGetErrorString(_e);                          \
            return VG_ERR_HIP;                                                                     \
        }                                                                                          \
    } while (0)

extern "C" {
__global__ void fe_clahe_lut_kernel(FeDev d, int clip_limit, float lut_scale);
__global__ void fe_clahe_apply_kernel(FeDev d, uint8_t* const* dst_planes);
__global__ void fe_copy_kernel(FeDev d, uint8_t* const* dst_planes);
__global__ void fe_pyrdown_kernel(const uint8_t* const* src_planes, uint8_t* const* dst_planes, int sw, int sh, int waves_per_strip);
__global__ void fe_pyrdown_tile_kernel(const uint8_t* const* src_planes, uint8_t* const* dst_planes, int sw, int sh);
__global__ void fe_lk_kernel(FeDev d);
__global__ void fe_mineig_kernel(FeDev d, double quality);
hipError_t fe_launch_select(const FeDev& d, double quality, float min_dist, hipStream_t stream);
__global__ void fe_setmask_kernel(FeDev d, const float* pts_xy, const int* track_cnt, const int* npts, const uint8_t* const* base_masks,
                                  int radius, int* kept_index, int* n_kept, int* kept_xy);
__global__ void fe_stamp_kernel(FeDev d, const int* n_kept, const int* kept_xy, int radius);
__global__ void fe_lift_kernel(const float* pts_xy, int n, FeCamera cam, float* out_xy);
// vg_fe_read_image / vg_fe_read_image_batch (fe_frame.hip, fe_ransac.hip)
__global__ void fe_rb_after_lk_kernel(FeDev d, RbDev b);
__global__ void fe_rb_pick_kernel(FeDev d, RbDev b, int first, int end);
__global__ void fe_rb_setmask_kernel(FeDev d, RbDev b);
__global__ void fe_rb_finish_kernel(FeDev d, RbDev b);
__global__ void fe_rb_ransac7_kernel(RbDev b, const int* sched, int first, int end);
__global__ void fe_rb_count_kernel(RbDev b, int first, int end);
__global__ void fe_tk_commit_kernel(FeDev d, RbDev b, TkDev t);
}
void fe_ransac_tables(int nmax, std::vector<int>& sched, std::vector<int>& niters, int stride);

// resident state of vg_fe_read_image / vg_fe_read_image_batch: the tables of RbDev for every stream of the handle (one device
// allocation), the pinned mirrors of what travels ([input | block A | lifted survivors | block B | orders]), the RANSAC tables
struct RbState {
    char* dev = nullptr;
    char* host = nullptr;
    size_t in_bytes = 0, a_bytes = 0, un_bytes = 0, b_bytes = 0, ord_bytes = 0, ord_flags_bytes = 0;
    size_t o_ctl = 0, o_cam = 0, o_xy = 0;            // inside the input block
    char *d_in = nullptr, *d_a = nullptr, *d_b = nullptr, *d_ord = nullptr;
    int *d_sched = nullptr, *d_tab = nullptr;
    uint8_t* d_base = nullptr;                        // [S][H][W] copies of the callers' fisheye masks
    std::vector<const uint8_t*> base_src;
    bool ord_flags_set = false;                       // a walk-order flag on the device is 1 (all zero: the next frame without orders uploads none)
    RbDev b;
};
static void rb_free(RbState* q) {
    if (!q) return;
    (void)hipFree(q->dev); (void)hipFree(q->d_sched); (void)hipFree(q->d_tab); (void)hipFree(q->d_base);
    (void)hipHostFree(q->host);
    delete q;
}

// resident track lists of vg_fe_tracks_* (TkDev, fe_layout.h): two device copies of one block (a step reads dev[cur] and commits into
// dev[cur ^ 1], which becomes current when the step has succeeded), the pinned mirror the results are handed out from, and the one
// thing the host mirrors: each stream's list length, for the grid of the tracking kernel
struct TkState {
    char* dev[2] = {nullptr, nullptr};
    char* host = nullptr;
    int* h_cnt = nullptr;                             // pinned [S][cap]: the counts an order callback is handed come from here
    size_t bytes = 0, o_ids = 0, o_cnt = 0, o_xy = 0, o_un = 0, o_vel = 0, o_map = 0, o_mid = 0, o_obs = 0;
    int cur = 0;
    bool begun = false;
    std::vector<int> n;
};
static void tk_free(TkState* t) {
    if (!t) return;
    (void)hipFree(t->dev[0]); (void)hipFree(t->dev[1]); (void)hipHostFree(t->host); (void)hipHostFree(t->h_cnt);
    delete t;
}
static TkBuf tk_buf(const TkState* t, char* base) {
    TkBuf u;
    u.hdr = (int*)base; u.ids = (int*)(base + t->o_ids); u.cnt = (int*)(base + t->o_cnt); u.cur_xy = (float*)(base + t->o_xy);
    u.un_xy = (float*)(base + t->o_un); u.vel = (float*)(base + t->o_vel); u.in_map = (uint8_t*)(base + t->o_map);
    u.msg_id = (int*)(base + t->o_mid); u.msg_obs = (double*)(base + t->o_obs);
    return u;
}

struct FeState {
    FeDev d;
    int W = 0, H = 0, cams = 0, max_pts = 0;
    int flip = 0;                         // which plane set is "current"
    uint8_t* planes[2] = {nullptr, nullptr};   // two pyramids per camera, all levels, contiguous
    uint8_t* planes_alloc[2] = {nullptr, nullptr};   // (what hipMalloc returned: planes[k] - FE_SLACK)
    uint8_t* raw_alloc = nullptr;
    uint8_t** d_ptrs[2] = {nullptr, nullptr};  // device pointer tables [level*cams+cam]
    std::vector<uint8_t*> h_ptrs[2];
    // The same tables with level 0 pointing INTO the frame slot: pyramid set k <-> frame slot k.  A frame that is not equalized
    // is its own level 0 — the upload already put it into HBM, a copy into the pyramid's plane moves 361 KB per frame for
    // nothing (44 of 567 us per 256-stream step).  alias_on[k]: set k currently uses its frame slot as level 0.
    uint8_t** d_ptrs_alias[2] = {nullptr, nullptr};
    std::vector<uint8_t*> h_ptrs_alias[2];
    bool alias_on[2] = {false, false};
    size_t level_off[FE_MAX_LEVELS + 1];
    uint8_t* raw2[2] = {nullptr, nullptr};
    int raw_sel = 1;
    uint8_t *raw = nullptr, *lut = nullptr, *mask = nullptr, *status = nullptr;
    float *prev_xy = nullptr, *next_xy = nullptr, *err = nullptr, *eig = nullptr, *corners = nullptr;
    int *npts = nullptr, *max_corners = nullptr, *ncorners = nullptr;
    unsigned* ncand = nullptr;
    unsigned long long* keys = nullptr;
    std::vector<uint8_t> stage;           // pinned-ish host staging for strided uploads
    std::vector<int> h_npts;
    // setMask / lift, allocated on first use
    float* sm_pts = nullptr;
    int *sm_cnt = nullptr, *sm_n = nullptr, *sm_kidx = nullptr, *sm_nk = nullptr, *sm_kxy = nullptr;
    uint8_t* sm_base = nullptr;
    const uint8_t** sm_base_ptrs = nullptr;
    float *lift_in = nullptr, *lift_out = nullptr;
    bool have_prev = false;
    bool prev_clobbered = false;     // an upload has overwritten the frame slot the PREVIOUS pyramid uses as its level 0: no tracking until the next build
    std::vector<char> pushed_once;
    std::vector<FeCamera> cam;       // [cams] vg_fe_set_camera; cam_set[c] == 0: the pinhole of vg_fe_frame_in::intr
    std::vector<char> cam_set;
    RbState* rb = nullptr;
    TkState* tk = nullptr;
};

extern "C" void fe_state_destroy(FeState* s) {
    if (!s) return;
    for (int k = 0; k < 2; ++k) { (void)hipFree(s->planes_alloc[k]); (void)hipFree(s->d_ptrs[k]); (void)hipFree(s->d_ptrs_alias[k]); }
    (void)hipFree(s->raw_alloc); (void)hipFree(s->lut); (void)hipFree(s->mask); (void)hipFree(s->status);
    (void)hipFree(s->prev_xy); (void)hipFree(s->next_xy); (void)hipFree(s->err); (void)hipFree(s->eig);
    (void)hipFree(s->corners); (void)hipFree(s->npts); (void)hipFree(s->max_corners);
    (void)hipFree(s->ncorners); (void)hipFree(s->ncand); (void)hipFree(s->keys);
    (void)hipFree(s->sm_pts); (void)hipFree(s->sm_cnt); (void)hipFree(s->sm_n); (void)hipFree(s->sm_kidx); (void)hipFree(s->sm_nk);
    (void)hipFree(s->sm_kxy); (void)hipFree(s->sm_base); (void)hipFree((void*)s->sm_base_ptrs); (void)hipFree(s->lift_in); (void)hipFree(s->lift_out);
    rb_free(s->rb);
    tk_free(s->tk);
    delete s;
}

static void refresh(FeState* s) {
    const int a = s->flip, b = s->flip ^ 1;
    s->d.cur_planes = s->alias_on[a] ? s->d_ptrs_alias[a] : s->d_ptrs[a];
    s->d.prev_planes = s->alias_on[b] ? s->d_ptrs_alias[b] : s->d_ptrs[b];
}

extern "C" int vg_fe_configure(vg_handle* h, int width, int height, int n_cams, int max_points) {
    if (!h || width < 32 || height < 32 || n_cams < 1 || max_points < 1) return VG_ERR_BAD_ARG;
    if ((width * height) % 4) { h->err = "width*height must be a multiple of 4"; return VG_ERR_UNSUPPORTED; }
    HIPCHK(h, hipSetDevice(h->device));
    h->ba.seq.vio = false;                // (vg_vio_*: the bridge ends with the lists it reads)
    if (h->fe) { fe_state_destroy(h->fe); h->fe = nullptr; }
    FeState* s = new FeState();
    h->fe = s;
    s->W = width; s->H = height; s->cams = n_cams; s->max_pts = max_points;
    FeDev& d = s->d;
    memset(&d, 0, sizeof(d));
    d.W = width; d.H = height; d.cams = n_cams; d.max_level = 3; d.max_pts = max_points; d.max_count = 30;
    d.min_eig_thr = 1e-4f; d.eps2 = 0.01 * 0.01;
    // buildOpticalFlowPyramid: levels while both dims stay > winSize (21)
    int lw = width, lh = height, nl = 0;
    size_t off = 0;
    for (int l = 0; l < FE_MAX_LEVELS; ++l) {
        d.lw[l] = lw; d.lh[l] = lh;
        s->level_off[l] = off;
        off += ((size_t)lw * lh + 255) / 256 * 256;
        nl = l;
        const int nw = (lw + 1) / 2, nh = (lh + 1) / 2;
        if (nw <= 21 || nh <= 21) break;
        lw = nw; lh = nh;
    }
    d.max_level = nl;
    s->level_off[nl + 1] = off;
    const size_t per_cam = off, npix = (size_t)width * height;
    for (int k = 0; k < 2; ++k) {
        // (FE_SLACK bytes in front of and behind the planes: fe_pyrdown_kernel's 16-byte windows start 4 bytes before a row and end
        //  up to 12 bytes after it; what they read there is never used)
        HIPCHK(h, hipMalloc((void**)&s->planes_alloc[k], per_cam * n_cams + 2 * FE_SLACK));
        HIPCHK(h, hipMemset(s->planes_alloc[k], 0, per_cam * n_cams + 2 * FE_SLACK));
        s->planes[k] = s->planes_alloc[k] + FE_SLACK;
        s->h_ptrs[k].resize((size_t)(nl + 1) * n_cams);
        for (int l = 0; l <= nl; ++l)
            for (int c = 0; c < n_cams; ++c) s->h_ptrs[k][(size_t)l * n_cams + c] = s->planes[k] + (size_t)c * per_cam + s->level_off[l];
        HIPCHK(h, hipMalloc((void**)&s->d_ptrs[k], sizeof(uint8_t*) * s->h_ptrs[k].size()));
        HIPCHK(h, hipMemcpy(s->d_ptrs[k], s->h_ptrs[k].data(), sizeof(uint8_t*) * s->h_ptrs[k].size(), hipMemcpyHostToDevice));
    }
    // candidate keys per stream: a power of two (the fall-back sort is bitonic) that holds every 3x3 local maximum of a frame without
    // ties (W H / 4) -- 65536 for 752 x 480 -- so that the timing-dependent pruning bound of fe_mineig_kernel cannot overflow it on
    // larger frames either; an overflow (plateaus of equal positive values) is reported, never truncated silently
    {
        size_t cap = FE_CAND_CAP;
        while (cap < npix / 4) cap *= 2;
        d.cand_cap = (int)cap;
    }
    HIPCHK(h, hipMalloc((void**)&s->raw_alloc, 2 * npix * n_cams + 2 * FE_SLACK));
    HIPCHK(h, hipMemset(s->raw_alloc, 0, 2 * npix * n_cams + 2 * FE_SLACK));
    s->raw = s->raw_alloc + FE_SLACK;
    s->raw2[0] = s->raw; s->raw2[1] = s->raw + npix * n_cams;
    for (int k = 0; k < 2; ++k) {
        s->h_ptrs_alias[k] = s->h_ptrs[k];
        for (int c = 0; c < n_cams; ++c) s->h_ptrs_alias[k][c] = s->raw2[k] + (size_t)c * npix;
        HIPCHK(h, hipMalloc((void**)&s->d_ptrs_alias[k], sizeof(uint8_t*) * s->h_ptrs_alias[k].size()));
        HIPCHK(h, hipMemcpy(s->d_ptrs_alias[k], s->h_ptrs_alias[k].data(), sizeof(uint8_t*) * s->h_ptrs_alias[k].size(), hipMemcpyHostToDevice));
        s->alias_on[k] = false;
    }
    HIPCHK(h, hipMalloc((void**)&s->lut, (size_t)n_cams * 64 * 256));
    HIPCHK(h, hipMalloc((void**)&s->mask, npix * n_cams));
    HIPCHK(h, hipMemset(s->mask, 255, npix * n_cams));
    HIPCHK(h, hipMalloc((void**)&s->status, (size_t)n_cams * max_points));
    HIPCHK(h, hipMalloc((void**)&s->prev_xy, sizeof(float) * 2 * n_cams * max_points));
    HIPCHK(h, hipMalloc((void**)&s->next_xy, sizeof(float) * 2 * n_cams * max_points));
    HIPCHK(h, hipMalloc((void**)&s->err, sizeof(float) * n_cams * max_points));
    HIPCHK(h, hipMalloc((void**)&s->corners, sizeof(float) * 2 * n_cams * max_points));
    HIPCHK(h, hipMalloc((void**)&s->npts, sizeof(int) * n_cams));
    HIPCHK(h, hipMemset(s->npts, 0, sizeof(int) * n_cams));
    HIPCHK(h, hipMalloc((void**)&s->max_corners, sizeof(int) * n_cams));
    HIPCHK(h, hipMalloc((void**)&s->ncorners, sizeof(int) * n_cams));
    HIPCHK(h, hipMalloc((void**)&s->ncand, sizeof(unsigned) * FE_CNT_STRIDE * n_cams));
    HIPCHK(h, hipMalloc((void**)&s->keys, sizeof(unsigned long long) * (size_t)d.cand_cap * n_cams));
    d.raw = s->raw2[s->raw_sel]; d.lut = s->lut; d.npts = s->npts; d.prev_xy = s->prev_xy; d.next_xy = s->next_xy; d.status = s->status;
    d.err = s->err; d.eig = nullptr; d.keep_eig = 0; d.mask = s->mask; d.ncand = s->ncand; d.keys = s->keys;
    d.max_corners = s->max_corners; d.corners = s->corners; d.ncorners = s->ncorners;
    s->h_npts.assign(n_cams, 0);
    s->pushed_once.assign(n_cams, 0);
    s->cam.assign(n_cams, FeCamera());
    s->cam_set.assign(n_cams, 0);
    refresh(s);
    return VG_OK;
}

// the frames of all streams into the slot of the next build; `strides`: the row pitch per stream, or NULL = `stride` for every stream
static int fe_upload_async(vg_handle* h, const uint8_t* const* imgs, int stride, const int* strides = nullptr) {
    if (!h || !h->fe || !imgs) return VG_ERR_BAD_ARG;
    FeState* s = h->fe;
    const size_t npix = (size_t)s->W * s->H;
    auto pitch = [&](int c) { return strides ? strides[c] : stride; };
    for (int c = 0; c < s->cams; ++c)                 // validate before touching any state
        if (!imgs[c]) { h->err = "vg_fe_upload_frames: every stream needs a frame (batched streams advance together)"; return VG_ERR_BAD_ARG; }
    for (int c = 0; c < s->cams; ++c)
        if (pitch(c) < s->W) { h->err = "vg_fe_upload_frames: stride smaller than the frame width"; return VG_ERR_BAD_ARG; }
    // into the frame slot of the pyramid set the next build fills (set k <-> slot k): never the slot the CURRENT pyramid may be
    // using as its level 0 -- that image is the "previous" one of the next tracking step
    s->raw_sel = s->flip ^ 1;
    s->d.raw = s->raw2[s->raw_sel];
    // That slot may be level 0 of the PREVIOUS pyramid (frame n - 1, aliased): uploading frame n + 1 before frame n has been tracked
    // would make vg_fe_track* read the new image as the old one.  The order upload -> build -> track is fine (the build rotates the
    // sets); upload -> track is refused until a build has run.
    s->prev_clobbered = s->have_prev && s->alias_on[s->flip ^ 1];
    // frames that follow each other in memory without padding (one buffer for all streams: a ring of a capture driver, the bench's
    // staging area) travel as ONE copy; otherwise one copy per stream (2-D when its rows are padded)
    bool contiguous = true;
    for (int c = 0; c < s->cams && contiguous; ++c) contiguous = pitch(c) == s->W && (c == 0 || imgs[c] == imgs[c - 1] + npix);
    if (contiguous) {
        HIPCHK(h, hipMemcpyAsync(s->raw2[s->raw_sel], imgs[0], npix * s->cams, hipMemcpyHostToDevice, h->stream));
    } else {
        for (int c = 0; c < s->cams; ++c) {
            if (pitch(c) == s->W) HIPCHK(h, hipMemcpyAsync(s->raw2[s->raw_sel] + (size_t)c * npix, imgs[c], npix, hipMemcpyHostToDevice, h->stream));
            else HIPCHK(h, hipMemcpy2DAsync(s->raw2[s->raw_sel] + (size_t)c * npix, s->W, imgs[c], pitch(c), s->W, s->H, hipMemcpyHostToDevice, h->stream));
        }
    }
    return VG_OK;
}

extern "C" int vg_fe_upload_frames(vg_handle* h, const uint8_t* const* imgs, int stride) {
    VG_RANGE("vg_fe_upload_frames");
    const int rc = fe_upload_async(h, imgs, stride);
    if (rc) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return VG_OK;
}

extern "C" int vg_fe_frame_slot(vg_handle* h) {
    return (h && h->fe) ? h->fe->raw_sel : -1;
}

extern "C" int vg_fe_select_frames(vg_handle* h, int slot) {
    if (!h || !h->fe || slot < 0 || slot > 1) return VG_ERR_BAD_ARG;
    h->fe->raw_sel = slot;
    h->fe->d.raw = h->fe->raw2[slot];
    return VG_OK;
}

// why the frames of this handle cannot be equalized, or nullptr
static const char* fe_clahe_refusal(const FeDev& d) {
    if (d.W % 8 || d.H % 8) return "CLAHE needs width and height divisible by 8";
    // (fe_clahe_apply_kernel lays the interpolation cells of a row over the 256 threads of a workgroup: W / 8 / 4 + 3 of them)
    if (d.W / 8 / 4 + 3 > 256) return "CLAHE: frame wider than the interpolation-cell tiling (W / 32 + 3 > 256)";
    return nullptr;
}

extern "C" int vg_fe_build_async(vg_handle* h, int equalize) {
    VG_RANGE("vg_fe_build_async");
    if (!h || !h->fe) return VG_ERR_BAD_ARG;
    FeState* s = h->fe;
    if (const char* why = equalize ? fe_clahe_refusal(s->d) : nullptr) { h->err = why; return VG_ERR_UNSUPPORTED; }
    const bool first = !s->have_prev;
    s->prev_clobbered = false;
    s->flip ^= 1;                                     // previous <- current (only after the arguments are known to be valid)
    // level 0 = the frame slot itself when the frame is used as it is and sits in the slot that belongs to this pyramid set
    // (the normal alternation: upload -> build -> upload -> build); otherwise it is written into the set's own plane
    const bool alias = !equalize && !first && s->raw_sel == s->flip;
    s->alias_on[s->flip] = alias;
    refresh(s);
    const FeDev& d = s->d;
    uint8_t* const* cur0 = alias ? s->d_ptrs_alias[s->flip] : s->d_ptrs[s->flip];
    if (equalize) {
        const int area = (d.W / 8) * (d.H / 8);
        int clip = (int)(3.0 * area / 256);
        clip = clip < 1 ? 1 : clip;
        hipLaunchKernelGGL(fe_clahe_lut_kernel, dim3(64, d.cams), dim3(256), 0, h->stream, d, clip, 255.f / area);
        hipLaunchKernelGGL(fe_clahe_apply_kernel, dim3(9, 9, d.cams), dim3(256), 0, h->stream, d, cur0);      // one workgroup per interpolation cell
    } else if (!alias) {
        hipLaunchKernelGGL(fe_copy_kernel, dim3(256, d.cams), dim3(256), 0, h->stream, d, cur0);
    }
    for (int l = 1; l <= d.max_level; ++l) {
        const int sw = d.lw[l - 1], sh = d.lh[l - 1];
        if ((sw & 3) == 0) {
            // thread = 4 output columns x 8 output rows, a wavefront = 256 columns of one strip of rows (fe_kernels.hip)
            const int dw = sw / 2, dh = (sh + 1) / 2, wps = ((dw + 3) / 4 + 63) / 64, strips = (dh + 7) / 8;
            hipLaunchKernelGGL(fe_pyrdown_kernel, dim3((strips * wps + 3) / 4, 1, d.cams), dim3(256), 0, h->stream,
                               (const uint8_t* const*)(cur0 + (size_t)(l - 1) * d.cams), cur0 + (size_t)l * d.cams, sw, sh, wps);
        } else {
            hipLaunchKernelGGL(fe_pyrdown_tile_kernel, dim3(((sw + 1) / 2 + 63) / 64, ((sh + 1) / 2 + 15) / 16, d.cams), dim3(256), 0, h->stream,
                               (const uint8_t* const*)(cur0 + (size_t)(l - 1) * d.cams), cur0 + (size_t)l * d.cams, sw, sh);
        }
    }
    HIPCHK(h, hipGetLastError());
    if (first) {
        // prev_img = cur_img = forw_img = img on the first frame (feature_tracker.cpp:97-100)
        const size_t bytes = s->level_off[d.max_level + 1] * d.cams;
        HIPCHK(h, hipMemcpyAsync(s->planes[s->flip ^ 1], s->planes[s->flip], bytes, hipMemcpyDeviceToDevice, h->stream));
        s->have_prev = true;
    }
    return VG_OK;
}

extern "C" int vg_fe_push_frames(vg_handle* h, const uint8_t* const* imgs, int stride, int equalize) {
    VG_RANGE("vg_fe_push_frames");
    int rc = vg_fe_upload_frames(h, imgs, stride);
    if (rc) return rc;
    rc = vg_fe_build_async(h, equalize);
    if (rc) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return VG_OK;
}

extern "C" int vg_fe_track_upload(vg_handle* h, const float* prev_xy, const int* n) {
    if (!h || !h->fe || !prev_xy || !n) return VG_ERR_BAD_ARG;
    FeState* s = h->fe;
    for (int c = 0; c < s->cams; ++c) {
        if (n[c] < 0 || n[c] > s->max_pts) { h->err = "point count out of range"; return VG_ERR_BAD_ARG; }
        s->h_npts[c] = n[c];
    }
    HIPCHK(h, hipMemcpyAsync(s->prev_xy, prev_xy, sizeof(float) * 2 * s->cams * s->max_pts, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(s->npts, n, sizeof(int) * s->cams, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return VG_OK;
}

extern "C" int vg_fe_track_async(vg_handle* h) {
    VG_RANGE("vg_fe_track_async");
    if (!h || !h->fe) return VG_ERR_BAD_ARG;
    FeState* s = h->fe;
    if (s->prev_clobbered) {
        h->err = "vg_fe_track: a frame was uploaded into the slot of the previous image since the last build (upload -> build -> track)";
        return VG_ERR_BAD_ARG;
    }
    int nmax = 0;
    for (int c = 0; c < s->cams; ++c) nmax = nmax > s->h_npts[c] ? nmax : s->h_npts[c];
    if (nmax == 0) return VG_OK;
    hipLaunchKernelGGL(fe_lk_kernel, dim3(nmax, s->cams), dim3(64), 0, h->stream, s->d);
    HIPCHK(h, hipGetLastError());
    return VG_OK;
}

extern "C" int vg_fe_track_download(vg_handle* h, float* next_xy, uint8_t* status, float* err) {
    if (!h || !h->fe) return VG_ERR_BAD_ARG;
    FeState* s = h->fe;
    const size_t n = (size_t)s->cams * s->max_pts;
    if (next_xy) HIPCHK(h, hipMemcpyAsync(next_xy, s->next_xy, sizeof(float) * 2 * n, hipMemcpyDeviceToHost, h->stream));
    if (status) HIPCHK(h, hipMemcpyAsync(status, s->status, n, hipMemcpyDeviceToHost, h->stream));
    if (err) HIPCHK(h, hipMemcpyAsync(err, s->err, sizeof(float) * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return VG_OK;
}

extern "C" int vg_fe_track(vg_handle* h, int cam, const float* prev_xy, int n, float* next_xy, uint8_t* status, float* err) {
    VG_RANGE("vg_fe_track");
    if (!h || !h->fe || cam < 0 || cam >= h->fe->cams || n < 0 || n > h->fe->max_pts || (n && (!prev_xy || !next_xy || !status)))
        return VG_ERR_BAD_ARG;
    FeState* s = h->fe;
    if (n == 0) return VG_OK;
    const size_t o = (size_t)cam * s->max_pts;
    std::vector<int> saved = s->h_npts;
    for (int c = 0; c < s->cams; ++c) s->h_npts[c] = (c == cam) ? n : 0;
    HIPCHK(h, hipMemcpyAsync(s->prev_xy + o * 2, prev_xy, sizeof(float) * 2 * n, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(s->npts, s->h_npts.data(), sizeof(int) * s->cams, hipMemcpyHostToDevice, h->stream));
    int rc = vg_fe_track_async(h);
    if (rc) { s->h_npts = saved; return rc; }
    HIPCHK(h, hipMemcpyAsync(next_xy, s->next_xy + o * 2, sizeof(float) * 2 * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(status, s->status + o, n, hipMemcpyDeviceToHost, h->stream));
    if (err) HIPCHK(h, hipMemcpyAsync(err, s->err + o, sizeof(float) * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    // the single-stream call borrowed the batched point counts: put the other streams' counts back (host and device)
    s->h_npts = saved;
    HIPCHK(h, hipMemcpy(s->npts, s->h_npts.data(), sizeof(int) * s->cams, hipMemcpyHostToDevice));
    return VG_OK;
}

extern "C" int vg_fe_detect_upload(vg_handle* h, const uint8_t* const* masks, const int* max_corners) {
    if (!h || !h->fe || !max_corners) return VG_ERR_BAD_ARG;
    FeState* s = h->fe;
    const size_t npix = (size_t)s->W * s->H;
    for (int c = 0; c < s->cams; ++c) {
        if (max_corners[c] < 0 || max_corners[c] > s->max_pts) { h->err = "max_corners out of range"; return VG_ERR_BAD_ARG; }
        if (masks && masks[c]) HIPCHK(h, hipMemcpyAsync(s->mask + (size_t)c * npix, masks[c], npix, hipMemcpyHostToDevice, h->stream));
        else HIPCHK(h, hipMemsetAsync(s->mask + (size_t)c * npix, 255, npix, h->stream));
    }
    HIPCHK(h, hipMemcpyAsync(s->max_corners, max_corners, sizeof(int) * s->cams, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return VG_OK;
}

static const char* const FE_CAND_OVERFLOW = "goodFeaturesToTrack: candidate list overflow (more 3x3 maxima than the key buffer holds)";

// the min-distance cell grid of the detection holds FE_MAX_CELLS cells
static int fe_cell_grid_check(vg_handle* h, const FeDev& d, double min_dist) {
    const int cell = (int)std::lrint(min_dist) < 1 ? 1 : (int)std::lrint(min_dist);
    if (((d.W + cell - 1) / cell) * ((d.H + cell - 1) / cell) > FE_MAX_CELLS) { h->err = "min_dist too small for the cell grid"; return VG_ERR_UNSUPPORTED; }
    return VG_OK;
}

// goodFeaturesToTrack of every stream of `d` (max_corners and the mask are on the device)
static int fe_detect_launch(vg_handle* h, const FeDev& d, double quality, double min_dist) {
    const int rc = fe_cell_grid_check(h, d, min_dist);
    if (rc) return rc;
    HIPCHK(h, hipMemsetAsync(d.ncand, 0, sizeof(unsigned) * FE_CNT_STRIDE * d.cams, h->stream));
    // min-eigenvalue map + candidates in one kernel (64 x 16 tiles), then the exact threshold, the sort and the min-distance walk
    const dim3 g((d.W + 63) / 64, (d.H + 15) / 16, d.cams);
    hipLaunchKernelGGL(fe_mineig_kernel, g, dim3(256), 0, h->stream, d, quality);
    HIPCHK(h, fe_launch_select(d, quality, (float)min_dist, h->stream));
    HIPCHK(h, hipGetLastError());
    return VG_OK;
}

extern "C" int vg_fe_detect_async(vg_handle* h, double quality, double min_dist) {
    VG_RANGE("vg_fe_detect_async");
    if (!h || !h->fe) return VG_ERR_BAD_ARG;
    return fe_detect_launch(h, h->fe->d, quality, min_dist);
}

extern "C" int vg_fe_detect_download(vg_handle* h, float* out_xy, int* out_n) {
    if (!h || !h->fe || !out_xy || !out_n) return VG_ERR_BAD_ARG;
    FeState* s = h->fe;
    HIPCHK(h, hipMemcpyAsync(out_xy, s->corners, sizeof(float) * 2 * s->cams * s->max_pts, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(out_n, s->ncorners, sizeof(int) * s->cams, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int c = 0; c < s->cams; ++c)
        if (out_n[c] < 0) { out_n[c] = 0; h->err = FE_CAND_OVERFLOW; return VG_ERR_UNSUPPORTED; }
    return VG_OK;
}

// stream `cam` alone, with the mask that is on the device: run, read its count, report overflow, copy its n corners
static int fe_detect_stream(vg_handle* h, int cam, int max_corners, double quality, double min_dist, float* out_xy, int* out_n) {
    FeState* s = h->fe;
    std::vector<int> mc(s->cams, 0);
    mc[cam] = max_corners;
    HIPCHK(h, hipMemcpyAsync(s->max_corners, mc.data(), sizeof(int) * s->cams, hipMemcpyHostToDevice, h->stream));
    int rc = vg_fe_detect_async(h, quality, min_dist);
    if (rc) return rc;
    int n = 0;
    HIPCHK(h, hipMemcpyAsync(&n, s->ncorners + cam, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (n < 0) { h->err = FE_CAND_OVERFLOW; return VG_ERR_UNSUPPORTED; }
    if (n > 0) HIPCHK(h, hipMemcpy(out_xy, s->corners + (size_t)cam * s->max_pts * 2, sizeof(float) * 2 * n, hipMemcpyDeviceToHost));
    *out_n = n;
    return VG_OK;
}

extern "C" int vg_fe_detect(vg_handle* h, int cam, const uint8_t* mask, int max_corners, double quality, double min_dist,
                            float* out_xy, int* out_n) {
    VG_RANGE("vg_fe_detect");
    if (!h || !h->fe || cam < 0 || cam >= h->fe->cams || !out_xy || !out_n || max_corners < 0 || max_corners > h->fe->max_pts)
        return VG_ERR_BAD_ARG;
    FeState* s = h->fe;
    *out_n = 0;
    if (max_corners == 0) return VG_OK;
    const size_t npix = (size_t)s->W * s->H;
    if (mask) HIPCHK(h, hipMemcpyAsync(s->mask + (size_t)cam * npix, mask, npix, hipMemcpyHostToDevice, h->stream));
    else HIPCHK(h, hipMemsetAsync(s->mask + (size_t)cam * npix, 255, npix, h->stream));
    return fe_detect_stream(h, cam, max_corners, quality, min_dist, out_xy, out_n);
}

// ---- FeatureTracker::setMask on the device (feature_tracker.cpp:36-69)
extern "C" int vg_fe_set_mask(vg_handle* h, const float* pts_xy, const int* track_cnt, const int* n, const uint8_t* const* base_masks,
                              int radius, int* kept_index, int* n_kept) {
    VG_RANGE("vg_fe_set_mask");
    if (!h || !h->fe || !pts_xy || !track_cnt || !n || !kept_index || !n_kept || radius < 0) return VG_ERR_BAD_ARG;
    FeState* s = h->fe;
    if (s->max_pts > 2048) { h->err = "vg_fe_set_mask: max_points > 2048"; return VG_ERR_UNSUPPORTED; }
    for (int c = 0; c < s->cams; ++c)
        if (n[c] < 0 || n[c] > s->max_pts) { h->err = "vg_fe_set_mask: point count out of range"; return VG_ERR_BAD_ARG; }
    const size_t npix = (size_t)s->W * s->H, cap = (size_t)s->cams * s->max_pts;
    if (!s->sm_pts) {
        HIPCHK(h, hipMalloc((void**)&s->sm_pts, sizeof(float) * 2 * cap));
        HIPCHK(h, hipMalloc((void**)&s->sm_cnt, sizeof(int) * cap));
        HIPCHK(h, hipMalloc((void**)&s->sm_n, sizeof(int) * s->cams));
        HIPCHK(h, hipMalloc((void**)&s->sm_kidx, sizeof(int) * cap));
        HIPCHK(h, hipMalloc((void**)&s->sm_nk, sizeof(int) * s->cams));
        HIPCHK(h, hipMalloc((void**)&s->sm_kxy, sizeof(int) * 2 * cap));
        HIPCHK(h, hipMalloc((void**)&s->sm_base_ptrs, sizeof(uint8_t*) * s->cams));
    }
    bool any_base = false;
    for (int c = 0; c < s->cams; ++c) any_base = any_base || (base_masks && base_masks[c]);
    if (any_base && !s->sm_base) HIPCHK(h, hipMalloc((void**)&s->sm_base, npix * s->cams));
    std::vector<const uint8_t*> ptrs(s->cams, nullptr);
    for (int c = 0; c < s->cams; ++c) {
        uint8_t* dm = s->mask + (size_t)c * npix;
        if (base_masks && base_masks[c]) {
            HIPCHK(h, hipMemcpyAsync(s->sm_base + (size_t)c * npix, base_masks[c], npix, hipMemcpyHostToDevice, h->stream));
            HIPCHK(h, hipMemcpyAsync(dm, s->sm_base + (size_t)c * npix, npix, hipMemcpyDeviceToDevice, h->stream));
            ptrs[c] = s->sm_base + (size_t)c * npix;
        } else {
            HIPCHK(h, hipMemsetAsync(dm, 255, npix, h->stream));
        }
    }
    HIPCHK(h, hipMemcpyAsync((void*)s->sm_base_ptrs, ptrs.data(), sizeof(uint8_t*) * s->cams, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(s->sm_pts, pts_xy, sizeof(float) * 2 * cap, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(s->sm_cnt, track_cnt, sizeof(int) * cap, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(s->sm_n, n, sizeof(int) * s->cams, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(fe_setmask_kernel, dim3(s->cams), dim3(256), 0, h->stream, s->d, s->sm_pts, s->sm_cnt, s->sm_n,
                       any_base ? s->sm_base_ptrs : (const uint8_t* const*)nullptr, radius, s->sm_kidx, s->sm_nk, s->sm_kxy);
    hipLaunchKernelGGL(fe_stamp_kernel, dim3(s->max_pts, s->cams), dim3(256), 0, h->stream, s->d, s->sm_nk, s->sm_kxy, radius);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(kept_index, s->sm_kidx, sizeof(int) * cap, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(n_kept, s->sm_nk, sizeof(int) * s->cams, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return VG_OK;
}

// goodFeaturesToTrack with the mask vg_fe_set_mask left on the device (no mask upload)
extern "C" int vg_fe_detect_masked(vg_handle* h, int cam, int max_corners, double quality, double min_dist, float* out_xy, int* out_n) {
    VG_RANGE("vg_fe_detect_masked");
    if (!h || !h->fe || cam < 0 || cam >= h->fe->cams || !out_xy || !out_n || max_corners < 0 || max_corners > h->fe->max_pts)
        return VG_ERR_BAD_ARG;
    FeState* s = h->fe;
    *out_n = 0;
    if (max_corners == 0) return VG_OK;
    return fe_detect_stream(h, cam, max_corners, quality, min_dist, out_xy, out_n);
}

extern "C" int vg_fe_get_mask(vg_handle* h, int cam, uint8_t* out) {
    if (!h || !h->fe || cam < 0 || cam >= h->fe->cams || !out) return VG_ERR_BAD_ARG;
    FeState* s = h->fe;
    const size_t npix = (size_t)s->W * s->H;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(out, s->mask + (size_t)cam * npix, npix, hipMemcpyDeviceToHost));
    return VG_OK;
}

// ---- camera models (fe_camera.h)
static FeCamera fe_pinhole(const double* intr) {
    FeCamera c;
    c.model = FE_CAM_PINHOLE;
    for (int i = 0; i < 8; ++i) c.p[i] = intr[i];
    c.xi = 0.0;
    return c;
}
// the camera stream `c` lifts with: the one vg_fe_set_camera gave it, else the pinhole of the frame's intr
static FeCamera fe_stream_camera(const FeState* s, int c, const double* intr) { return s->cam_set[c] ? s->cam[c] : fe_pinhole(intr); }

// (fe_camera_check, a caller's vg_fe_camera -> FeCamera or the reason it is refused: fe_camera.h, shared with vg_kf_add)
extern "C" int vg_fe_set_camera(vg_handle* h, int cam, const vg_fe_camera* camera) {
    if (!h) return VG_ERR_BAD_ARG;
    if (!h->fe) { h->err = "vg_fe_set_camera: the handle has no front end (vg_fe_configure)"; return VG_ERR_BAD_ARG; }
    FeState* s = h->fe;
    if (cam < 0 || cam >= s->cams) { h->err = "vg_fe_set_camera: no such stream"; return VG_ERR_BAD_ARG; }
    if (!camera) { s->cam_set[cam] = 0; return VG_OK; }
    FeCamera c;
    if (const char* why = fe_camera_check(camera, &c)) { h->err = std::string("vg_fe_set_camera: ") + why; return VG_ERR_BAD_ARG; }
    s->cam[cam] = c;
    s->cam_set[cam] = 1;
    return VG_OK;
}

static int fe_lift_points(vg_handle* h, const char* who, const FeCamera& c, const float* pts_xy, int n, float* out_xy) {
    FeState* s = h->fe;
    if (n == 0) return VG_OK;
    if ((size_t)n > (size_t)s->cams * s->max_pts) { h->err = std::string(who) + ": more points than configured"; return VG_ERR_BAD_ARG; }
    if (!s->lift_in) {
        HIPCHK(h, hipMalloc((void**)&s->lift_in, sizeof(float) * 2 * s->cams * s->max_pts));
        HIPCHK(h, hipMalloc((void**)&s->lift_out, sizeof(float) * 2 * s->cams * s->max_pts));
    }
    HIPCHK(h, hipMemcpyAsync(s->lift_in, pts_xy, sizeof(float) * 2 * n, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(fe_lift_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, (const float*)s->lift_in, n, c, s->lift_out);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(out_xy, s->lift_out, sizeof(float) * 2 * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return VG_OK;
}

// liftProjective of any camera model for a batch of points (feature_tracker.cpp:258-271)
extern "C" int vg_fe_lift(vg_handle* h, const vg_fe_camera* camera, const float* pts_xy, int n, float* out_xy) {
    if (!h) return VG_ERR_BAD_ARG;
    if (!h->fe) { h->err = "vg_fe_lift: the handle has no front end (vg_fe_configure)"; return VG_ERR_BAD_ARG; }
    if (n < 0 || !camera || (n > 0 && (!pts_xy || !out_xy))) { h->err = "vg_fe_lift: camera / points / n"; return VG_ERR_BAD_ARG; }
    FeCamera c;
    if (const char* why = fe_camera_check(camera, &c)) { h->err = std::string("vg_fe_lift: ") + why; return VG_ERR_BAD_ARG; }
    return fe_lift_points(h, "vg_fe_lift", c, pts_xy, n, out_xy);
}

// PinholeCamera::liftProjective for a batch of points: vg_fe_lift with the pinhole of `intr`
extern "C" int vg_fe_undistort(vg_handle* h, const float* pts_xy, int n, const double* intr, float* out_xy) {
    if (!h || !h->fe || n < 0 || !intr || (n > 0 && (!pts_xy || !out_xy))) return VG_ERR_BAD_ARG;
    return fe_lift_points(h, "vg_fe_undistort", fe_pinhole(intr), pts_xy, n, out_xy);
}

extern "C" int vg_fe_get_level(vg_handle* h, int cam, int which, int level, uint8_t* out, int* w, int* hgt) {
    if (!h || !h->fe || cam < 0 || cam >= h->fe->cams || level < 0 || level > h->fe->d.max_level || !out) return VG_ERR_BAD_ARG;
    FeState* s = h->fe;
    const int set = which ? (s->flip ^ 1) : s->flip;
    const int lw = s->d.lw[level], lh = s->d.lh[level];
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const std::vector<uint8_t*>& tab = s->alias_on[set] ? s->h_ptrs_alias[set] : s->h_ptrs[set];
    HIPCHK(h, hipMemcpy(out, tab[(size_t)level * s->cams + cam], (size_t)lw * lh, hipMemcpyDeviceToHost));
    if (w) *w = lw;
    if (hgt) *hgt = lh;
    return VG_OK;
}

// The min-eigenvalue map is an LDS-only intermediate of the detection since round 4; a caller that wants to look at it (the parity
// tests do) asks for it before the detection: the map of every following detection is then written to HBM as well.
extern "C" int vg_fe_keep_eig(vg_handle* h, int on) {
    if (!h || !h->fe) return VG_ERR_BAD_ARG;
    FeState* s = h->fe;
    if (on && !s->eig) {
        HIPCHK(h, hipMalloc((void**)&s->eig, sizeof(float) * (size_t)s->W * s->H * s->cams));
        HIPCHK(h, hipMemset(s->eig, 0, sizeof(float) * (size_t)s->W * s->H * s->cams));       // (vg_fe_get_eig before any detection: zeros, not stale memory)
    }
    s->d.eig = s->eig;
    s->d.keep_eig = on ? 1 : 0;
    return VG_OK;
}

extern "C" int vg_fe_get_eig(vg_handle* h, int cam, float* out) {
    if (!h || !h->fe || cam < 0 || cam >= h->fe->cams || !out) return VG_ERR_BAD_ARG;
    FeState* s = h->fe;
    if (!s->d.keep_eig) { h->err = "vg_fe_get_eig: call vg_fe_keep_eig(h, 1) before the detection whose map is wanted"; return VG_ERR_BAD_ARG; }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(out, s->eig + (size_t)cam * s->W * s->H, sizeof(float) * s->W * s->H, hipMemcpyDeviceToHost));
    return VG_OK;
}

// ================================================================================================ one call per frame, every stream
static size_t ri_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

static int rb_build(vg_handle* h, FeState* s, RbState* q) {
    const size_t cap = (size_t)s->max_pts, S = (size_t)s->cams;
    RbDev& b = q->b;
    memset(&b, 0, sizeof(b));
    b.S = (int)S; b.cap = (int)cap;
    // input block: npts | control ints | cameras | cur_pts
    q->o_ctl = ri_up(sizeof(int) * S, 256);
    q->o_cam = q->o_ctl + ri_up(sizeof(int) * RI_CTL_INTS * S, 256);
    q->o_xy = q->o_cam + ri_up(sizeof(RiCam) * S, 256);
    q->in_bytes = q->o_xy + ri_up(sizeof(float) * 2 * cap * S, 256);
    b.a_st = 64; b.a_sf = b.a_st + ri_up(cap, 16); b.a_fw = b.a_sf + ri_up(cap, 16);
    b.a_stride = ri_up(b.a_fw + sizeof(float) * 2 * cap, 256);
    q->a_bytes = b.a_stride * S;
    q->un_bytes = ri_up(sizeof(float) * 2 * cap * S, 256);
    b.b_k = 64; b.b_nw = b.b_k + sizeof(int) * cap; b.b_un = b.b_nw + sizeof(float) * 2 * cap;
    b.b_stride = ri_up(b.b_un + sizeof(float) * 2 * cap, 256);
    q->b_bytes = b.b_stride * S;
    q->ord_flags_bytes = ri_up(sizeof(int) * S, 256);
    q->ord_bytes = q->ord_flags_bytes + ri_up(sizeof(int) * cap * S, 256);
    const size_t mirrored = q->in_bytes + q->a_bytes + q->un_bytes + q->b_bytes + q->ord_bytes;
    // device only: idx1 | idx2 | p1 | p2 | kept_xy | nk | RANSAC scratch (models, counts, inlier words: about 0.4 MB per stream)
    b.words_n = (int)((std::min<size_t>(cap, FE_RANSAC_MAXPTS) + 63) / 64);
    const size_t o_idx1 = mirrored, o_idx2 = o_idx1 + ri_up(sizeof(int) * cap * S, 256), o_p1 = o_idx2 + ri_up(sizeof(int) * cap * S, 256);
    const size_t o_p2 = o_p1 + ri_up(sizeof(float) * 2 * cap * S, 256), o_kxy = o_p2 + ri_up(sizeof(float) * 2 * cap * S, 256);
    const size_t o_nk = o_kxy + ri_up(sizeof(int) * 2 * cap * S, 256), o_mod = o_nk + ri_up(sizeof(int) * S, 256);
    const size_t o_cnt = o_mod + sizeof(double) * 27 * FE_RANSAC_MAXIT * S, o_w = o_cnt + ri_up(sizeof(int) * FE_RANSAC_MAXIT * S, 256);
    const size_t total = o_w + sizeof(unsigned long long) * (size_t)b.words_n * FE_RANSAC_MAXIT * S;
    HIPCHK(h, hipMalloc((void**)&q->dev, total));
    HIPCHK(h, hipMemset(q->dev, 0, total));
    HIPCHK(h, hipHostMalloc((void**)&q->host, mirrored, 0));
    memset(q->host, 0, mirrored);
    q->d_in = q->dev; q->d_a = q->d_in + q->in_bytes; q->d_b = q->d_a + q->a_bytes + q->un_bytes; q->d_ord = q->d_b + q->b_bytes;
    b.npts = (const int*)q->d_in; b.ctl = (int*)(q->d_in + q->o_ctl); b.cam = (const RiCam*)(q->d_in + q->o_cam);
    b.xy_in = (const float*)(q->d_in + q->o_xy);
    b.a = q->d_a; b.a_un = (float*)(q->d_a + q->a_bytes); b.b = q->d_b;
    b.ord_flag = (const int*)q->d_ord; b.order = (const int*)(q->d_ord + q->ord_flags_bytes);
    b.idx1 = (int*)(q->dev + o_idx1); b.idx2 = (int*)(q->dev + o_idx2); b.p1 = (float*)(q->dev + o_p1); b.p2 = (float*)(q->dev + o_p2);
    b.kept_xy = (int*)(q->dev + o_kxy); b.nk = (int*)(q->dev + o_nk);
    b.models = (double*)(q->dev + o_mod); b.count = (int*)(q->dev + o_cnt); b.words = (unsigned long long*)(q->dev + o_w);
    const int nmax = (int)std::min<size_t>(cap, FE_RANSAC_MAXPTS);
    std::vector<int> sched, tab;
    b.tab_stride = nmax + 1;
    fe_ransac_tables(nmax, sched, tab, b.tab_stride);
    HIPCHK(h, hipMalloc((void**)&q->d_sched, sizeof(int) * std::max<size_t>(sched.size(), 1)));
    HIPCHK(h, hipMalloc((void**)&q->d_tab, sizeof(int) * tab.size()));
    if (!sched.empty()) HIPCHK(h, hipMemcpy(q->d_sched, sched.data(), sizeof(int) * sched.size(), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(q->d_tab, tab.data(), sizeof(int) * tab.size(), hipMemcpyHostToDevice));
    b.niters_tab = q->d_tab;
    q->base_src.assign(S, nullptr);
    return VG_OK;
}

// (the state is attached to the handle only when it is complete: a failed allocation leaves nothing half-made behind)
static int rb_ensure(vg_handle* h, FeState* s) {
    if (s->rb) return VG_OK;
    RbState* q = new RbState();
    const int rc = rb_build(h, s, q);
    if (rc != VG_OK) { rb_free(q); return rc; }
    s->rb = q;
    return VG_OK;
}

// FeatureTracker::readImage for the S streams of the handle, the body of vg_fe_read_image (S == 1) and vg_fe_read_image_batch, which
// have checked h, in, out and S == n_cams; `who` is the entry point the caller used, for the messages.
// `tin` != NULL: the frame of vg_fe_tracks_step -- in[c].n is the length of stream c's resident list and the points are NOT uploaded
// (the tracking reads them where the last commit left them), the walk-order callbacks are tin[c].order, and the frame ends with
// fe_tk_commit_kernel and one download of the new lists instead of block B (tk_collect, below, turns it into `tout`).
// `lists` == false (vg_vio_step_async without VG_VIO_LISTS): only the header block of the new lists comes down, `tout` carries counts.
static int tk_collect(vg_handle* h, const char* who, const int S, const vg_fe_frame_out* fo, vg_fe_tracks_out* tout, bool lists);
static int fe_read_image_streams(vg_handle* h, const char* who, const int S, const vg_fe_frame_in* in, vg_fe_frame_out* out,
                                 const vg_fe_tracks_in* tin = nullptr, vg_fe_tracks_out* tout = nullptr, bool lists = true) {
    FeState* s = h->fe;
    TkState* const tk = tin ? s->tk : nullptr;
    auto refuse = [&](int code, const char* why) { h->err = std::string(who) + ": " + why; return code; };
    if (s->max_pts > 2048) return refuse(VG_ERR_UNSUPPORTED, "max_points > 2048");
    // ---- everything that follows from the arguments alone is refused here: no frame has gone up, no stream has moved
    int n_img = 0, n_pub = 0, first_pub = -1, nmax = 0;
    bool any_ransac = false, any_base = false;
    for (int c = 0; c < S; ++c) {
        const vg_fe_frame_in& f = in[c];
        if (f.struct_size != (int)sizeof(vg_fe_frame_in) || f.n < 0 || (!tk && f.n && !f.cur_xy)) return refuse(VG_ERR_BAD_ARG, "struct_size / n / cur_xy of a stream");
        if (f.n > s->max_pts || f.max_cnt < 0 || f.max_cnt > s->max_pts) return refuse(VG_ERR_BAD_ARG, "n / max_cnt beyond max_points of vg_fe_configure");
        if (f.publish && (f.min_dist < 0 || !(f.f_threshold > 0) || !(f.quality > 0))) return refuse(VG_ERR_BAD_ARG, "min_dist / f_threshold / quality");
        if (f.n > 0 && !s->have_prev) return refuse(VG_ERR_BAD_ARG, "points to track but no previous frame");
        if (f.img && f.stride < s->W) return refuse(VG_ERR_BAD_ARG, "stride smaller than the frame width");
        if ((f.equalize != 0) != (in[0].equalize != 0)) return refuse(VG_ERR_BAD_ARG, "equalize differs between the streams (the image build takes one value)");
        n_img += f.img ? 1 : 0;
        nmax = std::max(nmax, f.n);
        if (f.publish) {
            if (first_pub < 0) first_pub = c;
            else if (f.quality != in[first_pub].quality || f.min_dist != in[first_pub].min_dist)
                return refuse(VG_ERR_BAD_ARG, "quality / min_dist differ between the streams that publish (the detection takes one value)");
            ++n_pub;
            any_ransac = any_ransac || f.n >= 15;
            any_base = any_base || f.base_mask;
        }
    }
    if (n_img != 0 && n_img != S) return refuse(VG_ERR_BAD_ARG, "frames for some streams only (all, or none = the resident frames)");
    const int equalize = in[0].equalize;
    if (const char* why = equalize ? fe_clahe_refusal(s->d) : nullptr) { h->err = why; return VG_ERR_UNSUPPORTED; }
    const int radius = n_pub ? in[first_pub].min_dist : 0;
    const double quality = n_pub ? in[first_pub].quality : 0.01;
    int rc = n_pub ? fe_cell_grid_check(h, s->d, radius) : VG_OK;
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    rc = rb_ensure(h, s);
    if (rc) return rc;
    RbState* q = s->rb;
    const RbDev& b = q->b;
    const size_t npix = (size_t)s->W * s->H, cap = (size_t)b.cap;
    for (int c = 0; c < S; ++c) memset(&out[c], 0, sizeof(out[c]));
    // the fisheye masks travel once per stream (the reference loads them at start-up, feature_tracker_node.cpp)
    if (any_base && !q->d_base) HIPCHK(h, hipMalloc((void**)&q->d_base, npix * S));
    RbDev bd = b;
    bd.base = q->d_base;
    TkDev td;
    const size_t tk_down = tk ? (lists ? tk->bytes : sizeof(int) * TK_HDR_INTS * (size_t)S) : 0;
    if (tk) {
        td.from = tk_buf(tk, tk->dev[tk->cur]); td.to = tk_buf(tk, tk->dev[tk->cur ^ 1]);
        bd.xy_in = td.from.cur_xy;
    }
    for (int c = 0; c < S; ++c)
        if (in[c].publish && in[c].base_mask && in[c].base_mask != q->base_src[c]) {
            HIPCHK(h, hipMemcpyAsync(q->d_base + (size_t)c * npix, in[c].base_mask, npix, hipMemcpyHostToDevice, h->stream));
            q->base_src[c] = in[c].base_mask;
        }
    // ---- upload: the frames (unless they are resident), then ONE block with the point counts, control ints, cameras and cur_pts
    if (n_img) {
        std::vector<const uint8_t*> imgs((size_t)S);
        std::vector<int> strides((size_t)S);
        for (int c = 0; c < S; ++c) { imgs[c] = in[c].img; strides[c] = in[c].stride; }
        rc = fe_upload_async(h, imgs.data(), 0, strides.data());
        if (rc) return rc;
    }
    {
        int* hn = (int*)q->host;
        int* hctl = (int*)(q->host + q->o_ctl);
        RiCam* hcam = (RiCam*)(q->host + q->o_cam);
        float* hxy = (float*)(q->host + q->o_xy);
        memset(hctl, 0, sizeof(int) * RI_CTL_INTS * S);
        for (int c = 0; c < S; ++c) {
            const vg_fe_frame_in& f = in[c];
            hn[c] = f.n;
            hctl[c * RI_CTL_INTS + RI_N] = f.n; hctl[c * RI_CTL_INTS + RI_PUBLISH] = f.publish ? 1 : 0; hctl[c * RI_CTL_INTS + RI_BEST] = -1;
            RiCam& k = hcam[c];
            k.focal = f.focal_length; k.half_w = s->W / 2.0; k.half_h = s->H / 2.0;
            k.cam = fe_stream_camera(s, c, f.intr);
            k.thresh2 = (float)(f.f_threshold * f.f_threshold);
            k.max_cnt = f.max_cnt; k.radius = f.min_dist; k.has_base = (f.publish && f.base_mask) ? 1 : 0;
            if (tk) memcpy(hctl + c * RI_CTL_INTS + RI_STAMP, &tin[c].stamp, sizeof(double));
            else if (f.n) memcpy(hxy + (size_t)c * cap * 2, f.cur_xy, sizeof(float) * 2 * f.n);
        }
        // (cur_pts of the last stream end where its points end; resident lists: the control ints and the cameras are all that travels)
        const size_t bytes = tk ? q->o_xy : q->o_xy + sizeof(float) * 2 * (cap * (S - 1) + in[S - 1].n);
        HIPCHK(h, hipMemcpyAsync(q->d_in, q->host, bytes, hipMemcpyHostToDevice, h->stream));
    }
    rc = vg_fe_build_async(h, equalize);
    if (rc) return rc;
    FeDev d = s->d;
    d.npts = b.npts; d.prev_xy = bd.xy_in; d.skip_idle = 1;
    if (nmax > 0) hipLaunchKernelGGL(fe_lk_kernel, dim3(nmax, S), dim3(64), 0, h->stream, d);
    hipLaunchKernelGGL(fe_rb_after_lk_kernel, dim3(S), dim3(256), 0, h->stream, d, bd);
    // ---- rejectWithF (:169-202) of every stream that publishes; the kernels leave at once for a stream with fewer than 15 survivors.
    // One stream evaluates all iterations in one part (a launch per step); more streams RB_CHUNK0 of them, then what the bookkeeping
    // left to do (fe_ransac.hip).  The only place that asks how many streams there are.
    if (any_ransac) {
        const int chunk = S == 1 ? FE_RANSAC_MAXIT : RB_CHUNK0;
        hipLaunchKernelGGL(fe_rb_ransac7_kernel, dim3((chunk + 6) / 7, S), dim3(64), 0, h->stream, bd, (const int*)q->d_sched, 0, chunk);
        hipLaunchKernelGGL(fe_rb_count_kernel, dim3(chunk, S), dim3(64), 0, h->stream, bd, 0, chunk);
        hipLaunchKernelGGL(fe_rb_pick_kernel, dim3(S), dim3(256), 0, h->stream, d, bd, 0, chunk);
        if (chunk < FE_RANSAC_MAXIT) {
            hipLaunchKernelGGL(fe_rb_ransac7_kernel, dim3(8, S), dim3(64), 0, h->stream, bd, (const int*)q->d_sched, chunk, FE_RANSAC_MAXIT);
            hipLaunchKernelGGL(fe_rb_count_kernel, dim3(56, S), dim3(64), 0, h->stream, bd, chunk, FE_RANSAC_MAXIT);
            hipLaunchKernelGGL(fe_rb_pick_kernel, dim3(S), dim3(256), 0, h->stream, d, bd, chunk, FE_RANSAC_MAXIT);
        }
    }
    HIPCHK(h, hipGetLastError());
    char* hA = q->host + q->in_bytes;
    char* hUn = hA + q->a_bytes;
    char* hB = hUn + q->un_bytes;
    char* hOrd = hB + q->b_bytes;
    // ONE download: block A of every stream, and the lifted survivors when a stream ends its frame here
    if (tk) {
        // resident lists: a step in which no stream publishes is committed here and its lists come down with block A; the counts of
        // the lists travel too when a callback will ask for them
        bool any_cb = false;
        for (int c = 0; c < S; ++c) any_cb = any_cb || (in[c].publish && tin[c].order);
        if (n_pub == 0) {
            hipLaunchKernelGGL(fe_tk_commit_kernel, dim3(S), dim3(256), 0, h->stream, d, bd, td);
            HIPCHK(h, hipGetLastError());
            HIPCHK(h, hipMemcpyAsync(tk->host, tk->dev[tk->cur ^ 1], tk_down, hipMemcpyDeviceToHost, h->stream));
        }
        if (any_cb) HIPCHK(h, hipMemcpyAsync(tk->h_cnt, td.from.cnt, sizeof(int) * cap * S, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(hA, q->d_a, q->a_bytes, hipMemcpyDeviceToHost, h->stream));
    } else
        HIPCHK(h, hipMemcpyAsync(hA, q->d_a, q->a_bytes + (n_pub < S ? q->un_bytes : 0), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int c = 0; c < S; ++c) {
        vg_fe_frame_out& o = out[c];
        char* a = hA + (size_t)c * b.a_stride;
        const int* ahdr = (const int*)a;
        o.status_lk = (const uint8_t*)(a + b.a_st); o.status_f = (const uint8_t*)(a + b.a_sf); o.forw_xy = (const float*)(a + b.a_fw);
        o.n1 = ahdr[RI_N1];
        if (!in[c].publish) {
            o.n2 = o.n_final = o.n1;
            o.un_xy = (const float*)hUn + (size_t)c * cap * 2;
            o.ransac_best = -1;
        } else {
            o.n2 = ahdr[RI_N2]; o.ransac_ran = ahdr[RI_RANSAC]; o.fallback = ahdr[RI_FALLBACK];
            o.ransac_best = ahdr[RI_BEST]; o.ransac_niters = ahdr[RI_NITERS];
        }
        if (o.n1 < 0 || o.n1 > in[c].n || o.n2 < 0 || o.n2 > o.n1) return refuse(VG_ERR_NUMERIC, "inconsistent counts from the device");
    }
    if (n_pub == 0) return tk ? tk_collect(h, who, S, out, tout, lists) : VG_OK;
    // ---- the streams whose estimate the device could not finish (LMedS range, a sample OpenCV would have redrawn): the lifted point
    // sets come back, vg_fe_reject_with_f runs the exact schedule, and the survivor list goes up again
    for (int c = 0; c < S; ++c) {
        vg_fe_frame_out& o = out[c];
        if (!in[c].publish || !o.fallback) continue;
        const int n1 = o.n1;
        std::vector<float> pp((size_t)4 * n1);
        HIPCHK(h, hipMemcpyAsync(pp.data(), b.p1 + (size_t)c * cap * 2, sizeof(float) * 2 * n1, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(pp.data() + 2 * n1, b.p2 + (size_t)c * cap * 2, sizeof(float) * 2 * n1, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        uint8_t* sf = const_cast<uint8_t*>(o.status_f);
        rc = vg_fe_reject_with_f(h, pp.data(), pp.data() + 2 * n1, n1, in[c].f_threshold, sf, nullptr, nullptr);
        if (rc) return rc;
        std::vector<int> idx2;
        for (int i = 0, k = 0; i < in[c].n; ++i)
            if (o.status_lk[i]) { if (sf[k]) idx2.push_back(i); ++k; }
        o.n2 = (int)idx2.size();
        if (o.n2) HIPCHK(h, hipMemcpy(b.idx2 + (size_t)c * cap, idx2.data(), sizeof(int) * idx2.size(), hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(b.ctl + (size_t)c * RI_CTL_INTS + RI_N2, &o.n2, sizeof(int), hipMemcpyHostToDevice));
        o.ransac_best = -1; o.ransac_niters = 0;
    }
    // ---- setMask (:36-69): the order of the walk is the caller's (include/vinsgpu.h): the callbacks in ascending stream order on this
    // thread, then ONE upload of all orders
    int* hflag = (int*)hOrd;
    int* horder = (int*)(hOrd + q->ord_flags_bytes);
    bool any_order = false;
    int max_n2 = 0;
    for (int c = 0; c < S; ++c) {
        hflag[c] = 0;
        if (!in[c].publish) continue;
        const int n2 = out[c].n2;
        max_n2 = std::max(max_n2, n2);
        if (!(tk ? (bool)tin[c].order : (bool)in[c].order) || n2 <= 0) continue;
        int* ord = horder + (size_t)c * cap;
        for (int k = 0; k < n2; ++k) ord[k] = -1;
        int cb_rc;
        if (tk) {
            // the keys setMask sorts by: track_cnt + 1 of the survivors of rejectWithF, in list order
            std::vector<int> keys((size_t)n2);
            const int* cnt = tk->h_cnt + (size_t)c * cap;
            int k1 = 0, k2 = 0;
            for (int i = 0; i < in[c].n; ++i) {
                if (!out[c].status_lk[i]) continue;
                if ((!out[c].ransac_ran || out[c].status_f[k1]) && k2 < n2) keys[k2++] = cnt[i] + 1;
                ++k1;
            }
            if (k2 != n2) return refuse(VG_ERR_NUMERIC, "inconsistent counts from the device");
            cb_rc = tin[c].order(tin[c].user, c, n2, keys.data(), ord);
        } else
            cb_rc = in[c].order(in[c].user, &out[c], ord);
        if (cb_rc != 0) return refuse(VG_ERR_BAD_ARG, "the order callback of a stream failed");
        std::vector<char> seen((size_t)n2, 0);
        for (int k = 0; k < n2; ++k) {
            if (ord[k] < 0 || ord[k] >= n2 || seen[ord[k]]) return refuse(VG_ERR_BAD_ARG, "an order callback did not return a permutation");
            seen[ord[k]] = 1;
        }
        hflag[c] = 1;
        any_order = true;
    }
    if (any_order || q->ord_flags_set) HIPCHK(h, hipMemcpyAsync(q->d_ord, hOrd, any_order ? q->ord_bytes : sizeof(int) * S, hipMemcpyHostToDevice, h->stream));
    q->ord_flags_set = any_order;
    // the masks of the streams that publish: the fisheye mask or 255 (runs of streams without one: one fill)
    for (int c = 0; c < S;) {
        if (!in[c].publish) { ++c; continue; }
        if (in[c].base_mask) {
            HIPCHK(h, hipMemcpyAsync(s->mask + (size_t)c * npix, q->d_base + (size_t)c * npix, npix, hipMemcpyDeviceToDevice, h->stream));
            ++c;
            continue;
        }
        int e = c;
        while (e < S && in[e].publish && !in[e].base_mask) ++e;
        HIPCHK(h, hipMemsetAsync(s->mask + (size_t)c * npix, 255, npix * (e - c), h->stream));
        c = e;
    }
    hipLaunchKernelGGL(fe_rb_setmask_kernel, dim3(S), dim3(64), 0, h->stream, d, bd);
    if (max_n2 > 0) hipLaunchKernelGGL(fe_stamp_kernel, dim3(max_n2, S), dim3(256), 0, h->stream, d, (const int*)b.nk, (const int*)b.kept_xy, radius);
    // ---- goodFeaturesToTrack(forw_img, n_pts, MAX_CNT - forw_pts.size(), 0.01, MIN_DIST, mask) (:144-149) of the streams that publish
    // (the others leave the kernels at once) + addPoints + undistortedPoints
    rc = fe_detect_launch(h, d, quality, (double)radius);
    if (rc) return rc;
    hipLaunchKernelGGL(fe_rb_finish_kernel, dim3(S), dim3(256), 0, h->stream, d, bd);
    if (tk) {
        hipLaunchKernelGGL(fe_tk_commit_kernel, dim3(S), dim3(256), 0, h->stream, d, bd, td);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(tk->host, tk->dev[tk->cur ^ 1], tk_down, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return tk_collect(h, who, S, out, tout, lists);
    }
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(hB, q->d_b, q->b_bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int c = 0; c < S; ++c) {
        if (!in[c].publish) continue;
        vg_fe_frame_out& o = out[c];
        char* q2 = hB + (size_t)c * b.b_stride;
        const int* bhdr = (const int*)q2;
        if (bhdr[RI_NNEW] < 0) { h->err = FE_CAND_OVERFLOW; return VG_ERR_UNSUPPORTED; }
        o.n_kept = bhdr[RI_NK]; o.n_new = bhdr[RI_NNEW]; o.n_final = o.n_kept + o.n_new;
        o.kept = (const int*)(q2 + b.b_k); o.new_xy = (const float*)(q2 + b.b_nw); o.un_xy = (const float*)(q2 + b.b_un);
    }
    return VG_OK;
}

extern "C" int vg_fe_read_image(vg_handle* h, const vg_fe_frame_in* in, vg_fe_frame_out* out) {
    VG_RANGE("vg_fe_read_image");
    if (!h || !h->fe || !in || !out || in->struct_size != (int)sizeof(vg_fe_frame_in) || !in->img) return VG_ERR_BAD_ARG;
    if (h->fe->cams != 1) { h->err = "vg_fe_read_image: one stream per handle (vg_fe_configure with n_cams == 1)"; return VG_ERR_UNSUPPORTED; }
    return fe_read_image_streams(h, "vg_fe_read_image", 1, in, out);
}

extern "C" int vg_fe_read_image_batch(vg_handle* h, int n_streams, const vg_fe_frame_in* in, vg_fe_frame_out* out) {
    VG_RANGE("vg_fe_read_image_batch");
    if (!h || !h->fe || !in || !out || n_streams < 1) return VG_ERR_BAD_ARG;
    if (n_streams != h->fe->cams) { h->err = "vg_fe_read_image_batch: n_streams differs from n_cams of vg_fe_configure (the batched streams advance together)"; return VG_ERR_BAD_ARG; }
    return fe_read_image_streams(h, "vg_fe_read_image_batch", n_streams, in, out);
}

// ================================================================================================ track lists resident on the device
static int tk_ensure(vg_handle* h, FeState* s) {
    if (s->tk) return VG_OK;
    TkState* t = new TkState();
    const size_t cap = (size_t)s->max_pts, S = (size_t)s->cams;
    t->o_ids = ri_up(sizeof(int) * TK_HDR_INTS * S, 256);
    t->o_cnt = t->o_ids + ri_up(sizeof(int) * cap * S, 256);
    t->o_xy = t->o_cnt + ri_up(sizeof(int) * cap * S, 256);
    t->o_un = t->o_xy + ri_up(sizeof(float) * 2 * cap * S, 256);
    t->o_vel = t->o_un + ri_up(sizeof(float) * 2 * cap * S, 256);
    t->o_map = t->o_vel + ri_up(sizeof(float) * 2 * cap * S, 256);
    t->o_mid = t->o_map + ri_up(cap * S, 256);
    t->o_obs = t->o_mid + ri_up(sizeof(int) * cap * S, 256);
    t->bytes = t->o_obs + ri_up(sizeof(double) * 7 * cap * S, 256);
    t->n.assign(S, 0);
    if (hipMalloc((void**)&t->dev[0], t->bytes) != hipSuccess || hipMalloc((void**)&t->dev[1], t->bytes) != hipSuccess ||
        hipHostMalloc((void**)&t->host, t->bytes, 0) != hipSuccess || hipHostMalloc((void**)&t->h_cnt, sizeof(int) * cap * S, 0) != hipSuccess) {
        tk_free(t);
        h->err = "vg_fe_tracks_begin: out of memory for the resident track lists";
        return VG_ERR_HIP;
    }
    s->tk = t;
    return VG_OK;
}

extern "C" int vg_fe_tracks_begin(vg_handle* h) {
    if (!h) return VG_ERR_BAD_ARG;
    if (!h->fe) { h->err = "vg_fe_tracks_begin: the handle has no front end (vg_fe_configure)"; return VG_ERR_BAD_ARG; }
    FeState* s = h->fe;
    if (s->max_pts > TK_MAX) { h->err = "vg_fe_tracks_begin: max_points > 2048"; return VG_ERR_UNSUPPORTED; }
    HIPCHK(h, hipSetDevice(h->device));
    const int rc = tk_ensure(h, s);
    if (rc) return rc;
    TkState* t = s->tk;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemset(t->dev[0], 0, t->bytes));
    HIPCHK(h, hipMemset(t->dev[1], 0, t->bytes));
    t->cur = 0;
    t->n.assign((size_t)s->cams, 0);
    t->begun = true;
    h->ba.seq.vio = false;                // (vg_vio_*: a bridge over the lists just emptied ends here)
    return VG_OK;
}

// the lists the commit kernel left in the pinned mirror -> the caller's vg_fe_tracks_out; the step has succeeded: they become current
static int tk_collect(vg_handle* h, const char* who, const int S, const vg_fe_frame_out* fo, vg_fe_tracks_out* tout, bool lists) {
    FeState* s = h->fe;
    TkState* t = s->tk;
    const size_t cap = (size_t)s->max_pts;
    const TkBuf u = tk_buf(t, t->host);
    for (int c = 0; c < S; ++c) {
        const int* hd = u.hdr + (size_t)c * TK_HDR_INTS;
        if (hd[TK_NNEW] < 0) { h->err = FE_CAND_OVERFLOW; return VG_ERR_UNSUPPORTED; }
        if (hd[TK_N] < 0 || hd[TK_N] > (int)cap || hd[TK_NMSG] < 0 || hd[TK_NMSG] > hd[TK_N]) {
            h->err = std::string(who) + ": inconsistent counts from the device";
            return VG_ERR_NUMERIC;
        }
    }
    for (int c = 0; c < S; ++c) {
        const int* hd = u.hdr + (size_t)c * TK_HDR_INTS;
        vg_fe_tracks_out& o = tout[c];
        memset(&o, 0, sizeof(o));
        o.n = hd[TK_N]; o.n_id = hd[TK_NID]; o.n_msg = hd[TK_NMSG];
        o.n1 = fo[c].n1; o.n2 = fo[c].n2; o.ransac_ran = fo[c].ransac_ran; o.n_kept = hd[TK_NK]; o.n_new = hd[TK_NNEW];
        o.fallback = fo[c].fallback; o.ransac_best = fo[c].ransac_best; o.ransac_niters = fo[c].ransac_niters;
        t->n[c] = o.n;
        if (!lists) continue;
        o.ids = u.ids + c * cap; o.track_cnt = u.cnt + c * cap; o.cur_xy = u.cur_xy + c * cap * 2; o.un_xy = u.un_xy + c * cap * 2;
        o.vel_xy = u.vel + c * cap * 2; o.msg_id = u.msg_id + c * cap; o.msg_obs = u.msg_obs + c * cap * 7;
    }
    t->cur ^= 1;
    return VG_OK;
}

// the body of vg_fe_tracks_step; vg_vio_step_async (ba_host.hip) runs the same frame under its own name, with or without the lists
extern "C" int fe_tracks_step_impl(vg_handle* h, const char* who, int n_streams, const vg_fe_tracks_in* in, vg_fe_tracks_out* out, int lists) {
    if (!h || !h->fe || !in || !out || n_streams < 1) return VG_ERR_BAD_ARG;
    FeState* s = h->fe;
    if (n_streams != s->cams) { h->err = std::string(who) + ": n_streams differs from n_cams of vg_fe_configure (the streams advance together)"; return VG_ERR_BAD_ARG; }
    if (!s->tk || !s->tk->begun) { h->err = std::string(who) + ": no resident lists (vg_fe_tracks_begin)"; return VG_ERR_BAD_ARG; }
    std::vector<vg_fe_frame_in> fin((size_t)n_streams);
    std::vector<vg_fe_frame_out> fout((size_t)n_streams);
    for (int c = 0; c < n_streams; ++c) {
        const vg_fe_tracks_in& t = in[c];
        if (t.struct_size != (int)sizeof(vg_fe_tracks_in)) { h->err = std::string(who) + ": struct_size of a stream"; return VG_ERR_BAD_ARG; }
        vg_fe_frame_in& f = fin[c];
        memset(&f, 0, sizeof(f));
        f.struct_size = (int)sizeof(vg_fe_frame_in);
        f.img = t.img; f.stride = t.stride; f.equalize = t.equalize; f.publish = t.publish;
        f.n = s->tk->n[c];
        f.max_cnt = t.max_cnt; f.min_dist = t.min_dist; f.quality = t.quality; f.f_threshold = t.f_threshold; f.focal_length = t.focal_length;
        memcpy(f.intr, t.intr, sizeof(f.intr));
        f.base_mask = t.base_mask;
    }
    const int rc = fe_read_image_streams(h, who, n_streams, fin.data(), fout.data(), in, out, lists != 0);
    // (an error after the upload: the lists stand as they were -- only a finished step makes the committed copy current -- but the
    //  frames have moved)
    return rc;
}

extern "C" int vg_fe_tracks_step(vg_handle* h, int n_streams, const vg_fe_tracks_in* in, vg_fe_tracks_out* out) {
    VG_RANGE("vg_fe_tracks_step");
    return fe_tracks_step_impl(h, "vg_fe_tracks_step", n_streams, in, out, 1);
}

// what vg_vio_begin / vg_vio_step_async ask the front end: streams and capacity of the resident lists (VG_ERR_BAD_ARG: none begun) ...
extern "C" int fe_vio_limits(vg_handle* h, int* n_cams, int* max_points) {
    FeState* s = h->fe;
    if (!s || !s->tk || !s->tk->begun) return VG_ERR_BAD_ARG;
    *n_cams = s->cams; *max_points = s->max_pts;
    return VG_OK;
}
// ... and where the commit kernel of the last finished step left every stream's message, on the device
extern "C" void fe_vio_message(vg_handle* h, const int** tk_hdr, const int** msg_id, const double** msg_obs) {
    const TkState* t = h->fe->tk;
    const TkBuf u = tk_buf(t, t->dev[t->cur]);
    *tk_hdr = u.hdr; *msg_id = u.msg_id; *msg_obs = u.msg_obs;
}

extern "C" int vg_fe_tracks_get(vg_handle* h, int cam, vg_fe_tracks_state* st) {
    if (!h || !h->fe || !st) return VG_ERR_BAD_ARG;
    FeState* s = h->fe;
    if (!s->tk || !s->tk->begun) { h->err = "vg_fe_tracks_get: no resident lists (vg_fe_tracks_begin)"; return VG_ERR_BAD_ARG; }
    if (cam < 0 || cam >= s->cams || st->struct_size != (int)sizeof(vg_fe_tracks_state)) { h->err = "vg_fe_tracks_get: stream / struct_size"; return VG_ERR_BAD_ARG; }
    TkState* t = s->tk;
    const size_t cap = (size_t)s->max_pts, c = (size_t)cam;
    const TkBuf u = tk_buf(t, t->dev[t->cur]);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    int hd[TK_HDR_INTS];
    HIPCHK(h, hipMemcpy(hd, u.hdr + c * TK_HDR_INTS, sizeof(hd), hipMemcpyDeviceToHost));
    const int n = hd[TK_N];
    if (n < 0 || n > (int)cap) { h->err = "vg_fe_tracks_get: inconsistent counts from the device"; return VG_ERR_NUMERIC; }
    st->n = n; st->n_id = hd[TK_NID];
    memcpy(&st->prev_time, hd + TK_TIME, sizeof(double));
    if (n && st->cur_xy) HIPCHK(h, hipMemcpy(st->cur_xy, u.cur_xy + c * cap * 2, sizeof(float) * 2 * n, hipMemcpyDeviceToHost));
    if (n && st->ids) HIPCHK(h, hipMemcpy(st->ids, u.ids + c * cap, sizeof(int) * n, hipMemcpyDeviceToHost));
    if (n && st->track_cnt) HIPCHK(h, hipMemcpy(st->track_cnt, u.cnt + c * cap, sizeof(int) * n, hipMemcpyDeviceToHost));
    if (n && st->un_xy) HIPCHK(h, hipMemcpy(st->un_xy, u.un_xy + c * cap * 2, sizeof(float) * 2 * n, hipMemcpyDeviceToHost));
    if (n && st->in_map) HIPCHK(h, hipMemcpy(st->in_map, u.in_map + c * cap, n, hipMemcpyDeviceToHost));
    return VG_OK;
}

extern "C" int vg_fe_tracks_set(vg_handle* h, int cam, const vg_fe_tracks_state* st) {
    if (!h || !h->fe || !st) return VG_ERR_BAD_ARG;
    FeState* s = h->fe;
    auto refuse = [&](const char* why) { h->err = std::string("vg_fe_tracks_set: ") + why; return VG_ERR_BAD_ARG; };
    if (!s->tk || !s->tk->begun) return refuse("no resident lists (vg_fe_tracks_begin)");
    if (cam < 0 || cam >= s->cams || st->struct_size != (int)sizeof(vg_fe_tracks_state)) return refuse("stream / struct_size");
    const int n = st->n;
    if (n < 0 || n > s->max_pts || st->n_id < 0) return refuse("n beyond max_points of vg_fe_configure, or a negative n_id");
    if (n && (!st->cur_xy || !st->ids || !st->track_cnt || (st->un_xy && !st->in_map))) return refuse("cur_xy / ids / track_cnt (and in_map with un_xy) are required");
    {
        std::vector<int> sorted(st->ids, st->ids + n);
        std::sort(sorted.begin(), sorted.end());
        for (int k = 0; k < n; ++k) {
            if (sorted[k] < 0 || sorted[k] >= st->n_id) return refuse("an id is negative or not below n_id");
            if (k && sorted[k] == sorted[k - 1]) return refuse("an id occurs twice");
        }
    }
    TkState* t = s->tk;
    const size_t cap = (size_t)s->max_pts, c = (size_t)cam;
    const TkBuf u = tk_buf(t, t->dev[t->cur]);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    int hd[TK_HDR_INTS];
    memset(hd, 0, sizeof(hd));
    hd[TK_N] = n; hd[TK_NID] = st->n_id;
    memcpy(hd + TK_TIME, &st->prev_time, sizeof(double));
    if (n) {
        std::vector<float> un((size_t)2 * n, 0.f);
        std::vector<uint8_t> in_map((size_t)n, 0);
        if (st->un_xy) {
            memcpy(un.data(), st->un_xy, sizeof(float) * 2 * n);
            for (int k = 0; k < n; ++k) in_map[k] = st->in_map[k] ? 1 : 0;
        }
        HIPCHK(h, hipMemcpy(u.cur_xy + c * cap * 2, st->cur_xy, sizeof(float) * 2 * n, hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(u.ids + c * cap, st->ids, sizeof(int) * n, hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(u.cnt + c * cap, st->track_cnt, sizeof(int) * n, hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(u.un_xy + c * cap * 2, un.data(), sizeof(float) * 2 * n, hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(u.in_map + c * cap, in_map.data(), n, hipMemcpyHostToDevice));
    }
    HIPCHK(h, hipMemcpy(u.hdr + c * TK_HDR_INTS, hd, sizeof(hd), hipMemcpyHostToDevice));
    t->n[c] = n;
    return VG_OK;
}
