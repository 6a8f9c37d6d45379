// triangulate.hip — FeatureManager::triangulate (vins_estimator/src/feature_manager.cpp:202-257) on gfx950:
// the initial inverse-depth source of every landmark that Estimator::optimization() then refines
// (solveOdometry, estimator.cpp:596-598; SURVEY.md 8(f) row 4, first half).
//
// One thread per landmark: the 2n x 4 DLT matrix (rows f0*P2 - f2*P0, f1*P2 - f2*P1 of the camera matrices relative
// to the first observing frame, :222-241) lives in a thread-private LDS column ([element][thread], conflict-free);
// its right singular vector of the smallest singular value comes from a one-sided (Hestenes) Jacobi SVD on the four
// columns — the same quantity the reference takes from Eigen::JacobiSVD(...).matrixV().rightCols<1>() (:244);
// depth = v[2] / v[3], replaced by INIT_DEPTH when < 0.1 (:245-254).
#include "vg_range.h"
#include <hip/hip_runtime.h>
#include <vector>
#include "ba_math.h"
#include "tri_dlt.h"
#include "vg_handle.h"
#include "../../include/vinsgpu.h"

extern "C" __global__ __launch_bounds__(64) void triangulate_kernel(int K, const double* __restrict__ Ps, const double* __restrict__ Rs,
                                                                    const double* __restrict__ tic, const double* __restrict__ ric, int L,
                                                                    const int* __restrict__ start, const int* __restrict__ nobs,
                                                                    const int* __restrict__ obs_off, const double* __restrict__ points,
                                                                    double init_depth, double* __restrict__ depth) {
    __shared__ double A[TRI_ROWS * 4][64];
    const int t = threadIdx.x, l = blockIdx.x * 64 + t;
    if (l >= L) return;
    double Ric[9], Tic[3];
    for (int k = 0; k < 9; ++k) Ric[k] = ric[k];
    for (int k = 0; k < 3; ++k) Tic[k] = tic[k];
    const double* pts = points + 3 * (size_t)obs_off[l];
    depth[l] = tri_dlt_depth(A, t, Ps, Rs, Ric, Tic, start[l], nobs[l],
                             [pts](int j, double* p) { p[0] = pts[3 * j]; p[1] = pts[3 * j + 1]; p[2] = pts[3 * j + 2]; }, init_depth);
}

extern "C" int vg_triangulate(vg_handle* h, int K, const double* Ps, const double* Rs, const double* tic, const double* ric, int L,
                              const int* start, const int* nobs, const int* obs_off, const double* points, double init_depth,
                              double* depth) {
    VG_RANGE("vg_triangulate");
    if (!h || K < 1 || !Ps || !Rs || !tic || !ric || L < 0 || (L > 0 && (!start || !nobs || !obs_off || !points || !depth))) return VG_ERR_BAD_ARG;
    if (L == 0) return VG_OK;
    size_t npt = 0;
    for (int l = 0; l < L; ++l) {
        if (nobs[l] < 1 || start[l] < 0 || start[l] + nobs[l] > K || obs_off[l] < 0) { h->err = "vg_triangulate: inconsistent track table"; return VG_ERR_BAD_ARG; }
        if (nobs[l] > TRI_MAXOBS) { h->err = "vg_triangulate: more than 12 observations per landmark"; return VG_ERR_UNSUPPORTED; }
        npt = std::max(npt, (size_t)obs_off[l] + nobs[l]);
    }
    hipError_t e = hipSetDevice(h->device);
    double *d_ps = nullptr, *d_rs = nullptr, *d_ext = nullptr, *d_pts = nullptr, *d_dep = nullptr;
    int* d_tab = nullptr;
    auto fail = [&](hipError_t err) {
        h->err = std::string("vg_triangulate: ") + hipGetErrorString(err);
        (void)hipFree(d_ps); (void)hipFree(d_rs); (void)hipFree(d_ext); (void)hipFree(d_pts); (void)hipFree(d_dep); (void)hipFree(d_tab);
        return VG_ERR_HIP;
    };
    if (e != hipSuccess) return fail(e);
    std::vector<double> ext(12);
    for (int k = 0; k < 3; ++k) ext[k] = tic[k];
    for (int k = 0; k < 9; ++k) ext[3 + k] = ric[k];
    std::vector<int> tab((size_t)3 * L);
    for (int l = 0; l < L; ++l) { tab[l] = start[l]; tab[L + l] = nobs[l]; tab[2 * L + l] = obs_off[l]; }
    if ((e = hipMalloc((void**)&d_ps, sizeof(double) * 3 * K)) != hipSuccess) return fail(e);
    if ((e = hipMalloc((void**)&d_rs, sizeof(double) * 9 * K)) != hipSuccess) return fail(e);
    if ((e = hipMalloc((void**)&d_ext, sizeof(double) * 12)) != hipSuccess) return fail(e);
    if ((e = hipMalloc((void**)&d_pts, sizeof(double) * 3 * npt)) != hipSuccess) return fail(e);
    if ((e = hipMalloc((void**)&d_dep, sizeof(double) * L)) != hipSuccess) return fail(e);
    if ((e = hipMalloc((void**)&d_tab, sizeof(int) * 3 * L)) != hipSuccess) return fail(e);
    if ((e = hipMemcpyAsync(d_ps, Ps, sizeof(double) * 3 * K, hipMemcpyHostToDevice, h->stream)) != hipSuccess) return fail(e);
    if ((e = hipMemcpyAsync(d_rs, Rs, sizeof(double) * 9 * K, hipMemcpyHostToDevice, h->stream)) != hipSuccess) return fail(e);
    if ((e = hipMemcpyAsync(d_ext, ext.data(), sizeof(double) * 12, hipMemcpyHostToDevice, h->stream)) != hipSuccess) return fail(e);
    if ((e = hipMemcpyAsync(d_pts, points, sizeof(double) * 3 * npt, hipMemcpyHostToDevice, h->stream)) != hipSuccess) return fail(e);
    if ((e = hipMemcpyAsync(d_tab, tab.data(), sizeof(int) * 3 * L, hipMemcpyHostToDevice, h->stream)) != hipSuccess) return fail(e);
    hipLaunchKernelGGL(triangulate_kernel, dim3((L + 63) / 64), dim3(64), 0, h->stream, K, d_ps, d_rs, d_ext, d_ext + 3, L, d_tab, d_tab + L,
                       d_tab + 2 * L, d_pts, init_depth, d_dep);
    if ((e = hipGetLastError()) != hipSuccess) return fail(e);
    if ((e = hipMemcpyAsync(depth, d_dep, sizeof(double) * L, hipMemcpyDeviceToHost, h->stream)) != hipSuccess) return fail(e);
    if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return fail(e);
    (void)hipFree(d_ps); (void)hipFree(d_rs); (void)hipFree(d_ext); (void)hipFree(d_pts); (void)hipFree(d_dep); (void)hipFree(d_tab);
    return VG_OK;
}

// ---- vg_init_sfm: GlobalSFM::construct and the per-frame PnP of Estimator::initialStructure for N windows.  Two launches on the
// handle's stream between one upload and one download:
//   init_sfm_kernel        one workgroup (SFM_NT threads) per window: the chain, the triangulations, the full BA, the key entries
//   init_sfm_frame_kernel  one workgroup per (window, non-key entry of all_image_frame): its PnP from the finished structure
// The device functions are csrc/init_sfm.h, the LDS carve csrc/init_sfm_carve.h.
#include <algorithm>
#include <cmath>
#include <string>
#include "init_sfm.h"

static_assert(SF_OK == VG_SFM_OK && SF_FAILED_PNP == VG_SFM_FAILED_PNP && SF_FAILED_BA == VG_SFM_FAILED_BA && SF_FAILED_FRAME == VG_SFM_FAILED_FRAME &&
              SF_NUMERIC == VG_SFM_NUMERIC && SFM_MAX_FRAMES == VG_SFM_MAX_FRAMES && SFM_MAX_FEATURES == VG_SFM_MAX_FEATURES &&
              SFM_MAX_ITERS == VG_SFM_MAX_ITERS, "init_sfm.h repeats the header's constants");

extern __shared__ __attribute__((aligned(16))) char ba_smem[];
#define SF_NK 5     // ints per non-key entry: window | entry | guess | first point | points

extern "C" __global__ __launch_bounds__(SFM_NT) void init_sfm_kernel(int nwin, const int* __restrict__ wi, const int* __restrict__ start,
                                                                     const int* __restrict__ nobs, const int* __restrict__ off,
                                                                     const int* __restrict__ allkey, const double* __restrict__ par,
                                                                     const double* __restrict__ obs, double* __restrict__ res,
                                                                     double* __restrict__ fr, double* __restrict__ ft, double* __restrict__ tr,
                                                                     double* __restrict__ al) {
    const int wd = blockIdx.x, tid = threadIdx.x;
    if (wd >= nwin) return;
    const int* q = wi + SF_WI * wd;
    SfWin w;
    w.F = q[0]; w.l = q[1]; w.n = q[2]; w.n_all = q[3];
    w.start = start + q[4]; w.nobs = nobs + q[4]; w.off = off + q[4];
    w.obs = obs + 2 * (size_t)q[5];
    w.res = res + (size_t)SF_RES * wd; w.fr = fr + (size_t)SF_FR * q[6]; w.ft = ft + (size_t)SF_FT * q[4];
    w.tr = tr + (size_t)SF_TR * SFM_MAX_ITERS * wd;
    const int st = sf_window(w, (double*)ba_smem, par + (size_t)SF_PAR * wd, allkey + q[7], al + (size_t)SF_AL * q[7], tid);
    if (tid == 0) w.res[0] = (double)st;
}

extern "C" __global__ __launch_bounds__(SFM_NT) void init_sfm_frame_kernel(int nnk, const int* __restrict__ nk, const int* __restrict__ wi,
                                                                           const int* __restrict__ feat, const double* __restrict__ xy,
                                                                           const double* __restrict__ par, const double* __restrict__ res,
                                                                           const double* __restrict__ fr, const double* __restrict__ ft,
                                                                           double* __restrict__ al) {
    __shared__ double red[(SFM_NW + 1) * SFM_NRED];
    const int e = blockIdx.x, tid = threadIdx.x;
    if (e >= nnk) return;
    const int* k = nk + SF_NK * e;
    const int wd = k[0];
    if (res[(size_t)SF_RES * wd] != 0.0) return;            // construct failed: the entry stays zero
    const int* q = wi + SF_WI * wd;
    double* o = al + (size_t)SF_AL * (q[7] + k[1]);
    const int st = sf_frame(red, k[4], feat + k[3], xy + 2 * (size_t)k[3], fr + (size_t)SF_FR * (q[6] + k[2]), ft + (size_t)SF_FT * q[4],
                            par + (size_t)SF_PAR * wd + 12, o, tid);
    if (tid == 0) o[13] = (double)st;
}

static bool sf_all_finite(const double* p, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(p[i])) return false;
    return true;
}

// C-ABI: see include/vinsgpu.h
extern "C" int vg_init_sfm(vg_handle* h, int n_windows, const vg_sfm_in* in, vg_sfm_out* out) {
    VG_RANGE("vg_init_sfm");
    if (!h) return VG_ERR_BAD_ARG;
    auto bad = [&](int w, const char* what) {
        h->err = "vg_init_sfm: window " + std::to_string(w) + ": " + what;
        return VG_ERR_BAD_ARG;
    };
    if (n_windows <= 0 || !in || !out) { h->err = "vg_init_sfm: n_windows <= 0 or a NULL argument"; return VG_ERR_BAD_ARG; }
    // ---- everything that follows from the arguments alone, before anything is uploaded or written
    size_t nF = 0, nFeat = 0, nObs = 0, nAll = 0, nPt = 0, nNk = 0;
    int lds_max = 0;
    std::vector<int> ids;
    for (int w = 0; w < n_windows; ++w) {
        const vg_sfm_in& a = in[w];
        if (a.struct_size != sizeof(vg_sfm_in)) return bad(w, "vg_sfm_in::struct_size");
        if (out[w].struct_size != sizeof(vg_sfm_out)) return bad(w, "vg_sfm_out::struct_size");
        const int F = a.n_frames, n = a.n_feat, A = a.n_all;
        if (F < SFM_MIN_FRAMES || F > VG_SFM_MAX_FRAMES) return bad(w, "n_frames outside 3 .. VG_SFM_MAX_FRAMES");
        if (a.l < 0 || a.l > F - 2) return bad(w, "l outside [0, n_frames - 2]");
        if (n < 1 || n > VG_SFM_MAX_FEATURES) return bad(w, "n_feat outside 1 .. VG_SFM_MAX_FEATURES");
        if (!a.feature_id || !a.start || !a.nobs || !a.obs_off || !a.points) return bad(w, "a NULL table");
        if (A < 0 || (A > 0 && (!a.all_key || !a.all_guess || !a.all_off))) return bad(w, "n_all < 0 or a NULL table");
        if (a.obs_off[0] < 0) return bad(w, "obs_off[0] < 0");
        size_t no = 0;
        for (int j = 0; j < n; ++j) {
            if (a.nobs[j] < 1 || a.start[j] < 0 || a.start[j] + a.nobs[j] > F) return bad(w, "start + nobs > n_frames or nobs < 1");
            if (j > 0 && a.obs_off[j] < a.obs_off[j - 1] + a.nobs[j - 1]) return bad(w, "obs_off does not ascend");
            if (!sf_all_finite(a.points + 3 * (size_t)a.obs_off[j], 3 * (size_t)a.nobs[j])) return bad(w, "a non-finite input");
            no += a.nobs[j];
        }
        ids.assign(a.feature_id, a.feature_id + n);
        std::sort(ids.begin(), ids.end());
        if (std::adjacent_find(ids.begin(), ids.end()) != ids.end()) return bad(w, "duplicate feature_id");
        if (!sf_all_finite(a.relative_R, 9) || !sf_all_finite(a.relative_T, 3) || !sf_all_finite(a.ric, 9)) return bad(w, "a non-finite input");
        int next = 0;
        size_t np = 0, nn = 0;
        for (int e = 0; e < A; ++e) {
            if (a.all_key[e] >= 0) {
                if (a.all_key[e] != next) return bad(w, "all_key does not ascend over 0 .. n_frames - 1");
                ++next;
                continue;
            }
            if (a.all_guess[e] < 0 || a.all_guess[e] >= F) return bad(w, "all_guess outside [0, n_frames)");
            const int p0 = a.all_off[e], p1 = a.all_off[e + 1];
            if (p0 < 0 || p1 < p0) return bad(w, "all_off does not ascend");
            if (p1 > p0 && (!a.all_id || !a.all_xy)) return bad(w, "a NULL table");
            if (p1 > p0 && !sf_all_finite(a.all_xy + 2 * (size_t)p0, 2 * (size_t)(p1 - p0))) return bad(w, "a non-finite input");
            np += p1 - p0; ++nn;
        }
        if (A > 0 && next != F) return bad(w, "all_key does not cover 0 .. n_frames - 1 exactly once");
        const SfmLds c = sfm_lds(F, n);
        if (c.ch < 1) return bad(w, "the window does not fit the LDS carve");
        lds_max = std::max(lds_max, c.end);
        nF += F; nFeat += n; nObs += no; nAll += A; nPt += np; nNk += nn;
    }
    if (nObs > (size_t)0x3fffffff || nPt > (size_t)0x3fffffff) { h->err = "vg_init_sfm: too many observations for one call"; return VG_ERR_BAD_ARG; }
    // ---- one host image of the upload: doubles [par | obs | xy], ints [wi | start | nobs | off | allkey | feat | nk]; the download follows
    const size_t o_par = 0, o_obs = o_par + (size_t)SF_PAR * n_windows, o_xy = o_obs + 2 * nObs, n_in = o_xy + 2 * (nPt ? nPt : 1);
    const size_t o_res = 0, o_fr = o_res + (size_t)SF_RES * n_windows, o_ft = o_fr + (size_t)SF_FR * nF, o_tr = o_ft + (size_t)SF_FT * nFeat,
                 o_al = o_tr + (size_t)SF_TR * SFM_MAX_ITERS * n_windows, n_out = o_al + (size_t)SF_AL * (nAll ? nAll : 1);
    const size_t i_wi = 0, i_st = i_wi + (size_t)SF_WI * n_windows, i_nb = i_st + nFeat, i_of = i_nb + nFeat, i_ak = i_of + nFeat,
                 i_ft = i_ak + (nAll ? nAll : 1), i_nk = i_ft + (nPt ? nPt : 1), n_int = (i_nk + SF_NK * (nNk ? nNk : 1) + 1) & ~(size_t)1;
    std::vector<double> hin(n_in, 0.0), hout(n_out);
    std::vector<int> hint(n_int, 0);
    {
        size_t f = 0, ft = 0, ob = 0, al = 0, pt = 0, nk = 0;
        std::vector<std::pair<int, int>> byid;
        for (int w = 0; w < n_windows; ++w) {
            const vg_sfm_in& a = in[w];
            const int F = a.n_frames, n = a.n_feat, A = a.n_all;
            int* wi = hint.data() + i_wi + (size_t)SF_WI * w;
            wi[0] = F; wi[1] = a.l; wi[2] = n; wi[3] = A; wi[4] = (int)ft; wi[5] = (int)ob; wi[6] = (int)f; wi[7] = (int)al;
            double* p = hin.data() + o_par + (size_t)SF_PAR * w;
            std::copy(a.relative_R, a.relative_R + 9, p); std::copy(a.relative_T, a.relative_T + 3, p + 9); std::copy(a.ric, a.ric + 9, p + 12);
            int no = 0;
            byid.clear();
            for (int j = 0; j < n; ++j) {
                hint[i_st + ft + j] = a.start[j]; hint[i_nb + ft + j] = a.nobs[j]; hint[i_of + ft + j] = no;
                for (int k = 0; k < a.nobs[j]; ++k) {
                    const double* s = a.points + 3 * ((size_t)a.obs_off[j] + k);
                    hin[o_obs + 2 * (ob + no + k)] = s[0]; hin[o_obs + 2 * (ob + no + k) + 1] = s[1];
                }
                no += a.nobs[j];
                byid.emplace_back(a.feature_id[j], j);
            }
            std::sort(byid.begin(), byid.end());
            for (int e = 0; e < A; ++e) {
                hint[i_ak + al + e] = a.all_key[e];
                if (a.all_key[e] >= 0) continue;
                const int p0 = a.all_off[e], p1 = a.all_off[e + 1];
                int* k = hint.data() + i_nk + SF_NK * nk;
                k[0] = w; k[1] = e; k[2] = a.all_guess[e]; k[3] = (int)pt; k[4] = p1 - p0;
                for (int q = p0; q < p1; ++q) {
                    auto it = std::lower_bound(byid.begin(), byid.end(), std::make_pair(a.all_id[q], -1));
                    hint[i_ft + pt] = (it != byid.end() && it->first == a.all_id[q]) ? it->second : -1;
                    hin[o_xy + 2 * pt] = a.all_xy[2 * (size_t)q]; hin[o_xy + 2 * pt + 1] = a.all_xy[2 * (size_t)q + 1];
                    ++pt;
                }
                ++nk;
            }
            f += F; ft += n; ob += no; al += A;
        }
    }
    hipError_t e = hipSetDevice(h->device);
    auto fail = [&](hipError_t err) { h->err = std::string("vg_init_sfm: ") + hipGetErrorString(err); return VG_ERR_HIP; };
    if (e != hipSuccess) return fail(e);
    const size_t need = (n_in + n_out) * sizeof(double) + n_int * sizeof(int);
    if (need > h->imu_cap) {                                // the scratch of vg_imu_preintegrate / vg_init_align (all three calls are synchronous)
        if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return fail(e);
        (void)hipFree(h->imu_buf);
        h->imu_buf = nullptr; h->imu_cap = 0;
        if ((e = hipMalloc(&h->imu_buf, 2 * need)) != hipSuccess) return fail(e);
        h->imu_cap = 2 * need;
    }
    double* d_in = (double*)h->imu_buf;
    double* d_out = d_in + n_in;
    int* d_int = (int*)(d_out + n_out);
    const size_t lds = (size_t)lds_max * sizeof(double);
    // (the limit belongs to the function, not to the call: always the whole CU, so that no other thread's smaller call can lower it
    //  between this line and the launch)
    if ((e = hipFuncSetAttribute((const void*)init_sfm_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, SFM_CU_LDS)) != hipSuccess) return fail(e);
    if ((e = hipMemcpyAsync(d_in, hin.data(), n_in * sizeof(double), hipMemcpyHostToDevice, h->stream)) != hipSuccess) return fail(e);
    if ((e = hipMemcpyAsync(d_int, hint.data(), n_int * sizeof(int), hipMemcpyHostToDevice, h->stream)) != hipSuccess) return fail(e);
    if ((e = hipMemsetAsync(d_out, 0, n_out * sizeof(double), h->stream)) != hipSuccess) return fail(e);
    struct Events {                                         // destroyed on every way out
        hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
        ~Events() { for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x); }
    } evs;
    hipEvent_t* ev = evs.ev;
    const bool timed = out[0].device_ms != nullptr;
    if (timed)
        for (int i = 0; i < 3; ++i)
            if ((e = hipEventCreate(&ev[i])) != hipSuccess) return fail(e);
    if (timed && (e = hipEventRecord(ev[0], h->stream)) != hipSuccess) return fail(e);
    hipLaunchKernelGGL(init_sfm_kernel, dim3(n_windows), dim3(SFM_NT), lds, h->stream, n_windows, d_int + i_wi, d_int + i_st, d_int + i_nb,
                       d_int + i_of, d_int + i_ak, d_in + o_par, d_in + o_obs, d_out + o_res, d_out + o_fr, d_out + o_ft, d_out + o_tr,
                       d_out + o_al);
    if (timed && (e = hipEventRecord(ev[1], h->stream)) != hipSuccess) return fail(e);
    if (nNk > 0)
        hipLaunchKernelGGL(init_sfm_frame_kernel, dim3((unsigned)nNk), dim3(SFM_NT), 0, h->stream, (int)nNk, d_int + i_nk, d_int + i_wi,
                           d_int + i_ft, d_in + o_xy, d_in + o_par, d_out + o_res, d_out + o_fr, d_out + o_ft, d_out + o_al);
    if (timed && (e = hipEventRecord(ev[2], h->stream)) != hipSuccess) return fail(e);
    if ((e = hipGetLastError()) != hipSuccess) return fail(e);
    if ((e = hipMemcpyAsync(hout.data(), d_out, n_out * sizeof(double), hipMemcpyDeviceToHost, h->stream)) != hipSuccess) return fail(e);
    if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return fail(e);
    if (timed) {
        float a = 0.f, b = 0.f;
        if ((e = hipEventElapsedTime(&a, ev[0], ev[1])) != hipSuccess || (e = hipEventElapsedTime(&b, ev[1], ev[2])) != hipSuccess) return fail(e);
        out[0].device_ms[0] = a; out[0].device_ms[1] = b;
    }
    {
        size_t f = 0, ft = 0, al = 0;
        for (int w = 0; w < n_windows; ++w) {
            const int F = in[w].n_frames, n = in[w].n_feat, A = in[w].n_all;
            const double* r = hout.data() + o_res + (size_t)SF_RES * w;
            const double* pf = hout.data() + o_fr + (size_t)SF_FR * f;
            const double* pt = hout.data() + o_ft + (size_t)SF_FT * ft;
            const double* pa = hout.data() + o_al + (size_t)SF_AL * al;
            const double* tr = hout.data() + o_tr + (size_t)SF_TR * SFM_MAX_ITERS * w;
            vg_sfm_out& o = out[w];
            int st = (int)r[0];
            const bool built = st == VG_SFM_OK || st == VG_SFM_FAILED_BA;       // construct reached the BA: the taps and the state exist
            if (st == VG_SFM_OK)
                for (int a = 0; a < A && st == VG_SFM_OK; ++a)
                    if (pa[SF_AL * a + 12] == 0.0) st = (int)pa[SF_AL * a + 13];
            o.status = st;
            o.ba_iters = (int)r[1]; o.ba_termination = (int)r[2]; o.final_cost = r[3];
            for (int k = 0; k < VG_SFM_MAX_ITERS; ++k) {
                o.it_cost[k] = tr[SF_TR * k]; o.it_cost_cand[k] = tr[SF_TR * k + 1]; o.it_model[k] = tr[SF_TR * k + 2];
                o.it_radius[k] = tr[SF_TR * k + 3]; o.it_flags[k] = (int)tr[SF_TR * k + 4];
            }
            for (int i = 0; i < F; ++i) {
                const double* q = pf + SF_FR * i;
                if (o.q) std::copy(q, q + 4, o.q + 4 * i);
                if (o.T) std::copy(q + 4, q + 7, o.T + 3 * i);
                if (o.q0) std::copy(q + 7, q + 11, o.q0 + 4 * i);
                if (o.T0) std::copy(q + 11, q + 14, o.T0 + 3 * i);
                if (o.pnp_iters) o.pnp_iters[i] = (int)q[14];
                if (o.pnp_up) o.pnp_up[i] = (int)q[15];
            }
            for (int j = 0; j < n; ++j) {
                const double* q = pt + SF_FT * j;
                if (o.state) o.state[j] = built ? (int)q[0] : 0;
                if (o.position) std::copy(q + 1, q + 4, o.position + 3 * j);
                if (o.position0)
                    for (int k = 0; k < 3; ++k) o.position0[3 * j + k] = built ? q[4 + k] : 0.0;
            }
            for (int a = 0; a < A; ++a) {
                const double* q = pa + SF_AL * a;
                if (o.R_all) std::copy(q, q + 9, o.R_all + 9 * a);
                if (o.T_all) std::copy(q + 9, q + 12, o.T_all + 3 * a);
                if (o.is_key) o.is_key[a] = ((int)r[0] == VG_SFM_OK && in[w].all_key[a] >= 0) ? 1 : 0;
            }
            f += F; ft += n; al += A;
        }
    }
    return VG_OK;
}
