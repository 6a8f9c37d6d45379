// imu_preint.hip — batched IMU pre-integration on gfx950: IntegrationBase::push_back / propagate /
// midPointIntegration / repropagate (vins_estimator/src/factor/integration_base.h:30-158), i.e. the step in
// Estimator::processIMU (estimator.cpp:93-101) that produces the constants IMUFactor::Evaluate consumes
// (the caller-side neighbour of the BA hot path).
//
// One wavefront per frame interval (the intervals of all windows of a batch are independent); the per-sample body is
// csrc/imu_step.h, shared with the sequences that integrate on the device (csrc/ba_seq.hip).  repropagate() is the same
// computation started from the stored first sample with new linearisation biases, so one entry point serves both.
#include "vg_range.h"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include "ba_math.h"
#include "imu_step.h"
#include "init_align.h"
#include "vg_handle.h"
#include "../../include/vinsgpu.h"

extern "C" __global__ __launch_bounds__(64) void imu_preint_kernel(int n, const int* __restrict__ off, const double* __restrict__ samples,
                                                                   const double* __restrict__ first, const double* __restrict__ bias,
                                                                   double acc_n, double gyr_n, double acc_w, double gyr_w,
                                                                   double* __restrict__ out) {
    __shared__ ImuPreLds s;
    const int k = blockIdx.x, lane = threadIdx.x;
    if (k >= n) return;
    ImuRun r;
    imu_enter(s, r, nullptr, first + 6 * k, bias + 6 * k, acc_n, gyr_n, acc_w, gyr_w, lane);
    for (int si = off[k]; si < off[k + 1]; ++si) imu_push_back(s, r, samples + (size_t)si * 7, lane);
    imu_leave(s, r, out + (size_t)k * IMU_OUT, lane);
}

// C-ABI: see include/vinsgpu.h
extern "C" int vg_imu_preintegrate(vg_handle* h, int n_intervals, const int* sample_off, const double* samples, const double* first,
                                   const double* bias, const double* noise, vg_imu_preint* out) {
    VG_RANGE("vg_imu_preintegrate");
    if (!h || n_intervals <= 0 || !sample_off || !samples || !first || !bias || !noise || !out) return VG_ERR_BAD_ARG;
    if (sample_off[0] != 0) { h->err = "vg_imu_preintegrate: sample_off[0] must be 0"; return VG_ERR_BAD_ARG; }
    for (int k = 0; k < n_intervals; ++k)
        if (sample_off[k + 1] < sample_off[k]) { h->err = "vg_imu_preintegrate: sample_off must be non-decreasing"; return VG_ERR_BAD_ARG; }
    const size_t S = (size_t)sample_off[n_intervals];
    hipError_t e = hipSetDevice(h->device);
    std::vector<double> host((size_t)n_intervals * IMU_OUT);
    auto fail = [&](hipError_t err) { h->err = std::string("vg_imu_preintegrate: ") + hipGetErrorString(err); return VG_ERR_HIP; };
    if (e != hipSuccess) return fail(e);
    // one scratch allocation per handle, grown on demand (this call sits on the per-frame path of a sequence: a hipMalloc /
    // hipFree pair per call would synchronise the device every frame): [samples | first | bias | out | offsets]
    const size_t nd = 7 * (S ? S : 1) + 12 * (size_t)n_intervals + (size_t)IMU_OUT * n_intervals;
    const size_t need = nd * sizeof(double) + sizeof(int) * ((size_t)n_intervals + 1);
    if (need > h->imu_cap) {
        if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return fail(e);
        (void)hipFree(h->imu_buf);
        h->imu_buf = nullptr; h->imu_cap = 0;
        if ((e = hipMalloc(&h->imu_buf, 2 * need)) != hipSuccess) return fail(e);
        h->imu_cap = 2 * need;
    }
    double* d_s = (double*)h->imu_buf;
    double* d_f = d_s + 7 * (S ? S : 1);
    double* d_b = d_f + 6 * (size_t)n_intervals;
    double* d_o = d_b + 6 * (size_t)n_intervals;
    int* d_off = (int*)(d_o + (size_t)IMU_OUT * n_intervals);
    if ((e = hipMemcpyAsync(d_off, sample_off, sizeof(int) * (n_intervals + 1), hipMemcpyHostToDevice, h->stream)) != hipSuccess) return fail(e);
    if (S && (e = hipMemcpyAsync(d_s, samples, sizeof(double) * 7 * S, hipMemcpyHostToDevice, h->stream)) != hipSuccess) return fail(e);
    if ((e = hipMemcpyAsync(d_f, first, sizeof(double) * 6 * n_intervals, hipMemcpyHostToDevice, h->stream)) != hipSuccess) return fail(e);
    if ((e = hipMemcpyAsync(d_b, bias, sizeof(double) * 6 * n_intervals, hipMemcpyHostToDevice, h->stream)) != hipSuccess) return fail(e);
    hipLaunchKernelGGL(imu_preint_kernel, dim3(n_intervals), dim3(64), 0, h->stream, n_intervals, d_off, d_s, d_f, d_b,
                       noise[0], noise[1], noise[2], noise[3], d_o);
    if ((e = hipGetLastError()) != hipSuccess) return fail(e);
    if ((e = hipMemcpyAsync(host.data(), d_o, sizeof(double) * IMU_OUT * n_intervals, hipMemcpyDeviceToHost, h->stream)) != hipSuccess) return fail(e);
    if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return fail(e);
    for (int k = 0; k < n_intervals; ++k) {
        const double* o = host.data() + (size_t)k * IMU_OUT;
        vg_imu_preint& q = out[k];
        q.sum_dt = o[0];
        for (int i = 0; i < 3; ++i) { q.delta_p[i] = o[1 + i]; q.delta_v[i] = o[8 + i]; q.linearized_ba[i] = o[11 + i]; q.linearized_bg[i] = o[14 + i]; }
        for (int i = 0; i < 4; ++i) q.delta_q[i] = o[4 + i];
        for (int i = 0; i < 225; ++i) { q.jacobian[i] = o[17 + i]; q.covariance[i] = o[242 + i]; }
        q.valid = 1;
        q._pad = 0;
    }
    return VG_OK;
}

// ---- vg_init_align: VisualIMUAlignment + the state change of visualInitialAlign.  Four launches on the handle's stream:
//   imu_preint_kernel      the intervals of all windows with (ba0, bg0)                  (one wavefront per interval, as above)
//   init_align_bias_kernel solveGyroscopeBias per window; the biases (0, bg0 + delta_bg)  (one wavefront per window)
//   imu_preint_kernel      again with those: the records the call returns, the SAME kernel vg_imu_preintegrate launches
//   init_align_kernel      LinearAlignment, RefineGravity, the window stage              (one workgroup = one wavefront per window)
// The device functions are csrc/init_align.h, the LDS carve csrc/init_align_carve.h.
static_assert(AL_OK == VG_ALIGN_OK && AL_FAILED_LINEAR == VG_ALIGN_FAILED_LINEAR && AL_FAILED_REFINE == VG_ALIGN_FAILED_REFINE &&
              AL_NUMERIC == VG_ALIGN_NUMERIC && AL_MAX_FRAMES == VG_ALIGN_MAX_FRAMES, "init_align.h repeats the header's constants");
static_assert(sizeof(vg_imu_preint) == (IMU_OUT + 1) * sizeof(double), "a record is IMU_OUT doubles and the valid flag");

extern __shared__ __attribute__((aligned(16))) char ba_smem[];
#define AL_WI 5     // ints per window: F | K | first frame | first interval | first key
#define AL_RES_NOBIAS 27    // res[27] != 0: solveGyroscopeBias failed, the records were not re-propagated
extern "C" __global__ __launch_bounds__(64) void init_align_bias_kernel(int nwin, const int* __restrict__ wi, const double* __restrict__ R,
                                                                        const double* __restrict__ par, const double* __restrict__ rec,
                                                                        double* __restrict__ res, double* __restrict__ bias) {
    const int w = blockIdx.x, lane = threadIdx.x;
    if (w >= nwin) return;
    const int F = wi[AL_WI * w], fb = wi[AL_WI * w + 2], ib = wi[AL_WI * w + 3];
    double* r = res + (size_t)AL_RES * w;
    const int st = al_gyro_bias(F, R + (size_t)9 * fb, rec + (size_t)IMU_OUT * ib, par + (size_t)AL_PAR * w, r, bias + (size_t)6 * ib, lane);
    if (lane == 0) { r[0] = (double)st; r[AL_RES_NOBIAS] = st == AL_OK ? 0.0 : 1.0; }
}

extern "C" __global__ __launch_bounds__(64) void init_align_kernel(int nwin, const int* __restrict__ wi, const int* __restrict__ key,
                                                                   const double* __restrict__ R, const double* __restrict__ T,
                                                                   const double* __restrict__ par, const double* __restrict__ rec,
                                                                   double* __restrict__ res, double* __restrict__ vbody,
                                                                   double* __restrict__ win) {
    const int w = blockIdx.x, lane = threadIdx.x;
    if (w >= nwin) return;
    double* r = res + (size_t)AL_RES * w;
    if (r[0] != 0.0) return;                                // solveGyroscopeBias failed
    const int F = wi[AL_WI * w], K = wi[AL_WI * w + 1], fb = wi[AL_WI * w + 2], ib = wi[AL_WI * w + 3], kb = wi[AL_WI * w + 4];
    const int st = al_window((double*)ba_smem, F, K, R + (size_t)9 * fb, T + (size_t)3 * fb, rec + (size_t)IMU_OUT * ib, key + kb,
                             par + (size_t)AL_PAR * w, r, vbody + (size_t)3 * fb, win + (size_t)AL_WIN * kb, lane);
    if (lane == 0) r[0] = (double)st;
}

static void imu_record_from(const double* o, vg_imu_preint& q) {
    q.sum_dt = o[0];
    for (int i = 0; i < 3; ++i) { q.delta_p[i] = o[1 + i]; q.delta_v[i] = o[8 + i]; q.linearized_ba[i] = o[11 + i]; q.linearized_bg[i] = o[14 + i]; }
    for (int i = 0; i < 4; ++i) q.delta_q[i] = o[4 + i];
    for (int i = 0; i < 225; ++i) { q.jacobian[i] = o[17 + i]; q.covariance[i] = o[242 + i]; }
    q.valid = 1;
    q._pad = 0;
}

static bool al_all_finite(const double* p, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(p[i])) return false;
    return true;
}

// C-ABI: see include/vinsgpu.h
extern "C" int vg_init_align(vg_handle* h, int n_windows, const vg_align_in* in, vg_align_out* out) {
    VG_RANGE("vg_init_align");
    if (!h) return VG_ERR_BAD_ARG;
    auto bad = [&](int w, const char* what) {
        h->err = "vg_init_align: window " + std::to_string(w) + ": " + what;
        return VG_ERR_BAD_ARG;
    };
    if (n_windows <= 0 || !in || !out) { h->err = "vg_init_align: n_windows <= 0 or a NULL argument"; return VG_ERR_BAD_ARG; }
    // ---- everything that follows from the arguments alone, before anything is uploaded or written
    size_t nF = 0, nI = 0, nK = 0, nS = 0;
    int Fmax = 0;
    for (int w = 0; w < n_windows; ++w) {
        const vg_align_in& a = in[w];
        if (a.struct_size != sizeof(vg_align_in)) return bad(w, "vg_align_in::struct_size");
        if (out[w].struct_size != sizeof(vg_align_out)) return bad(w, "vg_align_out::struct_size");
        const int F = a.n_frames, K = a.n_key;
        if (F < 2 || F > VG_ALIGN_MAX_FRAMES) return bad(w, "n_frames outside 2 .. VG_ALIGN_MAX_FRAMES");
        if (!a.R || !a.T || !a.sample_off || !a.samples || !a.first) return bad(w, "a NULL table");
        if (K != 0 && (K < 2 || K > F)) return bad(w, "n_key is neither 0 nor 2 .. n_frames");
        if (K > 0 && !a.key) return bad(w, "n_key > 0 without a key list");
        if (K > 0 && (!out[w].Ps || !out[w].Rs || !out[w].Vs)) return bad(w, "n_key > 0 without Ps / Rs / Vs");
        if (a.sample_off[0] < 0) return bad(w, "sample_off[0] < 0");
        for (int k = 0; k + 1 < F; ++k)
            if (a.sample_off[k + 1] <= a.sample_off[k]) return bad(w, "sample_off does not ascend (an empty interval)");
        for (int k = 0; k < K; ++k)
            if (a.key[k] < 0 || a.key[k] >= F || (k > 0 && a.key[k] <= a.key[k - 1])) return bad(w, "key does not ascend inside [0, n_frames)");
        const size_t s0 = (size_t)a.sample_off[0], s1 = (size_t)a.sample_off[F - 1];
        if (!al_all_finite(a.R, 9 * (size_t)F) || !al_all_finite(a.T, 3 * (size_t)F) || !al_all_finite(a.samples + 7 * s0, 7 * (s1 - s0)) ||
            !al_all_finite(a.first, 6 * (size_t)(F - 1)) || !al_all_finite(a.ba0, 3) || !al_all_finite(a.bg0, 3) || !al_all_finite(a.noise, 4) ||
            !al_all_finite(a.tic, 3) || !std::isfinite(a.g_norm))
            return bad(w, "a non-finite input");
        nF += F; nI += F - 1; nK += K; nS += s1 - s0;
        Fmax = F > Fmax ? F : Fmax;
    }
    if (nS > (size_t)0x7fffffff / 7) { h->err = "vg_init_align: too many sample rows for one call"; return VG_ERR_BAD_ARG; }
    // ---- one host image of the upload: doubles [R | T | samples | first | par | bias], ints [wi | ioff | key]; the download follows it
    const size_t o_R = 0, o_T = o_R + 9 * nF, o_s = o_T + 3 * nF, o_f = o_s + 7 * nS, o_par = o_f + 6 * nI, o_b = o_par + (size_t)AL_PAR * n_windows, n_in = o_b + 6 * nI;
    const size_t o_res = 0, o_vb = o_res + (size_t)AL_RES * n_windows, o_rec = o_vb + 3 * nF, o_win = o_rec + (size_t)IMU_OUT * nI,
                 n_out = o_win + (size_t)AL_WIN * (nK ? nK : 1);
    const size_t i_wi = 0, i_so = i_wi + (size_t)AL_WI * n_windows, i_key = i_so + nI + 1, n_int = (i_key + (nK ? nK : 1) + 1) & ~(size_t)1;
    std::vector<double> hin(n_in), hout(n_out);
    std::vector<int> hint(n_int, 0);
    {
        size_t f = 0, iv = 0, kk = 0, sr = 0;
        for (int w = 0; w < n_windows; ++w) {
            const vg_align_in& a = in[w];
            const int F = a.n_frames, K = a.n_key, s0 = a.sample_off[0], ns = a.sample_off[F - 1] - s0;
            int* wi = hint.data() + i_wi + (size_t)AL_WI * w;
            wi[0] = F; wi[1] = K; wi[2] = (int)f; wi[3] = (int)iv; wi[4] = (int)kk;
            std::copy(a.R, a.R + 9 * F, hin.data() + o_R + 9 * f);
            std::copy(a.T, a.T + 3 * F, hin.data() + o_T + 3 * f);
            std::copy(a.samples + 7 * (size_t)s0, a.samples + 7 * (size_t)(s0 + ns), hin.data() + o_s + 7 * sr);
            std::copy(a.first, a.first + 6 * (F - 1), hin.data() + o_f + 6 * iv);
            double* p = hin.data() + o_par + (size_t)AL_PAR * w;
            for (int i = 0; i < 3; ++i) { p[i] = a.ba0[i]; p[3 + i] = a.bg0[i]; p[10 + i] = a.tic[i]; }
            for (int i = 0; i < 4; ++i) p[6 + i] = a.noise[i];
            p[13] = a.g_norm;
            for (int k = 0; k < F; ++k) hint[i_so + iv + k] = (int)sr + (a.sample_off[k] - s0);     // rows of the packed sample table: interval iv + k is
                                                                                                     // [ioff[iv + k], ioff[iv + k + 1]); the next window starts where this one ends
            for (int k = 0; k + 1 < F; ++k)
                for (int i = 0; i < 3; ++i) { hin[o_b + 6 * (iv + k) + i] = a.ba0[i]; hin[o_b + 6 * (iv + k) + 3 + i] = a.bg0[i]; }
            for (int k = 0; k < K; ++k) hint[i_key + kk + k] = a.key[k];
            f += F; iv += F - 1; kk += K; sr += ns;
        }
    }
    hipError_t e = hipSetDevice(h->device);
    auto fail = [&](hipError_t err) { h->err = std::string("vg_init_align: ") + hipGetErrorString(err); return VG_ERR_HIP; };
    if (e != hipSuccess) return fail(e);
    const size_t need = (n_in + n_out) * sizeof(double) + n_int * sizeof(int);
    if (need > h->imu_cap) {                                // the scratch of vg_imu_preintegrate (both calls are synchronous)
        if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return fail(e);
        (void)hipFree(h->imu_buf);
        h->imu_buf = nullptr; h->imu_cap = 0;
        if ((e = hipMalloc(&h->imu_buf, 2 * need)) != hipSuccess) return fail(e);
        h->imu_cap = 2 * need;
    }
    double* d_in = (double*)h->imu_buf;
    double* d_out = d_in + n_in;
    int* d_int = (int*)(d_out + n_out);
    const AlignLds carve = align_lds(Fmax);
    const size_t lds = (size_t)carve.end * sizeof(double);
    if ((e = hipFuncSetAttribute((const void*)init_align_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(align_lds(AL_MAX_FRAMES).end * sizeof(double)))) != hipSuccess) return fail(e);
    if ((e = hipMemcpyAsync(d_in, hin.data(), n_in * sizeof(double), hipMemcpyHostToDevice, h->stream)) != hipSuccess) return fail(e);
    if ((e = hipMemcpyAsync(d_int, hint.data(), n_int * sizeof(int), hipMemcpyHostToDevice, h->stream)) != hipSuccess) return fail(e);
    if ((e = hipMemsetAsync(d_out, 0, n_out * sizeof(double), h->stream)) != hipSuccess) return fail(e);
    // imu_preint_kernel takes one set of noise densities per launch: one launch per run of windows that share theirs (usually one)
    auto integrate = [&]() {
        size_t iv = 0;
        for (int w0 = 0; w0 < n_windows;) {
            int w1 = w0 + 1;
            size_t n = (size_t)in[w0].n_frames - 1;
            while (w1 < n_windows && std::memcmp(in[w1].noise, in[w0].noise, sizeof(in[w0].noise)) == 0) n += (size_t)in[w1++].n_frames - 1;
            const double* nz = in[w0].noise;
            hipLaunchKernelGGL(imu_preint_kernel, dim3((unsigned)n), dim3(64), 0, h->stream, (int)n, d_int + i_so + iv, d_in + o_s, d_in + o_f + 6 * iv,
                               d_in + o_b + 6 * iv, nz[0], nz[1], nz[2], nz[3], d_out + o_rec + (size_t)IMU_OUT * iv);
            iv += n; w0 = w1;
        }
    };
    integrate();
    hipLaunchKernelGGL(init_align_bias_kernel, dim3(n_windows), dim3(64), 0, h->stream, n_windows, d_int + i_wi, d_in + o_R, d_in + o_par,
                       d_out + o_rec, d_out + o_res, d_in + o_b);
    integrate();
    hipLaunchKernelGGL(init_align_kernel, dim3(n_windows), dim3(64), lds, h->stream, n_windows, d_int + i_wi, d_int + i_key, d_in + o_R,
                       d_in + o_T, d_in + o_par, d_out + o_rec, d_out + o_res, d_out + o_vb, d_out + o_win);
    if ((e = hipGetLastError()) != hipSuccess) return fail(e);
    if ((e = hipMemcpyAsync(hout.data(), d_out, n_out * sizeof(double), hipMemcpyDeviceToHost, h->stream)) != hipSuccess) return fail(e);
    if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return fail(e);
    {
        size_t f = 0, iv = 0, kk = 0;
        for (int w = 0; w < n_windows; ++w) {
            const int F = in[w].n_frames, K = in[w].n_key;
            const double* r = hout.data() + o_res + (size_t)AL_RES * w;
            vg_align_out& o = out[w];
            o.status = (int)r[0];
            for (int i = 0; i < 3; ++i) { o.delta_bg[i] = r[1 + i]; o.bg[i] = r[4 + i]; o.g_lin[i] = r[7 + i]; o.g_c0[i] = r[11 + i]; o.g_w[i] = r[15 + i]; }
            o.s_lin = r[10]; o.s = r[14];
            for (int i = 0; i < 9; ++i) o.R0[i] = r[18 + i];
            if (o.v_body) std::copy(hout.data() + o_vb + 3 * f, hout.data() + o_vb + 3 * (f + F), o.v_body);
            if (o.records)
                for (int k = 0; k < F - 1; ++k) {
                    if (r[AL_RES_NOBIAS] != 0.0) std::memset(&o.records[k], 0, sizeof(vg_imu_preint));
                    else imu_record_from(hout.data() + o_rec + (size_t)IMU_OUT * (iv + k), o.records[k]);
                }
            for (int k = 0; k < K; ++k) {
                const double* q = hout.data() + o_win + (size_t)AL_WIN * (kk + k);
                std::copy(q, q + 3, o.Ps + 3 * k); std::copy(q + 3, q + 12, o.Rs + 9 * k); std::copy(q + 12, q + 15, o.Vs + 3 * k);
            }
            f += F; iv += F - 1; kk += K;
        }
    }
    return VG_OK;
}
