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
#include <vector>
#include "ba_math.h"
#include "imu_step.h"
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
