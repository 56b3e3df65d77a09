// nus_metrics.cpp -- host side of the image-quality metrics (nus_metrics_* in include/nuscaler_hip.h): the argument checks,
// which run before any HIP call, the enqueue of the device entry point, and the per-device buffers of the host entry point.
#include "nus_metrics.hpp"

#include <mutex>

#include "nus_host.hpp"
#include "nus_host_util.hpp"
#include "nus_transfer.hpp"

namespace nus {

namespace {

constexpr int kMetricMse = 1, kMetricSsim = 2; // nus_metric
constexpr int kMaxDevices = 64;

int fail(int status, const std::string &msg)
{
    set_thread_error(msg);
    return status;
}

int fail_hip(hipError_t e, const char *what)
{
    (void)hipGetLastError();
    return fail(e == hipErrorOutOfMemory ? kOutOfMemory : kHipError, fmt("HIP error in %s: %s", what, hipGetErrorString(e)));
}

// checks of the shape and the metric mask every entry point shares; kOk or the failure, with `who` in its text
int check_shape(const char *who, uint32_t w, uint32_t h, uint32_t frames, int what)
{
    if (w == 0 || h == 0 || frames == 0) return fail(kInvalidArgument, fmt("%s: width, height and frames must be non-zero", who));
    if (what == 0 || (what & ~(kMetricMse | kMetricSsim)))
        return fail(kInvalidArgument, fmt("%s: what must be NUS_METRIC_MSE, NUS_METRIC_SSIM or both (got %d)", who, what));
    if ((uint64_t)w * h > ((uint64_t)1 << 30)) return fail(kInvalidArgument, fmt("%s: %ux%u frames are too large", who, w, h));
    if ((what & kMetricSsim) && (w < 11 || h < 11))
        return fail(kInvalidArgument, fmt("%s: SSIM needs frames of at least 11 x 11 pixels (got %ux%u)", who, w, h));
    const MetricsShape s = metrics_shape(w, h, frames, what & kMetricMse, what & kMetricSsim);
    // one 1-D launch holds at most 2^32 - 1 work-items: fewer than 2^24 workgroups of kMetricsBlock lanes
    const uint64_t blocks = (uint64_t)std::max(s.sse_blocks, s.ssim_blocks) * frames;
    if (blocks * kMetricsBlock > UINT32_MAX)
        return fail(kInvalidArgument, fmt("%s: %u frames of %ux%u are too many for one launch (%llu workgroups of %u, at most %u)", who,
                                          frames, w, h, (unsigned long long)blocks, kMetricsBlock, UINT32_MAX / kMetricsBlock));
    return kOk;
}

bool misaligned(const void *p, uintptr_t to) { return (reinterpret_cast<uintptr_t>(p) % to) != 0; }

// the host entry point's device buffers, one set per device, kept for reuse (grown when a larger frame arrives)
struct Slot {
    std::mutex m;
    uint8_t *d_a = nullptr, *d_b = nullptr;
    size_t frame_cap = 0;
    void *ws = nullptr;
    size_t ws_cap = 0;
    double *d_out = nullptr;
    hipStream_t stream = nullptr;
};

Slot &slot_of(int device)
{
    static Slot *slots = new Slot[kMaxDevices]; // never destroyed: the runtime may be gone before a static destructor runs
    return slots[device];
}

int grow(void **p, size_t *cap, size_t bytes, const char *what)
{
    if (*cap >= bytes && *p) return kOk;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    const hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) return fail_hip(e, what);
    *cap = bytes;
    return kOk;
}

} // namespace

size_t metrics_workspace_size(uint32_t w, uint32_t h, uint32_t frames, int what)
{
    if (check_shape("nus_metrics_workspace_size", w, h, frames, what) != kOk) return 0;
    return metrics_shape(w, h, frames, what & kMetricMse, what & kMetricSsim).workspace_bytes;
}

int metrics_compare_device(const void *d_a, size_t a_stride, const void *d_b, size_t b_stride, uint32_t w, uint32_t h,
                           uint32_t frames, int what, void *d_workspace, size_t workspace_bytes, double *d_out, hipStream_t stream)
{
    const char *who = "nus_metrics_compare_device";
    if (!d_a || !d_b || !d_workspace || !d_out) return fail(kInvalidArgument, fmt("%s: null pointer", who));
    if (misaligned(d_a, 4) || misaligned(d_b, 4) || a_stride % 4 || b_stride % 4)
        return fail(kInvalidArgument, fmt("%s: frame pointers and strides must be multiples of 4 bytes", who));
    if (misaligned(d_workspace, 8) || misaligned(d_out, 8))
        return fail(kInvalidArgument, fmt("%s: workspace and output must be 8-byte aligned", who));
    const int st = check_shape(who, w, h, frames, what);
    if (st != kOk) return st;
    const size_t frame_bytes = (size_t)w * h * 4;
    if (a_stride < frame_bytes || b_stride < frame_bytes)
        return fail(kInvalidArgument, fmt("%s: strides (%zu, %zu) are smaller than a %ux%u frame (%zu bytes)", who, a_stride, b_stride,
                                          w, h, frame_bytes));
    const size_t need = metrics_shape(w, h, frames, what & kMetricMse, what & kMetricSsim).workspace_bytes;
    if (workspace_bytes < need)
        return fail(kInvalidArgument, fmt("%s: workspace of %zu bytes, %zu needed (nus_metrics_workspace_size)", who, workspace_bytes, need));
    if (device_count() <= 0) return fail(kNoDevice, fmt("%s: no HIP device available", who));
    const hipError_t e = launch_metrics(static_cast<const uint8_t *>(d_a), a_stride, static_cast<const uint8_t *>(d_b), b_stride, w, h,
                                        frames, what & kMetricMse, what & kMetricSsim, d_workspace, d_out, stream);
    if (e != hipSuccess) return fail_hip(e, "metrics launch");
    return kOk;
}

int metrics_compare(int device, const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len, uint32_t w, uint32_t h, int what,
                    double *out)
{
    const char *who = "nus_metrics_compare";
    if (!a || !b || !out) return fail(kInvalidArgument, fmt("%s: null pointer", who));
    const int st = check_shape(who, w, h, 1, what);
    if (st != kOk) return st;
    if (a_len != b_len) return fail(kSizeMismatch, "Images must have the same dimensions"); // common.rs:486-488
    const size_t frame_bytes = (size_t)w * h * 4;
    if (a_len != frame_bytes)
        return fail(kSizeMismatch, fmt("Input data size (%zu) does not match expected input buffer size (%zu for %ux%u)", a_len,
                                       frame_bytes, w, h));
    const int n = device_count();
    if (n <= 0) return fail(kNoDevice, fmt("%s: no HIP device available", who));
    if (device < 0 || device >= n || device >= kMaxDevices) return fail(kNoDevice, fmt("%s: no HIP device %d", who, device));

    Slot &s = slot_of(device);
    std::lock_guard<std::mutex> lock(s.m);
    NUS_HIP(hipSetDevice(device));
    if (!s.stream) NUS_HIP(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
    if (s.frame_cap < frame_bytes) {
        if (s.d_a) (void)hipFree(s.d_a);
        if (s.d_b) (void)hipFree(s.d_b);
        s.d_a = s.d_b = nullptr;
        s.frame_cap = 0;
        NUS_HIP(hipMalloc(reinterpret_cast<void **>(&s.d_a), frame_bytes));
        NUS_HIP(hipMalloc(reinterpret_cast<void **>(&s.d_b), frame_bytes));
        s.frame_cap = frame_bytes;
    }
    const size_t need = metrics_shape(w, h, 1, what & kMetricMse, what & kMetricSsim).workspace_bytes;
    int r = grow(&s.ws, &s.ws_cap, need, "hipMalloc(metrics workspace)");
    if (r != kOk) return r;
    if (!s.d_out) NUS_HIP(hipMalloc(reinterpret_cast<void **>(&s.d_out), 3 * sizeof(double)));
    // the library's own road for the caller's (possibly pageable) buffers: never handed to the runtime
    if ((r = upload(s.d_a, a, frame_bytes, s.stream)) != kOk) return r;
    if ((r = upload(s.d_b, b, frame_bytes, s.stream)) != kOk) return r;
    if ((r = metrics_compare_device(s.d_a, frame_bytes, s.d_b, frame_bytes, w, h, 1, what, s.ws, s.ws_cap, s.d_out, s.stream)) != kOk)
        return r;
    return download(out, s.d_out, 3 * sizeof(double), s.stream);
}

} // namespace nus
