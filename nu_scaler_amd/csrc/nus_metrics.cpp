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
constexpr uint64_t kMaxPixels = (uint64_t)1 << 30;

// checks of the shape and the metric mask every entry point shares; kOk or the failure, with `who` in its text
int check_shape(const char *who, uint32_t w, uint32_t h, uint32_t frames, int what)
{
    if (w == 0 || h == 0 || frames == 0) return fail(kInvalidArgument, fmt("%s: width, height and frames must be non-zero", who));
    if (what == 0 || (what & ~(kMetricMse | kMetricSsim)))
        return fail(kInvalidArgument, fmt("%s: what must be NUS_METRIC_MSE, NUS_METRIC_SSIM or both (got %d)", who, what));
    if (check_frame_area(who, w, h, kMaxPixels) != kOk) return kInvalidArgument;
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
    if (misaligned(d_workspace, 8) || misaligned(d_out, 8))
        return fail(kInvalidArgument, fmt("%s: workspace and output must be 8-byte aligned", who));
    int st = check_shape(who, w, h, frames, what);
    if (st != kOk || (st = check_pairs(who, d_a, a_stride, d_b, b_stride, w, h)) != kOk) return st;
    const size_t need = metrics_shape(w, h, frames, what & kMetricMse, what & kMetricSsim).workspace_bytes;
    if ((st = check_workspace(who, workspace_bytes, need, "nus_metrics_workspace_size")) != kOk) return st;
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
    int r = check_device(who, device);
    if (r != kOk) return r;

    static PairScratch *const scratch = new PairScratch[kMaxDevices]; // never destroyed: see DeviceBuffer
    PairScratch &s = scratch[device];
    std::lock_guard<std::mutex> lock(s.m);
    const size_t need = metrics_shape(w, h, 1, what & kMetricMse, what & kMetricSsim).workspace_bytes;
    if ((r = s.prepare(device, frame_bytes, need, 3 * sizeof(double))) != kOk) return r;
    // the library's own road for the caller's (possibly pageable) buffers: never handed to the runtime
    if ((r = upload(s.a.get(), a, frame_bytes, s.stream)) != kOk) return r;
    if ((r = upload(s.b.get(), b, frame_bytes, s.stream)) != kOk) return r;
    if ((r = metrics_compare_device(s.a.get(), frame_bytes, s.b.get(), frame_bytes, w, h, 1, what, s.workspace.get(), s.workspace.capacity(),
                                    static_cast<double *>(s.result.get()), s.stream)) != kOk)
        return r;
    return download(out, s.result.get(), 3 * sizeof(double), s.stream);
}

} // namespace nus
