// nus_host_interp.cpp -- HipFrameInterpolator: the host side of the two-frame warp + blend path
// (WgpuFrameInterpolator::interpolate_py, nu_scaler_core/src/wgpu_interpolator.rs:215-491).  See nus_host.hpp.
#include "nus_host.hpp"

#include "nus_copy.hpp"
#include "nus_host_util.hpp"
#include "nus_retime.hpp"

#include <cstring>

namespace nus {

// ---------------------------------------------------------------------------------
// HipFrameInterpolator
// ---------------------------------------------------------------------------------

namespace {
constexpr uint64_t kMaxPixels = (1ull << 31) - 1;
} // namespace

HipFrameInterpolator::HipFrameInterpolator(int wg_preset) : wg_preset_(wg_preset) {}

HipFrameInterpolator::~HipFrameInterpolator()
{
    release();
    if (device_ready_) {
        if (k_begin_) (void)hipEventDestroy(k_begin_);
        if (k_end_) (void)hipEventDestroy(k_end_);
        if (half_done_) (void)hipEventDestroy(half_done_);
        if (stream_) (void)hipStreamDestroy(stream_);
    }
}

int HipFrameInterpolator::set_device(int device)
{
    std::lock_guard<std::mutex> lk(mu_);
    if (device < 0) return fail(kInvalidArgument, "negative device index");
    if (device_ready_) return fail(kInvalidArgument, "set_device must precede the first interpolation");
    device_ = device;
    return kOk;
}

void HipFrameInterpolator::release()
{
    if (!device_ready_) return;
    (void)hipSetDevice(device_);
    if (stream_) (void)hipStreamSynchronize(stream_);
    if (d_a_) (void)hipFree(d_a_);
    if (d_b_) (void)hipFree(d_b_);
    if (d_out_) (void)hipFree(d_out_);
    if (d_flow_) (void)hipFree(d_flow_);
    pinned_free(h_stage_);
    pinned_free(h_flow_);
    d_a_ = d_b_ = d_out_ = nullptr;
    d_flow_ = nullptr;
    h_stage_ = nullptr;
    h_flow_ = nullptr;
    cap_bytes_ = 0;
    cap_out_ = 0;
    cap_flows_ = 0;
}

int HipFrameInterpolator::ensure(size_t frame_bytes, uint32_t n_flows, uint32_t n_out)
{
    if (!device_ready_) {
        const int rc = select_device(device_);
        if (rc != kOk) return rc;
        NUS_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
        NUS_HIP(hipEventCreate(&k_begin_));
        NUS_HIP(hipEventCreate(&k_end_));
        NUS_HIP(hipEventCreateWithFlags(&half_done_, hipEventDisableTiming));
        device_ready_ = true;
    }
    NUS_HIP(hipSetDevice(device_));
    if (frame_bytes > cap_bytes_ || n_flows > cap_flows_ || n_out > cap_out_) {
        // the reference reallocates its textures on every call (wgpu_interpolator.rs:253-321);
        // here buffers persist and only grow.
        const size_t want = frame_bytes > cap_bytes_ ? frame_bytes : cap_bytes_;
        const uint32_t outs = n_out > cap_out_ ? n_out : cap_out_;
        const uint32_t flows = n_flows > cap_flows_ ? n_flows : cap_flows_;
        release();
        NUS_HIP(hipMalloc(reinterpret_cast<void **>(&d_a_), want));
        NUS_HIP(hipMalloc(reinterpret_cast<void **>(&d_b_), want));
        NUS_HIP(hipMalloc(reinterpret_cast<void **>(&d_out_), want * outs));
        NUS_HIP(pinned_alloc(reinterpret_cast<void **>(&h_stage_), want * (2 + outs)));
        if (flows) { // (the select warp's two flows back to back)
            NUS_HIP(hipMalloc(reinterpret_cast<void **>(&d_flow_), want * 2 * flows));
            NUS_HIP(pinned_alloc(reinterpret_cast<void **>(&h_flow_), want * 2 * flows));
        }
        cap_bytes_ = want;
        cap_out_ = outs;
        cap_flows_ = flows;
    }
    return kOk;
}

int HipFrameInterpolator::initialize(uint32_t width, uint32_t height)
{
    std::lock_guard<std::mutex> lk(mu_);
    int rc = pass(check_dims("initialize", width, height, kMaxPixels));
    if (rc != kOk) return rc;
    if (init_w_ == width && init_h_ == height) return kOk; // interpolation/mod.rs:306-308
    rc = ensure((size_t)width * height * 4, 0);
    if (rc != kOk) return rc;
    init_w_ = width;
    init_h_ = height;
    error_.clear();
    return kOk;
}

int HipFrameInterpolator::interpolate_frames(const uint8_t *frame1, size_t len1, const uint8_t *frame2, size_t len2, float t,
                                             uint8_t *out, size_t out_cap)
{
    uint32_t w, h;
    {
        std::lock_guard<std::mutex> lk(mu_);
        if (init_w_ == 0) return fail(kNotInitialized, "Interpolator not initialized"); // interpolation/mod.rs:368-370
        w = init_w_;
        h = init_h_;
    }
    return interpolate(frame1, len1, frame2, len2, nullptr, w, h, t, out, out_cap);
}

int HipFrameInterpolator::set_quality(InterpolationQuality q)
{
    std::lock_guard<std::mutex> lk(mu_);
    if (q != InterpolationQuality::High && q != InterpolationQuality::Medium && q != InterpolationQuality::Low)
        return fail(kInvalidArgument, "unknown interpolation quality");
    quality_ = q;
    return kOk;
}

int HipFrameInterpolator::interpolate(const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len, const float *flow,
                                      uint32_t w, uint32_t h, float t, uint8_t *out, size_t out_cap)
{
    return host_call("interpolate", a, a_len, b, b_len, flow, nullptr, false, w, h, t, nullptr, 0, false, out, out_cap);
}

int HipFrameInterpolator::interpolate_multi(const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len, const float *flow,
                                            uint32_t w, uint32_t h, const float *times, uint32_t n_times, uint8_t *out, size_t out_cap)
{
    return host_call("nus_interp_interpolate_multi", a, a_len, b, b_len, flow, nullptr, false, w, h, 0.0f, times, n_times, true, out, out_cap);
}

int HipFrameInterpolator::interpolate_select(const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len, const float *flow_fwd,
                                             const float *flow_bwd, uint32_t w, uint32_t h, const float *times, uint32_t n_times, uint8_t *out,
                                             size_t out_cap)
{
    return host_call("nus_interp_interpolate_select", a, a_len, b, b_len, flow_fwd, flow_bwd, true, w, h, 0.0f, times, n_times, true, out,
                     out_cap);
}

int HipFrameInterpolator::host_call(const char *who, const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len, const float *flow,
                                    const float *flow_bwd, bool select, uint32_t w, uint32_t h, float t, const float *times,
                                    uint32_t n_times, bool multi, uint8_t *out, size_t out_cap)
{
    std::lock_guard<std::mutex> lk(mu_);
    int st = pass(check_dims(who, w, h, kMaxPixels));
    if (st != kOk || (st = pass(check_frame_lengths(a_len, b_len, w, h))) != kOk) return st;
    if (!a || !b || !out) return fail(kInvalidArgument, fmt("%s: null frame pointer", who));
    if (select && (!flow || !flow_bwd)) return fail(kInvalidArgument, fmt("%s: null flow pointer (the select warp takes both flows)", who));
    const size_t expected = (size_t)w * h * 4;
    if (!multi) {
        if (out_cap < expected) return fail(kInvalidArgument, fmt("%s: output capacity too small", who));
    } else {
        if ((st = pass(check_interp_times(who, times, n_times))) != kOk) return st;
        if (out_cap / n_times < expected)
            return fail(kInvalidArgument, fmt("%s: output capacity %zu below n_times * w * h * 4 = %zu", who, out_cap, (size_t)n_times * expected));
    }
    return host_pass(a, b, flow, select ? flow_bwd : nullptr, w, h, t, times, n_times, out);
}

int HipFrameInterpolator::host_pass(const uint8_t *a, const uint8_t *b, const float *flow, const float *flow_bwd, uint32_t w, uint32_t h,
                                    float t, const float *times, uint32_t n_times, uint8_t *out)
{
    const size_t expected = (size_t)w * h * 4, total = expected * (n_times ? n_times : 1);
    int rc = ensure(expected, flow_bwd ? 2 : (flow ? 1 : 0), n_times ? n_times : 1);
    if (rc != kOk) return rc;
    uint8_t *ha = h_stage_, *hb = h_stage_ + cap_bytes_, *ho = h_stage_ + 2 * cap_bytes_;
    // while the pair is staged, uploaded and on the GPU, idle workers of the copy pool make the pages of the result buffer
    // present (a buffer fresh from the allocator -- what interpolate_py returns -- otherwise takes its faults in the copy-out)
    struct Populate {
        CopyTicket t;
        ~Populate() { parallel_copy_wait(t); } // on every way out: queued requests point into `out`
    } populate;
    if (parallel_populate_prepare(out, total)) parallel_populate_async(out, total, populate.t);
    // stage A, start its DMA, stage B meanwhile (the reference uploads both synchronously:
    // wgpu_interpolator.rs:253-321)
    parallel_copy(ha, a, expected);
    NUS_HIP(hipMemcpyAsync(d_a_, ha, expected, hipMemcpyHostToDevice, stream_));
    parallel_copy(hb, b, expected);
    NUS_HIP(hipMemcpyAsync(d_b_, hb, expected, hipMemcpyHostToDevice, stream_));
    if (flow) {
        parallel_copy(h_flow_, flow, expected * 2);
        NUS_HIP(hipMemcpyAsync(d_flow_, h_flow_, expected * 2, hipMemcpyHostToDevice, stream_));
    }
    float *d_bwd = nullptr;
    if (flow_bwd) { // the second flow of the select warp, behind the first (cap_bytes_ * 2 bytes each)
        float *const h_bwd = h_flow_ + cap_bytes_ / 2;
        d_bwd = d_flow_ + cap_bytes_ / 2;
        parallel_copy(h_bwd, flow_bwd, expected * 2);
        NUS_HIP(hipMemcpyAsync(d_bwd, h_bwd, expected * 2, hipMemcpyHostToDevice, stream_));
    }
    WarpLaunch L;
    L.a = d_a_;
    L.b = d_b_;
    L.flow = flow ? d_flow_ : nullptr;
    L.out = d_out_;
    L.a_stride = L.b_stride = expected;
    L.w = w;
    L.h = h;
    L.t = t;
    L.times = times;
    L.n_times = n_times;
    L.n_pairs = 1;
    L.stream = stream_;
    L.fma = fma_;
    L.project = project_;
    L.in_sel = input_selector(in_format_);
    NUS_HIP(hipEventRecord(k_begin_, stream_));
    hipError_t e = flow_bwd ? launch_warp_blend_select(WarpSelectLaunch{L, d_bwd}) : launch_warp_blend(L);
    if (e != hipSuccess) return fail_hip(e, flow_bwd ? "select warp+blend launch" : "warp+blend launch");
    NUS_HIP(hipEventRecord(k_end_, stream_));
    // the frames come back in two halves: the host copy of the first overlaps the DMA of the second
    const size_t half = (total / 2 + 4095) & ~(size_t)4095;
    const size_t first = half < total ? half : total;
    NUS_HIP(hipMemcpyAsync(ho, d_out_, first, hipMemcpyDeviceToHost, stream_));
    NUS_HIP(hipEventRecord(half_done_, stream_));
    if (first < total) NUS_HIP(hipMemcpyAsync(ho + first, d_out_ + first, total - first, hipMemcpyDeviceToHost, stream_));
    NUS_HIP(hipEventSynchronize(half_done_));
    parallel_copy(out, ho, first);
    NUS_HIP(hipStreamSynchronize(stream_));
    if (first < total) parallel_copy(out + first, ho + first, total - first);
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, k_begin_, k_end_) == hipSuccess) {
        have_ms_ = true;
        last_ms_ = ms;
    } else {
        (void)hipGetLastError();
    }
    return kOk;
}

int HipFrameInterpolator::interpolate_device(const void *d_a, size_t a_stride, const void *d_b, size_t b_stride,
                                             const void *d_flow, uint32_t w, uint32_t h, float t, void *d_out,
                                             uint32_t n_pairs, hipStream_t stream)
{
    return device_call("interpolate_device", d_a, a_stride, d_b, b_stride, d_flow, nullptr, false, w, h, t, nullptr, 0, false, d_out, 0, n_pairs,
                       stream);
}

int HipFrameInterpolator::interpolate_multi_device(const void *d_a, size_t a_stride, const void *d_b, size_t b_stride,
                                                   const void *d_flow, uint32_t w, uint32_t h, const float *times, uint32_t n_times,
                                                   void *d_out, size_t out_pair_stride, uint32_t n_pairs, hipStream_t stream)
{
    return device_call("nus_interp_interpolate_multi_device", d_a, a_stride, d_b, b_stride, d_flow, nullptr, false, w, h, 0.5f, times, n_times,
                       true, d_out, out_pair_stride, n_pairs, stream);
}

int HipFrameInterpolator::interpolate_select_device(const void *d_a, size_t a_stride, const void *d_b, size_t b_stride, const void *d_flow_fwd,
                                                    const void *d_flow_bwd, uint32_t w, uint32_t h, const float *times, uint32_t n_times,
                                                    void *d_out, size_t out_pair_stride, uint32_t n_pairs, hipStream_t stream)
{
    return device_call("nus_interp_interpolate_select_device", d_a, a_stride, d_b, b_stride, d_flow_fwd, d_flow_bwd, true, w, h, 0.5f, times,
                       n_times, true, d_out, out_pair_stride, n_pairs, stream);
}

int HipFrameInterpolator::device_call(const char *who, const void *d_a, size_t a_stride, const void *d_b, size_t b_stride,
                                      const void *d_flow, const void *d_flow_bwd, bool select, uint32_t w, uint32_t h, float t,
                                      const float *times, uint32_t n_times, bool multi, void *d_out, size_t out_pair_stride,
                                      uint32_t n_pairs, hipStream_t stream)
{
    std::lock_guard<std::mutex> lk(mu_);
    int st = pass(check_dims(who, w, h, kMaxPixels));
    if (st != kOk) return st;
    if (!d_a || !d_b || !d_out) return fail(kInvalidArgument, fmt("%s: null device pointer", who));
    if (select && (!d_flow || !d_flow_bwd)) return fail(kInvalidArgument, fmt("%s: null flow pointer (the select warp takes both flows)", who));
    if (multi && (st = pass(check_interp_times(who, times, n_times))) != kOk) return st;
    if (!multi && n_pairs == 0) return kOk; // (the single-time form has always answered this before it looks at the alignment)
    if ((st = pass(check_pixel_aligned(who, d_a, a_stride, d_b, b_stride, d_out, d_flow, flow_half_ ? 4 : 8))) != kOk) return st;
    if (select && (st = pass(check_pixel_aligned(who, d_a, a_stride, d_b, b_stride, d_out, d_flow_bwd, flow_half_ ? 4 : 8))) != kOk) return st;
    if (multi && (st = pass(check_out_pair_stride(who, out_pair_stride, n_times, (size_t)w * h * 4))) != kOk) return st;
    if (n_pairs == 0) return kOk;
    if (device_count() <= 0) return fail(kNoDevice, "no HIP device available (the gfx950 path has no CPU fallback)");
    NUS_HIP(hipSetDevice(device_));
    WarpLaunch L;
    L.a = static_cast<const uint8_t *>(d_a);
    L.b = static_cast<const uint8_t *>(d_b);
    L.flow = static_cast<const float *>(d_flow);
    L.flow_half = flow_half_;
    L.fma = fma_;
    L.out = static_cast<uint8_t *>(d_out);
    L.a_stride = a_stride;
    L.b_stride = b_stride;
    L.w = w;
    L.h = h;
    L.t = t;
    L.times = times;
    L.n_times = n_times;
    L.out_pair_stride = out_pair_stride;
    L.n_pairs = n_pairs;
    L.stream = stream;
    L.in_sel = input_selector(in_format_);
    L.project = project_;
    const hipError_t e = select ? launch_warp_blend_select(WarpSelectLaunch{L, static_cast<const float *>(d_flow_bwd)}) : launch_warp_blend(L);
    if (e != hipSuccess) return fail_hip(e, select ? "select warp+blend launch" : multi ? "multi-time warp+blend launch" : "warp+blend launch");
    return kOk;
}

int HipFrameInterpolator::retime_device(const void *d_frames, size_t frame_stride, uint32_t n_frames, const void *d_flows, uint32_t w,
                                        uint32_t h, uint32_t num, uint32_t den, void *d_out, size_t out_frame_stride, hipStream_t stream)
{
    return retime_call("nus_interp_retime_device", d_frames, frame_stride, n_frames, d_flows, nullptr, false, w, h, num, den, d_out,
                       out_frame_stride, stream);
}

int HipFrameInterpolator::retime_select_device(const void *d_frames, size_t frame_stride, uint32_t n_frames, const void *d_flows_fwd,
                                               const void *d_flows_bwd, uint32_t w, uint32_t h, uint32_t num, uint32_t den, void *d_out,
                                               size_t out_frame_stride, hipStream_t stream)
{
    return retime_call("nus_interp_retime_select_device", d_frames, frame_stride, n_frames, d_flows_fwd, d_flows_bwd, true, w, h, num, den,
                       d_out, out_frame_stride, stream);
}

int HipFrameInterpolator::retime_call(const char *who, const void *d_frames, size_t frame_stride, uint32_t n_frames, const void *d_flows,
                                      const void *d_flows_bwd, bool select, uint32_t w, uint32_t h, uint32_t num, uint32_t den, void *d_out,
                                      size_t out_frame_stride, hipStream_t stream)
{
    std::lock_guard<std::mutex> lk(mu_);
    if (select && (!d_flows || !d_flows_bwd)) return fail(kInvalidArgument, fmt("%s: null flow pointer (the select warp takes both flows)", who));
    RetimeRatio r;
    int st = pass(check_retime(who, n_frames, num, den, r));
    if (st != kOk || (st = pass(check_dims(who, w, h, kMaxPixels))) != kOk) return st;
    if (!d_frames || !d_out) return fail(kInvalidArgument, fmt("%s: null device pointer", who));
    const size_t frame_bytes = (size_t)w * h * 4;
    if ((st = pass(check_pixel_aligned(who, d_frames, frame_stride, d_frames, frame_stride, d_out, d_flows, flow_half_ ? 4 : 8))) != kOk) return st;
    if (select && (st = pass(check_pixel_aligned(who, d_frames, frame_stride, d_frames, frame_stride, d_out, d_flows_bwd, flow_half_ ? 4 : 8))) != kOk)
        return st;
    if (frame_stride < frame_bytes)
        return fail(kInvalidArgument, fmt("%s: frame_stride %zu is smaller than a %ux%u frame (%zu bytes)", who, frame_stride, w, h, frame_bytes));
    if ((st = pass(check_out_frame_stride(who, out_frame_stride, frame_bytes))) != kOk) return st;
    if (device_count() <= 0) return fail(kNoDevice, "no HIP device available (the gfx950 path has no CPU fallback)");
    NUS_HIP(hipSetDevice(device_));
    RetimeLaunch L;
    L.frames = static_cast<const uint8_t *>(d_frames), L.frame_stride = frame_stride;
    L.first_pair = 0, L.n_pairs = n_frames - 1, L.w = w, L.h = h, L.num = r.num, L.den = r.den;
    L.out = static_cast<uint8_t *>(d_out), L.out_frame_stride = out_frame_stride ? out_frame_stride : frame_bytes;
    L.in_sel = input_selector(in_format_), L.stream = stream;
    RetimeWarp V;
    V.flow = d_flows, V.flow_half = flow_half_, V.fma = fma_, V.project = d_flows ? project_ : 0;
    V.flow_bwd = select ? d_flows_bwd : nullptr;
    const hipError_t e = enqueue_retime(L, V, true);
    if (e != hipSuccess) return fail_hip(e, select ? "retime select warp+blend launch" : "retime warp+blend launch");
    return kOk;
}

int HipFrameInterpolator::set_mode(int mode)
{
    std::lock_guard<std::mutex> lk(mu_);
    if (mode != 0 && mode != 1) return fail(kInvalidArgument, "unknown interpolation mode");
    fma_ = mode == 1;
    return kOk;
}

int HipFrameInterpolator::set_flow_project(uint32_t rounds)
{
    std::lock_guard<std::mutex> lk(mu_);
    if (rounds > kFlowMaxProject)
        return fail(kInvalidArgument, fmt("nus_interp_set_flow_project: 0 .. %u projection rounds, got %u", kFlowMaxProject, rounds));
    project_ = rounds;
    return kOk;
}

int HipFrameInterpolator::set_flow_format(int format)
{
    std::lock_guard<std::mutex> lk(mu_);
    if (format != 0 && format != 1) return fail(kInvalidArgument, "unknown flow format");
    flow_half_ = format == 1;
    return kOk;
}

int HipFrameInterpolator::set_input_format(int format)
{
    std::lock_guard<std::mutex> lk(mu_);
    if (format < 0 || format > 3) return fail(kInvalidArgument, "unknown input format");
    in_format_ = format;
    return kOk;
}

bool HipFrameInterpolator::last_gpu_ms(double *ms) const
{
    std::lock_guard<std::mutex> lk(mu_);
    if (!have_ms_) return false;
    if (ms) *ms = last_ms_;
    return true;
}

} // namespace nus
