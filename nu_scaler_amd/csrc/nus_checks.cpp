// nus_checks.cpp -- see nus_checks.hpp.
#include "nus_checks.hpp"

#include <cstdarg>
#include <cstdio>

namespace nus {

namespace {
thread_local std::string g_thread_error;
} // namespace

void set_thread_error(const std::string &msg) { g_thread_error = msg; }
const char *thread_error() { return g_thread_error.c_str(); }

std::string fmt(const char *f, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}

int fail(int status, const std::string &msg)
{
    set_thread_error(msg);
    return status;
}

int check_dims(const char *who, uint32_t w, uint32_t h, uint64_t max_pixels, const char *text)
{
    if (w == 0 || h == 0 || (uint64_t)w * h > max_pixels) return fail(kInvalidArgument, fmt("%s: %s", who, text));
    return kOk;
}

int check_frame_area(const char *who, uint32_t w, uint32_t h, uint64_t max_pixels)
{
    if ((uint64_t)w * h > max_pixels) return fail(kInvalidArgument, fmt("%s: %ux%u frames are too large", who, w, h));
    return kOk;
}

int check_pairs(const char *who, const void *a, size_t a_stride, const void *b, size_t b_stride, uint32_t w, uint32_t h)
{
    if (misaligned(a, 4) || misaligned(b, 4) || a_stride % 4 || b_stride % 4)
        return fail(kInvalidArgument, fmt("%s: frame pointers and strides must be multiples of 4 bytes", who));
    const size_t frame_bytes = (size_t)w * h * 4;
    if (a_stride < frame_bytes || b_stride < frame_bytes)
        return fail(kInvalidArgument, fmt("%s: strides (%zu, %zu) are smaller than a %ux%u frame (%zu bytes)", who, a_stride, b_stride,
                                          w, h, frame_bytes));
    return kOk;
}

int check_pixel_aligned(const char *who, const void *a, size_t a_stride, const void *b, size_t b_stride, const void *out,
                        const void *flow, uintptr_t flow_align, const void *also)
{
    if (misaligned(a, 4) || misaligned(b, 4) || misaligned(out, 4) || a_stride % 4 || b_stride % 4 || misaligned(also, 4) ||
        misaligned(flow, flow_align))
        return fail(kInvalidArgument, fmt("%s: pointers/strides must be pixel aligned", who));
    return kOk;
}

int check_frame_lengths(size_t a_len, size_t b_len, uint32_t w, uint32_t h)
{
    const size_t expected = (size_t)w * h * 4;
    if (a_len != expected || b_len != expected)
        return fail(kSizeMismatch, fmt("Expected %zu bytes per frame for %ux%ux4 RGBA, got frame_a: %zu bytes, frame_b: %zu bytes",
                                       expected, w, h, a_len, b_len));
    return kOk;
}

int check_interp_times(const char *who, const float *times, uint32_t n_times)
{
    if (!times) return fail(kInvalidArgument, fmt("%s: times is null", who));
    if (n_times == 0 || n_times > kMaxInterpTimes)
        return fail(kInvalidArgument, fmt("%s: n_times must be 1..%u, got %u", who, kMaxInterpTimes, n_times));
    for (uint32_t k = 0; k < n_times; ++k)
        if (!(times[k] >= 0.0f && times[k] <= 1.0f))
            return fail(kInvalidArgument, fmt("%s: times[%u] = %g is not in [0, 1]", who, k, (double)times[k]));
    return kOk;
}

int check_out_pair_stride(const char *who, size_t out_pair_stride, uint32_t n_times, size_t frame_bytes)
{
    if (out_pair_stride != 0 && (out_pair_stride < n_times * frame_bytes || out_pair_stride % 4))
        return fail(kInvalidArgument, fmt("%s: out_pair_stride %zu must be 0 or a multiple of 4 of at least n_times * w * h * 4 = %zu", who,
                                          out_pair_stride, n_times * frame_bytes));
    return kOk;
}

int check_workspace(const char *who, size_t workspace_bytes, size_t need, const char *sizer)
{
    if (workspace_bytes < need)
        return fail(kInvalidArgument, fmt("%s: workspace of %zu bytes, %zu needed (%s)", who, workspace_bytes, need, sizer));
    return kOk;
}

} // namespace nus
