// nus_retime.cpp -- host side of the frame-rate conversion that belongs to no handle (nus_retime_* and
// nus_scene_apply_cuts_retime_device of include/nuscaler_hip.h): the argument checks every retime entry point shares, which run
// before any HIP call, the schedule as a host table, and the enqueue of the two handle-free device entry points.
#include "nus_retime.hpp"

#include <numeric>

#include "nus_host.hpp"
#include "nus_host_util.hpp"
#include "nus_scene.hpp"

namespace nus {

int check_retime(const char *who, uint64_t n_frames, uint32_t num, uint32_t den, RetimeRatio &r)
{
    if (num == 0 || den == 0) return fail(kInvalidArgument, fmt("%s: the ratio's terms must be non-zero, got %u/%u", who, num, den));
    if (num > kRetimeMaxTerm || den > kRetimeMaxTerm)
        return fail(kInvalidArgument, fmt("%s: the ratio's terms must be at most %u, got %u/%u", who, kRetimeMaxTerm, num, den));
    const uint32_t g = std::gcd(num, den);
    r.num = num / g, r.den = den / g;
    if (r.num > kRetimeMaxRatio * r.den)
        return fail(kInvalidArgument, fmt("%s: the ratio must be at most %u, got %u/%u", who, kRetimeMaxRatio, num, den));
    if (n_frames < 2) return fail(kInvalidArgument, fmt("%s: a stream needs at least 2 frames", who));
    return kOk;
}

int check_out_frame_stride(const char *who, size_t out_frame_stride, size_t frame_bytes)
{
    if (out_frame_stride != 0 && (out_frame_stride < frame_bytes || out_frame_stride % 4))
        return fail(kInvalidArgument, fmt("%s: out_frame_stride must be 0 or a multiple of 4 of at least w * h * 4 = %zu bytes, got %zu", who,
                                          frame_bytes, out_frame_stride));
    return kOk;
}

int64_t retime_count_checked(uint64_t n_frames, uint32_t num, uint32_t den)
{
    RetimeRatio r;
    const int st = check_retime("nus_retime_count", n_frames, num, den, r);
    return st != kOk ? st : (int64_t)retime_count(n_frames, r);
}

int retime_schedule(uint64_t n_frames, uint32_t num, uint32_t den, uint64_t first, uint64_t count, RetimeEntry *out)
{
    static const char *const who = "nus_retime_schedule";
    RetimeRatio r;
    const int st = check_retime(who, n_frames, num, den, r);
    if (st != kOk) return st;
    const uint64_t n_out = retime_count(n_frames, r);
    if (first > n_out || count > n_out - first)
        return fail(kInvalidArgument, fmt("%s: the window [%llu, %llu + %llu) is outside the %llu outputs", who, (unsigned long long)first,
                                          (unsigned long long)first, (unsigned long long)count, (unsigned long long)n_out));
    if (count != 0 && !out) return fail(kInvalidArgument, fmt("%s: null pointer", who));
    for (uint64_t i = 0; i < count; ++i) out[i] = retime_entry(first + i, r);
    return kOk;
}

int retime_schedule_device(uint32_t n_frames, uint32_t num, uint32_t den, void *d_entries, void *stream)
{
    static const char *const who = "nus_retime_schedule_device";
    RetimeRatio r;
    const int st = check_retime(who, n_frames, num, den, r);
    if (st != kOk) return st;
    if (!d_entries || misaligned(d_entries, 4)) return fail(kInvalidArgument, fmt("%s: d_entries must be a 4-byte aligned device pointer", who));
    if (device_count() <= 0) return fail(kNoDevice, fmt("%s: no HIP device available", who));
    const hipError_t e = launch_retime_table(n_frames, r.num, r.den, d_entries, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail_hip(e, "retime-table launch");
    return kOk;
}

int scene_apply_cuts_retime_device(const void *d_frames, size_t frame_stride, uint32_t n_frames, uint32_t w, uint32_t h, int format,
                                   uint32_t num, uint32_t den, const uint8_t *d_cut, void *d_out, size_t out_frame_stride, void *stream)
{
    static const char *const who = "nus_scene_apply_cuts_retime_device";
    RetimeRatio r;
    int st = check_retime(who, n_frames, num, den, r);
    if (st != kOk) return st;
    if (!d_frames || !d_cut || !d_out) return fail(kInvalidArgument, fmt("%s: null pointer", who));
    if (w == 0 || h == 0) return fail(kInvalidArgument, fmt("%s: width and height must be non-zero", who));
    if ((st = check_frame_area(who, w, h, (uint64_t)1 << 30)) != kOk) return st;
    if (format < 0 || format > 3) return fail(kInvalidArgument, fmt("%s: unknown pixel format %d", who, format));
    if ((st = check_pairs(who, d_frames, frame_stride, d_frames, frame_stride, w, h)) != kOk) return st;
    if (misaligned(d_out, 4)) return fail(kInvalidArgument, fmt("%s: d_out must be 4-byte aligned", who));
    const size_t frame_bytes = (size_t)w * h * 4;
    if ((st = check_out_frame_stride(who, out_frame_stride, frame_bytes)) != kOk) return st;
    if (device_count() <= 0) return fail(kNoDevice, fmt("%s: no HIP device available", who));
    RetimeLaunch L;
    L.frames = static_cast<const uint8_t *>(d_frames), L.frame_stride = frame_stride;
    L.first_pair = 0, L.n_pairs = n_frames - 1, L.w = w, L.h = h, L.num = r.num, L.den = r.den;
    L.out = static_cast<uint8_t *>(d_out), L.out_frame_stride = out_frame_stride ? out_frame_stride : frame_bytes;
    L.in_sel = input_selector(format), L.stream = static_cast<hipStream_t>(stream);
    const hipError_t e = launch_scene_apply_retime(L, d_cut);
    if (e != hipSuccess) return fail_hip(e, "retime scene-apply launch");
    return kOk;
}

} // namespace nus
