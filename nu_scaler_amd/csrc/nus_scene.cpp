// nus_scene.cpp -- host side of the scene-cut detector (nus_scene_* in include/nuscaler_hip.h): the argument checks, which run
// before any HIP call, the enqueue of the device entry points, and the per-device buffers of the host entry point.
#include "nus_scene.hpp"

#include <algorithm>
#include <cstring>
#include <mutex>

#include "nus_host.hpp"
#include "nus_host_util.hpp"
#include "nus_transfer.hpp"

namespace nus {

namespace {

constexpr uint64_t kMaxPixels = (uint64_t)1 << 30;

int check_shape(const char *who, uint32_t w, uint32_t h, uint32_t n_pairs)
{
    if (w == 0 || h == 0) return fail(kInvalidArgument, fmt("%s: width and height must be non-zero", who));
    if (check_frame_area(who, w, h, kMaxPixels) != kOk) return kInvalidArgument;
    const std::string bad = check_scene_launch(w, h, n_pairs);
    if (!bad.empty()) return fail(kInvalidArgument, fmt("%s: %s", who, bad.c_str()));
    return kOk;
}

int check_format(const char *who, int format)
{
    if (format < 0 || format > 3) return fail(kInvalidArgument, fmt("%s: unknown pixel format %d", who, format));
    return kOk;
}

} // namespace

std::string check_scene_launch(uint32_t w, uint32_t h, uint32_t n_pairs)
{
    // one 1-D launch holds at most 2^32 - 1 work-items
    const SceneShape s = scene_shape(w, h, 1);
    const uint64_t blocks = (uint64_t)std::max(s.measure_blocks, s.apply_blocks) * std::max<uint32_t>(n_pairs, 1);
    if (blocks * kSceneBlock > UINT32_MAX)
        return fmt("%u pairs of %ux%u are too many for one launch (%llu workgroups of %u, at most %u)", n_pairs, w, h,
                   (unsigned long long)blocks, kSceneBlock, UINT32_MAX / kSceneBlock);
    return std::string();
}

std::string check_scene_thresholds(uint32_t mad_threshold, uint32_t hist_permille)
{
    if (mad_threshold > 255) return fmt("mad_threshold must be 0..255, got %u", mad_threshold);
    if (hist_permille > 1000) return fmt("hist_permille must be 0..1000, got %u", hist_permille);
    return std::string();
}

uint32_t scene_from_a_mask(const float *times, uint32_t n_times)
{
    uint32_t m = 0;
    for (uint32_t k = 0; k < n_times; ++k)
        if (times[k] < 0.5f) m |= 1u << k;
    return m;
}

size_t scene_workspace_size(uint32_t w, uint32_t h, uint32_t n_pairs)
{
    if (check_shape("nus_scene_workspace_size", w, h, n_pairs) != kOk) return 0;
    return scene_shape(w, h, n_pairs ? n_pairs : 1).workspace_bytes;
}

int scene_detect_device(const void *d_a, size_t a_stride, const void *d_b, size_t b_stride, uint32_t w, uint32_t h, uint32_t n_pairs,
                        int format, uint32_t mad_threshold, uint32_t hist_permille, void *d_workspace, size_t workspace_bytes,
                        void *d_measures, uint8_t *d_cut, hipStream_t stream)
{
    const char *who = "nus_scene_detect_device";
    if (!d_a || !d_b || !d_workspace || !d_cut) return fail(kInvalidArgument, fmt("%s: null pointer", who));
    int st = check_shape(who, w, h, n_pairs);
    if (st != kOk || (st = check_format(who, format)) != kOk || (st = check_pairs(who, d_a, a_stride, d_b, b_stride, w, h)) != kOk) return st;
    const std::string bad = check_scene_thresholds(mad_threshold, hist_permille);
    if (!bad.empty()) return fail(kInvalidArgument, fmt("%s: %s", who, bad.c_str()));
    if (misaligned(d_workspace, 8) || misaligned(d_measures, 8))
        return fail(kInvalidArgument, fmt("%s: workspace and measures must be 8-byte aligned", who));
    if ((st = check_workspace(who, workspace_bytes, scene_shape(w, h, n_pairs ? n_pairs : 1).workspace_bytes, "nus_scene_workspace_size")) != kOk)
        return st;
    if (n_pairs == 0) return kOk;
    if (device_count() <= 0) return fail(kNoDevice, fmt("%s: no HIP device available", who));
    SceneLaunch L;
    L.a = static_cast<const uint8_t *>(d_a);
    L.b = static_cast<const uint8_t *>(d_b);
    L.a_stride = a_stride, L.b_stride = b_stride, L.w = w, L.h = h, L.n_pairs = n_pairs, L.format = format, L.stream = stream;
    const hipError_t e = launch_scene_detect(L, mad_threshold, hist_permille, d_workspace, d_measures, d_cut);
    if (e != hipSuccess) return fail_hip(e, "scene-detect launch");
    return kOk;
}

int scene_apply_cuts_device(const void *d_a, size_t a_stride, const void *d_b, size_t b_stride, uint32_t w, uint32_t h, int format,
                            const float *times, uint32_t n_times, const uint8_t *d_cut, void *d_out, size_t out_pair_stride,
                            uint32_t n_pairs, hipStream_t stream)
{
    const char *who = "nus_scene_apply_cuts_device";
    if (!d_a || !d_b || !d_cut || !d_out) return fail(kInvalidArgument, fmt("%s: null pointer", who));
    int st = check_shape(who, w, h, n_pairs);
    if (st != kOk || (st = check_format(who, format)) != kOk || (st = check_pairs(who, d_a, a_stride, d_b, b_stride, w, h)) != kOk) return st;
    if ((st = check_interp_times(who, times, n_times)) != kOk) return st;
    if (misaligned(d_out, 4)) return fail(kInvalidArgument, fmt("%s: d_out must be 4-byte aligned", who));
    const size_t frame_bytes = (size_t)w * h * 4;
    if ((st = check_out_pair_stride(who, out_pair_stride, n_times, frame_bytes)) != kOk) return st;
    if (n_pairs == 0) return kOk;
    if (device_count() <= 0) return fail(kNoDevice, fmt("%s: no HIP device available", who));
    SceneLaunch L;
    L.a = static_cast<const uint8_t *>(d_a);
    L.b = static_cast<const uint8_t *>(d_b);
    L.a_stride = a_stride, L.b_stride = b_stride, L.w = w, L.h = h, L.n_pairs = n_pairs, L.format = format, L.stream = stream;
    const hipError_t e = launch_scene_apply(L, n_times, scene_from_a_mask(times, n_times), d_cut, static_cast<uint8_t *>(d_out),
                                            out_pair_stride ? out_pair_stride : n_times * frame_bytes);
    if (e != hipSuccess) return fail_hip(e, "scene-apply launch");
    return kOk;
}

int scene_detect(int device, const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len, uint32_t w, uint32_t h, int format,
                 uint32_t mad_threshold, uint32_t hist_permille, void *measures_out, uint8_t *cut_out)
{
    const char *who = "nus_scene_detect";
    if (!a || !b || !cut_out) return fail(kInvalidArgument, fmt("%s: null pointer", who));
    int st = check_shape(who, w, h, 1);
    if (st != kOk || (st = check_format(who, format)) != kOk) return st;
    const std::string bad = check_scene_thresholds(mad_threshold, hist_permille);
    if (!bad.empty()) return fail(kInvalidArgument, fmt("%s: %s", who, bad.c_str()));
    if (a_len != b_len) return fail(kSizeMismatch, "Images must have the same dimensions"); // as nus_metrics_compare
    const size_t frame_bytes = (size_t)w * h * 4;
    if (a_len != frame_bytes)
        return fail(kSizeMismatch, fmt("Input data size (%zu) does not match expected input buffer size (%zu for %ux%u)", a_len,
                                       frame_bytes, w, h));
    int r = check_device(who, device);
    if (r != kOk) return r;

    static PairScratch *const scratch = new PairScratch[kMaxDevices]; // never destroyed: see DeviceBuffer
    PairScratch &s = scratch[device];
    std::lock_guard<std::mutex> lock(s.m);
    if ((r = s.prepare(device, frame_bytes, scene_shape(w, h, 1).workspace_bytes, 32)) != kOk) return r;
    uint8_t *const d_res = static_cast<uint8_t *>(s.result.get()); // 16 bytes of measures, then the flag
    // the library's own road for the caller's (possibly pageable) buffers: never handed to the runtime
    if ((r = upload(s.a.get(), a, frame_bytes, s.stream)) != kOk) return r;
    if ((r = upload(s.b.get(), b, frame_bytes, s.stream)) != kOk) return r;
    if ((r = scene_detect_device(s.a.get(), frame_bytes, s.b.get(), frame_bytes, w, h, 1, format, mad_threshold, hist_permille,
                                 s.workspace.get(), s.workspace.capacity(), d_res, d_res + 16, s.stream)) != kOk)
        return r;
    uint8_t res[17];
    if ((r = download(res, d_res, sizeof res, s.stream)) != kOk) return r;
    if (measures_out) memcpy(measures_out, res, 16);
    *cut_out = res[16];
    return kOk;
}

} // namespace nus
