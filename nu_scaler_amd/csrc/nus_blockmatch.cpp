// nus_blockmatch.cpp -- host side of the block-matching motion estimator: the rank tables of the tie orders, the argument
// checks (all before any HIP call), the enqueue of the device entry point and the host entry points' device buffers.
#include "nus_blockmatch.hpp"

#include <algorithm>

#include "nus_host.hpp"
#include "nus_host_util.hpp"
#include "nus_retime.hpp"
#include "nus_scene.hpp"
#include "nus_transfer.hpp"

namespace nus {

namespace {

// where the tables of (R, order) start in the handle's device array: per radius 1 .. kBmMaxRadius and per order, rank then cand
size_t table_offset(uint32_t R, int order)
{
    size_t o = 0;
    for (uint32_t r = 1; r < R; ++r) o += (size_t)4 * (2 * r + 1) * (2 * r + 1);
    return o + (size_t)order * 2 * (2 * R + 1) * (2 * R + 1);
}

constexpr uint64_t kMaxPixels = (1ull << 31) - 1;

size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }

} // namespace

void bm_rank_tables(uint32_t R, int order, std::vector<uint16_t> &rank, std::vector<uint16_t> &cand)
{
    const int D = 2 * (int)R + 1, n = D * D;
    cand.resize(n);
    rank.resize(n);
    for (int c = 0; c < n; ++c) cand[c] = (uint16_t)c; // scan order: dy outer, dx inner, ascending
    if (order == kBmTiesCenter) {
        const auto d2 = [&](int c) {
            const int dy = c / D - (int)R, dx = c % D - (int)R;
            return dx * dx + dy * dy;
        };
        std::stable_sort(cand.begin(), cand.end(), [&](uint16_t p, uint16_t q) { return d2(p) < d2(q); });
    }
    for (int r = 0; r < n; ++r) rank[cand[r]] = (uint16_t)r;
}

BlockMatcher::~BlockMatcher()
{
    if (!d_tables_ && !arena_.get() && !stream_) return;
    (void)hipSetDevice(device_);
    if (stream_) {
        (void)hipStreamSynchronize(stream_);
        (void)hipStreamDestroy(stream_);
    }
    arena_.release();
    if (d_tables_) (void)hipFree(d_tables_);
}

int BlockMatcher::set_device(int device)
{
    std::lock_guard<std::mutex> lk(mu_);
    if (device < 0) return fail(kInvalidArgument, "nus_bm_set_device: negative device index");
    if (d_tables_) return fail(kInvalidArgument, "nus_bm_set_device: must precede the first estimate");
    device_ = device;
    return kOk;
}

int BlockMatcher::set_params(uint32_t block_size, uint32_t search_radius)
{
    std::lock_guard<std::mutex> lk(mu_);
    if (block_size != 8 && block_size != 16 && block_size != 32)
        return fail(kInvalidArgument, fmt("nus_bm_set_params: block_size must be 8, 16 or 32, got %u", block_size));
    if (search_radius < 1 || search_radius > kBmMaxRadius)
        return fail(kInvalidArgument, fmt("nus_bm_set_params: search_radius must be 1..%u, got %u", kBmMaxRadius, search_radius));
    bs_ = block_size;
    radius_ = search_radius;
    return kOk;
}

int BlockMatcher::set_quality(int quality)
{
    std::lock_guard<std::mutex> lk(mu_);
    static const uint32_t preset[3][2] = {{8, 24}, {16, 16}, {32, 8}}; // interpolation/mod.rs:531-542
    if (quality < 0 || quality > 2) return fail(kInvalidArgument, fmt("nus_bm_set_quality: unknown interpolation quality %d", quality));
    bs_ = preset[quality][0];
    radius_ = preset[quality][1];
    return kOk;
}

int BlockMatcher::set_tie_order(int order)
{
    std::lock_guard<std::mutex> lk(mu_);
    if (order != kBmTiesScan && order != kBmTiesCenter)
        return fail(kInvalidArgument, fmt("nus_bm_set_tie_order: order must be NUS_BM_TIES_SCAN or NUS_BM_TIES_CENTER, got %d", order));
    order_ = order;
    return kOk;
}

int BlockMatcher::set_refine(int enabled)
{
    std::lock_guard<std::mutex> lk(mu_);
    if (enabled != 0 && enabled != 1) return fail(kInvalidArgument, fmt("nus_bm_set_refine: 0 or 1, got %d", enabled));
    refine_ = enabled == 1;
    return kOk;
}

int BlockMatcher::set_bidirectional(int enabled, uint32_t tolerance)
{
    std::lock_guard<std::mutex> lk(mu_);
    if (enabled != 0 && enabled != 1) return fail(kInvalidArgument, fmt("nus_bm_set_bidirectional: 0 or 1, got %d", enabled));
    if (tolerance > kBmMaxTolerance)
        return fail(kInvalidArgument, fmt("nus_bm_set_bidirectional: tolerance must be 0..%u, got %u", kBmMaxTolerance, tolerance));
    bidir_ = enabled == 1;
    tolerance_ = tolerance;
    return kOk;
}

int BlockMatcher::set_scene_detect(int enabled, uint32_t mad_threshold, uint32_t hist_permille)
{
    std::lock_guard<std::mutex> lk(mu_);
    if (enabled != 0 && enabled != 1) return fail(kInvalidArgument, fmt("nus_bm_set_scene_detect: 0 or 1, got %d", enabled));
    const std::string bad = check_scene_thresholds(mad_threshold, hist_permille);
    if (!bad.empty()) return fail(kInvalidArgument, fmt("nus_bm_set_scene_detect: %s", bad.c_str()));
    scene_ = enabled == 1;
    scene_mad_ = mad_threshold;
    scene_hist_ = hist_permille;
    return kOk;
}

int BlockMatcher::check_shape(const char *who, uint32_t w, uint32_t h, uint32_t n_pairs)
{
    const int st = pass(check_dims(who, w, h, kMaxPixels));
    if (st != kOk) return st;
    // the search grid is (runs, block rows, pairs): 65535 on its second and third axis
    if ((h + bs_ - 1) / bs_ > 65535u || n_pairs > 65535u)
        return fail(kInvalidArgument, fmt("%s: %u pairs of %ux%u are too many for one launch (at most 65535 pairs and block rows)", who,
                                          n_pairs, w, h));
    return kOk;
}

size_t BlockMatcher::workspace_size(uint32_t w, uint32_t h, uint32_t n_pairs)
{
    std::lock_guard<std::mutex> lk(mu_);
    if (check_shape("nus_bm_workspace_size", w, h, n_pairs) != kOk) return 0;
    return bm_shape(w, h, bs_, n_pairs ? n_pairs : 1, bidir_).workspace_bytes;
}

int BlockMatcher::ensure_tables()
{
    int rc = select_device(device_);
    if (rc != kOk || d_tables_) return rc;
    std::vector<uint16_t> all, rank, cand;
    for (uint32_t R = 1; R <= kBmMaxRadius; ++R)
        for (int order = 0; order < 2; ++order) {
            bm_rank_tables(R, order, rank, cand);
            all.insert(all.end(), rank.begin(), rank.end());
            all.insert(all.end(), cand.begin(), cand.end());
        }
    uint16_t *d = nullptr;
    NUS_HIP(hipMalloc(reinterpret_cast<void **>(&d), all.size() * sizeof(uint16_t)));
    rc = pass(upload(d, all.data(), all.size() * sizeof(uint16_t), nullptr));
    if (rc == kOk) {
        const hipError_t e = hipStreamSynchronize(nullptr); // in place for every stream from here on
        if (e != hipSuccess) rc = fail_hip(e, "hipStreamSynchronize");
    }
    if (rc != kOk) {
        (void)hipFree(d);
        return rc;
    }
    d_tables_ = d;
    return kOk;
}

int BlockMatcher::enqueue(const void *d_a, size_t a_stride, const void *d_b, size_t b_stride, uint32_t w, uint32_t h, uint32_t n_pairs,
                          void *d_workspace, void *d_vectors, void *d_sad, void *d_flags, void *d_flow, int flow_format,
                          hipStream_t stream)
{
    const int rc = ensure_tables();
    if (rc != kOk) return rc;
    BmLaunch L;
    L.a = static_cast<const uint8_t *>(d_a);
    L.b = static_cast<const uint8_t *>(d_b);
    L.a_stride = a_stride;
    L.b_stride = b_stride;
    L.w = w;
    L.h = h;
    L.n_pairs = n_pairs;
    L.bs = bs_;
    L.R = radius_;
    L.rank = d_tables_ + table_offset(radius_, order_);
    L.cand = L.rank + (size_t)(2 * radius_ + 1) * (2 * radius_ + 1);
    L.workspace = d_workspace;
    L.refine = refine_;
    L.bidir = bidir_;
    L.tolerance = tolerance_;
    L.vectors = static_cast<int16_t *>(d_vectors);
    L.sad = static_cast<uint32_t *>(d_sad);
    L.flags = static_cast<uint8_t *>(d_flags);
    L.flow = d_flow;
    L.flow_half = flow_format == 1;
    L.stream = stream;
    const hipError_t e = launch_blockmatch(L);
    if (e != hipSuccess) return fail_hip(e, "block-matching launch");
    return kOk;
}

int BlockMatcher::estimate_device(const void *d_a, size_t a_stride, const void *d_b, size_t b_stride, uint32_t w, uint32_t h,
                                  uint32_t n_pairs, void *d_workspace, size_t workspace_bytes, void *d_vectors, void *d_sad,
                                  void *d_flags, void *d_flow, int flow_format, hipStream_t stream)
{
    static const char *const who = "nus_bm_estimate_device";
    std::lock_guard<std::mutex> lk(mu_);
    int st = check_shape(who, w, h, n_pairs);
    if (st != kOk) return st;
    if (!d_a || !d_b || !d_workspace || !d_vectors) return fail(kInvalidArgument, fmt("%s: null device pointer", who));
    if (flow_format != 0 && flow_format != 1)
        return fail(kInvalidArgument, fmt("%s: flow_format must be NUS_FLOW_F32 or NUS_FLOW_F16", who));
    if ((st = pass(check_pixel_aligned(who, d_a, a_stride, d_b, b_stride, d_vectors, d_flow, flow_format == 1 ? 4 : 8, d_sad))) != kOk) return st;
    if (misaligned(d_workspace, 16)) return fail(kInvalidArgument, fmt("%s: workspace must be 16-byte aligned", who));
    const size_t need = bm_shape(w, h, bs_, n_pairs ? n_pairs : 1, bidir_).workspace_bytes;
    if ((st = pass(check_workspace(who, workspace_bytes, need, "nus_bm_workspace_size"))) != kOk) return st;
    if (n_pairs == 0) return kOk;
    return enqueue(d_a, a_stride, d_b, b_stride, w, h, n_pairs, d_workspace, d_vectors, d_sad, d_flags, d_flow, flow_format, stream);
}

int BlockMatcher::warp_device(const void *d_a, size_t a_stride, const void *d_b, size_t b_stride, uint32_t w, uint32_t h, uint32_t n_pairs,
                              const void *d_vectors, const float *times, uint32_t n_times, int mode, void *d_out, size_t out_pair_stride,
                              hipStream_t stream)
{
    static const char *const who = "nus_bm_warp_device";
    std::lock_guard<std::mutex> lk(mu_);
    int st = pass(check_dims(who, w, h, kMaxPixels));
    if (st != kOk) return st;
    if (!d_a || !d_b || !d_vectors || !d_out) return fail(kInvalidArgument, fmt("%s: null device pointer", who));
    if ((st = pass(check_interp_times(who, times, n_times))) != kOk) return st;
    if (mode != 0 && mode != 1) return fail(kInvalidArgument, fmt("%s: mode must be NUS_INTERP_MODE_EXACT or NUS_INTERP_MODE_FMA", who));
    if ((st = pass(check_pixel_aligned(who, d_a, a_stride, d_b, b_stride, d_out, d_vectors, 4))) != kOk) return st;
    if ((st = pass(check_out_pair_stride(who, out_pair_stride, n_times, (size_t)w * h * 4))) != kOk) return st;
    if (n_pairs == 0) return kOk;
    if ((st = select_device(device_)) != kOk) return st;
    return enqueue_warp(d_a, a_stride, d_b, b_stride, w, h, n_pairs, d_vectors, times, n_times, mode, d_out, out_pair_stride, stream);
}

int BlockMatcher::enqueue_warp(const void *d_a, size_t a_stride, const void *d_b, size_t b_stride, uint32_t w, uint32_t h,
                               uint32_t n_pairs, const void *d_vectors, const float *times, uint32_t n_times, int mode, void *d_out,
                               size_t out_pair_stride, hipStream_t stream)
{
    BmWarpLaunch L;
    L.a = static_cast<const uint8_t *>(d_a);
    L.b = static_cast<const uint8_t *>(d_b);
    L.a_stride = a_stride;
    L.b_stride = b_stride;
    L.w = w;
    L.h = h;
    L.n_pairs = n_pairs;
    L.bs = bs_;
    L.vectors = static_cast<const int16_t *>(d_vectors);
    L.times = times;
    L.n_times = n_times;
    L.fma = mode == 1;
    L.out = static_cast<uint8_t *>(d_out);
    L.out_pair_stride = out_pair_stride;
    L.stream = stream;
    const hipError_t e = launch_bm_warp(L);
    if (e != hipSuccess) return fail_hip(e, "block-vector warp+blend launch");
    return kOk;
}

// The stream entry point's workspace: the search's (with the forward-backward check's part while that is on), the vectors of every pair (used when the caller keeps none) and, with
// detection on, the detector's workspace and one flag byte per pair.
BlockMatcher::StreamLayout BlockMatcher::stream_layout(uint32_t w, uint32_t h, uint32_t n_pairs) const
{
    StreamLayout l;
    const BmShape s = bm_shape(w, h, bs_, n_pairs, bidir_);
    l.o_vec = up16(s.workspace_bytes);
    l.o_scene = l.o_vec + up16((size_t)n_pairs * s.blocks_x * s.blocks_y * 4);
    l.o_cut = l.o_scene + (scene_ ? up16(scene_shape(w, h, n_pairs).workspace_bytes) : 0);
    l.total = l.o_cut + (scene_ ? up16(n_pairs) : 0);
    return l;
}

size_t BlockMatcher::stream_workspace_size(uint32_t w, uint32_t h, uint32_t n_frames)
{
    static const char *const who = "nus_bm_stream_workspace_size";
    std::lock_guard<std::mutex> lk(mu_);
    const uint32_t n_pairs = n_frames < 2 ? 1 : n_frames - 1;
    if (check_shape(who, w, h, n_pairs) != kOk) return 0;
    if (scene_) {
        const std::string too_many = check_scene_launch(w, h, n_pairs);
        if (!too_many.empty()) {
            fail(kInvalidArgument, fmt("%s: %s", who, too_many.c_str()));
            return 0;
        }
    }
    return stream_layout(w, h, n_pairs).total;
}

int BlockMatcher::interpolate_multi_device_stream(const void *d_frames, size_t frame_stride, uint32_t n_frames, uint32_t w, uint32_t h,
                                                  const float *times, uint32_t n_times, int mode, void *d_workspace,
                                                  size_t workspace_bytes, void *d_vectors, void *d_mid, size_t mid_pair_stride,
                                                  hipStream_t stream)
{
    static const char *const who = "nus_bm_interpolate_multi_device_stream";
    std::lock_guard<std::mutex> lk(mu_);
    const uint32_t n_pairs = n_frames < 2 ? 1 : n_frames - 1;
    int st = check_shape(who, w, h, n_pairs);
    if (st != kOk) return st;
    if (!d_frames || !d_workspace || !d_mid) return fail(kInvalidArgument, fmt("%s: null device pointer", who));
    if ((st = pass(check_interp_times(who, times, n_times))) != kOk) return st;
    if (mode != 0 && mode != 1) return fail(kInvalidArgument, fmt("%s: mode must be NUS_INTERP_MODE_EXACT or NUS_INTERP_MODE_FMA", who));
    const size_t frame_bytes = (size_t)w * h * 4;
    if ((st = pass(check_pixel_aligned(who, d_frames, frame_stride, d_frames, frame_stride, d_mid, d_vectors, 4))) != kOk) return st;
    if (frame_stride < frame_bytes)
        return fail(kInvalidArgument, fmt("%s: frame_stride %zu is smaller than a %ux%u frame (%zu bytes)", who, frame_stride, w, h, frame_bytes));
    if ((st = pass(check_out_pair_stride(who, mid_pair_stride, n_times, frame_bytes))) != kOk) return st;
    if (misaligned(d_workspace, 16)) return fail(kInvalidArgument, fmt("%s: workspace must be 16-byte aligned", who));
    if (scene_) {
        const std::string too_many = check_scene_launch(w, h, n_pairs);
        if (!too_many.empty()) return fail(kInvalidArgument, fmt("%s: %s", who, too_many.c_str()));
    }
    const StreamLayout l = stream_layout(w, h, n_pairs);
    if ((st = pass(check_workspace(who, workspace_bytes, l.total, "nus_bm_stream_workspace_size"))) != kOk) return st;
    if (n_frames < 2) return kOk;
    const uint8_t *const a = static_cast<const uint8_t *>(d_frames), *const b = a + frame_stride;
    uint8_t *const ws = static_cast<uint8_t *>(d_workspace);
    void *const vec = d_vectors ? d_vectors : ws + l.o_vec;
    // one search over all pairs -> the confidence pass (or the forward-backward check) -> one warp from the block vectors -> with
    // detection on, the detector (it reads the frames only) and the flagged pairs' frames overwritten with repeats, as
    // interpolate() does for its one pair
    int rc = enqueue(a, frame_stride, b, frame_stride, w, h, n_pairs, ws, vec, nullptr, nullptr, nullptr, 0, stream);
    if (rc != kOk) return rc;
    if ((rc = enqueue_warp(a, frame_stride, b, frame_stride, w, h, n_pairs, vec, times, n_times, mode, d_mid, mid_pair_stride, stream)) != kOk)
        return rc;
    if (scene_) {
        SceneLaunch S;
        S.a = a;
        S.b = b;
        S.a_stride = S.b_stride = frame_stride;
        S.w = w, S.h = h, S.n_pairs = n_pairs, S.stream = stream;
        hipError_t es = launch_scene_detect(S, scene_mad_, scene_hist_, ws + l.o_scene, nullptr, ws + l.o_cut);
        if (es != hipSuccess) return fail_hip(es, "scene-detect launch");
        es = launch_scene_apply(S, n_times, scene_from_a_mask(times, n_times), ws + l.o_cut, static_cast<uint8_t *>(d_mid),
                                mid_pair_stride ? mid_pair_stride : (size_t)n_times * frame_bytes);
        if (es != hipSuccess) return fail_hip(es, "scene-apply launch");
    }
    return kOk;
}

int BlockMatcher::retime_device_stream(const void *d_frames, size_t frame_stride, uint32_t n_frames, uint32_t w, uint32_t h, uint32_t num,
                                       uint32_t den, int mode, void *d_workspace, size_t workspace_bytes, void *d_vectors, void *d_out,
                                       size_t out_frame_stride, hipStream_t stream)
{
    static const char *const who = "nus_bm_retime_device_stream";
    std::lock_guard<std::mutex> lk(mu_);
    RetimeRatio r;
    int st = pass(check_retime(who, n_frames, num, den, r));
    if (st != kOk) return st;
    const uint32_t n_pairs = n_frames - 1;
    if ((st = check_shape(who, w, h, n_pairs)) != kOk) return st;
    if (!d_frames || !d_workspace || !d_out) return fail(kInvalidArgument, fmt("%s: null device pointer", who));
    if (mode != 0 && mode != 1) return fail(kInvalidArgument, fmt("%s: mode must be NUS_INTERP_MODE_EXACT or NUS_INTERP_MODE_FMA", who));
    const size_t frame_bytes = (size_t)w * h * 4;
    if ((st = pass(check_pixel_aligned(who, d_frames, frame_stride, d_frames, frame_stride, d_out, d_vectors, 4))) != kOk) return st;
    if (frame_stride < frame_bytes)
        return fail(kInvalidArgument, fmt("%s: frame_stride %zu is smaller than a %ux%u frame (%zu bytes)", who, frame_stride, w, h, frame_bytes));
    if ((st = pass(check_out_frame_stride(who, out_frame_stride, frame_bytes))) != kOk) return st;
    if (misaligned(d_workspace, 16)) return fail(kInvalidArgument, fmt("%s: workspace must be 16-byte aligned", who));
    if (scene_) {
        const std::string too_many = check_scene_launch(w, h, n_pairs);
        if (!too_many.empty()) return fail(kInvalidArgument, fmt("%s: %s", who, too_many.c_str()));
    }
    const StreamLayout l = stream_layout(w, h, n_pairs);
    if ((st = pass(check_workspace(who, workspace_bytes, l.total, "nus_bm_stream_workspace_size"))) != kOk) return st;
    const uint8_t *const a = static_cast<const uint8_t *>(d_frames), *const b = a + frame_stride;
    uint8_t *const ws = static_cast<uint8_t *>(d_workspace);
    void *const vec = d_vectors ? d_vectors : ws + l.o_vec;
    // one search over all pairs -> the confidence pass (or the forward-backward check) -> the retime warp from the block vectors
    // and the real frames -> with detection on, the detector and the cut pairs' in-between outputs overwritten with repeats
    int rc = enqueue(a, frame_stride, b, frame_stride, w, h, n_pairs, ws, vec, nullptr, nullptr, nullptr, 0, stream);
    if (rc != kOk) return rc;
    RetimeLaunch L;
    L.frames = a, L.frame_stride = frame_stride, L.first_pair = 0, L.n_pairs = n_pairs, L.w = w, L.h = h, L.num = r.num, L.den = r.den;
    L.out = static_cast<uint8_t *>(d_out), L.out_frame_stride = out_frame_stride ? out_frame_stride : frame_bytes, L.stream = stream;
    RetimeWarp V;
    V.vectors = static_cast<const int16_t *>(vec), V.bs = bs_, V.fma = mode == 1;
    hipError_t e = enqueue_retime(L, V, true);
    if (e != hipSuccess) return fail_hip(e, "retime block-vector warp+blend launch");
    if (scene_) {
        SceneLaunch S;
        S.a = a, S.b = b, S.a_stride = S.b_stride = frame_stride;
        S.w = w, S.h = h, S.n_pairs = n_pairs, S.stream = stream;
        if ((e = launch_scene_detect(S, scene_mad_, scene_hist_, ws + l.o_scene, nullptr, ws + l.o_cut)) != hipSuccess)
            return fail_hip(e, "scene-detect launch");
        if ((e = launch_scene_apply_retime(L, ws + l.o_cut)) != hipSuccess) return fail_hip(e, "retime scene-apply launch");
    }
    return kOk;
}

int BlockMatcher::check_host_frames(const char *who, const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len, uint32_t w,
                                    uint32_t h)
{
    int st = check_shape(who, w, h, 1);
    if (st != kOk || (st = pass(check_frame_lengths(a_len, b_len, w, h))) != kOk) return st; // as nus_interp_interpolate
    if (!a || !b) return fail(kInvalidArgument, fmt("%s: null frame pointer", who));
    return kOk;
}

int BlockMatcher::ensure_host(size_t bytes)
{
    const int rc = ensure_tables();
    if (rc != kOk) return rc;
    if (!stream_) NUS_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    return pass(arena_.reserve(bytes, stream_));
}

int BlockMatcher::estimate(const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len, uint32_t w, uint32_t h, int16_t *vectors_out,
                           uint32_t *sad_out, uint8_t *flags_out)
{
    static const char *const who = "nus_bm_estimate";
    std::lock_guard<std::mutex> lk(mu_);
    const int st = check_host_frames(who, a, a_len, b, b_len, w, h);
    if (st != kOk) return st;
    if (!vectors_out) return fail(kInvalidArgument, fmt("%s: vectors_out is null", who));
    const BmShape s = bm_shape(w, h, bs_, 1, bidir_);
    const size_t frame = up16((size_t)w * h * 4), nb = (size_t)s.blocks_x * s.blocks_y;
    const size_t o_b = frame, o_ws = 2 * frame, o_vec = o_ws + up16(s.workspace_bytes), o_sad = o_vec + up16(nb * 4),
                 o_flags = o_sad + up16(nb * 4), total = o_flags + up16(nb);
    int rc = ensure_host(total);
    if (rc != kOk) return rc;
    uint8_t *const arena = static_cast<uint8_t *>(arena_.get());
    if ((rc = pass(upload(arena, a, a_len, stream_))) != kOk) return rc;
    if ((rc = pass(upload(arena + o_b, b, b_len, stream_))) != kOk) return rc;
    rc = enqueue(arena, a_len, arena + o_b, b_len, w, h, 1, arena + o_ws, arena + o_vec, arena + o_sad, arena + o_flags, nullptr, 0,
                 stream_);
    if (rc != kOk) return rc;
    if ((rc = pass(download(vectors_out, arena + o_vec, nb * 4, stream_))) != kOk) return rc;
    if (sad_out && (rc = pass(download(sad_out, arena + o_sad, nb * 4, stream_))) != kOk) return rc;
    if (flags_out && (rc = pass(download(flags_out, arena + o_flags, nb, stream_))) != kOk) return rc;
    return kOk;
}

int BlockMatcher::interpolate(const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len, uint32_t w, uint32_t h, const float *times,
                              uint32_t n_times, int mode, uint8_t *out, size_t out_cap)
{
    static const char *const who = "nus_bm_interpolate";
    std::lock_guard<std::mutex> lk(mu_);
    int st = check_host_frames(who, a, a_len, b, b_len, w, h);
    if (st != kOk) return st;
    if (!out) return fail(kInvalidArgument, fmt("%s: null frame pointer", who));
    if ((st = pass(check_interp_times(who, times, n_times))) != kOk) return st;
    if (mode != 0 && mode != 1) return fail(kInvalidArgument, fmt("%s: mode must be NUS_INTERP_MODE_EXACT or NUS_INTERP_MODE_FMA", who));
    const size_t expected = (size_t)w * h * 4;
    if (out_cap / n_times < expected)
        return fail(kInvalidArgument, fmt("%s: output capacity %zu below n_times * w * h * 4 = %zu", who, out_cap, (size_t)n_times * expected));
    const BmShape s = bm_shape(w, h, bs_, 1, bidir_);
    const size_t frame = up16(expected), nb = (size_t)s.blocks_x * s.blocks_y;
    const size_t o_b = frame, o_ws = 2 * frame, o_vec = o_ws + up16(s.workspace_bytes), o_flow = o_vec + up16(nb * 4), o_out = o_flow + frame,
                 out_end = o_out + (size_t)n_times * expected,
                 // with detection on: the detector's workspace and the pair's flag byte behind the frames
                 o_scene = up16(out_end), scene_ws = up16(scene_shape(w, h, 1).workspace_bytes),
                 total = scene_ ? o_scene + scene_ws + 16 : out_end;
    int rc = ensure_host(total);
    if (rc != kOk) return rc;
    uint8_t *const arena = static_cast<uint8_t *>(arena_.get());
    if ((rc = pass(upload(arena, a, a_len, stream_))) != kOk) return rc;
    if ((rc = pass(upload(arena + o_b, b, b_len, stream_))) != kOk) return rc;
    SceneLaunch S; // detect -> estimate + warp as without detection -> a flagged pair's frames overwritten with repeats
    S.a = arena;
    S.b = arena + o_b;
    S.a_stride = S.b_stride = expected;
    S.w = w, S.h = h, S.stream = stream_;
    uint8_t *const cut = arena + o_scene + scene_ws;
    if (scene_) {
        const hipError_t es = launch_scene_detect(S, scene_mad_, scene_hist_, arena + o_scene, nullptr, cut);
        if (es != hipSuccess) return fail_hip(es, "scene-detect launch");
    }
    // estimate -> dense flow as 2 x f16 per pixel (the vectors are integers of magnitude <= 24: exact) -> multi-time warp
    rc = enqueue(arena, a_len, arena + o_b, b_len, w, h, 1, arena + o_ws, arena + o_vec, nullptr, nullptr, arena + o_flow, 1, stream_);
    if (rc != kOk) return rc;
    WarpLaunch L;
    L.a = arena;
    L.b = arena + o_b;
    L.flow = reinterpret_cast<const float *>(arena + o_flow);
    L.flow_half = true;
    L.fma = mode == 1;
    L.out = arena + o_out;
    L.a_stride = L.b_stride = expected;
    L.w = w;
    L.h = h;
    L.times = times;
    L.n_times = n_times;
    L.n_pairs = 1;
    L.stream = stream_;
    const hipError_t e = launch_warp_blend(L);
    if (e != hipSuccess) return fail_hip(e, "multi-time warp+blend launch");
    if (scene_) {
        const hipError_t es = launch_scene_apply(S, n_times, scene_from_a_mask(times, n_times), cut, arena + o_out, (size_t)n_times * expected);
        if (es != hipSuccess) return fail_hip(es, "scene-apply launch");
    }
    return pass(download(out, arena + o_out, (size_t)n_times * expected, stream_));
}

} // namespace nus
