// nus_yuv_resize.cpp -- host side of the planar up-scaler of I420 and tight NV12 frames (nus_yuv_resizer* / nus_yuv420_resize* /
// nus_nv12_resize* in include/nuscaler_hip.h): the dimension rule, the four axis tables, the argument checks, which run before any HIP call, the
// tables' upload on the handle's first device call, the two launches per batch, and the host entry point's buffers.
#include "nus_yuv_resize.hpp"

#include <algorithm>

#include "nus_tables.hpp"
#include "nus_transfer.hpp"

namespace nus {

namespace {

constexpr uint64_t kMaxPixels = (uint64_t)1 << 30;
constexpr uint32_t kMaxOutHeight = 65535u * 4; // the per-sample kernel puts four rows in a workgroup and the row groups on grid.y

size_t i420_bytes(uint32_t w, uint32_t h) { return (size_t)w * h + 2 * (size_t)(w / 2) * (h / 2); } // (even dimensions)

} // namespace

YuvResizer::~YuvResizer()
{
    if (!d_tables_ && !d_in_.get() && !d_out_.get() && !stream_) return;
    (void)hipSetDevice(device_);
    if (stream_) {
        (void)hipStreamSynchronize(stream_);
        (void)hipStreamDestroy(stream_);
    }
    d_in_.release();
    d_out_.release();
    if (d_tables_) (void)hipFree(d_tables_);
}

void YuvResizer::drop_tables()
{
    if (!d_tables_) return;
    (void)hipSetDevice(device_);
    (void)hipFree(d_tables_); // (waits for the work that reads them)
    d_tables_ = nullptr;
}

int YuvResizer::set_device(int device)
{
    std::lock_guard<std::mutex> lk(mu_);
    if (device < 0) return fail(kInvalidArgument, "nus_yuv_resizer_set_device: negative device index");
    if (device_used_) return fail(kInvalidArgument, "nus_yuv_resizer_set_device: must precede the first device call");
    device_ = device;
    return kOk;
}

int YuvResizer::initialize(uint32_t iw, uint32_t ih, uint32_t ow, uint32_t oh, int algorithm, int siting, int mode)
{
    static const char *const who = "nus_yuv_resizer_initialize";
    std::lock_guard<std::mutex> lk(mu_);
    if (iw == 0 || ih == 0 || ow == 0 || oh == 0) return fail(kInvalidArgument, fmt("%s: width and height must be non-zero", who));
    int st = pass(check_frame_area(who, iw, ih, kMaxPixels));
    if (st != kOk || (st = pass(check_frame_area(who, ow, oh, kMaxPixels))) != kOk) return st;
    if (oh > kMaxOutHeight) return fail(kInvalidArgument, fmt("%s: an output height above %u is not supported, got %u", who, kMaxOutHeight, oh));
    if (siting != 0 && siting != 1) return fail(kInvalidArgument, fmt("%s: unknown siting %d", who, siting));
    if (mode != 0 && mode != 1) return fail(kInvalidArgument, fmt("%s: unknown mode %d", who, mode));
    ResizeFilter filter;
    if (algorithm == 2) filter = ResizeFilter::Lanczos3;
    else if (algorithm == 3) filter = ResizeFilter::CatmullRom;
    else if (algorithm == 4) filter = ResizeFilter::Triangle;
    else
        return fail(kUnsupported, fmt("%s: algorithm %d is not supported: the planes are resampled with NUS_ALG_LANCZOS3, NUS_ALG_BICUBIC or "
                                      "NUS_ALG_TRIANGLE (the RGBA route, nus_upscaler, takes the others)", who, algorithm));
    if ((iw | ih | ow | oh) & 1u)
        return fail(kUnsupported, fmt("%s: %ux%u -> %ux%u: all four dimensions must be even, so that the chroma planes are exactly half "
                                      "the luma planes (the RGBA route, nus_upscaler, takes odd sizes)", who, iw, ih, ow, oh));
    if (ow < iw || oh < ih)
        return fail(kUnsupported, fmt("%s: %ux%u -> %ux%u: down-scaling on an axis is not supported, the output must be at least the "
                                      "input on both (the RGBA route, nus_upscaler, scales down)", who, iw, ih, ow, oh));
    const float phi_cx = siting == 1 ? 0.25f : 0.5f;
    const uint32_t in_n[2][2] = {{iw, ih}, {iw / 2, ih / 2}}, out_n[2][2] = {{ow, oh}, {ow / 2, oh / 2}};
    Axis fresh[2][2];
    size_t words = 0;
    for (int p = 0; p < 2; ++p)
        for (int a = 0; a < 2; ++a) {
            Axis &A = fresh[p][a];
            A.in_n = in_n[p][a], A.out_n = out_n[p][a];
            A.left.resize(A.out_n), A.ntaps.resize(A.out_n), A.w.resize((size_t)A.out_n * kResizeMaxTaps);
            A.max_taps = build_resize_axis(filter, A.in_n, A.out_n, A.left.data(), A.ntaps.data(), A.w.data(), (p == 1 && a == 0) ? phi_cx : 0.5f);
            if (A.max_taps < 0) return fail(kUnsupported, fmt("%s: a tap window exceeds NUS_RESIZE_MAX_TAPS", who));
            // the row kernel's geometry along this axis as a plane's x axis: the widest dword-aligned input footprint of a wave's
            // segment and the widest union of the windows of a lane's run; 0 where the run does not divide the axis
            if (a == 0 && (A.out_n % kPlaneRun) == 0 && A.max_taps <= 8) {
                for (uint32_t x0 = 0; x0 < A.out_n; x0 += kPlaneSegment) {
                    const uint32_t xl = std::min(x0 + kPlaneSegment, A.out_n) - 1;
                    const int32_t c0 = A.left[x0] & ~3, cmax = A.left[xl] + (int32_t)A.ntaps[xl];
                    A.ncols_max = std::max(A.ncols_max, (uint32_t)((cmax - c0 + 3) & ~3));
                }
                for (uint32_t x = 0; x < A.out_n; x += kPlaneRun) {
                    int32_t end = 0;
                    for (uint32_t i = 0; i < kPlaneRun; ++i) end = std::max(end, A.left[x + i] + (int32_t)A.ntaps[x + i]);
                    A.union_taps = std::max(A.union_taps, (uint32_t)(end - A.left[x]));
                }
            }
            // the same for the plane of U,V pairs of an NV12 frame: a segment is kPairSegment output cells, a run two of them
            if (p == 1 && a == 0 && (A.out_n % kPairRun) == 0 && (A.in_n % 2) == 0 && A.max_taps <= 8) {
                for (uint32_t x0 = 0; x0 < A.out_n; x0 += kPairSegment) {
                    const uint32_t xl = std::min(x0 + kPairSegment, A.out_n) - 1;
                    const int32_t c0 = (2 * A.left[x0]) & ~3, cmax = 2 * (A.left[xl] + (int32_t)A.ntaps[xl]);
                    A.pair_ncols_max = std::max(A.pair_ncols_max, (uint32_t)((cmax - c0 + 3) & ~3));
                }
                for (uint32_t x = 0; x < A.out_n; x += kPairRun) {
                    const int32_t end = std::max(A.left[x] + (int32_t)A.ntaps[x], A.left[x + 1] + (int32_t)A.ntaps[x + 1]);
                    A.pair_union = std::max(A.pair_union, (uint32_t)(end - A.left[x]));
                }
            }
            A.d_offset = words;
            words += (size_t)A.out_n * (2 + kResizeMaxTaps);
        }
    drop_tables(); // (a handle initialised again uploads again)
    for (int p = 0; p < 2; ++p)
        for (int a = 0; a < 2; ++a) axis_[p][a] = std::move(fresh[p][a]);
    iw_ = iw, ih_ = ih, ow_ = ow, oh_ = oh;
    in_bytes_ = i420_bytes(iw, ih), out_bytes_ = i420_bytes(ow, oh);
    exact_ = mode == 1;
    ready_ = true;
    return kOk;
}

int YuvResizer::export_axis(int plane, int axis, int32_t *left, uint32_t *ntaps, float *weights)
{
    static const char *const who = "nus_yuv_resizer_export_axis";
    std::lock_guard<std::mutex> lk(mu_);
    if (!left || !ntaps || !weights) return fail(kInvalidArgument, fmt("%s: null pointer", who));
    if (!ready_) return fail(kNotInitialized, fmt("%s: the resizer is not initialized", who));
    if (plane != 0 && plane != 1) return fail(kInvalidArgument, fmt("%s: unknown plane %d (0 luma, 1 chroma)", who, plane));
    if (axis != 0 && axis != 1) return fail(kInvalidArgument, fmt("%s: unknown axis %d (0 x, 1 y)", who, axis));
    const Axis &A = axis_[plane][axis];
    std::copy(A.left.begin(), A.left.end(), left);
    std::copy(A.ntaps.begin(), A.ntaps.end(), ntaps);
    std::copy(A.w.begin(), A.w.end(), weights);
    return kOk;
}

int YuvResizer::ensure_tables(const char *who)
{
    int rc = pass(check_device(who, device_));
    if (rc != kOk) return rc;
    device_used_ = true;
    NUS_HIP(hipSetDevice(device_));
    if (d_tables_) return kOk;
    size_t words = 0;
    for (auto &pl : axis_)
        for (auto &A : pl) words = std::max(words, A.d_offset + (size_t)A.out_n * (2 + kResizeMaxTaps));
    std::vector<uint32_t> blob(words);
    for (auto &pl : axis_)
        for (auto &A : pl) {
            uint32_t *const at = blob.data() + A.d_offset;
            std::copy(A.left.begin(), A.left.end(), reinterpret_cast<int32_t *>(at));
            std::copy(A.ntaps.begin(), A.ntaps.end(), at + A.out_n);
            std::copy(A.w.begin(), A.w.end(), reinterpret_cast<float *>(at + 2 * (size_t)A.out_n));
        }
    uint32_t *d = nullptr;
    NUS_HIP(hipMalloc(reinterpret_cast<void **>(&d), words * sizeof(uint32_t)));
    rc = pass(upload(d, blob.data(), words * sizeof(uint32_t), nullptr)); // the pinned road, not a copy from pageable memory
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

int YuvResizer::enqueue(const char *who, const uint8_t *d_in, size_t in_stride, uint8_t *d_out, size_t out_stride, uint32_t n_frames,
                        hipStream_t stream, bool nv12)
{
    if (iw_ == ow_ && ih_ == oh_) { // imageops::resize returns a copy when the dimensions are unchanged
        const hipError_t e = launch_frame_copy(d_in, in_stride, d_out, out_stride, in_bytes_, n_frames, stream);
        return e != hipSuccess ? fail_hip(e, "frame copy launch") : kOk;
    }
    for (int p = 0; p < 2; ++p) {
        const Axis &X = axis_[p][0], &Y = axis_[p][1];
        PlaneResizeLaunch L;
        L.in = d_in, L.out = d_out, L.in_frame_stride = in_stride, L.out_frame_stride = out_stride;
        L.n_frames = n_frames, L.planes_per_frame = (p == 0 || nv12) ? 1 : 2;
        L.iw = X.in_n, L.ih = Y.in_n, L.ow = X.out_n, L.oh = Y.out_n;
        if (p == 1) {
            L.in_plane_offset = (size_t)iw_ * ih_, L.in_plane_step = (size_t)L.iw * L.ih;
            L.out_plane_offset = (size_t)ow_ * oh_, L.out_plane_step = (size_t)L.ow * L.oh;
        }
        const uint32_t *const tx = d_tables_ + X.d_offset, *const ty = d_tables_ + Y.d_offset;
        L.t.lx = reinterpret_cast<const int32_t *>(tx), L.t.nx = tx + X.out_n, L.t.wx = reinterpret_cast<const float *>(tx + 2 * (size_t)X.out_n);
        L.t.ly = reinterpret_cast<const int32_t *>(ty), L.t.ny = ty + Y.out_n, L.t.wy = reinterpret_cast<const float *>(ty + 2 * (size_t)Y.out_n);
        L.table_stride = kResizeMaxTaps, L.max_taps = (uint32_t)std::max(X.max_taps, Y.max_taps);
        L.ncols_max = X.ncols_max, L.union_taps = X.union_taps;
        L.exact = exact_, L.stream = stream;
        if (p == 1 && nv12) { // one plane of U,V pairs where I420 has two planes: same tables, the pair kernels' geometry
            L.in_plane_step = L.out_plane_step = 0;
            L.ncols_max = X.pair_ncols_max, L.union_taps = X.pair_union;
            const hipError_t e = launch_pair_resize(L);
            if (e != hipSuccess) return fail_hip(e, "pair-plane resize launch");
            continue;
        }
        const hipError_t e = launch_plane_resize(L);
        if (e != hipSuccess) return fail_hip(e, p == 0 ? "luma resize launch" : "chroma resize launch");
    }
    (void)who;
    return kOk;
}

int YuvResizer::device_call(const char *who, bool nv12, const void *d_in, size_t in_frame_stride, void *d_out, size_t out_frame_stride,
                            uint32_t n_frames, hipStream_t stream)
{
    std::lock_guard<std::mutex> lk(mu_);
    if (!d_in || !d_out) return fail(kInvalidArgument, fmt("%s: null pointer", who));
    if (!ready_) return fail(kNotInitialized, fmt("%s: the resizer is not initialized", who));
    if (n_frames == 0) return fail(kInvalidArgument, fmt("%s: n_frames must be at least 1", who));
    if (in_frame_stride != 0 && in_frame_stride < in_bytes_)
        return fail(kInvalidArgument, fmt("%s: in_frame_stride must be 0 or at least %zu, got %zu", who, in_bytes_, in_frame_stride));
    if (out_frame_stride != 0 && out_frame_stride < out_bytes_)
        return fail(kInvalidArgument, fmt("%s: out_frame_stride must be 0 or at least %zu, got %zu", who, out_bytes_, out_frame_stride));
    const int rc = ensure_tables(who);
    if (rc != kOk) return rc;
    return enqueue(who, static_cast<const uint8_t *>(d_in), in_frame_stride ? in_frame_stride : in_bytes_, static_cast<uint8_t *>(d_out),
                   out_frame_stride ? out_frame_stride : out_bytes_, n_frames, stream, nv12);
}

int YuvResizer::host_call(const char *who, bool nv12, const uint8_t *in, size_t in_len, uint8_t *out, size_t out_cap)
{
    std::lock_guard<std::mutex> lk(mu_);
    if (!in || !out) return fail(kInvalidArgument, fmt("%s: null pointer", who));
    if (!ready_) return fail(kNotInitialized, fmt("%s: the resizer is not initialized", who));
    if (in_len != in_bytes_)
        return fail(kSizeMismatch, fmt("%s: in_len (%zu) does not match the frame size (%zu for %ux%u)", who, in_len, in_bytes_, iw_, ih_));
    if (out_cap < out_bytes_)
        return fail(kSizeMismatch, fmt("%s: out_cap (%zu) is below the frame size (%zu for %ux%u)", who, out_cap, out_bytes_, ow_, oh_));
    int rc = ensure_tables(who);
    if (rc != kOk) return rc;
    if (!stream_) NUS_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    if ((rc = pass(d_in_.reserve(in_bytes_, stream_))) != kOk || (rc = pass(d_out_.reserve(out_bytes_, stream_))) != kOk) return rc;
    if ((rc = pass(upload(d_in_.get(), in, in_bytes_, stream_))) != kOk) return rc;
    if ((rc = enqueue(who, static_cast<const uint8_t *>(d_in_.get()), in_bytes_, static_cast<uint8_t *>(d_out_.get()), out_bytes_, 1, stream_, nv12)) != kOk)
        return rc;
    return pass(download(out, d_out_.get(), out_bytes_, stream_));
}

int YuvResizer::resize_device(const void *d_in, size_t in_frame_stride, void *d_out, size_t out_frame_stride, uint32_t n_frames,
                              hipStream_t stream)
{
    return device_call("nus_yuv420_resize_device", false, d_in, in_frame_stride, d_out, out_frame_stride, n_frames, stream);
}

int YuvResizer::resize(const uint8_t *in, size_t in_len, uint8_t *out, size_t out_cap)
{
    return host_call("nus_yuv420_resize", false, in, in_len, out, out_cap);
}

int YuvResizer::resize_nv12_device(const void *d_in, size_t in_frame_stride, void *d_out, size_t out_frame_stride, uint32_t n_frames,
                                   hipStream_t stream)
{
    return device_call("nus_nv12_resize_device", true, d_in, in_frame_stride, d_out, out_frame_stride, n_frames, stream);
}

int YuvResizer::resize_nv12(const uint8_t *in, size_t in_len, uint8_t *out, size_t out_cap)
{
    return host_call("nus_nv12_resize", true, in, in_len, out, out_cap);
}

} // namespace nus
