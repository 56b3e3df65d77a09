// nus_yuv.cpp -- host side of the YUV 4:2:0 conversions (nus_yuv* and nus_nv12* in include/nuscaler_hip.h): the coefficient tables,
// the NV12 layout rule, the argument checks, which run before any HIP call, the enqueue of the device entry points, and the
// per-device buffers of the host ones.
#include "nus_yuv.hpp"

#include <cmath>
#include <mutex>

#include "nus_host_util.hpp"
#include "nus_transfer.hpp"

namespace nus {

namespace {

constexpr uint64_t kMaxPixels = (uint64_t)1 << 30;
constexpr uint32_t kMaxHeight = 65535u * 8; // the kernels put four chroma rows in a workgroup and the row groups on grid.y

int32_t q14(double x) { return (int32_t)std::floor(x * 16384.0 + 0.5); }

int check_dims_yuv(const char *who, uint32_t w, uint32_t h)
{
    if (w == 0 || h == 0) return fail(kInvalidArgument, fmt("%s: width and height must be non-zero", who));
    if (check_frame_area(who, w, h, kMaxPixels) != kOk) return kInvalidArgument;
    if (h > kMaxHeight) return fail(kInvalidArgument, fmt("%s: a height above %u is not supported, got %u", who, kMaxHeight, h));
    return kOk;
}

int check_formats(const char *who, const YuvFormat *f, int rgba_format)
{
    if (f->matrix != 0 && f->matrix != 1) return fail(kInvalidArgument, fmt("%s: unknown matrix %d", who, f->matrix));
    if (f->range != 0 && f->range != 1) return fail(kInvalidArgument, fmt("%s: unknown range %d", who, f->range));
    if (f->siting != 0 && f->siting != 1) return fail(kInvalidArgument, fmt("%s: unknown siting %d", who, f->siting));
    if (f->chroma_filter != 0 && f->chroma_filter != 1) return fail(kInvalidArgument, fmt("%s: unknown chroma_filter %d", who, f->chroma_filter));
    if (rgba_format < 0 || rgba_format > 3) return fail(kInvalidArgument, fmt("%s: unknown pixel format %d", who, rgba_format));
    return kOk;
}

size_t frame_bytes_unchecked(uint32_t w, uint32_t h) { return (size_t)w * h + 2 * (((size_t)w + 1) / 2) * (((size_t)h + 1) / 2); }

// every check of a device entry point; fills the launch
int prepare_device(const char *who, const void *d_yuv, size_t yuv_frame_stride, const void *d_rgba, size_t rgba_frame_stride, uint32_t w,
                   uint32_t h, const YuvFormat *f, int rgba_format, uint32_t n_frames, hipStream_t stream, YuvLaunch *L)
{
    if (!d_yuv || !d_rgba || !f) return fail(kInvalidArgument, fmt("%s: null pointer", who));
    int st = check_dims_yuv(who, w, h);
    if (st != kOk || (st = check_formats(who, f, rgba_format)) != kOk) return st;
    if (n_frames == 0) return fail(kInvalidArgument, fmt("%s: n_frames must be at least 1", who));
    const size_t yuv_bytes = frame_bytes_unchecked(w, h), rgba_bytes = (size_t)w * h * 4;
    if (rgba_frame_stride != 0 && (rgba_frame_stride < rgba_bytes || (rgba_frame_stride % 4) != 0))
        return fail(kInvalidArgument, fmt("%s: rgba_frame_stride must be 0 or a multiple of 4 of at least %zu, got %zu", who, rgba_bytes, rgba_frame_stride));
    if (yuv_frame_stride != 0 && yuv_frame_stride < yuv_bytes)
        return fail(kInvalidArgument, fmt("%s: yuv_frame_stride must be 0 or at least %zu, got %zu", who, yuv_bytes, yuv_frame_stride));
    if (misaligned(d_rgba, 4)) return fail(kInvalidArgument, fmt("%s: the RGBA frames must be 4-byte aligned", who));
    L->yuv = static_cast<uint8_t *>(const_cast<void *>(d_yuv)), L->rgba = static_cast<uint8_t *>(const_cast<void *>(d_rgba));
    L->yuv_frame_stride = yuv_frame_stride ? yuv_frame_stride : yuv_bytes;
    L->rgba_frame_stride = rgba_frame_stride ? rgba_frame_stride : rgba_bytes;
    L->w = w, L->h = h, L->n_frames = n_frames, L->siting = f->siting, L->chroma_filter = f->chroma_filter;
    yuv_coefficients(f->matrix, f->range, L->to_yuv, L->to_rgb, &L->y_offset);
    L->sel = input_selector(rgba_format), L->stream = stream;
    return kOk;
}

// what the host entry points check before they touch a device: `src_len` must be the source frame, `dst_cap` hold the other
int check_host(const char *who, size_t src_len, size_t src_bytes, const char *src_name, size_t dst_cap, size_t dst_bytes,
               const char *dst_name, uint32_t w, uint32_t h)
{
    if (src_len != src_bytes)
        return fail(kSizeMismatch, fmt("%s: %s (%zu) does not match the frame size (%zu for %ux%u)", who, src_name, src_len, src_bytes, w, h));
    if (dst_cap < dst_bytes) return fail(kSizeMismatch, fmt("%s: %s (%zu) is below the frame size (%zu for %ux%u)", who, dst_name, dst_cap, dst_bytes, w, h));
    return kOk;
}

PairScratch &scratch_of(int device)
{
    static PairScratch *const scratch = new PairScratch[kMaxDevices]; // never destroyed: see DeviceBuffer
    return scratch[device];
}

} // namespace

size_t yuv420_frame_bytes(uint32_t w, uint32_t h)
{
    if (check_dims_yuv("nus_yuv420_frame_bytes", w, h) != kOk) return 0;
    return frame_bytes_unchecked(w, h);
}

int yuv_coefficients(int matrix, int range, int32_t *to_yuv, int32_t *to_rgb, int32_t *y_offset)
{
    const char *who = "nus_yuv_coefficients";
    if (!to_yuv || !to_rgb) return fail(kInvalidArgument, fmt("%s: null pointer", who));
    if (matrix != 0 && matrix != 1) return fail(kInvalidArgument, fmt("%s: unknown matrix %d", who, matrix));
    if (range != 0 && range != 1) return fail(kInvalidArgument, fmt("%s: unknown range %d", who, range));
    const double kr = matrix == 0 ? 0.299 : 0.2126, kb = matrix == 0 ? 0.114 : 0.0722, kg = 1.0 - kr - kb;
    const double ys = range == 0 ? 219.0 : 255.0, cs = range == 0 ? 224.0 : 255.0;
    to_yuv[0] = q14(kr * ys / 255.0), to_yuv[1] = q14(kg * ys / 255.0), to_yuv[2] = q14(kb * ys / 255.0);
    to_yuv[3] = q14(-kr / (2.0 * (1.0 - kb)) * cs / 255.0), to_yuv[4] = q14(-kg / (2.0 * (1.0 - kb)) * cs / 255.0);
    to_yuv[5] = q14((1.0 - kb) / (2.0 * (1.0 - kb)) * cs / 255.0);
    to_yuv[6] = q14((1.0 - kr) / (2.0 * (1.0 - kr)) * cs / 255.0), to_yuv[7] = q14(-kg / (2.0 * (1.0 - kr)) * cs / 255.0);
    to_yuv[8] = q14(-kb / (2.0 * (1.0 - kr)) * cs / 255.0);
    to_rgb[0] = q14(255.0 / ys), to_rgb[1] = q14(2.0 * (1.0 - kr) * 255.0 / cs), to_rgb[2] = q14(2.0 * (1.0 - kb) * 255.0 / cs);
    to_rgb[3] = q14(-2.0 * kb * (1.0 - kb) / kg * 255.0 / cs), to_rgb[4] = q14(-2.0 * kr * (1.0 - kr) / kg * 255.0 / cs);
    if (y_offset) *y_offset = range == 0 ? 16 : 0;
    return kOk;
}

int yuv420_to_rgba8_device(const void *d_yuv, size_t yuv_frame_stride, uint32_t w, uint32_t h, const YuvFormat *f, int rgba_format,
                           void *d_rgba, size_t rgba_frame_stride, uint32_t n_frames, hipStream_t stream)
{
    YuvLaunch L;
    const int st = prepare_device("nus_yuv420_to_rgba8_device", d_yuv, yuv_frame_stride, d_rgba, rgba_frame_stride, w, h, f, rgba_format,
                                  n_frames, stream, &L);
    if (st != kOk) return st;
    if (device_count() <= 0) return fail(kNoDevice, "nus_yuv420_to_rgba8_device: no HIP device available");
    const hipError_t e = launch_yuv_to_rgba(L);
    return e != hipSuccess ? fail_hip(e, "yuv-to-rgba launch") : kOk;
}

int rgba8_to_yuv420_device(const void *d_rgba, size_t rgba_frame_stride, uint32_t w, uint32_t h, const YuvFormat *f, int rgba_format,
                           void *d_yuv, size_t yuv_frame_stride, uint32_t n_frames, hipStream_t stream)
{
    YuvLaunch L;
    const int st = prepare_device("nus_rgba8_to_yuv420_device", d_yuv, yuv_frame_stride, d_rgba, rgba_frame_stride, w, h, f, rgba_format,
                                  n_frames, stream, &L);
    if (st != kOk) return st;
    if (device_count() <= 0) return fail(kNoDevice, "nus_rgba8_to_yuv420_device: no HIP device available");
    const hipError_t e = launch_rgba_to_yuv(L);
    return e != hipSuccess ? fail_hip(e, "rgba-to-yuv launch") : kOk;
}

int yuv420_to_rgba8(int device, const uint8_t *yuv, size_t yuv_len, uint32_t w, uint32_t h, const YuvFormat *f, int rgba_format,
                    uint8_t *rgba, size_t rgba_cap)
{
    const char *who = "nus_yuv420_to_rgba8";
    if (!yuv || !rgba || !f) return fail(kInvalidArgument, fmt("%s: null pointer", who));
    int r = check_dims_yuv(who, w, h);
    if (r != kOk || (r = check_formats(who, f, rgba_format)) != kOk) return r;
    const size_t yuv_bytes = frame_bytes_unchecked(w, h), rgba_bytes = (size_t)w * h * 4;
    if ((r = check_host(who, yuv_len, yuv_bytes, "yuv_len", rgba_cap, rgba_bytes, "rgba_cap", w, h)) != kOk) return r;
    if ((r = check_device(who, device)) != kOk) return r;
    PairScratch &s = scratch_of(device);
    std::lock_guard<std::mutex> lock(s.m);
    if ((r = s.prepare(device, rgba_bytes, 0, 0)) != kOk) return r;
    if ((r = upload(s.a.get(), yuv, yuv_bytes, s.stream)) != kOk) return r;
    if ((r = yuv420_to_rgba8_device(s.a.get(), 0, w, h, f, rgba_format, s.b.get(), 0, 1, s.stream)) != kOk) return r;
    return download(rgba, s.b.get(), rgba_bytes, s.stream);
}

int rgba8_to_yuv420(int device, const uint8_t *rgba, size_t rgba_len, uint32_t w, uint32_t h, const YuvFormat *f, int rgba_format,
                    uint8_t *yuv, size_t yuv_cap)
{
    const char *who = "nus_rgba8_to_yuv420";
    if (!yuv || !rgba || !f) return fail(kInvalidArgument, fmt("%s: null pointer", who));
    int r = check_dims_yuv(who, w, h);
    if (r != kOk || (r = check_formats(who, f, rgba_format)) != kOk) return r;
    const size_t yuv_bytes = frame_bytes_unchecked(w, h), rgba_bytes = (size_t)w * h * 4;
    if ((r = check_host(who, rgba_len, rgba_bytes, "rgba_len", yuv_cap, yuv_bytes, "yuv_cap", w, h)) != kOk) return r;
    if ((r = check_device(who, device)) != kOk) return r;
    PairScratch &s = scratch_of(device);
    std::lock_guard<std::mutex> lock(s.m);
    if ((r = s.prepare(device, rgba_bytes, 0, 0)) != kOk) return r;
    if ((r = upload(s.a.get(), rgba, rgba_bytes, s.stream)) != kOk) return r;
    if ((r = rgba8_to_yuv420_device(s.a.get(), 0, w, h, f, rgba_format, s.b.get(), 0, 1, s.stream)) != kOk) return r;
    return download(yuv, s.b.get(), yuv_bytes, s.stream);
}

// ---- NV12 frames ------------------------------------------------------------------------------------------------------------------

int resolve_nv12(const char *who, uint32_t w, uint32_t h, const Nv12Layout *layout, Nv12Frame *out)
{
    const size_t cw = ((size_t)w + 1) / 2, ch = ((size_t)h + 1) / 2;
    if (!layout || layout->pitch == 0) {
        if (layout && layout->uv_offset != 0)
            return fail(kInvalidArgument, fmt("%s: a layout with pitch 0 (tight) must have uv_offset 0, got %zu", who, layout->uv_offset));
        out->y_pitch = w, out->uv_pitch = 2 * cw, out->uv_offset = (size_t)w * h, out->bytes = frame_bytes_unchecked(w, h);
        return kOk;
    }
    const size_t pitch = layout->pitch;
    if (pitch < 2 * cw) return fail(kInvalidArgument, fmt("%s: pitch must be 0 or at least %zu, got %zu", who, 2 * cw, pitch));
    if (pitch > ((size_t)1 << 40)) return fail(kInvalidArgument, fmt("%s: pitch %zu is too large", who, pitch));
    const size_t y_bytes = pitch * h;
    if (layout->uv_offset != 0 && layout->uv_offset < y_bytes)
        return fail(kInvalidArgument, fmt("%s: uv_offset must be 0 or at least %zu, got %zu", who, y_bytes, layout->uv_offset));
    if (layout->uv_offset > ((size_t)1 << 62)) return fail(kInvalidArgument, fmt("%s: uv_offset %zu is too large", who, layout->uv_offset));
    out->y_pitch = out->uv_pitch = pitch;
    out->uv_offset = layout->uv_offset ? layout->uv_offset : y_bytes;
    out->bytes = out->uv_offset + pitch * ch;
    return kOk;
}

size_t nv12_frame_bytes(uint32_t w, uint32_t h, const Nv12Layout *layout)
{
    const char *who = "nus_nv12_frame_bytes";
    Nv12Frame f;
    if (check_dims_yuv(who, w, h) != kOk || resolve_nv12(who, w, h, layout, &f) != kOk) return 0;
    return f.bytes;
}

namespace {

// every check of an NV12 <-> RGBA device entry point; fills the launch
int prepare_nv12(const char *who, const void *d_nv12, const Nv12Layout *layout, size_t nv12_frame_stride, const void *d_rgba,
                 size_t rgba_frame_stride, uint32_t w, uint32_t h, const YuvFormat *f, int rgba_format, uint32_t n_frames, hipStream_t stream,
                 Nv12Launch *L)
{
    if (!d_nv12 || !d_rgba || !f) return fail(kInvalidArgument, fmt("%s: null pointer", who));
    int st = check_dims_yuv(who, w, h);
    if (st != kOk || (st = check_formats(who, f, rgba_format)) != kOk) return st;
    if (n_frames == 0) return fail(kInvalidArgument, fmt("%s: n_frames must be at least 1", who));
    Nv12Frame fr;
    if ((st = resolve_nv12(who, w, h, layout, &fr)) != kOk) return st;
    const size_t rgba_bytes = (size_t)w * h * 4;
    if (rgba_frame_stride != 0 && (rgba_frame_stride < rgba_bytes || (rgba_frame_stride % 4) != 0))
        return fail(kInvalidArgument, fmt("%s: rgba_frame_stride must be 0 or a multiple of 4 of at least %zu, got %zu", who, rgba_bytes, rgba_frame_stride));
    if (nv12_frame_stride != 0 && nv12_frame_stride < fr.bytes)
        return fail(kInvalidArgument, fmt("%s: nv12_frame_stride must be 0 or at least %zu, got %zu", who, fr.bytes, nv12_frame_stride));
    if (misaligned(d_rgba, 4)) return fail(kInvalidArgument, fmt("%s: the RGBA frames must be 4-byte aligned", who));
    YuvLaunch &C = L->c;
    C.yuv = static_cast<uint8_t *>(const_cast<void *>(d_nv12)), C.rgba = static_cast<uint8_t *>(const_cast<void *>(d_rgba));
    C.yuv_frame_stride = nv12_frame_stride ? nv12_frame_stride : fr.bytes;
    C.rgba_frame_stride = rgba_frame_stride ? rgba_frame_stride : rgba_bytes;
    C.w = w, C.h = h, C.n_frames = n_frames, C.siting = f->siting, C.chroma_filter = f->chroma_filter;
    yuv_coefficients(f->matrix, f->range, C.to_yuv, C.to_rgb, &C.y_offset);
    C.sel = input_selector(rgba_format), C.stream = stream;
    L->y_pitch = fr.y_pitch, L->uv_pitch = fr.uv_pitch, L->uv_offset = fr.uv_offset;
    return kOk;
}

// every check of a repack entry point; fills the launch
int prepare_repack(const char *who, const void *d_i420, size_t i420_frame_stride, const void *d_nv12, const Nv12Layout *layout,
                   size_t nv12_frame_stride, uint32_t w, uint32_t h, uint32_t n_frames, hipStream_t stream, Nv12RepackLaunch *L)
{
    if (!d_i420 || !d_nv12) return fail(kInvalidArgument, fmt("%s: null pointer", who));
    int st = check_dims_yuv(who, w, h);
    if (st != kOk) return st;
    if (n_frames == 0) return fail(kInvalidArgument, fmt("%s: n_frames must be at least 1", who));
    Nv12Frame fr;
    if ((st = resolve_nv12(who, w, h, layout, &fr)) != kOk) return st;
    const size_t i420_bytes = frame_bytes_unchecked(w, h);
    if (i420_frame_stride != 0 && i420_frame_stride < i420_bytes)
        return fail(kInvalidArgument, fmt("%s: i420_frame_stride must be 0 or at least %zu, got %zu", who, i420_bytes, i420_frame_stride));
    if (nv12_frame_stride != 0 && nv12_frame_stride < fr.bytes)
        return fail(kInvalidArgument, fmt("%s: nv12_frame_stride must be 0 or at least %zu, got %zu", who, fr.bytes, nv12_frame_stride));
    L->i420 = static_cast<uint8_t *>(const_cast<void *>(d_i420)), L->nv12 = static_cast<uint8_t *>(const_cast<void *>(d_nv12));
    L->i420_frame_stride = i420_frame_stride ? i420_frame_stride : i420_bytes;
    L->nv12_frame_stride = nv12_frame_stride ? nv12_frame_stride : fr.bytes;
    L->y_pitch = fr.y_pitch, L->uv_pitch = fr.uv_pitch, L->uv_offset = fr.uv_offset;
    L->w = w, L->h = h, L->n_frames = n_frames, L->stream = stream;
    return kOk;
}

} // namespace

int nv12_to_rgba8_device(const void *d_nv12, const Nv12Layout *layout, size_t nv12_frame_stride, uint32_t w, uint32_t h, const YuvFormat *f,
                         int rgba_format, void *d_rgba, size_t rgba_frame_stride, uint32_t n_frames, hipStream_t stream)
{
    Nv12Launch L;
    const int st = prepare_nv12("nus_nv12_to_rgba8_device", d_nv12, layout, nv12_frame_stride, d_rgba, rgba_frame_stride, w, h, f, rgba_format,
                                n_frames, stream, &L);
    if (st != kOk) return st;
    if (device_count() <= 0) return fail(kNoDevice, "nus_nv12_to_rgba8_device: no HIP device available");
    const hipError_t e = launch_nv12_to_rgba(L);
    return e != hipSuccess ? fail_hip(e, "nv12-to-rgba launch") : kOk;
}

int rgba8_to_nv12_device(const void *d_rgba, size_t rgba_frame_stride, uint32_t w, uint32_t h, const YuvFormat *f, int rgba_format,
                         void *d_nv12, const Nv12Layout *layout, size_t nv12_frame_stride, uint32_t n_frames, hipStream_t stream)
{
    Nv12Launch L;
    const int st = prepare_nv12("nus_rgba8_to_nv12_device", d_nv12, layout, nv12_frame_stride, d_rgba, rgba_frame_stride, w, h, f, rgba_format,
                                n_frames, stream, &L);
    if (st != kOk) return st;
    if (device_count() <= 0) return fail(kNoDevice, "nus_rgba8_to_nv12_device: no HIP device available");
    const hipError_t e = launch_rgba_to_nv12(L);
    return e != hipSuccess ? fail_hip(e, "rgba-to-nv12 launch") : kOk;
}

int nv12_to_rgba8(int device, const uint8_t *nv12, size_t nv12_len, uint32_t w, uint32_t h, const YuvFormat *f, int rgba_format,
                  uint8_t *rgba, size_t rgba_cap)
{
    const char *who = "nus_nv12_to_rgba8";
    if (!nv12 || !rgba || !f) return fail(kInvalidArgument, fmt("%s: null pointer", who));
    int r = check_dims_yuv(who, w, h);
    if (r != kOk || (r = check_formats(who, f, rgba_format)) != kOk) return r;
    const size_t nv12_bytes = frame_bytes_unchecked(w, h), rgba_bytes = (size_t)w * h * 4;
    if ((r = check_host(who, nv12_len, nv12_bytes, "nv12_len", rgba_cap, rgba_bytes, "rgba_cap", w, h)) != kOk) return r;
    if ((r = check_device(who, device)) != kOk) return r;
    PairScratch &s = scratch_of(device);
    std::lock_guard<std::mutex> lock(s.m);
    if ((r = s.prepare(device, rgba_bytes, 0, 0)) != kOk) return r;
    if ((r = upload(s.a.get(), nv12, nv12_bytes, s.stream)) != kOk) return r;
    if ((r = nv12_to_rgba8_device(s.a.get(), nullptr, 0, w, h, f, rgba_format, s.b.get(), 0, 1, s.stream)) != kOk) return r;
    return download(rgba, s.b.get(), rgba_bytes, s.stream);
}

int rgba8_to_nv12(int device, const uint8_t *rgba, size_t rgba_len, uint32_t w, uint32_t h, const YuvFormat *f, int rgba_format,
                  uint8_t *nv12, size_t nv12_cap)
{
    const char *who = "nus_rgba8_to_nv12";
    if (!nv12 || !rgba || !f) return fail(kInvalidArgument, fmt("%s: null pointer", who));
    int r = check_dims_yuv(who, w, h);
    if (r != kOk || (r = check_formats(who, f, rgba_format)) != kOk) return r;
    const size_t nv12_bytes = frame_bytes_unchecked(w, h), rgba_bytes = (size_t)w * h * 4;
    if ((r = check_host(who, rgba_len, rgba_bytes, "rgba_len", nv12_cap, nv12_bytes, "nv12_cap", w, h)) != kOk) return r;
    if ((r = check_device(who, device)) != kOk) return r;
    PairScratch &s = scratch_of(device);
    std::lock_guard<std::mutex> lock(s.m);
    if ((r = s.prepare(device, rgba_bytes, 0, 0)) != kOk) return r;
    if ((r = upload(s.a.get(), rgba, rgba_bytes, s.stream)) != kOk) return r;
    if ((r = rgba8_to_nv12_device(s.a.get(), 0, w, h, f, rgba_format, s.b.get(), nullptr, 0, 1, s.stream)) != kOk) return r;
    return download(nv12, s.b.get(), nv12_bytes, s.stream);
}

int yuv420_to_nv12_device(const void *d_i420, size_t i420_frame_stride, uint32_t w, uint32_t h, void *d_nv12, const Nv12Layout *layout,
                          size_t nv12_frame_stride, uint32_t n_frames, hipStream_t stream)
{
    Nv12RepackLaunch L;
    const int st = prepare_repack("nus_yuv420_to_nv12_device", d_i420, i420_frame_stride, d_nv12, layout, nv12_frame_stride, w, h, n_frames, stream, &L);
    if (st != kOk) return st;
    if (device_count() <= 0) return fail(kNoDevice, "nus_yuv420_to_nv12_device: no HIP device available");
    const hipError_t e = launch_i420_to_nv12(L);
    return e != hipSuccess ? fail_hip(e, "i420-to-nv12 launch") : kOk;
}

int nv12_to_yuv420_device(const void *d_nv12, const Nv12Layout *layout, size_t nv12_frame_stride, uint32_t w, uint32_t h, void *d_i420,
                          size_t i420_frame_stride, uint32_t n_frames, hipStream_t stream)
{
    Nv12RepackLaunch L;
    const int st = prepare_repack("nus_nv12_to_yuv420_device", d_i420, i420_frame_stride, d_nv12, layout, nv12_frame_stride, w, h, n_frames, stream, &L);
    if (st != kOk) return st;
    if (device_count() <= 0) return fail(kNoDevice, "nus_nv12_to_yuv420_device: no HIP device available");
    const hipError_t e = launch_nv12_to_i420(L);
    return e != hipSuccess ? fail_hip(e, "nv12-to-i420 launch") : kOk;
}

} // namespace nus
