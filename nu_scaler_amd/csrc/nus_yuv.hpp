// nus_yuv.hpp -- 8-bit planar YUV 4:2:0 (I420) <-> RGBA8 (nus_yuv* of include/nuscaler_hip.h; kernels in nus_k_yuv.hip).  Every
// function returns a Status (nus_checks.hpp) and leaves its text in the thread's error slot; argument checks come before any HIP
// call and their texts name the C entry point.  Handle-free, like nus_scene.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace nus {

struct YuvFormat { // nus_yuv_format
    int matrix, range, siting, chroma_filter;
};

// w * h + 2 * ((w + 1) / 2) * ((h + 1) / 2); 0 (and the reason in the thread's error slot) for dimensions the kernels do not take
size_t yuv420_frame_bytes(uint32_t w, uint32_t h);
// The Q14 tables of include/nuscaler_hip.h's contract, derived in double: to_yuv = Yc, Uc, Vc over (R, G, B); to_rgb = cy, rv, bu,
// gu, gv.  Host only.  The luma offset Yo (16 / 0) goes to *y_offset if given.
int yuv_coefficients(int matrix, int range, int32_t *to_yuv, int32_t *to_rgb, int32_t *y_offset = nullptr);

int yuv420_to_rgba8_device(const void *d_yuv, size_t yuv_frame_stride, uint32_t w, uint32_t h, const YuvFormat *fmt, int rgba_format,
                           void *d_rgba, size_t rgba_frame_stride, uint32_t n_frames, hipStream_t stream);
int rgba8_to_yuv420_device(const void *d_rgba, size_t rgba_frame_stride, uint32_t w, uint32_t h, const YuvFormat *fmt, int rgba_format,
                           void *d_yuv, size_t yuv_frame_stride, uint32_t n_frames, hipStream_t stream);
// one host frame each, through upload / download and device buffers kept per device
int yuv420_to_rgba8(int device, const uint8_t *yuv, size_t yuv_len, uint32_t w, uint32_t h, const YuvFormat *fmt, int rgba_format,
                    uint8_t *rgba, size_t rgba_cap);
int rgba8_to_yuv420(int device, const uint8_t *rgba, size_t rgba_len, uint32_t w, uint32_t h, const YuvFormat *fmt, int rgba_format,
                    uint8_t *yuv, size_t yuv_cap);

// ---- NV12 frames ("NV12 frames" in include/nuscaler_hip.h; kernels in nus_k_nv12.hip) ----------------------------------------------
struct Nv12Layout { // nus_nv12_layout
    size_t pitch, uv_offset;
};
// the layout resolved for w x h: where the rows and the pair plane lie, and the bytes of a frame
struct Nv12Frame {
    size_t y_pitch = 0, uv_pitch = 0, uv_offset = 0, bytes = 0;
};
// "<who>: ..." and kInvalidArgument for a layout the contract does not take (w, h already checked); null = tight
int resolve_nv12(const char *who, uint32_t w, uint32_t h, const Nv12Layout *layout, Nv12Frame *out);
size_t nv12_frame_bytes(uint32_t w, uint32_t h, const Nv12Layout *layout); // 0 and the reason in the thread's error slot

int nv12_to_rgba8_device(const void *d_nv12, const Nv12Layout *layout, size_t nv12_frame_stride, uint32_t w, uint32_t h, const YuvFormat *fmt,
                         int rgba_format, void *d_rgba, size_t rgba_frame_stride, uint32_t n_frames, hipStream_t stream);
int rgba8_to_nv12_device(const void *d_rgba, size_t rgba_frame_stride, uint32_t w, uint32_t h, const YuvFormat *fmt, int rgba_format,
                         void *d_nv12, const Nv12Layout *layout, size_t nv12_frame_stride, uint32_t n_frames, hipStream_t stream);
// one tight host frame each, as yuv420_to_rgba8 / rgba8_to_yuv420
int nv12_to_rgba8(int device, const uint8_t *nv12, size_t nv12_len, uint32_t w, uint32_t h, const YuvFormat *fmt, int rgba_format,
                  uint8_t *rgba, size_t rgba_cap);
int rgba8_to_nv12(int device, const uint8_t *rgba, size_t rgba_len, uint32_t w, uint32_t h, const YuvFormat *fmt, int rgba_format,
                  uint8_t *nv12, size_t nv12_cap);
// the repack: bytes only
int yuv420_to_nv12_device(const void *d_i420, size_t i420_frame_stride, uint32_t w, uint32_t h, void *d_nv12, const Nv12Layout *layout,
                          size_t nv12_frame_stride, uint32_t n_frames, hipStream_t stream);
int nv12_to_yuv420_device(const void *d_nv12, const Nv12Layout *layout, size_t nv12_frame_stride, uint32_t w, uint32_t h, void *d_i420,
                          size_t i420_frame_stride, uint32_t n_frames, hipStream_t stream);

} // namespace nus
