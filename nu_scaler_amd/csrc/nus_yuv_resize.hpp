// nus_yuv_resize.hpp -- host side of the planar up-scaler of I420 and tight NV12 frames (nus_yuv_resizer of include/nuscaler_hip.h,
// where the contract is written; kernels in nus_k_yuv_resize.hip, and nus_k_nv12_resize.hip for the plane of U,V pairs).  Every
// function returns a Status (nus_checks.hpp); argument checks come before any HIP call and their texts name the C entry point.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <mutex>
#include <vector>

#include "nus_host_util.hpp"

namespace nus {

class YuvResizer : public HostErrors {
public:
    YuvResizer() = default;
    ~YuvResizer();
    YuvResizer(const YuvResizer &) = delete;
    YuvResizer &operator=(const YuvResizer &) = delete;

    int set_device(int device);
    // Builds the four axis tables (luma x / y, chroma x / y) on the host; no HIP call.
    int initialize(uint32_t iw, uint32_t ih, uint32_t ow, uint32_t oh, int algorithm, int siting, int mode);
    int export_axis(int plane, int axis, int32_t *left, uint32_t *ntaps, float *weights);
    int resize_device(const void *d_in, size_t in_frame_stride, void *d_out, size_t out_frame_stride, uint32_t n_frames, hipStream_t stream);
    int resize(const uint8_t *in, size_t in_len, uint8_t *out, size_t out_cap);
    // the same on tight NV12 frames: the luma launch unchanged, one launch over the plane of U,V pairs (nus_k_nv12_resize.hip)
    int resize_nv12_device(const void *d_in, size_t in_frame_stride, void *d_out, size_t out_frame_stride, uint32_t n_frames, hipStream_t stream);
    int resize_nv12(const uint8_t *in, size_t in_len, uint8_t *out, size_t out_cap);

private:
    struct Axis { // build_resize_axis' tables and what the row kernel needs to know of them
        uint32_t in_n = 0, out_n = 0;
        std::vector<int32_t> left;
        std::vector<uint32_t> ntaps;
        std::vector<float> w; // out_n * kResizeMaxTaps
        int max_taps = 0;
        uint32_t ncols_max = 0, union_taps = 0; // as the x axis of a plane (the row kernel's geometry)
        // as the x axis of a plane of U,V pairs (the pair row kernel's geometry): widest dword-aligned input footprint of a wave's
        // segment in BYTES, widest union of the windows of a lane's run of two pairs in cells; 0 where that kernel does not fit
        uint32_t pair_ncols_max = 0, pair_union = 0;
        size_t d_offset = 0;                    // of left / ntaps / w in the device blob, in 4-byte words
    };
    int ensure_tables(const char *who); // first device use: the device current, the four axes uploaded once
    int enqueue(const char *who, const uint8_t *d_in, size_t in_stride, uint8_t *d_out, size_t out_stride, uint32_t n_frames, hipStream_t stream,
                bool nv12 = false);
    int device_call(const char *who, bool nv12, const void *d_in, size_t in_frame_stride, void *d_out, size_t out_frame_stride, uint32_t n_frames,
                    hipStream_t stream);
    int host_call(const char *who, bool nv12, const uint8_t *in, size_t in_len, uint8_t *out, size_t out_cap);
    void drop_tables();

    mutable std::mutex mu_;
    int device_ = 0;
    bool ready_ = false, exact_ = false;
    uint32_t iw_ = 0, ih_ = 0, ow_ = 0, oh_ = 0;
    size_t in_bytes_ = 0, out_bytes_ = 0;
    Axis axis_[2][2]; // [plane: luma, chroma][axis: x, y]
    uint32_t *d_tables_ = nullptr;
    bool device_used_ = false;
    hipStream_t stream_ = nullptr;
    DeviceBuffer d_in_, d_out_;
};

} // namespace nus
