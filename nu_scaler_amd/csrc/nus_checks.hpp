// nus_checks.hpp -- the status codes, the calling thread's error text and the argument checks that more than one host entry point
// makes.  No HIP here: every check runs before any HIP call, and tests/c_abi/host_checks_sanitize.cpp builds this unit alone with
// a plain C++ compiler.  Each check returns kOk, or the failed status with the thread's error text set; `who` is the C entry point
// the text names.  Internal.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>

namespace nus {

// nus_status values (kept in sync with include/nuscaler_hip.h).
enum Status : int {
    kOk = 0,
    kInvalidArgument = -1,
    kNotInitialized = -2,
    kSizeMismatch = -3,
    kHipError = -4,
    kNoDevice = -5,
    kUnsupported = -6,
    kOutOfMemory = -7,
};

constexpr int kMaxDevices = 64;         // per-device state (transfer rings, pair scratch) is an array of this many
constexpr uint32_t kMaxInterpTimes = 7; // == kInterpMaxTimes of nus_kernels.hpp (asserted in nus_host_util.hpp)

void set_thread_error(const std::string &msg);
const char *thread_error();

std::string fmt(const char *f, ...) __attribute__((format(printf, 1, 2)));

int fail(int status, const std::string &msg); // sets the thread's error text, returns `status`

inline bool misaligned(const void *p, uintptr_t to) { return (reinterpret_cast<uintptr_t>(p) % to) != 0; }

// "<who>: <text>" unless w, h are non-zero and w * h <= max_pixels
int check_dims(const char *who, uint32_t w, uint32_t h, uint64_t max_pixels, const char *text = "bad dimensions");
// "<who>: WxH frames are too large" when w * h > max_pixels (the callers have refused zero with a text of their own)
int check_frame_area(const char *who, uint32_t w, uint32_t h, uint64_t max_pixels);
// frame pointers and strides of pairs: multiples of 4 bytes, strides of at least one w x h frame
int check_pairs(const char *who, const void *a, size_t a_stride, const void *b, size_t b_stride, uint32_t w, uint32_t h);
// "pointers/strides must be pixel aligned": frames, strides, `out` and `also` to 4 bytes, `flow` to flow_align (null: not checked)
int check_pixel_aligned(const char *who, const void *a, size_t a_stride, const void *b, size_t b_stride, const void *out,
                        const void *flow, uintptr_t flow_align, const void *also = nullptr);
// both host frames w * h * 4 bytes long, else kSizeMismatch with the reference's text (wgpu_interpolator.rs:234-237)
int check_frame_lengths(size_t a_len, size_t b_len, uint32_t w, uint32_t h);
// the time set of the multi-time entry points: 1 .. kMaxInterpTimes times, each in [0, 1] (NaN is not)
int check_interp_times(const char *who, const float *times, uint32_t n_times);
// 0 (tightly packed) or a multiple of 4 of at least n_times frames
int check_out_pair_stride(const char *who, size_t out_pair_stride, uint32_t n_times, size_t frame_bytes);
// the caller's workspace against what `sizer` (the C function that says so) asks for
int check_workspace(const char *who, size_t workspace_bytes, size_t need, const char *sizer);

} // namespace nus
