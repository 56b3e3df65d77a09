// nus_metrics.hpp -- image-quality metrics of frame pairs (nus_metrics_* of include/nuscaler_hip.h; kernels in nus_k_metrics.hip).
// Every function returns a Status (nus_host.hpp) and leaves its text in the thread's error slot; argument checks come before
// any HIP call.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace nus {

// 0 (and the reason in the thread's error slot) for an invalid shape or metric mask
size_t metrics_workspace_size(uint32_t w, uint32_t h, uint32_t frames, int what);
int metrics_compare_device(const void *d_a, size_t a_stride, const void *d_b, size_t b_stride, uint32_t w, uint32_t h,
                           uint32_t frames, int what, void *d_workspace, size_t workspace_bytes, double *d_out, hipStream_t stream);
int metrics_compare(int device, const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len, uint32_t w, uint32_t h, int what,
                    double *out);

} // namespace nus
