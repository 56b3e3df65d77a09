// nus_scene.hpp -- scene-cut detection of frame pairs and the cut-aware output rule (nus_scene_* of include/nuscaler_hip.h;
// kernels in nus_k_scene.hip).  Every function returns a Status (nus_host.hpp) and leaves its text in the thread's error slot;
// argument checks come before any HIP call and their texts name the C entry point.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

namespace nus {

constexpr uint32_t kSceneDefaultMad = 20, kSceneDefaultHistPermille = 400; // settings, not measurements

// empty when (mad_threshold, hist_permille) are settings the detector takes, else what is wrong with them
std::string check_scene_thresholds(uint32_t mad_threshold, uint32_t hist_permille);

// empty when n_pairs pairs of w x h frames fit one launch of every scene kernel (at most 2^32 - 1 work-items), else the reason
std::string check_scene_launch(uint32_t w, uint32_t h, uint32_t n_pairs);

// 0 (and the reason in the thread's error slot) for an invalid shape
size_t scene_workspace_size(uint32_t w, uint32_t h, uint32_t n_pairs);
int scene_detect_device(const void *d_a, size_t a_stride, const void *d_b, size_t b_stride, uint32_t w, uint32_t h, uint32_t n_pairs,
                        int format, uint32_t mad_threshold, uint32_t hist_permille, void *d_workspace, size_t workspace_bytes,
                        void *d_measures, uint8_t *d_cut, hipStream_t stream);
// measures_out (may be null): {u64 sad, u32 hist_l1, u32 0}; cut_out: one u8
int scene_detect(int device, const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len, uint32_t w, uint32_t h, int format,
                 uint32_t mad_threshold, uint32_t hist_permille, void *measures_out, uint8_t *cut_out);
int scene_apply_cuts_device(const void *d_a, size_t a_stride, const void *d_b, size_t b_stride, uint32_t w, uint32_t h, int format,
                            const float *times, uint32_t n_times, const uint8_t *d_cut, void *d_out, size_t out_pair_stride,
                            uint32_t n_pairs, hipStream_t stream);
// bit k set = times[k] < 0.5: frame k of a cut pair repeats A, else B
uint32_t scene_from_a_mask(const float *times, uint32_t n_times);

} // namespace nus
