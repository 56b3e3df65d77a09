// nus_blockmatch.hpp -- host side of the block-matching motion estimator (nus_bm_* of include/nuscaler_hip.h; kernels in
// nus_k_blockmatch.hip): BlockMatchingInterpolator of nu_scaler_core/src/interpolation/mod.rs:513-911.  Every function returns a
// Status (nus_host.hpp); argument checks come before any HIP call and their texts name the C entry point.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <mutex>
#include <string>
#include <vector>

#include "nus_host_util.hpp"

namespace nus {

constexpr int kBmTiesScan = 0, kBmTiesCenter = 1; // nus_bm_tie_order

// Place of every candidate of a (2R + 1)^2 search in the tie order (rank[(dy + R) * (2R + 1) + dx + R]) and the inverse
// (cand[rank]).  Host only.
void bm_rank_tables(uint32_t R, int order, std::vector<uint16_t> &rank, std::vector<uint16_t> &cand);

class BlockMatcher : public HostErrors {
public:
    BlockMatcher() = default;
    ~BlockMatcher();
    BlockMatcher(const BlockMatcher &) = delete;
    BlockMatcher &operator=(const BlockMatcher &) = delete;

    int set_device(int device);
    int set_params(uint32_t block_size, uint32_t search_radius);
    int set_quality(int quality); // nus_interp_quality_level: High 8 / 24, Medium 16 / 16, Low 32 / 8 (interpolation/mod.rs:531-542)
    int set_tie_order(int order);
    int set_refine(int enabled);
    // Forward-backward check (nus_bm_set_bidirectional): off by default.  On, every pair is searched both ways and the blocks the
    // two searches disagree on are repaired; the confidence pass is not run, and both workspaces grow.
    int set_bidirectional(int enabled, uint32_t tolerance);
    // Scene-cut detection in front of interpolate() and the cut-aware output rule behind it (nus_scene_* of the C header): off by
    // default.  On, the frames of a pair the detector flags are repeats of the nearer real frame.
    int set_scene_detect(int enabled, uint32_t mad_threshold, uint32_t hist_permille);
    size_t workspace_size(uint32_t w, uint32_t h, uint32_t n_pairs); // 0 and the reason for an invalid shape
    int estimate_device(const void *d_a, size_t a_stride, const void *d_b, size_t b_stride, uint32_t w, uint32_t h, uint32_t n_pairs,
                        void *d_workspace, size_t workspace_bytes, void *d_vectors, void *d_sad, void *d_flags, void *d_flow,
                        int flow_format, hipStream_t stream);
    // warp + blend of n_pairs pairs straight from their block vectors (estimate_device's layout at this handle's block size):
    // enqueue only.  Frames, strides, time set, mode and out_pair_stride as the dense multi-time warp's.
    int warp_device(const void *d_a, size_t a_stride, const void *d_b, size_t b_stride, uint32_t w, uint32_t h, uint32_t n_pairs,
                    const void *d_vectors, const float *times, uint32_t n_times, int mode, void *d_out, size_t out_pair_stride,
                    hipStream_t stream);
    // n_frames frames frame_stride apart -> the frames of every pair (k, k + 1): search, confidence pass or forward-backward check, warp_device's kernel and,
    // with detection on, the cut rule.  Enqueue only; the workspace is the caller's.
    size_t stream_workspace_size(uint32_t w, uint32_t h, uint32_t n_frames); // 0 and the reason for an invalid shape
    int interpolate_multi_device_stream(const void *d_frames, size_t frame_stride, uint32_t n_frames, uint32_t w, uint32_t h,
                                        const float *times, uint32_t n_times, int mode, void *d_workspace, size_t workspace_bytes,
                                        void *d_vectors, void *d_mid, size_t mid_pair_stride, hipStream_t stream);
    // Frame-rate conversion of the stream by num / den (nus_bm_retime_device_stream; the schedule is nus_retime.hpp's): the search
    // and the confidence pass as above, then the retime warp from the block vectors and the copy of the real frames; output j at
    // d_out + j * out_frame_stride (0: tightly packed).  The workspace is stream_workspace_size's.
    int retime_device_stream(const void *d_frames, size_t frame_stride, uint32_t n_frames, uint32_t w, uint32_t h, uint32_t num,
                             uint32_t den, int mode, void *d_workspace, size_t workspace_bytes, void *d_vectors, void *d_out,
                             size_t out_frame_stride, hipStream_t stream);
    int estimate(const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len, uint32_t w, uint32_t h, int16_t *vectors_out,
                 uint32_t *sad_out, uint8_t *flags_out);
    int interpolate(const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len, uint32_t w, uint32_t h, const float *times,
                    uint32_t n_times, int mode, uint8_t *out, size_t out_cap);

private:
    struct StreamLayout { // offsets into the stream entry point's workspace (the search's own part starts it)
        size_t o_vec = 0, o_scene = 0, o_cut = 0, total = 0;
    };
    StreamLayout stream_layout(uint32_t w, uint32_t h, uint32_t n_pairs) const;
    int enqueue_warp(const void *d_a, size_t a_stride, const void *d_b, size_t b_stride, uint32_t w, uint32_t h, uint32_t n_pairs,
                     const void *d_vectors, const float *times, uint32_t n_times, int mode, void *d_out, size_t out_pair_stride,
                     hipStream_t stream);
    int check_shape(const char *who, uint32_t w, uint32_t h, uint32_t n_pairs);
    int check_host_frames(const char *who, const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len, uint32_t w, uint32_t h);
    int ensure_tables();                 // first device use: the rank tables of every radius and both orders, once
    int ensure_host(size_t bytes);       // the host entry points' device arena
    int enqueue(const void *d_a, size_t a_stride, const void *d_b, size_t b_stride, uint32_t w, uint32_t h, uint32_t n_pairs,
                void *d_workspace, void *d_vectors, void *d_sad, void *d_flags, void *d_flow, int flow_format, hipStream_t stream);

    mutable std::mutex mu_;
    int device_ = 0;
    uint32_t bs_ = 16, radius_ = 16; // Medium
    int order_ = kBmTiesCenter;
    bool refine_ = true;
    bool bidir_ = false;
    uint32_t tolerance_ = 2;
    bool scene_ = false;
    uint32_t scene_mad_ = 20, scene_hist_ = 400;
    uint16_t *d_tables_ = nullptr;
    hipStream_t stream_ = nullptr;
    DeviceBuffer arena_;
};

} // namespace nus
