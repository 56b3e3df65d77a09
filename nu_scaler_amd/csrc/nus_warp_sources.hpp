// nus_warp_sources.hpp -- the three vector sources of warp_blend_tile (nus_warp_device.hpp): the dense flow at the thread's own
// pixels (k_warp_blend_flow, nus_k_interp.hip), the flow projected to the in-between time (k_warp_blend_flow_proj,
// nus_k_warp_project.hip) and the per-block vectors (k_bm_warp, nus_k_bm_warp.hip).  In a header because the rate-conversion
// kernels (nus_k_retime.hip) instantiate the tile with each of them and another time source: the same code, the same bytes.
#pragma once

#include "nus_device.hpp"
#include "nus_flow_project_device.hpp"
#include "nus_warp_device.hpp"

#include <hip/hip_fp16.h>

namespace nus {

namespace {

__device__ __forceinline__ float2 widen(uint32_t bits) // one 2 x f16 flow vector
{
    const __half2 hf = *reinterpret_cast<const __half2 *>(&bits);
    return make_float2(__low2float(hf), __high2float(hf));
}

// XV = 2: the two flow vectors of a row are one 16-byte (8-byte) load (w even and the plane 16-byte aligned, host-checked).
// HALF: the flow field is the Rg16Float texture of the reference's live path (wgpu_interpolator.rs:276), widened exactly.
template <bool HALF, int XV, int RV>
struct DenseFlowSource {
    static constexpr bool kSwizzle = true;
    const void *flow;
    float2 f[RV][XV];

    __device__ __forceinline__ void load(uint32_t ybase, uint32_t x0, uint32_t w, uint32_t h, size_t npx)
    {
#pragma unroll
        for (int j = 0; j < RV; ++j) {
            const size_t idx = (size_t)blockIdx.z * npx + (size_t)umin(ybase + 4 * j, h - 1) * w + x0;
            if (XV == 2 && HALF) {
                const uint2 raw = *reinterpret_cast<const uint2 *>(static_cast<const uint32_t *>(flow) + idx);
                f[j][0] = widen(raw.x), f[j][XV - 1] = widen(raw.y);
            } else if (XV == 2) {
                const float4 v = *reinterpret_cast<const float4 *>(static_cast<const float2 *>(flow) + idx);
                f[j][0] = make_float2(v.x, v.y), f[j][XV - 1] = make_float2(v.z, v.w);
            } else {
                f[j][0] = HALF ? widen(static_cast<const uint32_t *>(flow)[idx]) : static_cast<const float2 *>(flow)[idx];
            }
        }
    }
    __device__ __forceinline__ void at_time(uint32_t, uint32_t, uint32_t, uint32_t, float, float, float) {}
    __device__ __forceinline__ float2 vec(int j, int i) const { return f[j][i]; }
};

// The thread's own flow vectors are loaded first; per time, the N rounds run round by round over all the thread's pixels, so the
// gathers of a round -- two loads per pixel, independent chains -- are in flight together.  The flow plane is reached through a
// buffer resource bound to the pair's own plane, like the frames.
template <bool HALF, int XV, int RV>
struct ProjectedFlowSource {
    static constexpr bool kSwizzle = true;
    static constexpr uint32_t kCellBytes = HALF ? 4 : 8;
    const void *flow;
    uint32_t rounds;
    __amdgpu_buffer_rsrc_t rf;
    float2 f[RV][XV], g[RV][XV];

    __device__ __forceinline__ void load(uint32_t ybase, uint32_t x0, uint32_t w, uint32_t h, size_t npx)
    {
        typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        // the pair's own flow plane (below 4 GiB: host-checked): a coordinate outside it reads zeros, never another pair's vectors
        rf = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(static_cast<const uint8_t *>(flow) + (size_t)blockIdx.z * npx * kCellBytes),
                                               0, (uint32_t)(npx * kCellBytes), 0x00020000);
#pragma unroll
        for (int j = 0; j < RV; ++j) {
            const uint32_t off = (umin(ybase + 4 * j, h - 1) * w + x0) * kCellBytes;
            if (XV == 2) { // (w even: both cells are in the row)
                if (HALF) {
                    const u32x2 raw = __builtin_amdgcn_raw_buffer_load_b64(rf, off, 0, 0);
                    f[j][0] = half2_bits_to_float2(raw.x), f[j][XV - 1] = half2_bits_to_float2(raw.y);
                } else {
                    const u32x4 raw = __builtin_amdgcn_raw_buffer_load_b128(rf, off, 0, 0);
                    f[j][0] = make_float2(__uint_as_float(raw.x), __uint_as_float(raw.y));
                    f[j][XV - 1] = make_float2(__uint_as_float(raw.z), __uint_as_float(raw.w));
                }
            } else {
                if (HALF) {
                    f[j][0] = half2_bits_to_float2(__builtin_amdgcn_raw_buffer_load_b32(rf, off, 0, 0));
                } else {
                    const u32x2 raw = __builtin_amdgcn_raw_buffer_load_b64(rf, off, 0, 0);
                    f[j][0] = make_float2(__uint_as_float(raw.x), __uint_as_float(raw.y));
                }
            }
        }
    }
    __device__ __forceinline__ void at_time(uint32_t ybase, uint32_t x0, uint32_t w, uint32_t h, float wmax, float hmax, float tv)
    {
#pragma unroll
        for (int j = 0; j < RV; ++j)
#pragma unroll
            for (int i = 0; i < XV; ++i) g[j][i] = f[j][i];
#pragma unroll 1
        for (uint32_t r = 0; r < rounds; ++r) { // round by round: the gathers of all the thread's pixels issued, then their lerps
            ProjectGather<HALF> G[RV][XV];
#pragma unroll
            for (int j = 0; j < RV; ++j) {
                const float yfl = (float)umin(ybase + 4 * j, h - 1); // (rows past the frame repeat the last row's: no branch between the chains)
#pragma unroll
                for (int i = 0; i < XV; ++i)
                    G[j][i] = project_gather_corner<HALF>(rf, w, wmax, hmax, w - 2, h - 2, (float)(x0 + i), yfl, g[j][i], tv);
            }
#pragma unroll
            for (int j = 0; j < RV; ++j)
#pragma unroll
                for (int i = 0; i < XV; ++i) g[j][i] = project_finish_corner<HALF>(G[j][i]);
        }
    }
    __device__ __forceinline__ float2 vec(int j, int i) const { return g[j][i]; }
};

// The thread's XV pixels start at a multiple of XV and the block size is a multiple of XV, so they lie in ONE block: one 4-byte
// vector load per row of the thread.  No input channel selector: the block-matching path takes RGBA frames.
template <int RV>
struct BlockVectorSource {
    static constexpr bool kSwizzle = false;
    const short2 *vectors;
    uint32_t bs_log2, blocks_x, blocks_y;
    float2 f[RV];

    __device__ __forceinline__ void load(uint32_t ybase, uint32_t x0, uint32_t w, uint32_t h, size_t npx)
    {
        const short2 *const pair_vectors = vectors + (size_t)blockIdx.z * blocks_x * blocks_y;
        const uint32_t bx = x0 >> bs_log2; // x0 % XV == 0 and XV divides the block size: the thread's XV pixels share the block
#pragma unroll
        for (int j = 0; j < RV; ++j) {
            const short2 v = pair_vectors[(size_t)(umin(ybase + 4 * j, h - 1) >> bs_log2) * blocks_x + bx];
            f[j] = make_float2((float)v.x, (float)v.y);
        }
    }
    __device__ __forceinline__ void at_time(uint32_t, uint32_t, uint32_t, uint32_t, float, float, float) {}
    __device__ __forceinline__ float2 vec(int j, int) const { return f[j]; } // (one f for all i: one copy of what does not depend on x)
};

} // namespace

} // namespace nus
