// nus_flow_project_device.hpp -- one round of the flow projection (nus_interp_set_flow_project / nus_flow_set_project of
// include/nuscaler_hip.h; BUILD-DEFINED, the reference has nothing like it), device code shared by the projecting warp kernels and
// by k_flow_project (nus_k_warp_project.hip): the same expressions in both, so the same values.
//
// The estimator's flow f lives on frame A's grid.  The content that is at output pixel p at time t came from the A-pixel q with
// q + t f(q) = p, and its vector is f(q), not f(p).  A round replaces the vector g a pixel holds by the bilinear sample of f at
// p - t g, clamped into the frame:
//     qx = clamp(x - t g.x, 0, w - 1), qy likewise (one product, one subtraction);  x0 = floor(qx), x1 = min(x0 + 1, w - 1),
//     fx = qx - x0;  top = f[y0][x0] (1 - fx) + f[y0][x1] fx, bot the same in row y1;  g = top (1 - fy) + bot fy
// per component, every product and sum rounded separately in BOTH warp modes (the unit is compiled with -ffp-contract=off and
// nothing here asks for a fused operation): the warp's FMA mode changes the two frame samples that follow, not the vector.
#pragma once

#include "nus_device.hpp"

#include <hip/hip_fp16.h>

namespace nus {

namespace {

__device__ __forceinline__ float2 half2_bits_to_float2(uint32_t bits)
{
    const __half2 hf = *reinterpret_cast<const __half2 *>(&bits);
    return make_float2(__low2float(hf), __high2float(hf));
}

__device__ __forceinline__ float2 project_lerp(float2 f00, float2 f01, float2 f10, float2 f11, float fx, float nfx, float fy, float nfy)
{
    const float tx = f00.x * nfx + f01.x * fx, ty = f00.y * nfx + f01.y * fx;
    const float bx = f10.x * nfx + f11.x * fx, by = f10.y * nfx + f11.y * fx;
    return make_float2(tx * nfy + bx * fy, ty * nfy + by * fy);
}

// Flows of at least 2 x 2 cells whose plane is below 4 GiB, seen through a buffer resource bound to the pair's own plane (a wrong
// coordinate reads zeros, never a neighbouring pair).  The corner form of sample_corner (nus_warp_device.hpp): the texel pair
// starts at xb = min(x0, w - 2), the row pair at yb = min(y0, h - 2), the fractions are taken against that corner -- the rule's
// away from the border; at the right / bottom border, where the rule has x0 = x1 = w - 1 and fraction 0, they are exactly 1 and
// select the same texel: f(w-2) * 0 + f(w-1) * 1 = f(w-1) as a value for every finite flow.  Two loads per round (the two cells of a
// row are 16 / 8 consecutive bytes, the next row through the instruction's scalar offset), all four cells always inside the plane.
// wmax / hmax / tv: per-lane copies of wave-uniform constants.
// A round is written in two halves so that a thread with several pixels can issue the gathers of all of them before it waits for
// the first (project_gather_corner for every pixel, then project_finish_corner for every pixel).
template <bool HALF>
struct ProjectGather {
    typedef uint32_t raw_t __attribute__((ext_vector_type(HALF ? 2 : 4)));
    raw_t r0, r1; // the cell pair of row yb and of row yb + 1
    float fx, fy;
};

template <bool HALF>
__device__ __forceinline__ ProjectGather<HALF> project_gather_corner(__amdgpu_buffer_rsrc_t rf, uint32_t w, float wmax, float hmax,
                                                                     uint32_t xbmax, uint32_t ybmax, float xfl, float yfl, float2 g, float tv)
{
    const float qx = __builtin_amdgcn_fmed3f(xfl - tv * g.x, 0.0f, wmax);
    const float qy = __builtin_amdgcn_fmed3f(yfl - tv * g.y, 0.0f, hmax);
    const uint32_t xb = umin((uint32_t)qx, xbmax), yb = umin((uint32_t)qy, ybmax); // truncation = floor, q >= 0
    const uint32_t cell = __umul24(yb, w) + xb; // (w, h < 2^24 and the plane below 4 GiB: host-checked)
    ProjectGather<HALF> G;
    G.fx = qx - (float)xb, G.fy = qy - (float)yb;
    if constexpr (HALF) {
        G.r0 = __builtin_amdgcn_raw_buffer_load_b64(rf, cell * 4u, 0, 0);
        G.r1 = __builtin_amdgcn_raw_buffer_load_b64(rf, cell * 4u, w * 4u, 0);
    } else {
        G.r0 = __builtin_amdgcn_raw_buffer_load_b128(rf, cell * 8u, 0, 0);
        G.r1 = __builtin_amdgcn_raw_buffer_load_b128(rf, cell * 8u, w * 8u, 0);
    }
    return G;
}

template <bool HALF>
__device__ __forceinline__ float2 project_finish_corner(const ProjectGather<HALF> &G)
{
    const float nfx = 1.0f - G.fx, nfy = 1.0f - G.fy;
    float2 f00, f01, f10, f11;
    if constexpr (HALF) {
        f00 = half2_bits_to_float2(G.r0.x), f01 = half2_bits_to_float2(G.r0.y);
        f10 = half2_bits_to_float2(G.r1.x), f11 = half2_bits_to_float2(G.r1.y);
    } else {
        f00 = make_float2(__uint_as_float(G.r0.x), __uint_as_float(G.r0.y)), f01 = make_float2(__uint_as_float(G.r0.z), __uint_as_float(G.r0.w));
        f10 = make_float2(__uint_as_float(G.r1.x), __uint_as_float(G.r1.y)), f11 = make_float2(__uint_as_float(G.r1.z), __uint_as_float(G.r1.w));
    }
    return project_lerp(f00, f01, f10, f11, G.fx, nfx, G.fy, nfy);
}

template <bool HALF>
__device__ __forceinline__ float2 project_round_corner(__amdgpu_buffer_rsrc_t rf, uint32_t w, float wmax, float hmax, uint32_t xbmax,
                                                       uint32_t ybmax, float xfl, float yfl, float2 g, float tv)
{
    return project_finish_corner<HALF>(project_gather_corner<HALF>(rf, w, wmax, hmax, xbmax, ybmax, xfl, yfl, g, tv));
}

// The rule as written, 64-bit addressing and border selects: flows narrower or lower than 2 cells, or planes of 4 GiB and more.
// `flow` is the pair's own plane; every coordinate is clamped into it before it is used.
__device__ __forceinline__ float2 project_round_plain(const void *__restrict__ flow, bool half, uint32_t w, uint32_t h, float xfl, float yfl,
                                                      float2 g, float t)
{
    const float qx = fminf(fmaxf(xfl - t * g.x, 0.0f), (float)(w - 1));
    const float qy = fminf(fmaxf(yfl - t * g.y, 0.0f), (float)(h - 1));
    const float xf0 = floorf(qx), yf0 = floorf(qy);
    const uint32_t x0 = umin((uint32_t)xf0, w - 1), y0 = umin((uint32_t)yf0, h - 1); // (umin: a NaN flow, out of contract, stays inside)
    const uint32_t x1 = umin(x0 + 1, w - 1), y1 = umin(y0 + 1, h - 1);
    const float fx = qx - xf0, fy = qy - yf0;
    const float nfx = 1.0f - fx, nfy = 1.0f - fy;
    const size_t r0 = (size_t)y0 * w, r1 = (size_t)y1 * w;
    float2 f00, f01, f10, f11;
    if (half) {
        const uint32_t *p = static_cast<const uint32_t *>(flow);
        f00 = half2_bits_to_float2(p[r0 + x0]), f01 = half2_bits_to_float2(p[r0 + x1]);
        f10 = half2_bits_to_float2(p[r1 + x0]), f11 = half2_bits_to_float2(p[r1 + x1]);
    } else {
        const float2 *p = static_cast<const float2 *>(flow);
        f00 = p[r0 + x0], f01 = p[r0 + x1], f10 = p[r1 + x0], f11 = p[r1 + x1];
    }
    return project_lerp(f00, f01, f10, f11, fx, nfx, fy, nfy);
}

} // namespace

} // namespace nus
