// nus_warp_select_device.hpp -- the tile body of the select warp (nus_k_warp_select.hip has the method and the layout): in a header
// because the rate-conversion kernel k_retime_flow_sel (nus_k_retime.hip) instantiates it with the schedule as its time source --
// the same code, the same bytes, as nus_warp_sources.hpp does for warp_blend_tile.
#pragma once

#include "nus_device.hpp"
#include "nus_warp_sources.hpp"

namespace nus {

namespace {

// Rows per thread.  Two candidates double the live sample registers of the dense tile, so the choice is this unit's own: a thread
// owns two pixels either way, 2 x 1 on even widths and 1 x 2 on odd ones (DESIGN section 8.1 has the compiler's register counts:
// 2 x 2 needs 76 .. 96 VGPRs, five waves per SIMD; these need 41 .. 73, six to eight).  NUS_SEL_RV_PAIR = 2 builds 2 x 2 (A/B knob).
#ifndef NUS_SEL_RV_PAIR
#define NUS_SEL_RV_PAIR 1
#endif
constexpr int kSelRV[2] = {2, NUS_SEL_RV_PAIR}; // [pair]

template <int MODE, bool HALF, int XV, int RV, typename TIMES>
__device__ __forceinline__ void warp_select_tile_at(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, const void *__restrict__ flow_fwd,
                                                    const void *__restrict__ flow_bwd, size_t a_stride, size_t b_stride, uint32_t w, uint32_t h,
                                                    uint32_t sel, uint32_t rounds, TIMES times)
{
    static_assert(XV == 1 || XV == 2, "one pixel, or a pair of an even-width frame");
    const uint32_t ybase = __builtin_amdgcn_readfirstlane(blockIdx.y * (4 * RV) + threadIdx.y);
    const uint32_t x0 = (blockIdx.x * kWave + threadIdx.x) * XV;
    if (ybase >= h || x0 >= w) return;
    const size_t npx = (size_t)w * h;
    const uint32_t frame_bytes = (uint32_t)(npx * 4), row_bytes = w * 4;
    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint8_t *>(a + (size_t)blockIdx.z * a_stride), 0, frame_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint8_t *>(b + (size_t)blockIdx.z * b_stride), 0, frame_bytes, 0x00020000);
    // per-lane copies of the wave-uniform constants: scalar operands halve the VALU issue rate on gfx950
    float wmax = (float)(w - 1), hmax = (float)(h - 1);
    asm volatile("" : "+v"(wmax), "+v"(hmax));
    times.begin();
    ProjectedFlowSource<HALF, XV, RV> F, R; // (their load and their vectors; the rounds run below, for both flows together)
    F.flow = flow_fwd, R.flow = flow_bwd;
    F.load(ybase, x0, w, h, npx);
    R.load(ybase, x0, w, h, npx);
    const uint32_t nk = times.count();
    for (uint32_t k = 0; k < nk; ++k) {
        float tv = times.time(k);
        asm volatile("" : "+v"(tv));
        const float nt = 1.0f - tv;
        uint32_t *const frame_out = times.frame(k, npx);
#pragma unroll
        for (int j = 0; j < RV; ++j)
#pragma unroll
            for (int i = 0; i < XV; ++i) F.g[j][i] = F.f[j][i], R.g[j][i] = R.f[j][i];
#pragma unroll 1
        for (uint32_t r = 0; r < rounds; ++r) { // F at time t, R at time nt: the gathers of both and of all pixels, then their lerps
            ProjectGather<HALF> GF[RV][XV], GR[RV][XV];
#pragma unroll
            for (int j = 0; j < RV; ++j) {
                const float yfl = (float)umin(ybase + 4 * j, h - 1); // (rows past the frame repeat the last row's)
#pragma unroll
                for (int i = 0; i < XV; ++i) {
                    GF[j][i] = project_gather_corner<HALF>(F.rf, w, wmax, hmax, w - 2, h - 2, (float)(x0 + i), yfl, F.g[j][i], tv);
                    GR[j][i] = project_gather_corner<HALF>(R.rf, w, wmax, hmax, w - 2, h - 2, (float)(x0 + i), yfl, R.g[j][i], nt);
                }
            }
#pragma unroll
            for (int j = 0; j < RV; ++j)
#pragma unroll
                for (int i = 0; i < XV; ++i) F.g[j][i] = project_finish_corner<HALF>(GF[j][i]), R.g[j][i] = project_finish_corner<HALF>(GR[j][i]);
        }
#pragma unroll
        for (int j = 0; j < RV; ++j) {
            const uint32_t y = ybase + 4 * j;
            if (y >= h) break; // wave-uniform
            const float yfl = (float)y;
            uint32_t o[XV];
#pragma unroll
            for (int i = 0; i < XV; ++i) {
                const float2 gf = F.g[j][i], gr = make_float2(-R.g[j][i].x, -R.g[j][i].y);
                float4 saf, sbf, sar, sbr;
                warp_sample_pair<MODE>(ra, rb, row_bytes, wmax, hmax, w - 2, h - 2, (float)(x0 + i), yfl, gf, tv, nt, saf, sbf);
                warp_sample_pair<MODE>(ra, rb, row_bytes, wmax, hmax, w - 2, h - 2, (float)(x0 + i), yfl, gr, tv, nt, sar, sbr);
                const bool back = warp_sample_error(sar, sbr) < warp_sample_error(saf, sbf); // a tie goes forward
                const float4 sa = make_float4(back ? sar.x : saf.x, back ? sar.y : saf.y, back ? sar.z : saf.z, back ? sar.w : saf.w);
                const float4 sb = make_float4(back ? sbr.x : sbf.x, back ? sbr.y : sbf.y, back ? sbr.z : sbf.z, back ? sbr.w : sbf.w);
                o[i] = swz(warp_blend_pack(sa, sb, tv, nt), sel);
            }
            uint32_t *dst = frame_out + (size_t)y * w + x0;
            if (XV == 2) {
                store_out8<false>(dst, make_uint2(o[0], o[XV - 1]));
            } else {
                dst[0] = o[0];
            }
        }
    }
}

} // namespace

} // namespace nus
