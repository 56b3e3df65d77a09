// nus_k_warp_select.hip -- the select warp: the dense-flow warp + blend with TWO flows per pair, the estimate A -> B and the estimate
// B -> A, each output pixel warped with the vector whose two samples agree better (WarpSelectLaunch;
// nus_interp_interpolate_select_device / nus_flow_set_bidirectional of include/nuscaler_hip.h).  BUILD-DEFINED: the reference has
// nothing like it.
//
// A Horn-Schunck flow is worst where its first frame's content has no counterpart in the second -- background about to be covered,
// content leaving the frame -- and the flow the other way round is worst somewhere else.  Per output pixel p and time t, nt = 1 - t:
//     gF = F projected N rounds at t                  (nus_flow_project_device.hpp; F lives on A's grid)
//     gR = -(R projected N rounds at nt)              (R lives on B's grid: the content at p came from the B-pixel q with q + nt R(q) = p)
//     per candidate g: sa = A at p - t g, sb = B at p + nt g, truncated   (warp_sample_pair: warp_blend_pixel's samples, in the mode)
//     e(g) = |sa0 - sb0| + |sa1 - sb1| + |sa2 - sb2|                      (warp_sample_error)
//     the backward candidate wins iff e(gR) < e(gF); the pixel is warp_blend_pack of the winner's samples
// The samples of both candidates are taken and the winner's are blended: nothing is sampled twice.
//
// The layout is warp_blend_tile's (nus_warp_device.hpp): blocks of (64, 4), a thread owns XV consecutive pixels in each of RV rows,
// its own vectors of both flows are loaded first, the wave-uniform constants live in per-lane copies.  A projection round gathers
// for both flows and all the thread's pixels before the first lerp, so 2 XV RV independent chains are in flight together and N
// rounds cost N exposed gather latencies, as in k_warp_blend_flow_proj, not 2 N.  Frames and both flow planes are reached through
// buffer resources bound to the pair's own planes.  The tile body itself, warp_select_tile_at, is in nus_warp_select_device.hpp: the
// rate conversion (k_retime_flow_sel, nus_k_retime.hip) instantiates it with the schedule as its time source.
#include "nus_device.hpp"
#include "nus_warp_select_device.hpp"
#include "nus_warp_sources.hpp"

namespace nus {

namespace {

template <int MODE, bool HALF, int XV, int RV, bool MT>
__global__ __launch_bounds__(256) void k_warp_blend_flow_sel(
    const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, const void *__restrict__ flow_fwd, const void *__restrict__ flow_bwd,
    uint8_t *__restrict__ out, size_t a_stride, size_t b_stride, size_t out_pair_stride, uint32_t w, uint32_t h, TimeSet ts, uint32_t sel,
    uint32_t rounds)
{
    warp_select_tile_at<MODE, HALF, XV, RV>(a, b, flow_fwd, flow_bwd, a_stride, b_stride, w, h, sel, rounds,
                                            PairTimes<MT>{ts, out, out_pair_stride, nullptr});
}

// Frames narrower or lower than 2 pixels, or frames / flow planes of 4 GiB and more: one pixel per thread, 64-bit addressing,
// border selects (EXACT arithmetic), as k_warp_blend_flow_proj_tiny.
template <bool MT>
__global__ __launch_bounds__(256) void k_warp_blend_flow_sel_tiny(
    const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, const void *__restrict__ flow_fwd, const void *__restrict__ flow_bwd, bool half,
    uint8_t *__restrict__ out, size_t a_stride, size_t b_stride, size_t out_pair_stride, uint32_t w, uint32_t h, TimeSet ts, uint32_t sel,
    uint32_t rounds)
{
    const uint32_t y = blockIdx.y * 4 + threadIdx.y, x = blockIdx.x * kWave + threadIdx.x;
    if (y >= h || x >= w) return;
    const size_t npx = (size_t)w * h, pix = (size_t)y * w + x;
    const uint32_t *fa = reinterpret_cast<const uint32_t *>(a + (size_t)blockIdx.z * a_stride);
    const uint32_t *fb = reinterpret_cast<const uint32_t *>(b + (size_t)blockIdx.z * b_stride);
    const size_t plane_bytes = npx * (half ? 4 : 8); // the pair's own planes
    const void *const pf = static_cast<const uint8_t *>(flow_fwd) + (size_t)blockIdx.z * plane_bytes;
    const void *const pr = static_cast<const uint8_t *>(flow_bwd) + (size_t)blockIdx.z * plane_bytes;
    const float2 f = half ? half2_bits_to_float2(static_cast<const uint32_t *>(pf)[pix]) : static_cast<const float2 *>(pf)[pix];
    const float2 rv = half ? half2_bits_to_float2(static_cast<const uint32_t *>(pr)[pix]) : static_cast<const float2 *>(pr)[pix];
    const uint32_t nk = MT ? ts.n : 1;
    for (uint32_t k = 0; k < nk; ++k) {
        const float t = ts.t[k], nt = 1.0f - t;
        float2 gf = f, gb = rv;
        for (uint32_t r = 0; r < rounds; ++r) {
            gf = project_round_plain(pf, half, w, h, (float)x, (float)y, gf, t);
            gb = project_round_plain(pr, half, w, h, (float)x, (float)y, gb, nt);
        }
        float4 saf, sbf, sar, sbr;
        warp_sample_pair_plain(fa, fb, w, h, x, y, gf, t, nt, saf, sbf);
        warp_sample_pair_plain(fa, fb, w, h, x, y, make_float2(-gb.x, -gb.y), t, nt, sar, sbr);
        const bool back = warp_sample_error(sar, sbr) < warp_sample_error(saf, sbf);
        const uint32_t o = back ? warp_blend_pack(sar, sbr, t, nt) : warp_blend_pack(saf, sbf, t, nt);
        reinterpret_cast<uint32_t *>(out + (size_t)blockIdx.z * out_pair_stride + (size_t)k * npx * 4)[pix] = swz(o, sel);
    }
}

} // namespace

hipError_t launch_warp_blend_select(const WarpSelectLaunch &S)
{
    const WarpLaunch &L = S.warp;
    if (L.flow == nullptr || S.flow_bwd == nullptr || L.project > kFlowMaxProject) return hipErrorInvalidValue;
    const size_t npx = (size_t)L.w * L.h;
    TimeSet ts;
    if (!warp_time_set(L.t, L.times, L.n_times, ts)) return hipErrorInvalidValue;
    const bool mt = ts.n > 1;
    const size_t out_stride = warp_out_stride(L.out_pair_stride, ts, npx);
    const uint32_t cell_bytes = L.flow_half ? 4 : 8;
    return for_grid_z_chunks(L.n_pairs, [&](uint32_t done, uint32_t n) {
        const uint8_t *a = L.a + (size_t)done * L.a_stride;
        const uint8_t *b = L.b + (size_t)done * L.b_stride;
        uint8_t *out = L.out + (size_t)done * out_stride;
        const void *ff = reinterpret_cast<const uint8_t *>(L.flow) + (size_t)done * npx * cell_bytes;
        const void *fr = reinterpret_cast<const uint8_t *>(S.flow_bwd) + (size_t)done * npx * cell_bytes;
        const dim3 block(kWave, 4);
        if (!warp_corner_ok(L.w, L.h, cell_bytes)) {
            hipLaunchKernelGGL(mt ? k_warp_blend_flow_sel_tiny<true> : k_warp_blend_flow_sel_tiny<false>, warp_grid(L.w, L.h, 1, 1, n), block, 0,
                               L.stream, a, b, ff, fr, L.flow_half, out, L.a_stride, L.b_stride, out_stride, L.w, L.h, ts, L.in_sel, L.project);
            return;
        }
        // a pair of pixels per thread where the frame's width is even and the pair's 8-byte store is aligned
        const bool xv_ok = (L.w % 2) == 0 && (reinterpret_cast<uintptr_t>(out) % 8) == 0 && (out_stride % 8) == 0;
#define NUS_WS(M, H, X) {k_warp_blend_flow_sel<M, H, X, kSelRV[X - 1], false>, k_warp_blend_flow_sel<M, H, X, kSelRV[X - 1], true>}
        static constexpr decltype(&k_warp_blend_flow_sel<kWarpExact, false, 1, kSelRV[0], false>) kernels[2][2][2][2] = { // [fma][half][pair][mt]
            {{NUS_WS(kWarpExact, false, 1), NUS_WS(kWarpExact, false, 2)}, {NUS_WS(kWarpExact, true, 1), NUS_WS(kWarpExact, true, 2)}},
            {{NUS_WS(kWarpFma, false, 1), NUS_WS(kWarpFma, false, 2)}, {NUS_WS(kWarpFma, true, 1), NUS_WS(kWarpFma, true, 2)}}};
#undef NUS_WS
        hipLaunchKernelGGL(kernels[L.fma][L.flow_half][xv_ok][mt], warp_grid(L.w, L.h, xv_ok ? 2 : 1, kSelRV[xv_ok], n), block, 0, L.stream, a, b, ff,
                           fr, out, L.a_stride, L.b_stride, out_stride, L.w, L.h, ts, L.in_sel, L.project);
    });
}

} // namespace nus
