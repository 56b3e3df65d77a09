// nus_k_warp_project.hip -- the dense-flow warp + blend with the flow evaluated at the in-between time ("projection rounds",
// WarpLaunch::project; nus_interp_set_flow_project / nus_flow_set_project of include/nuscaler_hip.h) and the projection on its own
// (k_flow_project, nus_flow_project).  BUILD-DEFINED: the reference has nothing like it.
//
// k_warp_blend_flow (nus_k_interp.hip) reads the flow at the OUTPUT pixel p.  The flow lives on frame A's grid, so within t |f|
// pixels of a motion boundary that is the wrong vector.  Here each pixel first runs N rounds of g <- bilinear f at (p - t g)
// (nus_flow_project_device.hpp), then the unchanged warp_blend_pixel with g in place of f(p).
//
// The layout is warp_blend_tile's (nus_warp_device.hpp), shared with k_warp_blend_flow and k_bm_warp: a thread owns XV consecutive
// pixels in each of RV rows and its own flow vectors are loaded first.  What this unit adds is the tile's per-time step: the N
// rounds run round by round over all the thread's pixels, so the gathers of a round -- two loads per pixel, independent chains --
// are in flight together; then the tile's warp_blend_pixel and stores.  A round's gather depends on the round before it, so N
// rounds are N exposed gather latencies per time which only the occupancy hides: the price of the mode.
// The flow plane is reached through a buffer resource bound to the pair's own plane, like the frames.
#include "nus_device.hpp"
#include "nus_warp_sources.hpp"

namespace nus {

namespace {

template <int MODE, bool HALF, int XV, int RV, bool MT>
__global__ __launch_bounds__(256) void k_warp_blend_flow_proj(
    const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, const void *__restrict__ flow,
    uint8_t *__restrict__ out, size_t a_stride, size_t b_stride, size_t out_pair_stride, uint32_t w, uint32_t h, TimeSet ts,
    uint32_t sel, uint32_t rounds)
{
    ProjectedFlowSource<HALF, XV, RV> src; // (a buffer resource has no initializer: the members are set by name and by load)
    src.flow = flow, src.rounds = rounds;
    warp_blend_tile<MODE, XV, RV, MT>(a, b, out, a_stride, b_stride, out_pair_stride, w, h, ts, sel, src);
}

// Frames narrower or lower than 2 pixels, or frames / flow planes of 4 GiB and more: one pixel per thread, 64-bit addressing
// (EXACT arithmetic), as k_warp_blend_flow_tiny.
template <bool MT>
__global__ __launch_bounds__(256) void k_warp_blend_flow_proj_tiny(
    const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, const void *__restrict__ flow, bool half,
    uint8_t *__restrict__ out, size_t a_stride, size_t b_stride, size_t out_pair_stride, uint32_t w, uint32_t h, TimeSet ts,
    uint32_t sel, uint32_t rounds)
{
    const uint32_t y = blockIdx.y * 4 + threadIdx.y, x = blockIdx.x * kWave + threadIdx.x;
    if (y >= h || x >= w) return;
    const size_t npx = (size_t)w * h, pix = (size_t)y * w + x;
    const uint32_t *fa = reinterpret_cast<const uint32_t *>(a + (size_t)blockIdx.z * a_stride);
    const uint32_t *fb = reinterpret_cast<const uint32_t *>(b + (size_t)blockIdx.z * b_stride);
    const void *const plane = static_cast<const uint8_t *>(flow) + (size_t)blockIdx.z * npx * (half ? 4 : 8); // the pair's own
    const float2 f = half ? half2_bits_to_float2(static_cast<const uint32_t *>(plane)[pix]) : static_cast<const float2 *>(plane)[pix];
    const uint32_t nk = MT ? ts.n : 1;
    for (uint32_t k = 0; k < nk; ++k) {
        const float t = ts.t[k];
        float2 g = f;
        for (uint32_t r = 0; r < rounds; ++r) g = project_round_plain(plane, half, w, h, (float)x, (float)y, g, t);
        const uint32_t o = warp_blend_pixel_plain(fa, fb, w, h, x, y, g, t, 1.0f - t);
        reinterpret_cast<uint32_t *>(out + (size_t)blockIdx.z * out_pair_stride + (size_t)k * npx * 4)[pix] = swz(o, sel);
    }
}

// The projection on its own: g after `rounds` rounds at time t, one cell per thread, f32 flows, flows on the grid's z axis.
// CORNER: the buffer-resource form of the warp kernel; otherwise the plain form of the tiny-frame kernel.
template <bool CORNER>
__global__ __launch_bounds__(256) void k_flow_project(const float2 *__restrict__ in_all, float2 *__restrict__ out_all, uint32_t w, uint32_t h,
                                                      float t, uint32_t rounds)
{
    const uint32_t y = __builtin_amdgcn_readfirstlane(blockIdx.y * 4 + threadIdx.y), x = blockIdx.x * kWave + threadIdx.x;
    if (y >= h || x >= w) return;
    const size_t npx = (size_t)w * h, pix = (size_t)y * w + x;
    const float2 *const in = in_all + (size_t)blockIdx.z * npx;
    float2 g = in[pix];
    if (CORNER) {
        const __amdgpu_buffer_rsrc_t rf =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<float2 *>(in), 0, (uint32_t)(npx * 8), 0x00020000);
        float wmax = (float)(w - 1), hmax = (float)(h - 1), tv = t;
        asm volatile("" : "+v"(wmax), "+v"(hmax), "+v"(tv));
#pragma unroll 1
        for (uint32_t r = 0; r < rounds; ++r) g = project_round_corner<false>(rf, w, wmax, hmax, w - 2, h - 2, (float)x, (float)y, g, tv);
    } else {
        for (uint32_t r = 0; r < rounds; ++r) g = project_round_plain(in, false, w, h, (float)x, (float)y, g, t);
    }
    out_all[(size_t)blockIdx.z * npx + pix] = g;
}

} // namespace

hipError_t launch_flow_project(const FlowProjectLaunch &L)
{
    if (L.rounds > kFlowMaxProject || L.in == nullptr || L.out == nullptr || L.in == L.out || !(L.t == L.t)) return hipErrorInvalidValue;
    const auto kernel = warp_corner_ok(L.img.w, L.img.h, 8) ? k_flow_project<true> : k_flow_project<false>;
    hipLaunchKernelGGL(kernel, warp_grid(L.img.w, L.img.h, 1, 1, L.img.n), dim3(kWave, 4), 0, L.img.stream, reinterpret_cast<const float2 *>(L.in),
                       reinterpret_cast<float2 *>(L.out), L.img.w, L.img.h, L.t, L.rounds);
    return hipGetLastError();
}

// launch_warp_blend's branch for project > 0 with a flow: the same time set, pair split and output layout.
hipError_t launch_warp_blend_project(const WarpLaunch &L)
{
    if (L.flow == nullptr || L.project == 0 || L.project > kFlowMaxProject) return hipErrorInvalidValue;
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
        const void *fl = reinterpret_cast<const uint8_t *>(L.flow) + (size_t)done * npx * cell_bytes;
        const dim3 block(kWave, 4);
        if (!warp_corner_ok(L.w, L.h, cell_bytes)) {
            hipLaunchKernelGGL(mt ? k_warp_blend_flow_proj_tiny<true> : k_warp_blend_flow_proj_tiny<false>, warp_grid(L.w, L.h, 1, 1, n), block,
                               0, L.stream, a, b, fl, L.flow_half, out, L.a_stride, L.b_stride, out_stride, L.w, L.h, ts, L.in_sel, L.project);
            return;
        }
        // a pair of pixels per thread where the frame's width is even and the pair's 8-byte store is aligned
        const bool xv_ok = (L.w % 2) == 0 && (reinterpret_cast<uintptr_t>(out) % 8) == 0 && (out_stride % 8) == 0;
#define NUS_WP(M, H, X) {k_warp_blend_flow_proj<M, H, X, kWarpRV, false>, k_warp_blend_flow_proj<M, H, X, kWarpRV, true>}
        static constexpr decltype(&k_warp_blend_flow_proj<kWarpExact, false, 1, kWarpRV, false>) kernels[2][2][2][2] = { // [fma][half][pair][mt]
            {{NUS_WP(kWarpExact, false, 1), NUS_WP(kWarpExact, false, 2)}, {NUS_WP(kWarpExact, true, 1), NUS_WP(kWarpExact, true, 2)}},
            {{NUS_WP(kWarpFma, false, 1), NUS_WP(kWarpFma, false, 2)}, {NUS_WP(kWarpFma, true, 1), NUS_WP(kWarpFma, true, 2)}}};
#undef NUS_WP
        hipLaunchKernelGGL(kernels[L.fma][L.flow_half][xv_ok][mt], warp_grid(L.w, L.h, xv_ok ? 2 : 1, kWarpRV, n), block, 0, L.stream, a, b,
                           fl, out, L.a_stride, L.b_stride, out_stride, L.w, L.h, ts, L.in_sel, L.project);
    });
}

} // namespace nus
