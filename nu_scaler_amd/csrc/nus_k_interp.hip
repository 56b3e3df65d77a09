// nus_k_interp.hip -- two-frame warp + blend and the BGRA -> RGBA swizzle.
//   warp+blend nu_scaler_core/src/shaders/warp_blend.wgsl:18-47 (geometry),
//              nu_scaler_core/src/interpolation/mod.rs:386-411, :467-510 (rounding)
#include "nus_device.hpp"
#include "nus_warp_sources.hpp"

namespace nus {

namespace {

// ---------------------------------------------------------------------------------
// Warp + blend
// ---------------------------------------------------------------------------------

// Zero flow (the live reference behaviour, wgpu_interpolator.rs:275-295): sample
// positions are the pixel centres, so the bilinear samples are the pixels themselves
// and the kernel is a streaming blend, 4 pixels (16 B) per lane.

// MT: the multi-time form -- each lane loads its A and B pixels once, then blends and stores them once per time of the set (frame
// k of the pair at out + k * npx * 4).  MT = false is the single-time kernel: the set's one time, no loop.
template <bool VEC, bool MT>
__global__ __launch_bounds__(256) void k_blend_zero_flow(
    const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, uint8_t *__restrict__ out,
    size_t a_stride, size_t b_stride, size_t out_pair_stride, size_t npx, TimeSet ts, uint32_t sel)
{
    const uint32_t *pa = reinterpret_cast<const uint32_t *>(a + (size_t)blockIdx.y * a_stride);
    const uint32_t *pb = reinterpret_cast<const uint32_t *>(b + (size_t)blockIdx.y * b_stride);
    uint8_t *const pair_out = out + (size_t)blockIdx.y * out_pair_stride;
    const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * (VEC ? 4 : 1);
    if (i >= npx) return;
    const uint32_t nk = MT ? ts.n : 1;
    if (VEC) {
        const uint4 va = *reinterpret_cast<const uint4 *>(pa + i);
        const uint4 vb = *reinterpret_cast<const uint4 *>(pb + i);
        for (uint32_t k = 0; k < nk; ++k) {
            float t = ts.t[k];
            if (MT) asm volatile("" : "+v"(t)); // per-lane copy (scalar operands halve the VALU issue rate on gfx950)
            const float nt = 1.0f - t;
            uint32_t *po = reinterpret_cast<uint32_t *>(pair_out + (size_t)k * npx * 4);
            // per-channel arithmetic: swizzling the blended pixel equals blending swizzled inputs
            store_out16<false>(po + i, swz4(make_uint4(blend_px(va.x, vb.x, t, nt), blend_px(va.y, vb.y, t, nt),
                                                                 blend_px(va.z, vb.z, t, nt), blend_px(va.w, vb.w, t, nt)), sel));
        }
    } else {
        const uint32_t va = pa[i], vb = pb[i];
        for (uint32_t k = 0; k < nk; ++k) {
            float t = ts.t[k];
            if (MT) asm volatile("" : "+v"(t));
            const float nt = 1.0f - t;
            reinterpret_cast<uint32_t *>(pair_out + (size_t)k * npx * 4)[i] = swz(blend_px(va, vb, t, nt), sel);
        }
    }
}

// ---------------------------------------------------------------------------------
// Warp + blend with a dense flow field, rewritten in round 3 around the instruction count (the kernel is bound by SIMD
// issue: ~180 VALU instructions per pixel in the form above, 0.47-0.51 of the HBM roofline).
//
// One bilinear sample, frames of at least 2 x 2 pixels seen through a buffer resource (32-bit offsets):
//  * the texel pair starts at xb = min(x0, w - 2) and the row pair at yb = min(y0, h - 2), so all four texels are always
//    inside the frame -- two 8-byte loads, the second one row_bytes further through the instruction's scalar offset, no
//    border selects -- and the fractions are taken against THAT corner: xf = x - xb, yf = y - yb.  Away from the border
//    these are the reference's fractions (x - floor(x)); at the right / bottom border, where the reference has x0 = x1 =
//    w - 1 and fraction 0 (interpolation/mod.rs:474-483), they are exactly 1 and select the same texel:
//    p(w-2) * (1 - 1) + p(w-1) * 1 = p(w-1), bit for bit in either mode;
//  * MODE_EXACT: every product and sum separately, the CPU's roundings (bit-exact against the oracle);
//    MODE_FMA  : each of the three lerps of a sample as one multiply and one fused multiply-add, fma(b, f, a (1 - f)): 24
//    instead of 36 operations per sample (and the sample positions as one FMA each), inside the +-1 LSB contract of the
//    interpolation path (measured on noise frames with random flows: < 0.1 % of the samples differ, none by more than
//    one count).  The blend of the two samples is exact in both modes (see warp_blend_pixel).
// The truncation of each sample to u8 (sample_frame returns u8: interpolation/mod.rs:506) stays in both modes.
// Dense flow (2 x f32 or 2 x f16 per pixel, delta A -> B): A sampled at p - t*flow, B at p + (1-t)*flow
// (warp_blend.wgsl:36-37 in texel space).  The layout -- threads, rows, times, stores -- is warp_blend_tile's
// (nus_warp_device.hpp), shared with the block-vector and the projecting kernels; the vectors are DenseFlowSource's
// (nus_warp_sources.hpp): the flow at the thread's own pixels.  XV = 2: the two flow vectors of a row are one 16-byte (8-byte) load (w even and the plane 16-byte aligned,
// host-checked).  HALF: the flow field is the Rg16Float texture of the reference's live path (wgpu_interpolator.rs:276), widened
// exactly.
template <int MODE, bool HALF, int XV, int RV, bool MT>
__global__ __launch_bounds__(256) void k_warp_blend_flow(
    const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, const void *__restrict__ flow,
    uint8_t *__restrict__ out, size_t a_stride, size_t b_stride, size_t out_pair_stride, uint32_t w, uint32_t h, TimeSet ts,
    uint32_t sel)
{
    warp_blend_tile<MODE, XV, RV, MT>(a, b, out, a_stride, b_stride, out_pair_stride, w, h, ts, sel, DenseFlowSource<HALF, XV, RV>{flow, {}});
}

// Frames narrower or lower than 2 pixels, or of 4 GiB and more: one pixel per thread, 64-bit addressing (EXACT arithmetic).
// MT: the flow vector is loaded once and the pixel of every time of the set stored (frame k at out + k * w * h * 4); MT = false is
// the single-time kernel: the set's one time, no loop.
template <bool MT>
__global__ __launch_bounds__(256) void k_warp_blend_flow_tiny(
    const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, const void *__restrict__ flow, bool half,
    uint8_t *__restrict__ out, size_t a_stride, size_t b_stride, size_t out_pair_stride, uint32_t w, uint32_t h, TimeSet ts,
    uint32_t sel)
{
    const uint32_t y = blockIdx.y * 4 + threadIdx.y, x = blockIdx.x * kWave + threadIdx.x;
    if (y >= h || x >= w) return;
    const size_t npx = (size_t)w * h, idx = (size_t)blockIdx.z * npx + (size_t)y * w + x, pix = (size_t)y * w + x;
    const uint32_t *fa = reinterpret_cast<const uint32_t *>(a + (size_t)blockIdx.z * a_stride);
    const uint32_t *fb = reinterpret_cast<const uint32_t *>(b + (size_t)blockIdx.z * b_stride);
    const float2 f = half ? widen(static_cast<const uint32_t *>(flow)[idx]) : static_cast<const float2 *>(flow)[idx];
    const uint32_t nk = MT ? ts.n : 1;
    for (uint32_t k = 0; k < nk; ++k) {
        const float t = ts.t[k];
        const uint32_t o = warp_blend_pixel_plain(fa, fb, w, h, x, y, f, t, 1.0f - t);
        reinterpret_cast<uint32_t *>(out + (size_t)blockIdx.z * out_pair_stride + (size_t)k * npx * 4)[pix] = swz(o, sel);
    }
}

// ---------------------------------------------------------------------------------
// BGRA -> RGBA swizzle of captured frames (nu_scaler_core/src/lib.rs:251-270), 4 px per lane
// ---------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t swap_rb(uint32_t p)
{
    return __builtin_amdgcn_perm(p, p, 0x03000102u); // bytes (2, 1, 0, 3): one v_perm_b32
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_swizzle_bgra(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, size_t npx)
{
    const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * (VEC ? 4 : 1);
    if (i >= npx) return;
    if (VEC) {
        const uint4 v = *reinterpret_cast<const uint4 *>(in + i);
        store_out16<false>(out + i, make_uint4(swap_rb(v.x), swap_rb(v.y), swap_rb(v.z), swap_rb(v.w)));
    } else {
        out[i] = swap_rb(in[i]);
    }
}

} // namespace

hipError_t launch_swizzle_bgra(const uint8_t *in, uint8_t *out, size_t npx, hipStream_t stream)
{
    const bool vec = (npx % 4) == 0 && (reinterpret_cast<uintptr_t>(in) % 16) == 0 && (reinterpret_cast<uintptr_t>(out) % 16) == 0;
    const size_t items = vec ? npx / 4 : npx;
    const dim3 block(256), grid((uint32_t)((items + 255) / 256));
    if (vec)
        hipLaunchKernelGGL(k_swizzle_bgra<true>, grid, block, 0, stream, reinterpret_cast<const uint32_t *>(in), reinterpret_cast<uint32_t *>(out), npx);
    else
        hipLaunchKernelGGL(k_swizzle_bgra<false>, grid, block, 0, stream, reinterpret_cast<const uint32_t *>(in), reinterpret_cast<uint32_t *>(out), npx);
    return hipGetLastError();
}

hipError_t launch_warp_blend(const WarpLaunch &L)
{
    if (L.project > 0 && L.flow != nullptr) return launch_warp_blend_project(L); // nus_k_warp_project.hip; off: everything below, as before
    const size_t npx = (size_t)L.w * L.h;
    TimeSet ts;
    if (!warp_time_set(L.t, L.times, L.n_times, ts)) return hipErrorInvalidValue;
    const bool mt = ts.n > 1;
    const size_t out_stride = warp_out_stride(L.out_pair_stride, ts, npx);
    return for_grid_z_chunks(L.n_pairs, [&](uint32_t done, uint32_t n) {
        const uint8_t *a = L.a + (size_t)done * L.a_stride;
        const uint8_t *b = L.b + (size_t)done * L.b_stride;
        uint8_t *out = L.out + (size_t)done * out_stride;
        if (L.flow == nullptr) {
            const bool vec = (npx % 4) == 0 && (L.a_stride % 16) == 0 && (L.b_stride % 16) == 0 && (out_stride % 16) == 0 &&
                             (reinterpret_cast<uintptr_t>(a) % 16) == 0 && (reinterpret_cast<uintptr_t>(b) % 16) == 0 &&
                             (reinterpret_cast<uintptr_t>(out) % 16) == 0;
            const size_t items = vec ? npx / 4 : npx;
            const dim3 block(256), grid((uint32_t)((items + 255) / 256), n);
#define NUS_ZB(V, MT) hipLaunchKernelGGL((k_blend_zero_flow<V, MT>), grid, block, 0, L.stream, a, b, out, L.a_stride, L.b_stride, out_stride, npx, ts, L.in_sel)
            if (vec) {
                if (mt) NUS_ZB(true, true); else NUS_ZB(true, false);
            } else {
                if (mt) NUS_ZB(false, true); else NUS_ZB(false, false);
            }
#undef NUS_ZB
            return;
        }
        const void *fl = reinterpret_cast<const uint8_t *>(L.flow) + (size_t)done * npx * (L.flow_half ? 4 : 8);
        const dim3 block(kWave, 4);
        if (!warp_corner_ok(L.w, L.h, 0)) { // (the flow is read through 64-bit addresses: no bound on its plane)
            hipLaunchKernelGGL(mt ? k_warp_blend_flow_tiny<true> : k_warp_blend_flow_tiny<false>, warp_grid(L.w, L.h, 1, 1, n), block, 0,
                               L.stream, a, b, fl, L.flow_half, out, L.a_stride, L.b_stride, out_stride, L.w, L.h, ts, L.in_sel);
            return;
        }
        // a pair of pixels per thread: its output pixels are one 8-byte store, its f32 flow vectors one 16-byte load
        const bool xv_ok = (L.w % 2) == 0 && (reinterpret_cast<uintptr_t>(fl) % 16) == 0 && (reinterpret_cast<uintptr_t>(out) % 8) == 0 &&
                           (out_stride % 8) == 0;
#define NUS_WB(M, H, X) {k_warp_blend_flow<M, H, X, kWarpRV, false>, k_warp_blend_flow<M, H, X, kWarpRV, true>}
        static constexpr decltype(&k_warp_blend_flow<kWarpExact, false, 1, kWarpRV, false>) kernels[2][2][2][2] = { // [fma][half][pair][mt]
            {{NUS_WB(kWarpExact, false, 1), NUS_WB(kWarpExact, false, 2)}, {NUS_WB(kWarpExact, true, 1), NUS_WB(kWarpExact, true, 2)}},
            {{NUS_WB(kWarpFma, false, 1), NUS_WB(kWarpFma, false, 2)}, {NUS_WB(kWarpFma, true, 1), NUS_WB(kWarpFma, true, 2)}}};
#undef NUS_WB
        hipLaunchKernelGGL(kernels[L.fma][L.flow_half][xv_ok][mt], warp_grid(L.w, L.h, xv_ok ? 2 : 1, kWarpRV, n), block, 0, L.stream, a, b,
                           fl, out, L.a_stride, L.b_stride, out_stride, L.w, L.h, ts, L.in_sel);
    });
}

} // namespace nus
