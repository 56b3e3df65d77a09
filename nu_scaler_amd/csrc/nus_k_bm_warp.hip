// nus_k_bm_warp.hip -- two-frame warp + blend straight from per-block motion vectors (nus_bm_warp_device in
// include/nuscaler_hip.h): what k_bm_flow (nus_k_blockmatch.hip) followed by k_warp_blend_flow (nus_k_interp.hip) writes, without
// the dense flow field in between.
//
//   k_bm_warp<MODE, XV, RV, MT>  the dense kernel's layout -- blockDim (64, 4), a thread owns XV consecutive pixels in each of RV
//                    rows (y, y + 4, ..), frames seen through buffer resources -- and its per-pixel arithmetic, warp_blend_pixel
//                    (nus_warp_device.hpp), so both modes write the dense route's bytes.  What the block structure changes:
//                     * the thread's XV pixels start at a multiple of XV and the block size is a multiple of XV, so they lie in ONE
//                       block: one 4-byte vector load per row of the thread (from blocks_x * blocks_y * 4 bytes per pair, which
//                       stay in the cache) instead of 4-8 bytes of flow per pixel from HBM, and no flow field written before;
//                     * with one vector for the XV pixels, everything that depends on (v, t, y) alone is the same expression for
//                       all of them and is computed once per thread row and time: the products t v and (1 - t) v, both samples'
//                       row -- clamp, corner row, vertical fraction and its complement, the row's byte offset -- 2 of the 4
//                       coordinates of every sample.  Nothing is rounded differently for that: the expressions are
//                       warp_blend_pixel's, evaluated once instead of XV times.
//                    XV = 2 (w even, 8-byte stores), else 1.  Four pixels per thread (16-byte stores) was measured and is
//                    slower than the dense kernel, as the same layout was there (nus_k_interp.hip): a wave's gathers spread over
//                    twice the cache lines.  DESIGN 8.5 has the numbers.
//   k_bm_warp_tiny<MT>  frames narrower or lower than 2 pixels, or of 4 GiB and more: one pixel per thread, 64-bit addressing,
//                    EXACT arithmetic (as k_warp_blend_flow_tiny).
// No float flow field, no atomics, no LDS, no scratch.  Vectors beyond +-kBmMaxRadius are the caller's breach of contract, not a
// memory fault: every sample position is clamped to the frame before it is used.
#include "nus_device.hpp"
#include "nus_warp_device.hpp"

namespace nus {

namespace {

template <int MODE, int XV, int RV, bool MT>
__global__ __launch_bounds__(256) void k_bm_warp(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b,
                                                 const short2 *__restrict__ vectors, uint8_t *__restrict__ out, size_t a_stride,
                                                 size_t b_stride, size_t out_pair_stride, uint32_t w, uint32_t h, uint32_t bs_log2,
                                                 uint32_t blocks_x, uint32_t blocks_y, TimeSet ts)
{
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
    const short2 *const pair_vectors = vectors + (size_t)blockIdx.z * blocks_x * blocks_y;
    const uint32_t bx = x0 >> bs_log2; // x0 % XV == 0 and XV divides the block size: the thread's XV pixels share the block
    float2 f[RV];
#pragma unroll
    for (int j = 0; j < RV; ++j) { // the vectors of the thread's rows first (rows past the frame: the last row's)
        const short2 v = pair_vectors[(size_t)(umin(ybase + 4 * j, h - 1) >> bs_log2) * blocks_x + bx];
        f[j] = make_float2((float)v.x, (float)v.y);
    }
    const uint32_t nk = MT ? ts.n : 1;
    for (uint32_t k = 0; k < nk; ++k) {
        float tv = ts.t[k];
        asm volatile("" : "+v"(tv));
        const float nt = 1.0f - tv;
        uint32_t *const frame_out = reinterpret_cast<uint32_t *>(out + (size_t)blockIdx.z * out_pair_stride + (size_t)k * npx * 4);
#pragma unroll
        for (int j = 0; j < RV; ++j) {
            const uint32_t y = ybase + 4 * j;
            if (y >= h) break; // wave-uniform
            const float yfl = (float)y;
            uint32_t o[XV];
#pragma unroll
            for (int i = 0; i < XV; ++i) // (one f for all i: the compiler keeps one copy of what does not depend on x)
                o[i] = warp_blend_pixel<MODE>(ra, rb, row_bytes, wmax, hmax, w - 2, h - 2, (float)(x0 + i), yfl, f[j], tv, nt);
            uint32_t *dst = frame_out + (size_t)y * w + x0;
            if (XV == 2) {
                store_out8<false>(dst, make_uint2(o[0], o[1]));
            } else {
                dst[0] = o[0];
            }
        }
    }
}

template <bool MT>
__global__ __launch_bounds__(256) void k_bm_warp_tiny(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b,
                                                      const short2 *__restrict__ vectors, uint8_t *__restrict__ out, size_t a_stride,
                                                      size_t b_stride, size_t out_pair_stride, uint32_t w, uint32_t h,
                                                      uint32_t bs_log2, uint32_t blocks_x, uint32_t blocks_y, TimeSet ts)
{
    const uint32_t y = blockIdx.y * 4 + threadIdx.y, x = blockIdx.x * kWave + threadIdx.x;
    if (y >= h || x >= w) return;
    const size_t npx = (size_t)w * h, pix = (size_t)y * w + x;
    const uint32_t *fa = reinterpret_cast<const uint32_t *>(a + (size_t)blockIdx.z * a_stride);
    const uint32_t *fb = reinterpret_cast<const uint32_t *>(b + (size_t)blockIdx.z * b_stride);
    const short2 v = vectors[((size_t)blockIdx.z * blocks_y + (y >> bs_log2)) * blocks_x + (x >> bs_log2)];
    const float2 f = make_float2((float)v.x, (float)v.y);
    const uint32_t nk = MT ? ts.n : 1;
    for (uint32_t k = 0; k < nk; ++k) {
        const float t = ts.t[k];
        const float nt = 1.0f - t;
        const float4 sa = sample_trunc(fa, w, h, (float)x - t * f.x, (float)y - t * f.y);
        const float4 sb = sample_trunc(fb, w, h, (float)x + nt * f.x, (float)y + nt * f.y);
        uint32_t o = 0;
        o = pack_trunc_u8(nt * sa.x + t * sb.x, 0, o);
        o = pack_trunc_u8(nt * sa.y + t * sb.y, 1, o);
        o = pack_trunc_u8(nt * sa.z + t * sb.z, 2, o);
        o = pack_trunc_u8(nt * sa.w + t * sb.w, 3, o);
        reinterpret_cast<uint32_t *>(out + (size_t)blockIdx.z * out_pair_stride + (size_t)k * npx * 4)[pix] = o;
    }
}

} // namespace

hipError_t launch_bm_warp(const BmWarpLaunch &L)
{
    if (L.n_times == 0 || L.n_times > kInterpMaxTimes || L.times == nullptr) return hipErrorInvalidValue;
    const size_t npx = (size_t)L.w * L.h;
    TimeSet ts{};
    for (uint32_t k = 0; k < L.n_times; ++k) ts.t[k] = L.times[k];
    ts.n = L.n_times;
    const bool mt = ts.n > 1;
    const size_t out_stride = L.out_pair_stride ? L.out_pair_stride : ts.n * npx * 4;
    uint32_t lg = 3;
    while ((1u << lg) < L.bs) ++lg;
    const uint32_t blocks_x = cdiv(L.w, L.bs), blocks_y = cdiv(L.h, L.bs);
    for (uint32_t done = 0; done < L.n_pairs;) {
        const uint32_t n = L.n_pairs - done < kMaxGridZ ? L.n_pairs - done : kMaxGridZ;
        const uint8_t *a = L.a + (size_t)done * L.a_stride;
        const uint8_t *b = L.b + (size_t)done * L.b_stride;
        uint8_t *out = L.out + (size_t)done * out_stride;
        const short2 *vec = reinterpret_cast<const short2 *>(L.vectors) + (size_t)done * blocks_x * blocks_y;
        const bool corner = L.w >= 2 && L.h >= 2 && npx * 4 < (1ull << 32) && L.w * 4ull < (1u << 24) && L.h < (1u << 24);
        if (!corner) {
            const dim3 block(kWave, 4), grid(cdiv(L.w, 64), cdiv(L.h, 4), n);
            if (mt)
                hipLaunchKernelGGL(k_bm_warp_tiny<true>, grid, block, 0, L.stream, a, b, vec, out, L.a_stride, L.b_stride, out_stride, L.w,
                                   L.h, lg, blocks_x, blocks_y, ts);
            else
                hipLaunchKernelGGL(k_bm_warp_tiny<false>, grid, block, 0, L.stream, a, b, vec, out, L.a_stride, L.b_stride, out_stride, L.w,
                                   L.h, lg, blocks_x, blocks_y, ts);
        } else {
            constexpr int RV = 2;
            // the thread's XV output pixels are one store: their alignment in every frame of every pair
            const auto fits = [&](uint32_t xv) {
                return (L.w % xv) == 0 && (reinterpret_cast<uintptr_t>(out) % (4 * xv)) == 0 &&
                       (out_stride % (4 * xv)) == 0;
            };
            const uint32_t xv = fits(2) ? 2 : 1;
            const dim3 block(kWave, 4), grid(cdiv(L.w, 64 * xv), cdiv(L.h, 4 * RV), n);
#define NUS_BW(M, X, MT) hipLaunchKernelGGL((k_bm_warp<M, X, RV, MT>), grid, block, 0, L.stream, a, b, vec, out, L.a_stride, L.b_stride, out_stride, L.w, L.h, lg, blocks_x, blocks_y, ts)
#define NUS_BW_T(M, X) do { if (mt) NUS_BW(M, X, true); else NUS_BW(M, X, false); } while (0)
#define NUS_BW_X(M) do { if (xv == 2) NUS_BW_T(M, 2); else NUS_BW_T(M, 1); } while (0)
            if (L.fma) NUS_BW_X(kWarpFma); else NUS_BW_X(kWarpExact);
#undef NUS_BW_X
#undef NUS_BW_T
#undef NUS_BW
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        done += n;
    }
    return hipSuccess;
}

} // namespace nus
