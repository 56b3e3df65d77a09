// nus_k_bm_warp.hip -- two-frame warp + blend straight from per-block motion vectors (nus_bm_warp_device in
// include/nuscaler_hip.h): what k_bm_flow (nus_k_blockmatch.hip) followed by k_warp_blend_flow (nus_k_interp.hip) writes, without
// the dense flow field in between.
//
//   k_bm_warp<MODE, XV, RV, MT>  warp_blend_tile (nus_warp_device.hpp) -- the layout and the per-pixel arithmetic of the dense
//                    kernel, the same code -- fed from the block vectors, so both modes write the dense route's bytes
//                    (tests/test_gpu_bm_warp.py holds them to it).  What the block structure changes:
//                     * the thread's XV pixels start at a multiple of XV and the block size is a multiple of XV, so they lie in ONE
//                       block: one 4-byte vector load per row of the thread (from blocks_x * blocks_y * 4 bytes per pair, which
//                       stay in the cache) instead of 4-8 bytes of flow per pixel from HBM, and no flow field written before;
//                     * with one vector for the XV pixels, everything that depends on (v, t, y) alone is the same expression for
//                       all of them and the compiler computes it once per thread row and time: the products t v and (1 - t) v,
//                       both samples' row -- clamp, corner row, vertical fraction and its complement, the row's byte offset -- 2
//                       of the 4 coordinates of every sample.  Nothing is rounded differently for that: the expressions are
//                       warp_blend_pixel's, evaluated once instead of XV times.
//                    XV = 2 (w even, 8-byte stores), else 1.  Four pixels per thread (16-byte stores) was measured and is
//                    slower than the dense kernel, as the same layout was there: a wave's gathers spread over twice the cache
//                    lines.  DESIGN 8.5 has the numbers.  No input channel selector: the block-matching path takes RGBA frames.
//   k_bm_warp_tiny<MT>  frames narrower or lower than 2 pixels, or of 4 GiB and more: one pixel per thread, 64-bit addressing,
//                    EXACT arithmetic (warp_blend_pixel_plain, as k_warp_blend_flow_tiny).
// No float flow field, no atomics, no LDS, no scratch.  Vectors beyond +-kBmMaxRadius are the caller's breach of contract, not a
// memory fault: every sample position is clamped to the frame before it is used.
#include "nus_device.hpp"
#include "nus_warp_sources.hpp"

namespace nus {

namespace {

template <int MODE, int XV, int RV, bool MT>
__global__ __launch_bounds__(256) void k_bm_warp(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b,
                                                 const short2 *__restrict__ vectors, uint8_t *__restrict__ out, size_t a_stride,
                                                 size_t b_stride, size_t out_pair_stride, uint32_t w, uint32_t h, uint32_t bs_log2,
                                                 uint32_t blocks_x, uint32_t blocks_y, TimeSet ts)
{
    warp_blend_tile<MODE, XV, RV, MT>(a, b, out, a_stride, b_stride, out_pair_stride, w, h, ts, kSelRGBA,
                                      BlockVectorSource<RV>{vectors, bs_log2, blocks_x, blocks_y, {}});
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
        reinterpret_cast<uint32_t *>(out + (size_t)blockIdx.z * out_pair_stride + (size_t)k * npx * 4)[pix] =
            warp_blend_pixel_plain(fa, fb, w, h, x, y, f, t, 1.0f - t);
    }
}

} // namespace

hipError_t launch_bm_warp(const BmWarpLaunch &L)
{
    TimeSet ts;
    if (L.n_times == 0 || !warp_time_set(0.0f, L.times, L.n_times, ts)) return hipErrorInvalidValue;
    const size_t npx = (size_t)L.w * L.h;
    const bool mt = ts.n > 1;
    const size_t out_stride = warp_out_stride(L.out_pair_stride, ts, npx);
    uint32_t lg = 3;
    while ((1u << lg) < L.bs) ++lg;
    const uint32_t blocks_x = cdiv(L.w, L.bs), blocks_y = cdiv(L.h, L.bs);
    return for_grid_z_chunks(L.n_pairs, [&](uint32_t done, uint32_t n) {
        const uint8_t *a = L.a + (size_t)done * L.a_stride;
        const uint8_t *b = L.b + (size_t)done * L.b_stride;
        uint8_t *out = L.out + (size_t)done * out_stride;
        const short2 *vec = reinterpret_cast<const short2 *>(L.vectors) + (size_t)done * blocks_x * blocks_y;
        const dim3 block(kWave, 4);
        if (!warp_corner_ok(L.w, L.h, 0)) {
            hipLaunchKernelGGL(mt ? k_bm_warp_tiny<true> : k_bm_warp_tiny<false>, warp_grid(L.w, L.h, 1, 1, n), block, 0, L.stream, a, b, vec,
                               out, L.a_stride, L.b_stride, out_stride, L.w, L.h, lg, blocks_x, blocks_y, ts);
            return;
        }
        // the thread's XV output pixels are one store: their alignment in every frame of every pair
        const auto fits = [&](uint32_t xv) {
            return (L.w % xv) == 0 && (reinterpret_cast<uintptr_t>(out) % (4 * xv)) == 0 && (out_stride % (4 * xv)) == 0;
        };
        const uint32_t xv = fits(2) ? 2 : 1;
#define NUS_BW(M, X) {k_bm_warp<M, X, kWarpRV, false>, k_bm_warp<M, X, kWarpRV, true>}
        static constexpr decltype(&k_bm_warp<kWarpExact, 1, kWarpRV, false>) kernels[2][2][2] = { // [fma][pair][mt]
            {NUS_BW(kWarpExact, 1), NUS_BW(kWarpExact, 2)}, {NUS_BW(kWarpFma, 1), NUS_BW(kWarpFma, 2)}};
#undef NUS_BW
        hipLaunchKernelGGL(kernels[L.fma][xv == 2][mt], warp_grid(L.w, L.h, xv, kWarpRV, n), block, 0, L.stream, a, b, vec, out, L.a_stride,
                           L.b_stride, out_stride, L.w, L.h, lg, blocks_x, blocks_y, ts);
    });
}

} // namespace nus
