// nus_warp_device.hpp -- the flow-driven warp + blend, device code and launcher helpers shared by its three kernel families:
// k_warp_blend_flow (dense flow, nus_k_interp.hip), k_bm_warp (block vectors, nus_k_bm_warp.hip) and k_warp_blend_flow_proj (flow
// projected to the in-between time, nus_k_warp_project.hip).  One pixel's arithmetic (warp_blend_pixel) and the tile around it
// (warp_blend_tile) are written once; a family supplies only where a pixel's vector comes from, so all three write the same bytes
// for the same vectors.  The select warp (k_warp_blend_flow_sel, nus_k_warp_select.hip) samples with two candidate vectors per pixel
// and blends the samples of one: it takes the pixel in its two halves, warp_sample_pair and warp_blend_pack.
//   geometry nu_scaler_core/src/shaders/warp_blend.wgsl:25-43, rounding nu_scaler_core/src/interpolation/mod.rs:386-411, :467-510
#pragma once

#include "nus_device.hpp"

namespace nus {

namespace {

constexpr int kWarpExact = 0, kWarpFma = 1;

template <int MODE>
__device__ __forceinline__ float lerp_mode(float a, float b, float f, float nf)
{
    if (MODE == kWarpFma) return __builtin_fmaf(b, f, a * nf); // (the form a + f (b - a) makes the compiler subtract the packed
                                                               // bytes and convert the difference: two slow-class instructions)
    return a * nf + b * f;
}

template <int MODE>
__device__ __forceinline__ float4 sample_corner(__amdgpu_buffer_rsrc_t rs, uint32_t row_bytes, float wmax, float hmax,
                                                uint32_t xbmax, uint32_t ybmax, float x, float y)
{
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    x = __builtin_amdgcn_fmed3f(x, 0.0f, wmax); // clamp to [0, w-1] (interpolation/mod.rs:470-471)
    y = __builtin_amdgcn_fmed3f(y, 0.0f, hmax);
    const uint32_t xb = umin((uint32_t)x, xbmax), yb = umin((uint32_t)y, ybmax); // (uint32_t): truncation = floor, x >= 0
    const float xf = x - (float)xb, yf = y - (float)yb;
    const float nxf = 1.0f - xf, nyf = 1.0f - yf;
    const uint32_t off = __umul24(yb, row_bytes) + xb * 4u;
    const u32x2 r0 = __builtin_amdgcn_raw_buffer_load_b64(rs, off, 0, 0);
    const u32x2 r1 = __builtin_amdgcn_raw_buffer_load_b64(rs, off, row_bytes, 0); // next row: scalar offset, always in range
    float r[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float top = lerp_mode<MODE>(ch_f32(r0.x, c), ch_f32(r0.y, c), xf, nxf);
        const float bottom = lerp_mode<MODE>(ch_f32(r1.x, c), ch_f32(r1.y, c), xf, nxf);
        r[c] = floorf(lerp_mode<MODE>(top, bottom, yf, nyf)); // `value as u8`: 0 <= value <= 255 (+ an ulp in FMA mode)
    }
    return make_float4(r[0], r[1], r[2], r[3]);
}

// The one-pixel-per-thread kernels' sample (frames narrower or lower than 2 pixels, or of 4 GiB and more: 64-bit addressing, border
// selects).  interpolation/mod.rs:467-510: clamp, bilinear, truncate to u8 -- returned as the four truncated
// channel values still in f32 (floor of a value in [0, 255]) so the blend needs no unpack.
__device__ __forceinline__ float4 sample_trunc(const uint32_t *__restrict__ f, uint32_t w, uint32_t h, float x, float y)
{
    x = fminf(fmaxf(x, 0.0f), (float)(w - 1));
    y = fminf(fmaxf(y, 0.0f), (float)(h - 1));
    const float xfl = floorf(x), yfl = floorf(y);
    const uint32_t x0 = (uint32_t)xfl, y0 = (uint32_t)yfl;
    const uint32_t x1 = umin(x0 + 1, w - 1), y1 = umin(y0 + 1, h - 1);
    const float xf = x - xfl, yf = y - yfl;
    const float nxf = 1.0f - xf, nyf = 1.0f - yf;
    const uint32_t p00 = f[(size_t)y0 * w + x0], p01 = f[(size_t)y0 * w + x1];
    const uint32_t p10 = f[(size_t)y1 * w + x0], p11 = f[(size_t)y1 * w + x1];
    float r[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float top = ch_f32(p00, c) * nxf + ch_f32(p01, c) * xf;
        const float bottom = ch_f32(p10, c) * nxf + ch_f32(p11, c) * xf;
        const float value = top * nyf + bottom * yf;
        r[c] = fminf(floorf(value), 255.0f); // `value as u8`; value >= 0 here
    }
    return make_float4(r[0], r[1], r[2], r[3]);
}

// The pixel in its two halves, for the select warp (nus_k_warp_select.hip), which samples with two candidate vectors and blends the
// samples of one: warp_sample_pair is the two truncated samples, warp_blend_pack their blend.
template <int MODE>
__device__ __forceinline__ void warp_sample_pair(__amdgpu_buffer_rsrc_t ra, __amdgpu_buffer_rsrc_t rb, uint32_t row_bytes, float wmax,
                                                 float hmax, uint32_t xbmax, uint32_t ybmax, float xfl, float yfl, float2 f, float tv,
                                                 float nt, float4 &sa, float4 &sb)
{
    float ax, ay, bx, by;
    if (MODE == kWarpFma) {
        ax = __builtin_fmaf(-tv, f.x, xfl), ay = __builtin_fmaf(-tv, f.y, yfl);
        bx = __builtin_fmaf(nt, f.x, xfl), by = __builtin_fmaf(nt, f.y, yfl);
    } else {
        ax = xfl - tv * f.x, ay = yfl - tv * f.y;
        bx = xfl + nt * f.x, by = yfl + nt * f.y;
    }
    sa = sample_corner<MODE>(ra, row_bytes, wmax, hmax, xbmax, ybmax, ax, ay);
    sb = sample_corner<MODE>(rb, row_bytes, wmax, hmax, xbmax, ybmax, bx, by);
}

__device__ __forceinline__ uint32_t warp_blend_pack(const float4 &sa, const float4 &sb, float tv, float nt)
{
    uint32_t p = 0;
    p = pack_trunc_u8(nt * sa.x + tv * sb.x, 0, p);
    p = pack_trunc_u8(nt * sa.y + tv * sb.y, 1, p);
    p = pack_trunc_u8(nt * sa.z + tv * sb.z, 2, p);
    p = pack_trunc_u8(nt * sa.w + tv * sb.w, 3, p);
    return p;
}

// One output pixel at (xfl, yfl) with flow f (delta A -> B): A sampled at p - t f, B at p + (1 - t) f, each sample truncated to u8 as
// sample_frame returns it, then the blend of the two truncated samples with the CPU's three roundings in BOTH modes: with integer
// operands and a t like 0.3 a tenth of the exact results are integers themselves (0.7 * 10 + 0.3 * 20 = 13), and there the truncation
// turns any other rounding sequence into a count of difference (measured: 0.25 % of the samples with a fused blend).
// tv / nt / wmax / hmax: per-lane copies of wave-uniform constants (scalar operands halve the VALU issue rate on gfx950).
template <int MODE>
__device__ __forceinline__ uint32_t warp_blend_pixel(__amdgpu_buffer_rsrc_t ra, __amdgpu_buffer_rsrc_t rb, uint32_t row_bytes, float wmax,
                                                     float hmax, uint32_t xbmax, uint32_t ybmax, float xfl, float yfl, float2 f, float tv,
                                                     float nt)
{
    float4 sa, sb;
    warp_sample_pair<MODE>(ra, rb, row_bytes, wmax, hmax, xbmax, ybmax, xfl, yfl, f, tv, nt, sa, sb);
    return warp_blend_pack(sa, sb, tv, nt);
}

// The same pixel for the one-pixel-per-thread kernels (sample_trunc's frames): EXACT arithmetic, the input's channel order.
__device__ __forceinline__ void warp_sample_pair_plain(const uint32_t *__restrict__ fa, const uint32_t *__restrict__ fb, uint32_t w, uint32_t h,
                                                       uint32_t x, uint32_t y, float2 f, float t, float nt, float4 &sa, float4 &sb)
{
    sa = sample_trunc(fa, w, h, (float)x - t * f.x, (float)y - t * f.y);
    sb = sample_trunc(fb, w, h, (float)x + nt * f.x, (float)y + nt * f.y);
}

__device__ __forceinline__ uint32_t warp_blend_pixel_plain(const uint32_t *__restrict__ fa, const uint32_t *__restrict__ fb, uint32_t w,
                                                           uint32_t h, uint32_t x, uint32_t y, float2 f, float t, float nt)
{
    float4 sa, sb;
    warp_sample_pair_plain(fa, fb, w, h, x, y, f, t, nt, sa, sb);
    return warp_blend_pack(sa, sb, t, nt);
}

// What the select warp's pixel votes with: the summed absolute difference of the two samples' three colour counts as stored (alpha
// does not vote) -- an integer 0 .. 765, exact in f32, the same for RGBA and BGRA input order.
__device__ __forceinline__ float warp_sample_error(const float4 &sa, const float4 &sb)
{
    return (fabsf(sa.x - sb.x) + fabsf(sa.y - sb.y)) + fabsf(sa.z - sb.z);
}

// The tile of the three dense kernels, frames of at least 2 x 2 pixels below 4 GiB (warp_corner_ok).  blockDim = (64, 4); a thread
// owns XV consecutive pixels in each of RV rows (y, y + 4, .. of the block's 4 RV): its vectors are fetched first, then the gathers
// of its pixels -- independent chains -- are in flight together.  XV = 2 (frame width even, host-checked): the two pixels are one
// 8-byte store and a wave's gathers stay on few cache lines; else XV = 1.  Four pixels per thread (16-byte stores) was measured
// and rejected: a wave's gathers spread over four times the cache lines and the kernel stops being bound by its arithmetic
// (profiles/r03_warp_kernel_layouts_ab.txt, us per 1080p pair EXACT / FMA: 1 x 4 9.6-10.4 / 8.5-8.7; 4 x 1 11.2-13.1 / 11.1-13.1;
// 2 x 2 8.7-9.3 / 7.9-8.5).
// MT: the multi-time form -- the vectors are fetched once, then the pixels are warped, blended and stored once per time of the set
// (frame k of the pair at out + k * w * h * 4; the gathers of the later times hit the lines the first one brought into the L2).
// MT = false is the single-time kernel: the set's one time, no loop.
// SRC supplies the vectors:
//   load(ybase, x0, w, h, npx)                     once, before the times: the thread's own vectors (rows past the frame: the last row's)
//   at_time(ybase, x0, w, h, wmax, hmax, tv)       once per time, before the pixels
//   vec(j, i)                                      the vector of pixel i of thread row j
//   kSwizzle                                       whether the family has an input channel selector (sel)
constexpr int kWarpRV = 2;

// TIMES supplies what the tile writes for the block's pair (blockIdx.z), all of it wave-uniform:
//   begin()                                        once, before the vectors are loaded
//   count()                                        how many frames
//   time(k)                                        frame k's time
//   frame(k, npx)                                  where frame k goes
// PairTimes: the launch's time set, frame k of the pair at pair_out + k * w * h * 4 (MT = false: the set's one time, no loop).
// The rate-conversion kernels (nus_k_retime.hip) take both from the conversion's schedule instead.
template <bool MT>
struct PairTimes {
    const TimeSet &ts;
    uint8_t *out;
    size_t out_pair_stride;
    uint8_t *pair_out;
    __device__ __forceinline__ void begin() { pair_out = out + (size_t)blockIdx.z * out_pair_stride; }
    __device__ __forceinline__ uint32_t count() const { return MT ? ts.n : 1; }
    __device__ __forceinline__ float time(uint32_t k) const { return ts.t[k]; }
    __device__ __forceinline__ uint32_t *frame(uint32_t k, size_t npx) const { return reinterpret_cast<uint32_t *>(pair_out + (size_t)k * npx * 4); }
};

template <int MODE, int XV, int RV, typename SRC, typename TIMES>
__device__ __forceinline__ void warp_blend_tile_at(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, size_t a_stride,
                                                   size_t b_stride, uint32_t w, uint32_t h, uint32_t sel, SRC src, TIMES times)
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
    src.load(ybase, x0, w, h, npx);
    const uint32_t nk = times.count();
    for (uint32_t k = 0; k < nk; ++k) {
        float tv = times.time(k);
        asm volatile("" : "+v"(tv));
        const float nt = 1.0f - tv;
        uint32_t *const frame_out = times.frame(k, npx);
        src.at_time(ybase, x0, w, h, wmax, hmax, tv);
#pragma unroll
        for (int j = 0; j < RV; ++j) {
            const uint32_t y = ybase + 4 * j;
            if (y >= h) break; // wave-uniform
            const float yfl = (float)y;
            uint32_t o[XV];
#pragma unroll
            for (int i = 0; i < XV; ++i) {
                const uint32_t p = warp_blend_pixel<MODE>(ra, rb, row_bytes, wmax, hmax, w - 2, h - 2, (float)(x0 + i), yfl, src.vec(j, i), tv, nt);
                o[i] = SRC::kSwizzle ? swz(p, sel) : p;
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

// the tile of a launch with one time set for all its pairs
template <int MODE, int XV, int RV, bool MT, typename SRC>
__device__ __forceinline__ void warp_blend_tile(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, uint8_t *__restrict__ out,
                                                size_t a_stride, size_t b_stride, size_t out_pair_stride, uint32_t w, uint32_t h,
                                                const TimeSet &ts, uint32_t sel, SRC src)
{
    warp_blend_tile_at<MODE, XV, RV>(a, b, a_stride, b_stride, w, h, sel, src, PairTimes<MT>{ts, out, out_pair_stride, nullptr});
}

// ---------------------------------------------------------------------------------
// What the three launchers share (host)
// ---------------------------------------------------------------------------------

// The launch's times: times[0 .. n_times), or the one time t where n_times is 0.  false: more than kInterpMaxTimes, or no array.
inline bool warp_time_set(float t, const float *times, uint32_t n_times, TimeSet &ts)
{
    if (n_times > kInterpMaxTimes || (n_times > 0 && times == nullptr)) return false;
    ts = TimeSet{};
    ts.n = n_times ? n_times : 1;
    ts.t[0] = t;
    for (uint32_t k = 0; k < n_times; ++k) ts.t[k] = times[k];
    return true;
}

// bytes between the outputs of consecutive pairs: the caller's, or the pair's frames tightly packed
inline size_t warp_out_stride(size_t out_pair_stride, const TimeSet &ts, size_t npx) { return out_pair_stride ? out_pair_stride : ts.n * npx * 4; }

// What the tile (and the corner form of the projection) needs: every texel pair inside the frame, 32-bit byte offsets into the
// frames and into a flow plane of flow_cell_bytes per pixel (0: no flow plane is addressed that way), 24-bit multiplies.  Frames
// that fail it go to the _tiny kernels.
inline bool warp_corner_ok(uint32_t w, uint32_t h, uint32_t flow_cell_bytes)
{
    const size_t npx = (size_t)w * h;
    return w >= 2 && h >= 2 && npx * 4 < (1ull << 32) && npx * flow_cell_bytes < (1ull << 32) && w * 4ull < (1u << 24) && h < (1u << 24);
}

// grid of a (64, 4) block whose threads own xv x rv pixels; pairs on z
inline dim3 warp_grid(uint32_t w, uint32_t h, uint32_t xv, uint32_t rv, uint32_t n) { return dim3(cdiv(w, kWave * xv), cdiv(h, 4 * rv), n); }

} // namespace

} // namespace nus
