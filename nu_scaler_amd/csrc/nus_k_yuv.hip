// nus_k_yuv.hip -- 8-bit planar YUV 4:2:0 (I420) <-> RGBA8 over device-resident frame batches: the nus_yuv420_* / nus_rgba8_to_yuv420*
// entry points of include/nuscaler_hip.h, where the integer contract is written.  BUILD-DEFINED: the reference has no YUV.
//
// Pure streaming, 5.5 bytes per pixel, no reuse beyond a chroma row: no LDS, no atomics, no scratch.  All arithmetic is int32 in
// Q14 (S = 14, one rounding per output byte); the coefficient tables come with the launch (YuvLaunch::to_yuv / to_rgb, built on
// the host by yuv_coefficients) and every kernel takes a per-lane copy of them.
//   k_yuv_to_rgba<FILTER, SITING>      a thread owns 8 pixels in the two luma rows of one chroma row: two 8-byte Y loads, the
//                    chroma of the run as one dword per plane and row (bilinear: three rows, and the clamped neighbour byte on
//                    either side), four 16-byte RGBA stores.
//   k_rgba_to_yuv<SITING>              a thread owns 16 x 2 pixels: eight 16-byte loads (left siting: the clamped pixel left of the
//                    run as well), two 16-byte Y stores, one 8-byte store each for U and V.
//   k_yuv_to_rgba_px / k_rgba_to_yuv_cell   one pixel / one chroma cell per thread, 64-bit addressing, byte accesses on the YUV
//                    side: widths that do not fill the run, bases or strides that break the alignment, frames of 4 GiB and more.
// The launcher picks the form from w, the bases and both strides (yuv_shape).  Frame i of a batch is at base + i * stride on either
// side; frames go on grid.z through for_grid_z_chunks; gaps between frames are never written.
#include "nus_yuv_device.hpp" // the per-pixel arithmetic, shared with nus_k_nv12.hip

namespace nus {

namespace {

// ---- the aligned forms ------------------------------------------------------------------------------------------------------------

// six cells of one chroma row around a run of four: c[0] = cell cx0 - 1 (clamped), c[1 .. 4] the run (one dword), c[5] = cell cx0 + 4
// (clamped)
template <int SITING>
__device__ __forceinline__ void chroma_row6(const uint8_t *row, uint32_t cx0, uint32_t cw, int (&c)[6])
{
    const uint32_t d = *reinterpret_cast<const uint32_t *>(row + cx0);
#pragma unroll
    for (int i = 0; i < 4; ++i) c[1 + i] = (int)byte_of(d, i);
    c[0] = SITING == 0 ? (int)row[cx0 > 0 ? cx0 - 1 : 0] : 0; // (left siting never looks left)
    c[5] = (int)row[umin(cx0 + 4, cw - 1)];
}

template <int FILTER, int SITING>
__global__ __launch_bounds__(256) void k_yuv_to_rgba(const uint8_t *__restrict__ yuv, size_t yuv_stride, uint8_t *__restrict__ rgba,
                                                     size_t rgba_stride, uint32_t w, uint32_t h, YuvTables T, uint32_t sel)
{
    const uint32_t run = blockIdx.x * kWave + threadIdx.x, cy = blockIdx.y * 4 + threadIdx.y;
    const uint32_t cw = w >> 1, ch = (h + 1) >> 1; // (w % 8 == 0)
    if (run * 8 >= w || cy >= ch) return;
    lane_copies(T);
    asm volatile("" : "+v"(sel));
    const uint8_t *const Y = yuv + (size_t)blockIdx.z * yuv_stride;
    const uint8_t *const U = Y + (size_t)w * h, *const V = U + (size_t)cw * ch;
    uint32_t *const out = reinterpret_cast<uint32_t *>(rgba + (size_t)blockIdx.z * rgba_stride);
    const uint32_t x0 = run * 8, cx0 = run * 4, y0 = cy * 2;
    const bool two = y0 + 1 < h; // (an odd height: the last chroma row has one luma row)
    const uint2 ya = *reinterpret_cast<const uint2 *>(Y + (size_t)y0 * w + x0);
    const uint2 yb = *reinterpret_cast<const uint2 *>(Y + (size_t)(two ? y0 + 1 : y0) * w + x0); // (without a branch: the row again)

    int ut[6], ub[6], vt[6], vb[6]; // chroma of the top / bottom luma row per cell cx0 - 1 .. cx0 + 4: code values, or sums of weight 4
    if (FILTER == 0) {
        const uint32_t du = *reinterpret_cast<const uint32_t *>(U + (size_t)cy * cw + cx0);
        const uint32_t dv = *reinterpret_cast<const uint32_t *>(V + (size_t)cy * cw + cx0);
#pragma unroll
        for (int i = 0; i < 4; ++i) ut[1 + i] = ub[1 + i] = (int)byte_of(du, i) - 128, vt[1 + i] = vb[1 + i] = (int)byte_of(dv, i) - 128;
    } else {
        const size_t rm = (size_t)(cy > 0 ? cy - 1 : 0) * cw, r0 = (size_t)cy * cw, rp = (size_t)umin(cy + 1, ch - 1) * cw;
        int a[6], b[6], c[6];
        chroma_row6<SITING>(U + rm, cx0, cw, a), chroma_row6<SITING>(U + r0, cx0, cw, b), chroma_row6<SITING>(U + rp, cx0, cw, c);
#pragma unroll
        for (int i = 0; i < 6; ++i) ut[i] = a[i] + 3 * b[i], ub[i] = 3 * b[i] + c[i];
        chroma_row6<SITING>(V + rm, cx0, cw, a), chroma_row6<SITING>(V + r0, cx0, cw, b), chroma_row6<SITING>(V + rp, cx0, cw, c);
#pragma unroll
        for (int i = 0; i < 6; ++i) vt[i] = a[i] + 3 * b[i], vb[i] = 3 * b[i] + c[i];
    }
    uint32_t pa[8], pb[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int j = 1 + (k >> 1);
        const int la = (int)byte_of(k < 4 ? ya.x : ya.y, k & 3), lb = (int)byte_of(k < 4 ? yb.x : yb.y, k & 3);
        if (FILTER == 0) {
            pa[k] = swz(yuv_pixel<0>(la, ut[j], vt[j], T), sel);
            pb[k] = swz(yuv_pixel<0>(lb, ub[j], vb[j], T), sel);
        } else {
            const bool odd = (k & 1) != 0;
            pa[k] = swz(yuv_pixel<4>(la, chroma_h<SITING>(odd, ut[j - 1], ut[j], ut[j + 1]) - 2048,
                                     chroma_h<SITING>(odd, vt[j - 1], vt[j], vt[j + 1]) - 2048, T), sel);
            pb[k] = swz(yuv_pixel<4>(lb, chroma_h<SITING>(odd, ub[j - 1], ub[j], ub[j + 1]) - 2048,
                                     chroma_h<SITING>(odd, vb[j - 1], vb[j], vb[j + 1]) - 2048, T), sel);
        }
    }
    uint32_t *const oa = out + (size_t)y0 * w + x0;
    store_out16<false>(oa, make_uint4(pa[0], pa[1], pa[2], pa[3]));
    store_out16<false>(oa + 4, make_uint4(pa[4], pa[5], pa[6], pa[7]));
    if (two) {
        store_out16<false>(oa + w, make_uint4(pb[0], pb[1], pb[2], pb[3]));
        store_out16<false>(oa + w + 4, make_uint4(pb[4], pb[5], pb[6], pb[7]));
    }
}

template <int SITING>
__global__ __launch_bounds__(256) void k_rgba_to_yuv(const uint8_t *__restrict__ rgba, size_t rgba_stride, uint8_t *__restrict__ yuv,
                                                     size_t yuv_stride, uint32_t w, uint32_t h, YuvTables T, uint32_t sel)
{
    const uint32_t run = blockIdx.x * kWave + threadIdx.x, cy = blockIdx.y * 4 + threadIdx.y;
    const uint32_t cw = w >> 1, ch = (h + 1) >> 1; // (w % 16 == 0)
    if (run * 16 >= w || cy >= ch) return;
    lane_copies(T);
    asm volatile("" : "+v"(sel));
    const uint32_t *const in = reinterpret_cast<const uint32_t *>(rgba + (size_t)blockIdx.z * rgba_stride);
    uint8_t *const Y = yuv + (size_t)blockIdx.z * yuv_stride;
    uint8_t *const U = Y + (size_t)w * h, *const V = U + (size_t)cw * ch;
    const uint32_t x0 = run * 16, cx0 = run * 8, y0 = cy * 2;
    const bool two = y0 + 1 < h;
    const uint32_t *const ra = in + (size_t)y0 * w + x0, *const rb = two ? ra + w : ra; // (the row below, clamped into the frame)
    uint32_t pa[17], pb[17]; // [0]: the pixel left of the run (left siting), [1 .. 16]: the run
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint4 a = swz4(*reinterpret_cast<const uint4 *>(ra + 4 * q), sel), b = swz4(*reinterpret_cast<const uint4 *>(rb + 4 * q), sel);
        pa[1 + 4 * q] = a.x, pa[2 + 4 * q] = a.y, pa[3 + 4 * q] = a.z, pa[4 + 4 * q] = a.w;
        pb[1 + 4 * q] = b.x, pb[2 + 4 * q] = b.y, pb[3 + 4 * q] = b.z, pb[4 + 4 * q] = b.w;
    }
    if (SITING == 1) {
        pa[0] = x0 > 0 ? swz(ra[-1], sel) : pa[1];
        pb[0] = x0 > 0 ? swz(rb[-1], sel) : pb[1];
    }
    uint32_t la[4], lb[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        la[q] = lb[q] = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            la[q] |= (uint32_t)luma_of(pa[1 + 4 * q + i], T) << (8 * i);
            lb[q] |= (uint32_t)luma_of(pb[1 + 4 * q + i], T) << (8 * i);
        }
    }
    store_out16<false>(reinterpret_cast<uint32_t *>(Y + (size_t)y0 * w + x0), make_uint4(la[0], la[1], la[2], la[3]));
    if (two) store_out16<false>(reinterpret_cast<uint32_t *>(Y + (size_t)(y0 + 1) * w + x0), make_uint4(lb[0], lb[1], lb[2], lb[3]));
    uint32_t u[2] = {0, 0}, v[2] = {0, 0};
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        // tap sums, R and B side by side in one word (a sum is at most 8 * 255)
        uint32_t srb, sg;
        const int i = 1 + 2 * c;
        if (SITING == 0) {
            srb = (pa[i] & 0xff00ffu) + (pa[i + 1] & 0xff00ffu) + (pb[i] & 0xff00ffu) + (pb[i + 1] & 0xff00ffu);
            sg = byte_of(pa[i], 1) + byte_of(pa[i + 1], 1) + byte_of(pb[i], 1) + byte_of(pb[i + 1], 1);
            u[c >> 2] |= chroma_of<1, 2>(srb, sg, T) << (8 * (c & 3));
            v[c >> 2] |= chroma_of<2, 2>(srb, sg, T) << (8 * (c & 3));
        } else {
            srb = (pa[i - 1] & 0xff00ffu) + 2 * (pa[i] & 0xff00ffu) + (pa[i + 1] & 0xff00ffu) + (pb[i - 1] & 0xff00ffu) +
                  2 * (pb[i] & 0xff00ffu) + (pb[i + 1] & 0xff00ffu);
            sg = byte_of(pa[i - 1], 1) + 2 * byte_of(pa[i], 1) + byte_of(pa[i + 1], 1) + byte_of(pb[i - 1], 1) + 2 * byte_of(pb[i], 1) +
                 byte_of(pb[i + 1], 1);
            u[c >> 2] |= chroma_of<1, 3>(srb, sg, T) << (8 * (c & 3));
            v[c >> 2] |= chroma_of<2, 3>(srb, sg, T) << (8 * (c & 3));
        }
    }
    store_out8<false>(reinterpret_cast<uint32_t *>(U + (size_t)cy * cw + cx0), make_uint2(u[0], u[1]));
    store_out8<false>(reinterpret_cast<uint32_t *>(V + (size_t)cy * cw + cx0), make_uint2(v[0], v[1]));
}

// ---- the scalar forms -------------------------------------------------------------------------------------------------------------

// bilinear chroma at luma position (x, y) as a sum of weight 16; chroma coordinates clamped
template <int SITING>
__device__ __forceinline__ int chroma16_at(const uint8_t *plane, size_t cw, size_t ch, size_t x, size_t y)
{
    const size_t cx = x >> 1, cy = y >> 1;
    const bool oy = (y & 1) != 0, ox = (x & 1) != 0;
    const size_t ra = (oy ? cy : (cy > 0 ? cy - 1 : 0)) * cw, rb = (oy ? (cy + 1 < ch ? cy + 1 : ch - 1) : cy) * cw;
    const int wa = oy ? 3 : 1;
    const size_t xl = cx > 0 ? cx - 1 : 0, xr = cx + 1 < cw ? cx + 1 : cw - 1;
    const int l = wa * plane[ra + xl] + (4 - wa) * plane[rb + xl];
    const int m = wa * plane[ra + cx] + (4 - wa) * plane[rb + cx];
    const int r = wa * plane[ra + xr] + (4 - wa) * plane[rb + xr];
    return chroma_h<SITING>(ox, l, m, r);
}

template <int FILTER, int SITING>
__global__ __launch_bounds__(256) void k_yuv_to_rgba_px(const uint8_t *__restrict__ yuv, size_t yuv_stride, uint8_t *__restrict__ rgba,
                                                        size_t rgba_stride, uint32_t w, uint32_t h, YuvTables T, uint32_t sel)
{
    const size_t x = (size_t)blockIdx.x * kWave + threadIdx.x, y = (size_t)blockIdx.y * 4 + threadIdx.y;
    if (x >= w || y >= h) return;
    const size_t cw = ((size_t)w + 1) >> 1, ch = ((size_t)h + 1) >> 1;
    const uint8_t *const Y = yuv + (size_t)blockIdx.z * yuv_stride;
    const uint8_t *const U = Y + (size_t)w * h, *const V = U + cw * ch;
    uint32_t *const out = reinterpret_cast<uint32_t *>(rgba + (size_t)blockIdx.z * rgba_stride);
    const int l = Y[y * w + x];
    uint32_t p;
    if (FILTER == 0) {
        const size_t c = (y >> 1) * cw + (x >> 1);
        p = yuv_pixel<0>(l, (int)U[c] - 128, (int)V[c] - 128, T);
    } else {
        p = yuv_pixel<4>(l, chroma16_at<SITING>(U, cw, ch, x, y) - 2048, chroma16_at<SITING>(V, cw, ch, x, y) - 2048, T);
    }
    out[y * w + x] = swz(p, sel);
}

template <int SITING>
__global__ __launch_bounds__(256) void k_rgba_to_yuv_cell(const uint8_t *__restrict__ rgba, size_t rgba_stride, uint8_t *__restrict__ yuv,
                                                          size_t yuv_stride, uint32_t w, uint32_t h, YuvTables T, uint32_t sel)
{
    const size_t cx = (size_t)blockIdx.x * kWave + threadIdx.x, cy = (size_t)blockIdx.y * 4 + threadIdx.y;
    const size_t cw = ((size_t)w + 1) >> 1, ch = ((size_t)h + 1) >> 1;
    if (cx >= cw || cy >= ch) return;
    const uint32_t *const in = reinterpret_cast<const uint32_t *>(rgba + (size_t)blockIdx.z * rgba_stride);
    uint8_t *const Y = yuv + (size_t)blockIdx.z * yuv_stride;
    uint8_t *const U = Y + (size_t)w * h, *const V = U + cw * ch;
    const size_t x0 = 2 * cx, y0 = 2 * cy;
    const bool right = x0 + 1 < w, below = y0 + 1 < h;
    const size_t x1 = right ? x0 + 1 : x0, xm = x0 > 0 ? x0 - 1 : 0; // tap coordinates, clamped into the frame
    const uint32_t *const ra = in + y0 * w, *const rb = below ? ra + w : ra;
    const uint32_t a0 = swz(ra[x0], sel), a1 = swz(ra[x1], sel), b0 = swz(rb[x0], sel), b1 = swz(rb[x1], sel);
    Y[y0 * w + x0] = (uint8_t)luma_of(a0, T);
    if (right) Y[y0 * w + x0 + 1] = (uint8_t)luma_of(a1, T);
    if (below) Y[(y0 + 1) * w + x0] = (uint8_t)luma_of(b0, T);
    if (right && below) Y[(y0 + 1) * w + x0 + 1] = (uint8_t)luma_of(b1, T);
    if (SITING == 0) {
        const uint32_t srb = (a0 & 0xff00ffu) + (a1 & 0xff00ffu) + (b0 & 0xff00ffu) + (b1 & 0xff00ffu);
        const uint32_t sg = byte_of(a0, 1) + byte_of(a1, 1) + byte_of(b0, 1) + byte_of(b1, 1);
        U[cy * cw + cx] = (uint8_t)chroma_of<1, 2>(srb, sg, T);
        V[cy * cw + cx] = (uint8_t)chroma_of<2, 2>(srb, sg, T);
    } else {
        const uint32_t am = swz(ra[xm], sel), bm = swz(rb[xm], sel);
        const uint32_t srb = (am & 0xff00ffu) + 2 * (a0 & 0xff00ffu) + (a1 & 0xff00ffu) + (bm & 0xff00ffu) + 2 * (b0 & 0xff00ffu) + (b1 & 0xff00ffu);
        const uint32_t sg = byte_of(am, 1) + 2 * byte_of(a0, 1) + byte_of(a1, 1) + byte_of(bm, 1) + 2 * byte_of(b0, 1) + byte_of(b1, 1);
        U[cy * cw + cx] = (uint8_t)chroma_of<1, 3>(srb, sg, T);
        V[cy * cw + cx] = (uint8_t)chroma_of<2, 3>(srb, sg, T);
    }
}

// ---- launch -----------------------------------------------------------------------------------------------------------------------

inline bool yuv_launch_ok(const YuvLaunch &L)
{
    const size_t cw = ((size_t)L.w + 1) / 2, ch = ((size_t)L.h + 1) / 2;
    return L.yuv && L.rgba && L.w && L.h && L.n_frames && (L.siting | 1) == 1 && (L.chroma_filter | 1) == 1 &&
           L.rgba_frame_stride >= (size_t)L.w * L.h * 4 && L.yuv_frame_stride >= (size_t)L.w * L.h + 2 * cw * ch && (L.rgba_frame_stride % 4) == 0 &&
           aligned_to(L.rgba, 4) && cdiv((uint32_t)ch, 4) <= 65535;
}

// The form of a launch: the aligned kernels where the width fills the thread's run (8 pixels towards RGBA, 16 towards YUV), every
// base and stride keeps the run's widest access aligned (16 bytes on the RGBA side; 8 / 16 on the YUV side, which aligns the
// chroma planes' dword / 8-byte accesses too: their offsets w h and cw ch are multiples of the run) and the RGBA frame stays
// below 4 GiB; else the scalar kernels.
struct YuvShape {
    bool vec;
    dim3 grid;
};
inline YuvShape yuv_shape(const YuvLaunch &L, bool to_rgba, uint32_t n)
{
    const uint32_t run = to_rgba ? 8 : 16, yuv_align = to_rgba ? 8 : 16;
    YuvShape s;
    s.vec = (L.w % run) == 0 && (uint64_t)L.w * L.h * 4 < ((uint64_t)1 << 32) && aligned_to(L.rgba, 16) && (L.rgba_frame_stride % 16) == 0 &&
            aligned_to(L.yuv, yuv_align) && (L.yuv_frame_stride % yuv_align) == 0;
    const uint32_t ch = (L.h + 1) / 2;
    if (s.vec)
        s.grid = dim3(cdiv(L.w / run, kWave), cdiv(ch, 4), n);
    else if (to_rgba)
        s.grid = dim3(cdiv(L.w, kWave), cdiv(L.h, 4), n);
    else
        s.grid = dim3(cdiv((L.w + 1) / 2, kWave), cdiv(ch, 4), n);
    return s;
}

} // namespace

hipError_t launch_yuv_to_rgba(const YuvLaunch &L)
{
    if (!yuv_launch_ok(L)) return hipErrorInvalidValue;
    const YuvTables T = yuv_tables(L);
    return for_grid_z_chunks(L.n_frames, [&](uint32_t done, uint32_t n) {
        YuvLaunch C = L;
        C.yuv = L.yuv + (size_t)done * L.yuv_frame_stride, C.rgba = L.rgba + (size_t)done * L.rgba_frame_stride;
        const YuvShape s = yuv_shape(C, true, n);
        const dim3 block(kWave, 4);
#define NUS_YR(K) {{K<0, 0>, K<0, 1>}, {K<1, 0>, K<1, 1>}}
        static constexpr decltype(&k_yuv_to_rgba<0, 0>) kernels[2][2][2] = {NUS_YR(k_yuv_to_rgba_px), NUS_YR(k_yuv_to_rgba)}; // [vec][filter][siting]
#undef NUS_YR
        hipLaunchKernelGGL(kernels[s.vec][L.chroma_filter][L.siting], s.grid, block, 0, L.stream, C.yuv, L.yuv_frame_stride, C.rgba,
                           L.rgba_frame_stride, L.w, L.h, T, L.sel);
    });
}

hipError_t launch_rgba_to_yuv(const YuvLaunch &L)
{
    if (!yuv_launch_ok(L)) return hipErrorInvalidValue;
    const YuvTables T = yuv_tables(L);
    return for_grid_z_chunks(L.n_frames, [&](uint32_t done, uint32_t n) {
        YuvLaunch C = L;
        C.yuv = L.yuv + (size_t)done * L.yuv_frame_stride, C.rgba = L.rgba + (size_t)done * L.rgba_frame_stride;
        const YuvShape s = yuv_shape(C, false, n);
        const dim3 block(kWave, 4);
        static constexpr decltype(&k_rgba_to_yuv<0>) kernels[2][2] = {{k_rgba_to_yuv_cell<0>, k_rgba_to_yuv_cell<1>},
                                                                      {k_rgba_to_yuv<0>, k_rgba_to_yuv<1>}}; // [vec][siting]
        hipLaunchKernelGGL(kernels[s.vec][L.siting], s.grid, block, 0, L.stream, static_cast<const uint8_t *>(C.rgba), L.rgba_frame_stride,
                           C.yuv, L.yuv_frame_stride, L.w, L.h, T, L.sel);
    });
}

} // namespace nus
