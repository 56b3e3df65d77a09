// nus_k_nv12.hip -- 8-bit NV12 (a Y plane and one plane of interleaved U,V byte pairs, rows a pitch apart) <-> RGBA8, and the
// repack between NV12 and I420, over device-resident frame batches: the nus_nv12_* / nus_rgba8_to_nv12* / nus_yuv420_to_nv12_device
// entry points of include/nuscaler_hip.h ("NV12 frames").  BUILD-DEFINED: the reference has no YUV.
//
// The arithmetic is nus_k_yuv.hip's, through the same device functions (nus_yuv_device.hpp): every byte is the I420 kernels' byte,
// the chroma bytes lie elsewhere.  Pure streaming: no LDS, no atomics, no scratch.
//   k_nv12_to_rgba<FILTER, SITING>     a thread owns 8 pixels in the two luma rows of one chroma row: two 8-byte Y loads, the
//                    chroma of the run -- four U,V pairs -- as ONE 8-byte load per chroma row (bilinear: three rows, and the clamped
//                    neighbour pair on either side as a 2-byte load), four 16-byte RGBA stores.
//   k_rgba_to_nv12<SITING>             a thread owns 16 x 2 pixels: eight 16-byte loads (left siting: the clamped pixel left of the
//                    run as well), two 16-byte Y stores, the run's eight pairs as ONE 16-byte store.
//   k_nv12_to_rgba_px / k_rgba_to_nv12_cell   one pixel / one chroma cell per thread, 64-bit addressing, byte accesses on the NV12
//                    side: widths that do not fill the run, and any base, pitch, uv_offset or stride that breaks the alignment.
//   k_nv12_repack<TO_NV12, VEC>        the repack, either way, bytes only: blockIdx.y walks the h luma rows, then the ch chroma rows.
//                    VEC: a thread moves 16 luma bytes, or 8 U + 8 V bytes (two 8-byte accesses on the planar side, one 16-byte
//                    access on the pair side); else one luma byte / one cell.
// The launcher picks the form per launch (nv12_shape, repack_vec).  Frame i of a batch is at base + i * stride on either side;
// frames go on grid.z through for_grid_z_chunks; row padding, the gap between the planes and the gaps between frames are never
// written.
#include "nus_yuv_device.hpp"

namespace nus {

namespace {

struct Nv12Geom { // by value in the kernel arguments
    size_t fs, y_pitch, uv_pitch, uv_offset;
};

// ---- the aligned forms ------------------------------------------------------------------------------------------------------------

// six cells of one row of pairs around a run of four: [0] = cell cx0 - 1 (clamped), [1 .. 4] the run (one 8-byte load), [5] = cell
// cx0 + 4 (clamped)
template <int SITING>
__device__ __forceinline__ void pair_row6(const uint8_t *row, uint32_t cx0, uint32_t cw, int (&u)[6], int (&v)[6])
{
    const uint2 d = *reinterpret_cast<const uint2 *>(row + 2 * (size_t)cx0);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t two = i < 2 ? d.x : d.y;
        u[1 + i] = (int)byte_of(two, 2 * (i & 1)), v[1 + i] = (int)byte_of(two, 2 * (i & 1) + 1);
    }
    const uint32_t l = SITING == 0 ? *reinterpret_cast<const uint16_t *>(row + 2 * (size_t)(cx0 > 0 ? cx0 - 1 : 0)) : 0u; // (left siting never looks left)
    const uint32_t r = *reinterpret_cast<const uint16_t *>(row + 2 * (size_t)umin(cx0 + 4, cw - 1));
    u[0] = (int)(l & 0xffu), v[0] = (int)(l >> 8), u[5] = (int)(r & 0xffu), v[5] = (int)(r >> 8);
}

template <int FILTER, int SITING>
__global__ __launch_bounds__(256) void k_nv12_to_rgba(const uint8_t *__restrict__ nv12, Nv12Geom G, uint8_t *__restrict__ rgba, size_t rgba_stride,
                                                      uint32_t w, uint32_t h, YuvTables T, uint32_t sel)
{
    const uint32_t run = blockIdx.x * kWave + threadIdx.x, cy = blockIdx.y * 4 + threadIdx.y;
    const uint32_t cw = w >> 1, ch = (h + 1) >> 1; // (w % 8 == 0)
    if (run * 8 >= w || cy >= ch) return;
    lane_copies(T);
    asm volatile("" : "+v"(sel));
    const uint8_t *const Y = nv12 + (size_t)blockIdx.z * G.fs;
    const uint8_t *const UV = Y + G.uv_offset;
    uint32_t *const out = reinterpret_cast<uint32_t *>(rgba + (size_t)blockIdx.z * rgba_stride);
    const uint32_t x0 = run * 8, cx0 = run * 4, y0 = cy * 2;
    const bool two = y0 + 1 < h; // (an odd height: the last chroma row has one luma row)
    const uint2 ya = *reinterpret_cast<const uint2 *>(Y + (size_t)y0 * G.y_pitch + x0);
    const uint2 yb = *reinterpret_cast<const uint2 *>(Y + (size_t)(two ? y0 + 1 : y0) * G.y_pitch + x0); // (without a branch: the row again)

    int ut[6], ub[6], vt[6], vb[6]; // chroma of the top / bottom luma row per cell cx0 - 1 .. cx0 + 4: code values, or sums of weight 4
    if (FILTER == 0) {
        const uint2 d = *reinterpret_cast<const uint2 *>(UV + (size_t)cy * G.uv_pitch + 2 * (size_t)cx0);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t pr = i < 2 ? d.x : d.y;
            ut[1 + i] = ub[1 + i] = (int)byte_of(pr, 2 * (i & 1)) - 128, vt[1 + i] = vb[1 + i] = (int)byte_of(pr, 2 * (i & 1) + 1) - 128;
        }
    } else {
        const uint8_t *const rm = UV + (size_t)(cy > 0 ? cy - 1 : 0) * G.uv_pitch, *const r0 = UV + (size_t)cy * G.uv_pitch;
        const uint8_t *const rp = UV + (size_t)umin(cy + 1, ch - 1) * G.uv_pitch;
        int ua[6], u0[6], uc[6], va[6], v0[6], vc[6];
        pair_row6<SITING>(rm, cx0, cw, ua, va), pair_row6<SITING>(r0, cx0, cw, u0, v0), pair_row6<SITING>(rp, cx0, cw, uc, vc);
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            ut[i] = ua[i] + 3 * u0[i], ub[i] = 3 * u0[i] + uc[i];
            vt[i] = va[i] + 3 * v0[i], vb[i] = 3 * v0[i] + vc[i];
        }
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
__global__ __launch_bounds__(256) void k_rgba_to_nv12(const uint8_t *__restrict__ rgba, size_t rgba_stride, uint8_t *__restrict__ nv12, Nv12Geom G,
                                                      uint32_t w, uint32_t h, YuvTables T, uint32_t sel)
{
    const uint32_t run = blockIdx.x * kWave + threadIdx.x, cy = blockIdx.y * 4 + threadIdx.y;
    const uint32_t ch = (h + 1) >> 1; // (w % 16 == 0)
    if (run * 16 >= w || cy >= ch) return;
    lane_copies(T);
    asm volatile("" : "+v"(sel));
    const uint32_t *const in = reinterpret_cast<const uint32_t *>(rgba + (size_t)blockIdx.z * rgba_stride);
    uint8_t *const Y = nv12 + (size_t)blockIdx.z * G.fs;
    uint8_t *const UV = Y + G.uv_offset;
    const uint32_t x0 = run * 16, y0 = cy * 2;
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
    store_out16<false>(reinterpret_cast<uint32_t *>(Y + (size_t)y0 * G.y_pitch + x0), make_uint4(la[0], la[1], la[2], la[3]));
    if (two) store_out16<false>(reinterpret_cast<uint32_t *>(Y + (size_t)(y0 + 1) * G.y_pitch + x0), make_uint4(lb[0], lb[1], lb[2], lb[3]));
    uint32_t uv[4] = {0, 0, 0, 0}; // eight U,V pairs: two to a word
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        // tap sums, R and B side by side in one word (a sum is at most 8 * 255)
        uint32_t srb, sg, pair;
        const int i = 1 + 2 * c;
        if (SITING == 0) {
            srb = (pa[i] & 0xff00ffu) + (pa[i + 1] & 0xff00ffu) + (pb[i] & 0xff00ffu) + (pb[i + 1] & 0xff00ffu);
            sg = byte_of(pa[i], 1) + byte_of(pa[i + 1], 1) + byte_of(pb[i], 1) + byte_of(pb[i + 1], 1);
            pair = chroma_of<1, 2>(srb, sg, T) | (chroma_of<2, 2>(srb, sg, T) << 8);
        } else {
            srb = (pa[i - 1] & 0xff00ffu) + 2 * (pa[i] & 0xff00ffu) + (pa[i + 1] & 0xff00ffu) + (pb[i - 1] & 0xff00ffu) +
                  2 * (pb[i] & 0xff00ffu) + (pb[i + 1] & 0xff00ffu);
            sg = byte_of(pa[i - 1], 1) + 2 * byte_of(pa[i], 1) + byte_of(pa[i + 1], 1) + byte_of(pb[i - 1], 1) + 2 * byte_of(pb[i], 1) +
                 byte_of(pb[i + 1], 1);
            pair = chroma_of<1, 3>(srb, sg, T) | (chroma_of<2, 3>(srb, sg, T) << 8);
        }
        uv[c >> 1] |= pair << (16 * (c & 1));
    }
    store_out16<false>(reinterpret_cast<uint32_t *>(UV + (size_t)cy * G.uv_pitch + x0), make_uint4(uv[0], uv[1], uv[2], uv[3])); // (pair 8 run at byte 16 run)
}

// ---- the scalar forms -------------------------------------------------------------------------------------------------------------

// bilinear chroma of channel c (0 U, 1 V) at luma position (x, y) as a sum of weight 16; chroma coordinates clamped
template <int SITING>
__device__ __forceinline__ int pair16_at(const uint8_t *uv, size_t pitch, size_t cw, size_t ch, size_t x, size_t y, size_t c)
{
    const size_t cx = x >> 1, cy = y >> 1;
    const bool oy = (y & 1) != 0, ox = (x & 1) != 0;
    const size_t ra = (oy ? cy : (cy > 0 ? cy - 1 : 0)) * pitch + c, rb = (oy ? (cy + 1 < ch ? cy + 1 : ch - 1) : cy) * pitch + c;
    const int wa = oy ? 3 : 1;
    const size_t xl = 2 * (cx > 0 ? cx - 1 : 0), xm = 2 * cx, xr = 2 * (cx + 1 < cw ? cx + 1 : cw - 1);
    const int l = wa * uv[ra + xl] + (4 - wa) * uv[rb + xl];
    const int m = wa * uv[ra + xm] + (4 - wa) * uv[rb + xm];
    const int r = wa * uv[ra + xr] + (4 - wa) * uv[rb + xr];
    return chroma_h<SITING>(ox, l, m, r);
}

// (rows beyond gridDim.y * 4 are walked: a frame may have more than 4 * 65535 luma rows)
template <int FILTER, int SITING>
__global__ __launch_bounds__(256) void k_nv12_to_rgba_px(const uint8_t *__restrict__ nv12, Nv12Geom G, uint8_t *__restrict__ rgba, size_t rgba_stride,
                                                         uint32_t w, uint32_t h, YuvTables T, uint32_t sel)
{
    const size_t x = (size_t)blockIdx.x * kWave + threadIdx.x;
    if (x >= w) return;
    const size_t cw = ((size_t)w + 1) >> 1, ch = ((size_t)h + 1) >> 1;
    const uint8_t *const Y = nv12 + (size_t)blockIdx.z * G.fs;
    const uint8_t *const UV = Y + G.uv_offset;
    uint32_t *const out = reinterpret_cast<uint32_t *>(rgba + (size_t)blockIdx.z * rgba_stride);
    for (size_t y = (size_t)blockIdx.y * 4 + threadIdx.y; y < h; y += (size_t)gridDim.y * 4) {
        const int l = Y[y * G.y_pitch + x];
        uint32_t p;
        if (FILTER == 0) {
            const uint8_t *const c = UV + (y >> 1) * G.uv_pitch + 2 * (x >> 1);
            p = yuv_pixel<0>(l, (int)c[0] - 128, (int)c[1] - 128, T);
        } else {
            p = yuv_pixel<4>(l, pair16_at<SITING>(UV, G.uv_pitch, cw, ch, x, y, 0) - 2048, pair16_at<SITING>(UV, G.uv_pitch, cw, ch, x, y, 1) - 2048, T);
        }
        out[y * w + x] = swz(p, sel);
    }
}

template <int SITING>
__global__ __launch_bounds__(256) void k_rgba_to_nv12_cell(const uint8_t *__restrict__ rgba, size_t rgba_stride, uint8_t *__restrict__ nv12, Nv12Geom G,
                                                           uint32_t w, uint32_t h, YuvTables T, uint32_t sel)
{
    const size_t cx = (size_t)blockIdx.x * kWave + threadIdx.x, cy = (size_t)blockIdx.y * 4 + threadIdx.y;
    const size_t cw = ((size_t)w + 1) >> 1, ch = ((size_t)h + 1) >> 1;
    if (cx >= cw || cy >= ch) return;
    const uint32_t *const in = reinterpret_cast<const uint32_t *>(rgba + (size_t)blockIdx.z * rgba_stride);
    uint8_t *const Y = nv12 + (size_t)blockIdx.z * G.fs;
    uint8_t *const UV = Y + G.uv_offset;
    const size_t x0 = 2 * cx, y0 = 2 * cy;
    const bool right = x0 + 1 < w, below = y0 + 1 < h;
    const size_t x1 = right ? x0 + 1 : x0, xm = x0 > 0 ? x0 - 1 : 0; // tap coordinates, clamped into the frame
    const uint32_t *const ra = in + y0 * w, *const rb = below ? ra + w : ra;
    const uint32_t a0 = swz(ra[x0], sel), a1 = swz(ra[x1], sel), b0 = swz(rb[x0], sel), b1 = swz(rb[x1], sel);
    Y[y0 * G.y_pitch + x0] = (uint8_t)luma_of(a0, T);
    if (right) Y[y0 * G.y_pitch + x0 + 1] = (uint8_t)luma_of(a1, T);
    if (below) Y[(y0 + 1) * G.y_pitch + x0] = (uint8_t)luma_of(b0, T);
    if (right && below) Y[(y0 + 1) * G.y_pitch + x0 + 1] = (uint8_t)luma_of(b1, T);
    uint8_t *const cell = UV + cy * G.uv_pitch + 2 * cx;
    if (SITING == 0) {
        const uint32_t srb = (a0 & 0xff00ffu) + (a1 & 0xff00ffu) + (b0 & 0xff00ffu) + (b1 & 0xff00ffu);
        const uint32_t sg = byte_of(a0, 1) + byte_of(a1, 1) + byte_of(b0, 1) + byte_of(b1, 1);
        cell[0] = (uint8_t)chroma_of<1, 2>(srb, sg, T);
        cell[1] = (uint8_t)chroma_of<2, 2>(srb, sg, T);
    } else {
        const uint32_t am = swz(ra[xm], sel), bm = swz(rb[xm], sel);
        const uint32_t srb = (am & 0xff00ffu) + 2 * (a0 & 0xff00ffu) + (a1 & 0xff00ffu) + (bm & 0xff00ffu) + 2 * (b0 & 0xff00ffu) + (b1 & 0xff00ffu);
        const uint32_t sg = byte_of(am, 1) + 2 * byte_of(a0, 1) + byte_of(a1, 1) + byte_of(bm, 1) + 2 * byte_of(b0, 1) + byte_of(b1, 1);
        cell[0] = (uint8_t)chroma_of<1, 3>(srb, sg, T);
        cell[1] = (uint8_t)chroma_of<2, 3>(srb, sg, T);
    }
}

// ---- the repack -------------------------------------------------------------------------------------------------------------------

// eight U and eight V bytes <-> their eight pairs
// (plain shifts: the compiler makes one v_perm_b32 of each word)
__device__ __forceinline__ uint32_t pairs_of(uint32_t u, uint32_t v, int i) // cells 2 i and 2 i + 1 of four: U V U V
{
    return byte_of(u, 2 * i) | (byte_of(v, 2 * i) << 8) | (byte_of(u, 2 * i + 1) << 16) | (byte_of(v, 2 * i + 1) << 24);
}
__device__ __forceinline__ uint32_t channel_of(uint32_t a, uint32_t b, int c) // channel c of the four pairs in the words a, b
{
    return byte_of(a, c) | (byte_of(a, 2 + c) << 8) | (byte_of(b, c) << 16) | (byte_of(b, 2 + c) << 24);
}
__device__ __forceinline__ uint4 interleave8(uint2 u, uint2 v)
{
    return make_uint4(pairs_of(u.x, v.x, 0), pairs_of(u.x, v.x, 1), pairs_of(u.y, v.y, 0), pairs_of(u.y, v.y, 1));
}
__device__ __forceinline__ void deinterleave8(uint4 p, uint2 &u, uint2 &v)
{
    u = make_uint2(channel_of(p.x, p.y, 0), channel_of(p.z, p.w, 0));
    v = make_uint2(channel_of(p.x, p.y, 1), channel_of(p.z, p.w, 1));
}

// TO_NV12: planes -> pairs; else pairs -> planes.  Row r of the walk: luma row r for r < h, then chroma row r - h.
template <bool TO_NV12, bool VEC>
__global__ __launch_bounds__(256) void k_nv12_repack(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, size_t i420_stride, Nv12Geom G,
                                                     uint32_t w, uint32_t h)
{
    const size_t t = (size_t)blockIdx.x * kWave + threadIdx.x;
    const size_t cw = ((size_t)w + 1) >> 1, ch = ((size_t)h + 1) >> 1, rows = (size_t)h + ch;
    const uint8_t *const s = src + (size_t)blockIdx.z * (TO_NV12 ? i420_stride : G.fs);
    uint8_t *const d = dst + (size_t)blockIdx.z * (TO_NV12 ? G.fs : i420_stride);
    const size_t u_off = (size_t)w * h, v_off = u_off + cw * ch;
    for (size_t r = (size_t)blockIdx.y * 4 + threadIdx.y; r < rows; r += (size_t)gridDim.y * 4) {
        if (r < h) {
            const size_t a = r * w, b = r * G.y_pitch; // planar, NV12
            if (VEC) {
                if (t * 16 >= w) continue; // (w % 16 == 0)
                if (TO_NV12) *reinterpret_cast<uint4 *>(d + b + 16 * t) = *reinterpret_cast<const uint4 *>(s + a + 16 * t);
                else *reinterpret_cast<uint4 *>(d + a + 16 * t) = *reinterpret_cast<const uint4 *>(s + b + 16 * t);
            } else {
                if (t >= w) continue;
                if (TO_NV12) d[b + t] = s[a + t];
                else d[a + t] = s[b + t];
            }
        } else {
            const size_t cy = r - h;
            const size_t a = cy * cw, b = G.uv_offset + cy * G.uv_pitch;
            if (VEC) {
                if (t * 8 >= cw) continue; // (cw % 8 == 0)
                if (TO_NV12) {
                    const uint2 u = *reinterpret_cast<const uint2 *>(s + u_off + a + 8 * t), v = *reinterpret_cast<const uint2 *>(s + v_off + a + 8 * t);
                    *reinterpret_cast<uint4 *>(d + b + 16 * t) = interleave8(u, v);
                } else {
                    uint2 u, v;
                    deinterleave8(*reinterpret_cast<const uint4 *>(s + b + 16 * t), u, v);
                    *reinterpret_cast<uint2 *>(d + u_off + a + 8 * t) = u;
                    *reinterpret_cast<uint2 *>(d + v_off + a + 8 * t) = v;
                }
            } else {
                if (t >= cw) continue;
                if (TO_NV12) d[b + 2 * t] = s[u_off + a + t], d[b + 2 * t + 1] = s[v_off + a + t];
                else d[u_off + a + t] = s[b + 2 * t], d[v_off + a + t] = s[b + 2 * t + 1];
            }
        }
    }
}

// ---- launch -----------------------------------------------------------------------------------------------------------------------

inline bool nv12_layout_ok(uint32_t w, uint32_t h, size_t y_pitch, size_t uv_pitch, size_t uv_offset, size_t fs)
{
    const size_t cw = ((size_t)w + 1) / 2, ch = ((size_t)h + 1) / 2;
    return w && h && y_pitch >= w && uv_pitch >= 2 * cw && uv_offset >= y_pitch * (h - 1) + w && fs >= uv_offset + uv_pitch * (ch - 1) + 2 * cw;
}

inline bool nv12_launch_ok(const Nv12Launch &L)
{
    const YuvLaunch &C = L.c;
    return C.yuv && C.rgba && C.n_frames && (C.siting | 1) == 1 && (C.chroma_filter | 1) == 1 &&
           nv12_layout_ok(C.w, C.h, L.y_pitch, L.uv_pitch, L.uv_offset, C.yuv_frame_stride) && C.rgba_frame_stride >= (size_t)C.w * C.h * 4 &&
           (C.rgba_frame_stride % 4) == 0 && aligned_to(C.rgba, 4) && cdiv((C.h + 1) / 2, 4) <= 65535;
}

// The form of a launch: the aligned kernels where the width fills the thread's run (8 pixels towards RGBA, 16 towards NV12), the
// NV12 base, both pitches, uv_offset and the frame stride keep the run's widest access aligned (8 / 16 bytes), the RGBA side keeps
// its 16-byte accesses aligned and the RGBA frame stays below 4 GiB; else the scalar kernels.
struct Nv12Shape {
    bool vec;
    dim3 grid;
};
inline Nv12Shape nv12_shape(const Nv12Launch &L, bool to_rgba, uint32_t n)
{
    const YuvLaunch &C = L.c;
    const uint32_t run = to_rgba ? 8 : 16;
    const size_t a = run; // the NV12 side's widest access: 8 bytes towards RGBA, 16 towards NV12
    Nv12Shape s;
    s.vec = (C.w % run) == 0 && (uint64_t)C.w * C.h * 4 < ((uint64_t)1 << 32) && aligned_to(C.rgba, 16) && (C.rgba_frame_stride % 16) == 0 &&
            aligned_to(C.yuv, a) && (C.yuv_frame_stride % a) == 0 && (L.y_pitch % a) == 0 && (L.uv_pitch % a) == 0 && (L.uv_offset % a) == 0;
    const uint32_t ch = (C.h + 1) / 2;
    if (s.vec)
        s.grid = dim3(cdiv(C.w / run, kWave), cdiv(ch, 4), n);
    else if (to_rgba)
        s.grid = dim3(cdiv(C.w, kWave), cdiv(C.h, 4) < 65535u ? cdiv(C.h, 4) : 65535u, n);
    else
        s.grid = dim3(cdiv((C.w + 1) / 2, kWave), cdiv(ch, 4), n);
    return s;
}

inline bool repack_vec(const Nv12RepackLaunch &L)
{
    return (L.w % 16) == 0 && aligned_to(L.i420, 16) && aligned_to(L.nv12, 16) && (L.i420_frame_stride % 16) == 0 && (L.nv12_frame_stride % 16) == 0 &&
           (L.y_pitch % 16) == 0 && (L.uv_pitch % 16) == 0 && (L.uv_offset % 16) == 0;
}

template <bool TO_NV12>
hipError_t launch_repack(const Nv12RepackLaunch &L)
{
    const size_t cw = ((size_t)L.w + 1) / 2, ch = ((size_t)L.h + 1) / 2;
    if (!L.i420 || !L.nv12 || !L.n_frames || !nv12_layout_ok(L.w, L.h, L.y_pitch, L.uv_pitch, L.uv_offset, L.nv12_frame_stride) ||
        L.i420_frame_stride < (size_t)L.w * L.h + 2 * cw * ch)
        return hipErrorInvalidValue;
    const bool vec = repack_vec(L);
    const uint64_t rows = (uint64_t)L.h + ch;
    const dim3 grid(cdiv(vec ? L.w / 16 : L.w, kWave), (uint32_t)((rows + 3) / 4 < 65535 ? (rows + 3) / 4 : 65535), 1), block(kWave, 4);
    const Nv12Geom G{L.nv12_frame_stride, L.y_pitch, L.uv_pitch, L.uv_offset};
    return for_grid_z_chunks(L.n_frames, [&](uint32_t done, uint32_t n) {
        const uint8_t *const pl = L.i420 + (size_t)done * L.i420_frame_stride, *const nv = L.nv12 + (size_t)done * L.nv12_frame_stride;
        const uint8_t *const src = TO_NV12 ? pl : nv;
        uint8_t *const dst = const_cast<uint8_t *>(TO_NV12 ? nv : pl);
        const dim3 g(grid.x, grid.y, n);
        if (vec) hipLaunchKernelGGL((k_nv12_repack<TO_NV12, true>), g, block, 0, L.stream, src, dst, L.i420_frame_stride, G, L.w, L.h);
        else hipLaunchKernelGGL((k_nv12_repack<TO_NV12, false>), g, block, 0, L.stream, src, dst, L.i420_frame_stride, G, L.w, L.h);
    });
}

} // namespace

hipError_t launch_nv12_to_rgba(const Nv12Launch &L)
{
    if (!nv12_launch_ok(L)) return hipErrorInvalidValue;
    const YuvTables T = yuv_tables(L.c);
    const Nv12Geom G{L.c.yuv_frame_stride, L.y_pitch, L.uv_pitch, L.uv_offset};
    return for_grid_z_chunks(L.c.n_frames, [&](uint32_t done, uint32_t n) {
        Nv12Launch C = L;
        C.c.yuv = L.c.yuv + (size_t)done * L.c.yuv_frame_stride, C.c.rgba = L.c.rgba + (size_t)done * L.c.rgba_frame_stride;
        const Nv12Shape s = nv12_shape(C, true, n);
        const dim3 block(kWave, 4);
#define NUS_NR(K) {{K<0, 0>, K<0, 1>}, {K<1, 0>, K<1, 1>}}
        static constexpr decltype(&k_nv12_to_rgba<0, 0>) kernels[2][2][2] = {NUS_NR(k_nv12_to_rgba_px), NUS_NR(k_nv12_to_rgba)}; // [vec][filter][siting]
#undef NUS_NR
        hipLaunchKernelGGL(kernels[s.vec][L.c.chroma_filter][L.c.siting], s.grid, block, 0, L.c.stream, static_cast<const uint8_t *>(C.c.yuv), G,
                           C.c.rgba, L.c.rgba_frame_stride, L.c.w, L.c.h, T, L.c.sel);
    });
}

hipError_t launch_rgba_to_nv12(const Nv12Launch &L)
{
    if (!nv12_launch_ok(L)) return hipErrorInvalidValue;
    const YuvTables T = yuv_tables(L.c);
    const Nv12Geom G{L.c.yuv_frame_stride, L.y_pitch, L.uv_pitch, L.uv_offset};
    return for_grid_z_chunks(L.c.n_frames, [&](uint32_t done, uint32_t n) {
        Nv12Launch C = L;
        C.c.yuv = L.c.yuv + (size_t)done * L.c.yuv_frame_stride, C.c.rgba = L.c.rgba + (size_t)done * L.c.rgba_frame_stride;
        const Nv12Shape s = nv12_shape(C, false, n);
        const dim3 block(kWave, 4);
        static constexpr decltype(&k_rgba_to_nv12<0>) kernels[2][2] = {{k_rgba_to_nv12_cell<0>, k_rgba_to_nv12_cell<1>},
                                                                       {k_rgba_to_nv12<0>, k_rgba_to_nv12<1>}}; // [vec][siting]
        hipLaunchKernelGGL(kernels[s.vec][L.c.siting], s.grid, block, 0, L.c.stream, static_cast<const uint8_t *>(C.c.rgba), L.c.rgba_frame_stride,
                           C.c.yuv, G, L.c.w, L.c.h, T, L.c.sel);
    });
}

hipError_t launch_i420_to_nv12(const Nv12RepackLaunch &L) { return launch_repack<true>(L); }
hipError_t launch_nv12_to_i420(const Nv12RepackLaunch &L) { return launch_repack<false>(L); }

} // namespace nus
