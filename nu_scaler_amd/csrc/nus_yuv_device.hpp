// nus_yuv_device.hpp -- the per-pixel arithmetic of the YUV 4:2:0 <-> RGBA8 kernels (the integer contract of include/nuscaler_hip.h,
// "YUV 4:2:0 frames"), shared by the units that differ only in where the chroma bytes lie: nus_k_yuv.hip (I420: planes) and
// nus_k_nv12.hip (NV12: U,V pairs).  All arithmetic is int32 in Q14 (S = 14, one rounding per output byte).  Device code only.
#pragma once

#include "nus_device.hpp"

namespace nus {

namespace {

constexpr int kYuvS = 14, kYuvH = 1 << 13;

struct YuvTables { // by value in the kernel arguments
    int32_t yuv[9]; // Yc, Uc, Vc rows over (R, G, B)
    int32_t rgb[5]; // cy, rv, bu, gu, gv
    int32_t yo;
};

// per-lane copies of the wave-uniform tables (scalar operands halve the VALU issue rate on gfx950)
__device__ __forceinline__ void lane_copies(YuvTables &T)
{
#pragma unroll
    for (int i = 0; i < 9; ++i) asm volatile("" : "+v"(T.yuv[i]));
#pragma unroll
    for (int i = 0; i < 5; ++i) asm volatile("" : "+v"(T.rgb[i]));
    asm volatile("" : "+v"(T.yo));
}

__device__ __forceinline__ uint32_t clamp8(int v) { return (uint32_t)clampi(v, 0, 255); }

// One RGBA pixel (R in byte 0, alpha 255) from a luma byte and the chroma (u, v): code values minus 128 (LG = 0, nearest), or the
// bilinear sums of weight 16 minus 16 * 128 (LG = 4).  One rounding per channel.
template <int LG>
__device__ __forceinline__ uint32_t yuv_pixel(int y, int u, int v, const YuvTables &T)
{
    const int base = T.rgb[0] * (y - T.yo) * (1 << LG) + (kYuvH << LG);
    int r = (base + T.rgb[1] * v) >> (kYuvS + LG);
    int g = (base + T.rgb[3] * u + T.rgb[4] * v) >> (kYuvS + LG);
    int b = (base + T.rgb[2] * u) >> (kYuvS + LG);
    // The shifts stay apart from the clamps: left together, the compiler joins two of them into one v_ashr_pk_u8_i32 and ORs the
    // third byte into its result as if the upper half of that result were zero -- on the MI355X the pixels then came out with
    // B | (bits 23:16 of G's sum) in the third byte.
    asm volatile("" : "+v"(r), "+v"(g), "+v"(b));
    return clamp8(r) | (clamp8(g) << 8) | (clamp8(b) << 16) | 0xff000000u;
}

// The horizontal step of the bilinear chroma for luma column x of cell c: `l`, `m`, `r` are the (vertically filtered, weight 4)
// values of cells c - 1, c, c + 1.
template <int SITING>
__device__ __forceinline__ int chroma_h(bool odd, int l, int m, int r)
{
    if (SITING == 0) return odd ? 3 * m + r : l + 3 * m; // centre: the luma pair straddles the cell's sample
    return odd ? 2 * m + 2 * r : 4 * m;                  // left: the even luma column is the cell's sample
}

__device__ __forceinline__ int luma_of(uint32_t p, const YuvTables &T)
{
    const int r = p & 0xff, g = (p >> 8) & 0xff, b = (p >> 16) & 0xff;
    return (int)clamp8(((T.yuv[0] * r + T.yuv[1] * g + T.yuv[2] * b + kYuvH) >> kYuvS) + T.yo);
}

// U (ROW = 1) or V (ROW = 2) of one cell from its tap sums: rb = SR | SB << 16, g = SG; the weights total 1 << LGW.
template <int ROW, int LGW>
__device__ __forceinline__ uint32_t chroma_of(uint32_t rb, uint32_t g, const YuvTables &T)
{
    const int sr = rb & 0xffff, sb = rb >> 16;
    return clamp8(((T.yuv[3 * ROW] * sr + T.yuv[3 * ROW + 1] * (int)g + T.yuv[3 * ROW + 2] * sb + (kYuvH << LGW)) >> (kYuvS + LGW)) + 128);
}

__device__ __forceinline__ uint32_t byte_of(uint32_t v, int i) { return (v >> (8 * i)) & 0xffu; }

inline bool aligned_to(const void *p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) % n) == 0; }

inline YuvTables yuv_tables(const YuvLaunch &L)
{
    YuvTables T;
    for (int i = 0; i < 9; ++i) T.yuv[i] = L.to_yuv[i];
    for (int i = 0; i < 5; ++i) T.rgb[i] = L.to_rgb[i];
    T.yo = L.y_offset;
    return T;
}

} // namespace

} // namespace nus
