// nus_k_metrics.hip -- image-quality metrics of frame pairs on the GPU (gfx950): MSE, PSNR and SSIM of RGBA8 frames, alpha
// ignored.  ErrorMetrics::calculate (Nu_scale/src/upscale/common.rs:475-543) is the reference for MSE / PSNR; its SSIM is a
// placeholder there, so SSIM follows Wang et al. 2004: per channel on 0..255, 11 x 11 Gaussian window (sigma 1.5, weights
// normalised to 1), population statistics, C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2, averaged over the (W-10) x (H-10) centres
// whose window lies inside the frame and over R, G, B.
//
// Determinism: every launch writes its per-block partials to a workspace (SSE as u64, SSIM as f64), and k_metrics_finish
// adds them in a fixed order.  No float atomics anywhere: the same inputs give the same bytes on every run.
//   k_metrics_sse       MSE only: one streaming read of both frames, 16 B per lane where both frame bases allow it.
//   k_metrics_ssim      SSIM (and the SSE of the same pixels when MSE is asked too): a 64 x 32 tile of valid centres per
//                       workgroup, staged with its 5-pixel halo in LDS; per channel a horizontal 11-tap pass into LDS, then a
//                       vertical 11-tap pass in registers, over the five statistics.
//   k_metrics_finish    one workgroup per frame: [mse, psnr, ssim], NaN for what was not asked.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "nus_kernels.hpp"

namespace nus {

namespace {

typedef unsigned long long u64;

constexpr unsigned kBlock = kMetricsBlock;
constexpr unsigned kSseItems = 8; // 4-pixel items per lane of k_metrics_sse: 32 pixels * 3 * 255^2 fits a u32 partial

// SSIM tile: kTX x kTY valid centres, staged with a kHalo ring; rows of the staged frames padded to a 16-byte multiple
constexpr int kHalo = 5, kTX = 64, kTY = 32;
constexpr int kSX = kTX + 2 * kHalo, kSY = kTY + 2 * kHalo, kSXP = 76;
constexpr int kRunH = 4;  // horizontal pass: outputs per item (reads kRunH + 10 staged pixels)
constexpr int kRunV = 8;  // vertical pass: output rows per lane
constexpr int kItemsH = kSY * (kTX / kRunH);
static_assert(kSXP >= kSX && kSXP % 4 == 0 && (kTX / kRunH) * kRunH == kTX, "tile shape");
static_assert(kTX * (kTY / kRunV) == (int)kBlock, "one vertical run per lane");

// the normalised Gaussian, sigma 1.5, taps -5..5 (the f64 weights rounded to f32; symmetric)
__device__ constexpr float kG[6] = {0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c40p-3f, 0x1.106560p-2f};

__device__ __forceinline__ uint32_t px_sse(uint32_t a, uint32_t b)
{
    const int d0 = (int)(a & 255u) - (int)(b & 255u);
    const int d1 = (int)((a >> 8) & 255u) - (int)((b >> 8) & 255u);
    const int d2 = (int)((a >> 16) & 255u) - (int)((b >> 16) & 255u);
    return (uint32_t)(d0 * d0 + d1 * d1 + d2 * d2);
}

// sum over the workgroup, the same order on every run (xor butterfly per wave, then the waves in index order)
template <typename T>
__device__ T block_sum(T v, T *red)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63u) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    T s = red[0];
#pragma unroll
    for (unsigned k = 1; k < kBlock / 64; ++k) s += red[k];
    return s;
}

// grid: blocks_per_frame * frames; block k of frame f covers the 4-pixel items [k * 2048, (k + 1) * 2048)
__global__ __launch_bounds__(256) void k_metrics_sse(const uint8_t *__restrict__ a, size_t a_stride, const uint8_t *__restrict__ b,
                                                     size_t b_stride, uint32_t npx, uint32_t blocks_per_frame, u64 *__restrict__ part)
{
    __shared__ u64 red[kBlock / 64];
    const uint32_t f = blockIdx.x / blocks_per_frame, k = blockIdx.x - f * blocks_per_frame;
    const uint8_t *pa = a + (size_t)f * a_stride, *pb = b + (size_t)f * b_stride;
    const uint32_t n4 = npx / 4, base = k * (kBlock * kSseItems) + threadIdx.x;
    uint32_t acc = 0;
    if (((reinterpret_cast<uintptr_t>(pa) | reinterpret_cast<uintptr_t>(pb)) & 15u) == 0) {
        const uint4 *qa = reinterpret_cast<const uint4 *>(pa), *qb = reinterpret_cast<const uint4 *>(pb);
        uint4 va[kSseItems], vb[kSseItems];
#pragma unroll
        for (unsigned j = 0; j < kSseItems; ++j) {
            const uint32_t i = base + j * kBlock;
            va[j] = i < n4 ? qa[i] : uint4{0, 0, 0, 0};
            vb[j] = i < n4 ? qb[i] : uint4{0, 0, 0, 0};
        }
#pragma unroll
        for (unsigned j = 0; j < kSseItems; ++j)
            acc += px_sse(va[j].x, vb[j].x) + px_sse(va[j].y, vb[j].y) + px_sse(va[j].z, vb[j].z) + px_sse(va[j].w, vb[j].w);
    } else { // a frame base that is only 4-byte aligned (odd W*H with a tight stride): dword loads
        const uint32_t *wa = reinterpret_cast<const uint32_t *>(pa), *wb = reinterpret_cast<const uint32_t *>(pb);
#pragma unroll
        for (unsigned j = 0; j < kSseItems; ++j) {
            const uint32_t i = base + j * kBlock;
            if (i < n4) {
#pragma unroll
                for (unsigned q = 0; q < 4; ++q) acc += px_sse(wa[4 * i + q], wb[4 * i + q]);
            }
        }
    }
    if (k == 0 && threadIdx.x < (npx & 3u)) { // the last npx % 4 pixels
        const uint32_t *wa = reinterpret_cast<const uint32_t *>(pa), *wb = reinterpret_cast<const uint32_t *>(pb);
        acc += px_sse(wa[4 * n4 + threadIdx.x], wb[4 * n4 + threadIdx.x]);
    }
    const u64 s = block_sum<u64>((u64)acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// keeps a value in a VGPR, so the weight FMAs take VGPR operands only: the repository's instruction-rate probe measured
// v_fmac_f32 with an SGPR operand at 4.3 cycles per wave-instruction against 2.3 with VGPRs (profiles/r01_probe_valu_instruction_
// rates.txt; literal operands were not probed), and v_pk_fma_f32, which hipcc forms from some of these FMAs, needs VGPR
// operands.  What the pinning changes in this kernel's time was not measured.
__device__ __forceinline__ float in_vgpr(float x)
{
    asm volatile("" : "+v"(x));
    return x;
}

// grid: tiles_x * tiles_y * frames.  Staged pixel (r, c) of tile (tx, ty) is frame pixel (tx * kTX + c, ty * kTY + r); the tile's
// centres are the staged pixels kHalo..kHalo + kTX - 1 of rows kHalo..kHalo + kTY - 1 that lie in the frame's valid area.
// WITH_SSE: each frame pixel is counted by exactly one tile -- the centres it holds, plus the outer 5-pixel ring of the frame for
// the tiles on the frame's border.
template <bool WITH_SSE>
__global__ __launch_bounds__(256, 2) void k_metrics_ssim(const uint8_t *__restrict__ a, size_t a_stride, const uint8_t *__restrict__ b,
                                                         size_t b_stride, uint32_t w, uint32_t h, uint32_t tiles_x, uint32_t tiles_y,
                                                         double *__restrict__ ssim_part, u64 *__restrict__ sse_part)
{
    __shared__ __attribute__((aligned(16))) uint32_t sA[kSY][kSXP];
    __shared__ __attribute__((aligned(16))) uint32_t sB[kSY][kSXP];
    __shared__ __attribute__((aligned(16))) float sH[5][kSY][kTX];
    __shared__ double red[kBlock / 64];
    __shared__ u64 red_u[kBlock / 64];

    const uint32_t tiles = tiles_x * tiles_y;
    const uint32_t f = blockIdx.x / tiles, t = blockIdx.x - f * tiles;
    const uint32_t ty = t / tiles_x, tx = t - ty * tiles_x;
    const uint32_t x0 = tx * kTX, y0 = ty * kTY;
    const uint32_t *pa = reinterpret_cast<const uint32_t *>(a + (size_t)f * a_stride);
    const uint32_t *pb = reinterpret_cast<const uint32_t *>(b + (size_t)f * b_stride);

    // pixels whose SSE this tile counts
    const uint32_t own_x0 = tx == 0 ? 0 : x0 + kHalo, own_x1 = tx + 1 == tiles_x ? w : x0 + kHalo + kTX;
    const uint32_t own_y0 = ty == 0 ? 0 : y0 + kHalo, own_y1 = ty + 1 == tiles_y ? h : y0 + kHalo + kTY;
    uint32_t sse = 0;
    for (uint32_t i = threadIdx.x; i < (uint32_t)(kSY * kSX); i += kBlock) {
        const uint32_t r = i / kSX, c = i - r * kSX;
        const uint32_t gx = x0 + c, gy = y0 + r;
        uint32_t va = 0, vb = 0;
        if (gx < w && gy < h) {
            const size_t o = (size_t)gy * w + gx;
            va = pa[o];
            vb = pb[o];
            if (WITH_SSE && gx >= own_x0 && gx < own_x1 && gy >= own_y0 && gy < own_y1) sse += px_sse(va, vb);
        }
        sA[r][c] = va;
        sB[r][c] = vb;
    }
    __syncthreads();

    float g6[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) g6[k] = in_vgpr(kG[k]);
#define NUS_G(tp) g6[(tp) <= 5 ? (tp) : 10 - (tp)]

    const uint32_t lx = threadIdx.x & (kTX - 1), run = threadIdx.x / kTX;
    const bool col_ok = x0 + lx + 2 * kHalo < w;
    double ssim_sum = 0.0;
    for (uint32_t ch = 0; ch < 3; ++ch) {
        const uint32_t sh = 8 * ch;
        // horizontal: item (r, q) filters staged row r for the centre columns kRunH * q .. kRunH * q + kRunH - 1
        for (int it = threadIdx.x; it < kItemsH; it += kBlock) {
            const int r = it / (kTX / kRunH), q = it - r * (kTX / kRunH);
            const uint4 *ra = reinterpret_cast<const uint4 *>(&sA[r][kRunH * q]);
            const uint4 *rb = reinterpret_cast<const uint4 *>(&sB[r][kRunH * q]);
            uint32_t pxa[16], pxb[16];
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const uint4 qa = ra[v], qb = rb[v];
                pxa[4 * v] = qa.x, pxa[4 * v + 1] = qa.y, pxa[4 * v + 2] = qa.z, pxa[4 * v + 3] = qa.w;
                pxb[4 * v] = qb.x, pxb[4 * v + 1] = qb.y, pxb[4 * v + 2] = qb.z, pxb[4 * v + 3] = qb.w;
            }
            float acc[5][kRunH];
#pragma unroll
            for (int s = 0; s < 5; ++s)
#pragma unroll
                for (int o = 0; o < kRunH; ++o) acc[s][o] = 0.0f;
#pragma unroll
            for (int j = 0; j < kRunH + 10; ++j) {
                // offset domain: x - 128 keeps every product and square an exact f32 integer
                const float x = (float)((pxa[j] >> sh) & 255u) - 128.0f, y = (float)((pxb[j] >> sh) & 255u) - 128.0f;
                const float xx = x * x, yy = y * y, xy = x * y;
#pragma unroll
                for (int o = 0; o < kRunH; ++o) {
                    const int tp = j - o;
                    if (tp >= 0 && tp <= 10) {
                        acc[0][o] = __builtin_fmaf(NUS_G(tp), x, acc[0][o]);
                        acc[1][o] = __builtin_fmaf(NUS_G(tp), y, acc[1][o]);
                        acc[2][o] = __builtin_fmaf(NUS_G(tp), xx, acc[2][o]);
                        acc[3][o] = __builtin_fmaf(NUS_G(tp), yy, acc[3][o]);
                        acc[4][o] = __builtin_fmaf(NUS_G(tp), xy, acc[4][o]);
                    }
                }
            }
#pragma unroll
            for (int s = 0; s < 5; ++s)
                *reinterpret_cast<float4 *>(&sH[s][r][kRunH * q]) = float4{acc[s][0], acc[s][1], acc[s][2], acc[s][3]};
        }
        __syncthreads();
        // vertical: lane (lx, run) filters column lx for the centre rows kRunV * run .. kRunV * run + kRunV - 1
        float m[5][kRunV];
#pragma unroll
        for (int s = 0; s < 5; ++s)
#pragma unroll
            for (int o = 0; o < kRunV; ++o) m[s][o] = 0.0f;
#pragma unroll
        for (int j = 0; j < kRunV + 10; ++j) {
            float v[5];
#pragma unroll
            for (int s = 0; s < 5; ++s) v[s] = sH[s][kRunV * run + j][lx];
#pragma unroll
            for (int o = 0; o < kRunV; ++o) {
                const int tp = j - o;
                if (tp >= 0 && tp <= 10) {
#pragma unroll
                    for (int s = 0; s < 5; ++s) m[s][o] = __builtin_fmaf(NUS_G(tp), v[s], m[s][o]);
                }
            }
        }
        __syncthreads(); // sH is rewritten by the next channel
        if (col_ok) {
            const float C1 = 6.5025f, C2 = 58.5225f;
#pragma unroll
            for (int o = 0; o < kRunV; ++o) {
                if (y0 + kRunV * run + o + 2 * kHalo < h) {
                    const float mxo = m[0][o], myo = m[1][o];
                    const float sxx = m[2][o] - mxo * mxo, syy = m[3][o] - myo * myo, sxy = m[4][o] - mxo * myo;
                    const float mx = mxo + 128.0f, my = myo + 128.0f;
                    // 2*mx*my and mx^2 + my^2 from the same rounded means: identical frames give exactly 1
                    const float num = (2.0f * mx * my + C1) * (2.0f * sxy + C2);
                    const float den = (mx * mx + my * my + C1) * (sxx + syy + C2);
                    ssim_sum += (double)(num / den);
                }
            }
        }
    }
#undef NUS_G
    const double s = block_sum<double>(ssim_sum, red);
    if (threadIdx.x == 0) ssim_part[blockIdx.x] = s;
    if (WITH_SSE) {
        const u64 e = block_sum<u64>((u64)sse, red_u);
        if (threadIdx.x == 0) sse_part[blockIdx.x] = e;
    }
}

// one workgroup per frame: the frame's partials in a fixed order (lane-strided, then the block sum)
__global__ __launch_bounds__(256) void k_metrics_finish(const u64 *__restrict__ sse_part, uint32_t sse_blocks,
                                                        const double *__restrict__ ssim_part, uint32_t ssim_blocks, uint32_t w,
                                                        uint32_t h, double *__restrict__ out)
{
    __shared__ u64 red_u[kBlock / 64];
    __shared__ double red[kBlock / 64];
    const uint32_t f = blockIdx.x;
    const double nan = __longlong_as_double(0x7ff8000000000000ll); // positive quiet NaN: prints as "nan"
    double mse = nan, psnr = nan, ssim = nan;
    if (sse_part) {
        u64 e = 0;
        for (uint32_t k = threadIdx.x; k < sse_blocks; k += kBlock) e += sse_part[(size_t)f * sse_blocks + k];
        e = block_sum<u64>(e, red_u);
        // common.rs:494-519: SSE / (3 W H), 20 log10(255 / sqrt(MSE)), +inf at MSE 0
        mse = (double)e / ((double)w * (double)h * 3.0);
        psnr = mse > 0.0 ? 20.0 * log10(255.0 / sqrt(mse)) : __longlong_as_double(0x7ff0000000000000ll);
    }
    if (ssim_part) {
        double s = 0.0;
        for (uint32_t k = threadIdx.x; k < ssim_blocks; k += kBlock) s += ssim_part[(size_t)f * ssim_blocks + k];
        s = block_sum<double>(s, red);
        ssim = s / (3.0 * (double)(w - 10) * (double)(h - 10));
    }
    if (threadIdx.x == 0) {
        out[3 * (size_t)f] = mse;
        out[3 * (size_t)f + 1] = psnr;
        out[3 * (size_t)f + 2] = ssim;
    }
}

} // namespace

MetricsShape metrics_shape(uint32_t w, uint32_t h, uint32_t frames, bool mse, bool ssim)
{
    MetricsShape s;
    const uint64_t n4 = ((uint64_t)w * h) / 4;
    s.sse_blocks = mse && !ssim ? (uint32_t)std::max<uint64_t>(1, (n4 + kBlock * kSseItems - 1) / (kBlock * kSseItems)) : 0;
    if (ssim) {
        s.tiles_x = (w - 10 + kTX - 1) / kTX;
        s.tiles_y = (h - 10 + kTY - 1) / kTY;
        s.ssim_blocks = s.tiles_x * s.tiles_y;
        if (mse) s.sse_blocks = s.ssim_blocks; // the SSE comes out of the SSIM kernel, one partial per tile
    }
    s.sse_offset = 0;
    s.ssim_offset = (size_t)s.sse_blocks * frames * sizeof(u64);
    s.workspace_bytes = s.ssim_offset + (size_t)s.ssim_blocks * frames * sizeof(double);
    return s;
}

hipError_t launch_metrics(const uint8_t *a, size_t a_stride, const uint8_t *b, size_t b_stride, uint32_t w, uint32_t h,
                          uint32_t frames, bool mse, bool ssim, void *workspace, double *out, hipStream_t stream)
{
    const MetricsShape s = metrics_shape(w, h, frames, mse, ssim);
    u64 *sse_part = mse ? reinterpret_cast<u64 *>(static_cast<uint8_t *>(workspace) + s.sse_offset) : nullptr;
    double *ssim_part = ssim ? reinterpret_cast<double *>(static_cast<uint8_t *>(workspace) + s.ssim_offset) : nullptr;
    if (ssim) {
        const dim3 grid(s.ssim_blocks * frames);
        if (mse) hipLaunchKernelGGL(k_metrics_ssim<true>, grid, dim3(kBlock), 0, stream, a, a_stride, b, b_stride, w, h, s.tiles_x,
                                    s.tiles_y, ssim_part, sse_part);
        else hipLaunchKernelGGL(k_metrics_ssim<false>, grid, dim3(kBlock), 0, stream, a, a_stride, b, b_stride, w, h, s.tiles_x,
                                s.tiles_y, ssim_part, sse_part);
    } else {
        hipLaunchKernelGGL(k_metrics_sse, dim3(s.sse_blocks * frames), dim3(kBlock), 0, stream, a, a_stride, b, b_stride, w * h,
                           s.sse_blocks, sse_part);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_metrics_finish, dim3(frames), dim3(kBlock), 0, stream, sse_part, s.sse_blocks, ssim_part, s.ssim_blocks, w,
                       h, out);
    return hipGetLastError();
}

} // namespace nus
