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
//                       workgroup, staged with its 5-pixel halo in LDS; per channel and for each of the five statistics in turn a
//                       horizontal 11-tap pass into one f64 plane in LDS, then a vertical 11-tap pass in registers.  The
//                       statistics and sigma_xx, sigma_yy, sigma_xy are f64: in f32 their cancellation against C2 cost up to
//                       1.2e-4 of SSIM on flat frames (Precision); the ratio is f32.
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

// keeps a value in VGPRs, so the weight FMAs take VGPR operands only: the repository's instruction-rate probe measured
// v_fmac_f32 with an SGPR operand at 4.3 cycles per wave-instruction against 2.3 with VGPRs (profiles/r01_probe_valu_instruction_
// rates.txt; v_fma_f64 was not probed).  What the pinning changes in this kernel's time was not measured.
__device__ __forceinline__ double in_vgpr(double x)
{
    asm volatile("" : "+v"(x));
    return x;
}

#define NUS_G(tp) g6[(tp) <= 5 ? (tp) : 10 - (tp)]

// One of the five window statistics of one channel over the whole tile, in f64: S = 0..4 is x, y, x^2, y^2, xy of the channel at
// bit `sh`.  Horizontal 11-tap pass of the staged rows into sH, then the vertical pass of column lx into m[0..kRunV).  The weights
// are f32 values (24 bits) and the pixel terms integers below 2^16, so every product and every horizontal sum is exact in f64 (a
// multiple of 2^-33 below 2^16: 49 bits); the vertical FMAs round at 2^-53 relative, eight decimal digits below what the
// differences E[x^2] - mu^2 need against C2.  Ends with a barrier: sH is free for the next statistic.
template <int S>
__device__ __forceinline__ void ssim_stat(const uint32_t (*sA)[kSXP], const uint32_t (*sB)[kSXP], double (*sH)[kTX], uint32_t sh,
                                          const double (&g6)[6], uint32_t lx, uint32_t run, double (&m)[kRunV])
{
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
        double acc[kRunH];
#pragma unroll
        for (int o = 0; o < kRunH; ++o) acc[o] = 0.0;
#pragma unroll
        for (int j = 0; j < kRunH + 10; ++j) {
            const uint32_t x = (pxa[j] >> sh) & 255u, y = (pxb[j] >> sh) & 255u;
            const double v = (double)(S == 0 ? x : S == 1 ? y : S == 2 ? x * x : S == 3 ? y * y : x * y);
#pragma unroll
            for (int o = 0; o < kRunH; ++o) {
                const int tp = j - o;
                if (tp >= 0 && tp <= 10) acc[o] = __builtin_fma(NUS_G(tp), v, acc[o]);
            }
        }
        *reinterpret_cast<double2 *>(&sH[r][kRunH * q]) = double2{acc[0], acc[1]};
        *reinterpret_cast<double2 *>(&sH[r][kRunH * q + 2]) = double2{acc[2], acc[3]};
    }
    __syncthreads();
    // vertical: lane (lx, run) filters column lx for the centre rows kRunV * run .. kRunV * run + kRunV - 1
#pragma unroll
    for (int o = 0; o < kRunV; ++o) m[o] = 0.0;
#pragma unroll
    for (int j = 0; j < kRunV + 10; ++j) {
        const double v = sH[kRunV * run + j][lx];
#pragma unroll
        for (int o = 0; o < kRunV; ++o) {
            const int tp = j - o;
            if (tp >= 0 && tp <= 10) m[o] = __builtin_fma(NUS_G(tp), v, m[o]);
        }
    }
    __syncthreads();
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
    __shared__ __attribute__((aligned(16))) double sH[kSY][kTX]; // one statistic at a time
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

    double g6[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) g6[k] = in_vgpr((double)kG[k]);

    const uint32_t lx = threadIdx.x & (kTX - 1), run = threadIdx.x / kTX;
    const bool col_ok = x0 + lx + 2 * kHalo < w;
    double ssim_sum = 0.0;
    for (uint32_t ch = 0; ch < 3; ++ch) {
        const uint32_t sh = 8 * ch;
        double mx[kRunV], my[kRunV], mxx[kRunV], myy[kRunV], mxy[kRunV];
        ssim_stat<0>(sA, sB, sH, sh, g6, lx, run, mx);
        ssim_stat<1>(sA, sB, sH, sh, g6, lx, run, my);
        ssim_stat<2>(sA, sB, sH, sh, g6, lx, run, mxx);
        ssim_stat<3>(sA, sB, sH, sh, g6, lx, run, myy);
        ssim_stat<4>(sA, sB, sH, sh, g6, lx, run, mxy);
        if (col_ok) {
            const float C1 = 6.5025f, C2 = 58.5225f;
#pragma unroll
            for (int o = 0; o < kRunV; ++o) {
                if (y0 + kRunV * run + o + 2 * kHalo < h) {
                    // the three differences in f64 (in f32 they miss float64 by up to 1.2e-4 of SSIM on flat frames), then
                    // rounded once; the ratio itself is f32
                    const float sxx = (float)(mxx[o] - mx[o] * mx[o]), syy = (float)(myy[o] - my[o] * my[o]);
                    const float sxy = (float)(mxy[o] - mx[o] * my[o]);
                    const float ux = (float)mx[o], uy = (float)my[o];
                    // 2*ux*uy and ux^2 + uy^2 from the same rounded means: identical frames give exactly 1
                    const float num = (2.0f * ux * uy + C1) * (2.0f * sxy + C2);
                    const float den = (ux * ux + uy * uy + C1) * (sxx + syy + C2);
                    ssim_sum += (double)(num / den);
                }
            }
        }
    }
    const double s = block_sum<double>(ssim_sum, red);
    if (threadIdx.x == 0) ssim_part[blockIdx.x] = s;
    if (WITH_SSE) {
        const u64 e = block_sum<u64>((u64)sse, red_u);
        if (threadIdx.x == 0) sse_part[blockIdx.x] = e;
    }
}
#undef NUS_G

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
