// nus_k_scene.hip -- scene-cut detection of RGBA8 frame pairs and the cut-aware output rule (gfx950); nus_scene_* of
// include/nuscaler_hip.h, where the contract is written.  Build-defined: the reference has no such stage (its GUI interpolates
// every pair, nu_scaler_py/nu_scaler/main.py:999-1008).  Integer work throughout, no float anywhere, no global atomics: per-
// workgroup partials go to a workspace and k_scene_finish adds them, so the same inputs give the same bytes on every run, at
// every batch position and for every batch size.
//   k_scene_measure  one streaming read of both frames, 16 B per lane where both frame bases allow it: the SAD of R, G, B with
//                    v_sad_u8 (alpha masked), the luma bin (Y >> 3) of every pixel of A and of B with one v_dot4_u32_u8 and a
//                    shift.  Histogram: 64 bins x 64 lane-private columns in LDS (16 KiB), bumped with ds_add_u32: lanes of a
//                    wave never share an address or, within a 32-lane half, a bank; the four waves of the workgroup share
//                    the columns, hence the atomic.  (Dev macro NUS_SCENE_HIST_BALLOT=1 builds the form it was measured
//                    against: per bin a ballot and a popcount into wave-uniform counters, 32 compares per pixel; DESIGN.md
//                    8.6 has both numbers.)  Per workgroup: u64 SAD and 2 x 32 u32 bins.
//   k_scene_finish   one workgroup per pair: the partials, hist_l1, the decision in 64-bit integer products, measures and flag.
//   k_scene_apply    flag-conditional copy: a workgroup whose pair is not cut leaves after one flag load; a cut pair's frame k
//                    is A (time < 0.5) or B through the input selector, 16 B per lane where the bases allow it.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "nus_device.hpp"
#include "nus_kernels.hpp"

namespace nus {

namespace {

typedef unsigned long long u64;

constexpr unsigned kBlock = kSceneBlock;
constexpr unsigned kItems = 8;                        // 4-pixel items per lane of k_scene_measure: 32 pixels * 765 fits a u32
constexpr unsigned kMeasurePixels = kBlock * kItems * 4; // pixels of one frame per measure workgroup
constexpr unsigned kApplyPixels = kBlock * 16;        // pixels per apply workgroup
#ifndef NUS_SCENE_HIST_BALLOT
#define NUS_SCENE_HIST_BALLOT 0 // dev macro, A/B timing only: 1 builds the ballot / popcount histogram instead of the LDS columns
#endif
constexpr bool kBallot = NUS_SCENE_HIST_BALLOT != 0;

// luma bin of one pixel: Y = (77 R + 150 G + 29 B + 128) >> 8, bin = Y >> 3 = (sum + 128) >> 11.  `wsel` holds the weights of
// bytes 0..3 (alpha 0), so a BGR order swaps the outer two.
__device__ __forceinline__ uint32_t luma_bin(uint32_t p, uint32_t wsel)
{
    return __builtin_amdgcn_udot4(p, wsel, 128u, false) >> 11;
}

__device__ __forceinline__ void count_px(uint32_t p, bool valid, uint32_t wsel, uint32_t *col, uint32_t (&cnt)[32])
{
    const uint32_t bin = luma_bin(p, wsel);
    if (!kBallot) {
        if (valid) atomicAdd(col + bin * 64u, 1u); // LDS: ds_add_u32, the value is not read back
    } else {
        const uint32_t bv = valid ? bin : 32u;
#pragma unroll
        for (uint32_t k = 0; k < 32; ++k) cnt[k] += (uint32_t)__popcll(__ballot(bv == k));
    }
}

__device__ __forceinline__ u64 block_sum_u64(u64 v, u64 *red)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63u) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    u64 s = red[0];
#pragma unroll
    for (unsigned k = 1; k < kBlock / 64; ++k) s += red[k];
    return s;
}

// grid: blocks_per_pair * n_pairs; block k of pair i covers the 4-pixel items [k * 2048, (k + 1) * 2048) of both frames.
// part_sad[block], part_hist[block][64]: bins 0..31 of A, then of B.
__global__ __launch_bounds__(256) void k_scene_measure(const uint8_t *__restrict__ a, size_t a_stride, const uint8_t *__restrict__ b,
                                                       size_t b_stride, uint32_t npx, uint32_t blocks_per_pair, uint32_t wsel,
                                                       u64 *__restrict__ part_sad, uint32_t *__restrict__ part_hist)
{
    __shared__ uint32_t s_hist[kBallot ? (kBlock / 64) * 64 : 64 * 64];
    __shared__ u64 red[kBlock / 64];
    const uint32_t pr = blockIdx.x / blocks_per_pair, k = blockIdx.x - pr * blocks_per_pair;
    const uint8_t *pa = a + (size_t)pr * a_stride, *pb = b + (size_t)pr * b_stride;
    const uint32_t *wa = reinterpret_cast<const uint32_t *>(pa), *wb = reinterpret_cast<const uint32_t *>(pb);
    const uint32_t n4 = npx / 4, base = k * (kBlock * kItems) + threadIdx.x, lane = threadIdx.x & 63u;
    if (!kBallot) {
#pragma unroll
        for (unsigned j = 0; j < 16; ++j) s_hist[threadIdx.x + j * kBlock] = 0;
        __syncthreads();
    }
    uint32_t *const col_a = s_hist + lane, *const col_b = s_hist + 32 * 64 + lane; // COLUMNS: [bin][lane]
    uint32_t cnt_a[32], cnt_b[32];
#pragma unroll
    for (int q = 0; q < 32; ++q) cnt_a[q] = cnt_b[q] = 0;

    uint4 va[kItems], vb[kItems];
    if (((reinterpret_cast<uintptr_t>(pa) | reinterpret_cast<uintptr_t>(pb)) & 15u) == 0) {
        const uint4 *qa = reinterpret_cast<const uint4 *>(pa), *qb = reinterpret_cast<const uint4 *>(pb);
#pragma unroll
        for (unsigned j = 0; j < kItems; ++j) {
            const uint32_t i = base + j * kBlock;
            va[j] = i < n4 ? qa[i] : uint4{0, 0, 0, 0};
            vb[j] = i < n4 ? qb[i] : uint4{0, 0, 0, 0};
        }
    } else { // a frame base that is only 4-byte aligned (odd W*H with a tight stride): dword loads
#pragma unroll
        for (unsigned j = 0; j < kItems; ++j) {
            const uint32_t i = base + j * kBlock;
            va[j] = vb[j] = uint4{0, 0, 0, 0};
            if (i < n4) {
                va[j] = uint4{wa[4 * i], wa[4 * i + 1], wa[4 * i + 2], wa[4 * i + 3]};
                vb[j] = uint4{wb[4 * i], wb[4 * i + 1], wb[4 * i + 2], wb[4 * i + 3]};
            }
        }
    }
    uint32_t sad = 0;
#pragma unroll
    for (unsigned j = 0; j < kItems; ++j) {
        const bool ok = base + j * kBlock < n4;
        const uint32_t xa[4] = {va[j].x, va[j].y, va[j].z, va[j].w}, xb[4] = {vb[j].x, vb[j].y, vb[j].z, vb[j].w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            sad = __builtin_amdgcn_sad_u8(xa[q] & 0x00FFFFFFu, xb[q] & 0x00FFFFFFu, sad);
            count_px(xa[q], ok, wsel, col_a, cnt_a);
            count_px(xb[q], ok, wsel, col_b, cnt_b);
        }
    }
    if (k == 0 && (npx & 3u)) { // the last npx % 4 pixels
        const bool ok = threadIdx.x < (npx & 3u);
        const uint32_t xa = ok ? wa[4 * n4 + threadIdx.x] : 0u, xb = ok ? wb[4 * n4 + threadIdx.x] : 0u;
        sad = __builtin_amdgcn_sad_u8(xa & 0x00FFFFFFu, xb & 0x00FFFFFFu, sad);
        count_px(xa, ok, wsel, col_a, cnt_a);
        count_px(xb, ok, wsel, col_b, cnt_b);
    }
    const u64 s = block_sum_u64((u64)sad, red);
    if (threadIdx.x == 0) part_sad[blockIdx.x] = s;

    uint32_t *const ph = part_hist + (size_t)blockIdx.x * 64;
    if (!kBallot) {
        __syncthreads();
        // four lanes per bin, 16 columns each (rotated by the bin: the 16 bins of a 32-lane half read 16 different banks)
        const uint32_t bin = threadIdx.x >> 2, q = threadIdx.x & 3u;
        uint32_t v = 0;
#pragma unroll
        for (uint32_t j = 0; j < 16; ++j) v += s_hist[bin * 64 + q * 16 + ((j + bin) & 15u)];
        v += __shfl_xor(v, 1);
        v += __shfl_xor(v, 2);
        if (q == 0) ph[bin] = v;
    } else {
        uint32_t v = 0; // lane l takes counter l of its wave (compare-selects: a lane-indexed read of the array would go to scratch)
#pragma unroll
        for (uint32_t q = 0; q < 32; ++q) {
            v = lane == q ? cnt_a[q] : v;
            v = lane == q + 32 ? cnt_b[q] : v;
        }
        s_hist[threadIdx.x] = v;
        __syncthreads();
        if (threadIdx.x < 64) ph[threadIdx.x] = s_hist[threadIdx.x] + s_hist[64 + threadIdx.x] + s_hist[128 + threadIdx.x] + s_hist[192 + threadIdx.x];
    }
}

// one workgroup per pair.  cut <=> sad >= mad_threshold * 3 W H and hist_l1 * 1000 >= hist_permille * 2 W H, in 64-bit integers.
__global__ __launch_bounds__(256) void k_scene_finish(const u64 *__restrict__ part_sad, const uint32_t *__restrict__ part_hist,
                                                      uint32_t blocks_per_pair, uint32_t npx, uint32_t mad_threshold,
                                                      uint32_t hist_permille, uint32_t *__restrict__ measures, uint8_t *__restrict__ cut)
{
    __shared__ u64 red[kBlock / 64];
    __shared__ uint32_t s_h[kBlock];
    const uint32_t pr = blockIdx.x;
    const size_t first = (size_t)pr * blocks_per_pair;
    u64 e = 0;
    for (uint32_t k = threadIdx.x; k < blocks_per_pair; k += kBlock) e += part_sad[first + k];
    e = block_sum_u64(e, red);
    const uint32_t bin = threadIdx.x & 63u;
    uint32_t v = 0;
    for (uint32_t k = threadIdx.x >> 6; k < blocks_per_pair; k += kBlock / 64) v += part_hist[(first + k) * 64 + bin];
    s_h[threadIdx.x] = v;
    __syncthreads();
    if (threadIdx.x < 64) { // wave 0
        const uint32_t hsum = s_h[bin] + s_h[64 + bin] + s_h[128 + bin] + s_h[192 + bin]; // bins of A in lanes 0..31, of B in 32..63
        const uint32_t other = __shfl_xor(hsum, 32);
        uint32_t d = bin < 32 ? (hsum > other ? hsum - other : other - hsum) : 0u;
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) d += __shfl_xor(d, o);
        if (threadIdx.x == 0) {
            const bool is_cut = e >= (u64)mad_threshold * 3ull * npx && (u64)d * 1000ull >= (u64)hist_permille * 2ull * npx;
            if (measures) {
                uint32_t *m = measures + 4 * (size_t)pr; // {u64 sad, u32 hist_l1, u32 reserved}
                m[0] = (uint32_t)e;
                m[1] = (uint32_t)(e >> 32);
                m[2] = d;
                m[3] = 0;
            }
            cut[pr] = is_cut ? 1 : 0;
        }
    }
}

// grid: blocks_per_pair * n_pairs; block k of pair i covers pixels [k * 4096, (k + 1) * 4096) of every frame of the pair.
// from_a: bit j set = frame j is a copy of A (its time is below one half), else of B.
__global__ __launch_bounds__(256) void k_scene_apply(const uint8_t *__restrict__ a, size_t a_stride, const uint8_t *__restrict__ b,
                                                     size_t b_stride, const uint8_t *__restrict__ cut, uint8_t *__restrict__ out,
                                                     size_t out_pair_stride, uint32_t npx, uint32_t blocks_per_pair, uint32_t n_times,
                                                     uint32_t from_a, uint32_t sel)
{
    const uint32_t pr = blockIdx.x / blocks_per_pair, k = blockIdx.x - pr * blocks_per_pair;
    if (cut[pr] == 0) return;
    const uint8_t *pa = a + (size_t)pr * a_stride, *pb = b + (size_t)pr * b_stride;
    uint8_t *po = out + (size_t)pr * out_pair_stride;
    const bool need_a = from_a != 0, need_b = (from_a ^ ((1u << n_times) - 1u)) != 0;
    if ((((reinterpret_cast<uintptr_t>(pa) | reinterpret_cast<uintptr_t>(pb) | reinterpret_cast<uintptr_t>(po)) & 15u) == 0) &&
        (npx & 3u) == 0) {
        const uint4 *qa = reinterpret_cast<const uint4 *>(pa), *qb = reinterpret_cast<const uint4 *>(pb);
        const uint32_t n4 = npx / 4;
#pragma unroll
        for (unsigned j = 0; j < 4; ++j) {
            const uint32_t i = k * (kApplyPixels / 4) + threadIdx.x + j * kBlock;
            if (i < n4) {
                const uint4 va = need_a ? swz4(qa[i], sel) : uint4{0, 0, 0, 0}, vb = need_b ? swz4(qb[i], sel) : uint4{0, 0, 0, 0};
                for (uint32_t f = 0; f < n_times; ++f) {
                    uint4 *dst = reinterpret_cast<uint4 *>(po + (size_t)f * npx * 4) + i;
                    if ((from_a >> f) & 1u) *dst = va;
                    else *dst = vb;
                }
            }
        }
    } else {
        const uint32_t *wa = reinterpret_cast<const uint32_t *>(pa), *wb = reinterpret_cast<const uint32_t *>(pb);
#pragma unroll 1
        for (unsigned j = 0; j < 16; ++j) {
            const uint32_t i = k * kApplyPixels + threadIdx.x + j * kBlock;
            if (i < npx) {
                const uint32_t va = need_a ? swz(wa[i], sel) : 0u, vb = need_b ? swz(wb[i], sel) : 0u;
                for (uint32_t f = 0; f < n_times; ++f)
                    reinterpret_cast<uint32_t *>(po + (size_t)f * npx * 4)[i] = ((from_a >> f) & 1u) ? va : vb;
            }
        }
    }
}

} // namespace

SceneShape scene_shape(uint32_t w, uint32_t h, uint32_t n_pairs)
{
    SceneShape s;
    const uint64_t npx = (uint64_t)w * h;
    s.measure_blocks = (uint32_t)std::max<uint64_t>(1, (npx + kMeasurePixels - 1) / kMeasurePixels);
    s.apply_blocks = (uint32_t)std::max<uint64_t>(1, (npx + kApplyPixels - 1) / kApplyPixels);
    s.sad_offset = 0;
    s.hist_offset = (size_t)s.measure_blocks * n_pairs * sizeof(u64);
    s.workspace_bytes = s.hist_offset + (size_t)s.measure_blocks * n_pairs * 64 * sizeof(uint32_t);
    return s;
}

hipError_t launch_scene_detect(const SceneLaunch &L, uint32_t mad_threshold, uint32_t hist_permille, void *workspace, void *measures,
                               uint8_t *cut)
{
    const SceneShape s = scene_shape(L.w, L.h, L.n_pairs);
    u64 *part_sad = reinterpret_cast<u64 *>(static_cast<uint8_t *>(workspace) + s.sad_offset);
    uint32_t *part_hist = reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(workspace) + s.hist_offset);
    const bool bgr = L.format == 1 || L.format == 3; // nus_pixel_format: the weights of bytes 0 and 2 change places
    const uint32_t wsel = bgr ? (29u | 150u << 8 | 77u << 16) : (77u | 150u << 8 | 29u << 16);
    const dim3 grid(s.measure_blocks * L.n_pairs);
    hipLaunchKernelGGL(k_scene_measure, grid, dim3(kBlock), 0, L.stream, L.a, L.a_stride, L.b, L.b_stride, L.w * L.h, s.measure_blocks,
                       wsel, part_sad, part_hist);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_scene_finish, dim3(L.n_pairs), dim3(kBlock), 0, L.stream, part_sad, part_hist, s.measure_blocks, L.w * L.h,
                       mad_threshold, hist_permille, static_cast<uint32_t *>(measures), cut);
    return hipGetLastError();
}

hipError_t launch_scene_apply(const SceneLaunch &L, uint32_t n_times, uint32_t from_a, const uint8_t *cut, uint8_t *out,
                              size_t out_pair_stride)
{
    const SceneShape s = scene_shape(L.w, L.h, L.n_pairs);
    hipLaunchKernelGGL(k_scene_apply, dim3(s.apply_blocks * L.n_pairs), dim3(kBlock), 0, L.stream, L.a, L.a_stride, L.b, L.b_stride, cut,
                       out, out_pair_stride, L.w * L.h, s.apply_blocks, n_times, from_a, input_selector(L.format));
    return hipGetLastError();
}

} // namespace nus
