// nus_k_yuv_resize.hip -- separable resampling of the 8-bit planes of I420 frame batches (gfx950, wave64): the kernels behind
// nus_yuv420_resize[_device] of include/nuscaler_hip.h, where the contract is written.  BUILD-DEFINED: the reference has no YUV.
//
// The arithmetic is k_resize_rows' (nus_k_resize.hip; image-0.24.9 imageops::resize) on one channel: per output row a vertical
// pass V[col] = sum_j wy[y][j] * in[ly[y] + j][col] in f32, taps ascending, then the horizontal sum of each output's taps, taps
// ascending, clamp to 0 .. 255, round (pack_u8<EXACT>); mac<EXACT> gives the two modes.  What is new is the layout: bytes.
//   k_plane_rows<EXACT, UNION>   blockDim (64, 4): the four waves own four adjacent segments of 256 output columns of the same
//                    block of output rows, each wave with an f32 LDS row of its own (no workgroup barrier).  V pass: a lane reads
//                    one dword -- four input columns -- of every tap row, then converts and accumulates, and stores its four
//                    sums as one 16-byte LDS write.  H pass: a lane owns FOUR adjacent output bytes; their windows overlap almost
//                    entirely on an up-scale, so it reads their union (<= UNION columns) from LDS once and gives every output a
//                    UNION-long weight vector that is zero outside its own window (the extra terms are exact +-0: same bits);
//                    the four bytes leave as one dword store.  No byte access anywhere.
//                    Needs: both widths multiples of 4, every plane of the launch dword aligned on either side, windows of at
//                    most 8 taps, unions of at most 12.  What the public entry points can ask for is less: over every x axis
//                    the row form takes for input widths 4 .. 1100 and output widths in .. 4 in, at either sample position, no
//                    window has more than 7 taps and no union more than 10 columns (Lanczos-3; Catmull-Rom 5 and 8, Triangle 3
//                    and 6; all reached at ratio 1; tests/test_yuv_resize_host.py holds the bound).  So in that range the UNION
//                    = 12 instances are compiled and never launched; they stay until a follow-up removes them on that bound.
//   k_plane_px<EXACT>            one output byte per thread, 64-bit addressing, byte accesses, any tap count: the same operations
//                    in the same order, so the same bytes.  Odd chroma widths, odd plane addresses, offset bases, odd strides.
//   k_frame_copy<T>              equal sizes: the frame is copied, as imageops::resize does.
// The launcher picks the form per plane class (plane_rows_form).  Planes go on grid.z through for_grid_z_chunks: the luma plane
// of every frame in one launch, both chroma planes of every frame (they share their tables) in another.
// The vertical weights of a row are wave-uniform and reach the FMAs through per-lane copies: left in SGPRs they appear as scalar
// operands of every v_fma_f32 of the V pass, which halves the issue rate of those chains (as in k_resize_rows).
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): k_plane_rows FMA / EXACT, UNION 10: 114 / 116 VGPRs, UNION
// 12: 120 / 122 (four waves per SIMD), 60 SGPRs; k_plane_px 23 VGPRs; no scratch in any kernel.  LDS per workgroup: 4 x
// (ncols_max + 16) x 4 bytes, ncols_max the widest dword-aligned input footprint of a segment: 2.5 KB at x2, 4.5 KB at x1.
// Measured: 1080p -> 4K takes 23 us a frame, 0.12 of the stream-copy probe's rate for the same bytes.  Asking
// for row y + 1's dwords and weights ahead of row y's H pass changed nothing (22.9 us, 138 - 144 VGPRs) and was not kept.
#include "nus_device.hpp"

namespace nus {

namespace {

constexpr uint32_t kPlaneSlack = 16; // zeroed LDS entries behind each row: a union window may read past the row's end

struct PlaneGeom { // by value in the kernel arguments
    size_t in_fs, out_fs, in_off, in_step, out_off, out_step;
    uint32_t ppf, z0; // planes per frame; index of the launch's first plane in the batch
    uint32_t iw, ih, ow, oh, stride;
};

__device__ __forceinline__ const uint8_t *plane_in(const uint8_t *in, const PlaneGeom &G)
{
    const uint32_t z = G.z0 + blockIdx.z;
    return in + (size_t)(z / G.ppf) * G.in_fs + G.in_off + (size_t)(z % G.ppf) * G.in_step;
}
__device__ __forceinline__ uint8_t *plane_out(uint8_t *out, const PlaneGeom &G)
{
    const uint32_t z = G.z0 + blockIdx.z;
    return out + (size_t)(z / G.ppf) * G.out_fs + G.out_off + (size_t)(z % G.ppf) * G.out_step;
}

template <bool EXACT, int UNION>
__global__ __launch_bounds__(256) void k_plane_rows(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, PlaneTables T, PlaneGeom G,
                                                    uint32_t rows_per_block, uint32_t ncols_max)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int N = (int)kPlaneRun;
    static_assert(N == 4, "a lane's run is one dword");
    static_assert(UNION >= 8 && UNION <= (int)kPlaneSlack, "the slack behind a row covers a union window");
    float *const s_v = reinterpret_cast<float *>(smem) + (size_t)threadIdx.y * (ncols_max + kPlaneSlack); // (ncols_max % 4 == 0)
    const uint32_t seg = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + threadIdx.y);
    const uint32_t X0 = seg * kPlaneSegment;
    if (X0 >= G.ow) return; // whole wave; no workgroup barriers below
    const uint32_t Xlast = umin(X0 + kPlaneSegment, G.ow) - 1;
    const int32_t cmin = T.lx[X0];
    const int32_t cmax = T.lx[Xlast] + (int32_t)T.nx[Xlast]; // <= iw
    const int32_t c0 = cmin & ~3;                            // the V pass walks whole dwords of the input rows
    const int32_t nrow = ((cmax - c0) + 3) & ~3;             // <= ncols_max (host: YuvResizer::initialize)
    const uint32_t x = X0 + threadIdx.x * N;
    const bool lane_active = x < G.ow; // (ow % 4 == 0: an active lane owns four outputs)
    const uint32_t y_begin = blockIdx.y * rows_per_block;
    const uint32_t y_end = umin(y_begin + rows_per_block, G.oh);
    const uint8_t *const src_plane = plane_in(in, G);
    uint8_t *const dst = plane_out(out, G) + x;

    if (threadIdx.x < kPlaneSlack) s_v[nrow + threadIdx.x] = 0.0f;
    // union window: the weights of output i re-based to the first output's left column
    int32_t hl0;
    float hu[N][UNION];
    {
        int32_t hl[N];
#pragma unroll
        for (int i = 0; i < N; ++i) hl[i] = T.lx[lane_active ? x + i : 0] - c0;
        hl0 = hl[0];
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const uint32_t xo = lane_active ? x + i : 0;
            const int32_t shift = hl[i] - hl[0]; // >= 0: left edges do not decrease with x
#pragma unroll
            for (int j = 0; j < UNION; ++j) {
                const int32_t k = j - shift;
                const float w = T.wx[(size_t)xo * G.stride + (uint32_t)(k < 0 ? 0 : (k > 7 ? 7 : k))];
                hu[i][j] = (k >= 0 && k < 8) ? w : 0.0f;
            }
        }
    }

    for (uint32_t y = y_begin; y < y_end; ++y) {
        const int32_t ly = uniform_load(T.ly, y);
        const uint32_t ny = uniform_load(T.ny, y);
        float wv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            wv[j] = uniform_load(T.wy, (size_t)y * G.stride + j); // zero padded beyond ny
            asm volatile("" : "+v"(wv[j]));                        // VGPR copy: see the head comment
        }
        const uint8_t *const src = src_plane + (size_t)ly * G.iw;
        // V pass: one dword of every tap row per lane per sweep, all requested before the first is consumed
        for (int32_t col = c0 + 4 * (int32_t)threadIdx.x; col < cmax; col += 4 * kWave) {
            uint32_t p[8];
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if ((uint32_t)j < ny) p[j] = *reinterpret_cast<const uint32_t *>(src + (size_t)j * G.iw + col); // wave-uniform branch
            float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if ((uint32_t)j < ny) {
#pragma unroll
                    for (int m = 0; m < 4; ++m) v[m] = mac<EXACT>(v[m], ch_f32(p[j], m), wv[j]);
                }
            }
            *reinterpret_cast<float4 *>(s_v + (col - c0)) = make_float4(v[0], v[1], v[2], v[3]); // (columns < iw: real values)
        }
        // A wave only ever reads the LDS row it wrote itself, and the LDS executes one wave's instructions in order: no workgroup
        // barrier, just keep the compiler from reordering.
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (lane_active) {
            float R[UNION];
#pragma unroll
            for (int j = 0; j < UNION; ++j) R[j] = s_v[hl0 + j];
            uint32_t o = 0;
#pragma unroll
            for (int i = 0; i < N; ++i) {
                float h = 0.0f;
#pragma unroll
                for (int j = 0; j < UNION; ++j) h = mac<EXACT>(h, R[j], hu[i][j]);
                o = pack_u8<EXACT>(h, i, o);
            }
            *reinterpret_cast<uint32_t *>(dst + (size_t)y * G.ow) = o;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); // the next row's V pass overwrites s_v
        __builtin_amdgcn_wave_barrier();
    }
}

// One output byte per thread: for every horizontal tap column the vertical sum first (f32, taps ascending), then the horizontal
// sum -- the operation order of the row kernel and of the two-pass CPU algorithm.  blockDim = (64, 4).
template <bool EXACT>
__global__ __launch_bounds__(256) void k_plane_px(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, PlaneTables T, PlaneGeom G)
{
    const size_t x = (size_t)blockIdx.x * kWave + threadIdx.x, y = (size_t)blockIdx.y * 4 + threadIdx.y;
    if (x >= G.ow || y >= G.oh) return;
    const int32_t lx = T.lx[x], ly = T.ly[y];
    const uint32_t nx = T.nx[x], ny = T.ny[y];
    const float *const wx = T.wx + x * G.stride, *const wy = T.wy + y * G.stride;
    const uint8_t *const src = plane_in(in, G) + (size_t)ly * G.iw + (size_t)lx;
    float h = 0.0f;
    for (uint32_t a = 0; a < nx; ++a) {
        float v = 0.0f;
        for (uint32_t b = 0; b < ny; ++b) v = mac<EXACT>(v, (float)src[(size_t)b * G.iw + a], wy[b]);
        h = mac<EXACT>(h, v, wx[a]);
    }
    plane_out(out, G)[y * G.ow + x] = (uint8_t)pack_u8<EXACT>(h, 0, 0u);
}

template <typename T>
__global__ __launch_bounds__(256) void k_frame_copy(const uint8_t *__restrict__ in, size_t in_fs, uint8_t *__restrict__ out, size_t out_fs,
                                                    size_t units, uint32_t z0)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= units) return;
    const size_t f = (size_t)z0 + blockIdx.z;
    reinterpret_cast<T *>(out + f * out_fs)[i] = reinterpret_cast<const T *>(in + f * in_fs)[i];
}

inline bool dword(const void *p) { return (reinterpret_cast<uintptr_t>(p) % 4) == 0; }

inline bool plane_launch_ok(const PlaneResizeLaunch &L)
{
    return L.in && L.out && L.iw && L.ih && L.ow && L.oh && L.n_frames && (L.planes_per_frame == 1 || L.planes_per_frame == 2) && L.t.lx &&
           L.t.ly && L.t.nx && L.t.ny && L.t.wx && L.t.wy && L.table_stride >= 8 && L.max_taps >= 1 && L.max_taps <= L.table_stride &&
           L.in_frame_stride && L.out_frame_stride && cdiv(L.oh, 4) <= 65535 && (uint64_t)L.n_frames * L.planes_per_frame <= 0xFFFFFFFFull;
}

} // namespace

bool plane_rows_form(const PlaneResizeLaunch &L)
{
    return (L.iw % 4) == 0 && (L.ow % 4) == 0 && dword(L.in) && dword(L.out) && (L.in_frame_stride % 4) == 0 && (L.out_frame_stride % 4) == 0 &&
           (L.in_plane_offset % 4) == 0 && (L.out_plane_offset % 4) == 0 && (L.planes_per_frame == 1 || ((L.in_plane_step % 4) == 0 && (L.out_plane_step % 4) == 0)) &&
           L.max_taps <= 8 && L.union_taps >= 1 && L.union_taps <= kPlaneMaxUnion && L.ncols_max >= 4 && (L.ncols_max % 4) == 0 && L.ncols_max <= 4096;
}

hipError_t launch_plane_resize(const PlaneResizeLaunch &L)
{
    if (!plane_launch_ok(L)) return hipErrorInvalidValue;
    const bool rows = plane_rows_form(L);
    const uint32_t planes = L.n_frames * L.planes_per_frame;
    return for_grid_z_chunks(planes, [&](uint32_t done, uint32_t n) {
        const PlaneGeom G{L.in_frame_stride, L.out_frame_stride, L.in_plane_offset, L.in_plane_step, L.out_plane_offset, L.out_plane_step,
                          L.planes_per_frame, done, L.iw, L.ih, L.ow, L.oh, L.table_stride};
        const dim3 block(kWave, 4);
        if (!rows) {
            const dim3 grid(cdiv(L.ow, kWave), cdiv(L.oh, 4), n);
            if (L.exact) hipLaunchKernelGGL(k_plane_px<true>, grid, block, 0, L.stream, L.in, L.out, L.t, G);
            else hipLaunchKernelGGL(k_plane_px<false>, grid, block, 0, L.stream, L.in, L.out, L.t, G);
            return;
        }
        const uint64_t blocks_x = cdiv(cdiv(L.ow, kPlaneSegment), 4);
        uint64_t rpb = (uint64_t)L.oh * blocks_x * n / 4096; // a few thousand blocks per launch ...
        rpb = rpb < 8 ? 8 : (rpb > 32 ? 32 : rpb);            // ... each with rows enough to amortise its union weights
        const dim3 grid((uint32_t)blocks_x, cdiv(L.oh, (uint32_t)rpb), n);
        const size_t lds = (size_t)4 * (L.ncols_max + kPlaneSlack) * sizeof(float);
#define NUS_PR(E, U) hipLaunchKernelGGL((k_plane_rows<E, U>), grid, block, lds, L.stream, L.in, L.out, L.t, G, (uint32_t)rpb, L.ncols_max)
        if (L.exact) {
            if (L.union_taps <= 10) NUS_PR(true, 10);
            else NUS_PR(true, 12);
        } else {
            if (L.union_taps <= 10) NUS_PR(false, 10);
            else NUS_PR(false, 12);
        }
#undef NUS_PR
    });
}

hipError_t launch_frame_copy(const uint8_t *in, size_t in_frame_stride, uint8_t *out, size_t out_frame_stride, size_t frame_bytes,
                             uint32_t n_frames, hipStream_t stream)
{
    if (!in || !out || !frame_bytes || !n_frames || in_frame_stride < frame_bytes || out_frame_stride < frame_bytes) return hipErrorInvalidValue;
    const bool wide = dword(in) && dword(out) && (in_frame_stride % 4) == 0 && (out_frame_stride % 4) == 0 && (frame_bytes % 4) == 0;
    const size_t units = wide ? frame_bytes / 4 : frame_bytes;
    if ((units + 255) / 256 > 0x7FFFFFFFull) return hipErrorInvalidValue;
    return for_grid_z_chunks(n_frames, [&](uint32_t done, uint32_t n) {
        const dim3 grid((uint32_t)((units + 255) / 256), 1, n);
        if (wide) hipLaunchKernelGGL(k_frame_copy<uint32_t>, grid, dim3(256), 0, stream, in, in_frame_stride, out, out_frame_stride, units, done);
        else hipLaunchKernelGGL(k_frame_copy<uint8_t>, grid, dim3(256), 0, stream, in, in_frame_stride, out, out_frame_stride, units, done);
    });
}

} // namespace nus
