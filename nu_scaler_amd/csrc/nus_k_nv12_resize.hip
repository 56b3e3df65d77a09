// nus_k_nv12_resize.hip -- separable resampling of the plane of interleaved U,V byte pairs of tight NV12 frame batches (gfx950,
// wave64): the chroma launch behind nus_nv12_resize[_device] of include/nuscaler_hip.h.  The luma plane of an NV12 frame sits
// where it sits in I420 and goes through nus_k_yuv_resize.hip unchanged.  BUILD-DEFINED: the reference has no YUV.
//
// The arithmetic and its order are nus_k_yuv_resize.hip's: per output row a vertical pass in f32, taps ascending, then the
// horizontal sum of each output's taps, taps ascending, then pack_u8<EXACT>.  U and V share their tables, so the output is that
// unit's output on the two de-interleaved planes, interleaved again, bit for bit in both modes.
//   k_pair_rows<EXACT, UNION>    k_plane_rows on byte pairs.  blockDim (64, 4): the four waves own four adjacent segments of 128
//                    output pairs (256 output bytes) of the same block of output rows, each wave with an f32 LDS row of its own
//                    (no workgroup barrier).  V pass: channel-blind -- the existing V pass over a row of 2 iw bytes: a lane reads
//                    one dword (two input pairs) of every tap row, accumulates, and stores its four sums as one 16-byte LDS
//                    write.  H pass: a lane owns four adjacent output bytes, now TWO pairs; it reads the union of the two pairs'
//                    windows (<= UNION cells, both channels: one 8-byte LDS read per cell) and sums each of its four outputs over
//                    a UNION-long weight vector, zero outside the pair's own window (exact +-0 terms: same bits), that the
//                    pair's U and V share; the four bytes leave as one dword store.  No byte access anywhere.
//                    Needs: 2 iw and 2 ow multiples of 4, the pair plane of every frame dword aligned on either side, windows
//                    of at most 8 taps, unions of at most 8.  Over every chroma x axis the row form takes for luma input widths
//                    4 .. 1100 and output widths in .. 4 in, at either sample position, no window has more than 7 taps and no
//                    two-pair union more than 8 cells (Lanczos-3 8, Catmull-Rom 6, Triangle 4: taps + 1;
//                    tests/test_nv12_host.py holds the scan), so UNION = 8 is the one instance compiled per mode.
//   k_pair_px<EXACT>             one output byte per thread, 64-bit addressing, byte accesses, any tap count: k_plane_px with the
//                    tap columns 2 bytes apart and the channel taken from the byte's parity.  Any alignment.
// Frames go on grid.z through for_grid_z_chunks.  The vertical weights reach the FMAs through per-lane copies, as in k_plane_rows.
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): see tests/test_nv12_asm.py -- k_pair_rows stays within 128 VGPRs
// (four waves per SIMD), no scratch, no static LDS.  LDS per workgroup: 4 x (ncols_max + 16) x 4 bytes, ncols_max the widest
// dword-aligned input footprint of a segment in bytes.
#include "nus_device.hpp"

namespace nus {

namespace {

constexpr uint32_t kPairSlack = 16; // zeroed LDS entries behind each row: a union window may read past the row's end (2 x UNION)

struct PairGeom { // by value in the kernel arguments
    size_t in_fs, out_fs, in_off, out_off;
    uint32_t z0;               // index of the launch's first frame in the batch
    uint32_t ib, ih, ob, oh;   // row lengths in BYTES (2 x cells), heights
    uint32_t stride;
};

template <bool EXACT, int UNION>
__global__ __launch_bounds__(256) void k_pair_rows(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, PlaneTables T, PairGeom G,
                                                   uint32_t rows_per_block, uint32_t ncols_max)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int N = (int)kPairRun;
    static_assert(N == 2, "a lane's run is one dword: two pairs");
    static_assert(UNION >= 8 && 2 * UNION <= (int)kPairSlack, "the slack behind a row covers a union window");
    float *const s_v = reinterpret_cast<float *>(smem) + (size_t)threadIdx.y * (ncols_max + kPairSlack); // (ncols_max % 4 == 0)
    const uint32_t seg = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + threadIdx.y);
    const uint32_t ow = G.ob >> 1;       // output cells of a row
    const uint32_t P0 = seg * kPairSegment; // first output cell of the segment
    if (P0 >= ow) return; // whole wave; no workgroup barriers below
    const uint32_t Plast = umin(P0 + kPairSegment, ow) - 1;
    const int32_t cmin = 2 * T.lx[P0];                                  // input BYTES from here on
    const int32_t cmax = 2 * (T.lx[Plast] + (int32_t)T.nx[Plast]);      // <= ib
    const int32_t c0 = cmin & ~3;                                       // the V pass walks whole dwords of the input rows
    const int32_t nrow = ((cmax - c0) + 3) & ~3;                        // <= ncols_max (host: YuvResizer::initialize)
    const uint32_t p = P0 + threadIdx.x * N;
    const bool lane_active = p < ow; // (ow % 2 == 0: an active lane owns two pairs)
    const uint32_t y_begin = blockIdx.y * rows_per_block;
    const uint32_t y_end = umin(y_begin + rows_per_block, G.oh);
    const uint32_t z = G.z0 + blockIdx.z;
    const uint8_t *const src_plane = in + (size_t)z * G.in_fs + G.in_off;
    uint8_t *const dst = out + (size_t)z * G.out_fs + G.out_off + 2 * (size_t)p;

    if (threadIdx.x < kPairSlack) s_v[nrow + threadIdx.x] = 0.0f;
    // union window: the weights of pair i re-based to the first pair's left column
    int32_t hl0; // LDS index of the first pair's left cell, channel U
    float hu[N][UNION];
    {
        int32_t hl[N];
#pragma unroll
        for (int i = 0; i < N; ++i) hl[i] = T.lx[lane_active ? p + i : 0];
        hl0 = 2 * hl[0] - c0;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const uint32_t po = lane_active ? p + i : 0;
            const int32_t shift = hl[i] - hl[0]; // >= 0: left edges do not decrease with x
#pragma unroll
            for (int j = 0; j < UNION; ++j) {
                const int32_t k = j - shift;
                const float w = T.wx[(size_t)po * G.stride + (uint32_t)(k < 0 ? 0 : (k > 7 ? 7 : k))];
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
        const uint8_t *const src = src_plane + (size_t)ly * G.ib;
        // V pass: one dword of every tap row per lane per sweep, all requested before the first is consumed
        for (int32_t col = c0 + 4 * (int32_t)threadIdx.x; col < cmax; col += 4 * kWave) {
            uint32_t q[8];
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if ((uint32_t)j < ny) q[j] = *reinterpret_cast<const uint32_t *>(src + (size_t)j * G.ib + col); // wave-uniform branch
            float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if ((uint32_t)j < ny) {
#pragma unroll
                    for (int m = 0; m < 4; ++m) v[m] = mac<EXACT>(v[m], ch_f32(q[j], m), wv[j]);
                }
            }
            *reinterpret_cast<float4 *>(s_v + (col - c0)) = make_float4(v[0], v[1], v[2], v[3]); // (bytes < ib: real values)
        }
        // A wave only ever reads the LDS row it wrote itself, and the LDS executes one wave's instructions in order: no workgroup
        // barrier, just keep the compiler from reordering.
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (lane_active) {
            float2 R[UNION]; // (x, y) = (U, V) of cell hl[0] + j; hl0 is even: 8-byte aligned
#pragma unroll
            for (int j = 0; j < UNION; ++j) R[j] = *reinterpret_cast<const float2 *>(s_v + hl0 + 2 * j);
            uint32_t o = 0;
#pragma unroll
            for (int i = 0; i < N; ++i) {
                float hu_ = 0.0f, hv_ = 0.0f;
#pragma unroll
                for (int j = 0; j < UNION; ++j) hu_ = mac<EXACT>(hu_, R[j].x, hu[i][j]), hv_ = mac<EXACT>(hv_, R[j].y, hu[i][j]);
                o = pack_u8<EXACT>(hu_, 2 * i, o);
                o = pack_u8<EXACT>(hv_, 2 * i + 1, o);
            }
            *reinterpret_cast<uint32_t *>(dst + (size_t)y * G.ob) = o;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); // the next row's V pass overwrites s_v
        __builtin_amdgcn_wave_barrier();
    }
}

// One output byte per thread: for every horizontal tap column the vertical sum first (f32, taps ascending), then the horizontal
// sum -- the operation order of the row kernel and of the two-pass CPU algorithm.  blockDim = (64, 4).
template <bool EXACT>
__global__ __launch_bounds__(256) void k_pair_px(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, PlaneTables T, PairGeom G)
{
    const size_t x = (size_t)blockIdx.x * kWave + threadIdx.x, y = (size_t)blockIdx.y * 4 + threadIdx.y; // x: an output BYTE
    if (x >= G.ob || y >= G.oh) return;
    const size_t cx = x >> 1, c = x & 1;
    const int32_t lx = T.lx[cx], ly = T.ly[y];
    const uint32_t nx = T.nx[cx], ny = T.ny[y];
    const float *const wx = T.wx + cx * G.stride, *const wy = T.wy + y * G.stride;
    const size_t z = (size_t)G.z0 + blockIdx.z;
    const uint8_t *const src = in + z * G.in_fs + G.in_off + (size_t)ly * G.ib + 2 * (size_t)lx + c;
    float h = 0.0f;
    for (uint32_t a = 0; a < nx; ++a) {
        float v = 0.0f;
        for (uint32_t b = 0; b < ny; ++b) v = mac<EXACT>(v, (float)src[(size_t)b * G.ib + 2 * (size_t)a], wy[b]);
        h = mac<EXACT>(h, v, wx[a]);
    }
    out[z * G.out_fs + G.out_off + y * G.ob + x] = (uint8_t)pack_u8<EXACT>(h, 0, 0u);
}

inline bool dword(const void *p) { return (reinterpret_cast<uintptr_t>(p) % 4) == 0; }

inline bool pair_launch_ok(const PlaneResizeLaunch &L)
{
    return L.in && L.out && L.iw && L.ih && L.ow && L.oh && L.n_frames && L.planes_per_frame == 1 && L.iw <= 0x7FFFFFFFu / 2 && L.ow <= 0x7FFFFFFFu / 2 &&
           L.t.lx && L.t.ly && L.t.nx && L.t.ny && L.t.wx && L.t.wy && L.table_stride >= 8 && L.max_taps >= 1 && L.max_taps <= L.table_stride &&
           L.in_frame_stride && L.out_frame_stride && cdiv(L.oh, 4) <= 65535;
}

} // namespace

bool pair_rows_form(const PlaneResizeLaunch &L)
{
    return (L.iw % 2) == 0 && (L.ow % 2) == 0 && dword(L.in) && dword(L.out) && (L.in_frame_stride % 4) == 0 && (L.out_frame_stride % 4) == 0 &&
           (L.in_plane_offset % 4) == 0 && (L.out_plane_offset % 4) == 0 && L.max_taps <= 8 && L.union_taps >= 1 && L.union_taps <= kPairMaxUnion &&
           L.ncols_max >= 4 && (L.ncols_max % 4) == 0 && L.ncols_max <= 4096;
}

hipError_t launch_pair_resize(const PlaneResizeLaunch &L)
{
    if (!pair_launch_ok(L)) return hipErrorInvalidValue;
    const bool rows = pair_rows_form(L);
    return for_grid_z_chunks(L.n_frames, [&](uint32_t done, uint32_t n) {
        const PairGeom G{L.in_frame_stride, L.out_frame_stride, L.in_plane_offset, L.out_plane_offset, done, 2 * L.iw, L.ih, 2 * L.ow, L.oh, L.table_stride};
        const dim3 block(kWave, 4);
        if (!rows) {
            const dim3 grid(cdiv(2 * L.ow, kWave), cdiv(L.oh, 4), n);
            if (L.exact) hipLaunchKernelGGL(k_pair_px<true>, grid, block, 0, L.stream, L.in, L.out, L.t, G);
            else hipLaunchKernelGGL(k_pair_px<false>, grid, block, 0, L.stream, L.in, L.out, L.t, G);
            return;
        }
        const uint64_t blocks_x = cdiv(cdiv(L.ow, kPairSegment), 4);
        uint64_t rpb = (uint64_t)L.oh * blocks_x * n / 4096; // a few thousand blocks per launch ...
        rpb = rpb < 8 ? 8 : (rpb > 32 ? 32 : rpb);            // ... each with rows enough to amortise its union weights
        const dim3 grid((uint32_t)blocks_x, cdiv(L.oh, (uint32_t)rpb), n);
        const size_t lds = (size_t)4 * (L.ncols_max + kPairSlack) * sizeof(float);
        if (L.exact) hipLaunchKernelGGL((k_pair_rows<true, 8>), grid, block, lds, L.stream, L.in, L.out, L.t, G, (uint32_t)rpb, L.ncols_max);
        else hipLaunchKernelGGL((k_pair_rows<false, 8>), grid, block, lds, L.stream, L.in, L.out, L.t, G, (uint32_t)rpb, L.ncols_max);
    });
}

} // namespace nus
