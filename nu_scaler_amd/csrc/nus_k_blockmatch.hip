// nus_k_blockmatch.hip -- block-matching motion estimation on the GPU (gfx950): the full SAD search of
// BlockMatchingInterpolator (nu_scaler_core/src/interpolation/mod.rs:555-622), its confidence pass (:795-910) over the block
// grid, and the expansion of the block vectors to the dense flow the warp kernels read.  Integer work, no atomics (the only float
// instructions are the reciprocal steps of the compiler's integer divisions, outside the row loop).
//
//   k_bm_search<BS>  one workgroup per run of 64 / BS neighbouring blocks of one block row.  The part of frame B every candidate
//                    of the run can touch -- (2R + BS) rows of 2R + 64 pixels -- is staged once in LDS with alpha cleared.  A lane
//                    owns two candidates (dx, dx + 1) of one dy: per block row it reads BS / 2 + 1 aligned pixel pairs
//                    (8-byte LDS reads) and does 2 BS byte-SADs (v_sad_u8: |dR| + |dG| + |dB| + |0 - 0| and the accumulate in one
//                    lane-op), the A pixel as a scalar operand -- the block's A row is the same for every candidate, so it is
//                    loaded once per wave through the scalar cache.  The row pitch of the LDS window is 2 (R + 1) + 64 dwords:
//                    lane t of a chunk then reads the dword pair 2 t (mod 64), every bank once per 32 lanes.
//                    The winner is the plain minimum of the key sad << 12 | rank (sad < 2^20, rank < 2401 < 2^12): the tie order
//                    is the rank table the host built, not a code path.  Keys are reduced per wave with a butterfly and per
//                    block through LDS.
//   k_bm_rough       per 256 blocks of a pair: does any block with bx, by >= 1 differ from its left or top neighbour by more
//                    than 10 (L1)?  One word per workgroup into the workspace.
//   k_bm_refine      ORs those words (the pair's motion is not smooth), then zeroes every interior block whose L1 differences
//                    to its 8 neighbours sum to 35 or more, and writes vectors and flags.
//   k_bm_flow<HALF>  every pixel gets its block's vector as (dx, dy), 2 x f32 or 2 x f16 (|v| <= 24: exact in both).
// The forward-backward check runs k_bm_search a second time with the frames exchanged; its own two kernels are in
// nus_k_bm_bidir.hip.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "nus_kernels.hpp"

namespace nus {

namespace {

constexpr int kRun = (int)kBmRunPixels; // pixels of frame A per workgroup, along x
constexpr uint32_t kRgb = 0x00FFFFFFu;  // RGBA8, little endian: alpha is the top byte
constexpr uint32_t kNoMatch = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t sad4(uint32_t b, uint32_t a, uint32_t acc) { return __builtin_amdgcn_sad_u8(b, a, acc); }

// The SADs of one lane's two candidates over the block's rows.  p: the lane's first dword pair in the LDS window (candidate 0
// starts at its first dword, candidate 1 at its second); arow: the block's first A pixel (uniform over the wave).
// FULL: the block is BS pixels wide; otherwise only its first cols_a columns lie in frame A and count.
template <int BS, bool FULL>
__device__ __forceinline__ void bm_rows(const uint32_t *p, int pitch, const uint32_t *arow, uint32_t w, int rows_a, int cols_a,
                                        uint32_t &acc0, uint32_t &acc1)
{
    for (int py = 0; py < rows_a; ++py) {
        uint32_t A[BS], M[BS];
#pragma unroll
        for (int px = 0; px < BS; ++px) {
            M[px] = (FULL || px < cols_a) ? kRgb : 0u;
            A[px] = (FULL || px < cols_a) ? (arow[px] & kRgb) : 0u;
        }
        uint2 v[BS / 2 + 1];
#pragma unroll
        for (int i = 0; i <= BS / 2; ++i) v[i] = reinterpret_cast<const uint2 *>(p)[i];
#pragma unroll
        for (int i = 0; i < BS / 2; ++i) {
            const uint32_t m0 = M[2 * i], m1 = M[2 * i + 1];
            acc0 = sad4(FULL ? v[i].x : (v[i].x & m0), A[2 * i], acc0);
            acc0 = sad4(FULL ? v[i].y : (v[i].y & m1), A[2 * i + 1], acc0);
            acc1 = sad4(FULL ? v[i].y : (v[i].y & m0), A[2 * i], acc1);
            acc1 = sad4(FULL ? v[i + 1].x : (v[i + 1].x & m1), A[2 * i + 1], acc1);
        }
        p += pitch;
        arow += w;
    }
}

// grid: (runs of 64 pixels, block rows, pairs); dynamic LDS: (2R + BS) rows of 2R + 66 dwords.
// rank[(dy + R) * (2R + 1) + dx + R]: the candidate's place in the tie order; cand[rank]: the inverse.
template <int BS>
__global__ __launch_bounds__(256) void k_bm_search(const uint8_t *__restrict__ a, size_t a_stride, const uint8_t *__restrict__ b,
                                                   size_t b_stride, uint32_t w, uint32_t h, int R, const uint16_t *__restrict__ rank,
                                                   const uint16_t *__restrict__ cand, uint32_t blocks_x, uint32_t blocks_y,
                                                   int16_t *__restrict__ vectors, uint32_t *__restrict__ sad)
{
    constexpr int NB = kRun / BS;                 // blocks per run
    constexpr int WPB = NB >= 4 ? 1 : 4 / NB;     // waves that share one block's candidates
    extern __shared__ __attribute__((aligned(16))) uint32_t win[];
    __shared__ uint32_t s_best[NB * WPB];
    const int pitch = 2 * R + 2 + kRun, rows = 2 * R + BS;
    const int X0 = (int)blockIdx.x * kRun, y0 = (int)blockIdx.y * BS;
    const uint32_t pair = blockIdx.z;
    const uint32_t *pa = reinterpret_cast<const uint32_t *>(a + (size_t)pair * a_stride);
    const uint32_t *pb = reinterpret_cast<const uint32_t *>(b + (size_t)pair * b_stride);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63u);

    // frame B's window: rows y0 - R .. y0 + R + BS - 1, columns X0 - R .. X0 + R + 65; zero outside the frame (no admitted
    // candidate reads those)
    for (int r = wave; r < rows; r += 4) {
        const int y = y0 - R + r;
        const bool row_in = y >= 0 && y < (int)h;
        for (int c = lane; c < pitch; c += 64) {
            const int x = X0 - R + c;
            uint32_t v = 0;
            if (row_in && x >= 0 && x < (int)w) v = pb[(size_t)y * w + (uint32_t)x] & kRgb;
            win[r * pitch + c] = v;
        }
    }
    __syncthreads();

    const int D = 2 * R + 1, P = R + 1, T = D * P; // T lane tasks per block: (dy, pair of dx)
    const int nchunks = (T + 63) / 64;
    const int rows_a = min(BS, (int)h - y0);
    for (int k = wave / WPB; k < NB; k += 4 / WPB) {
        const int x0 = X0 + k * BS;
        if (x0 >= (int)w) break;
        const int cols_a = min(BS, (int)w - x0);
        const uint32_t *arow = pa + (size_t)y0 * w + (uint32_t)x0;
        uint32_t best = kNoMatch;
        for (int c = wave % WPB; c < nchunks; c += WPB) {
            int t = c * 64 + lane;
            const bool live = t < T;
            if (!live) t = 0;
            const int dyi = t / P, j = t - dyi * P;
            const uint32_t *p = win + dyi * pitch + k * BS + 2 * j;
            uint32_t acc0 = 0, acc1 = 0;
            if (cols_a == BS)
                bm_rows<BS, true>(p, pitch, arow, w, rows_a, cols_a, acc0, acc1);
            else
                bm_rows<BS, false>(p, pitch, arow, w, rows_a, cols_a, acc0, acc1);
            // admitted: the candidate block lies wholly inside frame B
            const int dy = dyi - R, dx0 = 2 * j - R;
            const bool oky = live && y0 + dy >= 0 && y0 + dy + BS <= (int)h;
            const bool ok0 = oky && x0 + dx0 >= 0 && x0 + dx0 + BS <= (int)w;
            const bool ok1 = oky && 2 * j + 1 < D && x0 + dx0 + 1 >= 0 && x0 + dx0 + 1 + BS <= (int)w;
            const uint32_t k0 = ok0 ? ((acc0 << 12) | rank[dyi * D + 2 * j]) : kNoMatch;
            const uint32_t k1 = ok1 ? ((acc1 << 12) | rank[dyi * D + 2 * j + 1]) : kNoMatch;
            best = min(best, min(k0, k1));
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) best = min(best, (uint32_t)__shfl_xor((int)best, o));
        if (lane == 0) s_best[k * WPB + wave % WPB] = best;
    }
    __syncthreads();
    if (threadIdx.x < (unsigned)NB) {
        const int k = (int)threadIdx.x;
        const uint32_t bx = blockIdx.x * NB + k;
        if (bx < blocks_x) {
            uint32_t key = s_best[k * WPB];
#pragma unroll
            for (int i = 1; i < WPB; ++i) key = min(key, s_best[k * WPB + i]);
            int dx = 0, dy = 0;
            uint32_t s = kNoMatch;
            if (key != kNoMatch) {
                const int c = cand[key & 0xFFFu];
                dy = c / D - R;
                dx = c - (c / D) * D - R;
                s = key >> 12;
            }
            const size_t o = ((size_t)pair * blocks_y + blockIdx.y) * blocks_x + bx;
            vectors[2 * o] = (int16_t)dx;
            vectors[2 * o + 1] = (int16_t)dy;
            if (sad) sad[o] = s;
        }
    }
}

// true on every lane iff `v` is true on some lane of the 256-lane workgroup (a vote per wave, the four votes through LDS: no atomic)
__device__ __forceinline__ bool block_any(bool v, uint32_t *votes)
{
    const bool wave_any = __ballot(v) != 0;
    if ((threadIdx.x & 63u) == 0) votes[threadIdx.x >> 6] = wave_any ? 1u : 0u;
    __syncthreads();
    return (votes[0] | votes[1] | votes[2] | votes[3]) != 0;
}

__device__ __forceinline__ int l1(short2 p, short2 q) { return abs((int)p.x - (int)q.x) + abs((int)p.y - (int)q.y); }

// grid: (ceil(blocks / 256), pairs).  rough[pair * gridDim.x + blockIdx.x] = some block of these 256 breaks smoothness
__global__ __launch_bounds__(256) void k_bm_rough(const short2 *__restrict__ raw, uint32_t blocks_x, uint32_t blocks_y,
                                                  uint32_t *__restrict__ rough)
{
    const uint32_t n = blocks_x * blocks_y, i = blockIdx.x * 256u + threadIdx.x;
    const short2 *v = raw + (size_t)blockIdx.y * n;
    __shared__ uint32_t votes[4];
    bool bad = false;
    if (i < n) {
        const uint32_t by = i / blocks_x, bx = i - by * blocks_x;
        if (bx >= 1 && by >= 1) bad = l1(v[i], v[i - 1]) > 10 || l1(v[i], v[i - blocks_x]) > 10;
    }
    const bool any = block_any(bad, votes);
    if (threadIdx.x == 0) rough[blockIdx.y * gridDim.x + blockIdx.x] = any ? 1u : 0u;
}

// same grid.  flags: bit 0 = this block was zeroed, bit 1 = the pair's motion is not smooth (every block of the pair)
__global__ __launch_bounds__(256) void k_bm_refine(const short2 *__restrict__ raw, const uint32_t *__restrict__ rough,
                                                   uint32_t blocks_x, uint32_t blocks_y, short2 *__restrict__ vectors,
                                                   uint8_t *__restrict__ flags)
{
    const uint32_t n = blocks_x * blocks_y, i = blockIdx.x * 256u + threadIdx.x;
    const short2 *v = raw + (size_t)blockIdx.y * n;
    __shared__ uint32_t votes[4];
    uint32_t any = 0;
    for (uint32_t g = threadIdx.x; g < gridDim.x; g += 256u) any |= rough[blockIdx.y * gridDim.x + g];
    const bool not_smooth = block_any(any != 0, votes);
    if (i >= n) return;
    short2 out = v[i];
    uint32_t f = not_smooth ? 2u : 0u;
    const uint32_t by = i / blocks_x, bx = i - by * blocks_x;
    if (not_smooth && bx > 0 && by > 0 && bx + 1 < blocks_x && by + 1 < blocks_y) {
        int sum = 0;
#pragma unroll
        for (int oy = -1; oy <= 1; ++oy)
#pragma unroll
            for (int ox = -1; ox <= 1; ++ox)
                if (ox != 0 || oy != 0) sum += l1(out, v[(size_t)((int)by + oy) * blocks_x + (uint32_t)((int)bx + ox)]);
        if (sum >= 35) { // 1 / (1 + 0.1 sum / 8) < 0.7 in f32: 34 gives 0.70175, 35 gives 0.69565
            out = short2{0, 0};
            f |= 1u;
        }
    }
    vectors[(size_t)blockIdx.y * n + i] = out;
    if (flags) flags[(size_t)blockIdx.y * n + i] = (uint8_t)f;
}

__global__ __launch_bounds__(256) void k_bm_zero_flags(uint8_t *__restrict__ flags, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n) flags[i] = 0;
}

// grid: (ceil(w h / 256), pairs).  flow[pair][y][x] = (dx, dy) of the pixel's block
template <bool HALF>
__global__ __launch_bounds__(256) void k_bm_flow(const short2 *__restrict__ vectors, uint32_t w, uint32_t h, uint32_t bs_log2,
                                                 uint32_t blocks_x, uint32_t blocks_y, void *__restrict__ flow)
{
    const uint32_t npx = w * h, i = blockIdx.x * 256u + threadIdx.x;
    if (i >= npx) return;
    const uint32_t y = i / w, x = i - y * w;
    const short2 v = vectors[((size_t)blockIdx.y * blocks_y + (y >> bs_log2)) * blocks_x + (x >> bs_log2)];
    const size_t o = (size_t)blockIdx.y * npx + i;
    if (HALF) {
        const _Float16 fx = (_Float16)(float)v.x, fy = (_Float16)(float)v.y;
        reinterpret_cast<uint32_t *>(flow)[o] =
            (uint32_t)__builtin_bit_cast(uint16_t, fx) | ((uint32_t)__builtin_bit_cast(uint16_t, fy) << 16);
    } else {
        reinterpret_cast<float2 *>(flow)[o] = float2{(float)v.x, (float)v.y};
    }
}

} // namespace

BmShape bm_shape(uint32_t w, uint32_t h, uint32_t bs, uint32_t n_pairs, bool bidir)
{
    BmShape s;
    s.blocks_x = (w + bs - 1) / bs;
    s.blocks_y = (h + bs - 1) / bs;
    s.runs_x = (w + kBmRunPixels - 1) / kBmRunPixels;
    s.rough_groups = (uint32_t)(((uint64_t)s.blocks_x * s.blocks_y + 255) / 256);
    const size_t raw = (size_t)n_pairs * s.blocks_x * s.blocks_y * 4;
    s.rough_offset = (raw + 15) & ~(size_t)15;
    s.workspace_bytes = s.rough_offset + (size_t)n_pairs * s.rough_groups * 4;
    if (bidir) {
        const auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
        s.g_offset = up16(s.workspace_bytes);
        s.sad_g_offset = s.g_offset + up16(raw);
        s.sad_f_offset = s.sad_g_offset + up16(raw);
        s.chosen_offset = s.sad_f_offset + up16(raw);
        s.state_offset = s.chosen_offset + up16(raw);
        s.workspace_bytes = s.state_offset + raw / 4;
    }
    return s;
}

size_t bm_lds_bytes(uint32_t bs, uint32_t R) { return (size_t)(2 * R + bs) * (2 * R + 2 + kBmRunPixels) * 4; }

hipError_t launch_blockmatch(const BmLaunch &L)
{
    const BmShape s = bm_shape(L.w, L.h, L.bs, L.n_pairs, L.bidir);
    uint8_t *const ws = static_cast<uint8_t *>(L.workspace);
    int16_t *raw = (L.refine || L.bidir) ? static_cast<int16_t *>(L.workspace) : L.vectors;
    uint32_t *sad = L.sad;
    if (L.bidir && !sad) sad = reinterpret_cast<uint32_t *>(ws + s.sad_f_offset); // the check reads them
    const dim3 grid(s.runs_x, s.blocks_y, L.n_pairs);
    const size_t lds = bm_lds_bytes(L.bs, L.R);
    // the blocks of `from` searched in `to`
    const auto search = [&](const uint8_t *from, size_t from_stride, const uint8_t *to, size_t to_stride, int16_t *v, uint32_t *sd) {
#define NUS_BM_SEARCH(BS)                                                                                                          \
    hipLaunchKernelGGL(k_bm_search<BS>, grid, dim3(256), lds, L.stream, from, from_stride, to, to_stride, L.w, L.h, (int)L.R, L.rank, \
                       L.cand, s.blocks_x, s.blocks_y, v, sd)
        if (L.bs == 8)
            NUS_BM_SEARCH(8);
        else if (L.bs == 16)
            NUS_BM_SEARCH(16);
        else
            NUS_BM_SEARCH(32);
#undef NUS_BM_SEARCH
        return hipGetLastError();
    };
    hipError_t e = search(L.a, L.a_stride, L.b, L.b_stride, raw, sad);
    if (e != hipSuccess) return e;
    const size_t nblocks = (size_t)L.n_pairs * s.blocks_x * s.blocks_y;
    uint32_t lg = 3;
    while ((1u << lg) < L.bs) ++lg;
    if (L.bidir) {
        // the same search with the frames exchanged: B's blocks in A, on the same grid
        int16_t *const bwd = reinterpret_cast<int16_t *>(ws + s.g_offset);
        uint32_t *const sad_b = reinterpret_cast<uint32_t *>(ws + s.sad_g_offset);
        if ((e = search(L.b, L.b_stride, L.a, L.a_stride, bwd, sad_b)) != hipSuccess) return e;
        BmBidirLaunch C;
        C.fwd = raw, C.sad_f = sad, C.bwd = bwd, C.sad_b = sad_b;
        C.w = L.w, C.h = L.h, C.n_pairs = L.n_pairs, C.bs_log2 = lg, C.blocks_x = s.blocks_x, C.blocks_y = s.blocks_y;
        C.tolerance = L.tolerance;
        C.chosen = reinterpret_cast<int16_t *>(ws + s.chosen_offset);
        C.state = ws + s.state_offset;
        C.vectors = L.vectors, C.flags = L.flags, C.stream = L.stream;
        if ((e = launch_bm_bidir(C)) != hipSuccess) return e;
    } else if (L.refine) {
        uint32_t *rough = reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(L.workspace) + s.rough_offset);
        const dim3 g(s.rough_groups, L.n_pairs);
        hipLaunchKernelGGL(k_bm_rough, g, dim3(256), 0, L.stream, reinterpret_cast<const short2 *>(raw), s.blocks_x, s.blocks_y, rough);
        hipLaunchKernelGGL(k_bm_refine, g, dim3(256), 0, L.stream, reinterpret_cast<const short2 *>(raw), rough, s.blocks_x, s.blocks_y,
                           reinterpret_cast<short2 *>(L.vectors), L.flags);
    } else if (L.flags) {
        hipLaunchKernelGGL(k_bm_zero_flags, dim3((unsigned)((nblocks + 255) / 256)), dim3(256), 0, L.stream, L.flags, nblocks);
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (L.flow) {
        const dim3 g((L.w * L.h + 255) / 256, L.n_pairs);
        if (L.flow_half)
            hipLaunchKernelGGL(k_bm_flow<true>, g, dim3(256), 0, L.stream, reinterpret_cast<const short2 *>(L.vectors), L.w, L.h, lg,
                               s.blocks_x, s.blocks_y, L.flow);
        else
            hipLaunchKernelGGL(k_bm_flow<false>, g, dim3(256), 0, L.stream, reinterpret_cast<const short2 *>(L.vectors), L.w, L.h, lg,
                               s.blocks_x, s.blocks_y, L.flow);
        e = hipGetLastError();
    }
    return e;
}

} // namespace nus
