// nus_k_bm_bidir.hip -- the forward-backward check of the block matcher (gfx950; nus_bm_set_bidirectional in
// include/nuscaler_hip.h, where the rule is written).  launch_blockmatch (nus_k_blockmatch.hip) has run k_bm_search both ways --
// F, sadF: A's blocks in B; G, sadG: B's blocks in A, on the same grid -- and hands the four fields over.  Two kernels, one lane
// per block, the pair in grid.y as the confidence pass has it.  Integer instructions only; no LDS, no atomics, no scratch.
//
//   k_bm_bidir_choose  is the block's forward winner answered by the backward winner of the block it points at (and the other
//                      way round)?  Keeps F, or takes -G of the same grid position, or marks the block unresolved.  Reads 8 + 8
//                      bytes per field and block, writes a vector and a state byte.
//   k_bm_bidir_fill    an unresolved block takes, per component, the lower median of its resolved neighbours: the 8 values
//                      through a fixed 19-exchange sorting network in registers (missing ones as a sentinel that sorts last),
//                      the element picked by selects (indexing a local array would put it in scratch).
#include <hip/hip_runtime.h>

#include "nus_kernels.hpp"

namespace nus {

namespace {

constexpr uint32_t kNoMatch = 0xFFFFFFFFu;
constexpr uint32_t kUnresolved = 0x80u; // state byte of the choose step; otherwise the flag bits it set (0 or 4)
constexpr uint32_t kFromBackward = 4u, kFilled = 8u, kNoNeighbour = 16u;

// Is block (bx, by) of the search p -> q consistent: does the winner of the q-side block its centre lands in (clamped into the
// frame) point back at it within `tol` (L1)?  Both are indices of one pair's grid; cx <= (w - 1) >> lg = blocks_x - 1.
__device__ __forceinline__ bool bm_consistent(short2 p, uint32_t sad_p, const short2 *__restrict__ q, const uint32_t *__restrict__ sad_q,
                                              uint32_t bx, uint32_t by, uint32_t w, uint32_t h, uint32_t lg, uint32_t blocks_x, int tol)
{
    const int half = (1 << lg) >> 1;
    const int cx = min(max((int)(bx << lg) + (int)p.x + half, 0), (int)w - 1) >> lg;
    const int cy = min(max((int)(by << lg) + (int)p.y + half, 0), (int)h - 1) >> lg;
    const uint32_t o = (uint32_t)cy * blocks_x + (uint32_t)cx;
    const short2 g = q[o];
    return sad_p != kNoMatch && sad_q[o] != kNoMatch && abs((int)p.x + (int)g.x) + abs((int)p.y + (int)g.y) <= tol;
}

// grid: (ceil(blocks / 256), pairs).  chosen = F where A's block is consistent, else -G where B's block at the same grid position
// is (state 4), else unresolved (state 0x80; the vector written is 0 and never read)
__global__ __launch_bounds__(256) void k_bm_bidir_choose(const short2 *__restrict__ fwd, const uint32_t *__restrict__ sad_f,
                                                         const short2 *__restrict__ bwd, const uint32_t *__restrict__ sad_b, uint32_t w,
                                                         uint32_t h, uint32_t bs_log2, uint32_t blocks_x, uint32_t blocks_y, int tol,
                                                         short2 *__restrict__ chosen, uint8_t *__restrict__ state)
{
    const uint32_t n = blocks_x * blocks_y, i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const size_t base = (size_t)blockIdx.y * n;
    const short2 *F = fwd + base, *G = bwd + base;
    const uint32_t *sF = sad_f + base, *sG = sad_b + base;
    const uint32_t by = i / blocks_x, bx = i - by * blocks_x;
    const short2 f = F[i], g = G[i];
    const bool ok_a = bm_consistent(f, sF[i], G, sG, bx, by, w, h, bs_log2, blocks_x, tol);
    const bool ok_b = bm_consistent(g, sG[i], F, sF, bx, by, w, h, bs_log2, blocks_x, tol);
    short2 v = f;
    uint32_t st = 0;
    if (!ok_a) {
        v = ok_b ? short2{(short)-g.x, (short)-g.y} : short2{0, 0};
        st = ok_b ? kFromBackward : kUnresolved;
    }
    chosen[base + i] = v;
    state[base + i] = (uint8_t)st;
}

__device__ __forceinline__ void bm_cx(int &a, int &b)
{
    const int lo = min(a, b), hi = max(a, b);
    a = lo;
    b = hi;
}

// element (n - 1) / 2 of the ascending order of 8 values of which the n present ones are below the sentinel; n >= 1
__device__ __forceinline__ int bm_lower_median8(int v0, int v1, int v2, int v3, int v4, int v5, int v6, int v7, int n)
{
    bm_cx(v0, v2), bm_cx(v1, v3), bm_cx(v4, v6), bm_cx(v5, v7);
    bm_cx(v0, v4), bm_cx(v1, v5), bm_cx(v2, v6), bm_cx(v3, v7);
    bm_cx(v0, v1), bm_cx(v2, v3), bm_cx(v4, v5), bm_cx(v6, v7);
    bm_cx(v2, v4), bm_cx(v3, v5);
    bm_cx(v1, v4), bm_cx(v3, v6);
    bm_cx(v1, v2), bm_cx(v3, v4), bm_cx(v5, v6);
    const int k = (n - 1) >> 1; // 0 .. 3
    return k == 0 ? v0 : k == 1 ? v1 : k == 2 ? v2 : v3;
}

// same grid.  Reads the choose step's result only, so the order of the blocks does not matter.  flags: bit 2 = taken from the
// backward search, bit 3 = filled from the neighbours, bit 4 = no resolved neighbour, zero vector
__global__ __launch_bounds__(256) void k_bm_bidir_fill(const short2 *__restrict__ chosen, const uint8_t *__restrict__ state,
                                                       uint32_t blocks_x, uint32_t blocks_y, short2 *__restrict__ vectors,
                                                       uint8_t *__restrict__ flags)
{
    constexpr int kLast = 0x7FFF; // above every component (|v| <= 24)
    const uint32_t n = blocks_x * blocks_y, i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const size_t base = (size_t)blockIdx.y * n;
    const short2 *V = chosen + base;
    const uint8_t *S = state + base;
    short2 out = V[i];
    uint32_t f = S[i];
    if (f == kUnresolved) {
        const int by = (int)(i / blocks_x), bx = (int)(i - (uint32_t)by * blocks_x);
        int x[8], y[8], cnt = 0; // indexed by unrolled constants only: registers
        int k = 0;
#pragma unroll
        for (int oy = -1; oy <= 1; ++oy)
#pragma unroll
            for (int ox = -1; ox <= 1; ++ox) {
                if (ox == 0 && oy == 0) continue;
                const int nx = bx + ox, ny = by + oy;
                bool have = nx >= 0 && ny >= 0 && nx < (int)blocks_x && ny < (int)blocks_y;
                short2 v = short2{0, 0};
                if (have) {
                    const uint32_t o = (uint32_t)ny * blocks_x + (uint32_t)nx;
                    have = S[o] != kUnresolved;
                    v = V[o];
                }
                x[k] = have ? (int)v.x : kLast;
                y[k] = have ? (int)v.y : kLast;
                cnt += have ? 1 : 0;
                ++k;
            }
        if (cnt == 0) {
            out = short2{0, 0};
            f = kNoNeighbour;
        } else {
            out.x = (short)bm_lower_median8(x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7], cnt);
            out.y = (short)bm_lower_median8(y[0], y[1], y[2], y[3], y[4], y[5], y[6], y[7], cnt);
            f = kFilled;
        }
    }
    vectors[base + i] = out;
    if (flags) flags[base + i] = (uint8_t)f;
}

} // namespace

hipError_t launch_bm_bidir(const BmBidirLaunch &L)
{
    const uint32_t groups = (uint32_t)(((uint64_t)L.blocks_x * L.blocks_y + 255) / 256);
    const dim3 g(groups, L.n_pairs);
    short2 *const chosen = reinterpret_cast<short2 *>(L.chosen);
    hipLaunchKernelGGL(k_bm_bidir_choose, g, dim3(256), 0, L.stream, reinterpret_cast<const short2 *>(L.fwd), L.sad_f,
                       reinterpret_cast<const short2 *>(L.bwd), L.sad_b, L.w, L.h, L.bs_log2, L.blocks_x, L.blocks_y, (int)L.tolerance,
                       chosen, L.state);
    hipLaunchKernelGGL(k_bm_bidir_fill, g, dim3(256), 0, L.stream, chosen, L.state, L.blocks_x, L.blocks_y,
                       reinterpret_cast<short2 *>(L.vectors), L.flags);
    return hipGetLastError();
}

} // namespace nus
