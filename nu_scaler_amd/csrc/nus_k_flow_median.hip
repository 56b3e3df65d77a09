// nus_k_flow_median.hip -- component-wise S x S median of a flow field (S = 3 or 5; nus_flow_set_median of include/nuscaler_hip.h):
// what the estimator runs behind every Jacobi run of a level when the setting is on.  u and v are filtered separately, the window
// is centred on the cell, coordinates are clamped into the level (replicated border).
//
// One workgroup takes a 64 x 16 tile of one pair's level (pairs on the grid's z axis): its 256 lanes stage the tile and a halo
// of S / 2 cells as float2 in LDS ((64 + 2R) x (16 + 2R) x 8 B: 9.3 / 10.6 KiB), every load clamped into the level, so no lane
// reads outside it whatever the level's size.  A wave then owns 4 rows of 64 cells; a lane reads its S x S window with
// ds_read_b64 -- consecutive lanes, consecutive 8-byte cells: conflict-free -- and selects the median of each component in
// registers with a fixed compare-exchange network of v_min_f32 / v_max_f32 pairs (19 exchanges for 9 values, 99 for 25; the
// networks were checked on every 0-1 input, which by the 0-1 principle covers every input): no data-dependent branch, no sort
// of the whole window.  A selection rounds nothing: the output is one of the inputs (either zero where +0 and -0 tie; NaNs are
// out of contract).
//
// The input and the output must not overlap: a tile's halo is another tile's output.
#include "nus_device.hpp"

#include <utility>

namespace nus {

namespace {

constexpr int kMedTW = 64, kMedTH = 16, kMedThreads = 256;

struct Exchange {
    unsigned char lo, hi; // after the exchange p[lo] = min, p[hi] = max
};

// median of 9 (J. L. Smith / A. Paeth, Graphics Gems): the result in p[4]
constexpr Exchange kNet9[] = {{1, 2}, {4, 5}, {7, 8}, {0, 1}, {3, 4}, {6, 7}, {1, 2}, {4, 5}, {7, 8}, {0, 3},
                              {5, 8}, {4, 7}, {3, 6}, {1, 4}, {2, 5}, {4, 7}, {4, 2}, {6, 4}, {4, 2}};
// median of 25 (Graphics Gems, as N. Devillard's "Fast median search" lists it): the result in p[12]
constexpr Exchange kNet25[] = {
    {0, 1},   {3, 4},   {2, 4},   {2, 3},   {6, 7},   {5, 7},   {5, 6},   {9, 10},  {8, 10},  {8, 9},   {12, 13}, {11, 13}, {11, 12}, {15, 16},
    {14, 16}, {14, 15}, {18, 19}, {17, 19}, {17, 18}, {21, 22}, {20, 22}, {20, 21}, {23, 24}, {2, 5},   {3, 6},   {0, 6},   {0, 3},   {4, 7},
    {1, 7},   {1, 4},   {11, 14}, {8, 14},  {8, 11},  {12, 15}, {9, 15},  {9, 12},  {13, 16}, {10, 16}, {10, 13}, {20, 23}, {17, 23}, {17, 20},
    {21, 24}, {18, 24}, {18, 21}, {19, 22}, {8, 17},  {9, 18},  {0, 18},  {0, 9},   {10, 19}, {1, 19},  {1, 10},  {11, 20}, {2, 20},  {2, 11},
    {12, 21}, {3, 21},  {3, 12},  {13, 22}, {4, 22},  {4, 13},  {14, 23}, {5, 23},  {5, 14},  {15, 24}, {6, 24},  {6, 15},  {7, 16},  {7, 19},
    {13, 21}, {15, 23}, {7, 13},  {7, 15},  {1, 9},   {3, 11},  {5, 17},  {11, 17}, {9, 17},  {4, 10},  {6, 12},  {7, 14},  {4, 6},   {4, 7},
    {12, 14}, {10, 14}, {6, 7},   {10, 12}, {6, 10},  {6, 17},  {12, 17}, {7, 17},  {7, 10},  {12, 18}, {7, 12},  {10, 18}, {12, 20}, {10, 20},
    {10, 12}};
static_assert(sizeof(kNet9) / sizeof(Exchange) == 19 && sizeof(kNet25) / sizeof(Exchange) == 99, "the published exchange counts");

// exchange I of the network, its two register indices compile-time constants
template <int S, int I>
__device__ __forceinline__ void exchange(float (&p)[S * S])
{
    constexpr Exchange e = S == 3 ? kNet9[I < 19 ? I : 0] : kNet25[I];
    const float a = p[e.lo], b = p[e.hi];
    p[e.lo] = __builtin_fminf(a, b);
    p[e.hi] = __builtin_fmaxf(a, b);
}
template <int S, int... I>
__device__ __forceinline__ float median_of(float (&p)[S * S], std::integer_sequence<int, I...>)
{
    (exchange<S, I>(p), ...);
    return p[S * S / 2];
}
template <int S>
__device__ __forceinline__ float median_of(float (&p)[S * S])
{
    return median_of<S>(p, std::make_integer_sequence<int, S == 3 ? 19 : 99>{});
}

template <int S>
__global__ __launch_bounds__(kMedThreads) void k_flow_median(const float2 *__restrict__ in_all, size_t in_stride,
                                                            float2 *__restrict__ out_all, size_t out_stride, int w, int h)
{
    static_assert(S == 3 || S == 5, "3 x 3 or 5 x 5");
    constexpr int R = S / 2, LW = kMedTW + 2 * R, LH = kMedTH + 2 * R;
    __shared__ float2 tile[LH][LW];
    const float2 *const in = in_all + blockIdx.z * in_stride;
    float2 *const out = out_all + blockIdx.z * out_stride;
    const int x0 = blockIdx.x * kMedTW, y0 = blockIdx.y * kMedTH;
    for (int i = threadIdx.x; i < LW * LH; i += kMedThreads) {
        const int ly = i / LW, lx = i - ly * LW;
        const int gx = clampi(x0 + lx - R, 0, w - 1), gy = clampi(y0 + ly - R, 0, h - 1);
        tile[ly][lx] = in[(size_t)gy * w + gx];
    }
    __syncthreads();
    const int lx = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave; // (kMedTW == kWave: a wave's lanes are a row of cells)
    const int x = x0 + lx;
    if (x >= w) return;
#pragma unroll 1
    for (int ly = wave; ly < kMedTH; ly += kMedThreads / kWave) {
        const int y = y0 + ly;
        if (y >= h) break; // wave-uniform
        float u[S * S], v[S * S];
#pragma unroll
        for (int dy = 0; dy < S; ++dy)
#pragma unroll
            for (int dx = 0; dx < S; ++dx) {
                const float2 c = tile[ly + dy][lx + dx];
                u[dy * S + dx] = c.x;
                v[dy * S + dx] = c.y;
            }
        out[(size_t)y * w + x] = make_float2(median_of<S>(u), median_of<S>(v));
    }
}

} // namespace

hipError_t launch_flow_median(const FlowMedianLaunch &L)
{
    static_assert(kMedTW == kWave && kMedThreads % kWave == 0, "a wave's lanes are one row of the tile");
    if ((L.size != 3 && L.size != 5) || L.in == nullptr || L.out == nullptr || L.in == L.out) return hipErrorInvalidValue;
    const dim3 block(kMedThreads), grid(cdiv(L.img.w, kMedTW), cdiv(L.img.h, kMedTH), L.img.n);
    const auto kernel = L.size == 3 ? k_flow_median<3> : k_flow_median<5>;
    hipLaunchKernelGGL(kernel, grid, block, 0, L.img.stream, reinterpret_cast<const float2 *>(L.in), L.in_stride,
                       reinterpret_cast<float2 *>(L.out), L.out_stride, (int)L.img.w, (int)L.img.h);
    return hipGetLastError();
}

} // namespace nus
