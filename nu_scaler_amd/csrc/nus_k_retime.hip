// nus_k_retime.hip -- frame-rate conversion by a rational ratio (24 -> 60 fps) over a device-resident stream: the nus_*_retime_*
// entry points of include/nuscaler_hip.h, where the contract is written.  BUILD-DEFINED: the reference has no rate conversion.
//
// Every pair of the stream has its own set of in-between times, some pairs none; the schedule is retime_pair (nus_retime.hpp), a
// wave-uniform integer function of (pair, num, den) that the kernels evaluate themselves -- no table in memory, no host in the loop.
//   k_retime_flow / _proj / _bm   warp_blend_tile (nus_warp_device.hpp) with the vector sources of the dense-flow, projected-flow and
//                    block-vector warps (nus_warp_sources.hpp) and RetimeTimes as the time source: where the multi-time kernels take
//                    (t, frame) from the launch's TimeSet and pair_out + k * frame_bytes, these take them from the schedule.  The
//                    per-pixel code is the same, so an in-between output is byte for byte the single-time kernel's at t_j.  A pair's
//                    vectors are fetched once for all its outputs; a pair without in-between outputs leaves after the schedule.
//   k_retime_flow_sel             warp_select_tile_at (nus_warp_select_device.hpp) with both flows of every pair and the schedule: the
//                    select warp's per-pixel code, so an in-between output is byte for byte k_warp_blend_flow_sel's at t_j.
//   k_retime_warp_tiny<KIND>      the three families' one-pixel-per-thread forms (frames the tile does not take: warp_corner_ok).
//   k_retime_flow_sel_tiny        ... and the select warp's (k_warp_blend_flow_sel_tiny's body).
//   k_retime_blend   the zero-flow streaming blend (k_blend_zero_flow's arithmetic).
//   k_retime_real    REAL-FRAME OUTPUTS (r_j == 0, the stream's last frame included) COME FROM THIS COPY KERNEL OF ITS OWN, not from
//                    the warps: frame k with (k num) % den == 0 goes through the input selector to output k num / den -- the bytes
//                    of the zero-flow blend at t = 0.  The warps skip those outputs.
//   k_retime_scene_apply          k_scene_apply's rule on the schedule: a cut pair's in-between outputs become copies of A (t_j < 0.5)
//                    or B.
//   k_retime_table   the schedule written out (nus_retime_schedule_device: a diagnostic).
// Output j of the stream is at out + j * out_frame_stride; gaps are never written.  No atomics, no LDS, no scratch.
#include "nus_device.hpp"
#include "nus_retime.hpp"
#include "nus_warp_select_device.hpp"
#include "nus_warp_sources.hpp"

namespace nus {

namespace {

struct RetimeArgs { // by value in the kernel arguments
    uint8_t *out;
    size_t out_frame_stride;
    uint32_t first_pair; // of the launch: local pair i is pair first_pair + i of the stream
    uint32_t num, den;
};

// The in-between outputs of one pair: the pair's outputs without the real frame (remainder 0) that may lead them.
struct RetimeTimes {
    uint8_t *out;
    size_t stride;
    uint64_t first;
    uint32_t n, rem, num, den;

    __device__ __forceinline__ RetimeTimes(const RetimeArgs &R, uint32_t local_pair)
    {
        const RetimePair p = retime_pair((uint64_t)R.first_pair + local_pair, R.num, R.den);
        const uint32_t skip = (p.count != 0 && p.rem0 == 0) ? 1u : 0u;
        out = R.out, stride = R.out_frame_stride, num = R.num, den = R.den;
        first = p.first + skip, n = p.count - skip, rem = p.rem0 + skip * R.den;
    }
    __device__ __forceinline__ void begin() {} // (the kernels evaluate the schedule first: a pair without in-between outputs leaves there)
    __device__ __forceinline__ uint32_t count() const { return n; }
    __device__ __forceinline__ float time(uint32_t k) const { return retime_time(rem + k * den, num); }
    __device__ __forceinline__ uint32_t *frame(uint32_t k, size_t) const { return reinterpret_cast<uint32_t *>(out + (first + k) * stride); }
};

template <int MODE, bool HALF, int XV, int RV>
__global__ __launch_bounds__(256) void k_retime_flow(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b,
                                                     const void *__restrict__ flow, size_t frame_stride, uint32_t w, uint32_t h,
                                                     RetimeArgs R, uint32_t sel)
{
    const RetimeTimes T(R, blockIdx.z);
    if (T.count() == 0) return;
    warp_blend_tile_at<MODE, XV, RV>(a, b, frame_stride, frame_stride, w, h, sel, DenseFlowSource<HALF, XV, RV>{flow, {}}, T);
}

template <int MODE, bool HALF, int XV, int RV>
__global__ __launch_bounds__(256) void k_retime_flow_proj(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b,
                                                          const void *__restrict__ flow, size_t frame_stride, uint32_t w, uint32_t h,
                                                          RetimeArgs R, uint32_t sel, uint32_t rounds)
{
    const RetimeTimes T(R, blockIdx.z);
    if (T.count() == 0) return;
    ProjectedFlowSource<HALF, XV, RV> src;
    src.flow = flow, src.rounds = rounds;
    warp_blend_tile_at<MODE, XV, RV>(a, b, frame_stride, frame_stride, w, h, sel, src, T);
}

// The schedule for the select tile, whose loop over the outputs is the register-heaviest of the unit: `num` is made opaque per output,
// in a scalar register, so that the division's loop-invariant half (the conversion and reciprocal of num) is not hoisted into
// vector registers that would then live across the whole tile, and the wave-uniform quotient goes back into a scalar register, as the
// multi-time kernel's times are (the tile makes its own per-lane copy).  The same division, the same t_j.
struct RetimeSelTimes : RetimeTimes {
    __device__ __forceinline__ RetimeSelTimes(const RetimeArgs &R, uint32_t local_pair) : RetimeTimes(R, local_pair) {}
    __device__ __forceinline__ float time(uint32_t k) const
    {
        uint32_t n = num;
        asm volatile("" : "+s"(n));
        return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(retime_time(rem + k * den, n))));
    }
};

// Both flows of the pair, each pixel warped with the vector whose two samples agree better.  The pair's own vectors of both flows are
// loaded once for all its outputs; the projection rounds depend on t and run per output.
// The occupancy asked for is the multi-time select kernel's of the same form or better (7 waves per SIMD with f32 flows, 8 with
// halves): left alone, the register allocator ends one register above the f32 pair form's step.
template <int MODE, bool HALF, int XV, int RV>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(HALF ? 8 : 7))) void k_retime_flow_sel(
    const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, const void *__restrict__ flow_fwd, const void *__restrict__ flow_bwd,
    size_t frame_stride, uint32_t w, uint32_t h, RetimeArgs R, uint32_t sel, uint32_t rounds)
{
    const RetimeSelTimes T(R, blockIdx.z);
    if (T.count() == 0) return;
    warp_select_tile_at<MODE, HALF, XV, RV>(a, b, flow_fwd, flow_bwd, frame_stride, frame_stride, w, h, sel, rounds, T);
}

template <int MODE, int XV, int RV>
__global__ __launch_bounds__(256) void k_retime_bm(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b,
                                                   const short2 *__restrict__ vectors, size_t frame_stride, uint32_t w, uint32_t h,
                                                   RetimeArgs R, uint32_t bs_log2, uint32_t blocks_x, uint32_t blocks_y)
{
    const RetimeTimes T(R, blockIdx.z);
    if (T.count() == 0) return;
    warp_blend_tile_at<MODE, XV, RV>(a, b, frame_stride, frame_stride, w, h, kSelRGBA, BlockVectorSource<RV>{vectors, bs_log2, blocks_x, blocks_y, {}}, T);
}

// Frames narrower or lower than 2 pixels, or of 4 GiB and more: one pixel per thread, 64-bit addressing, EXACT arithmetic -- the
// bodies of k_warp_blend_flow_tiny, k_warp_blend_flow_proj_tiny and k_bm_warp_tiny with the schedule's times.
constexpr int kTinyDense = 0, kTinyProjected = 1, kTinyBlocks = 2;
template <int KIND>
__global__ __launch_bounds__(256) void k_retime_warp_tiny(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b,
                                                          const void *__restrict__ vec, bool half, size_t frame_stride, uint32_t w,
                                                          uint32_t h, RetimeArgs R, uint32_t sel, uint32_t rounds, uint32_t bs_log2,
                                                          uint32_t blocks_x, uint32_t blocks_y)
{
    const uint32_t y = blockIdx.y * 4 + threadIdx.y, x = blockIdx.x * kWave + threadIdx.x;
    if (y >= h || x >= w) return;
    const RetimeTimes T(R, blockIdx.z);
    const size_t npx = (size_t)w * h, pix = (size_t)y * w + x;
    const uint32_t *fa = reinterpret_cast<const uint32_t *>(a + (size_t)blockIdx.z * frame_stride);
    const uint32_t *fb = reinterpret_cast<const uint32_t *>(b + (size_t)blockIdx.z * frame_stride);
    // the pair's own flow plane (the flow kinds only: block vectors have no plane)
    const void *const plane = KIND == kTinyBlocks ? nullptr : static_cast<const uint8_t *>(vec) + (size_t)blockIdx.z * npx * (half ? 4 : 8);
    float2 f;
    if (KIND == kTinyBlocks) {
        const short2 v = static_cast<const short2 *>(vec)[((size_t)blockIdx.z * blocks_y + (y >> bs_log2)) * blocks_x + (x >> bs_log2)];
        f = make_float2((float)v.x, (float)v.y);
    } else {
        f = half ? half2_bits_to_float2(static_cast<const uint32_t *>(plane)[pix]) : static_cast<const float2 *>(plane)[pix];
    }
    for (uint32_t k = 0; k < T.count(); ++k) {
        const float t = T.time(k);
        float2 g = f;
        if (KIND == kTinyProjected)
            for (uint32_t r = 0; r < rounds; ++r) g = project_round_plain(plane, half, w, h, (float)x, (float)y, g, t);
        const uint32_t o = warp_blend_pixel_plain(fa, fb, w, h, x, y, g, t, 1.0f - t);
        T.frame(k, npx)[pix] = KIND == kTinyBlocks ? o : swz(o, sel);
    }
}

// The select warp's one-pixel-per-thread form: the body of k_warp_blend_flow_sel_tiny with the schedule's times.
__global__ __launch_bounds__(256) void k_retime_flow_sel_tiny(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b,
                                                              const void *__restrict__ flow_fwd, const void *__restrict__ flow_bwd, bool half,
                                                              size_t frame_stride, uint32_t w, uint32_t h, RetimeArgs R, uint32_t sel,
                                                              uint32_t rounds)
{
    const uint32_t y = blockIdx.y * 4 + threadIdx.y, x = blockIdx.x * kWave + threadIdx.x;
    if (y >= h || x >= w) return;
    const RetimeTimes T(R, blockIdx.z);
    const size_t npx = (size_t)w * h, pix = (size_t)y * w + x;
    const uint32_t *fa = reinterpret_cast<const uint32_t *>(a + (size_t)blockIdx.z * frame_stride);
    const uint32_t *fb = reinterpret_cast<const uint32_t *>(b + (size_t)blockIdx.z * frame_stride);
    const size_t plane_bytes = npx * (half ? 4 : 8); // the pair's own planes
    const void *const pf = static_cast<const uint8_t *>(flow_fwd) + (size_t)blockIdx.z * plane_bytes;
    const void *const pr = static_cast<const uint8_t *>(flow_bwd) + (size_t)blockIdx.z * plane_bytes;
    const float2 f = half ? half2_bits_to_float2(static_cast<const uint32_t *>(pf)[pix]) : static_cast<const float2 *>(pf)[pix];
    const float2 rv = half ? half2_bits_to_float2(static_cast<const uint32_t *>(pr)[pix]) : static_cast<const float2 *>(pr)[pix];
    for (uint32_t k = 0; k < T.count(); ++k) {
        const float t = T.time(k), nt = 1.0f - t;
        float2 gf = f, gb = rv;
        for (uint32_t r = 0; r < rounds; ++r) {
            gf = project_round_plain(pf, half, w, h, (float)x, (float)y, gf, t);
            gb = project_round_plain(pr, half, w, h, (float)x, (float)y, gb, nt);
        }
        float4 saf, sbf, sar, sbr;
        warp_sample_pair_plain(fa, fb, w, h, x, y, gf, t, nt, saf, sbf);
        warp_sample_pair_plain(fa, fb, w, h, x, y, make_float2(-gb.x, -gb.y), t, nt, sar, sbr);
        const bool back = warp_sample_error(sar, sbr) < warp_sample_error(saf, sbf);
        const uint32_t o = back ? warp_blend_pack(sar, sbr, t, nt) : warp_blend_pack(saf, sbf, t, nt);
        T.frame(k, npx)[pix] = swz(o, sel);
    }
}

// Zero flow: each lane loads its A and B pixels once, then blends and stores them once per in-between output of the pair.
template <bool VEC>
__global__ __launch_bounds__(256) void k_retime_blend(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, size_t frame_stride,
                                                      size_t npx, RetimeArgs R, uint32_t sel)
{
    const RetimeTimes T(R, blockIdx.y);
    if (T.count() == 0) return;
    const uint32_t *pa = reinterpret_cast<const uint32_t *>(a + (size_t)blockIdx.y * frame_stride);
    const uint32_t *pb = reinterpret_cast<const uint32_t *>(b + (size_t)blockIdx.y * frame_stride);
    const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * (VEC ? 4 : 1);
    if (i >= npx) return;
    if (VEC) {
        const uint4 va = *reinterpret_cast<const uint4 *>(pa + i);
        const uint4 vb = *reinterpret_cast<const uint4 *>(pb + i);
        for (uint32_t k = 0; k < T.count(); ++k) {
            float t = T.time(k);
            asm volatile("" : "+v"(t)); // per-lane copy (scalar operands halve the VALU issue rate on gfx950)
            const float nt = 1.0f - t;
            store_out16<false>(T.frame(k, npx) + i, swz4(make_uint4(blend_px(va.x, vb.x, t, nt), blend_px(va.y, vb.y, t, nt),
                                                                  blend_px(va.z, vb.z, t, nt), blend_px(va.w, vb.w, t, nt)), sel));
        }
    } else {
        const uint32_t va = pa[i], vb = pb[i];
        for (uint32_t k = 0; k < T.count(); ++k) {
            float t = T.time(k);
            asm volatile("" : "+v"(t));
            T.frame(k, npx)[i] = swz(blend_px(va, vb, t, 1.0f - t), sel);
        }
    }
}

// Real-frame outputs.  grid.y: frames of the launch; frame k = first_pair + blockIdx.y is an output iff den divides k num.
template <bool VEC>
__global__ __launch_bounds__(256) void k_retime_real(const uint8_t *__restrict__ frames, size_t frame_stride, size_t npx, RetimeArgs R,
                                                     uint32_t sel)
{
    const uint64_t at = ((uint64_t)R.first_pair + blockIdx.y) * R.num, j = at / R.den;
    if (j * R.den != at) return;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(frames + (size_t)blockIdx.y * frame_stride);
    uint32_t *dst = reinterpret_cast<uint32_t *>(R.out + j * R.out_frame_stride);
    const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * (VEC ? 4 : 1);
    if (i >= npx) return;
    if (VEC) {
        store_out16<false>(dst + i, swz4(*reinterpret_cast<const uint4 *>(src + i), sel));
    } else {
        dst[i] = swz(src[i], sel);
    }
}

// The cut rule.  grid.y: pairs of the launch; a pair that is not cut leaves after one flag load.
template <bool VEC>
__global__ __launch_bounds__(256) void k_retime_scene_apply(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, size_t frame_stride,
                                                            size_t npx, const uint8_t *__restrict__ cut, RetimeArgs R, uint32_t sel)
{
    if (cut[blockIdx.y] == 0) return;
    const RetimeTimes T(R, blockIdx.y);
    if (T.count() == 0) return;
    const uint32_t *pa = reinterpret_cast<const uint32_t *>(a + (size_t)blockIdx.y * frame_stride);
    const uint32_t *pb = reinterpret_cast<const uint32_t *>(b + (size_t)blockIdx.y * frame_stride);
    const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * (VEC ? 4 : 1);
    if (i >= npx) return;
    if (VEC) {
        const uint4 va = swz4(*reinterpret_cast<const uint4 *>(pa + i), sel), vb = swz4(*reinterpret_cast<const uint4 *>(pb + i), sel);
        for (uint32_t k = 0; k < T.count(); ++k) *reinterpret_cast<uint4 *>(T.frame(k, npx) + i) = T.time(k) < 0.5f ? va : vb;
    } else {
        const uint32_t va = swz(pa[i], sel), vb = swz(pb[i], sel);
        for (uint32_t k = 0; k < T.count(); ++k) T.frame(k, npx)[i] = T.time(k) < 0.5f ? va : vb;
    }
}

// One thread per frame k: the entries of pair k's outputs, real frame included; the last frame has no pair behind it and writes its
// own entry alone.
__global__ __launch_bounds__(256) void k_retime_table(uint32_t n_frames, uint32_t num, uint32_t den, RetimeEntry *__restrict__ entries)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_frames) return;
    const RetimePair p = retime_pair(k, num, den);
    const uint32_t cnt = k + 1 < n_frames ? p.count : (p.rem0 == 0 ? 1u : 0u);
    for (uint32_t i = 0; i < cnt; ++i) {
        const uint32_t rem = p.rem0 + i * den;
        entries[p.first + i] = RetimeEntry{k, rem, retime_time(rem, num), 0u};
    }
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) % 16) == 0; }

inline bool retime_launch_ok(const RetimeLaunch &L)
{
    return L.frames && L.out && L.num >= 1 && L.den >= 1 && L.w && L.h && L.frame_stride >= (size_t)L.w * L.h * 4 &&
           L.out_frame_stride >= (size_t)L.w * L.h * 4;
}

// the streaming kernels' shape: 4 pixels per lane where every base and stride allows 16-byte accesses
struct StreamShape {
    bool vec;
    dim3 grid(uint32_t n) const { return dim3(blocks, n); }
    uint32_t blocks;
};
inline StreamShape stream_shape(const RetimeLaunch &L, const uint8_t *frames)
{
    const size_t npx = (size_t)L.w * L.h;
    StreamShape s;
    s.vec = (npx % 4) == 0 && (L.frame_stride % 16) == 0 && (L.out_frame_stride % 16) == 0 && aligned16(frames) && aligned16(L.out);
    const size_t items = s.vec ? npx / 4 : npx;
    s.blocks = (uint32_t)((items + 255) / 256);
    return s;
}

} // namespace

hipError_t launch_retime_warp(const RetimeLaunch &L, const RetimeWarp &V)
{
    if (!retime_launch_ok(L) || V.project > kFlowMaxProject) return hipErrorInvalidValue;
    if (V.flow_bwd != nullptr && (V.flow == nullptr || V.vectors != nullptr)) return hipErrorInvalidValue; // the select warp takes both flows, and flows only
    const size_t npx = (size_t)L.w * L.h;
    const uint32_t cell_bytes = V.flow_half ? 4 : 8;
    uint32_t lg = 3;
    while ((1u << lg) < V.bs) ++lg;
    const uint32_t blocks_x = cdiv(L.w, V.bs), blocks_y = cdiv(L.h, V.bs);
    return for_grid_z_chunks(L.n_pairs, [&](uint32_t done, uint32_t n) {
        const uint8_t *a = L.frames + (size_t)done * L.frame_stride, *b = a + L.frame_stride;
        const RetimeArgs R{L.out, L.out_frame_stride, L.first_pair + done, L.num, L.den};
        const dim3 block(kWave, 4);
        // a pair of pixels per thread: the 8-byte store's alignment in every output frame
        const bool pair_ok = (L.w % 2) == 0 && (reinterpret_cast<uintptr_t>(L.out) % 8) == 0 && (L.out_frame_stride % 8) == 0;
        if (V.vectors != nullptr) {
            const short2 *vec = reinterpret_cast<const short2 *>(V.vectors) + (size_t)done * blocks_x * blocks_y;
            if (!warp_corner_ok(L.w, L.h, 0)) {
                hipLaunchKernelGGL(k_retime_warp_tiny<kTinyBlocks>, warp_grid(L.w, L.h, 1, 1, n), block, 0, L.stream, a, b,
                                   static_cast<const void *>(vec), false, L.frame_stride, L.w, L.h, R, kSelRGBA, 0u, lg, blocks_x, blocks_y);
                return;
            }
            static constexpr decltype(&k_retime_bm<kWarpExact, 1, kWarpRV>) kernels[2][2] = { // [fma][pair]
                {k_retime_bm<kWarpExact, 1, kWarpRV>, k_retime_bm<kWarpExact, 2, kWarpRV>},
                {k_retime_bm<kWarpFma, 1, kWarpRV>, k_retime_bm<kWarpFma, 2, kWarpRV>}};
            hipLaunchKernelGGL(kernels[V.fma][pair_ok], warp_grid(L.w, L.h, pair_ok ? 2 : 1, kWarpRV, n), block, 0, L.stream, a, b, vec,
                               L.frame_stride, L.w, L.h, R, lg, blocks_x, blocks_y);
            return;
        }
        if (V.flow == nullptr) {
            const StreamShape s = stream_shape(L, a);
            if (s.vec)
                hipLaunchKernelGGL(k_retime_blend<true>, s.grid(n), dim3(256), 0, L.stream, a, b, L.frame_stride, npx, R, L.in_sel);
            else
                hipLaunchKernelGGL(k_retime_blend<false>, s.grid(n), dim3(256), 0, L.stream, a, b, L.frame_stride, npx, R, L.in_sel);
            return;
        }
        const void *fl = static_cast<const uint8_t *>(V.flow) + (size_t)done * npx * cell_bytes;
        if (V.flow_bwd != nullptr) { // the select warp, with or without projection rounds
            const void *fr = static_cast<const uint8_t *>(V.flow_bwd) + (size_t)done * npx * cell_bytes;
            if (!warp_corner_ok(L.w, L.h, cell_bytes)) {
                hipLaunchKernelGGL(k_retime_flow_sel_tiny, warp_grid(L.w, L.h, 1, 1, n), block, 0, L.stream, a, b, fl, fr, V.flow_half,
                                   L.frame_stride, L.w, L.h, R, L.in_sel, V.project);
                return;
            }
#define NUS_RS(M, H) {k_retime_flow_sel<M, H, 1, kSelRV[0]>, k_retime_flow_sel<M, H, 2, kSelRV[1]>}
            static constexpr decltype(&k_retime_flow_sel<kWarpExact, false, 1, kSelRV[0]>) kernels[2][2][2] = { // [fma][half][pair]
                {NUS_RS(kWarpExact, false), NUS_RS(kWarpExact, true)}, {NUS_RS(kWarpFma, false), NUS_RS(kWarpFma, true)}};
#undef NUS_RS
            // (the select tile's rows per thread are its own: kSelRV, not kWarpRV)
            hipLaunchKernelGGL(kernels[V.fma][V.flow_half][pair_ok], warp_grid(L.w, L.h, pair_ok ? 2 : 1, kSelRV[pair_ok], n), block, 0, L.stream, a,
                               b, fl, fr, L.frame_stride, L.w, L.h, R, L.in_sel, V.project);
            return;
        }
        if (V.project > 0) {
            if (!warp_corner_ok(L.w, L.h, cell_bytes)) {
                hipLaunchKernelGGL(k_retime_warp_tiny<kTinyProjected>, warp_grid(L.w, L.h, 1, 1, n), block, 0, L.stream, a, b, fl, V.flow_half,
                                   L.frame_stride, L.w, L.h, R, L.in_sel, V.project, 0u, 0u, 0u);
                return;
            }
#define NUS_RP(M, H) {k_retime_flow_proj<M, H, 1, kWarpRV>, k_retime_flow_proj<M, H, 2, kWarpRV>}
            static constexpr decltype(&k_retime_flow_proj<kWarpExact, false, 1, kWarpRV>) kernels[2][2][2] = { // [fma][half][pair]
                {NUS_RP(kWarpExact, false), NUS_RP(kWarpExact, true)}, {NUS_RP(kWarpFma, false), NUS_RP(kWarpFma, true)}};
#undef NUS_RP
            hipLaunchKernelGGL(kernels[V.fma][V.flow_half][pair_ok], warp_grid(L.w, L.h, pair_ok ? 2 : 1, kWarpRV, n), block, 0, L.stream, a, b,
                               fl, L.frame_stride, L.w, L.h, R, L.in_sel, V.project);
            return;
        }
        if (!warp_corner_ok(L.w, L.h, 0)) { // (the flow is read through 64-bit addresses: no bound on its plane)
            hipLaunchKernelGGL(k_retime_warp_tiny<kTinyDense>, warp_grid(L.w, L.h, 1, 1, n), block, 0, L.stream, a, b, fl, V.flow_half,
                               L.frame_stride, L.w, L.h, R, L.in_sel, 0u, 0u, 0u, 0u);
            return;
        }
        const bool xv_ok = pair_ok && aligned16(fl); // its f32 flow vectors are one 16-byte load
#define NUS_RF(M, H) {k_retime_flow<M, H, 1, kWarpRV>, k_retime_flow<M, H, 2, kWarpRV>}
        static constexpr decltype(&k_retime_flow<kWarpExact, false, 1, kWarpRV>) kernels[2][2][2] = { // [fma][half][pair]
            {NUS_RF(kWarpExact, false), NUS_RF(kWarpExact, true)}, {NUS_RF(kWarpFma, false), NUS_RF(kWarpFma, true)}};
#undef NUS_RF
        hipLaunchKernelGGL(kernels[V.fma][V.flow_half][xv_ok], warp_grid(L.w, L.h, xv_ok ? 2 : 1, kWarpRV, n), block, 0, L.stream, a, b, fl,
                           L.frame_stride, L.w, L.h, R, L.in_sel);
    });
}

hipError_t launch_retime_real(const RetimeLaunch &L, uint32_t n_frames)
{
    if (!retime_launch_ok(L)) return hipErrorInvalidValue;
    const size_t npx = (size_t)L.w * L.h;
    return for_grid_z_chunks(n_frames, [&](uint32_t done, uint32_t n) {
        const uint8_t *frames = L.frames + (size_t)done * L.frame_stride;
        const RetimeArgs R{L.out, L.out_frame_stride, L.first_pair + done, L.num, L.den};
        const StreamShape s = stream_shape(L, frames);
        if (s.vec)
            hipLaunchKernelGGL(k_retime_real<true>, s.grid(n), dim3(256), 0, L.stream, frames, L.frame_stride, npx, R, L.in_sel);
        else
            hipLaunchKernelGGL(k_retime_real<false>, s.grid(n), dim3(256), 0, L.stream, frames, L.frame_stride, npx, R, L.in_sel);
    });
}

hipError_t launch_scene_apply_retime(const RetimeLaunch &L, const uint8_t *cut)
{
    if (!retime_launch_ok(L) || !cut) return hipErrorInvalidValue;
    const size_t npx = (size_t)L.w * L.h;
    return for_grid_z_chunks(L.n_pairs, [&](uint32_t done, uint32_t n) {
        const uint8_t *a = L.frames + (size_t)done * L.frame_stride, *b = a + L.frame_stride;
        const RetimeArgs R{L.out, L.out_frame_stride, L.first_pair + done, L.num, L.den};
        const StreamShape s = stream_shape(L, a);
        if (s.vec)
            hipLaunchKernelGGL(k_retime_scene_apply<true>, s.grid(n), dim3(256), 0, L.stream, a, b, L.frame_stride, npx, cut + done, R, L.in_sel);
        else
            hipLaunchKernelGGL(k_retime_scene_apply<false>, s.grid(n), dim3(256), 0, L.stream, a, b, L.frame_stride, npx, cut + done, R, L.in_sel);
    });
}

hipError_t launch_retime_table(uint32_t n_frames, uint32_t num, uint32_t den, void *entries, hipStream_t stream)
{
    if (n_frames < 2 || num == 0 || den == 0 || !entries) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_retime_table, dim3((uint32_t)(((uint64_t)n_frames + 255) / 256)), dim3(256), 0, stream, n_frames, num, den, static_cast<RetimeEntry *>(entries));
    return hipGetLastError();
}

} // namespace nus
