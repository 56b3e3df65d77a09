// nus_kernels.hpp -- launch interface between the host classes and the gfx950 kernels.
// Everything here is device-pointer based; no allocation, no synchronisation
// (safe to capture into a hipGraph).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "nus_plan.hpp" // Variant, variant_name(), lanczos_pq_supported(): the kernel selection, HIP-free

namespace nus {

// Device-side tables of one initialised upscaler (built on the host by nus_tables.cpp).
struct DeviceTables {
    // nearest: source index per output index
    const uint32_t *nn_sx = nullptr, *nn_sy = nullptr;
    // bilinear: i0 and fraction per output index
    const uint32_t *bl_x0 = nullptr, *bl_y0 = nullptr;
    const float *bl_fx = nullptr, *bl_fy = nullptr;
    // lanczos general: tap window per output index, weights [n][taps_stride]
    const int32_t *lz_lx = nullptr, *lz_ly = nullptr;
    const uint32_t *lz_nx = nullptr, *lz_ny = nullptr;
    const float *lz_wx = nullptr, *lz_wy = nullptr;
    uint32_t lz_stride = 0;
    // down-scaling stream kernel: per input row 7 slot weights + completion word, and the completing row per output row
    const uint32_t *lz_down_rows = nullptr;
    const int32_t *lz_down_done = nullptr;
    // lanczos x2 fast path: per-output-row weights in the 6-tap phase frame [oh][6]
    const float *lz_wy6 = nullptr;
    const float *lz_wx6 = nullptr; // P/Q kernel: per-output-column weights in the 6-tap phase frame [ow][6]
    float lz_wxe[6] = {0}, lz_wxo[6] = {0}; // interior horizontal weights, even / odd outputs
    float lz_wx_left[48] = {0}, lz_wx_right[48] = {0}; // phase-frame weights of the 8 edge outputs per side
    float lz_wxs[4][6] = {{0}};                        // integer factors x3 / x4: interior weights per phase
    float lz_wxs_left[16][6] = {{0}}, lz_wxs_right[16][6] = {{0}}; // ... and of the 4 S edge outputs per side
    // x3: interior weights by class of the input index (nus_tables.hpp: lanczos_xs_weight_classes); null at x4
    const uint32_t *lz_xs_cls_x = nullptr, *lz_xs_cls_y = nullptr; // [iw], [ih]
    const float *lz_xs_wcls_x = nullptr, *lz_xs_wcls_y = nullptr;  // [classes][S][6]
};

// v_perm_b32 selectors applied to every loaded input pixel: RGBA8 as is, or BGRA8 (capture order,
// nu_scaler_core/src/lib.rs:251-270) swizzled to RGBA on the way in.
constexpr uint32_t kSelRGBA = 0x03020100u, kSelBGRA = 0x03000102u;
// ... and the X variants (alpha byte undefined, as BGRX capture surfaces): selector byte 0x0D yields 0xFF, so the
// pixel enters every kernel opaque and the output alpha is 255.
constexpr uint32_t kSelRGBX = 0x0D020100u, kSelBGRX = 0x0D000102u;
inline uint32_t input_selector(int format) // nus_pixel_format
{
    switch (format) {
    case 1: return kSelBGRA;
    case 2: return kSelRGBX;
    case 3: return kSelBGRX;
    default: return kSelRGBA;
    }
}

struct UpscaleLaunch {
    const uint8_t *in = nullptr; // n_frames contiguous frames
    uint8_t *out = nullptr;
    uint32_t iw = 0, ih = 0, ow = 0, oh = 0;
    uint32_t n_frames = 1;
    hipStream_t stream = nullptr;
    // x2 resize kernels only: input frame stride in bytes (0 = tightly packed), and an optional
    // second frame per unit to blend with on the fly (zero-flow in-between frame at blend_t)
    size_t in_stride = 0;
    const uint8_t *in_b = nullptr;
    size_t in_b_stride = 0;
    float blend_t = 0.5f;
    uint32_t in_sel = kSelRGBA; // input channel order
    // Exact-x2 kernels only (nearest, bilinear, the resize filters): input rows [row0, row0 + rows) of the frame instead of all
    // of it (rows == 0: all).  The kernels still see the whole frame -- tap rows beyond the range are read, not clamped -- so the
    // host path can upscale a frame band by band while the rest of it is still on the bus (HipUpscaler::upscale).  row0 must be
    // a multiple of the kernel's rows per wave (launch_lanczos_x2's rows_per_wave; 4 for the others).
    uint32_t row0 = 0, rows = 0;
};

hipError_t launch_nearest_table(const UpscaleLaunch &L, const DeviceTables &T);
hipError_t launch_nearest_x2(const UpscaleLaunch &L);
hipError_t launch_nearest_ratio(const UpscaleLaunch &L); // exact x3/2, x4/3, x3, x4 (host-checked table shape: source index Q (o / P) + (o % P) Q / P)
hipError_t launch_bilinear_table(const UpscaleLaunch &L, const DeviceTables &T, bool wgsl_form);
hipError_t launch_bilinear_x2_int(const UpscaleLaunch &L);
// exact x3/2, x4/3, x3, x4, CPU form (host-checked table shape: i0 = Q (o / P) + (o % P) Q / P, fraction 0 where (o % P) Q % P == 0)
hipError_t launch_bilinear_ratio(const UpscaleLaunch &L, const DeviceTables &T);
// edge_only: evaluate only the first and last `edge_cols` output columns.
hipError_t launch_lanczos_general(const UpscaleLaunch &L, const DeviceTables &T, bool exact,
                                  uint32_t edge_cols);
// ncols_max: widest input-column footprint of a 64*N-column output segment (LDS row length);
// small_taps: every tap window has <= 8 taps.
// union_taps: widest union of the tap windows of 4 adjacent outputs (x % 4 == 0), 0 = unknown / do not use.
hipError_t launch_resize_rows(const UpscaleLaunch &L, const DeviceTables &T, bool exact, uint32_t ncols_max,
                              bool small_taps, uint32_t union_taps);
// Up-scaling variant (ow % 4 == 0, <= 7 vertical / <= 8 horizontal taps, first tap row advancing by <= 1
// per output row, ncols_max <= 192): vertical taps from a register window.
// outputs_per_lane: 4 (segments of 256 output columns) or 2 (segments of 128); ncols_max and union_taps are for that width.
hipError_t launch_resize_win(const UpscaleLaunch &L, const DeviceTables &T, bool exact, uint32_t ncols_max,
                             uint32_t union_taps, uint32_t outputs_per_lane);
// Down-scaling variant (nus_k_resize_down.hip): needs T.lz_down_rows / lz_down_done (build_down_stream_tables
// succeeded: 7 accumulator slots suffice), seg_w = output columns per wave (<= 64), ncols_max = widest footprint of a
// seg_w-column output segment <= 320.  max_taps_x: widest horizontal window (<= 32).
hipError_t launch_resize_down(const UpscaleLaunch &L, const DeviceTables &T, bool exact, uint32_t ncols_max,
                              uint32_t max_taps_x, uint32_t seg_w);
// main x2 kernel only: the first / last kLanczosX2EdgeCols output columns are NOT written;
// follow it with launch_lanczos_x2_edges(L, T, exact).
hipError_t launch_lanczos_x2(const UpscaleLaunch &L, const DeviceTables &T, bool exact,
                             uint32_t rows_per_wave);

hipError_t launch_lanczos_x2_edges(const UpscaleLaunch &L, const DeviceTables &T, bool exact);
// One pipeline step over n_frames pairs (L.in = A_k, L.in_b = B_k) in ONE launch of the x2 kernel: L.out = the up-scaled real
// frames, out_mid = the up-scaled in-between frames (blend of the pair at L.blend_t), mid = the in-between frames themselves
// (n_frames tightly packed input-size frames; may be null).  order: 0 = frame-major, 1 = row-block-major wave order.
// Main kernel only: follow it with launch_lanczos_x2_edges for both outputs.
struct UnitOutputs {
    uint8_t *out_mid = nullptr;
    uint8_t *mid = nullptr;
    uint32_t order = 1;
};
hipError_t launch_lanczos_x2_unit(const UpscaleLaunch &L, const DeviceTables &T, bool exact, uint32_t rows_per_wave,
                                  const UnitOutputs &U);
// exact x3 / x4 (factor): main kernel only, the first / last 4 * factor output columns are NOT written;
// follow it with launch_lanczos_xs_edges(L, T, exact, factor).
hipError_t launch_lanczos_xs(const UpscaleLaunch &L, const DeviceTables &T, bool exact, uint32_t factor,
                             uint32_t rows_per_wave);
hipError_t launch_lanczos_xs_edges(const UpscaleLaunch &L, const DeviceTables &T, bool exact, uint32_t factor);
// exact x3/2 (2 ow == 3 iw, 2 oh == 3 ih, iw % 8 == 0, ih even): main kernel only, the first / last 12 output columns are
// NOT written; follow it with launch_lanczos_r32_edges(L, T, exact).
hipError_t launch_lanczos_r32(const UpscaleLaunch &L, const DeviceTables &T, bool exact, uint32_t rows_per_wave);
hipError_t launch_lanczos_r32_edges(const UpscaleLaunch &L, const DeviceTables &T, bool exact);
// exact x4/3 (3 ow == 4 iw, 3 oh == 4 ih, iw % 12 == 0): main kernel only, the first / last 8 output columns are NOT written;
// follow it with launch_lanczos_r43_edges(L, T, exact).
hipError_t launch_lanczos_r43(const UpscaleLaunch &L, const DeviceTables &T, bool exact, uint32_t rows_per_wave);
hipError_t launch_lanczos_r43_edges(const UpscaleLaunch &L, const DeviceTables &T, bool exact);
// x5/4, x6/5, x7/5, x8/5, x5/3, x5/2, x7/2 (Q ow == P iw, Q oh == P ih, iw % Q == 0, ih % Q == 0, ow % 4 == 0; T.lz_wx6 / T.lz_wy6: the tables in frame form,
// nus_tables.hpp: lanczos_pq_phase_frame).  Writes every output column: no edge pass.
uint32_t lanczos_pq_strip_cols(uint32_t P, uint32_t Q); // input columns per wave
hipError_t launch_lanczos_pq(const UpscaleLaunch &L, const DeviceTables &T, bool exact, uint32_t P, uint32_t Q, uint32_t rows_per_wave,
                             bool narrow);
// FSR1-style passes (fsr.rs:24-260).  mode 0: EASU, 1: RCAS (iw == ow, ih == oh), 2: EASU then RCAS fused.
// fast: EASU in FAST arithmetic where the LDS source tile applies (nus_k_fsr.hip; option "fsr_fast")
hipError_t launch_fsr1(const UpscaleLaunch &L, int mode, float easu_sharpness, float rcas_sharpness, bool fast = false);

constexpr uint32_t kLanczosX2EdgeCols = 8; // output columns left to the general kernel per side
#ifndef NUS_LZ_STRIP_COLS
#define NUS_LZ_STRIP_COLS 240 // 60 storing lanes: a strip's output rows are whole 128-B lines (x2: 1920 B = 15 lines; 1080p is 8
                             // strips exactly); 248 = all 62 non-halo lanes storing, strip joints in mid-line (dev macro, A/B)
#endif
constexpr uint32_t kLanczosX2StripCols = NUS_LZ_STRIP_COLS; // input columns produced per wave (lanes 1 .. StripCols / 4, 4 columns each)

// The in-between times of one warp + blend launch, passed by value in the kernel arguments (no device buffer, no copy): every
// pair's A, B and flow are read once and the frame of each time is stored (NUS_INTERP_MAX_TIMES in the C header).
constexpr uint32_t kInterpMaxTimes = 7;
struct TimeSet {
    float t[kInterpMaxTimes];
    uint32_t n;
};

struct WarpLaunch {
    const uint8_t *a = nullptr, *b = nullptr;
    const float *flow = nullptr; // nullptr: zero flow
    bool flow_half = false;      // the flow field is 2 x f16 per pixel (Rg16Float, wgpu_interpolator.rs:276), not 2 x f32
    bool fma = false;            // dense-flow warp in fused multiply-adds (+-1 LSB) instead of the CPU's separate roundings
    uint8_t *out = nullptr;
    size_t a_stride = 0, b_stride = 0; // bytes between consecutive pairs
    uint32_t w = 0, h = 0;
    float t = 0.5f;
    const float *times = nullptr; // n_times > 0: the frames at times[0 .. n_times) instead of the one at t
    uint32_t n_times = 0;
    size_t out_pair_stride = 0; // bytes between the outputs of consecutive pairs; 0: the pair's frames tightly packed
    uint32_t n_pairs = 1;
    hipStream_t stream = nullptr;
    uint32_t in_sel = kSelRGBA; // channel order of both input frames (the output is RGBA)
    uint32_t project = 0;       // projection rounds (0 .. kFlowMaxProject) of the dense-flow warp: see launch_warp_blend_project
};

// Frame k of pair i goes to out + i * out_pair_stride + k * w * h * 4.  One time runs the single-time kernels; more, their
// multi-time instantiations (the same per-pixel arithmetic, looped over the times after the loads).  With project > 0 and a flow
// it hands the launch to launch_warp_blend_project.  The dense-flow kernels of both and launch_bm_warp's are one tile body
// (warp_blend_tile, nus_warp_device.hpp) fed from three vector sources; the three launchers share its host helpers.
hipError_t launch_warp_blend(const WarpLaunch &L);

// The flow evaluated at the in-between time (nus_k_warp_project.hip; BUILD-DEFINED).  Per output pixel p and time t: g = f(p), then
// `project` rounds of g = bilinear f at clamp(p - t g) -- separate roundings in both warp modes -- then the warp + blend of
// launch_warp_blend with g in place of f(p).  Every gather stays inside its own pair's flow plane.  L.flow != nullptr, 1 <= L.project.
constexpr uint32_t kFlowMaxProject = 4; // NUS_FLOW_MAX_PROJECT
hipError_t launch_warp_blend_project(const WarpLaunch &L);

// The select warp (nus_k_warp_select.hip; BUILD-DEFINED): two flows per pair, warp.flow = F (A -> B, on A's grid) and flow_bwd = R
// (B -> A, on B's grid), both in warp.flow_half's format, pair i's planes at i * w * h cells.  Per output pixel and time t the
// candidates are gF = F projected warp.project (0 .. kFlowMaxProject) rounds at t and gR = -(R projected as many rounds at 1 - t);
// each is sampled as launch_warp_blend samples; the pixel is the blend of the samples of the candidate whose two samples differ
// less over the three colour bytes (a tie: the forward one).  Times, pair split and output layout are launch_warp_blend's.
struct WarpSelectLaunch {
    WarpLaunch warp;
    const float *flow_bwd = nullptr;
};
hipError_t launch_warp_blend_select(const WarpSelectLaunch &L);

// BGRA -> RGBA (in place allowed: in == out).
hipError_t launch_swizzle_bgra(const uint8_t *in, uint8_t *out, size_t npx, hipStream_t stream);

// Optical-flow front end (f32 RGBA images, float2 flows; device pointers).
hipError_t launch_rgba8_to_f32(const uint8_t *in, float *out, uint32_t w, uint32_t h, hipStream_t stream);
hipError_t launch_blur(const float *in, float *out, uint32_t w, uint32_t h, bool horizontal, hipStream_t stream);
hipError_t launch_downsample(const float *in, float *out, uint32_t w, uint32_t h, hipStream_t stream);
hipError_t launch_horn_schunck(const float *i1, const float *i2, const float *flow_in, float *flow_out, uint32_t w,
                               uint32_t h, float lambda, hipStream_t stream);
// What the batch launchers below share: `n` independent images / pairs of w x h on the grid's z (streamed kernels: y) axis.
struct FlowImages {
    uint32_t w = 0, h = 0;
    uint32_t n = 1; // buffer b of item z is at b + z * (b's stride member); n = 1 ignores the strides
    hipStream_t stream = nullptr;
};
// `kernel`: LDS-tile or register-pipelined ("streamed") form of the pyramid and the multi-step Jacobi kernels
enum JacobiKernel { kJacobiAuto = 0, kJacobiTiles = 1, kJacobiStream = 2, kJacobiStreamFast = 3 }; // Fast: k_hs_stream_fast, every level
// blur H + blur V + downsample of one level in one launch; the level itself is written as its luminance plane (w*h floats),
// which is all Horn-Schunck reads of it.
struct PyramidLevelLaunch {
    FlowImages img;
    const void *in = nullptr; // RGBA8 (u8_input) or f32 RGBA; launch_pyramid_level_fast: RGBA8 or the previous level's `next`
    bool u8_input = false;
    float *level_lum = nullptr;
    float *next = nullptr; // input of the next level, quarter size: f32 RGBA (fast: one float per pixel); null at the last level
    size_t in_stride = 0;  // in bytes for an RGBA8 input, else in elements of the buffer (float4, or float for the fast kernel)
    size_t lum_stride = 0, next_stride = 0; // in floats; in float4 for the exact kernels' `next`
};
hipError_t launch_pyramid_level(const PyramidLevelLaunch &L, int kernel);
hipError_t launch_pyramid_level_fast(const PyramidLevelLaunch &L); // k_pyramid_fast: luminance only
// Derivatives once per level: coef = 3 floats (ix, iy, it) per cell.
struct HsPrepareLaunch {
    FlowImages img;
    const float *i1 = nullptr, *i2 = nullptr; // f32 RGBA level images, or their luminance planes (luminance_planes)
    bool luminance_planes = false;
    float *coef = nullptr;
    size_t img_stride = 0, coef_stride = 0; // in pixels of the images; in floats
};
hipError_t launch_hs_prepare(const HsPrepareLaunch &L);
// The flow of the next coarser level (cw x ch), which a level continues: upsampled to w x h, its vectors times `scale`.
struct HsCoarseFlow {
    const float *flow = nullptr; // null: none
    uint32_t w = 0, h = 0;
    float scale = 0.0f;
    size_t stride = 0; // in cells (float2)
};
// launch_hs_prepare on luminance planes + launch_flow_upsample of `coarse` into `flow` (item stride in cells), one launch.
hipError_t launch_hs_level_setup(const HsPrepareLaunch &L, const HsCoarseFlow &coarse, float *flow, size_t flow_stride);
// The level setup of a re-linearisation round (FlowParams::warps): frame B's luminance sampled bilinearly through the level's current
// flow f0, and the triple (Ix, Iy, It' = L2w - L1 - Ix u0 - Iy v0) into L.coef.  `coarse` set (round 1): f0 is that flow upsampled, and
// it is stored at flow_out; else f0 is `flow` (null: zero flow -- launch_hs_prepare's triple).  L.i1 / L.i2 are only read.
hipError_t launch_hs_warp_setup(const HsPrepareLaunch &L, const HsCoarseFlow &coarse, const float *flow, size_t flow_stride, float *flow_out,
                                size_t flow_out_stride);
// n cells of 2 x f32 -> 2 x f16 (round to nearest even)
hipError_t launch_flow_to_half(const float *src, void *dst, size_t n_cells, hipStream_t stream);
// `iterations` Jacobi steps of one level, K per launch (derivatives once per level, the steps in LDS tiles or a register pipeline).
struct HsIterateLaunch {
    FlowImages img;
    const float *coef = nullptr; // launch_hs_prepare's coefficients; or, for the kernel to take the derivatives from as it goes where
    const float *lum1 = nullptr; // the level streams (hs_iterate_streams): the luminance plane of the pair's first frame, the second's
    size_t coef_stride = 0, lum_stride = 0; // one lum_stride further
    float lambda = 0.0f;
    uint32_t iterations = 0; // split evenly over the launches
    bool zero_start = false; // from zero flow, without reading flow_a
    float *flow_a = nullptr, *flow_b = nullptr; // ping-pong, the flow so far in flow_a
    float *final_out = nullptr;                 // set: the last launch writes here instead
    size_t flow_stride = 0, final_stride = 0;   // in cells (float2)
    int kernel = kJacobiAuto;
    HsCoarseFlow coarse; // streamed kernels on luminance planes: the first launch starts from this flow, upsampled as it loads it
    // the level's FINAL flow as 2 x IEEE half per cell (round to nearest even) instead of 2 x f32: the reference's live flow layout,
    // Rg16Float (wgpu_interpolator.rs:276), for a warp that reads it that way.  Honoured if the last launch is the FAST streamed
    // kernel (HsIterateResult::wrote_half says so); everything else leaves f32 and the caller converts (launch_flow_to_half).
    bool final_half = false;
};
struct HsIterateResult {
    float *flow = nullptr, *spare = nullptr; // where the result is (final_out, if given), and the other buffer of the ping-pong
    bool wrote_half = false;                 // the last launch stored halves (L.final_half)
};
hipError_t launch_hs_iterate(const HsIterateLaunch &L, HsIterateResult *result);
bool hs_iterate_streams(uint32_t w, uint32_t h, uint32_t n, int kernel);
// bilinear upsample of `coarse` into D.n flows of D.w x D.h at dst (item stride in cells)
hipError_t launch_flow_upsample(const FlowImages &D, const HsCoarseFlow &coarse, float *dst, size_t dst_stride);
// Component-wise size x size median (3 or 5) of img.n flows of img.w x img.h (nus_k_flow_median.hip; FlowParams::median): the
// window centred on the cell, coordinates clamped into the flow.  `in` and `out` must not overlap (one tile's halo is another's
// output); strides in cells (float2).
struct FlowMedianLaunch {
    FlowImages img;
    uint32_t size = 3;
    const float *in = nullptr;
    float *out = nullptr;
    size_t in_stride = 0, out_stride = 0;
};
hipError_t launch_flow_median(const FlowMedianLaunch &L);
// The projection alone: out = g after `rounds` rounds (0 .. kFlowMaxProject) at time t, for img.n tightly packed f32 flows of
// img.w x img.h; the device function of the projecting warp kernels.  `in` and `out` must not overlap (a cell gathers its neighbours).
struct FlowProjectLaunch {
    FlowImages img;
    float t = 0.5f;
    uint32_t rounds = 1;
    const float *in = nullptr;
    float *out = nullptr;
};
hipError_t launch_flow_project(const FlowProjectLaunch &L);

// Box calibration (nus_k_probe.hip; bench.py's denominators, not on the product path): kind 0 hipMemcpyDtoDAsync, 1 stream
// copy, 2 write-only, 3 read-only (d_dst: 4 bytes of device memory), 4 one read : four writes (d_dst holds 4 * bytes),
// 5 VGPR-only FMA chains (kProbeValuBlocks blocks of 256 lanes, 16 chains of `iters` FMAs each; d_dst: that many floats).
constexpr uint32_t kProbeValuBlocks = 2048;
hipError_t launch_probe(int kind, const void *d_src, void *d_dst, size_t bytes, uint32_t iters, hipStream_t stream);

// Image-quality metrics of frame pairs (nus_k_metrics.hip; nus_metrics_* in include/nuscaler_hip.h).  Frame i of A at
// a + i * a_stride, of B at b + i * b_stride (4-byte aligned); the workspace holds per-block partials -- u64 SSE at
// sse_offset, f64 SSIM at ssim_offset -- and out receives [mse, psnr, ssim] per frame (NaN for what was not asked).
// SSIM needs w, h >= 11.  Kernels: k_metrics_sse (MSE alone), k_metrics_ssim (SSIM, with the SSE when both are asked),
// k_metrics_finish.
constexpr uint32_t kMetricsBlock = 256; // lanes per workgroup of every metrics kernel
struct MetricsShape {
    uint32_t sse_blocks = 0, ssim_blocks = 0; // partials per frame
    uint32_t tiles_x = 0, tiles_y = 0;        // SSIM tiles per frame
    size_t sse_offset = 0, ssim_offset = 0, workspace_bytes = 0;
};
MetricsShape metrics_shape(uint32_t w, uint32_t h, uint32_t frames, bool mse, bool ssim); // host only, no device needed
hipError_t launch_metrics(const uint8_t *a, size_t a_stride, const uint8_t *b, size_t b_stride, uint32_t w, uint32_t h,
                          uint32_t frames, bool mse, bool ssim, void *workspace, double *out, hipStream_t stream);

// Block-matching motion estimation (nus_k_blockmatch.hip; nus_bm_* in include/nuscaler_hip.h).  Pair i reads A at
// a + i * a_stride and B at b + i * b_stride (4-byte aligned); block (bx, by) of pair i is entry (i * blocks_y + by) * blocks_x + bx
// of vectors (2 x int16: dx, dy), sad and flags.  The workspace holds the raw winners (2 x int16 per block) and, at rough_offset,
// one word per 256 blocks for the smoothness test.  With the forward-backward check (bidir) it also holds, per block and 16-byte
// aligned each, the backward winners G and their SADs, the forward SADs (used when the caller keeps none), the vectors of the
// choose step and that step's state bytes.
constexpr uint32_t kBmRunPixels = 64; // frame-A pixels per search workgroup along x: 64 / bs neighbouring blocks share one LDS window
constexpr uint32_t kBmMaxRadius = 24;
struct BmShape {
    uint32_t blocks_x = 0, blocks_y = 0, runs_x = 0, rough_groups = 0;
    size_t rough_offset = 0, workspace_bytes = 0;
    size_t g_offset = 0, sad_g_offset = 0, sad_f_offset = 0, chosen_offset = 0, state_offset = 0; // bidir only
};
constexpr uint32_t kBmMaxTolerance = 96; // 2 components of two vectors of magnitude <= 24 each: a larger one changes nothing
BmShape bm_shape(uint32_t w, uint32_t h, uint32_t bs, uint32_t n_pairs, bool bidir = false); // host only
size_t bm_lds_bytes(uint32_t bs, uint32_t R);                            // dynamic LDS of one search workgroup
struct BmLaunch {
    const uint8_t *a = nullptr, *b = nullptr;
    size_t a_stride = 0, b_stride = 0;
    uint32_t w = 0, h = 0, n_pairs = 1;
    uint32_t bs = 16, R = 16;                       // bs in {8, 16, 32}, R in 1 .. kBmMaxRadius
    const uint16_t *rank = nullptr, *cand = nullptr; // (2R + 1)^2 entries each: candidate -> place in the tie order, and back
    void *workspace = nullptr;
    bool refine = true;        // confidence pass; off: vectors are the raw winners, flags 0
    bool bidir = false;        // forward-backward check in place of the confidence pass (refine is then not looked at)
    uint32_t tolerance = 2;    // of the check, 0 .. kBmMaxTolerance
    int16_t *vectors = nullptr;
    uint32_t *sad = nullptr;   // may be null
    uint8_t *flags = nullptr;  // may be null
    void *flow = nullptr;      // may be null; w * h cells per pair, 2 x f32 or 2 x f16
    bool flow_half = false;
    hipStream_t stream = nullptr;
};
hipError_t launch_blockmatch(const BmLaunch &L);

// The forward-backward check behind the two searches (nus_k_bm_bidir.hip; launch_blockmatch calls it with bidir set).  All fields
// in launch_blockmatch's per-block layout over n_pairs pairs; chosen (2 x int16) and state (u8) are the workspace's.
struct BmBidirLaunch {
    const int16_t *fwd = nullptr, *bwd = nullptr;    // raw winners A -> B and B -> A
    const uint32_t *sad_f = nullptr, *sad_b = nullptr;
    uint32_t w = 0, h = 0, n_pairs = 1, bs_log2 = 4, blocks_x = 0, blocks_y = 0;
    uint32_t tolerance = 2;
    int16_t *chosen = nullptr;
    uint8_t *state = nullptr;
    int16_t *vectors = nullptr;
    uint8_t *flags = nullptr; // may be null
    hipStream_t stream = nullptr;
};
hipError_t launch_bm_bidir(const BmBidirLaunch &L);

// Warp + blend straight from the block vectors (nus_k_bm_warp.hip; nus_bm_warp_device): the frames launch_warp_blend writes from
// the flow launch_blockmatch expands those vectors to, byte for byte (the same tile body reading another vector source), without
// that flow.  RGBA8 frames; vectors in launch_blockmatch's layout at
// block size bs; frame k of pair i at out + i * out_pair_stride + k * w * h * 4.
struct BmWarpLaunch {
    const uint8_t *a = nullptr, *b = nullptr;
    size_t a_stride = 0, b_stride = 0; // bytes between consecutive pairs
    uint32_t w = 0, h = 0, n_pairs = 1;
    uint32_t bs = 16;               // 8, 16 or 32
    const int16_t *vectors = nullptr;
    const float *times = nullptr;   // 1 .. kInterpMaxTimes
    uint32_t n_times = 0;
    bool fma = false;               // as WarpLaunch::fma
    uint8_t *out = nullptr;
    size_t out_pair_stride = 0;     // 0: the pair's frames tightly packed
    hipStream_t stream = nullptr;
};
hipError_t launch_bm_warp(const BmWarpLaunch &L);

// Scene-cut detection and the cut-aware output rule (nus_k_scene.hip; nus_scene_* in include/nuscaler_hip.h).  Pair i reads A at
// a + i * a_stride and B at b + i * b_stride (4-byte aligned).  The workspace holds the measure kernel's per-workgroup partials:
// u64 SADs at sad_offset, 64 u32 bins (32 of A, 32 of B) at hist_offset.
constexpr uint32_t kSceneBlock = 256; // lanes per workgroup of every scene kernel
struct SceneShape {
    uint32_t measure_blocks = 0, apply_blocks = 0; // workgroups per pair
    size_t sad_offset = 0, hist_offset = 0, workspace_bytes = 0;
};
SceneShape scene_shape(uint32_t w, uint32_t h, uint32_t n_pairs); // host only
struct SceneLaunch {
    const uint8_t *a = nullptr, *b = nullptr;
    size_t a_stride = 0, b_stride = 0;
    uint32_t w = 0, h = 0, n_pairs = 1;
    int format = 0; // nus_pixel_format of both frames
    hipStream_t stream = nullptr;
};
// measures (may be null): per pair {u64 sad, u32 hist_l1, u32 0}; cut: one u8 0 / 1 per pair
hipError_t launch_scene_detect(const SceneLaunch &L, uint32_t mad_threshold, uint32_t hist_permille, void *workspace, void *measures,
                               uint8_t *cut);
// for every pair with cut[i] != 0: frame k of the pair at out + i * out_pair_stride + k * w * h * 4 becomes a copy of A (bit k of
// from_a set) or of B, through the input selector of L.format; other pairs are neither read nor written
hipError_t launch_scene_apply(const SceneLaunch &L, uint32_t n_times, uint32_t from_a, const uint8_t *cut, uint8_t *out,
                              size_t out_pair_stride);

// Frame-rate conversion by the reduced ratio num / den (nus_k_retime.hip; the schedule is retime_pair of nus_retime.hpp).  Output j
// of the whole stream goes to out + j * out_frame_stride.  A launch covers the pairs [first_pair, first_pair + n_pairs) of the
// stream -- `frames` is frame first_pair, the pair's B one frame_stride further; `flow` / `vectors` / `cut` are entry first_pair's --
// so that the estimators' chunks and the grid-z chunks all index one global schedule while `out` stays the stream's.
struct RetimeLaunch {
    const uint8_t *frames = nullptr;
    size_t frame_stride = 0;
    uint32_t first_pair = 0, n_pairs = 0;
    uint32_t w = 0, h = 0;
    uint32_t num = 1, den = 1;
    uint8_t *out = nullptr;
    size_t out_frame_stride = 0; // bytes, at least w * h * 4
    uint32_t in_sel = kSelRGBA;
    hipStream_t stream = nullptr;
};
// The in-between outputs (r_j != 0) of the launch's pairs: each pair's vectors fetched once, every one of its outputs warped,
// blended and stored -- warp_blend_tile with the schedule as its time source, fed from the vector source given:
//   vectors != nullptr  block vectors at block size bs (launch_bm_warp's layout; RGBA frames, no selector);
//   flow != nullptr     dense flow, 2 x f32 or 2 x f16 per pixel, with `project` rounds of the projection (launch_warp_blend's);
//   flow and flow_bwd   the select warp (launch_warp_blend_select's): flow_bwd is the flow B -> A of every pair on B's grid, in
//                       flow's format and layout, with `project` rounds on both.  flow_bwd with vectors, or without flow: refused;
//   neither             zero flow: the streaming blend.
// Real-frame outputs are NOT written here: launch_retime_real.
struct RetimeWarp {
    const void *flow = nullptr;
    bool flow_half = false, fma = false;
    uint32_t project = 0;
    const int16_t *vectors = nullptr;
    uint32_t bs = 16;
    const void *flow_bwd = nullptr;
};
hipError_t launch_retime_warp(const RetimeLaunch &L, const RetimeWarp &V);
// The real-frame outputs (r_j == 0) among the n_frames frames that start at the launch's first one (L.frames is frame
// L.first_pair; L.n_pairs is not looked at): frame k with (k num) % den == 0 is copied through the input selector to output
// k num / den; the other frames are not read.  A copy kernel of its own.
hipError_t launch_retime_real(const RetimeLaunch &L, uint32_t n_frames);
// The two launches every retime entry point ends with: the in-between outputs of the launch's pairs from V's vectors, then the
// real-frame outputs among those pairs' first frames -- and, with the stream's last chunk, the stream's last frame.
inline hipError_t enqueue_retime(const RetimeLaunch &L, const RetimeWarp &V, bool last_chunk)
{
    const hipError_t e = launch_retime_warp(L, V);
    return e != hipSuccess ? e : launch_retime_real(L, L.n_pairs + (last_chunk ? 1 : 0));
}
// For every pair of the launch with cut[i] != 0 (i local): each of its in-between outputs becomes the copy (through the selector)
// of the pair's A if t_j < 0.5, else of its B.  Pairs that are not cut are neither read nor written.
hipError_t launch_scene_apply_retime(const RetimeLaunch &L, const uint8_t *cut);
// entries: n_out x {u32 pair, u32 rem, f32 t, u32 0}, one thread per FRAME k: the entries of pair k's outputs through retime_pair; the
// last frame has no pair behind it and writes its own entry alone
hipError_t launch_retime_table(uint32_t n_frames, uint32_t num, uint32_t den, void *entries, hipStream_t stream);

// 8-bit planar YUV 4:2:0 (I420) <-> RGBA8 (nus_k_yuv.hip; nus_yuv420_* in include/nuscaler_hip.h, where the integer contract is
// written).  Frame i of the batch: its Y, U and V planes, rows tight, from yuv + i * yuv_frame_stride; its pixels from
// rgba + i * rgba_frame_stride (4-byte aligned, the stride a multiple of 4).  Both strides in bytes and at least one frame (never 0
// here); the gaps are not written.  The side a launch reads is only read.  to_yuv / to_rgb / y_offset: the Q14 tables of the
// format's matrix and range (yuv_coefficients of nus_yuv.hpp); `sel`: input_selector of the RGBA side's nus_pixel_format, applied
// to the pixels loaded (to YUV) or stored (to RGBA; alpha 255).  chroma_filter is to-RGBA's alone.
struct YuvLaunch {
    uint8_t *yuv = nullptr, *rgba = nullptr;
    size_t yuv_frame_stride = 0, rgba_frame_stride = 0;
    uint32_t w = 0, h = 0, n_frames = 1;
    int siting = 0, chroma_filter = 0; // NUS_YUV_SITING_*, NUS_YUV_CHROMA_* (matrix and range are in the tables)
    int32_t to_yuv[9] = {0}, to_rgb[5] = {0}, y_offset = 0;
    uint32_t sel = kSelRGBA;
    hipStream_t stream = nullptr;
};
// The form is chosen per launch: the aligned kernels (8 pixels x 2 rows per thread towards RGBA, 16 x 2 towards YUV) where the
// width fills the run and every base and stride keeps its 16-byte accesses aligned, else one pixel / one chroma cell per thread.
hipError_t launch_yuv_to_rgba(const YuvLaunch &L);
hipError_t launch_rgba_to_yuv(const YuvLaunch &L);

// The same conversions on NV12 frames (nus_k_nv12.hip; "NV12 frames" in include/nuscaler_hip.h): `c.yuv` is the NV12 base and
// c.yuv_frame_stride its frame stride.  Frame i: Y rows y_pitch apart from the base, the rows of U,V byte pairs uv_pitch apart from
// base + uv_offset (tight: w, 2 cw and w h; pitched: the layout's pitch twice and its uv_offset) -- all three as resolved by the
// host, never 0.  Row padding, the gap between the planes and the gaps between frames are not written.  Every byte is the I420
// launch's byte.
struct Nv12Launch {
    YuvLaunch c;
    size_t y_pitch = 0, uv_pitch = 0, uv_offset = 0;
};
// The form is chosen per launch: the aligned kernels (8 x 2 pixels per thread and one 8-byte load of four pairs per chroma row
// towards RGBA; 16 x 2 and one 16-byte store of eight pairs towards NV12) where the width fills the run and the base, both
// pitches, uv_offset and the stride are multiples of 8 / 16 (the RGBA side as in YuvLaunch), else one pixel / one cell per thread.
hipError_t launch_nv12_to_rgba(const Nv12Launch &L);
hipError_t launch_rgba_to_nv12(const Nv12Launch &L);
// I420 <-> NV12: bytes only.  `i420` frames are tight planes, i420_frame_stride apart; the NV12 side as in Nv12Launch.  A thread
// moves 16 luma bytes, or 8 U + 8 V bytes as one 16-byte access on the pair side, where the width is a multiple of 16 and every
// base, pitch, offset and stride is; else one byte / one cell per thread.
struct Nv12RepackLaunch {
    uint8_t *i420 = nullptr, *nv12 = nullptr; // the side a launch reads is only read
    size_t i420_frame_stride = 0, nv12_frame_stride = 0;
    size_t y_pitch = 0, uv_pitch = 0, uv_offset = 0;
    uint32_t w = 0, h = 0, n_frames = 1;
    hipStream_t stream = nullptr;
};
hipError_t launch_i420_to_nv12(const Nv12RepackLaunch &L);
hipError_t launch_nv12_to_i420(const Nv12RepackLaunch &L);

// Separable resampling of the 8-bit planes of I420 frame batches (nus_k_yuv_resize.hip; nus_yuv_resizer of include/nuscaler_hip.h,
// where the contract is written).  One launch resamples one CLASS of planes: the luma plane of every frame (planes_per_frame 1)
// or both chroma planes (2), which share their tables.  Plane p of frame i starts at base + i * frame_stride + plane_offset +
// p * plane_step on either side; rows tight, iw x ih bytes in, ow x oh out.  Tables as build_resize_axis lays them out, in device
// memory, table_stride floats per output; max_taps the widest window of the four axes' two that this class uses.
struct PlaneTables {
    const int32_t *lx = nullptr, *ly = nullptr;
    const uint32_t *nx = nullptr, *ny = nullptr;
    const float *wx = nullptr, *wy = nullptr;
};
struct PlaneResizeLaunch {
    const uint8_t *in = nullptr;
    uint8_t *out = nullptr;
    size_t in_frame_stride = 0, out_frame_stride = 0; // bytes, never 0 here
    size_t in_plane_offset = 0, in_plane_step = 0, out_plane_offset = 0, out_plane_step = 0;
    uint32_t planes_per_frame = 1, n_frames = 1;
    uint32_t iw = 0, ih = 0, ow = 0, oh = 0;
    PlaneTables t;
    uint32_t table_stride = 0, max_taps = 0;
    // the row kernel's geometry, from the host's copy of the x tables (YuvResizer::initialize): widest LDS row of a wave's segment
    // and widest union of a lane's windows; union_taps 0 = the geometry does not fit the row kernel
    uint32_t ncols_max = 0, union_taps = 0;
    bool exact = false;
    hipStream_t stream = nullptr;
};
constexpr uint32_t kPlaneRun = 4;                 // adjacent output bytes a lane of the row kernel owns: one dword
constexpr uint32_t kPlaneSegment = 64 * kPlaneRun; // output columns of one wave
constexpr uint32_t kPlaneMaxUnion = 12;
// The row kernel (a lane owns kPlaneRun adjacent outputs, dword accesses) where both widths are multiples of 4, every plane of
// the class starts on a dword on either side, no window has more than 8 taps and the geometry fits; else one output per thread.
bool plane_rows_form(const PlaneResizeLaunch &L);
hipError_t launch_plane_resize(const PlaneResizeLaunch &L);
// The chroma class of tight NV12 frames (nus_k_nv12_resize.hip): ONE plane of U,V byte pairs per frame (planes_per_frame 1, the
// plane steps unused), iw x ih cells in and ow x oh out, rows of 2 iw / 2 ow bytes; both channels take the same tables.  The same
// operations in the same order as launch_plane_resize on the two de-interleaved planes, so the same bytes.  ncols_max / union_taps
// here: the widest dword-aligned input footprint of a wave's segment (128 output pairs) in BYTES, and the widest union of the
// windows of a lane's run of two pairs in cells (YuvResizer::initialize).
constexpr uint32_t kPairRun = 2;                 // adjacent output pairs a lane of the row kernel owns: one dword
constexpr uint32_t kPairSegment = 64 * kPairRun; // output pairs of one wave
constexpr uint32_t kPairMaxUnion = 8;            // a run of two needs at most taps + 1 columns, and no up-scale has more than 7 taps
// The row kernel where both row lengths are multiples of 4 bytes, the pair plane starts on a dword on either side, no window has
// more than 8 taps and the geometry fits; else one output byte per thread.
bool pair_rows_form(const PlaneResizeLaunch &L);
hipError_t launch_pair_resize(const PlaneResizeLaunch &L);
// n_frames frames of frame_bytes each, the strides apart: a copy kernel (dwords where everything is dword aligned, else bytes)
hipError_t launch_frame_copy(const uint8_t *in, size_t in_frame_stride, uint8_t *out, size_t out_frame_stride, size_t frame_bytes,
                             uint32_t n_frames, hipStream_t stream);

} // namespace nus
