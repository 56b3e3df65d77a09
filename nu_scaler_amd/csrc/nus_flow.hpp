// nus_flow.hpp -- optical-flow front end of the frame interpolator ("next" row, SURVEY.md
// section 8f rank 1): mirrors WgpuFrameInterpolator::build_pyramid / compute_coarse_flow
// (nu_scaler_core/src/wgpu_interpolator.rs:969-1203) on HIP, plus the coarse-to-fine
// warm start the reference sketches but never wires (its refine path is dead code).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <functional>
#include <initializer_list>
#include <mutex>
#include <string>
#include <utility>

#include "nus_host_util.hpp"

namespace nus {

// What every estimate takes: pyramid levels (1..12), Jacobi steps on the coarsest level and on each finer one, the smoothness weight.
// warps (0..kFlowMaxWarps; the handle's setting, set_warps): rounds per finer level, each re-linearising the data term about the
// level's current flow -- frame B sampled through it -- before its refine_iters steps.  0: linearised about zero flow, the
// upsampled flow only the Jacobi start value.
// median (0, 3 or 5; the handle's setting, set_median): after every Jacobi run of a level -- the coarsest level's steps, a finer
// level's, each round's of a warped level -- the level's flow is replaced by its component-wise median x median median (window
// centred, border replicated) before the next stage reads it.  A run of zero steps is followed by none.  0: no such stage.
constexpr uint32_t kFlowMaxWarps = 4;  // NUS_FLOW_MAX_WARPS
constexpr uint32_t kFlowMedianMax = 5; // NUS_FLOW_MEDIAN_MAX
struct FlowParams {
    uint32_t levels = 0, coarse_iters = 0, refine_iters = 0;
    float lambda = 0.0f;
    uint32_t warps = 0;
    uint32_t median = 0;
};

class HipFlowEstimator : public HostErrors {
public:
    HipFlowEstimator() = default;
    ~HipFlowEstimator();
    HipFlowEstimator(const HipFlowEstimator &) = delete;
    HipFlowEstimator &operator=(const HipFlowEstimator &) = delete;

    int set_device(int device);
    // 0: one plain kernel per Jacobi step and per pyramid pass (the shader's structure).  1 (default): the fused pyramid kernel,
    // derivatives once per level and K Jacobi steps per launch, LDS tiles or the streamed (register-pipelined) kernel by the size
    // of the level's batch.  2: as 1, always LDS tiles.  3: as 1, always streamed.  Bit-identical results.
    int set_tiled(int mode);

    // Primitives on host buffers (parity tests, integration).  f32 RGBA images, float2 flows.
    int rgba8_to_f32(const uint8_t *in, uint32_t w, uint32_t h, float *out);
    int blur(const float *in, uint32_t w, uint32_t h, float *out);        // H pass then V pass
    int downsample(const float *in, uint32_t w, uint32_t h, float *out);  // -> ((w+1)/2, (h+1)/2)
    int horn_schunck(const float *i1, const float *i2, const float *flow_in_or_null, uint32_t w, uint32_t h,
                     float lambda, uint32_t iterations, float *flow_out);
    int upsample(const float *src, uint32_t sw, uint32_t sh, float *dst, uint32_t dw, uint32_t dh, float scale);
    // The stage set_median adds behind every Jacobi run, on its own: the component-wise size x size median (3 or 5) of a flow.
    int median(const float *flow_in, uint32_t w, uint32_t h, uint32_t size, float *flow_out);
    // The projection set_project puts in front of the warp, on its own: g of every cell after `rounds` rounds at time t (launch_flow_project).
    int project(const float *flow_in, uint32_t w, uint32_t h, float t, uint32_t rounds, float *flow_out);
    // The two halves of a re-linearised level (set_warps).  warp_coefficients: (Ix, Iy, It') per cell, w*h*3 floats, with frame B's
    // luminance sampled through `flow` (null: zero flow, i.e. It = L2 - L1).  horn_schunck_coef: Jacobi steps on such coefficients.
    int warp_coefficients(const float *i1, const float *i2, const float *flow_or_null, uint32_t w, uint32_t h, float *coef_out);
    int horn_schunck_coef(const float *coef, const float *flow_in_or_null, uint32_t w, uint32_t h, float lambda, uint32_t iterations,
                          float *flow_out);

    // Full estimator: RGBA8 frames -> dense flow (w*h*2 floats, pixel delta A -> B).
    int estimate(const uint8_t *a, const uint8_t *b, uint32_t w, uint32_t h, const FlowParams &p, float *flow_out);
    // 0 EXACT (default): every stage bit-identical to the oracle's restatement of the shaders; 1 FAST: the Jacobi steps of the
    // estimators (estimate, estimate_device, estimate_device_stream) in separable sums / reciprocals / FMAs -- flow within 1e-3 px.
    // The primitives (blur, downsample, horn_schunck, upsample) are always exact.
    int set_mode(int mode);
    int mode() const { return fast_ ? 1 : 0; }
    // Re-linearisation rounds per finer level of every estimator entry point (FlowParams::warps), 0 (default) .. kFlowMaxWarps.  A
    // warped level's Jacobi steps run on coefficient planes in the exact kernels, in FAST mode too (inside FAST's contract).
    int set_warps(uint32_t warps);
    int warps() const { return (int)warps_; }
    // Median filter of the level's flow behind every Jacobi run of every estimator entry point (FlowParams::median): 0 (default,
    // off), 3 or 5.  A selection, so EXACT and FAST run the same kernel; the Jacobi launch that would have written the caller's
    // buffer (or Rg16Float halves) writes the workspace instead, and the median writes the caller's f32 buffer.
    int set_median(uint32_t size);
    int median_size() const { return (int)median_; }
    // Projection rounds of the warp behind the estimator (WarpLaunch::project; interpolate_device_stream and
    // interpolate_multi_device_stream), 0 (default) .. kFlowMaxProject.  The estimate and the flows handed out are untouched.
    int set_project(uint32_t rounds);
    int project_rounds() const { return (int)project_; }
    // Both flows of every pair and the select warp behind them (WarpSelectLaunch; nus_flow_set_bidirectional): off by default.  On,
    // interpolate_device_stream and interpolate_multi_device_stream also estimate every pair B -> A -- the same schedule on the same
    // pyramids, the two luminance planes swapped -- and warp with launch_warp_blend_select.  The forward flows are the bytes they
    // were (d_flows receives them alone); the backward ones stay in the workspace, in slots of their own which turning the setting
    // off frees (so that off means the old workspace as well as the old kernels and bytes).  retime_device_stream refuses the setting;
    // estimate_both_device_stream and retime_select_device_stream, which do the same work on request, do not look at it.
    int set_bidirectional(int enabled);
    int bidirectional() const { return bidir_ ? 1 : 0; }
    // Bytes of device workspace the handle holds (the sum of its grow-only slots): what "reserves the workspace it did" is checked with.
    size_t workspace_bytes();
    // TEST HOOK (nus_flow_fill_workspace; refused unless the process has NUS_TEST_HOOKS=1, read per call): every byte of every slot,
    // over its whole capacity, set to `byte_value` (0..255) on `stream`, which is synchronised before the call returns.  A handle
    // that has reserved nothing: kOk, no HIP call.
    int fill_workspace(int byte_value, hipStream_t stream);
    // Scene-cut detection in front of interpolate_multi_device_stream and the cut-aware output rule behind it (nus_scene_* of the C
    // header): off by default.  On, the in-between frames of a pair the detector flags are repeats of the nearer real frame.
    int set_scene_detect(int enabled, uint32_t mad_threshold, uint32_t hist_permille);
    int estimate_device(const void *d_a, const void *d_b, uint32_t w, uint32_t h, const FlowParams &p, void *d_flow_out,
                        hipStream_t stream);
    // n_frames consecutive RGBA8 frames -> n_frames - 1 flows (k -> k+1), each pyramid built once.
    int estimate_device_stream(const void *d_frames, uint32_t n_frames, uint32_t w, uint32_t h, const FlowParams &p, void *d_flows,
                               hipStream_t stream);
    // The reference's intended interpolate() as ONE pipeline (wgpu_interpolator.rs:881-935: pyramid -> coarse flow -> warp): the
    // flows of estimate_device_stream AND the n_frames - 1 in-between frames at time t warped + blended with them (dense-flow warp
    // in FMA mode) into d_mid: the warp kernel runs behind the estimator on the flow where it is (the caller's buffer, or the
    // workspace when d_flows == nullptr).  (The warp inside the finest level's last Jacobi launch, on the flow it has just finished,
    // was built, measured and removed -- same bytes, slower; the code is in git at d74dcbc.)
    // flow_half: the flows between estimator and warp -- and at d_flows, if given -- as 2 x IEEE half per pixel (Rg16Float, the
    // reference's live flow layout: wgpu_interpolator.rs:276), each the f32 flow rounded to nearest even; the warp reads them as such.
    int interpolate_device_stream(const void *d_frames, uint32_t n_frames, uint32_t w, uint32_t h, const FlowParams &p, float t,
                                  void *d_flows, void *d_mid, hipStream_t stream, bool flow_half = false);
    // As interpolate_device_stream, the frames at n_times times per pair from ONE estimate of each pair's flow: one multi-time
    // warp launch (FMA mode) behind the estimator, never the fused one.  Frame j of pair k at d_mid + k * mid_pair_stride +
    // j * w * h * 4 (0: tightly packed).  The arguments are checked before any HIP call; the flows at d_flows are the same bytes.
    int interpolate_multi_device_stream(const void *d_frames, uint32_t n_frames, uint32_t w, uint32_t h, const FlowParams &p,
                                        const float *times, uint32_t n_times, bool flow_half, void *d_flows, void *d_mid,
                                        size_t mid_pair_stride, hipStream_t stream);
    // Frame-rate conversion of the stream by num / den (nus_flow_retime_device_stream; the schedule is nus_retime.hpp's): the
    // estimator, then the retime warp in FMA mode over each chunk's pairs and the copy of the real frames -- the bytes of
    // estimate_device_stream followed by HipFrameInterpolator::retime_device in FMA mode.  Output j at d_out + j * out_frame_stride
    // (0: tightly packed).  Honours warps, median, project and scene detection; the flows at d_flows are the estimate's.
    int retime_device_stream(const void *d_frames, uint32_t n_frames, uint32_t w, uint32_t h, const FlowParams &p, uint32_t num,
                             uint32_t den, bool flow_half, void *d_flows, void *d_out, size_t out_frame_stride, hipStream_t stream);
    // Both flows of every pair of the stream (nus_flow_estimate_both_device_stream), f32: d_flows_fwd receives the bytes of
    // estimate_device_stream, d_flows_bwd pair k's flow frame k+1 -> frame k on frame k+1's grid -- the backward solve of
    // set_bidirectional (the same pyramids, the two planes swapped, the handle's warps and median), written to the caller's buffer
    // instead of kBwdFlows.  Does not look at the bidirectional setting.
    int estimate_both_device_stream(const void *d_frames, uint32_t n_frames, uint32_t w, uint32_t h, const FlowParams &p, void *d_flows_fwd,
                                    void *d_flows_bwd, hipStream_t stream);
    // retime_device_stream with both flows and the select warp (nus_flow_retime_select_device_stream): the bytes of
    // estimate_both_device_stream followed by HipFrameInterpolator::retime_select_device in FMA mode.  Either flow pointer may be
    // null: that direction then stays in the workspace.  Does not look at the bidirectional setting; at most 28 bytes per pixel and
    // pair of a chunk more workspace than retime_device_stream.
    int retime_select_device_stream(const void *d_frames, uint32_t n_frames, uint32_t w, uint32_t h, const FlowParams &p, uint32_t num,
                                    uint32_t den, bool flow_half, void *d_flows_fwd, void *d_flows_bwd, void *d_out, size_t out_frame_stride,
                                    hipStream_t stream);

private:
    // The grow-only device workspace.  Slots 0, 1, 4 and 5 have two names: the pair path's (plan / build_pyramid / solve, and the
    // primitives), then -- after the bar -- the batch path's (solve_batch).  solve_levels names none of them: its caller says where
    // the levels, the coefficients and the flows are (Schedule).
    enum Slot : int {
        kImage = 0, kLevelInOdd = 0,  // w*h*16: a primitive's input, a pyramid level's input | inputs of the odd levels of all frames
        kTemp = 1, kLevelInEven = 1,  // w*h*16: a primitive's output, blur temp, then the level's coefficients | ... of the even levels
        kFlowA = 2, kFlowB = 3,       // flow ping-pong: w*h*8 | [pair][level cells]
        kPyrA = 4, kLum = 4,          // frame A's pyramid, levels packed (horn_schunck: coefficients) | luminance planes [level][frame][cells]
        kPyrB = 5, kCoef = 5,         // frame B's pyramid | coefficients [pair][cells][3]
        kHostA = 6, kHostB = 7,       // estimate(): the host's RGBA8 frames; kHostB then takes the flow on its way back
        kFastPair = 8,                // estimate_device in FAST mode: the pair as a two-frame stream
        kPairFlow = 9,                // one pair's f32 flow that no caller's buffer takes
        kFlowsHalf = 10,              // a chunk's flows as Rg16Float, likewise
        kScene = 11,                  // the scene detector's workspace and cut flags
        kFwdFlows = 12,               // set_bidirectional: a chunk's forward flows that no caller's buffer takes (the backward solve reuses the ping-pong)
        kBwdFlows = 13,               // ... its backward flows as the warp reads them (pair path: the f32 flow, then its halves)
        kBwdCoef = 14,                // ... the backward solve's coefficients [pair][cells][3]
    };
    static constexpr int kSlotCount = 15;
    FlowParams with_warps(FlowParams p) const { return p.warps = warps_, p.median = median_, p; } // (mu_ held) what the entry points hand on: the handle's settings
    // the finer levels of such an estimate take `warps` rounds of launch_hs_warp_setup + Jacobi steps on coefficient planes
    static bool warped(const FlowParams &p) { return p.warps > 0 && p.refine_iters > 0; }
    struct MidTimes { // the multi-time warp behind the estimator (interpolate_multi_device_stream)
        const float *times = nullptr;
        uint32_t n = 0;
        size_t pair_stride = 0; // bytes between the in-between frames of consecutive pairs
    };
    struct RetimeJob { // the retime warp behind the estimator (retime_device_stream)
        uint32_t num = 1, den = 1; // reduced
        size_t out_frame_stride = 0;
        uint32_t n_pairs = 0;      // of the whole stream
    };
    struct StreamJob { // n_frames consecutive frames -> flows and / or in-between frames of the n_frames - 1 pairs
        const uint8_t *frames = nullptr;
        uint32_t n_frames = 0, w = 0, h = 0;
        uint8_t *flows = nullptr, *mid = nullptr; // either may be null, not both
        float t = 0.5f;                           // time of the in-between frame, unless
        bool flow_half = false;
        const MidTimes *mt = nullptr;             // ... several per pair
        const RetimeJob *rt = nullptr;            // ... or the outputs of a rate conversion: mid is then the STREAM's output base
        uint32_t first_pair = 0;                  // of this job in the stream (the rate conversion's schedule is global)
        uint32_t project = 0;                     // the warp's projection rounds (set_project)
        bool bidir = false;                       // with mid: the flows B -> A as well, and the select warp (set_bidirectional)
        uint8_t *flows_bwd = nullptr;             // the caller's buffer for the flows B -> A (the *_both_* / *_select_* entry points):
                                                  // with it the backward solve runs without mid too
        hipStream_t stream = nullptr;
        size_t frame_bytes() const { return (size_t)w * h * 4; }
        size_t flow_bytes() const { return (size_t)w * h * (flow_half ? 4 : 8); }
        size_t mid_stride() const { return mt ? mt->pair_stride : frame_bytes(); }
        StreamJob pairs(uint32_t k0, uint32_t n) const; // the job of pairs [k0, k0 + n)
        StreamJob(const void *d_frames, uint32_t n, uint32_t w_, uint32_t h_, void *d_flows, void *d_mid, hipStream_t s)
            : frames(static_cast<const uint8_t *>(d_frames)), n_frames(n), w(w_), h(h_), flows(static_cast<uint8_t *>(d_flows)),
              mid(static_cast<uint8_t *>(d_mid)), stream(s) {}
    };
    struct Pyramid { // level geometry; levels are packed at `offset` (16 bytes per pixel reserved)
        uint32_t levels = 0, w[12] = {0}, h[12] = {0};
        size_t offset[12] = {0}, total = 0;
    };
    // Where one run of the coarse-to-fine schedule (solve_levels) finds and leaves things: n pairs per launch, the pairs on the grid's
    // z / y axis.  A level's item stride (in cells; 0 for a single pair) is also that of its flows and, x 3, of its coefficients.
    struct Schedule {
        uint32_t n = 1;
        const Pyramid *g = nullptr;
        FlowParams p;
        hipStream_t stream = nullptr;
        struct {
            const float *i1, *i2; // the level of each pair's two frames
            size_t stride;
            int kernel;           // JacobiKernel of the level's steps, unless it is warped: then warped_kernel
        } level[12] = {};
        int warped_kernel = 0;
        bool luminance_planes = true; // false: the levels are f32 RGBA
        bool per_step = false;        // set_tiled(0): one launch_horn_schunck per step; the coefficient kernels only for warped rounds
        bool stream_planes = false;   // a level that streams takes its derivatives from the planes, not from coefficient planes
                                      // (setting it for a single pair is a performance experiment for a later change: it changes launches)
        float *coef = nullptr;
        float *flow_a = nullptr, *flow_b = nullptr; // ping-pong
        float *out = nullptr;                       // the caller's buffer (item stride: level 0's), or null
        bool half = false;                          // the final flow is wanted as Rg16Float
        // a warped level: every one but the coarsest; it runs the exact kernels on coefficient planes, FAST or not (k_hs_stream_fast
        // takes It from the luminance planes itself; the exact result is inside FAST's contract)
        bool warped_level(uint32_t l) const { return warped(p) && l + 1 < g->levels; }
        int kernel(uint32_t l) const { return warped_level(l) ? warped_kernel : level[l].kernel; }
        bool from_planes(uint32_t l) const; // level l needs no coefficient planes
    };
    struct Solved { // where level 0's flow ended up (the caller's buffer or the workspace), and whether the last launch stored halves
        float *flow = nullptr;
        bool wrote_half = false;
    };
    struct Staged { // a slot a primitive needs, and the host buffer (if any) that fills it
        Slot slot;
        size_t bytes;
        const void *host;
    };
    // What the host primitives share: lock, checks (dimensions, then `pointers_ok`), device, `stage` reserved and uploaded, `work`
    // (the launches; it names the device buffer that holds the result), `out_bytes` of it downloaded, synchronised.
    int primitive(std::initializer_list<std::pair<uint32_t, uint32_t>> dims, bool pointers_ok, std::initializer_list<Staged> stage,
                  void *out, size_t out_bytes, const std::function<int(const void *&result)> &work);
    // (all below: mu_ held)
    int plan(uint32_t w, uint32_t h, uint32_t levels, Pyramid &g); // geometry + workspace
    int build_pyramid(const void *frame, Slot pyr, const Pyramid &g, hipStream_t stream);
    int solve(Slot pyr_a, Slot pyr_b, const Pyramid &g, const FlowParams &p, void *d_flow_out, hipStream_t stream);
    int solve_levels(const Schedule &D, Solved &done);   // the schedule itself, for solve and solve_batch
    // behind it: the flow where and as J wants it -- in `out` if there is one, else where it is or (halves) in `half_slot` -> placed
    int place_flow(const StreamJob &J, const Solved &s, void *out, Slot half_slot, const void *&placed);
    int estimate_pair(const void *d_a, const void *d_b, uint32_t w, uint32_t h, const FlowParams &p, void *d_flow_out,
                      hipStream_t stream);
    // multi-step kernels, a chunk of consecutive pairs per launch (pairs on the grid's y / z axis): as many as fit the
    // workspace budget (64 MB per 1080p pair, 88 MB with coefficient planes), at most 150 (round 6; 100 and 6 GiB before: with
    // more pairs per launch the levels are cut into fewer row blocks, i.e. fewer halo rows are recomputed -- the motion step with
    // chunks of 150 units 19.5 - 19.7 against 20.0 - 20.4 ms per 300 units, profiles/r06_flow_chunk_size.txt; 12 GiB of the
    // GPU's 288);  64 -> 100 pairs per chunk had been 76 -> 71 us per pair (profiles/r02_flow_jacobi_streamed_ab.txt)
    static constexpr uint32_t kStreamMaxChunkPairs = 150;
    static constexpr size_t kStreamWorkspaceBytes = (size_t)12 << 30;
    int stream_impl(const StreamJob &J, const FlowParams &p);
    // what retime_device_stream and retime_select_device_stream share: the checks, the job, the cut rule behind it
    int retime_stream_call(const char *who, bool select, const void *d_frames, uint32_t n_frames, uint32_t w, uint32_t h, const FlowParams &p,
                           uint32_t num, uint32_t den, bool flow_half, void *d_flows, void *d_flows_bwd, void *d_out, size_t out_frame_stride,
                           hipStream_t stream);
    int solve_batch(const StreamJob &J, const Pyramid &g, const FlowParams &p); // J: one chunk
    static WarpLaunch warp_behind(const StreamJob &J, const void *flow); // the warp kernel behind the estimator, over J's pairs
    // ... launched; J.rt: the retime warp and the real frames; J.bidir: the select warp with the flows B -> A at flow_bwd (with J.rt:
    // the retime select warp)
    static hipError_t launch_warp_behind(const StreamJob &J, const void *flow, const void *flow_bwd = nullptr);
    int ensure_device();
    static constexpr uint64_t kMaxPixels = (1ull << 28) - 1;
    int check_size(uint32_t w, uint32_t h) { return pass(check_dims("flow", w, h, kMaxPixels, "bad image dimensions")); }
    int reserve(size_t bytes, Slot slot);
    float *f32(Slot slot) const { return static_cast<float *>(slot_[slot].get()); }
    uint8_t *u8(Slot slot) const { return static_cast<uint8_t *>(slot_[slot].get()); }
    void release();

    std::mutex mu_;
    int device_ = 0;
    bool ready_ = false;
    bool tiled_ = true;
    int jacobi_ = 0; // JacobiKernel
    uint32_t warps_ = 0; // set_warps
    uint32_t median_ = 0; // set_median
    uint32_t project_ = 0; // set_project
    bool bidir_ = false; // set_bidirectional
    bool fast_ = false; // set_mode(1): the estimator's Jacobi steps in FAST arithmetic (k_hs_stream_fast), every level streamed
    hipStream_t stream_ = nullptr;
    hipStream_t call_stream_ = nullptr; // (mu_ held) the stream of the entry point in progress: reserve() waits for it before it frees
    bool scene_ = false; // set_scene_detect
    uint32_t scene_mad_ = 20, scene_hist_ = 400;
    DeviceBuffer slot_[kSlotCount];
};

} // namespace nus
