// nus_flow.cpp -- see nus_flow.hpp.
#include "nus_flow.hpp"

#include <cstdlib>
#include <cstring>

#include "nus_host.hpp"
#include "nus_host_util.hpp"
#include "nus_retime.hpp"
#include "nus_kernels.hpp"
#include "nus_scene.hpp"
#include "nus_transfer.hpp"

namespace nus {

HipFlowEstimator::~HipFlowEstimator() { release(); }

int HipFlowEstimator::set_tiled(int mode)
{
    std::lock_guard<std::mutex> lk(mu_);
    if (mode < 0 || mode > 3) return fail(kInvalidArgument, "set_tiled: 0 plain, 1 multi-step (kernel chosen by size), 2 LDS tiles, 3 streamed");
    tiled_ = mode != 0;
    jacobi_ = mode == 2 ? kJacobiTiles : (mode == 3 ? kJacobiStream : kJacobiAuto);
    return kOk;
}

int HipFlowEstimator::set_mode(int mode)
{
    std::lock_guard<std::mutex> lk(mu_);
    if (mode != 0 && mode != 1) return fail(kInvalidArgument, "set_mode: 0 exact, 1 fast");
    fast_ = mode == 1;
    return kOk;
}

int HipFlowEstimator::set_warps(uint32_t warps)
{
    std::lock_guard<std::mutex> lk(mu_);
    if (warps > kFlowMaxWarps) return fail(kInvalidArgument, fmt("nus_flow_set_warps: 0..%u rounds, got %u", kFlowMaxWarps, warps));
    warps_ = warps;
    return kOk;
}

int HipFlowEstimator::set_median(uint32_t size)
{
    std::lock_guard<std::mutex> lk(mu_);
    if (size != 0 && size != 3 && size != 5) return fail(kInvalidArgument, fmt("nus_flow_set_median: 0 (off), 3 or 5, got %u", size));
    median_ = size;
    return kOk;
}

int HipFlowEstimator::set_project(uint32_t rounds)
{
    std::lock_guard<std::mutex> lk(mu_);
    if (rounds > kFlowMaxProject)
        return fail(kInvalidArgument, fmt("nus_flow_set_project: 0 .. %u projection rounds, got %u", kFlowMaxProject, rounds));
    project_ = rounds;
    return kOk;
}

int HipFlowEstimator::set_bidirectional(int enabled)
{
    std::lock_guard<std::mutex> lk(mu_);
    if (enabled != 0 && enabled != 1) return fail(kInvalidArgument, fmt("nus_flow_set_bidirectional: 0 or 1, got %d", enabled));
    if (bidir_ && enabled == 0 && ready_ && (slot_[kFwdFlows].get() || slot_[kBwdFlows].get() || slot_[kBwdCoef].get())) {
        // off is the old workspace too: the setting's own slots go, behind whatever the device still runs in them
        NUS_HIP(hipSetDevice(device_));
        NUS_HIP(hipDeviceSynchronize());
        for (Slot s : {kFwdFlows, kBwdFlows, kBwdCoef}) slot_[s].release();
    }
    bidir_ = enabled == 1;
    return kOk;
}

size_t HipFlowEstimator::workspace_bytes()
{
    std::lock_guard<std::mutex> lk(mu_);
    size_t total = 0;
    for (const DeviceBuffer &s : slot_) total += s.capacity();
    return total;
}

// TEST HOOK: what the workspace held before a call must not show in the call's results (tests/test_gpu_flow_workspace.py).  The
// slots are reachable from nowhere else, so the poison has to come from inside.
int HipFlowEstimator::fill_workspace(int byte_value, hipStream_t stream)
{
    std::lock_guard<std::mutex> lk(mu_);
    // refused unless the PROCESS asked for test hooks (as nus_upscaler_set_option's "inject_retire_error")
    const char *hooks = getenv("NUS_TEST_HOOKS");
    if (!hooks || strcmp(hooks, "1") != 0) return fail(kInvalidArgument, "nus_flow_fill_workspace: a test hook (NUS_TEST_HOOKS=1 only)");
    if (byte_value < 0 || byte_value > 255) return fail(kInvalidArgument, fmt("nus_flow_fill_workspace: a byte value 0..255, got %d", byte_value));
    if (!ready_) return kOk; // nothing reserved yet: no HIP call
    bool any = false;
    for (const DeviceBuffer &s : slot_) any = any || s.capacity() != 0;
    if (!any) return kOk;
    NUS_HIP(hipSetDevice(device_));
    for (const DeviceBuffer &s : slot_)
        if (s.capacity() != 0) NUS_HIP(hipMemsetAsync(s.get(), byte_value, s.capacity(), stream));
    // the host entry points run on the handle's own stream: they see the fill only once `stream` has finished
    NUS_HIP(hipStreamSynchronize(stream));
    return kOk;
}

int HipFlowEstimator::set_device(int device)
{
    std::lock_guard<std::mutex> lk(mu_);
    if (device < 0) return fail(kInvalidArgument, "negative device index");
    if (ready_) return fail(kInvalidArgument, "set_device must precede the first call");
    device_ = device;
    return kOk;
}

int HipFlowEstimator::ensure_device()
{
    const int n = device_count();
    if (n <= 0) return fail(kNoDevice, "no HIP device available (the gfx950 path has no CPU fallback)");
    if (device_ >= n) return fail(kNoDevice, "requested HIP device not present");
    NUS_HIP(hipSetDevice(device_));
    if (!ready_) {
        NUS_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
        ready_ = true;
    }
    return kOk;
}

// Growing a slot frees the old memory: behind everything the handle has queued on its own stream AND on the stream of the call in
// progress (the stream rule of the header: one stream's calls need no synchronisation between them, so the call before may still
// be running in the slot).  hipFree's own implicit device synchronisation is documented; this does not lean on it.
int HipFlowEstimator::reserve(size_t bytes, Slot slot)
{
    DeviceBuffer &s = slot_[slot];
    if (bytes > s.capacity() && s.get() && call_stream_ != stream_) NUS_HIP(hipStreamSynchronize(call_stream_));
    return pass(s.reserve(bytes, stream_));
}

void HipFlowEstimator::release()
{
    if (!ready_) return;
    (void)hipSetDevice(device_);
    (void)hipStreamSynchronize(stream_);
    for (DeviceBuffer &s : slot_) s.release();
    (void)hipStreamDestroy(stream_);
    ready_ = false;
}

// (The host entry points move their images through the library's own pinned ring, nus_transfer.hpp: upload / download.  A caller's
// pageable buffer is never handed to the runtime's copy.)
int HipFlowEstimator::primitive(std::initializer_list<std::pair<uint32_t, uint32_t>> dims, bool pointers_ok,
                                std::initializer_list<Staged> stage, void *out, size_t out_bytes,
                                const std::function<int(const void *&result)> &work)
{
    std::lock_guard<std::mutex> lk(mu_);
    int rc;
    for (const auto &d : dims)
        if ((rc = check_size(d.first, d.second)) != kOk) return rc;
    if (!pointers_ok) return fail(kInvalidArgument, "flow: null pointer");
    if ((rc = ensure_device()) != kOk) return rc;
    call_stream_ = stream_;
    for (const Staged &s : stage)
        if ((rc = reserve(s.bytes, s.slot)) != kOk) return rc;
    for (const Staged &s : stage)
        if (s.host && (rc = pass(upload(slot_[s.slot].get(), s.host, s.bytes, stream_))) != kOk) return rc;
    const void *result = nullptr;
    if ((rc = work(result)) != kOk || (rc = pass(download(out, result, out_bytes, stream_))) != kOk) return rc;
    NUS_HIP(hipStreamSynchronize(stream_));
    return kOk;
}

int HipFlowEstimator::rgba8_to_f32(const uint8_t *in, uint32_t w, uint32_t h, float *out)
{
    const size_t npx = (size_t)w * h;
    return primitive({{w, h}}, in && out, {{kImage, npx * 4, in}, {kTemp, npx * 16, nullptr}}, out, npx * 16, [&](const void *&result) -> int {
        NUS_HIP(launch_rgba8_to_f32(u8(kImage), f32(kTemp), w, h, stream_));
        result = f32(kTemp);
        return kOk;
    });
}

int HipFlowEstimator::blur(const float *in, uint32_t w, uint32_t h, float *out)
{
    const size_t bytes = (size_t)w * h * 16;
    return primitive({{w, h}}, in && out, {{kImage, bytes, in}, {kTemp, bytes, nullptr}}, out, bytes, [&](const void *&result) -> int {
        NUS_HIP(launch_blur(f32(kImage), f32(kTemp), w, h, true, stream_));
        NUS_HIP(launch_blur(f32(kTemp), f32(kImage), w, h, false, stream_));
        result = f32(kImage);
        return kOk;
    });
}

int HipFlowEstimator::downsample(const float *in, uint32_t w, uint32_t h, float *out)
{
    const size_t bytes = (size_t)w * h * 16, obytes = (size_t)((w + 1) / 2) * ((h + 1) / 2) * 16;
    return primitive({{w, h}}, in && out, {{kImage, bytes, in}, {kTemp, obytes, nullptr}}, out, obytes, [&](const void *&result) -> int {
        NUS_HIP(launch_downsample(f32(kImage), f32(kTemp), w, h, stream_));
        result = f32(kTemp);
        return kOk;
    });
}

int HipFlowEstimator::horn_schunck(const float *i1, const float *i2, const float *flow_in, uint32_t w, uint32_t h,
                                   float lambda, uint32_t iterations, float *flow_out)
{
    const size_t ib = (size_t)w * h * 16, fb = (size_t)w * h * 8;
    return primitive({{w, h}}, i1 && i2 && flow_out, {{kImage, ib, i1}, {kTemp, ib, i2}, {kFlowA, fb, flow_in}, {kFlowB, fb, nullptr}},
                     flow_out, fb, [&](const void *&result) -> int {
        if (!flow_in) NUS_HIP(hipMemsetAsync(f32(kFlowA), 0, fb, stream_)); // compute_coarse_flow clears the flow (:1136-1154)
        float *f0 = f32(kFlowA), *f1 = f32(kFlowB);
        if (tiled_) {
            const int rc = reserve(ib, kPyrA); // 3 floats of coefficients per cell
            if (rc != kOk) return rc;
            HsPrepareLaunch P;
            P.img = {w, h, 1, stream_};
            P.i1 = f32(kImage), P.i2 = f32(kTemp), P.coef = f32(kPyrA);
            NUS_HIP(launch_hs_prepare(P));
            HsIterateLaunch I;
            I.img = P.img;
            I.coef = P.coef, I.lambda = lambda, I.iterations = iterations, I.flow_a = f0, I.flow_b = f1, I.kernel = jacobi_;
            HsIterateResult R;
            NUS_HIP(launch_hs_iterate(I, &R));
            f0 = R.flow;
        } else {
            for (uint32_t i = 0; i < iterations; ++i, std::swap(f0, f1)) // ping-pong as :1156-1193
                NUS_HIP(launch_horn_schunck(f32(kImage), f32(kTemp), f0, f1, w, h, lambda, stream_));
        }
        result = f0;
        return kOk;
    });
}

int HipFlowEstimator::warp_coefficients(const float *i1, const float *i2, const float *flow, uint32_t w, uint32_t h, float *coef_out)
{
    const size_t ib = (size_t)w * h * 16, fb = (size_t)w * h * 8, cb = (size_t)w * h * 12;
    return primitive({{w, h}}, i1 && i2 && coef_out, {{kImage, ib, i1}, {kTemp, ib, i2}, {kFlowA, fb, flow}, {kPyrA, cb, nullptr}}, coef_out, cb,
                     [&](const void *&result) -> int {
        HsPrepareLaunch P;
        P.img = {w, h, 1, stream_};
        P.i1 = f32(kImage), P.i2 = f32(kTemp), P.coef = f32(kPyrA);
        NUS_HIP(launch_hs_warp_setup(P, HsCoarseFlow{}, flow ? f32(kFlowA) : nullptr, 0, nullptr, 0));
        result = f32(kPyrA);
        return kOk;
    });
}

int HipFlowEstimator::horn_schunck_coef(const float *coef, const float *flow_in, uint32_t w, uint32_t h, float lambda, uint32_t iterations,
                                        float *flow_out)
{
    const size_t fb = (size_t)w * h * 8, cb = (size_t)w * h * 12;
    return primitive({{w, h}}, coef && flow_out, {{kPyrA, cb, coef}, {kFlowA, fb, flow_in}, {kFlowB, fb, nullptr}}, flow_out, fb,
                     [&](const void *&result) -> int {
        if (!flow_in) NUS_HIP(hipMemsetAsync(f32(kFlowA), 0, fb, stream_));
        HsIterateLaunch I;
        I.img = {w, h, 1, stream_};
        I.coef = f32(kPyrA), I.lambda = lambda, I.iterations = iterations, I.flow_a = f32(kFlowA), I.flow_b = f32(kFlowB), I.kernel = jacobi_;
        HsIterateResult R;
        R.flow = I.flow_a; // (no step: the start value)
        NUS_HIP(launch_hs_iterate(I, &R));
        result = R.flow;
        return kOk;
    });
}

int HipFlowEstimator::upsample(const float *src, uint32_t sw, uint32_t sh, float *dst, uint32_t dw, uint32_t dh, float scale)
{
    const size_t sb = (size_t)sw * sh * 8, db = (size_t)dw * dh * 8;
    return primitive({{sw, sh}, {dw, dh}}, src && dst, {{kFlowA, sb, src}, {kFlowB, db, nullptr}}, dst, db, [&](const void *&result) -> int {
        NUS_HIP(launch_flow_upsample({dw, dh, 1, stream_}, HsCoarseFlow{f32(kFlowA), sw, sh, scale, 0}, f32(kFlowB), 0));
        result = f32(kFlowB);
        return kOk;
    });
}

int HipFlowEstimator::median(const float *flow_in, uint32_t w, uint32_t h, uint32_t size, float *flow_out)
{
    if (size != 3 && size != 5) {
        std::lock_guard<std::mutex> lk(mu_);
        return fail(kInvalidArgument, fmt("nus_flow_median: size 3 or 5, got %u", size));
    }
    const size_t fb = (size_t)w * h * 8;
    return primitive({{w, h}}, flow_in && flow_out, {{kFlowA, fb, flow_in}, {kFlowB, fb, nullptr}}, flow_out, fb, [&](const void *&result) -> int {
        FlowMedianLaunch M;
        M.img = {w, h, 1, stream_};
        M.size = size, M.in = f32(kFlowA), M.out = f32(kFlowB);
        NUS_HIP(launch_flow_median(M));
        result = f32(kFlowB);
        return kOk;
    });
}

int HipFlowEstimator::project(const float *flow_in, uint32_t w, uint32_t h, float t, uint32_t rounds, float *flow_out)
{
    if (rounds > kFlowMaxProject || t != t) {
        std::lock_guard<std::mutex> lk(mu_);
        if (t != t) return fail(kInvalidArgument, "nus_flow_project: t is NaN");
        return fail(kInvalidArgument, fmt("nus_flow_project: 0 .. %u projection rounds, got %u", kFlowMaxProject, rounds));
    }
    if (!flow_in || !flow_out) {
        std::lock_guard<std::mutex> lk(mu_);
        return fail(kInvalidArgument, "nus_flow_project: null pointer");
    }
    const size_t fb = (size_t)w * h * 8;
    return primitive({{w, h}}, true, {{kFlowA, fb, flow_in}, {kFlowB, fb, nullptr}}, flow_out, fb, [&](const void *&result) -> int {
        FlowProjectLaunch P;
        P.img = {w, h, 1, stream_};
        P.t = t, P.rounds = rounds, P.in = f32(kFlowA), P.out = f32(kFlowB);
        NUS_HIP(launch_flow_project(P));
        result = f32(kFlowB);
        return kOk;
    });
}

int HipFlowEstimator::plan(uint32_t w, uint32_t h, uint32_t levels, Pyramid &g)
{
    if (levels == 0 || levels > 12) return fail(kInvalidArgument, "flow: levels must be 1..12");
    int rc = ensure_device();
    if (rc != kOk) return rc;
    // level geometry (build_pyramid: next = (cur + 1) / 2, wgpu_interpolator.rs:1008-1009)
    g.total = 0;
    g.levels = 0;
    for (uint32_t l = 0, cw = w, ch = h; l < levels; ++l) {
        g.w[l] = cw;
        g.h[l] = ch;
        g.offset[l] = g.total;
        g.total += (size_t)cw * ch * 16;
        g.levels = l + 1;
        if (cw == 1 && ch == 1) break;
        cw = (cw + 1) / 2;
        ch = (ch + 1) / 2;
    }
    const size_t ib = (size_t)w * h * 16, fb = (size_t)w * h * 8;
    if ((rc = reserve(ib, kImage)) != kOk || (rc = reserve(ib, kTemp)) != kOk || (rc = reserve(fb, kFlowA)) != kOk ||
        (rc = reserve(fb, kFlowB)) != kOk || (rc = reserve(g.total, kPyrA)) != kOk || (rc = reserve(g.total, kPyrB)) != kOk)
        return rc;
    return kOk;
}

// Pyramid of one RGBA8 frame into slot `pyr` (kPyrA or kPyrB).
int HipFlowEstimator::build_pyramid(const void *frame, Slot pyr, const Pyramid &g, hipStream_t stream)
{
    float *cur = f32(kImage), *tmp = f32(kTemp);
    if (tiled_) {
        // fused level kernel: writes the level's luminance plane (at the level's offset; the
        // f32 RGBA level itself is not needed) and the downsampled input of level l+1, which
        // ping-pongs between cur and tmp
        float *nxt[2] = {cur, tmp};
        PyramidLevelLaunch P;
        P.in = frame;
        for (uint32_t l = 0; l < g.levels; ++l) {
            P.img = {g.w[l], g.h[l], 1, stream};
            P.u8_input = l == 0;
            P.level_lum = reinterpret_cast<float *>(u8(pyr) + g.offset[l]);
            P.next = l + 1 < g.levels ? nxt[l & 1] : nullptr;
            NUS_HIP(launch_pyramid_level(P, jacobi_));
            P.in = P.next;
        }
        return kOk;
    }
    NUS_HIP(launch_rgba8_to_f32(static_cast<const uint8_t *>(frame), cur, g.w[0], g.h[0], stream));
    for (uint32_t l = 0; l < g.levels; ++l) {
        float *level = reinterpret_cast<float *>(u8(pyr) + g.offset[l]);
        NUS_HIP(launch_blur(cur, tmp, g.w[l], g.h[l], true, stream));
        NUS_HIP(launch_blur(tmp, level, g.w[l], g.h[l], false, stream));
        if (l + 1 < g.levels) NUS_HIP(launch_downsample(level, cur, g.w[l], g.h[l], stream));
    }
    return kOk;
}

// A level whose Jacobi steps run in the streamed kernel needs no coefficient planes: that kernel takes the derivatives from the
// luminance planes of the pair's two frames as it goes.
bool HipFlowEstimator::Schedule::from_planes(uint32_t l) const
{
    return stream_planes && !warped_level(l) && hs_iterate_streams(g->w[l], g->h[l], n, kernel(l));
}

// The coarse-to-fine Horn-Schunck schedule of D.n pairs, every stage one launch over all of them: the coarsest level from zero flow
// (compute_coarse_flow, :1136-1154), each finer one from the flow of the level below, upsampled.
int HipFlowEstimator::solve_levels(const Schedule &D, Solved &done)
{
    int rc;
    const Pyramid &g = *D.g;
    const FlowParams &p = D.p;
    const hipStream_t stream = D.stream;
    const uint32_t L = g.levels - 1;
    float *f0 = D.flow_a, *f1 = D.flow_b;
    auto images = [&](uint32_t l) { return FlowImages{g.w[l], g.h[l], D.n, stream}; };
    // the derivatives of level l from the level of each pair's two frames
    auto prepare = [&](uint32_t l) {
        HsPrepareLaunch P;
        P.img = images(l);
        P.i1 = D.level[l].i1, P.i2 = D.level[l].i2, P.luminance_planes = D.luminance_planes, P.img_stride = D.level[l].stride;
        P.coef = D.coef, P.coef_stride = D.level[l].stride * 3;
        return P;
    };
    // the flow of level l + 1, in f0, as level l takes it up
    auto coarse_of = [&](uint32_t l) { return HsCoarseFlow{f0, g.w[l + 1], g.h[l + 1], 2.0f, D.level[l + 1].stride}; };
    // Who may write the caller's buffer: the launch that finishes level 0.  Without the median that is a Jacobi launch -- for
    // Rg16Float only the FAST streamed kernel's, which stores halves itself (every other kernel writes 2 x f32 per cell and must be
    // kept in the workspace, its flow converted afterwards).  With the median no Jacobi launch finishes level 0: each writes the
    // workspace, f32, and the median behind the last one writes the caller's f32 buffer if there is one.
    const bool fast_last = D.kernel(0) == kJacobiStreamFast && (L > 0 ? p.refine_iters > 0 : p.coarse_iters > 0);
    float *const jacobi_out = p.median || (D.half && !fast_last) ? nullptr : D.out;
    float *const median_out = D.half ? nullptr : D.out;
    // One Jacobi run of level l on the flow in f0 (no steps: nothing), and the median behind it.  `last`: no further round of the
    // level follows; `zero`: from zero flow, f0 is not read; `coarse`: f0 is the flow of level l + 1, which the first launch upsamples
    // as it loads it.
    auto run = [&](uint32_t l, uint32_t iters, bool last, bool zero = false, bool coarse = false) -> int {
        if (iters == 0) return kOk;
        if (D.per_step && !D.warped_level(l)) {
            for (uint32_t i = 0; i < iters; ++i, std::swap(f0, f1))
                NUS_HIP(launch_horn_schunck(D.level[l].i1, D.level[l].i2, f0, f1, g.w[l], g.h[l], p.lambda, stream));
        } else {
            HsIterateLaunch I;
            I.img = images(l);
            I.coef = D.coef, I.coef_stride = D.level[l].stride * 3;
            I.lum1 = D.from_planes(l) ? D.level[l].i1 : nullptr, I.lum_stride = D.level[l].stride;
            I.lambda = p.lambda, I.iterations = iters, I.zero_start = zero;
            I.flow_a = f0, I.flow_b = f1, I.flow_stride = D.level[l].stride;
            I.final_out = l == 0 && last ? jacobi_out : nullptr, I.final_stride = D.level[0].stride;
            I.kernel = D.kernel(l);
            if (coarse) I.coarse = coarse_of(l);
            I.final_half = l == 0 && D.half && !p.median;
            HsIterateResult R;
            NUS_HIP(launch_hs_iterate(I, &R));
            f0 = R.flow, f1 = R.spare;
            if (l == 0) done.wrote_half = R.wrote_half;
        }
        if (p.median) { // from the buffer the run left into the other one, the two names swapped
            FlowMedianLaunch M;
            M.img = images(l);
            M.size = p.median, M.in = f0, M.in_stride = M.out_stride = D.level[l].stride;
            M.out = l == 0 && last && median_out ? median_out : f1;
            NUS_HIP(launch_flow_median(M));
            if (M.out == f1) f1 = f0;
            f0 = M.out;
        }
        return kOk;
    };
    // coarsest level: the multi-step kernels take zero flow as a null input
    const bool zero = !D.per_step && p.coarse_iters > 0;
    if (!zero) NUS_HIP(hipMemsetAsync(f0, 0, (size_t)g.w[L] * g.h[L] * D.n * 8, stream));
    if (zero && !D.from_planes(L)) NUS_HIP(launch_hs_prepare(prepare(L)));
    if ((rc = run(L, p.coarse_iters, true, zero)) != kOk) return rc;
    for (uint32_t l = L; l-- > 0;) {
        if (D.warped_level(l)) { // each round: the level's coefficients about the flow it has (round 1: the upsampled one), then the steps
            for (uint32_t r = 0; r < p.warps; ++r) {
                if (r == 0) {
                    NUS_HIP(launch_hs_warp_setup(prepare(l), coarse_of(l), nullptr, 0, f1, D.level[l].stride));
                    std::swap(f0, f1);
                } else {
                    NUS_HIP(launch_hs_warp_setup(prepare(l), HsCoarseFlow{}, f0, D.level[l].stride, nullptr, 0));
                }
                if ((rc = run(l, p.refine_iters, r + 1 == p.warps)) != kOk) return rc;
            }
        } else if (p.refine_iters > 0 && D.from_planes(l)) { // derivatives and upsampled flow both computed inside the Jacobi kernel
            if ((rc = run(l, p.refine_iters, true, false, true)) != kOk) return rc;
        } else {
            if (!D.per_step && p.refine_iters > 0) // the level's derivatives and the upsampled flow in one launch
                NUS_HIP(launch_hs_level_setup(prepare(l), coarse_of(l), f1, D.level[l].stride));
            else
                NUS_HIP(launch_flow_upsample(images(l), coarse_of(l), f1, D.level[l].stride));
            std::swap(f0, f1);
            if ((rc = run(l, p.refine_iters, true)) != kOk) return rc;
        }
    }
    done.flow = f0;
    return kOk;
}

// The flow solve_levels left, where and as J wants it -- f32 or Rg16Float, in `out` if there is one (the caller's buffer, or the
// slot that keeps a forward flow from the backward solve); else it stays where it is, its halves in `half_slot`.
int HipFlowEstimator::place_flow(const StreamJob &J, const Solved &s, void *out, Slot half_slot, const void *&placed)
{
    const size_t cells = (size_t)J.w * J.h * (J.n_frames - 1);
    const void *final_flow = s.flow;
    if (!J.flow_half || s.wrote_half) { // as wanted already (halves: the launch wrote them, into the caller's buffer if there is one)
        if (out && s.flow != out) NUS_HIP(hipMemcpyAsync(out, s.flow, cells * (J.flow_half ? 4 : 8), hipMemcpyDeviceToDevice, J.stream));
        if (out) final_flow = out;
    } else { // 2 x f32 per cell in the workspace: converted into the caller's buffer, or beside it
        void *dst = out;
        if (!dst) {
            const int rc = reserve(cells * 4, half_slot);
            if (rc != kOk) return rc;
            dst = u8(half_slot);
        }
        NUS_HIP(launch_flow_to_half(s.flow, dst, cells, J.stream));
        final_flow = dst;
    }
    placed = final_flow;
    return kOk;
}

// Coarse-to-fine Horn-Schunck between the pyramids in slots `pyr_a` and `pyr_b`: one pair, its f32 flow to d_flow_out.
int HipFlowEstimator::solve(Slot pyr_a, Slot pyr_b, const Pyramid &g, const FlowParams &p, void *d_flow_out, hipStream_t stream)
{
    Schedule D;
    D.g = &g, D.p = p, D.stream = stream;
    for (uint32_t l = 0; l < g.levels; ++l)
        D.level[l] = {reinterpret_cast<const float *>(u8(pyr_a) + g.offset[l]), reinterpret_cast<const float *>(u8(pyr_b) + g.offset[l]), 0, jacobi_};
    D.warped_kernel = jacobi_;
    D.luminance_planes = tiled_, D.per_step = !tiled_; // (the plain kernels' pyramids hold f32 RGBA levels)
    D.coef = f32(kTemp); // the blur temp, which is free once the pyramids exist (slot 5, the batch path's kCoef, is frame B's pyramid here)
    D.flow_a = f32(kFlowA), D.flow_b = f32(kFlowB), D.out = static_cast<float *>(d_flow_out);
    Solved done;
    const int rc = solve_levels(D, done);
    const void *placed;
    return rc != kOk ? rc : place_flow(StreamJob(nullptr, 2, g.w[0], g.h[0], d_flow_out, nullptr, stream), done, d_flow_out, kFlowsHalf, placed);
}

int HipFlowEstimator::estimate_device(const void *d_a, const void *d_b, uint32_t w, uint32_t h, const FlowParams &p, void *d_flow_out,
                                      hipStream_t stream)
{
    std::lock_guard<std::mutex> lk(mu_);
    call_stream_ = stream;
    return estimate_pair(d_a, d_b, w, h, with_warps(p), d_flow_out, stream);
}

int HipFlowEstimator::estimate_pair(const void *d_a, const void *d_b, uint32_t w, uint32_t h, const FlowParams &p, void *d_flow_out,
                                    hipStream_t stream)
{
    int rc = check_size(w, h);
    if (rc != kOk) return rc;
    if (!d_a || !d_b || !d_flow_out) return fail(kInvalidArgument, "flow: null device pointer");
    Pyramid g;
    if ((rc = plan(w, h, p.levels, g)) != kOk) return rc;
    // FAST arithmetic lives in the batch solver's register-pipelined kernels, which need a batch (or a frame) big enough to fill
    // the GPU; a single 1080p pair is 576 waves -- the LDS-tile kernels of the exact path are 2.7x faster there (220 against
    // 605 us when that was measured; the exact pair takes 245 us today), and their result satisfies FAST's contract trivially.
    // So a pair alone takes the FAST kernels only where the finest level would stream anyway, or where the streamed kernel is
    // forced (set_tiled(3)).
    if (fast_ && (jacobi_ == kJacobiStream || (jacobi_ == kJacobiAuto && hs_iterate_streams(g.w[0], g.h[0], 1, kJacobiAuto)))) {
        const size_t fb = (size_t)w * h * 4;
        if ((rc = reserve(2 * fb, kFastPair)) != kOk) return rc;
        NUS_HIP(hipMemcpyAsync(u8(kFastPair), d_a, fb, hipMemcpyDeviceToDevice, stream));
        NUS_HIP(hipMemcpyAsync(u8(kFastPair) + fb, d_b, fb, hipMemcpyDeviceToDevice, stream));
        return solve_batch(StreamJob(u8(kFastPair), 2, w, h, d_flow_out, nullptr, stream), g, p);
    }
    if ((rc = build_pyramid(d_a, kPyrA, g, stream)) != kOk || (rc = build_pyramid(d_b, kPyrB, g, stream)) != kOk) return rc;
    return solve(kPyrA, kPyrB, g, p, d_flow_out, stream);
}

// Flows between consecutive frames of a device-resident stream: frame k+1's pyramid, built for the
// pair (k, k+1), is frame A's pyramid of the pair (k+1, k+2), so each frame's pyramid is built once.
int HipFlowEstimator::estimate_device_stream(const void *d_frames, uint32_t n_frames, uint32_t w, uint32_t h, const FlowParams &p,
                                             void *d_flows, hipStream_t stream)
{
    std::lock_guard<std::mutex> lk(mu_);
    if (!d_flows) return fail(kInvalidArgument, "flow: null device pointer");
    call_stream_ = stream;
    return stream_impl(StreamJob(d_frames, n_frames, w, h, d_flows, nullptr, stream), with_warps(p));
}

int HipFlowEstimator::interpolate_device_stream(const void *d_frames, uint32_t n_frames, uint32_t w, uint32_t h, const FlowParams &p,
                                                float t, void *d_flows, void *d_mid, hipStream_t stream, bool flow_half)
{
    std::lock_guard<std::mutex> lk(mu_);
    if (!d_mid) return fail(kInvalidArgument, "flow: null device pointer");
    if (!(t >= 0.0f && t <= 1.0f)) return fail(kInvalidArgument, "flow: t must be in [0, 1]");
    if (misaligned(d_mid, 16) || misaligned(d_flows, 16))
        return fail(kInvalidArgument, "flow: device pointers must be 16-byte aligned");
    StreamJob J(d_frames, n_frames, w, h, d_flows, d_mid, stream);
    J.t = t, J.flow_half = flow_half, J.project = project_, J.bidir = bidir_;
    call_stream_ = stream;
    return stream_impl(J, with_warps(p));
}

int HipFlowEstimator::interpolate_multi_device_stream(const void *d_frames, uint32_t n_frames, uint32_t w, uint32_t h, const FlowParams &p,
                                                      const float *times, uint32_t n_times, bool flow_half, void *d_flows, void *d_mid,
                                                      size_t mid_pair_stride, hipStream_t stream)
{
    static const char *const who = "nus_flow_interpolate_multi_device_stream";
    std::lock_guard<std::mutex> lk(mu_);
    int rc = pass(check_dims(who, w, h, kMaxPixels, "bad image dimensions"));
    if (rc != kOk) return rc;
    if (!d_frames || !d_mid) return fail(kInvalidArgument, std::string(who) + ": null device pointer");
    if (n_frames < 2) return fail(kInvalidArgument, std::string(who) + ": a stream needs at least 2 frames");
    if ((rc = pass(check_interp_times(who, times, n_times))) != kOk) return rc;
    if (misaligned(d_mid, 16) || misaligned(d_flows, 16) || misaligned(d_frames, 4))
        return fail(kInvalidArgument, std::string(who) + ": d_mid and d_flows must be 16-byte aligned, d_frames 4-byte aligned");
    const size_t frame_bytes = (size_t)w * h * 4;
    if (mid_pair_stride != 0 && (mid_pair_stride < n_times * frame_bytes || mid_pair_stride % 4))
        return fail(kInvalidArgument, std::string(who) + ": mid_pair_stride must be 0 or a multiple of 4 of at least n_times * w * h * 4 bytes");
    const uint32_t n_pairs = n_frames - 1;
    if (scene_) {
        const std::string too_many = check_scene_launch(w, h, n_pairs);
        if (!too_many.empty()) return fail(kInvalidArgument, std::string(who) + ": " + too_many);
    }
    const MidTimes mt{times, n_times, mid_pair_stride ? mid_pair_stride : n_times * frame_bytes};
    StreamJob J(d_frames, n_frames, w, h, d_flows, d_mid, stream);
    J.t = times[0], J.flow_half = flow_half, J.mt = &mt, J.project = project_, J.bidir = bidir_;
    call_stream_ = stream;
    if ((rc = stream_impl(J, with_warps(p))) != kOk || !scene_) return rc;
    // behind estimate + warp, the detector (it reads the frames only, so its place in the order is free) and the flagged pairs'
    // frames overwritten with repeats
    const size_t ws_bytes = scene_shape(w, h, n_pairs).workspace_bytes;
    if ((rc = reserve(ws_bytes + n_pairs, kScene)) != kOk) return rc;
    uint8_t *cut = u8(kScene) + ws_bytes;
    SceneLaunch S;
    S.a = J.frames, S.b = S.a + frame_bytes, S.a_stride = S.b_stride = frame_bytes;
    S.w = w, S.h = h, S.n_pairs = n_pairs, S.stream = stream;
    NUS_HIP(launch_scene_detect(S, scene_mad_, scene_hist_, u8(kScene), nullptr, cut));
    NUS_HIP(launch_scene_apply(S, n_times, scene_from_a_mask(times, n_times), cut, J.mid, mt.pair_stride));
    return kOk;
}

int HipFlowEstimator::retime_device_stream(const void *d_frames, uint32_t n_frames, uint32_t w, uint32_t h, const FlowParams &p, uint32_t num,
                                           uint32_t den, bool flow_half, void *d_flows, void *d_out, size_t out_frame_stride,
                                           hipStream_t stream)
{
    static const char *const who = "nus_flow_retime_device_stream";
    std::lock_guard<std::mutex> lk(mu_);
    if (bidir_) return fail(kInvalidArgument, std::string(who) + ": bidirectional flow is not supported by rate conversion yet");
    return retime_stream_call(who, false, d_frames, n_frames, w, h, p, num, den, flow_half, d_flows, nullptr, d_out, out_frame_stride, stream);
}

int HipFlowEstimator::retime_select_device_stream(const void *d_frames, uint32_t n_frames, uint32_t w, uint32_t h, const FlowParams &p,
                                                  uint32_t num, uint32_t den, bool flow_half, void *d_flows_fwd, void *d_flows_bwd, void *d_out,
                                                  size_t out_frame_stride, hipStream_t stream)
{
    std::lock_guard<std::mutex> lk(mu_); // (the bidirectional setting is not looked at: this entry point is the request)
    return retime_stream_call("nus_flow_retime_select_device_stream", true, d_frames, n_frames, w, h, p, num, den, flow_half, d_flows_fwd,
                              d_flows_bwd, d_out, out_frame_stride, stream);
}

int HipFlowEstimator::estimate_both_device_stream(const void *d_frames, uint32_t n_frames, uint32_t w, uint32_t h, const FlowParams &p,
                                                  void *d_flows_fwd, void *d_flows_bwd, hipStream_t stream)
{
    std::lock_guard<std::mutex> lk(mu_);
    if (!d_flows_fwd || !d_flows_bwd) return fail(kInvalidArgument, "nus_flow_estimate_both_device_stream: null device pointer");
    StreamJob J(d_frames, n_frames, w, h, d_flows_fwd, nullptr, stream);
    J.flows_bwd = static_cast<uint8_t *>(d_flows_bwd);
    call_stream_ = stream;
    return stream_impl(J, with_warps(p));
}

// (mu_ held)
int HipFlowEstimator::retime_stream_call(const char *who, bool select, const void *d_frames, uint32_t n_frames, uint32_t w, uint32_t h,
                                         const FlowParams &p, uint32_t num, uint32_t den, bool flow_half, void *d_flows, void *d_flows_bwd,
                                         void *d_out, size_t out_frame_stride, hipStream_t stream)
{
    RetimeRatio r;
    int rc = pass(check_retime(who, n_frames, num, den, r));
    if (rc != kOk || (rc = pass(check_dims(who, w, h, kMaxPixels, "bad image dimensions"))) != kOk) return rc;
    if (!d_frames || !d_out) return fail(kInvalidArgument, std::string(who) + ": null device pointer");
    if (misaligned(d_out, 16) || misaligned(d_flows, 16) || misaligned(d_flows_bwd, 16) || misaligned(d_frames, 4))
        return fail(kInvalidArgument, std::string(who) + ": d_out and d_flows must be 16-byte aligned, d_frames 4-byte aligned");
    const size_t frame_bytes = (size_t)w * h * 4;
    if ((rc = pass(check_out_frame_stride(who, out_frame_stride, frame_bytes))) != kOk) return rc;
    const uint32_t n_pairs = n_frames - 1;
    if (scene_) {
        const std::string too_many = check_scene_launch(w, h, n_pairs);
        if (!too_many.empty()) return fail(kInvalidArgument, std::string(who) + ": " + too_many);
    }
    const RetimeJob rt{r.num, r.den, out_frame_stride ? out_frame_stride : frame_bytes, n_pairs};
    StreamJob J(d_frames, n_frames, w, h, d_flows, d_out, stream);
    J.flow_half = flow_half, J.rt = &rt, J.project = project_;
    J.bidir = select, J.flows_bwd = static_cast<uint8_t *>(d_flows_bwd);
    call_stream_ = stream;
    if ((rc = stream_impl(J, with_warps(p))) != kOk || !scene_) return rc;
    // behind estimate + warp, the detector and the cut pairs' in-between outputs overwritten with repeats
    const size_t ws_bytes = scene_shape(w, h, n_pairs).workspace_bytes;
    if ((rc = reserve(ws_bytes + n_pairs, kScene)) != kOk) return rc;
    uint8_t *cut = u8(kScene) + ws_bytes;
    SceneLaunch S;
    S.a = J.frames, S.b = S.a + frame_bytes, S.a_stride = S.b_stride = frame_bytes;
    S.w = w, S.h = h, S.n_pairs = n_pairs, S.stream = stream;
    NUS_HIP(launch_scene_detect(S, scene_mad_, scene_hist_, u8(kScene), nullptr, cut));
    RetimeLaunch L;
    L.frames = J.frames, L.frame_stride = frame_bytes, L.first_pair = 0, L.n_pairs = n_pairs, L.w = w, L.h = h;
    L.num = r.num, L.den = r.den, L.out = J.mid, L.out_frame_stride = rt.out_frame_stride, L.stream = stream;
    NUS_HIP(launch_scene_apply_retime(L, cut));
    return kOk;
}

int HipFlowEstimator::set_scene_detect(int enabled, uint32_t mad_threshold, uint32_t hist_permille)
{
    std::lock_guard<std::mutex> lk(mu_);
    if (enabled != 0 && enabled != 1) return fail(kInvalidArgument, fmt("nus_flow_set_scene_detect: 0 or 1, got %d", enabled));
    const std::string bad = check_scene_thresholds(mad_threshold, hist_permille);
    if (!bad.empty()) return fail(kInvalidArgument, "nus_flow_set_scene_detect: " + bad);
    scene_ = enabled == 1;
    scene_mad_ = mad_threshold;
    scene_hist_ = hist_permille;
    return kOk;
}

HipFlowEstimator::StreamJob HipFlowEstimator::StreamJob::pairs(uint32_t k0, uint32_t n) const
{
    StreamJob S = *this;
    S.frames += (size_t)k0 * frame_bytes();
    S.n_frames = n + 1;
    if (flows) S.flows += (size_t)k0 * flow_bytes();
    if (flows_bwd) S.flows_bwd += (size_t)k0 * flow_bytes();
    if (mid && !rt) S.mid += (size_t)k0 * mid_stride();
    S.first_pair += k0;
    return S;
}

hipError_t HipFlowEstimator::launch_warp_behind(const StreamJob &J, const void *flow, const void *flow_bwd)
{
    if (J.bidir && !J.rt) return launch_warp_blend_select(WarpSelectLaunch{warp_behind(J, flow), static_cast<const float *>(flow_bwd)});
    if (!J.rt) return launch_warp_blend(warp_behind(J, flow));
    RetimeLaunch L;
    L.frames = J.frames, L.frame_stride = J.frame_bytes();
    L.first_pair = J.first_pair, L.n_pairs = J.n_frames - 1, L.w = J.w, L.h = J.h, L.num = J.rt->num, L.den = J.rt->den;
    L.out = J.mid, L.out_frame_stride = J.rt->out_frame_stride, L.stream = J.stream;
    RetimeWarp V;
    V.flow = flow, V.flow_half = J.flow_half, V.fma = true, V.project = J.project;
    if (J.bidir) V.flow_bwd = flow_bwd; // the retime select warp
    return enqueue_retime(L, V, J.first_pair + L.n_pairs == J.rt->n_pairs);
}

WarpLaunch HipFlowEstimator::warp_behind(const StreamJob &J, const void *flow)
{
    WarpLaunch L;
    L.a = J.frames, L.b = L.a + J.frame_bytes(), L.a_stride = L.b_stride = J.frame_bytes();
    L.flow = static_cast<const float *>(flow), L.flow_half = J.flow_half, L.fma = true;
    L.out = J.mid;
    L.w = J.w, L.h = J.h, L.t = J.t, L.n_pairs = J.n_frames - 1, L.stream = J.stream;
    if (J.mt) L.times = J.mt->times, L.n_times = J.mt->n, L.out_pair_stride = J.mt->pair_stride;
    L.project = J.project;
    return L;
}

// (called with mu_ held)  J.flows may be null when J.mid is not: the caller wants the in-between frames only.
int HipFlowEstimator::stream_impl(const StreamJob &J, const FlowParams &p)
{
    const uint32_t w = J.w, h = J.h;
    int rc = check_size(w, h);
    if (rc != kOk) return rc;
    if (!J.frames || (!J.flows && !J.mid)) return fail(kInvalidArgument, "flow: null device pointer");
    if (J.n_frames < 2) return fail(kInvalidArgument, "flow: a stream needs at least 2 frames");
    Pyramid g;
    if ((rc = plan(w, h, p.levels, g)) != kOk) return rc;
    const uint32_t n_pairs = J.n_frames - 1;
    if (!tiled_ && !fast_) { // the shader-shaped kernels, pair by pair (each frame's pyramid still built once)
        if ((J.mid && !J.flows) || J.flow_half) { // (they write a pair's f32 flow where they are told to: one pair's worth of workspace)
            if ((rc = reserve((size_t)w * h * 8, kPairFlow)) != kOk) return rc;
        }
        if (J.flow_half && !J.flows && (rc = reserve(J.flow_bytes(), kFlowsHalf)) != kOk) return rc;
        const bool bidir = (J.bidir && J.mid) || J.flows_bwd;
        const size_t f32_bytes = (size_t)w * h * 8;
        // (a caller's buffer takes the backward flow as the warp reads it; its f32 form needs the slot only where that is halves)
        if (bidir && (!J.flows_bwd || J.flow_half) &&
            (rc = reserve(f32_bytes + (J.flow_half && !J.flows_bwd ? J.flow_bytes() : 0), kBwdFlows)) != kOk)
            return rc;
        if ((rc = build_pyramid(J.frames, kPyrA, g, J.stream)) != kOk) return rc;
        for (uint32_t k = 0; k < n_pairs; ++k) {
            const StreamJob P = J.pairs(k, 1);
            const Slot pyr_a = k & 1 ? kPyrB : kPyrA, pyr_b = k & 1 ? kPyrA : kPyrB;
            if ((rc = build_pyramid(P.frames + P.frame_bytes(), pyr_b, g, J.stream)) != kOk) return rc;
            void *fl = P.flows && !J.flow_half ? static_cast<void *>(P.flows) : u8(kPairFlow);
            if ((rc = solve(pyr_a, pyr_b, g, p, fl, J.stream)) != kOk) return rc;
            if (J.flow_half) {
                void *hf = P.flows ? static_cast<void *>(P.flows) : u8(kFlowsHalf);
                NUS_HIP(launch_flow_to_half(static_cast<const float *>(fl), hf, (size_t)w * h, J.stream));
                fl = hf;
            }
            const void *bwd = nullptr;
            if (bidir) { // the same pyramids the other way round (the forward flow is out of the ping-pong by now)
                void *bf = P.flows_bwd && !J.flow_half ? static_cast<void *>(P.flows_bwd) : u8(kBwdFlows);
                if ((rc = solve(pyr_b, pyr_a, g, p, bf, J.stream)) != kOk) return rc;
                bwd = bf;
                if (J.flow_half) {
                    void *hb = P.flows_bwd ? static_cast<void *>(P.flows_bwd) : u8(kBwdFlows) + f32_bytes;
                    NUS_HIP(launch_flow_to_half(static_cast<const float *>(bf), hb, (size_t)w * h, J.stream));
                    bwd = hb;
                }
            }
            if (J.mid) NUS_HIP(launch_warp_behind(P, fl, bwd));
        }
        return kOk;
    }
    // Tiled kernels: the pairs of a chunk go through every stage TOGETHER, one launch per stage with the pairs on the
    // grid's z axis -- a 480x270 level of one pair is 510 tiles (two per CU, latency bound); of 64 pairs it fills the GPU.
    // per pair: luminance planes 4/3 x 4 B, level inputs (1/4 + 1/16) x 16 B, two flows 16 B per pixel -- and 12 B of
    // coefficients if some level's Jacobi steps run on LDS tiles (the streamed kernel takes them from the planes)
    // (dev overrides, round 6 -- measured and left at the defaults: profiles/r06_flow_chunk_size.txt)
    const char *env_pairs = getenv("NUS_FLOW_MAX_CHUNK_PAIRS"), *env_gb = getenv("NUS_FLOW_WORKSPACE_GB");
    const uint32_t max_pairs = env_pairs && atoi(env_pairs) > 0 ? (uint32_t)atoi(env_pairs) : kStreamMaxChunkPairs;
    const size_t workspace = env_gb && atoi(env_gb) > 0 ? (size_t)atoi(env_gb) << 30 : kStreamWorkspaceBytes;
    auto chunk_for = [&](size_t bytes_per_pixel) {
        const uint32_t c = (uint32_t)(workspace / ((size_t)w * h * bytes_per_pixel));
        return c < 1 ? 1u : (c > max_pairs ? max_pairs : c);
    };
    // set_bidirectional: two more flow buffers, 16 B -- the forward flows kept from the backward solve and the backward flows -- and
    // the backward solve's own coefficients, 12 B
    const size_t bidir_bytes = (J.bidir && J.mid) || J.flows_bwd ? 28 : 0;
    uint32_t chunk = chunk_for(31 + bidir_bytes);
    if (chunk > n_pairs) chunk = n_pairs;
    for (uint32_t l = 0; l < g.levels; ++l) // (a warped level -- every one but the coarsest -- always takes coefficient planes)
        if ((warped(p) && l + 1 < g.levels) ||
            !hs_iterate_streams(g.w[l], g.h[l], chunk, fast_ && jacobi_ == kJacobiStream ? kJacobiStreamFast : jacobi_)) {
            chunk = chunk_for(43 + bidir_bytes);
            break;
        }
    for (uint32_t c0 = 0; c0 < n_pairs; c0 += chunk)
        if ((rc = solve_batch(J.pairs(c0, n_pairs - c0 < chunk ? n_pairs - c0 : chunk), g, p)) != kOk) return rc;
    return kOk;
}

// The pairs of J (one chunk) -> their flows, every stage one launch over the whole chunk.  With J.mid also the pairs' in-between
// frames (see interpolate_device_stream); J.flows may then be null.
int HipFlowEstimator::solve_batch(const StreamJob &J, const Pyramid &g, const FlowParams &p)
{
    int rc;
    const uint32_t pairs = J.n_frames - 1;
    const hipStream_t stream = J.stream;
    Schedule D;
    D.n = pairs, D.g = &g, D.p = p, D.stream = stream;
    D.warped_kernel = jacobi_, D.stream_planes = true, D.half = J.flow_half;
    // The Jacobi kernel of a level.  FAST: k_hs_stream_fast where the level's batch would stream anyway (or the streamed kernel
    // is forced), the exact LDS-tile kernel -- on the FAST pyramid's planes -- where it would not (a small batch's coarse levels).
    for (uint32_t l = 0; l < g.levels; ++l) {
        if (!fast_ || jacobi_ == kJacobiTiles) D.level[l].kernel = jacobi_;
        else if (jacobi_ == kJacobiStream) D.level[l].kernel = kJacobiStreamFast;
        else D.level[l].kernel = hs_iterate_streams(g.w[l], g.h[l], pairs, kJacobiAuto) ? kJacobiStreamFast : kJacobiTiles;
    }
    // The luminance-only pyramid streams rows per wave as well: where level 0 of the batch is too small for that, the exact
    // LDS-tile pyramid runs instead (its planes serve either Jacobi kernel).  (The same pyramid with warps as without.)
    const bool fast_pyramid = fast_ && (jacobi_ == kJacobiStream || D.level[0].kernel == kJacobiStreamFast);
    const int jacobi = fast_ ? (fast_pyramid ? kJacobiStream : kJacobiTiles) : jacobi_; // (for the exact pyramid launcher's choice)
    const uint32_t nf = pairs + 1, nl = g.levels;
    size_t cells[13] = {0}, lum_off[12], lum_total = 0; // (0 beyond the last level)
    for (uint32_t l = 0; l < nl; ++l) {
        cells[l] = (size_t)g.w[l] * g.h[l];
        lum_off[l] = lum_total;
        lum_total += cells[l] * nf;
    }
    // (the largest level input each of the two buffers holds is the first)
    if ((rc = reserve(cells[1] * nf * 16, kLevelInOdd)) != kOk || (rc = reserve(cells[2] * nf * 16, kLevelInEven)) != kOk ||
        (rc = reserve(cells[0] * pairs * 8, kFlowA)) != kOk || (rc = reserve(cells[0] * pairs * 8, kFlowB)) != kOk ||
        (rc = reserve(lum_total * 4, kLum)) != kOk)
        return rc;
    size_t coef_cells = 0;
    for (uint32_t l = 0; l < nl; ++l)
        if (!D.from_planes(l) && cells[l] > coef_cells) coef_cells = cells[l];
    if (coef_cells != 0 && (rc = reserve(coef_cells * pairs * 12, kCoef)) != kOk) return rc;
    float *level_in[2] = {f32(kLevelInOdd), f32(kLevelInEven)}; // input of level l: [(l - 1) & 1]
    float *lum = f32(kLum);
    // pyramids of all frames, level by level
    for (uint32_t l = 0; l < nl; ++l) {
        PyramidLevelLaunch P;
        P.img = {g.w[l], g.h[l], nf, stream};
        P.in = l == 0 ? static_cast<const void *>(J.frames) : level_in[(l - 1) & 1];
        P.u8_input = l == 0;
        P.in_stride = l == 0 ? cells[0] * 4 /* bytes */ : cells[l] /* float4 */;
        P.level_lum = lum + lum_off[l], P.lum_stride = cells[l];
        P.next = l + 1 < nl ? level_in[l & 1] : nullptr, P.next_stride = cells[l + 1];
        // luminance only: one float per pixel between the levels (the buffers are sized for four)
        NUS_HIP(fast_pyramid ? launch_pyramid_level_fast(P) : launch_pyramid_level(P, jacobi));
        // the planes of each pair's two frames are consecutive planes of the level
        D.level[l].i1 = P.level_lum, D.level[l].i2 = P.level_lum + cells[l], D.level[l].stride = cells[l];
    }
    const bool bidir = (J.bidir && J.mid) || J.flows_bwd;
    void *fwd_out = J.flows, *bwd_out = J.flows_bwd;
    if (bidir) { // the forward flows must outlive the backward solve, which runs in the same ping-pong
        if ((!fwd_out && (rc = reserve(cells[0] * pairs * (J.flow_half ? 4 : 8), kFwdFlows)) != kOk) ||
            (!bwd_out && (rc = reserve(cells[0] * pairs * (J.flow_half ? 4 : 8), kBwdFlows)) != kOk) ||
            (rc = reserve(cells[0] * pairs * 12, kBwdCoef)) != kOk)
            return rc;
        if (!fwd_out) fwd_out = u8(kFwdFlows);
        if (!bwd_out) bwd_out = u8(kBwdFlows);
    }
    D.coef = f32(kCoef), D.flow_a = f32(kFlowA), D.flow_b = f32(kFlowB), D.out = static_cast<float *>(fwd_out);
    Solved done;
    const void *flow = nullptr, *flow_bwd = nullptr;
    if ((rc = solve_levels(D, done)) != kOk || (rc = place_flow(J, done, fwd_out, kFlowsHalf, flow)) != kOk) return rc;
    if (bidir) {
        // B -> A: the same schedule on the same planes, each pair's two swapped.  The streamed kernels that take their derivatives
        // from the planes find the second frame's one plane BEHIND the first's, so this solve runs on coefficient planes, which
        // name both -- the exact kernels, in FAST mode too (as a warped level: inside FAST's contract).
        Schedule B = D;
        B.stream_planes = false;
        for (uint32_t l = 0; l < nl; ++l) std::swap(B.level[l].i1, B.level[l].i2), B.level[l].kernel = jacobi_;
        B.coef = f32(kBwdCoef), B.out = static_cast<float *>(bwd_out);
        Solved back;
        if ((rc = solve_levels(B, back)) != kOk || (rc = place_flow(J, back, bwd_out, kBwdFlows, flow_bwd)) != kOk) return rc;
    }
    if (J.mid) NUS_HIP(launch_warp_behind(J, flow, flow_bwd));
    return kOk;
}

// One lock across stage, estimate and download: no other thread's call can reuse the staging slots in between.
int HipFlowEstimator::estimate(const uint8_t *a, const uint8_t *b, uint32_t w, uint32_t h, const FlowParams &p, float *flow_out)
{
    std::lock_guard<std::mutex> lk(mu_);
    int rc = check_size(w, h);
    if (rc != kOk) return rc;
    if (!a || !b || !flow_out) return fail(kInvalidArgument, "flow: null pointer");
    if ((rc = ensure_device()) != kOk) return rc;
    call_stream_ = stream_;
    const size_t fbytes = (size_t)w * h * 4;
    if ((rc = reserve(fbytes, kHostA)) != kOk || (rc = reserve((size_t)w * h * 8, kHostB)) != kOk) return rc;
    if ((rc = pass(upload(u8(kHostA), a, fbytes, stream_))) != kOk || (rc = pass(upload(u8(kHostB), b, fbytes, stream_))) != kOk) return rc;
    // kHostB doubles as the flow output once frame B has been converted (the estimate copies
    // into it last, after every reader of frame B has been enqueued on the same stream)
    if ((rc = estimate_pair(u8(kHostA), u8(kHostB), w, h, with_warps(p), u8(kHostB), stream_)) != kOk ||
        (rc = pass(download(flow_out, u8(kHostB), (size_t)w * h * 8, stream_))) != kOk)
        return rc;
    NUS_HIP(hipStreamSynchronize(stream_));
    return kOk;
}

} // namespace nus
