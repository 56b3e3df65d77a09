// nus_cli.cpp -- `nu_scaler_cli`: the image-file commands of the north star's CLI as a native program on the
// C ABI (include/nuscaler_hip.h).  Shape: `upscale_image_file` of the legacy crate
// (Nu_scale/src/upscale/mod.rs:307-338) and the option names of its `fullscreen` subcommand
// (Nu_scale/src/main.rs:36-73: --tech, --quality, --algorithm).
//
//   nu_scaler_cli upscale <in.png> <out.png> [--algorithm A] [--scale S] [--tech T] [--quality Q] [--device N]
//   nu_scaler_cli interpolate <a.png> <b.png> <out.png> [--t X | --multiplier M] [--flow [--flow-warps N] [--flow-median 0|3|5] [--flow-project N] [--flow-bidirectional]] [--device N]
//                             [--method block_matching [--quality high|medium|low] [--bidirectional [--bidir-tolerance N]]]
//   nu_scaler_cli retime --from R --to R [--method M] [flow / block flags, --flow-bidirectional] [--scene-detect] OUT_%04d.png IN0.png IN1.png ...
//   nu_scaler_cli scene <a.png> <b.png> [--mad N] [--hist N] [--device N]   (the scene-cut detector: cut=0|1 mad=.. hist_permille=..)
//   nu_scaler_cli compare <a.png> <b.png> [--device N]   (MSE / PSNR / SSIM, ErrorMetrics: Nu_scale/src/upscale/common.rs:475-543)
//   nu_scaler_cli png-copy <in.png> <out.png>        (decode + encode only; no GPU: codec self-check)
//
// Pixels go through the HIP kernels only: without a device the commands fail.
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../../include/nuscaler_hip.h"
#include "nus_png.hpp"

namespace {

int fail(const std::string &msg)
{
    std::fprintf(stderr, "nu_scaler_cli: error: %s\n", msg.c_str());
    return 1;
}

int usage(int rc)
{
    std::fprintf(rc ? stderr : stdout,
                 "usage: nu_scaler_cli upscale <in.png> <out.png> [--algorithm nearest|bilinear|bicubic|lanczos3|triangle|fsr1|easu]\n"
                 "                             [--scale S] [--tech fsr|fallback|none] [--quality ultra|quality|balanced|performance]\n"
                 "                             [--device N]\n"
                 "       nu_scaler_cli interpolate <a.png> <b.png> <out.png> [--t X | --multiplier 2..8] [--flow [--flow-warps 0..4]\n"
                 "                             [--flow-median 0|3|5] [--flow-project 0..4] [--flow-bidirectional]] [--device N]\n"
                 "                             (--flow-project: rounds that look the flow up where each output pixel's content came from;\n"
                 "                              --flow-bidirectional: both flows, each pixel takes the vector whose samples agree better)\n"
                 "                             [--method block_matching [--quality high|medium|low]] [--scene-detect]\n"
                 "                             [--bidirectional [--bidir-tolerance 0..96]]   (block matching: forward-backward check)\n"
                 "       nu_scaler_cli retime --from 24 --to 60 [--method optical_flow|block_matching|blend] [--flow-warps 0..4]\n"
                 "                             [--flow-median 0|3|5] [--flow-project 0..4] [--flow-bidirectional] [--bidirectional]\n"
                 "                             [--scene-detect] [--device N]\n"
                 "                             OUT_%%04d.png IN0.png IN1.png ...   (rates: integers or A/B; to/from reduced: terms <= 4096, <= 8)\n"
                 "       nu_scaler_cli scene <a.png> <b.png> [--mad 0..255] [--hist 0..1000] [--device N]\n"
                 "       nu_scaler_cli compare <a.png> <b.png> [--device N]\n"
                 "       nu_scaler_cli png-copy <in.png> <out.png>\n");
    return rc;
}

struct Args {
    std::vector<std::string> positional;
    std::map<std::string, std::string> options;
    bool flow = false;
    bool scene_detect = false;
    bool bidirectional = false;
    bool flow_bidirectional = false;
};

bool parse(int argc, char **argv, Args &a, std::string &err)
{
    for (int i = 2; i < argc; ++i) {
        const std::string s = argv[i];
        if (s == "--flow") {
            a.flow = true;
        } else if (s == "--scene-detect") {
            a.scene_detect = true;
        } else if (s == "--bidirectional") {
            a.bidirectional = true;
        } else if (s == "--flow-bidirectional") {
            a.flow_bidirectional = true;
        } else if (s.rfind("--", 0) == 0) {
            if (i + 1 >= argc) {
                err = "option " + s + " needs a value";
                return false;
            }
            a.options[s.substr(2)] = argv[++i];
        } else {
            a.positional.push_back(s);
        }
    }
    return true;
}

std::string lower(std::string s)
{
    for (char &c : s) c = (char)std::tolower((unsigned char)c);
    return s;
}

int quality_of(const std::string &q)
{
    const std::string s = lower(q);
    if (s == "ultra") return NUS_QUALITY_ULTRA;
    if (s == "balanced") return NUS_QUALITY_BALANCED;
    if (s == "performance") return NUS_QUALITY_PERFORMANCE;
    return NUS_QUALITY_QUALITY; // unknown strings default, as lib.rs:51-57
}

int cmd_upscale(const Args &a)
{
    if (a.positional.size() != 2) return usage(2);
    const auto opt = [&](const char *k, const char *dflt) {
        auto it = a.options.find(k);
        return it == a.options.end() ? std::string(dflt) : it->second;
    };
    const std::string tech = lower(opt("tech", "fallback")), quality = lower(opt("quality", "quality"));
    const float scale = (float)std::atof(opt("scale", "2.0").c_str());
    nus_cli::Image in;
    std::string err = nus_cli::read_png(a.positional[0], in);
    if (!err.empty()) return fail(err);
    if (tech == "none") { // PassThroughUpscaler
        err = nus_cli::write_png(a.positional[1], in);
        if (!err.empty()) return fail(err);
        std::printf("%s: %ux%u\n", a.positional[1].c_str(), in.width, in.height);
        return 0;
    }
    if (tech == "dlss") return fail("technology 'dlss' is not available on this device");
    if (tech != "fallback" && tech != "fsr" && tech != "wgpu") return fail("unknown technology '" + tech + "'");
    // (w as f32 * scale) as u32 -- Nu_scale/src/upscale/mod.rs:320-321
    const uint32_t ow = (uint32_t)((float)in.width * scale), oh = (uint32_t)((float)in.height * scale);
    if (ow == 0 || oh == 0) return fail("scale factor gives an empty output image");
    std::string alg = lower(opt("algorithm", ""));
    if (tech == "fsr") {
        alg = "fsr1";
    } else if (alg.empty()) { // quality -> algorithm, Nu_scale/src/upscale/mod.rs:295-303
        alg = quality == "ultra" ? "lanczos3" : (quality == "performance" ? "bilinear" : "bicubic");
    }
    static const std::map<std::string, int> kAlg = {
        {"nearest", NUS_ALG_NEAREST}, {"bilinear", NUS_ALG_BILINEAR}, {"lanczos3", NUS_ALG_LANCZOS3}, {"lanczos", NUS_ALG_LANCZOS3},
        {"bicubic", NUS_ALG_BICUBIC}, {"catmullrom", NUS_ALG_BICUBIC}, {"triangle", NUS_ALG_TRIANGLE},
        {"fsr1", NUS_ALG_FSR1}, {"fsr", NUS_ALG_FSR1}, {"easu", NUS_ALG_FSR_EASU}};
    const auto it = kAlg.find(alg);
    nus_upscaler *u = nus_upscaler_create(it == kAlg.end() ? NUS_ALG_NEAREST : it->second, quality_of(quality));
    if (!u) return fail(nus_last_error());
    int rc = nus_upscaler_set_device(u, std::atoi(opt("device", "0").c_str()));
    if (rc == NUS_OK) rc = nus_upscaler_initialize(u, in.width, in.height, ow, oh);
    nus_cli::Image out;
    out.width = ow;
    out.height = oh;
    out.rgba.resize((size_t)ow * oh * 4);
    if (rc == NUS_OK) rc = nus_upscaler_upscale(u, in.rgba.data(), in.rgba.size(), out.rgba.data(), out.rgba.size());
    if (rc != NUS_OK) {
        const std::string msg = nus_upscaler_last_error(u);
        nus_upscaler_destroy(u);
        return fail(msg);
    }
    nus_upscaler_destroy(u);
    err = nus_cli::write_png(a.positional[1], out);
    if (!err.empty()) return fail(err);
    std::printf("%s: %ux%u\n", a.positional[1].c_str(), ow, oh);
    return 0;
}

// <stem>_<k><ext>: where --multiplier M writes the frame at t = k / M
std::string multi_path(const std::string &out, uint32_t k)
{
    const size_t slash = out.find_last_of('/'), dot = out.find_last_of('.');
    const bool has_ext = dot != std::string::npos && (slash == std::string::npos || dot > slash);
    const std::string stem = has_ext ? out.substr(0, dot) : out, ext = has_ext ? out.substr(dot) : "";
    return stem + "_" + std::to_string(k) + ext;
}

int cmd_interpolate(const Args &a)
{
    if (a.positional.size() != 3) return usage(2);
    const auto m_it = a.options.find("multiplier");
    if (a.scene_detect && m_it == a.options.end()) {
        std::fprintf(stderr, "nu_scaler_cli: error: --scene-detect needs --multiplier\n");
        return usage(2);
    }
    uint32_t multiplier = 0; // 0: one frame at --t
    if (m_it != a.options.end()) { // usage errors before anything is read or written
        if (a.options.count("t")) {
            std::fprintf(stderr, "nu_scaler_cli: error: --multiplier and --t exclude each other\n");
            return usage(2);
        }
        char *end = nullptr;
        const long m = std::strtol(m_it->second.c_str(), &end, 10);
        if (end == m_it->second.c_str() || *end != '\0' || m < 2 || m > NUS_INTERP_MAX_TIMES + 1) {
            std::fprintf(stderr, "nu_scaler_cli: error: --multiplier must be from 2 to %d\n", NUS_INTERP_MAX_TIMES + 1);
            return usage(2);
        }
        multiplier = (uint32_t)m;
    }
    const auto method_it = a.options.find("method");
    int bm_quality = -1; // >= 0: --method block_matching at this nus_interp_quality_level
    if (method_it != a.options.end()) {
        if (a.flow) {
            std::fprintf(stderr, "nu_scaler_cli: error: --method and --flow exclude each other\n");
            return usage(2);
        }
        if (lower(method_it->second) != "block_matching") {
            std::fprintf(stderr, "nu_scaler_cli: error: --method must be block_matching, got %s\n", method_it->second.c_str());
            return usage(2);
        }
        const auto q_it = a.options.find("quality");
        const std::string q = q_it == a.options.end() ? "medium" : lower(q_it->second);
        bm_quality = q == "high" ? NUS_INTERP_QUALITY_HIGH : q == "medium" ? NUS_INTERP_QUALITY_MEDIUM : q == "low" ? NUS_INTERP_QUALITY_LOW : -1;
        if (bm_quality < 0) {
            std::fprintf(stderr, "nu_scaler_cli: error: --quality must be high, medium or low, got %s\n", q.c_str());
            return usage(2);
        }
    }
    const auto tol_it = a.options.find("bidir-tolerance");
    uint32_t bidir_tolerance = NUS_BM_BIDIR_DEFAULT_TOLERANCE;
    if ((a.bidirectional || tol_it != a.options.end()) && bm_quality < 0) {
        std::fprintf(stderr, "nu_scaler_cli: error: --bidirectional needs --method block_matching\n");
        return usage(2);
    }
    if (tol_it != a.options.end()) {
        if (!a.bidirectional) {
            std::fprintf(stderr, "nu_scaler_cli: error: --bidir-tolerance needs --bidirectional\n");
            return usage(2);
        }
        char *end = nullptr;
        const long v = std::strtol(tol_it->second.c_str(), &end, 10);
        if (end == tol_it->second.c_str() || *end != '\0' || v < 0 || v > 96) {
            std::fprintf(stderr, "nu_scaler_cli: error: --bidir-tolerance must be from 0 to 96\n");
            return usage(2);
        }
        bidir_tolerance = (uint32_t)v;
    }
    const auto warps_it = a.options.find("flow-warps");
    uint32_t flow_warps = 0; // the estimator's re-linearisation rounds per finer level (nus_flow_set_warps)
    if (warps_it != a.options.end()) {
        if (!a.flow) {
            std::fprintf(stderr, "nu_scaler_cli: error: --flow-warps needs --flow\n");
            return usage(2);
        }
        char *end = nullptr;
        const long v = std::strtol(warps_it->second.c_str(), &end, 10);
        if (end == warps_it->second.c_str() || *end != '\0' || v < 0 || v > NUS_FLOW_MAX_WARPS) {
            std::fprintf(stderr, "nu_scaler_cli: error: --flow-warps must be from 0 to %d\n", NUS_FLOW_MAX_WARPS);
            return usage(2);
        }
        flow_warps = (uint32_t)v;
    }
    const auto median_it = a.options.find("flow-median");
    uint32_t flow_median = 0; // the estimator's median filter behind every Jacobi run (nus_flow_set_median)
    if (median_it != a.options.end()) {
        if (!a.flow) {
            std::fprintf(stderr, "nu_scaler_cli: error: --flow-median needs --flow\n");
            return usage(2);
        }
        char *end = nullptr;
        const long v = std::strtol(median_it->second.c_str(), &end, 10);
        if (end == median_it->second.c_str() || *end != '\0' || (v != 0 && v != 3 && v != 5)) {
            std::fprintf(stderr, "nu_scaler_cli: error: --flow-median must be 0, 3 or 5\n");
            return usage(2);
        }
        flow_median = (uint32_t)v;
    }
    const auto project_it = a.options.find("flow-project");
    uint32_t flow_project = 0; // projection rounds of the warp with the estimated flow (nus_interp_set_flow_project)
    if (project_it != a.options.end()) {
        if (!a.flow) {
            std::fprintf(stderr, "nu_scaler_cli: error: --flow-project needs --flow\n");
            return usage(2);
        }
        char *end = nullptr;
        const long v = std::strtol(project_it->second.c_str(), &end, 10);
        if (end == project_it->second.c_str() || *end != '\0' || v < 0 || v > NUS_FLOW_MAX_PROJECT) {
            std::fprintf(stderr, "nu_scaler_cli: error: --flow-project must be from 0 to %d\n", NUS_FLOW_MAX_PROJECT);
            return usage(2);
        }
        flow_project = (uint32_t)v;
    }
    if (a.flow_bidirectional && !a.flow) { // both flows and the select warp (nus_interp_interpolate_select)
        std::fprintf(stderr, "nu_scaler_cli: error: --flow-bidirectional needs --flow\n");
        return usage(2);
    }
    nus_cli::Image fa, fb;
    std::string err = nus_cli::read_png(a.positional[0], fa);
    if (err.empty()) err = nus_cli::read_png(a.positional[1], fb);
    if (!err.empty()) return fail(err);
    if (fa.width != fb.width || fa.height != fb.height) return fail("frame sizes differ");
    const auto t_it = a.options.find("t");
    const float t = t_it == a.options.end() ? 0.5f : (float)std::atof(t_it->second.c_str());
    const auto d_it = a.options.find("device");
    const int device = d_it == a.options.end() ? 0 : std::atoi(d_it->second.c_str());
    if (bm_quality >= 0) { // block matching -> dense flow -> warp, one library call for all the frames
        const uint32_t n = multiplier ? multiplier - 1 : 1;
        std::vector<float> times(n, t);
        for (uint32_t k = 1; multiplier && k <= n; ++k) times[k - 1] = (float)((double)k / (double)multiplier);
        std::vector<uint8_t> frames(fa.rgba.size() * n);
        nus_blockmatch *bm = nus_bm_create();
        if (!bm) return fail(nus_last_error());
        int rc = nus_bm_set_device(bm, device);
        if (rc == NUS_OK) rc = nus_bm_set_quality(bm, bm_quality);
        if (rc == NUS_OK && a.bidirectional) rc = nus_bm_set_bidirectional(bm, 1, bidir_tolerance);
        if (rc == NUS_OK && a.scene_detect) rc = nus_bm_set_scene_detect(bm, 1, NUS_SCENE_DEFAULT_MAD, NUS_SCENE_DEFAULT_HIST_PERMILLE);
        if (rc == NUS_OK)
            rc = nus_bm_interpolate(bm, fa.rgba.data(), fa.rgba.size(), fb.rgba.data(), fb.rgba.size(), fa.width, fa.height, times.data(),
                                    n, NUS_INTERP_MODE_EXACT, frames.data(), frames.size());
        const std::string msg = rc == NUS_OK ? "" : nus_bm_last_error(bm);
        nus_bm_destroy(bm);
        if (rc != NUS_OK) return fail(msg);
        for (uint32_t k = 1; k <= n; ++k) {
            nus_cli::Image out;
            out.width = fa.width;
            out.height = fa.height;
            out.rgba.assign(frames.begin() + (size_t)(k - 1) * fa.rgba.size(), frames.begin() + (size_t)k * fa.rgba.size());
            const std::string path = multiplier ? multi_path(a.positional[2], k) : a.positional[2];
            err = nus_cli::write_png(path, out);
            if (!err.empty()) return fail(err);
            std::printf("%s\n", path.c_str());
        }
        return 0;
    }
    std::vector<float> flow, flow_bwd;
    if (a.flow) { // pyramid + Horn-Schunck front end instead of the reference's zero flow
        nus_flow *f = nus_flow_create();
        if (!f) return fail(nus_last_error());
        flow.resize((size_t)fa.width * fa.height * 2);
        int rc = nus_flow_set_device(f, device);
        if (rc == NUS_OK) rc = nus_flow_set_warps(f, flow_warps);
        if (rc == NUS_OK) rc = nus_flow_set_median(f, flow_median);
        // 3 levels, 50 coarse + 10 refining Jacobi steps, lambda as the Python mirror's FlowEstimator defaults
        if (rc == NUS_OK)
            rc = nus_flow_estimate(f, fa.rgba.data(), fb.rgba.data(), fa.width, fa.height, 3, 50, 10, 0.0004f, flow.data());
        if (rc == NUS_OK && a.flow_bidirectional) { // the same estimate B -> A
            flow_bwd.resize(flow.size());
            rc = nus_flow_estimate(f, fb.rgba.data(), fa.rgba.data(), fa.width, fa.height, 3, 50, 10, 0.0004f, flow_bwd.data());
        }
        const std::string msg = rc == NUS_OK ? "" : nus_flow_last_error(f);
        nus_flow_destroy(f);
        if (rc != NUS_OK) return fail(msg);
    }
    nus_interp *it = nus_interp_create(NUS_WG_WIDE_32X8);
    if (!it) return fail(nus_last_error());
    if (multiplier) { // the M - 1 frames at t = k / M from one call (the flow, if any, estimated once above)
        const uint32_t n = multiplier - 1;
        std::vector<float> times(n);
        for (uint32_t k = 1; k <= n; ++k) times[k - 1] = (float)((double)k / (double)multiplier);
        std::vector<uint8_t> frames(fa.rgba.size() * n);
        uint8_t cut = 0;
        if (a.scene_detect && nus_scene_detect(device, fa.rgba.data(), fa.rgba.size(), fb.rgba.data(), fb.rgba.size(), fa.width, fa.height,
                                               NUS_FORMAT_RGBA8, NUS_SCENE_DEFAULT_MAD, NUS_SCENE_DEFAULT_HIST_PERMILLE, nullptr,
                                               &cut) != NUS_OK) {
            nus_interp_destroy(it);
            return fail(nus_last_error());
        }
        if (cut) // a scene cut: repeats of the nearer frame -- the zero-flow launch at t = 0 / 1 (nus_scene_apply_cuts_device's copy)
            for (float &tk : times) tk = tk < 0.5f ? 0.0f : 1.0f;
        int rc = nus_interp_set_device(it, device);
        if (rc == NUS_OK) rc = nus_interp_set_flow_project(it, flow_project);
        if (rc == NUS_OK && a.flow_bidirectional && !cut)
            rc = nus_interp_interpolate_select(it, fa.rgba.data(), fa.rgba.size(), fb.rgba.data(), fb.rgba.size(), flow.data(),
                                               flow_bwd.data(), fa.width, fa.height, times.data(), n, frames.data(), frames.size());
        else if (rc == NUS_OK)
            rc = nus_interp_interpolate_multi(it, fa.rgba.data(), fa.rgba.size(), fb.rgba.data(), fb.rgba.size(),
                                              a.flow && !cut ? flow.data() : nullptr, fa.width, fa.height, times.data(), n, frames.data(),
                                              frames.size());
        const std::string msg = rc == NUS_OK ? "" : nus_interp_last_error(it);
        nus_interp_destroy(it);
        if (rc != NUS_OK) return fail(msg);
        for (uint32_t k = 1; k <= n; ++k) {
            nus_cli::Image out;
            out.width = fa.width;
            out.height = fa.height;
            out.rgba.assign(frames.begin() + (size_t)(k - 1) * fa.rgba.size(), frames.begin() + (size_t)k * fa.rgba.size());
            const std::string path = multi_path(a.positional[2], k);
            err = nus_cli::write_png(path, out);
            if (!err.empty()) return fail(err);
            std::printf("%s\n", path.c_str());
        }
        return 0;
    }
    nus_cli::Image out;
    out.width = fa.width;
    out.height = fa.height;
    out.rgba.resize(fa.rgba.size());
    int rc = nus_interp_set_device(it, device);
    if (rc == NUS_OK) rc = nus_interp_set_flow_project(it, flow_project);
    if (rc == NUS_OK && a.flow_bidirectional)
        rc = nus_interp_interpolate_select(it, fa.rgba.data(), fa.rgba.size(), fb.rgba.data(), fb.rgba.size(), flow.data(), flow_bwd.data(),
                                           fa.width, fa.height, &t, 1, out.rgba.data(), out.rgba.size());
    else if (rc == NUS_OK)
        rc = nus_interp_interpolate(it, fa.rgba.data(), fa.rgba.size(), fb.rgba.data(), fb.rgba.size(),
                                    a.flow ? flow.data() : nullptr, fa.width, fa.height, t, out.rgba.data(), out.rgba.size());
    const std::string msg = rc == NUS_OK ? "" : nus_interp_last_error(it);
    nus_interp_destroy(it);
    if (rc != NUS_OK) return fail(msg);
    err = nus_cli::write_png(a.positional[2], out);
    if (!err.empty()) return fail(err);
    std::printf("%s: %ux%u\n", a.positional[2].c_str(), out.width, out.height);
    return 0;
}

// one line, the same as `python -m nu_scaler_amd.cli compare`: mse=.. psnr=.. ssim=.. (inf / nan where they apply; SSIM is asked
// only when both sides are at least 11 pixels)
int cmd_compare(const Args &a)
{
    if (a.positional.size() != 2) return usage(2);
    nus_cli::Image fa, fb;
    std::string err = nus_cli::read_png(a.positional[0], fa);
    if (err.empty()) err = nus_cli::read_png(a.positional[1], fb);
    if (!err.empty()) return fail(err);
    if (fa.width != fb.width || fa.height != fb.height) return fail("Images must have the same dimensions");
    const auto d_it = a.options.find("device");
    const int device = d_it == a.options.end() ? 0 : std::atoi(d_it->second.c_str());
    const int what = NUS_METRIC_MSE | (fa.width >= 11 && fa.height >= 11 ? NUS_METRIC_SSIM : 0);
    double m[3] = {0, 0, 0};
    if (nus_metrics_compare(device, fa.rgba.data(), fa.rgba.size(), fb.rgba.data(), fb.rgba.size(), fa.width, fa.height, what, m) !=
        NUS_OK)
        return fail(nus_last_error());
    std::printf("mse=%.6f psnr=%.6f ssim=%.6f\n", m[0], m[1], m[2]);
    return 0;
}

// one line, the same as `python -m nu_scaler_amd.cli scene`
int cmd_scene(const Args &a)
{
    if (a.positional.size() != 2) return usage(2);
    long mad = NUS_SCENE_DEFAULT_MAD, hist = NUS_SCENE_DEFAULT_HIST_PERMILLE;
    const auto m_it = a.options.find("mad"), h_it = a.options.find("hist");
    if (m_it != a.options.end()) mad = std::atol(m_it->second.c_str());
    if (h_it != a.options.end()) hist = std::atol(h_it->second.c_str());
    if (mad < 0 || mad > 255 || hist < 0 || hist > 1000) { // usage errors before anything is read
        std::fprintf(stderr, "nu_scaler_cli: error: --mad must be from 0 to 255 and --hist from 0 to 1000\n");
        return usage(2);
    }
    nus_cli::Image fa, fb;
    std::string err = nus_cli::read_png(a.positional[0], fa);
    if (err.empty()) err = nus_cli::read_png(a.positional[1], fb);
    if (!err.empty()) return fail(err);
    if (fa.width != fb.width || fa.height != fb.height) return fail("Images must have the same dimensions");
    const auto d_it = a.options.find("device");
    const int device = d_it == a.options.end() ? 0 : std::atoi(d_it->second.c_str());
    nus_scene_measures m = {0, 0, 0};
    uint8_t cut = 0;
    if (nus_scene_detect(device, fa.rgba.data(), fa.rgba.size(), fb.rgba.data(), fb.rgba.size(), fa.width, fa.height, NUS_FORMAT_RGBA8,
                         (uint32_t)mad, (uint32_t)hist, &m, &cut) != NUS_OK)
        return fail(nus_last_error());
    const double px = (double)fa.width * fa.height;
    std::printf("cut=%d mad=%.3f hist_permille=%.1f\n", (int)cut, (double)m.sad / (3.0 * px), (double)m.hist_l1 * 1000.0 / (2.0 * px));
    return 0;
}

int cmd_png_copy(const Args &a)
{
    if (a.positional.size() != 2) return usage(2);
    nus_cli::Image img;
    std::string err = nus_cli::read_png(a.positional[0], img);
    if (err.empty()) err = nus_cli::write_png(a.positional[1], img);
    if (!err.empty()) return fail(err);
    std::printf("%s: %ux%u\n", a.positional[1].c_str(), img.width, img.height);
    return 0;
}

// "24" or "24000/1001" -> (n, d), both positive and below 2^31
bool parse_rate(const std::string &s, uint64_t &n, uint64_t &d)
{
    const size_t slash = s.find('/');
    const std::string a = s.substr(0, slash), b = slash == std::string::npos ? "1" : s.substr(slash + 1);
    for (const std::string *p : {&a, &b})
        if (p->empty() || p->size() > 9 || p->find_first_not_of("0123456789") != std::string::npos) return false;
    n = std::strtoull(a.c_str(), nullptr, 10), d = std::strtoull(b.c_str(), nullptr, 10);
    return n != 0 && d != 0;
}

uint64_t gcd_u64(uint64_t a, uint64_t b)
{
    while (b) {
        const uint64_t r = a % b;
        a = b, b = r;
    }
    return a;
}

// exactly one integer conversion (%d, %4d, %04d) and no other '%'
bool pattern_ok(const std::string &p)
{
    const size_t at = p.find('%');
    if (at == std::string::npos || p.find('%', at + 1) != std::string::npos) return false;
    size_t i = at + 1;
    while (i < p.size() && std::isdigit((unsigned char)p[i])) ++i;
    return i < p.size() && p[i] == 'd' && i - at <= 4;
}

std::string pattern_path(const std::string &p, uint64_t j)
{
    char buf[64];
    const size_t at = p.find('%'), d = p.find('d', at);
    std::snprintf(buf, sizeof buf, p.substr(at, d - at + 1).c_str(), (int)j);
    return p.substr(0, at) + buf + p.substr(d + 1);
}

// retime --from 24 --to 60 [...] OUT_%04d.png IN0.png IN1.png ...: the schedule from nus_retime_schedule; a real-frame output is
// the input frame, the in-between outputs of a pair come from one host call of the method per pair -- which by the contract of the
// retime entry points are the bytes the device-resident conversion (`python -m nu_scaler_amd.cli retime`) writes.
int cmd_retime(const Args &a)
{
    // usage errors before anything is read or written
    const auto from_it = a.options.find("from"), to_it = a.options.find("to");
    uint64_t fn, fd, tn, td;
    if (from_it == a.options.end() || to_it == a.options.end() || !parse_rate(from_it->second, fn, fd) || !parse_rate(to_it->second, tn, td)) {
        std::fprintf(stderr, "nu_scaler_cli: error: retime needs --from and --to, each a positive integer or a fraction A/B\n");
        return usage(2);
    }
    uint64_t num = tn * fd, den = td * fn;
    const uint64_t g = gcd_u64(num, den);
    num /= g, den /= g;
    if (num > NUS_RETIME_MAX_TERM || den > NUS_RETIME_MAX_TERM || num > (uint64_t)(NUS_INTERP_MAX_TIMES + 1) * den) {
        std::fprintf(stderr, "nu_scaler_cli: error: the reduced ratio %llu/%llu needs terms of at most %d and a value of at most %d\n",
                     (unsigned long long)num, (unsigned long long)den, NUS_RETIME_MAX_TERM, NUS_INTERP_MAX_TIMES + 1);
        return usage(2);
    }
    if (a.positional.empty() || !pattern_ok(a.positional[0])) {
        std::fprintf(stderr, "nu_scaler_cli: error: the output pattern needs exactly one %%d conversion (as OUT_%%04d.png)\n");
        return usage(2);
    }
    if (a.positional.size() < 3) {
        std::fprintf(stderr, "nu_scaler_cli: error: retime needs at least 2 input frames\n");
        return usage(2);
    }
    const auto method_it = a.options.find("method");
    const std::string method = method_it == a.options.end() ? "optical_flow" : lower(method_it->second);
    if (method != "optical_flow" && method != "block_matching" && method != "blend") {
        std::fprintf(stderr, "nu_scaler_cli: error: --method must be optical_flow, block_matching or blend, got %s\n", method.c_str());
        return usage(2);
    }
    long flow_opt[3] = {0, 0, 0}; // warps, median, project
    const char *const flow_names[3] = {"flow-warps", "flow-median", "flow-project"};
    for (int i = 0; i < 3; ++i) {
        const auto it = a.options.find(flow_names[i]);
        if (it == a.options.end()) continue;
        char *end = nullptr;
        const long v = std::strtol(it->second.c_str(), &end, 10);
        const bool in_range = i == 1 ? (v == 0 || v == 3 || v == 5) : (v >= 0 && v <= (i == 0 ? NUS_FLOW_MAX_WARPS : NUS_FLOW_MAX_PROJECT));
        if (method != "optical_flow" || end == it->second.c_str() || *end != '\0' || !in_range) {
            std::fprintf(stderr, "nu_scaler_cli: error: --%s needs --method optical_flow and a value in range, got %s\n", flow_names[i],
                         it->second.c_str());
            return usage(2);
        }
        flow_opt[i] = v;
    }
    if (a.flow_bidirectional && method != "optical_flow") {
        std::fprintf(stderr, "nu_scaler_cli: error: --flow-bidirectional needs --method optical_flow\n");
        return usage(2);
    }
    if (a.bidirectional && method != "block_matching") {
        std::fprintf(stderr, "nu_scaler_cli: error: --bidirectional needs --method block_matching\n");
        return usage(2);
    }
    const auto d_it = a.options.find("device");
    const int device = d_it == a.options.end() ? 0 : std::atoi(d_it->second.c_str());

    const uint32_t n = (uint32_t)(a.positional.size() - 1);
    std::vector<nus_cli::Image> in(n);
    for (uint32_t k = 0; k < n; ++k) {
        const std::string err = nus_cli::read_png(a.positional[k + 1], in[k]);
        if (!err.empty()) return fail(err);
        if (in[k].width != in[0].width || in[k].height != in[0].height) return fail("frame sizes differ");
    }
    const uint32_t w = in[0].width, h = in[0].height;
    const size_t fb = in[0].rgba.size();
    const int64_t n_out = nus_retime_count(n, (uint32_t)num, (uint32_t)den);
    if (n_out < 0) return fail(nus_last_error());
    std::vector<nus_retime_entry> sched((size_t)n_out);
    if (nus_retime_schedule(n, (uint32_t)num, (uint32_t)den, 0, (uint64_t)n_out, sched.data()) != NUS_OK) return fail(nus_last_error());

    nus_blockmatch *bm = nullptr;
    nus_flow *fl = nullptr;
    nus_interp *it = nullptr;
    int rc = NUS_OK;
    std::string msg;
    if (method == "block_matching") {
        if (!(bm = nus_bm_create())) return fail(nus_last_error());
        rc = nus_bm_set_device(bm, device);
        if (rc == NUS_OK) rc = nus_bm_set_quality(bm, NUS_INTERP_QUALITY_MEDIUM);
        if (rc == NUS_OK && a.bidirectional) rc = nus_bm_set_bidirectional(bm, 1, NUS_BM_BIDIR_DEFAULT_TOLERANCE);
        if (rc == NUS_OK && a.scene_detect) rc = nus_bm_set_scene_detect(bm, 1, NUS_SCENE_DEFAULT_MAD, NUS_SCENE_DEFAULT_HIST_PERMILLE);
        if (rc != NUS_OK) msg = nus_bm_last_error(bm);
    } else {
        if (!(it = nus_interp_create(NUS_WG_WIDE_32X8))) return fail(nus_last_error());
        rc = nus_interp_set_device(it, device);
        if (rc == NUS_OK) rc = nus_interp_set_flow_project(it, (uint32_t)flow_opt[2]);
        if (rc != NUS_OK) msg = nus_interp_last_error(it);
        if (rc == NUS_OK && method == "optical_flow") {
            if (!(fl = nus_flow_create())) {
                nus_interp_destroy(it);
                return fail(nus_last_error());
            }
            rc = nus_flow_set_device(fl, device);
            if (rc == NUS_OK) rc = nus_flow_set_warps(fl, (uint32_t)flow_opt[0]);
            if (rc == NUS_OK) rc = nus_flow_set_median(fl, (uint32_t)flow_opt[1]);
            if (rc != NUS_OK) msg = nus_flow_last_error(fl);
        }
    }
    std::vector<float> flow, flow_bwd, times;
    std::vector<uint8_t> frames;
    std::string err;
    for (size_t j = 0; rc == NUS_OK && err.empty() && j < sched.size();) {
        const uint32_t k = sched[j].pair;
        nus_cli::Image out;
        out.width = w, out.height = h;
        if (sched[j].rem == 0) { // a real frame
            out.rgba = in[k].rgba;
            err = nus_cli::write_png(pattern_path(a.positional[0], j), out);
            if (err.empty()) std::printf("%s\n", pattern_path(a.positional[0], j).c_str());
            ++j;
            continue;
        }
        size_t end = j; // the in-between outputs of pair k: one call
        times.clear();
        while (end < sched.size() && sched[end].pair == k && sched[end].rem != 0) times.push_back(sched[end++].t);
        const uint32_t nt = (uint32_t)times.size();
        frames.resize(fb * nt);
        const uint8_t *pa = in[k].rgba.data(), *pb = in[k + 1].rgba.data();
        if (bm) {
            rc = nus_bm_interpolate(bm, pa, fb, pb, fb, w, h, times.data(), nt, NUS_INTERP_MODE_EXACT, frames.data(), frames.size());
            if (rc != NUS_OK) msg = nus_bm_last_error(bm);
        } else {
            uint8_t cut = 0;
            if (a.scene_detect && (rc = nus_scene_detect(device, pa, fb, pb, fb, w, h, NUS_FORMAT_RGBA8, NUS_SCENE_DEFAULT_MAD,
                                                         NUS_SCENE_DEFAULT_HIST_PERMILLE, nullptr, &cut)) != NUS_OK)
                msg = nus_last_error();
            if (rc == NUS_OK && cut) // repeats of the nearer frame: the zero-flow launch at t = 0 / 1
                for (float &tk : times) tk = tk < 0.5f ? 0.0f : 1.0f;
            if (rc == NUS_OK && fl && !cut) {
                flow.resize((size_t)w * h * 2);
                // 3 levels, 50 coarse + 10 refining Jacobi steps, lambda as the Python mirror's FlowEstimator defaults
                rc = nus_flow_estimate(fl, pa, pb, w, h, 3, 50, 10, 0.0004f, flow.data());
                if (rc == NUS_OK && a.flow_bidirectional) { // the same estimate B -> A
                    flow_bwd.resize(flow.size());
                    rc = nus_flow_estimate(fl, pb, pa, w, h, 3, 50, 10, 0.0004f, flow_bwd.data());
                }
                if (rc != NUS_OK) msg = nus_flow_last_error(fl);
            }
            if (rc == NUS_OK && fl && !cut && a.flow_bidirectional) { // both flows and the select warp
                rc = nus_interp_interpolate_select(it, pa, fb, pb, fb, flow.data(), flow_bwd.data(), w, h, times.data(), nt, frames.data(),
                                                   frames.size());
                if (rc != NUS_OK) msg = nus_interp_last_error(it);
            } else if (rc == NUS_OK) {
                rc = nus_interp_interpolate_multi(it, pa, fb, pb, fb, fl && !cut ? flow.data() : nullptr, w, h, times.data(), nt,
                                                  frames.data(), frames.size());
                if (rc != NUS_OK) msg = nus_interp_last_error(it);
            }
        }
        for (uint32_t i = 0; rc == NUS_OK && err.empty() && i < nt; ++i) {
            out.rgba.assign(frames.begin() + (size_t)i * fb, frames.begin() + (size_t)(i + 1) * fb);
            err = nus_cli::write_png(pattern_path(a.positional[0], j + i), out);
            if (err.empty()) std::printf("%s\n", pattern_path(a.positional[0], j + i).c_str());
        }
        j = end;
    }
    if (bm) nus_bm_destroy(bm);
    if (fl) nus_flow_destroy(fl);
    if (it) nus_interp_destroy(it);
    if (rc != NUS_OK) return fail(msg);
    if (!err.empty()) return fail(err);
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc < 2) return usage(2);
    const std::string cmd = argv[1];
    if (cmd == "--help" || cmd == "-h" || cmd == "help") return usage(0);
    Args a;
    std::string err;
    if (!parse(argc, argv, a, err)) return fail(err);
    if (cmd == "upscale") return cmd_upscale(a);
    if (cmd == "interpolate") return cmd_interpolate(a);
    if (cmd == "retime") return cmd_retime(a);
    if (cmd == "compare") return cmd_compare(a);
    if (cmd == "scene") return cmd_scene(a);
    if (cmd == "png-copy") return cmd_png_copy(a);
    return usage(2);
}
