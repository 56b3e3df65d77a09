// nus_cli.cpp -- `nu_scaler_cli`: the image-file commands of the north star's CLI as a native program on the
// C ABI (include/nuscaler_hip.h).  Shape: `upscale_image_file` of the legacy crate
// (Nu_scale/src/upscale/mod.rs:307-338) and the option names of its `fullscreen` subcommand
// (Nu_scale/src/main.rs:36-73: --tech, --quality, --algorithm).
//
//   nu_scaler_cli upscale <in.png> <out.png> [--algorithm A] [--scale S] [--tech T] [--quality Q] [--device N]
//   nu_scaler_cli interpolate <a.png> <b.png> <out.png> [--t X | --multiplier M] [--flow [--flow-warps N] [--flow-median 0|3|5] [--flow-project N]] [--device N]
//                             [--method block_matching [--quality high|medium|low] [--bidirectional [--bidir-tolerance N]]]
//   nu_scaler_cli scene <a.png> <b.png> [--mad N] [--hist N] [--device N]   (the scene-cut detector: cut=0|1 mad=.. hist_permille=..)
//   nu_scaler_cli compare <a.png> <b.png> [--device N]   (MSE / PSNR / SSIM, ErrorMetrics: Nu_scale/src/upscale/common.rs:475-543)
//   nu_scaler_cli png-copy <in.png> <out.png>        (decode + encode only; no GPU: codec self-check)
//
// Pixels go through the HIP kernels only: without a device the commands fail.
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
                 "                             [--flow-median 0|3|5] [--flow-project 0..4]] [--device N]\n"
                 "                             (--flow-project: rounds that look the flow up where each output pixel's content came from)\n"
                 "                             [--method block_matching [--quality high|medium|low]] [--scene-detect]\n"
                 "                             [--bidirectional [--bidir-tolerance 0..96]]   (block matching: forward-backward check)\n"
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
    std::vector<float> flow;
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
        if (rc == NUS_OK)
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
    if (rc == NUS_OK)
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
    if (cmd == "compare") return cmd_compare(a);
    if (cmd == "scene") return cmd_scene(a);
    if (cmd == "png-copy") return cmd_png_copy(a);
    return usage(2);
}
