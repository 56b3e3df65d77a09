// Host-only driver of the kernel selection (nus_plan.cpp + nus_tables.cpp, no HIP; tests/test_host_logic.py builds it with plain g++
// and again with -fsanitize=address,undefined).
//
//  * stdout: one JSON document with plan_kernels()'s answer for every case below -- the variant name, every scalar field and, for
//    every vector of the plan, its length and the CRC-32 of its bytes.  The test compares it with tests/golden/kernel_plan_parent.json,
//    recorded from the member-function selection this unit replaced.
//  * for every case plan_kernels() is called twice with the same inputs, and once more behind a call for ANOTHER shape: the three plans
//    must be identical (a plan is built from nothing but its inputs).
//  * equal_row_blocks() against the four expressions it replaced in HipUpscaler::enqueue(), written out here as they stood.
// stderr: "fresh bad N" and "row_blocks compared M bad N"; exit status 1 if either N is not 0.
#include "nus_plan.hpp"

#include <cstdio>
#include <cstring>
#include <string>

using namespace nus;

namespace {

uint32_t crc32_of(const void *data, size_t n) // CRC-32 (IEEE 802.3, as zlib.crc32)
{
    const uint8_t *p = static_cast<const uint8_t *>(data);
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) {
        c ^= p[i];
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
    }
    return ~c;
}

template <class T>
void put_vector(std::string &s, const std::vector<T> &v, bool last = false)
{
    char buf[64];
    snprintf(buf, sizeof buf, "[%zu,%u]%s", v.size(), v.empty() ? 0u : crc32_of(v.data(), v.size() * sizeof(T)), last ? "" : ",");
    s += buf;
}

// the fields of a plan as the JSON of one case (after its id)
std::string fields(const KernelPlan &p)
{
    char buf[256];
    snprintf(buf, sizeof buf, "\"variant\":\"%s\",\"s\":[%u,%u,%u,%d,%d,%u,%u,%d,%u,%u],\"v\":[", variant_name(p.variant), p.xs_factor, p.pq_p,
             p.pq_q, (int)p.pq_narrow, (int)p.pq_exact_fallback, p.ncols_max, p.union_taps, (int)p.small_taps, p.win_outputs_per_lane,
             p.down_seg_w);
    std::string s = buf;
    put_vector(s, p.down_rows);
    put_vector(s, p.down_done);
    put_vector(s, p.wx6);
    put_vector(s, p.wy6);
    put_vector(s, p.xs_cls_x);
    put_vector(s, p.xs_cls_y);
    put_vector(s, p.xs_wcls_x);
    put_vector(s, p.xs_wcls_y, true);
    return s + "]";
}
const char *kHeader = "\"scalars\":[\"xs_factor\",\"pq_p\",\"pq_q\",\"pq_narrow\",\"pq_exact_fallback\",\"ncols_max\",\"union_taps\",\"small_taps\","
                      "\"win_outputs_per_lane\",\"down_seg_w\"],\n"
                      "\"vectors\":[\"down_rows\",\"down_done\",\"wx6\",\"wy6\",\"xs_cls_x\",\"xs_cls_y\",\"xs_wcls_x\",\"xs_wcls_y\"],\n";

bool same(const KernelPlan &a, const KernelPlan &b)
{
    return a.variant == b.variant && a.xs_factor == b.xs_factor && a.pq_p == b.pq_p && a.pq_q == b.pq_q && a.pq_narrow == b.pq_narrow &&
           a.pq_exact_fallback == b.pq_exact_fallback && a.ncols_max == b.ncols_max && a.union_taps == b.union_taps &&
           a.small_taps == b.small_taps && a.win_outputs_per_lane == b.win_outputs_per_lane && a.down_seg_w == b.down_seg_w &&
           a.down_rows == b.down_rows && a.down_done == b.down_done && a.xs_cls_x == b.xs_cls_x && a.xs_cls_y == b.xs_cls_y &&
           // the weights byte for byte (operator== of float would call two NaNs different and -0 and 0 the same)
           a.wx6.size() == b.wx6.size() && a.wy6.size() == b.wy6.size() && a.xs_wcls_x.size() == b.xs_wcls_x.size() &&
           a.xs_wcls_y.size() == b.xs_wcls_y.size() && (a.wx6.empty() || !memcmp(a.wx6.data(), b.wx6.data(), a.wx6.size() * 4)) &&
           (a.wy6.empty() || !memcmp(a.wy6.data(), b.wy6.data(), a.wy6.size() * 4)) &&
           (a.xs_wcls_x.empty() || !memcmp(a.xs_wcls_x.data(), b.xs_wcls_x.data(), a.xs_wcls_x.size() * 4)) &&
           (a.xs_wcls_y.empty() || !memcmp(a.xs_wcls_y.data(), b.xs_wcls_y.data(), a.xs_wcls_y.size() * 4));
}

struct Shape {
    uint32_t iw, ih, ow, oh;
};
const Shape kShapes[] = {
    // the workload's own: 1080p -> 4K, 720p -> 1080p, 1080p -> 1440p, 1440p -> 4K, 768p -> 1080p, 864p -> 4K, 4K -> 1080p, 4K -> 720p
    {1920, 1080, 3840, 2160}, {1280, 720, 1920, 1080}, {1920, 1080, 2560, 1440}, {2560, 1440, 3840, 2160}, {1366, 768, 1920, 1080},
    {1536, 864, 3840, 2160}, {3840, 2160, 1920, 1080}, {3840, 2160, 1280, 720},
    // every fixed-ratio family at its smallest accepted size, and one step below it: x2, x3, x4, x3/2, x4/3
    {16, 16, 32, 32}, {12, 16, 24, 32}, {16, 16, 48, 48}, {12, 16, 36, 48}, {16, 16, 64, 64}, {12, 16, 48, 64},
    {32, 16, 48, 24}, {24, 16, 36, 24}, {48, 18, 64, 24}, {36, 18, 48, 24},
    // the eight P/Q factors at iw >= 32, ih >= 12, once with ow % 4 == 0 and once without (x8/5: ow = 8 (iw / 5) is always one)
    {32, 12, 40, 15}, {36, 12, 45, 15},   // x5/4
    {40, 15, 48, 18}, {35, 15, 42, 18},   // x6/5
    {36, 12, 60, 20}, {33, 12, 55, 20},   // x5/3
    {32, 12, 80, 30}, {34, 12, 85, 30},   // x5/2
    {32, 12, 112, 42}, {34, 12, 119, 42}, // x7/2
    {40, 15, 56, 21}, {35, 15, 49, 21},   // x7/5
    {35, 15, 56, 24},                     // x8/5
    {40, 15, 72, 27}, {35, 15, 63, 27},   // x9/5
    // the odd ones: no ratio at all, x0.4, x0.21 (windows wider than the table), x1, x1.006, x1.4, x10
    {100, 60, 237, 141}, {500, 500, 200, 200}, {1000, 1000, 210, 210}, {9, 9, 9, 9}, {64, 64, 64, 64}, {517, 40, 520, 41},
    {100, 60, 140, 84}, {480, 270, 680, 384}, {32, 24, 320, 240}, {100, 37, 1000, 99},
    // ... and the small ones the handle is run on (tests/test_gpu_parity.py): x1/2 down, x3/2 below the resize kernel's width
    {64, 64, 32, 32}, {32, 12, 48, 18},
};

struct OptionSet {
    const char *name;
    PlanOptions opt;
};
std::vector<OptionSet> option_sets()
{
    std::vector<OptionSet> v(6);
    v[0].name = "defaults";
    v[1].name = "force_general", v[1].opt.force_general = true;
    v[2].name = "force_rows", v[2].opt.force_rows = true;
    v[3].name = "force_per_pixel", v[3].opt.force_per_pixel = true;
    v[4].name = "down_seg_width=48", v[4].opt.down_seg_width = 48;
    v[5].name = "wgsl_bilinear", v[5].opt.wgsl_bilinear = true;
    return v;
}

struct Alg {
    const char *name;
    Algorithm a;
    ResizeFilter filter;
    bool resize;
};
const Alg kAlgs[] = {{"nearest", Algorithm::Nearest, ResizeFilter::Lanczos3, false},  {"bilinear", Algorithm::Bilinear, ResizeFilter::Lanczos3, false},
                     {"lanczos3", Algorithm::Lanczos3, ResizeFilter::Lanczos3, true}, {"bicubic", Algorithm::Bicubic, ResizeFilter::CatmullRom, true},
                     {"triangle", Algorithm::Triangle, ResizeFilter::Triangle, true}, {"fsr1", Algorithm::Fsr1, ResizeFilter::Lanczos3, false}};

// ---- equal_row_blocks() against HipUpscaler::enqueue()'s four computations, as they stood --------------------------------------

constexpr uint32_t kLanczosX2StripCols = 240; // nus_kernels.hpp

uint32_t parent_r43(uint32_t iw_, uint32_t ih_, uint32_t n_frames)
{
    const uint64_t rows_total = (uint64_t)ih_ * ((iw_ + 185) / 186) * n_frames;
    uint64_t t = rows_total / 12288;
    t = t < 12 ? 12 : (t > 36 ? 36 : t);
    const uint64_t blocks = (ih_ + t - 1) / t;
    return (uint32_t)(((ih_ + blocks - 1) / blocks + 2) / 3 * 3);
}

uint32_t parent_pq(uint32_t iw_, uint32_t ih_, uint32_t n_frames, uint32_t cols, uint32_t pq_q_)
{
    const uint64_t rows_total = (uint64_t)ih_ * ((iw_ + cols - 1) / cols) * n_frames;
    uint64_t t = rows_total / 12288;
    t = t < 12 ? 12 : (t > 36 ? 36 : t);
    const uint64_t blocks = (ih_ + t - 1) / t;
    return (uint32_t)(((ih_ + blocks - 1) / blocks + pq_q_ - 1) / pq_q_ * pq_q_);
}

uint32_t parent_r32(uint32_t iw_, uint32_t ih_, uint32_t n_frames)
{
    const uint64_t rows_total = (uint64_t)ih_ * ((iw_ + 239) / 240) * n_frames;
    uint64_t t = rows_total / 12288;
    t = t < 12 ? 12 : (t > 48 ? 48 : t);
    const uint64_t blocks = (ih_ + t - 1) / t;
    return (uint32_t)((ih_ + blocks - 1) / blocks + 1) & ~1u;
}

uint32_t parent_xs(uint32_t iw_, uint32_t ih_, uint32_t n_frames)
{
    const uint64_t rows_total = (uint64_t)ih_ * ((iw_ + kLanczosX2StripCols - 1) / kLanczosX2StripCols) * n_frames;
    uint64_t t = rows_total / 16384;
    t = t < 8 ? 8 : (t > 16 ? 16 : t);
    const uint64_t blocks = (ih_ + t - 1) / t;
    return (uint32_t)((ih_ + blocks - 1) / blocks);
}

int check_row_blocks()
{
    // every supported P / Q with the input columns of its strip (PqGeom<P, Q>::kStripCols, nus_k_lanczos_pq.hpp)
    const uint32_t pq[][3] = {{5, 4, 240}, {6, 5, 310}, {5, 3, 180}, {5, 2, 120}, {7, 2, 120}, {7, 5, 300}, {8, 5, 310}, {9, 5, 300}};
    unsigned compared = 0, bad = 0;
    auto strips = [](uint32_t iw, uint32_t cols) { return (iw + cols - 1) / cols; };
    for (uint32_t ih : {12u, 16u, 18u, 24u, 60u, 720u, 1080u, 1440u, 2160u})
        for (uint32_t iw : {32u, 48u, 186u, 240u, 1280u, 1920u, 3840u})
            for (uint32_t n : {1u, 2u, 12u, 300u}) {
                bad += equal_row_blocks(ih, strips(iw, 186), n, 12288, 12, 36, 3) != parent_r43(iw, ih, n);
                bad += equal_row_blocks(ih, strips(iw, 240), n, 12288, 12, 48, 2) != parent_r32(iw, ih, n);
                bad += equal_row_blocks(ih, strips(iw, kLanczosX2StripCols), n, 16384, 8, 16, 1) != parent_xs(iw, ih, n);
                compared += 3;
                for (const auto &f : pq) {
                    if (!lanczos_pq_supported(f[0], f[1])) ++bad;
                    bad += equal_row_blocks(ih, strips(iw, f[2]), n, 12288, 12, 36, f[1]) != parent_pq(iw, ih, n, f[2], f[1]);
                    ++compared;
                }
            }
    fprintf(stderr, "row_blocks compared %u bad %u\n", compared, bad);
    return bad ? 1 : 0;
}

} // namespace

int main()
{
    const std::vector<OptionSet> sets = option_sets();
    unsigned fresh_bad = 0, cases = 0;
    AxisTables px, py; // the tables of the case before: the "other shape" of the freshness check
    PlanOptions popt;
    Algorithm palg = Algorithm::Nearest;
    printf("{%s\"cases\":[", kHeader);
    for (const Alg &alg : kAlgs)
        for (const OptionSet &os : sets)
            for (const Shape &sh : kShapes) { // (innermost: the case before is always another shape)
                AxisTables tx, ty;
                build_axis_tables(sh.iw, sh.ow, os.opt.wgsl_bilinear, tx, alg.filter);
                build_axis_tables(sh.ih, sh.oh, os.opt.wgsl_bilinear, ty, alg.filter);
                printf("%s\n{\"id\":\"%s %ux%u->%ux%u %s\",", cases++ ? "," : "", alg.name, sh.iw, sh.ih, sh.ow, sh.oh, os.name);
                // (a window wider than the table: initialize() refuses the shape before it selects anything)
                if (alg.resize && (tx.lz_max_taps < 0 || ty.lz_max_taps < 0)) {
                    printf("\"variant\":\"unsupported\",\"s\":[],\"v\":[]}");
                    continue;
                }
                const KernelPlan plan = plan_kernels(alg.a, os.opt, tx, ty);
                printf("%s}", fields(plan).c_str());
                if (!same(plan, plan_kernels(alg.a, os.opt, tx, ty))) ++fresh_bad;
                if (px.out_n) {
                    (void)plan_kernels(palg, popt, px, py);
                    if (!same(plan, plan_kernels(alg.a, os.opt, tx, ty))) ++fresh_bad;
                }
                px = std::move(tx), py = std::move(ty), popt = os.opt, palg = alg.a;
            }
    printf("\n]}\n");
    fprintf(stderr, "cases %u fresh bad %u\n", cases, fresh_bad);
    return check_row_blocks() | (fresh_bad ? 1 : 0);
}
