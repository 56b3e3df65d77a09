// nus_plan.cpp -- the kernel selection of an upscaler handle (nus_plan.hpp).
#include "nus_plan.hpp"

#include <cstring>

namespace nus {

const char *variant_name(Variant v)
{
    switch (v) {
    case Variant::NearestTable: return "nearest_table";
    case Variant::NearestX2: return "nearest_x2_vec16";
    case Variant::NearestRatio: return "nearest_ratio";
    case Variant::BilinearTable: return "bilinear_table_f32";
    case Variant::BilinearX2Int: return "bilinear_x2_packed_u8";
    case Variant::BilinearRatio: return "bilinear_ratio_f32";
    case Variant::LanczosGeneral: return "lanczos3_general";
    case Variant::ResizeRows: return "resize_rows_lds";
    case Variant::ResizeWin: return "resize_regwin_lds";
    case Variant::ResizeDown: return "resize_down_stream";
    case Variant::LanczosX2RegWin: return "lanczos3_x2_regwin";
    case Variant::LanczosXsRegWin: return "lanczos3_xs_regwin";
    case Variant::LanczosR32RegWin: return "lanczos3_r32_regwin";
    case Variant::LanczosR43RegWin: return "lanczos3_r43_regwin";
    case Variant::LanczosPqRegWin: return "lanczos3_pq_regwin";
    case Variant::FsrEasu: return "fsr1_easu_tile";
    case Variant::FsrRcas: return "fsr1_rcas_rows";
    case Variant::Fsr1Fused: return "fsr1_easu_rcas_fused_lds";
    case Variant::Fsr1TwoPass: return "fsr1_easu_then_rcas_rows";
    }
    return "?";
}

bool lanczos_pq_supported(uint32_t P, uint32_t Q)
{
    return (P == 5 && Q == 4) || (P == 6 && Q == 5) || (P == 5 && Q == 3) || (P == 5 && Q == 2) || (P == 7 && Q == 2) ||
           (P == 7 && Q == 5) || (P == 8 && Q == 5) || (P == 9 && Q == 5);
}

uint32_t equal_row_blocks(uint32_t ih, uint32_t strips, uint32_t n_frames, uint32_t rows_per_round, uint32_t lo, uint32_t hi,
                          uint32_t multiple)
{
    const uint64_t rows_total = (uint64_t)ih * strips * n_frames;
    uint64_t t = rows_total / rows_per_round;
    t = t < lo ? lo : (t > hi ? hi : t);
    const uint64_t blocks = (ih + t - 1) / t;
    return (uint32_t)(((ih + blocks - 1) / blocks + multiple - 1) / multiple * multiple);
}

namespace {

// One selection: the inputs, and the plan it fills in.
struct Selection {
    const PlanOptions &opt;
    const AxisTables &tx, &ty;
    const uint32_t iw, ih, ow, oh;
    KernelPlan p;

    Selection(const PlanOptions &o, const AxisTables &x, const AxisTables &y)
        : opt(o), tx(x), ty(y), iw(x.in_n), ih(y.in_n), ow(x.out_n), oh(y.out_n)
    {
    }

    // widest input-column footprint of a `segw`-column output segment (what one wave's LDS row / register columns must hold)
    uint32_t widest_footprint(uint32_t segw) const
    {
        uint32_t widest = 0;
        for (uint32_t x0 = 0; x0 < ow; x0 += segw) {
            const uint32_t xl = (x0 + segw < ow ? x0 + segw : ow) - 1;
            const uint32_t span = (uint32_t)(tx.lz_left[xl] + (int32_t)tx.lz_ntaps[xl] - tx.lz_left[x0]);
            if (span > widest) widest = span;
        }
        return widest;
    }

    // widest union of the tap windows of `n` adjacent outputs (a lane's outputs in the union-window H pass); ow % n == 0.  For two
    // outputs per lane a window is as long as the axis's widest one (7 for Lanczos-3 on an up-scale; the table's slots beyond a window's
    // taps hold zeros), so that their union fits the 8-tap pass; for four the table's 8 slots as before (counted tightly, x1.4 - x1.5 would
    // move from the plain 8-slot pass to the 10-tap union with its weights in LDS, which is slower there: 768p -> 1080p 6.1 -> 7.3 us)
    uint32_t widest_union(uint32_t n) const
    {
        uint32_t widest = 0;
        const uint32_t taps = n == 2 && tx.lz_max_taps > 0 && tx.lz_max_taps < 8 ? (uint32_t)tx.lz_max_taps : 8u;
        for (uint32_t x0 = 0; x0 < ow; x0 += n) {
            const uint32_t u = (uint32_t)(tx.lz_left[x0 + n - 1] - tx.lz_left[x0]) + taps;
            if (u > widest) widest = u;
        }
        return widest;
    }

    // Kernel for the resize filters (Lanczos-3 / Catmull-Rom / Triangle), most specialised first.
    void choose_resize_variant(bool x2)
    {
        p.variant = Variant::LanczosGeneral; // per-pixel fallback
        const bool addressable = (uint64_t)ow * oh * 4 < (1ull << 31); // buffer-resource addressing of the output frame
        // exact x2: fixed interior weights; same ratio on both axes, so the two passes share the same 12 numbers
        if (x2 && iw >= 16 && ih >= 16 && addressable && lanczos_x2_phase_frame(tx, p.wx6) && lanczos_x2_phase_frame(ty, p.wy6) &&
            lanczos_x2_interior_uniform(tx, p.wx6) && lanczos_x2_interior_uniform(ty, p.wy6) &&
            memcmp(&p.wx6[(size_t)8 * 6], &p.wy6[(size_t)8 * 6], 12 * sizeof(float)) == 0) {
            p.variant = Variant::LanczosX2RegWin;
            return;
        }
        // integer factors x3 / x4: the same register-window design (nus_k_lanczos_xs.hip).  x4: the interior weights are
        // uniform (one set per phase, the same numbers on both axes).  x3: they move with the binade of the coordinate
        // (nus_tables.hpp), so every lane / row takes the set of its class
        for (uint32_t S = 3; S <= 4 && !opt.force_general; ++S) {
            if (ow != S * iw || oh != S * ih || (iw % 4) != 0 || iw < 16 || ih < 16 || !addressable) continue;
            if (!lanczos_xs_phase_frame(tx, S, p.wx6) || !lanczos_xs_phase_frame(ty, S, p.wy6)) continue;
            if (lanczos_xs_interior_uniform(tx, S, p.wx6) && lanczos_xs_interior_uniform(ty, S, p.wy6) &&
                memcmp(&p.wx6[(size_t)8 * S * 6], &p.wy6[(size_t)8 * S * 6], (size_t)S * 6 * sizeof(float)) == 0) {
                p.xs_factor = S;
                p.variant = Variant::LanczosXsRegWin;
                return;
            }
            if (S == 3 && lanczos_xs_weight_classes(tx, S, p.wx6, true, p.xs_cls_x, p.xs_wcls_x) &&
                lanczos_xs_weight_classes(ty, S, p.wy6, false, p.xs_cls_y, p.xs_wcls_y)) {
                p.xs_factor = S;
                p.variant = Variant::LanczosXsRegWin;
                return;
            }
            clear_classes();
        }
        // x3/2 (720p -> 1080p, 1440p -> 4K): the same design with three output rows per input row pair (nus_k_lanczos_r32.hip);
        // weights by class of the input pair on both axes, as at x3
        if (!opt.force_general && 2 * (uint64_t)ow == 3 * (uint64_t)iw && 2 * (uint64_t)oh == 3 * (uint64_t)ih && (iw % 8) == 0 &&
            (ih % 2) == 0 && iw >= 32 && ih >= 16 && addressable && lanczos_r32_phase_frame(tx, p.wx6) &&
            lanczos_r32_phase_frame(ty, p.wy6) && lanczos_r32_weight_classes(tx, p.wx6, true, p.xs_cls_x, p.xs_wcls_x) &&
            lanczos_r32_weight_classes(ty, p.wy6, false, p.xs_cls_y, p.xs_wcls_y)) {
            p.variant = Variant::LanczosR32RegWin;
            return;
        }
        clear_classes();
        // x4/3 (1080p -> 1440p): four output rows per group of three input rows (nus_k_lanczos_r43.hip); the ratio 3/4 is exact in
        // f32, so the interior weights are uniform (one set per phase, the same numbers on both axes), as at x2 and x4
        if (!opt.force_general && 3 * (uint64_t)ow == 4 * (uint64_t)iw && 3 * (uint64_t)oh == 4 * (uint64_t)ih && (iw % 12) == 0 &&
            (ih % 3) == 0 && iw >= 48 && ih >= 18 && addressable && lanczos_r43_phase_frame(tx, p.wx6) &&
            lanczos_r43_phase_frame(ty, p.wy6) && lanczos_r43_interior_uniform(tx, p.wx6) && lanczos_r43_interior_uniform(ty, p.wy6) &&
            memcmp(&p.wx6[(size_t)8 * 6], &p.wy6[(size_t)8 * 6], 24 * sizeof(float)) == 0) {
            p.variant = Variant::LanczosR43RegWin;
            return;
        }
        // x5/4, x6/5, x5/3, x5/2: P output rows per group of Q input rows, every output's weights from the tables in frame form
        // (nus_k_lanczos_pq.hip); the ratios are not exact in f32, so nothing about the weights is assumed beyond their frames
        if (!opt.force_general && ow > iw && addressable && iw >= 32 && ih >= 12) {
            uint64_t a = ow, b = iw;
            while (b) {
                const uint64_t r = a % b;
                a = b, b = r;
            }
            const uint32_t P = (uint32_t)(ow / a), Q = (uint32_t)(iw / a);
            if (lanczos_pq_supported(P, Q) && (uint64_t)oh * Q == (uint64_t)ih * P && (iw % Q) == 0 && (ih % Q) == 0 && (ow % 4) == 0 &&
                lanczos_pq_phase_frame(tx, P, Q, p.wx6) && lanczos_pq_phase_frame(ty, P, Q, p.wy6)) {
                p.pq_p = P, p.pq_q = Q;
                // a filter of support 2 or less (Catmull-Rom, Triangle): slots 0 and 5 of every output's frame are zero on both axes, and
                // the kernel may sum slots 1 .. 4 only (checked on the tables themselves, border outputs included)
                auto edge_slots_zero = [](const std::vector<float> &w6) {
                    for (size_t o = 0; o + 6 <= w6.size(); o += 6)
                        if (w6[o] != 0.0f || w6[o + 5] != 0.0f) return false;
                    return true;
                };
                p.pq_narrow = edge_slots_zero(p.wx6) && edge_slots_zero(p.wy6);
            }
        }
        if (p.pq_p) {
            // The any-scale kernel's parameters as well: at x6/5, x8/5, x9/5 the kernel's EXACT instantiations hold 250 - 430 registers (one
            // wave per SIMD) and lose to it (1080p: 11.2 / 25.4 / 30.0 against 8.3 / 19.9 / 28.5 us; x7/5 wins, 11.6 against 17.4), so EXACT
            // mode -- which can be switched on after initialize() -- takes it there (HipUpscaler::enqueue)
            choose_general_resize_variant();
            p.pq_exact_fallback = p.variant == Variant::ResizeWin && p.pq_q == 5 && p.pq_p != 7;
            p.variant = Variant::LanczosPqRegWin;
            return;
        }
        choose_general_resize_variant();
    }

    // (a ratio's weight classes did not hold on both axes: the next candidate starts without them)
    void clear_classes() { p.xs_cls_x.clear(), p.xs_cls_y.clear(), p.xs_wcls_x.clear(), p.xs_wcls_y.clear(); }

    // ... and the kernels for every other shape: streamed down-scaling, the register-window / LDS-row any-scale kernels, per pixel
    void choose_general_resize_variant()
    {
        p.variant = Variant::LanczosGeneral;
        if (opt.force_per_pixel) return;
        // vertical down-scaling: stream the input rows through 7 accumulator slots, if the windows allow it and a
        // 64-column output segment's footprint fits 5 columns per lane
        if (ih > oh && tx.lz_max_taps <= 32 && !opt.force_rows) {
            const uint32_t widest64 = widest_footprint(64);
            if (build_down_stream_tables(ty, p.down_rows, p.down_done) && widest64 <= 320) {
                p.variant = Variant::ResizeDown;
                // Output columns per wave: every lane carries ceil(footprint / 64) input columns through the vertical pass whether
                // the segment fills them or not, so a slightly narrower segment whose footprint fits one column per lane fewer is
                // cheaper (2x down: 58 outputs over 128 columns instead of 64 over 140 = 3 columns per lane, a third of them idle).
                // Cost per output column ~ (vertical FMAs of a lane per output row + its horizontal pass: an LDS read and 4 FMAs per
                // tap of the compiled trip count, priced at 10) / width, calibrated on profiles/r03_resize_down_segment_width_ab.txt
                // (4K -> 1080p: 58 columns 16.9 us against 20.1 at 64; 4K -> 720p, 32-tap passes: 64 stays, 57 is 4 % slower).
                p.down_seg_w = 64;
                p.ncols_max = widest64;
                if (opt.down_seg_width == 0) {
                    const double rows_per_out = (double)ih / oh;
                    double best = 0.0;
                    for (uint32_t w = 64; w >= 40; --w) {
                        const uint32_t fp = widest_footprint(w);
                        const double cost = (28.0 * ((fp + 63) / 64) * rows_per_out + 10.0 * (tx.lz_max_taps > 16 ? 32 : 16) + 30.0) / w;
                        if (w == 64 || cost < best * 0.97) best = cost, p.down_seg_w = w, p.ncols_max = fp;
                    }
                } else { // option "down_seg_width" (tests, A/B timing)
                    p.down_seg_w = opt.down_seg_width > 64 ? 64 : opt.down_seg_width;
                    p.ncols_max = widest_footprint(p.down_seg_w);
                    if (p.ncols_max > 320) p.down_seg_w = 64, p.ncols_max = widest64;
                }
                return;
            }
        }
        // LDS row kernel: the widest segment footprint must fit the per-wave LDS row (4 waves x 640 x 16 B = 40 KiB per block)
        const uint32_t widest = widest_footprint((ow % 4) == 0 ? 256 : 64);
        if (widest > 640) return;
        p.variant = Variant::ResizeRows;
        p.ncols_max = widest;
        p.small_taps = tx.lz_max_taps <= 8 && ty.lz_max_taps <= 8;
        if ((ow % 4) != 0 || !p.small_taps) return;
        p.union_taps = widest_union(4); // union-window H pass, 4 outputs per lane
        // register-window variant: up-scaling shapes whose first tap row moves by at most one per output row
        bool win_ok = ty.lz_max_taps <= 7 && !opt.force_rows;
        for (uint32_t y = 1; win_ok && y < oh; ++y) {
            const int32_t d = ty.lz_left[y] - ty.lz_left[y - 1];
            win_ok = d == 0 || d == 1;
        }
        if (!win_ok) return;
        // Four outputs per lane (segments of 256 output columns) from x2 up.  Below x2 two outputs per lane win wherever their 8-tap union
        // pass applies (two input columns per lane, union weights in registers, rows through the ring -- the four-output shape there needs
        // three columns per lane and keeps its union weights in LDS): 768p -> 1080p 7.2 -> 6.5, x1.7 18.6 -> 15.8, x1.9 21.2 -> 19.0 us per
        // frame; from x2.2 up the four-output shape is the faster one again (profiles/r05_resize_win_rotating_window.txt)
        const bool two_per_lane = 2 * (uint64_t)iw > ow && widest_footprint(128) <= 128 && widest_union(2) <= 8;
        if (widest <= 192 && !two_per_lane) {
            p.variant = Variant::ResizeWin;
            return;
        }
        // factors x1.0 .. x2: two outputs per lane, segments of 128 output columns
        const uint32_t widest2 = widest_footprint(128);
        if (widest2 > 192) return;
        p.variant = Variant::ResizeWin;
        p.win_outputs_per_lane = 2;
        p.ncols_max = widest2;
        p.union_taps = widest_union(2);
    }

    // One of the small rational factors P/Q the fixed-ratio nearest / bilinear kernels are built for, with tables of exactly the
    // shape they assume on both axes: source index Q (o / P) + (o % P) Q / P and, for bilinear, fraction 0 where the phase lands
    // on a pixel ((o % P) Q % P == 0).
    bool ratio_shape(bool bilinear) const
    {
        static const uint32_t kRatios[][2] = {{3, 2}, {4, 3}, {3, 1}, {4, 1}, {2, 1}, {5, 4}, {6, 5}, {5, 3}, {5, 2}, {7, 2}, {7, 5}};
        for (const auto &r : kRatios) { // (x8/5: the table kernel is the faster one for nearest too, 5.6 against 5.8 us at 1080p)
            const uint32_t P = r[0], Q = r[1];
            if ((uint64_t)ow * Q != (uint64_t)iw * P || (uint64_t)oh * Q != (uint64_t)ih * P || iw % Q != 0 || ih % Q != 0) continue;
            // bilinear at x5/2 and x7/2: five / seven lerped outputs from two input columns per lane leave the fixed-ratio kernel behind the
            // table kernel (864p -> 4K: 11.7 against 10.6 us per frame, profiles/r05_nearest_bilinear_pq_ratios.txt); nearest gains at every factor
            if (bilinear && Q == 2 && P >= 5) return false;
            if (bilinear && Q == 5 && P >= 7) return false; // (nearest only: Q + 1 lerped rows of 4 P values do not fit the registers)
            bool ok = true;
            for (const AxisTables *t : {&tx, &ty})
                for (uint32_t o = 0; ok && o < t->out_n; ++o) {
                    const uint32_t want = Q * (o / P) + (o % P) * Q / P;
                    ok = bilinear ? (t->bl_i0[o] == want && (((o % P) * Q) % P != 0 || t->bl_frac[o] == 0.0f)) : t->nn_src[o] == want;
                }
            return ok;
        }
        return false;
    }

    void choose_variant(Algorithm algorithm)
    {
        const bool x2 = ow == 2 * iw && oh == 2 * ih && (iw % 4) == 0 && !opt.force_general;
        switch (algorithm) {
        case Algorithm::Nearest:
            p.variant = x2 ? Variant::NearestX2 : Variant::NearestTable;
            if (!x2 && !opt.force_general && ratio_shape(false)) p.variant = Variant::NearestRatio;
            break;
        case Algorithm::Bilinear: {
            // The packed-integer x2 kernel is valid iff the CPU-form tables are exactly
            // i0 = o>>1, frac = 0 / 0.5 (and frac 0 at the clamped last sample).
            bool ok = x2 && !opt.wgsl_bilinear;
            for (const AxisTables *t : {&tx, &ty}) {
                for (uint32_t o = 0; ok && o < t->out_n; ++o) {
                    const bool last_odd = (o & 1) && (o >> 1) == t->in_n - 1;
                    const float want = (o & 1) && !last_odd ? 0.5f : 0.0f;
                    ok = t->bl_i0[o] == (o >> 1) && t->bl_frac[o] == want;
                }
            }
            p.variant = ok ? Variant::BilinearX2Int : Variant::BilinearTable;
            if (!ok && !opt.wgsl_bilinear && !opt.force_general && ratio_shape(true)) p.variant = Variant::BilinearRatio;
            break;
        }
        case Algorithm::Lanczos3:
        case Algorithm::Bicubic:
        case Algorithm::Triangle: choose_resize_variant(x2); break;
        case Algorithm::Fsr1:
            // two kernels with the EASU image in HBM between them beat the fused LDS tile on real frames (1080p -> 4K: EASU 65.5 + RCAS rows
            // 21.7 against 98.2 us fused; FAST 43.0 + 21.7 against 80.2): the tile's phases add up, the two launches overlap their own
            p.variant = opt.fsr_two_pass && (size_t)ow * oh * 4 >= ((size_t)1 << 20) ? Variant::Fsr1TwoPass : Variant::Fsr1Fused;
            break;
        case Algorithm::FsrEasu: p.variant = Variant::FsrEasu; break;
        case Algorithm::FsrRcas: p.variant = Variant::FsrRcas; break;
        }
    }
};

} // namespace

KernelPlan plan_kernels(Algorithm algorithm, const PlanOptions &opt, const AxisTables &tx, const AxisTables &ty)
{
    Selection s(opt, tx, ty);
    s.choose_variant(algorithm);
    return std::move(s.p);
}

} // namespace nus
