// nus_plan.hpp -- which kernel an upscaler handle runs, as a value: plan_kernels() is a pure function of the algorithm, a handful
// of options and the two axes' tables (the dimensions are theirs).  No HIP here: the unit builds with a plain C++ compiler next to
// nus_tables.cpp, so the decision is tested on the CPU (tests/c_abi/kernel_plan_dump.cpp).
#pragma once

#include <cstdint>
#include <vector>

#include "nus_tables.hpp"

namespace nus {

enum class Algorithm : int { Nearest = 0, Bilinear = 1, Lanczos3 = 2, Bicubic = 3, Triangle = 4, Fsr1 = 5, FsrEasu = 6, FsrRcas = 7 };

// Kernel variants (chosen once at initialize).
enum class Variant : int {
    NearestTable = 0, // any scale, index tables
    NearestX2,        // exact x2, 16-B loads/stores
    NearestRatio,     // exact x3/2, x4/3, x3, x4: an input group per lane copied into P outputs, a row group into P rows
    BilinearTable,    // any scale, f32, CPU or WGSL arithmetic
    BilinearX2Int,    // exact x2, CPU arithmetic done in packed-u8 integer ops
    BilinearRatio,    // exact x3/2, x4/3, x3, x4, CPU form: one input group per lane, P outputs, row groups
    LanczosGeneral,   // any scale, direct separable evaluation per output pixel (fallback)
    ResizeRows,       // any scale, separable: V pass into an LDS row, H pass out of it
    ResizeWin,        // up-scaling: V pass from a register row window (as the x2 kernel), H pass through the LDS row
    ResizeDown,       // down-scaling: input rows streamed once into the vertical sums of the 7 output rows in flight
    LanczosX2RegWin,  // exact x2, register sliding window + wave shifts
    LanczosXsRegWin,  // exact x3 / x4, same design with S output rows per input row
    LanczosR32RegWin, // exact x3/2, same design: three output rows per pair of input rows
    LanczosR43RegWin, // exact x4/3, same design: four output rows per group of three input rows
    LanczosPqRegWin,  // x5/4, x6/5, x5/3, x5/2, same design: P output rows per group of Q input rows, weights from the tables
    FsrEasu,          // FSR1-style EASU alone (any scale)
    FsrRcas,          // FSR1-style RCAS alone (same size in and out)
    Fsr1Fused,        // EASU tile (+1 px halo) in LDS, RCAS out of it
    Fsr1TwoPass,      // EASU into a scratch image in HBM, the row-walking RCAS out of it (frames of >= 1 MiB: faster than the fused tile)
};

const char *variant_name(Variant v);

// the factors P/Q the P/Q register-window resize kernel is instantiated for (nus_k_lanczos_pq.hip)
bool lanczos_pq_supported(uint32_t P, uint32_t Q);

// What the caller may ask of the selection (HipUpscaler::set_option / set_bilinear_variant; all before initialize()).
struct PlanOptions {
    bool force_general = false;
    bool force_per_pixel = false; // resize: never use the LDS row kernel
    bool force_rows = false;      // resize: never use the register-window variant of it
    bool wgsl_bilinear = false;
    bool fsr_two_pass = true;     // option "fsr_two_pass": 0 keeps the fused LDS tile at every size
    uint32_t down_seg_width = 0;  // option "down_seg_width": 0 = chosen by cost
};

// Everything the selection produces.  Default-constructed: nothing chosen yet.
struct KernelPlan {
    Variant variant = Variant::NearestTable;
    uint32_t xs_factor = 0;         // 3 / 4 when the integer-factor register-window kernel is selected
    uint32_t pq_p = 0, pq_q = 0;    // Variant::LanczosPqRegWin: the factor P / Q
    bool pq_narrow = false;         // ... and whether every output's frame slots 0 and 5 are zero (a support-2 filter: 4-tap sums)
    bool pq_exact_fallback = false; // ... and whether its EXACT mode runs on the any-scale kernel instead (Q = 5)
    uint32_t ncols_max = 0;         // LDS row length of the ResizeRows variant
    uint32_t union_taps = 0;        // widest union of the tap windows of 4 adjacent outputs (0: unused)
    bool small_taps = false;
    uint32_t win_outputs_per_lane = 4; // register-window resize: 4, or 2 for factors below ~x1.4
    uint32_t down_seg_w = 64;          // ResizeDown: output columns per wave
    std::vector<uint32_t> down_rows;   // ResizeDown: per-input-row slot weights + completion (build_down_stream_tables)
    std::vector<int32_t> down_done;
    std::vector<float> wx6, wy6;             // the fixed-ratio kernels' weights in frame form
    std::vector<uint32_t> xs_cls_x, xs_cls_y; // x3: weight class per input index, and the classes' weights
    std::vector<float> xs_wcls_x, xs_wcls_y;
};

// A fresh plan on every call: nothing of an earlier selection survives into it.
KernelPlan plan_kernels(Algorithm algorithm, const PlanOptions &opt, const AxisTables &tx, const AxisTables &ty);

// Rows per wave of the fixed-ratio register-window kernels on a batch: ih rows x strips x n_frames make rows_per_round rows per wave
// and round of the chip, clamped to lo .. hi; the frame is then cut into row blocks of equal height, rounded up to a multiple of
// `multiple` (the rows of a group at x3/2, x4/3 and P/Q; 1: as it comes).
uint32_t equal_row_blocks(uint32_t ih, uint32_t strips, uint32_t n_frames, uint32_t rows_per_round, uint32_t lo, uint32_t hi,
                          uint32_t multiple);

} // namespace nus
