// nus_retime.hpp -- frame-rate conversion by a rational ratio num / den = out_rate / in_rate (nus_retime_* and the *_retime_*
// entry points of include/nuscaler_hip.h, where the contract is written).  BUILD-DEFINED: the reference has no rate conversion.
//
// The schedule, in 64-bit integers, for n_frames >= 2 input frames and the REDUCED ratio:
//     n_out = ((n_frames - 1) num) / den + 1;   output j:  k_j = (j den) / num,  r_j = (j den) % num,  t_j = RN_f32(r_j / num)
// r_j == 0: output j is real frame k_j; else the in-between frame of pair (k_j, k_j + 1) at t_j.  Seen from pair k: its outputs are
// j = first .. first + count - 1 with first = ceil(k num / den), first + count = ceil((k + 1) num / den), and their remainders
// rem0, rem0 + den, .. (rem0 = first den - k num, every one below num).  retime_pair is that statement: the one function the
// kernels (nus_k_retime.hip) and the host table (nus_retime.cpp) both call.  No HIP here beyond the function attributes.
#pragma once

#include <cstddef>
#include <cstdint>

#include "nus_checks.hpp"

#if defined(__HIPCC__)
#define NUS_RETIME_FN __host__ __device__ inline
#else
#define NUS_RETIME_FN inline
#endif

namespace nus {

constexpr uint32_t kRetimeMaxTerm = 4096; // NUS_RETIME_MAX_TERM
constexpr uint32_t kRetimeMaxRatio = kMaxInterpTimes + 1;

struct RetimePair {
    uint64_t first; // index of the pair's first output
    uint32_t count; // outputs of the pair: 0 .. ceil(num / den)
    uint32_t rem0;  // remainder of the first; output first + i has rem0 + i * den
};

// wave-uniform integer code: pair < 2^32, num and den <= 4096, so every product is below 2^45
NUS_RETIME_FN RetimePair retime_pair(uint64_t pair, uint32_t num, uint32_t den)
{
    const uint64_t at = pair * num, first = (at + den - 1) / den, next = (at + num + den - 1) / den;
    return RetimePair{first, (uint32_t)(next - first), (uint32_t)(first * den - at)};
}

// t of a remainder: one correctly rounded f32 division of two integers that f32 holds exactly
NUS_RETIME_FN float retime_time(uint32_t rem, uint32_t num)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn((float)rem, (float)num);
#else
    return (float)rem / (float)num; // IEEE on the host (the units are built with -ffp-contract=off and without fast-math)
#endif
}

struct RetimeEntry { // nus_retime_entry
    uint32_t pair, rem;
    float t;
    uint32_t reserved;
};

struct RetimeRatio {
    uint32_t num = 0, den = 0; // reduced
};

// The checks every retime entry point makes before any HIP call; `who` is the C entry point the text names.  kOk and `r` set, or
// kInvalidArgument: a zero term, a term above kRetimeMaxTerm, a reduced ratio above kRetimeMaxRatio, n_frames < 2.
int check_retime(const char *who, uint64_t n_frames, uint32_t num, uint32_t den, RetimeRatio &r);
// 0 (tightly packed) or a multiple of 4 of at least one frame
int check_out_frame_stride(const char *who, size_t out_frame_stride, size_t frame_bytes);

inline uint64_t retime_count(uint64_t n_frames, const RetimeRatio &r) { return ((n_frames - 1) * r.num) / r.den + 1; }
inline RetimeEntry retime_entry(uint64_t j, const RetimeRatio &r)
{
    const uint64_t at = j * r.den;
    const uint32_t rem = (uint32_t)(at % r.num);
    return RetimeEntry{(uint32_t)(at / r.num), rem, retime_time(rem, r.num), 0};
}

// nus_retime_count / nus_retime_schedule / nus_retime_schedule_device
int64_t retime_count_checked(uint64_t n_frames, uint32_t num, uint32_t den);
int retime_schedule(uint64_t n_frames, uint32_t num, uint32_t den, uint64_t first, uint64_t count, RetimeEntry *out);
int retime_schedule_device(uint32_t n_frames, uint32_t num, uint32_t den, void *d_entries, void *stream /* hipStream_t */);
// nus_scene_apply_cuts_retime_device
int scene_apply_cuts_retime_device(const void *d_frames, size_t frame_stride, uint32_t n_frames, uint32_t w, uint32_t h, int format,
                                   uint32_t num, uint32_t den, const uint8_t *d_cut, void *d_out, size_t out_frame_stride,
                                   void *stream /* hipStream_t */);

} // namespace nus
