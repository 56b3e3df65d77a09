// Host-only driver for the sanitizer build (tests/test_host_logic.py): every argument check the host entry points share
// (nus_checks.cpp) swept over its boundary values, each answer compared with the rule written out here.  A wrong status -- or a
// failure without an error text that names the caller -- counts as bad and the program exits non-zero.
#include "nus_checks.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>

using namespace nus;

static int bad = 0, checks = 0;

// `got` is the status `want_ok ? kOk : fail_status`; a failure leaves a text that starts with `prefix`, a success leaves the text alone
static void expect(const char *what, int got, bool want_ok, int fail_status, const char *prefix)
{
    ++checks;
    const int want = want_ok ? kOk : fail_status;
    const bool text_ok = want_ok ? strcmp(thread_error(), "untouched") == 0 : strncmp(thread_error(), prefix, strlen(prefix)) == 0;
    if (got != want || !text_ok) {
        ++bad;
        printf("BAD %s: status %d (want %d), text \"%s\"\n", what, got, want, thread_error());
    }
    set_thread_error("untouched");
}

int main()
{
    const char *who = "caller";
    set_thread_error("untouched");
    alignas(16) static unsigned char mem[64];
    const uint32_t w = 16, h = 12;
    const size_t frame = (size_t)w * h * 4;

    // pointers: null (the callers refuse null before these checks: it counts as aligned here), aligned, off by 1 / 2 / 3
    const void *ptrs[] = {nullptr, mem, mem + 1, mem + 2, mem + 3, mem + 4};
    const size_t strides[] = {0, frame - 4, frame, frame + 2, frame + 4};
    for (const void *a : ptrs)
        for (const void *b : ptrs)
            for (size_t sa : strides)
                for (size_t sb : strides) {
                    const bool al = !misaligned(a, 4) && !misaligned(b, 4) && sa % 4 == 0 && sb % 4 == 0;
                    expect("check_pairs", check_pairs(who, a, sa, b, sb, w, h), al && sa >= frame && sb >= frame, kInvalidArgument, "caller: ");
                    for (const void *out : ptrs)
                        for (uintptr_t fa : {(uintptr_t)4, (uintptr_t)8}) {
                            const void *flows[] = {nullptr, mem, mem + 4, mem + 8, mem + 2};
                            for (const void *fl : flows) {
                                const bool ok = al && !misaligned(out, 4) && (reinterpret_cast<uintptr_t>(fl) % fa) == 0;
                                expect("check_pixel_aligned", check_pixel_aligned(who, a, sa, b, sb, out, fl, fa), ok, kInvalidArgument, "caller: ");
                            }
                        }
                }
    for (const void *also : ptrs)
        expect("check_pixel_aligned(also)", check_pixel_aligned(who, mem, frame, mem, frame, mem, nullptr, 8, also),
               reinterpret_cast<uintptr_t>(also) % 4 == 0, kInvalidArgument, "caller: ");

    // host frame lengths
    for (size_t la : {(size_t)0, frame - 1, frame, frame + 1})
        for (size_t lb : {(size_t)0, frame - 1, frame, frame + 1})
            expect("check_frame_lengths", check_frame_lengths(la, lb, w, h), la == frame && lb == frame, kSizeMismatch, "Expected 768 bytes");

    // times
    const float vals[] = {NAN, -0.1f, 0.0f, 1.0f, 1.5f};
    expect("check_interp_times(null)", check_interp_times(who, nullptr, 1), false, kInvalidArgument, "caller: times is null");
    for (uint32_t n : {0u, 1u, 7u, 8u})
        for (uint32_t pos = 0; pos < (n ? n : 1); ++pos)
            for (float v : vals) {
                float times[8] = {0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f};
                times[pos] = v;
                const bool ok = n >= 1 && n <= 7 && v >= 0.0f && v <= 1.0f;
                expect("check_interp_times", check_interp_times(who, times, n), ok, kInvalidArgument, "caller: ");
            }

    // dimensions: 0, 1 and each caller's limit +- 1 (metrics and scene: at most 2^30 pixels; the interpolators and the block
    // matcher: fewer than 2^31; the flow estimator: fewer than 2^28)
    const uint64_t limits[] = {(uint64_t)1 << 30, ((uint64_t)1 << 31) - 1, ((uint64_t)1 << 28) - 1};
    for (uint64_t lim : limits)
        for (uint64_t px : {(uint64_t)0, (uint64_t)1, lim - 1, lim, lim + 1}) {
            // px pixels as a px x 1 and a 1 x px frame
            const uint32_t dw = (uint32_t)px, dh = 1;
            expect("check_dims", check_dims(who, dw, dh, lim), px >= 1 && px <= lim, kInvalidArgument, "caller: bad dimensions");
            expect("check_dims(h, w)", check_dims(who, dh, dw, lim, "bad image dimensions"), px >= 1 && px <= lim, kInvalidArgument,
                   "caller: bad image dimensions");
            expect("check_frame_area", check_frame_area(who, dw, dh, lim), px <= lim, kInvalidArgument, "caller: ");
        }
    expect("check_dims(65536 x 65536)", check_dims(who, 65536, 65536, ((uint64_t)1 << 31) - 1), false, kInvalidArgument, "caller: ");
    expect("check_frame_area(32768 x 32768)", check_frame_area(who, 32768, 32768, (uint64_t)1 << 30), true, kInvalidArgument, "caller: ");
    expect("check_frame_area(32768 x 32769)", check_frame_area(who, 32768, 32769, (uint64_t)1 << 30), false, kInvalidArgument, "caller: ");

    // out_pair_stride
    for (uint32_t n : {1u, 3u, 7u})
        for (size_t s : {(size_t)0, n * frame - 4, n * frame, n * frame + 2, n * frame + 4})
            expect("check_out_pair_stride", check_out_pair_stride(who, s, n, frame), s == 0 || (s >= n * frame && s % 4 == 0), kInvalidArgument,
                   "caller: out_pair_stride");

    // workspace
    for (size_t need : {(size_t)0, (size_t)1, (size_t)4096})
        for (size_t have : {(size_t)0, need ? need - 1 : 0, need, need + 1})
            expect("check_workspace", check_workspace(who, have, need, "nus_x_workspace_size"), have >= need, kInvalidArgument,
                   "caller: workspace of ");
    if (check_workspace(who, 1, 2, "nus_x_workspace_size") != kInvalidArgument ||
        strcmp(thread_error(), "caller: workspace of 1 bytes, 2 needed (nus_x_workspace_size)") != 0)
        ++bad;

    // fail() and a text longer than fmt's buffer
    expect("fail", fail(kNoDevice, "caller: x"), false, kNoDevice, "caller: x");
    const std::string big(2000, 'x');
    if (fmt("%s", big.c_str()).size() != 511) ++bad;

    printf("checks %d bad %d\n", checks, bad);
    return bad ? 1 : 0;
}
