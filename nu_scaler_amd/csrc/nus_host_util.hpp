// nus_host_util.hpp -- small helpers shared by the host classes (nus_host.cpp, nus_host_interp.cpp).  Internal.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <string>

#include "nus_kernels.hpp"
#include "nus_ranges.hpp"

namespace nus {

namespace {

std::string fmt(const char *f, ...) __attribute__((format(printf, 1, 2)));
std::string fmt(const char *f, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}

// The time set of the multi-time interpolation entry points: 1 .. kInterpMaxTimes times, each in [0, 1] (NaN is not).  Returns
// what is wrong with it, empty when nothing is.
std::string check_interp_times(const float *times, uint32_t n_times)
{
    if (!times) return "times is null";
    if (n_times == 0 || n_times > kInterpMaxTimes) return fmt("n_times must be 1..%u, got %u", kInterpMaxTimes, n_times);
    for (uint32_t k = 0; k < n_times; ++k)
        if (!(times[k] >= 0.0f && times[k] <= 1.0f)) return fmt("times[%u] = %g is not in [0, 1]", k, (double)times[k]);
    return std::string();
}

// True when `p` is host memory the DMA engines can address directly
// (hipHostMalloc / hipHostRegister); pageable memory goes through pinned staging.
bool is_pinned_host(const void *p)
{
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError(); // pageable memory: not an error for us
        return false;
    }
    return attr.type == hipMemoryTypeHost;
}

// hipHostMalloc / hipHostFree that keep the library's record of its own pinned memory (nus_ranges.hpp)
hipError_t pinned_alloc(void **p, size_t bytes)
{
    const hipError_t e = hipHostMalloc(p, bytes, hipHostMallocDefault);
    if (e == hipSuccess) range_note(kRangeHostAlloc, *p, bytes);
    return e;
}

void pinned_free(void *p)
{
    if (!p) return;
    range_forget(kRangeHostAlloc, p);
    (void)hipHostFree(p);
}

int device_count()
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

} // namespace

} // namespace nus

// inside a member function of a class with fail_hip(): propagate a HIP error as a status code
#define NUS_HIP(call)                                     \
    do {                                                  \
        hipError_t e_ = (call);                           \
        if (e_ != hipSuccess) return fail_hip(e_, #call); \
    } while (0)
