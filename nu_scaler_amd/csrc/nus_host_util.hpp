// nus_host_util.hpp -- what the host modules share above the HIP runtime: error reporting, device selection, pinned memory and
// grow-only device buffers.  (The argument checks, which need no HIP, are in nus_checks.hpp.)  Internal.
#pragma once

#include <hip/hip_runtime.h>

#include <mutex>
#include <string>

#include "nus_checks.hpp"
#include "nus_kernels.hpp"
#include "nus_ranges.hpp"

namespace nus {

static_assert(kMaxInterpTimes == kInterpMaxTimes, "nus_checks.hpp and nus_kernels.hpp disagree about the multi-time limit");

// True when `p` is host memory the DMA engines can address directly
// (hipHostMalloc / hipHostRegister); pageable memory goes through pinned staging.
bool is_pinned_host(const void *p);

// hipHostMalloc / hipHostFree that keep the library's record of its own pinned memory (nus_ranges.hpp)
hipError_t pinned_alloc(void **p, size_t bytes);
void pinned_free(void *p);

int device_count(); // 0 when the runtime cannot say

// a HIP error as a status, its text in the thread's error ("HIP error in <what>: ...")
int fail_hip(hipError_t e, const char *what);

// "<who>: no HIP device available" / "<who>: no HIP device <device>" unless `device` is one this process can index
int check_device(const char *who, int device);

// Error state of a handle: the text last_error() returns, next to the calling thread's.  The host classes derive from it.
class HostErrors {
public:
    const char *last_error() const { return error_.c_str(); }

protected:
    int fail(int status, const std::string &msg);
    int fail_hip(hipError_t e, const char *what);
    // the status of a call that reports through the thread's error text only (the checks, upload / download, DeviceBuffer)
    int pass(int rc);
    // the handle's device made current; kNoDevice when there is none, or not that one
    int select_device(int device);

    std::string error_;
};

// Device memory that is kept for reuse and only grows.  No destructor: the per-device instances are never destroyed (the runtime
// may be gone before a static destructor runs); an owner with a lifetime calls release().
class DeviceBuffer {
public:
    DeviceBuffer() = default;
    DeviceBuffer(const DeviceBuffer &) = delete;
    DeviceBuffer &operator=(const DeviceBuffer &) = delete;

    // at least `bytes`; growing frees the old memory first, after work queued on `sync_before_free` (if given) has finished
    int reserve(size_t bytes, hipStream_t sync_before_free = nullptr);
    void *get() const { return p_; }
    size_t capacity() const { return cap_; }
    void release();

private:
    void *p_ = nullptr;
    size_t cap_ = 0;
};

// What a host entry point that compares two frames keeps per device: a stream, the pair, a workspace and a small result.
struct PairScratch {
    std::mutex m;
    hipStream_t stream = nullptr;
    DeviceBuffer a, b, workspace, result;

    // (m held, check_device passed)  the device current, the stream created, the buffers large enough
    int prepare(int device, size_t frame_bytes, size_t workspace_bytes, size_t result_bytes);
};

} // namespace nus

// where fail_hip() is in scope (a HostErrors member function, or the free one): propagate a HIP error as a status code
#define NUS_HIP(call)                                     \
    do {                                                  \
        hipError_t e_ = (call);                           \
        if (e_ != hipSuccess) return fail_hip(e_, #call); \
    } while (0)
