// nus_host_util.cpp -- see nus_host_util.hpp.
#include "nus_host_util.hpp"

namespace nus {

bool is_pinned_host(const void *p)
{
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError(); // pageable memory: not an error for us
        return false;
    }
    return attr.type == hipMemoryTypeHost;
}

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

int fail_hip(hipError_t e, const char *what)
{
    (void)hipGetLastError();
    return fail(e == hipErrorOutOfMemory ? kOutOfMemory : kHipError, fmt("HIP error in %s: %s", what, hipGetErrorString(e)));
}

int check_device(const char *who, int device)
{
    const int n = device_count();
    if (n <= 0) return fail(kNoDevice, fmt("%s: no HIP device available", who));
    if (device < 0 || device >= n || device >= kMaxDevices) return fail(kNoDevice, fmt("%s: no HIP device %d", who, device));
    return kOk;
}

int HostErrors::fail(int status, const std::string &msg)
{
    error_ = msg;
    return nus::fail(status, msg);
}

int HostErrors::fail_hip(hipError_t e, const char *what) { return pass(nus::fail_hip(e, what)); }

int HostErrors::pass(int rc)
{
    if (rc != kOk) error_ = thread_error();
    return rc;
}

int HostErrors::select_device(int device)
{
    const int n = device_count();
    if (n <= 0) return fail(kNoDevice, "no HIP device available (the gfx950 path has no CPU fallback)");
    if (device >= n) return fail(kNoDevice, fmt("HIP device %d requested but only %d present", device, n));
    NUS_HIP(hipSetDevice(device));
    return kOk;
}

int DeviceBuffer::reserve(size_t bytes, hipStream_t sync_before_free)
{
    if (bytes <= cap_) return kOk;
    if (p_) {
        if (sync_before_free) NUS_HIP(hipStreamSynchronize(sync_before_free));
        release();
    }
    NUS_HIP(hipMalloc(&p_, bytes));
    cap_ = bytes;
    return kOk;
}

void DeviceBuffer::release()
{
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
    cap_ = 0;
}

int PairScratch::prepare(int device, size_t frame_bytes, size_t workspace_bytes, size_t result_bytes)
{
    NUS_HIP(hipSetDevice(device));
    if (!stream) NUS_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    int rc;
    if ((rc = a.reserve(frame_bytes)) != kOk || (rc = b.reserve(frame_bytes)) != kOk || (rc = workspace.reserve(workspace_bytes)) != kOk)
        return rc;
    return result.reserve(result_bytes);
}

} // namespace nus
