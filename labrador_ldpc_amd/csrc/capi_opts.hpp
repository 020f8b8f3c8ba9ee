// capi_opts.hpp -- part of capi.hip (its one translation unit): the error channel, the opts ABI shim and device selection.
#pragma once

namespace {

thread_local std::string g_err;

int fail(int status, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return status;
}

// struct labrador_ldpc_hip_opts as the CALLER laid it out -> this build's layout: a field is read only if it lies inside the
// first struct_size bytes (0 = this header's layout up to `devices`), everything beyond is zero (include/labrador_ldpc_hip.h).
// Returns nullptr for a NULL opts, else `local`.
const labrador_ldpc_hip_opts *normalise_opts(const labrador_ldpc_hip_opts *opts, labrador_ldpc_hip_opts &local)
{
    if (!opts) return nullptr;
    local = labrador_ldpc_hip_opts{};
    // struct_size == 0 is the header's promise for clients written `= {0}`: "ABI 3's layout up to and including `devices`" --
    // a FROZEN 40 bytes, not this build's sizeof: once a field is appended, sizeof would read past what such a client allocated
    // (the ABI-2 padding-as-field bug again; round 3 advice).
    constexpr size_t ABI3_BASE_SIZE = 40;
    static_assert(offsetof(labrador_ldpc_hip_opts, devices) + sizeof(const int *) == ABI3_BASE_SIZE && sizeof(labrador_ldpc_hip_opts) >= ABI3_BASE_SIZE,
                  "the layout up to `devices` is frozen: append new fields behind it");
    size_t have = opts->struct_size ? opts->struct_size : ABI3_BASE_SIZE;
    if (have > sizeof(labrador_ldpc_hip_opts)) have = sizeof(labrador_ldpc_hip_opts);      // a newer client: fields this build does not know
    if (have < offsetof(labrador_ldpc_hip_opts, device)) have = offsetof(labrador_ldpc_hip_opts, device);
    std::memcpy(&local, opts, have);
    local.struct_size = sizeof(labrador_ldpc_hip_opts);
    return &local;
}

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(LABRADOR_LDPC_HIP_ERUNTIME, "%s: %s", #expr, hipGetErrorString(e_));       \
    } while (0)

bool device_is_gfx950(int dev)
{
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return false;
    return std::strncmp(prop.gcnArchName, "gfx950", 6) == 0;
}

// how many HIP devices there are -> *count; none (or no usable runtime) is ENODEV
int device_count_or_fail(int *count)
{
    *count = 0;
    if (hipGetDeviceCount(count) != hipSuccess || *count <= 0) {
        (void)hipGetLastError();
        return fail(LABRADOR_LDPC_HIP_ENODEV, "no HIP device available (decode_ms has no CPU path)");
    }
    return LABRADOR_LDPC_HIP_OK;
}

// Select the device the call should run on; returns a status and the previous device so the
// caller's context is left as found.
struct DeviceScope {
    int prev = -1;
    bool switched = false;
    int enter(const labrador_ldpc_hip_opts *opts)
    {
        int count = 0;
        if (int s = device_count_or_fail(&count)) return s;
        if (hipGetDevice(&prev) != hipSuccess) return fail(LABRADOR_LDPC_HIP_ERUNTIME, "hipGetDevice failed");
        int want = (opts && opts->device >= 0) ? opts->device : prev;
        if (want >= count) return fail(LABRADOR_LDPC_HIP_EINVAL, "device %d out of range (%d devices)", want, count);
        if (!device_is_gfx950(want))
            return fail(LABRADOR_LDPC_HIP_ENODEV, "device %d is not gfx950; this library carries gfx950 code only", want);
        if (want != prev) {
            if (hipSetDevice(want) != hipSuccess) return fail(LABRADOR_LDPC_HIP_ERUNTIME, "hipSetDevice(%d) failed", want);
            switched = true;
        }
        return LABRADOR_LDPC_HIP_OK;
    }
    ~DeviceScope() { if (switched) (void)hipSetDevice(prev); }
};

}  // namespace
