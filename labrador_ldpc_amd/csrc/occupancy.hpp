// occupancy.hpp -- how many workgroups of a kernel the current device holds at once, for the persistent launchers
// (decode_ms_launch.hpp, decode_ms_layered_launch.hpp, decode_ms_bs.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <atomic>

namespace ldpc {

// Resident workgroups of KERNEL at BLOCK threads per workgroup: occupancy x compute units, cached per device (one cache per
// instantiation).  A failed occupancy query counts one workgroup per CU, a failed CU count 256 CUs.
template <auto KERNEL, int BLOCK>
int resident_workgroups()
{
    static std::atomic<int> cached[64] = {};     // concurrent callers may both fill an entry: they store the same value
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    int v = cached[dev].load(std::memory_order_relaxed);
    if (v == 0) {
        int per_cu = 0, cus = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, KERNEL, BLOCK, 0) != hipSuccess || per_cu < 1) per_cu = 1;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
        v = per_cu * cus;
        cached[dev].store(v, std::memory_order_relaxed);
    }
    return v;
}

}  // namespace ldpc
