// decode_ms_layered_launch.hpp -- the host side that the layered launchers share (decode_ms_layered_f32.hip, decode_ms_corrected_f32.hip,
// decode_ms_fixed_layered.hip, decode_ms_fixed_corrected.hip): the persistent launch of one kernel, and the dispatch from (code,
// variant, app) to it.
#pragma once

#include "decode_ms_launch.hpp"          // claim_counter, persistent_grid, resident_workgroups, LDPC_TABLE_F32

namespace ldpc {

// Persistent workgroups over the codeword groups, as in launch_cfg_form (decode_ms_launch.hpp): the launch's queue for workgroups of
// 8 waves and more, the fixed stride on persistent_grid's 16x grid for the smaller ones; no queue where nothing iterates.
// KERNEL: a layered kernel; GEO: its LayeredGeometry / LayeredFixedGeometry; `extra`: the kernel's arguments behind `claim`.
template <auto KERNEL, class GEO, class T, class A, class... Extra>
hipError_t launch_layered(const T *llrs, A *app, uint8_t *output, uint32_t *iters, uint8_t *success, size_t batch, uint32_t maxiters,
                          hipStream_t stream, Extra... extra)
{
    if (batch == 0) return hipSuccess;
    const size_t groups = (batch + GEO::G - 1) / GEO::G;
    if (batch > 0xFFFFFFFFull || groups > 0x7FFFFFFFull) return hipErrorInvalidValue;   // (capi.hip slices larger batches)
    const size_t resident = resident_workgroups<KERNEL, GEO::WG>();
    uint32_t *claim = (maxiters == 0 || GEO::WG < 512) ? nullptr : claim_counter(stream);
    const size_t grid = persistent_grid(resident, claim != nullptr, groups);
    hipLaunchKernelGGL(KERNEL, dim3((unsigned)grid), dim3(GEO::WG), 0, stream,
                       llrs, app, output, iters, success, (uint32_t)batch, maxiters, claim, extra...);
    return hipGetLastError();
}

// The body of a layered launcher over (code, variant, app).  `variant` 0 is the only kernel: anything else is
// hipErrorInvalidConfiguration (EUNSUPPORTED).  Then LDPC_LAYERED_CALL(CODE, SOFT) -- the unit's own launch_layered call -- for the
// code's row of LDPC_TABLE_F32: the hard form for app == nullptr, else the soft form.
#define LDPC_LAYERED_CASE(CODE, ...) \
    case CODE: return app ? LDPC_LAYERED_CALL(CODE, true) : LDPC_LAYERED_CALL(CODE, false);
#define LDPC_LAYERED_DISPATCH()                                                                  \
    if (variant != 0) return hipErrorInvalidConfiguration;                                       \
    switch (code) {                                                                              \
        LDPC_TABLE_F32(LDPC_LAYERED_CASE)                                                        \
        default: return hipErrorInvalidValue;                                                    \
    }

}  // namespace ldpc
