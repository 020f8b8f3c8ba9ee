// decode_ms_fixed_layered.hip -- block-row layered min-sum decoding of i8 and i16 LLRs in fixed point (decode_ms_fixed_layered.hpp,
// DESIGN.md 4.7): a hard form and a soft-output form of one kernel per code and type, and their launcher.
#include "decode_ms_launch.hpp"
#include "decode_ms_fixed_layered.hpp"

namespace ldpc {

template <int CODE, class T, bool SOFT>
hipError_t launch_layered_fixed(const T *llrs, int32_t *app, uint8_t *output, uint32_t *iters, uint8_t *success, size_t batch,
                                uint32_t maxiters, hipStream_t stream)
{
    using GEO = LayeredFixedGeometry<CODE>;
    if (batch == 0) return hipSuccess;
    const size_t groups = (batch + GEO::G - 1) / GEO::G;
    if (batch > 0xFFFFFFFFull || groups > 0x7FFFFFFFull) return hipErrorInvalidValue;   // (capi.hip slices larger batches)
    const size_t resident = resident_workgroups<decode_ms_layered_fixed_kernel<CODE, T, SOFT>, GEO::WG>();
    uint32_t *claim = (maxiters == 0 || GEO::WG < 512) ? nullptr : claim_counter(stream);
    const size_t grid = persistent_grid(resident, claim != nullptr, groups);
    hipLaunchKernelGGL((decode_ms_layered_fixed_kernel<CODE, T, SOFT>), dim3((unsigned)grid), dim3(GEO::WG), 0, stream,
                       llrs, app, output, iters, success, (uint32_t)batch, maxiters, claim);
    return hipGetLastError();
}

// app == nullptr: the hard form.  `variant` 0 is the only kernel: anything else is hipErrorInvalidConfiguration (EUNSUPPORTED).
template <class T>
hipError_t launch_decode_ms_layered_fixed(int code, int variant, const T *llrs, int32_t *app, uint8_t *output, uint32_t *iters,
                                          uint8_t *success, size_t batch, uint32_t maxiters, hipStream_t stream)
{
    if (variant != 0) return hipErrorInvalidConfiguration;
#define LDPC_LAYERED_FIXED_CASE(CODE, ...)                                                                                    \
    case CODE:                                                                                                                \
        return app ? launch_layered_fixed<CODE, T, true>(llrs, app, output, iters, success, batch, maxiters, stream)         \
                   : launch_layered_fixed<CODE, T, false>(llrs, nullptr, output, iters, success, batch, maxiters, stream);
    switch (code) {
        LDPC_TABLE_F32(LDPC_LAYERED_FIXED_CASE)
        default: return hipErrorInvalidValue;
    }
#undef LDPC_LAYERED_FIXED_CASE
}

template hipError_t launch_decode_ms_layered_fixed<int8_t>(int, int, const int8_t *, int32_t *, uint8_t *, uint32_t *, uint8_t *, size_t,
                                                           uint32_t, hipStream_t);
template hipError_t launch_decode_ms_layered_fixed<int16_t>(int, int, const int16_t *, int32_t *, uint8_t *, uint32_t *, uint8_t *, size_t,
                                                            uint32_t, hipStream_t);

}  // namespace ldpc
