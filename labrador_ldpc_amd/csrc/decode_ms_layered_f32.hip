// decode_ms_layered_f32.hip -- block-row layered min-sum decoding of f32 LLRs (decode_ms_layered.hpp): a hard form
// and a soft-output form of one kernel per code, and their launcher.
#include "decode_ms_launch.hpp"
#include "decode_ms_layered.hpp"

namespace ldpc {

template <int CODE, bool SOFT>
hipError_t launch_layered(const float *llrs, float *app, uint8_t *output, uint32_t *iters, uint8_t *success, size_t batch,
                          uint32_t maxiters, hipStream_t stream)
{
    using GEO = LayeredGeometry<CODE>;
    if (batch == 0) return hipSuccess;
    const size_t groups = (batch + GEO::G - 1) / GEO::G;
    if (batch > 0xFFFFFFFFull || groups > 0x7FFFFFFFull) return hipErrorInvalidValue;   // (capi.hip slices larger batches)
    const size_t resident = resident_workgroups<decode_ms_layered_kernel<CODE, SOFT>, GEO::WG>();
    uint32_t *claim = (maxiters == 0 || GEO::WG < 512) ? nullptr : claim_counter(stream);
    const size_t grid = persistent_grid(resident, claim != nullptr, groups);
    hipLaunchKernelGGL((decode_ms_layered_kernel<CODE, SOFT>), dim3((unsigned)grid), dim3(GEO::WG), 0, stream,
                       llrs, app, output, iters, success, (uint32_t)batch, maxiters, claim);
    return hipGetLastError();
}

// app == nullptr: the hard form.  `variant` 0 is the only kernel: anything else is hipErrorInvalidConfiguration (EUNSUPPORTED).
hipError_t launch_decode_ms_layered(int code, int variant, const float *llrs, float *app, uint8_t *output, uint32_t *iters,
                                    uint8_t *success, size_t batch, uint32_t maxiters, hipStream_t stream)
{
    if (variant != 0) return hipErrorInvalidConfiguration;
#define LDPC_LAYERED_CASE(CODE, T, ...)                                                                                       \
    case CODE:                                                                                                                \
        return app ? launch_layered<CODE, true>(llrs, app, output, iters, success, batch, maxiters, stream)                  \
                   : launch_layered<CODE, false>(llrs, nullptr, output, iters, success, batch, maxiters, stream);
    switch (code) {
        LDPC_TABLE_F32(LDPC_LAYERED_CASE)
        default: return hipErrorInvalidValue;
    }
#undef LDPC_LAYERED_CASE
}

}  // namespace ldpc
