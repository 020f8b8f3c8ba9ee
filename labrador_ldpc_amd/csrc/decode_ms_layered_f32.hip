// decode_ms_layered_f32.hip -- block-row layered min-sum decoding of f32 LLRs (decode_ms_layered.hpp): a hard form
// and a soft-output form of one kernel per code, and their launcher.
#include "decode_ms_layered_launch.hpp"
#include "decode_ms_layered.hpp"

namespace ldpc {

#define LDPC_LAYERED_CALL(CODE, SOFT)                                                                                         \
    launch_layered<decode_ms_layered_kernel<CODE, SOFT>, LayeredGeometry<CODE>>(llrs, app, output, iters, success, batch, maxiters, stream)

hipError_t launch_decode_ms_layered(int code, int variant, const float *llrs, float *app, uint8_t *output, uint32_t *iters,
                                    uint8_t *success, size_t batch, uint32_t maxiters, hipStream_t stream)
{
    LDPC_LAYERED_DISPATCH()
}

}  // namespace ldpc
