// decode_ms_corrected_f32.hip -- layered min-sum decoding of f32 LLRs with normalized / offset check messages (decode_ms_layered.hpp
// with its correction step): a hard form and a soft-output form of one kernel per code, and their launcher.  A unit of
// its own, so that decode_ms_layered_f32.o holds exactly the kernels it held.
#include "decode_ms_layered_launch.hpp"
#include "decode_ms_layered.hpp"

namespace ldpc {

#define LDPC_LAYERED_CALL(CODE, SOFT)                                                                                         \
    launch_layered<decode_ms_corrected_kernel<CODE, SOFT>, LayeredGeometry<CODE>>(llrs, app, output, iters, success, batch, maxiters, stream, \
                                                                                  scale, offset)

hipError_t launch_decode_ms_layered_corrected(int code, int variant, const float *llrs, float *app, uint8_t *output, uint32_t *iters,
                                              uint8_t *success, size_t batch, uint32_t maxiters, float scale, float offset,
                                              hipStream_t stream)
{
    LDPC_LAYERED_DISPATCH()
}

}  // namespace ldpc
