// decode_ms_fixed_layered.hip -- block-row layered min-sum decoding of i8 and i16 LLRs in fixed point (decode_ms_fixed_layered.hpp,
// DESIGN.md 4.7): a hard form and a soft-output form of one kernel per code and type, and their launcher.
#include "decode_ms_layered_launch.hpp"
#include "decode_ms_fixed_layered.hpp"

namespace ldpc {

#define LDPC_LAYERED_CALL(CODE, SOFT)                                                                                         \
    launch_layered<decode_ms_layered_fixed_kernel<CODE, T, SOFT>, LayeredFixedGeometry<CODE>>(llrs, app, output, iters, success, batch, \
                                                                                              maxiters, stream)

template <class T>
hipError_t launch_decode_ms_layered_fixed(int code, int variant, const T *llrs, int32_t *app, uint8_t *output, uint32_t *iters,
                                          uint8_t *success, size_t batch, uint32_t maxiters, hipStream_t stream)
{
    LDPC_LAYERED_DISPATCH()
}

template hipError_t launch_decode_ms_layered_fixed<int8_t>(int, int, const int8_t *, int32_t *, uint8_t *, uint32_t *, uint8_t *, size_t,
                                                           uint32_t, hipStream_t);
template hipError_t launch_decode_ms_layered_fixed<int16_t>(int, int, const int16_t *, int32_t *, uint8_t *, uint32_t *, uint8_t *, size_t,
                                                            uint32_t, hipStream_t);

}  // namespace ldpc
