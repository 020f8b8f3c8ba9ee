// decode_ms_fixed_corrected.hip -- fixed-point layered min-sum decoding of i8 and i16 LLRs with normalized / offset check messages
// (decode_ms_fixed_layered.hpp with its correction step): a hard form and a soft-output form of one kernel per code and
// type, and their launcher.  A unit of its own, so that decode_ms_fixed_layered.o holds exactly the kernels it held.
#include "decode_ms_layered_launch.hpp"
#include "decode_ms_fixed_layered.hpp"

namespace ldpc {

#define LDPC_LAYERED_CALL(CODE, SOFT)                                                                                         \
    launch_layered<decode_ms_layered_fixed_corrected_kernel<CODE, T, SOFT>, LayeredFixedGeometry<CODE>>(                      \
        llrs, app, output, iters, success, batch, maxiters, stream, scale_num, scale_shift, offset)

template <class T>
hipError_t launch_decode_ms_layered_fixed_corrected(int code, int variant, const T *llrs, int32_t *app, uint8_t *output, uint32_t *iters,
                                                    uint8_t *success, size_t batch, uint32_t maxiters, uint32_t scale_num,
                                                    uint32_t scale_shift, uint32_t offset, hipStream_t stream)
{
    LDPC_LAYERED_DISPATCH()
}

template hipError_t launch_decode_ms_layered_fixed_corrected<int8_t>(int, int, const int8_t *, int32_t *, uint8_t *, uint32_t *, uint8_t *,
                                                                     size_t, uint32_t, uint32_t, uint32_t, uint32_t, hipStream_t);
template hipError_t launch_decode_ms_layered_fixed_corrected<int16_t>(int, int, const int16_t *, int32_t *, uint8_t *, uint32_t *,
                                                                      uint8_t *, size_t, uint32_t, uint32_t, uint32_t, uint32_t, hipStream_t);

}  // namespace ldpc
