// decode_ms_fixed_quantised.hip -- fixed-point layered min-sum decoding of f32 LLRs: the kernels of
// decode_ms_fixed_layered.hpp with a float source, whose loader quantises every LLR to i8 / i16 by the rule of llr_quantise.hpp as it
// fills the LDS marginals.  A hard form and a soft-output form, plain and with the correction step, of one kernel per code and type,
// and their launcher.  A unit of its own, so that decode_ms_fixed_layered.o and decode_ms_fixed_corrected.o hold exactly the kernels
// they held.
#include "decode_ms_layered_launch.hpp"
#include "decode_ms_fixed_layered.hpp"

namespace ldpc {

// One argument list for both forms; without CORRECTED the triple is not read.
template <int CODE, class T, bool SOFT, bool CORRECTED>
__global__ void __launch_bounds__(LayeredFixedGeometry<CODE>::WG)
decode_ms_layered_fixed_quantised_kernel(const float *__restrict__ llrs, int32_t *__restrict__ app, uint8_t *__restrict__ output,
                                         uint32_t *__restrict__ iters_out, uint8_t *__restrict__ success_out, uint32_t batch,
                                         uint32_t maxiters, uint32_t *claim, float scale, float flim, uint32_t scale_num,
                                         uint32_t scale_shift, uint32_t offset)
{
    __shared__ __attribute__((aligned(16))) char lds[LayeredFixedGeometry<CODE>::LDS_BYTES];
    decode_ms_layered_fixed_body<CODE, T, SOFT, CORRECTED, float>(llrs, app, output, iters_out, success_out, batch, maxiters, claim, lds,
                                                                  scale_num, scale_shift, offset, scale, flim);
}

#define LDPC_QUANTISED_CALL(CODE, SOFT, CORRECTED)                                                                            \
    launch_layered<decode_ms_layered_fixed_quantised_kernel<CODE, T, SOFT, CORRECTED>, LayeredFixedGeometry<CODE>>(           \
        llrs, app, output, iters, success, batch, maxiters, stream, scale, (float)lim, scale_num, scale_shift, offset)
#define LDPC_LAYERED_CALL(CODE, SOFT) (corrected ? LDPC_QUANTISED_CALL(CODE, SOFT, true) : LDPC_QUANTISED_CALL(CODE, SOFT, false))

template <class T>
hipError_t launch_decode_ms_layered_fixed_quantised(int code, int variant, const float *llrs, int32_t *app, uint8_t *output,
                                                    uint32_t *iters, uint8_t *success, size_t batch, uint32_t maxiters, float scale,
                                                    int lim, bool corrected, uint32_t scale_num, uint32_t scale_shift, uint32_t offset,
                                                    hipStream_t stream)
{
    LDPC_LAYERED_DISPATCH()
}

template hipError_t launch_decode_ms_layered_fixed_quantised<int8_t>(int, int, const float *, int32_t *, uint8_t *, uint32_t *, uint8_t *,
                                                                     size_t, uint32_t, float, int, bool, uint32_t, uint32_t, uint32_t,
                                                                     hipStream_t);
template hipError_t launch_decode_ms_layered_fixed_quantised<int16_t>(int, int, const float *, int32_t *, uint8_t *, uint32_t *, uint8_t *,
                                                                      size_t, uint32_t, float, int, bool, uint32_t, uint32_t, uint32_t,
                                                                      hipStream_t);

}  // namespace ldpc
