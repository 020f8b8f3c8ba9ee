// decode_ms_flooding_corrected_f32.hip -- flooding min-sum decoding of f32 LLRs with normalized / offset check messages
// (decode_ms_flooding_corrected.hpp): a hard form and a soft-output form of one kernel per code, and their launcher.
// Units of their own -- four objects from this source, -DFC_PART=0..3 -- so that every other object holds exactly the kernels it held.
#include "decode_ms_flooding_corrected.hpp"

namespace ldpc {

#ifndef FC_PART
#error "compile with -DFC_PART=0, 1, 2 or 3"
#endif

#if FC_PART == 0

#define LDPC_FC_EXTERN(CODE, IPT)                                                   \
    extern template hipError_t launch_flooding_corrected<CODE, IPT, false> LDPC_FC_SIG; \
    extern template hipError_t launch_flooding_corrected<CODE, IPT, true> LDPC_FC_SIG;
LDPC_FC_PART_1(LDPC_FC_EXTERN)
LDPC_FC_PART_2(LDPC_FC_EXTERN)
LDPC_FC_PART_3(LDPC_FC_EXTERN)

// one row of the f32 table (decode_ms_tables.hpp): the code's default indices per thread
#define LDPC_FC_CASE(CODE, T, DEF, ...)                                                                                              \
    case CODE:                                                                                                                       \
        return app ? launch_flooding_corrected<CODE, DEF, true>(llrs, app, output, iters, success, batch, maxiters, scale, offset, stream) \
                   : launch_flooding_corrected<CODE, DEF, false>(llrs, nullptr, output, iters, success, batch, maxiters, scale, offset, stream);

hipError_t launch_decode_ms_flooding_corrected(int code, int variant, const float *llrs, float *app, uint8_t *output, uint32_t *iters,
                                               uint8_t *success, size_t batch, uint32_t maxiters, float scale, float offset,
                                               hipStream_t stream)
{
    if (variant != 0) return hipErrorInvalidConfiguration;
    switch (code) { LDPC_TABLE_F32(LDPC_FC_CASE) }
    return hipErrorInvalidValue;
}

#else

#define LDPC_FC_CAT2(a, b) a##b
#define LDPC_FC_CAT(a, b) LDPC_FC_CAT2(a, b)
#define LDPC_FC_INSTANTIATE(CODE, IPT)                                       \
    template hipError_t launch_flooding_corrected<CODE, IPT, false> LDPC_FC_SIG; \
    template hipError_t launch_flooding_corrected<CODE, IPT, true> LDPC_FC_SIG;
LDPC_FC_CAT(LDPC_FC_PART_, FC_PART)(LDPC_FC_INSTANTIATE)

#endif

}  // namespace ldpc
