// decode_ms_soft_f32.hip -- decode_ms::<f32> with soft output (/root/reference/src/decoder.rs:347-475: the marginals `va`,
// :377, that decode_ms computes and drops).  The soft-output forms of every f32 kernel of decode_ms_f32.hip, dispatched by the
// same table (decode_ms_tables.hpp); kept out of the hard-only objects, whose kernels stay exactly what they are.
#include "decode_ms_launch.hpp"
#include "decode_ms_tables.hpp"

namespace ldpc {

// instantiated in decode_ms_soft_f32_part.hip (three more objects, as for the hard-only kernels)
#define LDPC_F32_SOFT_SIG (const float *, uint8_t *, uint32_t *, uint8_t *, size_t, uint32_t, hipStream_t, unsigned, float *)
extern template hipError_t launch_pair<TM8192, float, true> LDPC_F32_SOFT_SIG;
extern template hipError_t launch_pair<TM2048, float, true> LDPC_F32_SOFT_SIG;
extern template hipError_t launch_one<TM8192, float, 2, true> LDPC_F32_SOFT_SIG;
extern template hipError_t launch_one<TM8192, float, 4, true> LDPC_F32_SOFT_SIG;
extern template hipError_t launch_one<TM5120, float, 1, true> LDPC_F32_SOFT_SIG;
extern template hipError_t launch_one<TM6144, float, 1, true> LDPC_F32_SOFT_SIG;
extern template hipError_t launch_one<TM6144, float, 2, true> LDPC_F32_SOFT_SIG;

// every `variant` launch_decode_ms<float> accepts has a soft form
template <>
hipError_t launch_decode_ms_soft<float>(int code, int variant, const float *llrs, float *app, uint8_t *output, uint32_t *iters,
                                        uint8_t *success, size_t batch, uint32_t maxiters, hipStream_t stream)
{
    LDPC_SPLIT_VARIANT();
    if (variant == VARIANT_PAIR || (variant == 0 && code == TM8192)) {
        if (code == TM8192) return launch_pair<TM8192, float, true>(llrs, output, iters, success, batch, maxiters, stream, lflags, app);
        if (code == TM2048) return launch_pair<TM2048, float, true>(llrs, output, iters, success, batch, maxiters, stream, lflags, app);
        return hipErrorInvalidConfiguration;
    }
    switch (code) {
        LDPC_TABLE_F32(LDPC_SOFT_CASE)
        default: return hipErrorInvalidValue;
    }
}

}  // namespace ldpc
