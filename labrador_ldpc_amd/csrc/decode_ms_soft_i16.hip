// decode_ms_soft_i16.hip -- decode_ms::<i16> with soft output (/root/reference/src/decoder.rs:377): the soft-output forms of the
// kernels of decode_ms_i16.hip, dispatched by the same table (decode_ms_tables.hpp).
#include "decode_ms_launch.hpp"
#include "decode_ms_tables.hpp"

namespace ldpc {

template <>
hipError_t launch_decode_ms_soft<int16_t>(int code, int variant, const int16_t *llrs, int16_t *app, uint8_t *output, uint32_t *iters,
                                     uint8_t *success, size_t batch, uint32_t maxiters, hipStream_t stream)
{
    LDPC_SPLIT_VARIANT();
    if (variant == VARIANT_PAIR || (variant == 0 && code == TM8192)) {     // TM8192: the pair-ownership kernel
        if (code == TM8192) return launch_pair<TM8192, int16_t, true>(llrs, output, iters, success, batch, maxiters, stream, lflags, app);
        return hipErrorInvalidConfiguration;
    }
    switch (code) {
        LDPC_TABLE_I16(LDPC_SOFT_CASE)
        default: return hipErrorInvalidValue;
    }
}

}  // namespace ldpc
