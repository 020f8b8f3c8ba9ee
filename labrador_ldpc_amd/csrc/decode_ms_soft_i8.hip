// decode_ms_soft_i8.hip -- decode_ms::<i8> with soft output (/root/reference/src/decoder.rs:42-50, :377).
// Soft i8 runs the f32-pipe i8 kernels of decode_ms_i8.hip -- the ones its default dispatch takes for small or unaligned batches --
// in their soft-output form.  The bit-sliced kernels keep no marginals once a parity vote is taken (decode_ms_bitslice.hpp;
// DESIGN.md "Soft output"), so `variant` 64 (LABRADOR_LDPC_HIP_VARIANT_BITSLICE) has no soft form.
#include "decode_ms_launch.hpp"
#include "decode_ms_tables.hpp"

namespace ldpc {

template <>
hipError_t launch_decode_ms_soft<int8_t>(int code, int variant, const int8_t *llrs, int8_t *app, uint8_t *output, uint32_t *iters,
                                         uint8_t *success, size_t batch, uint32_t maxiters, hipStream_t stream)
{
    constexpr int VARIANT_BITSLICE = 64;
    LDPC_SPLIT_VARIANT();
    if (!valid_code(code)) return hipErrorInvalidValue;
    if (variant == VARIANT_BITSLICE) return hipErrorInvalidConfiguration;
    if (variant == VARIANT_PAIR || (variant == 0 && code == TM8192)) {     // TM8192: the pair-ownership kernel, as in decode_ms_i8.hip
        if (code == TM8192) return launch_pair<TM8192, int8_t, true>(llrs, output, iters, success, batch, maxiters, stream, lflags, app);
        return hipErrorInvalidConfiguration;
    }
    switch (code) {
        LDPC_TABLE_I8(LDPC_SOFT_CASE)
        default: return hipErrorInvalidValue;
    }
}

}  // namespace ldpc
