// decode_ms_i16.hip -- i16 instantiations of the min-sum kernel (decode_ms::<i16>,
// /root/reference/src/decoder.rs:51-59, :347-475; C entry capi/src/lib.rs:105-111).
#include "decode_ms_launch.hpp"
#include "decode_ms_tables.hpp"

namespace ldpc {

// code -> default and alternative indices per thread (decode_ms_tables.hpp: one table for the dispatch, decode_ms_reads_llrs_once
// and the soft-output dispatch)
#define LDPC_TABLE LDPC_TABLE_I16

template <>
hipError_t launch_decode_ms<int16_t>(int code, int variant, const int16_t *llrs, uint8_t *output,
                                    uint32_t *iters, uint8_t *success, size_t batch,
                                    uint32_t maxiters, hipStream_t stream)
{
    LDPC_SPLIT_VARIANT();
    // TM8192: pair-ownership kernel by default (decode_ms_pair.hpp), `variant` 2 / 4 = the (t, t + M/2) kernel
    if (variant == VARIANT_PAIR || (variant == 0 && code == TM8192)) {
        if (code == TM8192) return launch_pair<TM8192, int16_t>(llrs, output, iters, success, batch, maxiters, stream, lflags);
        return hipErrorInvalidConfiguration;
    }
    switch (code) {
        LDPC_TABLE(LDPC_CASE)
        default: return hipErrorInvalidValue;
    }
}

template <>
bool decode_ms_reads_llrs_once<int16_t>(int code, int variant)
{
    if (variant != 0) return false;
    if (code == TM8192) return true;             // the pair kernel holds its LLRs in registers
    switch (code) {
        LDPC_TABLE(LDPC_ONCE_CASE)
        default: return false;
    }
}

}  // namespace ldpc
