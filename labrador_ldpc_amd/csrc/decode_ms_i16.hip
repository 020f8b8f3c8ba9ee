// decode_ms_i16.hip -- i16 instantiations of the min-sum kernel (decode_ms::<i16>,
// /root/reference/src/decoder.rs:51-59, :347-475; C entry capi/src/lib.rs:105-111).
// With -DLDPC_SOFT=1 (decode_ms_soft_i16.o): their soft-output forms.
#include "decode_ms_launch.hpp"

namespace ldpc {

template hipError_t launch_decode_ms<int16_t, LDPC_SOFT>(int, int, const int16_t *, int16_t *, uint8_t *, uint32_t *, uint8_t *, size_t, uint32_t,
                                                         hipStream_t);
#if !LDPC_SOFT
template bool decode_ms_reads_llrs_once<int16_t>(int, int);
#endif

}  // namespace ldpc
