// decode_ms_f32.hip -- f32 instantiations of the min-sum kernel (decode_ms::<f32>,
// /root/reference/src/decoder.rs:69-77, :347-475; C entry capi/src/lib.rs:113-119).
// With -DLDPC_SOFT=1 (decode_ms_soft_f32.o): their soft-output forms; every `variant` of the hard-only dispatch has one.
#include "decode_ms_launch.hpp"

namespace ldpc {

// instantiated in decode_ms_f32_part.hip
#define LDPC_F32_EXTERN(...) extern template hipError_t __VA_ARGS__ LDPC_F32_SIG;
LDPC_F32_PART_1(LDPC_F32_EXTERN, LDPC_SOFT)
LDPC_F32_PART_2(LDPC_F32_EXTERN, LDPC_SOFT)
LDPC_F32_PART_3(LDPC_F32_EXTERN, LDPC_SOFT)

template hipError_t launch_decode_ms<float, LDPC_SOFT>(int, int, const float *, float *, uint8_t *, uint32_t *, uint8_t *, size_t, uint32_t,
                                                       hipStream_t);
#if !LDPC_SOFT
template bool decode_ms_reads_llrs_once<float>(int, int);
#endif

}  // namespace ldpc
