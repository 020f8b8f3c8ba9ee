// decode_ms_i32.hip -- i32 instantiations of the min-sum kernel (decode_ms::<i32>,
// /root/reference/src/decoder.rs:60-68, :347-475; the Rust generic accepts i32 although the reference's
// C API does not export it).  Integer arithmetic throughout (Ops<int32_t>, decode_ms_kernel.hpp).
// With -DLDPC_SOFT=1 (decode_ms_soft_i32.o): their soft-output forms.
#include "decode_ms_launch.hpp"

namespace ldpc {

template hipError_t launch_decode_ms<int32_t, LDPC_SOFT>(int, int, const int32_t *, int32_t *, uint8_t *, uint32_t *, uint8_t *, size_t, uint32_t,
                                                         hipStream_t);
#if !LDPC_SOFT
template bool decode_ms_reads_llrs_once<int32_t>(int, int);
#endif

}  // namespace ldpc
