// decode_ms_f32_part.hip -- the heavy f32 instantiations of the min-sum kernel, compiled as three objects of their own
// (Makefile: -DF32_PART=1/2/3, and with -DLDPC_SOFT=1 three more for the soft-output forms) so that the build stays parallel:
// decode_ms_f32.hip declares them `extern template`.
// (decode_ms::<f32>, /root/reference/src/decoder.rs:69-77, :347-475)
#include "decode_ms_launch.hpp"

namespace ldpc {

#ifndef F32_PART
#error "compile with -DF32_PART=1, 2 or 3"
#endif
#define F32_CAT2(a, b) a##b
#define F32_CAT(a, b) F32_CAT2(a, b)
#define LDPC_F32_INSTANTIATE(...) template hipError_t __VA_ARGS__ LDPC_F32_SIG;

F32_CAT(LDPC_F32_PART_, F32_PART)(LDPC_F32_INSTANTIATE, LDPC_SOFT)

}  // namespace ldpc
