// decode_ms_soft_f32_part.hip -- the heavy f32 soft-output instantiations, three objects of their own (Makefile: -DF32_PART=1/2/3),
// declared `extern template` in decode_ms_soft_f32.hip.  The split mirrors decode_ms_f32_part.hip.
#include "decode_ms_launch.hpp"

namespace ldpc {

#ifndef F32_PART
#error "compile with -DF32_PART=1, 2 or 3"
#endif
#define LDPC_F32_SOFT_SIG (const float *, uint8_t *, uint32_t *, uint8_t *, size_t, uint32_t, hipStream_t, unsigned, float *)

#if F32_PART == 1
template hipError_t launch_pair<TM8192, float, true> LDPC_F32_SOFT_SIG;
#elif F32_PART == 2
template hipError_t launch_pair<TM2048, float, true> LDPC_F32_SOFT_SIG;
template hipError_t launch_one<TM8192, float, 2, true> LDPC_F32_SOFT_SIG;
template hipError_t launch_one<TM8192, float, 4, true> LDPC_F32_SOFT_SIG;
#else
template hipError_t launch_one<TM5120, float, 1, true> LDPC_F32_SOFT_SIG;        // one-pass kernel and the two NaN passes
template hipError_t launch_one<TM6144, float, 1, true> LDPC_F32_SOFT_SIG;
template hipError_t launch_one<TM6144, float, 2, true> LDPC_F32_SOFT_SIG;
#endif

}  // namespace ldpc
