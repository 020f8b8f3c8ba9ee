// decode_ms_half_layered.hip -- layered min-sum decoding of f16 / bf16 LLRs: the corrected kernels of
// decode_ms_layered.hpp with a half-precision source, whose loader widens every LLR to f32 by the rule of llr_widen.hpp as it fills
// the LDS copy.  A hard form and a soft-output form of one kernel per code and format, and their launcher; the plain entries come
// here at (scale, offset) = (1, 0), which is the plain kernel's result bit for bit.  A unit of its own, so that
// decode_ms_layered_f32.o and decode_ms_corrected_f32.o hold exactly the kernels they held.
#include "decode_ms_layered_launch.hpp"
#include "decode_ms_layered.hpp"
#include <type_traits>

namespace ldpc {

template <int CODE, class H, bool SOFT>
__global__ void __launch_bounds__(LayeredGeometry<CODE>::WG)
decode_ms_half_layered_kernel(const H *__restrict__ llrs, float *__restrict__ app, uint8_t *__restrict__ output,
                              uint32_t *__restrict__ iters_out, uint8_t *__restrict__ success_out, uint32_t batch, uint32_t maxiters,
                              uint32_t *claim, float scale, float offset)
{
    static_assert(std::is_same_v<H, f16_llr> || std::is_same_v<H, bf16_llr>);
    __shared__ __attribute__((aligned(16))) char lds[LayeredGeometry<CODE>::LDS_BYTES];
    decode_ms_layered_body<CODE, SOFT, true, H>(llrs, app, output, iters_out, success_out, batch, maxiters, claim, lds, scale, offset);
}

#define LDPC_LAYERED_CALL(CODE, SOFT)                                                                                            \
    launch_layered<decode_ms_half_layered_kernel<CODE, H, SOFT>, LayeredGeometry<CODE>>(llrs, app, output, iters, success, batch, maxiters, \
                                                                                        stream, scale, offset)

template <class H>
hipError_t launch_decode_ms_half_layered(int code, int variant, const H *llrs, float *app, uint8_t *output, uint32_t *iters,
                                         uint8_t *success, size_t batch, uint32_t maxiters, float scale, float offset, hipStream_t stream)
{
    LDPC_LAYERED_DISPATCH()
}

template hipError_t launch_decode_ms_half_layered<f16_llr>(int, int, const f16_llr *, float *, uint8_t *, uint32_t *, uint8_t *, size_t,
                                                           uint32_t, float, float, hipStream_t);
template hipError_t launch_decode_ms_half_layered<bf16_llr>(int, int, const bf16_llr *, float *, uint8_t *, uint32_t *, uint8_t *, size_t,
                                                            uint32_t, float, float, hipStream_t);

}  // namespace ldpc
