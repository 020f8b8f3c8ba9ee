// decode_ms_bs_soft.hip -- gfx950 instantiation of the bit-sliced i8 min-sum decoder WITH soft output (decode_ms_bitslice.hpp,
// Decoder<..., SOFT = true>) for the one-wave TM codes -- TM1536, TM2048, TM6144, TM8192 -- and its launcher.
//
// The decoder of decode_ms_bs.hip with two things added: where an iteration stores a block column's hard word it keeps the seven
// magnitude planes of the same marginal under the same rule (Decoder::columns), in registers or in LDS as the code's plan says
// (BsPlan::SOFT_LDS), and an epilogue turns the planes back into bytes: app [batch][n + p] i8, the reference's saturating va
// (store_marginals).  Lockstep form only, at every batch size: no slot refill, no crossover to the f32-pipe kernels, no two-wave
// form (TM1280, TM5120).
//
// Compiled per unit like decode_ms_bs.hip (Makefile, -DBS_TU, the same scheduler flags per unit) into objects of its own: the plain
// and the corrected objects keep exactly the kernels they had.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "decode_ms_bitslice.hpp"
#include "decode_ms_bs_launch.hpp"
#include "decode_ms_protos.hpp"
#include "hip_backend.hpp"

namespace ldpc {
namespace bs {

template <int CODE>
__global__ void __launch_bounds__(64, BsPlan<CODE>::SOFT_WAVES_PER_SIMD)
decode_ms_bsa_kernel(const int8_t *__restrict__ llrs, int8_t *__restrict__ app, uint8_t *__restrict__ output, uint32_t *__restrict__ iters,
                     uint8_t *__restrict__ success, uint32_t batch, uint32_t maxiters, uint32_t ngroups)
{
    __shared__ __attribute__((aligned(16))) char lds[Geo<CODE>::LDS_BYTES_SOFT];
    HipBackend b{lds};
    init_kernel<CODE, HipBackend>(b);
    for (uint32_t g = blockIdx.x; g < ngroups; g += gridDim.x)
        decode_group<CODE, HipBackend, false, 8, true>(b, llrs, output, iters, success, batch, maxiters, g, 1, 0, 0, app);
}

// The soft form (decode_ms_bs_launch.hpp): the one-wave codes
struct SoftForm {
    static constexpr bool I8_ONLY = true;
    struct Args {
        const int8_t *llrs; int8_t *app; uint8_t *output; uint32_t *iters; uint8_t *success; size_t batch; uint32_t maxiters; hipStream_t stream;
    };
    using Codes = OneWaveCodes;
    template <int CODE>
    static hipError_t launch(const Args &a)
    {
        return launch_lockstep<decode_ms_bsa_kernel<CODE>, 64, BsPlan<CODE>::G>(a.stream, a.batch, a.maxiters, std::tuple{a.llrs, a.app, a.output, a.iters, a.success});
    }
};

}  // namespace bs

#if BS_TU == 2
template hipError_t bs::launch_in_unit2<bs::SoftForm>(int, const bs::SoftForm::Args &);
#else
hipError_t launch_decode_ms_bitsliced_soft(int code, const int8_t *llrs, int8_t *app, uint8_t *output, uint32_t *iters, uint8_t *success,
                                           size_t batch, uint32_t maxiters, hipStream_t stream)
{
    return bs::launch_form<bs::SoftForm>(code, {llrs, app, output, iters, success, batch, maxiters, stream});
}
#endif

}  // namespace ldpc
