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

#ifndef BS_TU
#error "decode_ms_bs_soft.hip is compiled per unit: -DBS_TU=1 (rate 1/2 + dispatch) or -DBS_TU=2 (rate 2/3)"
#endif

#include "decode_ms_bitslice.hpp"
#include "decode_ms_protos.hpp"
#include "hip_backend.hpp"

namespace ldpc {
namespace bs {

static_assert(PL == 8, "the soft form is built for i8 planes");

// what a CU must hold: the waves the kernel is compiled for, each with the soft layout's LDS
template <int CODE>
constexpr bool soft_lds_fits() { return 4 * BsPlan<CODE>::SOFT_WAVES_PER_SIMD * Geo<CODE>::LDS_BYTES_SOFT <= 163840; }
static_assert(soft_lds_fits<TM1536>() && soft_lds_fits<TM2048>() && soft_lds_fits<TM6144>() && soft_lds_fits<TM8192>(),
              "waves per CU the soft kernels are compiled for x LDS per wave <= 160 KB");

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

// one group of G codewords per workgroup, the hardware dispatcher hands them out (launch_lockstep of decode_ms_bs.hip)
template <int CODE>
hipError_t launch_lockstep_soft(const int8_t *llrs, int8_t *app, uint8_t *output, uint32_t *iters, uint8_t *success, size_t batch,
                                uint32_t maxiters, hipStream_t stream)
{
    constexpr int G = BsPlan<CODE>::G;
    if (batch == 0) return hipSuccess;
    if (batch > 0xFFFFFFFFull) return hipErrorInvalidValue;
    const size_t groups = (batch + G - 1) / G;
    const size_t grid = groups < 0x7FFFFFFFull ? groups : 0x7FFFFFFFull;
    hipLaunchKernelGGL(decode_ms_bsa_kernel<CODE>, dim3((unsigned)grid), dim3(64), 0, stream, llrs, app, output, iters, success, (uint32_t)batch,
                       maxiters, (uint32_t)groups);
    return hipGetLastError();
}

// the codes THIS compile unit builds (BsPlan::UNIT); hipErrorInvalidConfiguration for every other code
static hipError_t launch_soft_in_unit(int code, const int8_t *llrs, int8_t *app, uint8_t *output, uint32_t *iters, uint8_t *success, size_t batch,
                                      uint32_t maxiters, hipStream_t stream)
{
    auto built_here = [&](auto C_) {
        constexpr int CODE = decltype(C_)::value;
        if constexpr (BsPlan<CODE>::UNIT == BS_TU) return launch_lockstep_soft<CODE>(llrs, app, output, iters, success, batch, maxiters, stream);
        else return hipErrorInvalidConfiguration;
    };
    switch (code) {
        case TM1536: return built_here(IC<TM1536>{});
        case TM2048: return built_here(IC<TM2048>{});
        case TM6144: return built_here(IC<TM6144>{});
        case TM8192: return built_here(IC<TM8192>{});
        default: return hipErrorInvalidConfiguration;
    }
}

}  // namespace bs

hipError_t launch_decode_ms_bitsliced_soft_unit2(int code, const int8_t *llrs, int8_t *app, uint8_t *output, uint32_t *iters, uint8_t *success,
                                                 size_t batch, uint32_t maxiters, hipStream_t stream);
#if BS_TU == 2
hipError_t launch_decode_ms_bitsliced_soft_unit2(int code, const int8_t *llrs, int8_t *app, uint8_t *output, uint32_t *iters, uint8_t *success,
                                                 size_t batch, uint32_t maxiters, hipStream_t stream)
{
    return bs::launch_soft_in_unit(code, llrs, app, output, iters, success, batch, maxiters, stream);
}
#else
hipError_t launch_decode_ms_bitsliced_soft(int code, const int8_t *llrs, int8_t *app, uint8_t *output, uint32_t *iters, uint8_t *success,
                                           size_t batch, uint32_t maxiters, hipStream_t stream)
{
    if (!bs::bitsliced_soft_code(code)) return hipErrorInvalidConfiguration;
    if (bs::BS_DISPATCH[code].unit == BS_TU) return bs::launch_soft_in_unit(code, llrs, app, output, iters, success, batch, maxiters, stream);
    return launch_decode_ms_bitsliced_soft_unit2(code, llrs, app, output, iters, success, batch, maxiters, stream);
}
#endif

}  // namespace ldpc
