// decode_ms_bs_corrected_soft.hip -- gfx950 instantiation of the bit-sliced i8 min-sum decoder WITH normalized / offset check messages
// AND soft output (decode_ms_bitslice.hpp, Decoder<..., CORRECTED = true, MULBITS, SOFT = true>) for the one-wave TM
// codes -- TM1536, TM2048, TM6144, TM8192 -- and its launcher.
//
// The two switches are orthogonal in the decoder's text: the correction step rewrites a finished row's two minima behind the last block
// column (Decoder::correct_finished_rows), the soft form keeps a block column's marginal planes where its hard word is stored
// (Decoder::columns) and turns them into bytes in the epilogue (store_marginals).  This file is the kernels of decode_ms_bs_soft.hip
// with the triple of decode_ms_bs_corrected.hip: app [batch][n + p] i8 is the corrected decoder's saturating va.  Lockstep form only,
// at every batch size: no slot refill, no crossover to the f32-pipe kernels, no two-wave form (TM1280, TM5120).
//
// Compiled per unit like decode_ms_bs.hip (Makefile, -DBS_TU, the same scheduler flags per unit) into objects of its own: the plain,
// the corrected and the soft objects keep exactly the kernels they had.
#include <hip/hip_runtime.h>
#include <cstdint>

#ifndef BS_TU
#error "decode_ms_bs_corrected_soft.hip is compiled per unit: -DBS_TU=1 (rate 1/2 + dispatch) or -DBS_TU=2 (rate 2/3)"
#endif

#include "decode_ms_bitslice.hpp"
#include "decode_ms_protos.hpp"
#include "hip_backend.hpp"

namespace ldpc {
namespace bs {

static_assert(PL == 8, "the corrected soft form is built for i8 planes");

// Placement and launch bounds: the soft plan's (BsPlan::SOFT_LDS, SOFT_WAVES_PER_SIMD) for every form -- rate 1/2 keeps the planes in
// registers at two waves per SIMD, rate 2/3 in LDS at one (DESIGN.md 4.18 has what each form compiles to).
// what a CU must hold: the waves the kernel is compiled for, each with the soft layout's LDS
template <int CODE>
constexpr bool corrected_soft_lds_fits() { return 4 * BsPlan<CODE>::SOFT_WAVES_PER_SIMD * Geo<CODE>::LDS_BYTES_SOFT <= 163840; }
static_assert(corrected_soft_lds_fits<TM1536>() && corrected_soft_lds_fits<TM2048>() && corrected_soft_lds_fits<TM6144>() &&
              corrected_soft_lds_fits<TM8192>(), "waves per CU the corrected soft kernels are compiled for x LDS per wave <= 160 KB");

// MULBITS: the multiplier bits the form is built for (Decoder::correct_mag): 0 = the offset alone, 4, 8; the launcher picks the form
// from the call's scale (correction_mulbits).  Three kernels per code.
template <int CODE, int MULBITS>
__global__ void __launch_bounds__(64, BsPlan<CODE>::SOFT_WAVES_PER_SIMD)
decode_ms_bsca_kernel(const int8_t *__restrict__ llrs, int8_t *__restrict__ app, uint8_t *__restrict__ output, uint32_t *__restrict__ iters,
                      uint8_t *__restrict__ success, uint32_t batch, uint32_t maxiters, uint32_t ngroups, uint32_t scale_num,
                      uint32_t scale_shift, uint32_t offset)
{
    __shared__ __attribute__((aligned(16))) char lds[Geo<CODE>::LDS_BYTES_SOFT];
    HipBackend b{lds};
    init_kernel<CODE, HipBackend>(b);
    for (uint32_t g = blockIdx.x; g < ngroups; g += gridDim.x)
        decode_group<CODE, HipBackend, true, MULBITS, true>(b, llrs, output, iters, success, batch, maxiters, g, scale_num, scale_shift, offset,
                                                            app);
}

// one group of G codewords per workgroup, the hardware dispatcher hands them out (launch_lockstep of decode_ms_bs.hip)
template <int CODE, int MULBITS>
hipError_t launch_lockstep_corrected_soft(const int8_t *llrs, int8_t *app, uint8_t *output, uint32_t *iters, uint8_t *success, size_t batch,
                                          uint32_t maxiters, uint32_t scale_num, uint32_t scale_shift, uint32_t offset, hipStream_t stream)
{
    constexpr int G = BsPlan<CODE>::G;
    if (batch == 0) return hipSuccess;
    if (batch > 0xFFFFFFFFull) return hipErrorInvalidValue;
    const size_t groups = (batch + G - 1) / G;
    const size_t grid = groups < 0x7FFFFFFFull ? groups : 0x7FFFFFFFull;
    hipLaunchKernelGGL((decode_ms_bsca_kernel<CODE, MULBITS>), dim3((unsigned)grid), dim3(64), 0, stream, llrs, app, output, iters, success,
                       (uint32_t)batch, maxiters, (uint32_t)groups, scale_num, scale_shift, offset);
    return hipGetLastError();
}

// the codes THIS compile unit builds (BsPlan::UNIT); hipErrorInvalidConfiguration for every other code
static hipError_t launch_corrected_soft_in_unit(int code, const int8_t *llrs, int8_t *app, uint8_t *output, uint32_t *iters, uint8_t *success,
                                                size_t batch, uint32_t maxiters, uint32_t scale_num, uint32_t scale_shift, uint32_t offset,
                                                hipStream_t stream)
{
    auto form = [&](auto C_, auto M_) {
        constexpr int CODE = decltype(C_)::value, MULBITS = decltype(M_)::value;
        if constexpr (BsPlan<CODE>::UNIT == BS_TU)
            return launch_lockstep_corrected_soft<CODE, MULBITS>(llrs, app, output, iters, success, batch, maxiters, scale_num, scale_shift, offset,
                                                                 stream);
        else return hipErrorInvalidConfiguration;
    };
    auto built_here = [&](auto C_) {
        switch (correction_mulbits(scale_num, scale_shift)) {
            case 0: return form(C_, IC<0>{});
            case 4: return form(C_, IC<4>{});
            default: return form(C_, IC<8>{});
        }
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

hipError_t launch_decode_ms_bitsliced_corrected_soft_unit2(int code, const int8_t *llrs, int8_t *app, uint8_t *output, uint32_t *iters,
                                                           uint8_t *success, size_t batch, uint32_t maxiters, uint32_t scale_num,
                                                           uint32_t scale_shift, uint32_t offset, hipStream_t stream);
#if BS_TU == 2
hipError_t launch_decode_ms_bitsliced_corrected_soft_unit2(int code, const int8_t *llrs, int8_t *app, uint8_t *output, uint32_t *iters,
                                                           uint8_t *success, size_t batch, uint32_t maxiters, uint32_t scale_num,
                                                           uint32_t scale_shift, uint32_t offset, hipStream_t stream)
{
    return bs::launch_corrected_soft_in_unit(code, llrs, app, output, iters, success, batch, maxiters, scale_num, scale_shift, offset, stream);
}
#else
hipError_t launch_decode_ms_bitsliced_corrected_soft(int code, const int8_t *llrs, int8_t *app, uint8_t *output, uint32_t *iters,
                                                     uint8_t *success, size_t batch, uint32_t maxiters, uint32_t scale_num,
                                                     uint32_t scale_shift, uint32_t offset, hipStream_t stream)
{
    if (!bs::bitsliced_soft_code(code)) return hipErrorInvalidConfiguration;
    if (bs::BS_DISPATCH[code].unit == BS_TU)
        return bs::launch_corrected_soft_in_unit(code, llrs, app, output, iters, success, batch, maxiters, scale_num, scale_shift, offset, stream);
    return launch_decode_ms_bitsliced_corrected_soft_unit2(code, llrs, app, output, iters, success, batch, maxiters, scale_num, scale_shift, offset,
                                                           stream);
}
#endif

}  // namespace ldpc
