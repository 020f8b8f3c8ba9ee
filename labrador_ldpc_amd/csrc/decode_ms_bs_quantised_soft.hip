// decode_ms_bs_quantised_soft.hip -- gfx950 instantiation of the bit-sliced i8 min-sum decoder READING F32 LLRs WITH soft output
// (decode_ms_bitslice.hpp, decode_group<..., SOFT = true, QuantisedF32>) for the one-wave TM codes -- TM1536, TM2048,
// TM6144, TM8192 -- and its launchers.
//
// The soft kernels of decode_ms_bs_soft.hip (plain) and decode_ms_bs_corrected_soft.hip (normalized / offset check messages) with the
// loader's source of decode_ms_bs_quantised.hip.  The two switches meet nowhere in the decoder's text: the f32 loader fills the staging
// slab before the first iteration and nothing behind the slab knows what the rows were; the soft form keeps the marginal planes inside
// the iteration and turns them into bytes in the epilogue (store_marginals), whose slab lies in the LLR planes' area, dead by then.
// Per frame the four results are those of the i8 soft kernel on the frame quantised by llr_quantise.hip, bit for bit, without a
// quantised copy of the batch.  Lockstep forms only, at every batch size: no slot refill, no two-wave form (TM1280, TM5120).
//
// Compiled per unit like decode_ms_bs.hip (Makefile, -DBS_TU, the same scheduler flags per unit) into objects of its own: every other
// object keeps exactly the kernels it had.
#include <hip/hip_runtime.h>
#include <cstdint>

#ifndef BS_TU
#error "decode_ms_bs_quantised_soft.hip is compiled per unit: -DBS_TU=1 (rate 1/2 + dispatch) or -DBS_TU=2 (rate 2/3)"
#endif

#include "decode_ms_bitslice.hpp"
#include "decode_ms_protos.hpp"
#include "hip_backend.hpp"

namespace ldpc {
#if BS_PLANES == 8
namespace bs {

// Placement and launch bounds: the soft plan's (BsPlan::SOFT_LDS, SOFT_WAVES_PER_SIMD) for every form, as in
// decode_ms_bs_corrected_soft.hip -- rate 1/2 keeps the planes in registers at two waves per SIMD, rate 2/3 in LDS at one (DESIGN.md
// 4.20 has what each form compiles to).
// what a CU must hold: the waves the kernel is compiled for, each with the soft layout's LDS
template <int CODE>
constexpr bool quantised_soft_lds_fits() { return 4 * BsPlan<CODE>::SOFT_WAVES_PER_SIMD * Geo<CODE>::LDS_BYTES_SOFT <= 163840; }
static_assert(quantised_soft_lds_fits<TM1536>() && quantised_soft_lds_fits<TM2048>() && quantised_soft_lds_fits<TM6144>() &&
              quantised_soft_lds_fits<TM8192>(), "waves per CU the f32-reading soft kernels are compiled for x LDS per wave <= 160 KB");

// the plain form: decode_ms_bsa_kernel<CODE> on f32 rows
template <int CODE>
__global__ void __launch_bounds__(64, BsPlan<CODE>::SOFT_WAVES_PER_SIMD)
decode_ms_bsqa_kernel(const float *__restrict__ llrs, int8_t *__restrict__ app, uint8_t *__restrict__ output, uint32_t *__restrict__ iters,
                      uint8_t *__restrict__ success, uint32_t batch, uint32_t maxiters, uint32_t ngroups, float scale, float lim)
{
    __shared__ __attribute__((aligned(16))) char lds[Geo<CODE>::LDS_BYTES_SOFT];
    HipBackend b{lds};
    init_kernel<CODE, HipBackend>(b);
    for (uint32_t g = blockIdx.x; g < ngroups; g += gridDim.x)
        decode_group<CODE, HipBackend, false, 8, true, QuantisedF32>(b, llrs, output, iters, success, batch, maxiters, g, 1, 0, 0, app,
                                                                     QuantisedF32{scale, lim});
}

// the corrected form, MULBITS 0 / 4 / 8: decode_ms_bsca_kernel<CODE, MULBITS> on f32 rows
template <int CODE, int MULBITS>
__global__ void __launch_bounds__(64, BsPlan<CODE>::SOFT_WAVES_PER_SIMD)
decode_ms_bsqca_kernel(const float *__restrict__ llrs, int8_t *__restrict__ app, uint8_t *__restrict__ output, uint32_t *__restrict__ iters,
                       uint8_t *__restrict__ success, uint32_t batch, uint32_t maxiters, uint32_t ngroups, float scale, float lim,
                       uint32_t scale_num, uint32_t scale_shift, uint32_t offset)
{
    __shared__ __attribute__((aligned(16))) char lds[Geo<CODE>::LDS_BYTES_SOFT];
    HipBackend b{lds};
    init_kernel<CODE, HipBackend>(b);
    for (uint32_t g = blockIdx.x; g < ngroups; g += gridDim.x)
        decode_group<CODE, HipBackend, true, MULBITS, true, QuantisedF32>(b, llrs, output, iters, success, batch, maxiters, g, scale_num,
                                                                          scale_shift, offset, app, QuantisedF32{scale, lim});
}

// one group of G codewords per workgroup, the hardware dispatcher hands them out (launch_lockstep of decode_ms_bs.hip)
template <auto KERNEL, int G, class... Extra>
hipError_t launch_lockstep_quantised_soft(const float *llrs, int8_t *app, uint8_t *output, uint32_t *iters, uint8_t *success, size_t batch,
                                          uint32_t maxiters, hipStream_t stream, Extra... extra)
{
    if (batch == 0) return hipSuccess;
    if (batch > 0xFFFFFFFFull) return hipErrorInvalidValue;
    const size_t groups = (batch + G - 1) / G;
    const size_t grid = groups < 0x7FFFFFFFull ? groups : 0x7FFFFFFFull;
    hipLaunchKernelGGL(KERNEL, dim3((unsigned)grid), dim3(64), 0, stream, llrs, app, output, iters, success, (uint32_t)batch, maxiters,
                       (uint32_t)groups, extra...);
    return hipGetLastError();
}

// the codes THIS compile unit builds (BsPlan::UNIT); hipErrorInvalidConfiguration for every other code.  `corrected` chooses the form
// with the correction step, in the width the call's scale needs (correction_mulbits); else the triple is not read.
static hipError_t launch_quantised_soft_in_unit(int code, const float *llrs, int8_t *app, uint8_t *output, uint32_t *iters, uint8_t *success,
                                                size_t batch, uint32_t maxiters, float scale, float lim, bool corrected, uint32_t scale_num,
                                                uint32_t scale_shift, uint32_t offset, hipStream_t stream)
{
    auto form = [&](auto C_, auto M_) {
        constexpr int CODE = decltype(C_)::value, MULBITS = decltype(M_)::value;
        return launch_lockstep_quantised_soft<decode_ms_bsqca_kernel<CODE, MULBITS>, BsPlan<CODE>::G>(llrs, app, output, iters, success, batch,
                                                                                                       maxiters, stream, scale, lim, scale_num,
                                                                                                       scale_shift, offset);
    };
    auto built_here = [&](auto C_) {
        constexpr int CODE = decltype(C_)::value;
        if constexpr (BsPlan<CODE>::UNIT != BS_TU) return hipErrorInvalidConfiguration;
        else {
            if (!corrected)
                return launch_lockstep_quantised_soft<decode_ms_bsqa_kernel<CODE>, BsPlan<CODE>::G>(llrs, app, output, iters, success, batch,
                                                                                                    maxiters, stream, scale, lim);
            switch (correction_mulbits(scale_num, scale_shift)) {
                case 0: return form(C_, IC<0>{});
                case 4: return form(C_, IC<4>{});
                default: return form(C_, IC<8>{});
            }
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
#endif

hipError_t launch_decode_ms_bitsliced_quantised_soft_unit2(int code, const float *llrs, int8_t *app, uint8_t *output, uint32_t *iters,
                                                           uint8_t *success, size_t batch, uint32_t maxiters, float scale, float lim,
                                                           bool corrected, uint32_t scale_num, uint32_t scale_shift, uint32_t offset,
                                                           hipStream_t stream);
#if BS_TU == 2
hipError_t launch_decode_ms_bitsliced_quantised_soft_unit2(int code, const float *llrs, int8_t *app, uint8_t *output, uint32_t *iters,
                                                           uint8_t *success, size_t batch, uint32_t maxiters, float scale, float lim,
                                                           bool corrected, uint32_t scale_num, uint32_t scale_shift, uint32_t offset,
                                                           hipStream_t stream)
{
#if BS_PLANES == 8
    return bs::launch_quantised_soft_in_unit(code, llrs, app, output, iters, success, batch, maxiters, scale, lim, corrected, scale_num,
                                             scale_shift, offset, stream);
#else
    return hipErrorInvalidConfiguration;
#endif
}
#else
namespace {
hipError_t launch_quantised_soft(int code, const float *llrs, int8_t *app, uint8_t *output, uint32_t *iters, uint8_t *success, size_t batch,
                                 uint32_t maxiters, float scale, float lim, bool corrected, uint32_t scale_num, uint32_t scale_shift,
                                 uint32_t offset, hipStream_t stream)
{
#if BS_PLANES == 8
    if (!bs::bitsliced_soft_code(code)) return hipErrorInvalidConfiguration;
    if (bs::BS_DISPATCH[code].unit == BS_TU)
        return bs::launch_quantised_soft_in_unit(code, llrs, app, output, iters, success, batch, maxiters, scale, lim, corrected, scale_num,
                                                 scale_shift, offset, stream);
    return launch_decode_ms_bitsliced_quantised_soft_unit2(code, llrs, app, output, iters, success, batch, maxiters, scale, lim, corrected,
                                                           scale_num, scale_shift, offset, stream);
#else
    return hipErrorInvalidConfiguration;                       // (a 16-plane experiment build carries no f32 loader)
#endif
}
}  // namespace

hipError_t launch_decode_ms_bitsliced_quantised_soft(int code, const float *llrs, int8_t *app, uint8_t *output, uint32_t *iters,
                                                     uint8_t *success, size_t batch, uint32_t maxiters, float scale, int lim, hipStream_t stream)
{
    return launch_quantised_soft(code, llrs, app, output, iters, success, batch, maxiters, scale, (float)lim, false, 1, 0, 0, stream);
}

hipError_t launch_decode_ms_bitsliced_quantised_corrected_soft(int code, const float *llrs, int8_t *app, uint8_t *output, uint32_t *iters,
                                                               uint8_t *success, size_t batch, uint32_t maxiters, float scale, int lim,
                                                               uint32_t scale_num, uint32_t scale_shift, uint32_t offset, hipStream_t stream)
{
    return launch_quantised_soft(code, llrs, app, output, iters, success, batch, maxiters, scale, (float)lim, true, scale_num, scale_shift, offset,
                                 stream);
}
#endif

}  // namespace ldpc
