// decode_ms_bs_quantised.hip -- gfx950 instantiation of the bit-sliced i8 min-sum decoder READING F32 LLRs (decode_ms_bitslice.hpp,
// load_column_planes<..., QuantisedF32>) for the one-wave TM codes -- TM1536, TM2048, TM6144, TM8192 -- and its
// launchers.
//
// The decoders of decode_ms_bs.hip (plain) and decode_ms_bs_corrected.hip (normalized / offset check messages) with one thing changed:
// the loader's source.  The rows are f32; the loader quantises every LLR by the library's one rule (llr_quantise.hpp) at the call's
// (scale, lim) on its way into the staging slab, and everything behind the slab -- the bit transposes, the LLR planes in LDS, the
// iteration, the epilogue -- is the i8 kernels' text.  Per frame the results are those of the i8 kernel on the frame quantised by
// llr_quantise.hip, bit for bit, without a quantised copy of the batch.
// Lockstep forms only, at every batch size: no slot refill, no two-wave form (TM1280, TM5120), no soft output.
//
// Compiled per unit like decode_ms_bs.hip (Makefile, -DBS_TU, the same scheduler flags per unit) into objects of its own: every other
// object keeps exactly the kernels it had.
#include <hip/hip_runtime.h>
#include <cstdint>

#ifndef BS_TU
#error "decode_ms_bs_quantised.hip is compiled per unit: -DBS_TU=1 (rate 1/2 + dispatch) or -DBS_TU=2 (rate 2/3)"
#endif

#include "decode_ms_bitslice.hpp"
#include "decode_ms_protos.hpp"
#include "hip_backend.hpp"

namespace ldpc {
#if BS_PLANES == 8
namespace bs {

// the plain form: launch bounds of decode_ms_bs_kernel<CODE>
template <int CODE>
__global__ void __launch_bounds__(64, BsPlan<CODE>::WAVES_PER_SIMD)
decode_ms_bsq_kernel(const float *__restrict__ llrs, uint8_t *__restrict__ output, uint32_t *__restrict__ iters, uint8_t *__restrict__ success,
                     uint32_t batch, uint32_t maxiters, uint32_t ngroups, float scale, float lim)
{
    __shared__ __attribute__((aligned(16))) char lds[Geo<CODE>::LDS_BYTES];
    HipBackend b{lds};
    init_kernel<CODE, HipBackend>(b);
    for (uint32_t g = blockIdx.x; g < ngroups; g += gridDim.x)
        decode_group<CODE, HipBackend, false, 8, false, QuantisedF32>(b, llrs, output, iters, success, batch, maxiters, g, 1, 0, 0, nullptr,
                                                                      QuantisedF32{scale, lim});
}

// the corrected form, MULBITS 0 / 4 / 8 and launch bounds as decode_ms_bsc_kernel<CODE, MULBITS>
template <int CODE, int MULBITS>
__global__ void __launch_bounds__(64, (corrected_waves_per_simd<CODE, MULBITS>()))
decode_ms_bsqc_kernel(const float *__restrict__ llrs, uint8_t *__restrict__ output, uint32_t *__restrict__ iters, uint8_t *__restrict__ success,
                      uint32_t batch, uint32_t maxiters, uint32_t ngroups, float scale, float lim, uint32_t scale_num, uint32_t scale_shift,
                      uint32_t offset)
{
    __shared__ __attribute__((aligned(16))) char lds[Geo<CODE>::LDS_BYTES];
    HipBackend b{lds};
    init_kernel<CODE, HipBackend>(b);
    for (uint32_t g = blockIdx.x; g < ngroups; g += gridDim.x)
        decode_group<CODE, HipBackend, true, MULBITS, false, QuantisedF32>(b, llrs, output, iters, success, batch, maxiters, g, scale_num, scale_shift,
                                                                           offset, nullptr, QuantisedF32{scale, lim});
}

// one group of G codewords per workgroup, the hardware dispatcher hands them out (launch_lockstep of decode_ms_bs.hip)
template <auto KERNEL, int G, class... Extra>
hipError_t launch_lockstep_quantised(const float *llrs, uint8_t *output, uint32_t *iters, uint8_t *success, size_t batch, uint32_t maxiters,
                                     hipStream_t stream, Extra... extra)
{
    if (batch == 0) return hipSuccess;
    if (batch > 0xFFFFFFFFull) return hipErrorInvalidValue;
    const size_t groups = (batch + G - 1) / G;
    const size_t grid = groups < 0x7FFFFFFFull ? groups : 0x7FFFFFFFull;
    hipLaunchKernelGGL(KERNEL, dim3((unsigned)grid), dim3(64), 0, stream, llrs, output, iters, success, (uint32_t)batch, maxiters, (uint32_t)groups,
                       extra...);
    return hipGetLastError();
}

// the codes THIS compile unit builds (BsPlan::UNIT); hipErrorInvalidConfiguration for every other code.  `corrected` chooses the form
// with the correction step, in the width the call's scale needs (correction_mulbits); else the triple is not read.
static hipError_t launch_quantised_in_unit(int code, const float *llrs, uint8_t *output, uint32_t *iters, uint8_t *success, size_t batch,
                                           uint32_t maxiters, float scale, float lim, bool corrected, uint32_t scale_num, uint32_t scale_shift,
                                           uint32_t offset, hipStream_t stream)
{
    auto form = [&](auto C_, auto M_) {
        constexpr int CODE = decltype(C_)::value, MULBITS = decltype(M_)::value;
        return launch_lockstep_quantised<decode_ms_bsqc_kernel<CODE, MULBITS>, BsPlan<CODE>::G>(llrs, output, iters, success, batch, maxiters, stream,
                                                                                                 scale, lim, scale_num, scale_shift, offset);
    };
    auto built_here = [&](auto C_) {
        constexpr int CODE = decltype(C_)::value;
        if constexpr (BsPlan<CODE>::UNIT != BS_TU) return hipErrorInvalidConfiguration;
        else {
            if (!corrected)
                return launch_lockstep_quantised<decode_ms_bsq_kernel<CODE>, BsPlan<CODE>::G>(llrs, output, iters, success, batch, maxiters, stream,
                                                                                              scale, lim);
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

hipError_t launch_decode_ms_bitsliced_quantised_unit2(int code, const float *llrs, uint8_t *output, uint32_t *iters, uint8_t *success, size_t batch,
                                                      uint32_t maxiters, float scale, float lim, bool corrected, uint32_t scale_num,
                                                      uint32_t scale_shift, uint32_t offset, hipStream_t stream);
#if BS_TU == 2
hipError_t launch_decode_ms_bitsliced_quantised_unit2(int code, const float *llrs, uint8_t *output, uint32_t *iters, uint8_t *success, size_t batch,
                                                      uint32_t maxiters, float scale, float lim, bool corrected, uint32_t scale_num,
                                                      uint32_t scale_shift, uint32_t offset, hipStream_t stream)
{
#if BS_PLANES == 8
    return bs::launch_quantised_in_unit(code, llrs, output, iters, success, batch, maxiters, scale, lim, corrected, scale_num, scale_shift, offset,
                                        stream);
#else
    return hipErrorInvalidConfiguration;
#endif
}
#else
namespace {
hipError_t launch_quantised(int code, const float *llrs, uint8_t *output, uint32_t *iters, uint8_t *success, size_t batch, uint32_t maxiters,
                            float scale, float lim, bool corrected, uint32_t scale_num, uint32_t scale_shift, uint32_t offset, hipStream_t stream)
{
#if BS_PLANES == 8
    // (the one-wave lockstep codes: the soft form's four)
    if (!bs::bitsliced_soft_code(code)) return hipErrorInvalidConfiguration;
    if (bs::BS_DISPATCH[code].unit == BS_TU)
        return bs::launch_quantised_in_unit(code, llrs, output, iters, success, batch, maxiters, scale, lim, corrected, scale_num, scale_shift,
                                            offset, stream);
    return launch_decode_ms_bitsliced_quantised_unit2(code, llrs, output, iters, success, batch, maxiters, scale, lim, corrected, scale_num,
                                                      scale_shift, offset, stream);
#else
    return hipErrorInvalidConfiguration;                       // (a 16-plane experiment build carries no f32 loader)
#endif
}
}  // namespace

hipError_t launch_decode_ms_bitsliced_quantised(int code, const float *llrs, uint8_t *output, uint32_t *iters, uint8_t *success, size_t batch,
                                                uint32_t maxiters, float scale, int lim, hipStream_t stream)
{
    return launch_quantised(code, llrs, output, iters, success, batch, maxiters, scale, (float)lim, false, 1, 0, 0, stream);
}

hipError_t launch_decode_ms_bitsliced_quantised_corrected(int code, const float *llrs, uint8_t *output, uint32_t *iters, uint8_t *success,
                                                          size_t batch, uint32_t maxiters, float scale, int lim, uint32_t scale_num,
                                                          uint32_t scale_shift, uint32_t offset, hipStream_t stream)
{
    return launch_quantised(code, llrs, output, iters, success, batch, maxiters, scale, (float)lim, true, scale_num, scale_shift, offset, stream);
}
#endif

}  // namespace ldpc
