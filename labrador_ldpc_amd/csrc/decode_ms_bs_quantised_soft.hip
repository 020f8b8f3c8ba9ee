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

#include "decode_ms_bitslice.hpp"
#include "decode_ms_bs_launch.hpp"
#include "decode_ms_protos.hpp"
#include "hip_backend.hpp"

namespace ldpc {
#if BS_PLANES == 8
namespace bs {

// Placement and launch bounds: the soft plan's (BsPlan::SOFT_LDS, SOFT_WAVES_PER_SIMD) for every form, as in
// decode_ms_bs_corrected_soft.hip -- rate 1/2 keeps the planes in registers at two waves per SIMD, rate 2/3 in LDS at one (DESIGN.md
// 4.20 has what each form compiles to).
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

// The f32-reading soft form (decode_ms_bs_launch.hpp): the one-wave codes.  `corrected` chooses the kernel with the correction step, in
// the width the call's scale needs; else the triple is not read.
struct QuantisedSoftForm {
    static constexpr bool I8_ONLY = true;
    struct Args {
        const float *llrs; int8_t *app; uint8_t *output; uint32_t *iters; uint8_t *success; size_t batch; uint32_t maxiters; float scale, lim;
        bool corrected; uint32_t scale_num, scale_shift, offset; hipStream_t stream;
    };
    using Codes = OneWaveCodes;
    template <int CODE>
    static hipError_t launch(const Args &a)
    {
        constexpr int G = BsPlan<CODE>::G;
        const std::tuple lead{a.llrs, a.app, a.output, a.iters, a.success};
        if (!a.corrected) return launch_lockstep<decode_ms_bsqa_kernel<CODE>, 64, G>(a.stream, a.batch, a.maxiters, lead, a.scale, a.lim);
        return for_mulbits(a.scale_num, a.scale_shift, [&](auto M_) {
            return launch_lockstep<decode_ms_bsqca_kernel<CODE, decltype(M_)::value>, 64, G>(a.stream, a.batch, a.maxiters, lead, a.scale, a.lim, a.scale_num,
                                                                                             a.scale_shift, a.offset);
        });
    }
};

}  // namespace bs
#endif

#if BS_TU == 2
#if BS_PLANES == 8
template hipError_t bs::launch_in_unit2<bs::QuantisedSoftForm>(int, const bs::QuantisedSoftForm::Args &);
#endif
#else
namespace {
hipError_t launch_quantised_soft(int code, const float *llrs, int8_t *app, uint8_t *output, uint32_t *iters, uint8_t *success, size_t batch,
                                 uint32_t maxiters, float scale, float lim, bool corrected, uint32_t scale_num, uint32_t scale_shift,
                                 uint32_t offset, hipStream_t stream)
{
#if BS_PLANES == 8
    return bs::launch_form<bs::QuantisedSoftForm>(code, {llrs, app, output, iters, success, batch, maxiters, scale, lim, corrected, scale_num, scale_shift, offset, stream});
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
