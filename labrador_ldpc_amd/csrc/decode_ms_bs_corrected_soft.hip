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

#include "decode_ms_bitslice.hpp"
#include "decode_ms_bs_launch.hpp"
#include "decode_ms_protos.hpp"
#include "hip_backend.hpp"

namespace ldpc {
namespace bs {

// Placement and launch bounds: the soft plan's (BsPlan::SOFT_LDS, SOFT_WAVES_PER_SIMD) for every form -- rate 1/2 keeps the planes in
// registers at two waves per SIMD, rate 2/3 in LDS at one (DESIGN.md 4.18 has what each form compiles to).
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

// The corrected soft form (decode_ms_bs_launch.hpp): the one-wave codes, in the width the call's scale needs
struct CorrectedSoftForm {
    static constexpr bool I8_ONLY = true;
    struct Args {
        const int8_t *llrs; int8_t *app; uint8_t *output; uint32_t *iters; uint8_t *success; size_t batch; uint32_t maxiters;
        uint32_t scale_num, scale_shift, offset; hipStream_t stream;
    };
    using Codes = OneWaveCodes;
    template <int CODE>
    static hipError_t launch(const Args &a)
    {
        return for_mulbits(a.scale_num, a.scale_shift, [&](auto M_) {
            return launch_lockstep<decode_ms_bsca_kernel<CODE, decltype(M_)::value>, 64, BsPlan<CODE>::G>(
                a.stream, a.batch, a.maxiters, std::tuple{a.llrs, a.app, a.output, a.iters, a.success}, a.scale_num, a.scale_shift, a.offset);
        });
    }
};

}  // namespace bs

#if BS_TU == 2
template hipError_t bs::launch_in_unit2<bs::CorrectedSoftForm>(int, const bs::CorrectedSoftForm::Args &);
#else
hipError_t launch_decode_ms_bitsliced_corrected_soft(int code, const int8_t *llrs, int8_t *app, uint8_t *output, uint32_t *iters,
                                                     uint8_t *success, size_t batch, uint32_t maxiters, uint32_t scale_num,
                                                     uint32_t scale_shift, uint32_t offset, hipStream_t stream)
{
    return bs::launch_form<bs::CorrectedSoftForm>(code, {llrs, app, output, iters, success, batch, maxiters, scale_num, scale_shift, offset, stream});
}
#endif

}  // namespace ldpc
