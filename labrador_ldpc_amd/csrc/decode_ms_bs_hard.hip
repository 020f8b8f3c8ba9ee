// decode_ms_bs_hard.hip -- gfx950 instantiation of the bit-sliced i8 min-sum decoder READING PACKED HARD DECISIONS
// (decode_ms_bitslice.hpp, load_column_planes<..., PackedHard>) for the one-wave TM codes -- TM1536, TM2048, TM6144,
// TM8192 -- and its launchers.
//
// The decoders of decode_ms_bs.hip (plain) and decode_ms_bs_corrected.hip (normalized / offset check messages) with one thing changed:
// the loader's source.  The rows are packed bits, [batch][n / 8] MSB first, with an optional row of erasure bits per frame; the loader
// builds the eight planes of the i8 frame e -- e[j] = 0 where erased, else -magnitude where the bit is set, else +magnitude -- from the
// sign word itself: no byte slab, no byte gather, no transpose.  Everything behind the planes -- the LLR planes in LDS, the iteration,
// the epilogue -- is the i8 kernels' text.  Per frame the results are those of the i8 kernel on e, bit for bit, without an expanded
// copy of the batch.
// Lockstep forms only, at every batch size: no slot refill, no two-wave form (TM1280, TM5120), no soft output.
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

// the plain form: launch bounds of decode_ms_bs_kernel<CODE>
template <int CODE>
__global__ void __launch_bounds__(64, BsPlan<CODE>::WAVES_PER_SIMD)
decode_ms_bsh_kernel(const uint8_t *__restrict__ input, uint8_t *__restrict__ output, uint32_t *__restrict__ iters, uint8_t *__restrict__ success,
                     uint32_t batch, uint32_t maxiters, uint32_t ngroups, const uint8_t *__restrict__ erasures, uint32_t magnitude)
{
    __shared__ __attribute__((aligned(16))) char lds[Geo<CODE>::LDS_BYTES];
    HipBackend b{lds};
    init_kernel<CODE, HipBackend>(b);
    for (uint32_t g = blockIdx.x; g < ngroups; g += gridDim.x)
        decode_group<CODE, HipBackend, false, 8, false, PackedHard>(b, input, output, iters, success, batch, maxiters, g, 1, 0, 0, nullptr,
                                                                    PackedHard{magnitude, erasures});
}

// the corrected form, MULBITS 0 / 4 / 8 and launch bounds as decode_ms_bsc_kernel<CODE, MULBITS>
template <int CODE, int MULBITS>
__global__ void __launch_bounds__(64, (corrected_waves_per_simd<CODE, MULBITS>()))
decode_ms_bshc_kernel(const uint8_t *__restrict__ input, uint8_t *__restrict__ output, uint32_t *__restrict__ iters, uint8_t *__restrict__ success,
                      uint32_t batch, uint32_t maxiters, uint32_t ngroups, const uint8_t *__restrict__ erasures, uint32_t magnitude,
                      uint32_t scale_num, uint32_t scale_shift, uint32_t offset)
{
    __shared__ __attribute__((aligned(16))) char lds[Geo<CODE>::LDS_BYTES];
    HipBackend b{lds};
    init_kernel<CODE, HipBackend>(b);
    for (uint32_t g = blockIdx.x; g < ngroups; g += gridDim.x)
        decode_group<CODE, HipBackend, true, MULBITS, false, PackedHard>(b, input, output, iters, success, batch, maxiters, g, scale_num, scale_shift,
                                                                         offset, nullptr, PackedHard{magnitude, erasures});
}

// The packed-bit-reading form (decode_ms_bs_launch.hpp): the one-wave codes.  `corrected` chooses the kernel with the correction step,
// in the width the call's scale needs; else the triple is not read.  erasures: nullptr = no mask.
struct HardForm {
    static constexpr bool I8_ONLY = true;
    struct Args {
        const uint8_t *input, *erasures; uint8_t *output; uint32_t *iters; uint8_t *success; size_t batch; uint32_t maxiters, magnitude;
        bool corrected; uint32_t scale_num, scale_shift, offset; hipStream_t stream;
    };
    using Codes = OneWaveCodes;
    template <int CODE>
    static hipError_t launch(const Args &a)
    {
        constexpr int G = BsPlan<CODE>::G;
        const std::tuple lead{a.input, a.output, a.iters, a.success};
        if (!a.corrected) return launch_lockstep<decode_ms_bsh_kernel<CODE>, 64, G>(a.stream, a.batch, a.maxiters, lead, a.erasures, a.magnitude);
        return for_mulbits(a.scale_num, a.scale_shift, [&](auto M_) {
            return launch_lockstep<decode_ms_bshc_kernel<CODE, decltype(M_)::value>, 64, G>(a.stream, a.batch, a.maxiters, lead, a.erasures, a.magnitude,
                                                                                            a.scale_num, a.scale_shift, a.offset);
        });
    }
};

}  // namespace bs
#endif

#if BS_TU == 2
#if BS_PLANES == 8
template hipError_t bs::launch_in_unit2<bs::HardForm>(int, const bs::HardForm::Args &);
#endif
#else
namespace {
hipError_t launch_hard(int code, const uint8_t *input, const uint8_t *erasures, uint8_t *output, uint32_t *iters, uint8_t *success, size_t batch,
                       uint32_t maxiters, uint32_t magnitude, bool corrected, uint32_t scale_num, uint32_t scale_shift, uint32_t offset,
                       hipStream_t stream)
{
#if BS_PLANES == 8
    return bs::launch_form<bs::HardForm>(code, {input, erasures, output, iters, success, batch, maxiters, magnitude, corrected, scale_num, scale_shift, offset, stream});
#else
    return hipErrorInvalidConfiguration;                       // (a 16-plane experiment build carries no packed loader)
#endif
}
}  // namespace

hipError_t launch_decode_ms_bitsliced_hard(int code, const uint8_t *input, const uint8_t *erasures, uint8_t *output, uint32_t *iters,
                                           uint8_t *success, size_t batch, uint32_t maxiters, uint32_t magnitude, hipStream_t stream)
{
    return launch_hard(code, input, erasures, output, iters, success, batch, maxiters, magnitude, false, 1, 0, 0, stream);
}

hipError_t launch_decode_ms_bitsliced_hard_corrected(int code, const uint8_t *input, const uint8_t *erasures, uint8_t *output, uint32_t *iters,
                                                     uint8_t *success, size_t batch, uint32_t maxiters, uint32_t magnitude, uint32_t scale_num,
                                                     uint32_t scale_shift, uint32_t offset, hipStream_t stream)
{
    return launch_hard(code, input, erasures, output, iters, success, batch, maxiters, magnitude, true, scale_num, scale_shift, offset, stream);
}
#endif

}  // namespace ldpc
