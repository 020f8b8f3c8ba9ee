// decode_ms_bs_corrected.hip -- gfx950 instantiation of the bit-sliced i8 min-sum decoder WITH normalized / offset check messages
// (decode_ms_bitslice.hpp, Decoder<..., CORRECTED = true>) for the TM codes, and its launcher.
//
// The decoder of decode_ms_bs.hip with one step added: once per iteration and block row, the row's two minima -- converted back from
// keys to magnitudes in Decoder::finish_row -- each become max(((scale_num * m + half) >> scale_shift) - offset, 0)
// (Decoder::correct_mag).  The triple is the caller's, the same for every wave of the launch.
// Lockstep forms only -- one wave per group (rate 1/2, rate 2/3), two waves per group (rate 4/5) -- at every batch size: no slot
// refill, no crossover to the f32-pipe kernels.
//
// Compiled per unit like decode_ms_bs.hip (Makefile, -DBS_TU, the same scheduler flags per unit) into objects of its own: the plain
// objects keep exactly the kernels they had.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "decode_ms_bitslice.hpp"
#include "decode_ms_bitslice_split.hpp"
#include "decode_ms_bs_launch.hpp"
#include "decode_ms_protos.hpp"
#include "hip_backend.hpp"

namespace ldpc {
namespace bs {

// MULBITS: the multiplier bits the form is built for (Decoder::correct_mag): 0 = the offset alone, 4, 8; the launcher picks the form
// from the call's scale (correction_mulbits).  Three kernels per code.  The rate of the 8-bit form -- any scale with more than four
// fractional bits -- has not been measured.
// Waves per SIMD a form is compiled for: corrected_waves_per_simd() (decode_ms_bs_plan.hpp).
template <int CODE, int MULBITS>
__global__ void __launch_bounds__(64, (corrected_waves_per_simd<CODE, MULBITS>()))
decode_ms_bsc_kernel(const int8_t *__restrict__ llrs, uint8_t *__restrict__ output, uint32_t *__restrict__ iters,
                     uint8_t *__restrict__ success, uint32_t batch, uint32_t maxiters, uint32_t ngroups, uint32_t scale_num,
                     uint32_t scale_shift, uint32_t offset)
{
    __shared__ __attribute__((aligned(16))) char lds[Geo<CODE>::LDS_BYTES];
    HipBackend b{lds};
    init_kernel<CODE, HipBackend>(b);
    for (uint32_t g = blockIdx.x; g < ngroups; g += gridDim.x)
        decode_group<CODE, HipBackend, true, MULBITS>(b, llrs, output, iters, success, batch, maxiters, g, scale_num, scale_shift, offset);
}

template <int CODE, int HALF, int MULBITS>
__device__ __forceinline__ void split_wave_corrected(char *lds, const int8_t *llrs, uint8_t *output, uint32_t *iters, uint8_t *success,
                                                     uint32_t batch, uint32_t maxiters, uint32_t ngroups, uint32_t scale_num,
                                                     uint32_t scale_shift, uint32_t offset)
{
    HipBackend b{lds + SplitLayout<CODE>::template priv<HALF>()};
    SplitGroup<CODE, HipBackend, HALF, true, MULBITS> g;
    g.init(b);
    g.set_correction(scale_num, scale_shift, offset);
    for (uint32_t grp = blockIdx.x; grp < ngroups; grp += gridDim.x)
        decode_group_split<CODE, HipBackend, HALF>(b, g, llrs, output, iters, success, batch, maxiters, grp, [] { __syncthreads(); });
}

template <int CODE, int MULBITS>
__global__ void __launch_bounds__(128, (corrected_waves_per_simd<CODE, MULBITS>()))
decode_ms_bsc_split_kernel(const int8_t *__restrict__ llrs, uint8_t *__restrict__ output, uint32_t *__restrict__ iters,
                           uint8_t *__restrict__ success, uint32_t batch, uint32_t maxiters, uint32_t ngroups, uint32_t scale_num,
                           uint32_t scale_shift, uint32_t offset)
{
    __shared__ __attribute__((aligned(16))) char lds[SplitLayout<CODE>::BYTES];
    if (__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) == 0)
        split_wave_corrected<CODE, 0, MULBITS>(lds, llrs, output, iters, success, batch, maxiters, ngroups, scale_num, scale_shift, offset);
    else
        split_wave_corrected<CODE, 1, MULBITS>(lds, llrs, output, iters, success, batch, maxiters, ngroups, scale_num, scale_shift, offset);
}

// The corrected form (decode_ms_bs_launch.hpp): one wave or two per group as the code's plan says, in the width the call's scale needs
struct CorrectedForm {
    static constexpr bool I8_ONLY = true;
    struct Args {
        const int8_t *llrs; uint8_t *output; uint32_t *iters; uint8_t *success; size_t batch; uint32_t maxiters;
        uint32_t scale_num, scale_shift, offset; hipStream_t stream;
    };
    using Codes = TmCodes;
    template <int CODE>
    static hipError_t launch(const Args &a)
    {
        using PLAN = BsPlan<CODE>;
        return for_mulbits(a.scale_num, a.scale_shift, [&](auto M_) {
            constexpr int MULBITS = decltype(M_)::value;
            const std::tuple lead{a.llrs, a.output, a.iters, a.success};
            if constexpr (PLAN::TWO_WAVES)
                return launch_lockstep<decode_ms_bsc_split_kernel<CODE, MULBITS>, 128, PLAN::G>(a.stream, a.batch, a.maxiters, lead, a.scale_num, a.scale_shift, a.offset);
            else return launch_lockstep<decode_ms_bsc_kernel<CODE, MULBITS>, 64, PLAN::G>(a.stream, a.batch, a.maxiters, lead, a.scale_num, a.scale_shift, a.offset);
        });
    }
};

}  // namespace bs

#if BS_TU == 2
template hipError_t bs::launch_in_unit2<bs::CorrectedForm>(int, const bs::CorrectedForm::Args &);
#else
hipError_t launch_decode_ms_bitsliced_corrected(int code, const int8_t *llrs, uint8_t *output, uint32_t *iters, uint8_t *success, size_t batch,
                                                uint32_t maxiters, uint32_t scale_num, uint32_t scale_shift, uint32_t offset,
                                                hipStream_t stream)
{
    return bs::launch_form<bs::CorrectedForm>(code, {llrs, output, iters, success, batch, maxiters, scale_num, scale_shift, offset, stream});
}
#endif

}  // namespace ldpc
