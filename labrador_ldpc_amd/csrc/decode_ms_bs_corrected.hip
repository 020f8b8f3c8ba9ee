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

#ifndef BS_TU
#error "decode_ms_bs_corrected.hip is compiled per unit: -DBS_TU=1 (rate 1/2 + dispatch) or -DBS_TU=2 (rate 2/3, rate 4/5)"
#endif

#include "decode_ms_bitslice.hpp"
#include "decode_ms_bitslice_split.hpp"
#include "decode_ms_protos.hpp"
#include "hip_backend.hpp"

namespace ldpc {
namespace bs {

static_assert(PL == 8, "the corrected form is built for i8 planes");

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

// one group of G codewords per workgroup, the hardware dispatcher hands them out (launch_lockstep of decode_ms_bs.hip)
template <auto KERNEL, int BLOCK, int G>
hipError_t launch_lockstep_corrected(const int8_t *llrs, uint8_t *output, uint32_t *iters, uint8_t *success, size_t batch, uint32_t maxiters,
                                     uint32_t scale_num, uint32_t scale_shift, uint32_t offset, hipStream_t stream)
{
    if (batch == 0) return hipSuccess;
    if (batch > 0xFFFFFFFFull) return hipErrorInvalidValue;
    const size_t groups = (batch + G - 1) / G;
    const size_t grid = groups < 0x7FFFFFFFull ? groups : 0x7FFFFFFFull;
    hipLaunchKernelGGL(KERNEL, dim3((unsigned)grid), dim3(BLOCK), 0, stream, llrs, output, iters, success, (uint32_t)batch, maxiters, (uint32_t)groups,
                       scale_num, scale_shift, offset);
    return hipGetLastError();
}

// the codes THIS compile unit builds (BsPlan::UNIT); hipErrorInvalidConfiguration for every other code
static hipError_t launch_corrected_in_unit(int code, const int8_t *llrs, uint8_t *output, uint32_t *iters, uint8_t *success, size_t batch,
                                           uint32_t maxiters, uint32_t scale_num, uint32_t scale_shift, uint32_t offset, hipStream_t stream)
{
    auto form = [&](auto C_, auto M_) {
        constexpr int CODE = decltype(C_)::value, MULBITS = decltype(M_)::value;
        using PLAN = BsPlan<CODE>;
        if constexpr (PLAN::UNIT != BS_TU) return hipErrorInvalidConfiguration;
        else if constexpr (PLAN::TWO_WAVES)
            return launch_lockstep_corrected<decode_ms_bsc_split_kernel<CODE, MULBITS>, 128, PLAN::G>(llrs, output, iters, success, batch, maxiters,
                                                                                                       scale_num, scale_shift, offset, stream);
        else
            return launch_lockstep_corrected<decode_ms_bsc_kernel<CODE, MULBITS>, 64, PLAN::G>(llrs, output, iters, success, batch, maxiters,
                                                                                                scale_num, scale_shift, offset, stream);
    };
    auto built_here = [&](auto C_) {
        switch (correction_mulbits(scale_num, scale_shift)) {
            case 0: return form(C_, IC<0>{});
            case 4: return form(C_, IC<4>{});
            default: return form(C_, IC<8>{});
        }
    };
    switch (code) {
        case TM1280: return built_here(IC<TM1280>{});
        case TM1536: return built_here(IC<TM1536>{});
        case TM2048: return built_here(IC<TM2048>{});
        case TM5120: return built_here(IC<TM5120>{});
        case TM6144: return built_here(IC<TM6144>{});
        case TM8192: return built_here(IC<TM8192>{});
        default: return hipErrorInvalidConfiguration;
    }
}

}  // namespace bs

hipError_t launch_decode_ms_bitsliced_corrected_unit2(int code, const int8_t *llrs, uint8_t *output, uint32_t *iters, uint8_t *success,
                                                      size_t batch, uint32_t maxiters, uint32_t scale_num, uint32_t scale_shift,
                                                      uint32_t offset, hipStream_t stream);
#if BS_TU == 2
hipError_t launch_decode_ms_bitsliced_corrected_unit2(int code, const int8_t *llrs, uint8_t *output, uint32_t *iters, uint8_t *success,
                                                      size_t batch, uint32_t maxiters, uint32_t scale_num, uint32_t scale_shift,
                                                      uint32_t offset, hipStream_t stream)
{
    return bs::launch_corrected_in_unit(code, llrs, output, iters, success, batch, maxiters, scale_num, scale_shift, offset, stream);
}
#else
hipError_t launch_decode_ms_bitsliced_corrected(int code, const int8_t *llrs, uint8_t *output, uint32_t *iters, uint8_t *success, size_t batch,
                                                uint32_t maxiters, uint32_t scale_num, uint32_t scale_shift, uint32_t offset,
                                                hipStream_t stream)
{
    if (!bs::bitsliced_code(code)) return hipErrorInvalidConfiguration;
    if (bs::BS_DISPATCH[code].unit == BS_TU)
        return bs::launch_corrected_in_unit(code, llrs, output, iters, success, batch, maxiters, scale_num, scale_shift, offset, stream);
    return launch_decode_ms_bitsliced_corrected_unit2(code, llrs, output, iters, success, batch, maxiters, scale_num, scale_shift, offset, stream);
}
#endif

}  // namespace ldpc
