// decode_ms_flooding_corrected.hpp -- the f32 flooding decoders with normalized / offset check messages: the kernels
// of decode_ms_kernel.hpp and decode_ms_pair.hpp with their CORRECTED step, under names of their own, and their launchers.  Included
// only by decode_ms_flooding_corrected_f32.hip, so that every other object holds exactly the kernels it held.
//
// One kernel per code and output form, valid at every max_iters -- the fewest that meet the contract, not the fastest:
//   * the code's default f32 kernel: lean_mode(), the default indices per thread of decode_ms_tables.hpp, the pair kernel for TM8192;
//   * ONE form of the self-correction: 3 (v_mul_legacy + v_add + v_med3) where the kernel has a clamp-free loop, the kernel's own
//     otherwise.  The plain launcher's form 2 and the multiply form of the bounded test both need every nonzero value of a decode
//     to be at least 2^-43 (Ops<float>::self_correct_b), which a corrected magnitude is not: scale * m - offset can be any positive
//     float, a denormal included.  Form 3 asks only that nothing is NaN or infinite, and corrected magnitudes never exceed the
//     uncorrected ones, so the clamp-free loop's range vote (nocap_limit_for(max_iters, false)) holds as it stands;
//   * NaN LLRs in line (NANPASS 0), also for TM5120 and TM1280, whose plain launches take two passes over large batches;
//   * no notify form.
#pragma once

#include "decode_ms_launch.hpp"

namespace ldpc {

template <int CODE, int IPT, int LEAN>
constexpr int flooding_corrected_form()
{
    return has_nocap_loop<CODE, float, IPT, LEAN>() ? 3 : selfcorr_med3<CODE, float>();
}

template <int CODE, int IPT, int LEAN, int FORM, bool SOFT>
__global__ void __launch_bounds__((Geometry<CODE, float, IPT>::WG), (min_waves_per_simd<CODE, float, IPT, LEAN>()))
decode_ms_flooding_corrected_kernel(const float *__restrict__ llrs, float *__restrict__ app, uint8_t *__restrict__ output,
                                    uint32_t *__restrict__ iters_out, uint8_t *__restrict__ success_out,
                                    uint32_t batch, uint32_t maxiters, float nocap_limit, uint32_t *claim, uint32_t claim_k,
                                    float scale, float offset)
{
    decode_ms_kernel_main<CODE, float, IPT, LEAN, FORM, 0, SOFT, true>(llrs, output, iters_out, success_out, batch, maxiters, nocap_limit,
                                                                       claim, claim_k, app, scale, offset);
}

template <int CODE, bool SOFT>
__global__ void __launch_bounds__((PairGeometry<CODE, float>::NT))
decode_ms_pair_flooding_corrected_kernel(const float *__restrict__ llrs, float *__restrict__ app, uint8_t *__restrict__ output,
                                         uint32_t *__restrict__ iters_out, uint8_t *__restrict__ success_out, uint32_t batch,
                                         uint32_t maxiters, float nocap_limit, uint32_t *claim, float scale, float offset)
{
    using GEO = PairGeometry<CODE, float>;
    __shared__ __attribute__((aligned(16))) char lds[GEO::LDS_BYTES];
    const int jw = __builtin_amdgcn_readfirstlane((int)threadIdx.x) / (GEO::M / 8);          // quarter of this wave's indices
    if (jw == 0) decode_ms_pair_body<CODE, float, 0, 3, SOFT, true>(llrs, output, iters_out, success_out, batch, maxiters, nocap_limit, claim, lds, app, scale, offset);
    else if (jw == 1) decode_ms_pair_body<CODE, float, 1, 3, SOFT, true>(llrs, output, iters_out, success_out, batch, maxiters, nocap_limit, claim, lds, app, scale, offset);
    else if (jw == 2) decode_ms_pair_body<CODE, float, 2, 3, SOFT, true>(llrs, output, iters_out, success_out, batch, maxiters, nocap_limit, claim, lds, app, scale, offset);
    else decode_ms_pair_body<CODE, float, 3, 3, SOFT, true>(llrs, output, iters_out, success_out, batch, maxiters, nocap_limit, claim, lds, app, scale, offset);
}

// The launch of launch_cfg_form() / launch_pair_form() (decode_ms_launch.hpp) for the kernels above: the same persistent grid, the
// same queue for workgroups of eight waves and more, the fixed stride below that.  app == nullptr launches the hard form.
template <int CODE, int IPT, bool SOFT>
hipError_t launch_flooding_corrected(const float *llrs, float *app, uint8_t *output, uint32_t *iters, uint8_t *success, size_t batch,
                                     uint32_t maxiters, float scale, float offset, hipStream_t stream)
{
    if (batch == 0) return hipSuccess;
    if constexpr (CODE == TM8192) {
        static_assert(IPT == 2, "TM8192: the pair kernel owns two indices per thread");
        using GEO = PairGeometry<CODE, float>;
        if (batch > 0x7FFFFFFFull) return hipErrorInvalidValue;
        constexpr auto KERNEL = decode_ms_pair_flooding_corrected_kernel<CODE, SOFT>;
        const size_t resident = resident_workgroups<KERNEL, GEO::NT>();
        uint32_t *claim = maxiters == 0 ? nullptr : claim_counter(stream);
        const size_t grid = persistent_grid(resident, claim != nullptr, batch);
        hipLaunchKernelGGL(KERNEL, dim3((unsigned)grid), dim3(GEO::NT), 0, stream, llrs, app, output, iters, success, (uint32_t)batch,
                           maxiters, nocap_limit_for(maxiters, false), claim, scale, offset);
        return hipGetLastError();
    } else {
        constexpr int LEAN = lean_mode<CODE, float, IPT>();
        using GEO = Geometry<CODE, float, IPT>;
        const size_t groups = (batch + GEO::G - 1) / GEO::G;
        if (batch > 0xFFFFFFFFull || groups > 0x7FFFFFFFull) return hipErrorInvalidValue;   // (capi.hip slices larger batches)
        constexpr auto KERNEL = decode_ms_flooding_corrected_kernel<CODE, IPT, LEAN, flooding_corrected_form<CODE, IPT, LEAN>(), SOFT>;
        const size_t resident = resident_workgroups<KERNEL, GEO::WG>();
        constexpr bool queue_fed = GEO::WG >= 512;
        uint32_t *claim = (maxiters == 0 || !queue_fed) ? nullptr : claim_counter(stream);
        size_t K = 1;
        if (claim != nullptr) {
            K = claim_chunk<CODE, float, IPT>();
            while (K > 1 && groups < 8 * K * resident) K /= 2;
        }
        const size_t grid = persistent_grid(resident, claim != nullptr, (groups + K - 1) / K);
        hipLaunchKernelGGL(KERNEL, dim3((unsigned)grid), dim3(GEO::WG), 0, stream, llrs, app, output, iters, success, (uint32_t)batch,
                           maxiters, nocap_limit_for(maxiters, false), claim, (uint32_t)K, scale, offset);
        return hipGetLastError();
    }
}

// The heavy instantiations are objects of their own (Makefile: -DFC_PART=1/2/3), part 0 holds the TC codes and the dispatch.
#define LDPC_FC_SIG (const float *, float *, uint8_t *, uint32_t *, uint8_t *, size_t, uint32_t, float, float, hipStream_t)
#define LDPC_FC_PART_1(X) X(TM8192, 2)
#define LDPC_FC_PART_2(X) X(TM5120, 1) X(TM6144, 1)
#define LDPC_FC_PART_3(X) X(TM1280, 1) X(TM1536, 1) X(TM2048, 1)

}  // namespace ldpc
