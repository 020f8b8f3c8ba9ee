// decode_ms_bs_launch.hpp -- the one lockstep launch path of the bit-sliced i8 min-sum kernels: what the seven decode_ms_bs*.hip files
// (plain, corrected, soft, corrected soft, f32-reading, f32-reading soft, packed-hard-reading) share around their kernels.  Host text.
//
// A file describes its FORM and this header does the rest:
//     struct Form {
//         static constexpr bool I8_ONLY = ...;                         // false: the text compiles with 16 planes as well (the plain form)
//         struct Args { ... };                                         // the form's arguments, stated once
//         using Codes = TmCodes / OneWaveCodes;                        // the codes the form exists for
//         template <int CODE> static hipError_t launch(const Args &);  // which kernel, which block size: launch_lockstep<...>
//     };
// launch_form<Form>(code, args) -- called by the file's public launch_decode_ms_bitsliced* functions in its unit-1 compile -- takes the
// call to the compile unit that builds the code's kernels (BsPlan::UNIT; the Makefile compiles every file twice, -DBS_TU=1 / 2):
// this one, or unit 2 through launch_in_unit2<Form>, which the file's unit-2 compile instantiates explicitly:
//     #if BS_TU == 2
//     template hipError_t ldpc::bs::launch_in_unit2<ldpc::bs::Form>(int, const ldpc::bs::Form::Args &);
//     #endif
//
// Every template here but launch_in_unit2 is `static`: the two compiles of a file give the same names different bodies (BS_TU), which
// must not meet at link time.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>
#include <tuple>

#include "decode_ms_bitslice.hpp"           // IC, correction_mulbits, Geo (LDS_BYTES_SOFT); BsPlan through decode_ms_bs_plan.hpp

#ifndef BS_TU
#error "the bit-sliced kernels' files are compiled per unit: -DBS_TU=1 (rate 1/2 + dispatch) or -DBS_TU=2 (rate 2/3, rate 4/5)"
#endif

namespace ldpc {
namespace bs {

template <int... CODES> struct CodeList {};
using TmCodes = CodeList<TM1280, TM1536, TM2048, TM5120, TM6144, TM8192>;         // bitsliced_code()
using OneWaveCodes = CodeList<TM1536, TM2048, TM6144, TM8192>;                    // bitsliced_soft_code()

// what a CU must hold of the soft forms: the waves the kernel is compiled for, each with the soft layout's LDS
template <int... CODES>
constexpr bool soft_lds_fits(CodeList<CODES...>) { return ((4 * BsPlan<CODES>::SOFT_WAVES_PER_SIMD * Geo<CODES>::LDS_BYTES_SOFT <= 163840) && ...); }
static_assert(PL != 8 || soft_lds_fits(OneWaveCodes{}), "waves per CU the soft kernels are compiled for x LDS per wave <= 160 KB");

// lockstep: one group of G codewords per workgroup of BLOCK threads (64: one wave per group, 128: two), the hardware dispatcher hands
// them out.  KERNEL(lead..., batch, maxiters, ngroups, trail...)
template <auto KERNEL, int BLOCK, int G, class... Lead, class... Trail>
static hipError_t launch_lockstep(hipStream_t stream, size_t batch, uint32_t maxiters, const std::tuple<Lead...> &lead, Trail... trail)
{
    if (batch == 0) return hipSuccess;
    if (batch > 0xFFFFFFFFull) return hipErrorInvalidValue;
    const size_t groups = (batch + G - 1) / G;
    const size_t grid = groups < 0x7FFFFFFFull ? groups : 0x7FFFFFFFull;
    std::apply([&](Lead... l) { hipLaunchKernelGGL(KERNEL, dim3((unsigned)grid), dim3(BLOCK), 0, stream, l..., (uint32_t)batch, maxiters, (uint32_t)groups, trail...); },
               lead);
    return hipGetLastError();
}

// f(IC<CODE>) for the code of the list that is `code` and that THIS compile unit builds (BsPlan::UNIT); hipErrorInvalidConfiguration
// for every other code
template <int... CODES, class F>
static hipError_t for_code_built_here(CodeList<CODES...>, int code, F &&f)
{
    hipError_t e = hipErrorInvalidConfiguration;
    auto one = [&](auto C_) {
        constexpr int CODE = decltype(C_)::value;
        if constexpr (BsPlan<CODE>::UNIT == BS_TU) {
            if (code == CODE) e = f(C_);
        }
    };
    (one(IC<CODES>{}), ...);
    return e;
}

// f(IC<MULBITS>) for the multiplier bits the call's scale needs: the width a corrected form is built in (correction_mulbits)
template <class F>
static hipError_t for_mulbits(uint32_t scale_num, uint32_t scale_shift, F &&f)
{
    switch (correction_mulbits(scale_num, scale_shift)) {
        case 0: return f(IC<0>{});
        case 4: return f(IC<4>{});
        default: return f(IC<8>{});
    }
}

// Every form but the plain one is written for i8 planes (FORM::I8_ONLY): a 16-plane experiment build (tools/bs_alt_build.sh,
// -DBS_PLANES=16) compiles the plain file alone.  (The two f32-reading files compile there as well, to entries that return
// hipErrorInvalidConfiguration: #if BS_PLANES == 8 around their kernels and forms.)
template <class FORM>
static hipError_t launch_in_this_unit(int code, const typename FORM::Args &a)
{
    static_assert(PL == 8 || !FORM::I8_ONLY, "this form of the bit-sliced kernels is built for i8 planes");
    return for_code_built_here(typename FORM::Codes{}, code, [&](auto C_) { return FORM::template launch<decltype(C_)::value>(a); });
}

// the bridge from unit 1 to unit 2: declared for both, defined and instantiated (explicitly, by the form's file) in unit 2 alone
template <class FORM>
hipError_t launch_in_unit2(int code, const typename FORM::Args &a);
#if BS_TU == 2
template <class FORM>
hipError_t launch_in_unit2(int code, const typename FORM::Args &a) { return launch_in_this_unit<FORM>(code, a); }
#else
// unit 1's front of a form: a code outside the form's list -> hipErrorInvalidConfiguration
template <class FORM>
static hipError_t launch_form(int code, const typename FORM::Args &a)
{
    if (!bitsliced_code(code)) return hipErrorInvalidConfiguration;
    if (BS_DISPATCH[code].unit == BS_TU) return launch_in_this_unit<FORM>(code, a);
    // (a 16-plane experiment build carries the rate-1/2 codes only: those of unit 1)
    if constexpr (PL != 8) return hipErrorInvalidConfiguration;
    else return launch_in_unit2<FORM>(code, a);
}
#endif

}  // namespace bs
}  // namespace ldpc
