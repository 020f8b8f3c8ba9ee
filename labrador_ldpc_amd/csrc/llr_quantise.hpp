// llr_quantise.hpp -- f32 LLRs to the i8 / i16 LLRs of the integer decoders: the one rule, and its device launcher
// (llr_quantise.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace ldpc {
// The rule, for the host loop of capi.hip and the kernel alike:
//   p = scale * x                      one f32 multiply (the build has -ffp-contract=off and no fast-math: nothing fuses into it)
//   q = 0                              if p is NaN: an erasure.  Said here, not left to a cast or to what a float clamp does with NaN
//     = clamp(rint(p), -lim, lim)      otherwise; rint to nearest, ties to even (the default rounding mode)
// +-inf and products beyond the integers clamp to +-lim (the clamp is on the float, before the cast); -0.0 gives 0.
// 0 <= lim <= 32767, so `lim` is exact as a float and the clamped value fits T.
template <class T>
__host__ __device__ __forceinline__ T quantise_llr(float x, float scale, float lim)
{
    const float p = scale * x;
    // fmaxf / fminf return their other argument for a NaN, so r is always a number in [-lim, lim] and the cast is defined; the NaN's
    // own answer is the select behind it, without a branch
    const float r = fminf(fmaxf(rintf(p), -lim), lim);
    return p != p ? (T)0 : (T)(int)r;
}

// llrs [count] f32 -> q [count] of T (int8_t, int16_t) by the rule above.  Device pointers, both 16-byte aligned; `count` is a
// multiple of 4 (every code's n is a multiple of 128) and may exceed 32 bits; asynchronous on `stream`.  A count that is no multiple
// of 4 is hipErrorInvalidValue.
template <class T>
hipError_t launch_quantise(const float *llrs, T *q, size_t count, float scale, int lim, hipStream_t stream);
}
