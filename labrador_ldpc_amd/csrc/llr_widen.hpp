// llr_widen.hpp -- f16 / bf16 LLRs to the f32 LLRs of the float decoders: the one rule, and its device launcher
// (llr_widen.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace ldpc {
// The two formats, as the raw bits they travel in through the C ABI (const uint16_t *): an element type each, so that a kernel's
// source type says which rule its loader applies.
struct f16_llr { uint16_t bits; };         // IEEE binary16
struct bf16_llr { uint16_t bits; };        // the upper half of an f32
static_assert(sizeof(f16_llr) == 2 && alignof(f16_llr) == 2 && sizeof(bf16_llr) == 2 && alignof(bf16_llr) == 2);

// The rule, for the host loop of capi.hip, the streaming kernel and the fused loader of the layered kernels alike:
//   f16   the exact value: subnormals become the f32 normals they equal, +-0 and +-inf stay; a NaN becomes the QUIET f32 NaN of its
//         sign, payload << 13 with bit 22 set
//   bf16  bits << 16 reinterpreted; nothing else, a signalling NaN stays what it is
// The f16 value is the cast of a _Float16; the cast alone does not make the rule.  The device's conversion instruction quiets a
// signalling NaN, the host's conversion as the compiler emits it does not (0x7C01 came out as 0x7F802000), so the quiet bit is set
// here for every NaN, on both sides: a select and an OR per LLR behind the cast.
__host__ __device__ __forceinline__ float widen_llr(f16_llr h)
{
    _Float16 v;
    __builtin_memcpy(&v, &h.bits, sizeof v);
    float f = (float)v;
    uint32_t w;
    __builtin_memcpy(&w, &f, sizeof w);
    w |= f != f ? 0x00400000u : 0u;
    __builtin_memcpy(&f, &w, sizeof f);
    return f;
}
__host__ __device__ __forceinline__ float widen_llr(bf16_llr h)
{
    const uint32_t w = (uint32_t)h.bits << 16;
    float f;
    __builtin_memcpy(&f, &w, sizeof f);
    return f;
}
// (an f32 source is its own widening: what lets one loader serve the three)
__host__ __device__ __forceinline__ float widen_llr(float x) { return x; }

// llrs [count] of H (f16_llr, bf16_llr) -> out [count] f32 by the rule above.  Device pointers, both 16-byte aligned; `count` is a
// multiple of 8 (every code's n is a multiple of 128) and may exceed 32 bits; asynchronous on `stream`.  A count that is no multiple
// of 8 is hipErrorInvalidValue.
template <class H>
hipError_t launch_widen(const H *llrs, float *out, size_t count, hipStream_t stream);
}
