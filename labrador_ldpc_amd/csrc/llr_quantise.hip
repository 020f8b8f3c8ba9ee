// llr_quantise.hip -- f32 LLRs to i8 / i16 by the library's one quantisation rule (llr_quantise.hpp), batched and
// device-resident: what a receiver's soft values pass through on their way to the integer decoders.
// A flat map over batch * n LLRs (frames lie back to back, n is a multiple of 128) and pure streaming, in llr_convert.hip's shape:
// workgroups of 256, every thread moves QUADS of four LLRs -- one 16-byte load, so a wave reads 1 KB contiguous per instruction, and
// one 4-byte (i8) or 8-byte (i16) store of what the quad became, lane-contiguous too.  Four quads in flight per thread: all loads,
// then all converts and stores.  No LDS, no scratch.  The source is read once and read non-temporally; the stores are plain, so the
// quantised rows stay in L2 for the decoder that follows.
// Counts: 64-bit indexing, one thread per four quads, no grid-stride loop; a launch covers at most 2^30 workgroups (2^42 LLRs) and
// the launcher loops over more.
#include "llr_quantise.hpp"
#include <type_traits>

namespace ldpc {
namespace {

typedef float float4_ __attribute__((ext_vector_type(4)));
typedef unsigned uint2_ __attribute__((ext_vector_type(2)));

constexpr int UNROLL = 4;

template <class T>
__global__ void __launch_bounds__(256) quantise_kernel(const float *__restrict__ llrs, T *__restrict__ q, size_t quads, float scale, float lim)
{
    static_assert(std::is_same_v<T, int8_t> || std::is_same_v<T, int16_t>);
    const size_t i0 = (size_t)blockIdx.x * (256 * UNROLL) + threadIdx.x;
    float4_ raw[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
        const size_t i = i0 + (size_t)u * 256;
        if (i < quads) raw[u] = __builtin_nontemporal_load(reinterpret_cast<const float4_ *>(llrs) + i);
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
        const size_t i = i0 + (size_t)u * 256;
        if (i < quads) {
            T v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = quantise_llr<T>(raw[u][j], scale, lim);
            if constexpr (sizeof(T) == 1) {
                const unsigned w = (unsigned)(uint8_t)v[0] | (unsigned)(uint8_t)v[1] << 8 | (unsigned)(uint8_t)v[2] << 16 | (unsigned)(uint8_t)v[3] << 24;
                reinterpret_cast<unsigned *>(q)[i] = w;
            } else {
                const uint2_ w = {(unsigned)(uint16_t)v[0] | (unsigned)(uint16_t)v[1] << 16, (unsigned)(uint16_t)v[2] | (unsigned)(uint16_t)v[3] << 16};
                reinterpret_cast<uint2_ *>(q)[i] = w;
            }
        }
    }
}

}  // namespace

template <class T>
hipError_t launch_quantise(const float *llrs, T *q, size_t count, float scale, int lim, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    if (count % 4) return hipErrorInvalidValue;
    constexpr size_t PER_GROUP = 256 * UNROLL, SLICE = ((size_t)1 << 30) * PER_GROUP;       // quads per workgroup, per launch
    const size_t quads = count / 4;
    for (size_t q0 = 0; q0 < quads; q0 += SLICE) {
        const size_t nq = quads - q0 < SLICE ? quads - q0 : SLICE;
        hipLaunchKernelGGL(quantise_kernel<T>, dim3((unsigned)((nq + PER_GROUP - 1) / PER_GROUP)), dim3(256), 0, stream, llrs + q0 * 4,
                           q + q0 * 4, nq, scale, (float)lim);
    }
    return hipGetLastError();
}

template hipError_t launch_quantise<int8_t>(const float *, int8_t *, size_t, float, int, hipStream_t);
template hipError_t launch_quantise<int16_t>(const float *, int16_t *, size_t, float, int, hipStream_t);

}  // namespace ldpc
