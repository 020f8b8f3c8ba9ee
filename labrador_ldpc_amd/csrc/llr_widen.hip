// llr_widen.hip -- f16 / bf16 LLRs to f32 by the library's one widening rule (llr_widen.hpp), batched and
// device-resident: what soft values kept in two bytes pass through on their way to the flooding f32 decoders and the cascade.
// A flat map over batch * n LLRs (frames lie back to back, n is a multiple of 128) and pure streaming, in llr_quantise.hip's shape:
// workgroups of 256, every thread moves OCTETS of eight LLRs -- one 16-byte load, so a wave reads 1 KB contiguous per instruction, and
// two 16-byte stores of what the octet became.  Four octets in flight per thread: all loads, then all converts and stores.  No LDS,
// no scratch.  The source is read once and read non-temporally; the stores are plain, so the widened rows stay in L2 for the decoder
// that follows.
// Counts: 64-bit indexing, one thread per four octets, no grid-stride loop; a launch covers at most 2^30 workgroups (2^43 LLRs) and
// the launcher loops over more.
#include "llr_widen.hpp"
#include <type_traits>

namespace ldpc {
namespace {

typedef float float4_ __attribute__((ext_vector_type(4)));
typedef unsigned uint4_ __attribute__((ext_vector_type(4)));

constexpr int UNROLL = 4;

template <class H>
__global__ void __launch_bounds__(256) widen_kernel(const H *__restrict__ llrs, float *__restrict__ out, size_t octets)
{
    static_assert(std::is_same_v<H, f16_llr> || std::is_same_v<H, bf16_llr>);
    const size_t i0 = (size_t)blockIdx.x * (256 * UNROLL) + threadIdx.x;
    uint4_ raw[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
        const size_t i = i0 + (size_t)u * 256;
        if (i < octets) raw[u] = __builtin_nontemporal_load(reinterpret_cast<const uint4_ *>(llrs) + i);
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
        const size_t i = i0 + (size_t)u * 256;
        if (i < octets) {
            float4_ lo, hi;
#pragma unroll
            for (int j = 0; j < 2; ++j) {                    // word j holds LLRs 2j (low half) and 2j + 1
                lo[2 * j] = widen_llr(H{(uint16_t)(raw[u][j] & 0xFFFFu)});
                lo[2 * j + 1] = widen_llr(H{(uint16_t)(raw[u][j] >> 16)});
                hi[2 * j] = widen_llr(H{(uint16_t)(raw[u][2 + j] & 0xFFFFu)});
                hi[2 * j + 1] = widen_llr(H{(uint16_t)(raw[u][2 + j] >> 16)});
            }
            reinterpret_cast<float4_ *>(out)[2 * i] = lo;
            reinterpret_cast<float4_ *>(out)[2 * i + 1] = hi;
        }
    }
}

}  // namespace

template <class H>
hipError_t launch_widen(const H *llrs, float *out, size_t count, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    if (count % 8) return hipErrorInvalidValue;
    constexpr size_t PER_GROUP = 256 * UNROLL, SLICE = ((size_t)1 << 30) * PER_GROUP;       // octets per workgroup, per launch
    const size_t octets = count / 8;
    for (size_t o0 = 0; o0 < octets; o0 += SLICE) {
        const size_t no = octets - o0 < SLICE ? octets - o0 : SLICE;
        hipLaunchKernelGGL(widen_kernel<H>, dim3((unsigned)((no + PER_GROUP - 1) / PER_GROUP)), dim3(256), 0, stream, llrs + o0 * 8,
                           out + o0 * 8, no);
    }
    return hipGetLastError();
}

template hipError_t launch_widen<f16_llr>(const f16_llr *, float *, size_t, hipStream_t);
template hipError_t launch_widen<bf16_llr>(const bf16_llr *, float *, size_t, hipStream_t);

}  // namespace ldpc
