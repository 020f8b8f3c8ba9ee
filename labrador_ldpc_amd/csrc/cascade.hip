// cascade.hip -- what lies between the two stages of the cascade decode (labrador_ldpc_decode_ms_cascade_batch_*):
// the flooding decoder has run on a slice and left `success`; the frames it failed are listed (compact), their LLR rows are copied
// into a dense workspace (gather) for the layered decoder, and its dense results go back to the frames' own rows (scatter).  All three
// are pure streaming: no LDS, no scratch, a few registers; the only atomic is one add per wave on the counter of the list.
#include "cascade.hpp"

namespace ldpc {
namespace {

typedef int int4_ __attribute__((ext_vector_type(4)));

constexpr int GATHER_UNROLL = 4;                 // 16-byte pieces a thread has in flight, as llr_convert.hip
constexpr unsigned MAX_GRID = 1024;              // workgroups of 256: four waves per SIMD of 256 CUs; the loops stride over the rest

// One thread per frame.  A wave's failed frames take consecutive places in the list, in ascending order: their number is the
// popcount of the wave's ballot, their first place comes from one atomic add on the counter by the wave's first lane, a lane's
// place from the failed lanes below it.  Waves land in the order of their atomics: the list is a set, results are scattered by index.
__global__ void __launch_bounds__(256) cascade_compact_kernel(const uint8_t *__restrict__ success, uint8_t *__restrict__ stage,
                                                              uint32_t *__restrict__ list, uint32_t *__restrict__ count, uint32_t frames)
{
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    const bool inside = f < frames;
    const bool failed = inside && success[f] == 0;
    if (inside) stage[f] = 0;
    const unsigned long long mask = __ballot(failed);            // (every lane of the wave is here: nothing returned above)
    if (mask == 0) return;
    const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
    const int leader = __ffsll((long long)mask) - 1;             // the lowest failed lane
    uint32_t first = 0;
    if ((int)(threadIdx.x & 63u) == leader) first = atomicAdd(count, (uint32_t)__popcll(mask));
    first = (uint32_t)__builtin_amdgcn_readlane((int)first, leader);       // (leader is the same in every lane)
    if (failed) list[first + below] = f;
}

// dense row i = llrs row list[i].  ALIGNED: rows are whole 16-byte pieces at 16-byte aligned addresses; a flat (row, piece) index, so
// a wave's loads are 1 KB contiguous per instruction for rows of 1 KB and more and cover several rows of a shorter code; its stores
// are contiguous always.  `row` counts pieces then, and elements of T otherwise (a base aligned to its element only).
template <class T, bool ALIGNED>
__global__ void __launch_bounds__(256) cascade_gather_kernel(const T *__restrict__ llrs, uint32_t row, const uint32_t *__restrict__ list,
                                                             uint32_t total, T *__restrict__ dense)
{
    if constexpr (ALIGNED) {
        const int4_ *src = reinterpret_cast<const int4_ *>(llrs);
        int4_ *dst = reinterpret_cast<int4_ *>(dense);
        constexpr size_t SPAN = 256 * GATHER_UNROLL;
        for (size_t base = (size_t)blockIdx.x * SPAN + threadIdx.x; base < total; base += (size_t)gridDim.x * SPAN) {
            int4_ raw[GATHER_UNROLL];
#pragma unroll
            for (int u = 0; u < GATHER_UNROLL; ++u) {
                const size_t i = base + u * 256;
                if (i < total) {
                    const uint32_t r = (uint32_t)i / row, piece = (uint32_t)i - r * row;
                    raw[u] = __builtin_nontemporal_load(src + (size_t)list[r] * row + piece);      // (read once; stage 1 had its pass)
                }
            }
#pragma unroll
            for (int u = 0; u < GATHER_UNROLL; ++u) {
                const size_t i = base + u * 256;
                if (i < total) dst[i] = raw[u];                                                    // (plain: stage 2 reads it next)
            }
        }
    } else {
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
            const uint32_t r = (uint32_t)i / row, e = (uint32_t)i - r * row;
            dense[i] = llrs[(size_t)list[r] * row + e];
        }
    }
}

// The dense results back to the listed frames: `output` rows in 8-byte pieces over a flat (row, piece) index; the thread that moves
// a row's first piece also moves its iters and success and marks its stage.
__global__ void __launch_bounds__(256) cascade_scatter_kernel(const uint32_t *__restrict__ list, uint32_t row, uint32_t total,
                                                              const unsigned long long *__restrict__ d_output,
                                                              const uint32_t *__restrict__ d_iters, const uint8_t *__restrict__ d_success,
                                                              unsigned long long *__restrict__ output, uint32_t *__restrict__ iters,
                                                              uint8_t *__restrict__ success, uint8_t *__restrict__ stage)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const uint32_t r = (uint32_t)i / row, piece = (uint32_t)i - r * row;
        const uint32_t f = list[r];
        output[(size_t)f * row + piece] = d_output[i];
        if (piece == 0) {
            iters[f] = d_iters[r];
            success[f] = d_success[r];
            stage[f] = 1;
        }
    }
}

inline unsigned grid_for(size_t items, size_t per_group)
{
    const size_t g = (items + per_group - 1) / per_group;
    return (unsigned)(g < MAX_GRID ? g : MAX_GRID);
}

}  // namespace

hipError_t launch_cascade_compact(const uint8_t *success, uint8_t *stage, uint32_t *list, uint32_t *count, size_t frames, hipStream_t stream)
{
    if (frames == 0 || frames > ((size_t)1 << 30)) return hipErrorInvalidValue;
    if (hipError_t e = hipMemsetAsync(count, 0, sizeof(uint32_t), stream); e != hipSuccess) return e;
    hipLaunchKernelGGL(cascade_compact_kernel, dim3((unsigned)((frames + 255) / 256)), dim3(256), 0, stream, success, stage, list, count,
                       (uint32_t)frames);
    return hipGetLastError();
}

template <class T>
hipError_t launch_cascade_gather(const T *llrs, size_t n, const uint32_t *list, size_t listed, T *dense, hipStream_t stream)
{
    if (listed == 0) return hipSuccess;
    if (n == 0 || n * sizeof(T) % 16 || listed * n * sizeof(T) > 0xFFFFFFFFull || (uintptr_t)dense % 16) return hipErrorInvalidValue;
    if ((uintptr_t)llrs % 16 == 0) {
        const size_t row = n * sizeof(T) / 16, total = listed * row;
        hipLaunchKernelGGL((cascade_gather_kernel<T, true>), dim3(grid_for(total, 256 * GATHER_UNROLL)), dim3(256), 0, stream, llrs,
                           (uint32_t)row, list, (uint32_t)total, dense);
    } else {
        const size_t total = listed * n;
        hipLaunchKernelGGL((cascade_gather_kernel<T, false>), dim3(grid_for(total, 256)), dim3(256), 0, stream, llrs, (uint32_t)n, list,
                           (uint32_t)total, dense);
    }
    return hipGetLastError();
}

hipError_t launch_cascade_scatter(const uint32_t *list, size_t listed, const uint8_t *d_output, const uint32_t *d_iters,
                                  const uint8_t *d_success, size_t output_len, uint8_t *output, uint32_t *iters, uint8_t *success,
                                  uint8_t *stage, hipStream_t stream)
{
    if (listed == 0) return hipSuccess;
    if (output_len == 0 || output_len % 8 || listed * (output_len / 8) > 0xFFFFFFFFull || (uintptr_t)output % 8 || (uintptr_t)d_output % 8)
        return hipErrorInvalidValue;
    const size_t row = output_len / 8, total = listed * row;
    hipLaunchKernelGGL(cascade_scatter_kernel, dim3(grid_for(total, 256)), dim3(256), 0, stream, list, (uint32_t)row, (uint32_t)total,
                       reinterpret_cast<const unsigned long long *>(d_output), d_iters, d_success,
                       reinterpret_cast<unsigned long long *>(output), iters, success, stage);
    return hipGetLastError();
}

template hipError_t launch_cascade_gather<float>(const float *, size_t, const uint32_t *, size_t, float *, hipStream_t);
template hipError_t launch_cascade_gather<int8_t>(const int8_t *, size_t, const uint32_t *, size_t, int8_t *, hipStream_t);
template hipError_t launch_cascade_gather<int16_t>(const int16_t *, size_t, const uint32_t *, size_t, int16_t *, hipStream_t);

}  // namespace ldpc
