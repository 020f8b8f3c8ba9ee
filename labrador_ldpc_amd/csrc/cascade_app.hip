// cascade_app.hip -- the marginals of the soft cascade (labrador_ldpc_decode_ms_cascade_soft_batch_*) on their way to
// the caller's rows, beside the three kernels of cascade.hip and in their style: the dense rows of stage 2 back to the frames' rows
// (scatter_rows), and stage 1's integer marginals of the LLR type widened to int32 (widen_app).  Pure streaming: no LDS, no scratch,
// a flat index, a few registers.  A unit of its own so that cascade.o keeps exactly the kernels it had.
#include "cascade.hpp"
#include "codes.hpp"

#include <algorithm>
#include <type_traits>

namespace ldpc {
namespace {

typedef int int4_ __attribute__((ext_vector_type(4)));

constexpr unsigned MAX_GRID = 1024;              // workgroups of 256, as cascade.hip; the loop strides over the rest

// dest row list[i] = dense row i, rows of `row` 16-byte pieces (the marginals of the soft cascade): a flat (row, piece)
// index as cascade.hip's scatter has it, so the loads are contiguous always and a wave's stores 1 KB contiguous per instruction for rows of 1 KB and more.
__global__ void __launch_bounds__(256) cascade_scatter_rows_kernel(const uint32_t *__restrict__ list, uint32_t row, uint32_t total,
                                                                   const int4_ *__restrict__ dense, int4_ *__restrict__ dest)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const uint32_t r = (uint32_t)i / row, piece = (uint32_t)i - r * row;
        dest[(size_t)list[r] * row + piece] = dense[i];
    }
}

// dst[i] = src[i] sign-extended to 32 bits, in QUADS of four elements: one 4-byte (i8) or 8-byte (i16) load and one 16-byte store per
// lane and step, both lane-contiguous; four quads in flight per thread, all loads first, as llr_quantise.hip.  64-bit indexing, one
// thread per four quads, no grid-stride loop.  The source is a workspace block read once; the stores are the caller's rows.
constexpr int WIDEN_UNROLL = 4;
template <class T>
__global__ void __launch_bounds__(256) cascade_widen_app_kernel(const T *__restrict__ src, int32_t *__restrict__ dst, size_t quads)
{
    static_assert(sizeof(T) == 1 || sizeof(T) == 2);
    typedef unsigned uint2_ __attribute__((ext_vector_type(2)));
    using Raw = std::conditional_t<sizeof(T) == 1, unsigned, uint2_>;
    const size_t i0 = (size_t)blockIdx.x * (256 * WIDEN_UNROLL) + threadIdx.x;
    Raw raw[WIDEN_UNROLL];
#pragma unroll
    for (int u = 0; u < WIDEN_UNROLL; ++u) {
        const size_t i = i0 + (size_t)u * 256;
        if (i < quads) raw[u] = __builtin_nontemporal_load(reinterpret_cast<const Raw *>(src) + i);
    }
#pragma unroll
    for (int u = 0; u < WIDEN_UNROLL; ++u) {
        const size_t i = i0 + (size_t)u * 256;
        if (i < quads) {
            int4_ w;
            if constexpr (sizeof(T) == 1) {
                w = {(int)(int8_t)raw[u], (int)(int8_t)(raw[u] >> 8), (int)(int8_t)(raw[u] >> 16), (int)raw[u] >> 24};
            } else {
                w = {(int)(int16_t)raw[u][0], (int)raw[u][0] >> 16, (int)(int16_t)raw[u][1], (int)raw[u][1] >> 16};
            }
            reinterpret_cast<int4_ *>(dst)[i] = w;
        }
    }
}

}  // namespace

// a row of marginals, f32 or int32, is whole 16-byte pieces for every code
constexpr bool app_rows_are_whole_pieces()
{
    for (const CodeInfo &ci : CODES)
        if ((size_t)(ci.n + ci.p) * 4 % 16) return false;
    return true;
}
static_assert(app_rows_are_whole_pieces(), "launch_cascade_scatter_rows moves rows of (n + p) * 4 bytes in 16-byte pieces");

hipError_t launch_cascade_scatter_rows(const uint32_t *list, size_t listed, const void *dense, size_t row_bytes, void *dest, hipStream_t stream)
{
    if (listed == 0) return hipSuccess;
    if (row_bytes == 0 || row_bytes % 16 || listed * (row_bytes / 16) > 0xFFFFFFFFull || (uintptr_t)dense % 16 || (uintptr_t)dest % 16)
        return hipErrorInvalidValue;
    const size_t row = row_bytes / 16, total = listed * row;
    const unsigned grid = (unsigned)std::min<size_t>((total + 255) / 256, MAX_GRID);
    hipLaunchKernelGGL(cascade_scatter_rows_kernel, dim3(grid), dim3(256), 0, stream, list, (uint32_t)row, (uint32_t)total,
                       static_cast<const int4_ *>(dense), static_cast<int4_ *>(dest));
    return hipGetLastError();
}

template <class T>
hipError_t launch_cascade_widen_app(const T *src, int32_t *dst, size_t elems, hipStream_t stream)
{
    if (elems == 0) return hipSuccess;
    if (elems % 4 || (uintptr_t)src % 16 || (uintptr_t)dst % 16) return hipErrorInvalidValue;
    constexpr size_t PER_GROUP = 256 * WIDEN_UNROLL, SLICE = ((size_t)1 << 30) * PER_GROUP;       // quads per workgroup, per launch
    const size_t quads = elems / 4;
    for (size_t q0 = 0; q0 < quads; q0 += SLICE) {
        const size_t nq = quads - q0 < SLICE ? quads - q0 : SLICE;
        hipLaunchKernelGGL(cascade_widen_app_kernel<T>, dim3((unsigned)((nq + PER_GROUP - 1) / PER_GROUP)), dim3(256), 0, stream, src + q0 * 4,
                           dst + q0 * 4, nq);
    }
    return hipGetLastError();
}

template hipError_t launch_cascade_widen_app<int8_t>(const int8_t *, int32_t *, size_t, hipStream_t);
template hipError_t launch_cascade_widen_app<int16_t>(const int16_t *, int32_t *, size_t, hipStream_t);
}  // namespace ldpc
