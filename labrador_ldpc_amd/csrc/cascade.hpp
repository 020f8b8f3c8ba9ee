// cascade.hpp -- the streaming kernels between the two stages of the cascade decode (see cascade.hip), and the two
// more that the soft cascade moves its marginals with (cascade_app.hip).
// Declarations only: capi.hip calls them and does not see the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace ldpc {
// success [frames] -> list: the indices of the frames whose success is 0, *count of them (the launcher zeroes *count first), and
// stage [frames] = 0.  Indices ascend inside a wave; the order across waves is not defined.  frames <= 2^30.
hipError_t launch_cascade_compact(const uint8_t *success, uint8_t *stage, uint32_t *list, uint32_t *count, size_t frames,
                                  hipStream_t stream);
// dense [listed][n] = llrs [list[.]][n].  `dense` is 16-byte aligned, `llrs` to its element at least; listed * n * sizeof(T) < 2^32.
template <class T>
hipError_t launch_cascade_gather(const T *llrs, size_t n, const uint32_t *list, size_t listed, T *dense, hipStream_t stream);
// The dense results of the listed frames back to their rows: output [list[i]][output_len] = d_output [i][output_len] (both 8-byte
// aligned, output_len a multiple of 8), iters, success likewise, and stage [list[i]] = 1.  listed * output_len / 8 < 2^32.
hipError_t launch_cascade_scatter(const uint32_t *list, size_t listed, const uint8_t *d_output, const uint32_t *d_iters,
                                  const uint8_t *d_success, size_t output_len, uint8_t *output, uint32_t *iters, uint8_t *success,
                                  uint8_t *stage, hipStream_t stream);
// dest row list[i] = dense row i, rows of row_bytes (the dense marginals of stage 2 back to the frames' rows).  Both bases are
// 16-byte aligned and row_bytes is a multiple of 16 -- every code's (n + p) * 4 is (asserted in cascade_app.hip);
// listed * row_bytes / 16 < 2^32.  Anything else is hipErrorInvalidValue.
hipError_t launch_cascade_scatter_rows(const uint32_t *list, size_t listed, const void *dense, size_t row_bytes, void *dest,
                                       hipStream_t stream);
// dst [elems] = src [elems] sign-extended, T = int8_t / int16_t (stage 1's marginals of the LLR type into int32 rows).  Both bases
// are 16-byte aligned, elems is a multiple of 4 and may be any size_t: the launcher loops over launches of 2^30 workgroups.  The
// two ranges do not overlap.
template <class T>
hipError_t launch_cascade_widen_app(const T *src, int32_t *dst, size_t elems, hipStream_t stream);
}
