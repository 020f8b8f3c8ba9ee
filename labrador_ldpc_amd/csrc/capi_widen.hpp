// capi_widen.hpp -- part of capi.hip: f16 / bf16 LLRs to the f32 decoders (labrador_ldpc_widen_llrs_batch_*,
// labrador_ldpc_decode_ms_*_batch_f16 / _bf16): the host loop, and what the flooding and cascade entries do with one
// launch slice.
#pragma once

namespace {

// the host path: the rule element by element, where the data lies
template <class H>
void widen_host(const uint16_t *llrs, float *out, size_t count)
{
    for (size_t i = 0; i < count; ++i) out[i] = ldpc::widen_llr(H{llrs[i]});
}

// frames per widen + decode pair, from the f32 row size; LABRADOR_LDPC_HIP_WIDEN_CHUNK=<frames> lowers it, for tests
size_t widen_chunk_frames(size_t f32_row_bytes) { return workspace_chunk_frames(f32_row_bytes, "LABRADOR_LDPC_HIP_WIDEN_CHUNK"); }

// One launch slice of a decode from half-precision rows: in chunks, the rows are widened into the thread's workspace
// (converted_slice(), capi_quantise.hpp) and decode(f32 rows, first frame of the chunk, frames, stream) runs an f32 decoder on them.
template <class H, class Decode>
hipError_t widened_slice(const ldpc::CodeInfo &ci, const H *llrs, size_t nb, hipStream_t stream, const Decode &decode)
{
    const size_t n = ci.n;
    return converted_slice<float>(n, widen_chunk_frames(n * sizeof(float)), llrs, nb, stream,
                                  [](const H *in, float *w, size_t count, hipStream_t s) { return ldpc::launch_widen<H>(in, w, count, s); },
                                  decode);
}

}  // namespace
