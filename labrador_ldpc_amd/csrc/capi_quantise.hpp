// capi_quantise.hpp -- part of capi.hip: f32 LLRs to the integer decoders (labrador_ldpc_quantise_llrs_batch_*,
// labrador_ldpc_decode_ms_quantised_batch_*): the range of the quantiser's parameters, the host loop, and what the
// fused decode does with one launch slice.
#pragma once

namespace {

// scale finite and > 0, 0 <= lim <= the type's maximum: with these the rule of llr_quantise.hpp is defined for every f32 input
int check_quantiser(float scale, int lim, int tmax)
{
    if (!(scale > 0.0f && scale <= std::numeric_limits<float>::max()))
        return fail(LABRADOR_LDPC_HIP_EINVAL, "scale %g is not in (0, FLT_MAX]", (double)scale);
    if (lim < 0 || lim > tmax) return fail(LABRADOR_LDPC_HIP_EINVAL, "lim %d is not in 0 .. %d", lim, tmax);
    return LABRADOR_LDPC_HIP_OK;
}

// the host path: the rule element by element, where the data lies
template <class T>
void quantise_host(const float *llrs, T *q, size_t count, float scale, int lim)
{
    const float flim = (float)lim;
    for (size_t i = 0; i < count; ++i) q[i] = ldpc::quantise_llr<T>(llrs[i], scale, flim);
}

// frames per quantise + decode pair of the fused call; LABRADOR_LDPC_HIP_QUANT_CHUNK=<frames> lowers it, for tests
size_t quant_chunk_frames(size_t q_row_bytes) { return workspace_chunk_frames(q_row_bytes, "LABRADOR_LDPC_HIP_QUANT_CHUNK"); }

// The converted rows of a fused convert-and-decode call, between its two kernels -- the quantised rows here, the widened rows of
// capi_widen.hpp: grow-only, per calling thread and per device, with the cascade workspace's guard across streams.  Only `data` is
// used.
thread_local CascadeWorkspace g_converted;

// One launch slice of a fused convert-and-decode: in chunks of at most `chunk_frames`, the frames' rows of SRC are converted into
// rows of DST in the workspace and a decoder of DST runs on them.  convert(rows, dst, elements, stream) enqueues the conversion,
// decode(dst rows, first frame of the chunk, frames, stream) the decoder on the chunk's outputs.
template <class DST, class SRC, class Convert, class Decode>
hipError_t converted_slice(size_t n, size_t chunk_frames, const SRC *rows, size_t nb, hipStream_t stream, const Convert &convert,
                           const Decode &decode)
{
    CascadeWorkspace &ws = g_converted;
    if (hipError_t e = ws.ensure(); e != hipSuccess) return e;
    const size_t chunk = std::min(chunk_frames, nb);
    if (hipError_t e = ws.reserve(ws.data, chunk * n * sizeof(DST)); e != hipSuccess) return e;
    if (hipError_t e = ws.wait_for_last_use(stream); e != hipSuccess) return e;
    CascadeWorkspace::Use use{ws, stream};
    DST *const d = static_cast<DST *>(ws.data.p);
    for (size_t c0 = 0; c0 < nb; c0 += chunk) {
        const size_t nc = std::min(chunk, nb - c0);
        if (hipError_t e = convert(rows + c0 * n, d, nc * n, stream); e != hipSuccess) return e;
        if (hipError_t e = decode(d, c0, nc, stream); e != hipSuccess) return e;
    }
    return hipSuccess;
}

// One launch slice of the fused quantise-and-decode: the f32 rows are quantised to T at (scale, lim) and the decoder of T runs on
// them, in chunks of quant_chunk_frames().
template <class T, class Decode>
hipError_t quantised_slice(const ldpc::CodeInfo &ci, const float *llrs, size_t nb, float scale, int lim, hipStream_t stream, const Decode &decode)
{
    const size_t n = ci.n;
    return converted_slice<T>(n, quant_chunk_frames(n * sizeof(T)), llrs, nb, stream,
                              [=](const float *in, T *q, size_t count, hipStream_t s) { return ldpc::launch_quantise<T>(in, q, count, scale, lim, s); },
                              decode);
}

}  // namespace
