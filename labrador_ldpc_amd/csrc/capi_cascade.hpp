// capi_cascade.hpp -- part of capi.hip: the workspace of the cascade decode (labrador_ldpc_decode_ms_cascade_batch_*)
// and what it does with one launch slice.
#pragma once

namespace {

// Frames per launch on a workspace: what fits 256 MiB of LLR rows, at least 8192 (every code's 8192 rows fit 256 MiB, so a chunk's
// bytes and pieces always fit 32 bits).  The variable `env` names (=<frames>) lowers it, for tests; it is read per call.
size_t workspace_chunk_frames(size_t llr_row_bytes, const char *env_name)
{
    size_t c = ((size_t)256 << 20) / llr_row_bytes;
    if (c < 8192) c = 8192;
    if (const char *env = std::getenv(env_name)) {
        const long long v = std::atoll(env);
        if (v > 0 && (size_t)v < c) c = (size_t)v;
    }
    return c;
}
// failed frames per stage-2 launch of the cascade
size_t cascade_chunk_frames(size_t llr_row_bytes) { return workspace_chunk_frames(llr_row_bytes, "LABRADOR_LDPC_HIP_CASCADE_CHUNK"); }

// Device memory between the two stages, grow-only, per calling thread and per device like StagingPool: `index` holds the counter
// and the list of failed frames of a slice, `data` a chunk's gathered LLRs and dense stage-2 results (and, before them, a chunk of
// the integer soft cascade's stage-1 marginals).  Calls of one thread may use
// different streams: `last_use` is recorded on a call's stream behind its last use of the workspace, and the next call makes its
// own stream wait for it before it touches the workspace.  The count comes back through a pinned word, read after the call's own
// synchronisation, so it needs no such care.  The fused quantise-and-decode (capi_quantise.hpp) keeps a second one of these for its
// quantised rows and uses `data` alone.
struct CascadeWorkspace {
    struct Block { void *p = nullptr; size_t cap = 0; };
    Block index, data;
    uint32_t *count_host = nullptr;
    hipEvent_t last_use = nullptr;
    bool pending = false;                          // last_use has been recorded since the workspace was (re)made
    int dev = -1;
    void drop()
    {
        if (dev < 0) return;
        if (pending) (void)hipEventSynchronize(last_use);
        for (Block *b : {&index, &data}) {
            if (b->p) (void)hipFree(b->p);
            *b = Block{};
        }
        (void)hipEventDestroy(last_use);
        (void)hipHostFree(count_host);
        last_use = nullptr; count_host = nullptr; pending = false; dev = -1;
    }
    ~CascadeWorkspace() { drop(); }
    hipError_t ensure()
    {
        int cur = 0;
        hipError_t e = hipGetDevice(&cur);
        if (e != hipSuccess) return e;
        if (dev == cur) return hipSuccess;
        drop();
        if ((e = hipEventCreateWithFlags(&last_use, hipEventDisableTiming)) != hipSuccess) return e;
        if ((e = hipHostMalloc((void **)&count_host, 64, hipHostMallocDefault)) != hipSuccess) {
            (void)hipEventDestroy(last_use);
            last_use = nullptr; count_host = nullptr;
            return e;
        }
        dev = cur;
        return hipSuccess;
    }
    hipError_t reserve(Block &b, size_t bytes)
    {
        if (b.cap >= bytes) return hipSuccess;
        if (b.p) {
            if (pending) (void)hipEventSynchronize(last_use);       // an earlier call's work, maybe on another stream, may still use it
            (void)hipFree(b.p);
            b = Block{};
        }
        const hipError_t e = hipMalloc(&b.p, bytes);
        if (e != hipSuccess) { b.p = nullptr; return e; }
        b.cap = bytes;
        return hipSuccess;
    }
    // Before a call's first touch of the workspace: its stream waits for the last use of the call before.
    hipError_t wait_for_last_use(hipStream_t stream) { return pending ? hipStreamWaitEvent(stream, last_use, 0) : hipSuccess; }
    // Held from there to the way out, whichever it is: whatever was enqueued in between, the next call waits for it.
    struct Use {
        CascadeWorkspace &ws;
        hipStream_t stream;
        Use(CascadeWorkspace &w, hipStream_t s) : ws(w), stream(s) {}
        Use(const Use &) = delete;
        ~Use() { if (hipEventRecord(ws.last_use, stream) == hipSuccess) ws.pending = true; else (void)hipGetLastError(); }
    };
};
thread_local CascadeWorkspace g_cascade;

// One launch slice of the cascade: stage 1 on every frame, the list of the frames it failed, their count read back (the one
// synchronisation of `stream`), then gather, stage 2 and scatter in chunks of the failed frames.  stage1(llrs, app of T or NULL,
// output, iters, success, frames, stream) and stage2(dense llrs, dense app of A or NULL, dense output, dense iters, dense success,
// frames, stream) enqueue the two decoders.
// With `app` (the soft cascade; A = T for float, int32 for the integers) every frame's marginals go to its row of
// [nb][n + p]: stage 2 writes dense rows into the workspace, scattered like the rest.  Stage 1 of float writes the caller's rows
// themselves -- a frame that stage 2 takes is overwritten.  Stage 1 of the integers stores marginals of T: it runs in chunks of
// frames, back to back on the stream, each into the workspace's `data` block and widened from there into the caller's int32 rows
// (never in place: a parallel front-to-back widening overwrites sources not yet read); the workspace is therefore taken before
// stage 1 then, and `compact` still runs once, over the whole slice.
// M: the type of stage 1's marginals -- T, but for the cascade whose stage 1 reads f32 rows and quantises in its loader (DESIGN.md
// 4.20): T = float, M = int8_t, A = int32_t.
template <class T, class A = T, class M = T, class Stage1, class Stage2>
hipError_t cascade_slice(const ldpc::CodeInfo &ci, const T *llrs, uint8_t *output, uint32_t *iters, uint8_t *success, uint8_t *stage,
                         size_t nb, hipStream_t stream, const Stage1 &stage1, const Stage2 &stage2, A *app = nullptr)
{
    constexpr bool WIDENS = !std::is_same_v<M, A>;
    const size_t n = ci.n, np = (size_t)ci.n + ci.p, out_len = ci.output_len();
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    CascadeWorkspace &ws = g_cascade;
    constexpr size_t LIST_AT = 16;                                  // the counter's word, then the list
    std::optional<CascadeWorkspace::Use> use;
    auto take_workspace = [&]() -> hipError_t {
        if (hipError_t e = ws.ensure(); e != hipSuccess) return e;
        if (hipError_t e = ws.reserve(ws.index, LIST_AT + nb * sizeof(uint32_t)); e != hipSuccess) return e;
        if (hipError_t e = ws.wait_for_last_use(stream); e != hipSuccess) return e;
        use.emplace(ws, stream);
        return hipSuccess;
    };
    bool stage1_done = false;
    if constexpr (WIDENS) {
        if (app) {
            if (hipError_t e = take_workspace(); e != hipSuccess) return e;
            const size_t chunk = std::min(cascade_chunk_frames(np * sizeof(M)), nb);
            if (hipError_t e = ws.reserve(ws.data, up(chunk * np * sizeof(M))); e != hipSuccess) return e;
            M *const d_app = static_cast<M *>(ws.data.p);
            for (size_t f0 = 0; f0 < nb; f0 += chunk) {
                const size_t nf = std::min(chunk, nb - f0);
                if (hipError_t e = stage1(llrs + f0 * n, d_app, output + f0 * out_len, iters + f0, success + f0, nf, stream); e != hipSuccess)
                    return e;
                if (hipError_t e = ldpc::launch_cascade_widen_app<M>(d_app, app + f0 * np, nf * np, stream); e != hipSuccess) return e;
            }
            stage1_done = true;
        }
    }
    if (!stage1_done) {
        M *app1 = nullptr;
        if constexpr (!WIDENS) app1 = app;
        if (hipError_t e = stage1(llrs, app1, output, iters, success, nb, stream); e != hipSuccess) return e;
        if (hipError_t e = take_workspace(); e != hipSuccess) return e;
    }

    uint32_t *const count = static_cast<uint32_t *>(ws.index.p);
    uint32_t *const list = reinterpret_cast<uint32_t *>(static_cast<char *>(ws.index.p) + LIST_AT);
    if (hipError_t e = ldpc::launch_cascade_compact(success, stage, list, count, nb, stream); e != hipSuccess) return e;
    if (hipError_t e = hipMemcpyAsync(ws.count_host, count, sizeof(uint32_t), hipMemcpyDeviceToHost, stream); e != hipSuccess) return e;
    if (hipError_t e = hipStreamSynchronize(stream); e != hipSuccess) return e;
    const size_t failed = *ws.count_host;
    if (failed == 0) return hipSuccess;
    if (failed > nb) return hipErrorUnknown;

    // (a chunk's LLR rows fit 256 MiB, and with marginals its rows of them, the longer ones, do)
    const size_t chunk = std::min(cascade_chunk_frames(app ? np * sizeof(A) : n * sizeof(T)), failed);
    const size_t at_out = up(chunk * n * sizeof(T)), at_iters = at_out + up(chunk * out_len), at_ok = at_iters + up(chunk * sizeof(uint32_t));
    const size_t at_app = at_ok + up(chunk);
    if (hipError_t e = ws.reserve(ws.data, at_app + (app ? up(chunk * np * sizeof(A)) : 0)); e != hipSuccess) return e;
    char *const base = static_cast<char *>(ws.data.p);
    T *const d_llrs = reinterpret_cast<T *>(base);
    uint8_t *const d_out = reinterpret_cast<uint8_t *>(base + at_out), *const d_ok = reinterpret_cast<uint8_t *>(base + at_ok);
    uint32_t *const d_iters = reinterpret_cast<uint32_t *>(base + at_iters);
    A *const d_app = app ? reinterpret_cast<A *>(base + at_app) : nullptr;
    for (size_t c0 = 0; c0 < failed; c0 += chunk) {
        const size_t nc = std::min(chunk, failed - c0);
        if (hipError_t e = ldpc::launch_cascade_gather<T>(llrs, n, list + c0, nc, d_llrs, stream); e != hipSuccess) return e;
        if (hipError_t e = stage2(d_llrs, d_app, d_out, d_iters, d_ok, nc, stream); e != hipSuccess) return e;
        if (hipError_t e = ldpc::launch_cascade_scatter(list + c0, nc, d_out, d_iters, d_ok, out_len, output, iters, success, stage, stream);
            e != hipSuccess)
            return e;
        if (app)
            if (hipError_t e = ldpc::launch_cascade_scatter_rows(list + c0, nc, d_app, np * sizeof(A), app, stream); e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace
