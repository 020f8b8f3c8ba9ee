// capi_staging.hpp -- part of capi.hip: staging memory for the host-pointer entry points, the three-stream host pipeline and
// the launch slicer of device-resident batches.
#pragma once

namespace {

// Staging memory for the host-pointer entry points.  Each calling thread keeps a small set of
// grow-only device buffers per device, so the reference-shaped single-frame calls do not pay a
// hipMalloc/hipFree pair per frame (they are freed when the thread exits).
struct StagingPool {
    struct Slot { void *p = nullptr; size_t cap = 0; int dev = -1; };
    Slot slots[12];
    ~StagingPool() { for (auto &s : slots) if (s.p) (void)hipFree(s.p); }
    hipError_t get(int idx, size_t bytes, void **out)
    {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        Slot &s = slots[idx];
        if (s.p && (s.dev != dev || s.cap < bytes)) {
            (void)hipFree(s.p);                       // implicit sync: no work of ours still uses it (calls are synchronous)
            s.p = nullptr; s.cap = 0;
        }
        if (!s.p) {
            const size_t cap = bytes < 4096 ? 4096 : bytes;
            e = hipMalloc(&s.p, cap);
            if (e != hipSuccess) { s.p = nullptr; return e; }
            s.cap = cap; s.dev = dev;
        }
        *out = s.p;
        return hipSuccess;
    }
};
thread_local StagingPool g_pool;

// ---- host-pointer pipeline -----------------------------------------------------------------------
// The entry points that take HOST buffers stage them through the GPU in chunks.  With more than
// one chunk the three legs run on three streams -- host->device copy of chunk c+1, kernel of chunk
// c, device->host copy of chunk c's results (issued from a collector thread: pageable copies block
// their caller) -- with two sets of staging buffers, so the call runs at max(copy, kernel) per
// chunk instead of their sum (TM8192 f32 is copy-bound: 32 KB of LLRs in,
// 1.3 KB out per frame).  One chunk (the reference-shaped single-frame calls) takes the plain
// copy / launch / copy sequence on the caller's stream.
// Single-frame calls that were completed by a ticket (PinnedStage below) leave their stream un-synchronised: the runtime has not
// retired their records.  Which stream, and how many calls: per thread.
struct Unsynced {
    hipStream_t on = nullptr;
    unsigned calls = 0;
    // a stream with unretired records makes the runtime's next copy on it slower (a single-frame TM5120 f32 call -- copy in, kernel --
    // 52 -> 56 us): calls that will not be notified retire them first (the work is done: this costs a microsecond)
    hipError_t retire()
    {
        if (calls == 0) return hipSuccess;
        calls = 0;
        return hipStreamSynchronize(on);
    }
    void forget(hipStream_t s) { if (on == s) calls = 0; }      // (the stream is about to be destroyed, which completes its work)
};
thread_local Unsynced g_unsynced;

struct PipeStreams {                                  // per calling thread, per device
    int dev = -1;
    hipStream_t in = nullptr, run = nullptr, out = nullptr;
    hipEvent_t ev_in[2] = {}, ev_run[2] = {};
    void drop()
    {
        if (dev < 0) return;
        g_unsynced.forget(run);
        (void)hipStreamDestroy(in); (void)hipStreamDestroy(run); (void)hipStreamDestroy(out);
        for (int i = 0; i < 2; ++i) { (void)hipEventDestroy(ev_in[i]); (void)hipEventDestroy(ev_run[i]); }
        dev = -1;
    }
    hipError_t ensure()
    {
        int cur = 0;
        hipError_t e = hipGetDevice(&cur);
        if (e != hipSuccess) return e;
        if (dev == cur) return hipSuccess;
        drop();
        hipStream_t *st[3] = {&in, &run, &out};
        for (auto *sp : st)
            if ((e = hipStreamCreateWithFlags(sp, hipStreamNonBlocking)) != hipSuccess) return e;
        for (int i = 0; i < 2; ++i) {
            if ((e = hipEventCreateWithFlags(&ev_in[i], hipEventDisableTiming)) != hipSuccess) return e;
            if ((e = hipEventCreateWithFlags(&ev_run[i], hipEventDisableTiming)) != hipSuccess) return e;
        }
        dev = cur;
        return hipSuccess;
    }
    ~PipeStreams() { drop(); }
};
thread_local PipeStreams g_pipe;

struct HostOut { void *host; size_t bytes_per_item; };

// Small calls (the reference-shaped single-frame entry points above all) go through one pinned host
// buffer per thread: one copy in, one copy out of a single device block holding all outputs, instead of
// four pageable copies -- the call's latency is mostly copy and synchronisation overhead.
// The smallest calls (a frame or a few: DIRECT_CALL_BYTES) skip the copies as well: the kernel reads its input from the pinned
// buffer and writes its results into it across the link -- a launch and a synchronisation instead of copy, launch, copy,
// synchronisation (one frame through the reference-shaped entry, TC128 f32: 21.3 -> 17.4 us per call, TM8192 f32 58.4 -> 51.8:
// profiles/r03_final/single_frame_latency.txt).  The buffer is mapped into every device's address space for that
// (`dev` is its device-side address); kernels that read their input more than once (the register-lean f32 / f64 decoders
// re-read their LLRs in every iteration) still get it copied.  LABRADOR_LDPC_HIP_NO_DIRECT=1 keeps the copies.
// A direct call whose one kernel has one workgroup -- every single-frame call -- does not even synchronise: the kernel stores the
// call's ticket into a word behind the buffer when its results are written (notify.hpp) and the calling thread spins on that word:
// 12.5 -> 8.2 us for an empty kernel, TC128 f32 17.6 -> 13 us per call (profiles/r06_kbench/launch_floor.txt).
// LABRADOR_LDPC_HIP_NO_NOTIFY=1 synchronises as before.
struct PinnedStage {
    void *p = nullptr, *dev = nullptr;
    size_t cap = 0;
    uint32_t ticket = 0;                 // of the last notified call of this thread (the word behind the buffer holds it when that call is done)
    ~PinnedStage() { if (p) (void)hipHostFree(p); }
    hipError_t get(size_t bytes, void **out)
    {
        if (cap < bytes) {
            if (p) (void)hipHostFree(p);
            p = nullptr; dev = nullptr; cap = 0;
            const size_t want = bytes < (64u << 10) ? (64u << 10) : (bytes + 63) / 64 * 64;
            hipError_t e = hipHostMalloc(&p, want + 64, hipHostMallocPortable | hipHostMallocMapped);
            if (e != hipSuccess) { p = nullptr; return e; }
            if (hipHostGetDevicePointer(&dev, p, 0) != hipSuccess) { (void)hipGetLastError(); dev = nullptr; }
            cap = want;
            *flag_host() = ticket;
        }
        *out = p;
        return hipSuccess;
    }
    uint32_t *flag_host() const { return reinterpret_cast<uint32_t *>(static_cast<char *>(p) + cap); }
    uint32_t *flag_dev() const { return reinterpret_cast<uint32_t *>(static_cast<char *>(dev) + cap); }
};
thread_local PinnedStage g_pinned;
bool notify_enabled()
{
    static const bool off = ldpc::env_flag("LABRADOR_LDPC_HIP_NO_NOTIFY");
    return !off;
}
// spin until the kernel has stored `ticket`; now and then ask the runtime, since a kernel that faulted never will
hipError_t wait_ticket(const uint32_t *flag, uint32_t ticket, hipStream_t stream)
{
    for (unsigned spins = 1;; ++spins) {
        if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == ticket) return hipSuccess;
        if ((spins & 0x3FFFu) == 0) {
            const hipError_t q = hipStreamQuery(stream);
            if (q == hipSuccess) return __atomic_load_n(flag, __ATOMIC_ACQUIRE) == ticket ? hipSuccess : hipErrorUnknown;
            if (q != hipErrorNotReady) return q;
        }
#if defined(__x86_64__) || defined(__i386__)
        __builtin_ia32_pause();
#endif
    }
}
constexpr size_t SMALL_CALL_BYTES = 1u << 20, DIRECT_CALL_BYTES = 64u << 10;
bool direct_calls_enabled()
{
    static const bool off = ldpc::env_flag("LABRADOR_LDPC_HIP_NO_DIRECT");
    return !off;
}

// frames per chunk: about 128 MB of input, at least 8192 frames (the persistent kernels want
// tens of codewords per workgroup), at most 262144
// (LABRADOR_LDPC_HIP_CHUNK=<frames> overrides, for tests and tuning).
size_t chunk_items(size_t in_bytes_per_item)
{
    if (const char *env = std::getenv("LABRADOR_LDPC_HIP_CHUNK")) {
        const long v = std::atol(env);
        if (v > 0) return (size_t)v;
    }
    size_t c = ((size_t)128 << 20) / (in_bytes_per_item ? in_bytes_per_item : 1);
    if (c < 8192) c = 8192;
    if (c > 262144) c = 262144;
    return c;
}

// launch(d_in, d_in2, d_out[NOUT], first_item, n_items, stream) -> status code (0 = ok, error text set by the callee)
// (direct_in: the kernel reads every input byte once, so the smallest calls may let it read the pinned buffer itself)
// in2: a second input of in2_bytes_per_item per item, or NULL (then d_in2 is NULL): it is staged in the same device buffer as the
// first, behind it at the next 16-byte boundary, by a copy of its own where the two are not adjacent on the host.
template <int NOUT, class Launch>
int host_pipeline(const void *in, size_t in_bytes_per_item, const HostOut *outs, size_t items,
                  hipStream_t user_stream, Launch launch, bool direct_in = false, const void *in2 = nullptr, size_t in2_bytes_per_item = 0)
{
    if (!in2) in2_bytes_per_item = 0;
    static_assert(NOUT >= 1 && NOUT <= 5, "two staging sets of 1 + NOUT buffers share the 12 pool slots");
    constexpr int SET_SLOTS = NOUT <= 3 ? 4 : 1 + NOUT;        // pool slots per staging set
    // No stream given (the reference-shaped single-frame entries, every host-buffer call with opts == NULL): the calling THREAD's own
    // non-blocking stream, not the legacy null stream -- N host threads looping single-frame decodes (the unchanged-perftest shape,
    // perftest/src/main.rs:39-45) all queued on the one null stream and its synchronisation waited for every thread's work: 16 threads
    // delivered what 3 did (17 k calls/s; tests/c/threads_single_frame.c, round 6).  The call stays synchronous: it returns when its
    // results are in the caller's buffers.
    static const bool null_stream = ldpc::env_flag("LABRADOR_LDPC_HIP_NULL_STREAM");
    const bool own_stream = user_stream == nullptr;           // (a caller's stream is never left un-synchronised: it may be destroyed next)
    if (user_stream == nullptr && !null_stream) {             // (LABRADOR_LDPC_HIP_NULL_STREAM=1: the old behaviour, for A/B timing)
        HIP_TRY(g_pipe.ensure());
        user_stream = g_pipe.run;
    }
    {   // small call: pinned staging, one device block for all outputs
        size_t out_off[NOUT + 1];
        out_off[0] = 0;
        for (int o = 0; o < NOUT; ++o) out_off[o + 1] = (out_off[o] + items * outs[o].bytes_per_item + 15) / 16 * 16;
        const size_t in1_total = items * in_bytes_per_item, in1_pad = (in1_total + 15) / 16 * 16, in2_total = items * in2_bytes_per_item;
        const size_t in_total = in2 ? in1_pad + in2_total : in1_total, in_pad = (in_total + 15) / 16 * 16;
        if (in_pad + out_off[NOUT] <= SMALL_CALL_BYTES) {
            void *hbuf = nullptr, *dbuf_in = nullptr, *dbuf_out = nullptr;
            HIP_TRY(g_pinned.get(in_pad + out_off[NOUT], &hbuf));
            char *h_in = static_cast<char *>(hbuf), *h_out = h_in + in_pad;
            std::memcpy(h_in, in, in1_total);
            if (in2) std::memcpy(h_in + in1_pad, in2, in2_total);
            const bool direct = in_pad + out_off[NOUT] <= DIRECT_CALL_BYTES && g_pinned.dev != nullptr && direct_calls_enabled();
            char *const dev_in = static_cast<char *>(g_pinned.dev), *const dev_out = dev_in + in_pad;
            if (!(direct && direct_in)) {
                HIP_TRY(g_pool.get(0, in_pad, &dbuf_in));
                HIP_TRY(hipMemcpyAsync(dbuf_in, h_in, in_total, hipMemcpyHostToDevice, user_stream));
            } else {
                dbuf_in = dev_in;
            }
            if (!direct) HIP_TRY(g_pool.get(1, out_off[NOUT], &dbuf_out));
            void *d_outs[NOUT];
            for (int o = 0; o < NOUT; ++o) d_outs[o] = (direct ? dev_out : static_cast<char *>(dbuf_out)) + out_off[o];
            // (the launcher takes the request if this call is ONE kernel of ONE workgroup: notify.hpp)
            const bool ask = direct && direct_in && own_stream && notify_enabled();
            if (!ask || g_unsynced.on != user_stream) HIP_TRY(g_unsynced.retire());
            if (ask) ldpc::g_notify = ldpc::NotifyRequest{g_pinned.flag_dev(), g_pinned.ticket + 1, false};
            void *const dbuf_in2 = in2 ? static_cast<char *>(dbuf_in) + in1_pad : nullptr;
            const int st = launch(dbuf_in, dbuf_in2, d_outs, (size_t)0, items, user_stream);
            const bool notified = ldpc::g_notify.taken;
            ldpc::g_notify = ldpc::NotifyRequest{};
            if (notified) ++g_pinned.ticket;                  // (spent even if the launch then failed)
            if (st) return st;
            if (!direct) HIP_TRY(hipMemcpyAsync(h_out, dbuf_out, out_off[NOUT], hipMemcpyDeviceToHost, user_stream));
            if (notified) {
                HIP_TRY(wait_ticket(g_pinned.flag_host(), g_pinned.ticket, user_stream));
                g_unsynced.on = user_stream;
                if (++g_unsynced.calls >= 256) HIP_TRY(g_unsynced.retire());                 // (bounds what the runtime keeps)
            } else {
                HIP_TRY(hipStreamSynchronize(user_stream));
            }
            for (int o = 0; o < NOUT; ++o) std::memcpy(outs[o].host, h_out + out_off[o], items * outs[o].bytes_per_item);
            return LABRADOR_LDPC_HIP_OK;
        }
    }
    HIP_TRY(g_unsynced.retire());
    const size_t chunk_max = chunk_items(in_bytes_per_item + in2_bytes_per_item);
    const size_t chunk = items < chunk_max ? items : chunk_max;
    const size_t nchunks = (items + chunk - 1) / chunk;
    const int nsets = nchunks > 1 ? 2 : 1;
    void *d_in[2] = {}, *d_in2[2] = {}, *d_out[2][NOUT] = {};
    const size_t in2_at = (chunk * in_bytes_per_item + 15) / 16 * 16;          // the second input's place in a staging set's input buffer
    for (int s = 0; s < nsets; ++s) {
        HIP_TRY(g_pool.get(SET_SLOTS * s, in2 ? in2_at + chunk * in2_bytes_per_item : chunk * in_bytes_per_item, &d_in[s]));
        if (in2) d_in2[s] = static_cast<char *>(d_in[s]) + in2_at;
        for (int o = 0; o < NOUT; ++o) HIP_TRY(g_pool.get(SET_SLOTS * s + 1 + o, chunk * outs[o].bytes_per_item, &d_out[s][o]));
    }
    const char *src = static_cast<const char *>(in), *src2 = static_cast<const char *>(in2);

    if (nchunks == 1) {
        HIP_TRY(hipMemcpyAsync(d_in[0], src, items * in_bytes_per_item, hipMemcpyHostToDevice, user_stream));
        if (in2) HIP_TRY(hipMemcpyAsync(d_in2[0], src2, items * in2_bytes_per_item, hipMemcpyHostToDevice, user_stream));
        if (int st = launch(d_in[0], d_in2[0], d_out[0], (size_t)0, items, user_stream)) return st;
        for (int o = 0; o < NOUT; ++o)
            HIP_TRY(hipMemcpyAsync(outs[o].host, d_out[0][o], items * outs[o].bytes_per_item, hipMemcpyDeviceToHost, user_stream));
        HIP_TRY(hipStreamSynchronize(user_stream));
        return LABRADOR_LDPC_HIP_OK;
    }

    HIP_TRY(g_pipe.ensure());
    PipeStreams &ps = g_pipe;
    hipStream_t s_run = user_stream ? user_stream : ps.run;      // the legacy null stream would serialise the three legs
    struct Quiesce {                                             // nothing of ours may still touch the caller's memory on return
        hipStream_t a, b, c;
        ~Quiesce() { (void)hipStreamSynchronize(a); (void)hipStreamSynchronize(b); (void)hipStreamSynchronize(c); }
    } quiesce{ps.in, s_run, ps.out};

    // The copies to and from ordinary (pageable) host memory block the calling thread, so the
    // copy-out leg gets a thread of its own: this thread keeps the host->device copies back to
    // back (the leg that bounds the call), the collector drains results behind the kernels.
    struct Shared {
        std::mutex m;
        std::condition_variable cv;
        size_t issued = 0, collected = 0;          // chunks whose kernel is enqueued / whose results are out
        bool abort = false;
        int status = LABRADOR_LDPC_HIP_OK;
        std::string err;
    } sh;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));

    std::thread collector([&] {
        int st = LABRADOR_LDPC_HIP_OK;
        auto body = [&]() -> int {
            HIP_TRY(hipSetDevice(dev));
            for (size_t c = 0; c < nchunks; ++c) {
                {
                    std::unique_lock<std::mutex> lk(sh.m);
                    sh.cv.wait(lk, [&] { return sh.issued > c || sh.abort; });
                    if (sh.issued <= c) return LABRADOR_LDPC_HIP_OK;           // the issuing side failed
                }
                const int s = (int)(c & 1);
                const size_t f0 = c * chunk, nb = items - f0 < chunk ? items - f0 : chunk;
                HIP_TRY(hipStreamWaitEvent(ps.out, ps.ev_run[s], 0));
                for (int o = 0; o < NOUT; ++o)
                    HIP_TRY(hipMemcpyAsync(static_cast<char *>(outs[o].host) + f0 * outs[o].bytes_per_item, d_out[s][o],
                                           nb * outs[o].bytes_per_item, hipMemcpyDeviceToHost, ps.out));
                HIP_TRY(hipStreamSynchronize(ps.out));
                {
                    std::lock_guard<std::mutex> lk(sh.m);
                    sh.collected = c + 1;
                }
                sh.cv.notify_all();
            }
            return LABRADOR_LDPC_HIP_OK;
        };
        st = body();
        if (st != LABRADOR_LDPC_HIP_OK) {
            std::lock_guard<std::mutex> lk(sh.m);
            sh.abort = true; sh.status = st; sh.err = g_err;                   // g_err is this thread's own copy
        }
        sh.cv.notify_all();
    });

    auto issue_all = [&]() -> int {
        for (size_t c = 0; c < nchunks; ++c) {
            const int s = (int)(c & 1);
            const size_t f0 = c * chunk, nb = items - f0 < chunk ? items - f0 : chunk;
            if (c >= 2) {                                                      // staging set s is free once chunk c-2 is out
                std::unique_lock<std::mutex> lk(sh.m);
                sh.cv.wait(lk, [&] { return sh.collected + 2 > c || sh.abort; });
                if (sh.abort) return LABRADOR_LDPC_HIP_OK;                     // the collector's status is reported below
            }
            HIP_TRY(hipMemcpyAsync(d_in[s], src + f0 * in_bytes_per_item, nb * in_bytes_per_item, hipMemcpyHostToDevice, ps.in));
            if (in2) HIP_TRY(hipMemcpyAsync(d_in2[s], src2 + f0 * in2_bytes_per_item, nb * in2_bytes_per_item, hipMemcpyHostToDevice, ps.in));
            HIP_TRY(hipEventRecord(ps.ev_in[s], ps.in));
            HIP_TRY(hipStreamWaitEvent(s_run, ps.ev_in[s], 0));
            if (int st = launch(d_in[s], d_in2[s], d_out[s], f0, nb, s_run)) return st;
            HIP_TRY(hipEventRecord(ps.ev_run[s], s_run));
            {
                std::lock_guard<std::mutex> lk(sh.m);
                sh.issued = c + 1;
            }
            sh.cv.notify_all();
        }
        return LABRADOR_LDPC_HIP_OK;
    };
    const int st_issue = issue_all();
    if (st_issue != LABRADOR_LDPC_HIP_OK) {
        std::lock_guard<std::mutex> lk(sh.m);
        sh.abort = true;
    }
    sh.cv.notify_all();
    collector.join();
    if (st_issue != LABRADOR_LDPC_HIP_OK) return st_issue;
    if (sh.status != LABRADOR_LDPC_HIP_OK) { g_err = sh.err; return sh.status; }
    HIP_TRY(hipStreamSynchronize(s_run));
    return LABRADOR_LDPC_HIP_OK;
}

// ---- device-resident batches of any size ------------------------------------------------------------
// The kernels take a 32-bit frame count.  A device-resident batch is enqueued as launches of at most
// 2^30 frames (a multiple of every kernel's codewords-per-workgroup and of the 8-byte output alignment),
// so no size_t batch is ever truncated.
constexpr size_t MAX_LAUNCH_FRAMES = (size_t)1 << 30;

// (LABRADOR_LDPC_HIP_MAX_LAUNCH=<frames, a multiple of 8> lowers the slice for tests)
size_t max_launch_frames()
{
    if (const char *env = std::getenv("LABRADOR_LDPC_HIP_MAX_LAUNCH")) {
        const long long v = std::atoll(env);
        if (v >= 8 && (size_t)v <= MAX_LAUNCH_FRAMES && v % 8 == 0) return (size_t)v;
    }
    return MAX_LAUNCH_FRAMES;
}

template <class Launch>                                        // launch(first_frame, frames) -> hipError_t
hipError_t for_launch_slices(size_t batch, Launch launch)
{
    const size_t slice = max_launch_frames();
    for (size_t f0 = 0; f0 < batch; f0 += slice) {
        const size_t nb = batch - f0 < slice ? batch - f0 : slice;
        if (hipError_t e = launch(f0, nb); e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace
