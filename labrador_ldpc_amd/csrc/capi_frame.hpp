// capi_frame.hpp -- part of capi.hip: what every batched entry point shares.  The one batched call path (device set, device
// buffers in launch slices, host buffers through the pipeline), the call frame of the min-sum entries, the call frame of the
// element-wise converters, and the two corrections of the check messages as values.  The ORDER of a frame's steps is part of the
// ABI -- it decides which fault a call with two faults reports -- and is written here once.
#pragma once

namespace {

// ---- the corrections of the check messages, as the entries carry them ------------------------------------------------------------
// Normalized / offset min-sum in floats: 0 < scale <= 1 and 0 <= offset <= FLT_MAX: with these the correction of a
// finite magnitude is finite and never NaN.  The default is the identity, which passes.
struct Correction {
    float scale = 1.0f, offset = 0.0f;
    bool identity() const { return scale == 1.0f && offset == 0.0f; }
    int check() const
    {
        if (!(scale > 0.0f && scale <= 1.0f)) return fail(LABRADOR_LDPC_HIP_EINVAL, "scale %g is not in (0, 1]", (double)scale);
        if (!(offset >= 0.0f && offset <= std::numeric_limits<float>::max()))
            return fail(LABRADOR_LDPC_HIP_EINVAL, "offset %g is not in [0, FLT_MAX]", (double)offset);
        return LABRADOR_LDPC_HIP_OK;
    }
};
// ... in integers: 0 <= scale_shift <= 8, 1 <= scale_num <= 1 << scale_shift and 0 <= offset <= T's maximum: with
// these scale_num * m + half fits 32 bits for every magnitude m of T and the corrected magnitude is at most m.  The default is the
// identity, which passes; so does every triple for a T that is no integer, where no entry takes one.
struct FixedCorrection {
    uint32_t scale_num = 1, scale_shift = 0, offset = 0;
    bool identity() const { return scale_num == 1u << scale_shift && offset == 0; }
    template <class T>
    int check() const
    {
        if constexpr (std::is_integral_v<T>) {
            constexpr uint32_t tmax = (uint32_t)std::numeric_limits<T>::max();
            if (scale_shift > 8) return fail(LABRADOR_LDPC_HIP_EINVAL, "scale_shift %u is not in 0 .. 8", scale_shift);
            if (scale_num < 1 || scale_num > (1u << scale_shift))
                return fail(LABRADOR_LDPC_HIP_EINVAL, "scale_num %u is not in 1 .. 1 << scale_shift (%u)", scale_num, 1u << scale_shift);
            if (offset > tmax) return fail(LABRADOR_LDPC_HIP_EINVAL, "offset %u is not in 0 .. %u", offset, tmax);
        }
        return LABRADOR_LDPC_HIP_OK;
    }
};

// ---- one batched call path ------------------------------------------------------------------------------------------------------
// The buffers of a batched call: one input and up to five outputs, each an address and its bytes per item.  Item f of a buffer
// starts f * bytes behind its address -- the only pointer arithmetic of the shard re-entry, the device slices and the staged call.
// An output that is not there (a hard-only decode's `app`) is NULL and stays NULL; so does the second input, which one entry has
// (the erasure rows of the packed hard-decision decode).
struct Buffers {
    const void *in;
    size_t in_bytes;
    HostOut out[5];
    const void *in2 = nullptr;
    size_t in2_bytes = 0;
    Buffers from(size_t item) const
    {
        Buffers b = *this;
        b.in = static_cast<const char *>(in) + item * in_bytes;
        if (in2) b.in2 = static_cast<const char *>(in2) + item * in2_bytes;
        for (HostOut &o : b.out)
            if (o.host) o.host = static_cast<char *>(o.host) + item * o.bytes_per_item;
        return b;
    }
};
// a launch that takes the second input takes it behind the first: launch(in, in2, ...), else launch(in, ...).  The form is chosen by
// what the launch can be called with, so every launch handed to batched_call is a lambda with CONCRETE parameter types: a generic one
// (auto parameters) would be callable both ways and get `in2` where it expects its outputs.  minsum_call's slice launch takes `in2`
// for every min-sum entry -- NULL for all but the packed hard-decision ones -- so that the frame stays one function.
template <class Launch, class... Rest>
auto launch_with(const Launch &launch, const void *in, const void *in2, Rest... rest)
{
    if constexpr (std::is_invocable_v<const Launch &, const void *, const void *, Rest...>) return launch(in, in2, rest...);
    else return launch(in, rest...);
}

// What a batched entry does once its own arguments are checked: over a device set, every device's worker runs its share of the
// items through this function again; device-resident buffers are checked by the entry (device_checks() -> status, the text its own)
// and launched in slices on opts->stream; host buffers are staged through the pipeline.  launch(in, outs, n_items, stream) ->
// hipError_t enqueues the entry's kernel; status_of(hipError_t) -> status says what a failed launch means and sets its text.  The
// three are copied into the workers' jobs, so they hold what they need by value.
template <int NOUT, class Launch, class StatusOf, class DeviceChecks>
int batched_call(const Buffers &b, size_t batch, const labrador_ldpc_hip_opts *opts, const Launch &launch, const StatusOf &status_of,
                 const DeviceChecks &device_checks, bool direct_in = false)
{
    std::vector<int> devs;
    if (int s = device_set(opts, devs)) return s;
    if (!devs.empty())
        return run_sharded(devs, batch, opts->variant, [=](size_t f0, size_t nb, const labrador_ldpc_hip_opts *o) -> int {
            return batched_call<NOUT>(b.from(f0), nb, o, launch, status_of, device_checks, direct_in);
        });

    DeviceScope scope;
    if (int s = scope.enter(opts)) return s;
    hipStream_t stream = opts ? (hipStream_t)opts->stream : nullptr;
    if (opts && opts->memory == LABRADOR_LDPC_HIP_MEM_DEVICE) {
        if (int s = device_checks()) return s;
        return status_of(for_launch_slices(batch, [&](size_t f0, size_t nb) {
            const Buffers slice = b.from(f0);
            void *outs[NOUT];
            for (int o = 0; o < NOUT; ++o) outs[o] = slice.out[o].host;
            return launch_with(launch, slice.in, slice.in2, (void *const *)outs, nb, stream);
        }));
    }
    if (opts && opts->memory != LABRADOR_LDPC_HIP_MEM_HOST) return fail(LABRADOR_LDPC_HIP_EINVAL, "bad opts->memory");

    // host buffers: staged in chunks (arbitrarily large batches fit), copies overlapped with the kernel
    return host_pipeline<NOUT>(b.in, b.in_bytes, b.out, batch, stream,
                               [&](void *d_in, void *d_in2, void *const *d_out, size_t, size_t nb, hipStream_t st) -> int {
        return status_of(launch_with(launch, (const void *)d_in, (const void *)d_in2, d_out, nb, st));
    }, direct_in, b.in2, b.in2_bytes);
}

// status_of of the entries outside min-sum: "<name> launch: <the runtime's text>"
auto launch_status(const char *name)
{
    return [=](hipError_t e) -> int {
        if (e != hipSuccess) return fail(LABRADOR_LDPC_HIP_ERUNTIME, "%s launch: %s", name, hipGetErrorString(e));
        return LABRADOR_LDPC_HIP_OK;
    };
}

// ---- the call frame of the batched min-sum entries --------------------------------------------------------------------------------
// The buffers of a min-sum call -- the caller's, and again a launch's share of them, on the device.  `stage` [batch] exists for the
// cascade entries and `app` [batch][n + p], in elements of A, for the soft ones; an `app` given to an entry without one is ignored.
// `mask` exists for the packed hard-decision entries, whose rows -- input and mask alike -- are n / 8 bytes (`packed`); it may be NULL.
template <class In, class A>
struct MsBuffers {
    const In *llrs;
    uint8_t *output;
    uint32_t *iters;
    uint8_t *success;
    uint8_t *stage = nullptr;
    A *app = nullptr;
    bool has_stage = false, has_app = false;
    const In *mask = nullptr;
    bool packed = false;
};
// what a launch runs at: the code, opts->variant, and the caller's caps clamped to the kernels' 32 bits
struct MsRun {
    int code, variant;
    uint32_t maxit, maxsw;
};
// what an entry wants of the device side of a call
struct MsDevice {
    const char *unsupported;                          // the EUNSUPPORTED text of hipErrorInvalidConfiguration, a format of (variant, code)
    size_t llrs_align = 0;                            // with MEM_DEVICE `llrs` (and `mask`) has this alignment, else EINVAL; 0 asks for nothing
    // does the launch read every LLR exactly once?  Then the smallest host calls may let it read them across the link.
    bool (*reads_llrs_once)(int code, int variant) = [](int, int) { return false; };
    const char *llrs_name = "llrs";                   // what the entry calls its input in the alignment's text
};

// Every batched min-sum entry is this function and what it passes to it.  The steps, in the order that is the ABI's:
//   1 the error is cleared  2 opts are normalised  3 the code's range  4 early(): the entry's float pairs and quantiser, checked even
//   for an empty batch  5 the empty batch is OK  6 "NULL buffer"  7 late(): the entry's integer triples  8 the caps are clamped
//   9 support(variant, code): what the entry has no kernel for, EUNSUPPORTED with the arguments  10 the buffers, outputs in the order
//   output, iters, success, [stage], [app]  11 a failed launch's status  12 the device checks: output % 8, app % 16, llrs % align,
//   [mask % align].
// launch(MsRun, the slice's MsBuffers, frames, stream) -> hipError_t enqueues the decode; it and `dev` are copied into the workers'
// jobs of a sharded call, so they hold what they need by value.  Everything is a template parameter: nothing here allocates.
template <class In, class A, class Early, class Late, class Support, class Launch>
int minsum_call(int code, MsBuffers<In, A> b, size_t batch, size_t max_iters, size_t max_sweeps, const labrador_ldpc_hip_opts *opts,
                const MsDevice &dev, const Early &early, const Late &late, const Support &support, const Launch &launch)
{
    g_err.clear();
    labrador_ldpc_hip_opts opts_local;
    opts = normalise_opts(opts, opts_local);
    if (!ldpc::valid_code(code)) return fail(LABRADOR_LDPC_HIP_EINVAL, "code %d out of range", code);
    if (int s = early()) return s;
    if (batch == 0) return LABRADOR_LDPC_HIP_OK;
    if (!b.has_app) b.app = nullptr;
    if (!b.llrs || (b.has_app && !b.app) || !b.output || !b.iters || !b.success || (b.has_stage && !b.stage))
        return fail(LABRADOR_LDPC_HIP_EINVAL, "NULL buffer");
    if (int s = late()) return s;
    constexpr uint32_t CAP_MAX = 0xFFFFFFFEu;
    auto cap = [](size_t v) { return v > CAP_MAX ? CAP_MAX : (uint32_t)v; };
    const MsRun run{code, opts ? opts->variant : 0, cap(max_iters), cap(max_sweeps)};
    if (int s = support(run.variant, code)) return s;

    const ldpc::CodeInfo &ci = ldpc::CODES[code];
    const int app_at = b.has_stage ? 4 : 3;
    const size_t row_bytes = (b.packed ? (size_t)ci.n / 8 : (size_t)ci.n) * sizeof(In);
    Buffers bufs{b.llrs, row_bytes, {{b.output, (size_t)ci.output_len()}, {b.iters, sizeof(uint32_t)}, {b.success, 1}}};
    if (b.mask) bufs.in2 = b.mask, bufs.in2_bytes = row_bytes;
    if (b.has_stage) bufs.out[3] = {b.stage, 1};
    bufs.out[app_at] = {b.app, ((size_t)ci.n + ci.p) * sizeof(A)};
    auto slice_launch = [=](const void *in, const void *in2, void *const *out, size_t nb, hipStream_t st) {
        MsBuffers<In, A> s = b;
        s.mask = (const In *)in2;
        s.llrs = (const In *)in, s.output = (uint8_t *)out[0], s.iters = (uint32_t *)out[1], s.success = (uint8_t *)out[2];
        if (b.has_stage) s.stage = (uint8_t *)out[3];
        if (b.app) s.app = (A *)out[app_at];
        return launch(run, s, nb, st);
    };
    auto status_of = [=](hipError_t e) -> int {
        if (e == hipErrorInvalidConfiguration) return fail(LABRADOR_LDPC_HIP_EUNSUPPORTED, dev.unsupported, run.variant, code);
        if (e != hipSuccess) return fail(LABRADOR_LDPC_HIP_ERUNTIME, "kernel launch: %s", hipGetErrorString(e));
        return LABRADOR_LDPC_HIP_OK;
    };
    auto device_checks = [=]() -> int {
        if ((uintptr_t)b.output % 8) return fail(LABRADOR_LDPC_HIP_EINVAL, "device output buffer must be 8-byte aligned");
        if (b.app && (uintptr_t)b.app % 16) return fail(LABRADOR_LDPC_HIP_EINVAL, "device app buffer must be 16-byte aligned");
        if (dev.llrs_align && (uintptr_t)b.llrs % dev.llrs_align)
            return fail(LABRADOR_LDPC_HIP_EINVAL, "device %s buffer must be %zu-byte aligned", dev.llrs_name, dev.llrs_align);
        if (b.mask && dev.llrs_align && (uintptr_t)b.mask % dev.llrs_align)
            return fail(LABRADOR_LDPC_HIP_EINVAL, "device erasures buffer must be %zu-byte aligned", dev.llrs_align);
        return LABRADOR_LDPC_HIP_OK;
    };
    const bool direct_in = dev.reads_llrs_once(code, run.variant);
    switch (3 + (b.has_stage ? 1 : 0) + (b.app ? 1 : 0)) {
        case 3: return batched_call<3>(bufs, batch, opts, slice_launch, status_of, device_checks, direct_in);
        case 4: return batched_call<4>(bufs, batch, opts, slice_launch, status_of, device_checks, direct_in);
        default: return batched_call<5>(bufs, batch, opts, slice_launch, status_of, device_checks, direct_in);
    }
}
// for an entry that has none of a frame's checks
constexpr auto NO_CHECK = [](auto...) { return LABRADOR_LDPC_HIP_OK; };

// ---- the call frame of the element-wise converters --------------------------------------------------------------------------------
// Packed bits <-> LLRs, f32 -> i8 / i16, f16 / bf16 -> f32: host buffers are converted where they lie (the data is on the host and
// the conversion is cheaper than the PCIe crossing), device buffers by a streaming kernel on opts->stream, asynchronously.  The steps:
// the code, check() (the entry's own parameters, before the empty batch), the empty batch, NULL, host(n) for MEM_HOST or no opts, "bad
// opts->memory", the 16-byte alignment of the `aligned` device buffers in their order -- BEFORE the device is selected, unlike the
// decoders' and the encoder's device checks -- the device, and launch(n, stream) -> hipError_t, reported as "<name> launch: ...".
struct DeviceBuffer {
    const void *p;
    const char *what;
};
template <class Check, class Host, class Launch>
int convert_call(const char *name, int code, const void *in, void *out, size_t batch, const labrador_ldpc_hip_opts *opts,
                 std::initializer_list<DeviceBuffer> aligned, const Check &check, const Host &host, const Launch &launch)
{
    g_err.clear();
    labrador_ldpc_hip_opts opts_local;
    opts = normalise_opts(opts, opts_local);
    if (!ldpc::valid_code(code)) return fail(LABRADOR_LDPC_HIP_EINVAL, "code %d out of range", code);
    if (int s = check()) return s;
    if (batch == 0) return LABRADOR_LDPC_HIP_OK;
    if (!in || !out) return fail(LABRADOR_LDPC_HIP_EINVAL, "NULL buffer");
    const size_t n = ldpc::CODES[code].n;
    if (!opts || opts->memory == LABRADOR_LDPC_HIP_MEM_HOST) {
        host(n);
        return LABRADOR_LDPC_HIP_OK;
    }
    if (opts->memory != LABRADOR_LDPC_HIP_MEM_DEVICE) return fail(LABRADOR_LDPC_HIP_EINVAL, "bad opts->memory");
    for (const DeviceBuffer &d : aligned)
        if ((uintptr_t)d.p % 16) return fail(LABRADOR_LDPC_HIP_EINVAL, "device %s buffer must be 16-byte aligned", d.what);
    DeviceScope scope;
    if (int s = scope.enter(opts)) return s;
    return launch_status(name)(launch(n, (hipStream_t)opts->stream));
}

}  // namespace
