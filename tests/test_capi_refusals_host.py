"""What the C ABI's batched entry points refuse, and in which order: raw calls -> (status, a piece of last_error()).

Every family goes through the same host call path (csrc/capi.hip); this table pins what that path answers before it touches a
device, so that it can be rewritten without the answers moving.  Where the outcome depends on a device being present the
expectation branches on device_count(), as test_capi_host.py does.  TC128, batch 2; nothing here needs a GPU."""
import ctypes

import numpy as np
import pytest

import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode, HipOpts, MEM_HOST, MEM_DEVICE

OK, EINVAL, ENODEV, EUNSUPPORTED = 0, -1, -2, -4
CODE, BAD_CODE, BATCH = int(LDPCCode.TC128), 9, 2
GPU = la.device_count() > 0

# one buffer every pointer argument may point into: large enough for any argument of a batch-2 TC128 call, 16-byte aligned
_ARENA = np.zeros(1 << 16, dtype=np.uint8)
BUF = (_ARENA.ctypes.data + 15) // 16 * 16

# family -> (symbol, pointer arguments, arguments between batch and opts)
FAMILIES = {
    "bf": ("labrador_ldpc_decode_bf_batch", 4, (10,)),
    "encode": ("labrador_ldpc_encode_batch", 2, ()),
    "ms_batch_f32": ("labrador_ldpc_decode_ms_batch_f32", 4, (10,)),
    "ms_soft_batch_i8": ("labrador_ldpc_decode_ms_soft_batch_i8", 5, (10,)),
    "layered_batch_f32": ("labrador_ldpc_decode_ms_layered_batch_f32", 4, (10,)),
    "layered_corrected_batch_f32": ("labrador_ldpc_decode_ms_layered_corrected_batch_f32", 4, (10, 0.75, 0.0)),
    "layered_fixed_batch_i8": ("labrador_ldpc_decode_ms_layered_fixed_batch_i8", 4, (10,)),
    "hard_to_llrs_batch_f32": ("labrador_ldpc_hard_to_llrs_batch_f32", 2, ()),
    "llrs_to_hard_batch_i16": ("labrador_ldpc_llrs_to_hard_batch_i16", 2, ()),
}
ALL = sorted(FAMILIES)
SKELETONS = ["bf", "encode", "ms_batch_f32"]        # the three bodies that select a device set


def call(family, code=CODE, bufs=None, batch=BATCH, tail=None, opts=None):
    """-> (status, last_error()).  bufs: None = every pointer valid, else one address (or None) per pointer argument."""
    sym, nbuf, default_tail = FAMILIES[family]
    bufs = [BUF + 4096 * i for i in range(nbuf)] if bufs is None else bufs
    assert len(bufs) == nbuf
    st = getattr(la.lib, sym)(code, *bufs, batch, *(default_tail if tail is None else tail),
                              ctypes.byref(opts) if opts is not None else None)
    return st, la.last_error()


def nulls(family):
    return [None] * FAMILIES[family][1]


def refused(got, status, text):
    assert got[0] == status and text in got[1], got


# ---- the argument checks every family shares, in their order ----------------------------------------------------------------------
@pytest.mark.parametrize("family", ALL)
def test_bad_code_comes_before_null_buffers_and_before_an_empty_batch(family):
    refused(call(family, code=BAD_CODE, bufs=nulls(family)), EINVAL, "out of range")
    refused(call(family, code=BAD_CODE, batch=0), EINVAL, "out of range")
    refused(call(family, code=-1, batch=0, bufs=nulls(family)), EINVAL, "out of range")


@pytest.mark.parametrize("family", ALL)
def test_an_empty_batch_is_ok_whatever_the_buffers(family):
    assert call(family, batch=0, bufs=nulls(family)) == (OK, "")
    assert call(family, batch=0, bufs=nulls(family), opts=HipOpts(-1, MEM_DEVICE, None, 0, 0, None)) == (OK, "")


@pytest.mark.parametrize("family", ALL)
def test_each_null_buffer_is_refused(family):
    nbuf = FAMILIES[family][1]
    for i in range(nbuf):
        bufs = [BUF + 4096 * k for k in range(nbuf)]
        bufs[i] = None
        refused(call(family, bufs=bufs), EINVAL, "NULL buffer")


# ---- the corrected layered entries: scale and offset are checked with the arguments, before the empty batch -----------------------
@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
def test_corrected_entries_check_scale_and_offset_even_for_an_empty_batch(soft):
    sym = "labrador_ldpc_decode_ms_layered_corrected_soft_batch_f32" if soft else "labrador_ldpc_decode_ms_layered_corrected_batch_f32"
    fn = getattr(la.lib, sym)
    bufs = [None] * (5 if soft else 4)
    for scale, offset, text in ((0.0, 0.0, "scale"), (1.5, 0.0, "scale"), (1.0, -1.0, "offset"), (1.0, float("nan"), "offset"),
                                (float("nan"), 0.0, "scale"), (0.0, -1.0, "scale")):
        st = fn(CODE, *bufs, 0, 10, scale, offset, None)
        assert st == EINVAL and text in la.last_error() and "is not in" in la.last_error(), (scale, offset, la.last_error())
    assert fn(BAD_CODE, *bufs, 0, 10, 1.5, 0.0, None) == EINVAL and "out of range" in la.last_error()
    assert fn(CODE, *bufs, 0, 10, 1.0, 0.0, None) == OK and la.last_error() == ""


# ---- the fixed-point layered entries: variant 0 is the only kernel, said with the argument checks ---------------------------------
@pytest.mark.parametrize("sym,nbuf", [("labrador_ldpc_decode_ms_layered_fixed_batch_i8", 4), ("labrador_ldpc_decode_ms_layered_fixed_batch_i16", 4),
                                      ("labrador_ldpc_decode_ms_layered_fixed_soft_batch_i8", 5)])
def test_fixed_layered_variant_is_checked_after_the_buffers_and_before_the_device_set(sym, nbuf):
    fn = getattr(la.lib, sym)
    good = [BUF + 4096 * i for i in range(nbuf)]
    o = HipOpts(-1, MEM_HOST, None, 7, 0, None)
    assert fn(CODE, *([None] + good[1:]), BATCH, 10, ctypes.byref(o)) == EINVAL and "NULL buffer" in la.last_error()
    assert fn(CODE, *good, 0, 10, ctypes.byref(o)) == OK                    # an empty batch never gets as far as the variant
    devs = (ctypes.c_int * 2)(0, 0)
    o = HipOpts(-1, MEM_HOST, 0x1234, 7, 2, devs)                           # a device list with a stream is itself refused -- later
    assert fn(CODE, *good, BATCH, 10, ctypes.byref(o)) == EUNSUPPORTED and "variant 7" in la.last_error()
    o = HipOpts(-3, 2, None, 7, -1, None)                                   # ... as are these opts
    assert fn(CODE, *good, BATCH, 10, ctypes.byref(o)) == EUNSUPPORTED and "variant" in la.last_error()


# ---- device selection: everything that is refused before a device is asked for -----------------------------------------------------
@pytest.mark.parametrize("family", SKELETONS + ["ms_soft_batch_i8", "layered_corrected_batch_f32"])
def test_device_set_refusals(family):
    devs = (ctypes.c_int * 2)(0, 0)
    refused(call(family, opts=HipOpts(-1, MEM_HOST, None, 0, -1, None)), EINVAL, "opts->n_devices is negative")
    refused(call(family, opts=HipOpts(-3, MEM_HOST, None, 0, 0, None)), EINVAL, "bad opts->device -3")
    refused(call(family, opts=HipOpts(-3, MEM_HOST, None, 0, -1, None)), EINVAL, "opts->n_devices is negative")
    refused(call(family, opts=HipOpts(-1, MEM_DEVICE, None, 0, 2, devs)), EINVAL, "needs MEM_HOST")
    refused(call(family, opts=HipOpts(-1, MEM_DEVICE, 0x1234, 0, 2, devs)), EINVAL, "needs MEM_HOST")
    refused(call(family, opts=HipOpts(-1, 2, None, 0, 2, devs)), EINVAL, "needs MEM_HOST")
    refused(call(family, opts=HipOpts(-1, MEM_HOST, 0x1234, 0, 2, devs)), EINVAL, "must be NULL")
    refused(call(family, opts=HipOpts(la.DEVICE_ALL, MEM_DEVICE, None, 0, 0, None)), EINVAL, "needs MEM_HOST")
    refused(call(family, opts=HipOpts(la.DEVICE_ALL, MEM_HOST, 0x1234, 0, 0, None)), EINVAL, "must be NULL")
    # the list itself is looked at only once a device is known to exist
    got = call(family, opts=HipOpts(-1, MEM_HOST, None, 0, 2, None))
    refused(got, EINVAL, "devices is NULL") if GPU else refused(got, ENODEV, "no HIP device")
    bad = (ctypes.c_int * 2)(0, 4096)
    got = call(family, opts=HipOpts(-1, MEM_HOST, None, 0, 2, bad))
    refused(got, EINVAL, "devices[1] = 4096 out of range") if GPU else refused(got, ENODEV, "no HIP device")


@pytest.mark.parametrize("family", SKELETONS)
def test_single_device_refusals_follow_device_selection(family):
    """`memory` and the device-buffer alignment are looked at only with a device selected: without one the call is ENODEV."""
    got = call(family, opts=HipOpts(-1, 2, None, 0, 0, None))
    refused(got, EINVAL, "bad opts->memory") if GPU else refused(got, ENODEV, "no HIP device")
    got = call(family, opts=HipOpts(4096, MEM_HOST, None, 0, 0, None))
    refused(got, EINVAL, "device 4096 out of range") if GPU else refused(got, ENODEV, "no HIP device")


def test_ms_batch_device_buffer_alignment_is_checked_after_device_selection():
    bufs = [BUF, BUF + 4096 + 4, BUF + 8192, BUF + 12288]                   # output: 4-byte but not 8-byte aligned
    got = call("ms_batch_f32", bufs=bufs, opts=HipOpts(-1, MEM_DEVICE, None, 0, 0, None))
    refused(got, EINVAL, "device output buffer must be 8-byte aligned") if GPU else refused(got, ENODEV, "no HIP device")
    bufs = [BUF, BUF + 4096 + 4, BUF + 8192, BUF + 12288, BUF + 16384]      # app (the second pointer of a soft call): not 16-byte aligned
    got = call("ms_soft_batch_i8", bufs=bufs, opts=HipOpts(-1, MEM_DEVICE, None, 0, 0, None))
    refused(got, EINVAL, "device app buffer must be 16-byte aligned") if GPU else refused(got, ENODEV, "no HIP device")


# ---- batched LLR helpers: host buffers need no device, and their alignment check PRECEDES device selection ---------------------------
@pytest.mark.parametrize("suffix,dtype", [("i8", np.int8), ("i16", np.int16), ("i32", np.int32), ("f32", np.float32), ("f64", np.float64)])
def test_llr_batch_on_host_buffers_equals_the_per_frame_helpers(suffix, dtype):
    code = LDPCCode.TC128
    n, batch = code.n(), 3
    rng = np.random.default_rng(7)
    hard = rng.integers(0, 256, (batch, n // 8), dtype=np.uint8)
    want = np.zeros((batch, n), dtype=dtype)
    for f in range(batch):
        code.hard_to_llrs(hard[f], want[f])
    for opts in (None, HipOpts(-1, MEM_HOST, None, 0, 0, None), HipOpts(4096, MEM_HOST, 0x1234, 7, 0, None)):
        o = ctypes.byref(opts) if opts is not None else None
        llrs = np.zeros((batch, n), dtype=dtype)
        assert getattr(la.lib, "labrador_ldpc_hard_to_llrs_batch_" + suffix)(int(code), hard.ctypes.data, llrs.ctypes.data, batch, o) == OK
        assert (llrs == want).all() and set(np.unique(llrs).tolist()) == {-1, 1}
        noisy = (llrs * 3).astype(dtype)
        noisy[0, 5] = 0                                                      # zero is not negative: the bit stays clear
        back = np.full((batch, n // 8), 0xFF, dtype=np.uint8)
        assert getattr(la.lib, "labrador_ldpc_llrs_to_hard_batch_" + suffix)(int(code), noisy.ctypes.data, back.ctypes.data, batch, o) == OK
        per_frame = np.zeros_like(back)
        for f in range(batch):
            code.llrs_to_hard(noisy[f], per_frame[f])
        assert (back == per_frame).all()
        assert (back.reshape(-1)[1:] == hard.reshape(-1)[1:]).all() and back[0, 0] == hard[0, 0] & ~np.uint8(0x80 >> 5)


@pytest.mark.parametrize("family,llrs_at", [("hard_to_llrs_batch_f32", 1), ("llrs_to_hard_batch_i16", 0)])
def test_llr_batch_memory_and_alignment_are_checked_before_device_selection(family, llrs_at):
    refused(call(family, opts=HipOpts(-1, 2, None, 0, 0, None)), EINVAL, "bad opts->memory")
    refused(call(family, opts=HipOpts(4096, 2, None, 0, 0, None)), EINVAL, "bad opts->memory")
    bufs = [BUF, BUF + 4096]
    bufs[llrs_at] += 4                                                       # 4-byte but not 16-byte aligned
    refused(call(family, bufs=bufs, opts=HipOpts(-1, MEM_DEVICE, None, 0, 0, None)), EINVAL, "device llrs buffer must be 16-byte aligned")
    refused(call(family, bufs=bufs, opts=HipOpts(4096, MEM_DEVICE, None, 0, 0, None)), EINVAL, "16-byte aligned")
    # the other buffer's alignment is nobody's business; with aligned llrs the call goes on to select the device
    bufs = [BUF, BUF + 4096]
    bufs[1 - llrs_at] += 1
    got = call(family, bufs=bufs, opts=HipOpts(4096, MEM_DEVICE, None, 0, 0, None))
    refused(got, EINVAL, "device 4096 out of range") if GPU else refused(got, ENODEV, "no HIP device")


# ---- the channel ---------------------------------------------------------------------------------------------------------------------
def test_awgn_i8_checks_lim_first_then_the_code_then_the_pool():
    for name, first in (("labrador_ldpc_hip_awgn_i8", ()), ("labrador_ldpc_hip_awgn_i8_at", (5,))):
        fn = getattr(la.lib, name)
        for lim in (200, 128, -1):
            assert fn(BAD_CODE, None, 0, None, *first, BATCH, 1.0, 8.0, lim, 1, None) == EINVAL and "lim must be in 0..127" in la.last_error()
        assert fn(BAD_CODE, None, 0, None, *first, BATCH, 1.0, 8.0, 127, 1, None) == EINVAL and "out of range" in la.last_error()
        assert fn(CODE, None, 0, None, *first, 0, 1.0, 8.0, 31, 1, None) == OK
        assert fn(CODE, BUF, 0, BUF + 4096, *first, BATCH, 1.0, 8.0, 31, 1, None) == EINVAL and "bad codeword pool" in la.last_error()
        assert fn(CODE, None, 4, BUF + 4096, *first, BATCH, 1.0, 8.0, 31, 1, None) == EINVAL and "bad codeword pool" in la.last_error()
        assert fn(CODE, BUF, 1 << 32, BUF + 4096, *first, BATCH, 1.0, 8.0, 31, 1, None) == EINVAL and "bad codeword pool" in la.last_error()
        assert fn(CODE, BUF, 4, BUF + 4096 + 4, *first, BATCH, 1.0, 8.0, 31, 1, None) == EINVAL and "llrs must be 16-byte aligned" in la.last_error()
    for name, first in (("labrador_ldpc_hip_awgn_f32", ()), ("labrador_ldpc_hip_awgn_f32_at", (5,))):
        fn = getattr(la.lib, name)
        assert fn(BAD_CODE, None, 0, None, *first, BATCH, 1.0, 1, None) == EINVAL and "out of range" in la.last_error()
        assert fn(CODE, BUF, 0, BUF + 4096, *first, BATCH, 1.0, 1, None) == EINVAL and "bad codeword pool" in la.last_error()


# ---- device-resident parts on several GPUs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("suffix", ["f32", "i8"])
def test_multi_argument_checks(suffix):
    fn = getattr(la.lib, f"labrador_ldpc_decode_ms_batch_{suffix}_multi")
    assert fn(BAD_CODE, 0, None, None, None, None, None, None, 10, 0) == EINVAL and "out of range" in la.last_error()
    assert fn(CODE, 0, None, None, None, None, None, None, 10, 0) == OK and la.last_error() == ""
    devs, frames = (ctypes.c_int * 2)(0, 4096), (ctypes.c_size_t * 2)(0, BATCH)
    ptrs = [(ctypes.c_void_p * 2)(None, BUF + 4096 * i) for i in range(4)]
    addr = lambda a: ctypes.cast(a, ctypes.c_void_p).value
    args = [addr(devs)] + [addr(p) for p in ptrs] + [addr(frames)]
    assert fn(CODE, 1025, *args, 10, 0) == EINVAL and "too many parts" in la.last_error()
    for i in range(len(args)):
        holed = list(args)
        holed[i] = None
        assert fn(CODE, 2, *holed, 10, 0) == EINVAL and "NULL argument array" in la.last_error()
    # part 0 has no frames, so its NULL buffers are fine; part 1 names a device that does not exist
    st = fn(CODE, 2, *args, 10, 0)
    if GPU:
        assert st == EINVAL and "devices[1] = 4096 out of range" in la.last_error()
        ptrs[2][1] = None                                                    # ... and a part WITH frames may not have a NULL buffer
        devs[1] = 0
        assert fn(CODE, 2, *args, 10, 0) == EINVAL and "part 1: NULL buffer" in la.last_error()
    else:
        assert st == ENODEV and "no HIP device" in la.last_error()
