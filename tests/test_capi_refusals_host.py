"""What the C ABI's batched entry points refuse, and in which order: raw calls -> (status, a piece of last_error()).

Every family goes through the same host call path (csrc/capi.hip); this table pins what that path answers before it touches a
device, so that it can be rewritten without the answers moving.  Where the outcome depends on a device being present the
expectation branches on device_count(), as test_capi_host.py does.  TC128, batch 2 (TM1536 and TM1280 where a bit-sliced entry
looks at the code); nothing here needs a GPU."""
import ctypes

import numpy as np
import pytest

import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode, HipOpts, MEM_HOST, MEM_DEVICE

OK, EINVAL, ENODEV, EUNSUPPORTED = 0, -1, -2, -4
CODE, BAD_CODE, BATCH = int(LDPCCode.TC128), 9, 2
GPU = la.device_count() > 0

# one buffer every pointer argument may point into, 16-byte aligned: argument i of a call lies STRIDE * i behind BUF, which keeps the
# arguments of a batch-2 call apart on every code used here (the longest, TM1536 marginals in int32, are under 16 KiB)
STRIDE = 1 << 16
_ARENA = np.zeros(8 * STRIDE, dtype=np.uint8)
BUF = (_ARENA.ctypes.data + 15) // 16 * 16
TM1536, TM1280 = int(LDPCCode.TM1536), int(LDPCCode.TM1280)

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
# The rest of the min-sum families and the two converters.  Their tails are made of the caps (max_iters; the cascade's max_sweeps
# too) and of parameter groups: P = a float pair (scale, offset), Q = the quantiser's (scale, lim), T = an integer triple
# (scale_num, scale_shift, offset).  name -> (pointer arguments, caps, groups in the order of the arguments)
PAIR, QUANT, TRIPLE = (0.75, 0.0), (8.0, 31), (3, 2, 0)
GROUPS = {
    "corrected_batch_f32": (4, 1, "P"), "corrected_soft_batch_f32": (5, 1, "P"),
    "corrected_batch_i8": (4, 1, "T"), "bitsliced_soft_batch_i8": (5, 1, ""),
    "layered_fixed_corrected_batch_i8": (4, 1, "T"), "layered_fixed_corrected_batch_i16": (4, 1, "T"),
    "layered_fixed_corrected_soft_batch_i8": (5, 1, "T"), "layered_fixed_corrected_soft_batch_i16": (5, 1, "T"),
    "cascade_batch_f32": (5, 2, "P"), "cascade_batch_i8": (5, 2, "T"), "cascade_batch_i16": (5, 2, "T"),
    "cascade_corrected_batch_f32": (5, 2, "PP"), "cascade_corrected_batch_i8": (5, 2, "TT"),
    "cascade_soft_batch_f32": (6, 2, "PP"), "cascade_soft_batch_i8": (6, 2, "T"), "cascade_soft_batch_i16": (6, 2, "T"),
    "cascade_bitsliced_soft_batch_i8": (6, 2, "T"),
    "quantised_batch_i8": (4, 1, "Q"), "quantised_batch_i16": (4, 1, "Q"),
    "layered_quantised_batch_i8": (4, 1, "QT"), "layered_quantised_batch_i16": (4, 1, "QT"),
    "layered_quantised_soft_batch_i8": (5, 1, "QT"), "layered_quantised_soft_batch_i16": (5, 1, "QT"),
    "cascade_quantised_batch_i8": (5, 2, "QT"), "cascade_quantised_batch_i16": (5, 2, "QT"),
    "cascade_quantised_corrected_batch_i8": (5, 2, "QTT"),
    "batch_f16": (4, 1, ""), "batch_bf16": (4, 1, ""), "soft_batch_f16": (5, 1, ""), "soft_batch_bf16": (5, 1, ""),
    "layered_batch_f16": (4, 1, ""), "layered_batch_bf16": (4, 1, ""), "layered_soft_batch_f16": (5, 1, ""), "layered_soft_batch_bf16": (5, 1, ""),
    "layered_corrected_batch_f16": (4, 1, "P"), "layered_corrected_batch_bf16": (4, 1, "P"),
    "layered_corrected_soft_batch_f16": (5, 1, "P"), "layered_corrected_soft_batch_bf16": (5, 1, "P"),
    "cascade_batch_f16": (5, 2, "P"), "cascade_batch_bf16": (5, 2, "P"),
}
CONVERTERS = {"quantise_llrs_batch_i8": "Q", "quantise_llrs_batch_i16": "Q", "widen_llrs_batch_f16": "", "widen_llrs_batch_bf16": ""}


def tail_of(family, **groups):
    """The arguments between batch and opts: the caps, then every parameter group of the family -- P0=(1.5, 0.0) replaces its first
    pair, T1=... its second triple, Q0=... its quantiser."""
    ncaps, kinds = (0, CONVERTERS[family]) if family in CONVERTERS else GROUPS[family][1:]
    tail, seen = [10] * ncaps, {}
    for kind in kinds:
        i = seen[kind] = seen.get(kind, -1) + 1
        tail += groups.pop(f"{kind}{i}", {"P": PAIR, "Q": QUANT, "T": TRIPLE}[kind])
    assert not groups, groups
    return tuple(tail)


FAMILIES.update({name: ("labrador_ldpc_decode_ms_" + name, nbuf, tail_of(name)) for name, (nbuf, _, _) in GROUPS.items()})
FAMILIES.update({name: ("labrador_ldpc_" + name, 2, tail_of(name)) for name in CONVERTERS})
ALL = sorted(FAMILIES)
WITH = {kind: sorted(f for f, g in {**{n: g[2] for n, g in GROUPS.items()}, **CONVERTERS}.items() if kind in g) for kind in "PQT"}
SKELETONS = ["bf", "encode", "ms_batch_f32"]        # the three bodies that select a device set


def call(family, code=CODE, bufs=None, batch=BATCH, tail=None, opts=None):
    """-> (status, last_error()).  bufs: None = every pointer valid, else one address (or None) per pointer argument."""
    sym, nbuf, default_tail = FAMILIES[family]
    bufs = [BUF + STRIDE * i for i in range(nbuf)] if bufs is None else bufs
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


# ---- parameter groups: which of two faults a call reports ---------------------------------------------------------------------------
BAD_EARLY = {"P0": (1.5, 0.0), "Q0": (0.0, 31)}                             # a pair's scale above 1, a quantiser's scale of 0
BAD_TRIPLE = (3, 9, 0)                                                      # scale_shift 9
VARIANT7 = HipOpts(-1, MEM_HOST, None, 7, 0, None)


def refused_device_set(variant):
    """opts that are refused once the argument checks are over and before any device is asked for: a device list with a stream"""
    return HipOpts(-1, MEM_HOST, 0x1234, variant, 2, (ctypes.c_int * 2)(0, 0))


def passes_the_argument_checks(family, variant, **kw):
    refused(call(family, opts=refused_device_set(variant), **kw), EINVAL, "must be NULL")
    if not GPU:
        refused(call(family, opts=HipOpts(-1, MEM_HOST, None, variant, 0, None), **kw), ENODEV, "no HIP device")


def bad_early(family):
    kinds = CONVERTERS[family] if family in CONVERTERS else GROUPS[family][2]
    return {k: v for k, v in BAD_EARLY.items() if k[0] in kinds}


@pytest.mark.parametrize("family", sorted(set(WITH["P"] + WITH["Q"] + WITH["T"])))
def test_bad_code_comes_before_bad_parameters(family):
    kinds = CONVERTERS[family] if family in CONVERTERS else GROUPS[family][2]
    tail = tail_of(family, **bad_early(family), **({"T0": BAD_TRIPLE} if "T" in kinds else {}))
    refused(call(family, code=BAD_CODE, tail=tail), EINVAL, "out of range")
    refused(call(family, code=BAD_CODE, tail=tail, bufs=nulls(family), batch=0), EINVAL, "out of range")


@pytest.mark.parametrize("family", sorted(set(WITH["P"] + WITH["Q"])))
def test_float_pairs_and_the_quantiser_are_checked_even_for_an_empty_batch_with_null_buffers(family):
    for key, value in bad_early(family).items():
        text = "scale 1.5 is not in (0, 1]" if key[0] == "P" else "scale 0 is not in (0, FLT_MAX]"
        refused(call(family, tail=tail_of(family, **{key: value}), bufs=nulls(family), batch=0), EINVAL, text)
        refused(call(family, tail=tail_of(family, **{key: value}), bufs=nulls(family)), EINVAL, text)
    if family in WITH["P"]:
        refused(call(family, tail=tail_of(family, P0=(1.0, -1.0)), bufs=nulls(family), batch=0), EINVAL, "offset -1 is not in [0, FLT_MAX]")
    if family in WITH["Q"]:
        refused(call(family, tail=tail_of(family, Q0=(8.0, 40000)), bufs=nulls(family), batch=0), EINVAL, "lim 40000 is not in 0 .. ")
        refused(call(family, tail=tail_of(family, Q0=(8.0, -1)), bufs=nulls(family), batch=0), EINVAL, "lim -1 is not in 0 .. ")


@pytest.mark.parametrize("family", WITH["T"])
def test_integer_triples_are_checked_after_the_buffers_and_before_the_variant(family):
    nbuf = FAMILIES[family][1]
    for key, value, text in (("T0", BAD_TRIPLE, "scale_shift 9 is not in 0 .. 8"), ("T0", (5, 2, 0), "scale_num 5 is not in 1 .. 1 << scale_shift (4)"),
                             ("T0", (0, 0, 0), "scale_num 0 is not in"), ("T0", (3, 2, 40000), "offset 40000 is not in 0 .. "),
                             ("T1", BAD_TRIPLE, "scale_shift 9 is not in 0 .. 8")):
        if key == "T1" and GROUPS[family][2].count("T") < 2:
            continue
        tail = tail_of(family, **{key: value})
        assert call(family, tail=tail, batch=0) == (OK, "")
        assert call(family, tail=tail, batch=0, bufs=nulls(family)) == (OK, "")
        bufs = [BUF + STRIDE * i for i in range(nbuf)]
        bufs[-1] = None
        refused(call(family, tail=tail, bufs=bufs), EINVAL, "NULL buffer")
        refused(call(family, tail=tail), EINVAL, text)
        refused(call(family, tail=tail, opts=VARIANT7), EINVAL, text)                    # ... not EUNSUPPORTED
        refused(call(family, tail=tail, opts=refused_device_set(7)), EINVAL, text)
    i8 = family.endswith("i8")
    refused(call(family, tail=tail_of(family, T0=(3, 2, 128 if i8 else 32768))), EINVAL, "offset %d is not in 0 .. %d" % ((128, 127) if i8 else (32768, 32767)))


@pytest.mark.parametrize("family", ["cascade_corrected_batch_f32", "cascade_soft_batch_f32"])
def test_the_cascade_checks_the_flooding_pair_before_the_stage_2_pair(family):
    refused(call(family, tail=tail_of(family, P0=(1.5, 0.0), P1=(2.5, 0.0)), bufs=nulls(family), batch=0), EINVAL, "scale 1.5 is not in")
    refused(call(family, tail=tail_of(family, P0=(1.0, 0.0), P1=(2.5, 0.0)), bufs=nulls(family), batch=0), EINVAL, "scale 2.5 is not in")


@pytest.mark.parametrize("family", ["cascade_corrected_batch_i8", "cascade_quantised_corrected_batch_i8"])
def test_the_cascade_checks_the_flooding_triple_before_the_stage_2_triple(family):
    refused(call(family, tail=tail_of(family, T0=(3, 9, 0), T1=(3, 10, 0))), EINVAL, "scale_shift 9 is not in")
    refused(call(family, tail=tail_of(family, T0=(4, 2, 0), T1=(3, 10, 0))), EINVAL, "scale_shift 10 is not in")


@pytest.mark.parametrize("family", ["layered_quantised_batch_i8", "layered_quantised_batch_i16", "layered_quantised_soft_batch_i8",
                                    "layered_quantised_soft_batch_i16"])
def test_layered_quantised_order(family):
    """the quantiser before the empty batch, the triple after the buffers, the variant after the triple and before the device set"""
    nbuf = FAMILIES[family][1]
    refused(call(family, tail=tail_of(family, Q0=(0.0, 31), T0=BAD_TRIPLE), batch=0, bufs=nulls(family)), EINVAL, "scale 0 is not in (0, FLT_MAX]")
    refused(call(family, tail=tail_of(family, Q0=(0.0, 31), T0=BAD_TRIPLE), opts=VARIANT7), EINVAL, "scale 0 is not in (0, FLT_MAX]")
    refused(call(family, tail=tail_of(family, T0=BAD_TRIPLE), bufs=[None] + [BUF + STRIDE * i for i in range(1, nbuf)], opts=VARIANT7),
            EINVAL, "NULL buffer")
    refused(call(family, tail=tail_of(family, T0=BAD_TRIPLE), opts=VARIANT7), EINVAL, "scale_shift 9")
    assert call(family, batch=0, opts=VARIANT7) == (OK, "")
    refused(call(family, opts=VARIANT7), EUNSUPPORTED, "variant 7 not built for the layered schedule (only 0 is)")
    refused(call(family, opts=refused_device_set(7)), EUNSUPPORTED, "only 0 is")
    refused(call(family, opts=HipOpts(-3, 2, None, 7, -1, None)), EUNSUPPORTED, "only 0 is")
    passes_the_argument_checks(family, 0)


@pytest.mark.parametrize("family", ["layered_fixed_corrected_batch_i8", "layered_fixed_corrected_soft_batch_i16", "layered_batch_f16",
                                    "layered_soft_batch_bf16", "layered_corrected_batch_bf16", "layered_corrected_soft_batch_f16",
                                    "corrected_batch_f32", "corrected_soft_batch_f32"])
def test_variant_zero_only_is_said_with_the_arguments(family):
    text = "corrected flooding decoder (only 0 is; code 0)" if family.startswith("corrected") else "layered schedule (only 0 is)"
    assert call(family, batch=0, opts=VARIANT7) == (OK, "")
    refused(call(family, bufs=nulls(family), opts=VARIANT7), EINVAL, "NULL buffer")
    refused(call(family, opts=VARIANT7), EUNSUPPORTED, "variant 7 not built for the " + text)
    refused(call(family, opts=refused_device_set(7)), EUNSUPPORTED, "variant 7 not built for the " + text)
    passes_the_argument_checks(family, 0)


@pytest.mark.parametrize("family", ["ms_batch_f32", "layered_batch_f32", "layered_corrected_batch_f32", "batch_f16", "soft_batch_bf16",
                                    "quantised_batch_i8", "cascade_batch_i16", "cascade_quantised_batch_i8", "cascade_batch_bf16"])
def test_the_older_entries_leave_the_variant_to_their_launchers(family):
    passes_the_argument_checks(family, 7)


@pytest.mark.parametrize("family", ["cascade_corrected_batch_f32", "cascade_soft_batch_f32"])
def test_f32_cascade_variant_with_and_without_a_flooding_pair(family):
    corrected = tail_of(family, P0=(0.75, 0.0))
    refused(call(family, tail=corrected, opts=VARIANT7), EUNSUPPORTED, "variant 7 not built for the corrected flooding decoder (only 0 is; code 0)")
    refused(call(family, tail=corrected, opts=refused_device_set(7)), EUNSUPPORTED, "corrected flooding decoder")
    refused(call(family, tail=corrected, bufs=nulls(family), opts=VARIANT7), EINVAL, "NULL buffer")
    passes_the_argument_checks(family, 0, tail=corrected)
    passes_the_argument_checks(family, 7, tail=tail_of(family, P0=(1.0, 0.0)))           # the identity: the flooding launcher's own variants
    passes_the_argument_checks("cascade_batch_f32", 7)


def test_corrected_batch_i8_has_variant_0_on_the_tm_codes_only():
    text = "not built for the corrected bit-sliced flooding decoder on code %d (only variant 0 on the TM codes is)"
    refused(call("corrected_batch_i8", code=TM1536, opts=VARIANT7), EUNSUPPORTED, "variant 7 " + text % TM1536)
    refused(call("corrected_batch_i8", code=CODE), EUNSUPPORTED, "variant 0 " + text % CODE)
    refused(call("corrected_batch_i8", code=CODE, opts=refused_device_set(0)), EUNSUPPORTED, "corrected bit-sliced")
    refused(call("corrected_batch_i8", code=CODE, tail=tail_of("corrected_batch_i8", T0=(4, 2, 0))), EUNSUPPORTED, "corrected bit-sliced")
    passes_the_argument_checks("corrected_batch_i8", 0, code=TM1536)
    passes_the_argument_checks("corrected_batch_i8", 0, code=TM1280)


@pytest.mark.parametrize("family", ["cascade_corrected_batch_i8", "cascade_quantised_corrected_batch_i8"])
def test_cascade_stage_1_triple_has_variant_0_on_the_tm_codes_only(family):
    refused(call(family, code=CODE), EUNSUPPORTED, "variant 0 not built for the corrected bit-sliced flooding decoder on code 0")
    refused(call(family, code=TM1536, opts=VARIANT7), EUNSUPPORTED, "variant 7 not built for the corrected bit-sliced")
    refused(call(family, code=CODE, opts=refused_device_set(0)), EUNSUPPORTED, "corrected bit-sliced")
    passes_the_argument_checks(family, 0, code=TM1536)
    # an identity triple, however it is written, is today's flooding launcher: any code, the launcher's own variants
    passes_the_argument_checks(family, 7, code=CODE, tail=tail_of(family, T0=(4, 2, 0)))
    passes_the_argument_checks(family, 7, code=CODE, tail=tail_of(family, T0=(1, 0, 0)))


@pytest.mark.parametrize("family", ["bitsliced_soft_batch_i8", "cascade_bitsliced_soft_batch_i8"])
def test_bitsliced_soft_has_variant_0_on_the_one_wave_tm_codes_only(family):
    only = "not built for the soft bit-sliced flooding decoder on code %d (only variant 0 on TM1536, TM2048, TM6144 and TM8192 is)"
    refused(call(family, code=TM1280, opts=VARIANT7), EUNSUPPORTED, "variant 7 " + only % TM1280)         # the variant, not the two waves
    refused(call(family, code=TM1280), EUNSUPPORTED, "code %d decodes on the two-wave bit-sliced kernels" % TM1280)
    refused(call(family, code=CODE), EUNSUPPORTED, "variant 0 " + only % CODE)
    refused(call(family, code=CODE, opts=refused_device_set(0)), EUNSUPPORTED, "soft bit-sliced")
    refused(call(family, code=TM1280, bufs=nulls(family)), EINVAL, "NULL buffer")
    assert call(family, code=TM1280, batch=0, opts=VARIANT7) == (OK, "")
    passes_the_argument_checks(family, 0, code=TM1536)


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


@pytest.mark.parametrize("family,other", [("quantise_llrs_batch_i8", "q"), ("quantise_llrs_batch_i16", "q"), ("widen_llrs_batch_f16", "out"),
                                          ("widen_llrs_batch_bf16", "out")])
def test_quantise_and_widen_check_memory_and_both_alignments_before_device_selection(family, other):
    refused(call(family, opts=HipOpts(4096, 2, None, 0, 0, None)), EINVAL, "bad opts->memory")
    refused(call(family, bufs=[BUF + 4, BUF + STRIDE + 4], opts=HipOpts(4096, 2, None, 0, 0, None)), EINVAL, "bad opts->memory")
    dev = HipOpts(4096, MEM_DEVICE, None, 0, 0, None)
    refused(call(family, bufs=[BUF + 4, BUF + STRIDE + 4], opts=dev), EINVAL, "device llrs buffer must be 16-byte aligned")
    refused(call(family, bufs=[BUF, BUF + STRIDE + 4], opts=dev), EINVAL, f"device {other} buffer must be 16-byte aligned")
    refused(call(family, bufs=[None, BUF + STRIDE + 4], opts=dev), EINVAL, "NULL buffer")
    assert call(family, bufs=[BUF + 4, BUF + STRIDE + 4], batch=0, opts=dev) == (OK, "")
    got = call(family, opts=dev)
    refused(got, EINVAL, "device 4096 out of range") if GPU else refused(got, ENODEV, "no HIP device")
    # host buffers are converted where they lie, whatever their alignment and whatever the rest of opts says
    assert call(family, bufs=[BUF + 4, BUF + STRIDE + 4], opts=HipOpts(4096, MEM_HOST, 0x1234, 7, 0, None)) == (OK, "")
    assert call(family, bufs=[BUF + 4, BUF + STRIDE + 4]) == (OK, "")


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
