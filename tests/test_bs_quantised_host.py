"""f32 LLRs through the bit-sliced i8 kernels' own loader, what can be said without a GPU: the shared frames exercise
what they must, the three new symbols exist in the header, the library, the Python table and the Rust shim, the Python keywords choose
them and refuse what they must, and every refusal of the C entries comes in its order before any device work."""
import ctypes
import os
import re

import numpy as np
import pytest

import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode, HipOpts, MEM_HOST, MEM_DEVICE

import bs_quantised_frames as bqf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, ENODEV, EUNSUPPORTED = 0, -1, -2, -4
GPU = la.device_count() > 0
PLAIN = "labrador_ldpc_decode_ms_bitsliced_quantised_batch_i8"
CORRECTED = "labrador_ldpc_decode_ms_bitsliced_quantised_corrected_batch_i8"
CASCADE = "labrador_ldpc_decode_ms_cascade_bitsliced_quantised_batch_i8"


@pytest.mark.parametrize("name", bqf.NAMES)
def test_the_shared_frames_meet_their_conditions(name):
    x = bqf.frames(name)
    assert x.dtype == np.float32 and x.shape == (3 * bqf.GROUP[name] + 1, LDPCCode[name].n())
    assert np.isnan(x).all(axis=1).sum() == 1 and np.isposinf(x).all(axis=1).sum() == 1          # the two flat rows
    bqf.assert_conditions(name)


def test_the_launcher_picks_the_form_from_the_scale():
    assert [bqf.mulbits(t) for t in bqf.TRIPLES] == [4, 0, 8] and bqf.mulbits(bqf.IDENTITY) == 0


# ---- the symbols ----------------------------------------------------------------------------------------------------------------------
def test_the_new_symbols_are_declared_exported_bound_and_mirrored():
    header = open(os.path.join(ROOT, "include", "labrador_ldpc_hip.h")).read()
    shim = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for sym, nargs, like in ((PLAIN, 10, "labrador_ldpc_decode_ms_quantised_batch_i8"), (CORRECTED, 13, None),
                             (CASCADE, 18, "labrador_ldpc_decode_ms_cascade_quantised_corrected_batch_i8")):
        m = re.search(r"\bint %s\(([^;]*?)\);" % sym, header)
        assert m and len(m.group(1).split(",")) == nargs, sym
        assert sym in la.SYMBOLS and len(la.SYMBOLS[sym][1]) == nargs
        assert getattr(la.lib, sym) is not None
        assert re.search(r"pub fn %s\(" % sym, shim), sym
        if like:                                                                     # the argument list of the entry it stands beside
            assert [a.__name__ for a in la.SYMBOLS[sym][1]] == [a.__name__ for a in la.SYMBOLS[like][1]]
            theirs = re.search(r"\bint %s\s*\(([^;]*?)\);" % like, header).group(1)
            assert re.sub(r"\s+", " ", m.group(1)) == re.sub(r"\s+", " ", theirs)
    assert re.search(r"LABRADOR_LDPC_HIP_ABI\s+3\b", header)


# ---- the Python keywords ------------------------------------------------------------------------------------------------------------
class _SpyLib:
    """Stands where the package keeps its library: a quantised decode looked up through it is recorded with its arguments and reports
    success without doing anything; every other symbol is the library's own."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        if "quantised" not in name:
            return getattr(self.real, name)

        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


def test_python_keywords_choose_the_entry_point_and_pass_the_arguments(monkeypatch):
    code = LDPCCode.TM1536
    spy = _SpyLib(la.lib)
    monkeypatch.setattr(la, "lib", spy)
    llrs = np.ones((3, code.n()), np.float32)
    # flooding: without bitsliced the call is the one it was
    code.decode_ms_quantised_batch(llrs, "i8", 8.0, 31, 25)
    (name, args), = spy.calls
    assert name == "labrador_ldpc_decode_ms_quantised_batch_i8" and args[5:9] == (3, 25, 8.0, 31)
    for kw, sym, tail in (({}, PLAIN, ()), (dict(scale_num=13, scale_shift=4), CORRECTED, (13, 4, 0)), (dict(offset=1), CORRECTED, (1, 0, 1)),
                          (dict(scale_shift=4), CORRECTED, (16, 4, 0))):
        del spy.calls[:]
        code.decode_ms_quantised_batch(llrs, "i8", 4.0, 31, 25, bitsliced=True, **kw)
        (name, args), = spy.calls
        assert name == sym and len(args) == 1 + 4 + 4 + len(tail) + 1 and args[5:9 + len(tail)] == (3, 25, 4.0, 31) + tail, (name, kw)
        assert args[0] == int(code) and args[1] == llrs.ctypes.data
    del spy.calls[:]
    code.decode_ms_quantised_batch(llrs, maxiters=7, bitsliced=True)                  # lim defaults to the type's largest value
    assert spy.calls[0][1][5:9] == (3, 7, 8.0, 127)
    # the cascade
    for kw, t1 in (({}, (1, 0, 0)), (dict(flooding_scale_num=13, flooding_scale_shift=4), (13, 4, 0))):
        for stage2, t2 in (({}, (1, 0, 0)), (dict(scale_num=3, scale_shift=2, offset=1), (3, 2, 1))):
            del spy.calls[:]
            code.decode_ms_cascade_quantised_batch(llrs, "i8", 8.0, 31, 25, 7, bitsliced=True, **kw, **stage2)
            (name, args), = spy.calls
            assert name == CASCADE and len(args) == 18 and args[6:17] == (3, 25, 7, 8.0, 31) + t1 + t2, (name, kw, stage2)
    del spy.calls[:]
    code.decode_ms_cascade_quantised_batch(llrs, "i8", 8.0, 31, 25, 7)                # not bit-sliced: unchanged
    assert spy.calls[0][0] == "labrador_ldpc_decode_ms_cascade_quantised_batch_i8"
    # the refusals: the triple without bitsliced; i16 and a variant with it
    del spy.calls[:]
    for kw in (dict(scale_num=13, scale_shift=4), dict(offset=1), dict(scale_shift=0)):
        with pytest.raises(ValueError, match="bitsliced=True"):
            code.decode_ms_quantised_batch(llrs, **kw)
    with pytest.raises(ValueError, match="i8 only"):
        code.decode_ms_quantised_batch(llrs, "i16", bitsliced=True)
    with pytest.raises(ValueError, match="variant 0 only"):
        code.decode_ms_quantised_batch(llrs, bitsliced=True, variant=64)
    with pytest.raises(ValueError, match="i8 only"):
        code.decode_ms_cascade_quantised_batch(llrs, "i16", bitsliced=True)
    with pytest.raises(ValueError, match="variant 0 only"):
        code.decode_ms_cascade_quantised_batch(llrs, bitsliced=True, variant=64)
    with pytest.raises(KeyError):
        code.decode_ms_quantised_batch(llrs, "i32", bitsliced=True)
    with pytest.raises(ValueError, match="float32"):
        code.decode_ms_quantised_batch(np.ones((1, code.n()), np.int8), bitsliced=True)
    with pytest.raises(ValueError):
        code.decode_ms_quantised_batch(llrs, bitsliced=True, scale_num=-1)
    assert not spy.calls                                                             # ... before the library sees anything
    monkeypatch.undo()
    with pytest.raises(la.LdpcHipError, match="scale_shift 40"):
        code.decode_ms_quantised_batch(llrs, bitsliced=True, scale_shift=40)
    with pytest.raises(la.LdpcHipError, match="only variant 0 on TM1536, TM2048, TM6144 and TM8192"):
        LDPCCode.TM1280.decode_ms_quantised_batch(np.ones((1, 1280), np.float32), bitsliced=True)


# ---- the refusals, in their order, before any device work -----------------------------------------------------------------------------
TM1536, TM1280, TM5120, TC128 = int(LDPCCode.TM1536), int(LDPCCode.TM1280), int(LDPCCode.TM5120), int(LDPCCode.TC128)
STRIDE = 1 << 16
_ARENA = np.full(8 * STRIDE, 0x5A, dtype=np.uint8)
BUF = (_ARENA.ctypes.data + 15) // 16 * 16
VARIANT7 = HipOpts(-1, MEM_HOST, None, 7, 0, None)
ONLY = "not built for the f32-reading bit-sliced flooding decoder on code %d (only variant 0 on TM1536, TM2048, TM6144 and TM8192 is)"
BAD_TRIPLES = (((1, 9, 0), "scale_shift 9 is not in 0 .. 8"), ((5, 2, 0), "scale_num 5 is not in 1 .. 1 << scale_shift (4)"),
               ((0, 0, 0), "scale_num 0 is not in"), ((3, 2, 128), "offset 128 is not in 0 .. 127"))
BAD_QUANTISERS = (((0.0, 31), "scale 0 is not in (0, FLT_MAX]"), ((float("nan"), 31), "is not in (0, FLT_MAX]"),
                  ((float("inf"), 31), "is not in (0, FLT_MAX]"), ((-1.0, 31), "scale -1 is not in"), ((8.0, 128), "lim 128 is not in 0 .. 127"),
                  ((8.0, -1), "lim -1 is not in 0 .. 127"))


def refused_device_set(variant):
    """opts that are refused once the argument checks are over and before any device is asked for: a device list with a stream"""
    return HipOpts(-1, MEM_HOST, 0x1234, variant, 2, (ctypes.c_int * 2)(0, 0))


def call(sym, code, bufs, batch, tail, opts=None):
    st = getattr(la.lib, sym)(code, *bufs, batch, *tail, ctypes.byref(opts) if opts is not None else None)
    return st, la.last_error()


def refused(got, status, text):
    assert got[0] == status and text in got[1], got


@pytest.mark.parametrize("sym,nbuf,caps,ntriples", [(PLAIN, 4, (10,), 0), (CORRECTED, 4, (10,), 1), (CASCADE, 5, (10, 10), 2)])
def test_refusals_come_in_their_order_before_any_device_work(sym, nbuf, caps, ntriples):
    good = [BUF + STRIDE * i for i in range(nbuf)]
    nulls = [None] * nbuf
    ok3, bad = (13, 4, 0), (1, 9, 0)

    def tail(t1=ok3, t2=(3, 2, 0), q=(8.0, 31)):
        return caps + q + ((t1, t1 + t2)[ntriples - 1] if ntriples else ())
    # 1. the code, before everything
    refused(call(sym, 9, nulls, 0, tail(bad, q=(0.0, 31))), EINVAL, "out of range")
    refused(call(sym, -1, nulls, 2, tail(bad, q=(0.0, 31)), VARIANT7), EINVAL, "out of range")
    # 2. the quantiser's pair, even for an empty batch, whatever else is wrong
    for q, text in BAD_QUANTISERS:
        refused(call(sym, TM1280, nulls, 0, tail(bad, q=q), VARIANT7), EINVAL, text)
        refused(call(sym, TC128, nulls, 2, tail(bad, q=q), VARIANT7), EINVAL, text)
    # 3. the empty batch is OK and touches nothing, whatever else is wrong
    assert call(sym, TM1280, nulls, 0, tail(bad), VARIANT7) == (OK, "")
    assert call(sym, TC128, nulls, 0, tail(), HipOpts(-1, MEM_DEVICE, None, 0, 0, None)) == (OK, "")
    # 4. NULL buffers (the cascade: stage included), before the variant, the code family and the triples
    for i in range(nbuf):
        bufs = list(good)
        bufs[i] = None
        refused(call(sym, TM1280, bufs, 2, tail(bad), VARIANT7), EINVAL, "NULL buffer")
    # 5. the variant and the code family, with a text of their own -- before the triples, at any triple
    for t1 in (ok3, (1, 0, 0), bad):
        refused(call(sym, TM1536, good, 2, tail(t1), VARIANT7), EUNSUPPORTED, "variant 7 " + ONLY % TM1536)
        refused(call(sym, TM1536, good, 2, tail(t1), HipOpts(-1, MEM_HOST, None, 64, 0, None)), EUNSUPPORTED, "variant 64 " + ONLY % TM1536)
        for code in (TM1280, TM5120, TC128, int(LDPCCode.TC512)):
            refused(call(sym, code, good, 2, tail(t1)), EUNSUPPORTED, "variant 0 " + ONLY % code)
            refused(call(sym, code, good, 2, tail(t1), refused_device_set(0)), EUNSUPPORTED, "f32-reading bit-sliced")
    # 6. the triples (the cascade: stage 1's first, then stage 2's)
    if ntriples:
        for triple, text in BAD_TRIPLES:
            refused(call(sym, TM1536, good, 2, tail(triple)), EINVAL, text)
            refused(call(sym, TM1536, good, 2, tail(triple), refused_device_set(0)), EINVAL, text)
            if ntriples == 2:
                refused(call(sym, TM1536, good, 2, tail(ok3, triple)), EINVAL, text)
                refused(call(sym, TM1536, good, 2, tail((1, 0, 0), triple)), EINVAL, text)
        if ntriples == 2:
            refused(call(sym, TM1536, good, 2, tail((3, 9, 0), (3, 10, 0))), EINVAL, "scale_shift 9 is not in")
            refused(call(sym, TM1536, good, 2, tail((4, 2, 0), (3, 10, 0))), EINVAL, "scale_shift 10 is not in")
    # ... and what passes the argument checks goes on to the device set
    for code in (TM1536, int(LDPCCode.TM2048), int(LDPCCode.TM6144), int(LDPCCode.TM8192)):
        for t1 in (ok3, (1, 0, 0)):
            refused(call(sym, code, good, 2, tail(t1), refused_device_set(0)), EINVAL, "must be NULL")
    if not GPU:
        refused(call(sym, TM1536, good, 2, tail(), HipOpts(-1, MEM_HOST, None, 0, 0, None)), ENODEV, "no HIP device")
    # 7. with MEM_DEVICE the alignments, once a device is selected: output 8-byte, llrs 16-byte
    dev = HipOpts(-1, MEM_DEVICE, None, 0, 0, None)
    for at, off, text in ((1, 4, "device output buffer must be 8-byte aligned"), (0, 4, "device llrs buffer must be 16-byte aligned"),
                          (0, 8, "device llrs buffer must be 16-byte aligned")):
        bufs = list(good)
        bufs[at] += off
        got = call(sym, TM1536, bufs, 2, tail(), dev)
        refused(got, EINVAL, text) if GPU else refused(got, ENODEV, "no HIP device")
    assert (_ARENA == 0x5A).all()                                                   # nothing was written anywhere
