"""Packed hard decisions through the bit-sliced i8 kernels' own loader, what can be said without a GPU: the two new
symbols exist in the header, the library, the Python table and the Rust shim, the Python keywords choose them and pass the mask and
the magnitude, and every refusal of the C entries comes in its order before any device work."""
import ctypes
import os
import re

import numpy as np
import pytest

import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode, HipOpts, MEM_HOST, MEM_DEVICE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, ENODEV, EUNSUPPORTED = 0, -1, -2, -4
GPU = la.device_count() > 0
PLAIN = "labrador_ldpc_decode_ms_bitsliced_hard_batch_i8"
CORRECTED = "labrador_ldpc_decode_ms_bitsliced_hard_corrected_batch_i8"


# ---- the symbols ----------------------------------------------------------------------------------------------------------------------
def test_the_new_symbols_are_declared_exported_bound_and_mirrored():
    header = open(os.path.join(ROOT, "include", "labrador_ldpc_hip.h")).read()
    shim = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for sym, nargs in ((PLAIN, 10), (CORRECTED, 13)):
        m = re.search(r"\bint %s\(([^;]*?)\);" % sym, header)
        assert m and len(m.group(1).split(",")) == nargs, sym
        args = re.sub(r"\s+", " ", m.group(1))
        assert args.startswith("enum labrador_ldpc_code code, const uint8_t *input, const uint8_t *erasures, uint8_t *output, uint32_t *iters, "
                               "uint8_t *success, size_t batch, size_t max_iters, int magnitude, ")
        assert args.endswith("const struct labrador_ldpc_hip_opts *opts")
        assert sym in la.SYMBOLS and len(la.SYMBOLS[sym][1]) == nargs
        assert getattr(la.lib, sym) is not None
        r = re.search(r"pub fn %s\(([^;]*?)\) -> c_int;" % sym, shim)
        assert r and len(r.group(1).split(",")) == nargs, sym
        assert "erasures: *const u8" in r.group(1) and "magnitude: c_int" in r.group(1)
    assert "uint32_t scale_num, uint32_t scale_shift, uint32_t offset" in re.sub(r"\s+", " ", re.search(r"\bint %s\(([^;]*?)\);" % CORRECTED, header).group(1))
    assert re.search(r"LABRADOR_LDPC_HIP_ABI\s+3\b", header)
    assert la.lib.labrador_ldpc_hip_abi_version() == 3


# ---- the Python keywords ------------------------------------------------------------------------------------------------------------
class _SpyLib:
    """Stands where the package keeps its library: a packed hard-decision decode looked up through it is recorded with its arguments
    and reports success without doing anything; every other symbol is the library's own."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        if "bitsliced_hard" not in name:
            return getattr(self.real, name)

        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


def test_python_keywords_choose_the_entry_point_and_pass_the_arguments(monkeypatch):
    code = LDPCCode.TM1536
    spy = _SpyLib(la.lib)
    monkeypatch.setattr(la, "lib", spy)
    x = np.zeros((3, code.n() // 8), np.uint8)
    mask = np.ones((3, code.n() // 8), np.uint8)
    # the defaults: cap 50, magnitude 1, no mask -> NULL, the plain entry
    out, it, ok = code.decode_ms_hard_batch(x)
    (name, args), = spy.calls
    assert name == PLAIN and len(args) == 10
    assert args[:3] == (int(code), x.ctypes.data, None) and args[3:6] == (out.ctypes.data, it.ctypes.data, ok.ctypes.data) and args[6:9] == (3, 50, 1)
    assert out.shape == (3, code.output_len()) and it.shape == ok.shape == (3,)
    # the mask's pointer, the magnitude, the triple -> the corrected entry through _fixed_correction
    for kw, sym, tail in (({}, PLAIN, ()), (dict(scale_num=13, scale_shift=4), CORRECTED, (13, 4, 0)), (dict(offset=1), CORRECTED, (1, 0, 1)),
                          (dict(scale_shift=4), CORRECTED, (16, 4, 0))):
        for erasures, ptr in ((None, None), (mask, mask.ctypes.data)):
            del spy.calls[:]
            code.decode_ms_hard_batch(x, 25, 16, erasures, **kw)
            (name, args), = spy.calls
            assert name == sym and len(args) == 10 + len(tail), (name, kw)
            assert args[1:3] == (x.ctypes.data, ptr) and args[6:9 + len(tail)] == (3, 25, 16) + tail, (name, kw)
    # the caller's result buffers are the ones passed
    del spy.calls[:]
    o, i, s = np.zeros((3, code.output_len()), np.uint8), np.zeros(3, np.uint32), np.zeros(3, np.uint8)
    got = code.decode_ms_hard_batch(x, magnitude=5, erasures=mask, output=o, iters=i, success=s)
    assert got[0] is o and got[1] is i and got[2] is s and spy.calls[0][1][3:6] == (o.ctypes.data, i.ctypes.data, s.ctypes.data)
    # what Python itself refuses, before the library sees anything
    del spy.calls[:]
    with pytest.raises(ValueError, match="n/8"):
        code.decode_ms_hard_batch(np.zeros((3, code.n()), np.uint8))
    with pytest.raises(ValueError, match="erasures"):
        code.decode_ms_hard_batch(x, erasures=mask[:2])
    with pytest.raises(ValueError, match="numpy array"):
        code.decode_ms_hard_batch([[0] * (code.n() // 8)])
    with pytest.raises(ValueError, match="erasures"):
        code.decode_ms_hard_batch(x, erasures=mask.tolist())
    with pytest.raises(ValueError, match="input must be a uint8 array"):                 # (packed bits are never cast)
        code.decode_ms_hard_batch(x.astype(np.int32) + 256)
    with pytest.raises(ValueError, match="erasures must be a uint8 array"):
        code.decode_ms_hard_batch(x, erasures=mask.astype(np.float32))
    with pytest.raises(ValueError):
        code.decode_ms_hard_batch(x, scale_num=-1)
    with pytest.raises(TypeError):
        code.decode_ms_hard_batch(x, magnitude=1.5)
    assert not spy.calls
    monkeypatch.undo()
    # ... and what the library refuses
    with pytest.raises(la.LdpcHipError, match="magnitude 0 is not in 1 .. 127"):
        code.decode_ms_hard_batch(x, magnitude=0)
    with pytest.raises(la.LdpcHipError, match="magnitude 128 is not in 1 .. 127"):
        code.decode_ms_hard_batch(x, magnitude=128, erasures=mask)
    with pytest.raises(la.LdpcHipError, match="scale_shift 40"):
        code.decode_ms_hard_batch(x, scale_shift=40)
    with pytest.raises(la.LdpcHipError, match="only variant 0 on TM1536, TM2048, TM6144 and TM8192"):
        LDPCCode.TM1280.decode_ms_hard_batch(np.zeros((1, 160), np.uint8))


# ---- the refusals, in their order, before any device work -----------------------------------------------------------------------------
TM1536, TM1280, TM5120, TC128 = int(LDPCCode.TM1536), int(LDPCCode.TM1280), int(LDPCCode.TM5120), int(LDPCCode.TC128)
STRIDE = 1 << 16
_ARENA = np.full(8 * STRIDE, 0x5A, dtype=np.uint8)
BUF = (_ARENA.ctypes.data + 15) // 16 * 16
VARIANT7 = HipOpts(-1, MEM_HOST, None, 7, 0, None)
ONLY = "not built for the packed-hard-decision bit-sliced flooding decoder on code %d (only variant 0 on TM1536, TM2048, TM6144 and TM8192 is)"
BAD_TRIPLES = (((1, 9, 0), "scale_shift 9 is not in 0 .. 8"), ((5, 2, 0), "scale_num 5 is not in 1 .. 1 << scale_shift (4)"),
               ((0, 0, 0), "scale_num 0 is not in"), ((3, 2, 128), "offset 128 is not in 0 .. 127"))
BAD_MAGNITUDES = ((0, "magnitude 0 is not in 1 .. 127"), (128, "magnitude 128 is not in 1 .. 127"), (-1, "magnitude -1 is not in 1 .. 127"),
                  (256 + 16, "magnitude 272 is not in 1 .. 127"))


def refused_device_set(variant):
    """opts that are refused once the argument checks are over and before any device is asked for: a device list with a stream"""
    return HipOpts(-1, MEM_HOST, 0x1234, variant, 2, (ctypes.c_int * 2)(0, 0))


def call(sym, code, bufs, batch, tail, opts=None):
    st = getattr(la.lib, sym)(code, *bufs, batch, *tail, ctypes.byref(opts) if opts is not None else None)
    return st, la.last_error()


def refused(got, status, text):
    assert got[0] == status and text in got[1], got


@pytest.mark.parametrize("sym,corrected", [(PLAIN, False), (CORRECTED, True)])
def test_refusals_come_in_their_order_before_any_device_work(sym, corrected):
    # the buffers: input, erasures, output, iters, success
    good = [BUF + STRIDE * i for i in range(5)]
    nulls = [None] * 5
    ok3, bad = (13, 4, 0), (1, 9, 0)

    def tail(t=ok3, magnitude=16):
        return (10, magnitude) + (t if corrected else ())
    # 1. the code, before everything
    refused(call(sym, 9, nulls, 0, tail(bad, 0)), EINVAL, "out of range")
    refused(call(sym, -1, nulls, 2, tail(bad, 0), VARIANT7), EINVAL, "out of range")
    # 2. the magnitude, even for an empty batch, whatever else is wrong
    for magnitude, text in BAD_MAGNITUDES:
        refused(call(sym, TM1280, nulls, 0, tail(bad, magnitude), VARIANT7), EINVAL, text)
        refused(call(sym, TC128, nulls, 2, tail(bad, magnitude), VARIANT7), EINVAL, text)
    # 3. the empty batch is OK and touches nothing, whatever else is wrong
    assert call(sym, TM1280, nulls, 0, tail(bad), VARIANT7) == (OK, "")
    assert call(sym, TC128, nulls, 0, tail(), HipOpts(-1, MEM_DEVICE, None, 0, 0, None)) == (OK, "")
    for magnitude in (1, 127):
        assert call(sym, TM1536, nulls, 0, tail(magnitude=magnitude)) == (OK, "")
    # 4. NULL buffers -- but not the mask's --, before the variant, the code family and the triple
    for i in (0, 2, 3, 4):
        bufs = list(good)
        bufs[i] = None
        refused(call(sym, TM1280, bufs, 2, tail(bad), VARIANT7), EINVAL, "NULL buffer")
    no_mask = [good[0], None] + good[2:]
    # 5. the variant and the code family, with a text of their own -- before the triple, at any triple, with and without a mask
    for t in (ok3, (1, 0, 0), bad):
        for bufs in (good, no_mask):
            refused(call(sym, TM1536, bufs, 2, tail(t), VARIANT7), EUNSUPPORTED, "variant 7 " + ONLY % TM1536)
            refused(call(sym, TM1536, bufs, 2, tail(t), HipOpts(-1, MEM_HOST, None, 64, 0, None)), EUNSUPPORTED, "variant 64 " + ONLY % TM1536)
            for code in (TM1280, TM5120, TC128, int(LDPCCode.TC512)):
                refused(call(sym, code, bufs, 2, tail(t)), EUNSUPPORTED, "variant 0 " + ONLY % code)
                refused(call(sym, code, bufs, 2, tail(t), refused_device_set(0)), EUNSUPPORTED, "packed-hard-decision bit-sliced")
    # 6. the triple
    if corrected:
        for triple, text in BAD_TRIPLES:
            refused(call(sym, TM1536, good, 2, tail(triple)), EINVAL, text)
            refused(call(sym, TM1536, no_mask, 2, tail(triple), refused_device_set(0)), EINVAL, text)
    # ... and what passes the argument checks goes on to the device set
    for code in (TM1536, int(LDPCCode.TM2048), int(LDPCCode.TM6144), int(LDPCCode.TM8192)):
        for t in (ok3, (1, 0, 0)):
            for bufs in (good, no_mask):
                refused(call(sym, code, bufs, 2, tail(t), refused_device_set(0)), EINVAL, "must be NULL")
    if not GPU:
        refused(call(sym, TM1536, good, 2, tail(), HipOpts(-1, MEM_HOST, None, 0, 0, None)), ENODEV, "no HIP device")
    # 7. with MEM_DEVICE the alignments, once a device is selected: output 8-byte, input and erasures 4-byte
    dev = HipOpts(-1, MEM_DEVICE, None, 0, 0, None)
    for at, off, text in ((2, 4, "device output buffer must be 8-byte aligned"), (0, 2, "device input buffer must be 4-byte aligned"),
                          (0, 1, "device input buffer must be 4-byte aligned"), (1, 2, "device erasures buffer must be 4-byte aligned"),
                          (1, 3, "device erasures buffer must be 4-byte aligned")):
        bufs = list(good)
        bufs[at] += off
        got = call(sym, TM1536, bufs, 2, tail(), dev)
        refused(got, EINVAL, text) if GPU else refused(got, ENODEV, "no HIP device")
    assert (_ARENA == 0x5A).all()                                                   # nothing was written anywhere
