"""Soft output from the f32-reading bit-sliced i8 decoders and their cascade, what can be said without a GPU: the
shared frames exercise what they must, the three new symbols exist in the header, the library, the Python table and the Rust shim,
the two new Python methods choose them, pass their arguments and refuse what they must, and every refusal of the C entries comes in
its order -- each fault alone and in pairs -- before any device work.  The ABI version stays 3."""
import ctypes
import os
import re

import numpy as np
import pytest

import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode, HipOpts, MEM_HOST, MEM_DEVICE

import bs_quantised_soft_frames as bqs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, ENODEV, EUNSUPPORTED = 0, -1, -2, -4
GPU = la.device_count() > 0
PLAIN = "labrador_ldpc_decode_ms_bitsliced_quantised_soft_batch_i8"
CORRECTED = "labrador_ldpc_decode_ms_bitsliced_quantised_corrected_soft_batch_i8"
CASCADE = "labrador_ldpc_decode_ms_cascade_bitsliced_quantised_soft_batch_i8"
# (symbol, arguments, the hard entry it stands beside: the same list without `app`)
SYMBOLS = ((PLAIN, 11, "labrador_ldpc_decode_ms_bitsliced_quantised_batch_i8"),
           (CORRECTED, 14, "labrador_ldpc_decode_ms_bitsliced_quantised_corrected_batch_i8"),
           (CASCADE, 19, "labrador_ldpc_decode_ms_cascade_bitsliced_quantised_batch_i8"))


@pytest.mark.parametrize("name", bqs.NAMES)
def test_the_shared_frames_meet_their_conditions(name):
    """bs_quantised_frames.py's conditions, and marginals that reach -128 and 127 with failing frames in the plain form and at every
    triple, from the references alone"""
    x = bqs.frames(name)
    assert x.dtype == np.float32 and x.shape == (3 * bqs.GROUP[name] + 1, LDPCCode[name].n())
    bqs.assert_conditions(name)
    va, out, it, ok = bqs.expected_plain(name, 127, 25)
    assert va.dtype == np.int8 and va.shape == (len(x), LDPCCode[name].n() + LDPCCode[name].punctured_bits())
    assert np.array_equal(np.packbits((va < 0).astype(np.uint8), axis=1), out)            # the hard word is the marginal's sign
    assert not bqs.expected_plain(name, 127, 0)[0].any()


def test_the_launcher_picks_the_form_from_the_scale():
    assert [bqs.mulbits(t) for t in bqs.TRIPLES] == [4, 0, 8] and bqs.mulbits(bqs.IDENTITY) == 0


# ---- the symbols ----------------------------------------------------------------------------------------------------------------------
def test_the_new_symbols_are_declared_exported_bound_and_mirrored():
    header = open(os.path.join(ROOT, "include", "labrador_ldpc_hip.h")).read()
    shim = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for sym, nargs, hard in SYMBOLS:
        m = re.search(r"\bint %s\(([^;]*?)\);" % sym, header)
        assert m and len(m.group(1).split(",")) == nargs, sym
        assert sym in la.SYMBOLS and len(la.SYMBOLS[sym][1]) == nargs
        assert getattr(la.lib, sym) is not None
        assert re.search(r"pub fn %s\(" % sym, shim), sym
        # the argument list of the hard entry it stands beside, with `app` behind `llrs`
        args = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
        theirs = [re.sub(r"\s+", " ", a).strip() for a in re.search(r"\bint %s\s*\(([^;]*?)\);" % hard, header).group(1).split(",")]
        assert args[2] == ("int32_t *app" if sym == CASCADE else "int8_t *app"), args[2]
        assert args[:2] + args[3:] == theirs, (sym, args, theirs)
        assert [a.__name__ for a in la.SYMBOLS[sym][1]] == [a.__name__ for a in la.SYMBOLS[hard][1][:2] + [ctypes.c_void_p] + la.SYMBOLS[hard][1][2:]]
    assert re.search(r"LABRADOR_LDPC_HIP_ABI\s+3\b", header)
    assert la.lib.labrador_ldpc_hip_abi_version() == 3


def test_the_header_says_that_the_cascade_must_not_be_captured():
    header = open(os.path.join(ROOT, "include", "labrador_ldpc_hip.h")).read()
    block = header[header.index("WITH SOFT OUTPUT (DESIGN.md 4.20)"):header.index("int " + PLAIN)]
    assert "captured" in block and "SYNCHRONISES" in block and "16-byte aligned" in block


# ---- the Python methods -------------------------------------------------------------------------------------------------------------
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


def test_python_methods_choose_the_entry_point_and_pass_the_arguments(monkeypatch):
    code = LDPCCode.TM1536
    spy = _SpyLib(la.lib)
    monkeypatch.setattr(la, "lib", spy)
    llrs = np.ones((3, code.n()), np.float32)
    npv = code.n() + code.punctured_bits()
    for kw, sym, tail in (({}, PLAIN, ()), (dict(scale_num=13, scale_shift=4), CORRECTED, (13, 4, 0)), (dict(offset=1), CORRECTED, (1, 0, 1)),
                          (dict(scale_shift=4), CORRECTED, (16, 4, 0)), (dict(scale_num=1), CORRECTED, (1, 0, 0))):
        del spy.calls[:]
        res = code.decode_ms_bitsliced_quantised_soft_batch(llrs, 4.0, 31, 25, **kw)
        (name, args), = spy.calls
        assert name == sym and len(args) == 1 + 5 + 4 + len(tail) + 1 and args[6:10 + len(tail)] == (3, 25, 4.0, 31) + tail, (name, kw)
        assert args[0] == int(code) and args[1] == llrs.ctypes.data
        assert len(res) == 4 and res[0].dtype == np.int8 and res[0].shape == (3, npv) and args[2] == res[0].ctypes.data
        assert res[1].shape == (3, code.output_len()) and args[3] == res[1].ctypes.data
    del spy.calls[:]
    code.decode_ms_bitsliced_quantised_soft_batch(llrs, 8.0, 127)                       # maxiters defaults to 50
    assert spy.calls[0][1][6:10] == (3, 50, 8.0, 127)
    # the cascade
    for kw, t1 in (({}, (1, 0, 0)), (dict(flooding_scale_num=13, flooding_scale_shift=4), (13, 4, 0)), (dict(flooding_offset=1), (1, 0, 1))):
        for stage2, t2 in (({}, (1, 0, 0)), (dict(scale_num=3, scale_shift=2, offset=1), (3, 2, 1))):
            del spy.calls[:]
            res = code.decode_ms_cascade_bitsliced_quantised_soft_batch(llrs, 8.0, 31, 25, 7, **kw, **stage2)
            (name, args), = spy.calls
            assert name == CASCADE and len(args) == 19 and args[7:18] == (3, 25, 7, 8.0, 31) + t1 + t2, (name, kw, stage2)
            assert len(res) == 5 and res[0].dtype == np.int32 and res[0].shape == (3, npv) and res[4].dtype == np.uint8
            assert [args[i] for i in range(1, 7)] == [llrs.ctypes.data] + [r.ctypes.data for r in res]
    del spy.calls[:]
    code.decode_ms_cascade_bitsliced_quantised_soft_batch(llrs, 8.0, 31, 9)             # max_sweeps None = maxiters
    assert spy.calls[0][1][7:10] == (3, 9, 9)
    # the refusals: any dtype but float32 is LdpcHipError; what a uint32_t would wrap silently is a ValueError
    del spy.calls[:]
    for dtype in (np.int8, np.int16, np.float64, np.float16):
        bad = np.ones((1, code.n()), dtype)
        with pytest.raises(la.LdpcHipError, match="no batched kernel"):
            code.decode_ms_bitsliced_quantised_soft_batch(bad, 8.0, 31)
        with pytest.raises(la.LdpcHipError, match="no batched kernel"):
            code.decode_ms_bitsliced_quantised_soft_batch(bad, 8.0, 31, offset=1)
        with pytest.raises(la.LdpcHipError, match="no batched kernel"):
            code.decode_ms_cascade_bitsliced_quantised_soft_batch(bad, 8.0, 31)
    with pytest.raises(ValueError):
        code.decode_ms_bitsliced_quantised_soft_batch(llrs, 8.0, 31, scale_num=-1)
    with pytest.raises(ValueError):
        code.decode_ms_cascade_bitsliced_quantised_soft_batch(llrs, 8.0, 31, flooding_offset=1 << 32)
    with pytest.raises(ValueError):
        code.decode_ms_bitsliced_quantised_soft_batch(llrs[:, :-1], 8.0, 31)
    with pytest.raises(TypeError):
        code.decode_ms_bitsliced_quantised_soft_batch(llrs, 8.0, 31.5)
    assert not spy.calls                                                             # ... before the library sees anything
    monkeypatch.undo()
    with pytest.raises(la.LdpcHipError, match="scale_shift 40"):
        code.decode_ms_bitsliced_quantised_soft_batch(llrs, 8.0, 31, scale_shift=40)
    with pytest.raises(la.LdpcHipError, match="lim 128"):
        code.decode_ms_cascade_bitsliced_quantised_soft_batch(llrs, 8.0, 128)
    for c in (LDPCCode.TM1280, LDPCCode.TC256):
        x = np.ones((1, c.n()), np.float32)
        with pytest.raises(la.LdpcHipError, match="only variant 0 on TM1536, TM2048, TM6144 and TM8192"):
            c.decode_ms_bitsliced_quantised_soft_batch(x, 8.0, 31)
        with pytest.raises(la.LdpcHipError, match="only variant 0 on TM1536, TM2048, TM6144 and TM8192"):
            c.decode_ms_cascade_bitsliced_quantised_soft_batch(x, 8.0, 31)


def test_the_existing_methods_keep_their_signatures():
    """the new entries are new methods: the hard ones have no `app`, the i8 soft ones no `scale`"""
    import inspect
    assert "app" not in inspect.signature(LDPCCode.decode_ms_quantised_batch).parameters
    assert "app" not in inspect.signature(LDPCCode.decode_ms_cascade_quantised_batch).parameters
    assert "scale" not in inspect.signature(LDPCCode.decode_ms_bitsliced_soft_batch).parameters
    assert list(inspect.signature(LDPCCode.decode_ms_bitsliced_quantised_soft_batch).parameters)[:5] == ["self", "llrs", "scale", "lim", "maxiters"]
    assert list(inspect.signature(LDPCCode.decode_ms_cascade_bitsliced_quantised_soft_batch).parameters)[:6] == \
        ["self", "llrs", "scale", "lim", "maxiters", "max_sweeps"]


# ---- the refusals, in their order, before any device work -----------------------------------------------------------------------------
TM1536, TM1280, TM5120, TC128 = int(LDPCCode.TM1536), int(LDPCCode.TM1280), int(LDPCCode.TM5120), int(LDPCCode.TC128)
STRIDE = 1 << 16
_ARENA = np.full(8 * STRIDE, 0x5A, dtype=np.uint8)
BUF = (_ARENA.ctypes.data + 15) // 16 * 16
VARIANT7 = HipOpts(-1, MEM_HOST, None, 7, 0, None)
ONLY = "not built for the f32-reading soft bit-sliced flooding decoder on code %d (only variant 0 on TM1536, TM2048, TM6144 and TM8192 is)"
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


@pytest.mark.parametrize("sym,nbuf,caps,ntriples", [(PLAIN, 5, (10,), 0), (CORRECTED, 5, (10,), 1), (CASCADE, 6, (10, 10), 2)])
def test_refusals_come_in_their_order_before_any_device_work(sym, nbuf, caps, ntriples):
    """buffers: llrs, app, output, iters, success [, stage]"""
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
    # 4. NULL buffers (`app` included; the cascade: `stage` too), before the variant, the code family and the triples
    for i in range(nbuf):
        bufs = list(good)
        bufs[i] = None
        refused(call(sym, TM1280, bufs, 2, tail(bad), VARIANT7), EINVAL, "NULL buffer")
        refused(call(sym, TM1536, bufs, 2, tail()), EINVAL, "NULL buffer")
    # 5. the variant and the code family, with a text of their own -- before the triples, at any triple
    for t1 in (ok3, (1, 0, 0), bad):
        refused(call(sym, TM1536, good, 2, tail(t1), VARIANT7), EUNSUPPORTED, "variant 7 " + ONLY % TM1536)
        refused(call(sym, TM1536, good, 2, tail(t1), HipOpts(-1, MEM_HOST, None, 64, 0, None)), EUNSUPPORTED, "variant 64 " + ONLY % TM1536)
        for code in (TM1280, TM5120, TC128, int(LDPCCode.TC512)):
            refused(call(sym, code, good, 2, tail(t1)), EUNSUPPORTED, "variant 0 " + ONLY % code)
            refused(call(sym, code, good, 2, tail(t1), VARIANT7), EUNSUPPORTED, "variant 7 " + ONLY % code)
            refused(call(sym, code, good, 2, tail(t1), refused_device_set(0)), EUNSUPPORTED, "f32-reading soft bit-sliced")
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
    # 7. with MEM_DEVICE the alignments, once a device is selected: output 8-byte, app and llrs 16-byte
    dev = HipOpts(-1, MEM_DEVICE, None, 0, 0, None)
    for at, off, text in ((2, 4, "device output buffer must be 8-byte aligned"), (1, 8, "device app buffer must be 16-byte aligned"),
                          (1, 4, "device app buffer must be 16-byte aligned"), (0, 4, "device llrs buffer must be 16-byte aligned"),
                          (0, 8, "device llrs buffer must be 16-byte aligned")):
        bufs = list(good)
        bufs[at] += off
        got = call(sym, TM1536, bufs, 2, tail(), dev)
        refused(got, EINVAL, text) if GPU else refused(got, ENODEV, "no HIP device")
    assert (_ARENA == 0x5A).all()                                                   # nothing was written anywhere
