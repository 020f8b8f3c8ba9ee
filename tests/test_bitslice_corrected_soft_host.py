"""Soft output from the corrected bit-sliced i8 kernels, what can be said without a GPU: the statement the kernels
are compared with (flooding_fixed_corrected_soft_restatement.py) is tied to the two references it extends, its two forms agree, the
shared frames exercise what they must under the corrected decoder alone, the two new symbols exist in the header, the library, the
Python table and the Rust shim, the Python keywords choose them, and every refusal comes in its order before any device work."""
import ctypes
import os
import re

import numpy as np
import pytest

import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode, HipOpts, MEM_HOST, MEM_DEVICE

import bs_corrected_soft_frames as bcf
import bs_soft_frames as bsf
import flooding_fixed_corrected_restatement as hard_statement
import flooding_fixed_corrected_soft_restatement as statement
import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, ENODEV, EUNSUPPORTED = 0, -1, -2, -4
GPU = la.device_count() > 0
ENTRY = "labrador_ldpc_decode_ms_bitsliced_corrected_soft_batch_i8"
CASCADE = "labrador_ldpc_decode_ms_cascade_bitsliced_corrected_soft_batch_i8"


# ---- the statement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", bcf.NAMES)
def test_the_statement_is_tied_to_the_oracle_and_to_the_hard_corrected_statement(name):
    """At (1,0,0) all four arrays are the oracle's soft decode; at every other triple the hard three are the hard corrected
    statement's; (255,8,0) maps every magnitude of 0 .. 127 to itself, so it is the oracle's soft decode again."""
    code = oracle.CODES.index(name)
    st, llrs = statement.structure(code), bcf.frames(name)
    for m in range(128):
        assert int(statement.correct(m, 255, 8, 0)) == m
    for triple in bcf.TRIPLES:
        got = bcf.expected(name, triple)
        hard = hard_statement.decode_caps(st, llrs, bcf.CAPS, *triple)
        for cap in bcf.CAPS:
            out, it, ok, va = got[cap]
            assert va.dtype == np.int8 and va.shape == (len(llrs), oracle.n(code) + oracle.p(code))
            for a, b in zip((out, it, ok), hard[cap]):
                assert np.array_equal(a, b), (name, triple, cap)
            if triple in (bcf.IDENTITY, (255, 8, 0)):
                for a, b in zip(got[cap], bsf.expected(name, cap)):
                    assert np.array_equal(a, b), (name, triple, cap)
            assert np.array_equal(np.packbits((va < 0).astype(np.uint8), axis=1), out) or cap == 0       # the hard word is the marginal's sign
        assert not got[0][3].any() and not got[0][0].any() and not got[0][2].any()


def test_the_two_forms_of_the_statement_agree():
    """whole arrays against one frame edge by edge, TM1536: near-threshold, corner and flat frames, converging and failing"""
    name = "TM1536"
    st, llrs = statement.structure(oracle.CODES.index(name)), bcf.frames(name)
    seen = set()
    for triple in ((13, 4, 0), (3, 2, 1)):
        want = bcf.expected(name, triple)
        for f in range(6):
            for cap in (0, 3, 25):
                out, it, ok, va = statement.decode_loop(st, llrs[f], cap, *triple)
                wo, wi, wk, wa = (a[f] for a in want[cap])
                assert np.array_equal(out, wo) and it == wi and ok == wk and np.array_equal(va, wa), (triple, f, cap)
                seen.add(int(ok))
    assert seen == {0, 1}                                                            # (both a converging and a failing decode were walked)


@pytest.mark.parametrize("name", bcf.NAMES)
def test_the_shared_frames_meet_their_conditions_under_the_corrected_statement(name):
    bcf.assert_conditions(name)


def test_the_launcher_picks_the_form_from_the_scale():
    assert [bcf.mulbits(t) for t in bcf.TRIPLES] == [0, 4, 0, 4, 8, 8]
    assert bcf.mulbits((16, 4, 0)) == 0 and bcf.mulbits((256, 8, 3)) == 0


# ---- the symbols ----------------------------------------------------------------------------------------------------------------------
def test_the_new_symbols_are_declared_exported_bound_and_mirrored():
    header = open(os.path.join(ROOT, "include", "labrador_ldpc_hip.h")).read()
    shim = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for sym, nargs in ((ENTRY, 12), (CASCADE, 17)):
        m = re.search(r"\bint %s\(([^;]*?)\);" % sym, header)
        assert m and len(m.group(1).split(",")) == nargs, sym
        assert sym in la.SYMBOLS and len(la.SYMBOLS[sym][1]) == nargs
        assert getattr(la.lib, sym) is not None
        assert re.search(r"pub fn %s\(" % sym, shim), sym
    assert "#define LABRADOR_LDPC_HIP_ABI 3" in header or re.search(r"LABRADOR_LDPC_HIP_ABI\s+3\b", header)


# ---- the Python keywords ------------------------------------------------------------------------------------------------------------
class _SpyLib:
    """Stands where the package keeps its library: a bit-sliced soft decode looked up through it is recorded with its arguments and
    reports success without doing anything; every other symbol is the library's own."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        if "bitsliced" not in name and "cascade_soft_batch" not in name:
            return getattr(self.real, name)

        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


KEYWORDS = (({}, None), (dict(scale_num=13, scale_shift=4), (13, 4, 0)), (dict(scale_shift=4), (16, 4, 0)), (dict(offset=1), (1, 0, 1)),
            (dict(scale_num=1), (1, 0, 0)), (dict(scale_shift=8, offset=2), (256, 8, 2)))


def test_python_keywords_choose_the_entry_point(monkeypatch):
    code = LDPCCode.TM1536
    spy = _SpyLib(la.lib)
    monkeypatch.setattr(la, "lib", spy)
    llrs = np.ones((3, code.n()), np.int8)
    for kw, triple in KEYWORDS:
        del spy.calls[:]
        code.decode_ms_bitsliced_soft_batch(llrs, 25, **kw)
        (name, args), = spy.calls
        if triple is None:
            assert name == "labrador_ldpc_decode_ms_bitsliced_soft_batch_i8" and len(args) == 1 + 5 + 3
        else:
            assert name == ENTRY and len(args) == 1 + 5 + 6 and args[6:11] == (3, 25) + triple, (name, kw)
    # the cascade: flooding_* with bitsliced choose the new symbol, the stage-2 triple keeps its place behind it
    for kw, triple in KEYWORDS:
        fkw = {"flooding_" + k: v for k, v in kw.items()}
        for stage2, t2 in (({}, (1, 0, 0)), (dict(scale_num=3, scale_shift=2, offset=1), (3, 2, 1))):
            del spy.calls[:]
            code.decode_ms_cascade_fixed_soft_batch(llrs, 25, 7, bitsliced=True, **fkw, **stage2)
            (name, args), = spy.calls
            if triple is None:
                assert name == "labrador_ldpc_decode_ms_cascade_bitsliced_soft_batch_i8" and args[7:13] == (3, 25, 7) + t2
            else:
                assert name == CASCADE and len(args) == 1 + 6 + 10 and args[7:16] == (3, 25, 7) + triple + t2, (name, kw)
            if triple is not None:
                with pytest.raises(ValueError, match="only bit-sliced"):
                    code.decode_ms_cascade_fixed_soft_batch(llrs, 25, 7, **fkw, **stage2)
    del spy.calls[:]
    code.decode_ms_cascade_fixed_soft_batch(llrs, 25, 7)                             # none given, not bit-sliced: unchanged
    (name, args), = spy.calls
    assert name == "labrador_ldpc_decode_ms_cascade_soft_batch_i8"
    # int8 only, whatever the keywords; what a uint32_t would wrap silently is refused here
    for dtype in (np.int16, np.float32):
        with pytest.raises(la.LdpcHipError, match="no batched kernel"):
            code.decode_ms_bitsliced_soft_batch(np.ones((1, code.n()), dtype), 25, offset=1)
        with pytest.raises(la.LdpcHipError, match="no batched kernel"):
            code.decode_ms_cascade_fixed_soft_batch(np.ones((1, code.n()), dtype), 25, bitsliced=True, flooding_offset=1)
    with pytest.raises(ValueError):
        code.decode_ms_bitsliced_soft_batch(llrs, 25, scale_num=-1)
    with pytest.raises(ValueError):
        code.decode_ms_cascade_fixed_soft_batch(llrs, 25, bitsliced=True, flooding_offset=1 << 32)
    with pytest.raises(TypeError):
        code.decode_ms_bitsliced_soft_batch(llrs, 25, offset=0.5)
    monkeypatch.undo()
    with pytest.raises(la.LdpcHipError, match="scale_shift 40"):
        code.decode_ms_bitsliced_soft_batch(llrs, 25, scale_shift=40)
    with pytest.raises(la.LdpcHipError, match="scale_shift 40"):
        code.decode_ms_cascade_fixed_soft_batch(llrs, 25, bitsliced=True, flooding_scale_shift=40)
    with pytest.raises(ValueError, match="only bit-sliced"):                         # ... before the library sees anything
        code.decode_ms_cascade_fixed_soft_batch(llrs, 25, flooding_scale_shift=40)


# ---- the refusals, in their order, before any device work -----------------------------------------------------------------------------
TM1536, TM1280, TC128 = int(LDPCCode.TM1536), int(LDPCCode.TM1280), int(LDPCCode.TC128)
STRIDE = 1 << 16
_ARENA = np.full(8 * STRIDE, 0x5A, dtype=np.uint8)
BUF = (_ARENA.ctypes.data + 15) // 16 * 16
VARIANT7 = HipOpts(-1, MEM_HOST, None, 7, 0, None)
ONLY = "not built for the soft bit-sliced flooding decoder on code %d (only variant 0 on TM1536, TM2048, TM6144 and TM8192 is)"
TWO_WAVE = "code %d decodes on the two-wave bit-sliced kernels (TM1280, TM5120), which have no soft form"
BAD_TRIPLES = (((1, 9, 0), "scale_shift 9 is not in 0 .. 8"), ((5, 2, 0), "scale_num 5 is not in 1 .. 1 << scale_shift (4)"),
               ((0, 0, 0), "scale_num 0 is not in"), ((3, 2, 128), "offset 128 is not in 0 .. 127"))


def refused_device_set(variant):
    """opts that are refused once the argument checks are over and before any device is asked for: a device list with a stream"""
    return HipOpts(-1, MEM_HOST, 0x1234, variant, 2, (ctypes.c_int * 2)(0, 0))


def call(sym, code, bufs, batch, tail, opts=None):
    st = getattr(la.lib, sym)(code, *bufs, batch, *tail, ctypes.byref(opts) if opts is not None else None)
    return st, la.last_error()


def refused(got, status, text):
    assert got[0] == status and text in got[1], got


@pytest.mark.parametrize("sym,nbuf,caps", [(ENTRY, 5, (10,)), (CASCADE, 6, (10, 10))])
def test_refusals_come_in_their_order_before_any_device_work(sym, nbuf, caps):
    good = [BUF + STRIDE * i for i in range(nbuf)]
    nulls = [None] * nbuf
    cascade = sym == CASCADE
    tail = lambda t1, t2=(3, 2, 0): caps + t1 + (t2 if cascade else ())            # noqa: E731
    bad, ok3 = (1, 9, 0), (13, 4, 0)
    # 1. the code, before everything
    refused(call(sym, 9, nulls, 0, tail(bad)), EINVAL, "out of range")
    refused(call(sym, -1, nulls, 2, tail(bad), VARIANT7), EINVAL, "out of range")
    # 2. the empty batch is OK and touches nothing, whatever else is wrong
    assert call(sym, TM1280, nulls, 0, tail(bad), VARIANT7) == (OK, "")
    assert call(sym, TC128, nulls, 0, tail(ok3), HipOpts(-1, MEM_DEVICE, None, 0, 0, None)) == (OK, "")
    # 3. NULL buffers, app included, before the triple
    for i in range(nbuf):
        bufs = list(good)
        bufs[i] = None
        refused(call(sym, TM1280, bufs, 2, tail(bad), VARIANT7), EINVAL, "NULL buffer")
    # 4. the triple (the cascade: stage 1's first, then stage 2's), before the variant and the code family
    for triple, text in BAD_TRIPLES:
        refused(call(sym, TM1280, good, 2, tail(triple), VARIANT7), EINVAL, text)
        refused(call(sym, TC128, good, 2, tail(triple), refused_device_set(7)), EINVAL, text)
        if cascade:
            refused(call(sym, TM1280, good, 2, tail(ok3, triple), VARIANT7), EINVAL, text)
            refused(call(sym, TM1280, good, 2, tail((1, 0, 0), triple), VARIANT7), EINVAL, text)
    if cascade:
        refused(call(sym, TM1536, good, 2, tail((3, 9, 0), (3, 10, 0))), EINVAL, "scale_shift 9 is not in")
        refused(call(sym, TM1536, good, 2, tail((4, 2, 0), (3, 10, 0))), EINVAL, "scale_shift 10 is not in")
    # 5. the variant and the code family, with the soft entry's texts -- at an identity triple as well
    for t1 in (ok3, (1, 0, 0), (16, 4, 0), (1, 0, 1)):
        refused(call(sym, TM1280, good, 2, tail(t1), VARIANT7), EUNSUPPORTED, "variant 7 " + ONLY % TM1280)      # the variant, not the two waves
        refused(call(sym, TM1536, good, 2, tail(t1), VARIANT7), EUNSUPPORTED, "variant 7 " + ONLY % TM1536)
        refused(call(sym, TM1280, good, 2, tail(t1)), EUNSUPPORTED, TWO_WAVE % TM1280)
        refused(call(sym, int(LDPCCode.TM5120), good, 2, tail(t1)), EUNSUPPORTED, TWO_WAVE % int(LDPCCode.TM5120))
        refused(call(sym, TC128, good, 2, tail(t1)), EUNSUPPORTED, "variant 0 " + ONLY % TC128)
        refused(call(sym, TC128, good, 2, tail(t1), refused_device_set(0)), EUNSUPPORTED, "soft bit-sliced")
        # ... and what passes the argument checks goes on to the device set
        for code in (TM1536, int(LDPCCode.TM2048), int(LDPCCode.TM6144), int(LDPCCode.TM8192)):
            refused(call(sym, code, good, 2, tail(t1), refused_device_set(0)), EINVAL, "must be NULL")
        if not GPU:
            refused(call(sym, TM1536, good, 2, tail(t1), HipOpts(-1, MEM_HOST, None, 0, 0, None)), ENODEV, "no HIP device")
    # 6. with MEM_DEVICE the alignments, once a device is selected: output 8-byte, app 16-byte, llrs 4-byte
    dev = HipOpts(-1, MEM_DEVICE, None, 0, 0, None)
    out_at = 2
    for at, off, text in ((out_at, 4, "device output buffer must be 8-byte aligned"), (1, 4, "device app buffer must be 16-byte aligned"),
                          (0, 2, "device llrs buffer must be 4-byte aligned")):
        bufs = list(good)
        bufs[at] += off
        got = call(sym, TM1536, bufs, 2, tail(ok3), dev)
        refused(got, EINVAL, text) if GPU else refused(got, ENODEV, "no HIP device")
    assert (_ARENA == 0x5A).all()                                                   # nothing was written anywhere
