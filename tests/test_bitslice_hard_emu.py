"""The bit-sliced i8 decoder reading packed hard decisions (labrador_ldpc_amd/csrc/decode_ms_bitslice.hpp, load_column_planes<...,
PackedHard>) validated WITHOUT a GPU: tests/c/bitslice_hard_emu.cpp instantiates the kernels' own source text -- the
packed loader, the iteration, the correction step, the epilogue -- with a backend whose wave register is an array of 64 lanes, whose LDS
accessors are bounds-checked against Geo::LDS_BYTES and whose global loads -- the packed loader's dwords included -- must stay inside
the batch's rows of `input` and of `erasures`.  This file compares the results frame by frame with the statements
(tests/bs_hard_frames.py: the numpy expansion of the contract, then the oracle or flooding_fixed_corrected_restatement.py).  The GPU
tests then only have to show that gfx950 executes the same text the same way (tests/test_gpu_bs_hard.py)."""
import ctypes

import numpy as np
import pytest

import bs_hard_frames as bhf
import bitslice_emu_build
import oracle

TM = bhf.NAMES
# the corrected form: every triple in the form the launcher picks -- (13,4,0) four bits, (1,0,1) the offset alone, (200,8,1) eight
FORMS = [(t, bhf.mulbits(t)) for t in bhf.TRIPLES]
assert [m for _, m in FORMS] == [4, 0, 8]


@pytest.fixture(scope="module")
def emu():
    """One shared object per code, the stale ones rebuilt in parallel (fully unrolled 64-lane code, five forms: about a minute each)."""
    libs = bitslice_emu_build.build("bitslice_hard_emu.cpp", ("decode_ms_bitslice.hpp", "codes.hpp", "decode_ms_bs_plan.hpp", "decode_ms_tuning.hpp"), TM)
    loaded = {}
    for name, L in libs.items():
        L.bsh_emu_decode.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_size_t] + [ctypes.c_uint32] * 5 + [ctypes.c_int]
        L.bsh_emu_decode_i8.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_size_t, ctypes.c_uint32]
        L.bsh_emu_mulbits.argtypes = [ctypes.c_uint32] * 2
        assert L.bsh_emu_code() == oracle.CODES.index(name)
        loaded[name] = L
    return loaded


def batches_of(g):
    return sorted({b for b in (g - 1, g, g + 1, 3 * g + 1) if b >= 1})      # a partial group and its padding lanes, whole groups


def run(L, code, x, m, cap, magnitude, triple, mulbits):
    """the emulated decode of packed frames x under mask rows m (None: no mask), each result with a guard row behind it.  The rows are
    copies of exactly the batch's size, so a load behind them is outside the window the emulator checks."""
    B = len(x)
    x = np.array(x[:B], np.uint8, order="C")
    m = None if m is None else np.array(m[:B], np.uint8, order="C")
    out = np.full((B + 1, oracle.output_len(code)), 0xEE, np.uint8)
    it, ok = np.full(B + 1, 0xEEEEEEEE, np.uint32), np.full(B + 1, 0xEE, np.uint8)
    st = L.bsh_emu_decode(x.ctypes.data, None if m is None else m.ctypes.data, out.ctypes.data, it.ctypes.data, ok.ctypes.data, B, cap, magnitude,
                          *triple, mulbits)
    assert st == 0, f"the kernel text left its LDS layout, the batch's rows or an alignment ({st})"
    assert (out[B] == 0xEE).all() and it[B] == 0xEEEEEEEE and ok[B] == 0xEE, "a result row behind the batch was written"
    return out[:B], it[:B], ok[:B]


def differing(got, want, B):
    (out, it, ok), (wo, wi, wk) = got, (a[:B] for a in want)
    return np.nonzero((out != wo).any(axis=1) | (it != wi) | (ok != wk))[0]


@pytest.mark.parametrize("name", TM)
def test_the_frames_meet_their_conditions(name):
    x, m = bhf.frames(name)
    g = bhf.GROUP[name]
    assert x.shape == m.shape == (3 * g + 1, oracle.n(oracle.CODES.index(name)) // 8)
    assert (x == 0).all(axis=1).sum() == 1 and (x == 0xFF).all(axis=1).sum() == 1                # the two flat rows
    assert [bool(r.any()) for r in m] == [i % 3 == 0 for i in range(len(m))]                      # every third frame has a mask
    bhf.assert_conditions(name)


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("name", TM)
def test_emulated_plain_form_equals_the_oracle_on_the_expanded_frames(emu, name, masked):
    code, L = oracle.CODES.index(name), emu[name]
    g = L.bsh_emu_group()
    assert g == bhf.GROUP[name]
    x, m = bhf.frames(name)
    for magnitude in bhf.MAGNITUDES:
        for cap in bhf.CAPS:
            want = bhf.expected_plain(name, magnitude, masked, cap)
            for B in batches_of(g):
                got = run(L, code, x[:B], m[:B] if masked else None, cap, magnitude, bhf.IDENTITY, -1)
                bad = differing(got, want, B)
                assert bad.size == 0, f"{name} magnitude {magnitude} cap {cap} batch {B}: frames {bad.tolist()[:8]} differ"


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("name", TM)
def test_emulated_corrected_form_equals_the_statement_on_the_expanded_frames(emu, name, masked):
    code, L = oracle.CODES.index(name), emu[name]
    g = L.bsh_emu_group()
    x, m = bhf.frames(name)
    for triple, mulbits in FORMS:
        assert L.bsh_emu_mulbits(triple[0], triple[1]) == mulbits
        want = bhf.expected_corrected(name, triple, masked)
        for cap in bhf.CAPS:
            for B in batches_of(g):
                got = run(L, code, x[:B], m[:B] if masked else None, cap, bhf.CORRECTED_MAGNITUDE, triple, mulbits)
                bad = differing(got, want[cap], B)
                assert bad.size == 0, f"{name} {triple}/{mulbits} cap {cap} batch {B}: frames {bad.tolist()[:8]} differ"
    # a triple that does not fit the form it is asked in, and a magnitude out of range, are refused by the emulator itself, not run
    assert L.bsh_emu_decode(None, None, None, None, None, 0, 1, 16, 13, 4, 0, 0) == 2
    assert L.bsh_emu_decode(None, None, None, None, None, 0, 1, 128, 1, 0, 0, -1) == 2


@pytest.mark.parametrize("name", TM)
def test_the_identity_triple_in_the_corrected_form_equals_the_plain_form(emu, name):
    """every spelling of the identity is the offset-only form's (correction_mulbits: scale_num << (8 - scale_shift) == 256)"""
    code, L = oracle.CODES.index(name), emu[name]
    B = 3 * L.bsh_emu_group() + 1
    x, m = bhf.frames(name)
    for cap in (3, 25):
        plain = run(L, code, x, m, cap, 16, bhf.IDENTITY, -1)
        for triple in ((1, 0, 0), (16, 4, 0), (256, 8, 0)):
            assert L.bsh_emu_mulbits(triple[0], triple[1]) == 0
            got = run(L, code, x, m, cap, 16, triple, 0)
            assert differing(got, plain, B).size == 0, (name, cap, triple)


@pytest.mark.parametrize("name", TM)
def test_the_i8_source_decoder_of_the_edited_header_still_equals_the_oracle(emu, name):
    code, L = oracle.CODES.index(name), emu[name]
    g = L.bsh_emu_group()
    for magnitude in (1, 127):
        e = bhf.expanded(name, magnitude, True)
        for cap in (0, 3, 25):
            want = bhf.expected_plain(name, magnitude, True, cap)
            for B in batches_of(g):
                x = np.ascontiguousarray(e[:B])
                out = np.full((B + 1, oracle.output_len(code)), 0xEE, np.uint8)
                it, ok = np.full(B + 1, 0xEEEEEEEE, np.uint32), np.full(B + 1, 0xEE, np.uint8)
                assert L.bsh_emu_decode_i8(x.ctypes.data, out.ctypes.data, it.ctypes.data, ok.ctypes.data, B, cap) == 0
                assert differing((out[:B], it[:B], ok[:B]), want, B).size == 0, (name, magnitude, cap, B)
                assert (out[B] == 0xEE).all() and it[B] == 0xEEEEEEEE and ok[B] == 0xEE
