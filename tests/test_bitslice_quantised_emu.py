"""The bit-sliced i8 decoder reading f32 LLRs (labrador_ldpc_amd/csrc/decode_ms_bitslice.hpp, load_column_planes<..., QuantisedF32>;
DESIGN.md 4.19) validated WITHOUT a GPU: tests/c/bitslice_quantised_emu.cpp instantiates the kernels' own source text -- the f32 loader,
the iteration, the correction step, the epilogue -- with a backend whose wave register is an array of 64 lanes, whose LDS accessors are
bounds-checked against Geo::LDS_BYTES and whose 16-byte global loads must stay inside the batch's rows, and whose quantiser is the
library's own ldpc::quantise_llr compiled by g++.  This file compares the results frame by frame with the statements
(tests/bs_quantised_frames.py: quantise_restatement.py, then the oracle or flooding_fixed_corrected_restatement.py).  The GPU tests
then only have to show that gfx950 executes the same text the same way (tests/test_gpu_bs_quantised.py)."""
import ctypes
import os

import numpy as np
import pytest

import bs_quantised_frames as bqf
import bitslice_emu_build
import oracle
import quantise_restatement

TM = bqf.NAMES
ROCM_INC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
# (the library's flags for the one multiply: nothing fused into it; the HIP headers llr_quantise.hpp needs)
F32_FLAGS = ["-fno-fast-math", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I" + ROCM_INC]
# the corrected form: every triple in the form the launcher picks -- (13,4,0) four bits, (1,0,1) the offset alone, (200,8,1) eight
FORMS = [(t, bqf.mulbits(t)) for t in bqf.TRIPLES]
assert [m for _, m in FORMS] == [4, 0, 8]


@pytest.fixture(scope="module")
def emu():
    """One shared object per code, the stale ones rebuilt in parallel (fully unrolled 64-lane code, five forms: about a minute each)."""
    libs = bitslice_emu_build.build("bitslice_quantised_emu.cpp", ("decode_ms_bitslice.hpp", "codes.hpp", "decode_ms_bs_plan.hpp", "decode_ms_tuning.hpp", "llr_quantise.hpp"), TM, F32_FLAGS)
    loaded = {}
    for name, L in libs.items():
        L.bsq_emu_decode.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_size_t, ctypes.c_uint32, ctypes.c_float, ctypes.c_float] + \
                                    [ctypes.c_uint32] * 3 + [ctypes.c_int]
        L.bsq_emu_decode_i8.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_size_t, ctypes.c_uint32]
        L.bsq_emu_quantise.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_float, ctypes.c_float]
        L.bsq_emu_quantise.restype = None
        L.bsq_emu_mulbits.argtypes = [ctypes.c_uint32] * 2
        assert L.bsq_emu_code() == oracle.CODES.index(name)
        loaded[name] = L
    return loaded


def batches_of(g):
    return sorted({b for b in (g - 1, g, g + 1, 3 * g + 1) if b >= 1})      # a partial group and its padding lanes, whole groups


def run(L, code, x, cap, lim, triple, mulbits):
    """the emulated decode of frames x, each result with a guard row behind it"""
    B = len(x)
    out = np.full((B + 1, oracle.output_len(code)), 0xEE, np.uint8)
    it, ok = np.full(B + 1, 0xEEEEEEEE, np.uint32), np.full(B + 1, 0xEE, np.uint8)
    st = L.bsq_emu_decode(x.ctypes.data, out.ctypes.data, it.ctypes.data, ok.ctypes.data, B, cap, bqf.SCALE, float(lim), *triple, mulbits)
    assert st == 0, f"the kernel text left its LDS layout, the batch's rows or an alignment ({st})"
    assert (out[B] == 0xEE).all() and it[B] == 0xEEEEEEEE and ok[B] == 0xEE, "a result row behind the batch was written"
    return out[:B], it[:B], ok[:B]


def differing(got, want, B):
    (out, it, ok), (wo, wi, wk) = got, (a[:B] for a in want)
    return np.nonzero((out != wo).any(axis=1) | (it != wi) | (ok != wk))[0]


@pytest.mark.parametrize("name", TM)
def test_the_g_plus_plus_build_compiles_the_librarys_quantiser(emu, name):
    """ldpc::quantise_llr as the emulator's build compiled it equals the restatement on the frames and on the corner vector"""
    L = emu[name]
    for lim in bqf.LIMS:
        for x in (bqf.frames(name).reshape(-1), quantise_restatement.edge_vector(bqf.SCALE, lim), bqf.corners()):
            x = np.ascontiguousarray(x, np.float32)
            q = np.full(len(x), 0x5E, np.int8)
            L.bsq_emu_quantise(x.ctypes.data, q.ctypes.data, len(x), bqf.SCALE, float(lim))
            assert (q == quantise_restatement.quantise(x, np.int8, bqf.SCALE, lim)).all()


@pytest.mark.parametrize("name", TM)
def test_emulated_plain_form_equals_the_oracle_on_the_quantised_frames(emu, name):
    code, L = oracle.CODES.index(name), emu[name]
    g = L.bsq_emu_group()
    assert g == bqf.GROUP[name]
    bqf.assert_conditions(name)
    llrs = bqf.frames(name)
    for lim in bqf.LIMS:
        for cap in bqf.CAPS:
            want = bqf.expected_plain(name, lim, cap)
            for B in batches_of(g):
                got = run(L, code, np.ascontiguousarray(llrs[:B]), cap, lim, bqf.IDENTITY, -1)
                bad = differing(got, want, B)
                assert bad.size == 0, f"{name} lim {lim} cap {cap} batch {B}: frames {bad.tolist()[:8]} differ"


@pytest.mark.parametrize("name", TM)
def test_emulated_corrected_form_equals_the_statement_on_the_quantised_frames(emu, name):
    code, L = oracle.CODES.index(name), emu[name]
    g = L.bsq_emu_group()
    llrs = bqf.frames(name)
    for triple, mulbits in FORMS:
        assert L.bsq_emu_mulbits(triple[0], triple[1]) == mulbits
        want = bqf.expected_corrected(name, triple)
        for cap in bqf.CAPS:
            for B in batches_of(g):
                got = run(L, code, np.ascontiguousarray(llrs[:B]), cap, 127, triple, mulbits)
                bad = differing(got, want[cap], B)
                assert bad.size == 0, f"{name} {triple}/{mulbits} cap {cap} batch {B}: frames {bad.tolist()[:8]} differ"
    # a triple that does not fit the form it is asked in is refused by the emulator itself, not run
    assert L.bsq_emu_decode(None, None, None, None, 0, 1, 8.0, 127.0, 13, 4, 0, 0) == 2


@pytest.mark.parametrize("name", TM)
def test_the_identity_triple_in_the_corrected_form_equals_the_plain_form(emu, name):
    """every spelling of the identity is the offset-only form's (correction_mulbits: scale_num << (8 - scale_shift) == 256)"""
    code, L = oracle.CODES.index(name), emu[name]
    B = 3 * L.bsq_emu_group() + 1
    x = np.ascontiguousarray(bqf.frames(name)[:B])
    for cap in (3, 25):
        plain = run(L, code, x, cap, 127, bqf.IDENTITY, -1)
        for triple in ((1, 0, 0), (16, 4, 0), (256, 8, 0)):
            assert L.bsq_emu_mulbits(triple[0], triple[1]) == 0
            got = run(L, code, x, cap, 127, triple, 0)
            assert differing(got, plain, B).size == 0, (name, cap, triple)


@pytest.mark.parametrize("name", TM)
def test_the_i8_source_decoder_of_the_edited_header_still_equals_the_oracle(emu, name):
    code, L = oracle.CODES.index(name), emu[name]
    g = L.bsq_emu_group()
    for lim in bqf.LIMS:
        q = bqf.quantised(name, lim)
        for cap in (0, 3, 25):
            want = bqf.expected_plain(name, lim, cap)
            for B in batches_of(g):
                x = np.ascontiguousarray(q[:B])
                out = np.full((B + 1, oracle.output_len(code)), 0xEE, np.uint8)
                it, ok = np.full(B + 1, 0xEEEEEEEE, np.uint32), np.full(B + 1, 0xEE, np.uint8)
                assert L.bsq_emu_decode_i8(x.ctypes.data, out.ctypes.data, it.ctypes.data, ok.ctypes.data, B, cap) == 0
                assert differing((out[:B], it[:B], ok[:B]), want, B).size == 0, (name, lim, cap, B)
                assert (out[B] == 0xEE).all() and it[B] == 0xEEEEEEEE and ok[B] == 0xEE
