"""The bit-sliced i8 decoder with normalized / offset check messages AND soft output (labrador_ldpc_amd/csrc/decode_ms_bitslice.hpp,
Decoder<..., CORRECTED = true, MULBITS, SOFT = true>) validated WITHOUT a GPU: tests/c/bitslice_corrected_soft_emu.cpp
instantiates the kernels' own source text -- iteration, correction step, kept planes, epilogue -- with a backend whose wave register is
an array of 64 lanes and whose LDS accessors are bounds-checked against the soft layout's size, and this file compares the marginals
and the hard results with the statement (tests/flooding_fixed_corrected_soft_restatement.py) frame by frame.  One placement of the
kept planes is built -- the soft plan's, for every form -- so one is emulated.  The GPU tests then only have to show that gfx950
executes the same text the same way (tests/test_gpu_bs_corrected_soft.py)."""
import ctypes

import numpy as np
import pytest

import bs_corrected_soft_frames as bcf
import bitslice_emu_build
import oracle

TM = bcf.NAMES
# every triple in the form the launcher picks, and (13,4,0) in the 8-bit form as well
FORMS = [(t, bcf.mulbits(t)) for t in bcf.TRIPLES] + [((13, 4, 0), 8)]


@pytest.fixture(scope="module")
def emu():
    """One shared object per code, the stale ones rebuilt in parallel (fully unrolled 64-lane code, three forms: ~1/2 minute each)."""
    libs = bitslice_emu_build.build("bitslice_corrected_soft_emu.cpp", ("decode_ms_bitslice.hpp", "decode_ms_bitslice_split.hpp", "codes.hpp", "decode_ms_bs_plan.hpp", "decode_ms_tuning.hpp"), TM)
    loaded = {}
    for name, L in libs.items():
        L.bsca_emu_decode.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_size_t] + [ctypes.c_uint32] * 4 + [ctypes.c_int]
        L.bsca_emu_mulbits.argtypes = [ctypes.c_uint32] * 2
        assert L.bsca_emu_code() == oracle.CODES.index(name)
        loaded[name] = L
    return loaded


@pytest.mark.parametrize("name", TM)
def test_emulated_corrected_soft_decoder_equals_the_statement(emu, name):
    code = oracle.CODES.index(name)
    L = emu[name]
    g = L.bsca_emu_group()
    assert g == bcf.GROUP[name]
    assert bool(L.bsca_emu_planes_in_lds()) == (name in ("TM1536", "TM6144"))             # the soft plan's placement
    bcf.assert_conditions(name)
    llrs = bcf.frames(name)
    npv = oracle.n(code) + oracle.p(code)
    batches = sorted({b for b in (g - 1, g, g + 1, 3 * g + 1) if b >= 1})                 # a partial group and its padding lanes, whole groups
    for triple, mulbits in FORMS:
        assert L.bsca_emu_mulbits(triple[0], triple[1]) == bcf.mulbits(triple) <= mulbits
        want = bcf.expected(name, triple)
        for cap in bcf.CAPS:
            for B in batches:
                x = np.ascontiguousarray(llrs[:B])
                app = np.full((B + 2, npv), 0x5E, np.int8)[1:]                            # (a guard row in front of and behind the result)
                out = np.full((B + 1, oracle.output_len(code)), 0xEE, np.uint8)
                it, ok = np.full(B + 1, 0xEEEEEEEE, np.uint32), np.full(B + 1, 0xEE, np.uint8)
                assert app.ctypes.data % 16 == 0
                st = L.bsca_emu_decode(x.ctypes.data, app.ctypes.data, out.ctypes.data, it.ctypes.data, ok.ctypes.data, B, cap, *triple, mulbits)
                assert st == 0, f"{name} {triple}/{mulbits} cap {cap} batch {B}: the kernel text left its LDS layout or broke an alignment ({st})"
                wo, wi, wk, wa = (a[:B] for a in want[cap])
                bad = np.nonzero((out[:B] != wo).any(axis=1) | (it[:B] != wi) | (ok[:B] != wk) | (app[:B] != wa).any(axis=1))[0]
                assert bad.size == 0, f"{name} {triple}/{mulbits} cap {cap} batch {B}: frames {bad.tolist()[:8]} differ"
                assert (app.base[0] == 0x5E).all() and (app[B] == 0x5E).all() and (out[B] == 0xEE).all() and it[B] == 0xEEEEEEEE and ok[B] == 0xEE
        assert not want[0][3].any()                                                       # (cap 0 was the all-zero marginals)
    # a triple that does not fit the form it is asked in is refused by the emulator itself, not run
    assert L.bsca_emu_decode(None, None, None, None, None, 0, 1, 13, 4, 0, 0) == 2 and L.bsca_emu_decode(None, None, None, None, None, 0, 1, 209, 8, 1, 4) == 2
