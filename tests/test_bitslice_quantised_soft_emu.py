"""The bit-sliced i8 decoder reading f32 LLRs WITH soft output (labrador_ldpc_amd/csrc/decode_ms_bitslice.hpp,
decode_group<..., SOFT = true, QuantisedF32>) validated WITHOUT a GPU: tests/c/bitslice_quantised_soft_emu.cpp
instantiates the kernels' own source text -- the f32 loader, the iteration, the correction step, the kept planes, store_marginals --
with a backend whose wave register is an array of 64 lanes, whose LDS accessors are bounds-checked against exactly Geo::LDS_BYTES_SOFT of
the shipped placement, whose 16-byte global loads must stay inside the batch's rows, and whose quantiser is the library's own
ldpc::quantise_llr compiled by g++.  This file compares the four results frame by frame with the statements
(tests/bs_quantised_soft_frames.py: quantise_restatement.py, then the oracle's soft decode or
flooding_fixed_corrected_soft_restatement.py) and with the emulated i8-source soft decoder fed the quantised frames; guard rows stand
behind every result array, `app` included.  The GPU tests then only have to show that gfx950 executes the same text the same way
(tests/test_gpu_bs_quantised_soft.py)."""
import ctypes
import os

import numpy as np
import pytest

import bs_quantised_soft_frames as bqs
import bitslice_emu_build
import oracle

TM = bqs.NAMES
ROCM_INC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
# (the library's flags for the one multiply: nothing fused into it; the HIP headers llr_quantise.hpp needs)
F32_FLAGS = ["-fno-fast-math", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I" + ROCM_INC]
# the corrected form: every triple in the form the launcher picks -- (13,4,0) four bits, (1,0,1) the offset alone, (200,8,1) eight
FORMS = [(t, bqs.mulbits(t)) for t in bqs.TRIPLES]
assert [m for _, m in FORMS] == [4, 0, 8]


@pytest.fixture(scope="module")
def emu():
    """One shared object per code, the stale ones rebuilt in parallel (fully unrolled 64-lane code, eight forms: a minute or two each)."""
    libs = bitslice_emu_build.build("bitslice_quantised_soft_emu.cpp", ("decode_ms_bitslice.hpp", "codes.hpp", "decode_ms_bs_plan.hpp", "decode_ms_tuning.hpp", "llr_quantise.hpp"), TM, F32_FLAGS)
    loaded = {}
    for name, L in libs.items():
        L.bsqa_emu_decode.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_size_t, ctypes.c_uint32, ctypes.c_float, ctypes.c_float] + \
                                     [ctypes.c_uint32] * 3 + [ctypes.c_int]
        L.bsqa_emu_decode_i8.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_size_t] + [ctypes.c_uint32] * 4 + [ctypes.c_int]
        L.bsqa_emu_mulbits.argtypes = [ctypes.c_uint32] * 2
        assert L.bsqa_emu_code() == oracle.CODES.index(name)
        loaded[name] = L
    return loaded


def batches_of(g):
    return sorted({b for b in (g - 1, g, g + 1, 3 * g + 1) if b >= 1})      # a partial group and its padding lanes, whole groups


def run(L, code, x, cap, lim, triple, mulbits):
    """the emulated soft decode of frames x -- float32: the f32 loader at (SCALE, lim); int8: the i8 source -- each result with a guard
    row behind it, `app` with one in front as well: (app, output, iters, success)"""
    B = len(x)
    npv = oracle.n(code) + oracle.p(code)
    app = np.full((B + 2, npv), 0x5E, np.int8)[1:]
    out = np.full((B + 1, oracle.output_len(code)), 0xEE, np.uint8)
    it, ok = np.full(B + 1, 0xEEEEEEEE, np.uint32), np.full(B + 1, 0xEE, np.uint8)
    assert app.ctypes.data % 16 == 0 and x.flags.c_contiguous
    if x.dtype == np.float32:
        st = L.bsqa_emu_decode(x.ctypes.data, app.ctypes.data, out.ctypes.data, it.ctypes.data, ok.ctypes.data, B, cap, bqs.SCALE, float(lim),
                               *triple, mulbits)
    else:
        assert x.dtype == np.int8
        st = L.bsqa_emu_decode_i8(x.ctypes.data, app.ctypes.data, out.ctypes.data, it.ctypes.data, ok.ctypes.data, B, cap, *triple, mulbits)
    assert st == 0, f"the kernel text left its LDS layout, the batch's rows or an alignment ({st})"
    assert (app.base[0] == 0x5E).all() and (app[B] == 0x5E).all(), "a row of app outside the batch was written"
    assert (out[B] == 0xEE).all() and it[B] == 0xEEEEEEEE and ok[B] == 0xEE, "a result row behind the batch was written"
    return app[:B], out[:B], it[:B], ok[:B]


def differing(got, want, B):
    (app, out, it, ok), (wa, wo, wi, wk) = got, (a[:B] for a in want)
    return np.nonzero((app != wa).any(axis=1) | (out != wo).any(axis=1) | (it != wi) | (ok != wk))[0]


@pytest.mark.parametrize("name", TM)
def test_emulated_plain_soft_form_equals_the_oracle_on_the_quantised_frames(emu, name):
    code, L = oracle.CODES.index(name), emu[name]
    g = L.bsqa_emu_group()
    assert g == bqs.GROUP[name]
    assert bool(L.bsqa_emu_planes_in_lds()) == (name in ("TM1536", "TM6144"))             # the soft plan's placement
    bqs.assert_conditions(name)
    llrs = bqs.frames(name)
    for lim in bqs.LIMS:
        for cap in bqs.CAPS:
            want = bqs.expected_plain(name, lim, cap)
            for B in batches_of(g):
                got = run(L, code, np.ascontiguousarray(llrs[:B]), cap, lim, bqs.IDENTITY, -1)
                bad = differing(got, want, B)
                assert bad.size == 0, f"{name} lim {lim} cap {cap} batch {B}: frames {bad.tolist()[:8]} differ"
                i8 = run(L, code, np.ascontiguousarray(bqs.quantised(name, lim)[:B]), cap, lim, bqs.IDENTITY, -1)
                assert differing(got, i8, B).size == 0, f"{name} lim {lim} cap {cap} batch {B}: the i8-source soft decoder differs"
        assert not bqs.expected_plain(name, lim, 0)[0].any()                              # (cap 0 was the all-zero marginals)


@pytest.mark.parametrize("name", TM)
def test_emulated_corrected_soft_form_equals_the_statement_on_the_quantised_frames(emu, name):
    code, L = oracle.CODES.index(name), emu[name]
    g = L.bsqa_emu_group()
    llrs = bqs.frames(name)
    for triple, mulbits in FORMS:
        assert L.bsqa_emu_mulbits(triple[0], triple[1]) == mulbits
        for lim in bqs.LIMS:
            want = bqs.expected_corrected(name, triple, lim)
            for cap in bqs.CAPS:
                for B in batches_of(g):
                    got = run(L, code, np.ascontiguousarray(llrs[:B]), cap, lim, triple, mulbits)
                    bad = differing(got, want[cap], B)
                    assert bad.size == 0, f"{name} {triple}/{mulbits} lim {lim} cap {cap} batch {B}: frames {bad.tolist()[:8]} differ"
                    i8 = run(L, code, np.ascontiguousarray(bqs.quantised(name, lim)[:B]), cap, lim, triple, mulbits)
                    assert differing(got, i8, B).size == 0, f"{name} {triple} lim {lim} cap {cap} batch {B}: the i8-source soft decoder differs"
    # a triple that does not fit the form it is asked in is refused by the emulator itself, not run
    assert L.bsqa_emu_decode(None, None, None, None, None, 0, 1, 8.0, 127.0, 13, 4, 0, 0) == 2


@pytest.mark.parametrize("name", TM)
def test_the_identity_triple_in_the_corrected_soft_form_equals_the_plain_soft_form(emu, name):
    """every spelling of the identity is the offset-only form's, and its four results are the plain kernel's"""
    code, L = oracle.CODES.index(name), emu[name]
    B = 3 * L.bsqa_emu_group() + 1
    x = np.ascontiguousarray(bqs.frames(name)[:B])
    for cap in (3, 25):
        plain = run(L, code, x, cap, 127, bqs.IDENTITY, -1)
        for triple in ((1, 0, 0), (16, 4, 0), (256, 8, 0)):
            assert L.bsqa_emu_mulbits(triple[0], triple[1]) == 0
            got = run(L, code, x, cap, 127, triple, 0)
            assert differing(got, plain, B).size == 0, (name, cap, triple)
