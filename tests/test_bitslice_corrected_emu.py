"""The bit-sliced i8 decoder with normalized / offset check messages (labrador_ldpc_amd/csrc/decode_ms_bitslice.hpp, Decoder<...,
CORRECTED = true>) validated WITHOUT a GPU: tests/c/bitslice_corrected_emu.cpp instantiates the kernels' own source
text with a backend whose wave register is an array of 64 lanes, and this file compares (a) the plane arithmetic of the step alone
with the formula, exhaustively, and (b) the whole decoder -- the one-wave form of TM1536, TM2048, TM6144 and TM8192 and the two-wave
form of TM1280 and TM5120, each in the form the launcher picks for the triple -- with tests/flooding_fixed_corrected_restatement.py.
The GPU tests then only have to show that gfx950 executes the same text the same way (tests/test_gpu_bs_corrected.py)."""
import ctypes

import numpy as np
import pytest

import edge_frames
import bitslice_emu_build
import oracle
import flooding_fixed_corrected_restatement as fr

TM = ["TM1280", "TM1536", "TM2048", "TM5120", "TM6144", "TM8192"]
TRIPLES = [(1, 0, 0), (13, 4, 0), (1, 0, 1), (3, 2, 1), (1, 1, 0), (255, 8, 0), (1, 8, 0), (16, 4, 127)]
CAPS = (0, 1, 3, 25)
OFFSETS = (0, 1, 2, 63, 127)


@pytest.fixture(scope="module")
def emu():
    """One shared object per code, the stale ones rebuilt in parallel (fully unrolled 64-lane code, three forms: ~1/2 minute each)."""
    libs = bitslice_emu_build.build("bitslice_corrected_emu.cpp", ("decode_ms_bitslice.hpp", "decode_ms_bitslice_split.hpp", "codes.hpp", "decode_ms_bs_plan.hpp", "decode_ms_tuning.hpp"), TM)
    loaded = {}
    for name, L in libs.items():
        L.bsc_emu_decode.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_size_t] + [ctypes.c_uint32] * 4
        L.bsc_emu_correct.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int]
        assert L.bsc_emu_code() == oracle.CODES.index(name)
        assert L.bsc_emu_two_waves() == (name in ("TM1280", "TM5120"))
        loaded[oracle.CODES.index(name)] = L
    return loaded


def test_the_plane_arithmetic_is_the_formula_exhaustively(emu):
    """Every valid (scale_num, scale_shift) -- 511 pairs --, every m in 0 .. 127, offsets {0, 1, 2, 63, 127}: in the form the launcher
    picks for the scale and, where the scale is not 1, in the widest form as well."""
    L = emu[oracle.CODES.index("TM2048")]
    m = np.arange(128, dtype=np.uint8)
    pairs = 0
    for shift in range(9):
        for num in range(1, (1 << shift) + 1):
            pairs += 1
            for off in OFFSETS:
                want = fr.correct(m, num, shift, off).astype(np.uint8)
                for form in (-1,) if num == 1 << shift else (-1, 8):
                    got = np.full(128, 0xEE, np.uint8)
                    assert L.bsc_emu_correct(m.ctypes.data, got.ctypes.data, 128, num, shift, off, form) == 0
                    assert np.array_equal(got, want), (num, shift, off, form)
    assert pairs == 511
    # a form narrower than the scale needs is refused, not computed
    got = np.zeros(128, np.uint8)
    assert L.bsc_emu_correct(m.ctypes.data, got.ctypes.data, 128, 13, 5, 0, 4) == -1
    assert L.bsc_emu_correct(m.ctypes.data, got.ctypes.data, 128, 13, 4, 0, 0) == -1


def frames_of(code, g, rng):
    """3 g + 1 frames: near-threshold AWGN frames quantised at the library's default scale 8, the corner rows among them"""
    n = oracle.n(code)
    ebn0 = {2: 1.9, 3: 2.7, 5: 3.7}[n // (n - oracle.k(code))]                  # rate 1/2, 2/3, 4/5
    awgn, _ = oracle.awgn_llrs(code, rng, max(3 * g + 1 - 6, 1), ebn0, np.int8)
    corner = edge_frames.integer_range_rows(code, np.int8, rng, 1)
    flat = np.stack([np.zeros(n, np.int8), np.full(n, -128, np.int8), np.full(n, 127, np.int8)])
    x = np.concatenate([awgn, corner, flat])
    return x[rng.permutation(len(x))][: 3 * g + 1] if len(x) >= 3 * g + 1 else x


@pytest.mark.parametrize("name", TM)
def test_emulated_corrected_decoder_equals_the_statement(emu, name):
    code = oracle.CODES.index(name)
    L = emu[code]
    g = L.bsc_emu_group()
    st = fr.structure(code)
    llrs = frames_of(code, g, np.random.default_rng(4100 + code))
    assert len(llrs) >= g + 1
    batches = sorted({b for b in (g - 1, g, g + 1, len(llrs)) if b >= 1})        # a partial group and its padding lanes, whole groups
    for triple in TRIPLES:
        want = fr.decode_caps(st, llrs, CAPS, *triple)
        for cap in CAPS:
            for B in batches:
                x = np.ascontiguousarray(llrs[:B])
                out = np.full((B + 1, oracle.output_len(code)), 0xEE, np.uint8)        # (a guard row behind each result)
                it, ok = np.full(B + 1, 0xEEEEEEEE, np.uint32), np.full(B + 1, 0xEE, np.uint8)
                assert L.bsc_emu_decode(x.ctypes.data, out.ctypes.data, it.ctypes.data, ok.ctypes.data, B, cap, *triple) == 0
                wo, wi, wk = (a[:B] for a in want[cap])
                bad = np.nonzero((out[:B] != wo).any(axis=1) | (it[:B] != wi) | (ok[:B] != wk))[0]
                assert bad.size == 0, f"{name} {triple} cap {cap} batch {B}: frames {bad.tolist()[:8]} differ"
                assert (out[B] == 0xEE).all() and it[B] == 0xEEEEEEEE and ok[B] == 0xEE
    # the identity is the plain decoder
    wo, wi, wk, _ = oracle.decode_ms_batch(code, llrs, 25)
    got = fr.decode(st, llrs, 25, 1, 0, 0)
    assert np.array_equal(got[0], wo) and np.array_equal(got[1], wi) and np.array_equal(got[2], wk)
