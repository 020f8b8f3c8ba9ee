"""The bit-sliced i8 decoder with soft output (labrador_ldpc_amd/csrc/decode_ms_bitslice.hpp, Decoder<..., SOFT = true>)
validated WITHOUT a GPU: tests/c/bitslice_soft_emu.cpp instantiates the kernels' own source text -- iteration, kept planes, epilogue --
with a backend whose wave register is an array of 64 lanes and whose LDS accessors are bounds-checked against the soft layout's size,
and this file compares the marginals and the hard results with the oracle frame by frame.  Both placements of the kept planes are
emulated for every code: the plan's (what the library ships) and the other one (what tools/bs_soft_rate.py measures against it).  The
GPU tests then only have to show that gfx950 executes the same text the same way (tests/test_gpu_bs_soft.py)."""
import ctypes

import numpy as np
import pytest

import bs_soft_frames as bsf
import bitslice_emu_build
import oracle

TM = bsf.NAMES
CAPS = bsf.CAPS
PLACEMENTS = ("plan", "other")


def other_placement_flags(name):
    """the -D switches that build the placement the plan did NOT choose (csrc/decode_ms_tuning.hpp: rate 1/2 ships registers, rate 2/3 LDS)"""
    rate12 = name in ("TM2048", "TM8192")
    return ["-DLDPC_TUNING_OVERRIDES_ALLOWED", "-DBS_SOFT_LDS_R12=1" if rate12 else "-DBS_SOFT_LDS_R23=0"]


@pytest.fixture(scope="module")
def emu():
    """One shared object per code and placement, the stale ones rebuilt in parallel (fully unrolled 64-lane code: ~1/2 minute each)."""
    libs = bitslice_emu_build.build("bitslice_soft_emu.cpp", ("decode_ms_bitslice.hpp", "decode_ms_bitslice_split.hpp", "codes.hpp", "decode_ms_bs_plan.hpp", "decode_ms_tuning.hpp"), TM,
                                    variants={"plan": lambda name: [], "other": other_placement_flags})
    loaded = {}
    for (name, placement), L in libs.items():
        L.bsa_emu_decode.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_size_t, ctypes.c_uint32]
        L.bsa_emu_decode_plain.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_size_t, ctypes.c_uint32]
        assert L.bsa_emu_code() == oracle.CODES.index(name)
        loaded[(oracle.CODES.index(name), placement)] = L
    return loaded


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("name", TM)
def test_emulated_soft_decoder_equals_the_oracle(emu, name, placement):
    code = oracle.CODES.index(name)
    L = emu[(code, placement)]
    g = L.bsa_emu_group()
    assert bool(L.bsa_emu_planes_in_lds()) == ((name in ("TM1536", "TM6144")) == (placement == "plan"))
    assert L.bsa_emu_lds_bytes() > L.bsa_emu_plain_lds_bytes() if L.bsa_emu_planes_in_lds() else L.bsa_emu_lds_bytes() == L.bsa_emu_plain_lds_bytes()
    assert g == bsf.GROUP[name]
    llrs, want = bsf.frames(name), {cap: bsf.expected(name, cap) for cap in CAPS}
    bsf.assert_conditions(name)
    npv = oracle.n(code) + oracle.p(code)
    batches = sorted({b for b in (g - 1, g, g + 1, 3 * g + 1) if b >= 1})        # a partial group and its padding lanes, whole groups
    for cap in CAPS:
        for B in batches:
            x = np.ascontiguousarray(llrs[:B])
            app = np.full((B + 1, npv), 0x5E, np.int8)                                 # (a guard row behind each result)
            out = np.full((B + 1, oracle.output_len(code)), 0xEE, np.uint8)
            it, ok = np.full(B + 1, 0xEEEEEEEE, np.uint32), np.full(B + 1, 0xEE, np.uint8)
            assert app.ctypes.data % 16 == 0
            assert L.bsa_emu_decode(x.ctypes.data, app.ctypes.data, out.ctypes.data, it.ctypes.data, ok.ctypes.data, B, cap) == 0, \
                f"{name} cap {cap} batch {B}: the kernel text left its LDS layout or broke an alignment"
            wo, wi, wk, wa = (a[:B] for a in want[cap])
            bad = np.nonzero((out[:B] != wo).any(axis=1) | (it[:B] != wi) | (ok[:B] != wk) | (app[:B] != wa).any(axis=1))[0]
            assert bad.size == 0, f"{name} {placement} cap {cap} batch {B}: frames {bad.tolist()[:8]} differ"
            assert (app[B] == 0x5E).all() and (out[B] == 0xEE).all() and it[B] == 0xEEEEEEEE and ok[B] == 0xEE
    assert not want[0][3].any()                                                      # (cap 0 was the all-zero marginals of decoder.rs:374)


@pytest.mark.parametrize("name", TM)
def test_emulated_plain_decoder_from_the_same_header_still_equals_the_oracle(emu, name):
    """SOFT = false of the edited header: the hard decoder, on the same frames"""
    code = oracle.CODES.index(name)
    L = emu[(code, "plan")]
    g = L.bsa_emu_group()
    llrs = bsf.frames(name)
    for cap in (0, 3, 25):
        wo, wi, wk, _ = oracle.decode_ms_batch(code, llrs, cap)
        for B in sorted({b for b in (g - 1, g + 1, len(llrs)) if b >= 1}):
            x = np.ascontiguousarray(llrs[:B])
            out = np.full((B + 1, oracle.output_len(code)), 0xEE, np.uint8)
            it, ok = np.full(B + 1, 0xEEEEEEEE, np.uint32), np.full(B + 1, 0xEE, np.uint8)
            assert L.bsa_emu_decode_plain(x.ctypes.data, out.ctypes.data, it.ctypes.data, ok.ctypes.data, B, cap) == 0
            assert np.array_equal(out[:B], wo[:B]) and np.array_equal(it[:B], wi[:B]) and np.array_equal(ok[:B], wk[:B]), (name, cap, B)
            assert (out[B] == 0xEE).all() and it[B] == 0xEEEEEEEE and ok[B] == 0xEE
