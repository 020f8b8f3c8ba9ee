"""Every (form, code, width) of the bit-sliced i8 decoders still reaches the kernel that decodes it, on the GPU: the six files of
csrc/decode_ms_bs*.hip share one launch path (csrc/decode_ms_bs_launch.hpp: the lockstep launch, the code switch, the width switch, the
bridge between the two compile units), and a call that took a wrong turn in it -- another code's kernel, another width, another
form -- decodes to something else or not at all.

Per one-wave code (TM1536, TM2048, TM6144, TM8192) at batch 1 and G + 1, per triple -- the identity (width 0), an offset without a
scale (width 0), (13, 4, 0) (width 4), (205, 8, 0) (width 8) --: the i8 hard, the i8 soft, the f32-reading hard and the f32-reading
soft entry give the same output, iters and success, the two soft ones the same marginals, and the i8 hard results are those of
tests/flooding_fixed_corrected_restatement.py.  At the identity the four PLAIN entries (no triple: the kernels without the correction
step) give these results as well.  The two-wave codes (TM1280, TM5120) have the hard i8 forms only.

Frames: float32 BPSK + AWGN observations (oracle.awgn_llrs), quantised ONCE by the library's own entry (quantise_llrs_batch, scale 8,
lim 127) for the i8 entries and the restatement; the f32-reading entries get the float rows.  Noise level and seed per code (FRAMES) were
chosen on the CPU with the restatement so that at max_iters 10 and at every triple, at least one of the G + 1 frames converges and at
least one runs to the cap -- both ways out of the kernels' iteration loop; the test asserts that mixture."""
import functools

import numpy as np
import pytest

import flooding_fixed_corrected_restatement as fr
import labrador_ldpc_amd as la
import oracle
from labrador_ldpc_amd import LDPCCode

pytestmark = pytest.mark.gpu

CAP = 10
SCALE, LIM = 8.0, 127
BS = 64                                                       # `variant` of the plain bit-sliced kernels in decode_ms_batch
IDENTITY = (1, 0, 0)
TRIPLES = [IDENTITY, (1, 0, 1), (13, 4, 0), (205, 8, 0)]      # multiplier bits 0, 0, 4, 8 (ldpc::bs::correction_mulbits)
# code -> (G, Eb/N0 in dB, seed of numpy's default_rng): see the docstring
FRAMES = {"TM1536": (8, 3.0, 7004), "TM2048": (4, 2.5, 7305), "TM6144": (2, 3.4, 7107), "TM8192": (1, 3.1, 7708),
          "TM1280": (16, 3.5, 7003), "TM5120": (4, 4.0, 7006)}
ONE_WAVE = ["TM1536", "TM2048", "TM6144", "TM8192"]
TWO_WAVES = ["TM1280", "TM5120"]


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if la.device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("the bit-sliced launch-path GPU tests need a gfx950 device")
    torch.cuda.set_device(0)


@functools.lru_cache(maxsize=None)
def frames(name):
    """(float rows, their int8 quantisation by the library, {triple: the restatement's (output, iters, success)}) of the code's G + 1
    frames; computed once and shared"""
    code = LDPCCode[name]
    g, ebn0, seed = FRAMES[name]
    y, _ = oracle.awgn_llrs(int(code), np.random.default_rng(seed), g + 1, ebn0, np.float32)
    q = np.asarray(code.quantise_llrs_batch(y, "i8", SCALE, LIM))
    st = fr.structure(int(code))
    want = {t: fr.decode(st, q, CAP, *t) for t in TRIPLES}
    for a in (y, q) + tuple(x for w in want.values() for x in w):
        a.setflags(write=False)
    return y, q, want


def kw_of(triple):
    return {"scale_num": triple[0], "scale_shift": triple[1], "offset": triple[2]}


def same(tag, got, want, names=("output", "iters", "success")):
    assert len(got) == len(want) == len(names), (tag, len(got), len(want))
    for g, w, what in zip(got, want, names):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (tag, what, g.shape, w.shape)
        bad = np.flatnonzero((g.reshape(len(w), -1).astype(np.int64) != w.reshape(len(w), -1).astype(np.int64)).any(axis=1))
        assert bad.size == 0, f"{tag}: {what} differs in frames {bad.tolist()[:8]}"


def assert_mixture(name, want):
    for triple, (_, iters, ok) in want.items():
        assert ok.any() and not ok.all(), (name, triple, ok.tolist())
        assert (iters[ok == 0] == CAP).all() and (iters[ok == 1] < CAP).all(), (name, triple, iters.tolist())


@pytest.mark.parametrize("name", ONE_WAVE)
def test_the_four_entries_agree_and_equal_the_statement(name):
    code = LDPCCode[name]
    y, q, want = frames(name)
    assert_mixture(name, want)
    for b in (1, FRAMES[name][0] + 1):
        for triple in TRIPLES:
            tag = f"{name} {triple} batch {b}"
            ref = tuple(x[:b] for x in want[triple])
            hard = code.decode_ms_corrected_fixed_batch(q[:b], *triple, maxiters=CAP)
            soft = code.decode_ms_bitsliced_soft_batch(q[:b], CAP, **kw_of(triple))
            hard_f32 = code.decode_ms_quantised_batch(y[:b], "i8", SCALE, LIM, CAP, bitsliced=True, **kw_of(triple))
            soft_f32 = code.decode_ms_bitsliced_quantised_soft_batch(y[:b], SCALE, LIM, CAP, **kw_of(triple))
            same(tag + ": i8 hard against the statement", hard, ref)
            same(tag + ": i8 soft", soft[1:], hard)
            same(tag + ": f32-reading hard", hard_f32, hard)
            same(tag + ": f32-reading soft", soft_f32[1:], hard)
            same(tag + ": the two soft entries' marginals", soft_f32[:1], soft[:1], ("app",))
            if triple == IDENTITY:                            # ... and the forms without the correction step
                plain_soft = code.decode_ms_bitsliced_soft_batch(q[:b], CAP)
                plain_soft_f32 = code.decode_ms_bitsliced_quantised_soft_batch(y[:b], SCALE, LIM, CAP)
                same(tag + ": plain i8 hard", code.decode_ms_batch(q[:b], CAP, variant=BS), hard)
                same(tag + ": plain i8 soft", plain_soft[1:], hard)
                same(tag + ": plain f32-reading hard", code.decode_ms_quantised_batch(y[:b], "i8", SCALE, LIM, CAP, bitsliced=True), hard)
                same(tag + ": plain f32-reading soft", plain_soft_f32[1:], hard)
                same(tag + ": the plain soft entries' marginals", plain_soft_f32[:1] + plain_soft[:1], soft[:1] * 2, ("app", "app"))


@pytest.mark.parametrize("name", TWO_WAVES)
def test_the_two_wave_hard_entries_equal_the_statement(name):
    code = LDPCCode[name]
    _, q, want = frames(name)
    assert_mixture(name, want)
    for b in (1, FRAMES[name][0] + 1):
        for triple in TRIPLES:
            ref = tuple(x[:b] for x in want[triple])
            same(f"{name} {triple} batch {b}", code.decode_ms_corrected_fixed_batch(q[:b], *triple, maxiters=CAP), ref)
        same(f"{name} plain batch {b}", code.decode_ms_batch(q[:b], CAP, variant=BS), tuple(x[:b] for x in want[IDENTITY]))


ENTRIES = {
    "plain i8 hard": lambda c, q, y, r: c.decode_ms_batch(q, CAP, variant=BS, **r),
    "i8 hard": lambda c, q, y, r: c.decode_ms_corrected_fixed_batch(q, 13, 4, 0, maxiters=CAP, **r),
    "plain i8 soft": lambda c, q, y, r: c.decode_ms_bitsliced_soft_batch(q, CAP, **r),
    "i8 soft": lambda c, q, y, r: c.decode_ms_bitsliced_soft_batch(q, CAP, scale_num=13, scale_shift=4, offset=0, **r),
    "plain f32-reading hard": lambda c, q, y, r: c.decode_ms_quantised_batch(y, "i8", SCALE, LIM, CAP, bitsliced=True, **r),
    "f32-reading hard": lambda c, q, y, r: c.decode_ms_quantised_batch(y, "i8", SCALE, LIM, CAP, bitsliced=True, scale_num=13, scale_shift=4,
                                                                       offset=0, **r),
    "plain f32-reading soft": lambda c, q, y, r: c.decode_ms_bitsliced_quantised_soft_batch(y, SCALE, LIM, CAP, **r),
    "f32-reading soft": lambda c, q, y, r: c.decode_ms_bitsliced_quantised_soft_batch(y, SCALE, LIM, CAP, scale_num=13, scale_shift=4, offset=0,
                                                                                      **r),
}


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_an_empty_batch_succeeds_and_writes_nothing(entry):
    """batch 0 through every entry, on device buffers: the result buffers are the empty heads of filled ones, which stay as they were"""
    import torch
    code = LDPCCode.TM2048
    fill = {"app": (torch.int8, 0x5E, (code.n() + code.punctured_bits(),)), "output": (torch.uint8, 0xEE, (code.output_len(),)),
            "iters": (torch.int32, -2, ()), "success": (torch.uint8, 0xEE, ())}
    if "soft" not in entry:
        del fill["app"]
    whole = {k: torch.full((2,) + shape, v, dtype=dt, device="cuda") for k, (dt, v, shape) in fill.items()}
    q = torch.zeros((2, code.n()), dtype=torch.int8, device="cuda")[:0]
    y = torch.zeros((2, code.n()), dtype=torch.float32, device="cuda")[:0]
    got = ENTRIES[entry](code, q, y, {k: t[:0] for k, t in whole.items()})
    torch.cuda.synchronize()
    assert len(got) == len(whole) and all(len(g) == 0 for g in got)
    for k, (_, v, _) in fill.items():
        assert bool((whole[k] == v).all()), (entry, k)
