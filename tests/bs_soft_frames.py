"""bs_soft_frames.py -- the frames of the bit-sliced soft-output tests (tests/test_bitslice_soft_emu.py on the CPU,
tests/test_gpu_bs_soft.py on the GPU) and what they must exercise.  TEST INFRASTRUCTURE ONLY.

Per code 3 G + 1 int8 frames (G = codewords per wave), by the recipe of tests/test_bitslice_corrected_emu.py::frames_of: near-threshold
AWGN at 1.9 dB (rate 1/2) or 2.7 dB (rate 2/3) quantised at scale 8, the integer corner rows of edge_frames.integer_range_rows, the
three flat rows 0 / -128 / 127, shuffled with seed 4200 + code.  The oracle's soft answers are computed once per (code, cap) and shared."""
import numpy as np

import edge_frames
import oracle

NAMES = ["TM1536", "TM2048", "TM6144", "TM8192"]
GROUP = {"TM1536": 8, "TM2048": 4, "TM6144": 2, "TM8192": 1}
CAPS = (0, 1, 3, 25)

_frames, _expected = {}, {}


def frames(name):
    """[3 G + 1, n] int8, read-only"""
    if name not in _frames:
        code, g = oracle.CODES.index(name), GROUP[name]
        rng = np.random.default_rng(4200 + code)
        n = oracle.n(code)
        ebn0 = {2: 1.9, 3: 2.7}[n // (n - oracle.k(code))]                       # rate 1/2, 2/3
        awgn, _ = oracle.awgn_llrs(code, rng, max(3 * g + 1 - 6, 1), ebn0, np.int8)
        corner = edge_frames.integer_range_rows(code, np.int8, rng, 1)
        flat = np.stack([np.zeros(n, np.int8), np.full(n, -128, np.int8), np.full(n, 127, np.int8)])
        x = np.concatenate([awgn, corner, flat])
        x = np.ascontiguousarray(x[rng.permutation(len(x))][: 3 * g + 1] if len(x) >= 3 * g + 1 else x)
        assert len(x) == 3 * g + 1
        x.setflags(write=False)
        _frames[name] = x
    return _frames[name]


def expected(name, cap):
    """oracle.decode_ms_soft_batch on the frames: (output, iters, success, va), read-only"""
    if (name, cap) not in _expected:
        res = oracle.decode_ms_soft_batch(oracle.CODES.index(name), frames(name), cap)
        for a in res:
            a.setflags(write=False)
        _expected[(name, cap)] = res
    return _expected[(name, cap)]


def assert_conditions(name):
    """What the frames must exercise, from the oracle's answer at cap 25, so that a pass cannot hide the frozen-lane or the saturation
    path: at least two groups of G consecutive frames that hold both a converged and a failed frame (G > 1); marginals that reach both
    -128 and 127; on TM8192 (one codeword per wave) a frame converging at iteration 0, one converging later, one failing."""
    g = GROUP[name]
    _, it, ok, va = expected(name, 25)
    if g > 1:
        mixed = sum(1 for s in range(0, len(ok) - g + 1, g) if 0 < int(ok[s:s + g].sum()) < g)
        assert mixed >= 2, f"{name}: {mixed} groups of {g} frames mix success and failure"
    assert va.min() == -128 and va.max() == 127, f"{name}: the expected marginals span {va.min()} .. {va.max()}"
    if name == "TM8192":
        assert ((ok == 1) & (it == 0)).any() and ((ok == 1) & (it > 0)).any() and (ok == 0).any(), (it.tolist(), ok.tolist())
