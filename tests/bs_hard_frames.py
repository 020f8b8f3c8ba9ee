"""bs_hard_frames.py -- the frames of the tests of the bit-sliced kernels' packed hard-decision loader (tests/test_bitslice_hard_emu.py
on the CPU, tests/test_gpu_bs_hard.py on the GPU) and what they must exercise.  TEST INFRASTRUCTURE ONLY.

Per code 3 G + 1 packed frames (G = codewords per wave) from a fixed seed: encoded random data with every bit flipped at a per-frame
probability drawn from four levels -- none, light, near the decoder's threshold on hard input, heavy (0.12) --, an all-zero row and an
all-ones row; shuffled.  Every third frame has an erasure mask that erases a random half of its flipped positions and a few unflipped
ones; the other frames' mask rows are all zero.

The expected answers come only from the numpy expansion of the contract -- e[j] = 0 where the erasure bit is set, else -magnitude where
the input bit is set, else +magnitude -- followed by the oracle's i8 decode (plain form) or by
tests/flooding_fixed_corrected_restatement.py (corrected form); each is computed once and shared read-only."""
import numpy as np

import flooding_fixed_corrected_restatement as corrected_statement
import oracle

NAMES = ["TM1536", "TM2048", "TM6144", "TM8192"]
GROUP = {"TM1536": 8, "TM2048": 4, "TM6144": 2, "TM8192": 1}
CAPS = (0, 1, 3, 25)
MAGNITUDES = (1, 5, 16, 127)
IDENTITY = (1, 0, 0)
# the corrected form's triples, one per multiplier width the launcher builds: (13,4,0) four bits, (1,0,1) the offset alone, (200,8,1) eight
TRIPLES = ((13, 4, 0), (1, 0, 1), (200, 8, 1))
CORRECTED_MAGNITUDE = 16
# flip probabilities: none, light, near the threshold of min-sum on +-1 input at cap 25 (measured on the oracle: the rate-1/2 codes
# decode all of 16 frames at 0.06 and most at 0.07, the rate-2/3 codes all at 0.03 and a few at 0.04), heavy
LEVELS = {"TM1536": (0.0, 0.02, 0.04, 0.12), "TM6144": (0.0, 0.02, 0.04, 0.12), "TM2048": (0.0, 0.03, 0.07, 0.12), "TM8192": (0.0, 0.03, 0.07, 0.12)}
UNFLIPPED_ERASED = 5
# chosen on the CPU so that assert_conditions() holds for every code
SEED = {"TM1536": 4100, "TM2048": 4101, "TM6144": 4112, "TM8192": 4215}


def mulbits(triple):
    """the multiplier bits of the form the launcher picks (bs::correction_mulbits)"""
    num = triple[0] << (8 - triple[1])
    return 0 if num == 256 else 4 if num & 15 == 0 else 8


_frames, _plain, _corrected = {}, {}, {}


def build_frames(name, seed):
    """(input [3 G + 1, n / 8], erasures [3 G + 1, n / 8]) uint8, packed MSB first"""
    code, g = oracle.CODES.index(name), GROUP[name]
    rng = np.random.default_rng(seed + code)
    n, k = oracle.n(code), oracle.k(code)
    count = 3 * g + 1
    rows, flips = [], []
    for _ in range(count - 2):
        cw = np.unpackbits(oracle.copy_encode(code, rng.integers(0, 256, k // 8, dtype=np.uint8)))
        f = (rng.random(n) < LEVELS[name][rng.integers(0, 4)]).astype(np.uint8)
        rows.append(cw ^ f)
        flips.append(f)
    rows += [np.zeros(n, np.uint8), np.ones(n, np.uint8)]
    flips += [np.zeros(n, np.uint8), np.zeros(n, np.uint8)]
    order = rng.permutation(count)
    bits, flips = np.stack(rows)[order], np.stack(flips)[order]
    mask = np.zeros((count, n), np.uint8)
    for r in range(0, count, 3):
        at = np.nonzero(flips[r])[0]
        mask[r, rng.permutation(at)[:(len(at) + 1) // 2]] = 1
        mask[r, rng.choice(np.nonzero(flips[r] == 0)[0], UNFLIPPED_ERASED, replace=False)] = 1
    x, m = np.packbits(bits, axis=1), np.packbits(mask, axis=1)
    assert x.shape == m.shape == (count, n // 8) and x.dtype == m.dtype == np.uint8
    x.setflags(write=False)
    m.setflags(write=False)
    return x, m


def frames(name):
    """(input, erasures): [3 G + 1, n / 8] uint8 each, read-only"""
    if name not in _frames:
        _frames[name] = build_frames(name, SEED[name])
    return _frames[name]


def expand(x, m, magnitude):
    """the contract's i8 frame e of packed rows x under packed mask rows m (None: no mask)"""
    assert 1 <= magnitude <= 127
    bits = np.unpackbits(np.asarray(x), axis=1)
    e = np.where(bits == 1, -magnitude, magnitude).astype(np.int8)
    if m is not None:
        e[np.unpackbits(np.asarray(m), axis=1) == 1] = 0
    return e


def expanded(name, magnitude, masked):
    x, m = frames(name)
    return expand(x, m if masked else None, magnitude)


def _frozen(res):
    for a in res:
        a.setflags(write=False)
    return res


def expected_plain(name, magnitude, masked, cap):
    """(output, iters, success) of the oracle's i8 decode of the expanded frames"""
    key = (name, magnitude, masked, cap)
    if key not in _plain:
        _plain[key] = _frozen(oracle.decode_ms_batch(oracle.CODES.index(name), expanded(name, magnitude, masked), cap)[:3])
    return _plain[key]


def expected_corrected(name, triple, masked, magnitude=CORRECTED_MAGNITUDE):
    """{cap: (output, iters, success)} over CAPS of the corrected statement on the expanded frames"""
    key = (name, triple, masked, magnitude)
    if key not in _corrected:
        res = corrected_statement.decode_caps(corrected_statement.structure(oracle.CODES.index(name)), expanded(name, magnitude, masked), CAPS,
                                              *triple)
        for r in res.values():
            _frozen(r)
        _corrected[key] = res
    return _corrected[key]


def conditions(name, pair=None):
    """the list of what does NOT hold (empty: all is well), from the reference alone at cap 25 and magnitude 1"""
    g, code = GROUP[name], oracle.CODES.index(name)
    x, m = frames(name) if pair is None else pair
    missing = []
    if not (expand(x, None, 1) == np.stack([oracle.hard_to_llrs(code, r, np.int8) for r in x])).all():
        missing.append("the expansion at magnitude 1 without a mask is not hard_to_llrs")
    out, it, ok = oracle.decode_ms_batch(code, expand(x, m, 1), 25)[:3]
    out0, it0, ok0 = oracle.decode_ms_batch(code, expand(x, None, 1), 25)[:3]
    if g > 1:
        mixed = sum(1 for s in range(0, len(ok) - g + 1, g) if 0 < int(ok[s:s + g].sum()) < g)
        if mixed < 2:
            missing.append(f"{mixed} groups of {g} frames mix success and failure")
    if not ((ok == 0).any() and len(set(it[ok == 1].tolist())) >= 2):
        missing.append(f"no failing frame, or fewer than two iteration counts among the successes: {it.tolist()} {ok.tolist()}")
    if not ((ok0 == 0) & (ok == 1)).any():
        missing.append("no frame fails without its mask and succeeds with it")
    big = oracle.decode_ms_batch(code, expand(x, m, 127), 25)[:3]
    if not ((big[0] != out).any(axis=1) | (big[1] != it) | (big[2] != ok)).any():
        missing.append("no frame's results at magnitude 127 differ from magnitude 1")
    return missing


def assert_conditions(name):
    """What the frames must exercise, from the reference alone, so that a pass cannot hide the frozen-lane path, the masked padding
    lanes, the mask or the saturation: for G > 1 at least two groups of G consecutive frames that mix success and failure; a failing
    frame and successes at two or more iteration counts; a frame that fails without its mask and succeeds with it; a frame whose
    results at magnitude 127 differ from those at magnitude 1; and the expansion at magnitude 1 without a mask is hard_to_llrs."""
    missing = conditions(name)
    assert not missing, f"{name}: {missing}"
