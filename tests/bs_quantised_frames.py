"""bs_quantised_frames.py -- the frames of the tests of the bit-sliced kernels' f32 loader (tests/test_bitslice_quantised_emu.py on the
CPU, tests/test_gpu_bs_quantised.py on the GPU) and what they must exercise.  TEST INFRASTRUCTURE ONLY.

Per code 3 G + 1 float32 frames (G = codewords per wave) from a fixed seed: near-threshold AWGN LLRs at 1.9 dB (rate 1/2) or 2.7 dB
(rate 2/3); every third of them salted at random positions with the quantiser's corners at scale 8 -- exact ties +-0.0625 (2 k + 1),
whose products lie at x.5, +-inf, NaN, -0.0, values beyond +-lim / scale, denormals --; a flat all-NaN row and a flat +inf row;
shuffled.

The expected answers come only from tests/quantise_restatement.py followed by the oracle's i8 decode (plain form), by
tests/flooding_fixed_corrected_restatement.py (corrected form) and by tests/cascade_restatement.py's composition of that with the
fixed-point layered restatements (cascade); each is computed once and shared read-only."""
import numpy as np

import flooding_fixed_corrected_restatement as corrected_statement
import oracle
import quantise_restatement

NAMES = ["TM1536", "TM2048", "TM6144", "TM8192"]
GROUP = {"TM1536": 8, "TM2048": 4, "TM6144": 2, "TM8192": 1}
CAPS = (0, 1, 3, 25)
SCALE = 8.0
LIMS = (127, 31)
IDENTITY = (1, 0, 0)
# the corrected form's triples, one per multiplier width the launcher builds: (13,4,0) four bits, (1,0,1) the offset alone, (200,8,1) eight
TRIPLES = ((13, 4, 0), (1, 0, 1), (200, 8, 1))
# the cascade pair of the GPU tests and of tools/bs_quantised_rate.py: stage 1 and stage 2 at (13,4,0)
CASCADE_PAIR = ((13, 4, 0), (13, 4, 0))
# chosen on the CPU so that assert_conditions() holds for every code
SEED = {"TM1536": 9100, "TM2048": 9100, "TM6144": 9100, "TM8192": 9100}


def mulbits(triple):
    """the multiplier bits of the form the launcher picks (bs::correction_mulbits)"""
    num = triple[0] << (8 - triple[1])
    return 0 if num == 256 else 4 if num & 15 == 0 else 8


def corners():
    """float32 values at which a quantiser at scale 8 goes wrong"""
    ties = [np.float32(0.0625) * np.float32(2 * k + 1) for k in range(0, 12)] + [np.float32(0.0625) * np.float32(2 * k + 1) for k in (30, 31, 126, 127)]
    vals = []
    for t in ties:
        vals += [t, -t]
    fmax = np.finfo(np.float32).max
    vals += [np.inf, -np.inf, np.nan, -0.0, 0.0, 16.5, -16.5, 100.0, -100.0, 4.0, -4.0, 3.9375, -3.9375, fmax, -fmax,
             np.float32(1e-45), -np.float32(1e-45), np.float32(1e-39), -np.float32(1e-39)]
    return np.array(vals, np.float32)


_frames, _quantised, _plain, _corrected, _cascade = {}, {}, {}, {}, {}


def build_frames(name, seed):
    code, g = oracle.CODES.index(name), GROUP[name]
    rng = np.random.default_rng(seed + code)
    n = oracle.n(code)
    ebn0 = {2: 1.9, 3: 2.7}[n // (n - oracle.k(code))]                           # rate 1/2, 2/3
    count = 3 * g + 1
    awgn, _ = oracle.awgn_llrs(code, rng, count - 2, ebn0, np.float32)
    salt = corners()
    for r in range(0, len(awgn), 3):
        awgn[r, rng.choice(n, len(salt), replace=False)] = salt
    flat = np.stack([np.full(n, np.nan, np.float32), np.full(n, np.inf, np.float32)])
    x = np.concatenate([awgn, flat])
    x = np.ascontiguousarray(x[rng.permutation(len(x))])
    assert x.shape == (count, n) and x.dtype == np.float32
    x.setflags(write=False)
    return x


def frames(name):
    """[3 G + 1, n] float32, read-only"""
    if name not in _frames:
        _frames[name] = build_frames(name, SEED[name])
    return _frames[name]


def quantised(name, lim, x=None):
    """the frames through tests/quantise_restatement.py at (SCALE, lim): [3 G + 1, n] int8, read-only"""
    if x is not None:
        return quantise_restatement.quantise(x, np.int8, SCALE, lim)
    if (name, lim) not in _quantised:
        q = quantise_restatement.quantise(frames(name), np.int8, SCALE, lim)
        q.setflags(write=False)
        _quantised[(name, lim)] = q
    return _quantised[(name, lim)]


def _frozen(res):
    for a in res:
        a.setflags(write=False)
    return res


def expected_plain(name, lim, cap):
    """(output, iters, success) of the oracle's i8 decode of the quantised frames"""
    if (name, lim, cap) not in _plain:
        _plain[(name, lim, cap)] = _frozen(oracle.decode_ms_batch(oracle.CODES.index(name), quantised(name, lim), cap)[:3])
    return _plain[(name, lim, cap)]


def expected_corrected(name, triple, lim=127):
    """{cap: (output, iters, success)} over CAPS of the corrected statement on the quantised frames"""
    if (name, triple, lim) not in _corrected:
        res = corrected_statement.decode_caps(corrected_statement.structure(oracle.CODES.index(name)), quantised(name, lim), CAPS, *triple)
        for r in res.values():
            _frozen(r)
        _corrected[(name, triple, lim)] = res
    return _corrected[(name, triple, lim)]


def expected_cascade(name, cap, sweeps, flooding, layered, lim=127):
    """(output, iters, success, stage) of the composition: the flooding statement at `flooding`, then the fixed-point layered statement
    at `layered` on the quantised frames the first stage failed"""
    key = (name, cap, sweeps, flooding, layered, lim)
    if key not in _cascade:
        import cascade_restatement                                   # (imports the package: only where the cascade is asked for)
        code = oracle.CODES.index(name)
        if flooding == IDENTITY:
            first = lambda q, c: oracle.decode_ms_batch(code, q, c)                                          # noqa: E731
        else:
            first = lambda q, c: corrected_statement.decode(corrected_statement.structure(code), q, c, *flooding)      # noqa: E731
        _cascade[key] = _frozen(cascade_restatement.compose(first, cascade_restatement.layered(code, layered), quantised(name, lim), cap, sweeps))
    return _cascade[key]


def conditions(name, x=None):
    """the list of what does NOT hold (empty: all is well), from the reference alone at cap 25, (SCALE, 127)"""
    g = GROUP[name]
    x = frames(name) if x is None else x
    missing = []
    q = quantised(name, 127, x)
    _, it, ok = oracle.decode_ms_batch(oracle.CODES.index(name), q, 25)[:3]
    if g > 1:
        mixed = sum(1 for s in range(0, len(ok) - g + 1, g) if 0 < int(ok[s:s + g].sum()) < g)
        if mixed < 2:
            missing.append(f"{mixed} groups of {g} frames mix success and failure")
    if name == "TM8192" and not (((ok == 1) & (it == 0)).any() and ((ok == 1) & (it > 0)).any() and (ok == 0).any()):
        missing.append(f"no frame at iteration 0, one later and one failing: {it.tolist()} {ok.tolist()}")
    with np.errstate(over="ignore", invalid="ignore"):
        p = np.float32(SCALE) * x
        tie = np.isfinite(p) & (np.abs(p) < 127) & (p - np.floor(p) == 0.5)
    for lim in LIMS:
        ql = quantised(name, lim, x)
        if not ((ql == -lim).any() and (ql == lim).any() and (ql[np.isnan(p)] == 0).all() and np.isnan(p).any()):
            missing.append(f"lim {lim}: no value at -lim, +lim or 0 from NaN")
    half_up = np.floor(p[tie] + np.float32(0.5))
    if not (q[tie] != half_up).any():
        missing.append("no tie that rounds to even differently than round-half-up")
    return missing


def assert_conditions(name):
    """What the frames must exercise, from the reference alone, so that a pass cannot hide the frozen-lane path, the masked padding
    lanes or a quantiser corner: for G > 1 at least two groups of G consecutive frames that mix success and failure; on TM8192 a frame
    converging at iteration 0, one converging later and one failing; at least one quantised value at each of -lim, +lim and
    0-from-NaN; at least one tie that rounds to even differently than round-half-up would."""
    missing = conditions(name)
    assert not missing, f"{name}: {missing}"
