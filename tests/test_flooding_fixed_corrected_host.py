"""The statement of normalized / offset min-sum on the i8 flooding schedule (tests/flooding_fixed_corrected_restatement.py; DESIGN.md
4.14), checked on the CPU: at every identity triple it is the oracle's decode_ms::<i8> on all six TM codes, its two forms agree away
from the identity, the step has the properties the contract names, and the frames it saves on TM2048 are pinned."""
import numpy as np
import pytest

import edge_frames
import oracle
import flooding_fixed_corrected_restatement as fr

TM = ["TM1280", "TM1536", "TM2048", "TM5120", "TM6144", "TM8192"]
IDENTITIES = [(1, 0, 0), (2, 1, 0), (256, 8, 0)]
CAPS = (0, 1, 3, 25)


def frames_of(code, rng):
    """near-threshold AWGN frames at the library's default scale, and the corner rows (+-127, -128, 0)"""
    n = oracle.n(code)
    ebn0 = {2: 2.0, 3: 2.8, 5: 3.8}[n // (n - oracle.k(code))]                  # rate 1/2, 2/3, 4/5
    awgn, _ = oracle.awgn_llrs(code, rng, 5, ebn0, np.int8)
    corner = edge_frames.integer_range_rows(code, np.int8, rng, 1)
    flat = np.stack([np.zeros(n, np.int8), np.full(n, -128, np.int8), np.full(n, 127, np.int8)])
    return np.concatenate([awgn, corner, flat])


@pytest.mark.parametrize("name", TM)
def test_identity_triples_are_the_oracle(name):
    code = oracle.CODES.index(name)
    st = fr.structure(code)
    llrs = frames_of(code, np.random.default_rng(1400 + code))
    want = {cap: oracle.decode_ms_batch(code, llrs, cap)[:3] for cap in CAPS}
    assert len(set(want[25][1].tolist())) > 2                       # frames that converge early, late and never
    for triple in IDENTITIES:
        got = fr.decode_caps(st, llrs, CAPS, *triple)
        for cap in CAPS:
            for g, w, what in zip(got[cap], want[cap], ("output", "iters", "success")):
                assert np.array_equal(g, w), (name, triple, cap, what)


@pytest.mark.parametrize("name", ["TM1280", "TM2048"])
def test_the_two_forms_agree_away_from_the_identity(name):
    code = oracle.CODES.index(name)
    st = fr.structure(code)
    llrs = frames_of(code, np.random.default_rng(1500 + code))[[0, 1, 5, 7, 9]]
    for triple in ((13, 4, 0), (1, 0, 1), (3, 2, 1), (1, 1, 0)):
        for cap in (0, 1, 6):
            out, it, ok = fr.decode(st, llrs, cap, *triple)
            for f in range(len(llrs)):
                lo, li, lk = fr.decode_loop(st, llrs[f], cap, *triple)
                assert np.array_equal(lo, out[f]) and li == it[f] and lk == ok[f], (name, triple, cap, f)


def test_the_step():
    m = np.arange(128)
    for shift in range(9):
        for num in range(1, (1 << shift) + 1):
            for off in (0, 1, 2, 63, 127):
                c = fr.correct(m, num, shift, off)
                assert c[0] == 0 and (c <= m).all() and (np.diff(c) >= 0).all()       # zero stays zero, never larger, monotone
        assert np.array_equal(fr.correct(m, 1 << shift, shift, 0), m)                 # the identity at every shift
    assert fr.correct(1, 1, 1, 0) == 1 and fr.correct(3, 1, 1, 0) == 2                # ties round half up
    assert not fr.correct(m, 1, 8, 0).any()                                           # 127 / 256 rounds to zero
    for bad in ((0, 0, 0), (2, 0, 0), (1, 9, 0), (1, 0, 128)):
        with pytest.raises(AssertionError):
            fr.check_triple(*bad)


# frames of 600 that flooding min-sum fails at cap 25, TM2048, oracle.awgn_llrs quantised at scale 8: plain, (13, 4, 0), (1, 0, 1)
SAVED = {1.7: (168, 112, 82), 2.0: (19, 6, 6)}


@pytest.mark.parametrize("ebn0", [1.7, 2.0])
def test_frames_saved_on_tm2048(ebn0):
    code = oracle.CODES.index("TM2048")
    st = fr.structure(code)
    llrs, _ = oracle.awgn_llrs(code, np.random.default_rng(4140 + int(round(10 * ebn0))), 600, ebn0, np.int8)
    failed = [int(600 - fr.decode(st, llrs, 25, *t)[2].sum()) for t in ((1, 0, 0), (13, 4, 0), (1, 0, 1))]
    print(f"TM2048 {ebn0} dB: failed of 600 at plain / (13,4,0) / (1,0,1): {failed}")
    assert failed[0] == int(600 - oracle.decode_ms_batch(code, llrs, 25)[2].sum())
    assert tuple(failed) == SAVED[ebn0]


def test_the_harness_refuses_the_flooding_triple_anywhere_else():
    """--fixed-flooding-scale / --fixed-flooding-offset: --llr i8 on the flooding schedule and the cascade; a ValueError anywhere else,
    raised before any device work."""
    from labrador_ldpc_amd import perftest
    common = ["--code", "TM1280", "--snrs", "4.0", "--noise", "ebn0", "--max-bits", "1e5"]
    for rest in (["--fixed-flooding-scale", "13/16"],                                                   # f32
                 ["--llr", "i16", "--schedule", "cascade", "--fixed-flooding-offset", "1"],
                 ["--llr", "i8", "--schedule", "layered", "--fixed-flooding-scale", "13/16"],
                 ["--llr", "f16", "--schedule", "cascade", "--fixed-flooding-offset", "1"],
                 ["--llr", "i8", "--schedule", "flooding", "--fixed-flooding-scale", "13/16", "--fixed-scale", "13/16"]):
        with pytest.raises(ValueError):
            perftest.main(common + rest)
    with pytest.raises(SystemExit):                                                                     # (not a power of two)
        perftest.main(common + ["--llr", "i8", "--fixed-flooding-scale", "13/15"])
    with pytest.raises(SystemExit):                                                                     # the non-cascade quantised entry has none
        perftest.main(common + ["--llr", "i8", "--schedule", "flooding", "--from-f32", "--fixed-flooding-scale", "13/16"])
