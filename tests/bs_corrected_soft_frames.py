"""bs_corrected_soft_frames.py -- what the tests of the corrected bit-sliced soft decoder share (tests/test_bitslice_corrected_soft_host.py
and tests/test_bitslice_corrected_soft_emu.py on the CPU, tests/test_gpu_bs_corrected_soft.py on the GPU).  TEST INFRASTRUCTURE ONLY.

The frames are those of bs_soft_frames.py (3 G + 1 per code).  The answers come from flooding_fixed_corrected_soft_restatement.py, one run
per (code, triple) to the largest cap, computed once and shared read-only."""

import bs_soft_frames as bsf
import flooding_fixed_corrected_soft_restatement as statement
import oracle

NAMES, GROUP, CAPS = bsf.NAMES, bsf.GROUP, bsf.CAPS
frames = bsf.frames

IDENTITY = (1, 0, 0)
# (13,4,0): a four-bit multiplier; (1,0,1): the offset alone; (3,2,1): both; (255,8,0): eight bits, and m -> m for every m <= 127;
# (209,8,1): eight bits, no identity
TRIPLES = (IDENTITY, (13, 4, 0), (1, 0, 1), (3, 2, 1), (255, 8, 0), (209, 8, 1))
CONDITION_TRIPLES = ((13, 4, 0), (1, 0, 1))       # the two whose frames are asserted to mix success and failure inside groups


def mulbits(triple):
    """the multiplier bits of the form the launcher picks (bs::correction_mulbits)"""
    num = triple[0] << (8 - triple[1])
    return 0 if num == 256 else 4 if num & 15 == 0 else 8


_expected = {}


def expected(name, triple):
    """{cap: (output, iters, success, va)} over CAPS, read-only"""
    if (name, triple) not in _expected:
        res = statement.decode_caps(statement.structure(oracle.CODES.index(name)), frames(name), CAPS, *triple)
        for r in res.values():
            for a in r:
                a.setflags(write=False)
        _expected[(name, triple)] = res
    return _expected[(name, triple)]


def assert_conditions(name):
    """What the frames must exercise under the CORRECTED statement alone, at cap 25: at (13,4,0) and at (1,0,1) at least two groups of G
    consecutive frames that hold both a converged and a failed frame (G > 1), on TM8192 a frame converging at iteration 0, one
    converging later and one failing; marginals that reach -128 and 127; and at least two frames whose marginals differ from the
    plain decoder's, so that a kernel that ignores the triple fails."""
    g = GROUP[name]
    plain_va = bsf.expected(name, 25)[3]
    for triple in CONDITION_TRIPLES:
        _, it, ok, va = expected(name, triple)[25]
        if g > 1:
            mixed = sum(1 for s in range(0, len(ok) - g + 1, g) if 0 < int(ok[s:s + g].sum()) < g)
            assert mixed >= 2, f"{name} {triple}: {mixed} groups of {g} frames mix success and failure"
        else:
            assert ((ok == 1) & (it == 0)).any() and ((ok == 1) & (it > 0)).any() and (ok == 0).any(), (triple, it.tolist(), ok.tolist())
        assert va.min() == -128 and va.max() == 127, f"{name} {triple}: the expected marginals span {va.min()} .. {va.max()}"
        differ = int((va != plain_va).any(axis=1).sum())
        assert differ >= 2, f"{name} {triple}: {differ} frames' marginals differ from the plain decoder's"
