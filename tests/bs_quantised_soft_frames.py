"""bs_quantised_soft_frames.py -- what the tests of the f32-reading bit-sliced SOFT decoders share (tests/test_bitslice_quantised_soft_emu.py
and tests/test_bs_quantised_soft_host.py on the CPU, tests/test_gpu_bs_quantised_soft.py on the GPU).  TEST
INFRASTRUCTURE ONLY.

The frames are those of bs_quantised_frames.py: 3 G + 1 float32 frames per code with the quantiser's corners salted in, chosen so that
groups mix success and failure.  The answers, marginals included, come only from tests/quantise_restatement.py followed by
oracle.decode_ms_soft_batch (plain form), by tests/flooding_fixed_corrected_soft_restatement.py (corrected form) and by
tests/cascade_soft_restatement.py's composition of those with the fixed-point layered soft statements (cascade); each is computed once
and shared read-only.  Every result tuple is in the order the library returns it: the marginals first."""
import numpy as np

import bs_quantised_frames as bqf
import flooding_fixed_corrected_soft_restatement as soft_statement
import oracle

NAMES, GROUP, CAPS, SCALE, LIMS = bqf.NAMES, bqf.GROUP, bqf.CAPS, bqf.SCALE, bqf.LIMS
IDENTITY, TRIPLES, CASCADE_PAIR = bqf.IDENTITY, bqf.TRIPLES, bqf.CASCADE_PAIR
frames, quantised, mulbits, corners = bqf.frames, bqf.quantised, bqf.mulbits, bqf.corners

_plain, _corrected, _cascade = {}, {}, {}


def _frozen(res):
    for a in res:
        a.setflags(write=False)
    return res


def expected_plain(name, lim, cap):
    """(va, output, iters, success) of the oracle's soft i8 decode of the quantised frames"""
    if (name, lim, cap) not in _plain:
        out, it, ok, va = oracle.decode_ms_soft_batch(oracle.CODES.index(name), quantised(name, lim), cap)[:4]
        _plain[(name, lim, cap)] = _frozen((va, out, it, ok))
    return _plain[(name, lim, cap)]


def expected_corrected(name, triple, lim=127):
    """{cap: (va, output, iters, success)} over CAPS of the corrected soft statement on the quantised frames"""
    if (name, triple, lim) not in _corrected:
        res = soft_statement.decode_caps(soft_statement.structure(oracle.CODES.index(name)), quantised(name, lim), CAPS, *triple)
        _corrected[(name, triple, lim)] = {cap: _frozen((va, out, it, ok)) for cap, (out, it, ok, va) in res.items()}
    return _corrected[(name, triple, lim)]


def expected_cascade(name, cap, sweeps, flooding, layered, lim=127):
    """(app int32, output, iters, success, stage) of the composition: the soft flooding statement at `flooding`, then the fixed-point
    layered soft statement at `layered` on the quantised frames the first stage failed"""
    key = (name, cap, sweeps, flooding, layered, lim)
    if key not in _cascade:
        import cascade_restatement                                   # (imports the package: only where the cascade is asked for)
        import cascade_soft_restatement
        code = oracle.CODES.index(name)
        if flooding == IDENTITY:
            first = lambda q, c: oracle.decode_ms_soft_batch(code, q, c)                                     # noqa: E731
        else:
            first = lambda q, c: soft_statement.decode(soft_statement.structure(code), q, c, *flooding)      # noqa: E731
        _cascade[key] = _frozen(cascade_soft_restatement.compose_soft(first, cascade_restatement.layered(code, layered), quantised(name, lim),
                                                                      cap, sweeps))
    return _cascade[key]


def conditions(name):
    """the list of what does NOT hold (empty: all is well), from the references alone at cap 25, (SCALE, 127): bs_quantised_frames.py's
    conditions, and for the plain form and each of TRIPLES marginals that reach both -128 and 127 and at least one failing frame"""
    missing = list(bqf.conditions(name))
    for form in (None,) + tuple(TRIPLES):
        va, _, _, ok = expected_plain(name, 127, 25) if form is None else expected_corrected(name, form)[25]
        if not (va.min() == -128 and va.max() == 127):
            missing.append(f"{form or 'plain'}: the expected marginals span {va.min()} .. {va.max()}")
        if not (ok == 0).any():
            missing.append(f"{form or 'plain'}: no failing frame")
    return missing


def assert_conditions(name):
    """What the frames must exercise so that a pass cannot hide the frozen-lane path, the masked padding lanes, a quantiser corner or
    the saturation of the marginals -- asserted from the references alone."""
    missing = conditions(name)
    assert not missing, f"{name}: {missing}"
