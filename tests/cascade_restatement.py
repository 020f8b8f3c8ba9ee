"""The contract of the two-stage ("cascade") decode (labrador_ldpc_decode_ms_cascade_batch_{f32,i8,i16}) restated on the
CPU.  It is a composition and nothing else: per frame, the flooding decoder at cap max_iters; where that fails, the layered decoder of
the LLR type at cap max_sweeps on the frame's ORIGINAL LLRs, whose results the frame then carries, success or not.  `stage` says which.

compose() is the composition itself, over any two decoders given as functions of (llrs, cap) -> (output, iters, success): the GPU tests
put the library's own separate entry points into it.  cascade() puts the CPU references into it: oracle.decode_ms_batch (the reference's
flooding decoder) and the four committed layered restatements -- tests/layered_restatement.py and layered_corrected_restatement.py for
f32, layered_fixed_restatement.py and layered_fixed_corrected_restatement.py for i8 / i16; an identity correction, (1, 0) or
(1 << k, k, 0), takes the plain ones, whose results are the same."""
import numpy as np

import layered_corrected_restatement as lcr
import layered_fixed_corrected_restatement as fcr
import layered_fixed_restatement as fr
import layered_helpers
import layered_restatement as lr
import oracle


def compose(first, second, llrs, max_iters, max_sweeps):
    """-> (output, iters u32, success u8, stage u8).  The second decoder sees only the frames the first one failed (frames are
    independent, so that is the same as decoding all of them and picking)."""
    out, it, ok = (np.array(x) for x in first(llrs, max_iters)[:3])
    it, ok = it.astype(np.uint32), ok.astype(np.uint8)
    stage = (ok == 0).astype(np.uint8)
    failed = np.flatnonzero(stage)
    if len(failed):
        o2, i2, s2 = second(llrs[failed], max_sweeps)[:3]
        out[failed], it[failed], ok[failed] = o2, i2, s2
    return out, it, ok, stage


def layered(code, correction=None):
    """The second stage's CPU reference as a function of (llrs, cap), by the LLR type: correction (scale, offset) for float32,
    (scale_num, scale_shift, offset) for int8 / int16; None is plain min-sum."""
    def decode(llrs, cap):
        if llrs.dtype == np.float32:
            st = layered_helpers.structure(code, lr.Structure)
            if correction is None or tuple(correction) == (1.0, 0.0):
                return lr.decode_layered(st, llrs, cap)
            return lcr.decode_layered_corrected(st, llrs, cap, *correction)
        st = layered_helpers.structure(code, fr.Structure)
        if correction is None or (correction[0] == 1 << correction[1] and correction[2] == 0):
            return fr.decode_fixed(st, llrs, cap)
        return fcr.decode_fixed_corrected(st, llrs, cap, *correction)
    return decode


def flooding(code):
    return lambda llrs, cap: oracle.decode_ms_batch(code, llrs, cap)


def cascade(code, llrs, max_iters, max_sweeps, correction=None):
    return compose(flooding(code), layered(code, correction), llrs, max_iters, max_sweeps)
