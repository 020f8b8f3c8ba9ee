"""The contract of the soft two-stage ("cascade") decode (labrador_ldpc_decode_ms_cascade_soft_batch_{f32,i8,i16})
restated on the CPU.  TEST INFRASTRUCTURE ONLY: never imported by the product.  It is tests/cascade_restatement.py with the marginals:
per frame, the soft flooding decoder at cap max_iters; where that fails, the soft layered decoder of the LLR type at cap max_sweeps on
the frame's ORIGINAL LLRs, whose results -- marginals included -- the frame then carries, success or not.

compose_soft() is the composition itself, over any two decoders given as functions of (llrs, cap) -> (output, iters, success, app):
the GPU tests put the library's own separate soft entry points into it.  cascade_soft() puts the CPU references into it:
oracle.decode_ms_soft_batch (the reference's flooding decoder and the marginals it leaves) or, for a stage-1 pair,
tests/flooding_corrected_restatement.py; and the four committed layered restatements with their `app`.

The marginals of float32 are float32.  Those of int8 / int16 are int32: a stage-0 row is the flooding decoder's saturating marginal of
the LLR type, astype(np.int32); a stage-1 row the fixed-point layered decoder's exact sum.  same_soft() compares float marginals as
values: NaN equals NaN, and -0.0 equals +0.0."""
import numpy as np

import cascade_restatement as cr
import flooding_corrected_restatement as fcr
import layered_helpers
import oracle


def compose_soft(first, second, llrs, max_iters, max_sweeps):
    """-> (app, output, iters u32, success u8, stage u8).  first / second return (output, iters, success, app, ...); the second sees
    only the frames the first one failed (frames are independent)."""
    out, it, ok, app = (np.array(x) for x in first(llrs, max_iters)[:4])
    it, ok = it.astype(np.uint32), ok.astype(np.uint8)
    if llrs.dtype != np.float32:
        app = app.astype(np.int32)
    stage = (ok == 0).astype(np.uint8)
    failed = np.flatnonzero(stage)
    if len(failed):
        o2, i2, s2, a2 = second(llrs[failed], max_sweeps)[:4]
        out[failed], it[failed], ok[failed], app[failed] = o2, i2, s2, a2
    return app, out, it, ok, stage


def flooding_soft(code, flooding=None):
    """The first stage's CPU reference as a function of (llrs, cap) -> (output, iters, success, app); `flooding`: the stage-1 pair
    (float32 only), None or (1, 0) the reference's decoder itself."""
    def decode(llrs, cap):
        if flooding is None or tuple(flooding) == (1.0, 0.0):
            return oracle.decode_ms_soft_batch(code, llrs, cap)
        assert llrs.dtype == np.float32
        return fcr.decode_flooding_corrected(layered_helpers.structure(code, fcr.Structure), llrs, cap, *flooding)
    return decode


def cascade_soft(code, llrs, max_iters, max_sweeps, correction=None, flooding=None):
    """The CPU statement: (app, output, iters, success, stage).  cascade_restatement.layered()'s decoders return their `app` fourth."""
    return compose_soft(flooding_soft(code, flooding), cr.layered(code, correction), llrs, max_iters, max_sweeps)


def same_soft(got, want, what=""):
    """All five arrays equal; float marginals as values (NaN == NaN, -0.0 == +0.0), integer ones exactly."""
    assert len(got) == len(want) == 5
    for name, g, w in zip(("app", "output", "iters", "success", "stage"), got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        if name == "app":
            assert g.dtype == w.dtype, (what, g.dtype, w.dtype)
        if g.dtype.kind == "f":
            diff = ~((g == w) | (np.isnan(g) & np.isnan(w)))
        else:
            diff = g.astype(np.int64) != w.astype(np.int64)
        bad = np.flatnonzero(diff.reshape(len(g), -1).any(axis=1))
        assert not len(bad), f"{what}: {name} differs in frames {bad[:8].tolist()} ({len(bad)} of {len(g)})"


# ---- the frames of the GPU tests (tests/test_gpu_cascade_soft.py), fixed here and checked on the CPU (tests/test_cascade_soft_host.py) --
# code name -> (seed, clean frames, their Eb/N0, frames at `ebn0`, frames of noise alone, ebn0).  `ebn0` is a few tenths of a dB under the
# code's working point, as tests/test_gpu_cascade.py picks it; the clean frames' is one at which three flooding iterations decode most
# of them (the larger TM codes need 10 dB for that: their punctured variables take an iteration or two whatever the noise).  So a cap
# of 3 decodes clean frames only and a cap of 25 some of the middle ones.  The counts leave a partial last codeword group (no multiple
# of 16) and, but for TM8192, more than 64 failed frames.
FRAMES = {"TC128": (4151, 40, 7.0, 90, 21, 3.5), "TM1280": (4152, 40, 7.0, 90, 21, 3.5), "TM2048": (4153, 40, 10.0, 90, 21, 2.0),
          "TM8192": (4154, 12, 10.0, 21, 8, 1.9)}
CAPS = ((3, 20), (25, 25))
_FRAMES = {}


def frames(code, dtype):
    """The read-only batch of (code, dtype): float32 as drawn, int8 / int16 quantised at 8 / 31."""
    key = (int(code), np.dtype(dtype))
    if key not in _FRAMES:
        seed, clean, clean_db, middle, noise, ebn0 = FRAMES[code.name]
        rng = np.random.default_rng(seed)
        y = np.concatenate([oracle.awgn_llrs(code, rng, clean, clean_db, np.float32)[0], oracle.awgn_llrs(code, rng, middle, ebn0, np.float32)[0],
                            rng.standard_normal((noise, code.n())).astype(np.float32)])
        y = y[np.random.default_rng(seed + 1).permutation(len(y))]
        y = np.ascontiguousarray(y if key[1] == np.float32 else layered_helpers.quantise(y, dtype, 8, 31))
        y.setflags(write=False)
        _FRAMES[key] = y
    return _FRAMES[key]
