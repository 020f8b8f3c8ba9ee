"""The contract of the f32-input forms of the fixed-point layered decoders and of the integer cascade
(labrador_ldpc_decode_ms_layered_quantised_{,soft_}batch_{i8,i16}, labrador_ldpc_decode_ms_cascade_quantised_batch_{i8,i16}; DESIGN.md
4.11) restated on the CPU.  Two compositions of committed restatements and nothing else: the quantiser's rule
(tests/quantise_restatement.py), then the fixed-point layered decoder (tests/layered_fixed_corrected_restatement.py, or
layered_fixed_restatement.py for an identity triple) or the cascade (tests/cascade_restatement.py)."""
import layered_fixed_corrected_restatement as fcr
import layered_fixed_restatement as fr
import layered_helpers
import cascade_restatement
import quantise_restatement as qr


def identity(triple):
    return triple is None or (triple[0] == 1 << triple[1] and triple[2] == 0)


def layered_quantised(code, y, dtype, scale, lim, cap, triple=None):
    """(output, iters, success, app, ...) of the fused layered call: the fixed-point restatement on the quantised frames."""
    st = layered_helpers.structure(code, fr.Structure)
    q = qr.quantise(y, dtype, scale, lim)
    if identity(triple):
        return fr.decode_fixed(st, q, cap)
    return fcr.decode_fixed_corrected(st, q, cap, *triple)


def cascade_quantised(code, y, dtype, scale, lim, max_iters, max_sweeps, triple=None):
    """(output, iters, success, stage) of the fused cascade call: the cascade restatement on the quantised frames."""
    return cascade_restatement.cascade(code, qr.quantise(y, dtype, scale, lim), max_iters, max_sweeps, None if identity(triple) else triple)
