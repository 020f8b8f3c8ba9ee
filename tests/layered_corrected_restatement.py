"""layered_corrected_restatement.py -- a CPU restatement of the layered min-sum schedule with NORMALIZED / OFFSET check messages
(labrador_ldpc_decode_ms_layered_corrected_{,soft_}batch_f32).

TEST INFRASTRUCTURE ONLY: imported by tests/ and tools/, never by the product.

The schedule is that of tests/layered_restatement.py with one step added.  Where a layer forms an edge's new check
message, the magnitude m = (min2[c] if |v[e]| == min1[c] else min1[c]), already capped at FLT_MAX, becomes

    t  = scale * m          one f32 multiply, rounded
    t  = t - offset         one f32 subtract, rounded (never fused with the multiply)
    m' = t if t > 0 else +0.0

and the signs are applied to m' as they are to m, a zero m' included.  Which of min1 / min2 an edge takes is decided on the uncorrected
|v|; everything else (self-correction, accumulation order, LLR canonicalisation, the stop rule, iters, success, output, app,
max_iters = 0) is the layered schedule unchanged.  With (scale, offset) = (1, 0) the step is the identity on every m the decoder forms
(finite, non-negative, never -0.0), so the results are then those of layered_restatement.decode_layered bit for bit.

Two statements, as there: decode_layered_corrected() over whole arrays and decode_layered_corrected_loop() one frame, edge by edge.
Both do the step in np.float32 with the two roundings written out.
"""
from __future__ import annotations

import numpy as np

import oracle
from layered_restatement import Structure, block_layers, canonical_llrs

FMAX = np.float32(np.finfo(np.float32).max)
ZERO = np.float32(0.0)


def correct(m, scale, offset):
    """The added step on an f32 array (or scalar) of message magnitudes."""
    m = np.asarray(m, dtype=np.float32)
    t = np.multiply(np.float32(scale), m, dtype=np.float32)          # rounded to f32
    t = np.subtract(t, np.float32(offset), dtype=np.float32)         # rounded to f32
    return np.where(t > 0, t, ZERO).astype(np.float32)


def _soft(va: np.ndarray, raw: np.ndarray, n: int) -> np.ndarray:
    out = (va + ZERO).astype(np.float32)                             # -0.0 -> +0.0
    nan = np.isnan(raw)
    out[:, :n][nan] = raw[nan]
    return out


def decode_layered_corrected(st: Structure, llrs: np.ndarray, maxiters: int, scale, offset):
    """llrs [frames, n] f32 -> (output [frames, V/8] u8, iters [frames] u32, success [frames] u8, app [frames, V] f32)."""
    raw = np.ascontiguousarray(llrs, dtype=np.float32)
    F = raw.shape[0]
    E, V, n = st.E, st.V, st.n
    output = np.zeros((F, V // 8), dtype=np.uint8)
    iters = np.full(F, maxiters, dtype=np.uint32)
    success = np.zeros(F, dtype=np.uint8)
    app = np.zeros((F, V), dtype=np.float32)
    if maxiters == 0 or F == 0:
        iters[:] = 0
        return output, iters, success, app
    L = canonical_llrs(raw)
    u = np.zeros((F, E + 1), dtype=np.float32)                 # column E: the pad edge (never written)
    v = np.zeros((F, E + 1), dtype=np.float32)
    live = np.arange(F)

    def marginals(ui, Li):
        va = np.zeros((len(Li), V), dtype=np.float32)
        va[:, :n] = Li
        for grp in st.rank_groups:
            va[:, st.var[grp]] = va[:, st.var[grp]] + ui[:, grp]
        return va

    va = None
    with np.errstate(all="ignore"):
        for it in range(maxiters):
            Li = L[live]
            for le, (tab, row_of_edge) in zip(st.layers, st.layer_tabs):
                va = marginals(u, Li)
                nv = va[:, st.var[le]] - u[:, le]
                old = v[:, le]
                keep = ((nv < 0) == (old < 0)) | (old == 0)
                v[:, le] = np.where(keep, nv, ZERO)
                a = np.abs(v)
                a[:, E] = np.inf
                at = np.sort(a[:, tab], axis=2)                    # [f, checks of the layer, maxdeg]
                min1 = np.minimum(at[:, :, 0], FMAX)
                min2 = np.minimum(at[:, :, 1], FMAX)
                neg = v < 0
                neg[:, E] = False
                sgn = np.logical_xor.reduce(neg[:, tab], axis=2)
                ve = v[:, le]
                m1, m2 = min1[:, row_of_edge], min2[:, row_of_edge]
                ue = correct(np.where(np.abs(ve) == m1, m2, m1), scale, offset)      # the added step, on the uncorrected choice
                ue = np.where(sgn[:, row_of_edge], -ue, ue)
                u[:, le] = np.where(ve < 0, -ue, ue)
            va = marginals(u, Li)
            hard = np.concatenate([va < 0, np.zeros((len(live), 1), dtype=bool)], axis=1)
            par = np.logical_xor.reduce(hard[:, np.where(st.by_check < E, st.var[np.minimum(st.by_check, E - 1)], V)], axis=2)
            done = ~par.any(axis=1)
            last = it + 1 == maxiters
            fin = np.ones(len(live), dtype=bool) if last else done
            if fin.any():
                fr = live[fin]
                output[fr] = np.packbits(va[fin] < 0, axis=1)
                iters[fr] = np.where(done[fin], it, maxiters)
                success[fr] = done[fin].astype(np.uint8)
                app[fr] = _soft(va[fin], raw[fr], n)
                stay = ~fin
                live, u, v = live[stay], u[stay], v[stay]
            if len(live) == 0:
                break
    return output, iters, success, app


def decode_layered_corrected_loop(code, llr: np.ndarray, maxiters: int, scale, offset, layers=None):
    """One frame, edge by edge, straight from the definition.  Returns (output u8[V/8], iters, success, app f32[V])."""
    chk, var = oracle.edges(code)
    chk = [int(c) for c in chk]
    var = [int(j) for j in var]
    E, n = len(chk), oracle.n(code)
    V = n + oracle.p(code)
    if layers is None:
        layers = block_layers(code, np.asarray(chk))
    f32 = np.float32
    scale, offset = f32(scale), f32(offset)
    raw = np.asarray(llr, dtype=np.float32)
    if maxiters == 0:
        return np.zeros(V // 8, np.uint8), 0, 0, np.zeros(V, np.float32)
    L = canonical_llrs(raw[None, :])[0]
    u = [f32(0.0)] * E
    v = [f32(0.0)] * E

    def marginals():
        va = [f32(0.0)] * V
        for j in range(n):
            va[j] = L[j]
        for e in range(E):                                     # edge order
            va[var[e]] = f32(va[var[e]] + u[e])
        return va

    va = None
    with np.errstate(all="ignore"):
        for it in range(maxiters):
            for le in layers:
                va = marginals()
                for e in le:
                    nv = f32(va[var[e]] - u[e])
                    if (nv < 0) == (v[e] < 0) or v[e] == 0:
                        v[e] = nv
                    else:
                        v[e] = f32(0.0)
                min1, min2, sgn = {}, {}, {}
                for e in le:
                    c, a = chk[e], f32(abs(v[e]))
                    m1, m2 = min1.get(c, FMAX), min2.get(c, FMAX)
                    if a < m1:
                        m2, m1 = m1, a
                    elif a < m2:
                        m2 = a
                    min1[c], min2[c] = m1, m2
                    sgn[c] = sgn.get(c, False) ^ bool(v[e] < 0)
                for e in le:
                    c = chk[e]
                    m = f32(min2[c] if abs(v[e]) == min1[c] else min1[c])
                    t = f32(scale * m)                             # rounded
                    t = f32(t - offset)                            # rounded
                    x = t if t > 0 else f32(0.0)
                    if sgn[c]:
                        x = -x
                    if v[e] < 0:
                        x = -x
                    u[e] = f32(x)
            va = marginals()
            par = [0] * (max(chk) + 1)
            for e in range(E):
                par[chk[e]] ^= int(va[var[e]] < 0)
            if not any(par):
                return np.packbits(np.array(va) < 0), it, 1, _soft(np.array([va], np.float32), raw[None, :], n)[0]
    return np.packbits(np.array(va) < 0), maxiters, 0, _soft(np.array([va], np.float32), raw[None, :], n)[0]
