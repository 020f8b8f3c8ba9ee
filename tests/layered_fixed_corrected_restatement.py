"""layered_fixed_corrected_restatement.py -- a CPU restatement of the fixed-point layered min-sum schedule with NORMALIZED / OFFSET
check messages in integers (labrador_ldpc_decode_ms_layered_fixed_corrected_{,soft_}batch_{i8,i16}).

TEST INFRASTRUCTURE ONLY: imported by tests/ and tools/, never by the product.

The schedule is that of tests/layered_fixed_restatement.py with one step added.  Where a layer forms an edge's new
check message, the magnitude m = (min2[c] if |v[e]| == min1[c] else min1[c]), 0 <= m <= T_MAX, becomes

    t  = (scale_num * m + ((1 << scale_shift) >> 1)) >> scale_shift        exact; round half up; scale_shift = 0 adds nothing
    m' = max(t - offset, 0)

and the signs are applied to m' as they are to m, a zero m' included.  Which of min1 / min2 an edge takes is decided on the
uncorrected |v|; everything else (the clamp of nv, the self-correction, the exact int32 marginals, the stop rule, iters, success,
output, the int32 app, max_iters = 0) is the fixed-point layered schedule unchanged.  0 <= scale_shift <= 8,
1 <= scale_num <= 1 << scale_shift, 0 <= offset <= T_MAX: then m' <= m, and (1 << k, k, 0) is the identity for every k.

Two statements, as there: decode_fixed_corrected() over whole arrays (int64 for the product) and decode_fixed_corrected_loop() one
frame, edge by edge, in Python integers.  Both also report, per frame, whether any nv was clamped before the result was returned.
"""
from __future__ import annotations

import numpy as np

import layered_restatement as lr
import oracle
from layered_fixed_restatement import Structure, tmax_of


def check_triple(scale_num, scale_shift, offset, tmax):
    assert 0 <= scale_shift <= 8 and 1 <= scale_num <= 1 << scale_shift and 0 <= offset <= tmax, (scale_num, scale_shift, offset)


def correct(m, scale_num, scale_shift, offset):
    """The added step on an integer array of message magnitudes."""
    t = (np.int64(scale_num) * np.asarray(m, dtype=np.int64) + np.int64((1 << scale_shift) >> 1)) >> np.int64(scale_shift)
    return np.maximum(t - np.int64(offset), 0).astype(np.int32)


def decode_fixed_corrected(st: Structure, llrs: np.ndarray, maxiters: int, scale_num: int, scale_shift: int, offset: int):
    """llrs [frames, n] int8 / int16 -> (output [frames, V/8] u8, iters [frames] u32, success [frames] u8, app [frames, V] i32,
    clamped [frames] bool)."""
    raw = np.ascontiguousarray(llrs)
    tmax = tmax_of(raw)
    check_triple(scale_num, scale_shift, offset, tmax)
    F = raw.shape[0]
    E, V, n = st.E, st.V, st.n
    output = np.zeros((F, V // 8), dtype=np.uint8)
    iters = np.full(F, maxiters, dtype=np.uint32)
    success = np.zeros(F, dtype=np.uint8)
    app = np.zeros((F, V), dtype=np.int32)
    clamped = np.zeros(F, dtype=bool)
    if maxiters == 0 or F == 0:
        iters[:] = 0
        return output, iters, success, app, clamped
    L = np.clip(raw.astype(np.int32), -tmax, tmax)
    u = np.zeros((F, E + 1), dtype=np.int32)                   # column E: the pad edge (never written)
    v = np.zeros((F, E + 1), dtype=np.int32)
    cl = np.zeros(F, dtype=bool)
    live = np.arange(F)

    def marginals(ui, Li):
        va = np.zeros((len(Li), V), dtype=np.int32)
        va[:, :n] = Li
        for grp in st.rank_groups:
            va[:, st.var[grp]] += ui[:, grp]
        return va

    for it in range(maxiters):
        Li = L[live]
        for le, (tab, row_of_edge) in zip(st.layers, st.layer_tabs):
            va = marginals(u, Li)
            wide = va[:, st.var[le]] - u[:, le]
            nv = np.clip(wide, -tmax, tmax)
            cl |= (nv != wide).any(axis=1)
            old = v[:, le]
            keep = ((nv < 0) == (old < 0)) | (old == 0)
            v[:, le] = np.where(keep, nv, 0)
            a = np.abs(v)
            a[:, E] = tmax                                     # an absent edge
            at = np.sort(a[:, tab], axis=2)                    # [f, checks of the layer, maxdeg]
            min1, min2 = at[:, :, 0], at[:, :, 1]
            neg = v < 0
            neg[:, E] = False
            sgn = np.logical_xor.reduce(neg[:, tab], axis=2)
            ve = v[:, le]
            m1, m2 = min1[:, row_of_edge], min2[:, row_of_edge]
            ue = correct(np.where(np.abs(ve) == m1, m2, m1), scale_num, scale_shift, offset)      # the added step, on the uncorrected choice
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
            app[fr] = va[fin]
            clamped[fr] = cl[fin]
            stay = ~fin
            live, u, v, cl = live[stay], u[stay], v[stay], cl[stay]
        if len(live) == 0:
            break
    return output, iters, success, app, clamped


def decode_fixed_corrected_loop(code, llr: np.ndarray, maxiters: int, scale_num: int, scale_shift: int, offset: int, layers=None):
    """One frame, edge by edge, straight from the definition, in Python integers.  Returns (output u8[V/8], iters, success,
    app i32[V], clamped)."""
    chk, var = oracle.edges(code)
    chk = [int(c) for c in chk]
    var = [int(j) for j in var]
    E, n = len(chk), oracle.n(code)
    V = n + oracle.p(code)
    if layers is None:
        layers = lr.block_layers(code, np.asarray(chk))
    tmax = tmax_of(llr)
    scale_num, scale_shift, offset = int(scale_num), int(scale_shift), int(offset)
    check_triple(scale_num, scale_shift, offset, tmax)
    if maxiters == 0:
        return np.zeros(V // 8, np.uint8), 0, 0, np.zeros(V, np.int32), False
    L = [max(-tmax, min(tmax, int(x))) for x in np.asarray(llr)]
    u = [0] * E
    v = [0] * E
    clamped = False

    def marginals():
        va = L + [0] * (V - n)
        for e in range(E):
            va[var[e]] += u[e]
        return va

    va = None
    for it in range(maxiters):
        for le in layers:
            va = marginals()
            for e in le:
                e = int(e)
                wide = va[var[e]] - u[e]
                nv = max(-tmax, min(tmax, wide))
                clamped = clamped or nv != wide
                v[e] = nv if (nv < 0) == (v[e] < 0) or v[e] == 0 else 0
            min1, min2, sgn = {}, {}, {}
            for e in le:
                e = int(e)
                c, a = chk[e], abs(v[e])
                m1, m2 = min1.get(c, tmax), min2.get(c, tmax)
                if a < m1:
                    m2, m1 = m1, a
                elif a < m2:
                    m2 = a
                min1[c], min2[c] = m1, m2
                sgn[c] = sgn.get(c, False) ^ (v[e] < 0)
            for e in le:
                e = int(e)
                c = chk[e]
                m = min2[c] if abs(v[e]) == min1[c] else min1[c]
                t = (scale_num * m + ((1 << scale_shift) >> 1)) >> scale_shift
                x = max(t - offset, 0)
                if sgn[c]:
                    x = -x
                if v[e] < 0:
                    x = -x
                u[e] = x
        va = marginals()
        par = [0] * (max(chk) + 1)
        for e in range(E):
            par[chk[e]] ^= int(va[var[e]] < 0)
        if not any(par):
            return np.packbits(np.array(va) < 0), it, 1, np.array(va, np.int32), clamped
    return np.packbits(np.array(va) < 0), maxiters, 0, np.array(va, np.int32), clamped
