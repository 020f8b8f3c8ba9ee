"""layered_fixed_restatement.py -- a CPU restatement of the FIXED-POINT block-row layered min-sum schedule for i8 and i16 LLRs
(csrc/decode_ms_fixed_layered.hpp).

TEST INFRASTRUCTURE ONLY: imported by tests/ and tools/, never by the product.

T is int8 or int16, T_MAX = 127 or 32767.  The contract:

    llr[j] = clamp(input[j], -T_MAX, T_MAX)                     (only T's minimum changes)
    u[e] = v[e] = 0 for every edge
    for it in 0 .. max_iters:
        for every layer, in order:
            va[j] = llr[j] (0 for punctured j) + sum of u[e] over the edges e of j                exact, in i32
            for e = (c, j) in the layer:  nv = clamp(va[j] - u[e], -T_MAX, T_MAX)
                                          v[e] = nv if hard(nv) == hard(v[e]) or v[e] == 0 else 0
            for every check c of the layer: min1, min2 of |v| (T_MAX where absent) and the sign product of its v
            for e = (c, j) in the layer: u[e] = (min2 if |v[e]| == min1[c] else min1[c]), negated by the sign product,
                                         negated again if v[e] < 0
        va = llr + sum of u
        if every check's parity over hard(va) is 0: output = hard(va), iters = it, success = 1; stop
    output = hard(va) of the last sweep, iters = max_iters, success = 0

hard(x) is x < 0.  |u| <= T_MAX and a variable has at most 6 edges, so |va| <= 7 * T_MAX: no sum overflows int32 and the order of
the sum cannot matter.  The only saturation is the clamp of nv.  The soft output is `va` of the returned sweep as int32; all zero
for max_iters = 0.

Two statements of it:
  * decode_fixed(): whole-array numpy over [frames, edges];
  * decode_fixed_loop(): one frame, one edge at a time, in Python integers, with the strict-`<` two-minimum update.
Both also report, per frame, whether any nv was clamped before the frame's result was returned.  The layers are an input
(layered_restatement.block_layers / one_layer); `sum_order` permutes the order in which a variable's u are summed.
"""
from __future__ import annotations

import numpy as np

import layered_restatement as lr
import oracle

T_MAX = {np.dtype(np.int8): 127, np.dtype(np.int16): 32767}


def tmax_of(llrs) -> int:
    return T_MAX[np.asarray(llrs).dtype]


class Structure(lr.Structure):
    """layered_restatement.Structure; with `sum_order` (a permutation of the edges) a variable's u are summed in that order."""

    def __init__(self, code, layers=None, sum_order=None):
        super().__init__(code, layers)
        if sum_order is not None:
            order = np.asarray(sum_order, dtype=np.int64)
            assert np.array_equal(np.sort(order), np.arange(self.E))
            seen = np.zeros(self.V, dtype=np.int64)
            rank = np.empty(self.E, dtype=np.int64)
            for e in order:
                rank[e] = seen[self.var[e]]
                seen[self.var[e]] += 1
            self.rank_groups = [np.nonzero(rank == r)[0] for r in range(int(rank.max()) + 1)]


def decode_fixed(st: Structure, llrs: np.ndarray, maxiters: int):
    """llrs [frames, n] int8 / int16 -> (output [frames, V/8] u8, iters [frames] u32, success [frames] u8, app [frames, V] i32,
    clamped [frames] bool)."""
    raw = np.ascontiguousarray(llrs)
    tmax = tmax_of(raw)
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
            ue = np.where(np.abs(ve) == m1, m2, m1)
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


def decode_fixed_loop(code, llr: np.ndarray, maxiters: int, layers=None, sum_order=None):
    """One frame, edge by edge, straight from the definition, in Python integers.  Returns (output u8[V/8], iters, success,
    app i32[V], clamped)."""
    chk, var = oracle.edges(code)
    chk = [int(c) for c in chk]
    var = [int(j) for j in var]
    E, n = len(chk), oracle.n(code)
    V = n + oracle.p(code)
    if layers is None:
        layers = lr.block_layers(code, np.asarray(chk))
    order = range(E) if sum_order is None else [int(e) for e in sum_order]
    tmax = tmax_of(llr)
    if maxiters == 0:
        return np.zeros(V // 8, np.uint8), 0, 0, np.zeros(V, np.int32), False
    L = [max(-tmax, min(tmax, int(x))) for x in np.asarray(llr)]
    u = [0] * E
    v = [0] * E
    clamped = False

    def marginals():
        va = L + [0] * (V - n)
        for e in order:
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
                x = min2[c] if abs(v[e]) == min1[c] else min1[c]
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
