"""layered_restatement.py -- a CPU restatement of the block-row LAYERED min-sum schedule for f32 LLRs.

TEST INFRASTRUCTURE ONLY: imported by tests/ and tools/, never by the product.

The schedule, as the library's layered kernels implement it (csrc/decode_ms_layered.hpp):

    u[e] = v[e] = 0 for every edge
    for it in 0 .. max_iters:
        for every layer, in order:
            va[j] = llr[j] (0 for punctured j), then += u[e] for the edges e of j in edge order
            for e = (c, j) in the layer:  nv = va[j] - u[e];  v[e] = nv if hard(nv) == hard(v[e]) or v[e] == 0 else 0
            for every check c of the layer: min1, min2 (capped at FLT_MAX) and the sign product of its v
            for e = (c, j) in the layer: u[e] = (min2 if |v[e]| == min1[c] else min1[c]), negated by the sign product,
                                         negated again if v[e] < 0
        va = llr + sum of u, as above
        if every check's parity over hard(va) is 0: output = hard(va), iters = it, success = 1; stop
    output = hard(va) of the last sweep, iters = max_iters, success = 0

hard(x) is x < 0.  LLRs are read as the library's f32 kernels read them: -0.0 as +0.0, NaN as +inf.  The soft output is `va` of the
returned sweep with -0.0 as +0.0 and a NaN exactly at each NaN LLR; all zero for max_iters = 0.

Two statements of it:
  * decode_layered(): whole-array numpy over [frames, edges], in the style of oracle/ms_numpy.py (marginals by occurrence rank,
    minima by sorting a padded per-check array);
  * decode_layered_loop(): one frame, one edge at a time, with the reference's strict-`<` two-minimum update -- for the small codes.
The layers are an input: block_layers() gives the block rows; one_layer() puts every edge in a single layer, and then sweep i is the
reference's iteration i + 1 (tests/test_layered_host.py ties it to the oracle that way).
"""
from __future__ import annotations

import numpy as np

import oracle

FMAX = np.float32(np.finfo(np.float32).max)


def submatrix_size(code) -> int:
    return int(oracle.L.oracle_code_submatrix_size(int(code)))


def block_layers(code, chk: np.ndarray) -> list:
    """Edge index arrays of the block rows of the prototype, in order (edges are row-major: each is a contiguous run)."""
    row = np.asarray(chk, dtype=np.int64) // submatrix_size(code)
    return [np.nonzero(row == r)[0] for r in range(int(row.max()) + 1)]


def one_layer(chk: np.ndarray) -> list:
    return [np.arange(len(chk))]


class Structure:
    """Index tables of a code and a layer list (whole-array form)."""

    def __init__(self, code, layers=None):
        chk, var = oracle.edges(code)
        self.chk = np.asarray(chk, dtype=np.int64)
        self.var = np.asarray(var, dtype=np.int64)
        self.E = len(self.chk)
        self.n = oracle.n(code)
        self.V = self.n + oracle.p(code)
        self.C = int(self.chk.max()) + 1
        self.layers = block_layers(code, self.chk) if layers is None else layers
        seen = np.zeros(self.V, dtype=np.int64)
        rank = np.empty(self.E, dtype=np.int64)
        for e in range(self.E):
            rank[e] = seen[self.var[e]]
            seen[self.var[e]] += 1
        self.rank_groups = [np.nonzero(rank == r)[0] for r in range(int(rank.max()) + 1)]
        deg = np.bincount(self.chk, minlength=self.C)
        self.maxdeg = int(deg.max())
        self.by_check = np.full((self.C, self.maxdeg), self.E, dtype=np.int64)      # pad -> dummy edge E
        fill = np.zeros(self.C, dtype=np.int64)
        for e in range(self.E):
            c = self.chk[e]
            self.by_check[c, fill[c]] = e
            fill[c] += 1
        # per layer: its checks' padded edge rows, and each layer edge's row / column in that table
        self.layer_tabs = []
        for le in self.layers:
            checks = np.unique(self.chk[le])
            tab = self.by_check[checks]
            pos = {c: i for i, c in enumerate(checks)}
            row_of_edge = np.array([pos[c] for c in self.chk[le]], dtype=np.int64)
            assert np.isin(tab[tab < self.E], le).all(), "a layer must hold every edge of its checks"
            self.layer_tabs.append((tab, row_of_edge))


def canonical_llrs(llrs: np.ndarray) -> np.ndarray:
    L = np.ascontiguousarray(llrs, dtype=np.float32) + np.float32(0.0)        # -0.0 -> +0.0
    return np.where(np.isnan(L), np.float32(np.inf), L).astype(np.float32)


def _soft(va: np.ndarray, raw: np.ndarray, n: int) -> np.ndarray:
    out = (va + np.float32(0.0)).astype(np.float32)
    nan = np.isnan(raw)
    out[:, :n][nan] = raw[nan]
    return out


def decode_layered(st: Structure, llrs: np.ndarray, maxiters: int):
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
    for it in range(maxiters):
        Li = L[live]
        for le, (tab, row_of_edge) in zip(st.layers, st.layer_tabs):
            va = marginals(u, Li)
            nv = va[:, st.var[le]] - u[:, le]
            old = v[:, le]
            keep = ((nv < 0) == (old < 0)) | (old == 0)
            v[:, le] = np.where(keep, nv, np.float32(0.0))
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
            app[fr] = _soft(va[fin], raw[fr], n)
            stay = ~fin
            live, u, v = live[stay], u[stay], v[stay]
        if len(live) == 0:
            break
    return output, iters, success, app


def decode_layered_loop(code, llr: np.ndarray, maxiters: int, layers=None):
    """One frame, edge by edge, straight from the definition.  Returns (output u8[V/8], iters, success, app f32[V])."""
    chk, var = oracle.edges(code)
    chk = [int(c) for c in chk]
    var = [int(j) for j in var]
    E, n = len(chk), oracle.n(code)
    V = n + oracle.p(code)
    if layers is None:
        layers = block_layers(code, np.asarray(chk))
    f32 = np.float32
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
                x = min2[c] if abs(v[e]) == min1[c] else min1[c]
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
