"""flooding_fixed_corrected_restatement.py -- a CPU restatement of the reference's flooding min-sum decoder on i8 LLRs with NORMALIZED /
OFFSET check messages in integers (labrador_ldpc_decode_ms_corrected_batch_i8).

TEST INFRASTRUCTURE ONLY: imported by tests/ and tools/, never by the product.

The schedule is decode_ms::<i8> (src/decoder.rs:347-475 with the i8 arithmetic of :42-50) as oracle/ms_numpy.py restates it, with one
step added.  Where an iteration forms an edge's check message (:391-395), the magnitude m = (min2[c] if |v[e]| == min1[c] else
min1[c]) -- the previous iteration's minima, 0 <= m <= 127; zero in iteration 0 -- becomes

    t  = (scale_num * m + ((1 << scale_shift) >> 1)) >> scale_shift        exact; round half up; scale_shift = 0 adds nothing
    m' = max(t - offset, 0)

and the signs are applied to m' as they are to m.  Which of min1 / min2 an edge takes is decided on the uncorrected values;
everything else (the saturating i8 arithmetic with |-128| = 127, self-correction, accumulation order, the stop rule, iters, success,
output, max_iters = 0) is the reference's decoder unchanged.  0 <= scale_shift <= 8, 1 <= scale_num <= 1 << scale_shift,
0 <= offset <= 127: then m' <= m, a zero stays zero, and (1 << k, k, 0) is the identity for every k.

Two statements: decode_caps() / decode() over whole arrays in int64, in the shape of oracle/ms_numpy.py (marginals by occurrence
rank, minima by sorting a padded table), and decode_loop() one frame, edge by edge in Python integers, with the running two-minimum
update of the reference.
"""
from __future__ import annotations

import numpy as np

import oracle

HI, LO = 127, -128


def check_triple(scale_num, scale_shift, offset):
    assert 0 <= scale_shift <= 8 and 1 <= scale_num <= 1 << scale_shift and 0 <= offset <= 127, (scale_num, scale_shift, offset)


def correct(m, scale_num, scale_shift, offset):
    """The added step on an integer array (or scalar) of message magnitudes."""
    t = (np.int64(scale_num) * np.asarray(m, dtype=np.int64) + np.int64((1 << scale_shift) >> 1)) >> np.int64(scale_shift)
    return np.maximum(t - np.int64(offset), 0)


class Structure:
    """Index tables derived once per code from the ordered edge list."""

    def __init__(self, code):
        chk, var = oracle.edges(code)
        self.chk, self.var = np.asarray(chk, dtype=np.int64), np.asarray(var, dtype=np.int64)
        self.E, self.n = len(self.chk), oracle.n(code)
        self.V = self.n + oracle.p(code)
        self.C = int(self.chk.max()) + 1
        seen = np.zeros(self.V, dtype=np.int64)
        rank = np.empty(self.E, dtype=np.int64)
        for e in range(self.E):                                   # occurrence rank of an edge among its variable's, in edge order
            rank[e] = seen[self.var[e]]
            seen[self.var[e]] += 1
        self.rank_groups = [np.nonzero(rank == r)[0] for r in range(int(rank.max()) + 1)]
        deg = np.bincount(self.chk, minlength=self.C)
        self.by_check = np.full((self.C, int(deg.max())), self.E, dtype=np.int64)      # pad entries: the dummy edge slot E
        fill = np.zeros(self.C, dtype=np.int64)
        for e in range(self.E):
            self.by_check[self.chk[e], fill[self.chk[e]]] = e
            fill[self.chk[e]] += 1


_STRUCTURES = {}


def structure(code):
    if code not in _STRUCTURES:
        _STRUCTURES[code] = Structure(code)
    return _STRUCTURES[code]


def decode_caps(st: Structure, llrs: np.ndarray, caps, scale_num, scale_shift, offset):
    """{cap: (output, iters, success)} for every cap of `caps` from ONE run to the largest of them.  The iterations of a decode do not
    depend on its cap: a frame that converges in iteration it < cap has that iteration's results at every such cap, and one that has
    not converged after iteration cap - 1 fails at that cap with that iteration's marginals."""
    check_triple(scale_num, scale_shift, offset)
    raw = np.ascontiguousarray(llrs)
    assert raw.dtype == np.int8
    L = raw.astype(np.int64)
    F = L.shape[0]
    E, C, V, n = st.E, st.C, st.V, st.n
    caps = sorted(set(int(c) for c in caps))
    res = {c: (np.zeros((F, V // 8), np.uint8), np.full(F, c, np.uint32), np.zeros(F, np.uint8)) for c in caps}
    add = lambda a, b: np.clip(a + b, LO, HI)                     # noqa: E731   saturating_add (:47)
    sub = lambda a, b: np.clip(a - b, LO, HI)                     # noqa: E731   saturating_sub (:48)
    mag = lambda a: np.minimum(np.abs(a), HI)                     # noqa: E731   saturating_abs: |-128| = 127 (:46)
    pack = lambda vals: np.packbits((vals < 0).astype(np.uint8), axis=1)     # noqa: E731   MSB first (:459)

    v = np.zeros((F, E), dtype=np.int64)
    min1 = np.zeros((F, C), dtype=np.int64)
    min2 = np.zeros((F, C), dtype=np.int64)
    sgn = np.zeros((F, C), dtype=bool)
    live = np.arange(F)
    pad = np.int64(1 << 40)
    for it in range(caps[-1] if caps else 0):
        if len(live) == 0:
            break
        m1e, m2e = min1[:, st.chk], min2[:, st.chk]
        m = np.where(mag(v) == m1e, m2e, m1e)                     # chosen on the uncorrected state
        u = correct(m, scale_num, scale_shift, offset)            # THE STEP
        u = np.where(sgn[:, st.chk], -u, u)
        u = np.where(v < 0, -u, u)
        va = np.zeros((len(live), V), dtype=np.int64)
        va[:, :n] = L[live]
        for grp in st.rank_groups:
            va[:, st.var[grp]] = add(va[:, st.var[grp]], u[:, grp])
        vae = va[:, st.var]
        nv = sub(vae, u)
        keep = ((nv < 0) == (v < 0)) | (v == 0)
        v = np.where(keep, nv, 0)
        a = np.concatenate([mag(v), np.broadcast_to(pad, (len(live), 1))], axis=1)[:, st.by_check]
        a.sort(axis=2)
        min1 = np.minimum(a[:, :, 0], HI)
        min2 = np.minimum(a[:, :, 1], HI)
        neg_v = np.concatenate([v < 0, np.zeros((len(live), 1), dtype=bool)], axis=1)[:, st.by_check]
        sgn = np.logical_xor.reduce(neg_v, axis=2)
        neg_va = np.concatenate([vae < 0, np.zeros((len(live), 1), dtype=bool)], axis=1)[:, st.by_check]
        parity = np.logical_xor.reduce(neg_va, axis=2)
        done = ~parity.any(axis=1)
        hard = pack(va)
        for c in caps:
            out, its, ok = res[c]
            if it < c:
                fr = live[done]
                out[fr], its[fr], ok[fr] = hard[done], it, 1
            if it == c - 1:                                       # the cap's last iteration: what has not converged fails as it is
                out[live[~done]] = hard[~done]
        stay = ~done
        live, v, min1, min2, sgn = live[stay], v[stay], min1[stay], min2[stay], sgn[stay]
    return res


def decode(st: Structure, llrs, maxiters, scale_num, scale_shift, offset):
    return decode_caps(st, llrs, [maxiters], scale_num, scale_shift, offset)[int(maxiters)]


def decode_loop(st: Structure, llrs_row, maxiters, scale_num, scale_shift, offset):
    """ONE frame, edge by edge in Python integers, in the reference's own loop order with its running two-minimum update (:430-434):
    (output [V/8] u8, iters, success)."""
    check_triple(scale_num, scale_shift, offset)
    E, C, V, n = st.E, st.C, st.V, st.n
    llr = [int(x) for x in llrs_row]
    chk, var = st.chk.tolist(), st.var.tolist()
    sat = lambda x: HI if x > HI else LO if x < LO else x         # noqa: E731
    half = (1 << scale_shift) >> 1
    u, v = [0] * E, [0] * E
    min1, min2, sg = [0] * C, [0] * C, [False] * C
    va = [0] * V
    for it in range(maxiters):
        va = llr + [0] * (V - n)
        for e in range(E):
            c = chk[e]
            av = min(abs(v[e]), HI)
            m = min2[c] if av == min1[c] else min1[c]
            m = max(((scale_num * m + half) >> scale_shift) - offset, 0)
            if sg[c]:
                m = -m
            if v[e] < 0:
                m = -m
            u[e] = m
            va[var[e]] = sat(va[var[e]] + m)
        n1, n2, ns, par = [HI] * C, [HI] * C, [False] * C, [False] * C
        for e in range(E):
            c = chk[e]
            nv = sat(va[var[e]] - u[e])
            if (nv < 0) != (v[e] < 0) and v[e] != 0:
                nv = 0
            v[e] = nv
            av = min(abs(nv), HI)
            if av < n1[c]:
                n1[c], n2[c] = av, n1[c]
            elif av < n2[c]:
                n2[c] = av
            if nv < 0:
                ns[c] = not ns[c]
            if va[var[e]] < 0:
                par[c] = not par[c]
        min1, min2, sg = n1, n2, ns
        if not any(par):
            return np.packbits(np.array([x < 0 for x in va], np.uint8)), it, 1
    return np.packbits(np.array([x < 0 for x in va], np.uint8)), maxiters, 0
