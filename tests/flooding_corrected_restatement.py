"""flooding_corrected_restatement.py -- a CPU restatement of the reference's flooding min-sum decoder on f32 LLRs with NORMALIZED /
OFFSET check messages (labrador_ldpc_decode_ms_corrected_{,soft_}batch_f32).

TEST INFRASTRUCTURE ONLY: imported by tests/ and tools/, never by the product.

The schedule is decode_ms::<f32> (src/decoder.rs:347-475) as oracle/ms_numpy.py restates it, with one step added.  Where an iteration
forms an edge's check message (:391-395), the magnitude m = (min2[c] if |v[e]| == min1[c] else min1[c]) -- the previous iteration's
minima, capped at FLT_MAX; zero in iteration 0 -- becomes

    t  = scale * m          one f32 multiply, rounded
    t  = t - offset         one f32 subtract, rounded (never fused with the multiply)
    m' = t if t > 0 else +0.0

and the signs are applied to m' as they are to m.  Which of min1 / min2 an edge takes is decided on the uncorrected values; everything
else (self-correction, accumulation order, the stop rule, iters, success, output, the marginals, max_iters = 0, NaN LLRs) is the
reference's decoder unchanged.  With (scale, offset) = (1, 0) the step is the identity on every m the decoder forms (finite,
non-negative, never -0.0), so the results are then the oracle's.

Two statements: decode_flooding_corrected() over whole arrays, in the shape of oracle/ms_numpy.py (marginals by occurrence rank,
minima by sorting a padded table; decode_flooding_corrected_caps() gives several caps from one run), and
decode_flooding_corrected_loop() one frame, edge by edge, with the running two-minimum update of the reference.  Both do the step in
np.float32 with the two roundings written out.
"""
from __future__ import annotations

import numpy as np

import oracle

FMAX = np.float32(np.finfo(np.float32).max)
ZERO = np.float32(0.0)


def correct(m, scale, offset):
    """The added step on an f32 array (or scalar) of message magnitudes."""
    m = np.asarray(m, dtype=np.float32)
    t = np.multiply(np.float32(scale), m, dtype=np.float32)          # rounded to f32
    t = np.subtract(t, np.float32(offset), dtype=np.float32)         # rounded to f32
    return np.where(t > 0, t, ZERO).astype(np.float32)


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


def decode_flooding_corrected_caps(st: Structure, llrs: np.ndarray, caps, scale, offset):
    """{cap: (output, iters, success, va)} for every cap of `caps` from ONE run to the largest of them.  The iterations of a decode do
    not depend on its cap: a frame that converges in iteration it < cap has that iteration's results at every such cap, and one that
    has not converged after iteration cap - 1 fails at that cap with that iteration's marginals."""
    L = np.ascontiguousarray(llrs, dtype=np.float32)
    F = L.shape[0]
    E, C, V, n = st.E, st.C, st.V, st.n
    caps = sorted(set(int(c) for c in caps))
    res = {c: (np.zeros((F, V // 8), np.uint8), np.full(F, c, np.uint32), np.zeros(F, np.uint8), np.zeros((F, V), np.float32)) for c in caps}
    v = np.zeros((F, E), dtype=np.float32)                            # the whole working area starts at zero (:374)
    min1 = np.zeros((F, C), dtype=np.float32)
    min2 = np.zeros((F, C), dtype=np.float32)
    sgn = np.zeros((F, C), dtype=bool)
    live = np.arange(F)
    pad_inf = np.float32(np.inf)
    with np.errstate(all="ignore"):
        for it in range(caps[-1]):
            if len(live) == 0:
                break
            m1e, m2e = min1[:, st.chk], min2[:, st.chk]
            u = correct(np.where(np.abs(v) == m1e, m2e, m1e), scale, offset)      # the added step, on the uncorrected choice
            u = np.where(sgn[:, st.chk], -u, u)
            u = np.where(v < 0, -u, u).astype(np.float32)
            va = np.zeros((len(live), V), dtype=np.float32)
            va[:, :n] = L[live]
            for grp in st.rank_groups:
                va[:, st.var[grp]] = va[:, st.var[grp]] + u[:, grp]
            vae = va[:, st.var]
            nv = vae - u
            keep = ((nv < 0) == (v < 0)) | (v == 0)
            v = np.where(keep, nv, ZERO).astype(np.float32)
            am = np.abs(v)
            am = np.where(np.isnan(am), pad_inf, am)                   # a NaN magnitude never passes the `<` of :430 / :433
            a = np.concatenate([am, np.full((len(live), 1), pad_inf, np.float32)], axis=1)[:, st.by_check]
            a.sort(axis=2)
            min1 = np.minimum(a[:, :, 0], FMAX).astype(np.float32)
            min2 = np.minimum(a[:, :, 1], FMAX).astype(np.float32)
            pad_f = np.zeros((len(live), 1), dtype=bool)
            sgn = np.logical_xor.reduce(np.concatenate([v < 0, pad_f], axis=1)[:, st.by_check], axis=2)
            parity = np.logical_xor.reduce(np.concatenate([vae < 0, pad_f], axis=1)[:, st.by_check], axis=2)
            done = ~parity.any(axis=1)                                # all checks satisfied (:453)
            hard = np.packbits(va < 0, axis=1)                        # strictly negative (:76), MSB first (:459)
            for c in caps:
                if c <= it:
                    continue
                sel = done if c > it + 1 else np.ones(len(live), dtype=bool)       # cap it + 1: the last iteration, converged or not
                fr = live[sel]
                output, iters, success, va_out = res[c]
                output[fr], va_out[fr] = hard[sel], va[sel]
                iters[fr] = np.where(done[sel], it, c)
                success[fr] = done[sel]
            stay = ~done
            live, v, min1, min2, sgn = live[stay], v[stay], min1[stay], min2[stay], sgn[stay]
    return res


def decode_flooding_corrected(st: Structure, llrs: np.ndarray, maxiters: int, scale, offset):
    """llrs [frames, n] f32 -> (output [frames, V/8] u8, iters [frames] u32, success [frames] u8, va [frames, V] f32): the marginals
    of the converging iteration, of the last one on failure, all zero for maxiters 0 -- as the reference leaves them (:377)."""
    return decode_flooding_corrected_caps(st, llrs, (maxiters,), scale, offset)[int(maxiters)]


def decode_flooding_corrected_loop(code, llr: np.ndarray, maxiters: int, scale, offset):
    """One frame, edge by edge, in the reference's own loop order.  Returns (output u8[V/8], iters, success, va f32[V])."""
    chk, var = oracle.edges(code)
    chk = [int(c) for c in chk]
    var = [int(j) for j in var]
    E, n = len(chk), oracle.n(code)
    V, C = n + oracle.p(code), max(chk) + 1
    f32 = np.float32
    scale, offset = f32(scale), f32(offset)
    L = np.asarray(llr, dtype=np.float32)
    v = [f32(0.0)] * E
    min1, min2, sgn = [f32(0.0)] * C, [f32(0.0)] * C, [False] * C
    va = [f32(0.0)] * V
    with np.errstate(all="ignore"):
        for it in range(maxiters):
            u = [f32(0.0)] * E
            va = [f32(0.0)] * V
            for j in range(n):
                va[j] = L[j]
            for e in range(E):                                        # :387-411
                c = chk[e]
                m = min2[c] if f32(abs(v[e])) == min1[c] else min1[c]
                t = f32(scale * m)                                    # rounded
                t = f32(t - offset)                                   # rounded
                x = t if t > 0 else f32(0.0)
                if sgn[c]:
                    x = -x
                if v[e] < 0:
                    x = -x
                u[e] = f32(x)
                va[var[e]] = f32(va[var[e]] + u[e])
            min1, min2, sgn = [FMAX] * C, [FMAX] * C, [False] * C     # :414-415
            par = [False] * C
            for e in range(E):                                        # :418-450
                c = chk[e]
                nv = f32(va[var[e]] - u[e])
                if (nv < 0) == (v[e] < 0) or v[e] == 0:
                    v[e] = nv
                else:
                    v[e] = f32(0.0)
                a = f32(abs(v[e]))
                if a < min1[c]:
                    min2[c], min1[c] = min1[c], a
                elif a < min2[c]:
                    min2[c] = a
                if v[e] < 0:
                    sgn[c] = not sgn[c]
                if va[var[e]] < 0:
                    par[c] = not par[c]
            if not any(par):
                return np.packbits(np.array(va, np.float32) < 0), it, 1, np.array(va, np.float32)
    return np.packbits(np.array(va, np.float32) < 0), maxiters, 0, np.array(va, np.float32)
