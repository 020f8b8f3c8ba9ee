"""flooding_fixed_corrected_soft_restatement.py -- flooding_fixed_corrected_restatement.py with the marginals kept: a CPU restatement of
labrador_ldpc_decode_ms_bitsliced_corrected_soft_batch_i8.

TEST INFRASTRUCTURE ONLY: imported by tests/ and tools/, never by the product.

The decoder is the one flooding_fixed_corrected_restatement.py states -- the reference's decode_ms::<i8> with every check message
magnitude m replaced by max(((scale_num * m + ((1 << scale_shift) >> 1)) >> scale_shift) - offset, 0) -- and the fourth result is its
marginal va [n + p] (src/decoder.rs:377, :408): the LLR (zero for a punctured variable, which come last) plus, saturating in the
reference's edge order, the CORRECTED check messages of the iteration.  A frame that converges in iteration it carries that
iteration's va, a frame that does not converge the va of the cap's last iteration, and at cap 0 nothing was ever formed: all zero
(:374).  Saturating i8: -128 is reached.

Two statements, as there: decode_caps() / decode() over whole arrays, decode_loop() one frame edge by edge in Python integers.
"""
from __future__ import annotations

import numpy as np

from flooding_fixed_corrected_restatement import HI, LO, Structure, check_triple, correct, structure  # noqa: F401  (re-exported)


def decode_caps(st: Structure, llrs: np.ndarray, caps, scale_num, scale_shift, offset):
    """{cap: (output, iters, success, va)} for every cap of `caps` from ONE run to the largest of them (the iterations of a decode do
    not depend on its cap).  va [frames][n + p] int8."""
    check_triple(scale_num, scale_shift, offset)
    raw = np.ascontiguousarray(llrs)
    assert raw.dtype == np.int8
    L = raw.astype(np.int64)
    F = L.shape[0]
    E, C, V, n = st.E, st.C, st.V, st.n
    caps = sorted(set(int(c) for c in caps))
    res = {c: (np.zeros((F, V // 8), np.uint8), np.full(F, c, np.uint32), np.zeros(F, np.uint8), np.zeros((F, V), np.int8)) for c in caps}
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
        va8 = va.astype(np.int8)                                  # (already inside -128 .. 127)
        for c in caps:
            out, its, ok, app = res[c]
            if it < c:
                fr = live[done]
                out[fr], its[fr], ok[fr], app[fr] = hard[done], it, 1, va8[done]
            if it == c - 1:                                       # the cap's last iteration: what has not converged fails as it is
                out[live[~done]] = hard[~done]
                app[live[~done]] = va8[~done]
        stay = ~done
        live, v, min1, min2, sgn = live[stay], v[stay], min1[stay], min2[stay], sgn[stay]
    return res


def decode(st: Structure, llrs, maxiters, scale_num, scale_shift, offset):
    return decode_caps(st, llrs, [maxiters], scale_num, scale_shift, offset)[int(maxiters)]


def decode_loop(st: Structure, llrs_row, maxiters, scale_num, scale_shift, offset):
    """ONE frame, edge by edge in Python integers, in the reference's own loop order with its running two-minimum update (:430-434):
    (output [V/8] u8, iters, success, va [V] int8)."""
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
            return np.packbits(np.array([x < 0 for x in va], np.uint8)), it, 1, np.array(va, np.int8)
    return np.packbits(np.array([x < 0 for x in va], np.uint8)), maxiters, 0, np.array(va, np.int8)
