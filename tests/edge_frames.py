"""edge_frames.py -- frames at the numeric edges of the decoders, shared by the CPU cross-checks of the references and the GPU tests.

TEST INFRASTRUCTURE ONLY.  The rows are those of tests/test_gpu_parity.py's corner and integer-range tests, built whole:
  * whole_frame_rows(): every LLR of the frame is special (all +0.0, all -0.0, every third / fifth zero, denormal frames, LLRs scaled
    so that sums overflow, every seventh +inf, every eleventh -inf, +-MAX of random sign) -- f32 and f64 alike;
  * integer_range_rows(): full-scale LLRs of random sign, full scale mixed with 0 and +-1, noisy frames clipped at the type's limits
    (i32: the scales of test_i32_parity up to +-2^31, and frames of nothing but INT_MIN / INT_MAX).
"""
from __future__ import annotations

import numpy as np

import oracle


def whole_frame_rows(code, dtype, rng, base_ebn0=3.0):
    """9 frames [9, n] of a float type."""
    dt = np.dtype(dtype)
    fi = np.finfo(dt)
    n = oracle.n(code)
    llrs, _ = oracle.awgn_llrs(code, rng, 9, base_ebn0, dt)
    llrs[0, :] = 0.0
    llrs[1, :] = -0.0
    llrs[2, ::3] = 0.0
    llrs[3, ::5] = -0.0
    llrs[4] *= dt.type(1e-41 if dt == np.float32 else 1e-310)      # denormals
    llrs[5] *= dt.type(1e37 if dt == np.float32 else 1e307)        # sums of finite LLRs overflow to +-inf
    llrs[6, ::7] = np.inf
    llrs[7, ::11] = -np.inf
    llrs[8] = np.where(rng.random(n) < 0.5, fi.max, -fi.max)
    return llrs


def integer_range_rows(code, dtype, rng, frames):
    """[3 * frames, n] for i8 / i16 (full scale, full scale with 0 / +-1, noisy and clipped); for i32 the scales of
    test_i32_parity (a few units to +-2^31, INT_MIN included) and full-scale frames of INT_MIN / INT_MAX."""
    info = np.iinfo(dtype)
    n = oracle.n(code)
    if np.dtype(dtype) == np.int32:
        parts = []
        for ebn0, scale in ((2.5, 3.0), (2.0, 1000.0), (3.0, 2.0 ** 24 + 1), (2.5, 3e8), (2.0, 1.5e9), (1.0, 4e9)):
            x, _ = oracle.awgn_llrs(code, rng, max(1, frames // 3), ebn0 + (1.5 if n <= 1280 else 0.0), np.int32, scale=scale,
                                    lim=2 ** 31 - 1)
            if scale > 1e9:
                x[x == -(2 ** 31 - 1)] = -2 ** 31
            parts.append(x)
        parts.append(np.where(rng.random((frames, n)) < 0.5, 2 ** 31 - 1, -2 ** 31).astype(np.int32))
        return np.concatenate(parts)
    full = np.where(rng.random((frames, n)) < 0.5, info.max, info.min).astype(dtype)
    mixed = full.copy()
    r = rng.random((frames, n))
    mixed[r < 0.25] = 0
    mixed[(r >= 0.25) & (r < 0.4)] = 1
    mixed[(r >= 0.4) & (r < 0.55)] = -1
    noisy, _ = oracle.awgn_llrs(code, rng, frames, 2.0 if n > 1280 else 4.0, dtype, scale=info.max / 1.5, lim=info.max)
    noisy[noisy == -info.max] = info.min
    return np.concatenate([full, mixed, noisy])


# ---- batches for the persistent-workgroup tests

WAVES_PER_CU = 32                                        # at most, on CDNA


def grid_bound(wg, g, queued, cus):
    """Most frames one round of a persistent grid can hold (decode_ms_launch.hpp, persistent_grid): resident workgroups <= 32 waves
    per CU / waves per workgroup; grid <= 16 x resident without the launch's queue, <= resident with it; g codewords per group."""
    resident = WAVES_PER_CU * cus // ((wg + 63) // 64)
    return (resident if queued else 16 * resident) * g


def batch_of(pool, kind, frames, g, rng):
    """Pool indices for `frames` frames, drawn so that the kinds of a workgroup's successive groups vary: each group of g codewords
    takes a kind at random (never the kind of the group before it) and its frames from that kind's entries, one in four frames of any
    kind."""
    groups = (frames + g - 1) // g
    k = rng.integers(0, 5, groups)
    for j in range(1, groups):                          # (a vectorised redraw would do; this is cheap enough at these sizes)
        if k[j] == k[j - 1]:
            k[j] = (k[j] + 1 + rng.integers(0, 4)) % 5
    by_kind = [np.flatnonzero(kind == c) for c in range(5)]
    idx = np.empty(groups * g, dtype=np.int64)
    kk = np.repeat(k, g)
    for c in range(5):
        sel = kk == c
        idx[sel] = by_kind[c][rng.integers(0, len(by_kind[c]), int(sel.sum()))]
    mix = rng.random(len(idx)) < 0.25
    idx[mix] = rng.integers(0, len(pool), int(mix.sum()))
    return idx[:frames]


def device_ref(ref):
    import torch
    out, it, ok, va = ref
    return (torch.from_numpy(out).cuda(), torch.from_numpy(it.astype(np.int32)).cuda(), torch.from_numpy(ok).cuda(),
            torch.from_numpy(va).cuda())


def check_on_device(tag, idx, res, dref, chunk=1 << 16):
    """Every frame of a device batch against its pool entry's reference (dref gathered by idx), a chunk of frames at a time."""
    import torch
    app, out, it, ok = res
    r_out, r_it, r_ok, r_app = dref
    for s in range(0, len(idx), chunk):
        i = idx[s: s + chunk]
        a, e = app[s: s + chunk], r_app[i]
        if a.dtype.is_floating_point:
            na, nb = torch.isnan(a), torch.isnan(e)
            bad = ((na != nb) | (~na & ~nb & (a != e))).any(dim=1)
        else:
            bad = (a != e).any(dim=1)
        bad |= (out[s: s + chunk] != r_out[i]).any(dim=1) | (it[s: s + chunk] != r_it[i]) | (ok[s: s + chunk] != r_ok[i])
        nbad = int(bad.sum())
        assert nbad == 0, f"{tag}: {nbad} frames differ, first {s + int(torch.nonzero(bad)[0])}"
