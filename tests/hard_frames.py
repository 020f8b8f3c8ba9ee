"""hard_frames.py -- small pools of hard-decision frames with their oracle results, shared by the GPU edge tests of the encoder
(tests/test_gpu_encode_edges.py) and of the bit-flipping decoder (tests/test_gpu_decode_bf_edges.py) and tied to the reference on
the CPU by tests/test_hard_frames_host.py.

TEST INFRASTRUCTURE ONLY.  The oracle decodes (encodes) every pool entry once; a GPU batch of any size is pool entries drawn by
index, so every frame of it has its oracle result and the comparison is a gather on the device:
  * bf_pool(code): 48 received words -- 16 error-free, 16 with 1-3 flipped bits, 16 with n/24 .. n/12 flipped bits -- with
    oracle.decode_bf's (output, iters, success) at 20 iterations and a class per frame (0: success at iteration 0, 1: success
    later, 2: failure); bf_results(code, maxiters) is the same pool at another cap;
  * enc_pool(code): 64 data blocks (all zero, all ones, the reference's known-answer input, eight single set bits, random) with
    oracle.copy_encode's codewords;
  * draw(): pool indices whose classes change from one group of g frames to the next (edge_frames.batch_of for three classes);
  * same_on_device(): exact comparison of device results with the pool's, naming the first differing frame.
"""
from __future__ import annotations

import functools

import numpy as np

import oracle

BF_FRAMES, ENC_BLOCKS, BF_ITERS = 48, 64, 20


def _frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


@functools.lru_cache(maxsize=None)
def bf_words(code):
    """[48, n/8] received words of bf_pool(code)."""
    code = int(code)
    n, k = oracle.n(code), oracle.k(code)
    rng = np.random.default_rng(7000 + code)
    words = np.zeros((BF_FRAMES, n // 8), dtype=np.uint8)
    for f in range(BF_FRAMES):
        words[f] = oracle.copy_encode(code, rng.integers(0, 256, k // 8, dtype=np.uint8))
        flips = 0 if f < 16 else int(rng.integers(1, 4)) if f < 32 else int(rng.integers(n // 24, n // 12))
        for pos in rng.choice(n, flips, replace=False):
            words[f, pos // 8] ^= 1 << (7 - pos % 8)
    return _frozen(words)[0]


@functools.lru_cache(maxsize=None)
def bf_results(code, maxiters=BF_ITERS):
    """(output [48, output_len] u8, iters [48] i32, success [48] u8) of oracle.decode_bf on bf_words(code) at `maxiters`."""
    code = int(code)
    words = bf_words(code)
    out = np.zeros((BF_FRAMES, oracle.output_len(code)), dtype=np.uint8)
    iters = np.zeros(BF_FRAMES, dtype=np.int32)
    ok = np.zeros(BF_FRAMES, dtype=np.uint8)
    for f in range(BF_FRAMES):
        ok[f], iters[f], out[f] = oracle.decode_bf(code, words[f], maxiters)
    return _frozen(out, iters, ok)


@functools.lru_cache(maxsize=None)
def bf_pool(code):
    """(words, (output, iters, success) at 20 iterations, class [48]): read-only, built once per code."""
    res = bf_results(code, BF_ITERS)
    _, iters, ok = res
    cls = np.where(ok == 0, 2, np.where(iters == 0, 0, 1)).astype(np.int64)
    return bf_words(code), res, _frozen(cls)[0]


@functools.lru_cache(maxsize=None)
def enc_pool(code):
    """(data [64, k/8], codewords [64, n/8]): read-only, built once per code."""
    code = int(code)
    n, k = oracle.n(code), oracle.k(code)
    kb = k // 8
    rng = np.random.default_rng(7100 + code)
    data = rng.integers(0, 256, (ENC_BLOCKS, kb), dtype=np.uint8)
    data[0] = 0
    data[1] = 0xFF
    data[2] = np.arange(kb, dtype=np.uint8)                  # the reference's known-answer input (src/encoder.rs:361-527)
    for j in range(8):                                       # one set bit: the parity is one row of the generator
        data[3 + j] = 0
        data[3 + j, j * kb // 8] = 0x80 >> j
    cws = np.zeros((ENC_BLOCKS, n // 8), dtype=np.uint8)
    for f in range(ENC_BLOCKS):
        cws[f] = oracle.copy_encode(code, data[f])
    return _frozen(data, cws)


def draw(classes, frames, g, rng):
    """Pool indices for `frames` frames: each group of g consecutive frames takes a class at random (never the class of the group
    before it) and its frames from that class's entries, one frame in four from the whole pool -- so the successive codewords of a
    wave or workgroup differ in kind."""
    ncls = int(classes.max()) + 1
    groups = (frames + g - 1) // g
    k = rng.integers(0, ncls, groups)
    step = rng.integers(1, ncls, groups)                     # a change of class: 1 .. ncls - 1
    for j in range(1, groups):
        if k[j] == k[j - 1]:
            k[j] = (k[j] + step[j]) % ncls
    by_class = [np.flatnonzero(classes == c) for c in range(ncls)]
    idx = np.empty(groups * g, dtype=np.int64)
    kk = np.repeat(k, g)
    for c in range(ncls):
        sel = kk == c
        idx[sel] = by_class[c][rng.integers(0, len(by_class[c]), int(sel.sum()))]
    mix = rng.random(len(idx)) < 0.25
    idx[mix] = rng.integers(0, len(classes), int(mix.sum()))
    return idx[:frames]


def on_device(arrays):
    """Copies of a pool's arrays on the current device."""
    import torch
    return tuple(torch.tensor(a).cuda() for a in arrays)


def same_on_device(tag, idx, got, ref, chunk=1 << 15):
    """Every frame of the device tensors `got` ([frames, ...] each) equals row idx[frame] of its partner in `ref` (device copies of
    a pool's arrays), exactly; gathered and compared a chunk of frames at a time."""
    import torch
    idx = torch.as_tensor(idx, device=got[0].device)
    for a in got:
        assert len(a) == len(idx), f"{tag}: {len(a)} frames for {len(idx)} indices"
    for s in range(0, len(idx), chunk):
        i = idx[s: s + chunk]
        bad = torch.zeros(len(i), dtype=torch.bool, device=idx.device)
        for a, r in zip(got, ref):
            d = a[s: s + chunk] != r[i]
            bad |= d.any(dim=1) if d.ndim == 2 else d
        nbad = int(bad.sum())
        assert nbad == 0, f"{tag}: {nbad} frames differ, first {s + int(torch.nonzero(bad)[0])}"
