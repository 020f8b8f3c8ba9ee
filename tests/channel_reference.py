"""channel_reference.py -- what csrc/channel.hip documents, restated in plain numpy (no GPU, no torch).

TEST INFRASTRUCTURE ONLY.  The channel writes  y = s + sigma * z  per sample, where
  * s is +1 for a clear and -1 for a set bit of codeword (frame mod pool), bits MSB first;
  * z comes from Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the known answers of the
    Random123 distribution are in tests/test_channel_reference_host.py): the block of quad q of GLOBAL frame f has the counter
    (q, f mod 2^32, f div 2^32, 0) and the key (seed mod 2^32, seed div 2^32); its words (x, y) give the Box-Muller pair of samples
    4q, 4q+1 and (z, w) that of samples 4q+2, 4q+3, with u1 = ((a >> 8) + 1) / 2^24 in (0, 1], u2 = (b >> 8) / 2^24 in [0, 1),
    r = sqrt(-2 ln u1) and the pair (r cos 2 pi u2, r sin 2 pi u2).
Written from that description as whole-array operations on [frames, quads] tables, not from the kernel's loop.  The integer part
is exact; frames64 / normals64 carry the floating part in float64 (the pass criterion of tests/test_gpu_channel_reference.py),
normals32_mirror / frames32_mirror round every step to f32 with correctly rounded log, sqrt, sin and cos (the CPU check of that
criterion's derivation, and an informational figure on the device)."""
from __future__ import annotations

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
PHILOX_M = (np.uint64(0xD2511F53), np.uint64(0xCD9E8D57))
PHILOX_W = (0x9E3779B9, 0xBB67AE85)
ROUNDS = 10
U = 2.0 ** -24                                     # unit roundoff of f32, and the spacing of the 24-bit uniforms


def philox4x32_10(ctr, key):
    """ctr: four uint64 arrays (values < 2^32) of one shape, key: two integers or arrays -> the four output words, uint64 < 2^32.
    One round: (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)); the key then advances by the Weyl
    constants mod 2^32."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in ctr)
    k0, k1 = (np.asarray(k, dtype=np.uint64) for k in key)
    assert all(int(np.max(v, initial=0)) <= 0xFFFFFFFF for v in (c0, c1, c2, c3, k0, k1))
    for _ in range(ROUNDS):
        p0 = PHILOX_M[0] * c0                      # 32 x 32 -> 64 bits: no wrap in uint64
        p1 = PHILOX_M[1] * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0 = (k0 + np.uint64(PHILOX_W[0])) & M32
        k1 = (k1 + np.uint64(PHILOX_W[1])) & M32
    return c0, c1, c2, c3


def uniform_words(n, first_frame, frames, seed):
    """The Philox words of frames [first_frame, first_frame + frames) of the job `seed`: uint64 [frames, n / 4, 4], values < 2^32.
    The frame index is the GLOBAL one (mod 2^64, as a uint64_t counts)."""
    assert n % 4 == 0 and 0 <= seed < 1 << 64 and 0 <= first_frame < 1 << 64
    glob = [(first_frame + i) % (1 << 64) for i in range(frames)]
    lo = np.array([g & 0xFFFFFFFF for g in glob], dtype=np.uint64).reshape(frames, 1)
    hi = np.array([g >> 32 for g in glob], dtype=np.uint64).reshape(frames, 1)
    q = np.arange(n // 4, dtype=np.uint64).reshape(1, n // 4)
    shape = (frames, n // 4)
    ctr = (np.broadcast_to(q, shape), np.broadcast_to(lo, shape), np.broadcast_to(hi, shape), np.zeros(shape, np.uint64))
    return np.stack(philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32)), axis=-1)


def _uniforms(words):
    """words [frames, quads, 4] -> (u1, u2) float64 [frames, quads, 2]: the pairs (x, y) and (z, w).  Exact in f32 and in f64."""
    a, b = words[..., 0::2], words[..., 1::2]
    u1 = ((a >> np.uint64(8)).astype(np.float64) + 1.0) * U
    u2 = (b >> np.uint64(8)).astype(np.float64) * U
    return u1, u2


def _cos_sin_2pi(u2):
    """(cos 2 pi u2, sin 2 pi u2) in float64 for u2 a multiple of 2^-24 in [0, 1).  The turn is split exactly into a count of
    quarter turns and a remainder of at most an eighth of a turn, so that the zeros (u2 = 0, 1/4, 1/2, 3/4) are exact zeros and nothing is lost
    to the rounding of 2 pi u2 near them."""
    k = np.rint(u2 * 4.0)                          # nearest quarter turn, 0..4
    f = u2 - k * 0.25                              # exact, |f| <= 1/8
    c, s = np.cos(2.0 * np.pi * f), np.sin(2.0 * np.pi * f)
    k = k.astype(np.int64) & 3
    cos = np.choose(k, [c, -s, -c, s])
    sin = np.choose(k, [s, c, -s, -c])
    return cos, sin


def _interleave(z0, z1):
    """[frames, quads, 2] x 2 -> [frames, n]: sample 4q + 2p + i is output i of pair p of quad q"""
    return np.stack([z0, z1], axis=-1).reshape(z0.shape[0], -1)


def normals64(n, first_frame, frames, seed, words=None):
    """The standard normals of the frames, float64 [frames, n].  (`words`: uniform_words of the same arguments, if at hand.)"""
    u1, u2 = _uniforms(uniform_words(n, first_frame, frames, seed) if words is None else words)
    r = np.sqrt(-2.0 * np.log(u1))
    c, s = _cos_sin_2pi(u2)
    return _interleave(r * c, r * s)


def normals32_mirror(n, first_frame, frames, seed, words=None):
    """The same sequence with every step rounded to f32; log, sqrt, cos and sin are evaluated in float64 on the f32 operand and then
    rounded, i.e. they are correctly rounded f32 functions (up to double rounding).  float32 [frames, n]."""
    u1, u2 = _uniforms(uniform_words(n, first_frame, frames, seed) if words is None else words)
    u1, u2 = u1.astype(np.float32), u2.astype(np.float32)                     # exact: 24-bit integers times 2^-24
    assert u1.dtype == np.float32
    lg = np.log(u1.astype(np.float64)).astype(np.float32)
    m = np.float32(-2.0) * lg                                                # exact
    r = np.sqrt(m.astype(np.float64)).astype(np.float32)
    c, s = _cos_sin_2pi(u2.astype(np.float64))                               # sincospi(2 u2): 2 u2 is exact
    c, s = c.astype(np.float32), s.astype(np.float32)
    return _interleave(r * c, r * s)                                         # numpy f32 products: one rounding each


def signs(code, pool_codewords, first_frame, frames):
    """+-1.0 float64 [frames, n]: frame f carries codeword (f mod pool), f the GLOBAL index (Python integers), bits MSB first."""
    pool_codewords = np.asarray(pool_codewords, dtype=np.uint8)
    n = int(code.n())
    assert pool_codewords.ndim == 2 and pool_codewords.shape[0] >= 1 and pool_codewords.shape[1] * 8 == n
    idx = [(first_frame + i) % pool_codewords.shape[0] for i in range(frames)]
    return 1.0 - 2.0 * np.unpackbits(pool_codewords[idx], axis=1, bitorder="big").astype(np.float64).reshape(frames, n)


def frames64(code, pool_codewords, first_frame, frames, sigma, seed, return_parts=False, words=None):
    """s + f32(sigma) * z in float64, [frames, n].  sigma is rounded to f32 first: the C entry takes a float.
    With return_parts: (y, s, z, sigma as the f32 value)."""
    s = signs(code, pool_codewords, first_frame, frames)
    z = normals64(int(code.n()), first_frame, frames, seed, words)
    sg = float(np.float32(sigma))
    y = s + sg * z
    return (y, s, z, sg) if return_parts else y


def frames32_mirror(code, pool_codewords, first_frame, frames, sigma, seed, words=None):
    """f32(s + f32(f32(sigma) * z32)) with z32 of normals32_mirror: float32 [frames, n]."""
    s = signs(code, pool_codewords, first_frame, frames).astype(np.float32)
    z = normals32_mirror(int(code.n()), first_frame, frames, seed, words)
    return s + np.float32(sigma) * z


def tolerance(y_ref, z_ref, sigma32, k):
    """The f32 pass criterion's right-hand side: u * (|y_ref| + K * sigma * |z_ref|), float64."""
    return U * (np.abs(y_ref) + k * sigma32 * np.abs(z_ref))
