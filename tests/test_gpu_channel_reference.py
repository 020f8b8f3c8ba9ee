"""The on-device channel (csrc/channel.hip: awgn_kernel) compared SAMPLE BY SAMPLE with tests/channel_reference.py, the float64
restatement of what channel.hip and include/labrador_ldpc_hip.h document: Philox4x32-10 with the counter (q, frame_lo, frame_hi, 0)
of the GLOBAL frame index and the key (seed_lo, seed_hi), 24-bit uniforms, Box-Muller, y = s + sigma * z.  tests/test_gpu_channel.py
checks the distribution; statistics cannot see noise that is shared between frames, seeds or quads, a generator that is not the
documented one, a wrong codeword of the pool or a wrong bit of it, or a write outside the batch.  These tests can.

Pass criterion for f32, every sample, u = 2^-24:

    |y_dev - y_ref| <= u * (|y_ref| + K * sigma * |z_ref|),     K = E_log + 2 E_sqrt + 2 E_sincospi + 2

An E-ulp function result has a relative error <= 2 E u.  (a >> 8) + 1, the scaling by 2^-24, 2 * u2 and -2 * log are exact in f32; the
square root halves the logarithm's relative error (E_log u) and adds its own (2 E_sqrt u); sincospi adds 2 E_sincospi u; r * c and
sigma * z are one rounding each (2 u: the library is built with -ffp-contract=off), and s + ... is one more, relative to y.  No copy
of the ROCm maximum-ulp table for logf / sqrtf / sincospif is installed beside the toolchain, so E = 2 is taken for each: K = 12, a
deliberate factor over the correctly rounded case (E = 0.5, K = 4.5), which tests/test_channel_reference_host.py verifies on the CPU.
Nothing measured on the device went into K.  Nothing is excluded from the f32 comparison: a sample with z_ref == 0 is held by |y_ref|.
Each comparison prints (-s) the largest deviation it saw as a fraction of this bound and in units of u * (|y_ref| + sigma |z_ref|),
the quantity docs/experiments.md records beside K (measured on an MI355X: at most 4.09), and on failure names the worst sample's Philox
words.  The fraction of the bound comes close to 1 in every large case and says nothing by itself: where z is near 0 the final
rounding of s + sigma * z alone may use all of u |y_ref|."""
import ctypes
import math

import numpy as np
import pytest

import channel_reference as cr
import labrador_ldpc_amd as la
from labrador_ldpc_amd import HipOpts, LDPCCode, LdpcHipError, MEM_DEVICE

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

K = 12.0                                        # E_log = E_sqrt = E_sincospi = 2 (module docstring)
SIGMA_2DB = 0.7943
CODES = list(LDPCCode)
EINVAL = -1


def _pool(code, rows, seed=7):
    """`rows` random codewords of the host encoder: uint8 [rows, n / 8]"""
    rng = np.random.default_rng(seed)
    cws = np.zeros((rows, code.n() // 8), np.uint8)
    for i in range(rows):
        code.copy_encode(rng.integers(0, 256, code.k() // 8, dtype=np.uint8), cws[i])
    return cws


def _dev():
    return torch.device("cuda", 0)


def _gen(code, cws, frames, sigma, seed, first=0, **kw):
    y = code.awgn_frames(torch.from_numpy(cws).to(_dev()), frames, sigma, seed=seed, first_frame=first, **kw)
    torch.cuda.synchronize()
    return y.cpu().numpy()


def _describe(words, f, j, y_dev, y_ref, z_ref):
    """what a reader needs to tell which function a deviating sample blames: its Philox words and the reference's intermediates"""
    q, p, i = j // 4, (j % 4) // 2, j % 2
    a, b = int(words[f, q, 2 * p]), int(words[f, q, 2 * p + 1])
    u1, u2 = ((a >> 8) + 1) * cr.U, (b >> 8) * cr.U
    r = math.sqrt(-2.0 * math.log(u1))
    return (f"frame {f} sample {j} (quad {q}, pair {p}, {'sin' if i else 'cos'} output): words a={a:#010x} b={b:#010x}, u1={u1!r} u2={u2!r}, "
            f"ln u1={math.log(u1)!r}, r={r!r}, z_ref={z_ref!r}, y_ref={y_ref!r}, y_dev={y_dev!r}")


def _check_f32(code, cws, first, frames, sigma, seed, y_dev, label, mirror=False):
    """every sample of y_dev [frames, n] against frames64 under the module's criterion; returns the largest normalised deviation"""
    assert y_dev.dtype == np.float32 and y_dev.shape == (frames, code.n())
    words = cr.uniform_words(code.n(), first, frames, seed)
    y_ref, _, z_ref, sg = cr.frames64(code, cws, first, frames, sigma, seed, return_parts=True, words=words)
    diff = np.abs(y_dev.astype(np.float64) - y_ref)
    tol = cr.tolerance(y_ref, z_ref, sg, K)
    frac = diff / tol                                                         # tol > 0: |y_ref| and |z_ref| are never both 0
    norm = diff / (cr.U * (np.abs(y_ref) + sg * np.abs(z_ref)))
    f, j = np.unravel_index(int(np.argmax(frac)), frac.shape)
    line = (f"{label}: {y_dev.size} samples, largest deviation {float(frac.max()):.3f} of the bound (K = {K:g}), "
            f"{float(norm.max()):.3f} u (|y| + sigma |z|)")
    if mirror:
        same = int((y_dev == cr.frames32_mirror(code, cws, first, frames, sigma, seed, words=words)).sum())
        line += f"; equal to the correctly rounded f32 mirror bit for bit: {same} of {y_dev.size} ({100.0 * same / y_dev.size:.2f} %)"
    print(line)
    assert np.isfinite(y_dev).all(), label
    assert (diff <= tol).all(), (f"{line}; {int((diff > tol).sum())} samples beyond the bound, the worst: "
                                 + _describe(words, f, j, float(y_dev[f, j]), float(y_ref[f, j]), float(z_ref[f, j])))
    return float(norm.max())


# ---- f32 against the reference --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("frames", [1, 64])
@pytest.mark.parametrize("code", CODES, ids=lambda c: c.name)
def test_f32_every_code_is_the_documented_generator(code, frames):
    """channel.hip awgn_kernel, all of it, at every quads_per_frame = n / 4 from 32 to 2048: `q = qd - local * quads_per_frame`, the
    Philox counter U4{q, frame, frame >> 32, 0}, `codewords[cwi * (n / 8) + q / 2]` and the MSB-first nibble.  Pool of 5."""
    cws = _pool(code, 5, seed=100 + int(code))
    seed = 0xA5A5_0000 + int(code)
    _check_f32(code, cws, 0, frames, SIGMA_2DB, seed, _gen(code, cws, frames, SIGMA_2DB, seed), f"{code.name} x {frames}", mirror=frames == 64)


@pytest.mark.parametrize("code,frames", [(LDPCCode.TC128, 65536 + 37), (LDPCCode.TM8192, 1024 + 3)], ids=["TC128", "TM8192"])
def test_f32_grid_stride_second_sweep_with_a_ragged_end(code, frames):
    """launch_awgn caps the grid at 256 * 32 workgroups of 256 threads = 2^21 quads; `qd += gridDim.x * blockDim.x` then carries a thread
    into a second sweep.  65 536 TC128 frames (32 quads each) or 1024 TM8192 frames (2048) fill the first sweep exactly; the rest is
    a second sweep that only some threads enter (`qd < total_quads`), on TC128 ending inside a workgroup.  Every sample compared."""
    quads, sweep = frames * (code.n() // 4), 256 * 32 * 256
    assert sweep < quads < 2 * sweep
    cws = _pool(code, 5, seed=31)
    seed = 0x5EED_0002
    _check_f32(code, cws, 0, frames, SIGMA_2DB, seed, _gen(code, cws, frames, SIGMA_2DB, seed), f"{code.name} x {frames}", mirror=True)


@pytest.mark.parametrize("first", [1, (1 << 32) - 3, (1 << 40) + 12345], ids=["1", "2^32-3", "2^40+12345"])
@pytest.mark.parametrize("code", [LDPCCode.TC256, LDPCCode.TM2048], ids=lambda c: c.name)
def test_f32_first_frame_feeds_both_counter_words_and_a_64_bit_modulo(code, first):
    """`frame = first_frame + local`, `(uint32_t)frame`, `(uint32_t)(frame >> 32)` and `frame % pool` with pool 3: 8 frames from
    2^32 - 3 cross the carry into the high counter word; beyond 2^40 a modulo taken on 32 bits picks other codewords.  The reference
    takes frame % pool on Python integers."""
    cws = _pool(code, 3, seed=5)
    seed = 0xF1F0
    _check_f32(code, cws, first, 8, SIGMA_2DB, seed, _gen(code, cws, 8, SIGMA_2DB, seed, first=first), f"{code.name} first_frame {first}")


@pytest.mark.parametrize("pool,frames,first", [(1, 7, 0), (3, 7, 0), (7, 7, 0), (100, 7, 95)],
                         ids=["pool1", "pool3", "pool=batch", "pool100_wraps"])
@pytest.mark.parametrize("code", [LDPCCode.TC512, LDPCCode.TM1536], ids=lambda c: c.name)
def test_f32_pool_sizes_around_the_batch(code, pool, frames, first):
    """`cwi = frame % pool`: a pool of one, one that is no power of two, one as large as the batch and one larger -- 100 codewords for the
    7 frames 95..101, which wrap to codewords 95..99, 0, 1."""
    cws = _pool(code, pool, seed=pool)
    seed = 0x9001 + pool
    _check_f32(code, cws, first, frames, SIGMA_2DB, seed, _gen(code, cws, frames, SIGMA_2DB, seed, first=first), f"{code.name} pool {pool}")


@pytest.mark.parametrize("seed", [0, 1, 1 << 32, 0xFFFFFFFFFFFFFFFF, 0x0123456789ABCDEF], ids=hex)
def test_f32_seed_is_the_64_bit_key(seed):
    """launch_awgn passes `(uint32_t)seed, (uint32_t)(seed >> 32)` as the Philox key (k0, k1): 2^32 has only the high word set and must
    not give the frames of seed 0."""
    code = LDPCCode.TM1280
    cws = _pool(code, 5, seed=17)
    _check_f32(code, cws, 0, 16, SIGMA_2DB, seed, _gen(code, cws, 16, SIGMA_2DB, seed), f"TM1280 seed {seed:#x}")


@pytest.mark.parametrize("sigma", [1e-3, 0.5, 1.2, 4.0])
def test_f32_sigma_scales_the_noise(sigma):
    """`s + sigma * z[j]`: the bound scales with sigma, so a small sigma holds the signal to an ulp of 1 and a large one the noise"""
    code = LDPCCode.TM6144
    cws = _pool(code, 5, seed=23)
    seed = 0x51 + int(sigma * 1000)
    _check_f32(code, cws, 3, 16, sigma, seed, _gen(code, cws, 16, sigma, seed, first=3), f"TM6144 sigma {sigma}")


@pytest.mark.parametrize("code", CODES, ids=lambda c: c.name)
def test_sigma_zero_writes_exactly_the_signs_of_the_pool(code):
    """With sigma == 0.0 the output is exactly +-1.0 = 1 - 2 * unpackbits(pool[frame % pool]): `byte = codewords[cwi * (n / 8) + q / 2]`,
    `nib = (q & 1) ? byte & 0xF : byte >> 4`, `(nib >> (3 - j)) & 1 ? -1 : +1` and `frame % pool`, with no tolerance, on every code."""
    cws = _pool(code, 5, seed=40 + int(code))
    first, frames = (1 << 33) + 2, 13
    y = _gen(code, cws, frames, 0.0, 0xD0, first=first)
    want = 1.0 - 2.0 * np.unpackbits(cws[[(first + i) % 5 for i in range(frames)]], axis=1).astype(np.float32)
    assert y.dtype == np.float32 and np.array_equal(y, want)
    assert np.array_equal(y, cr.frames64(code, cws, first, frames, 0.0, 0xD0).astype(np.float32))


def test_f32_the_frames_the_benchmark_times():
    """The benchmark's own job -- TM8192 f32, seed 0x1DBC + int(code), sigma of Eb/N0 = 2 dB, codewords drawn as the benchmark draws
    them -- at the eight shard starts r * 524 288 an 8-GPU run uses: the operating point of every published figure rests on these
    being s + sigma * N(0, 1) of the documented generator.  (16-codeword pool, 4 frames per shard start.)"""
    code = LDPCCode.TM8192
    sigma = float(np.sqrt(1.0 / (2.0 * (code.k() / code.n()) * 10.0 ** (2.0 / 10.0))))
    assert abs(sigma - SIGMA_2DB) < 1e-4
    cws = _pool(code, 16, seed=0x1DBC + int(code))
    seed = 0x1DBC + int(code)
    for r in range(8):
        first = r * 524288
        _check_f32(code, cws, first, 4, sigma, seed, _gen(code, cws, 4, sigma, seed, first=first), f"bench job shard {r}", mirror=True)


# ---- exact properties: sharding, bounds, streams, the plain entries ------------------------------------------------------------------

def _sentinel(dtype):
    return (torch.float32, 12345.0) if dtype == "f32" else (torch.int8, -128)       # neither can be produced: |y| <= 1 + 5.77 sigma, |q| <= lim <= 127


@pytest.mark.parametrize("dtype", ["f32", "i8"])
@pytest.mark.parametrize("code", [LDPCCode.TC512, LDPCCode.TM6144], ids=lambda c: c.name)
def test_a_batch_generated_in_pieces_is_the_batch(code, dtype):
    """channel.hip's promise that "a call that generates frames [a, b) of a job writes exactly bytes [a, b)": pieces of 1, 17, 0 and the
    rest, each with its own first_frame into a row slice of one tensor, equal the single call -- torch.equal, no tolerance."""
    cws = torch.from_numpy(_pool(code, 3, seed=9)).to(_dev())
    total, base, seed = 41, (1 << 32) - 20, 0x5A4D
    whole = code.awgn_frames(cws, total, SIGMA_2DB, seed=seed, dtype=dtype, first_frame=base)
    tdt, sent = _sentinel(dtype)
    out = torch.full((total, code.n()), sent, dtype=tdt, device=_dev())
    a = 0
    for size in (1, 17, 0, total - 18):
        code.awgn_frames(cws, size, SIGMA_2DB, seed=seed, dtype=dtype, first_frame=base + a, out=out[a:a + size])
        a += size
    torch.cuda.synchronize()
    assert a == total and torch.equal(out, whole)


@pytest.mark.parametrize("batch", [1, 65536 + 37], ids=["1", "second_sweep"])
@pytest.mark.parametrize("dtype", ["f32", "i8"])
def test_nothing_is_written_outside_the_batch(dtype, batch):
    """`qd < total_quads` and `dst = llrs + qd * 4`: `out` is rows [3, 3 + batch) of a tensor prefilled with a value the channel cannot
    produce; the three rows before and after keep it, every sample inside has lost it.  TC128, a batch of one (a quarter of a workgroup)
    and one that ends in the second grid sweep."""
    code = LDPCCode.TC128
    cws = torch.from_numpy(_pool(code, 5, seed=2)).to(_dev())
    tdt, sent = _sentinel(dtype)
    big = torch.full((batch + 6, code.n()), sent, dtype=tdt, device=_dev())
    code.awgn_frames(cws, batch, SIGMA_2DB, seed=77, dtype=dtype, out=big[3:3 + batch])
    torch.cuda.synchronize()
    assert bool((big[:3] == sent).all()) and bool((big[3 + batch:] == sent).all())
    assert bool((big[3:3 + batch] != sent).all())
    assert torch.equal(big[3:3 + batch], code.awgn_frames(cws, batch, SIGMA_2DB, seed=77, dtype=dtype))


@pytest.mark.parametrize("dtype", ["f32", "i8"])
def test_a_callers_stream_gives_the_default_streams_bytes(dtype):
    """capi.hip awgn(): `opts->stream` reaches hipLaunchKernelGGL; the frames do not depend on the stream they are made on"""
    code = LDPCCode.TM2048
    cws = torch.from_numpy(_pool(code, 5, seed=4)).to(_dev())
    want = code.awgn_frames(cws, 33, SIGMA_2DB, seed=0xABCD, dtype=dtype, first_frame=9)
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device=_dev())
    out = torch.zeros((33, code.n()), dtype=want.dtype, device=_dev())
    torch.cuda.synchronize()
    got = code.awgn_frames(cws, 33, SIGMA_2DB, seed=0xABCD, dtype=dtype, first_frame=9, out=out, stream=st.cuda_stream)
    st.synchronize()
    assert got is out and torch.equal(got, want)


def _opts():
    return HipOpts(0, MEM_DEVICE, torch.cuda.current_stream(_dev()).cuda_stream, 0, 0, None)


def test_the_plain_entries_are_the_at_entries_with_first_frame_zero():
    """capi.hip labrador_ldpc_hip_awgn_f32 / _i8 pass first_frame 0 to the same awgn<T>(): called through the library with ctypes, their
    bytes are awgn_frames(..., first_frame=0)'s."""
    code = LDPCCode.TM1536
    cws = torch.from_numpy(_pool(code, 5, seed=6)).to(_dev())
    seed, batch = 0x0123456789ABCDEF, 19
    opts = _opts()
    f = torch.zeros((batch, code.n()), dtype=torch.float32, device=_dev())
    q = torch.zeros((batch, code.n()), dtype=torch.int8, device=_dev())
    assert la.lib.labrador_ldpc_hip_awgn_f32(int(code), cws.data_ptr(), 5, f.data_ptr(), batch, SIGMA_2DB, seed, ctypes.byref(opts)) == 0
    assert la.lib.labrador_ldpc_hip_awgn_i8(int(code), cws.data_ptr(), 5, q.data_ptr(), batch, SIGMA_2DB, 30.0, 127, seed, ctypes.byref(opts)) == 0
    torch.cuda.synchronize()
    assert torch.equal(f, code.awgn_frames(cws, batch, SIGMA_2DB, seed=seed, dtype="f32", first_frame=0))
    assert torch.equal(q, code.awgn_frames(cws, batch, SIGMA_2DB, seed=seed, dtype="i8", scale=30.0, lim=127, first_frame=0))
    assert f.cpu().numpy().tobytes() == code.awgn_frames(cws, batch, SIGMA_2DB, seed=seed).cpu().numpy().tobytes()


# ---- i8 ---------------------------------------------------------------------------------------------------------------------------------

QUANT = [(8.0, 31), (30.0, 127), (8.0, 15), (1000.0, 127), (8.0, 0)]


@pytest.mark.parametrize("scale,lim", QUANT)
@pytest.mark.parametrize("code", CODES, ids=lambda c: c.name)
def test_i8_is_the_rounded_clamped_f32_frame_on_every_code(code, scale, lim):
    """Quant<int8_t>::q: `(int)rintf(scale * y)` clamped to [-lim, lim], of the very f32 sample the f32 kernel writes for the same
    (seed, first_frame) -- exactly, ties to even (torch.round), the product formed in f32.  lim = 0 writes nothing but 0; at scale 1000
    the clamp decides all but the samples within 0.1265 of zero, and both bounds occur."""
    cws = torch.from_numpy(_pool(code, 5, seed=60 + int(code))).to(_dev())
    seed, first, frames = 0xBEEF + lim, 1 << 32, 64
    y = code.awgn_frames(cws, frames, SIGMA_2DB, seed=seed, dtype="f32", first_frame=first)
    q = code.awgn_frames(cws, frames, SIGMA_2DB, seed=seed, dtype="i8", scale=scale, lim=lim, first_frame=first)
    torch.cuda.synchronize()
    assert q.dtype == torch.int8
    assert torch.equal(q, torch.clamp(torch.round(y * scale), -lim, lim).to(torch.int8))
    assert int(q.max()) <= lim and int(q.min()) >= -lim
    if lim == 0:
        assert not bool(q.any())
    if scale == 1000.0:
        assert int(q.max()) == 127 and int(q.min()) == -127
        # with the noise too small to reach zero every sample sits at the bound of its bit's sign
        small = code.awgn_frames(cws, frames, 0.05, seed=seed, dtype="i8", scale=scale, lim=lim, first_frame=first)
        sgn = code.awgn_frames(cws, frames, 0.0, seed=seed, dtype="f32", first_frame=first)
        assert torch.equal(small, (127 * sgn).to(torch.int8))


@pytest.mark.parametrize("scale,lim", [(8.0, 31), (30.0, 127), (8.0, 15)])
@pytest.mark.parametrize("code", CODES, ids=lambda c: c.name)
def test_i8_against_the_reference_away_from_rounding_ties(code, scale, lim):
    """The i8 kernel instance on its own, not through the f32 one: q_dev == clamp(rint(scale * y_ref), -lim, lim) for every sample whose
    scale * y_ref is farther from a tie (k + 1/2) than scale * tol + u |scale * y_ref| -- tol the f32 bound, the second term the rounding
    of the f32 product.  The excluded samples are chosen from the reference alone, must be at most 0.1 % (expected 2 * scale * tol, about
    1e-4 at scale 30) and must still be within 1 of the reference value.  (Scale 1000 is left to the test above: there the margin alone
    exceeds 0.1 % although the clamp decides those samples.)"""
    cws = _pool(code, 5, seed=80 + int(code))
    seed, first, frames = 0x18 + lim, 6, 64
    q = _gen(code, cws, frames, SIGMA_2DB, seed, first=first, dtype="i8", scale=scale, lim=lim).astype(np.int64)
    y_ref, _, z_ref, sg = cr.frames64(code, cws, first, frames, SIGMA_2DB, seed, return_parts=True)
    t = scale * y_ref
    margin = scale * cr.tolerance(y_ref, z_ref, sg, K) + cr.U * np.abs(t)
    tie_dist = np.abs(t - np.floor(t) - 0.5)
    excluded = tie_dist <= margin
    want = np.clip(np.rint(t), -lim, lim).astype(np.int64)
    share = float(excluded.mean())
    print(f"{code.name} scale {scale:g} lim {lim}: {int(excluded.sum())} of {t.size} samples within the margin of a tie ({share:.2e})")
    assert share <= 1e-3, share
    assert np.array_equal(q[~excluded], want[~excluded]), int((q != want)[~excluded].sum())
    assert int(np.abs(q - want).max()) <= 1
    assert int(np.abs(q).max()) <= lim


# ---- arguments -------------------------------------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused_and_write_nothing():
    """capi.hip awgn(): `pool == 0`, `lim < 0 || lim > 127` and `(uintptr_t)llrs % 16` return EINVAL before anything is launched: the
    sentinel-filled `out` is untouched.  `if (batch == 0) return OK` writes nothing either."""
    code = LDPCCode.TC256
    n = code.n()
    cws = torch.from_numpy(_pool(code, 5, seed=1)).to(_dev())
    f = torch.full((4, n), 12345.0, dtype=torch.float32, device=_dev())
    q = torch.full((4, n), -128, dtype=torch.int8, device=_dev())
    with pytest.raises(LdpcHipError, match="status -1"):
        code.awgn_frames(cws[:0], 4, SIGMA_2DB, seed=1, dtype="f32", out=f)
    with pytest.raises(LdpcHipError, match="status -1"):
        code.awgn_frames(cws[:0], 4, SIGMA_2DB, seed=1, dtype="i8", out=q)
    for lim in (-1, 128):
        with pytest.raises(LdpcHipError, match="status -1"):
            code.awgn_frames(cws, 4, SIGMA_2DB, seed=1, dtype="i8", lim=lim, out=q)
    # an f32 buffer that is 4-byte but not 16-byte aligned: the kernel stores float4
    opts = _opts()
    for entry, extra in ((la.lib.labrador_ldpc_hip_awgn_f32, ()), (la.lib.labrador_ldpc_hip_awgn_f32_at, (0,))):
        st = entry(int(code), cws.data_ptr(), 5, f.data_ptr() + 4, *extra, 3, SIGMA_2DB, 1, ctypes.byref(opts))
        assert st == EINVAL
        with pytest.raises(LdpcHipError, match="status -1"):
            la._check(st)
    # batch == 0: OK, nothing written (a NULL pool is not even looked at)
    assert la.lib.labrador_ldpc_hip_awgn_f32_at(int(code), cws.data_ptr(), 5, f.data_ptr(), 0, 0, SIGMA_2DB, 1, ctypes.byref(opts)) == 0
    assert la.lib.labrador_ldpc_hip_awgn_i8_at(int(code), cws.data_ptr(), 5, q.data_ptr(), 0, 0, SIGMA_2DB, 8.0, 31, 1, ctypes.byref(opts)) == 0
    assert tuple(code.awgn_frames(cws, 0, SIGMA_2DB, seed=1).shape) == (0, n)
    torch.cuda.synchronize()
    assert bool((f == 12345.0).all()) and bool((q == -128).all())
