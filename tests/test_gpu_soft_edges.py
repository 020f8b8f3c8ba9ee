"""Soft output of the flooding kernels (LDPCCode.decode_ms_soft_batch) at the numeric and batch edges that the hard-only parity tests
(tests/test_gpu_parity.py) cover: the clamp-free loop at its magnitude limit, the clamp form's extreme ratios and the bounded mode's
lower bound, long iteration caps (FORM 3 of the self-correction beyond 28 iterations), whole-frame extremes, the ends of the integer
ranges, two-pass NaN handling at real batch sizes, state left behind by earlier decodes, and persistent workgroups that decode more
than one group of codewords.

Every comparison has two parts: app equals the oracle's marginals va (oracle.decode_ms_soft_batch) as values, with NaN exactly where
va is NaN; output, iters and success equal the oracle's and those of the hard-only call on the same frames."""
import numpy as np
import pytest

import edge_frames
from kernel_inventory import F32_VARIANTS, F64_TUNED, F64_VARIANTS
import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode
import oracle

pytestmark = pytest.mark.gpu

ALL = list(LDPCCode)
CLAMP_CODES = [LDPCCode.TM8192, LDPCCode.TM2048, LDPCCode.TC512, LDPCCode.TM1536]


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if la.device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("the soft-output GPU tests need a gfx950 device")
    torch.cuda.set_device(0)


def bad_frames(app, ref):
    """Frames whose app differs from ref under the header's rule (floats as values, NaN where NaN; integers exactly)."""
    a, b = np.asarray(app), np.asarray(ref)
    if a.dtype.kind == "f":
        na, nb = np.isnan(a), np.isnan(b)
        return np.flatnonzero(((na != nb) | (~na & ~nb & (a != b))).any(axis=1))
    return np.flatnonzero((a != b).any(axis=1))


def soft_and_hard(code, llrs, maxiters, variant=0, ref=None):
    """Soft and hard-only call on the same frames against the oracle; returns the oracle's (out, iters, ok, va)."""
    app, out, it, ok = code.decode_ms_soft_batch(llrs, maxiters, variant=variant)
    out_h, it_h, ok_h = code.decode_ms_batch(llrs, maxiters, variant=variant)
    r = ref if ref is not None else oracle.decode_ms_soft_batch(code, llrs, maxiters)
    tag = f"{code.name} {llrs.dtype} variant {variant} maxiters {maxiters}"
    bad = bad_frames(app, r[3])
    assert bad.size == 0, f"{tag}: app differs from the oracle's va in frames {bad[:8]}"
    bad = np.flatnonzero((it != r[1]) | (ok != r[2]) | (out != r[0]).any(axis=1))
    assert bad.size == 0, f"{tag}: hard results differ from the oracle's in frames {bad[:8]}"
    assert (out == out_h).all() and (it == it_h).all() and (ok == ok_h).all(), f"{tag}: soft and hard-only calls differ"
    return r


def limit_exponents(maxiters):
    """log2 of the clamp-free loop's magnitude limit and of the clamp form's (nocap_limit_for, decode_ms_launch.hpp)."""
    return int(np.floor(126.0 - 2.8074 * maxiters)), int(np.floor(82.5 - 2.8074 * maxiters))


# ---------------------------------------------------------------------------------------------------------------------------- B1

@pytest.mark.parametrize("code", CLAMP_CODES, ids=lambda c: c.name)
def test_clamp_free_path_at_its_magnitude_limit(code):
    """Every |LLR| at either limit formula's bound (and one binade above, 2^64, 1.0), random signs, never converging, at caps 5 ... 300;
    then the same frames with every third LLR scaled by 2^-20."""
    rng = np.random.default_rng(64)
    signs = np.where(rng.random((12, code.n())) < 0.5, 1.0, -1.0).astype(np.float32)
    for maxiters in (5, 20, 25, 28, 29, 44, 60, 300):
        e, e2 = limit_exponents(maxiters)
        for mag in (2.0 ** max(e, -120), 2.0 ** min(max(e, -120) + 1, 127), 2.0 ** 64, 1.0,
                    2.0 ** max(e2, -19), 2.0 ** (max(e2, -19) + 1)):
            llrs = signs * np.float32(mag)
            _, it, ok, _ = soft_and_hard(code, llrs, maxiters)
            assert (ok == 0).all() and (it == maxiters).all(), "frames at the limit must keep iterating to the cap"
            llrs[:, ::3] *= np.float32(2.0 ** -20)
            soft_and_hard(code, llrs, maxiters)


@pytest.mark.parametrize("code", CLAMP_CODES, ids=lambda c: c.name)
def test_clamp_form_of_the_self_correction_with_extreme_magnitude_ratios(code):
    """LLRs at the top of the clamp form's range mixed with 2^-20 and exact zeros, signs disagreeing, on both sides of the switch
    between the two forms (28 / 29 iterations), and one binade above (the clamped loop)."""
    rng = np.random.default_rng(0xC1B)
    n = code.n()
    for maxiters in (8, 25, 28, 29, 40):
        top = 2.0 ** max(limit_exponents(maxiters)[1], 3)
        frames = []
        for f in range(10):
            mags = np.where(rng.random(n) < 0.5, top, 2.0 ** -20) * (1.0 + rng.random(n) * (f % 2))
            x = np.where(rng.random(n) < 0.5, 1.0, -1.0) * mags
            x[rng.random(n) < 0.05] = 0.0
            frames.append(x)
        llrs = np.asarray(frames, dtype=np.float32)
        soft_and_hard(code, llrs, maxiters)
        soft_and_hard(code, (llrs * np.float32(2.0)).astype(np.float32), maxiters)


@pytest.mark.parametrize("code", CLAMP_CODES, ids=lambda c: c.name)
def test_bounded_mode_at_the_small_end_of_its_llr_range(code):
    """Every nonzero |LLR| in [2^-20, 2^-19) (the multiply form), AWGN frames scaled below the bound, one LLR under it or denormal,
    and exact zeros of both signs (the bit-operation form)."""
    rng = np.random.default_rng(21)
    y, _ = oracle.awgn_llrs(code, rng, 24, 2.0, np.float32)
    mags = (np.float32(2.0 ** -20) * (1.0 + rng.random(y.shape))).astype(np.float32)
    at_bound = np.copysign(mags, y).astype(np.float32)
    soft_and_hard(code, at_bound, 25)
    soft_and_hard(code, (y * np.float32(2.0 ** -18)).astype(np.float32), 25)
    below = at_bound.copy()
    below[::2, 17] = np.float32(2.0 ** -21)
    below[1::4, 5] = np.float32(1e-42)
    below[3::4, ::9] = 0.0
    soft_and_hard(code, below, 25)
    zeros = at_bound.copy()
    zeros[:, ::3] = 0.0
    zeros[:, 1::3] = -0.0
    soft_and_hard(code, zeros, 25)


# ---------------------------------------------------------------------------------------------------------------------------- B2

@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int8, np.int16], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("code", ALL, ids=lambda c: c.name)
def test_long_caps_at_low_ebn0(code, dtype):
    """Frames that keep failing (0 and 1 dB) and some that converge late, at caps 29, 50 and 100 (f32: FORM 3 of the self-correction
    beyond 28) -- 50 for the narrow integer types."""
    rng = np.random.default_rng(0x10C + 10 * int(code) + [np.float32, np.float64, np.int8, np.int16].index(dtype))
    F = 4 if code.n() >= 5120 else 6
    parts = [oracle.awgn_llrs(code, rng, F, e, dtype)[0] for e in (0.0, 1.0, 2.0)]
    llrs = np.concatenate(parts)
    for maxiters in ((29, 50, 100) if np.dtype(dtype).kind == "f" else (50,)):
        _, it, ok, _ = soft_and_hard(code, llrs, maxiters)
        assert (ok == 0).any() and (it[ok == 0] == maxiters).all()


# ---------------------------------------------------------------------------------------------------------------------------- B3

@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("code", ALL, ids=lambda c: c.name)
def test_whole_frame_extremes_through_every_variant(code, dtype):
    """All +-0.0, every third / fifth zero, denormal frames, LLRs whose sums overflow, +-inf runs and +-MAX frames (the rows of
    test_f32_corner_values / test_f64_corner_values, whole) through every variant with a soft form, at caps 3, 20 and 50.  A +inf
    marginal of finite LLRs (an overflowing sum) must stay +inf in app: the epilogue's NaN check must only act at a NaN LLR."""
    rng = np.random.default_rng(0xF4A + int(code))
    llrs = edge_frames.whole_frame_rows(code, dtype, rng)
    variants = (F32_VARIANTS if dtype == np.float32 else F64_VARIANTS)[code]
    saw_inf = False
    for maxiters in (3, 20, 50):
        ref = oracle.decode_ms_soft_batch(code, llrs, maxiters)
        saw_inf |= bool(np.isinf(ref[3][[5, 8]]).any())
        for variant in variants:
            soft_and_hard(code, llrs, maxiters, variant=variant, ref=ref)
    assert saw_inf, "the overflow rows should reach an infinite marginal"


# ---------------------------------------------------------------------------------------------------------------------------- B4

@pytest.mark.parametrize("dtype", [np.int8, np.int16], ids=["i8", "i16"])
@pytest.mark.parametrize("code", ALL, ids=lambda c: c.name)
def test_integer_self_correction_at_the_ends_of_the_range(code, dtype):
    """Full-scale LLRs of random sign, full scale with 0 / +-1, noisy frames clipped at the type's limits, 50 iterations, every variant
    of the code with a soft form."""
    rng = np.random.default_rng(0xF7 + int(code) + np.iinfo(dtype).bits)
    llrs = edge_frames.integer_range_rows(code, dtype, rng, 8 if code.n() >= 5120 else 16)
    ref = oracle.decode_ms_soft_batch(code, llrs, 50)
    for variant in {LDPCCode.TM8192: (0, 2), LDPCCode.TM1536: (0, 2), LDPCCode.TM6144: (0, 2)}.get(code, (0,)):
        soft_and_hard(code, llrs, 50, variant=variant, ref=ref)


@pytest.mark.parametrize("code", ALL, ids=lambda c: c.name)
def test_i32_at_every_scale(code):
    """test_i32_parity's scales (a few units to +-2^31, INT_MIN included) and frames of nothing but INT_MIN / INT_MAX; TM8192 also on
    its (t, t + M/2) and pair kernels (variants 2 and 32)."""
    rng = np.random.default_rng(0x133 + int(code))
    llrs = edge_frames.integer_range_rows(code, np.int32, rng, 6 if code.n() >= 5120 else 12)
    for maxiters in (6, 25):
        ref = oracle.decode_ms_soft_batch(code, llrs, maxiters)
        for variant in ((0, 2, 32) if code == LDPCCode.TM8192 else (0,)):
            soft_and_hard(code, llrs, maxiters, variant=variant, ref=ref)


# ---------------------------------------------------------------------------------------------------------------------------- B5

def nan_base(code, rng):
    """test_nan_two_pass's frames: 24 clean ones (-0.0, +-inf runs) and 12 with NaNs of every kind."""
    n = code.n()
    clean, _ = oracle.awgn_llrs(code, rng, 24, 3.5, np.float32)
    clean[0, ::5] = -0.0
    clean[1, ::7] = np.inf
    clean[2, ::9] = -np.inf
    dirty, _ = oracle.awgn_llrs(code, rng, 12, 3.5, np.float32)
    pats = [np.uint32(v) for v in (0x7FC00000, 0xFFC00000, 0x7FA00000, 0xFFA00001)]
    u = dirty.view(np.uint32)
    for row in range(4):
        u[row, rng.integers(n)] = pats[row]
    for row in range(4, 8):
        for j, pos in enumerate(rng.permutation(n)[:40]):
            u[row, pos] = pats[j % 4]
    u[8, :] = pats[1]
    u[9, ::2] = pats[3]
    dirty[10, ::13] = np.inf
    u[10, 5::13] = pats[1]
    u[11, n - 1] = pats[1]
    return clean, dirty


@pytest.mark.parametrize("code", [LDPCCode.TM5120, LDPCCode.TM1280], ids=lambda c: c.name)
def test_nan_two_pass_at_real_batch_sizes(code):
    """The register-lean kernels' two-pass NaN handling with soft output: batches large enough for the default to take two passes,
    NaNs at the first and last codeword, in a run and scattered; variants 0 (default), 512 (one pass) and 1024 (two passes); every
    frame checked, on the device."""
    import torch
    rng = np.random.default_rng(0x7B + int(code))
    clean, dirty = nan_base(code, rng)
    base = np.concatenate([clean, dirty])
    nc, nd = len(clean), len(dirty)
    dref = edge_frames.device_ref(oracle.decode_ms_soft_batch(code, base, 25))
    big = 12000 if code == LDPCCode.TM5120 else 40000
    idx = rng.integers(0, nc, big)
    idx[0], idx[-1] = nc, nc + 11
    idx[1000:1000 + nd] = nc + np.arange(nd)
    idx[rng.integers(0, big, 300)] = nc + rng.integers(0, nd, 300)
    idx_d = torch.from_numpy(idx).cuda()
    d = torch.from_numpy(base).cuda()[idx_d].contiguous()
    for variant in (0, 512, 1024):
        res = code.decode_ms_soft_batch(d, 25, variant=variant)
        hard = code.decode_ms_batch(d, 25, variant=variant)
        torch.cuda.synchronize()
        edge_frames.check_on_device(f"{code.name} variant {variant}", idx_d, res, dref)
        for x, y in zip(res[1:], hard):
            assert torch.equal(x, y), f"{code.name} variant {variant}: soft and hard-only calls differ"
        del res, hard
    del d, dref
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------------------- B6

@pytest.mark.parametrize("dtype", [np.float32, np.int8, np.int16, np.int32, np.float64], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("code", ALL, ids=lambda c: c.name)
def test_small_caps_after_a_long_decode(code, dtype):
    """After a longer soft decode of other frames has left its state behind: cap 0 gives an all-zero app (and zero hard results), caps
    1 and 2 equal the oracle -- frames that are codewords already, frames that converge at the cap and frames that do not."""
    rng = np.random.default_rng(0x5A + 10 * int(code))
    scale, lim = (3e8, 2 ** 31 - 1) if dtype == np.int32 else (8.0, 31)
    other, _ = oracle.awgn_llrs(code, rng, 256, 1.0, dtype, scale=scale, lim=lim)
    llrs = np.concatenate([oracle.awgn_llrs(code, rng, F, e, dtype, scale=scale, lim=lim)[0] for F, e in ((24, 4.0), (8, 30.0))])
    for maxiters in (0, 1, 2):
        code.decode_ms_soft_batch(other, 8)
        if maxiters == 0:
            app, out, it, ok = code.decode_ms_soft_batch(llrs, 0)
            assert not app.any() and not out.any() and not it.any() and not ok.any()
        else:
            soft_and_hard(code, llrs, maxiters)


# ---------------------------------------------------------------------------------------------------------------------------- B7

def flooding_grid_bound(code, dtype, variant, cus):
    """(most frames one round of the persistent grid can hold, codewords per group) of the flooding launch (edge_frames.grid_bound):
    Geometry<CODE, T, IPT> with the default or the named IPT; the pair kernel (TM8192's default, variant 32) one codeword per workgroup
    of M / 2 threads; the launch's queue for workgroups of 512 threads and more unless the variant asks for the fixed stride."""
    M = code.submatrix_size()
    v = variant & ~0x700
    if code == LDPCCode.TM8192 and np.dtype(dtype) != np.float64 and v in (0, 32):
        wg, g = M // 2, 1
    else:
        ipt = (F64_TUNED[int(code)] if np.dtype(dtype) == np.float64 else 1) if v == 0 else v
        nt = M // (ipt & 15)
        g = 64 // nt if nt < 64 else 1
        wg = nt * g
    return edge_frames.grid_bound(wg, g, wg >= 512 and not variant & 256, cus), g


def mixed_pool(code, dtype, maxiters, rng):
    """Distinct frames of five kinds: converging, failing, overflowing (floats) or full scale (integers), NaN (floats) or full scale
    with 0 / +-1 (integers), at the clamp-free limit of `maxiters` (floats: both formulas) or noisy and clipped (integers).
    Returns (pool, kind of each entry)."""
    dt = np.dtype(dtype)
    n = code.n()
    F = 16
    hi = {0: 5.0, 1: 4.5, 2: 4.0}.get(int(code), 3.5)
    if dt.kind == "f":
        conv = oracle.awgn_llrs(code, rng, F, hi, dt)[0]
        fail = oracle.awgn_llrs(code, rng, F, 0.0, dt)[0]
        over = oracle.awgn_llrs(code, rng, F, 2.0, dt)[0] * dt.type(1e37 if dt == np.float32 else 1e307)
        nan = oracle.awgn_llrs(code, rng, F, 3.0, dt)[0]
        for f in range(F):
            nan[f, rng.choice(n, size=1 + 3 * f, replace=False)] = np.nan
        e, e2 = limit_exponents(maxiters)
        signs = np.where(rng.random((F, n)) < 0.5, 1.0, -1.0)
        limit = (signs * np.where(np.arange(F)[:, None] % 2 == 0, 2.0 ** e, 2.0 ** max(e2, -19))).astype(dt)
    else:                                               # (i8 / i16)
        conv = oracle.awgn_llrs(code, rng, F, hi, dt)[0]
        fail = oracle.awgn_llrs(code, rng, F, 0.0, dt)[0]
        over, nan, limit = np.split(edge_frames.integer_range_rows(code, dt, rng, F), 3)
    pool = np.concatenate([conv, fail, over, nan, limit]).astype(dt)
    kind = np.repeat(np.arange(5), F)
    return pool, kind


PERSIST = ([(c, np.float32, 0) for c in ALL]
           + [(c, np.float32, 256) for c in (LDPCCode.TM2048, LDPCCode.TM5120, LDPCCode.TM6144, LDPCCode.TM8192)]
           + [(c, np.int16, 0) for c in (LDPCCode.TC128, LDPCCode.TM1280, LDPCCode.TM2048, LDPCCode.TM8192)]
           + [(c, np.float64, 0) for c in (LDPCCode.TC256, LDPCCode.TM1280, LDPCCode.TM2048)])


def run_persistent(tag, decode, hard, code, dtype, pool, idx, ref, maxiters):
    """Prefilled outputs, two launches back to back on one stream, then one on a second stream; every frame against its pool entry."""
    import torch
    np_len = code.n() + code.punctured_bits()
    tdt = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64, np.dtype(np.int16): torch.int16}[np.dtype(dtype)]
    idx_d = torch.from_numpy(idx).cuda()
    d = torch.from_numpy(pool).cuda()[idx_d].contiguous()
    dref = edge_frames.device_ref(ref)
    B = len(idx)

    def sentinels():
        fill = -7.0e30 if np.dtype(dtype).kind == "f" else -12345
        return (torch.full((B, np_len), fill, dtype=tdt, device="cuda"), torch.full((B, code.output_len()), 0xEE, dtype=torch.uint8, device="cuda"),
                torch.full((B,), -2, dtype=torch.int32, device="cuda"), torch.full((B,), 7, dtype=torch.uint8, device="cuda"))

    bufs = [sentinels(), sentinels()]
    torch.cuda.synchronize()
    for b in bufs:
        decode(d, maxiters, app=b[0], output=b[1], iters=b[2], success=b[3])
    h = hard(d, maxiters)
    torch.cuda.synchronize()
    for r, b in enumerate(bufs):
        edge_frames.check_on_device(f"{tag} run {r}", idx_d, b, dref)
    for x, y in zip(bufs[0][1:], h):
        assert torch.equal(x, y), f"{tag}: soft and hard-only calls differ"
    del bufs, h
    b = sentinels()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        decode(d, maxiters, app=b[0], output=b[1], iters=b[2], success=b[3], stream=s.cuda_stream)
    s.synchronize()
    edge_frames.check_on_device(f"{tag} second stream", idx_d, b, dref)
    del b, d, dref, idx_d
    torch.cuda.empty_cache()


@pytest.mark.parametrize("code,dtype,variant", PERSIST, ids=lambda x: getattr(x, "name", str(x)) if not isinstance(x, type) else np.dtype(x).name)
def test_persistent_workgroups_decode_many_groups(code, dtype, variant):
    """A batch with more codeword groups than the largest grid the launch can have, so that workgroups decode group after group of
    mixed kinds (converging, failing, overflowing, NaN, at the clamp-free limit): every frame's app and hard results equal its pool
    entry's oracle result, in two launches back to back and one on another stream, into prefilled buffers."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    maxiters = 20
    bound, g = flooding_grid_bound(code, dtype, variant, cus)
    rng = np.random.default_rng(0x9E + 7 * int(code) + (variant >> 8))
    pool, kind = mixed_pool(code, dtype, maxiters, rng)
    ref = oracle.decode_ms_soft_batch(code, pool, maxiters)
    if np.dtype(dtype).kind == "f":
        lim = kind == 4
        assert (ref[2][lim] == 0).all() and (ref[1][lim] == maxiters).all(), "clamp-free-limit frames must fail at the cap"
    frames = bound + bound // 16 + 3
    assert frames > bound and (frames + g - 1) // g > bound // g
    idx = edge_frames.batch_of(pool, kind, frames, g, rng)
    decode = lambda *a, **k: code.decode_ms_soft_batch(*a, variant=variant, **k)      # noqa: E731
    hard = lambda *a: code.decode_ms_batch(*a, variant=variant)                       # noqa: E731
    run_persistent(f"{code.name} {np.dtype(dtype).name} variant {variant}", decode, hard, code, dtype, pool, idx, ref, maxiters)
