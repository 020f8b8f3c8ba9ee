"""Fixed-point layered min-sum decoding on the GPU (labrador_ldpc_decode_ms_layered_fixed_{,soft_}batch_{i8,i16},
LDPCCode.decode_ms_layered_fixed_batch and decode_ms_layered_fixed_soft_batch) against the CPU restatement of the contract
(tests/layered_fixed_restatement.py), bit for bit: output, iters, success and the int32 app -- for every code and both
types, iteration caps 0 / 1 / 2 / 3 / 25, AWGN frames (quantisations that clamp and that do not), corner frames, batch sizes around the
codewords per workgroup, one batch of many groups per persistent workgroup, both memory modes, a caller's stream, a device set with a
repeated ordinal and caller-supplied buffers.  Fewer frames fail than under flooding, and the BER harness runs with the new types."""
import ctypes

import numpy as np
import pytest

import edge_frames
import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode
import layered_fixed_restatement as fr
import layered_helpers
from layered_helpers import quantise
import oracle

pytestmark = pytest.mark.gpu

ALL = list(LDPCCode)
TYPES = (np.int8, np.int16)
EUNSUPPORTED = -4
EBN0 = {LDPCCode.TC128: (3.0, 4.5), LDPCCode.TC256: (2.5, 4.0), LDPCCode.TC512: (2.0, 3.0)}
CAPS = (0, 1, 2, 3, 25)
CASES = [(c, t) for c in ALL for t in TYPES]
IDS = [f"{c.name}-{np.dtype(t).name}" for c, t in CASES]


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if la.device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("the fixed-point layered GPU tests need a gfx950 device")
    torch.cuda.set_device(0)


def structure(code):
    return layered_helpers.structure(code, fr.Structure)


def awgn(code, rng, frames, ebn0, dtype, wide=False):
    """AWGN frames quantised at 8 / 31 (which clamps messages of i8 often), or for i16 with `wide` at 64 / 2047."""
    y, _ = oracle.awgn_llrs(code, rng, frames, ebn0, np.float32)
    return quantise(y, dtype, 64, 2047) if wide and dtype == np.int16 else quantise(y, dtype, 8, 31)


def corner_frames(code, dtype, rng):
    """All T_MAX, all -T_MAX, all T's minimum, all zero, alternating extremes (both phases, and minimum against T_MAX), and AWGN
    frames with extremes and zeros strewn in."""
    n, info = code.n(), np.iinfo(dtype)
    tmax = int(info.max)
    alt = np.where(np.arange(n) % 2 == 0, tmax, -tmax)
    rows = [np.full(n, tmax), np.full(n, -tmax), np.full(n, info.min), np.zeros(n), alt, -alt,
            np.where(np.arange(n) % 2 == 0, info.min, tmax), np.where(np.arange(n) % 3 == 0, 0, tmax)]
    noisy = awgn(code, rng, 6, 2.5, dtype, wide=True).astype(np.int64)
    for f in range(6):
        pos = rng.choice(n, size=1 + 7 * f, replace=False)
        noisy[f, pos] = rng.choice([tmax, -tmax, int(info.min), 0, 1, -1], size=len(pos))
    return np.concatenate([np.stack(rows), noisy]).astype(dtype)


def check(code, llrs, maxiters, out, iters, ok, app=None, ref=None):
    r_out, r_it, r_ok, r_app = (ref if ref is not None else fr.decode_fixed(structure(code), llrs, maxiters))[:4]
    assert (np.asarray(ok) == r_ok).all(), f"success differs in frames {np.flatnonzero(np.asarray(ok) != r_ok)[:8]}"
    assert (np.asarray(iters).astype(np.uint32) == r_it).all(), f"iters differ in frames {np.flatnonzero(np.asarray(iters) != r_it)[:8]}"
    assert (np.asarray(out) == r_out).all(), f"output differs in frames {np.flatnonzero((np.asarray(out) != r_out).any(axis=1))[:8]}"
    if app is not None:
        app = np.asarray(app)
        assert app.dtype == np.int32
        assert (app == r_app).all(), f"app differs in frames {np.flatnonzero((app != r_app).any(axis=1))[:8]}"


def both_calls(code, llrs, maxiters, ref=None):
    ref = ref if ref is not None else fr.decode_fixed(structure(code), llrs, maxiters)
    app, out, it, ok = code.decode_ms_layered_fixed_soft_batch(llrs, maxiters)
    check(code, llrs, maxiters, out, it, ok, app, ref=ref)
    out_h, it_h, ok_h = code.decode_ms_layered_fixed_batch(llrs, maxiters)
    check(code, llrs, maxiters, out_h, it_h, ok_h, ref=ref)
    return ref


@pytest.mark.parametrize("code,dtype", CASES, ids=IDS)
def test_awgn_frames_and_iteration_caps(code, dtype):
    rng = np.random.default_rng(700 + int(code))
    F = 24 if code.n() >= 5120 else 48
    saw_none = False
    for i, eb in enumerate(EBN0.get(code, (1.7, 2.5))):
        llrs = awgn(code, rng, F, eb, dtype, wide=(i == 1))
        for m in CAPS:
            saw_none |= not bool(both_calls(code, llrs, m)[4].all())
    assert saw_none                                          # frames without a clamp (test_corner_frames has the saturating ones)


@pytest.mark.parametrize("code,dtype", CASES, ids=IDS)
def test_corner_frames(code, dtype):
    llrs = corner_frames(code, dtype, np.random.default_rng(77 + int(code)))
    clamped = False
    for m in (0, 1, 2, 3, 25):
        clamped |= bool(both_calls(code, llrs, m)[4].any())
    assert clamped                                           # frames of extremes saturate nv


def codewords_per_workgroup(code):
    nt = code.submatrix_size() // (2 if code == LDPCCode.TM8192 else 1)
    return 64 // nt if nt < 64 else 1


@pytest.mark.parametrize("code", [LDPCCode.TC128, LDPCCode.TC256, LDPCCode.TM1280, LDPCCode.TM6144], ids=lambda c: c.name)
@pytest.mark.parametrize("dtype", TYPES, ids=lambda t: np.dtype(t).name)
def test_batch_sizes(code, dtype):
    """0, 1, G - 1, G, G + 1 (G codewords per workgroup: 4 and 2 for TC128 and TC256, else 1) and a few more that leave the last
    group partly empty."""
    g = codewords_per_workgroup(code)
    llrs = awgn(code, np.random.default_rng(21), 2 * g + 7, 2.5, dtype)
    for b in sorted({0, 1, g - 1, g, g + 1, 2 * g + 1, 2 * g + 7} - {-1}):
        app, out, it, ok = code.decode_ms_layered_fixed_soft_batch(llrs[:b], 25)
        assert app.shape == (b, code.n() + code.punctured_bits()) and out.shape == (b, code.output_len())
        check(code, llrs[:b], 25, out, it, ok, app)
        check(code, llrs[:b], 25, *code.decode_ms_layered_fixed_batch(llrs[:b], 25))


@pytest.mark.parametrize("code", [LDPCCode.TC128, LDPCCode.TM2048, LDPCCode.TM8192], ids=lambda c: c.name)
@pytest.mark.parametrize("dtype", TYPES, ids=lambda t: np.dtype(t).name)
def test_memory_modes_streams_device_sets_and_own_buffers(code, dtype):
    import torch
    tdt = torch.int8 if dtype == np.int8 else torch.int16
    llrs = awgn(code, np.random.default_rng(3), 40, 2.0, dtype)
    a = code.decode_ms_layered_fixed_soft_batch(llrs, 25)
    check(code, llrs, 25, *a[1:], a[0])
    b = code.decode_ms_layered_fixed_soft_batch(llrs, 25, devices=[0, 0])
    s = torch.cuda.Stream()
    d = torch.from_numpy(llrs).cuda()
    assert d.dtype == tdt
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        c = code.decode_ms_layered_fixed_soft_batch(d, 25, stream=s.cuda_stream)
        h = code.decode_ms_layered_fixed_batch(d, 25, stream=s.cuda_stream)
    s.synchronize()
    assert c[0].dtype == torch.int32
    c = [t.cpu().numpy() for t in c]
    h = [t.cpu().numpy() for t in h]
    for other in (b, c):
        for x, y in zip(other, a):
            assert (np.asarray(x) == np.asarray(y)).all()
    for x, y in zip(h, a[1:]):
        assert (np.asarray(x) == np.asarray(y)).all()
    hd = code.decode_ms_layered_fixed_batch(llrs, 25, devices=[0, 0])
    for x, y in zip(hd, a[1:]):
        assert (np.asarray(x) == np.asarray(y)).all()
    # caller-supplied result buffers, host and device: the call fills and returns them
    np_len = code.n() + code.punctured_bits()
    own = (np.full((40, np_len), -5, np.int32), np.full((40, code.output_len()), 0xEE, np.uint8), np.full(40, 77, np.uint32),
           np.full(40, 7, np.uint8))
    r = code.decode_ms_layered_fixed_soft_batch(llrs, 25, app=own[0], output=own[1], iters=own[2], success=own[3])
    for x, y, z in zip(r, own, a):
        assert x is y and (y == z).all()
    app_d = torch.full((40, np_len), -5, dtype=torch.int32, device="cuda")
    out = torch.full((40, code.output_len()), 0xEE, dtype=torch.uint8, device="cuda")
    it = torch.full((40,), -2, dtype=torch.int32, device="cuda")
    ok = torch.full((40,), 7, dtype=torch.uint8, device="cuda")
    r = code.decode_ms_layered_fixed_soft_batch(d, 25, app=app_d, output=out, iters=it, success=ok)
    torch.cuda.synchronize()
    for x, y, z in zip(r, (app_d, out, it, ok), a):
        assert x is y and (y.cpu().numpy() == z).all()
    with pytest.raises(ValueError):
        code.decode_ms_layered_fixed_soft_batch(d, 25, app=app_d.to(tdt))          # app is int32, never the LLR type
    # variant 0 is the only kernel; a misaligned device app buffer is refused
    suffix = "i8" if dtype == np.int8 else "i16"
    hard = getattr(la.lib, "labrador_ldpc_decode_ms_layered_fixed_batch_" + suffix)
    soft = getattr(la.lib, "labrador_ldpc_decode_ms_layered_fixed_soft_batch_" + suffix)
    raw = torch.empty(40 * np_len + 16, dtype=torch.int32, device="cuda")
    for variant in (1, 2, 32, 64, 256):
        opts = la.HipOpts(0, la.MEM_DEVICE, torch.cuda.current_stream().cuda_stream, variant, 0, None)
        assert hard(int(code), d.data_ptr(), out.data_ptr(), it.data_ptr(), ok.data_ptr(), 40, 25, ctypes.byref(opts)) == EUNSUPPORTED
    opts = la.HipOpts(0, la.MEM_DEVICE, torch.cuda.current_stream().cuda_stream, 0, 0, None)
    st = soft(int(code), d.data_ptr(), raw.data_ptr() + 4, out.data_ptr(), it.data_ptr(), ok.data_ptr(), 40, 25, ctypes.byref(opts))
    assert st == -1 and "16-byte aligned" in la.last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("code", [LDPCCode.TC256, LDPCCode.TM1536, LDPCCode.TM2048], ids=lambda c: c.name)
@pytest.mark.parametrize("dtype", TYPES, ids=lambda t: np.dtype(t).name)
def test_neighbours_of_a_failing_frame_are_untouched(code, dtype):
    """Frames that cannot converge (pure noise) between frames that do, decoded into the middle of larger prefilled buffers: every
    frame has its own restatement result, and the rows before and after the batch keep their fill."""
    import torch
    rng = np.random.default_rng(0xBAD + int(code))
    F = 25
    good = awgn(code, rng, F, 6.0, dtype)
    noise = rng.integers(-31, 32, size=(F, code.n())).astype(dtype)
    llrs = np.where((np.arange(F) % 3 == 1)[:, None], noise, good)
    ref = fr.decode_fixed(structure(code), llrs, 10)
    assert (ref[2][np.arange(F) % 3 == 1] == 0).all() and (ref[2][np.arange(F) % 3 != 1] == 1).all()
    np_len = code.n() + code.punctured_bits()
    app = torch.full((F + 2, np_len), -5, dtype=torch.int32, device="cuda")
    out = torch.full((F + 2, code.output_len()), 0xEE, dtype=torch.uint8, device="cuda")
    it = torch.full((F + 8,), -2, dtype=torch.int32, device="cuda")
    ok = torch.full((F + 16,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    code.decode_ms_layered_fixed_soft_batch(torch.from_numpy(llrs).cuda(), 10, app=app[1:F + 1], output=out[1:F + 1], iters=it[4:F + 4],
                                            success=ok[8:F + 8])
    torch.cuda.synchronize()
    check(code, llrs, 10, out[1:F + 1].cpu().numpy(), it[4:F + 4].cpu().numpy(), ok[8:F + 8].cpu().numpy(), app[1:F + 1].cpu().numpy(), ref=ref)
    assert bool((app[[0, F + 1]] == -5).all()) and bool((out[[0, F + 1]] == 0xEE).all())
    assert bool((it[:4] == -2).all()) and bool((it[F + 4:] == -2).all()) and bool((ok[:8] == 7).all()) and bool((ok[F + 8:] == 7).all())


@pytest.mark.parametrize("code,dtype", [(c, np.int8) for c in ALL] + [(LDPCCode.TC512, np.int16), (LDPCCode.TM8192, np.int16)],
                         ids=lambda v: v.name if isinstance(v, LDPCCode) else np.dtype(v).name)
def test_persistent_workgroups_decode_many_groups(code, dtype):
    """More codeword groups than the largest grid the launch can have (32 waves per CU, 16 x the resident set without the launch's
    queue), of mixed kinds (converging, failing, extremes, T's minimum, sparse): every frame's app and hard results equal its pool
    entry's restatement result, in two launches back to back and one on another stream, into prefilled buffers; the hard call on
    the same batch gives the same hard results."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nt = code.submatrix_size() // (2 if code == LDPCCode.TM8192 else 1)
    g = codewords_per_workgroup(code)
    wg = nt * g
    queued = wg >= 512
    bound = edge_frames.grid_bound(wg, g, queued, cus)
    maxiters = 20
    rng = np.random.default_rng(0x9F + int(code))
    n, F = code.n(), 12
    info = np.iinfo(dtype)
    conv = awgn(code, rng, F, {0: 5.0, 1: 4.5, 2: 4.0}.get(int(code), 3.5), dtype)
    fail = awgn(code, rng, F, 0.0, dtype)
    big = np.where(rng.random((F, n)) < 0.5, info.max, -info.max).astype(dtype)
    low = awgn(code, rng, F, 3.0, dtype, wide=True)
    for f in range(F):
        low[f, rng.choice(n, size=1 + 3 * f, replace=False)] = info.min
    sparse = np.where(rng.random((F, n)) < 0.8, 0, awgn(code, rng, F, 3.0, dtype)).astype(dtype)
    pool = np.concatenate([conv, fail, big, low, sparse])
    kind = np.repeat(np.arange(5), F)
    ref = fr.decode_fixed(structure(code), pool, maxiters)[:4]
    dref = edge_frames.device_ref(ref)
    frames = bound + bound // 16 + 3
    assert (frames + g - 1) // g > bound // g
    idx = edge_frames.batch_of(pool, kind, frames, g, rng)
    idx_d = torch.from_numpy(idx).cuda()
    d = torch.from_numpy(pool).cuda()[idx_d].contiguous()
    np_len = n + code.punctured_bits()
    tag = f"{code.name} {np.dtype(dtype).name} fixed layered ({'queue' if queued else 'fixed stride'})"

    def sentinels():
        return (torch.full((frames, np_len), -77777, dtype=torch.int32, device="cuda"),
                torch.full((frames, code.output_len()), 0xEE, dtype=torch.uint8, device="cuda"),
                torch.full((frames,), -2, dtype=torch.int32, device="cuda"), torch.full((frames,), 7, dtype=torch.uint8, device="cuda"))

    bufs = [sentinels(), sentinels()]
    torch.cuda.synchronize()
    for b in bufs:
        code.decode_ms_layered_fixed_soft_batch(d, maxiters, app=b[0], output=b[1], iters=b[2], success=b[3])
    h = code.decode_ms_layered_fixed_batch(d, maxiters)
    torch.cuda.synchronize()
    for r, b in enumerate(bufs):
        edge_frames.check_on_device(f"{tag} run {r}", idx_d, b, dref)
    for x, y in zip(bufs[0][1:], h):
        assert torch.equal(x, y), f"{tag}: soft and hard calls differ"
    del bufs, h
    b = sentinels()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        code.decode_ms_layered_fixed_soft_batch(d, maxiters, app=b[0], output=b[1], iters=b[2], success=b[3], stream=s.cuda_stream)
    s.synchronize()
    edge_frames.check_on_device(f"{tag} second stream", idx_d, b, dref)
    del b, d, dref, idx_d
    torch.cuda.empty_cache()


def test_fewer_failures_than_flooding_on_the_same_i8_frames():
    """TM2048 at 1.7 dB, 600 frames quantised at 8 / 31, cap 25: the fixed-point layered kernel fails strictly less often than
    decode_ms_batch on the same i8 frames (34 against 164 in the restatement and the oracle), and equals the restatement."""
    code = LDPCCode.TM2048
    y, _ = oracle.awgn_llrs(code, np.random.default_rng(1700), 600, 1.7, np.float32)
    llrs = quantise(y, np.int8, 8, 31)
    _, _, ok_f = code.decode_ms_batch(llrs, 25)
    out, it, ok_l = code.decode_ms_layered_fixed_batch(llrs, 25)
    print(f"TM2048 1.7 dB i8: flooding failures {(ok_f == 0).sum()}, fixed layered failures {(ok_l == 0).sum()}")
    assert (ok_l == 0).sum() < (ok_f == 0).sum()
    check(code, llrs, 25, out, it, ok_l)
    assert (ok_l == 0).sum() == 34 and (ok_f == 0).sum() == 164


def test_ber_harness_llr_types():
    """python -m labrador_ldpc_amd.perftest --schedule layered --llr {f32,i8,i16}: f32 stays the default, quantised layered decoding
    at 8 / 31 still beats f32 flooding on frames of the same seeds, and the options are checked."""
    from labrador_ldpc_amd import perftest
    code = LDPCCode.TM2048
    kw = dict(maxiters=25, batch=8192, max_bits=8192 * 1024 * 2, max_errors=1 << 40)
    t_f, _, e_f, _, fe_f = perftest.ms_trials(code, 1.7, "ebn0", **kw)
    a = perftest.ms_trials(code, 1.7, "ebn0", schedule="layered", **kw)
    b = perftest.ms_trials(code, 1.7, "ebn0", schedule="layered", llr="f32", **kw)
    assert a == b
    t8, _, e8, _, fe8 = perftest.ms_trials(code, 1.7, "ebn0", schedule="layered", llr="i8", **kw)
    t16, _, e16, _, fe16 = perftest.ms_trials(code, 1.7, "ebn0", schedule="layered", llr="i16", **kw)
    assert t8 == t16 == t_f
    print(f"TM2048 1.7 dB frame errors of {t_f}: f32 flooding {fe_f}, f32 layered {a[4]}, i8 fixed layered {fe8}, i16 {fe16}")
    assert fe8 < fe_f and fe16 < fe_f
    for bad in (dict(llr="i4", schedule="layered"), dict(llr="i8"), dict(llr="i8", schedule="layered", scale=0.8)):
        with pytest.raises(ValueError):
            perftest.ms_trials(code, 1.7, "ebn0", **bad, **kw)
    for t in ("i8", "i16"):
        assert perftest.main(["--code", "TC128", "--snrs", "3.0", "--noise", "ebn0", "--maxiters", "20", "--batch", "4096",
                              "--max-bits", "1e5", "--schedule", "layered", "--llr", t]) == 0
