"""Layered min-sum decoding on the GPU (labrador_ldpc_decode_ms_layered_{,soft_}batch_f32, LDPCCode.decode_ms_layered_batch and
decode_ms_layered_soft_batch) against the CPU restatement of the schedule (tests/layered_restatement.py), bit for bit: output, iters
and success exactly, app as values with NaN at the same positions -- for every code, iteration caps 0 / 1 / 2 / 3 / 25, AWGN frames
at several Eb/N0, corner values, both memory modes, a caller's stream, a device set, odd batch sizes and one large device batch.
The flooding call on the same frames still equals the oracle."""
import ctypes

import numpy as np
import pytest

import edge_frames
import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode
from layered_helpers import layered_grid_bound, same_app, structure
import layered_restatement as lr
import oracle

pytestmark = pytest.mark.gpu

ALL = list(LDPCCode)
EUNSUPPORTED = -4
EBN0 = {LDPCCode.TC128: (3.0, 4.5), LDPCCode.TC256: (2.5, 4.0), LDPCCode.TC512: (2.0, 3.0)}
CAPS = (0, 1, 2, 3, 25)


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if la.device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("the layered GPU tests need a gfx950 device")
    torch.cuda.set_device(0)


def frames_per_case(code):
    return 64 if code.n() >= 5120 else 96


def check(code, llrs, maxiters, out, iters, ok, app=None, ref=None):
    r_out, r_it, r_ok, r_app = ref if ref is not None else lr.decode_layered(structure(code), llrs, maxiters)
    assert (np.asarray(ok) == r_ok).all(), f"success differs in frames {np.flatnonzero(np.asarray(ok) != r_ok)[:8]}"
    assert (np.asarray(iters).astype(np.uint32) == r_it).all(), f"iters differ in frames {np.flatnonzero(np.asarray(iters) != r_it)[:8]}"
    assert (np.asarray(out) == r_out).all(), f"output differs in frames {np.flatnonzero((np.asarray(out) != r_out).any(axis=1))[:8]}"
    if app is not None:
        assert same_app(app, r_app)


@pytest.fixture(scope="module")
def awgn_cases():
    """{code: [(ebn0, llrs, {cap: reference})]}, built once (the restatement is the slow part)."""
    cases = {}
    for code in ALL:
        rng = np.random.default_rng(500 + int(code))
        pts = EBN0.get(code, (1.7, 2.0, 2.5))
        cases[code] = []
        for eb in pts:
            llrs, _ = oracle.awgn_llrs(code, rng, frames_per_case(code), eb, np.float32)
            cases[code].append((eb, llrs, {m: lr.decode_layered(structure(code), llrs, m) for m in CAPS}))
    return cases


@pytest.mark.parametrize("code", ALL, ids=lambda c: c.name)
def test_awgn_frames_and_iteration_caps(code, awgn_cases):
    for eb, llrs, refs in awgn_cases[code]:
        for m in CAPS:
            out, it, ok = code.decode_ms_layered_batch(llrs, m)
            check(code, llrs, m, out, it, ok, ref=refs[m])
            app, out_s, it_s, ok_s = code.decode_ms_layered_soft_batch(llrs, m)
            assert (out_s == out).all() and (it_s == it).all() and (ok_s == ok).all()     # the soft call's hard results
            check(code, llrs, m, out_s, it_s, ok_s, app, ref=refs[m])
        # the flooding call on the same frames still equals the oracle
        o_c, it_c, ok_c, _ = oracle.decode_ms_batch(code, llrs, 25)
        out, it, ok = code.decode_ms_batch(llrs, 25)
        assert (out == o_c).all() and (it == it_c).all() and (ok == ok_c).all()


def corner_frames(code, rng, frames=6):
    llrs, _ = oracle.awgn_llrs(code, rng, frames, 3.0, np.float32)
    n = code.n()
    fi = np.finfo(np.float32)
    specials = np.array([np.inf, -np.inf, 0.0, -0.0, fi.tiny / 4, -fi.tiny / 4, fi.max, -fi.max, np.nan], dtype=np.float32)
    neg_nan = np.array([np.nan], dtype=np.float32)
    neg_nan.view(np.uint32)[0] |= 1 << 31
    specials = np.concatenate([specials, neg_nan])
    for f in range(1, frames):
        pos = rng.choice(n, size=1 + f * 3, replace=False)
        llrs[f, pos] = rng.choice(specials, size=len(pos))
    llrs[frames - 1, :] = np.nan
    return llrs


@pytest.mark.parametrize("code", ALL, ids=lambda c: c.name)
def test_corner_values(code):
    """+-inf, +-0.0, denormals, +-FLT_MAX and NaN LLRs (both signs of NaN, and a frame of NaNs only)."""
    llrs = corner_frames(code, np.random.default_rng(77 + int(code)))
    for m in (0, 3, 25):
        app, out, it, ok = code.decode_ms_layered_soft_batch(llrs, m)
        check(code, llrs, m, out, it, ok, app)
        out_h, it_h, ok_h = code.decode_ms_layered_batch(llrs, m)
        assert (out == out_h).all() and (it == it_h).all() and (ok == ok_h).all()
        if m:
            assert (np.isnan(app[:, : code.n()]) == np.isnan(llrs)).all()


@pytest.mark.parametrize("code", ALL, ids=lambda c: c.name)
def test_nan_llr_gives_the_results_of_inf(code):
    rng = np.random.default_rng(9 + int(code))
    llrs, _ = oracle.awgn_llrs(code, rng, 8, 2.5, np.float32)
    for f in range(8):
        llrs[f, rng.choice(code.n(), size=1 + 5 * f, replace=False)] = np.nan
    inf = np.where(np.isnan(llrs), np.float32(np.inf), llrs)
    for m in (2, 25):
        a = code.decode_ms_layered_batch(llrs, m)
        b = code.decode_ms_layered_batch(inf, m)
        for x, y in zip(a, b):
            assert (x == y).all()


@pytest.mark.parametrize("code", [LDPCCode.TC128, LDPCCode.TM2048, LDPCCode.TM8192], ids=lambda c: c.name)
def test_memory_modes_streams_and_device_sets(code):
    import torch
    rng = np.random.default_rng(3)
    llrs, _ = oracle.awgn_llrs(code, rng, 40, 2.0, np.float32)
    a = code.decode_ms_layered_soft_batch(llrs, 25)
    check(code, llrs, 25, *a[1:], a[0])
    b = code.decode_ms_layered_soft_batch(llrs, 25, devices=[0, 0])
    s = torch.cuda.Stream()
    d = torch.from_numpy(llrs).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        c = code.decode_ms_layered_soft_batch(d, 25, stream=s.cuda_stream)
        h = code.decode_ms_layered_batch(d, 25, stream=s.cuda_stream)
    s.synchronize()
    c = [t.cpu().numpy() for t in c]
    h = [t.cpu().numpy() for t in h]
    for other in (b, c):
        assert same_app(other[0], a[0])
        for x, y in zip(other[1:], a[1:]):
            assert (np.asarray(x) == np.asarray(y)).all()
    for x, y in zip(h, a[1:]):
        assert (np.asarray(x) == np.asarray(y)).all()
    hd = code.decode_ms_layered_batch(llrs, 25, devices=[0, 0])
    for x, y in zip(hd, a[1:]):
        assert (np.asarray(x) == np.asarray(y)).all()
    # variant 0 is the only kernel; a misaligned device app buffer is refused
    np_len = code.n() + code.punctured_bits()
    out = torch.empty((40, code.output_len()), dtype=torch.uint8, device="cuda")
    it = torch.empty(40, dtype=torch.int32, device="cuda")
    ok = torch.empty(40, dtype=torch.uint8, device="cuda")
    raw = torch.empty(40 * np_len + 16, dtype=torch.float32, device="cuda")
    for variant in (1, 2, 32, 256):
        opts = la.HipOpts(0, la.MEM_DEVICE, torch.cuda.current_stream().cuda_stream, variant, 0, None)
        st = la.lib.labrador_ldpc_decode_ms_layered_batch_f32(int(code), d.data_ptr(), out.data_ptr(), it.data_ptr(), ok.data_ptr(), 40, 25,
                                                              ctypes.byref(opts))
        assert st == EUNSUPPORTED
    opts = la.HipOpts(0, la.MEM_DEVICE, torch.cuda.current_stream().cuda_stream, 0, 0, None)
    st = la.lib.labrador_ldpc_decode_ms_layered_soft_batch_f32(int(code), d.data_ptr(), raw.data_ptr() + 4, out.data_ptr(), it.data_ptr(),
                                                               ok.data_ptr(), 40, 25, ctypes.byref(opts))
    assert st == -1 and "16-byte aligned" in la.last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("code", [LDPCCode.TC128, LDPCCode.TC256, LDPCCode.TM1280, LDPCCode.TM6144], ids=lambda c: c.name)
def test_batch_sizes(code):
    """Batch 1 and batches that do not fill the last workgroup (the TC codes hold 64 / M codewords per workgroup)."""
    rng = np.random.default_rng(21)
    llrs, _ = oracle.awgn_llrs(code, rng, 11, 2.5, np.float32)
    for b in (1, 3, 5, 11):
        app, out, it, ok = code.decode_ms_layered_soft_batch(llrs[:b], 25)
        check(code, llrs[:b], 25, out, it, ok, app)


def test_large_device_batch():
    """262 144 device-resident TM2048 frames at 2 dB: a sample against the restatement, and the host call on the same frames gives
    the same results (digests of the device results equal the host results')."""
    import hashlib
    import torch
    code = LDPCCode.TM2048
    F = 262144
    rng = np.random.default_rng(2024)
    pool = np.stack([oracle.copy_encode(code, rng.integers(0, 256, code.k() // 8, dtype=np.uint8)) for _ in range(64)])
    sigma = float(np.sqrt(1.0 / (2.0 * (code.k() / code.n()) * 10.0 ** (2.0 / 10.0))))
    x = code.awgn_frames(torch.from_numpy(pool).cuda(), F, sigma, 2024, "f32")
    out, it, ok = code.decode_ms_layered_batch(x, 25)
    torch.cuda.synchronize()
    xh = x.cpu().numpy()
    outc, itc, okc = out.cpu().numpy(), it.cpu().numpy().astype(np.uint32), ok.cpu().numpy()
    oh, ih, kh = code.decode_ms_layered_batch(xh, 25)
    digest = lambda *a: hashlib.sha256(b"".join(np.ascontiguousarray(v).tobytes() for v in a)).hexdigest()     # noqa: E731
    assert digest(outc, itc, okc) == digest(oh, ih.astype(np.uint32), kh)
    sample = sorted({0, 1, F // 2, F - 1} | set(np.flatnonzero(okc == 0)[:8].tolist()) | set(range(100, 124)))
    check(code, xh[sample], 25, outc[sample], itc[sample], okc[sample])
    del x, out, it, ok
    torch.cuda.empty_cache()


def test_layered_beats_flooding_on_the_gpu():
    """The algorithmic point of the schedule, on the kernels themselves: at 25 iterations and 1.7 dB, TM2048 fails less often and
    takes fewer passes per frame under the layered schedule than under flooding."""
    code = LDPCCode.TM2048
    llrs, _ = oracle.awgn_llrs(code, np.random.default_rng(1700), 2000, 1.7, np.float32)
    _, it_f, ok_f = code.decode_ms_batch(llrs, 25)
    _, it_l, ok_l = code.decode_ms_layered_batch(llrs, 25)
    assert (ok_l == 0).sum() < (ok_f == 0).sum()
    # passes: flooding's iteration index counts the check at iteration 0 (the LLRs themselves); a layered sweep is a pass
    passes_f = np.where(ok_f == 1, it_f.astype(np.int64), 25).mean()
    passes_l = np.where(ok_l == 1, it_l.astype(np.int64) + 1, 25).mean()
    assert passes_l < passes_f


def test_ber_harness_schedule_switch():
    """python -m labrador_ldpc_amd.perftest --schedule {flooding,layered}: the same frames through both decoders; the layered curve
    lies at or below the flooding one, and flooding stays the default."""
    from labrador_ldpc_amd import perftest
    code = LDPCCode.TM2048
    kw = dict(maxiters=25, batch=8192, max_bits=8192 * 1024 * 2, max_errors=1 << 40)
    t_f, _, e_f, _, fe_f = perftest.ms_trials(code, 1.7, "ebn0", **kw)
    t_d, _, e_d, _, fe_d = perftest.ms_trials(code, 1.7, "ebn0", schedule="flooding", **kw)
    t_l, _, e_l, _, fe_l = perftest.ms_trials(code, 1.7, "ebn0", schedule="layered", **kw)
    assert (t_f, e_f, fe_f) == (t_d, e_d, fe_d) and t_l == t_f
    assert fe_l < fe_f
    with pytest.raises(ValueError):
        perftest.ms_trials(code, 1.7, "ebn0", schedule="nope", **kw)
    assert perftest.main(["--code", "TC128", "--snrs", "3.0", "--noise", "ebn0", "--maxiters", "20", "--batch", "4096",
                          "--max-bits", "1e5", "--schedule", "layered"]) == 0


def layered_calls(code, llrs, maxiters, ref=None):
    """Soft and hard layered calls on the same frames against the restatement (check() compares the soft call's app too)."""
    ref = ref if ref is not None else lr.decode_layered(structure(code), llrs, maxiters)
    app, out, it, ok = code.decode_ms_layered_soft_batch(llrs, maxiters)
    check(code, llrs, maxiters, out, it, ok, app, ref=ref)
    out_h, it_h, ok_h = code.decode_ms_layered_batch(llrs, maxiters)
    check(code, llrs, maxiters, out_h, it_h, ok_h, ref=ref)
    return ref


@pytest.mark.parametrize("code", ALL, ids=lambda c: c.name)
def test_whole_frame_extremes(code):
    """All +-0.0, every third / fifth zero, denormal frames, sums of finite LLRs that overflow to +-inf, +-inf runs and +-FLT_MAX
    frames, at caps 1, 3, 25 and 60: a +inf marginal of finite LLRs stays +inf in app."""
    llrs = edge_frames.whole_frame_rows(code, np.float32, np.random.default_rng(0xF4B + int(code)))
    saw_inf = False
    for m in (1, 3, 25, 60):
        ref = layered_calls(code, llrs, m)
        saw_inf |= bool(np.isinf(ref[3][[5, 8]]).any())
    assert saw_inf


@pytest.mark.parametrize("code", ALL, ids=lambda c: c.name)
def test_failing_frames_at_long_caps(code):
    """Frames that keep failing (0 and 1 dB) next to ones that converge late, at caps 50 and 100."""
    rng = np.random.default_rng(0x1A7 + int(code))
    F = 4 if code.n() >= 5120 else 6
    llrs = np.concatenate([oracle.awgn_llrs(code, rng, F, e, np.float32)[0] for e in (0.0, 1.0, 2.0)])
    for m in (50, 100):
        _, it, ok, _ = layered_calls(code, llrs, m)
        assert (ok == 0).any() and (it[ok == 0] == m).all()


@pytest.mark.parametrize("code", ALL, ids=lambda c: c.name)
def test_persistent_workgroups_decode_many_groups(code):
    """More codeword groups than the largest grid the launch can have -- the queue-fed kernels (TM2048, TM5120, TM6144, TM8192) and the
    fixed-stride ones (the TC codes, TM1280, TM1536) -- of mixed kinds (converging, failing, overflowing, NaN, +-FLT_MAX): every frame's
    app and hard results equal its pool entry's restatement result, in two launches back to back and one on another stream, into
    prefilled buffers; the hard call on the same batch gives the same hard results."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    bound, g, queued = layered_grid_bound(code, cus)
    maxiters = 20
    rng = np.random.default_rng(0x9F + int(code))
    n, F = code.n(), 12
    conv = oracle.awgn_llrs(code, rng, F, {0: 5.0, 1: 4.5, 2: 4.0}.get(int(code), 3.5), np.float32)[0]
    fail = oracle.awgn_llrs(code, rng, F, 0.0, np.float32)[0]
    over = oracle.awgn_llrs(code, rng, F, 2.0, np.float32)[0] * np.float32(1e37)
    nan = oracle.awgn_llrs(code, rng, F, 3.0, np.float32)[0]
    for f in range(F):
        nan[f, rng.choice(n, size=1 + 3 * f, replace=False)] = np.nan
    big = np.where(rng.random((F, n)) < 0.5, np.finfo(np.float32).max, -np.finfo(np.float32).max).astype(np.float32)
    pool = np.concatenate([conv, fail, over, nan, big])
    kind = np.repeat(np.arange(5), F)
    ref = lr.decode_layered(structure(code), pool, maxiters)
    dref = edge_frames.device_ref(ref)
    frames = bound + bound // 16 + 3
    assert (frames + g - 1) // g > bound // g
    idx = edge_frames.batch_of(pool, kind, frames, g, rng)
    idx_d = torch.from_numpy(idx).cuda()
    d = torch.from_numpy(pool).cuda()[idx_d].contiguous()
    np_len = n + code.punctured_bits()
    tag = f"{code.name} layered ({'queue' if queued else 'fixed stride'})"

    def sentinels():
        return (torch.full((frames, np_len), -7.0e30, dtype=torch.float32, device="cuda"),
                torch.full((frames, code.output_len()), 0xEE, dtype=torch.uint8, device="cuda"),
                torch.full((frames,), -2, dtype=torch.int32, device="cuda"), torch.full((frames,), 7, dtype=torch.uint8, device="cuda"))

    bufs = [sentinels(), sentinels()]
    torch.cuda.synchronize()
    for b in bufs:
        code.decode_ms_layered_soft_batch(d, maxiters, app=b[0], output=b[1], iters=b[2], success=b[3])
    h = code.decode_ms_layered_batch(d, maxiters)
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
        code.decode_ms_layered_soft_batch(d, maxiters, app=b[0], output=b[1], iters=b[2], success=b[3], stream=s.cuda_stream)
    s.synchronize()
    edge_frames.check_on_device(f"{tag} second stream", idx_d, b, dref)
    del b, d, dref, idx_d
    torch.cuda.empty_cache()
