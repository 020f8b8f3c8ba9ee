"""Fixed-point layered min-sum decoding with normalized / offset check messages on the GPU
(labrador_ldpc_decode_ms_layered_fixed_corrected_{,soft_}batch_{i8,i16}; the scale_num / scale_shift / offset keywords of
LDPCCode.decode_ms_layered_fixed_batch and decode_ms_layered_fixed_soft_batch) against the CPU restatement of the contract
(tests/layered_fixed_corrected_restatement.py), bit for bit: output, iters, success and the int32 app -- for every code
and both types, iteration caps 0 / 1 / 2 / 25, AWGN and corner frames, four parameter triples; the identity triple against the plain
fixed-point calls; batch sizes around the codewords per workgroup; more groups than the persistent grid holds on the queue and on the
stride path; host pointers, device pointers and a caller's stream; fewer failed frames than plain decoding; and the BER harness."""
import ctypes

import numpy as np
import pytest

import edge_frames
import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode
import layered_fixed_corrected_restatement as fcr
import layered_fixed_restatement as fr
import layered_helpers
from layered_helpers import quantise
import oracle
from test_gpu_layered_fixed import awgn, check, codewords_per_workgroup, corner_frames

pytestmark = pytest.mark.gpu

ALL = list(LDPCCode)
TYPES = (np.int8, np.int16)
CAPS = (0, 1, 2, 25)
CASES = [(c, t) for c in ALL for t in TYPES]
IDS = [f"{c.name}-{np.dtype(t).name}" for c, t in CASES]
# per code, an Eb/N0 at which some frames decode after a few sweeps and some fail
EBN0 = {LDPCCode.TC128: 3.0, LDPCCode.TC256: 2.5, LDPCCode.TC512: 2.0, LDPCCode.TM1280: 3.5, LDPCCode.TM1536: 2.5, LDPCCode.TM2048: 1.7,
        LDPCCode.TM5120: 3.2, LDPCCode.TM6144: 2.2, LDPCCode.TM8192: 1.7}


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if la.device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("the corrected fixed-point layered GPU tests need a gfx950 device")
    torch.cuda.set_device(0)


def structure(code):
    return layered_helpers.structure(code, fr.Structure)


def keywords(triple):
    return dict(scale_num=triple[0], scale_shift=triple[1], offset=triple[2])


def both_calls(code, llrs, maxiters, triple):
    ref = fcr.decode_fixed_corrected(structure(code), llrs, maxiters, *triple)
    app, out, it, ok = code.decode_ms_layered_fixed_soft_batch(llrs, maxiters, **keywords(triple))
    check(code, llrs, maxiters, out, it, ok, app, ref=ref)
    check(code, llrs, maxiters, *code.decode_ms_layered_fixed_batch(llrs, maxiters, **keywords(triple)), ref=ref)
    return ref


@pytest.mark.parametrize("code,dtype", CASES, ids=IDS)
def test_kernels_equal_the_restatement(code, dtype):
    """24 AWGN frames for n >= 5120, otherwise 48, at 8 / 31, and the corner frames of test_gpu_layered_fixed.py; the hard and the
    soft call; caps 0, 1, 2 and 25; a scale, an offset, the smallest scale and the largest offset."""
    rng = np.random.default_rng(4800 + int(code))
    tmax = int(np.iinfo(dtype).max)
    llrs = np.concatenate([awgn(code, rng, 24 if code.n() >= 5120 else 48, EBN0[code], dtype), corner_frames(code, dtype, rng)])
    stopped_early = differs = False
    for triple in ((13, 4, 0), (16, 4, 1), (1, 8, 0), (1, 0, tmax)):
        for m in CAPS:
            ref = both_calls(code, llrs, m, triple)
            stopped_early |= m == 25 and bool(((ref[2] == 1) & (ref[1] > 0)).any())
            if m == 25 and triple == (13, 4, 0):
                differs = any((x != y).any() for x, y in zip(ref[:4], fr.decode_fixed(structure(code), llrs, m)[:4]))
    assert stopped_early and differs                         # (frames that iterate, and a correction that changes something)


@pytest.mark.parametrize("code,dtype", CASES, ids=IDS)
def test_the_identity_triple_equals_the_plain_calls(code, dtype):
    """(16, 4, 0) through the corrected kernels against decode_ms_layered_fixed_{,soft_}batch on the same device buffers: exactly
    equal, app included."""
    import torch
    rng = np.random.default_rng(4900 + int(code))
    llrs = np.concatenate([awgn(code, rng, 24, 2.0, dtype), corner_frames(code, dtype, rng)])
    d = torch.from_numpy(llrs).cuda()
    for m in (0, 1, 25):
        plain = code.decode_ms_layered_fixed_soft_batch(d, m)
        same = code.decode_ms_layered_fixed_soft_batch(d, m, scale_num=16, scale_shift=4, offset=0)
        hard = code.decode_ms_layered_fixed_batch(d, m, scale_shift=4)
        torch.cuda.synchronize()
        for x, y in zip(plain, same):
            assert torch.equal(x, y), m
        for x, y in zip(plain[1:], hard):
            assert torch.equal(x, y), m


@pytest.mark.parametrize("code", [LDPCCode.TC128, LDPCCode.TC256, LDPCCode.TM1280], ids=lambda c: c.name)
@pytest.mark.parametrize("dtype", TYPES, ids=lambda t: np.dtype(t).name)
def test_batch_sizes(code, dtype):
    """0, 1, G - 1, G, G + 1 (G codewords per workgroup: 4 and 2 for TC128 and TC256, else 1) and two that leave the last group partly
    empty."""
    g = codewords_per_workgroup(code)
    triple = (13, 4, 1)
    llrs = awgn(code, np.random.default_rng(22), 2 * g + 7, 2.5, dtype)
    ref = fcr.decode_fixed_corrected(structure(code), llrs, 25, *triple)
    for b in sorted({0, 1, g - 1, g, g + 1, 2 * g + 1, 2 * g + 7} - {-1}):
        part = tuple(x[:b] for x in ref)
        app, out, it, ok = code.decode_ms_layered_fixed_soft_batch(llrs[:b], 25, **keywords(triple))
        assert app.shape == (b, code.n() + code.punctured_bits()) and out.shape == (b, code.output_len())
        check(code, llrs[:b], 25, out, it, ok, app, ref=part)
        check(code, llrs[:b], 25, *code.decode_ms_layered_fixed_batch(llrs[:b], 25, **keywords(triple)), ref=part)


@pytest.mark.parametrize("code", [LDPCCode.TM8192, LDPCCode.TC512], ids=lambda c: c.name)
def test_persistent_workgroups_decode_many_groups(code):
    """More codeword groups than the largest grid the launch can have -- TM8192 through the launch's queue, TC512 by the fixed stride
    -- from a small pool of frames of mixed kinds (converging, failing, extremes, T's minimum, sparse) tiled: every frame's app and
    hard results equal its pool entry's restatement result, into prefilled buffers; the hard call on the same batch gives the same
    hard results.  i8 at (13, 4, 0)."""
    import torch
    dtype, triple, maxiters = np.int8, (13, 4, 0), 20
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    bound, g, queued = layered_helpers.layered_grid_bound(code, cus)
    assert queued == (code == LDPCCode.TM8192)
    rng = np.random.default_rng(0xA0 + int(code))
    n, F = code.n(), 8
    info = np.iinfo(dtype)
    conv = awgn(code, rng, F, 4.0 if code == LDPCCode.TC512 else 3.5, dtype)
    fail = awgn(code, rng, F, 0.0, dtype)
    big = np.where(rng.random((F, n)) < 0.5, info.max, -info.max).astype(dtype)
    low = awgn(code, rng, F, 3.0, dtype)
    for f in range(F):
        low[f, rng.choice(n, size=1 + 3 * f, replace=False)] = info.min
    sparse = np.where(rng.random((F, n)) < 0.8, 0, awgn(code, rng, F, 3.0, dtype)).astype(dtype)
    pool = np.concatenate([conv, fail, big, low, sparse])
    kind = np.repeat(np.arange(5), F)                        # (edge_frames.batch_of draws from five kinds)
    ref = fcr.decode_fixed_corrected(structure(code), pool, maxiters, *triple)[:4]
    dref = edge_frames.device_ref(ref)
    frames = bound + bound // 16 + 3
    assert (frames + g - 1) // g > bound // g
    idx = edge_frames.batch_of(pool, kind, frames, g, rng)
    idx_d = torch.from_numpy(idx).cuda()
    d = torch.from_numpy(pool).cuda()[idx_d].contiguous()
    np_len = n + code.punctured_bits()
    b = (torch.full((frames, np_len), -77777, dtype=torch.int32, device="cuda"),
         torch.full((frames, code.output_len()), 0xEE, dtype=torch.uint8, device="cuda"),
         torch.full((frames,), -2, dtype=torch.int32, device="cuda"), torch.full((frames,), 7, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    code.decode_ms_layered_fixed_soft_batch(d, maxiters, app=b[0], output=b[1], iters=b[2], success=b[3], **keywords(triple))
    h = code.decode_ms_layered_fixed_batch(d, maxiters, **keywords(triple))
    torch.cuda.synchronize()
    edge_frames.check_on_device(f"{code.name} i8 corrected fixed layered ({'queue' if queued else 'fixed stride'})", idx_d, b, dref)
    for x, y in zip(b[1:], h):
        assert torch.equal(x, y)
    del b, h, d, dref, idx_d
    torch.cuda.empty_cache()


@pytest.mark.parametrize("dtype", TYPES, ids=lambda t: np.dtype(t).name)
def test_memory_modes_and_streams(dtype):
    """TM2048: host pointers, device pointers on the current stream, and device pointers on a stream of the caller's, the raw symbol
    included: all equal the restatement."""
    import torch
    code, triple = LDPCCode.TM2048, (13, 4, 1)
    llrs = awgn(code, np.random.default_rng(5), 40, 1.7, dtype)
    ref = fcr.decode_fixed_corrected(structure(code), llrs, 25, *triple)
    a = code.decode_ms_layered_fixed_soft_batch(llrs, 25, **keywords(triple))                    # host pointers
    check(code, llrs, 25, *a[1:], a[0], ref=ref)
    d = torch.from_numpy(llrs).cuda()
    c = code.decode_ms_layered_fixed_soft_batch(d, 25, **keywords(triple))                       # device pointers
    torch.cuda.synchronize()
    assert c[0].dtype == torch.int32
    check(code, llrs, 25, *(t.cpu().numpy() for t in c[1:]), c[0].cpu().numpy(), ref=ref)
    s = torch.cuda.Stream()
    np_len = code.n() + code.punctured_bits()
    app = torch.full((40, np_len), -5, dtype=torch.int32, device="cuda")
    out = torch.full((40, code.output_len()), 0xEE, dtype=torch.uint8, device="cuda")
    it = torch.full((40,), -2, dtype=torch.int32, device="cuda")
    ok = torch.full((40,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):                                                                   # a stream of the caller's
        h = code.decode_ms_layered_fixed_batch(d, 25, stream=s.cuda_stream, **keywords(triple))
        fn = getattr(la.lib, "labrador_ldpc_decode_ms_layered_fixed_corrected_soft_batch_" + ("i8" if dtype == np.int8 else "i16"))
        opts = la.HipOpts(0, la.MEM_DEVICE, s.cuda_stream, 0, 0, None)
        st = fn(int(code), d.data_ptr(), app.data_ptr(), out.data_ptr(), it.data_ptr(), ok.data_ptr(), 40, 25, *triple, ctypes.byref(opts))
        assert st == 0, la.last_error()
    s.synchronize()
    check(code, llrs, 25, *(t.cpu().numpy() for t in h), ref=ref)
    check(code, llrs, 25, out.cpu().numpy(), it.cpu().numpy(), ok.cpu().numpy(), app.cpu().numpy(), ref=ref)


def test_fewer_failures_than_plain_on_the_same_i8_frames():
    """TM2048 at 1.7 dB, 600 frames of default_rng(1700) quantised at 8 / 31, cap 25: the kernel at (13, 4, 0) leaves strictly fewer
    failed frames than the plain fixed-point kernel (14 against 34 in the restatements), and both equal their restatements."""
    code = LDPCCode.TM2048
    y, _ = oracle.awgn_llrs(code, np.random.default_rng(1700), 600, 1.7, np.float32)
    llrs = quantise(y, np.int8, 8, 31)
    out_p, it_p, ok_p = code.decode_ms_layered_fixed_batch(llrs, 25)
    out_c, it_c, ok_c = code.decode_ms_layered_fixed_batch(llrs, 25, scale_num=13, scale_shift=4)
    print(f"TM2048 1.7 dB i8: plain fixed layered failures {(ok_p == 0).sum()}, at 13/16 {(ok_c == 0).sum()}")
    assert (ok_c == 0).sum() < (ok_p == 0).sum()
    check(code, llrs, 25, out_p, it_p, ok_p)
    check(code, llrs, 25, out_c, it_c, ok_c, ref=fcr.decode_fixed_corrected(structure(code), llrs, 25, 13, 4, 0))


def test_ber_harness_runs_with_a_fixed_scale():
    from labrador_ldpc_amd import perftest
    assert perftest.main(["--code", "TC128", "--snrs", "3.0", "--noise", "ebn0", "--maxiters", "20", "--batch", "4096", "--max-bits", "1e5",
                          "--schedule", "layered", "--llr", "i8", "--fixed-scale", "13/16"]) == 0
    assert perftest.main(["--code", "TC128", "--snrs", "3.0", "--noise", "ebn0", "--maxiters", "20", "--batch", "4096", "--max-bits", "1e5",
                          "--schedule", "layered", "--llr", "i16", "--fixed-scale", "16/16", "--fixed-offset", "1"]) == 0
