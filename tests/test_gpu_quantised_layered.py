"""The f32-input forms of the fixed-point layered decoders and of the integer cascade on the GPU
(labrador_ldpc_decode_ms_layered_quantised_{,soft_}batch_{i8,i16}, labrador_ldpc_decode_ms_cascade_quantised_batch_{i8,i16};
LDPCCode.decode_ms_layered_quantised_batch, decode_ms_layered_quantised_soft_batch and decode_ms_cascade_quantised_batch; DESIGN.md
4.11) against the CPU restatement of their contract (tests/quantised_layered_restatement.py) and against the library's own separate
calls, bit for bit in output, iters, success, app and stage: every code and both types, caps 0 / 1 / 25, three triples, AWGN frames,
frames that fail and frames of the quantiser's edge values; batch sizes around the codewords per workgroup; more groups than the
persistent grid holds; host pointers, device pointers, a caller's stream and a repeated device; NaN frames; the cascade with both
chunk sizes lowered; the failure counts of DESIGN.md 4.8 and 4.9; and the BER harness."""
import ctypes
import functools

import numpy as np
import pytest

import cascade_restatement
import edge_frames
import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode
import layered_helpers
import oracle
import quantise_restatement as qr
import quantised_layered_restatement as qlr
from test_gpu_layered_fixed import check, codewords_per_workgroup
from test_gpu_layered_fixed_corrected import EBN0

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -4
BS = 64                                                     # LABRADOR_LDPC_HIP_VARIANT_BITSLICE
NP = qr.NP_DTYPE
PARAMS = {"i8": (8.0, 31), "i16": (64.0, 2047)}
SUFS = ("i8", "i16")
ALL = list(LDPCCode)
CASES = [(c, s) for c in ALL for s in SUFS]
IDS = [f"{c.name}-{s}" for c, s in CASES]
TRIPLES = ((16, 4, 0), (13, 4, 0), (16, 4, 1))


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if la.device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("the GPU tests of the f32-input layered decoders need a gfx950 device")
    torch.cuda.set_device(0)


def host(t):
    import torch
    a = t.cpu().numpy()
    return a.view(np.uint32) if t.dtype == torch.int32 and a.ndim == 1 else a


def keywords(triple):
    return {} if triple is None else dict(scale_num=triple[0], scale_shift=triple[1], offset=triple[2])


def same(got, want, what=""):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        bad = np.flatnonzero((g.astype(np.int64) != w.astype(np.int64)).reshape(len(g), max(1, g.size // max(1, len(g)))).any(axis=1))
        assert not len(bad), f"{what}: result {k} differs in frames {bad[:8].tolist()} ({len(bad)} of {len(g)})"


def edge_rows(code, suf, rng, rows, turn0=0):
    """[rows, n] float32: random values with a third of the quantiser's edge vector over the first 16, the middle 16 and the last 16
    LLRs of every row; the thirds rotate from row to row."""
    scale, lim = PARAMS[suf]
    n = code.n()
    y = (rng.normal(0, 6, (rows, n)) / scale * 8).astype(np.float32)
    edge = qr.edge_vector(scale, lim)
    assert len(edge) <= 48
    mid = (n // 2) & ~15
    for r in range(rows):
        e = np.roll(np.resize(edge, 48), 16 * (turn0 + r))
        y[r, :16], y[r, mid:mid + 16], y[r, -16:] = e[:16], e[16:32], e[32:]
    return y


# ---- 1. the kernels against the restatement -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def kernel_frames(code, suf):
    """the AWGN frames at the code's Eb/N0, four at 0 dB from the same generator, two rows of edge values"""
    rng = np.random.default_rng(5200 + int(code))
    y, _ = oracle.awgn_llrs(code, rng, 24 if code.n() >= 5120 else 48, EBN0[code], np.float32)
    noisy, _ = oracle.awgn_llrs(code, rng, 4, 0.0, np.float32)
    y = np.concatenate([y, noisy, edge_rows(code, suf, np.random.default_rng(5300 + int(code)), 2)])
    y.setflags(write=False)
    return y


@pytest.mark.parametrize("code,suf", CASES, ids=IDS)
def test_kernels_equal_the_restatement(code, suf):
    """The hard and the soft call, host buffers, at caps 0, 1 and 25 and three triples, the identity among them (the plain kernel
    form); at cap 25 the reference has a frame that iterates and succeeds and a frame that fails; and on the device the fused call
    equals quantise_llrs_batch followed by decode_ms_layered_fixed_soft_batch exactly."""
    import torch
    y = kernel_frames(code, suf)
    scale, lim = PARAMS[suf]
    q = qr.quantise(y, NP[suf], scale, lim)
    d = torch.from_numpy(np.array(y)).cuda()
    for triple in TRIPLES:
        for cap in (0, 1, 25):
            ref = qlr.layered_quantised(code, y, NP[suf], scale, lim, cap, triple)
            if cap == 25:
                iterated, failed = int(((ref[2] == 1) & (ref[1] > 0)).sum()), int((ref[2] == 0).sum())
                print(f"{code.name} {suf} {triple}: {iterated} frames succeed after the first sweep, {failed} fail, of {len(y)}")
                assert iterated > 0 and failed > 0
            app, out, it, ok = code.decode_ms_layered_quantised_soft_batch(y, suf, scale, lim, cap, **keywords(triple))
            check(code, q, cap, out, it, ok, app, ref=ref)
            check(code, q, cap, *code.decode_ms_layered_quantised_batch(y, suf, scale, lim, cap, **keywords(triple)), ref=ref)
            fused = code.decode_ms_layered_quantised_soft_batch(d, suf, scale, lim, cap, **keywords(triple))
            two = code.decode_ms_layered_fixed_soft_batch(code.quantise_llrs_batch(d, suf, scale, lim), cap, **keywords(triple))
            torch.cuda.synchronize()
            for a, b in zip(fused, two):
                assert torch.equal(a, b), (triple, cap)


# ---- 2. batch sizes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("code", [LDPCCode.TC128, LDPCCode.TC256, LDPCCode.TM1280], ids=lambda c: c.name)
@pytest.mark.parametrize("suf", SUFS)
def test_batch_sizes(code, suf):
    """0, 1, G - 1, G, G + 1, 2G + 1 and 2G + 7 frames (G codewords per workgroup: 4, 2, 1): the partial last group, whose dead slots
    quantise frame 0's row and drop it.  Device buffers, into prefilled results with a guard row behind them."""
    import torch
    g = codewords_per_workgroup(code)
    scale, lim = PARAMS[suf]
    triple = (13, 4, 1)
    rng = np.random.default_rng(23)
    y, _ = oracle.awgn_llrs(code, rng, 2 * g + 7, 2.5, np.float32)
    y[0] = edge_rows(code, suf, rng, 1)[0]                      # (frame 0 is the row the dead slots read)
    ref = qlr.layered_quantised(code, y, NP[suf], scale, lim, 25, triple)[:4]
    np_len = code.n() + code.punctured_bits()
    for b in sorted({0, 1, g - 1, g, g + 1, 2 * g + 1, 2 * g + 7} - {-1}):
        d = torch.from_numpy(y[:b].copy()).cuda()
        big = (torch.full((b + 1, np_len), -77777, dtype=torch.int32, device="cuda"),
               torch.full((b + 1, code.output_len()), 0xEE, dtype=torch.uint8, device="cuda"),
               torch.full((b + 1,), -2, dtype=torch.int32, device="cuda"), torch.full((b + 1,), 7, dtype=torch.uint8, device="cuda"))
        res = code.decode_ms_layered_quantised_soft_batch(d, suf, scale, lim, 25, app=big[0][:b], output=big[1][:b], iters=big[2][:b],
                                                          success=big[3][:b], **keywords(triple))
        hard = code.decode_ms_layered_quantised_batch(d, suf, scale, lim, 25, **keywords(triple))
        torch.cuda.synchronize()
        assert res[0].shape == (b, np_len) and res[1].shape == (b, code.output_len())
        same((host(res[1]), host(res[2]), host(res[3]), host(res[0])), tuple(x[:b] for x in ref), f"batch {b}")
        same(tuple(host(r) for r in hard), tuple(x[:b] for x in ref[:3]), f"batch {b}, hard")
        assert bool((big[0][b] == -77777).all()) and bool((big[1][b] == 0xEE).all()) and int(big[2][b]) == -2 and int(big[3][b]) == 7


# ---- 3. persistent workgroups ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("code", [LDPCCode.TM8192, LDPCCode.TC512], ids=lambda c: c.name)
def test_persistent_workgroups_decode_many_groups(code):
    """More codeword groups than the largest grid the launch can have -- TM8192 through the launch's queue, TC512 by the fixed stride
    -- so that the loader runs its second and later rounds on reused LDS: frames tiled from a pool of 8 converging, 8 failing and 8
    edge-valued f32 frames, i8 at (13, 4, 0), cap 20; every frame's app and hard results equal its pool entry's reference."""
    import torch
    suf, triple, maxiters = "i8", (13, 4, 0), 20
    scale, lim = PARAMS[suf]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    bound, g, queued = layered_helpers.layered_grid_bound(code, cus)
    assert queued == (code == LDPCCode.TM8192)
    rng = np.random.default_rng(0xB0 + int(code))
    conv, _ = oracle.awgn_llrs(code, rng, 8, 4.0 if code == LDPCCode.TC512 else 3.5, np.float32)
    fail, _ = oracle.awgn_llrs(code, rng, 8, 0.0, np.float32)
    pool = np.concatenate([conv, fail, edge_rows(code, suf, rng, 8)])
    kind = np.arange(len(pool)) % 5                          # (edge_frames.batch_of draws from five kinds)
    ref = qlr.layered_quantised(code, pool, NP[suf], scale, lim, maxiters, triple)[:4]
    assert ref[2][:8].all() and not ref[2][8:16].any()
    dref = edge_frames.device_ref(ref)
    frames = bound + bound // 16 + 3
    assert (frames + g - 1) // g > bound // g
    idx = edge_frames.batch_of(pool, kind, frames, g, rng)
    idx_d = torch.from_numpy(idx).cuda()
    d = torch.from_numpy(pool).cuda()[idx_d].contiguous()
    np_len = code.n() + code.punctured_bits()
    b = (torch.full((frames, np_len), -77777, dtype=torch.int32, device="cuda"),
         torch.full((frames, code.output_len()), 0xEE, dtype=torch.uint8, device="cuda"),
         torch.full((frames,), -2, dtype=torch.int32, device="cuda"), torch.full((frames,), 7, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    code.decode_ms_layered_quantised_soft_batch(d, suf, scale, lim, maxiters, app=b[0], output=b[1], iters=b[2], success=b[3], **keywords(triple))
    h = code.decode_ms_layered_quantised_batch(d, suf, scale, lim, maxiters, **keywords(triple))
    torch.cuda.synchronize()
    edge_frames.check_on_device(f"{code.name} i8 f32-source fixed layered ({'queue' if queued else 'fixed stride'})", idx_d, b, dref)
    for x, z in zip(b[1:], h):
        assert torch.equal(x, z)
    del b, h, d, dref, idx_d
    torch.cuda.empty_cache()


# ---- 4. memory modes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("suf", SUFS)
def test_memory_modes_streams_and_alignment(suf):
    """TM2048: host pointers, device pointers, a caller's stream through the raw symbol, devices=[0, 0]; a device `llrs` one float off
    decodes the same through the layered entries and is EINVAL, with nothing written, through the cascade entry; `output` and `app`
    four bytes off are EINVAL; variant 1 is EUNSUPPORTED on the layered entries."""
    import torch
    code, triple, cap, F = LDPCCode.TM2048, (13, 4, 1), 25, 40
    scale, lim = PARAMS[suf]
    y, _ = oracle.awgn_llrs(code, np.random.default_rng(6), F, 1.7, np.float32)
    q = qr.quantise(y, NP[suf], scale, lim)
    ref = qlr.layered_quantised(code, y, NP[suf], scale, lim, cap, triple)
    a = code.decode_ms_layered_quantised_soft_batch(y, suf, scale, lim, cap, **keywords(triple))                 # host pointers
    check(code, q, cap, *a[1:], a[0], ref=ref)
    a = code.decode_ms_layered_quantised_soft_batch(y, suf, scale, lim, cap, devices=[0, 0], **keywords(triple))  # a repeated device
    check(code, q, cap, *a[1:], a[0], ref=ref)
    check(code, q, cap, *code.decode_ms_layered_quantised_batch(y, suf, scale, lim, cap, devices=[0, 0], **keywords(triple)), ref=ref)
    d = torch.from_numpy(y).cuda()
    c = code.decode_ms_layered_quantised_soft_batch(d, suf, scale, lim, cap, **keywords(triple))                 # device pointers
    torch.cuda.synchronize()
    assert c[0].dtype == torch.int32
    check(code, q, cap, *(t.cpu().numpy() for t in c[1:]), c[0].cpu().numpy(), ref=ref)
    np_len = code.n() + code.punctured_bits()

    def prefilled():
        return (torch.full((F * np_len + 4,), -5, dtype=torch.int32, device="cuda"),
                torch.full((F * code.output_len() + 8,), 0xEE, dtype=torch.uint8, device="cuda"),
                torch.full((F,), -2, dtype=torch.int32, device="cuda"), torch.full((F,), 7, dtype=torch.uint8, device="cuda"),
                torch.full((F,), 9, dtype=torch.uint8, device="cuda"))

    def untouched(bufs):
        torch.cuda.synchronize()
        return all(bool((b == v).all()) for b, v in zip(bufs, (-5, 0xEE, -2, 7, 9)))
    soft_fn = getattr(la.lib, f"labrador_ldpc_decode_ms_layered_quantised_soft_batch_{suf}")
    hard_fn = getattr(la.lib, f"labrador_ldpc_decode_ms_layered_quantised_batch_{suf}")
    casc_fn = getattr(la.lib, f"labrador_ldpc_decode_ms_cascade_quantised_batch_{suf}")
    s = torch.cuda.Stream()
    app, out, it, ok, stage = prefilled()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):                                                                                   # a stream of the caller's
        h = code.decode_ms_layered_quantised_batch(d, suf, scale, lim, cap, stream=s.cuda_stream, **keywords(triple))
        opts = la.HipOpts(0, la.MEM_DEVICE, s.cuda_stream, 0, 0, None)
        st = soft_fn(int(code), d.data_ptr(), app.data_ptr(), out.data_ptr(), it.data_ptr(), ok.data_ptr(), F, cap, scale, lim, *triple,
                     ctypes.byref(opts))
        assert st == 0, la.last_error()
    s.synchronize()
    check(code, q, cap, *(t.cpu().numpy() for t in h), ref=ref)
    check(code, q, cap, out[:F * code.output_len()].view(F, -1).cpu().numpy(), it.cpu().numpy(), ok.cpu().numpy(),
          app[:F * np_len].view(F, np_len).cpu().numpy(), ref=ref)
    # `llrs` one float off: float alignment is all the layered kernels need
    shifted = torch.zeros(F * code.n() + 4, dtype=torch.float32, device="cuda")
    off = shifted[1:1 + F * code.n()].view(F, code.n())
    off.copy_(d)
    assert off.data_ptr() % 16 == 4
    c = code.decode_ms_layered_quantised_soft_batch(off, suf, scale, lim, cap, **keywords(triple))
    torch.cuda.synchronize()
    check(code, q, cap, *(t.cpu().numpy() for t in c[1:]), c[0].cpu().numpy(), ref=ref)
    check(code, q, cap, *(host(t) for t in code.decode_ms_layered_quantised_batch(off, suf, scale, lim, cap, **keywords(triple))), ref=ref)
    # ... and the cascade's streaming quantiser needs 16 bytes
    bufs = prefilled()
    app, out, it, ok, stage = bufs
    opts = la.HipOpts(0, la.MEM_DEVICE, torch.cuda.current_stream().cuda_stream, 0, 0, None)
    st = casc_fn(int(code), off.data_ptr(), out.data_ptr(), it.data_ptr(), ok.data_ptr(), stage.data_ptr(), F, cap, cap, scale, lim, *triple,
                 ctypes.byref(opts))
    assert st == EINVAL and la.last_error() == "device llrs buffer must be 16-byte aligned"
    with pytest.raises(la.LdpcHipError, match="device llrs buffer must be 16-byte aligned"):
        code.decode_ms_cascade_quantised_batch(off, suf, scale, lim, cap)
    # `output` and `app` four bytes off
    for fn, ptrs in ((hard_fn, (d.data_ptr(), out.data_ptr() + 4)), (soft_fn, (d.data_ptr(), app.data_ptr(), out.data_ptr() + 4)),
                     (casc_fn, (d.data_ptr(), out.data_ptr() + 4))):
        tail = (it.data_ptr(), ok.data_ptr()) + ((stage.data_ptr(), F, cap, cap) if fn is casc_fn else (F, cap))
        assert fn(int(code), *ptrs, *tail, scale, lim, *triple, ctypes.byref(opts)) == EINVAL
        assert la.last_error() == "device output buffer must be 8-byte aligned"
    st = soft_fn(int(code), d.data_ptr(), app.data_ptr() + 4, out.data_ptr(), it.data_ptr(), ok.data_ptr(), F, cap, scale, lim, *triple,
                 ctypes.byref(opts))
    assert st == EINVAL and la.last_error() == "device app buffer must be 16-byte aligned"
    # a variant other than 0
    opts = la.HipOpts(0, la.MEM_DEVICE, torch.cuda.current_stream().cuda_stream, 1, 0, None)
    st = hard_fn(int(code), d.data_ptr(), out.data_ptr(), it.data_ptr(), ok.data_ptr(), F, cap, scale, lim, *triple, ctypes.byref(opts))
    assert st == EUNSUPPORTED and "only 0 is" in la.last_error()
    st = soft_fn(int(code), d.data_ptr(), app.data_ptr(), out.data_ptr(), it.data_ptr(), ok.data_ptr(), F, cap, scale, lim, *triple,
                 ctypes.byref(opts))
    assert st == EUNSUPPORTED and "only 0 is" in la.last_error()
    for device in (y, d):
        with pytest.raises(la.LdpcHipError, match="status -4.*only 0 is"):
            code.decode_ms_layered_quantised_batch(device, suf, scale, lim, cap, variant=1)
    assert untouched(bufs)


# ---- 5. NaN frames --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("suf", SUFS)
def test_frames_of_nans_decode_as_all_zero_frames(suf):
    """NaN is an erasure: frames of NaN among ordinary ones give what frames of 0.0 give in their place, through all three methods,
    host and device buffers."""
    import torch
    code = LDPCCode.TM1280
    scale, lim = PARAMS[suf]
    y, _ = oracle.awgn_llrs(code, np.random.default_rng(42), 8, 3.2, np.float32)
    z = y.copy()
    y[[1, 6]] = np.nan
    z[[1, 6]] = 0.0
    for method in (code.decode_ms_layered_quantised_batch, code.decode_ms_layered_quantised_soft_batch, code.decode_ms_cascade_quantised_batch):
        for device in (False, True):
            a, b = (torch.from_numpy(v).cuda() for v in (y, z)) if device else (y, z)
            got, want = method(a, suf, scale, lim, 25, scale_num=13, scale_shift=4), method(b, suf, scale, lim, 25, scale_num=13, scale_shift=4)
            if device:
                torch.cuda.synchronize()
                got, want = tuple(host(t) for t in got), tuple(host(t) for t in want)
            same(got, want, f"NaN frames against zero frames, {method.__name__}")


# ---- 6. the cascade -------------------------------------------------------------------------------------------------------------------
# code: (seed, frames, Eb/N0, cap) of tests/test_gpu_quantise.py's CASES; per type (frames sent to stage 2, failures plain, failures at
# (13, 4, 0)) -- DESIGN.md 4.11's table, the restatement's counts (tests/test_quantised_layered_host.py)
TABLE = {LDPCCode.TC128: ((41, 64, 3.0, 20), {"i8": (3, 2, 2), "i16": (1, 0, 1)}),
         LDPCCode.TM1280: ((42, 48, 3.2, 25), {"i8": (10, 6, 6), "i16": (8, 3, 2)}),
         LDPCCode.TM2048: ((43, 48, 1.9, 25), {"i8": (3, 0, 0), "i16": (3, 0, 0)}),
         LDPCCode.TM8192: ((44, 12, 1.6, 25), {"i8": (6, 0, 0), "i16": (5, 0, 0)})}
CASCADE = [(c, s) for c in TABLE for s in SUFS]


@functools.lru_cache(maxsize=None)
def cascade_frames(code):
    seed, n, snr, _ = TABLE[code][0]
    y, _ = oracle.awgn_llrs(code, np.random.default_rng(seed), n, snr, np.float32)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def cascade_reference(code, suf, triple):
    cap = TABLE[code][0][3]
    ref = qlr.cascade_quantised(code, cascade_frames(code), NP[suf], *PARAMS[suf], cap, cap, triple)
    for x in ref:
        x.setflags(write=False)
    return ref


def cascade_call(code, y, suf, cap, sweeps, triple, device=False, **kw):
    import torch
    scale, lim = PARAMS[suf]
    if not device:
        return code.decode_ms_cascade_quantised_batch(y, suf, scale, lim, cap, max_sweeps=sweeps, **keywords(triple), **kw)
    res = code.decode_ms_cascade_quantised_batch(torch.from_numpy(np.array(y)).cuda(), suf, scale, lim, cap, max_sweeps=sweeps,
                                                 **keywords(triple), **kw)
    torch.cuda.synchronize()
    return tuple(host(r) for r in res)


def separate_calls(code, y, suf, cap, sweeps, triple, variant=0):
    """cascade_restatement.compose over the library's own separate calls on the device: quantise_llrs_batch, decode_ms_batch,
    decode_ms_layered_fixed_batch"""
    import torch
    q = host(code.quantise_llrs_batch(torch.from_numpy(np.array(y)).cuda(), suf, *PARAMS[suf]))

    def on_device(decode):
        def run(llrs, c):
            res = decode(torch.from_numpy(np.ascontiguousarray(llrs)).cuda(), c)
            torch.cuda.synchronize()
            return tuple(host(r) for r in res)
        return run
    return cascade_restatement.compose(on_device(lambda l, c: code.decode_ms_batch(l, c, variant=variant)),
                                       on_device(lambda l, c: code.decode_ms_layered_fixed_batch(l, c, **keywords(triple))), q, cap, sweeps)


@pytest.mark.parametrize("code,suf", CASCADE, ids=[f"{c.name}-{s}" for c, s in CASCADE])
def test_cascade_equals_the_separate_calls_and_the_restatement(code, suf, monkeypatch):
    cap = TABLE[code][0][3]
    y = cascade_frames(code)
    to_stage2, *failures = TABLE[code][1][suf]
    variants = (0, BS) if suf == "i8" and code >= LDPCCode.TM1280 else (0,)
    for triple, want_failed in zip((None, (13, 4, 0)), failures):
        ref = cascade_reference(code, suf, triple)
        print(f"{code.name} {suf} {triple}: {int(ref[3].sum())} frames to stage 2, {int((ref[2] == 0).sum())} failures")
        assert int(ref[3].sum()) == to_stage2 and int((ref[2] == 0).sum()) == want_failed
        for variant in variants:
            separate = separate_calls(code, y, suf, cap, cap, triple, variant)
            same(separate, ref, f"the separate calls against the restatement, {triple}, variant {variant}")
            same(cascade_call(code, y, suf, cap, cap, triple, device=True, variant=variant), separate, f"device buffers, {triple}, variant {variant}")
            same(cascade_call(code, y, suf, cap, cap, triple, variant=variant), separate, f"host buffers, {triple}, variant {variant}")
    triple = (13, 4, 0)
    ref = cascade_reference(code, suf, triple)
    same(cascade_call(code, y, suf, cap, cap, triple, devices=[0, 0]), ref, "host buffers over a repeated device")
    # several chunks with ragged last ones on both levels
    monkeypatch.setenv("LABRADOR_LDPC_HIP_QUANT_CHUNK", "7")
    monkeypatch.setenv("LABRADOR_LDPC_HIP_CASCADE_CHUNK", "2")
    assert len(y) % 7 and len(y) > 7
    same(cascade_call(code, y, suf, cap, cap, triple), ref, "host buffers, chunks of 7 and 2")
    same(cascade_call(code, y, suf, cap, cap, triple, device=True), ref, "device buffers, chunks of 7 and 2")
    # max_iters = 0: every frame goes to stage 2 (chunks of 2 still); max_sweeps = 0: what stage 1 failed is zeroed
    all2 = cascade_call(code, y, suf, 0, cap, triple, device=True)
    assert all2[3].all()
    same(all2[:3], qlr.layered_quantised(code, y, NP[suf], *PARAMS[suf], cap, triple)[:3], "max_iters = 0")
    monkeypatch.delenv("LABRADOR_LDPC_HIP_QUANT_CHUNK")
    monkeypatch.delenv("LABRADOR_LDPC_HIP_CASCADE_CHUNK")
    same(cascade_call(code, y, suf, 0, cap, triple), all2, "max_iters = 0, host buffers")
    for device in (False, True):
        out, it, ok, stage = cascade_call(code, y, suf, cap, 0, triple, device=device)
        assert (stage == ref[3]).all() and stage.any()
        assert not out[stage == 1].any() and not it[stage == 1].any() and not ok[stage == 1].any()
        same(tuple(x[stage == 0] for x in (out, it, ok)), tuple(x[stage == 0] for x in ref[:3]), "max_sweeps = 0")


@pytest.mark.parametrize("suf", SUFS)
def test_cascade_without_a_failure_is_stage_one(suf):
    """TM2048 at 6 dB: flooding decodes every frame, `stage` is all 0 and the results are decode_ms_quantised_batch's."""
    code = LDPCCode.TM2048
    y, _ = oracle.awgn_llrs(code, np.random.default_rng(60), 32, 6.0, np.float32)
    for device in (False, True):
        out, it, ok, stage = cascade_call(code, y, suf, 25, 25, (13, 4, 0), device=device)
        assert not stage.any() and ok.all()
        same((out, it, ok), code.decode_ms_quantised_batch(y, suf, *PARAMS[suf], 25), "6 dB")


def test_two_streams_share_both_workspaces():
    """Two cascade calls by one thread on two streams, different inputs and batch sizes, the second larger so that both workspaces
    grow while the first may still be using them; neither stream is synchronised in between."""
    import torch
    code, suf, triple = LDPCCode.TM2048, "i8", (13, 4, 0)
    cap = TABLE[code][0][3]
    ref = cascade_reference(code, suf, triple)
    y = cascade_frames(code)
    idx = [np.arange(5, 25), np.r_[np.arange(48), np.arange(47, -1, -1), np.arange(0, 48, 2)]]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    d = [torch.from_numpy(np.array(y[i])).cuda() for i in idx]
    torch.cuda.synchronize()
    got = []
    for x, s in zip(d, streams):
        with torch.cuda.stream(s):
            got.append(code.decode_ms_cascade_quantised_batch(x, suf, *PARAMS[suf], cap, stream=s.cuda_stream, **keywords(triple)))
    for s in streams:
        s.synchronize()
    for g, i in zip(got, idx):
        same(tuple(host(r) for r in g), tuple(r[i] for r in ref), f"two streams, {len(i)} frames")


# ---- 7. failure counts ----------------------------------------------------------------------------------------------------------------
def test_failure_counts_on_the_tm2048_frames():
    """The 600 TM2048 frames of default_rng(1700) at 1.7 dB, as f32, at 8 / 31 and cap 25: the layered call leaves 34 failures plain
    and 14 at (13, 4, 0) -- DESIGN.md 4.8's numbers, the quantiser is the same rule -- and the cascade leaves 14 with 164 frames
    decoded by stage 2 (4.9's)."""
    code = LDPCCode.TM2048
    y, _ = oracle.awgn_llrs(code, np.random.default_rng(1700), 600, 1.7, np.float32)
    plain = code.decode_ms_layered_quantised_batch(y, "i8", 8.0, 31, 25)[2]
    scaled = code.decode_ms_layered_quantised_batch(y, "i8", 8.0, 31, 25, scale_num=13, scale_shift=4)[2]
    _, _, ok, stage = code.decode_ms_cascade_quantised_batch(y, "i8", 8.0, 31, 25, scale_num=13, scale_shift=4)
    print(f"TM2048 1.7 dB f32 -> i8: layered failures {(plain == 0).sum()} plain, {(scaled == 0).sum()} at 13/16; cascade "
          f"{(ok == 0).sum()} with {stage.sum()} frames at stage 2")
    assert int((plain == 0).sum()) == 34 and int((scaled == 0).sum()) == 14
    assert int((ok == 0).sum()) == 14 and int(stage.sum()) == 164


# ---- 8. the BER harness ---------------------------------------------------------------------------------------------------------------
def test_ber_harness_runs_from_f32():
    from labrador_ldpc_amd import perftest
    base = ["--code", "TC128", "--snrs", "3.0", "--noise", "ebn0", "--maxiters", "20", "--batch", "4096", "--max-bits", "1e5", "--from-f32"]
    assert perftest.main(base + ["--schedule", "layered", "--llr", "i8", "--fixed-scale", "13/16"]) == 0
    assert perftest.main(base + ["--schedule", "cascade", "--llr", "i16", "--llr-scale", "64", "--llr-lim", "2047", "--fixed-scale", "13/16"]) == 0
