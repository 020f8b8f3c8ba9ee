"""The two-stage ("cascade") decode on the GPU (labrador_ldpc_decode_ms_cascade_batch_{f32,i8,i16}; LDPCCode.decode_ms_cascade_batch and
decode_ms_cascade_fixed_batch) against its contract: per frame, exactly the composition of the library's own unchanged
entries called separately -- decode_ms_batch, then the layered decoder of the type on the frames it failed -- put together in numpy
(tests/cascade_restatement.compose), and for TC128, TM1280 and TM2048 also the CPU restatement.  Every comparison is exact equality of
output, iters, success and stage."""
import ctypes
import functools

import numpy as np
import pytest

import cascade_restatement as cr
import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode
from layered_helpers import quantise
import oracle

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -4
ALL = list(LDPCCode)
TYPES = (np.float32, np.int8, np.int16)
CASES = [(c, t) for c in ALL for t in TYPES]
IDS = [f"{c.name}-{np.dtype(t).name}" for c, t in CASES]
# an Eb/N0 per code at which a few flooding iterations decode some frames and the layered decoder rescues some of the rest
MID = {LDPCCode.TC128: 3.5, LDPCCode.TC256: 3.0, LDPCCode.TC512: 2.5, LDPCCode.TM1280: 3.5, LDPCCode.TM1536: 2.8, LDPCCode.TM2048: 2.0,
       LDPCCode.TM5120: 3.3, LDPCCode.TM6144: 2.6, LDPCCode.TM8192: 1.9}
SWEEPS = 25
CPU_CODES = (LDPCCode.TC128, LDPCCode.TM1280, LDPCCode.TM2048)


def cap1(code):
    return 4 if code <= LDPCCode.TC512 else 6


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if la.device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("the cascade GPU tests need a gfx950 device")
    torch.cuda.set_device(0)


@functools.lru_cache(maxsize=None)
def pool(code, dtype):
    """48 frames: 16 at 7 dB, 16 at MID dB, 16 of noise alone; the integer types quantised at 8 / 31."""
    rng = np.random.default_rng(4100 + int(code))
    y = np.concatenate([oracle.awgn_llrs(code, rng, 16, 7.0, np.float32)[0], oracle.awgn_llrs(code, rng, 16, MID[code], np.float32)[0],
                        rng.standard_normal((16, code.n())).astype(np.float32)])
    y = y if dtype == np.float32 else quantise(y, dtype, 8, 31)
    y.setflags(write=False)
    return y


def separate(code, correction=None, variant=0):
    """The library's own two entries as functions of (llrs, cap), for cascade_restatement.compose."""
    def second(llrs, cap):
        if llrs.dtype == np.float32:
            scale, offset = correction or (1.0, 0.0)
            return code.decode_ms_layered_batch(llrs, cap, scale=scale, offset=offset)
        num, shift, offset = correction or (None, None, None)
        return code.decode_ms_layered_fixed_batch(llrs, cap, scale_num=num, scale_shift=shift, offset=offset)
    return (lambda llrs, cap: code.decode_ms_batch(llrs, cap, variant=variant)), second


def composed(code, llrs, max_iters, max_sweeps, correction=None, variant=0):
    return cr.compose(*separate(code, correction, variant), llrs, max_iters, max_sweeps)


@functools.lru_cache(maxsize=None)
def pool_results(code, dtype):
    """(the composition on the pool at the test caps, plain min-sum; the class of every pool frame: 0 decoded by stage 1, 1 rescued
    by stage 2, 2 failed by both) -- computed once, read by every test that draws batches from the pool."""
    ref = composed(code, pool(code, dtype), cap1(code), SWEEPS)
    kind = np.where(ref[3] == 0, 0, np.where(ref[2] == 1, 1, 2))
    for x in ref + (kind,):
        x.setflags(write=False)
    return ref, kind


def keywords(llrs, correction):
    if correction is None:
        return {}
    if _np_dtype(llrs) == np.float32:
        return dict(scale=correction[0], offset=correction[1])
    return dict(scale_num=correction[0], scale_shift=correction[1], offset=correction[2])


def _np_dtype(x):
    return x.dtype if isinstance(x, np.ndarray) else {"torch.float32": np.float32, "torch.int8": np.int8, "torch.int16": np.int16}[str(x.dtype)]


def cascade(code, llrs, max_iters, max_sweeps, correction=None, device=False, **kw):
    """The call under test, on host buffers or (device=True) on device buffers; numpy results either way."""
    method = code.decode_ms_cascade_batch if _np_dtype(llrs) == np.float32 else code.decode_ms_cascade_fixed_batch
    if not device:
        return method(llrs, max_iters, max_sweeps, **keywords(llrs, correction), **kw)
    import torch
    res = method(torch.from_numpy(np.ascontiguousarray(llrs)).cuda(), max_iters, max_sweeps, **keywords(llrs, correction), **kw)
    torch.cuda.synchronize()
    return tuple(r.cpu().numpy().view(np.uint32) if r.dtype == torch.int32 else r.cpu().numpy() for r in res)


def same(got, want, what=""):
    assert len(got) == len(want) == 4
    for name, g, w in zip(("output", "iters", "success", "stage"), got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.flatnonzero((g != w).reshape(len(g), -1).any(axis=1))
        assert not len(bad), f"{what}: {name} differs in frames {bad[:8].tolist()} ({len(bad)} of {len(g)})"


@pytest.mark.parametrize("code,dtype", CASES, ids=IDS)
def test_mixed_pool_equals_the_composition(code, dtype):
    """All three classes are in the pool -- decoded by stage 1, rescued by stage 2, failed by both -- and host and device calls give the
    composition of the two separate calls; on three codes also the CPU restatement."""
    llrs = pool(code, dtype)
    ref, kind = pool_results(code, dtype)
    counts = [int((kind == k).sum()) for k in range(3)]
    print(f"{code.name} {np.dtype(dtype).name}: stage 1 decodes {counts[0]}, stage 2 rescues {counts[1]}, both fail {counts[2]}")
    assert min(counts) >= 1, counts
    assert (ref[3] == (kind > 0)).all() and (ref[1][kind == 2] == SWEEPS).all() and (ref[1][kind == 0] < cap1(code)).all()
    same(cascade(code, llrs, cap1(code), SWEEPS), ref, "host buffers")
    same(cascade(code, llrs, cap1(code), SWEEPS, device=True), ref, "device buffers")
    if code in CPU_CODES:
        same(ref, cr.cascade(code, llrs, cap1(code), SWEEPS), "the library's composition against the CPU restatement")


def draw(code, dtype, idx):
    """The batch pool[idx] and what the cascade must return for it: frames are independent."""
    ref, _ = pool_results(code, dtype)
    idx = np.asarray(idx)
    return np.ascontiguousarray(pool(code, dtype)[idx]), tuple(x[idx] for x in ref)


@pytest.mark.parametrize("dtype", (np.float32, np.int8), ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("code", (LDPCCode.TC128, LDPCCode.TM1280), ids=lambda c: c.name)
def test_patterns_of_failures(code, dtype):
    """Batches drawn from the classified pool, on device buffers: one class only (all decoded by stage 1: `stage` all 0), one failure
    at the first and at the last index, alternating classes, and the wave edges of the compaction as batch sizes."""
    _, kind = pool_results(code, dtype)
    by = [np.flatnonzero(kind == k) for k in range(3)]
    rng = np.random.default_rng(7)
    for k in range(3):
        llrs, want = draw(code, dtype, rng.choice(by[k], 70))
        got = cascade(code, llrs, cap1(code), SWEEPS, device=True)
        same(got, want, f"class {k} only")
        assert (got[3] == (k > 0)).all() and (got[2] == (k < 2)).all()
    good = rng.choice(by[0], 130)
    for at in (0, 129):
        for k in (1, 2):
            idx = good.copy()
            idx[at] = by[k][0]
            llrs, want = draw(code, dtype, idx)
            got = cascade(code, llrs, cap1(code), SWEEPS, device=True)
            same(got, want, f"one frame of class {k} at {at}")
            assert got[3].sum() == 1 and got[3][at] == 1
    idx = np.array([by[j % 3][(j // 3) % len(by[j % 3])] for j in range(200)])
    llrs, want = draw(code, dtype, idx)
    same(cascade(code, llrs, cap1(code), SWEEPS, device=True), want, "alternating classes")
    for b in (1, 2, 63, 64, 65, 257):
        llrs, want = draw(code, dtype, rng.integers(0, 48, b))
        same(cascade(code, llrs, cap1(code), SWEEPS, device=True), want, f"batch {b}, device")
        if b in (1, 65):
            same(cascade(code, llrs, cap1(code), SWEEPS), want, f"batch {b}, host")


@pytest.mark.parametrize("dtype", TYPES, ids=lambda t: np.dtype(t).name)
def test_chunks_and_slices(dtype, monkeypatch):
    """About 50 failed frames in chunks of 8 (several, the last one partial), a device batch in launch slices of 16 frames, and both:
    the results of the unchunked call."""
    code = LDPCCode.TM1280
    _, kind = pool_results(code, dtype)
    rng = np.random.default_rng(11)
    idx = np.concatenate([rng.choice(np.flatnonzero(kind == 0), 67), rng.choice(np.flatnonzero(kind > 0), 51)])
    rng.shuffle(idx)
    llrs, want = draw(code, dtype, idx)
    assert want[3].sum() == 51
    plain = cascade(code, llrs, cap1(code), SWEEPS, device=True)
    same(plain, want, "unchunked")
    for env in (dict(LABRADOR_LDPC_HIP_CASCADE_CHUNK="8"), dict(LABRADOR_LDPC_HIP_MAX_LAUNCH="16"),
                dict(LABRADOR_LDPC_HIP_CASCADE_CHUNK="8", LABRADOR_LDPC_HIP_MAX_LAUNCH="16"), dict(LABRADOR_LDPC_HIP_CASCADE_CHUNK="1")):
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            same(cascade(code, llrs, cap1(code), SWEEPS, device=True), plain, f"device buffers, {env}")
            same(cascade(code, llrs, cap1(code), SWEEPS), plain, f"host buffers, {env}")
    with monkeypatch.context() as m:                          # host buffers staged in chunks of 32 frames, each with its own stage 2
        m.setenv("LABRADOR_LDPC_HIP_CHUNK", "32")
        big = np.ascontiguousarray(np.tile(llrs, (10, 1)))    # (past the small-call path: more than 1 MiB)
        same(cascade(code, big, cap1(code), SWEEPS), tuple(np.tile(x, (10,) + (1,) * (x.ndim - 1)) for x in plain), "staged chunks")


@pytest.mark.parametrize("dtype", TYPES, ids=lambda t: np.dtype(t).name)
def test_caps_of_zero(dtype):
    """max_iters = 0: the layered entry's results and `stage` all 1.  max_sweeps = 0: every frame stage 1 failed is zeroed.  Both."""
    code = LDPCCode.TM1280
    llrs = pool(code, dtype)
    layered = separate(code)[1](llrs, SWEEPS)
    for device in (False, True):
        got = cascade(code, llrs, 0, SWEEPS, device=device)
        same(got, tuple(layered) + (np.ones(48, np.uint8),), "max_iters = 0")
        got = cascade(code, llrs, cap1(code), 0, device=device)
        same(got, composed(code, llrs, cap1(code), 0), "max_sweeps = 0")
        failed = got[3] == 1
        assert failed.any() and not failed.all() and not got[0][failed].any() and not got[1][failed].any() and not got[2][failed].any()
        got = cascade(code, llrs, 0, 0, device=device)
        assert got[3].all() and not got[0].any() and not got[1].any() and not got[2].any()


def on_device_equals_layered(code, dtype, frames, seed):
    """max_iters = 0 on `frames` frames drawn from the pool, device-resident: every result equals the layered entry's on the same
    buffer, compared on the device."""
    import torch
    idx = torch.from_numpy(np.random.default_rng(seed).integers(0, 48, frames)).cuda()
    d = torch.from_numpy(pool(code, dtype)).cuda()[idx].contiguous()
    layered = (code.decode_ms_layered_batch if dtype == np.float32 else code.decode_ms_layered_fixed_batch)(d, SWEEPS)
    out = torch.full((frames, code.output_len()), 0xEE, dtype=torch.uint8, device="cuda")
    it = torch.full((frames,), -2, dtype=torch.int32, device="cuda")
    ok, stage = (torch.full((frames,), 7, dtype=torch.uint8, device="cuda") for _ in range(2))
    method = code.decode_ms_cascade_batch if dtype == np.float32 else code.decode_ms_cascade_fixed_batch
    method(d, 0, SWEEPS, output=out, iters=it, success=ok, stage=stage)
    torch.cuda.synchronize()
    assert torch.equal(out, layered[0]) and torch.equal(it, layered[1]) and torch.equal(ok, layered[2]) and bool((stage == 1).all())
    del d, layered, out, it, ok, stage
    torch.cuda.empty_cache()


def test_grid_coverage():
    """5000 TC128 frames, all of them listed; and 140 000 int8 ones, whose 1.12 M pieces of 16 bytes and 280 000 pieces of 8 are more than
    one pass of the gather's (1024 workgroups x 256 threads x 4 pieces) and the scatter's (1024 x 256) grids: their loops stride."""
    on_device_equals_layered(LDPCCode.TC128, np.float32, 5000, 1)
    on_device_equals_layered(LDPCCode.TC128, np.int8, 140000, 2)


CORRECTIONS = [(LDPCCode.TM2048, np.float32, (0.8125, 0.0)), (LDPCCode.TM2048, np.int8, (13, 4, 0)), (LDPCCode.TM1280, np.int16, (13, 4, 0)),
               (LDPCCode.TC128, np.int8, (16, 4, 1)), (LDPCCode.TM1280, np.int16, (16, 4, 1))]


@pytest.mark.parametrize("code,dtype,correction", CORRECTIONS,
                         ids=[f"{c.name}-{np.dtype(t).name}-{'_'.join(str(x) for x in k)}" for c, t, k in CORRECTIONS])
def test_corrections_reach_stage_two(code, dtype, correction):
    """Non-identity settings: the composition with the corrected layered entries, and the CPU restatement with the corrected
    restatements; an identity setting given explicitly is the plain call."""
    llrs = pool(code, dtype)
    want = composed(code, llrs, cap1(code), SWEEPS, correction)
    same(cascade(code, llrs, cap1(code), SWEEPS, correction), want, "host")
    same(cascade(code, llrs, cap1(code), SWEEPS, correction, device=True), want, "device")
    same(want, cr.cascade(code, llrs, cap1(code), SWEEPS, correction), "the CPU restatement")
    identity = (1.0, 0.0) if dtype == np.float32 else (16, 4, 0)
    same(cascade(code, llrs, cap1(code), SWEEPS, identity, device=True), pool_results(code, dtype)[0], "identity")


def raw_call(code, dtype, llrs_ptr, out_ptr, it_ptr, ok_ptr, stage_ptr, batch, stream, variant=0):
    suf = {np.float32: "f32", np.int8: "i8", np.int16: "i16"}[dtype]
    fn = getattr(la.lib, "labrador_ldpc_decode_ms_cascade_batch_" + suf)
    opts = la.HipOpts(0, la.MEM_DEVICE, stream, variant, 0, None)
    tail = (1.0, 0.0) if dtype == np.float32 else (1, 0, 0)
    return fn(int(code), llrs_ptr, out_ptr, it_ptr, ok_ptr, stage_ptr, batch, cap1(code), SWEEPS, *tail, ctypes.byref(opts))


@pytest.mark.parametrize("dtype", TYPES, ids=lambda t: np.dtype(t).name)
def test_buffers_and_streams(dtype):
    """A caller's stream; a device set with a repeated ordinal; result rows inside larger prefilled arrays whose neighbours keep their
    fill, on the host and on the device; an `llrs` base one element off 16-byte alignment; a misaligned device `output`."""
    import torch
    code = LDPCCode.TM1280
    llrs = pool(code, dtype)
    want, _ = pool_results(code, dtype)
    B, L = 48, code.output_len()
    s = torch.cuda.Stream()
    d = torch.from_numpy(llrs).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        got = (code.decode_ms_cascade_batch if dtype == np.float32 else code.decode_ms_cascade_fixed_batch)(d, cap1(code), SWEEPS, stream=s.cuda_stream)
    s.synchronize()
    same(tuple(x.cpu().numpy().view(np.uint32) if x.dtype == torch.int32 else x.cpu().numpy() for x in got), want, "a caller's stream")
    same(cascade(code, llrs, cap1(code), SWEEPS, devices=[0, 0]), want, "devices=[0, 0]")

    # rows 8 .. 8 + B of larger arrays
    big = (np.full((B + 16, L), 0xEE, np.uint8), np.full(B + 16, 0xABCDEF, np.uint32), np.full(B + 16, 7, np.uint8), np.full(B + 16, 9, np.uint8))
    rows = tuple(x[8:8 + B] for x in big)
    cascade(code, llrs, cap1(code), SWEEPS, output=rows[0], iters=rows[1], success=rows[2], stage=rows[3])
    same(rows, want, "host rows")
    for x, fill in zip(big, (0xEE, 0xABCDEF, 7, 9)):
        assert (x[:8] == fill).all() and (x[8 + B:] == fill).all()
    dbig = (torch.full((B + 16, L), 0xEE, dtype=torch.uint8, device="cuda"), torch.full((B + 16,), -2, dtype=torch.int32, device="cuda"),
            torch.full((B + 16,), 7, dtype=torch.uint8, device="cuda"), torch.full((B + 16,), 9, dtype=torch.uint8, device="cuda"))
    drows = tuple(x[8:8 + B] for x in dbig)
    (code.decode_ms_cascade_batch if dtype == np.float32 else code.decode_ms_cascade_fixed_batch)(
        d, cap1(code), SWEEPS, output=drows[0], iters=drows[1], success=drows[2], stage=drows[3])
    torch.cuda.synchronize()
    same(tuple(x.cpu().numpy().view(np.uint32) if x.dtype == torch.int32 else x.cpu().numpy() for x in drows), want, "device rows")
    for x, fill in zip(dbig, (0xEE, -2, 7, 9)):
        assert bool((x[:8] == fill).all()) and bool((x[8 + B:] == fill).all())

    # the element-wise gather: the base of `llrs` one element behind a 16-byte boundary
    flat = torch.zeros(B * code.n() + 16, dtype=d.dtype, device="cuda")
    shifted = flat[1:1 + B * code.n()].view(B, code.n())
    shifted.copy_(d)
    assert shifted.data_ptr() % 16 == d.element_size() and shifted.is_contiguous()
    out = torch.zeros((B, L), dtype=torch.uint8, device="cuda")
    it = torch.zeros(B, dtype=torch.int32, device="cuda")
    ok, stage = torch.zeros(B, dtype=torch.uint8, device="cuda"), torch.zeros(B, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    st = raw_call(code, dtype, shifted.data_ptr(), out.data_ptr(), it.data_ptr(), ok.data_ptr(), stage.data_ptr(), B,
                  torch.cuda.current_stream().cuda_stream)
    assert st == 0, la.last_error()
    torch.cuda.synchronize()
    same((out.cpu().numpy(), it.cpu().numpy().view(np.uint32), ok.cpu().numpy(), stage.cpu().numpy()), want, "llrs aligned to its element only")

    # a device `output` that is not 8-byte aligned is refused, and nothing is written
    wide = torch.full((B * L + 8,), 0xEE, dtype=torch.uint8, device="cuda")
    it.fill_(-2)
    torch.cuda.synchronize()
    st = raw_call(code, dtype, d.data_ptr(), wide.data_ptr() + 4, it.data_ptr(), ok.data_ptr(), stage.data_ptr(), B,
                  torch.cuda.current_stream().cuda_stream)
    assert st == EINVAL and "8-byte aligned" in la.last_error()
    torch.cuda.synchronize()
    assert bool((wide == 0xEE).all()) and bool((it == -2).all())


def test_two_streams_share_the_workspace():
    """Two calls back to back from one thread on two streams of the caller's, neither synchronised in between -- the second one's
    compaction, gather and stage 2 reuse the workspace the first one's are still using -- and a third on the first stream again."""
    import torch
    code = LDPCCode.TM2048
    rng = np.random.default_rng(5)
    batches = [draw(code, np.float32, rng.integers(0, 48, b)) for b in (300, 170, 90)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    d = [torch.from_numpy(llrs).cuda() for llrs, _ in batches]
    torch.cuda.synchronize()
    got = []
    for i, x in enumerate(d):
        s = streams[i % 2]
        with torch.cuda.stream(s):
            got.append(code.decode_ms_cascade_batch(x, cap1(code), SWEEPS, stream=s.cuda_stream))
    for s in streams:
        s.synchronize()
    for g, (_, want) in zip(got, batches):
        same((g[0].cpu().numpy(), g[1].cpu().numpy().view(np.uint32), g[2].cpu().numpy(), g[3].cpu().numpy()), want, "two streams")


def test_variants_choose_stage_one():
    """A TM code with i8 LLRs: `variant` 64, the bit-sliced kernel, as stage 1 gives what the default gives; a variant that
    decode_ms_batch has no kernel for is EUNSUPPORTED here too, before stage 2."""
    code, dtype = LDPCCode.TM1280, np.int8
    llrs = pool(code, dtype)
    want, _ = pool_results(code, dtype)
    same(cascade(code, llrs, cap1(code), SWEEPS, variant=64), want, "variant 64, host")
    same(cascade(code, llrs, cap1(code), SWEEPS, variant=64, device=True), want, "variant 64, device")
    with pytest.raises(la.LdpcHipError, match="status -4"):
        code.decode_ms_batch(llrs, cap1(code), variant=100)
    for device in (False, True):
        with pytest.raises(la.LdpcHipError, match="status -4.*not built"):
            cascade(code, llrs, cap1(code), SWEEPS, variant=100, device=device)


def test_tm2048_failure_counts():
    """TM2048 at 1.7 dB, 600 i8 frames of default_rng(1700) at 8 / 31, cap 25 in both stages: 164 frames go to stage 2; 34 fail plain and
    14 at (13, 4, 0), strictly fewer than decode_ms_batch fails."""
    code = LDPCCode.TM2048
    y, _ = oracle.awgn_llrs(code, np.random.default_rng(1700), 600, 1.7, np.float32)
    llrs = quantise(y, np.int8, 8, 31)
    flooding = int((code.decode_ms_batch(llrs, 25)[2] == 0).sum())
    for correction, failures in ((None, 34), ((13, 4, 0), 14)):
        out, it, ok, stage = cascade(code, llrs, 25, 25, correction, device=True)
        print(f"TM2048 1.7 dB i8 {correction}: flooding fails {flooding}, {int(stage.sum())} frames to stage 2, {int((ok == 0).sum())} failures")
        assert int(stage.sum()) == 164 == flooding and int((ok == 0).sum()) == failures < flooding
        same((out, it, ok, stage), composed(code, llrs, 25, 25, correction), str(correction))


def test_ber_harness_runs_the_cascade(capsys):
    """--schedule cascade returns 0 for f32, i8 and i16, and on the same seeds its frame errors do not exceed --schedule layered's."""
    from labrador_ldpc_amd import perftest
    base = ["--code", "TC128", "--snrs", "3.0", "--noise", "ebn0", "--maxiters", "20", "--batch", "4096", "--max-bits", "1e5"]
    assert perftest.main(base + ["--schedule", "cascade"]) == 0
    assert perftest.main(base + ["--schedule", "cascade", "--llr", "i8", "--fixed-scale", "13/16", "--max-sweeps", "25"]) == 0
    assert perftest.main(base + ["--schedule", "cascade", "--llr", "i16", "--fixed-offset", "1"]) == 0
    assert len(capsys.readouterr().out.strip().split("\n")) == 3
    for llr in ("f32", "i8", "i16"):
        fe = {s: perftest.ms_trials(LDPCCode.TC128, 3.0, "ebn0", maxiters=20, batch=4096, max_bits=1e5, schedule=s, llr=llr)[4]
              for s in ("layered", "cascade")}
        print(f"TC128 3 dB {llr}: frame errors {fe}")
        assert fe["cascade"] <= fe["layered"], (llr, fe)
