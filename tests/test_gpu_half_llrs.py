"""f16 / bf16 LLRs through the f32 decoders on the GPU (labrador_ldpc_widen_llrs_batch_{f16,bf16} and the 14 decoder entries of the two
formats).  The contract is "exactly the f32 entry on the widened frame": the widen kernel equals the host loop and
the numpy statement of the rule on every bit pattern, and every decoder entry equals the f32 entry of the same name on the widened
values bit for bit -- output, iters, success, app, stage -- from device tensors and from host rows, across chunks and launch slices,
at the least alignments the header states, and on the special values of the formats.  One case per kernel family is held to the CPU
references too."""
import ctypes
import functools

import numpy as np
import pytest

import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode
import cascade_restatement as cr
import guarded_buffers as gb
import layered_helpers
import layered_restatement as lr
import oracle

pytestmark = pytest.mark.gpu

OK, EINVAL = 0, -1
FORMATS = ("f16", "bf16")


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if la.device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("the half-precision GPU tests need a gfx950 device")
    torch.cuda.set_device(0)


# ---- the formats in numpy -----------------------------------------------------------------------------------------------------------------
def round_to(y, fmt):
    """float32 -> the format's bits (uint16), to nearest, ties to even (no NaN among the inputs)"""
    y = np.ascontiguousarray(y, np.float32)
    if fmt == "f16":
        return y.astype(np.float16).view(np.uint16)
    u = y.view(np.uint32)
    return ((u + (((u >> 16) & 1) + 0x7FFF)) >> 16).astype(np.uint16)


def widen(bits, fmt):
    """the rule of the header, stated in numpy: the format's bits -> float32"""
    if fmt == "bf16":
        return (bits.astype(np.uint32) << 16).view(np.float32)
    x = bits.view(np.float16)
    w = x.astype(np.float32).view(np.uint32).copy()
    w[np.isnan(x)] |= 0x00400000
    return w.view(np.float32)


def tdtype(fmt):
    import torch
    return torch.float16 if fmt == "f16" else torch.bfloat16


def dev(bits, fmt, lead=0):
    """the bits as a device tensor of the format; `lead`: elements the view starts behind a 16-byte boundary"""
    import torch
    flat = torch.empty(bits.size + 8, dtype=torch.int16, device="cuda")
    assert flat.data_ptr() % 16 == 0
    view = flat[lead:lead + bits.size]
    view.copy_(torch.from_numpy(np.ascontiguousarray(bits).view(np.int16).reshape(-1)))
    return view.view(tdtype(fmt)).view(bits.shape)


def dev_f32(w):
    import torch
    return torch.from_numpy(np.ascontiguousarray(w)).cuda()


def host(t):
    import torch
    if not type(t).__module__.startswith("torch"):
        return np.asarray(t)
    a = t.cpu().numpy()
    return a.view(np.uint32) if t.dtype == torch.int32 else a


def results(res):
    import torch
    torch.cuda.synchronize()
    return tuple(host(r) for r in res)


def same(got, want, what=""):
    """every array of a result equal bit for bit (float arrays as their words: a NaN must be the same NaN)"""
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = np.ascontiguousarray(host(g)), np.ascontiguousarray(host(w))
        assert g.shape == w.shape, (what, i, g.shape, w.shape)
        if g.dtype == np.float32:
            g, w = g.view(np.uint32), w.view(np.uint32)
        bad = np.flatnonzero((g.astype(np.int64) != w.astype(np.int64)).reshape(len(g), -1).any(axis=1))
        assert not len(bad), f"{what}: array {i} of the result differs in frames {bad[:8].tolist()} ({len(bad)} of {len(g)})"


def c_call(name, fmt, code, bits, cap, soft=False, stage=False, extra=(), variant=0):
    """An entry of the C ABI on HOST rows of raw bits (what Python cannot offer for bf16): -> the result arrays, `app` first."""
    batch = len(bits)
    bits = np.ascontiguousarray(bits)
    res = []
    if soft:
        res.append(np.full((batch, code.n() + code.punctured_bits()), -3.0, np.float32))
    res += [np.full((batch, code.output_len()), 0xEE, np.uint8), np.full(batch, 77, np.uint32), np.full(batch, 7, np.uint8)]
    if stage:
        res.append(np.full(batch, 9, np.uint8))
    opts = la.HipOpts(la.DEVICE_CURRENT, la.MEM_HOST, None, variant, 0, None)
    s = getattr(la.lib, name + fmt)(int(code), bits.ctypes.data, *(r.ctypes.data for r in res), batch, cap, *extra, ctypes.byref(opts))
    assert s == OK, (name + fmt, s, la.last_error())
    return tuple(res)


# ---- the widen kernel against the host loop -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_widen_kernel_equals_the_host_loop_on_every_bit_pattern(fmt):
    """All 65 536 patterns and one more TC128 frame: 513 frames, 8208 octets, so the ninth workgroup is partial.  The result stands
    between guard bands."""
    import torch
    code = LDPCCode.TC128
    bits = np.concatenate([np.arange(65536, dtype=np.uint16), np.arange(0x3C00, 0x3C00 + 128, dtype=np.uint16)]).reshape(513, code.n())
    want = widen(bits, fmt).view(np.uint32)
    fn = getattr(la.lib, "labrador_ldpc_widen_llrs_batch_" + fmt)
    out_host = np.zeros(bits.shape, np.float32)
    assert fn(int(code), bits.ctypes.data, out_host.ctypes.data, 513, None) == OK
    assert (out_host.view(np.uint32) == want).all()
    out, guard = gb.guarded(513, (code.n(),), torch.float32, 0, "cuda", name="out")
    src = dev(bits, fmt)
    got = code.widen_llrs_batch(src, out=out)
    torch.cuda.synchronize()
    assert got is out
    g = host(got).view(np.uint32)
    bad = np.argwhere(g != want)
    assert bad.size == 0, [(hex(bits[tuple(i)]), hex(g[tuple(i)]), hex(want[tuple(i)])) for i in bad[:8]]
    guard.check()
    assert (host(src.view(torch.int16)).view(np.uint16) == bits).all()


@pytest.mark.parametrize("fmt", FORMATS)
def test_misaligned_device_buffers_are_refused(fmt):
    """An `llrs` or an `out` that is not 16-byte aligned is EINVAL, and nothing is written; so for the flooding and cascade entries'
    `llrs` and every decoder's `output`."""
    import torch
    code = LDPCCode.TC128
    n = code.n()
    src = torch.zeros(2 * n + 8, dtype=torch.int16, device="cuda")
    dst = torch.full((2 * n + 8,), -7.5, dtype=torch.float32, device="cuda")
    opts = la.HipOpts(0, la.MEM_DEVICE, torch.cuda.current_stream().cuda_stream, 0, 0, None)
    fn = getattr(la.lib, "labrador_ldpc_widen_llrs_batch_" + fmt)
    for off in (2, 8):
        assert fn(int(code), src.data_ptr() + off, dst.data_ptr(), 2, ctypes.byref(opts)) == EINVAL
        assert la.last_error() == "device llrs buffer must be 16-byte aligned"
    for off in (4, 8):
        assert fn(int(code), src.data_ptr(), dst.data_ptr() + off, 2, ctypes.byref(opts)) == EINVAL
        assert la.last_error() == "device out buffer must be 16-byte aligned"
    with pytest.raises(la.LdpcHipError, match="16-byte aligned"):
        code.widen_llrs_batch(src[1:1 + 2 * n].view(tdtype(fmt)).view(2, n))
    out = torch.full((2 * code.output_len() + 8,), 0xEE, dtype=torch.uint8, device="cuda")
    it, ok = torch.full((2,), -2, dtype=torch.int32, device="cuda"), torch.full((2,), 7, dtype=torch.uint8, device="cuda")
    stage = torch.full((2,), 9, dtype=torch.uint8, device="cuda")
    flood = getattr(la.lib, "labrador_ldpc_decode_ms_batch_" + fmt)
    casc = getattr(la.lib, "labrador_ldpc_decode_ms_cascade_batch_" + fmt)
    lay = getattr(la.lib, "labrador_ldpc_decode_ms_layered_batch_" + fmt)
    p = (out.data_ptr(), it.data_ptr(), ok.data_ptr())
    assert flood(int(code), src.data_ptr() + 2, *p, 2, 10, ctypes.byref(opts)) == EINVAL
    assert la.last_error() == "device llrs buffer must be 16-byte aligned"
    assert casc(int(code), src.data_ptr() + 2, *p, stage.data_ptr(), 2, 10, 10, 1.0, 0.0, ctypes.byref(opts)) == EINVAL
    assert la.last_error() == "device llrs buffer must be 16-byte aligned"
    for fn2, tail in ((flood, (2, 10)), (lay, (2, 10))):
        assert fn2(int(code), src.data_ptr(), out.data_ptr() + 4, it.data_ptr(), ok.data_ptr(), *tail, ctypes.byref(opts)) == EINVAL
        assert la.last_error() == "device output buffer must be 8-byte aligned"
    torch.cuda.synchronize()
    assert bool((dst == -7.5).all()) and bool((out == 0xEE).all()) and bool((it == -2).all()) and bool((ok == 7).all())
    assert bool((stage == 9).all())


# ---- flooding -----------------------------------------------------------------------------------------------------------------------------
# code: (seed, frames, Eb/N0, cap) -- the cases of tests/test_gpu_quantise.py
CASES = {LDPCCode.TC128: (41, 64, 3.0, 20), LDPCCode.TM1280: (42, 48, 3.2, 25), LDPCCode.TM2048: (43, 48, 1.9, 25),
         LDPCCode.TM8192: (44, 12, 1.6, 25)}
FLOOD = [(c, f) for c in CASES for f in FORMATS]
IDS = [f"{c.name}-{f}" for c, f in FLOOD]


@functools.lru_cache(maxsize=None)
def frames(code, fmt):
    """(the case's frames rounded to the format as bits, their widening): made once, read-only"""
    seed, n, snr, _ = CASES[code]
    y, _ = oracle.awgn_llrs(code, np.random.default_rng(seed), n, snr, np.float32)
    bits = round_to(y, fmt)
    w = widen(bits, fmt)
    bits.setflags(write=False)
    w.setflags(write=False)
    return bits, w


@functools.lru_cache(maxsize=None)
def f32_flooding(code, fmt, variant, cap):
    """decode_ms_soft_batch on the widened frames as float32: the reference, once per case"""
    ref = results(code.decode_ms_soft_batch(dev_f32(frames(code, fmt)[1]), cap, variant=variant))
    for r in ref:
        r.setflags(write=False)
    return ref


@pytest.mark.parametrize("code,fmt", FLOOD, ids=IDS)
def test_flooding_equals_the_f32_entry_on_the_widened_frames(code, fmt, monkeypatch):
    cap = CASES[code][3]
    bits, w = frames(code, fmt)
    if code in (LDPCCode.TM2048, LDPCCode.TM8192) and fmt == "f16":
        assert (np.abs(w) < 2.0 ** -14).any()                                 # f16 subnormals or zeros are among the frames
    for variant in ((0, 2) if code == LDPCCode.TM8192 else (0,)):             # (TM8192: the pair kernel, and IPT 2)
        ref = f32_flooding(code, fmt, variant, cap)
        if variant == 0:
            same(ref[1:], oracle.decode_ms_batch(code, w, cap)[:3], "the f32 entry against the oracle")
            assert 0 < int((ref[3] == 0).sum()) < len(bits)
        same(results(code.decode_ms_soft_batch(dev(bits, fmt), cap, variant=variant)), ref, f"soft, device, variant {variant}")
        same(results(code.decode_ms_batch(dev(bits, fmt), cap, variant=variant)), ref[1:], f"hard, device, variant {variant}")
        same(c_call("labrador_ldpc_decode_ms_soft_batch_", fmt, code, bits, cap, soft=True, variant=variant), ref, f"soft, host, variant {variant}")
        same(c_call("labrador_ldpc_decode_ms_batch_", fmt, code, bits, cap, variant=variant), ref[1:], f"hard, host, variant {variant}")
    ref = f32_flooding(code, fmt, 0, cap)
    if fmt == "f16":                                                          # numpy rows through the Python method
        same(code.decode_ms_soft_batch(bits.view(np.float16), cap), ref, "soft, numpy float16")
    for env in (dict(LABRADOR_LDPC_HIP_WIDEN_CHUNK="8"), dict(LABRADOR_LDPC_HIP_MAX_LAUNCH="16")):
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            same(results(code.decode_ms_soft_batch(dev(bits, fmt), cap)), ref, f"soft, device, {env}")
            same(c_call("labrador_ldpc_decode_ms_batch_", fmt, code, bits, cap), ref[1:], f"hard, host, {env}")
    same(results(code.decode_ms_soft_batch(dev(bits, fmt), 0)), results(code.decode_ms_soft_batch(dev_f32(w), 0)), "maxiters = 0")


def test_a_variant_without_a_kernel_is_unsupported():
    """As decode_ms_batch on float32: EUNSUPPORTED with the flooding entry's text, for host and device buffers."""
    code = LDPCCode.TM1280
    bits = frames(code, "f16")[0][:4]
    for x in (bits.view(np.float16), dev(bits, "f16")):
        with pytest.raises(la.LdpcHipError, match="status -4.*kernel variant 100 not built for code 3"):
            code.decode_ms_batch(x, 10, variant=100)


# ---- layered --------------------------------------------------------------------------------------------------------------------------
LAYERED = [(c, f) for c in LDPCCode for f in FORMATS]
CORRECTIONS = ((1.0, 0.0), (0.8125, 0.0), (1.0, 0.1))


@functools.lru_cache(maxsize=None)
def layered_frames(code, fmt):
    """37 frames per code -- odd, so the last workgroup of TC128 (4 codewords) and TC256 (2) is partial -- near each rate's
    waterfall"""
    snr = 3.0 if code <= LDPCCode.TC512 else {LDPCCode.TM1280: 3.2, LDPCCode.TM5120: 3.2, LDPCCode.TM1536: 2.4, LDPCCode.TM6144: 2.4}.get(code, 1.8)
    y, _ = oracle.awgn_llrs(code, np.random.default_rng(500 + int(code)), 37, snr, np.float32)
    bits = round_to(y, fmt)
    return bits, widen(bits, fmt)


@pytest.mark.parametrize("code,fmt", LAYERED, ids=[f"{c.name}-{f}" for c, f in LAYERED])
def test_layered_equals_the_f32_entries_on_the_widened_frames(code, fmt):
    """Hard and soft, the three corrections, caps 0, 1 and 25, batches of 1 and 37; `llrs` one element behind a 16-byte boundary:
    2-byte aligned only."""
    bits, w = layered_frames(code, fmt)
    for batch in (1, 37):
        b, wf = bits[:batch], dev_f32(w[:batch])
        x = dev(b, fmt, lead=1)
        assert x.data_ptr() % 16 == 2
        for scale, offset in CORRECTIONS:
            for cap in (0, 1, 25):
                what = f"batch {batch}, ({scale}, {offset}), cap {cap}"
                ref = results(code.decode_ms_layered_soft_batch(wf, cap, scale=scale, offset=offset))
                same(results(code.decode_ms_layered_soft_batch(x, cap, scale=scale, offset=offset)), ref, "soft, " + what)
                same(results(code.decode_ms_layered_batch(x, cap, scale=scale, offset=offset)), ref[1:], "hard, " + what)
    # host rows, through the C entries (the plain ones and the corrected ones)
    ref = results(code.decode_ms_layered_soft_batch(dev_f32(w), 25))
    same(c_call("labrador_ldpc_decode_ms_layered_soft_batch_", fmt, code, bits, 25, soft=True), ref, "soft, host")
    same(c_call("labrador_ldpc_decode_ms_layered_batch_", fmt, code, bits, 25), ref[1:], "hard, host")
    ref = results(code.decode_ms_layered_soft_batch(dev_f32(w), 25, scale=0.8125))
    same(c_call("labrador_ldpc_decode_ms_layered_corrected_soft_batch_", fmt, code, bits, 25, soft=True, extra=(0.8125, 0.0)), ref, "corrected soft, host")
    same(c_call("labrador_ldpc_decode_ms_layered_corrected_batch_", fmt, code, bits, 25, extra=(0.8125, 0.0)), ref[1:], "corrected hard, host")


@pytest.mark.parametrize("fmt", FORMATS)
def test_layered_against_the_restatement(fmt):
    """TC128 and TM1280 at cap 25, plain: the CPU restatement of the layered schedule on the widened frames."""
    for code in (LDPCCode.TC128, LDPCCode.TM1280):
        bits, w = layered_frames(code, fmt)
        out, it, ok, app = lr.decode_layered(layered_helpers.structure(code), w, 25)
        got = results(code.decode_ms_layered_soft_batch(dev(bits, fmt), 25))
        same(got[1:], (out, it, ok), f"{code.name} against the restatement")
        assert layered_helpers.same_app(got[0], app)


# ---- special values -------------------------------------------------------------------------------------------------------------------
SPECIAL = {"f16": (0x0000, 0x8000, 0x0001, 0x8001, 0x7BFF, 0xFBFF, 0x7C00, 0xFC00, 0x7E00, 0xFE00),
           "bf16": (0x0000, 0x8000, 0x0001, 0x8001, 0x7F7F, 0xFF7F, 0x7F80, 0xFF80, 0x7FC0, 0xFFC0)}


@pytest.mark.parametrize("fmt", FORMATS)
def test_special_values_decode_as_their_widening(fmt):
    """One frame each of +-0, the smallest subnormal of either sign, the largest finite value of either sign, +-inf and a quiet NaN
    of either sign, and one frame of ordinary values with single NaNs in it, among ordinary frames: flooding and layered, hard and
    soft, equal the f32 entries on the widened bits."""
    for code in (LDPCCode.TC128, LDPCCode.TM2048):
        bits = np.array(frames(code, fmt)[0][:len(SPECIAL[fmt]) + 3])
        for f, v in enumerate(SPECIAL[fmt]):
            bits[f + 1] = v
        bits[-1, [0, 5, code.n() // 2, code.n() - 1]] = SPECIAL[fmt][8:10] * 2
        w = widen(bits, fmt)
        assert np.isnan(w[-1]).sum() == 4 and np.isnan(w[9]).all() and np.isinf(w[7]).all() and (w[3] != 0).all()
        x, wf = dev(bits, fmt), dev_f32(w)
        for cap in (1, 25):
            same(results(code.decode_ms_soft_batch(x, cap)), results(code.decode_ms_soft_batch(wf, cap)), f"{code.name} flooding, cap {cap}")
            same(results(code.decode_ms_batch(x, cap)), results(code.decode_ms_batch(wf, cap)), f"{code.name} flooding hard, cap {cap}")
            for scale, offset in CORRECTIONS[:2]:
                same(results(code.decode_ms_layered_soft_batch(x, cap, scale=scale, offset=offset)),
                     results(code.decode_ms_layered_soft_batch(wf, cap, scale=scale, offset=offset)), f"{code.name} layered ({scale}), cap {cap}")
                same(results(code.decode_ms_layered_batch(x, cap, scale=scale, offset=offset)),
                     results(code.decode_ms_layered_batch(wf, cap, scale=scale, offset=offset)), f"{code.name} layered hard ({scale}), cap {cap}")


# ---- the cascade ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("code,fmt", FLOOD, ids=IDS)
def test_cascade_equals_the_f32_cascade_on_the_widened_frames(code, fmt, monkeypatch):
    cap = CASES[code][3]
    bits, w = frames(code, fmt)
    ref = results(code.decode_ms_cascade_batch(dev_f32(w), cap, cap, scale=0.8125))
    stage = ref[3]
    print(f"{code.name} {fmt}: the f32 cascade sends {int(stage.sum())} of {len(stage)} frames to stage 2")
    assert 0 < int(stage.sum()) < len(stage)                                  # (from the reference: both stages carry frames)
    if code == LDPCCode.TC128:
        same(ref, cr.cascade(code, w, cap, cap, (0.8125, 0.0)), "the f32 cascade against the restatement")
    same(results(code.decode_ms_cascade_batch(dev(bits, fmt), cap, cap, scale=0.8125)), ref, "device")
    same(c_call("labrador_ldpc_decode_ms_cascade_batch_", fmt, code, bits, cap, stage=True, extra=(cap, 0.8125, 0.0)), ref, "host")
    with monkeypatch.context() as m:
        m.setenv("LABRADOR_LDPC_HIP_WIDEN_CHUNK", "8")
        same(results(code.decode_ms_cascade_batch(dev(bits, fmt), cap, cap, scale=0.8125)), ref, "device, chunks of 8")
    same(results(code.decode_ms_cascade_batch(dev(bits, fmt), cap, cap)), results(code.decode_ms_cascade_batch(dev_f32(w), cap, cap)), "plain stage 2")


# ---- dtype dispatch, two streams ------------------------------------------------------------------------------------------------------
def test_both_torch_dtypes_dispatch_and_two_streams_share_the_workspace():
    """A torch.float16 and a torch.bfloat16 tensor through decode_ms_batch, back to back on two streams by one thread, the second
    batch larger so that the workspace grows while the first may still be using it; neither stream is synchronised in between."""
    import torch
    code, cap = LDPCCode.TM2048, 25
    idx = {"f16": np.arange(5, 25), "bf16": np.r_[np.arange(48), np.arange(47, -1, -1), np.arange(0, 48, 2)]}
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    d = {f: dev(frames(code, f)[0][idx[f]], f) for f in FORMATS}
    assert d["f16"].dtype == torch.float16 and d["bf16"].dtype == torch.bfloat16
    torch.cuda.synchronize()
    got = {}
    for f, s in zip(FORMATS, streams):
        with torch.cuda.stream(s):
            got[f] = code.decode_ms_batch(d[f], cap, stream=s.cuda_stream)
    for s in streams:
        s.synchronize()
    for f in FORMATS:
        same(tuple(host(r) for r in got[f]), tuple(r[idx[f]] for r in f32_flooding(code, f, 0, cap)[1:]), f"two streams, {f}")


# ---- containment ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ("flooding", "layered", "cascade"))
@pytest.mark.parametrize("fmt", FORMATS)
def test_results_stay_inside_their_rows(family, fmt):
    """One case per family into views between guard bands, every buffer at the least alignment the header states: `output` 8 bytes,
    `app` 16, `iters` 4, `success` and `stage` 1; `llrs` 16 bytes for the flooding and cascade entries, 2 for the layered ones.  The
    input comes back unchanged."""
    import torch
    code = LDPCCode.TM1280
    cap = CASES[code][3]
    bits, w = frames(code, fmt)
    bits, w = bits[:37], w[:37]
    batch, npn = len(bits), code.n() + code.punctured_bits()
    llrs, g_llrs = gb.guarded_copy(bits.view(np.int16), 2 if family == "layered" else 0, "cuda")
    x = llrs.view(tdtype(fmt))
    frozen = gb.frozen(llrs)
    out, g_out = gb.guarded(batch, (code.output_len(),), torch.uint8, 8, "cuda", name="output")
    it, g_it = gb.guarded(batch, (), torch.int32, 4, "cuda", name="iters", prefill=-2)
    ok, g_ok = gb.guarded(batch, (), torch.uint8, 1, "cuda", name="success")
    guards = [g_llrs, g_out, g_it, g_ok]
    if family == "cascade":
        stage, g_stage = gb.guarded(batch, (), torch.uint8, 1, "cuda", name="stage")
        guards.append(g_stage)
        got = code.decode_ms_cascade_batch(x, cap, cap, scale=0.8125, output=out, iters=it, success=ok, stage=stage)
        ref = code.decode_ms_cascade_batch(dev_f32(w), cap, cap, scale=0.8125)
    else:
        app, g_app = gb.guarded(batch, (npn,), torch.float32, 0, "cuda", name="app", app=True)
        guards.append(g_app)
        method = code.decode_ms_soft_batch if family == "flooding" else code.decode_ms_layered_soft_batch
        got = method(x, cap, app=app, output=out, iters=it, success=ok)
        ref = method(dev_f32(w), cap)
    same(results(got), results(ref), family)
    for g in guards:
        g.check()
    frozen.check()


# ---- the harness ----------------------------------------------------------------------------------------------------------------------
def test_the_ber_harness_runs_the_half_formats():
    """--llr f16 / bf16: one point per schedule on a small batch; the frame errors are printed beside the f32 branch's."""
    from labrador_ldpc_amd import perftest
    code = LDPCCode.TC128
    for schedule in ("flooding", "layered", "cascade"):
        f32 = perftest.ms_trials(code, 3.0, "ebn0", 20, 512, 1, 10 ** 9, schedule=schedule)
        for fmt in FORMATS:
            trials, bits, errors, ber, fe = perftest.ms_trials(code, 3.0, "ebn0", 20, 512, 1, 10 ** 9, schedule=schedule, llr=fmt)
            print(f"{schedule} {fmt}: {fe} frame errors of {trials} (f32: {f32[4]})")
            assert trials == 512 and bits == 512 * code.k() and 0 <= fe < 512
    assert perftest.main(["--code", "TC128", "--snrs", "3.0", "--noise", "ebn0", "--maxiters", "20", "--batch", "256", "--max-bits", "1",
                          "--llr", "f16", "--schedule", "layered"]) == 0
