"""f32 LLRs through the bit-sliced i8 kernels' own loader, on the GPU (labrador_ldpc_decode_ms_bitsliced_quantised_batch_i8,
labrador_ldpc_decode_ms_bitsliced_quantised_corrected_batch_i8, labrador_ldpc_decode_ms_cascade_bitsliced_quantised_batch_i8; the
`bitsliced` keyword of LDPCCode.decode_ms_quantised_batch and decode_ms_cascade_quantised_batch), bit for bit against
the references of tests/bs_quantised_frames.py and against the existing two-pass entries: the four one-wave TM codes on the 3 G + 1
frames that the CPU emulation of the same kernel text passed (tests/test_bitslice_quantised_emu.py), caps 0 / 3 / 25, partial groups,
host and device buffers, one batch of 4 G 1024 + 3 frames, containment in guarded buffers at the least alignments, the refusals."""
import ctypes

import numpy as np
import pytest

import bs_quantised_frames as bqf
import guarded_buffers as gb
import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode

pytestmark = pytest.mark.gpu

CODES = [LDPCCode[n] for n in bqf.NAMES]
CAPS = (0, 3, 25)
EINVAL, OK, EUNSUPPORTED = -1, 0, -4
PLAIN = "labrador_ldpc_decode_ms_bitsliced_quantised_batch_i8"
CORRECTED = "labrador_ldpc_decode_ms_bitsliced_quantised_corrected_batch_i8"
CASCADE = "labrador_ldpc_decode_ms_cascade_bitsliced_quantised_batch_i8"
HARD = ("output", "iters", "success")
# the cascade's (cap, sweeps, stage-1 triple, stage-2 triple)
CASCADES = ((3, 20) + bqf.CASCADE_PAIR, (25, 25) + bqf.CASCADE_PAIR, (0, 5) + bqf.CASCADE_PAIR, (3, 20, bqf.IDENTITY, (3, 2, 1)),
            (3, 20, (1, 0, 1), bqf.IDENTITY))


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if la.device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("the f32-loader bit-sliced GPU tests need a gfx950 device")
    torch.cuda.set_device(0)


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def same(tag, got, want, names=HARD):
    assert len(got) == len(want) == len(names), (tag, len(got), len(want))
    for g, w, what in zip(got, want, names):
        g, w = host(g), host(w)
        assert g.shape == w.shape, (tag, what, g.shape, w.shape)
        bad = np.flatnonzero((g.reshape(len(w), -1).astype(np.int64) != w.reshape(len(w), -1).astype(np.int64)).any(axis=1))
        assert bad.size == 0, f"{tag}: {what} differs in frames {bad.tolist()[:8]}"


def kw_of(triple, prefix=""):
    return {prefix + "scale_num": triple[0], prefix + "scale_shift": triple[1], prefix + "offset": triple[2]}


def batches_of(g):
    return sorted({b for b in (g - 1, g, g + 1, 3 * g + 1) if b >= 1})


def first(res, b):
    return tuple(a[:b] for a in res)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("code", CODES, ids=lambda c: c.name)
def test_flooding_entries_equal_the_reference_and_the_two_pass_route(code, device):
    import torch
    name = code.name
    bqf.assert_conditions(name)
    llrs = bqf.frames(name)
    x = torch.from_numpy(np.array(llrs)).cuda() if device else llrs
    sync = torch.cuda.synchronize if device else (lambda: None)
    for b in batches_of(bqf.GROUP[name]):
        for cap in CAPS:
            for lim in bqf.LIMS:
                got = code.decode_ms_quantised_batch(x[:b], "i8", bqf.SCALE, lim, cap, bitsliced=True)
                two_pass = code.decode_ms_quantised_batch(x[:b], "i8", bqf.SCALE, lim, cap)
                sync()
                tag = f"{name} plain lim {lim} cap {cap} batch {b}"
                same(tag + ": the oracle on the quantised frames", got, first(bqf.expected_plain(name, lim, cap), b))
                same(tag + ": the two-pass entry", got, two_pass)
            for triple in bqf.TRIPLES:
                got = code.decode_ms_quantised_batch(x[:b], "i8", bqf.SCALE, 127, cap, bitsliced=True, **kw_of(triple))
                q = code.quantise_llrs_batch(x[:b], "i8", bqf.SCALE, 127)
                two_pass = code.decode_ms_corrected_fixed_batch(q, *triple, maxiters=cap)
                sync()
                tag = f"{name} {triple} cap {cap} batch {b}"
                same(tag + ": the corrected statement on the quantised frames", got, first(bqf.expected_corrected(name, triple)[cap], b))
                same(tag + ": quantise, then the corrected i8 entry", got, two_pass)
            # every spelling of the identity is the plain kernel's answer
            got = code.decode_ms_quantised_batch(x[:b], "i8", bqf.SCALE, 127, cap, bitsliced=True, scale_num=16, scale_shift=4)
            sync()
            same(f"{name} identity cap {cap} batch {b}", got, first(bqf.expected_plain(name, 127, cap), b))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("code", CODES, ids=lambda c: c.name)
def test_cascade_entry_equals_the_reference_and_the_two_pass_cascade(code, device):
    import torch
    name = code.name
    llrs = bqf.frames(name)
    x = torch.from_numpy(np.array(llrs)).cuda() if device else llrs
    names = HARD + ("stage",)
    stages = set()
    for cap, sweeps, t1, t2 in CASCADES:
        for b in sorted({bqf.GROUP[name] + 1, len(llrs)}):
            kw = dict(maxiters=cap, max_sweeps=sweeps, **kw_of(t2))
            fl = {} if t1 == bqf.IDENTITY else kw_of(t1, "flooding_")
            got = code.decode_ms_cascade_quantised_batch(x[:b], "i8", bqf.SCALE, 127, bitsliced=True, **fl, **kw)
            two_pass = code.decode_ms_cascade_quantised_batch(x[:b], "i8", bqf.SCALE, 127, **fl, **kw)
            if device:
                torch.cuda.synchronize()
            tag = f"{name} cascade {cap, sweeps} {t1} {t2} batch {b}"
            same(tag + ": the composition of the statements", got, first(bqf.expected_cascade(name, cap, sweeps, t1, t2), b), names)
            same(tag + ": the two-pass cascade", got, two_pass, names)
            stages |= set(host(got[3]).tolist())
    assert stages == {0, 1}                                                          # (both stages carried frames)


@pytest.mark.parametrize("code", CODES, ids=lambda c: c.name)
def test_a_large_batch_with_a_partial_last_group(code):
    """4 G 1024 + 3 frames, the 3 G + 1 frames repeated: more than one wave per CU, many groups, the last one partial"""
    import torch
    name, g = code.name, bqf.GROUP[code.name]
    b = 4 * g * 1024 + 3
    base = bqf.frames(name)
    idx = np.arange(b) % len(base)
    d = torch.from_numpy(np.array(base)).cuda()[torch.from_numpy(idx).cuda()].contiguous()
    assert d.shape == (b, code.n()) and d.data_ptr() % 16 == 0
    got = code.decode_ms_quantised_batch(d, "i8", bqf.SCALE, 31, 25, bitsliced=True)
    two_pass = code.decode_ms_quantised_batch(d, "i8", bqf.SCALE, 31, 25)
    t1, t2 = bqf.CASCADE_PAIR
    kw = dict(maxiters=3, max_sweeps=20, **kw_of(t1, "flooding_"), **kw_of(t2))
    cgot = code.decode_ms_cascade_quantised_batch(d, "i8", bqf.SCALE, 31, bitsliced=True, **kw)
    ctwo = code.decode_ms_cascade_quantised_batch(d, "i8", bqf.SCALE, 31, **kw)
    torch.cuda.synchronize()
    same(f"{name} batch {b}: the oracle", got, tuple(a[idx] for a in bqf.expected_plain(name, 31, 25)))
    same(f"{name} batch {b}: the two-pass entry", got, two_pass)
    same(f"{name} batch {b}: the cascade's reference", cgot, tuple(a[idx] for a in bqf.expected_cascade(name, 3, 20, t1, t2, 31)), HARD + ("stage",))
    same(f"{name} batch {b}: the two-pass cascade", cgot, ctwo, HARD + ("stage",))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("sym", [PLAIN, CORRECTED, CASCADE])
@pytest.mark.parametrize("code", CODES, ids=lambda c: c.name)
def test_the_entries_write_only_the_callers_result_rows(code, sym, device):
    """G + 1 frames (a partial last group) in guarded views at the least alignments the header admits: llrs on a 16-byte boundary,
    output 8 bytes past one, iters 4 past an 8-byte one, success and stage odd."""
    import torch
    name = code.name
    b = bqf.GROUP[name] + 1
    dev = "cuda" if device else None
    x, gx = gb.guarded_copy(np.array(bqf.frames(name)[:b]), 0, dev, name="llrs")
    out, go = gb.guarded(b, (code.output_len(),), np.uint8, 8, dev, name="output")
    it, gi = gb.guarded(b, (), np.int32, 4, dev, name="iters", prefill=-2)
    ok, gk = gb.guarded(b, (), np.uint8, 1, dev, name="success")
    stage, gs = gb.guarded(b, (), np.uint8, 1, dev, name="stage")
    inp = gb.frozen(x, "llrs")
    ptr = (lambda t: t.data_ptr()) if device else (lambda t: t.ctypes.data)
    assert ptr(x) % 16 == 0 and ptr(out) % 16 == 8 and ptr(it) % 8 == 4 and ptr(ok) % 2 == 1 and ptr(stage) % 2 == 1
    opts = la.HipOpts(0, la.MEM_DEVICE if device else la.MEM_HOST, None, 0, 0, None)
    if device:
        torch.cuda.synchronize()
    t1, t2 = bqf.CASCADE_PAIR
    if sym == PLAIN:
        st = getattr(la.lib, sym)(int(code), ptr(x), ptr(out), ptr(it), ptr(ok), b, 25, bqf.SCALE, 127, ctypes.byref(opts))
        want = first(bqf.expected_plain(name, 127, 25), b)
    elif sym == CORRECTED:
        st = getattr(la.lib, sym)(int(code), ptr(x), ptr(out), ptr(it), ptr(ok), b, 25, bqf.SCALE, 127, *t1, ctypes.byref(opts))
        want = first(bqf.expected_corrected(name, t1)[25], b)
    else:
        st = getattr(la.lib, sym)(int(code), ptr(x), ptr(out), ptr(it), ptr(ok), ptr(stage), b, 3, 20, bqf.SCALE, 127, *t1, *t2, ctypes.byref(opts))
        want = first(bqf.expected_cascade(name, 3, 20, t1, t2), b)
    assert st == OK, la.last_error()
    if device:
        torch.cuda.synchronize()
    for guard in (gx, go, gi, gk, gs, inp):
        guard.check()
    got = (out, host(it).astype(np.uint32), ok) + ((stage,) if sym == CASCADE else ())
    same(f"{name} {sym} guarded", got, want, HARD + (("stage",) if sym == CASCADE else ()))
    if sym != CASCADE:
        assert (host(stage) == 0xEE).all()                                           # (not an argument of the entry: untouched)


def raw_buffers(code, batch, device):
    """llrs, output, iters, success, stage with sentinel-filled results, and their addresses"""
    import torch
    if device:
        t = (torch.zeros((batch, code.n() + 4), dtype=torch.float32, device="cuda"),
             torch.full((batch, code.output_len()), 0xEE, dtype=torch.uint8, device="cuda"),
             torch.full((batch,), -2, dtype=torch.int32, device="cuda"), torch.full((batch,), 0xEE, dtype=torch.uint8, device="cuda"),
             torch.full((batch,), 0xEE, dtype=torch.uint8, device="cuda"))
        torch.cuda.synchronize()
        return t, [a.data_ptr() for a in t]
    t = (np.zeros((batch, code.n()), np.float32), np.full((batch, code.output_len()), 0xEE, np.uint8), np.full(batch, -2, np.int32),
         np.full(batch, 0xEE, np.uint8), np.full(batch, 0xEE, np.uint8))
    return t, [a.ctypes.data for a in t]


def untouched(t):
    return bool((host(t[1]) == 0xEE).all() and (host(t[2]) == -2).all() and (host(t[3]) == 0xEE).all() and (host(t[4]) == 0xEE).all())


def call(sym, code, p, opts=None, q=(8.0, 31)):
    o = ctypes.byref(opts) if opts is not None else None
    if sym == PLAIN:
        return getattr(la.lib, sym)(int(code), *p[:4], 2, 10, *q, o)
    if sym == CORRECTED:
        return getattr(la.lib, sym)(int(code), *p[:4], 2, 10, *q, 13, 4, 0, o)
    return getattr(la.lib, sym)(int(code), *p, 2, 10, 10, *q, 13, 4, 0, 13, 4, 0, o)


@pytest.mark.parametrize("sym", [PLAIN, CORRECTED, CASCADE])
def test_refusals_come_with_their_text_and_before_any_device_work(sym):
    import torch
    text = "f32-reading bit-sliced flooding decoder"
    for code in (LDPCCode.TM1280, LDPCCode.TM5120, LDPCCode.TC128, LDPCCode.TC512):
        keep, p = raw_buffers(code, 2, False)
        assert call(sym, code, p) == EUNSUPPORTED
        assert text in la.last_error() and "TM1536, TM2048, TM6144 and TM8192" in la.last_error(), la.last_error()
        assert untouched(keep)
    code = LDPCCode.TM2048
    keep, p = raw_buffers(code, 2, False)
    for variant in (64, 1):
        opts = la.HipOpts(0, la.MEM_HOST, None, variant, 0, None)
        assert call(sym, code, p, opts) == EUNSUPPORTED
        assert f"variant {variant}" in la.last_error() and text in la.last_error(), la.last_error()
    assert call(sym, code, p, q=(0.0, 31)) == EINVAL and "scale 0" in la.last_error()
    assert call(sym, code, p, q=(8.0, 128)) == EINVAL and "lim 128" in la.last_error()
    assert untouched(keep)
    # device rows off their alignment: llrs at 4 and at 8 mod 16, output at 4 mod 8
    dk, dp = raw_buffers(code, 3, True)
    opts = la.HipOpts(0, la.MEM_DEVICE, None, 0, 0, None)
    assert dp[0] % 16 == 0
    for off in (4, 8):
        assert call(sym, code, [dp[0] + off] + dp[1:], opts) == EINVAL
        assert "llrs buffer must be 16-byte aligned" in la.last_error(), la.last_error()
    assert call(sym, code, [dp[0], dp[1] + 4] + dp[2:], opts) == EINVAL
    assert "output buffer must be 8-byte aligned" in la.last_error(), la.last_error()
    torch.cuda.synchronize()
    assert untouched(dk)


def test_python_refusals_reach_the_library_with_its_texts():
    for code in (LDPCCode.TM1280, LDPCCode.TM5120, LDPCCode.TC256):
        x = np.zeros((2, code.n()), np.float32)
        with pytest.raises(la.LdpcHipError, match="f32-reading bit-sliced"):
            code.decode_ms_quantised_batch(x, bitsliced=True)
        with pytest.raises(la.LdpcHipError, match="f32-reading bit-sliced"):
            code.decode_ms_cascade_quantised_batch(x, bitsliced=True)
    with pytest.raises(ValueError, match="variant 0 only"):
        LDPCCode.TM2048.decode_ms_quantised_batch(np.zeros((2, 2048), np.float32), bitsliced=True, variant=64)


def test_a_device_set_shards_a_host_batch():
    code = LDPCCode.TM2048
    llrs = bqf.frames(code.name)
    want = first(bqf.expected_corrected(code.name, (13, 4, 0))[25], len(llrs))
    same("devices=[0, 0]", code.decode_ms_quantised_batch(llrs, "i8", bqf.SCALE, 127, 25, bitsliced=True, devices=[0, 0], **kw_of((13, 4, 0))), want)
