"""Soft output from the bit-sliced i8 flooding kernels, on the GPU (labrador_ldpc_decode_ms_bitsliced_soft_batch_i8,
labrador_ldpc_decode_ms_cascade_bitsliced_soft_batch_i8; LDPCCode.decode_ms_bitsliced_soft_batch and the `bitsliced` keyword of
decode_ms_cascade_fixed_soft_batch), bit for bit against the oracle, the f32-pipe soft entry and the lockstep hard
kernel: the four one-wave TM codes on the 3 G + 1 frames of tests/bs_soft_frames.py (what the CPU emulation of the same kernel text
passed, tests/test_bitslice_soft_emu.py), caps 0 / 1 / 3 / 25, host and device buffers, partial groups, containment in guarded
buffers at the least alignments, the cascade against the existing one, the refusals with their texts, a device set."""
import ctypes

import numpy as np
import pytest

import bs_soft_frames as bsf
import guarded_buffers as gb
import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode
import oracle

pytestmark = pytest.mark.gpu

CODES = [LDPCCode[n] for n in bsf.NAMES]
EINVAL, OK, EUNSUPPORTED = -1, 0, -4
SYM = "labrador_ldpc_decode_ms_bitsliced_soft_batch_i8"
CASCADE_SYM = "labrador_ldpc_decode_ms_cascade_bitsliced_soft_batch_i8"
LOCKSTEP = 64 | 256                                       # the bit-sliced kernel whatever the batch size, in its lockstep form


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if la.device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("the bit-sliced soft GPU tests need a gfx950 device")
    torch.cuda.set_device(0)


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def same(tag, got, want, names=("app", "output", "iters", "success")):
    assert len(got) == len(want) == len(names)
    for g, w, what in zip(got, want, names):
        g, w = host(g), host(w)
        assert g.shape == w.shape, (tag, what, g.shape, w.shape)
        bad = np.flatnonzero((g.reshape(len(w), -1).astype(np.int64) != w.reshape(len(w), -1).astype(np.int64)).any(axis=1))
        assert bad.size == 0, f"{tag}: {what} differs in frames {bad.tolist()[:8]}"


def oracle_soft(name, cap, b):
    o, it, ok, va = bsf.expected(name, cap)
    return va[:b], o[:b], it[:b], ok[:b]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("code", CODES, ids=lambda c: c.name)
def test_new_entry_equals_the_oracle_the_soft_entry_and_the_lockstep_hard_kernel(code, device):
    import torch
    bsf.assert_conditions(code.name)
    llrs = bsf.frames(code.name)
    x = torch.from_numpy(np.array(llrs)).cuda() if device else llrs
    b = len(llrs)
    for cap in bsf.CAPS:
        got = code.decode_ms_bitsliced_soft_batch(x, cap)
        pipe = code.decode_ms_soft_batch(x, cap)
        hard = code.decode_ms_batch(x, cap, variant=LOCKSTEP)
        if device:
            torch.cuda.synchronize()
        assert host(got[0]).dtype == np.int8
        same(f"{code.name} cap {cap}: the oracle", got, oracle_soft(code.name, cap, b))
        same(f"{code.name} cap {cap}: the f32-pipe soft entry", got, pipe)
        same(f"{code.name} cap {cap}: the lockstep hard kernel", got[1:], hard, ("output", "iters", "success"))
    assert not host(code.decode_ms_bitsliced_soft_batch(x, 0)[0]).any()


@pytest.mark.parametrize("code", CODES, ids=lambda c: c.name)
def test_partial_groups(code):
    import torch
    g = bsf.GROUP[code.name]
    llrs = bsf.frames(code.name)
    d = torch.from_numpy(np.array(llrs)).cuda()
    for b in sorted({b for b in (1, g - 1, g + 1) if b >= 1}):
        for cap in (3, 25):
            want = oracle_soft(code.name, cap, b)
            same(f"{code.name} batch {b} cap {cap} host", code.decode_ms_bitsliced_soft_batch(llrs[:b], cap), want)
            got = code.decode_ms_bitsliced_soft_batch(d[:b], cap)
            torch.cuda.synchronize()
            same(f"{code.name} batch {b} cap {cap} device", got, want)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("code", CODES, ids=lambda c: c.name)
def test_the_entry_writes_only_the_callers_result_rows(code, device):
    """G + 1 frames (a partial last group) into guarded views at the least alignments the header admits: app on a 16-byte boundary,
    output 8 bytes past one, iters 4 past an 8-byte one, success odd, llrs 4 bytes past a 16-byte boundary."""
    import torch
    b = bsf.GROUP[code.name] + 1
    dev = "cuda" if device else None
    llrs = np.array(bsf.frames(code.name)[:b])
    x, gx = gb.guarded_copy(llrs, 4, dev, name="llrs")
    app, ga = gb.guarded(b, (code.n() + code.punctured_bits(),), np.int8, 0, dev, name="app", app=True)
    out, go = gb.guarded(b, (code.output_len(),), np.uint8, 8, dev, name="output")
    it, gi = gb.guarded(b, (), np.int32, 4, dev, name="iters", prefill=-2)
    ok, gk = gb.guarded(b, (), np.uint8, 1, dev, name="success")
    inp = gb.frozen(x, "llrs")
    ptr = (lambda t: t.data_ptr()) if device else (lambda t: t.ctypes.data)
    assert ptr(app) % 16 == 0 and ptr(out) % 16 == 8 and ptr(it) % 8 == 4 and ptr(ok) % 2 == 1 and ptr(x) % 16 == 4
    opts = la.HipOpts(0, la.MEM_DEVICE if device else la.MEM_HOST, None, 0, 0, None)
    if device:
        torch.cuda.synchronize()
    st = getattr(la.lib, SYM)(int(code), ptr(x), ptr(app), ptr(out), ptr(it), ptr(ok), b, 25, ctypes.byref(opts))
    assert st == OK, la.last_error()
    if device:
        torch.cuda.synchronize()
    for guard in (gx, ga, go, gi, gk, inp):
        guard.check()
    same(f"{code.name} guarded", (app, out, host(it).astype(np.uint32), ok), oracle_soft(code.name, 25, b))


def cascade_frames(code):
    """half the frames at 9 dB, where flooding converges at iteration 2 or 3, half a little below the emulation's threshold frames,
    shuffled: at cap 3 stage 1 decodes some and fails the rest (the test asserts that both stages occur)"""
    rng = np.random.default_rng(4260 + int(code))
    frames = 3 * bsf.GROUP[code.name] + 29
    clean, _ = oracle.awgn_llrs(code, rng, frames // 2, 9.0, np.int8)
    noisy, _ = oracle.awgn_llrs(code, rng, frames - frames // 2, 1.6 if code is LDPCCode.TM2048 else 2.4, np.int8)
    return np.ascontiguousarray(np.concatenate([clean, noisy])[rng.permutation(frames)])


@pytest.mark.parametrize("code", [LDPCCode.TM2048, LDPCCode.TM1536], ids=lambda c: c.name)
def test_cascade_equals_the_existing_soft_cascade(code, monkeypatch):
    import torch
    llrs = cascade_frames(code)
    d = torch.from_numpy(llrs).cuda()
    names = ("app", "output", "iters", "success", "stage")
    both = False
    for cap, sweeps in ((3, 20), (0, 5)):
        kw = dict(maxiters=cap, max_sweeps=sweeps)
        want = code.decode_ms_cascade_fixed_soft_batch(llrs, bitsliced=False, **kw)
        assert want[0].dtype == np.int32
        stage = want[4]
        both |= bool(stage.any() and not stage.all())
        same(f"{code.name} caps {cap, sweeps} host", code.decode_ms_cascade_fixed_soft_batch(llrs, bitsliced=True, **kw), want, names)
        got = code.decode_ms_cascade_fixed_soft_batch(d, bitsliced=True, **kw)
        torch.cuda.synchronize()
        same(f"{code.name} caps {cap, sweeps} device", got, want, names)
        same(f"{code.name} caps {cap, sweeps} device, bitsliced=False", code.decode_ms_cascade_fixed_soft_batch(d, **kw), want, names)
        if cap:
            # stage 1 in several chunks (the variable is read per call), the last one partial
            with monkeypatch.context() as m:
                m.setenv("LABRADOR_LDPC_HIP_CASCADE_CHUNK", "5")
                assert len(llrs) > 10 and len(llrs) % 5
                same(f"{code.name} chunks host", code.decode_ms_cascade_fixed_soft_batch(llrs, bitsliced=True, **kw), want, names)
                got = code.decode_ms_cascade_fixed_soft_batch(d, bitsliced=True, **kw)
                torch.cuda.synchronize()
                same(f"{code.name} chunks device", got, want, names)
    assert both                                                          # (at one of the caps both stages carry frames)


def raw_buffers(code, batch, device):
    """llrs, app, output, iters, success with sentinel-filled results, and their addresses"""
    import torch
    npv = code.n() + code.punctured_bits()
    if device:
        t = (torch.zeros((batch, code.n()), dtype=torch.int8, device="cuda"), torch.full((batch, npv), 0x5E, dtype=torch.int8, device="cuda"),
             torch.full((batch, code.output_len()), 0xEE, dtype=torch.uint8, device="cuda"),
             torch.full((batch,), -2, dtype=torch.int32, device="cuda"), torch.full((batch,), 0xEE, dtype=torch.uint8, device="cuda"))
        torch.cuda.synchronize()
        return t, [x.data_ptr() for x in t]
    t = (np.zeros((batch, code.n()), np.int8), np.full((batch, npv), 0x5E, np.int8), np.full((batch, code.output_len()), 0xEE, np.uint8),
         np.full(batch, -2, np.int32), np.full(batch, 0xEE, np.uint8))
    return t, [x.ctypes.data for x in t]


def untouched(t):
    return bool((host(t[1]) == 0x5E).all() and (host(t[2]) == 0xEE).all() and (host(t[3]) == -2).all() and (host(t[4]) == 0xEE).all())


def test_refusals_come_with_their_text_and_before_any_device_work():
    import torch
    fn = getattr(la.lib, SYM)
    # code families: a TC code; the two rate-4/5 codes, whose text names the two-wave kernels
    for code, text in ((LDPCCode.TC128, "soft bit-sliced flooding decoder"), (LDPCCode.TM1280, "two-wave"), (LDPCCode.TM5120, "two-wave")):
        keep, p = raw_buffers(code, 2, False)
        assert fn(int(code), *p, 2, 10, None) == EUNSUPPORTED
        assert text in la.last_error() and "soft" in la.last_error(), la.last_error()
        assert untouched(keep)
        with pytest.raises(la.LdpcHipError):
            code.decode_ms_bitsliced_soft_batch(np.zeros((2, code.n()), np.int8))
    code = LDPCCode.TM2048
    keep, p = raw_buffers(code, 2, False)
    for variant in (64, 1):
        opts = la.HipOpts(0, la.MEM_HOST, None, variant, 0, None)
        assert fn(int(code), *p, 2, 10, ctypes.byref(opts)) == EUNSUPPORTED
        assert f"variant {variant}" in la.last_error() and "soft bit-sliced flooding decoder" in la.last_error(), la.last_error()
    # a NULL buffer, each of the five, `app` among them; a bad code; the empty batch with NULL pointers
    for i in range(5):
        q = list(p)
        q[i] = None
        assert fn(int(code), *q, 2, 10, None) == EINVAL and "NULL buffer" in la.last_error(), (i, la.last_error())
    assert fn(9, *p, 2, 10, None) == EINVAL and "out of range" in la.last_error()
    assert fn(int(code), None, None, None, None, None, 0, 10, None) == OK
    assert fn(int(LDPCCode.TM1280), None, None, None, None, None, 0, 10, None) == OK       # (an empty batch never gets as far as the code family)
    assert untouched(keep)
    # device buffers off their alignment: llrs at 2 mod 4, app at 8 mod 16
    dk, dp = raw_buffers(code, 3, True)
    opts = la.HipOpts(0, la.MEM_DEVICE, None, 0, 0, None)
    assert fn(int(code), dp[0] + 2, *dp[1:], 2, 10, ctypes.byref(opts)) == EINVAL
    assert "llrs buffer must be 4-byte aligned" in la.last_error(), la.last_error()
    assert fn(int(code), dp[0], dp[1] + 8, *dp[2:], 2, 10, ctypes.byref(opts)) == EINVAL
    assert "app buffer must be 16-byte aligned" in la.last_error(), la.last_error()
    torch.cuda.synchronize()
    assert untouched(dk)
    # the Python method: any other dtype
    for bad in (np.zeros((1, code.n()), np.int16), np.zeros((1, code.n()), np.float32)):
        with pytest.raises(la.LdpcHipError):
            code.decode_ms_bitsliced_soft_batch(bad)


def test_cascade_refusals():
    import torch
    fn = getattr(la.lib, CASCADE_SYM)
    for code, text in ((LDPCCode.TC256, "soft bit-sliced flooding decoder"), (LDPCCode.TM1280, "two-wave"), (LDPCCode.TM5120, "two-wave")):
        with pytest.raises(la.LdpcHipError, match=text):
            code.decode_ms_cascade_fixed_soft_batch(np.zeros((2, code.n()), np.int8), bitsliced=True)
    code = LDPCCode.TM2048
    q = np.zeros((2, code.n()), np.int8)
    for variant in (64, 1):
        with pytest.raises(la.LdpcHipError, match=f"variant {variant}"):
            code.decode_ms_cascade_fixed_soft_batch(q, bitsliced=True, variant=variant)
    with pytest.raises(la.LdpcHipError, match="scale_shift"):
        code.decode_ms_cascade_fixed_soft_batch(q, bitsliced=True, scale_num=1, scale_shift=9)
    with pytest.raises(la.LdpcHipError):
        code.decode_ms_cascade_fixed_soft_batch(np.zeros((2, code.n()), np.int16), bitsliced=True)
    # the existing entry still refuses `variant` 64 with its own text
    with pytest.raises(la.LdpcHipError, match="no soft-output form"):
        code.decode_ms_cascade_fixed_soft_batch(q, variant=64)
    # device llrs at 2 mod 4; a NULL app; the empty batch
    npv = code.n() + code.punctured_bits()
    flat = torch.zeros(2 * code.n() + 16, dtype=torch.int8, device="cuda")
    app = torch.full((2, npv), 0x5E5E5E5E, dtype=torch.int32, device="cuda")
    out = torch.full((2, code.output_len()), 0xEE, dtype=torch.uint8, device="cuda")
    it = torch.full((2,), -2, dtype=torch.int32, device="cuda")
    ok, stage = torch.full((2,), 0xEE, dtype=torch.uint8, device="cuda"), torch.full((2,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    opts = la.HipOpts(0, la.MEM_DEVICE, None, 0, 0, None)
    tail = (out.data_ptr(), it.data_ptr(), ok.data_ptr(), stage.data_ptr(), 2, 10, 10, 1, 0, 0, ctypes.byref(opts))
    assert fn(int(code), flat.data_ptr() + 2, app.data_ptr(), *tail) == EINVAL and "llrs buffer must be 4-byte aligned" in la.last_error()
    assert fn(int(code), flat.data_ptr(), None, *tail) == EINVAL and "NULL buffer" in la.last_error()
    assert fn(int(code), None, None, None, None, None, None, 0, 10, 10, 1, 0, 0, None) == OK
    torch.cuda.synchronize()
    assert bool((app == 0x5E5E5E5E).all() and (out == 0xEE).all() and (it == -2).all() and (ok == 0xEE).all() and (stage == 0xEE).all())


def test_a_device_set_shards_a_host_batch():
    code = LDPCCode.TM2048
    llrs = bsf.frames(code.name)
    want = code.decode_ms_bitsliced_soft_batch(llrs, 25)
    same("devices=[0, 0]", code.decode_ms_bitsliced_soft_batch(llrs, 25, devices=[0, 0]), want)
    same("devices=[0, 0] against the oracle", want, oracle_soft(code.name, 25, len(llrs)))
