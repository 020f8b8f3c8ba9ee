"""Soft output from the corrected bit-sliced i8 flooding kernels, on the GPU (labrador_ldpc_decode_ms_bitsliced_corrected_soft_batch_i8,
labrador_ldpc_decode_ms_cascade_bitsliced_corrected_soft_batch_i8; the triple keywords of LDPCCode.decode_ms_bitsliced_soft_batch and
the flooding_* keywords of decode_ms_cascade_fixed_soft_batch), bit for bit against the statement
(tests/flooding_fixed_corrected_soft_restatement.py) and the hard corrected entry: the four one-wave TM codes on the 3 G + 1 frames of
tests/bs_soft_frames.py (what the CPU emulation of the same kernel text passed, tests/test_bitslice_corrected_soft_emu.py), six
triples, caps 0 / 1 / 3 / 25, host and device buffers, the identity against the plain soft entry, partial groups, containment in
guarded buffers at the least alignments, the cascade against the composition of the separate calls and against the hard corrected
cascade, the refusals with their texts, a device set."""
import ctypes

import numpy as np
import pytest

import bs_corrected_soft_frames as bcf
import guarded_buffers as gb
import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode
import oracle

pytestmark = pytest.mark.gpu

CODES = [LDPCCode[n] for n in bcf.NAMES]
EINVAL, OK, EUNSUPPORTED = -1, 0, -4
SYM = "labrador_ldpc_decode_ms_bitsliced_corrected_soft_batch_i8"
CASCADE_SYM = "labrador_ldpc_decode_ms_cascade_bitsliced_corrected_soft_batch_i8"


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if la.device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("the corrected bit-sliced soft GPU tests need a gfx950 device")
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


def kw_of(triple):
    return dict(scale_num=triple[0], scale_shift=triple[1], offset=triple[2])


def stated(name, triple, cap, b):
    o, it, ok, va = bcf.expected(name, triple)[cap]
    return va[:b], o[:b], it[:b], ok[:b]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("code", CODES, ids=lambda c: c.name)
def test_new_entry_equals_the_statement_and_the_hard_corrected_entry(code, device):
    import torch
    bcf.assert_conditions(code.name)
    llrs = bcf.frames(code.name)
    x = torch.from_numpy(np.array(llrs)).cuda() if device else llrs
    b = len(llrs)
    for triple in bcf.TRIPLES:
        for cap in bcf.CAPS:
            got = code.decode_ms_bitsliced_soft_batch(x, cap, **kw_of(triple))
            hard = code.decode_ms_corrected_fixed_batch(x, *triple, maxiters=cap)
            if device:
                torch.cuda.synchronize()
            assert host(got[0]).dtype == np.int8
            same(f"{code.name} {triple} cap {cap}: the statement", got, stated(code.name, triple, cap, b))
            same(f"{code.name} {triple} cap {cap}: the hard corrected entry", got[1:], hard, ("output", "iters", "success"))
        assert not host(code.decode_ms_bitsliced_soft_batch(x, 0, **kw_of(triple))[0]).any()


@pytest.mark.parametrize("code", CODES, ids=lambda c: c.name)
def test_identity_triples_equal_the_plain_soft_entry(code):
    """(1,0,0) and (16,4,0) run the offset-only form, (255,8,0) the widest multiplier: the plain soft kernel's four results each time"""
    import torch
    llrs = bcf.frames(code.name)
    d = torch.from_numpy(np.array(llrs)).cuda()
    for cap in bcf.CAPS:
        want = code.decode_ms_bitsliced_soft_batch(d, cap)
        for triple in ((1, 0, 0), (16, 4, 0), (255, 8, 0)):
            got = code.decode_ms_bitsliced_soft_batch(d, cap, **kw_of(triple))
            torch.cuda.synchronize()
            same(f"{code.name} {triple} cap {cap}", got, want)


@pytest.mark.parametrize("code", CODES, ids=lambda c: c.name)
def test_partial_groups(code):
    import torch
    g = bcf.GROUP[code.name]
    llrs = bcf.frames(code.name)
    d = torch.from_numpy(np.array(llrs)).cuda()
    for triple in ((13, 4, 0), (209, 8, 1)):
        for b in sorted({b for b in (1, g - 1, g + 1) if b >= 1}):
            for cap in (3, 25):
                want = stated(code.name, triple, cap, b)
                same(f"{code.name} {triple} batch {b} cap {cap} host", code.decode_ms_bitsliced_soft_batch(llrs[:b], cap, **kw_of(triple)), want)
                got = code.decode_ms_bitsliced_soft_batch(d[:b], cap, **kw_of(triple))
                torch.cuda.synchronize()
                same(f"{code.name} {triple} batch {b} cap {cap} device", got, want)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("code", CODES, ids=lambda c: c.name)
def test_the_entry_writes_only_the_callers_result_rows(code, device):
    """G + 1 frames (a partial last group) into guarded views at the least alignments the header admits: app on a 16-byte boundary,
    output 8 bytes past one, iters 4 past an 8-byte one, success odd, llrs 4 bytes past a 16-byte boundary."""
    import torch
    b = bcf.GROUP[code.name] + 1
    dev = "cuda" if device else None
    triple = (13, 4, 0)
    llrs = np.array(bcf.frames(code.name)[:b])
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
    st = getattr(la.lib, SYM)(int(code), ptr(x), ptr(app), ptr(out), ptr(it), ptr(ok), b, 25, *triple, ctypes.byref(opts))
    assert st == OK, la.last_error()
    if device:
        torch.cuda.synchronize()
    for guard in (gx, ga, go, gi, gk, inp):
        guard.check()
    same(f"{code.name} guarded", (app, out, host(it).astype(np.uint32), ok), stated(code.name, triple, 25, b))


def cascade_frames(code):
    """half the frames at 9 dB, where flooding converges at iteration 2 or 3, half a little below the emulation's threshold frames,
    shuffled: at cap 3 stage 1 decodes some and fails the rest (the test asserts that both stages occur)"""
    rng = np.random.default_rng(4280 + int(code))
    frames = 3 * bcf.GROUP[code.name] + 29
    clean, _ = oracle.awgn_llrs(code, rng, frames // 2, 9.0, np.int8)
    noisy, _ = oracle.awgn_llrs(code, rng, frames - frames // 2, 1.6 if code is LDPCCode.TM2048 else 2.4, np.int8)
    return np.ascontiguousarray(np.concatenate([clean, noisy])[rng.permutation(frames)])


def composed(code, llrs, cap, sweeps, t1, t2):
    """the two separate soft calls, per frame: the new entry at cap `cap`, the soft fixed-point layered entry on what it failed"""
    a1, o1, i1, s1 = (host(r).copy() for r in code.decode_ms_bitsliced_soft_batch(llrs, cap, **kw_of(t1)))
    app, out, it, ok = a1.astype(np.int32), o1, i1, s1
    stage = (s1 == 0).astype(np.uint8)
    lost = np.flatnonzero(stage)
    if lost.size:
        a2, o2, i2, s2 = code.decode_ms_layered_fixed_soft_batch(np.ascontiguousarray(llrs[lost]), sweeps, **kw_of(t2))
        app[lost], out[lost], it[lost], ok[lost] = a2, o2, i2, s2
    return app, out, it, ok, stage


@pytest.mark.parametrize("code", [LDPCCode.TM2048, LDPCCode.TM1536], ids=lambda c: c.name)
def test_cascade_equals_the_composition_and_the_hard_corrected_cascade(code, monkeypatch):
    import torch
    llrs = cascade_frames(code)
    d = torch.from_numpy(llrs).cuda()
    names = ("app", "output", "iters", "success", "stage")
    t2 = (13, 4, 1)
    both = False
    for t1 in ((13, 4, 0), (1, 0, 1), (209, 8, 1)):
        fkw = {"flooding_" + k: v for k, v in kw_of(t1).items()}
        for cap, sweeps in ((3, 20), (0, 5)):
            kw = dict(maxiters=cap, max_sweeps=sweeps, **fkw, **kw_of(t2))
            want = composed(code, llrs, cap, sweeps, t1, t2)
            stage = want[4]
            both |= bool(stage.any() and not stage.all())
            got = code.decode_ms_cascade_fixed_soft_batch(llrs, bitsliced=True, **kw)
            assert got[0].dtype == np.int32
            same(f"{code.name} {t1} caps {cap, sweeps} host", got, want, names)
            hard = code.decode_ms_cascade_fixed_batch(llrs, **kw)
            same(f"{code.name} {t1} caps {cap, sweeps}: the hard corrected cascade", got[1:], hard, names[1:])
            gd = code.decode_ms_cascade_fixed_soft_batch(d, bitsliced=True, **kw)
            torch.cuda.synchronize()
            same(f"{code.name} {t1} caps {cap, sweeps} device", gd, want, names)
            if cap and t1 == (13, 4, 0):
                # stage 1 in several chunks (the variable is read per call), the last one partial
                with monkeypatch.context() as m:
                    m.setenv("LABRADOR_LDPC_HIP_CASCADE_CHUNK", "5")
                    assert len(llrs) > 10 and len(llrs) % 5
                    same(f"{code.name} chunks host", code.decode_ms_cascade_fixed_soft_batch(llrs, bitsliced=True, **kw), want, names)
                    gd = code.decode_ms_cascade_fixed_soft_batch(d, bitsliced=True, **kw)
                    torch.cuda.synchronize()
                    same(f"{code.name} chunks device", gd, want, names)
        assert both, t1                                                      # (at one of the caps both stages carry frames)
        both = False
    # an identity stage-1 triple is the plain bit-sliced soft cascade
    kw = dict(maxiters=3, max_sweeps=20, **kw_of(t2))
    same(f"{code.name} identity stage 1", code.decode_ms_cascade_fixed_soft_batch(llrs, bitsliced=True, flooding_scale_num=16, flooding_scale_shift=4, **kw),
         code.decode_ms_cascade_fixed_soft_batch(llrs, bitsliced=True, **kw), names)


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
    # code families: a TC code; the two rate-4/5 codes, whose text names the two-wave kernels -- at an identity triple as well
    for code, text in ((LDPCCode.TC128, "soft bit-sliced flooding decoder"), (LDPCCode.TM1280, "two-wave"), (LDPCCode.TM5120, "two-wave")):
        keep, p = raw_buffers(code, 2, False)
        for triple in ((13, 4, 0), (1, 0, 0)):
            assert fn(int(code), *p, 2, 10, *triple, None) == EUNSUPPORTED
            assert text in la.last_error() and "soft" in la.last_error(), la.last_error()
        assert fn(int(code), *p, 2, 10, 13, 9, 0, None) == EINVAL and "scale_shift 9" in la.last_error()        # the triple comes first
        assert untouched(keep)
        with pytest.raises(la.LdpcHipError, match=text):
            code.decode_ms_bitsliced_soft_batch(np.zeros((2, code.n()), np.int8), offset=1)
    code = LDPCCode.TM2048
    keep, p = raw_buffers(code, 2, False)
    for variant in (64, 1):
        opts = la.HipOpts(0, la.MEM_HOST, None, variant, 0, None)
        assert fn(int(code), *p, 2, 10, 13, 4, 0, ctypes.byref(opts)) == EUNSUPPORTED
        assert f"variant {variant}" in la.last_error() and "soft bit-sliced flooding decoder" in la.last_error(), la.last_error()
        assert fn(int(code), *p, 2, 10, 17, 4, 0, ctypes.byref(opts)) == EINVAL and "scale_num 17" in la.last_error()
    for triple, text in (((1, 9, 0), "scale_shift 9"), ((0, 0, 0), "scale_num 0"), ((3, 2, 128), "offset 128")):
        assert fn(int(code), *p, 2, 10, *triple, None) == EINVAL and text in la.last_error(), la.last_error()
    # a NULL buffer, each of the five, `app` among them, before the triple; a bad code; the empty batch with NULL pointers
    for i in range(5):
        q = list(p)
        q[i] = None
        assert fn(int(code), *q, 2, 10, 1, 9, 0, None) == EINVAL and "NULL buffer" in la.last_error(), (i, la.last_error())
    assert fn(9, *p, 2, 10, 1, 9, 0, None) == EINVAL and "out of range" in la.last_error()
    assert fn(int(code), None, None, None, None, None, 0, 10, 1, 9, 0, None) == OK
    assert fn(int(LDPCCode.TM1280), None, None, None, None, None, 0, 10, 13, 4, 0, None) == OK
    assert untouched(keep)
    # device buffers off their alignment: llrs at 2 mod 4, app at 8 mod 16, output at 4 mod 8
    dk, dp = raw_buffers(code, 3, True)
    opts = la.HipOpts(0, la.MEM_DEVICE, None, 0, 0, None)
    assert fn(int(code), dp[0] + 2, *dp[1:], 2, 10, 13, 4, 0, ctypes.byref(opts)) == EINVAL
    assert "llrs buffer must be 4-byte aligned" in la.last_error(), la.last_error()
    assert fn(int(code), dp[0], dp[1] + 8, *dp[2:], 2, 10, 13, 4, 0, ctypes.byref(opts)) == EINVAL
    assert "app buffer must be 16-byte aligned" in la.last_error(), la.last_error()
    assert fn(int(code), dp[0], dp[1], dp[2] + 4, *dp[3:], 2, 10, 13, 4, 0, ctypes.byref(opts)) == EINVAL
    assert "output buffer must be 8-byte aligned" in la.last_error(), la.last_error()
    torch.cuda.synchronize()
    assert untouched(dk)
    # the Python method: any other dtype
    for bad in (np.zeros((1, code.n()), np.int16), np.zeros((1, code.n()), np.float32)):
        with pytest.raises(la.LdpcHipError):
            code.decode_ms_bitsliced_soft_batch(bad, scale_num=13, scale_shift=4)


def test_cascade_refusals():
    import torch
    fn = getattr(la.lib, CASCADE_SYM)
    fl = dict(flooding_scale_num=13, flooding_scale_shift=4)
    for code, text in ((LDPCCode.TC256, "soft bit-sliced flooding decoder"), (LDPCCode.TM1280, "two-wave"), (LDPCCode.TM5120, "two-wave")):
        with pytest.raises(la.LdpcHipError, match=text):
            code.decode_ms_cascade_fixed_soft_batch(np.zeros((2, code.n()), np.int8), bitsliced=True, **fl)
    code = LDPCCode.TM2048
    q = np.zeros((2, code.n()), np.int8)
    for variant in (64, 1):
        with pytest.raises(la.LdpcHipError, match=f"variant {variant}"):
            code.decode_ms_cascade_fixed_soft_batch(q, bitsliced=True, variant=variant, **fl)
    with pytest.raises(la.LdpcHipError, match="scale_shift 9"):
        code.decode_ms_cascade_fixed_soft_batch(q, bitsliced=True, flooding_scale_num=1, flooding_scale_shift=9, scale_num=1, scale_shift=10)
    with pytest.raises(la.LdpcHipError, match="scale_shift 10"):
        code.decode_ms_cascade_fixed_soft_batch(q, bitsliced=True, scale_num=1, scale_shift=10, **fl)
    with pytest.raises(la.LdpcHipError):
        code.decode_ms_cascade_fixed_soft_batch(np.zeros((2, code.n()), np.int16), bitsliced=True, **fl)
    with pytest.raises(ValueError, match="only bit-sliced"):
        code.decode_ms_cascade_fixed_soft_batch(q, **fl)
    # device llrs at 2 mod 4; a NULL app; the empty batch
    npv = code.n() + code.punctured_bits()
    flat = torch.zeros(2 * code.n() + 16, dtype=torch.int8, device="cuda")
    app = torch.full((2, npv), 0x5E5E5E5E, dtype=torch.int32, device="cuda")
    out = torch.full((2, code.output_len()), 0xEE, dtype=torch.uint8, device="cuda")
    it = torch.full((2,), -2, dtype=torch.int32, device="cuda")
    ok, stage = torch.full((2,), 0xEE, dtype=torch.uint8, device="cuda"), torch.full((2,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    opts = la.HipOpts(0, la.MEM_DEVICE, None, 0, 0, None)
    tail = (out.data_ptr(), it.data_ptr(), ok.data_ptr(), stage.data_ptr(), 2, 10, 10, 13, 4, 0, 1, 0, 0, ctypes.byref(opts))
    assert fn(int(code), flat.data_ptr() + 2, app.data_ptr(), *tail) == EINVAL and "llrs buffer must be 4-byte aligned" in la.last_error()
    assert fn(int(code), flat.data_ptr(), None, *tail) == EINVAL and "NULL buffer" in la.last_error()
    assert fn(int(code), None, None, None, None, None, None, 0, 10, 10, 13, 4, 0, 1, 0, 0, None) == OK
    torch.cuda.synchronize()
    assert bool((app == 0x5E5E5E5E).all() and (out == 0xEE).all() and (it == -2).all() and (ok == 0xEE).all() and (stage == 0xEE).all())


def test_a_device_set_shards_a_host_batch():
    code = LDPCCode.TM2048
    triple = (13, 4, 0)
    llrs = bcf.frames(code.name)
    want = code.decode_ms_bitsliced_soft_batch(llrs, 25, **kw_of(triple))
    same("devices=[0, 0]", code.decode_ms_bitsliced_soft_batch(llrs, 25, devices=[0, 0], **kw_of(triple)), want)
    same("devices=[0, 0] against the statement", want, stated(code.name, triple, 25, len(llrs)))
