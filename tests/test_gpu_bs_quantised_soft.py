"""Soft output from the f32-reading bit-sliced i8 decoders and their cascade, on the GPU
(labrador_ldpc_decode_ms_bitsliced_quantised_soft_batch_i8, labrador_ldpc_decode_ms_bitsliced_quantised_corrected_soft_batch_i8,
labrador_ldpc_decode_ms_cascade_bitsliced_quantised_soft_batch_i8; LDPCCode.decode_ms_bitsliced_quantised_soft_batch and
decode_ms_cascade_bitsliced_quantised_soft_batch), bit for bit -- the marginals as well as the hard results -- against
the references of tests/bs_quantised_soft_frames.py and against the two-step route on the library's own quantiser: the four one-wave TM
codes on the 3 G + 1 frames that the CPU emulation of the same kernel text passed (tests/test_bitslice_quantised_soft_emu.py), caps
0 / 3 / 25, partial groups, host and device buffers, the cascade with both stages carrying frames, one batch of 4 G 1024 + 3 frames,
containment in guarded buffers at the least alignments, the refusals."""
import ctypes

import numpy as np
import pytest

import bs_quantised_soft_frames as bqs
import guarded_buffers as gb
import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode

pytestmark = pytest.mark.gpu

CODES = [LDPCCode[n] for n in bqs.NAMES]
CAPS = (0, 3, 25)
EINVAL, OK, EUNSUPPORTED = -1, 0, -4
PLAIN = "labrador_ldpc_decode_ms_bitsliced_quantised_soft_batch_i8"
CORRECTED = "labrador_ldpc_decode_ms_bitsliced_quantised_corrected_soft_batch_i8"
CASCADE = "labrador_ldpc_decode_ms_cascade_bitsliced_quantised_soft_batch_i8"
SOFT = ("app", "output", "iters", "success")
# the cascade's (cap, sweeps, stage-1 triple, stage-2 triple)
CASCADES = ((3, 20) + bqs.CASCADE_PAIR, (25, 25) + bqs.CASCADE_PAIR, (0, 5) + bqs.CASCADE_PAIR, (3, 20, bqs.IDENTITY, (3, 2, 1)),
            (3, 20, (1, 0, 1), bqs.IDENTITY))


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if la.device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("the f32-loader bit-sliced soft GPU tests need a gfx950 device")
    torch.cuda.set_device(0)


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def same(tag, got, want, names=SOFT):
    assert len(got) == len(want) == len(names), (tag, len(got), len(want))
    for g, w, what in zip(got, want, names):
        g, w = host(g), host(w)
        assert g.shape == w.shape, (tag, what, g.shape, w.shape)
        if what == "app":
            assert g.dtype == w.dtype, (tag, g.dtype, w.dtype)
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
def test_flooding_entries_equal_the_reference_and_the_two_step_route(code, device):
    import torch
    name = code.name
    bqs.assert_conditions(name)
    llrs = bqs.frames(name)
    x = torch.from_numpy(np.array(llrs)).cuda() if device else llrs
    sync = torch.cuda.synchronize if device else (lambda: None)
    for b in batches_of(bqs.GROUP[name]):
        for cap in CAPS:
            for lim in bqs.LIMS:
                got = code.decode_ms_bitsliced_quantised_soft_batch(x[:b], bqs.SCALE, lim, cap)
                two_step = code.decode_ms_bitsliced_soft_batch(code.quantise_llrs_batch(x[:b], "i8", bqs.SCALE, lim), cap)
                sync()
                assert host(got[0]).dtype == np.int8
                tag = f"{name} plain lim {lim} cap {cap} batch {b}"
                same(tag + ": the oracle's soft decode of the quantised frames", got, first(bqs.expected_plain(name, lim, cap), b))
                same(tag + ": quantise, then the i8 soft entry", got, two_step)
            for triple in bqs.TRIPLES:
                got = code.decode_ms_bitsliced_quantised_soft_batch(x[:b], bqs.SCALE, 127, cap, **kw_of(triple))
                two_step = code.decode_ms_bitsliced_soft_batch(code.quantise_llrs_batch(x[:b], "i8", bqs.SCALE, 127), cap, **kw_of(triple))
                sync()
                tag = f"{name} {triple} cap {cap} batch {b}"
                same(tag + ": the corrected soft statement on the quantised frames", got, first(bqs.expected_corrected(name, triple)[cap], b))
                same(tag + ": quantise, then the corrected i8 soft entry", got, two_step)
            # every spelling of the identity is the plain kernel's answer
            got = code.decode_ms_bitsliced_quantised_soft_batch(x[:b], bqs.SCALE, 127, cap, scale_num=16, scale_shift=4)
            sync()
            same(f"{name} identity cap {cap} batch {b}", got, first(bqs.expected_plain(name, 127, cap), b))
    assert not host(code.decode_ms_bitsliced_quantised_soft_batch(x, bqs.SCALE, 127, 0)[0]).any()         # (cap 0: all-zero marginals)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("code", CODES, ids=lambda c: c.name)
def test_hard_results_are_those_of_the_hard_f32_reading_entries(code, device):
    import torch
    name = code.name
    llrs = bqs.frames(name)
    x = torch.from_numpy(np.array(llrs)).cuda() if device else llrs
    for kw in ({}, kw_of((13, 4, 0))):
        got = code.decode_ms_bitsliced_quantised_soft_batch(x, bqs.SCALE, 31, 25, **kw)
        hard = code.decode_ms_quantised_batch(x, "i8", bqs.SCALE, 31, 25, bitsliced=True, **kw)
        if device:
            torch.cuda.synchronize()
        same(f"{name} {kw}: the hard entry", got[1:], hard, SOFT[1:])


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("code", CODES, ids=lambda c: c.name)
def test_cascade_entry_equals_the_composition_and_the_soft_i8_cascade_on_the_quantised_frames(code, device):
    import torch
    name = code.name
    llrs = bqs.frames(name)
    x = torch.from_numpy(np.array(llrs)).cuda() if device else llrs
    names = SOFT + ("stage",)
    stages = set()
    for cap, sweeps, t1, t2 in CASCADES:
        for b in sorted({bqs.GROUP[name] + 1, len(llrs)}):
            kw = dict(maxiters=cap, max_sweeps=sweeps, **kw_of(t2))
            fl = {} if t1 == bqs.IDENTITY else kw_of(t1, "flooding_")
            got = code.decode_ms_cascade_bitsliced_quantised_soft_batch(x[:b], bqs.SCALE, 127, **fl, **kw)
            two_step = code.decode_ms_cascade_fixed_soft_batch(code.quantise_llrs_batch(x[:b], "i8", bqs.SCALE, 127), bitsliced=True, **fl, **kw)
            if device:
                torch.cuda.synchronize()
            assert host(got[0]).dtype == np.int32
            tag = f"{name} cascade {cap, sweeps} {t1} {t2} batch {b}"
            same(tag + ": the composition of the statements", got, first(bqs.expected_cascade(name, cap, sweeps, t1, t2), b), names)
            same(tag + ": quantise, then the soft i8 cascade", got, two_step, names)
            stages |= set(host(got[4]).tolist())
            if cap and b == len(llrs):                                               # (both stages carried frames, in this very call)
                assert 0 < int(host(got[4]).sum()) < b, tag
    assert stages == {0, 1}


@pytest.mark.parametrize("code", [LDPCCode.TM2048, LDPCCode.TM1536], ids=lambda c: c.name)
def test_cascade_stage_one_in_several_chunks(code, monkeypatch):
    """stage 1 runs in chunks of the workspace (the variable is read per call): four frames each, the last one partial"""
    import torch
    name = code.name
    llrs = bqs.frames(name)
    assert len(llrs) > 8 and len(llrs) % 4
    t1, t2 = bqs.CASCADE_PAIR
    kw = dict(maxiters=3, max_sweeps=20, **kw_of(t1, "flooding_"), **kw_of(t2))
    want = bqs.expected_cascade(name, 3, 20, t1, t2)
    monkeypatch.setenv("LABRADOR_LDPC_HIP_CASCADE_CHUNK", "4")
    names = SOFT + ("stage",)
    same(f"{name} chunks host", code.decode_ms_cascade_bitsliced_quantised_soft_batch(llrs, bqs.SCALE, 127, **kw), want, names)
    got = code.decode_ms_cascade_bitsliced_quantised_soft_batch(torch.from_numpy(np.array(llrs)).cuda(), bqs.SCALE, 127, **kw)
    torch.cuda.synchronize()
    same(f"{name} chunks device", got, want, names)


@pytest.mark.parametrize("code", CODES, ids=lambda c: c.name)
def test_a_large_batch_with_a_partial_last_group(code):
    """4 G 1024 + 3 frames, the 3 G + 1 frames repeated: more than one wave per CU, many groups, the last one partial"""
    import torch
    name, g = code.name, bqs.GROUP[code.name]
    b = 4 * g * 1024 + 3
    base = bqs.frames(name)
    idx = np.arange(b) % len(base)
    d = torch.from_numpy(np.array(base)).cuda()[torch.from_numpy(idx).cuda()].contiguous()
    assert d.shape == (b, code.n()) and d.data_ptr() % 16 == 0
    q = code.quantise_llrs_batch(d, "i8", bqs.SCALE, 31)
    got = code.decode_ms_bitsliced_quantised_soft_batch(d, bqs.SCALE, 31, 25)
    two_step = code.decode_ms_bitsliced_soft_batch(q, 25)
    t1, t2 = bqs.CASCADE_PAIR
    cgot = code.decode_ms_bitsliced_quantised_soft_batch(d, bqs.SCALE, 31, 25, **kw_of(t1))
    ctwo = code.decode_ms_bitsliced_soft_batch(q, 25, **kw_of(t1))
    kw = dict(maxiters=3, max_sweeps=20, **kw_of(t1, "flooding_"), **kw_of(t2))
    sgot = code.decode_ms_cascade_bitsliced_quantised_soft_batch(d, bqs.SCALE, 31, **kw)
    stwo = code.decode_ms_cascade_fixed_soft_batch(q, bitsliced=True, **kw)
    torch.cuda.synchronize()
    same(f"{name} batch {b}: the oracle", got, tuple(a[idx] for a in bqs.expected_plain(name, 31, 25)))
    same(f"{name} batch {b}: the two-step route", got, two_step)
    same(f"{name} batch {b} {t1}: the two-step route", cgot, ctwo)
    same(f"{name} batch {b}: the two-step cascade", sgot, stwo, SOFT + ("stage",))
    assert 0 < int(host(sgot[4]).sum()) < b


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("sym", [PLAIN, CORRECTED, CASCADE])
@pytest.mark.parametrize("code", CODES, ids=lambda c: c.name)
def test_the_entries_write_only_the_callers_result_rows(code, sym, device):
    """G + 1 frames (a partial last group) in guarded views at the least alignments the header admits: llrs and app on a 16-byte
    boundary, output 8 bytes past one, iters 4 past an 8-byte one, success and stage odd."""
    import torch
    name = code.name
    b = bqs.GROUP[name] + 1
    dev = "cuda" if device else None
    npv = code.n() + code.punctured_bits()
    x, gx = gb.guarded_copy(np.array(bqs.frames(name)[:b]), 0, dev, name="llrs")
    app, ga = gb.guarded(b, (npv,), np.int32 if sym == CASCADE else np.int8, 0, dev, name="app", app=True)
    out, go = gb.guarded(b, (code.output_len(),), np.uint8, 8, dev, name="output")
    it, gi = gb.guarded(b, (), np.int32, 4, dev, name="iters", prefill=-2)
    ok, gk = gb.guarded(b, (), np.uint8, 1, dev, name="success")
    stage, gs = gb.guarded(b, (), np.uint8, 1, dev, name="stage")
    inp = gb.frozen(x, "llrs")
    ptr = (lambda t: t.data_ptr()) if device else (lambda t: t.ctypes.data)
    assert ptr(x) % 16 == 0 and ptr(app) % 16 == 0 and ptr(out) % 16 == 8 and ptr(it) % 8 == 4 and ptr(ok) % 2 == 1 and ptr(stage) % 2 == 1
    opts = la.HipOpts(0, la.MEM_DEVICE if device else la.MEM_HOST, None, 0, 0, None)
    if device:
        torch.cuda.synchronize()
    t1, t2 = bqs.CASCADE_PAIR
    if sym == PLAIN:
        st = getattr(la.lib, sym)(int(code), ptr(x), ptr(app), ptr(out), ptr(it), ptr(ok), b, 25, bqs.SCALE, 127, ctypes.byref(opts))
        want = first(bqs.expected_plain(name, 127, 25), b)
    elif sym == CORRECTED:
        st = getattr(la.lib, sym)(int(code), ptr(x), ptr(app), ptr(out), ptr(it), ptr(ok), b, 25, bqs.SCALE, 127, *t1, ctypes.byref(opts))
        want = first(bqs.expected_corrected(name, t1)[25], b)
    else:
        st = getattr(la.lib, sym)(int(code), ptr(x), ptr(app), ptr(out), ptr(it), ptr(ok), ptr(stage), b, 3, 20, bqs.SCALE, 127, *t1, *t2,
                                  ctypes.byref(opts))
        want = first(bqs.expected_cascade(name, 3, 20, t1, t2), b)
    assert st == OK, la.last_error()
    if device:
        torch.cuda.synchronize()
    for guard in (gx, ga, go, gi, gk, gs, inp):
        guard.check()
    got = (app, out, host(it).astype(np.uint32), ok) + ((stage,) if sym == CASCADE else ())
    same(f"{name} {sym} guarded", got, want, SOFT + (("stage",) if sym == CASCADE else ()))
    if sym != CASCADE:
        assert (host(stage) == 0xEE).all()                                           # (not an argument of the entry: untouched)


def raw_buffers(code, batch, device, cascade):
    """llrs, app, output, iters, success, stage with sentinel-filled results, and their addresses"""
    import torch
    npv = code.n() + code.punctured_bits()
    if device:
        t = (torch.zeros((batch, code.n() + 4), dtype=torch.float32, device="cuda"),
             torch.full((batch, npv + 16), 0x5E, dtype=torch.int32 if cascade else torch.int8, device="cuda"),
             torch.full((batch, code.output_len()), 0xEE, dtype=torch.uint8, device="cuda"),
             torch.full((batch,), -2, dtype=torch.int32, device="cuda"), torch.full((batch,), 0xEE, dtype=torch.uint8, device="cuda"),
             torch.full((batch,), 0xEE, dtype=torch.uint8, device="cuda"))
        torch.cuda.synchronize()
        return t, [a.data_ptr() for a in t]
    t = (np.zeros((batch, code.n()), np.float32), np.full((batch, npv), 0x5E, np.int32 if cascade else np.int8),
         np.full((batch, code.output_len()), 0xEE, np.uint8), np.full(batch, -2, np.int32), np.full(batch, 0xEE, np.uint8),
         np.full(batch, 0xEE, np.uint8))
    return t, [a.ctypes.data for a in t]


def untouched(t):
    return bool((host(t[1]) == 0x5E).all() and (host(t[2]) == 0xEE).all() and (host(t[3]) == -2).all() and (host(t[4]) == 0xEE).all() and
                (host(t[5]) == 0xEE).all())


def call(sym, code, p, opts=None, q=(8.0, 31), t1=(13, 4, 0), batch=2):
    o = ctypes.byref(opts) if opts is not None else None
    if sym == PLAIN:
        return getattr(la.lib, sym)(int(code), *p[:5], batch, 10, *q, o)
    if sym == CORRECTED:
        return getattr(la.lib, sym)(int(code), *p[:5], batch, 10, *q, *t1, o)
    return getattr(la.lib, sym)(int(code), *p, batch, 10, 10, *q, *t1, 13, 4, 0, o)


@pytest.mark.parametrize("sym", [PLAIN, CORRECTED, CASCADE])
def test_refusals_come_with_their_text_and_before_any_device_work(sym):
    import torch
    cascade = sym == CASCADE
    nbuf = 6 if cascade else 5
    text = "f32-reading soft bit-sliced flooding decoder"
    for code in (LDPCCode.TM1280, LDPCCode.TM5120, LDPCCode.TC128, LDPCCode.TC512):
        keep, p = raw_buffers(code, 2, False, cascade)
        assert call(sym, code, p) == EUNSUPPORTED
        assert text in la.last_error() and "TM1536, TM2048, TM6144 and TM8192" in la.last_error(), la.last_error()
        assert untouched(keep)
    code = LDPCCode.TM2048
    keep, p = raw_buffers(code, 2, False, cascade)
    for variant in (64, 1):
        opts = la.HipOpts(0, la.MEM_HOST, None, variant, 0, None)
        assert call(sym, code, p, opts) == EUNSUPPORTED
        assert f"variant {variant}" in la.last_error() and text in la.last_error(), la.last_error()
        if sym != PLAIN:                                                              # (the variant comes before the triple)
            assert call(sym, code, p, opts, t1=(1, 9, 0)) == EUNSUPPORTED and f"variant {variant}" in la.last_error()
    assert call(sym, code, p, q=(0.0, 31)) == EINVAL and "scale 0" in la.last_error()
    assert call(sym, code, p, q=(8.0, 128)) == EINVAL and "lim 128" in la.last_error()
    if sym != PLAIN:
        for triple, what in (((1, 9, 0), "scale_shift 9"), ((0, 0, 0), "scale_num 0"), ((3, 2, 128), "offset 128")):
            assert call(sym, code, p, t1=triple) == EINVAL and what in la.last_error(), la.last_error()
    # a NULL buffer, each of them, `app` (and `stage`) among them; a bad code; the empty batch with NULL pointers
    for i in range(nbuf):
        q = list(p)
        q[i] = None
        assert call(sym, code, q, t1=(1, 9, 0)) == EINVAL and "NULL buffer" in la.last_error(), (i, la.last_error())
    assert call(sym, 9, p) == EINVAL and "out of range" in la.last_error()
    assert call(sym, code, [None] * 6, batch=0, t1=(1, 9, 0)) == OK
    assert call(sym, LDPCCode.TM1280, [None] * 6, batch=0) == OK
    assert untouched(keep)
    # device rows off their alignment: llrs at 4 and at 8 mod 16, app at 8 mod 16, output at 4 mod 8
    dk, dp = raw_buffers(code, 3, True, cascade)
    opts = la.HipOpts(0, la.MEM_DEVICE, None, 0, 0, None)
    assert dp[0] % 16 == 0 and dp[1] % 16 == 0
    for off in (4, 8):
        assert call(sym, code, [dp[0] + off] + dp[1:], opts) == EINVAL
        assert "llrs buffer must be 16-byte aligned" in la.last_error(), la.last_error()
    assert call(sym, code, [dp[0], dp[1] + 8] + dp[2:], opts) == EINVAL
    assert "app buffer must be 16-byte aligned" in la.last_error(), la.last_error()
    assert call(sym, code, dp[:2] + [dp[2] + 4] + dp[3:], opts) == EINVAL
    assert "output buffer must be 8-byte aligned" in la.last_error(), la.last_error()
    torch.cuda.synchronize()
    assert untouched(dk)


def test_python_refusals_reach_the_library_with_its_texts():
    for code in (LDPCCode.TM1280, LDPCCode.TM5120, LDPCCode.TC256):
        x = np.zeros((2, code.n()), np.float32)
        with pytest.raises(la.LdpcHipError, match="f32-reading soft bit-sliced"):
            code.decode_ms_bitsliced_quantised_soft_batch(x, 8.0, 31)
        with pytest.raises(la.LdpcHipError, match="f32-reading soft bit-sliced"):
            code.decode_ms_bitsliced_quantised_soft_batch(x, 8.0, 31, offset=1)
        with pytest.raises(la.LdpcHipError, match="f32-reading soft bit-sliced"):
            code.decode_ms_cascade_bitsliced_quantised_soft_batch(x, 8.0, 31)
    code = LDPCCode.TM2048
    for bad in (np.zeros((1, code.n()), np.int8), np.zeros((1, code.n()), np.float64)):
        with pytest.raises(la.LdpcHipError, match="no batched kernel"):
            code.decode_ms_bitsliced_quantised_soft_batch(bad, 8.0, 31)
        with pytest.raises(la.LdpcHipError, match="no batched kernel"):
            code.decode_ms_cascade_bitsliced_quantised_soft_batch(bad, 8.0, 31)
    with pytest.raises(la.LdpcHipError, match="scale_shift 9"):
        code.decode_ms_cascade_bitsliced_quantised_soft_batch(np.zeros((1, code.n()), np.float32), 8.0, 31, flooding_scale_num=1,
                                                              flooding_scale_shift=9, scale_num=1, scale_shift=10)


def test_a_device_set_shards_a_host_batch():
    code = LDPCCode.TM2048
    llrs = bqs.frames(code.name)
    want = first(bqs.expected_corrected(code.name, (13, 4, 0))[25], len(llrs))
    same("devices=[0, 0]", code.decode_ms_bitsliced_quantised_soft_batch(llrs, bqs.SCALE, 127, 25, devices=[0, 0], **kw_of((13, 4, 0))), want)
    t1, t2 = bqs.CASCADE_PAIR
    same("devices=[0, 0] cascade", code.decode_ms_cascade_bitsliced_quantised_soft_batch(llrs, bqs.SCALE, 127, 3, 20, devices=[0, 0],
                                                                                        **kw_of(t1, "flooding_"), **kw_of(t2)),
         bqs.expected_cascade(code.name, 3, 20, t1, t2), SOFT + ("stage",))
