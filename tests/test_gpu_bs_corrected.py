"""Normalized / offset min-sum on the bit-sliced i8 flooding kernels of the TM codes, on the GPU (labrador_ldpc_decode_ms_corrected_batch_i8,
labrador_ldpc_decode_ms_cascade_corrected_batch_i8, labrador_ldpc_decode_ms_cascade_quantised_corrected_batch_i8;
LDPCCode.decode_ms_corrected_fixed_batch and the flooding_* keywords of the two integer cascades) against the CPU
statement of the contract (tests/flooding_fixed_corrected_restatement.py), bit for bit: output, iters and success -- all six codes,
batches of 1, G + 1 and 3 G + 1 codewords (G per wave or wave pair), caps 0 / 1 / 25, host and device buffers, three triples; the
identity triple against decode_ms_batch; the refusals, each with its text; containment in guarded buffers; the cascades against the
composition of the separate calls."""
import ctypes

import numpy as np
import pytest

import cascade_restatement
import edge_frames
import flooding_fixed_corrected_restatement as fr
import guarded_buffers as gb
import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode
import oracle

pytestmark = pytest.mark.gpu

TM = [LDPCCode.TM1280, LDPCCode.TM1536, LDPCCode.TM2048, LDPCCode.TM5120, LDPCCode.TM6144, LDPCCode.TM8192]
G = {LDPCCode.TM1280: 16, LDPCCode.TM1536: 8, LDPCCode.TM2048: 4, LDPCCode.TM5120: 4, LDPCCode.TM6144: 2, LDPCCode.TM8192: 1}
EBN0 = {LDPCCode.TM1280: 3.7, LDPCCode.TM1536: 2.7, LDPCCode.TM2048: 1.9, LDPCCode.TM5120: 3.5, LDPCCode.TM6144: 2.5, LDPCCode.TM8192: 1.8}
TRIPLES = [(13, 4, 0), (1, 0, 1), (3, 2, 1)]
CAPS = (0, 1, 25)
EINVAL, OK, EUNSUPPORTED = -1, 0, -4
SYM = "labrador_ldpc_decode_ms_corrected_batch_i8"


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if la.device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("the corrected bit-sliced GPU tests need a gfx950 device")
    torch.cuda.set_device(0)


def frames_of(code, rng, frames):
    """near-threshold AWGN frames quantised at the library's default scale 8, the last three replaced by corner rows (full scale of
    random sign, full scale mixed with 0 and +-1, noisy and clipped with -128 among them)"""
    llrs, _ = oracle.awgn_llrs(code, rng, frames, EBN0[code], np.int8)
    if frames >= 7:
        llrs[-3:] = edge_frames.integer_range_rows(code, np.int8, rng, 1)
    return llrs


def same(tag, got, want):
    for g, w, what in zip(got, want, ("output", "iters", "success")):
        g = g.cpu().numpy() if hasattr(g, "cpu") else np.asarray(g)
        bad = np.flatnonzero((g.reshape(len(w), -1) != np.asarray(w).reshape(len(w), -1)).any(axis=1))
        assert bad.size == 0, f"{tag}: {what} differs in frames {bad.tolist()[:8]}"


@pytest.mark.parametrize("code", TM, ids=lambda c: c.name)
def test_kernels_equal_the_statement(code):
    import torch
    g = G[code]
    llrs = frames_of(code, np.random.default_rng(4140 + int(code)), 3 * g + 1)
    d = torch.from_numpy(llrs).cuda()
    st = fr.structure(int(code))
    iterated = changed = False
    plain = {cap: oracle.decode_ms_batch(int(code), llrs, cap)[:3] for cap in CAPS}
    for triple in TRIPLES:
        want = fr.decode_caps(st, llrs, CAPS, *triple)
        iterated |= bool(((want[25][2] == 1) & (want[25][1] > 0)).any())
        changed |= any((x != y).any() for x, y in zip(want[25], plain[25]))
        for cap in CAPS:
            for b in (1, g + 1, 3 * g + 1):
                ref = tuple(x[:b] for x in want[cap])
                same(f"{code.name} {triple} cap {cap} batch {b} host", code.decode_ms_corrected_fixed_batch(llrs[:b], *triple, maxiters=cap), ref)
                res = code.decode_ms_corrected_fixed_batch(d[:b], *triple, maxiters=cap)
                torch.cuda.synchronize()
                same(f"{code.name} {triple} cap {cap} batch {b} device", res, ref)
    assert iterated and changed                               # (frames that iterate, and a correction that changes something)


@pytest.mark.parametrize("code", TM, ids=lambda c: c.name)
def test_the_identity_triple_equals_the_plain_decoder(code):
    """(1, 0, 0) through the corrected kernel against decode_ms_batch on the same int8 frames: bit for bit, whatever kernel the plain
    entry takes at these batch sizes."""
    import torch
    g = G[code]
    llrs = frames_of(code, np.random.default_rng(4240 + int(code)), 3 * g + 1)
    d = torch.from_numpy(llrs).cuda()
    for cap in CAPS:
        for b in (1, g + 1, 3 * g + 1):
            plain = code.decode_ms_batch(d[:b], cap)
            got = code.decode_ms_corrected_fixed_batch(d[:b], 1, 0, 0, maxiters=cap)
            torch.cuda.synchronize()
            for x, y, what in zip(got, plain, ("output", "iters", "success")):
                assert torch.equal(x, y), (code.name, cap, b, what)
            same(f"{code.name} identity cap {cap} batch {b} host", code.decode_ms_corrected_fixed_batch(llrs[:b], 1, 0, 0, maxiters=cap),
                 tuple(x.cpu().numpy() for x in plain))


def raw_buffers(code, batch, device):
    import torch
    if device:
        t = (torch.zeros((batch, code.n()), dtype=torch.int8, device="cuda"), torch.zeros((batch, code.output_len()), dtype=torch.uint8, device="cuda"),
             torch.zeros(batch, dtype=torch.int32, device="cuda"), torch.zeros(batch, dtype=torch.uint8, device="cuda"))
        return t, [x.data_ptr() for x in t]
    t = (np.zeros((batch, code.n()), np.int8), np.zeros((batch, code.output_len()), np.uint8), np.zeros(batch, np.uint32), np.zeros(batch, np.uint8))
    return t, [x.ctypes.data for x in t]


def test_refusals_come_with_their_text_and_before_any_device_work():
    """Every refusal is decided on the arguments: the result buffers still hold what they held."""
    import torch
    fn = getattr(la.lib, SYM)
    code = LDPCCode.TM2048
    keep, p = raw_buffers(code, 2, False)
    keep[1][:] = 0xEE
    # a TC code, whatever the triple (the identity included); a variant other than 0
    for tc in (LDPCCode.TC128, LDPCCode.TC512):
        k2, p2 = raw_buffers(tc, 2, False)
        for triple in ((13, 4, 0), (1, 0, 0)):
            assert fn(int(tc), *p2, 2, 10, *triple, None) == EUNSUPPORTED
            assert "corrected bit-sliced flooding decoder" in la.last_error() and "TM codes" in la.last_error(), la.last_error()
    for variant in (1, 64):
        opts = la.HipOpts(0, la.MEM_HOST, None, variant, 0, None)
        assert fn(int(code), *p, 2, 10, 13, 4, 0, ctypes.byref(opts)) == EUNSUPPORTED
        assert f"variant {variant}" in la.last_error() and "corrected bit-sliced flooding decoder" in la.last_error(), la.last_error()
    # each parameter one past its range
    for triple, text in (((1, 9, 0), "scale_shift"), ((0, 0, 0), "scale_num"), ((2, 0, 0), "scale_num"), ((17, 4, 0), "scale_num"),
                         ((257, 8, 0), "scale_num"), ((1, 0, 128), "offset")):
        assert fn(int(code), *p, 2, 10, *triple, None) == EINVAL, triple
        assert text in la.last_error() and "is not in" in la.last_error(), (triple, la.last_error())
    # a NULL buffer, each of the four; a bad code; the empty batch
    for i in range(4):
        q = list(p)
        q[i] = None
        assert fn(int(code), *q, 2, 10, 13, 4, 0, None) == EINVAL and "NULL buffer" in la.last_error()
    assert fn(9, *p, 2, 10, 13, 4, 0, None) == EINVAL and "out of range" in la.last_error()
    assert fn(int(code), None, None, None, None, 0, 10, 13, 4, 0, None) == OK
    assert fn(int(LDPCCode.TC128), None, None, None, None, 0, 10, 1, 9, 0, None) == OK      # (an empty batch never gets as far as the triple)
    assert (keep[1] == 0xEE).all() and not keep[2].any() and not keep[3].any()
    # a device llrs buffer off 4-byte alignment
    flat = torch.zeros(4 * code.n() + 16, dtype=torch.int8, device="cuda")
    dk, dp = raw_buffers(code, 2, True)
    dk[1][:] = 0xEE
    torch.cuda.synchronize()
    opts = la.HipOpts(0, la.MEM_DEVICE, None, 0, 0, None)
    for lead in (1, 2, 3):
        assert fn(int(code), flat.data_ptr() + lead, *dp[1:], 2, 10, 13, 4, 0, ctypes.byref(opts)) == EINVAL
        assert "llrs buffer must be 4-byte aligned" in la.last_error(), la.last_error()
    torch.cuda.synchronize()
    assert bool((dk[1] == 0xEE).all())
    # the Python method: any other dtype
    for bad in (np.zeros((1, code.n()), np.int16), np.zeros((1, code.n()), np.float32)):
        with pytest.raises(la.LdpcHipError):
            code.decode_ms_corrected_fixed_batch(bad, 13, 4, 0)


@pytest.mark.parametrize("code", [LDPCCode.TM1280, LDPCCode.TM2048, LDPCCode.TM8192], ids=lambda c: c.name)
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_the_entry_writes_only_the_callers_result_rows(code, device):
    """G + 1 frames (a partial last group) into guarded buffers at the least alignment the entry admits: llrs 4 bytes past a 16-byte
    boundary, output 8, iters 4, success 1."""
    import torch
    b = G[code] + 1
    dev = "cuda" if device else None
    llrs = frames_of(code, np.random.default_rng(4340 + int(code)), b)
    x, gx = gb.guarded_copy(llrs, 4, dev, name="llrs")
    out, go = gb.guarded(b, (code.output_len(),), np.uint8, 8, dev, name="output")
    it, gi = gb.guarded(b, (), np.int32, 4, dev, name="iters", prefill=-2)
    ok, gk = gb.guarded(b, (), np.uint8, 1, dev, name="success")
    inp = gb.frozen(x, "llrs")
    triple = (13, 4, 1)
    ptr = (lambda t: t.data_ptr()) if device else (lambda t: t.ctypes.data)
    opts = la.HipOpts(0, la.MEM_DEVICE if device else la.MEM_HOST, None, 0, 0, None)
    if device:
        torch.cuda.synchronize()
    st = getattr(la.lib, SYM)(int(code), ptr(x), ptr(out), ptr(it), ptr(ok), b, 25, *triple, ctypes.byref(opts))
    assert st == OK, la.last_error()
    if device:
        torch.cuda.synchronize()
    for guard in (gx, go, gi, gk, inp):
        guard.check()
    want = fr.decode(fr.structure(int(code)), llrs, 25, *triple)
    same(f"{code.name} guarded", (out, it.cpu().numpy().astype(np.uint32) if device else it.astype(np.uint32), ok), want)


@pytest.mark.parametrize("code", [LDPCCode.TM1280, LDPCCode.TM2048], ids=lambda c: c.name)
def test_cascades_equal_the_composition_of_the_separate_calls(code):
    """Both cascade entries with a stage-1 triple of (13, 4, 0), per frame and `stage` included, against flooding-then-layered composed
    from the library's separate entries; with an identity stage-1 triple, against today's cascade entries bit for bit."""
    import torch
    f1, f2 = (13, 4, 0), (13, 4, 1)
    rng = np.random.default_rng(4440 + int(code))
    y, _ = oracle.awgn_llrs(code, rng, 3 * G[code] + 9, EBN0[code] - 0.3, np.float32)
    q = code.quantise_llrs_batch(y, "i8", 8.0, 31)
    first = lambda x, cap: code.decode_ms_corrected_fixed_batch(x, *f1, maxiters=cap)                                  # noqa: E731
    second = lambda x, cap: code.decode_ms_layered_fixed_batch(x, cap, scale_num=f2[0], scale_shift=f2[1], offset=f2[2])  # noqa: E731
    mixed = False
    for cap, sweeps in ((3, 20), (25, 25)):
        want = cascade_restatement.compose(first, second, q, cap, sweeps)
        mixed |= bool(want[3].any() and not want[3].all())
        kw = dict(maxiters=cap, max_sweeps=sweeps, scale_num=f2[0], scale_shift=f2[1], offset=f2[2],
                  flooding_scale_num=f1[0], flooding_scale_shift=f1[1], flooding_offset=f1[2])
        for tag, got in (("host", code.decode_ms_cascade_fixed_batch(q, **kw)),
                         ("device", code.decode_ms_cascade_fixed_batch(torch.from_numpy(q).cuda(), **kw)),
                         ("quantised host", code.decode_ms_cascade_quantised_batch(y, "i8", 8.0, 31, **kw)),
                         ("quantised device", code.decode_ms_cascade_quantised_batch(torch.from_numpy(y).cuda(), "i8", 8.0, 31, **kw))):
            torch.cuda.synchronize()
            for g, w, what in zip(got, want, ("output", "iters", "success", "stage")):
                g = g.cpu().numpy() if hasattr(g, "cpu") else g
                assert np.array_equal(g.astype(w.dtype), w), (code.name, cap, tag, what)
        # an identity stage-1 triple IS today's entry, opts->variant honoured
        for variant in (0, 64):
            ident = dict(kw, flooding_scale_num=2, flooding_scale_shift=1, flooding_offset=0, variant=variant)
            today = {k: v for k, v in kw.items() if not k.startswith("flooding_")}
            for a, b in zip(code.decode_ms_cascade_fixed_batch(q, **ident), code.decode_ms_cascade_fixed_batch(q, variant=variant, **today)):
                assert np.array_equal(a, b), (code.name, cap, variant)
            for a, b in zip(code.decode_ms_cascade_quantised_batch(y, "i8", 8.0, 31, **ident),
                            code.decode_ms_cascade_quantised_batch(y, "i8", 8.0, 31, variant=variant, **today)):
                assert np.array_equal(a, b), (code.name, cap, variant)
    assert mixed                                                         # (at one of the caps both stages carry frames)


def test_cascade_refusals():
    code = LDPCCode.TM2048
    q = np.zeros((2, code.n()), np.int8)
    y = np.zeros((2, code.n()), np.float32)
    for call in (lambda **kw: code.decode_ms_cascade_fixed_batch(q, **kw), lambda **kw: code.decode_ms_cascade_quantised_batch(y, "i8", **kw)):
        with pytest.raises(la.LdpcHipError, match="corrected bit-sliced flooding decoder"):
            call(flooding_scale_num=13, flooding_scale_shift=4, variant=64)
        with pytest.raises(la.LdpcHipError, match="scale_shift"):
            call(flooding_scale_num=1, flooding_scale_shift=9)
        with pytest.raises(la.LdpcHipError, match="offset"):
            call(flooding_offset=128)
    tc = LDPCCode.TC256
    with pytest.raises(la.LdpcHipError, match="TM codes"):
        tc.decode_ms_cascade_fixed_batch(np.zeros((2, tc.n()), np.int8), flooding_offset=1)
    out = tc.decode_ms_cascade_fixed_batch(np.zeros((2, tc.n()), np.int8), flooding_scale_num=4, flooding_scale_shift=2)      # identity: any code
    assert len(out) == 4
    with pytest.raises(la.LdpcHipError):
        code.decode_ms_cascade_fixed_batch(np.zeros((2, code.n()), np.int16), flooding_offset=1)
    with pytest.raises(la.LdpcHipError):
        code.decode_ms_cascade_quantised_batch(y, "i16", flooding_offset=1)


def test_the_1_7_db_row_of_the_frames_table():
    """TM2048 at 1.7 dB, the 600 frames of tests/test_flooding_fixed_corrected_host.py, cap 25: the kernels fail what the statement
    fails (168 plain, 112 at (13, 4, 0), 82 at (1, 0, 1))."""
    code = LDPCCode.TM2048
    llrs, _ = oracle.awgn_llrs(code, np.random.default_rng(4140 + 17), 600, 1.7, np.int8)
    failed = [int((code.decode_ms_corrected_fixed_batch(llrs, *t, maxiters=25)[2] == 0).sum()) for t in ((1, 0, 0), (13, 4, 0), (1, 0, 1))]
    print(f"TM2048 1.7 dB: failed of 600 at plain / (13,4,0) / (1,0,1): {failed}")
    assert failed == [168, 112, 82]
    assert int((code.decode_ms_batch(llrs, 25)[2] == 0).sum()) == 168


def test_ber_harness_runs_with_a_fixed_flooding_scale():
    from labrador_ldpc_amd import perftest
    common = ["--code", "TM1280", "--snrs", "4.0", "--noise", "ebn0", "--maxiters", "20", "--batch", "2048", "--max-bits", "1e5", "--llr", "i8"]
    assert perftest.main(common + ["--schedule", "flooding", "--fixed-flooding-scale", "13/16"]) == 0
    assert perftest.main(common + ["--schedule", "cascade", "--fixed-flooding-offset", "1", "--fixed-scale", "13/16"]) == 0
    assert perftest.main(common + ["--schedule", "cascade", "--from-f32", "--fixed-flooding-scale", "13/16", "--fixed-flooding-offset", "1"]) == 0
