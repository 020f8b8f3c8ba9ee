"""Packed hard decisions through the bit-sliced i8 kernels' own loader, on the GPU (labrador_ldpc_decode_ms_bitsliced_hard_batch_i8,
labrador_ldpc_decode_ms_bitsliced_hard_corrected_batch_i8; LDPCCode.decode_ms_hard_batch), bit for bit against the
references of tests/bs_hard_frames.py and against the two-step route on the device -- hard_to_llrs_batch i8 times the magnitude and
masked, then decode_ms_batch / decode_ms_corrected_fixed_batch: the four one-wave TM codes on the 3 G + 1 frames that the CPU emulation
of the same kernel text passed (tests/test_bitslice_hard_emu.py), caps 0 / 3 / 25, partial groups, host and device buffers, with and
without the mask, one batch of 4 G 1024 + 3 frames, containment in guarded buffers at the least alignments, the refusals, a device set,
a graph-captured call per entry and perftest's --llr hard."""
import ctypes

import numpy as np
import pytest

import bs_hard_frames as bhf
import captured
import guarded_buffers as gb
import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode

pytestmark = pytest.mark.gpu

CODES = [LDPCCode[n] for n in bhf.NAMES]
CAPS = (0, 3, 25)
EINVAL, OK, EUNSUPPORTED = -1, 0, -4
PLAIN = "labrador_ldpc_decode_ms_bitsliced_hard_batch_i8"
CORRECTED = "labrador_ldpc_decode_ms_bitsliced_hard_corrected_batch_i8"
HARD = ("output", "iters", "success")
TRIPLE = (13, 4, 0)


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if la.device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("the packed-loader bit-sliced GPU tests need a gfx950 device")
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


def kw_of(triple):
    return {"scale_num": triple[0], "scale_shift": triple[1], "offset": triple[2]}


def batches_of(g):
    return sorted({b for b in (g - 1, g, g + 1, 3 * g + 1) if b >= 1})


def first(res, b):
    return tuple(a[:b] for a in res)


def expanded_on_device(code, x, m, magnitude):
    """the route the entry replaces, on the device: hard_to_llrs_batch i8 (+-1) times the magnitude, zero where the mask's bit is set"""
    import torch
    e = code.hard_to_llrs_batch(x, "i8") * magnitude
    if m is not None:
        shifts = torch.arange(7, -1, -1, device=m.device, dtype=torch.uint8)
        erased = ((m.unsqueeze(-1) >> shifts) & 1).reshape(len(m), -1).bool()
        e = torch.where(erased, torch.zeros_like(e), e)
    return e.to(torch.int8).contiguous()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("code", CODES, ids=lambda c: c.name)
def test_both_entries_equal_the_references_and_the_two_step_route(code, device):
    import torch
    name = code.name
    bhf.assert_conditions(name)
    xs, ms = bhf.frames(name)
    dx, dm = torch.from_numpy(np.array(xs)).cuda(), torch.from_numpy(np.array(ms)).cuda()
    x, m = (dx, dm) if device else (xs, ms)
    sync = torch.cuda.synchronize
    for b in batches_of(bhf.GROUP[name]):
        for cap in CAPS:
            for masked in (False, True):
                mask, dmask = (m[:b], dm[:b]) if masked else (None, None)
                for magnitude in bhf.MAGNITUDES:
                    got = code.decode_ms_hard_batch(x[:b], cap, magnitude, mask)
                    sync()
                    tag = f"{name} plain magnitude {magnitude} mask {masked} cap {cap} batch {b}"
                    same(tag + ": the oracle on the expanded frames", got, first(bhf.expected_plain(name, magnitude, masked, cap), b))
                    if device:                                               # (the route it replaces runs on the device: compared once)
                        two_step = code.decode_ms_batch(expanded_on_device(code, dx[:b], dmask, magnitude), cap)
                        sync()
                        same(tag + ": the two-step route", got, two_step)
                for triple in bhf.TRIPLES:
                    got = code.decode_ms_hard_batch(x[:b], cap, bhf.CORRECTED_MAGNITUDE, mask, **kw_of(triple))
                    sync()
                    tag = f"{name} {triple} mask {masked} cap {cap} batch {b}"
                    same(tag + ": the corrected statement on the expanded frames", got, first(bhf.expected_corrected(name, triple, masked)[cap], b))
                    if device:
                        e = expanded_on_device(code, dx[:b], dmask, bhf.CORRECTED_MAGNITUDE)
                        two_step = code.decode_ms_corrected_fixed_batch(e, *triple, maxiters=cap)
                        sync()
                        same(tag + ": the two-step route", got, two_step)
                # every spelling of the identity is the plain kernel's answer
                got = code.decode_ms_hard_batch(x[:b], cap, 16, mask, scale_num=16, scale_shift=4)
                sync()
                same(f"{name} identity mask {masked} cap {cap} batch {b}", got, first(bhf.expected_plain(name, 16, masked, cap), b))


@pytest.mark.parametrize("code", CODES, ids=lambda c: c.name)
def test_a_large_batch_with_a_partial_last_group(code):
    """4 G 1024 + 3 frames drawn from the 3 G + 1 by index: more than one wave per CU, more groups than one round of the grid's
    stride can hold on a small grid, the last group partial"""
    import torch
    name, g = code.name, bhf.GROUP[code.name]
    b = 4 * g * 1024 + 3
    xs, ms = bhf.frames(name)
    idx = np.arange(b) % len(xs)
    at = torch.from_numpy(idx).cuda()
    dx, dm = torch.from_numpy(np.array(xs)).cuda()[at].contiguous(), torch.from_numpy(np.array(ms)).cuda()[at].contiguous()
    assert dx.shape == (b, code.n() // 8) and dx.data_ptr() % 4 == 0 and dm.data_ptr() % 4 == 0
    got = code.decode_ms_hard_batch(dx, 25, 1, dm)
    cgot = code.decode_ms_hard_batch(dx, 25, 16, dm, **kw_of(TRIPLE))
    nomask = code.decode_ms_hard_batch(dx, 25, 127)
    two_step = code.decode_ms_batch(expanded_on_device(code, dx, dm, 1), 25)
    torch.cuda.synchronize()
    same(f"{name} batch {b}: the oracle", got, tuple(a[idx] for a in bhf.expected_plain(name, 1, True, 25)))
    same(f"{name} batch {b}: the two-step route", got, two_step)
    same(f"{name} batch {b}: the corrected statement", cgot, tuple(a[idx] for a in bhf.expected_corrected(name, TRIPLE, True)[25]))
    same(f"{name} batch {b}: magnitude 127 without a mask", nomask, tuple(a[idx] for a in bhf.expected_plain(name, 127, False, 25)))
    # the same batch from the host: two inputs staged in one chunk, then in chunks of 1000 frames through the three-stream pipeline
    # (the library reads the variable on every host-pointer call), with the mask and without
    hx, hm = np.ascontiguousarray(xs[idx]), np.ascontiguousarray(ms[idx])
    same(f"{name} batch {b} from the host", code.decode_ms_hard_batch(hx, 25, 1, hm), got)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("LABRADOR_LDPC_HIP_CHUNK", "1000")
        same(f"{name} batch {b} from the host in chunks", code.decode_ms_hard_batch(hx, 25, 1, hm), got)
        same(f"{name} batch {b - 1} from the host in chunks, no mask", code.decode_ms_hard_batch(hx[1:], 25, 127), tuple(a[1:] for a in nomask))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("sym", [PLAIN, CORRECTED])
@pytest.mark.parametrize("code", CODES, ids=lambda c: c.name)
def test_the_entries_write_only_the_callers_result_rows(code, sym, masked, device):
    """G + 1 frames (a partial last group) in guarded views at the least alignments the header admits: input and erasures 4 bytes past
    a 16-byte boundary, output 8 bytes past one, iters 4 past an 8-byte one, success odd."""
    import torch
    name = code.name
    b = bhf.GROUP[name] + 1
    dev = "cuda" if device else None
    xs, ms = bhf.frames(name)
    x, gx = gb.guarded_copy(np.array(xs[:b]), 4, dev, name="input")
    m, gm = gb.guarded_copy(np.array(ms[:b]), 4, dev, name="erasures")
    out, go = gb.guarded(b, (code.output_len(),), np.uint8, 8, dev, name="output")
    it, gi = gb.guarded(b, (), np.int32, 4, dev, name="iters", prefill=-2)
    ok, gk = gb.guarded(b, (), np.uint8, 1, dev, name="success")
    frozen = [gb.frozen(x, "input"), gb.frozen(m, "erasures")]
    ptr = (lambda t: t.data_ptr()) if device else (lambda t: t.ctypes.data)
    assert ptr(x) % 16 == 4 and ptr(m) % 16 == 4 and ptr(out) % 16 == 8 and ptr(it) % 8 == 4 and ptr(ok) % 2 == 1
    opts = la.HipOpts(0, la.MEM_DEVICE if device else la.MEM_HOST, None, 0, 0, None)
    if device:
        torch.cuda.synchronize()
    tail = (25, 16) + (TRIPLE if sym == CORRECTED else ())
    st = getattr(la.lib, sym)(int(code), ptr(x), ptr(m) if masked else None, ptr(out), ptr(it), ptr(ok), b, *tail, ctypes.byref(opts))
    assert st == OK, la.last_error()
    if device:
        torch.cuda.synchronize()
    for guard in [gx, gm, go, gi, gk] + frozen:
        guard.check()
    want = bhf.expected_corrected(name, TRIPLE, masked)[25] if sym == CORRECTED else bhf.expected_plain(name, 16, masked, 25)
    same(f"{name} {sym} guarded", (out, host(it).astype(np.uint32), ok), first(want, b))


def raw_buffers(code, batch, device):
    """input, erasures, output, iters, success with sentinel-filled results, and their addresses"""
    import torch
    if device:
        t = (torch.zeros((batch, code.n() // 8 + 4), dtype=torch.uint8, device="cuda"), torch.zeros((batch, code.n() // 8 + 4), dtype=torch.uint8, device="cuda"),
             torch.full((batch, code.output_len()), 0xEE, dtype=torch.uint8, device="cuda"),
             torch.full((batch,), -2, dtype=torch.int32, device="cuda"), torch.full((batch,), 0xEE, dtype=torch.uint8, device="cuda"))
        torch.cuda.synchronize()
        return t, [a.data_ptr() for a in t]
    t = (np.zeros((batch, code.n() // 8), np.uint8), np.zeros((batch, code.n() // 8), np.uint8), np.full((batch, code.output_len()), 0xEE, np.uint8),
         np.full(batch, -2, np.int32), np.full(batch, 0xEE, np.uint8))
    return t, [a.ctypes.data for a in t]


def untouched(t):
    return bool((host(t[2]) == 0xEE).all() and (host(t[3]) == -2).all() and (host(t[4]) == 0xEE).all())


def call(sym, code, p, opts=None, magnitude=16):
    o = ctypes.byref(opts) if opts is not None else None
    return getattr(la.lib, sym)(int(code), *p, 2, 10, magnitude, *(TRIPLE if sym == CORRECTED else ()), o)


@pytest.mark.parametrize("sym", [PLAIN, CORRECTED])
def test_refusals_come_with_their_text_and_before_any_device_work(sym):
    import torch
    text = "packed-hard-decision bit-sliced flooding decoder"
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
    assert call(sym, code, p, magnitude=0) == EINVAL and "magnitude 0" in la.last_error()
    assert call(sym, code, p, magnitude=128) == EINVAL and "magnitude 128" in la.last_error()
    assert untouched(keep)
    # device rows off their alignment: input and erasures at 1 and 2 mod 4, output at 4 mod 8
    dk, dp = raw_buffers(code, 3, True)
    opts = la.HipOpts(0, la.MEM_DEVICE, None, 0, 0, None)
    assert dp[0] % 4 == 0 and dp[1] % 4 == 0
    for off in (1, 2):
        assert call(sym, code, [dp[0] + off] + dp[1:], opts) == EINVAL
        assert "input buffer must be 4-byte aligned" in la.last_error(), la.last_error()
        assert call(sym, code, [dp[0], dp[1] + off] + dp[2:], opts) == EINVAL
        assert "erasures buffer must be 4-byte aligned" in la.last_error(), la.last_error()
    assert call(sym, code, [dp[0], dp[1], dp[2] + 4] + dp[3:], opts) == EINVAL
    assert "output buffer must be 8-byte aligned" in la.last_error(), la.last_error()
    torch.cuda.synchronize()
    assert untouched(dk)


def test_a_device_set_shards_a_host_batch():
    code = LDPCCode.TM2048
    x, m = bhf.frames(code.name)
    want = first(bhf.expected_corrected(code.name, TRIPLE, True)[25], len(x))
    same("devices=[0, 0] corrected", code.decode_ms_hard_batch(x, 25, 16, m, devices=[0, 0], **kw_of(TRIPLE)), want)
    same("devices=[0, 0] plain", code.decode_ms_hard_batch(x, 25, 5, m, devices=[0, 0]), bhf.expected_plain(code.name, 5, True, 25))
    same("devices=[0, 0] no mask", code.decode_ms_hard_batch(x, 25, 5, devices=[0, 0]), bhf.expected_plain(code.name, 5, False, 25))


@pytest.mark.parametrize("triple", [None, TRIPLE], ids=["plain", "corrected"])
def test_a_graph_captured_call_replays_on_other_frames(triple):
    """TM2048, G + 1 frames with their masks: eager, one capture, replays on a second and a third window of the frames, inputs unchanged"""
    import torch
    code, name = LDPCCode.TM2048, "TM2048"
    xs, ms = bhf.frames(name)
    b = bhf.GROUP[name] + 1
    starts = (0, 4, 8)
    assert starts[-1] + b == len(xs)
    ref = bhf.expected_plain(name, 16, True, 25) if triple is None else bhf.expected_corrected(name, triple, True)[25]
    refs = [dict(zip(HARD, (a[s:s + b] for a in ref))) for s in starts]
    assert len({tuple(r["success"].tolist()) for r in refs}) > 1                  # (the windows do not all decode alike)
    x, m = torch.empty((b, code.n() // 8), dtype=torch.uint8, device="cuda"), torch.empty((b, code.n() // 8), dtype=torch.uint8, device="cuda")
    out = torch.empty((b, code.output_len()), dtype=torch.uint8, device="cuda")
    it, ok = torch.empty(b, dtype=torch.int32, device="cuda"), torch.empty(b, dtype=torch.uint8, device="cuda")
    kw = {} if triple is None else kw_of(triple)
    case = captured.host_case(lambda: code.decode_ms_hard_batch(x, 25, 16, m, output=out, iters=it, success=ok, **kw), [x, m],
                              list(zip(HARD, (out, it, ok))), [[np.array(xs[s:s + b]), np.array(ms[s:s + b])] for s in starts], refs)
    captured.run(case, f"decode_ms_hard_batch {name} {triple}")


def test_perftest_on_hard_input_counts_the_errors_of_the_expanded_frames():
    """perftest --llr hard on 2 x 1024 TM2048 frames: the error counts of the same frames reduced to signs, expanded to +-16 int8 and
    decoded by decode_ms_batch"""
    import torch
    from labrador_ldpc_amd import perftest
    # (Eb/N0 3.5 dB: a hard decision is wrong with probability Q(sqrt(2 R Eb/N0)) = 0.067, where the frames' table has TM2048 mixed)
    code, batch, rounds, seed, snr, cap, magnitude = LDPCCode.TM2048, 1024, 2, 3, 3.5, 25, 16
    got = perftest.ms_trials(code, snr, "ebn0", cap, batch, max_bits=(rounds - 1) * batch * code.k(), max_errors=10 ** 9, seed=seed, llr="hard",
                             hard_magnitude=magnitude)
    sigma = perftest.sigma_for(code, snr, "ebn0")
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    errors = frame_errors = 0
    for r in range(rounds):
        data = torch.randint(0, 256, (batch, code.k() // 8), dtype=torch.uint8, device="cuda", generator=g)
        llrs = code.awgn_frames(code.encode_batch(data), batch, sigma, seed=(seed << 20) + r)
        e = torch.where(llrs < 0, -magnitude, magnitude).to(torch.int8).contiguous()
        out = code.decode_ms_batch(e, cap)[0]
        per_frame = np.unpackbits(host(out[:, :code.k() // 8] ^ data), axis=1).sum(axis=1, dtype=np.int64)
        errors += int(per_frame.sum())
        frame_errors += int((per_frame > 0).sum())
    assert got[0] == rounds * batch and got[1] == rounds * batch * code.k()
    assert (got[2], got[4]) == (errors, frame_errors) and 0 < frame_errors < rounds * batch, (got, errors, frame_errors)
    with pytest.raises(ValueError, match="hard LLRs belong to the flooding schedule"):
        perftest.ms_trials(code, snr, "ebn0", cap, batch, llr="hard", schedule="layered")
    with pytest.raises(ValueError, match="hard_magnitude belongs to hard LLRs"):
        perftest.ms_trials(code, snr, "ebn0", cap, batch, hard_magnitude=16)
