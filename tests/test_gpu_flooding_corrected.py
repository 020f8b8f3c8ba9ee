"""Normalized / offset min-sum on the flooding schedule on the GPU (labrador_ldpc_decode_ms_corrected_{,soft_}batch_f32 and
labrador_ldpc_decode_ms_cascade_corrected_batch_f32; the `scale` / `offset` keywords of LDPCCode.decode_ms_batch and
decode_ms_soft_batch, `flooding_scale` / `flooding_offset` of decode_ms_cascade_batch) against the CPU restatement
(tests/flooding_corrected_restatement.py), bit for bit: output, iters and success exactly, app as values with NaN at the same
positions, the hard call equal to the soft call -- every code, the parameter set P below, AWGN frames, corner values, the clamp-free
loop's limit frames, both memory modes, a caller's stream, a device set, odd batch sizes, more codeword groups than one round of the
persistent grid.  With (1, 0) the corrected symbols equal the plain flooding ones bit for bit, and at (0.8125, 0) and (1, 0.1) the
kernels fail less often and take fewer passes than plain flooding min-sum."""
import ctypes

import numpy as np
import pytest

import cascade_restatement as cr
import edge_frames
import flooding_corrected_restatement as fcr
import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode
from layered_helpers import same_app
import oracle

pytestmark = pytest.mark.gpu

ALL = list(LDPCCode)
EUNSUPPORTED = -4
FMAX = float(np.finfo(np.float32).max)
# (1, FLT_MAX): every message is zero and every iteration's marginals are the LLRs; the last two put denormals through the multiply and
# the subtract (not flushed) and magnitudes below the clamp-free loop's 2^-43 into its self-correction
P = ((1.0, 0.0), (0.8125, 0.0), (0.75, 0.0), (1.0, 0.1), (0.875, 0.05), (1.0, FMAX), (2.0 ** -126, 0.0), (1.0, 2.0 ** -149))
MAIN = ((0.8125, 0.0), (1.0, 0.1))
EBN0 = {LDPCCode.TC128: (3.0, 4.5), LDPCCode.TC256: (2.5, 4.0), LDPCCode.TC512: (2.0, 3.0)}      # the grid of tests/test_gpu_layered_corrected.py
CAPS = (0, 1, 2, 3, 25, 28, 29, 60)           # 28 / 29: either side of where the plain launcher switches self-correction forms
CLAMP_CODES = [LDPCCode.TM8192, LDPCCode.TM2048, LDPCCode.TC512, LDPCCode.TM1536]               # (tests/test_gpu_soft_edges.py)
pair_id = lambda p: f"{p[0]:g}-{p[1]:g}"      # noqa: E731
_ST = {}


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if la.device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("the corrected flooding GPU tests need a gfx950 device")
    torch.cuda.set_device(0)


def structure(code):
    if code not in _ST:
        _ST[code] = fcr.Structure(code)
    return _ST[code]


def check(tag, ref, out, iters, ok, app=None):
    r_out, r_it, r_ok, r_app = ref
    assert (np.asarray(ok) == r_ok).all(), f"{tag}: success differs in frames {np.flatnonzero(np.asarray(ok) != r_ok)[:8]}"
    assert (np.asarray(iters).astype(np.uint32) == r_it).all(), f"{tag}: iters differ in frames {np.flatnonzero(np.asarray(iters) != r_it)[:8]}"
    assert (np.asarray(out) == r_out).all(), f"{tag}: output differs in frames {np.flatnonzero((np.asarray(out) != r_out).any(axis=1))[:8]}"
    if app is not None:
        assert same_app(app, r_app), f"{tag}: app differs in frames {np.flatnonzero([not same_app(x, y) for x, y in zip(app, r_app)])[:8]}"


def both_calls(code, llrs, caps, scale, offset):
    """Soft and hard corrected calls on the same frames at every cap against the restatement (one run of it to the largest cap); the
    two calls agree on the hard results.  Returns {cap: the restatement's results}."""
    refs = fcr.decode_flooding_corrected_caps(structure(code), llrs, caps, scale, offset)
    for m in caps:
        tag = f"{code.name} ({scale:g}, {offset:g}) cap {m}"
        app, out, it, ok = code.decode_ms_soft_batch(llrs, m, scale=scale, offset=offset)
        check(tag, refs[m], out, it, ok, app)
        out_h, it_h, ok_h = code.decode_ms_batch(llrs, m, scale=scale, offset=offset)
        assert (out_h == out).all() and (it_h == it).all() and (ok_h == ok).all(), f"{tag}: soft and hard calls differ"
    return refs


def corner_frames(code, rng, frames=6):
    llrs, _ = oracle.awgn_llrs(code, rng, frames, 3.0, np.float32)
    n = code.n()
    fi = np.finfo(np.float32)
    specials = np.array([np.inf, -np.inf, 0.0, -0.0, fi.tiny / 4, -fi.tiny / 4, fi.max, -fi.max, np.nan], dtype=np.float32)
    neg_nan = np.array([np.nan], dtype=np.float32)
    neg_nan.view(np.uint32)[0] |= 1 << 31
    specials = np.concatenate([specials, neg_nan])
    for f in range(1, frames):
        pos = rng.choice(n, size=1 + f * 3, replace=False)
        llrs[f, pos] = rng.choice(specials, size=len(pos))
    llrs[frames - 1, :] = np.nan
    return llrs


@pytest.mark.parametrize("code", ALL, ids=lambda c: c.name)
@pytest.mark.parametrize("pair", MAIN, ids=pair_id)
def test_awgn_frames_and_iteration_caps(code, pair):
    """(0.8125, 0) and (1, 0.1) over the grid of tests/test_gpu_layered_corrected.py, 32 frames per Eb/N0 point (16 for n >= 5120),
    caps 0 / 1 / 2 / 3 / 25 and 28 / 29 / 60."""
    rng = np.random.default_rng(500 + int(code))
    F = 16 if code.n() >= 5120 else 32
    for eb in EBN0.get(code, (1.7, 2.0, 2.5)):
        llrs, _ = oracle.awgn_llrs(code, rng, F, eb, np.float32)
        both_calls(code, llrs, CAPS, *pair)


@pytest.mark.parametrize("code", [LDPCCode.TC128, LDPCCode.TM1280, LDPCCode.TM2048, LDPCCode.TM8192], ids=lambda c: c.name)
def test_every_parameter_pair(code):
    """All of P at caps 3 and 25 on a one-wave kernel, the register-lean one, the plain multi-wave one with its clamp-free loop and the
    pair kernel."""
    rng = np.random.default_rng(900 + int(code))
    llrs, _ = oracle.awgn_llrs(code, rng, 8 if code.n() >= 5120 else 24, EBN0.get(code, (1.7, 2.0))[-1], np.float32)
    for scale, offset in P:
        refs = both_calls(code, llrs, (3, 25), scale, offset)
        if (scale, offset) == (1.0, FMAX):
            for ref in refs.values():
                assert (ref[3][:, : code.n()] == llrs).all() and (ref[3][:, code.n():] == 0).all()


@pytest.mark.parametrize("code", ALL, ids=lambda c: c.name)
def test_unit_scale_and_zero_offset_equal_the_plain_flooding_kernels(code):
    """(1, 0) through the corrected symbols (the Python keywords at their defaults call the plain ones) against the plain flooding
    symbols, into prefilled buffers: output, iters, success and app bit for bit."""
    rng = np.random.default_rng(300 + int(code))
    F = 8 if code.n() >= 5120 else 24
    llrs = np.concatenate([oracle.awgn_llrs(code, rng, F, eb, np.float32)[0] for eb in EBN0.get(code, (1.7, 2.5))]
                          + [corner_frames(code, rng), edge_frames.whole_frame_rows(code, np.float32, rng)])
    B = len(llrs)
    np_len = code.n() + code.punctured_bits()
    for m in (0, 1, 3, 25):
        plain = code.decode_ms_soft_batch(llrs, m)
        app = np.full((B, np_len), -7.0e30, np.float32)
        out = np.full((B, code.output_len()), 0xEE, np.uint8)
        it = np.full(B, 77, np.uint32)
        ok = np.full(B, 7, np.uint8)
        st = la.lib.labrador_ldpc_decode_ms_corrected_soft_batch_f32(
            int(code), llrs.ctypes.data, app.ctypes.data, out.ctypes.data, it.ctypes.data, ok.ctypes.data, B, m, 1.0, 0.0, None)
        assert st == 0, la.last_error()
        assert (app.view(np.uint32) == plain[0].view(np.uint32)).all(), f"{code.name} cap {m}: app differs from the plain entry's"
        assert (out == plain[1]).all() and (it == plain[2]).all() and (ok == plain[3]).all()
        out_h = np.full((B, code.output_len()), 0xEE, np.uint8)
        it_h = np.full(B, 77, np.uint32)
        ok_h = np.full(B, 7, np.uint8)
        st = la.lib.labrador_ldpc_decode_ms_corrected_batch_f32(
            int(code), llrs.ctypes.data, out_h.ctypes.data, it_h.ctypes.data, ok_h.ctypes.data, B, m, 1.0, 0.0, None)
        assert st == 0, la.last_error()
        assert (out_h == plain[1]).all() and (it_h == plain[2]).all() and (ok_h == plain[3]).all()


@pytest.mark.parametrize("code", ALL, ids=lambda c: c.name)
@pytest.mark.parametrize("pair", MAIN, ids=pair_id)
def test_corner_values_and_whole_frame_extremes(code, pair):
    """+-inf, +-0.0, denormals, +-FLT_MAX and NaN LLRs (both signs of NaN, a frame of NaNs only), and the whole-frame edge rows (all
    +-0.0, denormal frames, sums that overflow, +-inf runs, +-FLT_MAX frames)."""
    rng = np.random.default_rng(77 + int(code))
    llrs = np.concatenate([corner_frames(code, rng), edge_frames.whole_frame_rows(code, np.float32, rng)])
    refs = both_calls(code, llrs, (0, 3, 25), *pair)
    for m in (3, 25):
        assert (np.isnan(refs[m][3][:, : code.n()]) == np.isnan(llrs)).all()


def limit_exponents(maxiters):
    """log2 of the clamp-free loop's magnitude limit and of the plain launcher's clamp form's (nocap_limit_for, decode_ms_launch.hpp)."""
    return int(np.floor(126.0 - 2.8074 * maxiters)), int(np.floor(82.5 - 2.8074 * maxiters))


@pytest.mark.parametrize("code", CLAMP_CODES, ids=lambda c: c.name)
def test_clamp_free_loop_at_its_magnitude_limit_and_with_extreme_ratios(code):
    """The frames of tests/test_gpu_soft_edges.py B1 at caps 25 / 28 / 29: every |LLR| at either limit formula's bound of each cap (and
    one binade above, 2^64, 1.0), random signs, plain and with every third LLR scaled by 2^-20 -- the range vote passes some and
    refuses others; and LLRs at the top of the clamp form's range mixed with 2^-20 and exact zeros, signs disagreeing, and doubled.
    Every frame is decoded at every one of the three caps."""
    rng = np.random.default_rng(64 + int(code))
    n = code.n()
    per = 1 if n >= 5120 else 2
    rows = []
    for maxiters in (25, 28, 29):
        e, e2 = limit_exponents(maxiters)
        for mag in (2.0 ** max(e, -120), 2.0 ** min(max(e, -120) + 1, 127), 2.0 ** 64, 1.0, 2.0 ** max(e2, -19), 2.0 ** (max(e2, -19) + 1)):
            x = (np.where(rng.random((per, n)) < 0.5, 1.0, -1.0) * mag).astype(np.float32)
            rows.append(x)
            y = x.copy()
            y[:, ::3] *= np.float32(2.0 ** -20)
            rows.append(y)
        top = 2.0 ** max(e2, 3)
        for f in range(2 * per):
            mags = np.where(rng.random(n) < 0.5, top, 2.0 ** -20) * (1.0 + rng.random(n) * (f % 2))
            x = np.where(rng.random(n) < 0.5, 1.0, -1.0) * mags
            x[rng.random(n) < 0.05] = 0.0
            rows.append(x[None, :].astype(np.float32))
            rows.append((x[None, :] * 2.0).astype(np.float32))
    llrs = np.concatenate(rows)
    both_calls(code, llrs, (25, 28, 29), 0.8125, 0.0)
    both_calls(code, llrs[::3], (25, 28, 29), 1.0, 0.1)


@pytest.mark.parametrize("code", [LDPCCode.TC128, LDPCCode.TC256, LDPCCode.TM1280, LDPCCode.TM6144], ids=lambda c: c.name)
def test_batch_sizes(code):
    """Batch 1 and batches that do not fill the last workgroup (the TC codes hold 64 / M codewords per workgroup)."""
    rng = np.random.default_rng(21)
    llrs, _ = oracle.awgn_llrs(code, rng, 11, 2.5, np.float32)
    for b in (1, 3, 5, 11):
        both_calls(code, llrs[:b], (25,), 0.8125, 0.0)
        both_calls(code, llrs[:b], (25,), 1.0, 0.1)


def flooding_grid_bound(code, cus):
    """(most frames one round of the persistent grid can hold, codewords per group, queue-fed?) of the corrected flooding launch
    (edge_frames.grid_bound; as tests/test_gpu_soft_edges.py has it for the plain launch at `variant` 0): the pair kernel for TM8192,
    one codeword per workgroup of M / 2 threads; else one index per thread; the launch's queue for workgroups of 512 threads and more."""
    M = code.submatrix_size()
    if code == LDPCCode.TM8192:
        wg, g = M // 2, 1
    else:
        g = 64 // M if M < 64 else 1
        wg = M * g
    return edge_frames.grid_bound(wg, g, wg >= 512, cus), g, wg >= 512


@pytest.mark.parametrize("code,pair", [(LDPCCode.TM1280, (0.8125, 0.0)), (LDPCCode.TM2048, (1.0, 0.1)), (LDPCCode.TM8192, (0.8125, 0.0))],
                         ids=["TM1280-fixed-stride", "TM2048-queue", "TM8192-pair"])
def test_persistent_workgroups_decode_many_groups(code, pair):
    """More codeword groups than the largest grid the launch can have, on a fixed-stride kernel, a queue-fed one and the pair kernel, of
    mixed kinds (converging, failing, overflowing, NaN, +-FLT_MAX): every frame's app and hard results equal its pool entry's
    restatement result, in two launches back to back, into prefilled buffers, compared on the device; the hard call on the same batch
    gives the same hard results."""
    import torch
    scale, offset = pair
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    bound, g, queued = flooding_grid_bound(code, cus)
    assert queued == (code != LDPCCode.TM1280)
    maxiters = 20
    rng = np.random.default_rng(0x9F + int(code))
    n, F = code.n(), 4 if code.n() >= 5120 else 8
    conv = oracle.awgn_llrs(code, rng, F, 3.5, np.float32)[0]
    fail = oracle.awgn_llrs(code, rng, F, 0.0, np.float32)[0]
    over = oracle.awgn_llrs(code, rng, F, 2.0, np.float32)[0] * np.float32(1e37)
    nan = oracle.awgn_llrs(code, rng, F, 3.0, np.float32)[0]
    for f in range(F):
        nan[f, rng.choice(n, size=1 + 3 * f, replace=False)] = np.nan
    big = np.where(rng.random((F, n)) < 0.5, np.finfo(np.float32).max, -np.finfo(np.float32).max).astype(np.float32)
    pool = np.concatenate([conv, fail, over, nan, big])
    kind = np.repeat(np.arange(5), F)
    dref = edge_frames.device_ref(fcr.decode_flooding_corrected(structure(code), pool, maxiters, scale, offset))
    frames = bound + bound // 16 + 3
    assert (frames + g - 1) // g > bound // g
    idx = edge_frames.batch_of(pool, kind, frames, g, rng)
    idx_d = torch.from_numpy(idx).cuda()
    d = torch.from_numpy(pool).cuda()[idx_d].contiguous()
    np_len = n + code.punctured_bits()
    tag = f"{code.name} corrected flooding ({'queue' if queued else 'fixed stride'})"

    def sentinels():
        return (torch.full((frames, np_len), -7.0e30, dtype=torch.float32, device="cuda"),
                torch.full((frames, code.output_len()), 0xEE, dtype=torch.uint8, device="cuda"),
                torch.full((frames,), -2, dtype=torch.int32, device="cuda"), torch.full((frames,), 7, dtype=torch.uint8, device="cuda"))

    bufs = [sentinels(), sentinels()]
    torch.cuda.synchronize()
    for b in bufs:
        code.decode_ms_soft_batch(d, maxiters, app=b[0], output=b[1], iters=b[2], success=b[3], scale=scale, offset=offset)
    h = code.decode_ms_batch(d, maxiters, scale=scale, offset=offset)
    torch.cuda.synchronize()
    for r, b in enumerate(bufs):
        edge_frames.check_on_device(f"{tag} run {r}", idx_d, b, dref)
    for x, y in zip(bufs[0][1:], h):
        assert torch.equal(x, y), f"{tag}: soft and hard calls differ"
    del bufs, h, d, dref, idx_d
    torch.cuda.empty_cache()


@pytest.mark.parametrize("code", [LDPCCode.TC128, LDPCCode.TM2048, LDPCCode.TM8192], ids=lambda c: c.name)
def test_memory_modes_streams_and_device_sets(code):
    import torch
    scale, offset = 0.875, 0.05
    kw = dict(scale=scale, offset=offset)
    rng = np.random.default_rng(3)
    llrs, _ = oracle.awgn_llrs(code, rng, 40, 2.0, np.float32)
    a = code.decode_ms_soft_batch(llrs, 25, **kw)
    check(code.name, fcr.decode_flooding_corrected(structure(code), llrs, 25, scale, offset), *a[1:], a[0])
    b = code.decode_ms_soft_batch(llrs, 25, devices=[0, 0], **kw)
    s = torch.cuda.Stream()
    d = torch.from_numpy(llrs).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        c = code.decode_ms_soft_batch(d, 25, stream=s.cuda_stream, **kw)
        h = code.decode_ms_batch(d, 25, stream=s.cuda_stream, **kw)
    s.synchronize()
    c = [t.cpu().numpy() for t in c]
    h = [t.cpu().numpy() for t in h]
    for other in (b, c):
        assert same_app(other[0], a[0])
        for x, y in zip(other[1:], a[1:]):
            assert (np.asarray(x) == np.asarray(y)).all()
    for x, y in zip(h, a[1:]):
        assert (np.asarray(x) == np.asarray(y)).all()
    hd = code.decode_ms_batch(llrs, 25, devices=[0, 0], **kw)
    for x, y in zip(hd, a[1:]):
        assert (np.asarray(x) == np.asarray(y)).all()
    # variant 0 is the only kernel; a misaligned device app buffer is refused
    np_len = code.n() + code.punctured_bits()
    out = torch.empty((40, code.output_len()), dtype=torch.uint8, device="cuda")
    it = torch.empty(40, dtype=torch.int32, device="cuda")
    ok = torch.empty(40, dtype=torch.uint8, device="cuda")
    raw = torch.empty(40 * np_len + 16, dtype=torch.float32, device="cuda")
    for variant in (1, 2, 32, 256):
        opts = la.HipOpts(0, la.MEM_DEVICE, torch.cuda.current_stream().cuda_stream, variant, 0, None)
        st = la.lib.labrador_ldpc_decode_ms_corrected_batch_f32(int(code), d.data_ptr(), out.data_ptr(), it.data_ptr(), ok.data_ptr(),
                                                                40, 25, scale, offset, ctypes.byref(opts))
        assert st == EUNSUPPORTED
        with pytest.raises(la.LdpcHipError):
            code.decode_ms_batch(d, 25, variant=variant, **kw)
        with pytest.raises(la.LdpcHipError):
            code.decode_ms_cascade_batch(d, 25, variant=variant, flooding_scale=scale, flooding_offset=offset)
    opts = la.HipOpts(0, la.MEM_DEVICE, torch.cuda.current_stream().cuda_stream, 0, 0, None)
    st = la.lib.labrador_ldpc_decode_ms_corrected_soft_batch_f32(int(code), d.data_ptr(), raw.data_ptr() + 4, out.data_ptr(),
                                                                 it.data_ptr(), ok.data_ptr(), 40, 25, scale, offset, ctypes.byref(opts))
    assert st == -1 and "16-byte aligned" in la.last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("code", [LDPCCode.TC128, LDPCCode.TM2048], ids=lambda c: c.name)
def test_cascade_with_a_corrected_first_stage(code):
    """Stage 1 at (0.8125, 0): the call equals the two separate calls composed per frame, `stage` included, from host and from device
    buffers; with the identity as stage 1's pair it equals decode_ms_cascade_batch as it was."""
    import torch
    rng = np.random.default_rng(0xCA5 + int(code))
    ebs = (2.0, 3.5) if code == LDPCCode.TC128 else (1.5, 1.9)
    llrs = np.concatenate([oracle.awgn_llrs(code, rng, 96, eb, np.float32)[0] for eb in ebs])
    for max_iters, max_sweeps, s2 in ((8, 25, (1.0, 0.0)), (25, 10, (0.75, 0.0)), (0, 5, (1.0, 0.1))):
        first = lambda rows, cap: code.decode_ms_batch(rows, cap, scale=0.8125, offset=0.0)                  # noqa: E731
        second = lambda rows, cap: code.decode_ms_layered_batch(rows, cap, scale=s2[0], offset=s2[1])        # noqa: E731
        want = cr.compose(first, second, llrs, max_iters, max_sweeps)
        got = code.decode_ms_cascade_batch(llrs, max_iters, max_sweeps, scale=s2[0], offset=s2[1], flooding_scale=0.8125)
        for x, y, what in zip(got, want, ("output", "iters", "success", "stage")):
            assert (np.asarray(x) == np.asarray(y)).all(), f"{code.name} {max_iters}/{max_sweeps}: {what} differs from the composition"
        if max_iters == 25:                                    # (both stages have frames to carry)
            assert 0 < int(np.asarray(got[3]).sum()) < len(llrs)
        dev = code.decode_ms_cascade_batch(torch.from_numpy(llrs).cuda(), max_iters, max_sweeps, scale=s2[0], offset=s2[1], flooding_scale=0.8125)
        torch.cuda.synchronize()
        for x, y in zip(dev, got):
            assert (x.cpu().numpy() == np.asarray(y)).all()
        today = code.decode_ms_cascade_batch(llrs, max_iters, max_sweeps, scale=s2[0], offset=s2[1])
        B = len(llrs)
        out, it = np.full((B, code.output_len()), 0xEE, np.uint8), np.full(B, 77, np.uint32)
        ok, stage = np.full(B, 7, np.uint8), np.full(B, 9, np.uint8)
        st = la.lib.labrador_ldpc_decode_ms_cascade_corrected_batch_f32(int(code), llrs.ctypes.data, out.ctypes.data, it.ctypes.data, ok.ctypes.data,
                                                                        stage.ctypes.data, B, max_iters, max_sweeps, 1.0, 0.0, s2[0], s2[1], None)
        assert st == 0, la.last_error()
        for x, y in zip((out, it, ok, stage), today):
            assert (x == np.asarray(y)).all()


def passes(it, ok, cap):
    return np.where(ok == 1, it.astype(np.int64) + 1, cap).mean()


def test_the_correction_beats_plain_flooding_min_sum_on_the_gpu():
    """The point of the feature, on the kernels themselves: TM2048 at 1.7 dB, cap 25, 600 frames of default_rng(1700).  Plain flooding
    fails 156 frames, (0.8125, 0) 99 and (1, 0.1) 74 -- the restatement's counts -- and each corrected mean pass count is below plain."""
    code = LDPCCode.TM2048
    llrs, _ = oracle.awgn_llrs(code, np.random.default_rng(1700), 600, 1.7, np.float32)
    _, it_p, ok_p = code.decode_ms_batch(llrs, 25)
    fail_p, pass_p = int((ok_p == 0).sum()), passes(it_p, ok_p, 25)
    got = {}
    for scale, offset in MAIN:
        _, it_c, ok_c = code.decode_ms_batch(llrs, 25, scale=scale, offset=offset)
        got[(scale, offset)] = int((ok_c == 0).sum())
        print(f"TM2048 1.7 dB ({scale}, {offset}): failures {got[(scale, offset)]} against {fail_p}, "
              f"passes {passes(it_c, ok_c, 25):.2f} against {pass_p:.2f}")
        assert passes(it_c, ok_c, 25) < pass_p
    assert (fail_p, got[MAIN[0]], got[MAIN[1]]) == (156, 99, 74)


def test_ber_harness_flooding_correction_switch():
    """perftest.ms_trials(..., flooding_scale=0.8125) counts fewer frame errors than plain flooding on the same frames, alone and as the
    cascade's first stage no more; the defaults give the plain counts."""
    from labrador_ldpc_amd import perftest
    code = LDPCCode.TM2048
    kw = dict(maxiters=25, batch=8192, max_bits=8192 * 1024 * 2, max_errors=1 << 40)
    t_p, _, e_p, _, fe_p = perftest.ms_trials(code, 1.7, "ebn0", **kw)
    t_d, _, e_d, _, fe_d = perftest.ms_trials(code, 1.7, "ebn0", flooding_scale=1.0, flooding_offset=0.0, **kw)
    t_c, _, e_c, _, fe_c = perftest.ms_trials(code, 1.7, "ebn0", flooding_scale=0.8125, **kw)
    print(f"TM2048 1.7 dB, {t_p} frames: frame errors {fe_p} plain flooding, {fe_c} with flooding_scale 0.8125")
    assert (t_p, e_p, fe_p) == (t_d, e_d, fe_d) and t_c == t_p
    assert fe_c < fe_p
    fe_k = perftest.ms_trials(code, 1.7, "ebn0", schedule="cascade", **kw)[4]
    fe_kc = perftest.ms_trials(code, 1.7, "ebn0", schedule="cascade", flooding_scale=0.8125, **kw)[4]
    print(f"  cascade: frame errors {fe_k} with plain stage 1, {fe_kc} with stage 1 at 0.8125")
    assert fe_kc <= fe_c and fe_k <= fe_p
    assert perftest.main(["--code", "TC128", "--snrs", "3.0", "--noise", "ebn0", "--maxiters", "20", "--batch", "4096",
                          "--max-bits", "1e5", "--flooding-scale", "0.8125", "--flooding-offset", "0.02"]) == 0
