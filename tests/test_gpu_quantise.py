"""The quantiser and the fused decode on the GPU (labrador_ldpc_quantise_llrs_batch_{i8,i16},
labrador_ldpc_decode_ms_quantised_batch_{i8,i16}; LDPCCode.quantise_llrs_batch and decode_ms_quantised_batch).  The
kernel equals the numpy restatement (tests/quantise_restatement.py) byte for byte, at the values where a quantiser goes wrong and at
the shapes where a flat streaming kernel does; the fused decode equals the library's own two calls made separately and the CPU
oracle on the restatement's frames, bit for bit in output, iters and success."""
import ctypes
import functools

import numpy as np
import pytest

import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode
import oracle
import quantise_restatement as qr

pytestmark = pytest.mark.gpu

EINVAL = -1
BS = 64                                                     # LABRADOR_LDPC_HIP_VARIANT_BITSLICE
NP = qr.NP_DTYPE
PARAMS = {"i8": (8.0, 31), "i16": (64.0, 2047)}
OTHER = {"i8": (0.37, 127), "i16": (1000.0, 32767)}


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if la.device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("the quantiser's GPU tests need a gfx950 device")
    torch.cuda.set_device(0)


def host(t):
    import torch
    a = t.cpu().numpy()
    return a.view(np.uint32) if t.dtype == torch.int32 else a


# ---- the kernel against the restatement -----------------------------------------------------------------------------------------------
# (code, batch): 128 LLRs, less than one workgroup's span of 4096; 640; 3840, a ragged tail across the unroll (3 full pieces of 1024
# LLRs and 768 of the fourth); 16384, four workgroups.  The kernel has no grid-stride loop, so there is no second round to provoke.
SHAPES = [(LDPCCode.TC128, 1), (LDPCCode.TC128, 5), (LDPCCode.TM1280, 3), (LDPCCode.TM8192, 2)]


def edge_frames(code, batch, scale, lim, seed, turn):
    """[batch, n] float32: random values with the edge vector's values over the first 16, the middle 16 and the last 16 LLRs of the
    buffer.  The vector has up to 48 values: a third of it stands at each place, and `turn` (0, 1, 2) rotates the thirds, so that
    over the three turns every value has stood at every place."""
    rng = np.random.default_rng(seed)
    y = (rng.normal(0, 6, batch * code.n()) / scale * 8).astype(np.float32)
    edge = qr.edge_vector(scale, lim)
    assert len(edge) <= 48
    edge = np.roll(np.resize(edge, 48), 16 * turn)
    mid = (len(y) // 2) & ~15
    y[:16], y[mid:mid + 16], y[-16:] = edge[:16], edge[16:32], edge[32:]
    return y.reshape(batch, code.n())


@pytest.mark.parametrize("suf", ("i8", "i16"))
@pytest.mark.parametrize("code,batch", SHAPES, ids=[f"{c.name}x{b}" for c, b in SHAPES])
def test_device_quantise_equals_the_restatement(code, batch, suf):
    import torch
    for scale, lim, turn in [(*p, t) for p in (PARAMS[suf], OTHER[suf]) for t in range(3)]:
        y = edge_frames(code, batch, scale, lim, 100 + batch, turn)
        want = qr.quantise(y, NP[suf], scale, lim)
        # the result inside a larger prefilled buffer: nothing is written outside it
        big = torch.full(((batch + 2) * code.n(),), 99, dtype=la._torch_dtypes()[suf], device="cuda")
        out = big[code.n():(batch + 1) * code.n()].view(batch, code.n())
        got = code.quantise_llrs_batch(torch.from_numpy(y).cuda(), suf, scale, lim, out=out)
        torch.cuda.synchronize()
        assert got is out
        g = host(got)
        bad = np.argwhere(g != want)
        assert bad.size == 0, (suf, scale, lim, [(y[tuple(i)], g[tuple(i)], want[tuple(i)]) for i in bad[:8]])
        assert bool((big[:code.n()] == 99).all()) and bool((big[(batch + 1) * code.n():] == 99).all())
        # ... and the host loop says the same
        assert (code.quantise_llrs_batch(y, suf, scale, lim) == want).all()
    assert not host(code.quantise_llrs_batch(torch.from_numpy(y).cuda(), suf, 8.0, 0)).any()
    tmax = int(np.iinfo(NP[suf]).max)
    assert (host(code.quantise_llrs_batch(torch.from_numpy(y).cuda(), suf, scale)) == qr.quantise(y, NP[suf], scale, tmax)).all()


@pytest.mark.parametrize("suf", ("i8", "i16"))
def test_misaligned_device_buffers_are_refused(suf):
    """An `llrs` or a `q` view offset by one element is EINVAL, and nothing is written."""
    import torch
    code = LDPCCode.TC128
    src = torch.ones(2 * code.n() + 4, dtype=torch.float32, device="cuda")
    dst = torch.full((2 * code.n() + 16,), 99, dtype=la._torch_dtypes()[suf], device="cuda")
    fn = getattr(la.lib, f"labrador_ldpc_quantise_llrs_batch_{suf}")
    opts = la.HipOpts(0, la.MEM_DEVICE, torch.cuda.current_stream().cuda_stream, 0, 0, None)
    esz = dst.element_size()
    assert fn(int(code), src.data_ptr() + 4, dst.data_ptr(), 2, 8.0, 31, ctypes.byref(opts)) == EINVAL
    assert la.last_error() == "device llrs buffer must be 16-byte aligned"
    assert fn(int(code), src.data_ptr(), dst.data_ptr() + esz, 2, 8.0, 31, ctypes.byref(opts)) == EINVAL
    assert la.last_error() == "device q buffer must be 16-byte aligned"
    with pytest.raises(la.LdpcHipError, match="16-byte aligned"):
        code.quantise_llrs_batch(src[1:1 + 2 * code.n()].view(2, code.n()), suf)
    with pytest.raises(la.LdpcHipError, match="16-byte aligned"):
        code.quantise_llrs_batch(src[:2 * code.n()].view(2, code.n()), suf, out=dst[1:1 + 2 * code.n()].view(2, code.n()))
    torch.cuda.synchronize()
    assert bool((dst == 99).all())
    # the fused entry: a device `llrs` one element off, a device `output` four bytes off
    fused = getattr(la.lib, f"labrador_ldpc_decode_ms_quantised_batch_{suf}")
    out = torch.full((2 * code.output_len() + 8,), 0xEE, dtype=torch.uint8, device="cuda")
    it, ok = torch.full((2,), -2, dtype=torch.int32, device="cuda"), torch.full((2,), 7, dtype=torch.uint8, device="cuda")
    assert fused(int(code), src.data_ptr() + 4, out.data_ptr(), it.data_ptr(), ok.data_ptr(), 2, 10, 8.0, 31, ctypes.byref(opts)) == EINVAL
    assert la.last_error() == "device llrs buffer must be 16-byte aligned"
    assert fused(int(code), src.data_ptr(), out.data_ptr() + 4, it.data_ptr(), ok.data_ptr(), 2, 10, 8.0, 31, ctypes.byref(opts)) == EINVAL
    assert la.last_error() == "device output buffer must be 8-byte aligned"
    torch.cuda.synchronize()
    assert bool((out == 0xEE).all()) and bool((it == -2).all()) and bool((ok == 7).all())


# ---- the fused decode against the two calls and the CPU oracle ---------------------------------------------------------------------------
# code: (seed, frames, Eb/N0, cap, frames the oracle fails at i8 8 / 31, at i16 64 / 2047)
CASES = {LDPCCode.TC128: (41, 64, 3.0, 20, 3, 1), LDPCCode.TM1280: (42, 48, 3.2, 25, 10, 8), LDPCCode.TM2048: (43, 48, 1.9, 25, 3, 3),
         LDPCCode.TM8192: (44, 12, 1.6, 25, 6, 5)}
FUSED = [(c, s) for c in CASES for s in ("i8", "i16")]


@functools.lru_cache(maxsize=None)
def frames(code):
    seed, n, snr, _, _, _ = CASES[code]
    y, _ = oracle.awgn_llrs(code, np.random.default_rng(seed), n, snr, np.float32)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def cpu_reference(code, suf):
    """decode_quantised on the CPU, once per case, read by every test that needs it"""
    ref = qr.decode_quantised(code, frames(code), NP[suf], *PARAMS[suf], CASES[code][3])
    for x in ref:
        x.setflags(write=False)
    return ref


def same(got, want, what=""):
    assert len(got) == len(want) == 3
    for name, g, w in zip(("output", "iters", "success"), got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.flatnonzero((g.astype(np.int64) != w.astype(np.int64)).reshape(len(g), -1).any(axis=1))
        assert not len(bad), f"{what}: {name} differs in frames {bad[:8].tolist()} ({len(bad)} of {len(g)})"


def fused(code, y, suf, cap, device=False, **kw):
    scale, lim = PARAMS[suf]
    if not device:
        return code.decode_ms_quantised_batch(y, suf, scale, lim, cap, **kw)
    import torch
    res = code.decode_ms_quantised_batch(torch.from_numpy(np.ascontiguousarray(y)).cuda(), suf, scale, lim, cap, **kw)
    torch.cuda.synchronize()
    return tuple(host(r) for r in res)


def two_calls(code, y, suf, cap, variant=0):
    """quantise_llrs_batch, then decode_ms_batch: on the device"""
    import torch
    q = code.quantise_llrs_batch(torch.from_numpy(np.ascontiguousarray(y)).cuda(), suf, *PARAMS[suf])
    res = code.decode_ms_batch(q, cap, variant=variant)
    torch.cuda.synchronize()
    return tuple(host(r) for r in res)


@pytest.mark.parametrize("code,suf", FUSED, ids=[f"{c.name}-{s}" for c, s in FUSED])
def test_fused_decode_equals_the_two_calls_and_the_oracle(code, suf, monkeypatch):
    cap = CASES[code][3]
    y = frames(code)
    ref = cpu_reference(code, suf)
    failed = int((ref[2] == 0).sum())
    print(f"{code.name} {suf}: the oracle fails {failed} of {len(y)} frames")
    assert failed == CASES[code][4 if suf == "i8" else 5] and 0 < failed < len(y)
    variants = (0, BS) if suf == "i8" and code >= LDPCCode.TM1280 else (0,)
    for variant in variants:
        separate = two_calls(code, y, suf, cap, variant)
        same(separate, ref, f"the two calls against the oracle, variant {variant}")
        same(fused(code, y, suf, cap, device=True, variant=variant), separate, f"device buffers, variant {variant}")
        same(fused(code, y, suf, cap, variant=variant), separate, f"host buffers, variant {variant}")
    # several chunks per slice with a ragged last one
    monkeypatch.setenv("LABRADOR_LDPC_HIP_QUANT_CHUNK", "7")
    assert len(y) % 7 and len(y) > 7
    same(fused(code, y, suf, cap), ref, "host buffers, chunks of 7")
    same(fused(code, y, suf, cap, device=True), ref, "device buffers, chunks of 7")
    monkeypatch.delenv("LABRADOR_LDPC_HIP_QUANT_CHUNK")
    # maxiters = 0 is what the composed calls make of it
    same(fused(code, y, suf, 0, device=True), two_calls(code, y, suf, 0), "maxiters = 0")
    same(fused(code, y, suf, 0), two_calls(code, y, suf, 0), "maxiters = 0, host")


@pytest.mark.parametrize("suf", ("i8", "i16"))
def test_a_frame_of_nans_decodes_as_the_all_zero_frame(suf):
    """NaN is an erasure: frames of NaN among ordinary ones give what frames of 0.0 give in their place, through the quantiser and
    through the fused decode, and that is the integer decoder's result on an all-zero frame."""
    code = LDPCCode.TM1280
    y = frames(code)[:8].copy()
    z = y.copy()
    y[[1, 6]] = np.nan
    z[[1, 6]] = 0.0
    import torch
    q = host(code.quantise_llrs_batch(torch.from_numpy(y).cuda(), suf, *PARAMS[suf]))
    assert not q[[1, 6]].any() and (q == qr.quantise(z, NP[suf], *PARAMS[suf])).all()
    zero = code.decode_ms_batch(np.zeros((1, code.n()), NP[suf]), 25)
    for device in (False, True):
        got, want = fused(code, y, suf, 25, device=device), fused(code, z, suf, 25, device=device)
        same(got, want, "NaN frames against zero frames")
        for f in (1, 6):
            same(tuple(g[f:f + 1] for g in got), zero, "a NaN frame against decode_ms_batch on zeros")


def test_two_streams_share_the_workspace():
    """Two fused calls by one thread on two streams, different inputs and batch sizes, the second larger so that the workspace grows
    while the first may still be using it; neither stream is synchronised in between."""
    import torch
    code, suf, cap = LDPCCode.TM2048, "i8", 25
    ref = cpu_reference(code, suf)
    y = frames(code)
    idx = [np.arange(5, 25), np.r_[np.arange(48), np.arange(47, -1, -1), np.arange(0, 48, 2)]]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    d = [torch.from_numpy(y[i]).cuda() for i in idx]
    torch.cuda.synchronize()
    got = []
    for x, s in zip(d, streams):
        with torch.cuda.stream(s):
            got.append(code.decode_ms_quantised_batch(x, suf, *PARAMS[suf], cap, stream=s.cuda_stream))
    for s in streams:
        s.synchronize()
    for g, i in zip(got, idx):
        same(tuple(host(r) for r in g), tuple(r[i] for r in ref), f"two streams, {len(i)} frames")


@pytest.mark.parametrize("suf", ("i8", "i16"))
def test_host_buffers_over_a_repeated_device(suf):
    """devices=[0, 0]: two workers of device 0, each with a workspace of its own, give the single-device result."""
    code = LDPCCode.TM1280
    same(fused(code, frames(code), suf, CASES[code][3], devices=[0, 0]), cpu_reference(code, suf), "devices=[0, 0]")


def test_a_variant_without_a_kernel_is_unsupported():
    """As decode_ms_batch: EUNSUPPORTED with the flooding entry's text, for host and device buffers."""
    code = LDPCCode.TM1280
    y = frames(code)[:4]
    for device in (False, True):
        with pytest.raises(la.LdpcHipError, match="status -4.*kernel variant 100 not built for code 3"):
            fused(code, y, "i8", 10, device=device, variant=100)
