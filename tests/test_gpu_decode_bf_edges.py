"""Batched GPU bit-flipping decoder (labrador_ldpc_decode_bf_batch: the byte-per-variable kernel of csrc/decode_bf.hip and the
bit-sliced kernel of csrc/decode_bf_bs.hip) past one pass of its grids and at the edges of its dispatch, against the CPU oracle
exactly: every frame of every batch is an entry of hard_frames.bf_pool, which oracle.decode_bf decoded, so
`(output, iters, success) == pool results[idx]` holds for the whole batch, compared on the device.  The frames of a batch are drawn
so that the successive codewords of a workgroup (wave) differ in kind: decoded at once, decoded after some iterations, not decoded.
Caller-provided result buffers start filled (0xEE / -2 / 7): a byte written outside the caller's rows shows."""
import ctypes
import functools

import numpy as np
import pytest

import hard_frames
import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TC_CODES = [c for c in LDPCCode if c.name.startswith("TC")]
TM_CODES = [c for c in LDPCCode if c.name.startswith("TM")]
ITERS = hard_frames.BF_ITERS
FILL_OUT, FILL_ITERS, FILL_OK = 0xEE, -2, 7


def group(code):
    """Codewords per wave of the bit-sliced kernel (decode_ms_bitslice.hpp, Geo<CODE>::G)."""
    return 64 // (code.submatrix_size() // 32)


def chunk(code):
    """Groups per queue draw (decode_bf_bs.hip, bf_chunk<CODE>())."""
    return 1 if code in (LDPCCode.TM1280, LDPCCode.TM5120) else 4


@functools.lru_cache(maxsize=None)
def _words(code):
    return hard_frames.on_device((hard_frames.bf_pool(code)[0],))[0]


@functools.lru_cache(maxsize=None)
def _ref(code, maxiters=ITERS):
    return hard_frames.on_device(hard_frames.bf_results(code, maxiters))


def _classes(code):
    return hard_frames.bf_pool(code)[2]


def _gather(code, idx):
    return _words(code)[torch.as_tensor(idx, device="cuda")]


def _raw(code, inp, out, it, ok, batch, maxiters, memory, stream=None):
    """labrador_ldpc_decode_bf_batch on buffers of the caller's (addresses)."""
    opts = la.HipOpts(la.DEVICE_CURRENT, memory, stream, 0)
    st = la.lib.labrador_ldpc_decode_bf_batch(int(code), inp, out, it, ok, batch, maxiters, ctypes.byref(opts))
    assert st == 0, la.last_error()


def _filled(rows, code):
    return (torch.full((rows, code.output_len()), FILL_OUT, dtype=torch.uint8, device="cuda"),
            torch.full((rows,), FILL_ITERS, dtype=torch.int32, device="cuda"),
            torch.full((rows,), FILL_OK, dtype=torch.uint8, device="cuda"))


def _fill(bufs):
    bufs[0].fill_(FILL_OUT); bufs[1].fill_(FILL_ITERS); bufs[2].fill_(FILL_OK)


@pytest.mark.parametrize("code", TM_CODES, ids=lambda c: c.name)
def test_bit_sliced_queue(code):
    """decode_bf_bs_kernel launches min(chunks, 16384) waves; a wave that has decoded its chunk of bf_chunk groups of G codewords
    draws the next from the queue word (c = gridDim.x + atomicAdd(queue, 1)).  Below F0 = 16384 x chunk x G frames no wave draws,
    so 9/8 F0 + 3 frames is the smallest kind of batch in which an eighth of the waves decode a drawn chunk after their own -- on
    the lane permutations bf_init_kernel left in LDS and with the part-filled last wave among the drawn ones.  Successive groups
    differ in class.  Two launches back to back on one stream (each allocates and frees its queue word there), one on a second
    stream, at 20 iterations and at the caps 0 (no pre-pass, no iteration) and 1."""
    g = group(code)
    f0 = 16384 * chunk(code) * g
    frames = 9 * f0 // 8 + 3
    idx = hard_frames.draw(_classes(code), frames, g, np.random.default_rng(8100 + int(code)))
    d_idx = torch.as_tensor(idx, device="cuda")
    d_in = _words(code)[d_idx]
    side = torch.cuda.Stream()
    for maxiters in (ITERS, 0, 1):
        first = code.decode_bf_batch(d_in, maxiters)
        second = code.decode_bf_batch(d_in, maxiters)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            third = code.decode_bf_batch(d_in, maxiters)
        side.synchronize()
        for tag, res in (("first", first), ("second", second), ("side stream", third)):
            hard_frames.same_on_device(f"{code.name} {frames} frames max_iters {maxiters} {tag}", d_idx, res, _ref(code, maxiters))
        del first, second, third
    del d_in, d_idx
    torch.cuda.empty_cache()


@pytest.mark.parametrize("code", TC_CODES + [LDPCCode.TM1280], ids=lambda c: c.name)
def test_byte_kernel_grid_loop(code):
    """decode_bf_kernel launches min(batch, 65536) workgroups and loops cw += gridDim.x: with 65536 + 4099 frames 4099 workgroups
    decode a second codeword on the bits[], cnt[] and maxv their first left in LDS.  The TC codes always run this kernel; TM1280
    runs it here because its `input` sits at an odd device address, which takes launch_decode_bf off the bit-sliced kernel (dword
    loads).  Classes drawn frame by frame, so codeword 65536 + w differs in kind from codeword w for most w."""
    frames = 65536 + 4099
    nb = code.n() // 8
    idx = hard_frames.draw(_classes(code), frames, 1, np.random.default_rng(8200 + int(code)))
    d_idx = torch.as_tensor(idx, device="cuda")
    if code is LDPCCode.TM1280:
        flat = torch.empty(1 + frames * nb, dtype=torch.uint8, device="cuda")
        d_in = flat[1:].view(frames, nb)
        d_in.copy_(_words(code)[d_idx])
        assert d_in.data_ptr() % 4 == 1
    else:
        d_in = _words(code)[d_idx]
    for maxiters in (ITERS, 0, 1):
        res = code.decode_bf_batch(d_in, maxiters)
        hard_frames.same_on_device(f"{code.name} {frames} frames max_iters {maxiters}", d_idx, res, _ref(code, maxiters))


@pytest.mark.parametrize("code", [LDPCCode.TM1280, LDPCCode.TM2048, LDPCCode.TM8192], ids=lambda c: c.name)
def test_threshold_between_the_kernels(code):
    """launch_decode_bf takes the bit-sliced kernel from BF_BITSLICE_MIN_GROUPS = 256 groups of G codewords up: 256 G - 1 frames run
    the byte kernel, 256 G and 256 G + 1 (one codeword in the last wave) the bit-sliced one.  Host and device buffers."""
    g = group(code)
    words, ref, cls = hard_frames.bf_pool(code)
    rng = np.random.default_rng(8300 + int(code))
    for frames in (256 * g - 1, 256 * g, 256 * g + 1):
        idx = hard_frames.draw(cls, frames, g, rng)
        res = code.decode_bf_batch(_gather(code, idx), ITERS)
        hard_frames.same_on_device(f"{code.name} {frames} frames device", idx, res, _ref(code))
        out, it, ok = code.decode_bf_batch(words[idx], ITERS)
        bad = np.flatnonzero((out != ref[0][idx]).any(axis=1) | (it.astype(np.int64) != ref[1][idx]) | (ok != ref[2][idx]))
        assert len(bad) == 0, f"{code.name} {frames} frames host: {len(bad)} frames differ, first {bad[0]}"


@pytest.mark.parametrize("code", [LDPCCode.TM2048, LDPCCode.TM8192], ids=lambda c: c.name)
def test_misaligned_device_buffers_above_the_threshold(code):
    """300 G + 3 frames would run the bit-sliced kernel, which loads and stores dwords: an `input` at base + 1 or base + 2, or an
    `output` at base + 2, sends the batch to the byte kernel instead.  The results equal the aligned call's and the pool's, and the
    two bytes in front of `output` and those behind it keep their fill."""
    g = group(code)
    frames = 300 * g + 3
    nb, ol = code.n() // 8, code.output_len()
    idx = hard_frames.draw(_classes(code), frames, g, np.random.default_rng(8400 + int(code)))
    d_in = _gather(code, idx)
    aligned = code.decode_bf_batch(d_in, ITERS)
    hard_frames.same_on_device(f"{code.name} aligned", idx, aligned, _ref(code))
    for off in (1, 2):
        flat = torch.empty(off + frames * nb, dtype=torch.uint8, device="cuda")
        shifted = flat[off:].view(frames, nb)
        shifted.copy_(d_in)
        assert shifted.data_ptr() % 4 == off
        res = code.decode_bf_batch(shifted, ITERS)
        hard_frames.same_on_device(f"{code.name} input + {off}", idx, res, _ref(code))
        assert all(torch.equal(a, b) for a, b in zip(res, aligned))
    flat = torch.full((2 + frames * ol + 30,), FILL_OUT, dtype=torch.uint8, device="cuda")
    out = flat[2: 2 + frames * ol].view(frames, ol)
    _, it, ok = _filled(frames, code)
    assert d_in.data_ptr() % 4 == 0 and out.data_ptr() % 4 == 2
    _raw(code, d_in.data_ptr(), out.data_ptr(), it.data_ptr(), ok.data_ptr(), frames, ITERS, la.MEM_DEVICE,
         torch.cuda.current_stream().cuda_stream)
    hard_frames.same_on_device(f"{code.name} output + 2", idx, (out, it, ok), _ref(code))
    assert all(torch.equal(a, b) for a, b in zip((out, it, ok), aligned))
    assert bool((flat[:2] == FILL_OUT).all()) and bool((flat[2 + frames * ol:] == FILL_OUT).all()), "guard bytes were written"


@pytest.mark.parametrize("code", [LDPCCode.TM1536, LDPCCode.TM5120], ids=lambda c: c.name)
def test_rows_of_larger_arrays(code):
    """`output`, `iters` and `success` are rows 8 .. 8 + B of arrays with 8 more rows on either side.  B = 300 G + 3 runs the
    bit-sliced kernel, whose last wave is part-filled (3 of G codewords) and which stores dwords under a validity mask; B = 5 runs
    the byte kernel, from device memory and through the host path's staging.  The rows on either side keep their fill."""
    g = group(code)
    words, ref, cls = hard_frames.bf_pool(code)
    rng = np.random.default_rng(8500 + int(code))
    for B in (300 * g + 3, 5):
        idx = hard_frames.draw(cls, B, g, rng)
        d_in = _gather(code, idx)
        bufs = _filled(B + 16, code)
        rows = tuple(b[8: 8 + B] for b in bufs)
        _raw(code, d_in.data_ptr(), *(r.data_ptr() for r in rows), B, ITERS, la.MEM_DEVICE, torch.cuda.current_stream().cuda_stream)
        hard_frames.same_on_device(f"{code.name} B={B} device rows", idx, rows, _ref(code))
        for b, fill in zip(bufs, (FILL_OUT, FILL_ITERS, FILL_OK)):
            assert bool((b[:8] == fill).all()) and bool((b[8 + B:] == fill).all()), f"{code.name} B={B}: rows outside the batch were written"
    B = 5
    idx = hard_frames.draw(cls, B, g, rng)
    h_in = np.ascontiguousarray(words[idx])
    h = (np.full((B + 16, code.output_len()), FILL_OUT, np.uint8), np.full(B + 16, FILL_ITERS, np.int32), np.full(B + 16, FILL_OK, np.uint8))
    rows = tuple(a[8: 8 + B] for a in h)
    _raw(code, h_in.ctypes.data, *(r.ctypes.data for r in rows), B, ITERS, la.MEM_HOST)
    for r, e in zip(rows, ref):
        assert (r == e[idx]).all()
    for a, fill in zip(h, (FILL_OUT, FILL_ITERS, FILL_OK)):
        assert (a[:8] == fill).all() and (a[8 + B:] == fill).all()


def test_two_streams_of_the_callers():
    """TM2048, 300 G + 3 and 500 G + 1 frames on two streams of the caller's, launched alternately three times each with no
    synchronisation in between: every launch of the bit-sliced kernel allocates, zeroes and frees its queue word on its own stream
    (hipMallocAsync), so no launch may see another's queue."""
    code = LDPCCode.TM2048
    g = group(code)
    rng = np.random.default_rng(8600)
    jobs = []
    for frames in (300 * g + 3, 500 * g + 1):
        idx = hard_frames.draw(_classes(code), frames, g, rng)
        jobs.append((idx, _gather(code, idx), torch.cuda.Stream(), []))
    torch.cuda.synchronize()                                            # the inputs are complete before the side streams start
    for _ in range(3):
        for idx, d_in, s, results in jobs:
            with torch.cuda.stream(s):
                results.append(code.decode_bf_batch(d_in, ITERS))
    for idx, d_in, s, results in jobs:
        s.synchronize()
        for r, res in enumerate(results):
            hard_frames.same_on_device(f"{code.name} {len(idx)} frames, launch {r}", idx, res, _ref(code))


def test_graph_capture_takes_the_byte_kernel():
    """TM5120, 300 G + 3 frames: outside a capture this batch runs the bit-sliced kernel, whose launcher allocates its queue word on
    the stream; inside one launch_decode_bf sees hipStreamIsCapturing and takes the byte kernel, which only enqueues.  One raw
    decode_bf_batch with outputs of the caller's is captured on the capture's side stream into a single linear graph and replayed
    twice over refilled outputs."""
    code = LDPCCode.TM5120
    g = group(code)
    frames = 300 * g + 3
    idx = hard_frames.draw(_classes(code), frames, g, np.random.default_rng(8700))
    d_in = _gather(code, idx)
    bufs = _filled(frames, code)

    def one_pass():
        _raw(code, d_in.data_ptr(), *(b.data_ptr() for b in bufs), frames, ITERS, la.MEM_DEVICE, torch.cuda.current_stream().cuda_stream)

    one_pass()                                   # warm-up outside the capture (module load): the bit-sliced kernel ...
    hard_frames.same_on_device(f"{code.name} before the capture", idx, bufs, _ref(code))
    code.decode_bf_batch(d_in[:5], ITERS)        # ... and the byte kernel
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        one_pass()
    for r in range(2):
        _fill(bufs)
        graph.replay()
        torch.cuda.synchronize()
        hard_frames.same_on_device(f"{code.name} replay {r}", idx, bufs, _ref(code))
