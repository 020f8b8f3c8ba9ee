"""Batched GPU encoder (labrador_ldpc_encode_batch, csrc/encode.hip) at the edges of its grids and of its dispatch, against the CPU
oracle bit for bit: every frame of every batch is an entry of hard_frames.enc_pool, whose codewords oracle.copy_encode made (tied to
the reference's known answers by tests/test_hard_frames_host.py), so `codewords == pool codewords[idx]` holds for the whole batch and
nothing is sampled.  Outputs start filled with 0xEE: a byte the kernel did not write, or wrote outside its rows, shows."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import hard_frames
import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FILL = 0xEE
K4096 = [LDPCCode.TM5120, LDPCCode.TM6144, LDPCCode.TM8192]
SMALL = (1, 2, 7, 8, 9, 15, 16, 17, 63, 249, 255, 256, 263)
# k = 4096: a batch below the resident grid gets one 8-frame group per workgroup (per_wg3 = 8), so grid.y = B / 8: 8, 9 and 16 --
# the XCD-aware workgroup map (a multiple of 8) on, off and on
SMALL_K4096 = (64, 72, 128)
ENV_1COL, ENV_PLAIN = "LABRADOR_LDPC_HIP_ENC_1COL", "LABRADOR_LDPC_HIP_ENC_PLAIN_MAP"


@functools.lru_cache(maxsize=None)
def _pool(code):
    """(data, codewords, data on the device, (codewords,) on the device) of the code's pool."""
    data, cws = hard_frames.enc_pool(code)
    return data, cws, hard_frames.on_device((data,))[0], hard_frames.on_device((cws,))


def _indices(rng, frames):
    """Pool indices for a batch: random, with every special block (zero, ones, known answer, single bits) in it where it fits."""
    idx = rng.integers(0, hard_frames.ENC_BLOCKS, frames)
    if frames >= 2 * hard_frames.ENC_BLOCKS:
        at = rng.choice(frames, hard_frames.ENC_BLOCKS, replace=False)
        idx[at] = np.arange(hard_frames.ENC_BLOCKS)
        idx[-1] = 1                                                     # the all-ones block last: the ragged end of the last group
    return idx


def _device_and_host(code, idx, tag):
    """One batch through device buffers and through host buffers, both equal to the pool's codewords."""
    data, cws, d_data, d_cws = _pool(code)
    out = torch.full((len(idx), code.n() // 8), FILL, dtype=torch.uint8, device="cuda")
    code.encode_batch(d_data[torch.as_tensor(idx, device="cuda")], codewords=out)
    hard_frames.same_on_device(f"{tag} device", idx, (out,), d_cws)
    host = np.full((len(idx), code.n() // 8), FILL, dtype=np.uint8)
    code.encode_batch(data[idx], codewords=host)
    bad = np.flatnonzero((host != cws[idx]).any(axis=1))
    assert len(bad) == 0, f"{tag} host: {len(bad)} frames differ, first {bad[0]}"


@pytest.mark.parametrize("code", list(LDPCCode), ids=lambda c: c.name)
def test_more_frames_than_any_grid_holds(code):
    """encode_kernel<KW>'s loop `for (f = cy; f < batch; f += gridDim.y)` and the frame ranges of encode_kernel_k4096_2col past their
    first trip.  launch_encode sizes grid.y to (resident workgroups x at most 4 rounds) / grid.x; a CU holds at most 8 workgroups of
    256 threads (32 waves), so grid.y <= 32 CUs / gx whatever the occupancy query answers, and a batch of that bound + 1/16 + 3
    frames gives every workgroup at least a second trip (the k = 4096 kernels: ranges of two and more 8-frame groups, the `more`
    hand-over of their double buffer, a ragged last range).  Twice back to back into fresh outputs, then through host buffers."""
    data, cws, d_data, d_cws = _pool(code)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    gx = (code.n() - code.k() + 255) // 256
    bound = 32 * cus // gx
    frames = bound + bound // 16 + 3
    idx = _indices(np.random.default_rng(7200 + int(code)), frames)
    d_in = d_data[torch.as_tensor(idx, device="cuda")]
    outs = [torch.full((frames, code.n() // 8), FILL, dtype=torch.uint8, device="cuda") for _ in range(2)]
    for out in outs:                                                    # (no synchronisation in between)
        code.encode_batch(d_in, codewords=out)
    for r, out in enumerate(outs):
        hard_frames.same_on_device(f"{code.name} {frames} frames, launch {r}", idx, (out,), d_cws)
    host = code.encode_batch(data[idx])
    bad = np.flatnonzero((host != cws[idx]).any(axis=1))
    assert len(bad) == 0, f"{code.name} host: {len(bad)} frames differ, first {bad[0]}"


def _small_batches(code, extra=()):
    rng = np.random.default_rng(7300 + int(code))
    for B in SMALL + (SMALL_K4096 if code in K4096 else ()) + tuple(extra):
        _device_and_host(code, _indices(rng, B), f"{code.name} B={B}")


@pytest.mark.parametrize("code", list(LDPCCode), ids=lambda c: c.name)
def test_small_and_ragged_batches(code):
    """Batches from one frame up: grid.y = batch below the resident grid, so the generic kernel's workgroups get one frame each and
    its XCD-aware map switches at grid.y = 8 (on for multiples of 8, rounded down to one otherwise).  The LDS-staged k = 4096 kernel
    stages 8 frames at a time and load_group zero-fills past the batch: batches 1 to 9 are one or two part-filled groups, 15 to 17
    and 63 end in one, and below the resident grid every workgroup gets one group (per_wg3 = 8), so B = 64, 72 and 128 give grid.y
    8, 9 and 16: the map on, off and on.  Host and device buffers."""
    _small_batches(code)


ROW_CODES = [LDPCCode.TC128, LDPCCode.TM1280, LDPCCode.TM2048] + K4096


def _rows(code, B):
    """(pool indices of B frames, data [B + 16, k/8] with the frames in rows 8 .. 8 + B and noise around them)."""
    data, _, _, _ = _pool(code)
    rng = np.random.default_rng(7400 + int(code) + B)
    idx = rng.integers(0, hard_frames.ENC_BLOCKS, B)
    big_in = rng.integers(0, 256, (B + 16, code.k() // 8), dtype=np.uint8)
    big_in[8: 8 + B] = data[idx]
    return idx, big_in


@pytest.mark.parametrize("B", [1, 9, 257])
@pytest.mark.parametrize("code", ROW_CODES, ids=lambda c: c.name)
def test_rows_of_a_larger_device_array(code, B):
    """`data` and `codewords` are rows 8 .. 8 + B of device arrays with 8 more rows on either side.  The systematic copy of the
    k = 4096 kernels stores 16 bytes per thread for the 8 frames of a group at once (guarded by fg + tid / 32 < f_end: B = 1, 9 and
    257 end in a group of one frame) and every parity store is a dword or two: the rows before and behind the caller's keep their
    0xEE."""
    _, _, _, d_cws = _pool(code)
    idx, big_in = _rows(code, B)
    d_in = torch.from_numpy(big_in).cuda()
    d_out = torch.full((B + 16, code.n() // 8), FILL, dtype=torch.uint8, device="cuda")
    code.encode_batch(d_in[8: 8 + B], codewords=d_out[8: 8 + B])
    hard_frames.same_on_device(f"{code.name} B={B} device rows", idx, (d_out[8: 8 + B],), d_cws)
    assert bool((d_out[:8] == FILL).all()), "rows before the batch were written"
    assert bool((d_out[8 + B:] == FILL).all()), "rows behind the batch were written"


@pytest.mark.parametrize("B", [1, 9, 257])
@pytest.mark.parametrize("code", ROW_CODES, ids=lambda c: c.name)
def test_rows_of_a_larger_host_array(code, B):
    """The same rows of host arrays: the staged copy-out of the host path (csrc/capi_staging.hpp) returns B frames to the caller's
    rows and nothing to the rows around them."""
    _, cws, _, _ = _pool(code)
    idx, big_in = _rows(code, B)
    h_out = np.full((B + 16, code.n() // 8), FILL, dtype=np.uint8)
    code.encode_batch(big_in[8: 8 + B], codewords=h_out[8: 8 + B])
    assert (h_out[8: 8 + B] == cws[idx]).all()
    assert (h_out[:8] == FILL).all() and (h_out[8 + B:] == FILL).all()


def _offset_views(code, B, off_in, off_out):
    """(data, codewords, flat output) with the device addresses of data / codewords `off_in` / `off_out` bytes past a 16-byte
    boundary; 32 guard bytes behind the codewords."""
    kb, nb = code.k() // 8, code.n() // 8
    flat_in = torch.zeros(off_in + B * kb, dtype=torch.uint8, device="cuda")
    flat_out = torch.full((off_out + B * nb + 32,), FILL, dtype=torch.uint8, device="cuda")
    assert flat_in.data_ptr() % 16 == 0 and flat_out.data_ptr() % 16 == 0
    return flat_in[off_in:].view(B, kb), flat_out[off_out: off_out + B * nb].view(B, nb), flat_out


@pytest.mark.parametrize("B", [1, 9, 257, 4091])
@pytest.mark.parametrize("code", K4096, ids=lambda c: c.name)
def test_unaligned_fallback_of_the_k4096_codes(code, B):
    """encode_kernel<128>: launch_encode takes it for the k = 4096 codes when `data` or `codewords` is 4-byte but not 16-byte
    aligned (the LDS-staged kernels load and store 16 bytes per thread).  Device `data` at base + 4, `codewords` at base + 4, and
    both; B = 4091 is past any resident grid of that kernel (grid.y <= 8 workgroups x CUs / gx, gx >= 4), so its frame loop iterates.  An offset of
    1 or 2 is refused by the entry and nothing is written."""
    data, cws, d_data, d_cws = _pool(code)
    nb = code.n() // 8
    idx = _indices(np.random.default_rng(7500 + int(code) + B), B)
    for off_in, off_out in ((4, 0), (0, 4), (4, 4)):
        d_in, d_out, flat = _offset_views(code, B, off_in, off_out)
        assert d_in.data_ptr() % 16 == off_in and d_out.data_ptr() % 16 == off_out
        d_in.copy_(d_data[torch.as_tensor(idx, device="cuda")])
        code.encode_batch(d_in, codewords=d_out)
        hard_frames.same_on_device(f"{code.name} B={B} data+{off_in} codewords+{off_out}", idx, (d_out,), d_cws)
        assert bool((flat[:off_out] == FILL).all()) and bool((flat[off_out + B * nb:] == FILL).all()), "guard bytes were written"
    if B == 9:
        for off_in, off_out in ((1, 0), (2, 0), (0, 1), (0, 2)):
            d_in, d_out, flat = _offset_views(code, B, off_in, off_out)
            with pytest.raises(la.LdpcHipError, match="device buffers must be 4-byte aligned"):
                code.encode_batch(d_in, codewords=d_out)
            torch.cuda.synchronize()
            assert bool((flat == FILL).all())


def test_two_streams_of_the_callers():
    """Two batches of different codes -- TM8192 on the LDS-staged kernel, TC256 on the generic one -- on two streams of the caller's,
    launched alternately without synchronising in between: each launch's work (kernel, generator table, occupancy query) belongs to
    its stream alone."""
    jobs = []
    for code, frames in ((LDPCCode.TM8192, 4091), (LDPCCode.TC256, 9001)):
        data, cws, d_data, d_cws = _pool(code)
        idx = _indices(np.random.default_rng(7600 + int(code)), frames)
        jobs.append((code, idx, d_data[torch.as_tensor(idx, device="cuda")], d_cws, torch.cuda.Stream(), []))
    torch.cuda.synchronize()                                            # the inputs are complete before the side streams start
    for _ in range(3):
        for code, idx, d_in, d_cws, s, outs in jobs:
            with torch.cuda.stream(s):
                outs.append(torch.full((len(idx), code.n() // 8), FILL, dtype=torch.uint8, device="cuda"))
            code.encode_batch(d_in, codewords=outs[-1], stream=s.cuda_stream)
    for code, idx, d_in, d_cws, s, outs in jobs:
        s.synchronize()
        for r, out in enumerate(outs):
            hard_frames.same_on_device(f"{code.name} stream launch {r}", idx, (out,), d_cws)


def test_one_column_kernel_and_plain_workgroup_map():
    """LABRADOR_LDPC_HIP_ENC_1COL=1 selects encode_kernel_k4096 (one parity column per thread over all of k) for the k = 4096 codes,
    LABRADOR_LDPC_HIP_ENC_PLAIN_MAP=1 the plain (blockIdx.x, blockIdx.y) workgroup map for every kernel.  Both are read once per
    process, so each runs in a fresh child process of its own, one after the other: the small and ragged batches of
    test_small_and_ragged_batches for all nine codes, and 4091 frames (past the resident grid of the k = 4096 kernels: ranges of
    several groups; TM2048: a full grid with the map) for TM2048 and the k = 4096 codes."""
    if os.environ.get(ENV_1COL) or os.environ.get(ENV_PLAIN):
        for code in LDPCCode:
            _small_batches(code, extra=(4091,) if code in K4096 + [LDPCCode.TM2048] else ())
        return
    for var in (ENV_1COL, ENV_PLAIN):
        env = dict(os.environ)
        env[var] = "1"
        r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu",
                            __file__ + "::test_one_column_kernel_and_plain_workgroup_map"],
                           env=env, capture_output=True, text=True, timeout=300,
                           cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        assert r.returncode == 0, f"{var}=1: " + r.stdout[-2000:] + r.stderr[-2000:]
