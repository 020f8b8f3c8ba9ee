"""What the batched entry points refuse once a device is selected (tests/test_capi_refusals_host.py has what comes before), and an
empty part of a multi-part call.  TC128, batch 4, device tensors; nothing malformed reaches a kernel."""
import ctypes

import numpy as np
import pytest

import oracle
import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode, HipOpts, MEM_DEVICE

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

EINVAL, BATCH = -1, 4
CODE = LDPCCode.TC128


def u8(n, dev):
    return torch.zeros(n, dtype=torch.uint8, device=dev)


def test_encode_batch_wants_both_device_buffers_4_byte_aligned():
    dev = torch.device("cuda", 0)
    data, cws = u8(BATCH * CODE.k() // 8 + 8, dev), u8(BATCH * CODE.n() // 8 + 8, dev)
    opts = HipOpts(0, MEM_DEVICE, None, 0)
    for d_off, c_off in ((1, 0), (0, 2), (3, 1)):
        st = la.lib.labrador_ldpc_encode_batch(int(CODE), data.data_ptr() + d_off, cws.data_ptr() + c_off, BATCH, ctypes.byref(opts))
        assert st == EINVAL and "device buffers must be 4-byte aligned" in la.last_error(), (d_off, c_off, la.last_error())


def test_bf_and_encode_refuse_an_unknown_memory_kind():
    dev = torch.device("cuda", 0)
    rx, out = u8(BATCH * CODE.n() // 8, dev), u8(BATCH * CODE.output_len(), dev)
    it, ok = torch.zeros(BATCH, dtype=torch.int32, device=dev), u8(BATCH, dev)
    for device in (0, -1):
        opts = HipOpts(device, 2, None, 0)
        st = la.lib.labrador_ldpc_decode_bf_batch(int(CODE), rx.data_ptr(), out.data_ptr(), it.data_ptr(), ok.data_ptr(), BATCH, 10,
                                                  ctypes.byref(opts))
        assert st == EINVAL and "bad opts->memory" in la.last_error()
        st = la.lib.labrador_ldpc_encode_batch(int(CODE), rx.data_ptr(), out.data_ptr(), BATCH, ctypes.byref(opts))
        assert st == EINVAL and "bad opts->memory" in la.last_error()


def test_ms_batch_checks_device_alignment_before_the_launcher_sees_the_variant():
    dev = torch.device("cuda", 0)
    llrs = torch.zeros((BATCH, CODE.n()), dtype=torch.float32, device=dev)
    out = u8(BATCH * CODE.output_len() + 8, dev)
    it, ok = torch.zeros(BATCH, dtype=torch.int32, device=dev), u8(BATCH, dev)
    opts = HipOpts(0, MEM_DEVICE, None, 7)
    st = la.lib.labrador_ldpc_decode_ms_batch_f32(int(CODE), llrs.data_ptr(), out.data_ptr() + 4, it.data_ptr(), ok.data_ptr(), BATCH, 10,
                                                  ctypes.byref(opts))
    assert st == EINVAL and "device output buffer must be 8-byte aligned" in la.last_error()
    st = la.lib.labrador_ldpc_decode_ms_batch_f32(int(CODE), llrs.data_ptr(), out.data_ptr(), it.data_ptr(), ok.data_ptr(), BATCH, 10,
                                                  ctypes.byref(opts))
    assert st == -4 and "variant 7" in la.last_error()       # ... and with the buffer aligned it is the variant's turn


def test_multi_call_skips_a_part_without_frames_and_null_buffers():
    dev = torch.device("cuda", 0)
    llrs, _ = oracle.awgn_llrs(CODE, np.random.default_rng(11), BATCH, 3.0, np.float32)
    d = torch.from_numpy(llrs).to(dev)
    want = [t.cpu().numpy() for t in CODE.decode_ms_batch(d, 20)]
    torch.cuda.synchronize(dev)
    for empty_first in (True, False):
        out = torch.full((BATCH, CODE.output_len()), 0xEE, dtype=torch.uint8, device=dev)
        it, ok = torch.full((BATCH,), -1, dtype=torch.int32, device=dev), torch.full((BATCH,), 0xEE, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        pair = lambda t, full: (t * 2)(*((None if t is ctypes.c_void_p else 0, full) if empty_first else (full, None if t is ctypes.c_void_p else 0)))
        ptrs = [pair(ctypes.c_void_p, t.data_ptr()) for t in (d, out, it, ok)]
        st = la.lib.labrador_ldpc_decode_ms_batch_f32_multi(int(CODE), 2, (ctypes.c_int * 2)(0, 0), *ptrs, pair(ctypes.c_size_t, BATCH), 20, 0)
        assert st == 0, la.last_error()
        got = [out.cpu().numpy(), it.cpu().numpy(), ok.cpu().numpy()]         # (the call returns with the results in place)
        assert all((g == w).all() for g, w in zip(got, want))
