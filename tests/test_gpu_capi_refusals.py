"""What the batched entry points refuse once a device is selected (tests/test_capi_refusals_host.py has what comes before), and an
empty part of a multi-part call.  TC128, batch 4 (the alignment order: batch 2, TM1536 for the bit-sliced entries), device tensors;
nothing malformed reaches a kernel."""
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


# (symbol, code, LLR element bytes, marginal element bytes, has `stage`, tail, the alignment of device llrs that the entry asks for)
ALIGNMENT_ORDER = [
    ("labrador_ldpc_decode_ms_soft_batch_f32", LDPCCode.TC128, 4, 4, False, (10,), 0),
    ("labrador_ldpc_decode_ms_soft_batch_f16", LDPCCode.TC128, 2, 4, False, (10,), 16),
    ("labrador_ldpc_decode_ms_bitsliced_soft_batch_i8", LDPCCode.TM1536, 1, 1, False, (10,), 4),
    ("labrador_ldpc_decode_ms_cascade_soft_batch_f32", LDPCCode.TC128, 4, 4, True, (10, 10, 1.0, 0.0, 1.0, 0.0), 0),
    ("labrador_ldpc_decode_ms_cascade_bitsliced_soft_batch_i8", LDPCCode.TM1536, 1, 4, True, (10, 10, 1, 0, 0), 4),
]


@pytest.mark.parametrize("sym,code,llr_bytes,app_bytes,has_stage,tail,llrs_align", ALIGNMENT_ORDER, ids=[a[0][24:] for a in ALIGNMENT_ORDER])
def test_device_alignment_is_reported_output_first_then_app_then_llrs(sym, code, llr_bytes, app_bytes, has_stage, tail, llrs_align):
    """With every device pointer misaligned the call names the output, then `app`, then `llrs`, as each is put right in turn."""
    dev, batch = torch.device("cuda", 0), 2
    llrs, app = u8(batch * code.n() * llr_bytes + 16, dev), u8(batch * 2 * code.n() * app_bytes + 16, dev)      # (n + p < 2 n)
    out, it, ok, stage = u8(batch * code.output_len() + 16, dev), torch.zeros(batch, dtype=torch.int32, device=dev), u8(batch, dev), u8(batch, dev)
    opts = HipOpts(0, MEM_DEVICE, None, 0)
    llrs_off = llrs_align // 2 if llrs_align else 0                                 # a multiple of the element size, not of the alignment

    def call(out_off, app_off, llrs_off):
        st = getattr(la.lib, sym)(int(code), llrs.data_ptr() + llrs_off, app.data_ptr() + app_off, out.data_ptr() + out_off, it.data_ptr(),
                                  ok.data_ptr(), *((stage.data_ptr(),) if has_stage else ()), batch, *tail, ctypes.byref(opts))
        return st, la.last_error()

    assert call(4, 8, llrs_off) == (EINVAL, "device output buffer must be 8-byte aligned")
    assert call(0, 8, llrs_off) == (EINVAL, "device app buffer must be 16-byte aligned")
    if llrs_align:
        assert call(0, 0, llrs_off) == (EINVAL, f"device llrs buffer must be {llrs_align}-byte aligned")


@pytest.mark.parametrize("suffix", ["i8", "i16"])
def test_layered_quantised_takes_device_llrs_of_any_f32_alignment(suffix):
    """no alignment is asked of its f32 rows beyond the element's own: the loader reads them one by one"""
    dev, batch = torch.device("cuda", 0), 2
    rows = torch.zeros(batch * CODE.n() + 4, dtype=torch.float32, device=dev)
    out, it, ok = u8(batch * CODE.output_len(), dev), torch.full((batch,), -1, dtype=torch.int32, device=dev), u8(batch, dev)
    opts = HipOpts(0, MEM_DEVICE, None, 0)
    fn = getattr(la.lib, "labrador_ldpc_decode_ms_layered_quantised_batch_" + suffix)
    for off in (4, 8, 12):
        assert rows.data_ptr() % 16 == 0
        st = fn(int(CODE), rows.data_ptr() + off, out.data_ptr(), it.data_ptr(), ok.data_ptr(), batch, 10, 8.0, 31, 3, 2, 0, ctypes.byref(opts))
        assert st == 0, la.last_error()
    torch.cuda.synchronize(dev)
    assert ok.cpu().numpy().all() and not out.cpu().numpy().any()                  # all-zero LLRs: the all-zero codeword, at once
    st = fn(int(CODE), rows.data_ptr() + 4, out.data_ptr() + 4, it.data_ptr(), ok.data_ptr(), batch, 10, 8.0, 31, 3, 2, 0, ctypes.byref(opts))
    assert st == EINVAL and "device output buffer must be 8-byte aligned" in la.last_error()


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
