"""CPU-side checks of the quantiser and the fused decode (labrador_ldpc_quantise_llrs_batch_{i8,i16},
labrador_ldpc_decode_ms_quantised_batch_{i8,i16}): the restatement (tests/quantise_restatement.py) is the rule the
tests of the layered decoders already use; the header declares and the library, the Python table and the Rust shim hold the four
entry points; the host loop equals the restatement byte for byte at the values where a quantiser goes wrong; the argument checks answer
in the documented order with their own texts before any device work; the Python methods refuse what they document; the two kernels
of llr_quantise.o have the shape they were written for.  No call here needs a GPU."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode
import layered_helpers
import quantise_restatement as qr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, OK = -1, 0
TYPES = (("i8", np.int8, "int8_t"), ("i16", np.int16, "int16_t"))
QUANTISE = [f"labrador_ldpc_quantise_llrs_batch_{t}" for t, _, _ in TYPES]
FUSED = [f"labrador_ldpc_decode_ms_quantised_batch_{t}" for t, _, _ in TYPES]
PARAMS = {"i8": ((8.0, 31), (0.37, 127)), "i16": ((64.0, 2047), (1000.0, 32767))}


# ---- the rule: passes without the feature, pins it ------------------------------------------------------------------------------------
def test_restatement_is_the_quantiser_of_the_layered_tests():
    """On finite input the restatement equals layered_helpers.quantise element for element, for every parameter set used below."""
    rng = np.random.default_rng(5)
    y = np.concatenate([rng.normal(0, 4, 20000), rng.normal(0, 400, 20000), rng.integers(-300, 300, 4000) / 16.0]).astype(np.float32)
    for suf, dtype, _ in TYPES:
        for scale, lim in PARAMS[suf]:
            assert (qr.quantise(y, dtype, scale, lim) == layered_helpers.quantise(y, dtype, scale, lim)).all(), (suf, scale, lim)
    # and what it says where that one says nothing: NaN is an erasure, infinities clamp, -0.0 is 0
    odd = np.array([np.nan, np.inf, -np.inf, -0.0, qr.FLT_MAX, -qr.FLT_MAX], np.float32)
    assert qr.quantise(odd, np.int8, 8, 31).tolist() == [0, 31, -31, 0, 31, -31]
    assert qr.quantise(odd, np.int16, 1000, 32767).tolist() == [0, 32767, -32767, 0, 32767, -32767]
    ties = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5], np.float32) / np.float32(8)
    assert qr.quantise(ties, np.int8, 8, 31).tolist() == [0, 2, 2, 0, -2, -2]


# ---- what fails without the feature ---------------------------------------------------------------------------------------------------
def test_header_declares_the_four_entry_points():
    text = open(os.path.join(ROOT, "include", "labrador_ldpc_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    tail = r"float scale,\s*int lim,\s*const struct labrador_ldpc_hip_opts \*opts\s*\)\s*;"
    for suf, _, t in TYPES:
        assert re.search(rf"int\s+labrador_ldpc_quantise_llrs_batch_{suf}\s*\(\s*enum labrador_ldpc_code code,\s*const float \*llrs,\s*"
                         rf"{t}\s*\*q,\s*size_t batch,\s*" + tail, src), suf
        assert re.search(rf"int\s+labrador_ldpc_decode_ms_quantised_batch_{suf}\s*\(\s*enum labrador_ldpc_code code,\s*const float \*llrs,\s*"
                         r"uint8_t \*output,\s*uint32_t \*iters,\s*uint8_t \*success,\s*size_t batch,\s*size_t max_iters,\s*" + tail, src), suf
    assert re.search(r"#define\s+LABRADOR_LDPC_HIP_ABI\s+3\b", text)                # additions only
    comment = text[text.index("Quantised LLRs from f32 soft values"):text.index("int labrador_ldpc_decode_ms_quantised_batch_i8")]
    assert "if p is NaN" in comment and "ties to even" in comment and "LABRADOR_LDPC_HIP_QUANT_CHUNK" in comment
    assert "captured into a graph" in comment


def test_library_python_and_rust_hold_the_four_entry_points():
    dll = ctypes.CDLL(la.LIB_PATH)
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for name in QUANTISE + FUSED:
        assert hasattr(dll, name) and name in la.SYMBOLS, name
        assert la.SYMBOLS[name][1][-3:-1] == [ctypes.c_float, ctypes.c_int]
        assert re.search(rf"pub fn {name}\s*\(code: LDPCCode, llrs: \*const f32, [^)]*scale: f32, lim: c_int, opts: \*const HipOpts\) -> c_int;",
                         rust), name
    assert len(la.SYMBOLS[QUANTISE[0]][1]) == 7 and len(la.SYMBOLS[FUSED[0]][1]) == 10
    assert la.lib.labrador_ldpc_hip_abi_version() == 3


def host_frames(code, batch, scale, lim, seed):
    """[batch, n] float32: the edge vector tiled over the first frame and placed at the end of the last, random values elsewhere"""
    rng = np.random.default_rng(seed)
    y = (rng.normal(0, 6, (batch, code.n())) / scale * 8).astype(np.float32)
    edge = qr.edge_vector(scale, lim)
    reps = code.n() // len(edge) + 1
    y[0] = np.tile(edge, reps)[:code.n()]
    y[-1, -len(edge):] = edge
    return y


@pytest.mark.parametrize("suf,dtype", [(s, d) for s, d, _ in TYPES], ids=[s for s, _, _ in TYPES])
def test_host_quantise_equals_the_restatement(suf, dtype):
    """numpy buffers take the library's host loop: byte for byte the restatement, edge vector and random frames, TC128 batch 3, at
    both parameter sets of the type; lim = 0 gives all zeros; the default lim is the type's maximum; `out` is written where it is."""
    code = LDPCCode.TC128
    for scale, lim in PARAMS[suf]:
        y = host_frames(code, 3, scale, lim, 11)
        want = qr.quantise(y, dtype, scale, lim)
        got = code.quantise_llrs_batch(y, suf, scale, lim)
        assert got.dtype == dtype and got.shape == y.shape
        bad = np.argwhere(got != want)
        assert bad.size == 0, (suf, scale, lim, [(y[tuple(i)], got[tuple(i)], want[tuple(i)]) for i in bad[:8]])
        assert set(np.unique(want[0])) >= {-lim, 0, lim}                        # the edge vector did its work
        # NULL opts is the host loop too
        raw = np.full_like(want, 99)
        fn = getattr(la.lib, f"labrador_ldpc_quantise_llrs_batch_{suf}")
        assert fn(int(code), y.ctypes.data, raw.ctypes.data, 3, scale, lim, None) == OK and (raw == want).all()
    y = host_frames(code, 3, 8.0, 5, 12)
    assert not code.quantise_llrs_batch(y, suf, 8.0, 0).any()
    tmax = int(np.iinfo(dtype).max)
    assert (code.quantise_llrs_batch(y, suf, 8.0) == qr.quantise(y, dtype, 8.0, tmax)).all()
    mine = np.full(y.shape, 77, dtype)
    assert code.quantise_llrs_batch(y, suf, 8.0, 5, out=mine) is mine and (mine == qr.quantise(y, dtype, 8.0, 5)).all()
    # a larger code, more frames: the loop runs over batch * n
    code = LDPCCode.TM1280
    y = host_frames(code, 5, 8.0, 31, 13)
    assert (code.quantise_llrs_batch(y, suf, 8.0, 31) == qr.quantise(y, dtype, 8.0, 31)).all()


def test_quantise_argument_checks_in_their_order():
    """The code; scale and lim -- before the empty batch --; the empty batch whatever the pointers; NULL buffers; opts->memory.  Exact
    status and text, all without a GPU, where a call that reached a device would say ENODEV."""
    code = LDPCCode.TC128
    for suf, dtype, _ in TYPES:
        tmax = int(np.iinfo(dtype).max)
        fn = getattr(la.lib, f"labrador_ldpc_quantise_llrs_batch_{suf}")
        y, q = np.ones((1, code.n()), np.float32), np.full((1, code.n()), 55, dtype)
        p = [y.ctypes.data, q.ctypes.data]
        for bad_code in (9, -1):
            assert fn(bad_code, *p, 1, float("nan"), -1, None) == EINVAL and la.last_error() == f"code {bad_code} out of range"   # the code comes first
        for scale, shown in ((float("nan"), "nan"), (float("inf"), "inf"), (0.0, "0"), (-2.0, "-2"), (float("-inf"), "-inf")):
            for batch, ptrs in ((0, p), (1, p), (1, [None, None])):                                      # ... before the empty batch
                assert fn(int(code), *ptrs, batch, scale, tmax + 1, None) == EINVAL                      # and scale before lim
                assert la.last_error() == f"scale {shown} is not in (0, FLT_MAX]", la.last_error()
        for lim in (-1, tmax + 1, 1 << 20):
            for batch, ptrs in ((0, p), (1, [None, None])):
                assert fn(int(code), *ptrs, batch, 8.0, lim, None) == EINVAL
                assert la.last_error() == f"lim {lim} is not in 0 .. {tmax}", la.last_error()
        for memory in (la.MEM_HOST, la.MEM_DEVICE, 7):
            opts = la.HipOpts(-1, memory, None, 0, 0, None)
            assert fn(int(code), None, None, 0, 8.0, tmax, ctypes.byref(opts)) == OK and la.last_error() == ""
            for ptrs in ([None, p[1]], [p[0], None]):
                assert fn(int(code), *ptrs, 1, 8.0, tmax, ctypes.byref(opts)) == EINVAL and la.last_error() == "NULL buffer"
        opts = la.HipOpts(-1, 7, None, 0, 0, None)
        assert fn(int(code), *p, 1, 8.0, tmax, ctypes.byref(opts)) == EINVAL and la.last_error() == "bad opts->memory"
        # misalignment of a device buffer is decided before the device is selected
        opts = la.HipOpts(-1, la.MEM_DEVICE, None, 0, 0, None)
        assert fn(int(code), 0x1000 + 4, 0x2000, 1, 8.0, tmax, ctypes.byref(opts)) == EINVAL
        assert la.last_error() == "device llrs buffer must be 16-byte aligned"
        assert fn(int(code), 0x1000, 0x2000 + 2, 1, 8.0, tmax, ctypes.byref(opts)) == EINVAL
        assert la.last_error() == "device q buffer must be 16-byte aligned"
        assert (q == 55).all()
        # host buffers ignore `device` and `devices`
        devs = (ctypes.c_int * 2)(40, 41)
        opts = la.HipOpts(99, la.MEM_HOST, None, 0, 2, devs)
        assert fn(int(code), *p, 1, 8.0, tmax, ctypes.byref(opts)) == OK and (q == 8).all()


def test_fused_argument_checks_up_to_the_device():
    """The fused entry: the same order up to where device work would begin -- the code, scale and lim, the empty batch, the buffers."""
    code = LDPCCode.TC128
    for suf, dtype, _ in TYPES:
        tmax = int(np.iinfo(dtype).max)
        fn = getattr(la.lib, f"labrador_ldpc_decode_ms_quantised_batch_{suf}")
        y = np.ones((1, code.n()), np.float32)
        out, it, ok = np.full((1, code.output_len()), 0xEE, np.uint8), np.full(1, 77, np.uint32), np.full(1, 7, np.uint8)
        p = [x.ctypes.data for x in (y, out, it, ok)]
        for bad_code in (9, -1):
            assert fn(bad_code, *p, 1, 10, 0.0, -1, None) == EINVAL and la.last_error() == f"code {bad_code} out of range"
        for scale, shown in ((float("nan"), "nan"), (float("inf"), "inf"), (0.0, "0"), (-2.0, "-2")):
            for batch, ptrs in ((0, p), (1, p), (1, [None] * 4)):
                assert fn(int(code), *ptrs, batch, 10, scale, -1, None) == EINVAL
                assert la.last_error() == f"scale {shown} is not in (0, FLT_MAX]", la.last_error()
        for lim in (-1, tmax + 1):
            for batch, ptrs in ((0, p), (1, [None] * 4)):
                assert fn(int(code), *ptrs, batch, 10, 8.0, lim, None) == EINVAL
                assert la.last_error() == f"lim {lim} is not in 0 .. {tmax}", la.last_error()
        assert fn(int(code), *([None] * 4), 0, 10, 8.0, tmax, None) == OK and la.last_error() == ""
        for i in range(4):
            ptrs = list(p)
            ptrs[i] = None
            for memory in (la.MEM_HOST, la.MEM_DEVICE):
                opts = la.HipOpts(-1, memory, None, 64, 0, None)
                assert fn(int(code), *ptrs, 1, 10, 8.0, tmax, ctypes.byref(opts)) == EINVAL and la.last_error() == "NULL buffer", i
        assert (out == 0xEE).all() and it[0] == 77 and ok[0] == 7


def test_python_methods_refuse_what_they_document():
    """Wrong shape or dtype is ValueError, an unknown `dtype` KeyError, like the neighbours; the ranges are the library's to refuse."""
    code = LDPCCode.TC128
    good = np.ones((2, code.n()), np.float32)
    for method in (code.quantise_llrs_batch, code.decode_ms_quantised_batch):
        for bad in (good[0], good[:, :-1], np.ones((2, code.n() + 1), np.float32), good.astype(np.float64), good.astype(np.int8),
                    [[1.0] * code.n()]):
            with pytest.raises(ValueError):
                method(bad)
        for bad in ("i32", "f32", "int8", np.int8, None):
            with pytest.raises(KeyError):
                method(good, bad)
        with pytest.raises(la.LdpcHipError, match="scale -1 is not in"):
            method(good, "i8", scale=-1.0)
        with pytest.raises(la.LdpcHipError, match="lim 128 is not in 0 .. 127"):
            method(good, "i8", lim=128)
        with pytest.raises(la.LdpcHipError, match="lim 32768 is not in 0 .. 32767"):
            method(good, "i16", lim=32768)
        with pytest.raises(TypeError):
            method(good, "i8", lim=3.5)
    for bad in (np.zeros((2, code.n()), np.int16), np.zeros((3, code.n()), np.int8), np.zeros((2, code.n()), np.int8)[:, ::-1], [0]):
        with pytest.raises(ValueError, match="out"):
            code.quantise_llrs_batch(good, "i8", out=bad)
    with pytest.raises(ValueError, match="output"):
        code.decode_ms_quantised_batch(good, output=np.zeros((2, code.output_len() + 1), np.uint8))
    with pytest.raises(ValueError, match="success"):
        code.decode_ms_quantised_batch(good, success=np.zeros(3, np.uint8))


class _SpyLib:
    """Stands where the package keeps its library: a fused decode looked up through it is recorded with its arguments and reports
    success without doing anything; every other symbol is the library's own."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        if not name.startswith("labrador_ldpc_decode_ms_quantised_"):
            return getattr(self.real, name)

        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


def test_fused_python_method_passes_its_arguments(monkeypatch):
    """(output, iters, success) come back; dtype chooses the entry; lim=None is the type's maximum; maxiters, scale, lim and the
    variant reach the entry as given."""
    code = LDPCCode.TC128
    spy = _SpyLib(la.lib)
    monkeypatch.setattr(la, "lib", spy)
    y = np.ones((3, code.n()), np.float32)
    for kw, name, tail in ((dict(), FUSED[0], (3, 50, 8.0, 127)), (dict(dtype="i16"), FUSED[1], (3, 50, 8.0, 32767)),
                           (dict(dtype="i16", scale=64, lim=2047, maxiters=25), FUSED[1], (3, 25, 64.0, 2047)),
                           (dict(lim=31, maxiters=0, variant=64), FUSED[0], (3, 0, 8.0, 31))):
        del spy.calls[:]
        res = code.decode_ms_quantised_batch(y, **kw)
        (got, args), = spy.calls
        assert got == name and len(args) == 10 and args[5:9] == tail, (kw, args)
        assert ctypes.cast(args[9], ctypes.POINTER(la.HipOpts)).contents.variant == kw.get("variant", 0)
        assert len(res) == 3 and res[0].shape == (3, code.output_len()) and res[1].dtype == np.uint32 and res[2].dtype == np.uint8


# ---- the shape of the two kernels -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def quantise_object():
    return layered_helpers.built_object("llr_quantise.o")


def test_quantise_kernels_stream(quantise_object):
    """llr_quantise.o holds quantise_kernel for int8_t and int16_t, nothing else; neither touches scratch or LDS; every load of LLRs is
    16 bytes per lane and non-temporal; a lane stores the 4 (i8) or 8 (i16) bytes its quad became."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    kernels = layered_helpers.kernels(quantise_object, "quantise_kernel")
    assert len(kernels) == 2 and len(layered_helpers.kernels(quantise_object, "")) == 2, sorted(kernels)
    text = {name: [t for _, t, _ in body] for name, body in kernels.items()}
    for name, lines in text.items():
        ops = [t.split()[0] for t in lines]
        assert not any(x.startswith(("scratch_", "ds_", "buffer_", "flat_")) or "atomic" in x for x in ops), name
        loads = [t for t in lines if t.split()[0].startswith("global_load")]
        stores = [t.split()[0] for t in lines if t.split()[0].startswith("global_store")]
        assert len(loads) == 4 and all(t.split()[0] == "global_load_dwordx4" and t.split()[-1] == "nt" for t in loads), (name, loads)
        want = "global_store_dword" if "IaE" in name else "global_store_dwordx2"            # (Ia = int8_t, Is = int16_t)
        assert len(stores) == 4 and set(stores) == {want}, (name, stores)
        assert sum(x.startswith("v_mul_f32") for x in ops) == 16 and not any("fma" in x or "mac" in x for x in ops), name    # one multiply per LLR
        assert sum(x.startswith("v_rndne_f32") for x in ops) == 16, name
    assert sorted("IaE" in k for k in text) == [False, True] and sorted("IsE" in k for k in text) == [False, True]
    res = kernel_resources.resources("build/csrc/llr_quantise.o")
    assert len(res) == 2
    for _, name, vgpr, spill, _, lds, scratch in res:
        assert int(spill) == 0 and int(lds) == 0 and int(scratch) == 0 and int(vgpr) <= 64, (name, vgpr, spill, lds, scratch)
