"""CPU-side checks of the soft two-stage decode (labrador_ldpc_decode_ms_cascade_soft_batch_{f32,i8,i16}): the header
declares and the library, the Python table and the Rust shim hold the three entry points; the Python methods reach them with the
right arguments; the argument checks answer in the hard cascade's order before any device work; the restatement
(tests/cascade_soft_restatement.py) agrees with the hard one on output, iters, success and stage; and the frames the GPU tests use put
frames into both stages.  No compute call needs a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import cascade_restatement as cr
import cascade_soft_restatement as csr
import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode
from layered_helpers import quantise
import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED, OK = -1, -4, 0
NAMES = [f"labrador_ldpc_decode_ms_cascade_soft_batch_{t}" for t in ("f32", "i8", "i16")]
FIXED = (("i8", np.int8), ("i16", np.int16))


# ---- what fails without the feature ---------------------------------------------------------------------------------------------------
def test_header_declares_the_soft_cascade_entry_points():
    text = open(os.path.join(ROOT, "include", "labrador_ldpc_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    head = (r"\s*\(\s*enum labrador_ldpc_code code,\s*const {t} \*llrs,\s*{a} \*app,\s*uint8_t \*output,\s*uint32_t \*iters,\s*"
            r"uint8_t \*success,\s*uint8_t \*stage,\s*size_t batch,\s*size_t max_iters,\s*size_t max_sweeps,\s*")
    tail = r"const struct labrador_ldpc_hip_opts \*opts\s*\)\s*;"
    assert re.search(r"int\s+labrador_ldpc_decode_ms_cascade_soft_batch_f32" + head.format(t="float", a="float") +
                     r"float flooding_scale,\s*float flooding_offset,\s*float scale,\s*float offset,\s*" + tail, src)
    for suf, t in (("i8", "int8_t"), ("i16", "int16_t")):
        assert re.search(rf"int\s+labrador_ldpc_decode_ms_cascade_soft_batch_{suf}" + head.format(t=t, a="int32_t") +
                         r"uint32_t scale_num,\s*uint32_t scale_shift,\s*uint32_t offset,\s*" + tail, src)
    assert re.search(r"#define\s+LABRADOR_LDPC_HIP_ABI\s+3\b", text)                # additions only
    comment = text[text.index("The cascade with SOFT OUTPUT"):text.index("int labrador_ldpc_decode_ms_cascade_soft_batch_f32")]
    assert "comparable only within a stage" in comment and "f32-PIPE RATE" in comment and "16-byte aligned" in comment


def test_library_python_and_rust_hold_the_soft_cascade_entry_points():
    dll = ctypes.CDLL(la.LIB_PATH)
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for name, app in zip(NAMES, ("f32", "i32", "i32")):
        assert hasattr(dll, name) and name in la.SYMBOLS
        assert la.SYMBOLS[name][1][1:7] == [ctypes.c_void_p] * 6 and la.SYMBOLS[name][1][7:10] == [ctypes.c_size_t] * 3
        assert re.search(rf"pub fn {name}\s*\([^)]*app: \*mut {app}, output: \*mut u8, [^)]*stage: \*mut u8, batch: usize, max_iters: usize, "
                         r"max_sweeps: usize, [^)]*opts: \*const HipOpts\) -> c_int;", rust), name
    assert la.SYMBOLS[NAMES[0]][1][10:14] == [ctypes.c_float] * 4
    assert la.SYMBOLS[NAMES[1]][1][10:13] == la.SYMBOLS[NAMES[2]][1][10:13] == [ctypes.c_uint32] * 3
    assert la.lib.labrador_ldpc_hip_abi_version() == 3


class _SpyLib:
    """Stands where the package keeps its library: a cascade decode looked up through it is recorded with its arguments and reports
    success without doing anything; every other symbol is the library's own."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        if not name.startswith("labrador_ldpc_decode_ms_cascade_"):
            return getattr(self.real, name)

        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


def test_python_methods_pass_their_arguments(monkeypatch):
    """(app, output, iters, success, stage) come back, app first; max_sweeps=None is maxiters; both pairs and the triple reach the entry
    as given, and none is the identity of the type; the caller's own buffers are the ones handed on."""
    code = LDPCCode.TC128
    V = code.n() + code.punctured_bits()
    spy = _SpyLib(la.lib)
    monkeypatch.setattr(la, "lib", spy)
    llrs = np.ones((3, code.n()), np.float32)
    for kw, tail in ((dict(), (3, 25, 25, 1.0, 0.0, 1.0, 0.0)), (dict(max_sweeps=7), (3, 25, 7, 1.0, 0.0, 1.0, 0.0)),
                     (dict(max_sweeps=0, scale=0.75), (3, 25, 0, 1.0, 0.0, 0.75, 0.0)), (dict(offset=0.5), (3, 25, 25, 1.0, 0.0, 1.0, 0.5)),
                     (dict(flooding_scale=0.8125, flooding_offset=0.25), (3, 25, 25, 0.8125, 0.25, 1.0, 0.0))):
        del spy.calls[:]
        res = code.decode_ms_cascade_soft_batch(llrs, 25, **kw)
        (name, args), = spy.calls
        assert name == NAMES[0] and len(args) == 15 and args[7:14] == tail, (kw, args)
        assert len(res) == 5 and res[0].shape == (3, V) and res[0].dtype == np.float32 and res[1].shape == (3, code.output_len())
        assert res[4].shape == (3,) and res[4].dtype == np.uint8 and res[2].dtype == np.uint32 and res[3].dtype == np.uint8
        assert args[1] == llrs.ctypes.data and args[2:7] == tuple(x.ctypes.data for x in res)
    for suf, dtype in FIXED:
        q = np.ones((3, code.n()), dtype)
        for kw, tail in ((dict(), (3, 25, 25, 1, 0, 0)), (dict(max_sweeps=9, scale_num=13, scale_shift=4), (3, 25, 9, 13, 4, 0)),
                         (dict(scale_shift=4), (3, 25, 25, 16, 4, 0)), (dict(offset=1), (3, 25, 25, 1, 0, 1))):
            del spy.calls[:]
            res = code.decode_ms_cascade_fixed_soft_batch(q, 25, **kw)
            (name, args), = spy.calls
            assert name == f"labrador_ldpc_decode_ms_cascade_soft_batch_{suf}" and len(args) == 14 and args[7:13] == tail, (kw, args)
            assert len(res) == 5 and res[0].shape == (3, V) and res[0].dtype == np.int32 and res[4].dtype == np.uint8
    mine = (np.zeros((3, V), np.float32), np.zeros((3, code.output_len()), np.uint8), np.zeros(3, np.uint32), np.zeros(3, np.uint8),
            np.zeros(3, np.uint8))
    del spy.calls[:]
    res = code.decode_ms_cascade_soft_batch(llrs, 25, app=mine[0], output=mine[1], iters=mine[2], success=mine[3], stage=mine[4])
    assert all(a is b for a, b in zip(res, mine))
    assert spy.calls[0][1][2:7] == tuple(x.ctypes.data for x in mine)


def test_python_methods_refuse_what_they_document():
    code = LDPCCode.TC128
    V = code.n() + code.punctured_bits()
    f32, i8 = np.ones((2, code.n()), np.float32), np.ones((2, code.n()), np.int8)
    for method, good, app_dtype, others in (
            (code.decode_ms_cascade_soft_batch, f32, np.float32, (i8, f32.astype(np.float64), f32.astype(np.float16), i8.astype(np.int16))),
            (code.decode_ms_cascade_fixed_soft_batch, i8, np.int32, (f32, i8.astype(np.int32), f32.astype(np.float64)))):
        for bad in others:                                                       # a type the entry does not have
            with pytest.raises(la.LdpcHipError, match="no batched kernel"):
                method(bad, 10)
        for bad in (good[0], good[:, :-1], [[1.0] * code.n()]):
            with pytest.raises(ValueError):
                method(bad, 10)
        wrong = np.int32 if app_dtype == np.float32 else np.int8
        for bad in (np.zeros((2, V), wrong), np.zeros((2, V), np.float64), np.zeros((2, V - 1), app_dtype), np.zeros((3, V), app_dtype),
                    np.zeros((2, 2 * V), app_dtype)[:, ::2], np.zeros(2 * V, app_dtype), [[0] * V] * 2):
            with pytest.raises(ValueError, match="app"):
                method(good, 10, app=bad)
        with pytest.raises(ValueError, match="stage"):
            method(good, 10, stage=np.zeros(3, np.uint8))
        with pytest.raises(ValueError, match="output"):
            method(good, 10, output=np.zeros((2, code.output_len() + 1), np.uint8))
    with pytest.raises(la.LdpcHipError, match="scale 1.5"):
        code.decode_ms_cascade_soft_batch(f32, 10, scale=1.5)
    with pytest.raises(la.LdpcHipError, match="scale 0 "):
        code.decode_ms_cascade_soft_batch(f32, 10, flooding_scale=0.0)
    with pytest.raises(la.LdpcHipError, match="scale_shift 40"):
        code.decode_ms_cascade_fixed_soft_batch(i8, 10, scale_shift=40)
    with pytest.raises(ValueError):
        code.decode_ms_cascade_fixed_soft_batch(i8, 10, scale_num=-1)
    with pytest.raises(TypeError):                                               # the integers have no stage-1 correction
        code.decode_ms_cascade_fixed_soft_batch(i8, 10, flooding_scale_num=13)


def buffers(code, dtype):
    V = code.n() + code.punctured_bits()
    llrs = np.ones((1, code.n()), dtype)
    app = np.full((1, V), 5, np.float32 if dtype == np.float32 else np.int32)
    out, it = np.full((1, code.output_len()), 0xEE, np.uint8), np.full(1, 77, np.uint32)
    ok, stage = np.full(1, 7, np.uint8), np.full(1, 9, np.uint8)
    arrays = (llrs, app, out, it, ok, stage)
    return arrays, [x.ctypes.data for x in arrays]


def untouched(arrays):
    llrs, app, out, it, ok, stage = arrays
    return bool((app == 5).all() and (out == 0xEE).all() and it[0] == 77 and ok[0] == 7 and stage[0] == 9)


def test_f32_argument_checks_come_before_any_device_work():
    """decode_cascade()'s order: the code, both pairs -- before the empty batch --, the empty batch whatever the pointers, the buffers
    (`app` and `stage` among them), then a stage-1 pair with a variant.  All without a GPU, where a call that reached a device would
    say ENODEV."""
    code = LDPCCode.TC128
    fn = la.lib.labrador_ldpc_decode_ms_cascade_soft_batch_f32
    arrays, p = buffers(code, np.float32)
    assert fn(9, *p, 1, 10, 10, 1.0, 0.0, 1.0, 0.0, None) == EINVAL and "out of range" in la.last_error()
    assert fn(-1, *p, 1, 10, 10, 1.0, 0.0, 2.0, 0.0, None) == EINVAL and "out of range" in la.last_error()      # the code comes first
    for pairs, text in (((1.0, 0.0, 1.5, 0.0), "scale 1.5"), ((0.0, 0.0, 1.0, 0.0), "scale 0 "), ((1.0, 0.0, 1.0, -1.0), "offset -1"),
                        ((1.0, -1.0, 1.0, 0.0), "offset -1"), ((float("nan"), 0.0, 1.0, 0.0), "scale"),
                        ((0.0, 0.0, 1.5, 0.0), "scale 0 ")):                                                     # stage 1's pair first
        for batch in (0, 1):                                                                                     # ... before the empty batch
            assert fn(int(code), *p, batch, 10, 10, *pairs, None) == EINVAL, (pairs, batch)
            assert text in la.last_error() and "is not in" in la.last_error(), la.last_error()
        assert fn(int(code), *([None] * 6), 1, 10, 10, *pairs, None) == EINVAL and "is not in" in la.last_error()
    assert fn(int(code), *p, 0, 10, 10, 0.8125, 0.0, 1.0, 0.5, None) == OK
    assert fn(int(code), *([None] * 6), 0, 10, 10, 1.0, 0.1, 1.0, 0.0, None) == OK
    for i in range(6):                                                                                           # 1: app, 5: stage
        q = list(p)
        q[i] = None
        for memory in (la.MEM_HOST, la.MEM_DEVICE):
            opts = la.HipOpts(-1, memory, None, 2, 0, None)
            assert fn(int(code), *q, 1, 10, 10, 1.0, 0.1, 1.0, 0.0, ctypes.byref(opts)) == EINVAL and "NULL" in la.last_error(), i
    for memory in (la.MEM_HOST, la.MEM_DEVICE):
        opts = la.HipOpts(-1, memory, None, 2, 0, None)
        assert fn(int(code), *p, 1, 10, 10, 1.0, 0.1, 1.0, 0.0, ctypes.byref(opts)) == EUNSUPPORTED
        assert "corrected flooding decoder" in la.last_error() and "variant 2" in la.last_error()
    assert untouched(arrays)


def test_fixed_argument_checks_come_before_any_device_work():
    """i8 and i16: the code, the empty batch, the buffers, and only then the triple, naming the parameter."""
    code = LDPCCode.TC128
    for suf, dtype in FIXED:
        tmax = int(np.iinfo(dtype).max)
        fn = getattr(la.lib, f"labrador_ldpc_decode_ms_cascade_soft_batch_{suf}")
        arrays, p = buffers(code, dtype)
        assert fn(9, *p, 1, 10, 10, 13, 4, 0, None) == EINVAL and "out of range" in la.last_error()
        assert fn(-1, *p, 1, 10, 10, 0, 9, 0, None) == EINVAL and "out of range" in la.last_error()
        assert fn(int(code), *p, 0, 10, 10, 0, 9, tmax + 1, None) == OK                                    # an empty batch gets no further
        assert fn(int(code), *([None] * 6), 0, 10, 10, 13, 4, 0, None) == OK
        for i in range(6):
            q = list(p)
            q[i] = None
            assert fn(int(code), *q, 1, 10, 10, 13, 4, 1, None) == EINVAL and "NULL" in la.last_error()
            assert fn(int(code), *q, 1, 10, 10, 0, 9, tmax + 1, None) == EINVAL and "NULL" in la.last_error()   # the buffers come first
        for memory in (la.MEM_HOST, la.MEM_DEVICE):
            opts = la.HipOpts(-1, memory, None, 0, 0, None)
            for triple, text in (((1, 9, 0), "scale_shift 9"), ((0, 0, 0), "scale_num"), ((17, 4, 0), "scale_num"),
                                 ((13, 4, tmax + 1), f"offset {tmax + 1}")):
                assert fn(int(code), *p, 1, 10, 10, *triple, ctypes.byref(opts)) == EINVAL, (suf, triple)
                assert text in la.last_error() and "is not in" in la.last_error(), la.last_error()
        assert untouched(arrays)


# ---- the restatement: passes without the feature ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (np.float32, np.int8), ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("code", (LDPCCode.TC128, LDPCCode.TM1280), ids=lambda c: c.name)
def test_hard_results_are_the_hard_cascades(code, dtype):
    """compose_soft's output, iters, success and stage equal cascade_restatement.cascade's at the same arguments, identity and not;
    a stage-0 row of the marginals is the flooding decoder's and a stage-1 row the layered decoder's."""
    llrs = csr.frames(code, dtype)[:48]
    correction = (1.0, 0.5) if dtype == np.float32 else (13, 4, 1)
    for caps in csr.CAPS:
        for corr in (None, correction):
            soft = csr.cascade_soft(code, llrs, *caps, corr)
            hard = cr.cascade(code, llrs, *caps, corr)
            for name, s, h in zip(("output", "iters", "success", "stage"), soft[1:], hard):
                assert s.dtype == h.dtype and (s == h).all(), (caps, corr, name)
            app, stage = soft[0], soft[4]
            assert app.dtype == (np.float32 if dtype == np.float32 else np.int32) and app.shape == (48, code.n() + code.punctured_bits())
            first = oracle.decode_ms_soft_batch(code, llrs, caps[0])[3]
            second = cr.layered(code, corr)(llrs, caps[1])[3]
            assert (app[stage == 0] == first[stage == 0]).all() and (app[stage == 1] == second[stage == 1]).all()


def test_same_soft_compares_float_marginals_as_values():
    z = np.zeros(2, np.uint8)
    a = np.array([[np.nan, -0.0, 1.0], [2.0, 0.0, np.inf]], np.float32)
    b = np.array([[np.nan, 0.0, 1.0], [2.0, -0.0, np.inf]], np.float32)
    csr.same_soft((a, z, z, z, z), (b, z, z, z, z))
    b[1, 0] = np.nan
    with pytest.raises(AssertionError, match="app differs in frames \\[1\\]"):
        csr.same_soft((a, z, z, z, z), (b, z, z, z, z))
    with pytest.raises(AssertionError):
        csr.same_soft((np.ones((2, 3), np.int32), z, z, z, z), (np.ones((2, 3), np.int64), z, z, z, z))


GPU_CASES = [(LDPCCode.TC128, np.float32), (LDPCCode.TM1280, np.float32), (LDPCCode.TM8192, np.float32), (LDPCCode.TC128, np.int8),
             (LDPCCode.TM1280, np.int8), (LDPCCode.TM2048, np.int8), (LDPCCode.TM2048, np.int16)]


@pytest.mark.parametrize("code,dtype", GPU_CASES, ids=[f"{c.name}-{np.dtype(t).name}" for c, t in GPU_CASES])
def test_the_gpu_tests_frames_reach_both_stages(code, dtype):
    """The condition the GPU tests rest on, met by the reference's flooding decoder alone (`stage` is its verdict): at BOTH tested caps
    both stages carry frames; the batch is no multiple of a codeword group; and, but for TM8192's 41 frames, more than 64 frames fail
    the first stage at cap 3, so that the compaction's places cross a wave."""
    llrs = csr.frames(code, dtype)
    assert len(llrs) % 16 != 0 and not llrs.flags.writeable
    for max_iters, _ in csr.CAPS:
        failed = int((oracle.decode_ms_batch(code, llrs, max_iters)[2] == 0).sum())
        print(f"{code.name} {np.dtype(dtype).name} cap {max_iters}: {failed} of {len(llrs)} frames go to stage 2")
        assert 1 <= failed < len(llrs)
        if max_iters == 3 and code != LDPCCode.TM8192:
            assert failed > 64


# ---- the shape of the two new kernels ---------------------------------------------------------------------------------------------------
def test_marginal_kernels_stream():
    """cascade_app.o holds the row scatter and the widening of each integer type, nothing else; none touches scratch, LDS or an atomic;
    the scatter moves 16 bytes per lane both ways; the widening loads 4 (int8) or 8 (int16) bytes per lane and stores 16."""
    import sys
    import layered_helpers
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    obj = layered_helpers.built_object("cascade_app.o")
    kernels = layered_helpers.kernels(obj, "cascade_")
    ops = {name: [t.split()[0] for _, t, _ in body] for name, body in kernels.items()}
    assert len(kernels) == 3 and len(layered_helpers.kernels(obj, "")) == 3, sorted(kernels)
    scatter, = [k for k in ops if "cascade_scatter_rows_kernel" in k]
    widen8, = [k for k in ops if "cascade_widen_app_kernel" in k and "IaE" in k]
    widen16, = [k for k in ops if "cascade_widen_app_kernel" in k and "IsE" in k]
    for name, o in ops.items():
        assert not any(x.startswith(("scratch_", "ds_", "buffer_")) or "atomic" in x for x in o), name
        assert {x for x in o if x.startswith("global_store")} == {"global_store_dwordx4"}, name
    loads = lambda k: {x for x in ops[k] if x.startswith("global_load")}
    assert loads(scatter) == {"global_load_dword", "global_load_dwordx4"}                                   # (dword: the list's entries)
    assert loads(widen8) == {"global_load_dword"} and loads(widen16) == {"global_load_dwordx2"}
    res = kernel_resources.resources("build/csrc/cascade_app.o")
    assert len(res) == 3
    for _, name, vgpr, spill, _, lds, scratch in res:
        assert int(spill) == 0 and int(lds) == 0 and int(scratch) == 0 and int(vgpr) <= 32, (name, vgpr, spill, lds, scratch)
