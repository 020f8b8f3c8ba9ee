"""CPU-side checks of the two-stage ("cascade") decode (labrador_ldpc_decode_ms_cascade_batch_{f32,i8,i16}): the
restatement (tests/cascade_restatement.py) reproduces the failure counts of the design's table and its edge cases; the header
declares and the library, the Python table and the Rust shim hold the three entry points; their argument checks answer in the
documented order before any device work; the Python methods refuse what they document; the three kernels of cascade.o have the
shape they were written for.  No compute call needs a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import cascade_restatement as cr
import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode
import layered_helpers
from layered_helpers import quantise
import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, OK = -1, 0
NAMES = [f"labrador_ldpc_decode_ms_cascade_batch_{t}" for t in ("f32", "i8", "i16")]
FIXED = (("i8", np.int8), ("i16", np.int16))


# ---- the restatement: passes without the feature, pins the numbers -----------------------------------------------------------------
@pytest.fixture(scope="module")
def tm2048_frames():
    y, _ = oracle.awgn_llrs(LDPCCode.TM2048, np.random.default_rng(1700), 600, 1.7, np.float32)
    return y


def test_i8_failure_counts_at_fixed_seeds(tm2048_frames):
    """TM2048 at 1.7 dB, 600 frames of default_rng(1700) at 8 / 31, cap 25 in both stages: flooding fails 164 frames, which go to stage
    2; 34 of them fail plain layered decoding too and 14 at (13, 4, 0) -- the layered decoder's own counts on all 600 frames."""
    code = LDPCCode.TM2048
    llrs = quantise(tm2048_frames, np.int8, 8, 31)
    for correction, failures in ((None, 34), ((13, 4, 0), 14)):
        out, it, ok, stage = cr.cascade(code, llrs, 25, 25, correction)
        print(f"TM2048 1.7 dB i8 {correction}: {int(stage.sum())} frames to stage 2, {int((ok == 0).sum())} failures")
        assert int(stage.sum()) == 164 and int((ok == 0).sum()) == failures
        alone = cr.layered(code, correction)(llrs, 25)
        assert int((alone[2] == 0).sum()) == failures
        assert not (ok[stage == 0] == 0).any() and (it[(ok == 0)] == 25).all()
        second = stage == 1                                    # the frames of stage 2 carry the layered decoder's results
        assert (out[second] == alone[0][second]).all() and (it[second] == alone[1][second]).all() and (ok[second] == alone[2][second]).all()


def test_f32_failure_counts_at_fixed_seeds(tm2048_frames):
    """The same frames as float32: 156 go to stage 2, 25 fail both stages."""
    out, it, ok, stage = cr.cascade(LDPCCode.TM2048, tm2048_frames, 25, 25)
    print(f"TM2048 1.7 dB f32: {int(stage.sum())} frames to stage 2, {int((ok == 0).sum())} failures")
    assert int(stage.sum()) == 156 and int((ok == 0).sum()) == 25


@pytest.mark.parametrize("dtype", (np.float32, np.int8, np.int16), ids=lambda t: np.dtype(t).name)
def test_caps_of_zero(dtype):
    """max_iters = 0 is the layered decoder on every frame; max_sweeps = 0 leaves every frame flooding failed zeroed."""
    code = LDPCCode.TC128
    y, _ = oracle.awgn_llrs(code, np.random.default_rng(3), 24, 3.0, np.float32)
    llrs = y if dtype == np.float32 else quantise(y, dtype, 8, 31)
    out, it, ok, stage = cr.cascade(code, llrs, 0, 25)
    alone = cr.layered(code)(llrs, 25)
    assert stage.all() and (out == alone[0]).all() and (it == alone[1]).all() and (ok == alone[2]).all()
    out, it, ok, stage = cr.cascade(code, llrs, 4, 0)
    first = oracle.decode_ms_batch(code, llrs, 4)
    assert (stage == (first[2] == 0)).all() and stage.any() and not stage.all()
    assert not out[stage == 1].any() and not it[stage == 1].any() and not ok[stage == 1].any()
    assert (out[stage == 0] == first[0][stage == 0]).all() and (it[stage == 0] == first[1][stage == 0]).all() and ok[stage == 0].all()


# ---- what fails without the feature ---------------------------------------------------------------------------------------------------
def test_header_declares_the_cascade_entry_points():
    text = open(os.path.join(ROOT, "include", "labrador_ldpc_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    head = (r"\s*\(\s*enum labrador_ldpc_code code,\s*const {t} \*llrs,\s*uint8_t \*output,\s*uint32_t \*iters,\s*uint8_t \*success,\s*"
            r"uint8_t \*stage,\s*size_t batch,\s*size_t max_iters,\s*size_t max_sweeps,\s*")
    tail = r"const struct labrador_ldpc_hip_opts \*opts\s*\)\s*;"
    assert re.search(r"int\s+labrador_ldpc_decode_ms_cascade_batch_f32" + head.format(t="float") + r"float scale,\s*float offset,\s*" + tail, src)
    for suf, t in (("i8", "int8_t"), ("i16", "int16_t")):
        assert re.search(rf"int\s+labrador_ldpc_decode_ms_cascade_batch_{suf}" + head.format(t=t) +
                         r"uint32_t scale_num,\s*uint32_t scale_shift,\s*uint32_t offset,\s*" + tail, src)
    assert re.search(r"#define\s+LABRADOR_LDPC_HIP_ABI\s+3\b", text)                # additions only
    comment = text[text.index('Two-stage ("cascade")'):text.index("int labrador_ldpc_decode_ms_cascade_batch_f32")]
    assert "once per launch slice" in comment and "captured into a graph" in comment


def test_library_python_and_rust_hold_the_cascade_entry_points():
    dll = ctypes.CDLL(la.LIB_PATH)
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for name in NAMES:
        assert hasattr(dll, name) and name in la.SYMBOLS
        assert la.SYMBOLS[name][1][6:9] == [ctypes.c_size_t] * 3
        assert re.search(rf"pub fn {name}\s*\([^)]*stage: \*mut u8, batch: usize, max_iters: usize, max_sweeps: usize, [^)]*"
                         r"opts: \*const HipOpts\) -> c_int;", rust), name
    assert la.SYMBOLS[NAMES[0]][1][9:11] == [ctypes.c_float] * 2
    assert la.SYMBOLS[NAMES[1]][1][9:12] == la.SYMBOLS[NAMES[2]][1][9:12] == [ctypes.c_uint32] * 3
    assert la.lib.labrador_ldpc_hip_abi_version() == 3


def buffers(code, dtype):
    llrs = np.ones((1, code.n()), dtype)
    out, it = np.full((1, code.output_len()), 0xEE, np.uint8), np.full(1, 77, np.uint32)
    ok, stage = np.full(1, 7, np.uint8), np.full(1, 9, np.uint8)
    return (llrs, out, it, ok, stage), [x.ctypes.data for x in (llrs, out, it, ok, stage)]


def test_f32_argument_checks_come_before_any_device_work():
    """The order of decode_batch(): the code, the range of (scale, offset) -- before the empty batch --, the empty batch whatever the
    pointers, then the buffers, `stage` among them.  All without a GPU, where a call that reached a device would say ENODEV."""
    code = LDPCCode.TC128
    fn = la.lib.labrador_ldpc_decode_ms_cascade_batch_f32
    arrays, p = buffers(code, np.float32)
    assert fn(9, *p, 1, 10, 10, 1.0, 0.0, None) == EINVAL and "out of range" in la.last_error()
    assert fn(-1, *p, 1, 10, 10, 2.0, 0.0, None) == EINVAL and "out of range" in la.last_error()           # the code comes first
    for scale, offset, text in ((0.0, 0.0, "scale"), (1.5, 0.0, "scale"), (float("nan"), 0.0, "scale"), (-0.5, 0.0, "scale"),
                                (1.0, -0.1, "offset"), (1.0, float("inf"), "offset"), (1.0, float("nan"), "offset")):
        for batch in (0, 1):                                                                               # ... before the empty batch
            assert fn(int(code), *p, batch, 10, 10, scale, offset, None) == EINVAL, (scale, offset, batch)
            assert text in la.last_error() and "is not in" in la.last_error()
        assert fn(int(code), *([None] * 5), 1, 10, 10, scale, offset, None) == EINVAL and "is not in" in la.last_error()
    assert fn(int(code), *p, 0, 10, 10, 0.8125, 0.0, None) == OK
    assert fn(int(code), *([None] * 5), 0, 10, 10, 1.0, 0.1, None) == OK
    for i in range(5):
        q = list(p)
        q[i] = None
        for memory in (la.MEM_HOST, la.MEM_DEVICE):
            opts = la.HipOpts(-1, memory, None, 3, 0, None)
            assert fn(int(code), *q, 1, 10, 10, 1.0, 0.0, ctypes.byref(opts)) == EINVAL and "NULL" in la.last_error(), i
    llrs, out, it, ok, stage = arrays
    assert (out == 0xEE).all() and it[0] == 77 and ok[0] == 7 and stage[0] == 9


def test_fixed_argument_checks_come_before_any_device_work():
    """i8 and i16: the code, the empty batch, the buffers, and only then the triple (as DESIGN.md 4.8 has it), naming the parameter."""
    code = LDPCCode.TC128
    for suf, dtype in FIXED:
        tmax = int(np.iinfo(dtype).max)
        fn = getattr(la.lib, f"labrador_ldpc_decode_ms_cascade_batch_{suf}")
        arrays, p = buffers(code, dtype)
        assert fn(9, *p, 1, 10, 10, 13, 4, 0, None) == EINVAL and "out of range" in la.last_error()
        assert fn(-1, *p, 1, 10, 10, 0, 9, 0, None) == EINVAL and "out of range" in la.last_error()
        assert fn(int(code), *p, 0, 10, 10, 0, 9, tmax + 1, None) == OK                                    # an empty batch gets no further
        assert fn(int(code), *([None] * 5), 0, 10, 10, 13, 4, 0, None) == OK
        for i in range(5):
            q = list(p)
            q[i] = None
            assert fn(int(code), *q, 1, 10, 10, 13, 4, 1, None) == EINVAL and "NULL" in la.last_error()
            assert fn(int(code), *q, 1, 10, 10, 0, 9, tmax + 1, None) == EINVAL and "NULL" in la.last_error()   # the buffers come first
        for memory in (la.MEM_HOST, la.MEM_DEVICE):
            for variant in (0, 3):
                opts = la.HipOpts(-1, memory, None, variant, 0, None)
                for triple, text in (((1, 9, 0), "scale_shift"), ((0, 0, 0), "scale_num"), ((17, 4, 0), "scale_num"), ((2, 0, 0), "scale_num"),
                                     ((257, 8, 0), "scale_num"), ((13, 4, tmax + 1), "offset"), ((1, 0, 0xFFFFFFFF), "offset")):
                    assert fn(int(code), *p, 1, 10, 10, *triple, ctypes.byref(opts)) == EINVAL, (suf, triple)
                    assert text in la.last_error() and "is not in" in la.last_error(), la.last_error()
        llrs, out, it, ok, stage = arrays
        assert (out == 0xEE).all() and it[0] == 77 and ok[0] == 7 and stage[0] == 9


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
    """(output, iters, success, stage) come back; max_sweeps=None is maxiters; the corrections reach the entry as given, and none is
    the identity of the type."""
    code = LDPCCode.TC128
    spy = _SpyLib(la.lib)
    monkeypatch.setattr(la, "lib", spy)
    llrs = np.ones((3, code.n()), np.float32)
    for kw, tail in ((dict(), (3, 25, 25, 1.0, 0.0)), (dict(max_sweeps=7), (3, 25, 7, 1.0, 0.0)), (dict(max_sweeps=0, scale=0.75), (3, 25, 0, 0.75, 0.0)),
                     (dict(offset=0.5), (3, 25, 25, 1.0, 0.5))):
        del spy.calls[:]
        res = code.decode_ms_cascade_batch(llrs, 25, **kw)
        (name, args), = spy.calls
        assert name == NAMES[0] and len(args) == 12 and args[6:11] == tail, (kw, args)
        assert len(res) == 4 and res[0].shape == (3, code.output_len()) and res[3].shape == (3,) and res[3].dtype == np.uint8
        assert res[1].dtype == np.uint32 and res[2].dtype == np.uint8
    for suf, dtype in FIXED:
        q = np.ones((3, code.n()), dtype)
        for kw, tail in ((dict(), (3, 25, 25, 1, 0, 0)), (dict(max_sweeps=9, scale_num=13, scale_shift=4), (3, 25, 9, 13, 4, 0)),
                         (dict(scale_shift=4), (3, 25, 25, 16, 4, 0)), (dict(offset=1), (3, 25, 25, 1, 0, 1))):
            del spy.calls[:]
            res = code.decode_ms_cascade_fixed_batch(q, 25, **kw)
            (name, args), = spy.calls
            assert name == f"labrador_ldpc_decode_ms_cascade_batch_{suf}" and len(args) == 13 and args[6:12] == tail, (kw, args)
            assert len(res) == 4 and res[3].shape == (3,) and res[3].dtype == np.uint8
    # the caller's own buffers are the ones handed on and returned
    mine = (np.zeros((3, code.output_len()), np.uint8), np.zeros(3, np.uint32), np.zeros(3, np.uint8), np.zeros(3, np.uint8))
    del spy.calls[:]
    res = code.decode_ms_cascade_batch(llrs, 25, output=mine[0], iters=mine[1], success=mine[2], stage=mine[3])
    assert all(a is b for a, b in zip(res, mine))
    assert spy.calls[0][1][2:6] == tuple(x.ctypes.data for x in mine)


def test_python_methods_refuse_what_they_document():
    code = LDPCCode.TC128
    f32, i8 = np.ones((2, code.n()), np.float32), np.ones((2, code.n()), np.int8)
    for method, good, others in ((code.decode_ms_cascade_batch, f32, (i8, f32.astype(np.float64), i8.astype(np.int32))),
                                 (code.decode_ms_cascade_fixed_batch, i8, (f32, i8.astype(np.int32), f32.astype(np.float64)))):
        for bad in others:                                                       # a type the entry does not have
            with pytest.raises((ValueError, la.LdpcHipError)):
                method(bad, 10)
        for bad in (good[0], good[:, :-1], np.ones((2, code.n() + 1), good.dtype), [[1.0] * code.n()]):
            with pytest.raises(ValueError):
                method(bad, 10)
        for bad in (np.zeros(3, np.uint8), np.zeros((2, 1), np.uint8), np.zeros(2, np.int8), np.zeros(2, np.uint32), np.zeros(4, np.uint8)[::2],
                    [0, 0]):
            with pytest.raises(ValueError, match="stage"):
                method(good, 10, stage=bad)
        with pytest.raises(ValueError, match="output"):
            method(good, 10, output=np.zeros((2, code.output_len() + 1), np.uint8))
        with pytest.raises(ValueError, match="success"):
            method(good, 10, success=np.zeros(3, np.uint8))
    with pytest.raises(la.LdpcHipError, match="scale 1.5"):
        code.decode_ms_cascade_batch(f32, 10, scale=1.5)
    with pytest.raises(la.LdpcHipError, match="scale_shift 40"):
        code.decode_ms_cascade_fixed_batch(i8, 10, scale_shift=40)
    with pytest.raises(ValueError):
        code.decode_ms_cascade_fixed_batch(i8, 10, scale_num=-1)


def test_the_ber_harness_knows_the_cascade():
    """--schedule cascade takes the layered schedule's options and --max-sweeps; the other schedules refuse --max-sweeps: decided
    before any device work."""
    from labrador_ldpc_amd import perftest
    code = LDPCCode.TC128
    for bad in (dict(schedule="layered", max_sweeps=5), dict(max_sweeps=5), dict(schedule="cascade", llr="i8", scale=0.8),
                dict(schedule="cascade", scale_num=13, scale_shift=4), dict(schedule="cascade", llr="f64")):
        with pytest.raises(ValueError):
            perftest.ms_trials(code, 3.0, "ebn0", **bad)
    for bad in (["--schedule", "layered", "--max-sweeps", "5"], ["--max-sweeps", "5"], ["--schedule", "cascade", "--fixed-scale", "13/16"],
                ["--schedule", "cascade", "--llr", "i8", "--scale", "0.8"], ["--schedule", "cascade", "--max-sweeps", "x"]):
        with pytest.raises(SystemExit) as e:
            perftest.main(["--code", "TC128", "--snrs", "3.0"] + bad)
        assert e.value.code == 2, bad


# ---- the shape of the three kernels ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cascade_object():
    return layered_helpers.built_object("cascade.o")


def test_cascade_kernels_stream(cascade_object):
    """cascade.o holds the compaction, the scatter and the gather of each LLR type in its two forms, nothing else; none touches scratch
    or LDS; the compaction has its one atomic; the aligned gathers move 16 bytes per lane both ways and the scatter 8."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    kernels = layered_helpers.kernels(cascade_object, "cascade_")
    ops = {name: [t.split()[0] for _, t, _ in body] for name, body in kernels.items()}
    assert len(kernels) == 8 and len(layered_helpers.kernels(cascade_object, "")) == 8, sorted(kernels)
    compact = [k for k in ops if "cascade_compact_kernel" in k]
    scatter = [k for k in ops if "cascade_scatter_kernel" in k]
    aligned = [k for k in ops if "cascade_gather_kernel" in k and "Lb1E" in k]
    plain = [k for k in ops if "cascade_gather_kernel" in k and "Lb0E" in k]
    assert (len(compact), len(scatter), len(aligned), len(plain)) == (1, 1, 3, 3), sorted(ops)
    for name, o in ops.items():
        assert not any(x.startswith(("scratch_", "ds_", "buffer_")) for x in o), name
        assert any(x.startswith(("global_atomic", "flat_atomic")) for x in o) == (name in compact), name
    assert [x for x in ops[compact[0]] if "atomic" in x] == ["global_atomic_add"]
    for name in aligned:
        loads = [x for x in ops[name] if x.startswith("global_load") and x != "global_load_dword"]      # (dword: the list's entries)
        stores = [x for x in ops[name] if x.startswith("global_store")]
        assert loads and set(loads) == {"global_load_dwordx4"} and set(stores) == {"global_store_dwordx4"}, (name, set(loads), set(stores))
    assert "global_load_dwordx2" in ops[scatter[0]] and "global_store_dwordx2" in ops[scatter[0]]
    res = kernel_resources.resources("build/csrc/cascade.o")
    assert len(res) == 8
    for _, name, vgpr, spill, _, lds, scratch in res:
        assert int(spill) == 0 and int(lds) == 0 and int(scratch) == 0 and int(vgpr) <= 64, (name, vgpr, spill, lds, scratch)
