"""CPU-side checks of the f32-input forms of the fixed-point layered decoders and of the integer cascade
(labrador_ldpc_decode_ms_layered_quantised_{,soft_}batch_{i8,i16}, labrador_ldpc_decode_ms_cascade_quantised_batch_{i8,i16}; DESIGN.md
4.11): the header declares and the library, the Python table and the Rust shim hold the six entry points; their argument checks answer
in the order of the entries they compose, with those entries' texts, before any device work; the Python methods and the BER harness
refuse what they document; the kernels of decode_ms_fixed_quantised.o have the LDS, no more scratch and no fewer waves per SIMD than
their integer-source counterparts; and the cascade restatement on the quantised frames of tests/test_gpu_quantise.py gives the counts
of the design's table.  No call here needs a GPU."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode
import layered_helpers
import oracle
import quantise_restatement as qr
import quantised_layered_restatement as qlr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, OK, EUNSUPPORTED = -1, 0, -4
TYPES = (("i8", np.int8), ("i16", np.int16))
HARD = [f"labrador_ldpc_decode_ms_layered_quantised_batch_{t}" for t, _ in TYPES]
SOFT = [f"labrador_ldpc_decode_ms_layered_quantised_soft_batch_{t}" for t, _ in TYPES]
CASCADE = [f"labrador_ldpc_decode_ms_cascade_quantised_batch_{t}" for t, _ in TYPES]
PARAMS = {"i8": (8.0, 31), "i16": (64.0, 2047)}


# ---- the restatement: passes without the feature, pins the numbers -------------------------------------------------------------------
# code: (seed, frames, Eb/N0, cap) of tests/test_gpu_quantise.py's CASES, then per type (sent to stage 2, failures plain, failures at
# (13, 4, 0)), the cap in both stages
TABLE = {LDPCCode.TC128: ((41, 64, 3.0, 20), {"i8": (3, 2, 2), "i16": (1, 0, 1)}),
         LDPCCode.TM1280: ((42, 48, 3.2, 25), {"i8": (10, 6, 6), "i16": (8, 3, 2)}),
         LDPCCode.TM2048: ((43, 48, 1.9, 25), {"i8": (3, 0, 0), "i16": (3, 0, 0)}),
         LDPCCode.TM8192: ((44, 12, 1.6, 25), {"i8": (6, 0, 0), "i16": (5, 0, 0)})}


@pytest.mark.parametrize("code", list(TABLE), ids=lambda c: c.name)
def test_cascade_restatement_counts_on_the_quantised_frames(code):
    (seed, frames, ebn0, cap), want = TABLE[code]
    y, _ = oracle.awgn_llrs(code, np.random.default_rng(seed), frames, ebn0, np.float32)
    for suf, dtype in TYPES:
        got = []
        for triple in (None, (13, 4, 0)):
            out, it, ok, stage = qlr.cascade_quantised(code, y, dtype, *PARAMS[suf], cap, cap, triple)
            got.append((int(stage.sum()), int((ok == 0).sum())))
            assert not (ok[stage == 0] == 0).any()
        print(f"{code.name} {suf}: {got[0][0]} frames to stage 2, {got[0][1]} failures plain, {got[1][1]} at (13, 4, 0)")
        assert got[0][0] == got[1][0] == want[suf][0] and (got[0][1], got[1][1]) == want[suf][1:], (suf, got)


# ---- what fails without the feature ---------------------------------------------------------------------------------------------------
def test_header_declares_the_six_entry_points():
    text = open(os.path.join(ROOT, "include", "labrador_ldpc_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    tail = (r"float scale,\s*int lim,\s*uint32_t scale_num,\s*uint32_t scale_shift,\s*uint32_t offset,\s*"
            r"const struct labrador_ldpc_hip_opts \*opts\s*\)\s*;")
    head = r"\s*\(\s*enum labrador_ldpc_code code,\s*const float \*llrs,\s*"
    res = r"uint8_t \*output,\s*uint32_t \*iters,\s*uint8_t \*success,\s*"
    for suf, _ in TYPES:
        assert re.search(rf"int\s+labrador_ldpc_decode_ms_layered_quantised_batch_{suf}" + head + res + r"size_t batch,\s*size_t max_iters,\s*" + tail, src)
        assert re.search(rf"int\s+labrador_ldpc_decode_ms_layered_quantised_soft_batch_{suf}" + head + r"int32_t \*app,\s*" + res +
                         r"size_t batch,\s*size_t max_iters,\s*" + tail, src)
        assert re.search(rf"int\s+labrador_ldpc_decode_ms_cascade_quantised_batch_{suf}" + head + res +
                         r"uint8_t \*stage,\s*size_t batch,\s*size_t max_iters,\s*size_t max_sweeps,\s*" + tail, src)
    assert re.search(r"#define\s+LABRADOR_LDPC_HIP_ABI\s+3\b", text)                # additions only
    comment = text[text.index("f32 LLRs through the integer cascade"):text.index("int labrador_ldpc_decode_ms_cascade_quantised_batch_i8")]
    assert "ONCE PER CHUNK" in comment and "captured into a graph" in comment
    assert "LABRADOR_LDPC_HIP_QUANT_CHUNK" in comment and "LABRADOR_LDPC_HIP_CASCADE_CHUNK" in comment


def test_library_python_and_rust_hold_the_six_entry_points():
    dll = ctypes.CDLL(la.LIB_PATH)
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for name in HARD + SOFT + CASCADE:
        assert hasattr(dll, name) and name in la.SYMBOLS, name
        assert la.SYMBOLS[name][1][-6:-1] == [ctypes.c_float, ctypes.c_int] + [ctypes.c_uint32] * 3
        assert re.search(rf"pub fn {name}\s*\(code: LDPCCode, llrs: \*const f32, [^)]*scale: f32, lim: c_int, scale_num: u32, scale_shift: u32, "
                         r"offset: u32, opts: \*const HipOpts\) -> c_int;", rust), name
    assert len(la.SYMBOLS[HARD[0]][1]) == 13 and len(la.SYMBOLS[SOFT[0]][1]) == 14 and len(la.SYMBOLS[CASCADE[0]][1]) == 15
    assert la.lib.labrador_ldpc_hip_abi_version() == 3
    for method in ("decode_ms_layered_quantised_batch", "decode_ms_layered_quantised_soft_batch", "decode_ms_cascade_quantised_batch"):
        assert callable(getattr(LDPCCode.TC128, method))


def entries(code, suf):
    """(name, function, buffers to keep, their pointers, the arguments between the buffers and `scale`) of the three entries of a type"""
    y = np.ones((1, code.n()), np.float32)
    app = np.full((1, code.n() + code.punctured_bits()), -5, np.int32)
    out, it = np.full((1, code.output_len()), 0xEE, np.uint8), np.full(1, 77, np.uint32)
    ok, stage = np.full(1, 7, np.uint8), np.full(1, 9, np.uint8)
    for name, arrays, caps in ((f"labrador_ldpc_decode_ms_layered_quantised_batch_{suf}", (y, out, it, ok), (10,)),
                               (f"labrador_ldpc_decode_ms_layered_quantised_soft_batch_{suf}", (y, app, out, it, ok), (10,)),
                               (f"labrador_ldpc_decode_ms_cascade_quantised_batch_{suf}", (y, out, it, ok, stage), (10, 10))):
        yield name, getattr(la.lib, name), arrays, [x.ctypes.data for x in arrays], caps


def test_argument_checks_in_their_order():
    """The code; scale and lim -- before the empty batch --; the empty batch whatever the pointers; NULL buffers, `app` and `stage`
    among them; the triple's range -- behind the buffers --; for the layered entries the variant.  Exact status and text, all without a
    GPU, where a call that reached a device would say ENODEV; the buffers stay as they were."""
    code = LDPCCode.TC128
    for suf, dtype in TYPES:
        tmax = int(np.iinfo(dtype).max)
        for name, fn, arrays, p, caps in entries(code, suf):
            before = [a.copy() for a in arrays]
            nul = [None] * len(p)
            layered = "cascade" not in name
            for bad_code in (9, -1):                                                                     # the code comes first
                assert fn(bad_code, *nul, 1, *caps, float("nan"), -1, 0, 9, 0, None) == EINVAL and la.last_error() == f"code {bad_code} out of range"
            for scale, shown in ((float("nan"), "nan"), (float("inf"), "inf"), (0.0, "0"), (-2.0, "-2")):
                for batch, ptrs in ((0, p), (1, p), (1, nul)):                                           # ... before the empty batch
                    assert fn(int(code), *ptrs, batch, *caps, scale, tmax + 1, 0, 9, 0, None) == EINVAL  # and scale before lim
                    assert la.last_error() == f"scale {shown} is not in (0, FLT_MAX]", (name, la.last_error())
            for lim in (-1, tmax + 1):
                for batch, ptrs in ((0, p), (1, nul)):
                    assert fn(int(code), *ptrs, batch, *caps, 8.0, lim, 0, 9, 0, None) == EINVAL
                    assert la.last_error() == f"lim {lim} is not in 0 .. {tmax}", (name, la.last_error())
            # the empty batch: OK whatever the pointers, the triple and the variant
            opts = la.HipOpts(-1, la.MEM_DEVICE, None, 3, 0, None)
            assert fn(int(code), *nul, 0, *caps, 8.0, tmax, 0, 9, tmax + 1, ctypes.byref(opts)) == OK and la.last_error() == ""
            assert fn(int(code), *p, 0, *caps, 8.0, tmax, 13, 4, 0, None) == OK
            for i in range(len(p)):                                                                      # the buffers before the triple
                ptrs = list(p)
                ptrs[i] = None
                for memory in (la.MEM_HOST, la.MEM_DEVICE):
                    opts = la.HipOpts(-1, memory, None, 3, 0, None)
                    assert fn(int(code), *ptrs, 1, *caps, 8.0, tmax, 0, 9, tmax + 1, ctypes.byref(opts)) == EINVAL, (name, i)
                    assert la.last_error() == "NULL buffer", (name, i, la.last_error())
            for memory in (la.MEM_HOST, la.MEM_DEVICE):
                for variant in (0, 3):                                                                   # the triple before the variant
                    opts = la.HipOpts(-1, memory, None, variant, 0, None)
                    for triple, text in (((1, 9, 0), "scale_shift 9 is not in 0 .. 8"), ((0, 4, 0), "scale_num 0 is not in 1 .. 1 << scale_shift (16)"),
                                         ((17, 4, 0), "scale_num 17 is not in 1 .. 1 << scale_shift (16)"),
                                         ((13, 4, tmax + 1), f"offset {tmax + 1} is not in 0 .. {tmax}")):
                        assert fn(int(code), *p, 1, *caps, 8.0, tmax, *triple, ctypes.byref(opts)) == EINVAL, (name, triple)
                        assert la.last_error() == text, (name, la.last_error())
                if layered:
                    for variant in (1, 64, -1):
                        opts = la.HipOpts(-1, memory, None, variant, 0, None)
                        for triple in ((13, 4, 0), (16, 4, 0), (1, 0, tmax)):
                            assert fn(int(code), *p, 1, *caps, 8.0, tmax, *triple, ctypes.byref(opts)) == EUNSUPPORTED, (name, variant, triple)
                            assert la.last_error() == f"kernel variant {variant} not built for the layered schedule (only 0 is)"
            for a, b in zip(arrays, before):
                assert (a == b).all(), name


def test_python_methods_refuse_what_they_document():
    """Wrong shape or dtype is ValueError, an unknown `dtype` KeyError, like the neighbours; what ctypes would wrap is refused; the
    ranges are the library's to refuse."""
    code = LDPCCode.TC128
    good = np.ones((2, code.n()), np.float32)
    for method in (code.decode_ms_layered_quantised_batch, code.decode_ms_layered_quantised_soft_batch, code.decode_ms_cascade_quantised_batch):
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
        with pytest.raises(la.LdpcHipError, match="scale_shift 9 is not in"):
            method(good, "i8", scale_shift=9)
        with pytest.raises(la.LdpcHipError, match="offset 128 is not in 0 .. 127"):
            method(good, "i8", offset=128)
        with pytest.raises(TypeError):
            method(good, "i8", lim=3.5)
        with pytest.raises(TypeError):
            method(good, "i8", offset=0.5)
        with pytest.raises(ValueError):
            method(good, "i8", scale_num=-1)
        with pytest.raises(ValueError, match="output"):
            method(good, output=np.zeros((2, code.output_len() + 1), np.uint8))
        with pytest.raises(ValueError, match="success"):
            method(good, success=np.zeros(3, np.uint8))
    for method in (code.decode_ms_layered_quantised_batch, code.decode_ms_layered_quantised_soft_batch):
        with pytest.raises(la.LdpcHipError, match="only 0 is"):
            method(good, "i8", variant=1)
    with pytest.raises(ValueError, match="app"):
        code.decode_ms_layered_quantised_soft_batch(good, app=np.zeros((2, code.n() + code.punctured_bits()), np.float32))
    with pytest.raises(ValueError, match="stage"):
        code.decode_ms_cascade_quantised_batch(good, stage=np.zeros(3, np.uint8))


class _SpyLib:
    """Stands where the package keeps its library: an f32-input decode looked up through it is recorded with its arguments and reports
    success without doing anything; every other symbol is the library's own."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        if "_quantised_" not in name:
            return getattr(self.real, name)

        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


def test_python_methods_pass_their_arguments(monkeypatch):
    """dtype chooses the entry; lim=None is the type's maximum; no triple is the identity (1, 0, 0); the caps, the quantiser's pair,
    the triple and the variant reach the entry as given; the results come back in the entries' order."""
    code = LDPCCode.TC128
    spy = _SpyLib(la.lib)
    monkeypatch.setattr(la, "lib", spy)
    y = np.ones((3, code.n()), np.float32)
    for kw, i, tail in ((dict(), 0, (8.0, 127, 1, 0, 0)), (dict(dtype="i16"), 1, (8.0, 32767, 1, 0, 0)),
                        (dict(dtype="i16", scale=64, lim=2047, scale_num=13, scale_shift=4), 1, (64.0, 2047, 13, 4, 0)),
                        (dict(lim=31, scale_shift=4, offset=1), 0, (8.0, 31, 16, 4, 1))):
        for method, names, nbuf, caps in ((code.decode_ms_layered_quantised_batch, HARD, 4, (3, 25)),
                                          (code.decode_ms_layered_quantised_soft_batch, SOFT, 5, (3, 25)),
                                          (code.decode_ms_cascade_quantised_batch, CASCADE, 5, (3, 25, 25))):
            del spy.calls[:]
            res = method(y, maxiters=25, **kw)
            (got, args), = spy.calls
            assert got == names[i] and args[1 + nbuf:-1] == caps + tail, (kw, got, args)
            assert len(res) == nbuf - 1
    del spy.calls[:]
    res = code.decode_ms_cascade_quantised_batch(y, "i8", 8.0, 31, 10, max_sweeps=7, variant=64)
    (got, args), = spy.calls
    assert args[6:9] == (3, 10, 7) and ctypes.cast(args[-1], ctypes.POINTER(la.HipOpts)).contents.variant == 64
    assert res[3].shape == (3,) and res[3].dtype == np.uint8
    app = code.decode_ms_layered_quantised_soft_batch(y, "i16")[0]
    assert app.dtype == np.int32 and app.shape == (3, code.n() + code.punctured_bits())


def test_the_ber_harness_checks_from_f32():
    """--from-f32 / from_f32=True belongs to the quantised LLRs of the layered schedule and the cascade: decided before any device
    work."""
    from labrador_ldpc_amd import perftest
    code = LDPCCode.TC128
    for bad in (dict(llr="f32", schedule="layered"), dict(llr="f32", schedule="cascade"), dict(llr="f32"), dict(llr="i8", schedule="flooding")):
        with pytest.raises(ValueError):
            perftest.ms_trials(code, 3.0, "ebn0", from_f32=True, **bad)
    for bad in (["--llr", "f32", "--schedule", "layered"], ["--schedule", "flooding"], ["--llr", "f32", "--schedule", "cascade"],
                ["--llr", "i8", "--schedule", "flooding"]):
        with pytest.raises(SystemExit) as e:
            perftest.main(["--code", "TC128", "--snrs", "3.0", "--from-f32"] + bad)
        assert e.value.code == 2, bad


# ---- the shape of the kernels ---------------------------------------------------------------------------------------------------------
def waves_per_simd(vgprs):
    """512 registers per lane of a SIMD, allocated in eights, at most 8 waves"""
    return min(8, 512 // ((vgprs + 7) // 8 * 8))


def test_quantised_kernels_keep_the_shape_of_their_integer_counterparts(capsys):
    """decode_ms_fixed_quantised.o holds 72 kernels: nine codes x {i8, i16} x {hard, soft} x {plain, corrected}.  Each against the
    kernel of the same code, type and form in decode_ms_fixed_layered.o (plain) or decode_ms_fixed_corrected.o: the LDS is the same
    to the byte (the geometry is the same type), scratch is not above it, and the waves per SIMD that the VGPR count allows are not
    below it.  The raw figures are printed."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    layered_helpers.built_object("decode_ms_fixed_quantised.o")

    def table(obj, pattern):
        out = {}
        for _, name, vgpr, spill, _, lds, scratch in kernel_resources.resources("build/csrc/" + obj):
            m = re.search(pattern, name)
            assert m, name
            out[m.group(1)] = (int(vgpr), int(spill), int(lds), int(scratch))
        return out
    plain = table("decode_ms_fixed_layered.o", r"decode_ms_layered_fixed_kernel<(.*?)>")
    corrected = table("decode_ms_fixed_corrected.o", r"decode_ms_layered_fixed_corrected_kernel<(.*?)>")
    new = table("decode_ms_fixed_quantised.o", r"decode_ms_layered_fixed_quantised_kernel<(.*?)>")
    assert len(plain) == len(corrected) == 36 and len(new) == 72
    lines = []
    for key, (vgpr, spill, lds, scratch) in sorted(new.items()):
        base, form = key.rsplit(", ", 1)
        assert form in ("true", "false")
        r_vgpr, r_spill, r_lds, r_scratch = (corrected if form == "true" else plain)[base]
        lines.append(f"<{key}>: {vgpr} VGPRs ({r_vgpr}), {spill} spilled ({r_spill}), {lds} B LDS ({r_lds}), {scratch} B scratch ({r_scratch})")
        assert lds == r_lds, lines[-1]
        assert scratch <= r_scratch, lines[-1]
        assert waves_per_simd(vgpr) >= waves_per_simd(r_vgpr), lines[-1]
    with capsys.disabled():
        print("\nf32-source kernel (its integer-source counterpart):\n" + "\n".join(lines))


def test_the_loader_quantises_with_one_unfused_multiply():
    """Every kernel of the new object multiplies and rounds (v_mul_f32, v_rndne_f32) and holds no fused multiply-add: the rule is one
    f32 product."""
    obj = layered_helpers.built_object("decode_ms_fixed_quantised.o")
    kernels = layered_helpers.kernels(obj, "decode_ms_layered_fixed_quantised_kernel")
    assert len(kernels) == 72
    for name, body in kernels.items():
        ops = [t.split()[0] for _, t, _ in body]
        assert any(o.startswith("v_mul_f32") for o in ops) and any(o.startswith("v_rndne_f32") for o in ops), name
        assert not any("fma" in o or "mac" in o for o in ops), name
