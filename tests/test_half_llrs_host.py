"""f16 / bf16 LLRs to the f32 decoders without a GPU: the header, the library, the Python table and the Rust shim
hold the 16 entry points; the host loop of labrador_ldpc_widen_llrs_batch_{f16,bf16} equals the rule on all 65 536 bit patterns; the
argument checks answer before any device work, as the f32 entry of the same name does; the Python methods choose the entry from the
dtype, return float32 marginals and keep refusing halves where they did; the new kernels have the shape the design states."""
import ctypes
import os
import re

import numpy as np
import pytest

import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode
import layered_helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, EUNSUPPORTED = 0, -1, -4
HALVES = ("f16", "bf16")
_OUT = r"uint8_t \*output,\s*uint32_t \*iters,\s*uint8_t \*success,\s*"
_CAPS = r"size_t batch,\s*size_t max_iters,\s*"
_CORR = r"float scale,\s*float offset,\s*"
# entry (without its suffix) -> what stands between `llrs` and `opts` in its declaration
ENTRIES = {
    "labrador_ldpc_widen_llrs_batch_": r"float \*out,\s*size_t batch,\s*",
    "labrador_ldpc_decode_ms_batch_": _OUT + _CAPS,
    "labrador_ldpc_decode_ms_soft_batch_": r"float \*app,\s*" + _OUT + _CAPS,
    "labrador_ldpc_decode_ms_layered_batch_": _OUT + _CAPS,
    "labrador_ldpc_decode_ms_layered_soft_batch_": r"float \*app,\s*" + _OUT + _CAPS,
    "labrador_ldpc_decode_ms_layered_corrected_batch_": _OUT + _CAPS + _CORR,
    "labrador_ldpc_decode_ms_layered_corrected_soft_batch_": r"float \*app,\s*" + _OUT + _CAPS + _CORR,
    "labrador_ldpc_decode_ms_cascade_batch_": _OUT + r"uint8_t \*stage,\s*" + _CAPS + r"size_t max_sweeps,\s*" + _CORR,
}
NAMES = [e + h for e in ENTRIES for h in HALVES]


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "labrador_ldpc_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert len(NAMES) == 16
    for entry, middle in ENTRIES.items():
        for h in HALVES:
            pat = (r"int " + entry + h + r"\s*\(\s*enum labrador_ldpc_code code,\s*const uint16_t \*llrs,\s*" + middle +
                   r"const struct labrador_ldpc_hip_opts \*opts\);")
            assert re.search(pat, src), entry + h
    assert re.search(r"#define LABRADOR_LDPC_HIP_ABI 3\b", text)               # symbols are only added


def test_library_python_and_rust_hold_the_entry_points():
    dll = ctypes.CDLL(la.LIB_PATH)
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for name in NAMES:
        assert getattr(dll, name) is not None
        assert name in la.SYMBOLS and la.SYMBOLS[name][0] is ctypes.c_int, name
        assert re.search(r"pub fn " + name + r"\(code: LDPCCode, llrs: \*const u16, ", rust), name


# ---- the rule, exhaustively, through the host loop ------------------------------------------------------------------------------------
def all_patterns():
    """all 65 536 bit patterns as 512 TC128 frames"""
    return np.arange(65536, dtype=np.uint16).reshape(512, LDPCCode.TC128.n())


def f16_rule(bits):
    """the statement of the f16 rule: numpy's exact widening, a NaN made quiet"""
    x = bits.view(np.float16)
    w = x.astype(np.float32).view(np.uint32).copy()
    w[np.isnan(x)] |= 0x00400000
    return w


def bf16_rule(bits):
    return bits.astype(np.uint32) << 16


def host_widen(suffix, bits):
    out = np.full(bits.shape, np.float32(-7.5), np.float32)
    fn = getattr(la.lib, "labrador_ldpc_widen_llrs_batch_" + suffix)
    assert fn(int(LDPCCode.TC128), bits.ctypes.data, out.ctypes.data, len(bits), None) == OK, la.last_error()
    return out.view(np.uint32)


def test_f16_rule_on_every_bit_pattern():
    bits = all_patterns()
    got, want = host_widen("f16", bits), f16_rule(bits)
    bad = np.argwhere(got != want)
    assert bad.size == 0, [(hex(bits[tuple(i)]), hex(got[tuple(i)]), hex(want[tuple(i)])) for i in bad[:8]]
    # what the rule says in words, on the statement itself
    flat, w = bits.reshape(-1), want.reshape(-1)
    assert w[0x0000] == 0x00000000 and w[0x8000] == 0x80000000                               # +-0
    assert w[0x7C00] == 0x7F800000 and w[0xFC00] == 0xFF800000                               # +-inf
    assert w[0x0001] == np.float32(2.0 ** -24).view(np.uint32)                               # the smallest subnormal, an f32 normal
    assert w[0x7BFF] == np.float32(65504).view(np.uint32) and w[0xFBFF] == np.float32(-65504).view(np.uint32)
    nan = (flat & 0x7C00 == 0x7C00) & (flat & 0x03FF != 0)
    assert nan.sum() == 2046
    assert (w[nan] == ((flat[nan].astype(np.uint32) & 0x8000) << 16 | 0x7FC00000 | (flat[nan].astype(np.uint32) & 0x03FF) << 13)).all()
    # the Python method says the same from a float16 array
    assert (LDPCCode.TC128.widen_llrs_batch(bits.view(np.float16)).view(np.uint32) == want).all()


def test_bf16_rule_on_every_bit_pattern():
    bits = all_patterns()
    got, want = host_widen("bf16", bits), bf16_rule(bits)
    bad = np.argwhere(got != want)
    assert bad.size == 0, [(hex(bits[tuple(i)]), hex(got[tuple(i)]), hex(want[tuple(i)])) for i in bad[:8]]


# ---- argument checks, in their order, without a device --------------------------------------------------------------------------------
def buffers(code, dtype):
    llrs = np.ones((1, code.n()), dtype)
    app = np.full((1, code.n() + code.punctured_bits()), -3.0, np.float32)
    out, it = np.full((1, code.output_len()), 0xEE, np.uint8), np.full(1, 77, np.uint32)
    ok, stage = np.full(1, 7, np.uint8), np.full(1, 9, np.uint8)
    return dict(llrs=llrs, app=app, output=out, iters=it, success=ok, stage=stage)


def entry_shape(entry):
    """(names of the pointers behind `code`, has max_sweeps, has the correction) of an entry"""
    ptrs = ["llrs"] + (["app"] if "soft" in entry else []) + ["output", "iters", "success"] + (["stage"] if "cascade" in entry else [])
    return ptrs, "cascade" in entry, "corrected" in entry or "cascade" in entry


def call(fn, ptrs, batch, sweeps, corr, pair, opts):
    tail = (batch, 10) + ((10,) if sweeps else ()) + (pair if corr else ())
    s = fn(*ptrs, *tail, None if opts is None else ctypes.byref(opts))
    return s, la.last_error()


@pytest.mark.parametrize("entry", [e for e in ENTRIES if "decode" in e], ids=lambda e: e[len("labrador_ldpc_decode_ms_"):-1])
def test_decoder_argument_checks_are_the_f32_entry_s(entry):
    """For the same arguments the _f16 and _bf16 entries answer what the _f32 entry of the same name answers, status and text: a bad
    code; for the corrected and cascade entries the correction's range, before the empty batch; the empty batch whatever the pointers;
    NULL buffers.  All without a GPU, where a call that reached a device would say so."""
    code = LDPCCode.TC128
    names, sweeps, corr = entry_shape(entry)
    f32 = getattr(la.lib, entry + "f32")
    ref = buffers(code, np.float32)
    p32 = [ref[k].ctypes.data for k in names]
    for h in HALVES:
        fn = getattr(la.lib, entry + h)
        mine = buffers(code, np.uint16)
        p = [mine[k].ctypes.data for k in names]

        def both(code_, ptrs32, ptrs, batch, pair=(1.0, 0.0), opts=None):
            want = call(f32, [code_] + ptrs32, batch, sweeps, corr, pair, opts)
            got = call(fn, [code_] + ptrs, batch, sweeps, corr, pair, opts)
            assert got == want, (entry + h, got, want)
            return got

        assert both(9, p32, p, 1)[0] == EINVAL and "out of range" in la.last_error()
        assert both(-1, p32, p, 1, (2.0, 0.0))[0] == EINVAL and "out of range" in la.last_error()       # the code comes first
        if corr:
            for pair in ((0.0, 0.0), (1.5, 0.0), (float("nan"), 0.0), (1.0, -0.1), (1.0, float("inf"))):
                for batch in (0, 1):                                                                    # ... before the empty batch
                    s, text = both(int(code), p32, p, batch, pair)
                    assert s == EINVAL and "is not in" in text, (pair, batch, text)
                assert both(int(code), [None] * len(p), [None] * len(p), 1, pair)[0] == EINVAL and "is not in" in la.last_error()
        assert both(int(code), p32, p, 0, (0.8125, 0.0))[0] == OK
        assert both(int(code), [None] * len(p), [None] * len(p), 0, (1.0, 0.1))[0] == OK
        for i in range(len(p)):
            q32, q = list(p32), list(p)
            q32[i] = q[i] = None
            for memory in (la.MEM_HOST, la.MEM_DEVICE):
                s, text = both(int(code), q32, q, 1, opts=la.HipOpts(-1, memory, None, 0, 0, None))
                assert s == EINVAL and "NULL" in text, (names[i], text)
        for k, v in buffers(code, np.uint16).items():
            assert (mine[k] == v).all(), k                                                              # nothing was written


@pytest.mark.parametrize("entry", [e for e in ENTRIES if "layered" in e], ids=lambda e: e[len("labrador_ldpc_decode_ms_"):-1])
def test_layered_entries_have_variant_zero_only(entry):
    """opts->variant != 0 is EUNSUPPORTED with the f32 entries' text, and it is said with the arguments: after the buffers, before any
    device work.  (The f32 entries leave it to their launchers, so on a machine without a GPU they fail earlier, for the missing
    device; where they get as far, the status and the text are the same.)"""
    code = LDPCCode.TC128
    names, sweeps, corr = entry_shape(entry)
    ref = buffers(code, np.float32)
    want_f32 = call(getattr(la.lib, entry + "f32"), [int(code)] + [ref[k].ctypes.data for k in names], 1, sweeps, corr, (1.0, 0.0),
                    la.HipOpts(-1, la.MEM_HOST, None, 3, 0, None))
    for h in HALVES:
        mine = buffers(code, np.uint16)
        p = [mine[k].ctypes.data for k in names]
        for memory in (la.MEM_HOST, la.MEM_DEVICE):
            got = call(getattr(la.lib, entry + h), [int(code)] + p, 1, sweeps, corr, (1.0, 0.0), la.HipOpts(-1, memory, None, 3, 0, None))
            assert got == (EUNSUPPORTED, "kernel variant 3 not built for the layered schedule (only 0 is)"), got
            if want_f32[0] == EUNSUPPORTED:
                assert got == want_f32
        q = list(p)
        q[0] = None                                                                                     # the buffers come first
        s, text = call(getattr(la.lib, entry + h), [int(code)] + q, 1, sweeps, corr, (1.0, 0.0), la.HipOpts(-1, la.MEM_HOST, None, 3, 0, None))
        assert s == EINVAL and "NULL" in text


def test_widen_argument_checks():
    """The code; the empty batch whatever the pointers; NULL buffers; opts->memory; with MEM_DEVICE the two alignments, before the
    device is selected."""
    code = LDPCCode.TC128
    for h in HALVES:
        fn = getattr(la.lib, "labrador_ldpc_widen_llrs_batch_" + h)
        bits, out = np.zeros((1, code.n()), np.uint16), np.full((1, code.n()), -7.5, np.float32)
        assert fn(9, bits.ctypes.data, out.ctypes.data, 1, None) == EINVAL and "out of range" in la.last_error()
        assert fn(int(code), None, None, 0, None) == OK
        assert fn(int(code), None, out.ctypes.data, 1, None) == EINVAL and "NULL" in la.last_error()
        assert fn(int(code), bits.ctypes.data, None, 1, None) == EINVAL and "NULL" in la.last_error()
        opts = la.HipOpts(-1, 5, None, 0, 0, None)
        assert fn(int(code), bits.ctypes.data, out.ctypes.data, 1, ctypes.byref(opts)) == EINVAL and "opts->memory" in la.last_error()
        opts = la.HipOpts(-1, la.MEM_DEVICE, None, 0, 0, None)
        assert fn(int(code), 0x1002, 0x2000, 1, ctypes.byref(opts)) == EINVAL
        assert la.last_error() == "device llrs buffer must be 16-byte aligned"
        assert fn(int(code), 0x1000, 0x2004, 1, ctypes.byref(opts)) == EINVAL
        assert la.last_error() == "device out buffer must be 16-byte aligned"
        assert (out == np.float32(-7.5)).all()


# ---- Python ------------------------------------------------------------------------------------------------------------------------------
class _SpyLib:
    """Stands where the package keeps its library: a call of a half-precision entry looked up through it is recorded with its
    arguments and reports success without doing anything; every other symbol is the library's own."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        if not name.endswith(("_f16", "_bf16")):
            return getattr(self.real, name)

        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


def test_python_methods_choose_the_entry_from_the_dtype(monkeypatch):
    code = LDPCCode.TC128
    spy = _SpyLib(la.lib)
    monkeypatch.setattr(la, "lib", spy)
    y = np.ones((3, code.n()), np.float16)
    npn = code.n() + code.punctured_bits()
    P = "labrador_ldpc_decode_ms_"
    for method, kw, name, tail, soft, extra in (
            (code.decode_ms_batch, dict(variant=2), P + "batch_f16", (3, 25), False, 0),
            (code.decode_ms_soft_batch, dict(), P + "soft_batch_f16", (3, 25), True, 0),
            (code.decode_ms_layered_batch, dict(), P + "layered_batch_f16", (3, 25), False, 0),
            (code.decode_ms_layered_batch, dict(scale=0.8125), P + "layered_corrected_batch_f16", (3, 25, 0.8125, 0.0), False, 0),
            (code.decode_ms_layered_soft_batch, dict(), P + "layered_soft_batch_f16", (3, 25), True, 0),
            (code.decode_ms_layered_soft_batch, dict(offset=0.1), P + "layered_corrected_soft_batch_f16", (3, 25, 1.0, 0.1), True, 0),
            (code.decode_ms_cascade_batch, dict(max_sweeps=7, scale=0.75), P + "cascade_batch_f16", (3, 25, 7, 0.75, 0.0), False, 1)):
        del spy.calls[:]
        res = method(y, 25, **kw)
        (got, args), = spy.calls
        first = 2 + soft + 3 + extra
        assert got == name and args[0] == int(code) and args[first:-1] == tail, (name, got, args)
        assert ctypes.cast(args[-1], ctypes.POINTER(la.HipOpts)).contents.variant == kw.get("variant", 0)
        assert len(res) == 3 + soft + extra
        if soft:
            assert res[0].dtype == np.float32 and res[0].shape == (3, npn) and args[2] == res[0].ctypes.data      # `app` is float32
        out, it, ok = res[soft:soft + 3]
        assert out.shape == (3, code.output_len()) and it.dtype == np.uint32 and ok.dtype == np.uint8
    # a float16 `app` of the caller's is not what the entry writes
    with pytest.raises(ValueError, match="app"):
        code.decode_ms_soft_batch(y, 25, app=np.zeros((3, npn), np.float16))
    mine = np.zeros((3, npn), np.float32)
    assert code.decode_ms_soft_batch(y, 25, app=mine)[0] is mine
    del spy.calls[:]
    out = code.widen_llrs_batch(y)
    (got, args), = spy.calls
    assert got == "labrador_ldpc_widen_llrs_batch_f16" and out.dtype == np.float32 and out.shape == y.shape and args[3] == 3


def test_python_keeps_refusing_halves_where_it_did():
    """np.uint16 is no LLR type anywhere, and the methods outside the f32 decoders' batched calls refuse float16 with the error they
    raised before."""
    code = LDPCCode.TC128
    f16, u16 = np.ones((2, code.n()), np.float16), np.ones((2, code.n()), np.uint16)
    for method in (code.decode_ms_batch, code.decode_ms_soft_batch, code.decode_ms_layered_batch, code.decode_ms_layered_soft_batch,
                   code.decode_ms_cascade_batch):
        with pytest.raises(la.LdpcHipError, match="no batched kernel for dtype uint16"):
            method(u16, 10)
    for method in (code.decode_ms_layered_fixed_batch, code.decode_ms_layered_fixed_soft_batch, code.decode_ms_cascade_fixed_batch):
        with pytest.raises(la.LdpcHipError, match="no batched kernel for dtype float16"):
            method(f16, 10)
    for method in (code.quantise_llrs_batch, code.decode_ms_quantised_batch, code.decode_ms_layered_quantised_batch,
                   code.decode_ms_layered_quantised_soft_batch, code.decode_ms_cascade_quantised_batch):
        with pytest.raises(ValueError, match="llrs must be float32"):
            method(f16)
    with pytest.raises(ValueError, match="llrs must be a numpy array of dtype"):
        code.decode_ms(f16[0], np.zeros(code.output_len(), np.uint8))
    with pytest.raises(ValueError, match="dtype must be one of"):
        code.llrs_to_hard_batch(f16)
    with pytest.raises(KeyError):
        code.llrs_to_hard(f16[0], np.zeros(code.n() // 8, np.uint8))
    for dtype in ("f16", "bf16"):
        with pytest.raises(KeyError):
            code.hard_to_llrs_batch(np.zeros((2, code.n() // 8), np.uint8), dtype)
    with pytest.raises(KeyError):
        code.hard_to_llrs(np.zeros(code.n() // 8, np.uint8), f16[0])
    with pytest.raises(ValueError, match="float16 or bfloat16"):
        code.widen_llrs_batch(u16)
    with pytest.raises(ValueError, match="float16 or bfloat16"):
        code.widen_llrs_batch(np.ones((2, code.n()), np.float32))
    assert np.dtype(np.float16) not in la._NP_SUFFIX and np.dtype(np.uint16) not in la._NP_HALF_SUFFIX


def test_the_ber_harness_knows_the_half_formats():
    """--llr f16 / bf16 go with the three schedules of the f32 branch; the integer branch's options are refused with them: decided
    before any device work."""
    from labrador_ldpc_amd import perftest
    code = LDPCCode.TC128
    for llr in HALVES:
        for bad in (dict(llr=llr, scale_num=13, scale_shift=4), dict(llr=llr, schedule="nonsense"),
                    dict(llr=llr, schedule="flooding", scale=0.8), dict(llr=llr, max_sweeps=5)):
            with pytest.raises(ValueError) as e:
                perftest.ms_trials(code, 3.0, "ebn0", **bad)
            assert "unknown LLR type" not in str(e.value), bad                                          # (the format itself is known)
        for bad in (["--llr", llr, "--fixed-scale", "13/16"], ["--llr", llr, "--max-sweeps", "5"]):
            with pytest.raises(SystemExit) as e:
                perftest.main(["--code", "TC128", "--snrs", "3.0"] + bad)
            assert e.value.code == 2, bad
    assert perftest.FLOAT_LLRS == ("f32", "f16", "bf16")
    with pytest.raises(SystemExit) as e:
        perftest.main(["--code", "TC128", "--snrs", "3.0", "--llr", "f8"])
    assert e.value.code == 2


# ---- the shape of the kernels ---------------------------------------------------------------------------------------------------------
def test_widen_kernels_stream():
    """llr_widen.o holds widen_kernel for the two formats, nothing else; neither touches scratch or LDS; every load of LLRs is 16
    bytes per lane and non-temporal; a lane stores the 32 bytes its octet became as two plain 16-byte stores; f16 converts, bf16
    shifts."""
    import kernel_resources                                  # (tools/ is on the path: layered_helpers put it there)
    obj = layered_helpers.built_object("llr_widen.o")
    kernels = layered_helpers.kernels(obj, "widen_kernel")
    assert len(kernels) == 2 and len(layered_helpers.kernels(obj, "")) == 2, sorted(kernels)
    assert sorted("bf16_llr" in k for k in kernels) == [False, True]
    for name, body in kernels.items():
        lines = [t for _, t, _ in body]
        ops = [t.split()[0] for t in lines]
        assert not any(x.startswith(("scratch_", "ds_", "buffer_", "flat_")) or "atomic" in x for x in ops), name
        loads = [t for t in lines if t.split()[0].startswith("global_load")]
        stores = [t for t in lines if t.split()[0].startswith("global_store")]
        assert len(loads) == 4 and all(t.split()[0] == "global_load_dwordx4" and t.split()[-1] == "nt" for t in loads), (name, loads)
        assert len(stores) == 8 and all(t.split()[0] == "global_store_dwordx4" and t.split()[-1] != "nt" for t in stores), (name, stores)
        assert (sum(x.startswith("v_cvt_f32_f16") for x in ops) == 32) == ("bf16_llr" not in name), name
    res = kernel_resources.resources(obj)
    assert len(res) == 2
    for _, name, vgpr, spill, _, lds, scratch in res:
        assert int(spill) == 0 and int(lds) == 0 and int(scratch) == 0 and int(vgpr) <= 64, (name, vgpr, spill, lds, scratch)


KERNEL = "decode_ms_half_layered_kernel"


def test_half_layered_kernels_keep_the_shape_of_the_corrected_f32_kernels(capsys):
    """decode_ms_half_layered.o holds 36 kernels: nine codes x {f16, bf16} x {hard, soft}, under a name the counts of the layered
    objects do not match.  Each against the kernel of the same code and form in decode_ms_corrected_f32.o: the LDS is the same to the
    byte.  No scratch instruction in a backward-branch span with a sweep's 8 barriers, none at all in the one-wave kernels (the TC
    codes).  The raw figures are printed."""
    import kernel_resources                                  # (tools/ is on the path: layered_helpers put it there)
    obj = layered_helpers.built_object("decode_ms_half_layered.o")
    kernels = layered_helpers.kernels(obj, KERNEL)
    assert len(kernels) == 36 and len(layered_helpers.kernels(obj, "")) == 36
    assert not any("decode_ms_layered_kernel" in k or "decode_ms_corrected_kernel" in k for k in kernels)
    assert sum("bf16_llr" in k for k in kernels) == 18 and sum("_7f16_llr" in k for k in kernels) == 18
    sweeps = 0
    for name, body in kernels.items():
        code = int(re.search(r"kernelILi(\d+)E", name).group(1))
        if code <= 2:
            assert not any(t.startswith("scratch_") for _, t, _ in body), name
            continue
        base, index = body[0][0], {b[0]: i for i, b in enumerate(body)}
        for i, (addr, text, tgt) in enumerate(body):
            if text.startswith(("s_cbranch", "s_branch")) and tgt is not None and base + tgt < addr and (base + tgt) in index:
                span = [t for _, t, _ in body[index[base + tgt]:i + 1]]
                if sum(t.startswith("s_barrier") for t in span) == 8:
                    sweeps += 1
                    assert not any(t.startswith("scratch_") for t in span), f"{name}: scratch inside the sweep loop"
    assert sweeps >= 24

    def table(o, pattern):
        out = {}
        for _, name, vgpr, spill, _, lds, scratch in kernel_resources.resources(os.path.join(ROOT, "build", "csrc", o)):
            m = re.search(pattern, name)
            assert m, name
            out[tuple(x.strip() for x in m.group(1).split(","))] = (int(vgpr), int(spill), int(lds), int(scratch))
        return out
    ref = table("decode_ms_corrected_f32.o", r"decode_ms_corrected_kernel<(.*?)>")
    new = table("decode_ms_half_layered.o", KERNEL + r"<(.*?)>")
    assert len(ref) == 18 and len(new) == 36
    lines = []
    for (code, fmt, soft), (vgpr, spill, lds, scratch) in sorted(new.items()):
        r_vgpr, r_spill, r_lds, r_scratch = ref[code, soft]
        lines.append(f"<{code}, {fmt}, {soft}>: {vgpr} VGPRs ({r_vgpr}), {spill} spilled ({r_spill}), {lds} B LDS ({r_lds}), "
                     f"{scratch} B scratch ({r_scratch})")
        assert lds == r_lds, lines[-1]
    with capsys.disabled():
        print("\nhalf-source kernel (its f32-source counterpart):\n" + "\n".join(lines))
