"""CPU-side checks of normalized / offset min-sum on the fixed-point layered schedule
(labrador_ldpc_decode_ms_layered_fixed_corrected_{,soft_}batch_{i8,i16}): the two statements of
tests/layered_fixed_corrected_restatement.py agree, (1 << k, k, 0) is the plain fixed-point restatement bit for bit, a power-of-two
scale with an integer offset is the f32 corrected restatement of DESIGN.md 4.6 on the same integers wherever nothing clamps, the failure
counts of the issue's table reproduce, the header declares and the library, the Python table and the Rust shim hold the four entry
points, their argument checks (the three parameters included) answer before any device work, the corrected kernels keep the shape of
the plain fixed ones, and the Python keywords and the BER harness route and refuse as documented.  No compute call needs a GPU."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode
import layered_corrected_restatement as lcr
import layered_fixed_corrected_restatement as fcr
import layered_fixed_restatement as fr
import layered_helpers
from layered_helpers import quantise
import layered_restatement as lr
import oracle
from test_layered_fixed_host import corner_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, OK, EUNSUPPORTED = -1, 0, -4
TYPES = (np.int8, np.int16)
NAMES = [f"labrador_ldpc_decode_ms_layered_fixed_corrected_{soft}batch_{t}" for soft in ("", "soft_") for t in ("i8", "i16")]


def triples(dtype):
    tmax = int(np.iinfo(dtype).max)
    return ((1, 0, 0), (16, 4, 0), (13, 4, 0), (1, 8, 0), (256, 8, 0), (1, 0, 1), (1, 0, tmax), (13, 4, 1))


def test_the_step_rounds_half_up_and_never_grows_a_magnitude():
    """The step itself on every magnitude of i8 and a spread of i16's: half up (13 / 16 of 2 is 1.625 -> 2, 1 / 2 of 1 is 0.5 -> 1, 1 / 256
    of 127 is 0.496 -> 0), m' <= m, the identity at (1 << k, k, 0), zero at an offset of T_MAX."""
    assert fcr.correct([0, 1, 2, 3, 8], 13, 4, 0).tolist() == [0, 1, 2, 2, 7]
    assert fcr.correct([1, 3], 1, 1, 0).tolist() == [1, 2] and fcr.correct([127, 128], 1, 8, 0).tolist() == [0, 1]
    assert fcr.correct([0, 1, 2, 31], 16, 4, 1).tolist() == [0, 0, 1, 30]
    for tmax in (127, 32767):
        m = np.unique(np.concatenate([np.arange(0, 300), np.arange(tmax - 300, tmax + 1)]).clip(0, tmax))
        for k in range(9):
            assert (fcr.correct(m, 1 << k, k, 0) == m).all()
            for num in {1, (1 << k) // 2 or 1, (13 << k) >> 4 or 1, 1 << k}:
                for offset in (0, 1, tmax):
                    c = fcr.correct(m, num, k, offset)
                    assert (c <= m).all() and (c >= 0).all()
                    exact = np.floor(num * m.astype(np.float64) / (1 << k) + 0.5) - offset
                    assert (c == np.maximum(exact, 0)).all()
        assert not fcr.correct(m, 1, 0, tmax).any()


@pytest.mark.parametrize("dtype", TYPES, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("code", [LDPCCode.TC128, LDPCCode.TM1280], ids=lambda c: c.name)
def test_whole_array_and_loop_statements_agree(code, dtype):
    """output, iters, success, app and the clamp flag, at caps 0, 1, 3 and 25 (TM1280: 25 on the first five frames only, as in
    test_layered_fixed_host.py -- the loop form is slow), on all the corner frames of test_layered_fixed_host.py, at every triple."""
    llrs = corner_frames(code, dtype, np.random.default_rng(7))
    st = fr.Structure(int(code))
    saw_clamp = False
    for triple in triples(dtype):
        for m in (0, 1, 3, 25):
            F = len(llrs) if (code == LDPCCode.TC128 or m < 25) else 5
            out, it, ok, app, cl = fcr.decode_fixed_corrected(st, llrs[:F], m, *triple)
            assert app.dtype == np.int32
            for f in range(F):
                o, i, s, a, c = fcr.decode_fixed_corrected_loop(code, llrs[f], m, *triple)
                assert (o == out[f]).all() and i == it[f] and s == ok[f] and (a == app[f]).all() and c == cl[f], (triple, m, f)
            saw_clamp |= bool(cl.any())
            if m == 0:
                assert not out.any() and not it.any() and not ok.any() and not app.any()
    assert saw_clamp
    # an offset of T_MAX leaves the LLRs: every message is zero
    tmax = int(np.iinfo(dtype).max)
    _, _, _, app, cl = fcr.decode_fixed_corrected(st, llrs, 3, 1, 0, tmax)
    assert (app[:, :code.n()] == np.maximum(llrs.astype(np.int32), -tmax)).all() and not app[:, code.n():].any() and not cl.any()


@pytest.mark.parametrize("code", list(LDPCCode), ids=lambda c: c.name)
def test_a_unit_scale_and_no_offset_are_the_plain_fixed_schedule(code):
    """(1 << k, k, 0) for k = 0, 4, 8: output, iters, success, app and the clamp flag equal layered_fixed_restatement.decode_fixed
    bit for bit -- both types, caps 1, 3 and 25, AWGN frames at 8 / 31 and corner frames."""
    st = fr.Structure(int(code))
    for dtype in TYPES:
        rng = np.random.default_rng(90 + int(code))
        y, _ = oracle.awgn_llrs(code, rng, 4 if code.n() >= 5120 else 12, 2.5, np.float32)
        llrs = np.concatenate([quantise(y, dtype, 8, 31), corner_frames(code, dtype, rng, noisy=2)])
        for m in (1, 3, 25):
            ref = fr.decode_fixed(st, llrs, m)
            for k in (0, 4, 8):
                got = fcr.decode_fixed_corrected(st, llrs, m, 1 << k, k, 0)
                assert all((x == y).all() for x, y in zip(ref, got)), (np.dtype(dtype).name, m, k)


@pytest.mark.parametrize("code,ebn0", [(LDPCCode.TC128, 3.0), (LDPCCode.TM1280, 3.0), (LDPCCode.TM2048, 1.7)], ids=lambda v: getattr(v, "name", None))
def test_a_power_of_two_scale_with_an_integer_offset_is_the_f32_corrected_schedule(code, ebn0):
    """Independent of the fixed-point restatements: with scale_num = 1 << k the scale is 1, and on the same integers given as float32
    tests/layered_corrected_restatement.py at (1.0, float(offset)) gives the same output, iters, success and app (as integers) --
    every f32 value is then a small exact integer.  That needs a frame in which no nv clamped; i16 at 8 / 31 has no other, so no frame
    is left out.  Offsets 0, 1 and 2, caps 1, 3 and 25."""
    F = {LDPCCode.TC128: 48, LDPCCode.TM1280: 24, LDPCCode.TM2048: 16}[code]
    y, _ = oracle.awgn_llrs(code, np.random.default_rng(1810 + int(code)), F, ebn0, np.float32)
    llrs = quantise(y, np.int16, 8, 31)
    st_i, st_f = fr.Structure(int(code)), lr.Structure(int(code))
    as_f32 = llrs.astype(np.float32)
    for k, offset in ((0, 0), (4, 1), (8, 2), (0, 2), (8, 1)):
        for m in (1, 3, 25):
            out, it, ok, app, clamped = fcr.decode_fixed_corrected(st_i, llrs, m, 1 << k, k, offset)
            assert not clamped.any()
            out_f, it_f, ok_f, app_f = lcr.decode_layered_corrected(st_f, as_f32, m, 1.0, float(offset))
            assert (out == out_f).all() and (it == it_f).all() and (ok == ok_f).all(), (k, offset, m)
            assert (app_f == np.rint(app_f)).all() and (app == app_f.astype(np.int32)).all(), (k, offset, m)


def failures(code, llrs, triple):
    st = layered_helpers.structure(code, fr.Structure)
    return int((fcr.decode_fixed_corrected(st, llrs, 25, *triple)[2] == 0).sum())


def test_failure_counts_at_fixed_seeds():
    """TM2048 at 1.7 dB, 600 frames of default_rng(1700) quantised to i8 at 8 / 31, cap 25: 34 failed frames at (16, 4, 0) -- plain --,
    14 at (13, 4, 0) and 6 at (16, 4, 1): both corrected settings fail strictly less often than plain."""
    code = LDPCCode.TM2048
    y, _ = oracle.awgn_llrs(code, np.random.default_rng(1700), 600, 1.7, np.float32)
    llrs = quantise(y, np.int8, 8, 31)
    plain, scaled, offs = (failures(code, llrs, t) for t in ((16, 4, 0), (13, 4, 0), (16, 4, 1)))
    print(f"TM2048 1.7 dB i8: failures {plain} plain, {scaled} at 13/16, {offs} at offset 1")
    assert scaled < plain and offs < plain
    assert (plain, scaled, offs) == (34, 14, 6)


def test_an_offset_is_not_free():
    """TM1280 at 3.5 dB, 600 frames of default_rng(1700), i8 at 8 / 31, cap 25: an offset of 1 fails MORE often than plain decoding
    (67 against 5) -- at 8 / 31 the messages of this code are often 1 to 3, and an offset of 1 wipes them out.  An offset is in units
    of the quantiser and has to be chosen for the code, the noise and the quantiser: the library has no default."""
    code = LDPCCode.TM1280
    y, _ = oracle.awgn_llrs(code, np.random.default_rng(1700), 600, 3.5, np.float32)
    llrs = quantise(y, np.int8, 8, 31)
    plain, offs = failures(code, llrs, (16, 4, 0)), failures(code, llrs, (16, 4, 1))
    print(f"TM1280 3.5 dB i8: failures {plain} plain, {offs} at offset 1")
    assert offs > plain
    assert (plain, offs) == (5, 67)


def test_header_declares_the_fixed_corrected_entry_points():
    text = open(os.path.join(ROOT, "include", "labrador_ldpc_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    tail = (r"size_t batch,\s*size_t max_iters,\s*uint32_t scale_num,\s*uint32_t scale_shift,\s*uint32_t offset,\s*"
            r"const struct labrador_ldpc_hip_opts \*opts\s*\)\s*;")
    for suf, t in (("i8", "int8_t"), ("i16", "int16_t")):
        assert re.search(rf"int\s+labrador_ldpc_decode_ms_layered_fixed_corrected_batch_{suf}\s*\(\s*enum labrador_ldpc_code code,\s*"
                         rf"const {t} \*llrs,\s*uint8_t \*output,\s*uint32_t \*iters,\s*uint8_t \*success,\s*" + tail, src)
        assert re.search(rf"int\s+labrador_ldpc_decode_ms_layered_fixed_corrected_soft_batch_{suf}\s*\(\s*enum labrador_ldpc_code code,\s*"
                         rf"const {t} \*llrs,\s*int32_t \*app,\s*uint8_t \*output,\s*uint32_t \*iters,\s*uint8_t \*success,\s*" + tail, src)
    assert re.search(r"#define\s+LABRADOR_LDPC_HIP_ABI\s+3\b", text)                # additions only


def test_library_python_and_rust_hold_the_fixed_corrected_entry_points():
    dll = ctypes.CDLL(la.LIB_PATH)
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for name in NAMES:
        assert hasattr(dll, name) and name in la.SYMBOLS
        assert la.SYMBOLS[name][1][-4:-1] == [ctypes.c_uint32] * 3
        assert re.search(rf"pub fn {name}\s*\([^)]*scale_num: u32, scale_shift: u32, offset: u32, opts: \*const HipOpts\) -> c_int;", rust), name
    assert la.lib.labrador_ldpc_hip_abi_version() == 3


def test_argument_checks_come_before_any_device_work():
    """A bad code, a NULL buffer, then the three parameters -- scale_shift 9, scale_num 0, scale_num (1 << shift) + 1, an offset of
    T_MAX + 1 -- are EINVAL naming the parameter, and a variant other than 0 is EUNSUPPORTED: all without a GPU, where a call that
    got as far as a device would answer ENODEV or ERUNTIME; the buffers stay as they were."""
    code = LDPCCode.TC128
    for suf, dtype in (("i8", np.int8), ("i16", np.int16)):
        tmax = int(np.iinfo(dtype).max)
        llrs = np.ones((1, code.n()), dtype)
        app = np.full((1, code.n() + code.punctured_bits()), -5, np.int32)
        out, it, ok = np.full((1, code.output_len()), 0xEE, np.uint8), np.full(1, 77, np.uint32), np.full(1, 7, np.uint8)
        hard = getattr(la.lib, f"labrador_ldpc_decode_ms_layered_fixed_corrected_batch_{suf}")
        soft = getattr(la.lib, f"labrador_ldpc_decode_ms_layered_fixed_corrected_soft_batch_{suf}")
        ph = [x.ctypes.data for x in (llrs, out, it, ok)]
        ps = [x.ctypes.data for x in (llrs, app, out, it, ok)]
        for fn, p in ((hard, ph), (soft, ps)):
            assert fn(9, *p, 1, 10, 13, 4, 0, None) == EINVAL
            assert fn(-1, *p, 1, 10, 0, 9, 0, None) == EINVAL
            assert "out of range" in la.last_error()
            for i in range(len(p)):
                q = list(p)
                q[i] = None
                assert fn(int(code), *q, 1, 10, 13, 4, 1, None) == EINVAL
                assert "NULL" in la.last_error()
                assert fn(int(code), *q, 1, 10, 0, 9, tmax + 1, None) == EINVAL            # the buffers come first
                assert "NULL" in la.last_error()
            assert fn(int(code), *p, 0, 10, 13, 4, 0, None) == OK
            assert fn(int(code), *([None] * len(p)), 0, 10, 16, 4, 1, None) == OK
            for memory in (la.MEM_HOST, la.MEM_DEVICE):
                for variant in (0, 3):                                                     # ... and the parameters before the variant
                    opts = la.HipOpts(-1, memory, None, variant, 0, None)
                    for triple, text in (((1, 9, 0), "scale_shift"), ((512, 9, 0), "scale_shift"), ((0, 0, 0), "scale_num"),
                                         ((0, 4, 0), "scale_num"), ((17, 4, 0), "scale_num"), ((2, 0, 0), "scale_num"),
                                         ((257, 8, 0), "scale_num"), ((13, 4, tmax + 1), "offset"), ((1, 0, 0xFFFFFFFF), "offset")):
                        assert fn(int(code), *p, 1, 10, *triple, ctypes.byref(opts)) == EINVAL, (suf, triple)
                        assert text in la.last_error() and "is not in" in la.last_error(), la.last_error()
                for variant in (1, 2, 64, -1):
                    opts = la.HipOpts(-1, memory, None, variant, 0, None)
                    for triple in ((13, 4, 0), (1, 0, tmax), (256, 8, 1)):
                        assert fn(int(code), *p, 1, 10, *triple, ctypes.byref(opts)) == EUNSUPPORTED, (suf, variant, triple)
                        assert "only 0 is" in la.last_error()
        assert (app == -5).all() and (out == 0xEE).all() and it[0] == 77 and ok[0] == 7


class _SpyLib:
    """Stands where the package keeps its library: a fixed-point layered decode looked up through it is recorded with its arguments
    and reports success without doing anything; every other symbol is the library's own."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        if not name.startswith("labrador_ldpc_decode_ms_layered_fixed_"):
            return getattr(self.real, name)

        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


def test_python_keywords_choose_the_entry_point(monkeypatch):
    """No keyword: the plain symbol, with the plain argument list.  Any keyword: the corrected symbol, the others at their defaults
    (scale_num = 1 << scale_shift, scale_shift = 0, offset = 0)."""
    code = LDPCCode.TC128
    spy = _SpyLib(la.lib)
    monkeypatch.setattr(la, "lib", spy)
    for suf, dtype in (("i8", np.int8), ("i16", np.int16)):
        llrs = np.ones((3, code.n()), dtype)
        for method, stem, nbuf in ((code.decode_ms_layered_fixed_batch, "labrador_ldpc_decode_ms_layered_fixed_", 4),
                                   (code.decode_ms_layered_fixed_soft_batch, "labrador_ldpc_decode_ms_layered_fixed_", 5)):
            soft = "soft_" if nbuf == 5 else ""
            for kw, triple in (({}, None), (dict(scale_num=13, scale_shift=4), (13, 4, 0)), (dict(scale_shift=4), (16, 4, 0)),
                               (dict(offset=1), (1, 0, 1)), (dict(scale_num=1), (1, 0, 0)), (dict(scale_shift=8, offset=2), (256, 8, 2)),
                               (dict(scale_num=16, scale_shift=4, offset=0), (16, 4, 0))):
                del spy.calls[:]
                method(llrs, 25, **kw)
                (name, args), = spy.calls
                if triple is None:
                    assert name == f"{stem}{soft}batch_{suf}" and len(args) == 1 + nbuf + 3
                else:
                    assert name == f"{stem}corrected_{soft}batch_{suf}" and len(args) == 1 + nbuf + 6, (name, kw)
                    assert args[1 + nbuf:1 + nbuf + 5] == (3, 25) + triple
    # what ctypes would wrap into a uint32_t silently is refused here; a float is no integer; the ranges are the library's
    one = np.ones((1, code.n()), np.int8)
    for bad in (dict(scale_num=-1), dict(scale_shift=1 << 32), dict(offset=(1 << 32) + 1)):
        with pytest.raises(ValueError):
            code.decode_ms_layered_fixed_batch(one, 25, **bad)
    with pytest.raises(TypeError):
        code.decode_ms_layered_fixed_batch(one, 25, offset=0.5)
    monkeypatch.undo()
    with pytest.raises(la.LdpcHipError, match="scale_shift 40"):
        code.decode_ms_layered_fixed_batch(one, 25, scale_shift=40)


def test_python_keywords_reach_the_librarys_checks():
    code = LDPCCode.TM1280
    for dtype in TYPES:
        llrs = np.ones((2, code.n()), dtype)
        tmax = int(np.iinfo(dtype).max)
        for kw, text in ((dict(scale_shift=9), "scale_shift"), (dict(scale_num=0), "scale_num"), (dict(scale_num=17, scale_shift=4), "scale_num"),
                         (dict(offset=tmax + 1), "offset")):
            with pytest.raises(la.LdpcHipError, match=text):
                code.decode_ms_layered_fixed_batch(llrs, 10, **kw)
            with pytest.raises(la.LdpcHipError, match=text):
                code.decode_ms_layered_fixed_soft_batch(llrs, 10, **kw)
        with pytest.raises(la.LdpcHipError, match="only 0 is"):
            code.decode_ms_layered_fixed_batch(llrs, 10, variant=2, scale_num=13, scale_shift=4)
        with pytest.raises(ValueError):
            code.decode_ms_layered_fixed_soft_batch(llrs, app=np.zeros((2, code.n()), np.int32), offset=1)
    with pytest.raises(la.LdpcHipError):
        code.decode_ms_layered_fixed_batch(np.ones((2, code.n()), np.float32), scale_num=13, scale_shift=4)      # i8 and i16 only


def test_the_ber_harness_checks_its_options():
    """The float scale and offset keep refusing quantised LLRs, the integer ones refuse f32 and the flooding schedule, and
    --fixed-scale takes NUM/DEN with DEN a power of two of at most 256 and NUM <= DEN: all decided before any device work."""
    from labrador_ldpc_amd import perftest
    code = LDPCCode.TC128
    for bad in (dict(llr="i8", schedule="layered", scale=0.8), dict(llr="i16", schedule="layered", offset=0.1),
                dict(schedule="layered", scale_num=13, scale_shift=4), dict(schedule="layered", llr="f32", fixed_offset=1),
                dict(scale_num=13, scale_shift=4), dict(llr="i8", fixed_offset=1)):
        with pytest.raises(ValueError):
            perftest.ms_trials(code, 3.0, "ebn0", **bad)
    assert perftest.fixed_scale("13/16") == (13, 4) and perftest.fixed_scale("1/1") == (1, 0) and perftest.fixed_scale("256/256") == (256, 8)
    base = ["--code", "TC128", "--snrs", "3.0", "--schedule", "layered", "--llr", "i8"]
    for bad in (["--fixed-scale", "3/5"], ["--fixed-scale", "300/256"], ["--fixed-scale", "0/16"], ["--fixed-scale", "1/512"],
                ["--fixed-scale", "0.8"], ["--fixed-offset", "-1"], ["--fixed-offset", "0.5"]):
        with pytest.raises(SystemExit) as e:
            perftest.main(base + bad)
        assert e.value.code == 2, bad
    for bad in (["--llr", "f32", "--fixed-scale", "13/16"], ["--schedule", "flooding", "--llr", "f32", "--fixed-offset", "1"]):
        with pytest.raises(SystemExit) as e:
            perftest.main(["--code", "TC128", "--snrs", "3.0", "--schedule", "layered"] + bad)
        assert e.value.code == 2, bad


@pytest.fixture(scope="module")
def corrected_object():
    return layered_helpers.built_object("decode_ms_fixed_corrected.o")


KERNEL = "decode_ms_layered_fixed_corrected_kernel"


def test_fixed_corrected_kernels_keep_their_sweep_loops_free_of_scratch(corrected_object):
    """The guard of test_layered_fixed_host.py on the new object: 36 kernels (both forms of all nine codes and both types), none of
    them a plain one; no scratch instruction in a backward-branch span with a sweep's 7 barriers, none at all in the one-wave kernels
    (the TC codes); the deltas of the shared cells land by LDS adds."""
    kernels = layered_helpers.kernels(corrected_object, KERNEL)
    assert len(kernels) == 36
    assert not layered_helpers.kernels(corrected_object, "decode_ms_layered_fixed_kernel")
    sweeps = 0
    for name, body in kernels.items():
        code = int(re.search(r"kernelILi(\d+)E", name).group(1))
        ops = [t.split()[0] for _, t, _ in body]
        assert "ds_add_u32" in ops and not any(o.startswith("flat_atomic") for o in ops), name
        if code <= 2:
            assert not any(o.startswith("scratch_") for o in ops), name
            assert "s_barrier" not in ops, name
            continue
        base, index = body[0][0], {b[0]: i for i, b in enumerate(body)}
        found = 0
        for i, (addr, text, tgt) in enumerate(body):
            if text.startswith(("s_cbranch", "s_branch")) and tgt is not None and base + tgt < addr and (base + tgt) in index:
                span = [t for _, t, _ in body[index[base + tgt]:i + 1]]
                if sum(t.startswith("s_barrier") for t in span) == 7:
                    found += 1
                    assert not any(t.startswith("scratch_") for t in span), f"{name}: scratch inside the sweep loop"
        assert found >= 1, name
        sweeps += found
    assert sweeps >= 24


VGPR_MARGIN = 8


def test_fixed_corrected_kernels_have_uniform_control_flow_and_fit(corrected_object, capsys):
    """At most 5 `s_cbranch_execnz` per kernel, the LDS of the plain kernels, and the VGPRs of the plain kernel of the same code, type
    and form plus at most VGPR_MARGIN.  The margin: the step needs the two corrected minima beside the uncorrected keys for a few
    instructions and nothing across a layer (its parameters are scalar), so 2 registers per check in flight -- 4 for TM8192's two
    checks per thread -- doubled for the allocator's granularity of 8.  Both figures of every kernel are printed."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    import scan_kernels
    layered_helpers.built_object("decode_ms_fixed_layered.o")
    table = scan_kernels.scan("build/csrc/decode_ms_fixed_corrected.o")
    assert len(table) == 36
    bad = {k: v for k, v in table.items() if v[1] > 5}
    assert not bad, bad
    res = kernel_resources.resources("build/csrc/decode_ms_fixed_corrected.o")
    assert len(res) == 36

    def key(name):
        return re.search(r"kernel<(.*?)>", name).group(1)
    plain = {key(name): int(vgpr) for _, name, vgpr, _, _, _, _ in kernel_resources.resources("build/csrc/decode_ms_fixed_layered.o")}
    assert len(plain) == 36
    with capsys.disabled():
        for _, name, vgpr, spill, _, lds, scratch in res:
            print(f"\n{name.split('(')[0][11:]}: {vgpr} VGPRs (plain {plain[key(name)]}, {spill} spilled), {lds} B LDS, {scratch} B scratch", end="")
    for _, name, vgpr, _, _, lds, _ in res:
        code = LDPCCode(int(re.search(r"kernel<(\d+),", name).group(1)))
        g = max(1, 64 // code.submatrix_size())
        assert int(lds) <= g * (4 * (code.n() + code.punctured_bits()) + 16) + 16, name
        assert int(vgpr) <= plain[key(name)] + VGPR_MARGIN, name
        assert int(vgpr) <= (128 if code == LDPCCode.TM8192 else 256), name
