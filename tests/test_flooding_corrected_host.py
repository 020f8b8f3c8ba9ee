"""CPU-side checks of normalized / offset min-sum on the flooding schedule (labrador_ldpc_decode_ms_corrected_{,soft_}batch_f32,
labrador_ldpc_decode_ms_cascade_corrected_batch_f32).  The restatement (tests/flooding_corrected_restatement.py) is
tied to the oracle at (1, 0) and to the pinned layered statement with one layer of all edges, its two statements agree, and it
reproduces the failure counts of the design's table.  Then what fails without the feature: the header declares and the library, the
Python table and the Rust shim hold the three entry points; their argument checks answer in the documented order before any device
work; the Python keywords and the harness switches do what they document.  No compute call needs a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import cascade_restatement as cr
import edge_frames
import flooding_corrected_restatement as fcr
import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode
import layered_corrected_restatement as lcr
from layered_helpers import same_app
from layered_restatement import one_layer
import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = list(LDPCCode)
EINVAL, EUNSUPPORTED, OK = -1, -4, 0
FMAX = float(np.finfo(np.float32).max)
HARD, SOFT, CASCADE = ("labrador_ldpc_decode_ms_corrected_batch_f32", "labrador_ldpc_decode_ms_corrected_soft_batch_f32",
                       "labrador_ldpc_decode_ms_cascade_corrected_batch_f32")
_ST = {}


def structure(code):
    if code not in _ST:
        _ST[code] = fcr.Structure(code)
    return _ST[code]


def corner_frames(code, rng, frames=6):
    """AWGN frames with +-inf, +-0.0, denormals, +-FLT_MAX and NaNs of both signs at random positions; the last one all NaN."""
    llrs, _ = oracle.awgn_llrs(code, rng, frames, 3.0, np.float32)
    fi = np.finfo(np.float32)
    specials = np.array([np.inf, -np.inf, 0.0, -0.0, fi.tiny / 4, -fi.tiny / 4, fi.max, -fi.max, np.nan], dtype=np.float32)
    neg_nan = np.array([np.nan], dtype=np.float32)
    neg_nan.view(np.uint32)[0] |= 1 << 31
    specials = np.concatenate([specials, neg_nan])
    for f in range(1, frames):
        pos = rng.choice(code.n(), size=1 + f * 3, replace=False)
        llrs[f, pos] = rng.choice(specials, size=len(pos))
    llrs[frames - 1, :] = np.nan
    return llrs


# ---- the restatement: passes without the feature, pins the numbers -----------------------------------------------------------------
@pytest.mark.parametrize("code", ALL, ids=lambda c: c.name)
def test_unit_scale_and_zero_offset_are_the_oracle(code):
    """(1, 0) against oracle.decode_ms_soft_batch at caps 0 / 1 / 3 / 25 on AWGN frames that converge and fail, corner values and the
    whole-frame edge rows: output, iters and success exactly, the marginals as values with NaN where NaN."""
    rng = np.random.default_rng(0xF1 + int(code))
    F = 2 if code.n() >= 5120 else 3
    llrs = np.concatenate([oracle.awgn_llrs(code, rng, F, e, np.float32)[0] for e in (0.5, 3.0)]
                          + [corner_frames(code, rng), edge_frames.whole_frame_rows(code, np.float32, rng)])
    got = fcr.decode_flooding_corrected_caps(structure(code), llrs, (0, 1, 3, 25), 1.0, 0.0)
    for m in (0, 1, 3, 25):
        out, it, ok, va = oracle.decode_ms_soft_batch(code, llrs, m)
        g = got[m]
        assert (g[0] == out).all() and (g[1] == it).all() and (g[2] == ok).all(), (code.name, m)
        for f in range(len(llrs)):
            assert same_app(g[3][f], va[f]), f"{code.name} cap {m} frame {f}: va differs from the oracle's"
        one = fcr.decode_flooding_corrected(structure(code), llrs, m, 1.0, 0.0)               # the one-cap form is the same run
        assert all((a == b).all() for a, b in zip(one[:3], g[:3])) and same_app(one[3], g[3])


@pytest.mark.parametrize("code,frames", [(LDPCCode.TC128, 8), (LDPCCode.TM1280, 2)], ids=["TC128", "TM1280"])
def test_one_layer_of_all_edges_is_the_flooding_schedule_one_iteration_behind(code, frames):
    """The tie to the pinned layered statement: for a frame not finished at iteration 0, corrected flooding at cap m + 1 equals
    layered_corrected_restatement.decode_layered_corrected_loop with ONE layer of all edges at cap m -- output, success, and iters one
    ahead (a sweep of that statement ends with the marginals and the parity test of the next flooding iteration)."""
    rng = np.random.default_rng(0x71E + int(code))
    llrs = np.concatenate([oracle.awgn_llrs(code, rng, frames // 2, e, np.float32)[0] for e in ((2.0, 4.0) if code == LDPCCode.TC128 else (1.5, 3.5))])
    chk, _ = oracle.edges(code)
    layers = one_layer(np.asarray(chk))
    pairs = ((0.8125, 0.0), (1.0, 0.1)) if code == LDPCCode.TC128 else ((0.875, 0.05),)
    compared = 0
    for scale, offset in pairs:
        got = fcr.decode_flooding_corrected_caps(structure(code), llrs, (2, 4, 26), scale, offset)
        for m in (1, 3, 25):
            out, it, ok, _ = got[m + 1]
            for f in range(len(llrs)):
                if ok[f] and it[f] == 0:
                    continue
                o2, i2, s2, _ = lcr.decode_layered_corrected_loop(code, llrs[f], m, scale, offset, layers=layers)
                assert (out[f] == o2).all() and int(ok[f]) == s2 and int(it[f]) == i2 + 1, (code.name, scale, offset, m, f)
                compared += 1
    assert compared >= len(pairs) * 3 * frames // 2


@pytest.mark.parametrize("code", [LDPCCode.TC128, LDPCCode.TC256, LDPCCode.TM1280], ids=lambda c: c.name)
def test_the_two_statements_agree(code):
    """Whole arrays against one frame edge by edge, with the reference's running two-minimum update: every parameter pair of the GPU
    tests at caps 0 / 1 / 3 / 25 (TM1280: 0 / 3 / 10), AWGN and corner frames."""
    rng = np.random.default_rng(0xA6 + int(code))
    small = code != LDPCCode.TM1280
    llrs = np.concatenate([oracle.awgn_llrs(code, rng, 2 if small else 1, e, np.float32)[0] for e in (1.0, 4.0)] + [corner_frames(code, rng, 4 if small else 2)])
    caps = (0, 1, 3, 25) if small else (0, 3, 10)
    pairs = ((1.0, 0.0), (0.8125, 0.0), (0.75, 0.0), (1.0, 0.1), (0.875, 0.05), (1.0, FMAX), (2.0 ** -126, 0.0), (1.0, 2.0 ** -149))
    for scale, offset in (pairs if small else pairs[1::3]):
        got = fcr.decode_flooding_corrected_caps(structure(code), llrs, caps, scale, offset)
        for m in caps:
            for f in range(len(llrs)):
                o, i, s, va = fcr.decode_flooding_corrected_loop(code, llrs[f], m, scale, offset)
                g = got[m]
                assert (g[0][f] == o).all() and int(g[1][f]) == i and int(g[2][f]) == s, (code.name, scale, offset, m, f)
                assert same_app(g[3][f], va), (code.name, scale, offset, m, f)


@pytest.mark.parametrize("code", [LDPCCode.TC128, LDPCCode.TM1280, LDPCCode.TM2048], ids=lambda c: c.name)
def test_an_offset_of_flt_max_leaves_the_llrs(code):
    """(1, FLT_MAX): every message is zero, so every iteration's marginals are the LLRs, with zeros at the punctured variables."""
    rng = np.random.default_rng(5)
    llrs, _ = oracle.awgn_llrs(code, rng, 6, 2.0, np.float32)
    for m in (1, 25):
        out, it, ok, va = fcr.decode_flooding_corrected(structure(code), llrs, m, 1.0, FMAX)
        assert (va[:, : code.n()] == llrs).all() and (va[:, code.n():] == 0).all()
        assert (out[:, : code.n() // 8] == np.packbits(llrs < 0, axis=1)).all()


@pytest.fixture(scope="module")
def tm2048_frames():
    return {eb: oracle.awgn_llrs(LDPCCode.TM2048, np.random.default_rng(seed), 600, eb, np.float32)[0] for eb, seed in ((1.7, 1700), (2.0, 2000))}


@pytest.fixture(scope="module")
def tm2048_13_16(tm2048_frames):
    return fcr.decode_flooding_corrected(structure(LDPCCode.TM2048), tm2048_frames[1.7], 25, 0.8125, 0.0)


def test_failure_counts_at_fixed_seeds(tm2048_frames, tm2048_13_16):
    """DESIGN.md 4.13's table: TM2048, cap 25, 600 frames.  1.7 dB, default_rng(1700): 156 frames fail plain flooding, 99 at
    (0.8125, 0), 74 at (1, 0.1); 2.0 dB, default_rng(2000): 26 / 13 / 10.  The mean iteration count falls with every correction."""
    code = LDPCCode.TM2048
    for eb, want in ((1.7, (156, 99, 74)), (2.0, (26, 13, 10))):
        llrs = tm2048_frames[eb]
        plain = oracle.decode_ms_batch(code, llrs, 25)
        res = [plain[1:3]]
        for pair in ((0.8125, 0.0), (1.0, 0.1)):
            r = tm2048_13_16 if (eb, pair) == (1.7, (0.8125, 0.0)) else fcr.decode_flooding_corrected(structure(code), llrs, 25, *pair)
            res.append(r[1:3])
        fails = tuple(int((ok == 0).sum()) for _, ok in res)
        means = [float(it.mean()) for it, _ in res]
        print(f"TM2048 {eb} dB: failures {fails}, mean iters {means}")
        assert fails == want
        assert means[1] < means[0] and means[2] < means[0]


def test_cascade_with_a_corrected_first_stage(tm2048_frames, tm2048_13_16):
    """The composition on the 1.7 dB frames: with stage 1 at (0.8125, 0), 99 frames go to stage 2, not 156; what both stages fail is
    never more than the layered decoder alone fails on all 600 frames, and the frames of stage 2 carry its results."""
    code = LDPCCode.TM2048
    llrs = tm2048_frames[1.7]
    alone = cr.layered(code)(llrs, 25)
    index = {row.tobytes(): f for f, row in enumerate(llrs)}

    def second(rows, cap):
        sel = [index[r.tobytes()] for r in rows]
        return tuple(x[sel] for x in alone[:3])

    out, it, ok, stage = cr.compose(lambda rows, cap: tm2048_13_16, second, llrs, 25, 25)
    print(f"TM2048 1.7 dB: {int(stage.sum())} frames to stage 2, {int((ok == 0).sum())} failures; layered alone {int((alone[2] == 0).sum())}")
    assert int(stage.sum()) == 99
    assert int((ok == 0).sum()) <= int((alone[2] == 0).sum())
    s2 = stage == 1
    assert (out[s2] == alone[0][s2]).all() and (it[s2] == alone[1][s2]).all() and (ok[s2] == alone[2][s2]).all()
    assert ok[~s2].all() and (out[~s2] == tm2048_13_16[0][~s2]).all()


# ---- what fails without the feature ---------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "labrador_ldpc_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    tail = r"float scale,\s*float offset,\s*const struct labrador_ldpc_hip_opts \*opts\s*\)\s*;"
    assert re.search(rf"int\s+{HARD}\s*\(\s*enum labrador_ldpc_code code,\s*const float \*llrs,\s*uint8_t \*output,\s*uint32_t \*iters,\s*"
                     r"uint8_t \*success,\s*size_t batch,\s*size_t max_iters,\s*" + tail, src)
    assert re.search(rf"int\s+{SOFT}\s*\(\s*enum labrador_ldpc_code code,\s*const float \*llrs,\s*float \*app,\s*uint8_t \*output,\s*"
                     r"uint32_t \*iters,\s*uint8_t \*success,\s*size_t batch,\s*size_t max_iters,\s*" + tail, src)
    assert re.search(rf"int\s+{CASCADE}\s*\(\s*enum labrador_ldpc_code code,\s*const float \*llrs,\s*uint8_t \*output,\s*uint32_t \*iters,\s*"
                     r"uint8_t \*success,\s*uint8_t \*stage,\s*size_t batch,\s*size_t max_iters,\s*size_t max_sweeps,\s*float flooding_scale,\s*"
                     r"float flooding_offset,\s*" + tail, src)
    assert re.search(r"#define\s+LABRADOR_LDPC_HIP_ABI\s+3\b", text)                # additions only
    comment = text[text.index("Flooding schedule with normalized / offset min-sum"):text.index(f"int {HARD}")]
    assert "never fused" in comment and "LABRADOR_LDPC_HIP_EUNSUPPORTED" in comment and "empty batch" in comment


def test_library_python_and_rust_hold_the_entry_points():
    dll = ctypes.CDLL(la.LIB_PATH)
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for name in (HARD, SOFT, CASCADE):
        assert hasattr(dll, name) and name in la.SYMBOLS
        assert re.search(rf"pub fn {name}\s*\([^)]*scale: f32, offset: f32, opts: \*const HipOpts\) -> c_int;", rust), name
    assert la.SYMBOLS[HARD][1][5:9] == [ctypes.c_size_t] * 2 + [ctypes.c_float] * 2
    assert la.SYMBOLS[SOFT][1][6:10] == [ctypes.c_size_t] * 2 + [ctypes.c_float] * 2
    assert la.SYMBOLS[CASCADE][1][6:13] == [ctypes.c_size_t] * 3 + [ctypes.c_float] * 4
    assert "flooding_scale: f32, flooding_offset: f32, scale: f32" in rust
    assert la.lib.labrador_ldpc_hip_abi_version() == 3


BAD_PAIRS = ((0.0, 0.0, "scale"), (1.5, 0.0, "scale"), (float("nan"), 0.0, "scale"), (-0.5, 0.0, "scale"), (float("inf"), 0.0, "scale"),
             (1.0, -0.1, "offset"), (1.0, float("inf"), "offset"), (1.0, float("nan"), "offset"))


def test_argument_checks_come_before_any_device_work():
    """The order of decode_batch(): the code, the range of (scale, offset) -- before the empty batch --, the empty batch whatever the
    pointers, the buffers (a NULL app among them), then `variant`.  All without a GPU, where a call that reached a device would say
    ENODEV."""
    code = LDPCCode.TC128
    llrs = np.ones((1, code.n()), np.float32)
    app = np.full((1, code.n() + code.punctured_bits()), -7.0, np.float32)
    out, it, ok = np.full((1, code.output_len()), 0xEE, np.uint8), np.full(1, 77, np.uint32), np.full(1, 7, np.uint8)
    hard_p = [x.ctypes.data for x in (llrs, out, it, ok)]
    soft_p = [x.ctypes.data for x in (llrs, app, out, it, ok)]
    for fn, p in ((getattr(la.lib, HARD), hard_p), (getattr(la.lib, SOFT), soft_p)):
        assert fn(9, *p, 1, 10, 1.0, 0.0, None) == EINVAL and "out of range" in la.last_error()
        assert fn(-1, *p, 1, 10, 2.0, 0.0, None) == EINVAL and "out of range" in la.last_error()              # the code comes first
        for scale, offset, text in BAD_PAIRS:
            for batch in (0, 1):                                                                              # ... before the empty batch
                assert fn(int(code), *p, batch, 10, scale, offset, None) == EINVAL, (scale, offset, batch)
                assert text in la.last_error() and "is not in" in la.last_error()
            assert fn(int(code), *([None] * len(p)), 1, 10, scale, offset, None) == EINVAL and "is not in" in la.last_error()
        assert fn(int(code), *p, 0, 10, 0.8125, 0.0, None) == OK
        assert fn(int(code), *([None] * len(p)), 0, 10, 1.0, 0.1, None) == OK
        for i in range(len(p)):                                                                               # a NULL buffer, app included
            q = list(p)
            q[i] = None
            for memory in (la.MEM_HOST, la.MEM_DEVICE):
                opts = la.HipOpts(-1, memory, None, 3, 0, None)                                               # ... comes before the variant
                assert fn(int(code), *q, 1, 10, 0.8125, 0.0, ctypes.byref(opts)) == EINVAL and "NULL" in la.last_error(), i
        for variant in (1, 2, 32, 256, -1):
            for memory in (la.MEM_HOST, la.MEM_DEVICE):
                opts = la.HipOpts(-1, memory, None, variant, 0, None)
                for pair in ((0.8125, 0.0), (1.0, 0.0)):                                                      # (the identity too: one kernel)
                    assert fn(int(code), *p, 1, 10, *pair, ctypes.byref(opts)) == EUNSUPPORTED, (variant, memory)
                    assert "corrected flooding decoder" in la.last_error()
    assert (out == 0xEE).all() and it[0] == 77 and ok[0] == 7 and (app == -7.0).all()


def test_cascade_argument_checks_come_before_any_device_work():
    """Both pairs are range-checked before the empty batch; a NULL buffer is EINVAL; a stage-1 pair other than the identity with a
    `variant` other than 0 is EUNSUPPORTED -- all before any device work."""
    code = LDPCCode.TC128
    fn = getattr(la.lib, CASCADE)
    llrs = np.ones((1, code.n()), np.float32)
    out, it = np.full((1, code.output_len()), 0xEE, np.uint8), np.full(1, 77, np.uint32)
    ok, stage = np.full(1, 7, np.uint8), np.full(1, 9, np.uint8)
    p = [x.ctypes.data for x in (llrs, out, it, ok, stage)]
    assert fn(9, *p, 1, 10, 10, 0.8125, 0.0, 1.0, 0.0, None) == EINVAL and "out of range" in la.last_error()
    for scale, offset, text in BAD_PAIRS:
        for batch in (0, 1):
            assert fn(int(code), *p, batch, 10, 10, scale, offset, 1.0, 0.0, None) == EINVAL, (scale, offset, batch)    # stage 1's pair
            assert text in la.last_error() and "is not in" in la.last_error()
            assert fn(int(code), *p, batch, 10, 10, 0.8125, 0.0, scale, offset, None) == EINVAL, (scale, offset, batch)  # stage 2's pair
            assert text in la.last_error() and "is not in" in la.last_error()
    assert fn(int(code), *p, 0, 10, 10, 0.8125, 0.0, 1.0, 0.1, None) == OK
    assert fn(int(code), *([None] * 5), 0, 10, 10, 1.0, 0.1, 0.75, 0.0, None) == OK
    for i in range(5):
        q = list(p)
        q[i] = None
        opts = la.HipOpts(-1, la.MEM_HOST, None, 3, 0, None)
        assert fn(int(code), *q, 1, 10, 10, 0.8125, 0.0, 1.0, 0.0, ctypes.byref(opts)) == EINVAL and "NULL" in la.last_error(), i
    for variant in (1, 2, 32, 256):
        for memory in (la.MEM_HOST, la.MEM_DEVICE):
            opts = la.HipOpts(-1, memory, None, variant, 0, None)
            for pair in ((0.8125, 0.0), (1.0, 0.1)):
                assert fn(int(code), *p, 1, 10, 10, *pair, 1.0, 0.0, ctypes.byref(opts)) == EUNSUPPORTED, (variant, memory, pair)
                assert "corrected flooding decoder" in la.last_error()
    assert (out == 0xEE).all() and it[0] == 77 and ok[0] == 7 and stage[0] == 9


class _SpyLib:
    """Stands where the package keeps its library: a batched min-sum decode looked up through it is recorded with its arguments and
    reports success without doing anything; every other symbol is the library's own."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        if not name.startswith("labrador_ldpc_decode_ms_"):
            return getattr(self.real, name)
        if not hasattr(self.real, name):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


def test_python_keywords(monkeypatch):
    """decode_ms_batch / decode_ms_soft_batch: the defaults call the plain entries, any other pair the corrected ones with the pair
    behind max_iters; decode_ms_cascade_batch: flooding_scale / flooding_offset likewise.  A non-default pair takes float32 only."""
    code = LDPCCode.TC128
    spy = _SpyLib(la.lib)
    monkeypatch.setattr(la, "lib", spy)
    llrs = np.ones((3, code.n()), np.float32)

    def one_call(method, *a, **kw):
        del spy.calls[:]
        res = method(*a, **kw)
        (name, args), = spy.calls
        return name, args, res

    name, args, res = one_call(code.decode_ms_batch, llrs, 25)
    assert name == "labrador_ldpc_decode_ms_batch_f32" and len(args) == 8 and len(res) == 3
    name, args, res = one_call(code.decode_ms_batch, llrs, 25, scale=1.0, offset=0.0)
    assert name == "labrador_ldpc_decode_ms_batch_f32" and len(args) == 8
    for kw, tail in ((dict(scale=0.8125), (3, 25, 0.8125, 0.0)), (dict(offset=0.5), (3, 25, 1.0, 0.5)), (dict(scale=0.75, offset=0.25), (3, 25, 0.75, 0.25))):
        name, args, res = one_call(code.decode_ms_batch, llrs, 25, **kw)
        assert name == HARD and len(args) == 10 and args[5:9] == tail and len(res) == 3, (kw, args)
        name, args, res = one_call(code.decode_ms_soft_batch, llrs, 25, **kw)
        assert name == SOFT and len(args) == 11 and args[6:10] == tail and len(res) == 4, (kw, args)
        assert res[0].shape == (3, code.n() + code.punctured_bits()) and res[0].dtype == np.float32
    name, args, res = one_call(code.decode_ms_soft_batch, llrs, 25)
    assert name == "labrador_ldpc_decode_ms_soft_batch_f32" and len(args) == 9
    name, args, res = one_call(code.decode_ms_cascade_batch, llrs, 25, scale=0.75)
    assert name == "labrador_ldpc_decode_ms_cascade_batch_f32" and args[6:11] == (3, 25, 25, 0.75, 0.0)
    for kw, tail in ((dict(flooding_scale=0.8125), (3, 25, 25, 0.8125, 0.0, 1.0, 0.0)),
                     (dict(flooding_offset=0.1, max_sweeps=7, scale=0.75, offset=0.5), (3, 25, 7, 1.0, 0.1, 0.75, 0.5))):
        name, args, res = one_call(code.decode_ms_cascade_batch, llrs, 25, **kw)
        assert name == CASCADE and len(args) == 14 and args[6:13] == tail and len(res) == 4, (kw, args)
        assert res[3].shape == (3,) and res[3].dtype == np.uint8
    # the variant travels in the options, where the library refuses it; a non-default pair has entries for float32 alone
    del spy.calls[:]
    for bad in (llrs.astype(np.float16), llrs.astype(np.int8), llrs.astype(np.int16), llrs.astype(np.int32), llrs.astype(np.float64)):
        assert len(code.decode_ms_batch(bad, 25)) == 3                          # (the defaults still take every type)
        for method, kw in ((code.decode_ms_batch, dict(scale=0.8125)), (code.decode_ms_batch, dict(offset=0.1)),
                           (code.decode_ms_soft_batch, dict(scale=0.8125))):
            with pytest.raises(la.LdpcHipError, match="no batched kernel"):
                method(bad, 25, **kw)
    for bad in (llrs.astype(np.float16), llrs.astype(np.int8)):
        with pytest.raises((la.LdpcHipError, ValueError)):
            code.decode_ms_cascade_batch(bad, 25, flooding_scale=0.8125)
    assert all(name.endswith(("_batch_f16", "_batch_i8", "_batch_i16", "_batch_i32", "_batch_f64")) for name, _ in spy.calls)


def test_python_keywords_reach_the_library_checks():
    code = LDPCCode.TC128
    llrs = np.ones((2, code.n()), np.float32)
    with pytest.raises(la.LdpcHipError, match="scale 1.5"):
        code.decode_ms_batch(llrs, 10, scale=1.5)
    with pytest.raises(la.LdpcHipError, match="offset -1"):
        code.decode_ms_soft_batch(llrs, 10, offset=-1.0)
    with pytest.raises(la.LdpcHipError, match="scale 0"):
        code.decode_ms_cascade_batch(llrs, 10, flooding_scale=0.0)
    with pytest.raises(la.LdpcHipError, match="corrected flooding decoder"):
        code.decode_ms_batch(llrs, 10, scale=0.8125, variant=2)
    with pytest.raises(la.LdpcHipError, match="corrected flooding decoder"):
        code.decode_ms_cascade_batch(llrs, 10, flooding_offset=0.1, variant=32)


def test_the_ber_harness_knows_the_flooding_correction():
    """flooding_scale / flooding_offset belong to the flooding schedule and the cascade on f32 LLRs: anywhere else a ValueError, decided
    before any device work; scale / offset with the flooding schedule stay a ValueError."""
    from labrador_ldpc_amd import perftest
    code = LDPCCode.TC128
    for bad in (dict(schedule="layered", flooding_scale=0.8125), dict(schedule="layered", flooding_offset=0.1),
                dict(schedule="flooding", llr="f16", flooding_scale=0.8125), dict(schedule="cascade", llr="bf16", flooding_offset=0.1),
                dict(schedule="cascade", llr="i8", flooding_scale=0.8125), dict(schedule="layered", llr="i16", flooding_scale=0.8125),
                dict(schedule="cascade", llr="i8", from_f32=True, flooding_scale=0.8125),
                dict(schedule="flooding", scale=0.8125), dict(schedule="flooding", offset=0.1, flooding_scale=0.8125)):
        with pytest.raises(ValueError):
            perftest.ms_trials(code, 3.0, "ebn0", **bad)
    for bad in (["--schedule", "layered", "--flooding-scale", "0.8125"], ["--schedule", "layered", "--flooding-offset", "0.1"],
                ["--llr", "f16", "--flooding-scale", "0.8125"], ["--schedule", "cascade", "--llr", "i8", "--flooding-offset", "0.1"]):
        with pytest.raises(ValueError):
            perftest.main(["--code", "TC128", "--snrs", "3.0"] + bad)
    with pytest.raises(SystemExit):
        perftest.main(["--code", "TC128", "--snrs", "3.0", "--flooding-scale", "x"])
    assert "--flooding-scale" in perftest.__doc__ and "--flooding-offset" in perftest.__doc__
