"""CPU-side checks of normalized / offset min-sum on the layered schedule (labrador_ldpc_decode_ms_layered_corrected_{,soft_}batch_f32,
DESIGN.md 4.6): the restatement of tests/layered_corrected_restatement.py with (scale, offset) = (1, 0) is the plain layered
restatement bit for bit, its two statements agree, the correction lowers the frame error count and the passes where it should, the
header declares and the library exports both entry points, their argument checks (the two parameters included) answer before any
device work, and the corrected kernels keep the shape of the layered ones.  No compute call needs a GPU."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import edge_frames
import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode
import layered_corrected_restatement as lcr
import layered_helpers
from layered_helpers import same_app
import layered_restatement as lr
import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, OK = -1, 0
FMAX = float(np.finfo(np.float32).max)
EXTREMES = ((1.0, FMAX), (2.0 ** -126, 0.0), (1.0, 2.0 ** -149))


def corner_frames(code, rng, frames=5):
    llrs, _ = oracle.awgn_llrs(code, rng, frames, 2.5, np.float32)
    fi = np.finfo(np.float32)
    specials = np.array([np.inf, -np.inf, 0.0, -0.0, fi.tiny / 4, -fi.tiny / 4, fi.max, -fi.max, np.nan], dtype=np.float32)
    for f in range(1, frames):
        pos = rng.choice(code.n(), size=1 + 4 * f, replace=False)
        llrs[f, pos] = rng.choice(specials, size=len(pos))
    return llrs


@pytest.mark.parametrize("code", list(LDPCCode), ids=lambda c: c.name)
def test_unit_scale_and_zero_offset_are_the_plain_layered_schedule(code):
    """(1, 0) is the identity on every message magnitude: output, iters, success and app (as bits, NaN where NaN) equal
    layered_restatement.decode_layered, caps 1 / 2 / 3 / 25, AWGN frames at two Eb/N0, corner values and the whole-frame edge rows."""
    rng = np.random.default_rng(60 + int(code))
    F = 6 if code.n() >= 5120 else 16
    a, _ = oracle.awgn_llrs(code, rng, F, 1.5, np.float32)
    b, _ = oracle.awgn_llrs(code, rng, F, 2.5, np.float32)
    llrs = np.concatenate([a, b, corner_frames(code, rng), edge_frames.whole_frame_rows(code, np.float32, rng)])
    st = lr.Structure(int(code))
    for m in (1, 2, 3, 25):
        out, it, ok, app = lr.decode_layered(st, llrs, m)
        out_c, it_c, ok_c, app_c = lcr.decode_layered_corrected(st, llrs, m, 1.0, 0.0)
        assert (out == out_c).all() and (it == it_c).all() and (ok == ok_c).all(), m
        assert same_app(app, app_c), m
        fin = ~np.isnan(app)
        assert (app[fin].view(np.uint32) == app_c[fin].view(np.uint32)).all(), m


PAIRS = ((0.8125, 0.0), (1.0, 0.1), (0.875, 0.05)) + EXTREMES


@pytest.mark.parametrize("code", [LDPCCode.TC128, LDPCCode.TM1280], ids=lambda c: c.name)
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]:g}-{p[1]:g}")
def test_vectorised_and_loop_statements_agree(code, pair):
    rng = np.random.default_rng(7)
    llrs = corner_frames(code, rng, 5 if code == LDPCCode.TC128 else 2)
    if code == LDPCCode.TC128:
        llrs = np.concatenate([llrs, edge_frames.whole_frame_rows(code, np.float32, np.random.default_rng(8))])
    st = lr.Structure(int(code))
    scale, offset = pair
    for m in (0, 1, 3, 25):
        out, it, ok, app = lcr.decode_layered_corrected(st, llrs, m, scale, offset)
        for f in range(len(llrs)):
            o, i, s, a = lcr.decode_layered_corrected_loop(code, llrs[f], m, scale, offset)
            assert (o == out[f]).all() and i == it[f] and s == ok[f], (m, f)
            assert same_app(a, app[f]), (m, f)
        if m:
            assert (np.isnan(app[:, : code.n()]) == np.isnan(llrs)).all()


def test_an_offset_of_flt_max_leaves_the_llrs():
    """(1, FLT_MAX): every message is zero, so every sweep's marginals are the LLRs themselves (punctured variables zero)."""
    code = LDPCCode.TC256
    llrs, _ = oracle.awgn_llrs(code, np.random.default_rng(5), 8, 3.0, np.float32)
    _, it, ok, app = lcr.decode_layered_corrected(lr.Structure(int(code)), llrs, 3, 1.0, FMAX)
    assert (app[:, : code.n()] == llrs).all() and (app[:, code.n():] == 0).all()


def passes(it, ok, cap):
    return np.where(ok == 1, it.astype(np.int64) + 1, cap).mean()


def test_the_correction_beats_plain_layered_min_sum_at_fixed_seeds():
    """TM2048 at 1.7 dB, cap 25, 300 frames of default_rng(17): (0.8125, 0) and (1, 0.1) each leave fewer failed frames than (1, 0)
    and take fewer passes per frame (a success at sweep i is i + 1 passes, a failure 25)."""
    code = LDPCCode.TM2048
    llrs, _ = oracle.awgn_llrs(code, np.random.default_rng(17), 300, 1.7, np.float32)
    st = lr.Structure(int(code))
    _, it_p, ok_p, _ = lcr.decode_layered_corrected(st, llrs, 25, 1.0, 0.0)
    fail_p, pass_p = int((ok_p == 0).sum()), passes(it_p, ok_p, 25)
    for scale, offset in ((0.8125, 0.0), (1.0, 0.1)):
        _, it_c, ok_c, _ = lcr.decode_layered_corrected(st, llrs, 25, scale, offset)
        print(f"TM2048 1.7 dB ({scale}, {offset}): failures {int((ok_c == 0).sum())} against {fail_p}, "
              f"passes {passes(it_c, ok_c, 25):.2f} against {pass_p:.2f}")
        assert int((ok_c == 0).sum()) < fail_p
        assert passes(it_c, ok_c, 25) < pass_p


HARD = "labrador_ldpc_decode_ms_layered_corrected_batch_f32"
SOFT = "labrador_ldpc_decode_ms_layered_corrected_soft_batch_f32"


def test_header_declares_the_corrected_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "labrador_ldpc_hip.h")).read(), flags=re.S)
    assert re.search(r"int\s+" + HARD + r"\s*\(\s*enum labrador_ldpc_code code,\s*const float \*llrs,\s*"
                     r"uint8_t \*output,\s*uint32_t \*iters,\s*uint8_t \*success,\s*size_t batch,\s*size_t max_iters,\s*"
                     r"float scale,\s*float offset,\s*const struct labrador_ldpc_hip_opts \*opts\s*\)\s*;", src)
    assert re.search(r"int\s+" + SOFT + r"\s*\(\s*enum labrador_ldpc_code code,\s*const float \*llrs,\s*"
                     r"float \*app,\s*uint8_t \*output,\s*uint32_t \*iters,\s*uint8_t \*success,\s*size_t batch,\s*size_t max_iters,\s*"
                     r"float scale,\s*float offset,\s*const struct labrador_ldpc_hip_opts \*opts\s*\)\s*;", src)


def test_library_exports_the_corrected_entry_points():
    dll = ctypes.CDLL(la.LIB_PATH)
    for name in (HARD, SOFT):
        assert hasattr(dll, name) and name in la.SYMBOLS
        assert la.SYMBOLS[name][1][-3:-1] == [ctypes.c_float, ctypes.c_float]


BAD_SCALES = (0.0, -0.5, float(np.nextafter(np.float32(1.0), np.float32(2.0))), float("nan"), float("inf"))
BAD_OFFSETS = (-1e-6, float("nan"), float("inf"))


def test_argument_checks_come_before_any_device_work():
    code = LDPCCode.TC128
    llrs = np.ones((1, code.n()), np.float32)
    app = np.zeros((1, code.n() + code.punctured_bits()), np.float32)
    out = np.zeros((1, code.output_len()), np.uint8)
    it = np.zeros(1, np.uint32)
    ok = np.zeros(1, np.uint8)
    hard = getattr(la.lib, HARD)
    soft = getattr(la.lib, SOFT)
    ph = [x.ctypes.data for x in (llrs, out, it, ok)]
    ps = [x.ctypes.data for x in (llrs, app, out, it, ok)]
    for fn, p in ((hard, ph), (soft, ps)):
        assert fn(9, *p, 1, 10, 1.0, 0.0, None) == EINVAL
        assert fn(-1, *p, 1, 10, 0.75, 0.0, None) == EINVAL
        assert "out of range" in la.last_error()
        for i in range(len(p)):
            q = list(p)
            q[i] = None
            assert fn(int(code), *q, 1, 10, 0.8125, 0.1, None) == EINVAL
            assert "NULL" in la.last_error()
        assert fn(int(code), *p, 0, 10, 0.8125, 0.0, None) == OK
        assert fn(int(code), *([None] * len(p)), 0, 10, 1.0, 0.1, None) == OK
        for batch in (1, 0):
            for scale in BAD_SCALES:
                assert fn(int(code), *p, batch, 10, scale, 0.0, None) == EINVAL, scale
                assert "scale" in la.last_error() and "offset" not in la.last_error()
            for offset in BAD_OFFSETS:
                assert fn(int(code), *p, batch, 10, 1.0, offset, None) == EINVAL, offset
                assert "offset" in la.last_error() and "scale" not in la.last_error()
    assert (app == 0).all() and (out == 0).all()


def test_python_keywords_check_parameters_and_buffers():
    code = LDPCCode.TM1280
    llrs = np.ones((2, code.n()), np.float32)
    for scale in BAD_SCALES:
        with pytest.raises(la.LdpcHipError, match="scale"):
            code.decode_ms_layered_batch(llrs, 10, scale=scale)
        with pytest.raises(la.LdpcHipError, match="scale"):
            code.decode_ms_layered_soft_batch(llrs, 10, scale=scale, offset=0.1)
    for offset in BAD_OFFSETS:
        with pytest.raises(la.LdpcHipError, match="offset"):
            code.decode_ms_layered_batch(llrs, 10, offset=offset)
        with pytest.raises(la.LdpcHipError, match="offset"):
            code.decode_ms_layered_soft_batch(llrs, 10, scale=0.8125, offset=offset)
    with pytest.raises(ValueError):
        code.decode_ms_layered_soft_batch(llrs, app=np.zeros((2, code.n()), np.float32), scale=0.8125)
    with pytest.raises(ValueError):
        code.decode_ms_layered_batch(llrs[:, :-1], offset=0.1)
    with pytest.raises(la.LdpcHipError):
        code.decode_ms_layered_batch(llrs.astype(np.int8), scale=0.8125)            # f32 only


def test_perftest_refuses_the_correction_with_the_flooding_schedule():
    from labrador_ldpc_amd import perftest
    with pytest.raises(ValueError):
        perftest.ms_trials(LDPCCode.TC128, 3.0, "ebn0", scale=0.8125)
    with pytest.raises(ValueError):
        perftest.ms_trials(LDPCCode.TC128, 3.0, "ebn0", schedule="flooding", offset=0.1)


@pytest.fixture(scope="module")
def corrected_object():
    return layered_helpers.built_object("decode_ms_corrected_f32.o")


KERNEL = "decode_ms_corrected_kernel"


def _kernels(obj):
    return layered_helpers.kernels(obj, KERNEL)


def test_corrected_kernels_keep_their_sweep_loops_free_of_scratch(corrected_object):
    """The guard of tests/test_layered_host.py on the new object: 18 kernels (both forms of all nine codes) whose names the counts of
    the layered and soft-output objects do not match; no scratch instruction in a backward-branch span with a sweep's 8 barriers, none at
    all in the one-wave kernels (the TC codes); and the correction is there: every kernel multiplies, subtracts and clamps."""
    kernels = _kernels(corrected_object)
    assert len(kernels) == 18
    assert not any("decode_ms_layered_kernel" in k or "soft_" in k for k in kernels)
    sweeps = 0
    for name, body in kernels.items():
        code = int(re.search(r"kernelILi(\d+)E", name).group(1))
        ops = [t.split()[0] for _, t, _ in body]
        assert any(o.startswith("v_mul_f32") for o in ops) and any(o.startswith("v_max_f32") for o in ops), name
        assert not any(o.startswith(("v_fma_f32", "v_fmac_f32", "v_mad_f32", "v_mac_f32", "v_pk_fma_f32")) for o in ops), name
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
    assert sweeps >= 12


def test_corrected_kernels_have_uniform_control_flow(corrected_object):
    """tests/test_kernel_shape.py's bound (16 EXEC-masked loops) for the corrected object."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import scan_kernels
    table = scan_kernels.scan("build/csrc/decode_ms_corrected_*.o")
    assert len(table) == 18
    bad = {k: v for k, v in table.items() if v[1] > 16}
    assert not bad, bad
