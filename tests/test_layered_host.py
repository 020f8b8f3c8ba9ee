"""CPU-side checks of the layered schedule (labrador_ldpc_decode_ms_layered_{,soft_}batch_f32): the restatement of
tests/layered_restatement.py is tied to the oracle (with every edge in one layer, sweep i is the reference's iteration i + 1), its two
statements agree, the layered schedule beats flooding where it should, the header declares and the library exports both entry points,
their argument checks answer before any device work, and the layered kernels keep their sweep loops free of scratch traffic.  No
compute call needs a GPU."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import edge_frames
import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode
import layered_helpers
import layered_restatement as lr
import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, OK = -1, 0


def corner_frames(code, rng, frames=5):
    llrs, _ = oracle.awgn_llrs(code, rng, frames, 2.5, np.float32)
    fi = np.finfo(np.float32)
    specials = np.array([np.inf, -np.inf, 0.0, -0.0, fi.tiny / 4, -fi.tiny / 4, fi.max, -fi.max, np.nan], dtype=np.float32)
    for f in range(1, frames):
        pos = rng.choice(code.n(), size=1 + 4 * f, replace=False)
        llrs[f, pos] = rng.choice(specials, size=len(pos))
    return llrs


@pytest.mark.parametrize("code", list(LDPCCode), ids=lambda c: c.name)
def test_one_layer_restatement_is_the_reference_one_iteration_on(code):
    """One layer holding every edge: (success, iters + 1) and output with cap m equal the oracle's with cap m + 1 (iters m against
    m + 1 on failure), and app equals the oracle's va as values (NaN where NaN), for every frame the reference does not finish at
    iteration 0 -- AWGN frames at two Eb/N0, corner values and the whole-frame edge rows."""
    rng = np.random.default_rng(40 + int(code))
    F = 12 if code.n() >= 5120 else 24
    a, _ = oracle.awgn_llrs(code, rng, F, 1.5, np.float32)
    b, _ = oracle.awgn_llrs(code, rng, F, 2.5, np.float32)
    llrs = np.concatenate([a, b, corner_frames(code, rng), edge_frames.whole_frame_rows(code, np.float32, rng)])
    st = lr.Structure(int(code), lr.one_layer(oracle.edges(code)[0]))
    compared = 0
    for m in (1, 2, 3, 25):
        out, it, ok, app = lr.decode_layered(st, llrs, m)
        _, _, _, va = oracle.decode_ms_soft_batch(code, llrs, m + 1)
        for f in range(len(llrs)):
            ok0, it0, _ = oracle.decode_ms(code, llrs[f], 1)
            if ok0 and it0 == 0:
                continue
            s, i, o = oracle.decode_ms(code, llrs[f], m + 1)
            assert bool(ok[f]) == s, (m, f)
            assert int(it[f]) + 1 == (i if s else m + 1), (m, f)
            assert (out[f] == o).all(), (m, f)
            na, nb = np.isnan(app[f]), np.isnan(va[f])
            assert (na == nb).all() and (app[f][~na] == va[f][~nb]).all(), (m, f)
            compared += 1
    assert compared >= 4 * len(llrs) // 2


@pytest.mark.parametrize("code", [LDPCCode.TC128, LDPCCode.TM1280], ids=lambda c: c.name)
def test_vectorised_and_loop_statements_agree(code):
    rng = np.random.default_rng(7)
    F = 6 if code == LDPCCode.TC128 else 2
    llrs = corner_frames(code, rng, F)
    _statements_agree(code, llrs, (0, 1, 3, 25))


@pytest.mark.parametrize("code", [LDPCCode.TC128, LDPCCode.TM1280], ids=lambda c: c.name)
def test_vectorised_and_loop_statements_agree_on_whole_frame_rows(code):
    """All +-0.0, every third / fifth zero, denormal frames, sums that overflow, +-inf runs and +-FLT_MAX frames."""
    _statements_agree(code, edge_frames.whole_frame_rows(code, np.float32, np.random.default_rng(8)), (1, 3, 25))


def _statements_agree(code, llrs, caps):
    st = lr.Structure(int(code))
    F = len(llrs)
    for m in caps:
        out, it, ok, app = lr.decode_layered(st, llrs, m)
        for f in range(F):
            o, i, s, a = lr.decode_layered_loop(code, llrs[f], m)
            assert (o == out[f]).all() and i == it[f] and s == ok[f], (m, f)
            na, nb = np.isnan(a), np.isnan(app[f])
            assert (na == nb).all() and (a[~na] == app[f][~nb]).all(), (m, f)
        if m:
            assert (np.isnan(app[:, : code.n()]) == np.isnan(llrs)).all()


def test_block_layers_are_the_prototype_rows():
    for code in LDPCCode:
        chk, _ = oracle.edges(code)
        layers = lr.block_layers(code, chk)
        assert len(layers) == (4 if code.name.startswith("TC") else 3)
        assert np.array_equal(np.concatenate(layers), np.arange(len(chk)))       # contiguous runs, in edge order


def test_layered_beats_flooding_at_fixed_seeds():
    """TM2048 at 1.7 dB, 25 iterations: fewer frame errors and fewer passes per frame than the reference's flooding schedule (the
    oracle).  Passes: a flooding decode that succeeds at iteration i made i message passes, a layered one at sweep i made i + 1."""
    code = LDPCCode.TM2048
    llrs, _ = oracle.awgn_llrs(code, np.random.default_rng(17), 300, 1.7, np.float32)
    _, it_f, ok_f, _ = oracle.decode_ms_batch(code, llrs, 25)
    _, it_l, ok_l, _ = lr.decode_layered(lr.Structure(int(code)), llrs, 25)
    assert (ok_l == 0).sum() < (ok_f == 0).sum()
    passes_f = np.where(ok_f == 1, it_f.astype(np.int64), 25).mean()
    passes_l = np.where(ok_l == 1, it_l.astype(np.int64) + 1, 25).mean()
    assert passes_l < passes_f


def test_header_declares_the_layered_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "labrador_ldpc_hip.h")).read(), flags=re.S)
    assert re.search(r"int\s+labrador_ldpc_decode_ms_layered_batch_f32\s*\(\s*enum labrador_ldpc_code code,\s*const float \*llrs,\s*"
                     r"uint8_t \*output,\s*uint32_t \*iters,\s*uint8_t \*success,\s*size_t batch,\s*size_t max_iters,\s*"
                     r"const struct labrador_ldpc_hip_opts \*opts\s*\)\s*;", src)
    assert re.search(r"int\s+labrador_ldpc_decode_ms_layered_soft_batch_f32\s*\(\s*enum labrador_ldpc_code code,\s*const float \*llrs,\s*"
                     r"float \*app,\s*uint8_t \*output,\s*uint32_t \*iters,\s*uint8_t \*success,\s*size_t batch,\s*size_t max_iters,\s*"
                     r"const struct labrador_ldpc_hip_opts \*opts\s*\)\s*;", src)


def test_library_exports_the_layered_entry_points():
    dll = ctypes.CDLL(la.LIB_PATH)
    for name in ("labrador_ldpc_decode_ms_layered_batch_f32", "labrador_ldpc_decode_ms_layered_soft_batch_f32"):
        assert hasattr(dll, name) and name in la.SYMBOLS


def test_argument_checks_come_before_any_device_work():
    code = LDPCCode.TC128
    llrs = np.ones((1, code.n()), np.float32)
    app = np.zeros((1, code.n() + code.punctured_bits()), np.float32)
    out = np.zeros((1, code.output_len()), np.uint8)
    it = np.zeros(1, np.uint32)
    ok = np.zeros(1, np.uint8)
    hard = la.lib.labrador_ldpc_decode_ms_layered_batch_f32
    soft = la.lib.labrador_ldpc_decode_ms_layered_soft_batch_f32
    ph = [x.ctypes.data for x in (llrs, out, it, ok)]
    ps = [x.ctypes.data for x in (llrs, app, out, it, ok)]
    for fn, p in ((hard, ph), (soft, ps)):
        assert fn(9, *p, 1, 10, None) == EINVAL
        assert fn(-1, *p, 1, 10, None) == EINVAL
        assert "out of range" in la.last_error()
        for i in range(len(p)):
            q = list(p)
            q[i] = None
            assert fn(int(code), *q, 1, 10, None) == EINVAL
            assert "NULL" in la.last_error()
        assert fn(int(code), *p, 0, 10, None) == OK
        assert fn(int(code), *([None] * len(p)), 0, 10, None) == OK
    assert (app == 0).all() and (out == 0).all()


def test_python_binding_checks_its_buffers():
    code = LDPCCode.TM1280
    llrs = np.ones((2, code.n()), np.float32)
    with pytest.raises(ValueError):
        code.decode_ms_layered_soft_batch(llrs, app=np.zeros((2, code.n()), np.float32))
    with pytest.raises(ValueError):
        code.decode_ms_layered_batch(llrs[:, :-1])
    with pytest.raises(la.LdpcHipError):
        code.decode_ms_layered_batch(llrs.astype(np.int8))            # f32 only


@pytest.fixture(scope="module")
def layered_object():
    return layered_helpers.built_object("decode_ms_layered_f32.o")


def _kernels(obj):
    return layered_helpers.kernels(obj, "decode_ms_layered_kernel")


def test_layered_kernels_keep_their_sweep_loops_free_of_scratch(layered_object):
    """The loop-spill guard of tests/test_soft_output_host.py for the layered kernels, whose sweep holds 2R + 2 barriers (R = 3 block
    rows of the TM codes) instead of the flooding iteration's 2: no scratch instruction in a backward-branch span with that many
    barriers; the one-wave kernels (the TC codes, no s_barrier) none at all.  Both forms of all nine codes."""
    kernels = _kernels(layered_object)
    assert len(kernels) == 18
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
    assert sweeps >= 12


def test_layered_kernels_have_uniform_control_flow(layered_object):
    """tests/test_kernel_shape.py's bound (16 EXEC-masked loops) for the layered object, which scan_kernels.scan() reads with the rest."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import scan_kernels
    table = scan_kernels.scan("build/csrc/decode_ms_layered_*.o")
    assert len(table) == 18
    bad = {k: v for k, v in table.items() if v[1] > 16}
    assert not bad, bad
