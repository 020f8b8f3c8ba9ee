"""CPU-side checks of the fixed-point layered schedule (labrador_ldpc_decode_ms_layered_fixed_{,soft_}batch_{i8,i16}):
the two statements of tests/layered_fixed_restatement.py agree, the restatement is tied to the oracle (with every edge in one layer,
sweep i is the reference's iteration i + 1 wherever nothing was clamped), the order in which a variable's u are summed does not
matter, the failure counts of the issue's table reproduce, the header declares and the library and the Rust shim hold the four entry
points, their argument checks answer before any device work, and the kernels keep their sweep loops free of scratch traffic.  No
compute call needs a GPU."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode
import layered_fixed_restatement as fr
import layered_helpers
from layered_helpers import quantise
import layered_restatement as lr
import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, OK, EUNSUPPORTED = -1, 0, -4
TYPES = (np.int8, np.int16)
NAMES = [f"labrador_ldpc_decode_ms_layered_fixed_{soft}batch_{t}" for soft in ("", "soft_") for t in ("i8", "i16")]


def corner_frames(code, dtype, rng, noisy=3):
    """All T_MAX, all -T_MAX, all T's minimum, all zero, alternating extremes, the minimum against T_MAX, and AWGN frames with
    extremes strewn in."""
    n, info = code.n(), np.iinfo(dtype)
    tmax = int(info.max)
    alt = np.where(np.arange(n) % 2 == 0, tmax, -tmax)
    rows = [np.full(n, tmax), np.full(n, -tmax), np.full(n, info.min), np.zeros(n), alt, -alt, np.where(np.arange(n) % 2 == 0, info.min, tmax)]
    y, _ = oracle.awgn_llrs(code, rng, noisy, 2.5, np.float32)
    extra = quantise(y, dtype, 8, 31).astype(np.int64)
    for f in range(noisy):
        pos = rng.choice(n, size=2 + 9 * f, replace=False)
        extra[f, pos] = rng.choice([tmax, -tmax, int(info.min), 0], size=len(pos))
    return np.concatenate([np.stack(rows), extra]).astype(dtype)


@pytest.mark.parametrize("dtype", TYPES, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("code", [LDPCCode.TC128, LDPCCode.TM1280], ids=lambda c: c.name)
def test_whole_array_and_loop_statements_agree(code, dtype):
    """output, iters, success, app and the clamp flag, at caps 0, 1, 3 and 25 (TM1280: 25 on the first frames only -- the loop form is
    slow), on corner frames: all T_MAX, all -T_MAX, all of T's minimum, all zero, alternating extremes."""
    llrs = corner_frames(code, dtype, np.random.default_rng(7))
    st = fr.Structure(int(code))
    saw_clamp = False
    for m in (0, 1, 3, 25):
        F = len(llrs) if (code == LDPCCode.TC128 or m < 25) else 5
        out, it, ok, app, cl = fr.decode_fixed(st, llrs[:F], m)
        assert app.dtype == np.int32
        for f in range(F):
            o, i, s, a, c = fr.decode_fixed_loop(code, llrs[f], m)
            assert (o == out[f]).all() and i == it[f] and s == ok[f] and (a == app[f]).all() and c == cl[f], (m, f)
        saw_clamp |= bool(cl.any())
        if m == 0:
            assert not out.any() and not it.any() and not ok.any() and not app.any()
    assert saw_clamp
    # T's minimum is read as -T_MAX
    lo = np.full((1, code.n()), np.iinfo(dtype).min, dtype)
    a, b = fr.decode_fixed(st, lo, 3), fr.decode_fixed(st, np.maximum(lo, -np.iinfo(dtype).max), 3)
    assert all((x == y).all() for x, y in zip(a, b))


# Quantisations of the tie below.  i16 at 8 / 31: no message can come near 32767.  i8: 8 / 31, but 4 / 15 for the rate-1/2 codes
# TM2048 and TM8192, whose messages at 8 / 31 reach 127 in a third and more of the frames (measured with the restatement on these
# frames: at most 3 of 120 frames with a clamp at the settings below, none for i16).
TIE_EBN0 = {0: 4.0, 1: 3.5, 2: 3.0, 3: 3.5, 4: 2.5, 5: 2.0, 6: 3.0, 7: 2.2, 8: 1.8}


def tie_quantiser(code, dtype):
    return (4, 15) if dtype == np.int8 and code in (LDPCCode.TM2048, LDPCCode.TM8192) else (8, 31)


@pytest.mark.parametrize("dtype", TYPES, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("code", list(LDPCCode), ids=lambda c: c.name)
def test_one_layer_restatement_is_the_reference_one_iteration_on(code, dtype):
    """One layer holding every edge: (success, iters + 1) and output with cap m equal oracle.decode_ms_batch's with cap m + 1 (iters m
    against m + 1 on failure), for every frame the reference does not finish at iteration 0 and in which no nv was clamped.  Only a
    clamp may leave a frame out: at most 10 % of the frames, and none at all for i16."""
    F = 40 if code.n() >= 5120 else 120
    y, _ = oracle.awgn_llrs(code, np.random.default_rng(1800 + int(code)), F, TIE_EBN0[int(code)], np.float32)
    llrs = quantise(y, dtype, *tie_quantiser(code, dtype))
    st = fr.Structure(int(code), lr.one_layer(oracle.edges(code)[0]))
    _, it0, ok0, _ = oracle.decode_ms_batch(code, llrs, 1)
    at_zero = (ok0 == 1) & (it0 == 0)
    for m in (1, 2, 3, 25):
        out, it, ok, _, clamped = fr.decode_fixed(st, llrs, m)
        assert clamped.sum() <= (0 if dtype == np.int16 else F // 10), (m, int(clamped.sum()))
        o_c, it_c, ok_c, _ = oracle.decode_ms_batch(code, llrs, m + 1)
        take = ~at_zero & ~clamped
        assert take.sum() >= F - F // 10 - at_zero.sum()
        assert (ok[take] == ok_c[take]).all(), m
        assert (it[take].astype(np.int64) + 1 == np.where(ok_c[take] == 1, it_c[take].astype(np.int64), m + 1)).all(), m
        assert (out[take] == o_c[take]).all(), m


@pytest.mark.parametrize("dtype", TYPES, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("code", [LDPCCode.TC256, LDPCCode.TM1280], ids=lambda c: c.name)
def test_the_order_of_a_marginals_sum_does_not_matter(code, dtype):
    """Shuffling the order in which a variable's u are summed changes nothing: both statements, frames that clamp included."""
    rng = np.random.default_rng(11)
    llrs = corner_frames(code, dtype, rng, noisy=5)
    E = len(oracle.edges(code)[0])
    ref = fr.decode_fixed(fr.Structure(int(code)), llrs, 25)
    for _ in range(3):
        order = rng.permutation(E)
        got = fr.decode_fixed(fr.Structure(int(code), sum_order=order), llrs, 25)
        assert all((x == y).all() for x, y in zip(ref, got))
    order = rng.permutation(E)
    for f in (4, len(llrs) - 1):
        a = fr.decode_fixed_loop(code, llrs[f], 3)
        b = fr.decode_fixed_loop(code, llrs[f], 3, sum_order=order)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("ebn0,fixed,flooding", [(1.7, 34, 164), (2.0, 0, 25)])
def test_failure_counts_at_fixed_seeds(ebn0, fixed, flooding):
    """TM2048, 600 frames of default_rng(1700) quantised to i8 at 8 / 31, cap 25: the fixed-point layered schedule fails 34 times at
    1.7 dB where flooding (the oracle on the same i8 frames) fails 164 times, and never at 2 dB where flooding fails 25 times."""
    code = LDPCCode.TM2048
    y, _ = oracle.awgn_llrs(code, np.random.default_rng(1700), 600, ebn0, np.float32)
    llrs = quantise(y, np.int8, 8, 31)
    _, _, ok_f, _ = oracle.decode_ms_batch(code, llrs, 25)
    _, _, ok_l, _, _ = fr.decode_fixed(fr.Structure(int(code)), llrs, 25)
    assert ((ok_l == 0).sum(), (ok_f == 0).sum()) == (fixed, flooding)


def test_header_declares_the_fixed_layered_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "labrador_ldpc_hip.h")).read(), flags=re.S)
    for suf, t in (("i8", "int8_t"), ("i16", "int16_t")):
        assert re.search(rf"int\s+labrador_ldpc_decode_ms_layered_fixed_batch_{suf}\s*\(\s*enum labrador_ldpc_code code,\s*const {t} \*llrs,\s*"
                         r"uint8_t \*output,\s*uint32_t \*iters,\s*uint8_t \*success,\s*size_t batch,\s*size_t max_iters,\s*"
                         r"const struct labrador_ldpc_hip_opts \*opts\s*\)\s*;", src)
        assert re.search(rf"int\s+labrador_ldpc_decode_ms_layered_fixed_soft_batch_{suf}\s*\(\s*enum labrador_ldpc_code code,\s*const {t} \*llrs,\s*"
                         r"int32_t \*app,\s*uint8_t \*output,\s*uint32_t \*iters,\s*uint8_t \*success,\s*size_t batch,\s*size_t max_iters,\s*"
                         r"const struct labrador_ldpc_hip_opts \*opts\s*\)\s*;", src)
    assert re.search(r"#define\s+LABRADOR_LDPC_HIP_ABI\s+3\b", open(os.path.join(ROOT, "include", "labrador_ldpc_hip.h")).read())


def test_library_python_and_rust_hold_the_fixed_layered_entry_points():
    dll = ctypes.CDLL(la.LIB_PATH)
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for name in NAMES:
        assert hasattr(dll, name) and name in la.SYMBOLS
        assert re.search(rf"pub fn {name}\s*\(", rust), name
    assert la.lib.labrador_ldpc_hip_abi_version() == 3


def test_argument_checks_come_before_any_device_work():
    code = LDPCCode.TC128
    for suf, dtype in (("i8", np.int8), ("i16", np.int16)):
        llrs = np.ones((1, code.n()), dtype)
        app = np.zeros((1, code.n() + code.punctured_bits()), np.int32)
        out = np.zeros((1, code.output_len()), np.uint8)
        it = np.zeros(1, np.uint32)
        ok = np.zeros(1, np.uint8)
        hard = getattr(la.lib, f"labrador_ldpc_decode_ms_layered_fixed_batch_{suf}")
        soft = getattr(la.lib, f"labrador_ldpc_decode_ms_layered_fixed_soft_batch_{suf}")
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
            bad_mem = la.HipOpts(-1, 7, None, 0, 0, None)
            assert fn(int(code), *p, 1, 10, ctypes.byref(bad_mem)) in (EINVAL, -2, -3)      # (without a device: ENODEV / ERUNTIME first)
        assert (app == 0).all() and (out == 0).all()


def test_python_binding_checks_its_buffers():
    code = LDPCCode.TM1280
    np_len = code.n() + code.punctured_bits()
    for dtype in TYPES:
        llrs = np.ones((2, code.n()), dtype)
        with pytest.raises(ValueError):
            code.decode_ms_layered_fixed_soft_batch(llrs, app=np.zeros((2, code.n()), np.int32))          # wrong shape
        with pytest.raises(ValueError):
            code.decode_ms_layered_fixed_soft_batch(llrs, app=np.zeros((2, np_len), dtype))               # app is int32, not the LLR type
        with pytest.raises(ValueError):
            code.decode_ms_layered_fixed_soft_batch(llrs, app=np.zeros((2, np_len), np.float32))
        with pytest.raises(ValueError):
            code.decode_ms_layered_fixed_batch(llrs[:, :-1])
        with pytest.raises(ValueError):
            code.decode_ms_layered_fixed_batch(llrs, output=np.zeros((2, code.output_len() + 1), np.uint8))
        with pytest.raises(ValueError):
            code.decode_ms_layered_fixed_batch(llrs[0])
    for dtype in (np.float32, np.int32, np.float64):
        with pytest.raises(la.LdpcHipError):
            code.decode_ms_layered_fixed_batch(np.ones((2, code.n()), dtype))                             # i8 and i16 only
        with pytest.raises(la.LdpcHipError):
            code.decode_ms_layered_fixed_soft_batch(np.ones((2, code.n()), dtype))
    # the existing soft calls still hand back app in the LLR type
    assert code.decode_ms_soft_batch(np.ones((0, code.n()), np.int8))[0].dtype == np.int8


def test_a_variant_other_than_zero_is_unsupported_before_any_device_work():
    """`variant` 0 is the only kernel: any other value is EUNSUPPORTED for the hard and the soft form of both types, with host and
    with device memory named in opts, decided with the argument checks -- so also on a machine without a GPU, where a call that got
    as far as a device would answer ENODEV or ERUNTIME instead.  The buffers stay as they were."""
    code = LDPCCode.TC128
    for suf, dtype in (("i8", np.int8), ("i16", np.int16)):
        llrs = np.ones((1, code.n()), dtype)
        app = np.full((1, code.n() + code.punctured_bits()), -5, np.int32)
        out, it, ok = np.full((1, code.output_len()), 0xEE, np.uint8), np.full(1, 77, np.uint32), np.full(1, 7, np.uint8)
        hard = getattr(la.lib, f"labrador_ldpc_decode_ms_layered_fixed_batch_{suf}")
        soft = getattr(la.lib, f"labrador_ldpc_decode_ms_layered_fixed_soft_batch_{suf}")
        ph = [x.ctypes.data for x in (llrs, out, it, ok)]
        ps = [x.ctypes.data for x in (llrs, app, out, it, ok)]
        for fn, p in ((hard, ph), (soft, ps)):
            for variant in (1, 2, 3, 32, 64, 256, -1):
                for memory in (la.MEM_HOST, la.MEM_DEVICE):
                    opts = la.HipOpts(-1, memory, None, variant, 0, None)
                    assert fn(int(code), *p, 1, 10, ctypes.byref(opts)) == EUNSUPPORTED, (suf, variant, memory)
                    assert "only 0 is" in la.last_error()
        assert (app == -5).all() and (out == 0xEE).all() and it[0] == 77 and ok[0] == 7
        with pytest.raises(la.LdpcHipError, match="only 0 is"):
            code.decode_ms_layered_fixed_batch(llrs, 10, variant=2)
        with pytest.raises(la.LdpcHipError, match="only 0 is"):
            code.decode_ms_layered_fixed_soft_batch(llrs, 10, variant=2)


@pytest.fixture(scope="module")
def fixed_object():
    return layered_helpers.built_object("decode_ms_fixed_layered.o")


def _kernels(obj):
    return layered_helpers.kernels(obj, "decode_ms_layered_fixed_kernel")


def test_fixed_layered_kernels_keep_their_sweep_loops_free_of_scratch(fixed_object):
    """A sweep of the TM codes holds 2 barriers per block row (every row has a cell of two or three terms) and one for the vote: 7.
    No scratch instruction in a backward-branch span with that many barriers; the one-wave kernels (the TC codes, no s_barrier) hold
    none at all.  The deltas of the shared cells land by LDS adds, and the scalar unit only loads.  Both forms of all nine
    codes and both types."""
    kernels = _kernels(fixed_object)
    assert len(kernels) == 36
    sweeps = 0
    for name, body in kernels.items():
        code = int(re.search(r"kernelILi(\d+)E", name).group(1))
        ops = [t.split()[0] for _, t, _ in body]
        assert "ds_add_u32" in ops and not any(o.startswith("flat_atomic") for o in ops), name
        assert not any(o.startswith("s_") and ("store" in o or "atomic" in o) for o in ops), name      # scalar memory operations only load
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


def test_fixed_layered_kernels_have_uniform_control_flow_and_fit(fixed_object, capsys):
    """At most 5 `s_cbranch_execnz` per kernel -- this file's bound, the issue's; the built kernels have at most 3 -- and the
    registers and LDS of every kernel, recorded: at most 128 VGPRs where a workgroup is 16 waves (TM8192), and the marginals of the
    largest code in 41 KB of LDS, so that several workgroups share a CU."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    import scan_kernels
    table = scan_kernels.scan("build/csrc/decode_ms_fixed_layered.o")
    assert len(table) == 36
    bad = {k: v for k, v in table.items() if v[1] > 5}
    assert not bad, bad
    res = kernel_resources.resources("build/csrc/decode_ms_fixed_layered.o")
    assert len(res) == 36
    with capsys.disabled():
        for _, name, vgpr, spill, _, lds, scratch in res:
            print(f"\n{name.split('(')[0][11:]}: {vgpr} VGPRs ({spill} spilled), {lds} B LDS, {scratch} B scratch", end="")
    for _, name, vgpr, _, _, lds, _ in res:
        code = LDPCCode(int(re.search(r"kernel<(\d+),", name).group(1)))
        g = max(1, 64 // code.submatrix_size())
        assert int(lds) <= g * (4 * (code.n() + code.punctured_bits()) + 16) + 16, name
        assert int(vgpr) <= (128 if code == LDPCCode.TM8192 else 256), name
