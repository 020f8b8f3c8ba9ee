"""Soft output on the GPU (labrador_ldpc_decode_ms_soft_batch_*, LDPCCode.decode_ms_soft_batch): the a-posteriori LLRs equal the
reference's marginals `va` (src/decoder.rs:377) as the oracle leaves them in its working area, and the hard results equal both
the oracle's and the hard-only call's -- for every code and LLR type, converging and failing frames, iteration caps 0 / 1 / 2 /
25, corner values, every variant, both sides of the batch-size switches, every memory mode and one large device batch.

Equality: integer types exactly; float types as values (-0.0 == +0.0: the kernels return +0.0) with NaN exactly where the oracle's
va is NaN (any payload)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode, LdpcHipError
import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = list(LDPCCode)
DTYPES = [np.float32, np.int8, np.int16, np.int32, np.float64]
SUF = {np.dtype(np.float32): "f32", np.dtype(np.int8): "i8", np.dtype(np.int16): "i16", np.dtype(np.int32): "i32",
       np.dtype(np.float64): "f64"}
EUNSUPPORTED = -4


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if la.device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("the soft-output GPU tests need a gfx950 device")
    torch.cuda.set_device(0)


def oracle_soft(code, llrs, maxiters):
    """One frame through the oracle: (ok, iters as the batched call reports them, output, va)."""
    code = int(code)
    llrs = np.ascontiguousarray(llrs)
    n, p = oracle.n(code), oracle.p(code)
    E = oracle.L.oracle_code_paritycheck_sum(code)
    out = np.zeros(oracle.output_len(code), np.uint8)
    w = np.zeros(oracle.L.oracle_ms_working_len(code), dtype=llrs.dtype)
    w8 = np.zeros(oracle.L.oracle_ms_working_u8_len(code), np.uint8)
    it = ctypes.c_size_t(0)
    ok = getattr(oracle.L, "oracle_decode_ms_" + SUF[llrs.dtype])(code, llrs.ctypes.data, out.ctypes.data, w.ctypes.data,
                                                                  w8.ctypes.data, maxiters, ctypes.byref(it))
    assert ok >= 0
    return bool(ok), (int(it.value) if ok else maxiters), out, w[2 * E: 2 * E + n + p].copy()


def same_app(a, b):
    """a == b under the rule of the header: floats as values with NaN where NaN, integers exactly."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        na, nb = np.isnan(a), np.isnan(b)
        return bool((na == nb).all() and (a[~na] == b[~nb]).all())
    return bool((a == b).all())


def check_frames(code, llrs, maxiters, app, out, iters, ok, sample=None):
    """Every frame (or the sampled ones) against the oracle, and the hard bits against the signs of app."""
    frames = range(len(llrs)) if sample is None else sample
    for f in frames:
        ok_c, it_c, out_c, va_c = oracle_soft(code, llrs[f], maxiters)
        assert same_app(app[f], va_c), f"{code.name} {llrs.dtype} frame {f} maxiters {maxiters}: app != oracle va"
        assert (out[f] == out_c).all() and bool(ok[f]) == ok_c and int(iters[f]) == it_c, f"{code.name} frame {f}: hard results"
    assert (np.packbits(np.asarray(app) < 0, axis=1) == np.asarray(out)).all()


def int_llrs(code, rng, frames, ebn0, dtype):
    if np.dtype(dtype) == np.int32:
        return oracle.awgn_llrs(code, rng, frames, ebn0, dtype, scale=3e8, lim=2 ** 31 - 1)[0]
    return oracle.awgn_llrs(code, rng, frames, ebn0, dtype)[0]


def frames_of(code, rng, frames, ebn0, dtype):
    return oracle.awgn_llrs(code, rng, frames, ebn0, dtype)[0] if np.dtype(dtype).kind == "f" else int_llrs(code, rng, frames, ebn0, dtype)


def status_of(fn):
    try:
        return 0, fn()
    except LdpcHipError as e:
        return int(str(e).split()[1].rstrip(":")), None


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("code", ALL, ids=lambda c: c.name)
def test_three_flip_frame(code, dtype):
    """test_decode_ms of the reference (src/decoder.rs:671-699) with soft output."""
    cw = oracle.copy_encode(code, np.arange(code.k() // 8, dtype=np.uint8))
    rx = cw.copy()
    rx[0] ^= 0xA8
    llrs = oracle.hard_to_llrs(code, rx, dtype)[None, :]
    app, out, iters, ok = code.decode_ms_soft_batch(llrs, 50)
    out_h, it_h, ok_h = code.decode_ms_batch(llrs, 50)
    assert ok[0] and (out[0, : code.n() // 8] == cw).all()
    assert (out == out_h).all() and (iters == it_h).all() and (ok == ok_h).all()
    check_frames(code, llrs, 50, app, out, iters, ok)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("code", ALL, ids=lambda c: c.name)
def test_awgn_frames_and_iteration_caps(code, dtype):
    """Converging and failing frames (-1 / 2 / 5 dB) at max_iters 0, 1, 2 and 25."""
    rng = np.random.default_rng(1000 + 10 * int(code) + DTYPES.index(dtype))
    llrs = np.concatenate([frames_of(code, rng, 4, e, dtype) for e in (-1.0, 2.0, 5.0)])
    seen_ok = seen_fail = False
    for maxiters in (0, 1, 2, 25):
        app, out, iters, ok = code.decode_ms_soft_batch(llrs, maxiters)
        out_h, it_h, ok_h = code.decode_ms_batch(llrs, maxiters)
        assert (out == out_h).all() and (iters == it_h).all() and (ok == ok_h).all()
        if maxiters == 0:
            assert (app == 0).all()
        check_frames(code, llrs, maxiters, app, out, iters, ok)
        if maxiters == 25:
            seen_ok, seen_fail = bool(ok.any()), bool((ok == 0).any())
    assert seen_ok and seen_fail, "the Eb/N0 values should give converging and failing frames"


def corner_frames(code, dtype, rng, frames=6):
    llrs = frames_of(code, rng, frames, 3.0, dtype)
    n = code.n()
    if np.dtype(dtype).kind == "f":
        fi = np.finfo(dtype)
        specials = np.array([np.inf, -np.inf, 0.0, -0.0, fi.tiny / 4, -fi.tiny / 4, fi.max, -fi.max, np.nan], dtype=dtype)
        neg_nan = np.array([np.nan], dtype=dtype)
        neg_nan.view(np.uint32 if np.dtype(dtype).itemsize == 4 else np.uint64)[0] |= (1 << (8 * np.dtype(dtype).itemsize - 1))
        specials = np.concatenate([specials, neg_nan])
    else:
        ii = np.iinfo(dtype)
        specials = np.array([ii.min, ii.max, ii.min + 1, 0], dtype=dtype)
    for f in range(1, frames):                   # frame 0 stays plain
        pos = rng.choice(n, size=1 + f * 3, replace=False)
        llrs[f, pos] = rng.choice(specials, size=len(pos))
    if np.dtype(dtype).kind == "f":
        llrs[frames - 1, :] = np.nan              # every LLR NaN
    else:
        llrs[frames - 1, :] = np.iinfo(dtype).min  # every LLR at the type's minimum
    return llrs


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("code", ALL, ids=lambda c: c.name)
def test_corner_values(code, dtype):
    """+-inf, +-0.0, denormals, +-MAX and NaN LLRs (float types; NaN under both NaN handlings), type min / max (integers)."""
    rng = np.random.default_rng(77 + int(code))
    llrs = corner_frames(code, dtype, rng)
    variants = (0, 512, 1024) if np.dtype(dtype).kind == "f" and dtype != np.float64 else (0,)
    for variant in variants:
        for maxiters in (0, 3, 25):
            app, out, iters, ok = code.decode_ms_soft_batch(llrs, maxiters, variant=variant)
            out_h, it_h, ok_h = code.decode_ms_batch(llrs, maxiters, variant=variant)
            assert (out == out_h).all() and (iters == it_h).all() and (ok == ok_h).all()
            check_frames(code, llrs, maxiters, app, out, iters, ok)
            if np.dtype(dtype).kind == "f" and maxiters:
                assert (np.isnan(app[:, : code.n()]) == np.isnan(llrs)).all()


def test_int8_saturates_at_minus_128():
    """Saturating arithmetic reaches the type's minimum exactly (saturating_add, src/decoder.rs:47)."""
    code = LDPCCode.TM2048
    llrs = np.full((2, code.n()), -128, np.int8)
    llrs[1, ::2] = 127
    app, out, iters, ok = code.decode_ms_soft_batch(llrs, 5)
    check_frames(code, llrs, 5, app, out, iters, ok)
    assert app.min() == -128 and app.max() == 127


CANDIDATE_VARIANTS = [1, 2, 4, 16, 17, 18, 20, 32, 33, 34, 36, 64, 100, 256, 257, 258, 288, 320, 512, 1024]
# (code, LLR type, variant) -> the variant the hard-only call accepts and the soft call refuses: the header's list
REFUSED = {"i8": lambda code, v: (v & ~0x700) == 64, "f64": lambda code, v: v != 100 and bool((v & ~0x700) & 32)}


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("code", ALL, ids=lambda c: c.name)
def test_every_variant_gives_identical_results_or_is_refused(code, dtype):
    rng = np.random.default_rng(5 + int(code))
    llrs = frames_of(code, rng, 6, 2.0, dtype)
    ref_app, ref_out, ref_it, ref_ok = code.decode_ms_soft_batch(llrs, 25)
    check_frames(code, llrs, 25, ref_app, ref_out, ref_it, ref_ok)
    suf = SUF[np.dtype(dtype)]
    for v in CANDIDATE_VARIANTS:
        sh, hard = status_of(lambda: code.decode_ms_batch(llrs, 25, variant=v))
        ss, soft = status_of(lambda: code.decode_ms_soft_batch(llrs, 25, variant=v))
        if sh != 0:
            assert ss == sh, f"{code.name} {suf} variant {v}: hard status {sh}, soft {ss}"
            continue
        if suf in REFUSED and REFUSED[suf](code, v):
            assert ss == EUNSUPPORTED, f"{code.name} {suf} variant {v}: expected EUNSUPPORTED, got {ss}"
            continue
        assert ss == 0, f"{code.name} {suf} variant {v}: the hard-only call accepts it, the soft call returns {ss}"
        app, out, it, ok = soft
        assert same_app(app, ref_app), f"{code.name} {suf} variant {v}: app differs"
        assert (out == hard[0]).all() and (it == hard[1]).all() and (ok == hard[2]).all()
        assert (out == ref_out).all() and (it == ref_it).all() and (ok == ref_ok).all()


def device_frames(code, dtype, frames, ebn0, seed):
    """Device-resident AWGN frames of any LLR type (awgn_frames makes f32 / i8; the others are derived on the device)."""
    import torch
    rng = np.random.default_rng(seed)
    pool = np.stack([oracle.copy_encode(code, rng.integers(0, 256, code.k() // 8, dtype=np.uint8)) for _ in range(64)])
    cws = torch.from_numpy(pool).cuda()
    sigma = float(np.sqrt(1.0 / (2.0 * (code.k() / code.n()) * 10.0 ** (ebn0 / 10.0))))
    if dtype == np.int8:
        x = code.awgn_frames(cws, frames, sigma, seed, "i8")
    else:
        x = code.awgn_frames(cws, frames, sigma, seed, "f32")
        if dtype == np.float64:
            x = x.double()
        elif dtype == np.int16:
            x = (x * 8).round().clamp(-31, 31).to(torch.int16)
        elif dtype == np.int32:
            x = (x.double() * 3e8).round().clamp(-2 ** 31, 2 ** 31 - 1).to(torch.int32)
    torch.cuda.synchronize()
    return x


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("code", ALL, ids=lambda c: c.name)
def test_default_dispatch_on_both_sides_of_the_batch_size_switches(code, dtype):
    """1 frame (single-workgroup launches, one-pass NaN handling) and 65 536 frames (two-pass NaN handling; the i8 bit-sliced
    switch of the hard-only call): every frame's hard results against the hard-only call, sampled frames' app against the oracle."""
    import torch
    x = device_frames(code, dtype, 65536, 1.5, 11 + int(code))
    for frames in (1, 65536):
        llrs = x[:frames]
        app, out, it, ok = code.decode_ms_soft_batch(llrs, 25)
        out_h, it_h, ok_h = code.decode_ms_batch(llrs, 25)
        torch.cuda.synchronize()
        assert torch.equal(out, out_h) and torch.equal(it, it_h) and torch.equal(ok, ok_h)
        okc = ok.cpu().numpy()
        sample = sorted({0, frames // 2, frames - 1} | set(np.flatnonzero(okc == 0)[:3].tolist()))
        h_llrs = llrs[sample].cpu().numpy()
        check_frames(code, h_llrs, 25, app[sample].cpu().numpy(), out[sample].cpu().numpy(), it[sample].cpu().numpy(),
                     okc[sample], sample=range(len(sample)))
        signs = torch.from_numpy(np.packbits((app < 0).cpu().numpy(), axis=1)).cuda()
        assert torch.equal(signs, out)
    del x
    torch.cuda.empty_cache()


@pytest.mark.parametrize("code,dtype", [(LDPCCode.TM8192, np.float32), (LDPCCode.TM5120, np.float32), (LDPCCode.TM1536, np.int8),
                                        (LDPCCode.TC512, np.int16), (LDPCCode.TM2048, np.float64)], ids=lambda x: str(x))
def test_memory_modes_agree(code, dtype):
    import torch
    rng = np.random.default_rng(3)
    llrs = frames_of(code, rng, 40, 2.0, dtype)
    a = code.decode_ms_soft_batch(llrs, 25)
    check_frames(code, llrs, 25, *a, sample=[0, 1, 39])
    b = code.decode_ms_soft_batch(llrs, 25, devices=[0, 0])
    s = torch.cuda.Stream()
    d = torch.from_numpy(llrs).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        c = code.decode_ms_soft_batch(d, 25, stream=s.cuda_stream)
    s.synchronize()
    c = [t.cpu().numpy() for t in c]
    for other in (b, c):
        assert same_app(other[0], a[0])
        for x, y in zip(other[1:], a[1:]):
            assert (np.asarray(x) == np.asarray(y)).all()
    # a misaligned device app buffer
    np_len = code.n() + code.punctured_bits()
    raw = torch.empty(40 * np_len + 16, dtype=d.dtype, device="cuda")
    out = torch.empty((40, code.output_len()), dtype=torch.uint8, device="cuda")
    it = torch.empty(40, dtype=torch.int32, device="cuda")
    ok = torch.empty(40, dtype=torch.uint8, device="cuda")
    opts = la.HipOpts(0, la.MEM_DEVICE, torch.cuda.current_stream().cuda_stream, 0, 0, None)
    fn = getattr(la.lib, "labrador_ldpc_decode_ms_soft_batch_" + SUF[np.dtype(dtype)])
    st = fn(int(code), d.data_ptr(), raw.data_ptr() + 4, out.data_ptr(), it.data_ptr(), ok.data_ptr(), 40, 25, ctypes.byref(opts))
    assert st == -1 and "16-byte aligned" in la.last_error()
    torch.cuda.synchronize()


def test_large_device_batch():
    """262 144 device-resident TM8192 f32 frames at 2 dB: every frame's hard results equal the hard-only call's; app equals the
    oracle for the first, middle and last frame and for up to eight failing frames."""
    import torch
    code = LDPCCode.TM8192
    F = 262144
    x = device_frames(code, np.float32, F, 2.0, 2024)
    app, out, it, ok = code.decode_ms_soft_batch(x, 25)
    out_h, it_h, ok_h = code.decode_ms_batch(x, 25)
    torch.cuda.synchronize()
    assert torch.equal(out, out_h) and torch.equal(it, it_h) and torch.equal(ok, ok_h)
    okc = ok.cpu().numpy()
    sample = sorted({0, F // 2, F - 1} | set(np.flatnonzero(okc == 0)[:8].tolist()))
    check_frames(code, x[sample].cpu().numpy(), 25, app[sample].cpu().numpy(), out[sample].cpu().numpy(), it[sample].cpu().numpy(),
                 okc[sample], sample=range(len(sample)))
    del x, app, out, it, ok, out_h, it_h, ok_h
    torch.cuda.empty_cache()


def test_c_client(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no C compiler")
    libdir = os.path.dirname(la.LIB_PATH)
    hipdir = next((d for d in ([os.path.dirname(la.HIP_RUNTIME)] if la.HIP_RUNTIME else []) + ["/opt/rocm/lib"]
                   if os.path.exists(os.path.join(d, "libamdhip64.so"))), "/opt/rocm/lib")
    exe = str(tmp_path / "soft_smoke")
    cmd = [cc, "-std=c11", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "soft_smoke.c"),
           "-o", exe, "-L" + libdir, "-llabrador_ldpc_hip", "-L" + hipdir, "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath," + hipdir]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "soft smoke ok" in r.stdout, r.stdout + r.stderr
