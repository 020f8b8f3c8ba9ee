"""CPU checks of the references the soft-output GPU tests compare against.  The flooding kernels' `app` is compared with the C oracle's
marginals `va` (src/decoder.rs:377, left in its working area); here the oracle's `va` is tied to the independently structured numpy
restatement (oracle/ms_numpy.py, return_va=True) for every code and LLR type at the numeric edges, and the threaded batch form of the
oracle's soft results (oracle.decode_ms_soft_batch) to the single-frame entry it wraps.  The layered restatement's soft output is tied
to the oracle's `va` in tests/test_layered_host.py.  No GPU needed."""
import ctypes
import sys

import numpy as np
import pytest

import edge_frames
import oracle
from labrador_ldpc_amd import LDPCCode

sys.path.insert(0, oracle.ORACLE_DIR)
import ms_numpy  # noqa: E402

ALL = list(LDPCCode)
DTYPES = [np.float32, np.int8, np.int16, np.int32, np.float64]
_ST = {}


def structure(code):
    if code not in _ST:
        chk, var = oracle.edges(code)
        _ST[code] = ms_numpy.Structure(chk, var, oracle.n(code) + oracle.p(code))
    return _ST[code]


def same_app(a, b):
    """Floats as values with NaN exactly where NaN (-0.0 == +0.0), integers exactly -- the rule of the soft-output header."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        na, nb = np.isnan(a), np.isnan(b)
        return bool((na == nb).all() and (a[~na] == b[~nb]).all())
    return bool((a == b).all())


def single_frame(code, llr, maxiters):
    """The oracle's single-frame entry, its va read out of the working area as tests/test_gpu_soft_output.py does."""
    code = int(code)
    llr = np.ascontiguousarray(llr)
    E, V = oracle.L.oracle_code_paritycheck_sum(code), oracle.n(code) + oracle.p(code)
    out = np.zeros(oracle.output_len(code), np.uint8)
    w = np.zeros(oracle.L.oracle_ms_working_len(code), dtype=llr.dtype)
    w8 = np.zeros(oracle.L.oracle_ms_working_u8_len(code), np.uint8)
    it = ctypes.c_size_t(0)
    ok = getattr(oracle.L, "oracle_decode_ms_" + oracle._SUF[llr.dtype])(code, llr.ctypes.data, out.ctypes.data, w.ctypes.data,
                                                                        w8.ctypes.data, maxiters, ctypes.byref(it))
    assert ok >= 0
    return bool(ok), (int(it.value) if ok else maxiters), out, w[2 * E: 2 * E + V].copy()


def edge_batch(code, dtype, rng):
    """AWGN frames that converge and fail, plus the whole-frame (floats) or integer-range (integers) edge rows."""
    dt = np.dtype(dtype)
    big = oracle.n(code) >= 5120
    if dt.kind == "f":
        awgn = np.concatenate([oracle.awgn_llrs(code, rng, 2 if big else 3, e, dt)[0] for e in (0.5, 3.0)])
        return np.concatenate([awgn, edge_frames.whole_frame_rows(code, dt, rng)])
    scale, lim = (3e8, 2 ** 31 - 1) if dt == np.int32 else (8.0, 31)
    awgn = np.concatenate([oracle.awgn_llrs(code, rng, 2 if big else 3, e, dt, scale=scale, lim=lim)[0] for e in (0.5, 3.0)])
    return np.concatenate([awgn, edge_frames.integer_range_rows(code, dt, rng, 2 if big else 3)])


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("code", ALL, ids=lambda c: c.name)
def test_numpy_restatement_va_is_the_oracle_va(code, dtype):
    """The C oracle's va equals ms_numpy's, frame for frame, at caps 0 / 1 / 2 / 25 / 50 (and so do the hard results): a
    transcription slip in either the oracle's accumulation order, its minima or its saturation shows up in the values."""
    rng = np.random.default_rng(0x5EA + 16 * int(code) + DTYPES.index(dtype))
    llrs = edge_batch(code, dtype, rng)
    st = structure(code)
    for maxiters in (0, 1, 2, 25, 50):
        o_n, i_n, k_n, va_n = ms_numpy.decode_ms(st, llrs, oracle.n(code), maxiters, return_va=True)
        o_c, i_c, k_c, va_c = oracle.decode_ms_soft_batch(code, llrs, maxiters)
        assert va_n.dtype == va_c.dtype == llrs.dtype and va_n.shape == va_c.shape
        for f in range(len(llrs)):
            assert same_app(va_n[f], va_c[f]), f"{code.name} {np.dtype(dtype).name} frame {f} maxiters {maxiters}: va differs"
        assert (o_n == o_c).all() and (i_n == i_c).all() and (k_n == k_c).all(), (code.name, maxiters)
        if maxiters == 0:
            assert not va_c.any()


@pytest.mark.parametrize("code,dtype", [(LDPCCode.TC128, np.float32), (LDPCCode.TM1280, np.int8), (LDPCCode.TM2048, np.float64),
                                        (LDPCCode.TM8192, np.int32), (LDPCCode.TC512, np.int16)], ids=lambda x: getattr(x, "name", str(x)))
def test_threaded_soft_batch_is_the_single_frame_entry(code, dtype):
    """oracle.decode_ms_soft_batch against per-frame calls of the single-frame entry, and its hard results against the oracle's
    batched call (which reports iters = max_iters on failure)."""
    rng = np.random.default_rng(0xB47 + int(code))
    llrs = edge_batch(code, dtype, rng)
    for maxiters in (0, 3, 30):
        out, it, ok, va = oracle.decode_ms_soft_batch(code, llrs, maxiters)
        o_b, i_b, k_b, _ = oracle.decode_ms_batch(code, llrs, maxiters)
        assert (out == o_b).all() and (it == i_b).all() and (ok == k_b).all()
        for f in range(len(llrs)):
            ok1, it1, out1, va1 = single_frame(code, llrs[f], maxiters)
            assert bool(ok[f]) == ok1 and int(it[f]) == it1 and (out[f] == out1).all()
            assert va[f].tobytes() == va1.tobytes(), f"frame {f}: va differs from the single-frame entry's"
    assert oracle.decode_ms_soft_batch(code, llrs[:0], 5)[3].shape == (0, oracle.n(code) + oracle.p(code))
