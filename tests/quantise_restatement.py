"""The library's quantisation rule in numpy (include/labrador_ldpc_hip.h, labrador_ldpc_quantise_llrs_batch_*), what
the host loop and the kernel are held to byte for byte, and the fused decode as the composition it is defined to be."""
import numpy as np

import oracle

NP_DTYPE = {"i8": np.int8, "i16": np.int16}
FLT_MAX = np.finfo(np.float32).max


def quantise(y, dtype, scale, lim):
    """p = scale * y as ONE float32 product; NaN -> 0, said before any cast; otherwise clip(rint(p), -lim, lim), ties to even."""
    y = np.asarray(y)
    assert y.dtype == np.float32
    with np.errstate(over="ignore", invalid="ignore"):
        p = np.float32(scale) * y
    assert p.dtype == np.float32
    nan = np.isnan(p)
    r = np.rint(np.where(nan, np.float32(0), p))
    return np.clip(r, np.float32(-lim), np.float32(lim)).astype(dtype)


def decode_quantised(code, y, dtype, scale, lim, cap):
    """(output, iters, success) of the fused call: the oracle's flooding decode of the quantised frames."""
    return oracle.decode_ms_batch(code, quantise(y, dtype, scale, lim), cap)[:3]


def edge_vector(scale, lim):
    """float32 values at which a quantiser goes wrong: ties at +-0.5, +-1.5, +-2.5 in units of 1 / scale, +-0.0, +-inf, NaN, +-FLT_MAX,
    denormals, and the values on either side of lim +- 0.5.  The ties are made as tie / scale in float32 and kept only as what
    they are: whatever product the float32 multiply then gives is the restatement's to round, as it is the library's."""
    s = np.float32(scale)
    vals = []
    for t in (0.5, 1.5, 2.5, lim - 0.5, lim + 0.5):
        x = np.float32(t) / s
        for v in (x, np.nextafter(x, np.float32(np.inf)), np.nextafter(x, np.float32(-np.inf))):
            vals += [v, -v]
    tiny = np.float32(1e-45)                                   # the smallest denormal
    vals += [0.0, -0.0, np.inf, -np.inf, np.nan, FLT_MAX, -FLT_MAX, tiny, -tiny, np.float32(1e-39), np.float32(-1e-39),
             np.float32(lim) / s, -np.float32(lim) / s, np.float32(lim + 1) / s, -np.float32(lim + 1) / s]
    return np.array(vals, np.float32)
