"""guarded_buffers.py -- result rows with a guard band on either side, and inputs that must come back unchanged.

TEST INFRASTRUCTURE ONLY.  The decoders are handed raw pointers.  A result tensor of exactly the batch's size hides a store one slot
past its end in the allocator's slack; a view into the middle of a larger allocation does not:

  * guarded(rows, row_shape, dtype, lead_bytes, device) returns (view, guard).  `view` is a contiguous [rows, *row_shape] array inside
    ONE flat byte allocation -- a torch tensor on `device`, or a numpy array for device None -- with a band of guard bytes before and
    after it.  Each band is at least 64 rows of the array (four times the largest codeword group of any kernel, 16) and at least 4096
    bytes.  Every byte of a band is the same: 0xA5 for byte arrays and for `app` of any type (the type's bit pattern of 0xA5
    repeated), 0x5A for the 32-bit `iters` (0x5A5A5A5A).  The view itself is prefilled with 0xEE bytes, or with `prefill` (-2 for
    `iters`), so a row the call never wrote fails the comparison of values.
  * `lead_bytes` moves the base of the view that many bytes past a 16-byte boundary: the least alignment an entry admits.  The residue
    of the address is asserted, so an allocator that changes its alignment cannot silently align the view.
  * guard.check() asserts that both bands still hold their fill and names the array, the side, the offset of the first offending byte
    relative to the view's first byte (negative before it, from the view's size upwards behind it) and the byte found.  Bands are
    compared as raw bytes (a float NaN never equals itself), device bands on the device.
  * frozen(array) keeps a copy of an input where it lives; its check() asserts the original is byte for byte what it was.
"""
from __future__ import annotations

import numpy as np

GUARD_ROWS = 64
GUARD_BYTES = 4096
VIEW_FILL = 0xEE
FILL_U8 = 0xA5                                             # byte arrays, and `app` of any type
FILL_32 = 0x5A                                             # every byte of 0x5A5A5A5A: the 32-bit arrays (`iters`)

_TORCH_NAMES = {"uint8": np.uint8, "int8": np.int8, "int16": np.int16, "int32": np.int32, "float32": np.float32, "float64": np.float64}


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def _np_dtype(dtype) -> np.dtype:
    """numpy's dtype of a numpy or torch dtype"""
    if type(dtype).__module__.startswith("torch"):
        return np.dtype(_TORCH_NAMES[str(dtype).split(".")[-1]])
    return np.dtype(dtype)


def guard_byte(dtype, app: bool = False) -> int:
    """The byte a band of an array of `dtype` is filled with (`app`: the array is a call's marginals)."""
    return FILL_32 if not app and _np_dtype(dtype).itemsize == 4 else FILL_U8


def band_bytes(row_bytes: int) -> int:
    """Size of one band: at least GUARD_ROWS rows and GUARD_BYTES bytes, a multiple of 16."""
    return (max(GUARD_ROWS * row_bytes, GUARD_BYTES) + 15) // 16 * 16


def _bytes_of(x):
    """`x` (contiguous) as a flat array of bytes, where it lives"""
    if _is_torch(x):
        import torch
        return x.reshape(-1).view(torch.uint8)
    return np.ascontiguousarray(x).reshape(-1).view(np.uint8)


def _first_difference(got, want):
    """(index, byte found) of the first byte of `got` that differs from `want` (two flat byte arrays of one size), or None"""
    if _is_torch(got):
        import torch
        if torch.equal(got, want):
            return None
        i = int(torch.nonzero(got != want)[0])
    else:
        if np.array_equal(got, want):
            return None
        i = int(np.flatnonzero(got != want)[0])
    return i, int(got[i])


class Guard:
    """The two bands around a guarded view."""

    def __init__(self, name, before, after, fill, body_bytes):
        self.name, self.before, self.after, self.fill, self.body_bytes = name, before, after, fill, body_bytes
        if _is_torch(before):
            import torch
            self._want = torch.full((max(len(before), len(after)),), fill, dtype=torch.uint8, device=before.device)
        else:
            self._want = np.full(max(len(before), len(after)), fill, np.uint8)

    def check(self):
        for side, band in (("before", self.before), ("after", self.after)):
            d = _first_difference(band, self._want[:len(band)])
            if d is not None:
                off = d[0] - len(band) if side == "before" else self.body_bytes + d[0]
                raise AssertionError(f"{self.name}: the guard band {side} the view was written: byte offset {off} relative to the view "
                                     f"holds 0x{d[1]:02X}, not the fill 0x{self.fill:02X}")


def guarded(rows, row_shape, dtype, lead_bytes=0, device=None, *, name="array", app=False, prefill=None):
    """(view[rows, *row_shape], Guard): see the module's text.  `device` None = numpy, else the torch device.  `app`: fill the bands
    as for marginals.  `prefill`: the value every element of the view starts with (None = 0xEE bytes)."""
    dt = _np_dtype(dtype)
    row_shape = tuple(row_shape)
    row_bytes = int(np.prod(row_shape, dtype=np.int64)) * dt.itemsize
    body = rows * row_bytes
    band = band_bytes(row_bytes)
    assert 0 <= lead_bytes and lead_bytes % dt.itemsize == 0, "the view must stay aligned to its element"
    fill = guard_byte(dt, app)
    total = 16 + band + lead_bytes + body + band
    if device is None:
        flat = np.empty(total, np.uint8)
        base = flat.ctypes.data
    else:
        import torch
        flat = torch.empty(total, dtype=torch.uint8, device=device)
        base = flat.data_ptr()
    pad = -base % 16
    start = pad + band + lead_bytes
    flat[pad:start] = fill
    flat[start:start + body] = VIEW_FILL
    flat[start + body:start + body + band] = fill
    before, after = flat[pad:start], flat[start + body:start + body + band]
    if device is None:
        view = flat[start:start + body].view(dt).reshape((rows,) + row_shape)
        ptr = view.ctypes.data
    else:
        tdt = dtype if type(dtype).__module__.startswith("torch") else getattr(torch, dt.name)
        view = flat[start:start + body].view(tdt).view((rows,) + row_shape)
        ptr = view.data_ptr()
        assert view.is_contiguous()
    if prefill is not None:
        view[...] = prefill
    assert ptr % 16 == lead_bytes % 16, f"{name}: the view's base is at {ptr % 16} mod 16, not the {lead_bytes % 16} asked for"
    assert len(before) >= max(GUARD_ROWS * row_bytes, GUARD_BYTES) and len(after) >= max(GUARD_ROWS * row_bytes, GUARD_BYTES)
    return view, Guard(name, before, after, fill, body)


def guarded_copy(src, lead_bytes=0, device=None, *, name="llrs"):
    """A guarded view that holds `src` (a numpy array [rows, ...]), for an input: (view, Guard)."""
    view, guard = guarded(src.shape[0], src.shape[1:], src.dtype, lead_bytes, device, name=name)
    if device is None:
        view[...] = src
    else:
        import torch
        view.copy_(torch.from_numpy(np.ascontiguousarray(src)))
    return view, guard


class Frozen:
    """A copy of an input, made where the input lives; check() asserts the input still equals it byte for byte."""

    def __init__(self, array, name="input"):
        self.name, self.array = name, array
        self.copy = array.clone() if _is_torch(array) else np.array(array, copy=True)

    def check(self):
        d = _first_difference(_bytes_of(self.array), _bytes_of(self.copy))
        if d is not None:
            raise AssertionError(f"{self.name}: the input was changed: byte offset {d[0]} holds 0x{d[1]:02X}, "
                                 f"not 0x{int(_bytes_of(self.copy)[d[0]]):02X}")


def frozen(array, name="input"):
    return Frozen(array, name)
