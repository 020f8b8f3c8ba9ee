"""The guard bands of tests/guarded_buffers.py can fail: a byte poked at either end of either band is found and named, for every dtype
the helper serves, and so is a changed byte of a frozen input; the base of a view has the residue that was asked for.  numpy buffers
only: no GPU."""
import re

import numpy as np
import pytest

import guarded_buffers as gb

# (dtype, is `app`, the band's byte): the decoders' u8 outputs, the 32-bit iters, and marginals / LLRs of the five types and int32
SERVED = [(np.uint8, False, 0xA5), (np.int32, False, 0x5A), (np.uint32, False, 0x5A), (np.int8, True, 0xA5), (np.int16, True, 0xA5),
          (np.int32, True, 0xA5), (np.float32, True, 0xA5), (np.float64, True, 0xA5), (np.int8, False, 0xA5), (np.int16, False, 0xA5),
          (np.float64, False, 0xA5)]
IDS = [f"{np.dtype(d).name}{'-app' if a else ''}" for d, a, _ in SERVED]
# the placements the containment tests ask for: (dtype, lead_bytes, modulus, residue)
RESIDUES = [(np.uint8, 8, 16, 8),       # output: 8 mod 16
            (np.int32, 4, 8, 4),        # iters: 4 mod 8
            (np.uint8, 1, 2, 1),        # success, stage: an odd address
            (np.float32, 0, 16, 0), (np.int32, 0, 16, 0), (np.float64, 0, 16, 0),     # app and 16-byte llrs
            (np.int8, 1, 16, 1), (np.int16, 2, 16, 2), (np.int32, 4, 16, 4), (np.float32, 4, 16, 4), (np.float64, 8, 16, 8)]   # llrs one element off


def offset_named(err) -> int:
    return int(re.search(r"byte offset (-?\d+)", str(err.value)).group(1))


@pytest.mark.parametrize("dtype,app,fill", SERVED, ids=IDS)
@pytest.mark.parametrize("rows,row_shape,lead", [(3, (5,), 0), (1, (), 1), (17, (1536,), 2)], ids=["3x5", "scalar-rows", "17x1536"])
def test_every_poke_is_found_and_named(dtype, app, fill, rows, row_shape, lead):
    lead *= np.dtype(dtype).itemsize
    view, guard = gb.guarded(rows, row_shape, dtype, lead, None, name="thing", app=app)
    body = view.nbytes
    assert view.shape == (rows,) + row_shape and view.dtype == np.dtype(dtype) and view.flags.c_contiguous and view.flags.writeable
    assert (view.reshape(-1).view(np.uint8) == 0xEE).all(), "the view starts with its own fill"
    row_bytes = body // rows
    for band in (guard.before, guard.after):
        assert len(band) >= 64 * row_bytes and len(band) >= 4096 and (band == fill).all()
    assert guard.before.ctypes.data + len(guard.before) == view.ctypes.data and view.ctypes.data + body == guard.after.ctypes.data
    guard.check()                                            # untouched: passes
    view[...] = 1                                            # writing the view itself is what a call does
    guard.check()
    for band, index, side, offset in ((guard.before, 0, "before", -len(guard.before)), (guard.before, -1, "before", -1),
                                      (guard.after, 0, "after", body), (guard.after, -1, "after", body + len(guard.after) - 1)):
        band[index] ^= 0x01                                  # one bit of one byte
        with pytest.raises(AssertionError, match=f"thing: the guard band {side} the view") as err:
            guard.check()
        assert offset_named(err) == offset and f"0x{fill ^ 1:02X}" in str(err.value)
        band[index] = fill
        guard.check()


def test_a_view_prefilled_with_a_value():
    view, guard = gb.guarded(9, (), np.int32, 4, None, name="iters", prefill=-2)
    assert (view == -2).all() and view.ctypes.data % 8 == 4
    guard.check()
    view, guard = gb.guarded(9, (), np.int32, 4, None, name="iters", prefill=-1)
    assert (view.view(np.uint32) == 0xFFFFFFFF).all()
    guard.check()


@pytest.mark.parametrize("dtype,lead,mod,residue", RESIDUES, ids=[f"{np.dtype(d).name}-{r}mod{m}" for d, _, m, r in RESIDUES])
def test_the_residues_asked_for_are_the_ones_produced(dtype, lead, mod, residue):
    for rows, row_shape in ((1, (7,)), (33, (16,)), (5, ())):
        view, guard = gb.guarded(rows, row_shape, dtype, lead, None)
        assert view.ctypes.data % mod == residue and view.ctypes.data % 16 == lead
        guard.check()


def test_a_lead_that_breaks_the_element_alignment_is_refused():
    with pytest.raises(AssertionError):
        gb.guarded(2, (4,), np.float32, 2, None)


@pytest.mark.parametrize("dtype", [np.uint8, np.int8, np.int16, np.int32, np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_frozen_finds_a_changed_byte(dtype):
    rng = np.random.default_rng(5)
    src = rng.integers(0, 100, (6, 40)).astype(dtype)
    if np.dtype(dtype).kind == "f":
        src[2, 3] = np.nan                                   # a NaN that stays the same NaN is no change
    view, guard = gb.guarded_copy(src, np.dtype(dtype).itemsize, None)
    assert view.ctypes.data % 16 == np.dtype(dtype).itemsize and view.tobytes() == src.tobytes()
    keep = gb.frozen(view, "llrs")
    keep.check()
    guard.check()
    raw = view.reshape(-1).view(np.uint8)
    for index in (0, view.nbytes // 2, view.nbytes - 1):
        raw[index] ^= 0x80
        with pytest.raises(AssertionError, match="llrs: the input was changed") as err:
            keep.check()
        assert offset_named(err) == index
        raw[index] ^= 0x80
        keep.check()
    guard.before[-1] = 0                                     # an input's own bands are checked like any other
    with pytest.raises(AssertionError, match="before"):
        guard.check()
