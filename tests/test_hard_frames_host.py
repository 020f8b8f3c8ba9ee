"""The frame pools of tests/hard_frames.py against the CPU oracle and the reference's known answers, without a GPU: the bit-flipping
pool holds enough frames of every class (success at once, success later, failure) with the iteration counts its classes stand for,
the encoder pool's codewords are systematic codewords of H and carry the reference's parity, and draw() / same_on_device() do what
the GPU tests rely on."""
import numpy as np
import pytest

import hard_frames
import oracle

CODES = list(range(len(oracle.CODES)))


@pytest.mark.parametrize("code", CODES, ids=lambda c: oracle.CODES[c])
def test_bf_pool_classes(code):
    words, (out, iters, ok), cls = hard_frames.bf_pool(code)
    nb = oracle.n(code) // 8
    assert words.shape == (48, nb) and out.shape == (48, oracle.output_len(code)) and iters.shape == ok.shape == cls.shape == (48,)
    for c in range(3):
        assert int((cls == c).sum()) >= 8, f"class {c}"
    assert (cls[:16] == 0).all()                                       # the error-free frames
    assert (ok[cls == 2] == 0).all() and (iters[cls == 2] == 20).all()
    assert (ok[cls == 0] == 1).all() and (iters[cls == 0] == 0).all() and (out[cls == 0][:, :nb] == words[cls == 0]).all()
    assert (ok[cls == 1] == 1).all() and (iters[cls == 1] > 0).all() and (iters[cls == 1] < 20).all()
    for f in np.flatnonzero(ok):                                       # whatever it reports as decoded is a codeword of H
        assert oracle.syndrome_weight(code, out[f]) == 0, f"frame {f}"
    for a in (words, out, iters, ok, cls):
        assert not a.flags.writeable
    assert hard_frames.bf_pool(code)[0] is words                       # cached


@pytest.mark.parametrize("code", CODES, ids=lambda c: oracle.CODES[c])
def test_bf_pool_at_other_caps(code):
    """max_iters 0: no pre-pass, no iteration, failure with the input as output; max_iters 1: only class 0 succeeds."""
    words, _, cls = hard_frames.bf_pool(code)
    nb = oracle.n(code) // 8
    out0, it0, ok0 = hard_frames.bf_results(code, 0)
    assert (ok0 == 0).all() and (it0 == 0).all() and (out0[:, :nb] == words).all() and not out0[:, nb:].any()
    out1, it1, ok1 = hard_frames.bf_results(code, 1)
    assert ((ok1 == 1) == (cls == 0)).all() and (it1[cls == 0] == 0).all() and (it1[cls != 0] == 1).all()


@pytest.mark.parametrize("code", CODES, ids=lambda c: oracle.CODES[c])
def test_enc_pool_codewords(code, kats):
    data, cws = hard_frames.enc_pool(code)
    n, k = oracle.n(code), oracle.k(code)
    assert data.shape == (64, k // 8) and cws.shape == (64, n // 8)
    assert (cws[:, : k // 8] == data).all()                             # systematic
    assert not data[0].any() and not cws[0].any() and (data[1] == 0xFF).all()
    assert cws[2, k // 8:].tolist() == kats["encode_parity"][oracle.CODES[code]]
    for j in range(8):
        assert int(np.unpackbits(data[3 + j]).sum()) == 1 and cws[3 + j, k // 8:].any()
    assert len({d.tobytes() for d in data}) == 64
    for f in range(64):
        # the erasure pre-pass of the hard-decision decoder supplies the punctured bits; with them the word has syndrome 0
        ok, iters, full = oracle.decode_bf(code, cws[f], 1)
        assert ok and iters == 0 and (full[: n // 8] == cws[f]).all(), f"block {f}"
        assert oracle.L.oracle_syndrome_weight(code, full.ctypes.data) == 0, f"block {f}"
    assert not data.flags.writeable and not cws.flags.writeable


@pytest.mark.parametrize("g", [1, 4, 16])
def test_draw_changes_class_between_groups(g):
    _, _, cls = hard_frames.bf_pool(3)
    rng = np.random.default_rng(1)
    frames = 4000 * g + 3
    idx = hard_frames.draw(cls, frames, g, rng)
    assert idx.shape == (frames,) and idx.min() >= 0 and idx.max() < 48
    assert len(np.unique(idx)) == 48                                   # every pool entry is used
    # the majority class of successive groups differs (a quarter of the frames is of any class)
    grp = cls[idx[: 4000 * g]].reshape(4000, g)
    major = np.array([np.bincount(r, minlength=3).argmax() for r in grp])
    if g >= 16:
        assert (major[1:] != major[:-1]).mean() > 0.95
    share = np.bincount(cls[idx], minlength=3) / frames
    assert (share > 0.2).all()


def test_same_on_device_names_the_first_differing_frame():
    torch = pytest.importorskip("torch")
    ref = (torch.arange(48 * 5, dtype=torch.uint8).reshape(48, 5), torch.arange(48, dtype=torch.int32))
    idx = np.random.default_rng(2).integers(0, 48, 1000)
    got = [ref[0][torch.as_tensor(idx)].clone(), ref[1][torch.as_tensor(idx)].clone()]
    hard_frames.same_on_device("same", idx, got, ref, chunk=64)
    got[1][777] += 1
    got[0][901, 4] ^= 1
    with pytest.raises(AssertionError, match="2 frames differ, first 777"):
        hard_frames.same_on_device("second array", idx, got, ref, chunk=1000)
    with pytest.raises(AssertionError, match="1 frames differ, first 777"):
        hard_frames.same_on_device("chunked", idx, got, ref, chunk=64)
